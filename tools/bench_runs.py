"""Run-posterior benchmark: ``Model.run_posteriors`` with 1 000 anchors at reach 16 / 64 / 200 beside the pass it contains and
beside the route it replaces, on the equal set of tools/bench_constrained.py (1 000 sequences of 200 items).

    python tools/bench_runs.py [--sequences 1000] [--length 200] [--anchors 1000] [--labels 2,8,32] [--reaches 16,64,200] [--out FILE]

Per label count one JSON line with the times of
  ``runs_reach_R``        one ``run_posteriors`` call over the batch with all the anchors at reach R (no marginals asked for): the
                          pass, the two walk launches, 2 x anchors x (R + 1) + 3 x anchors doubles back;
  ``runs_closed``         the same call with one closed-run query per anchor instead (the range [anchor - 2, anchor + 3), clipped);
  ``pass_one_anchor``     the same entry with ONE anchor at reach 0: the forward-backward pass of the batch with a walk of one item
                          behind it -- the pass alone, as this entry runs it (any-L kernels, nothing per item brought back);
  ``marginals_full``      the whole-sequence marginals of the same batch as a caller gets them (a 2-label model takes its own
                          kernels there; [n, L] doubles come back), and ``marginals_full_any_l`` through the any-L kernels;
  ``sample_runs``         ``sample_paths`` with the same anchors as run queries at N = ``--samples`` (1 000) paths, the paths kept
                          on the device: the route the exact distributions replace.
The calls are timed in turn, call by call, as in tools/bench_constrained.py (host clock and two HIP events on the null stream
around the synchronous call, which holds the plan, the upload, the launches and the download).  ``sampled_vs_exact`` compares
the sampled share of paths with the anchor inside the set with exp(log_anchor): the largest |difference| and the largest in
units of sigma = sqrt(max(p (1 - p) / N, 1 / N))."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gecco_amd import _native, synth  # noqa: E402
from tools.bench_constrained import timed_in_turn  # noqa: E402
from tools.bench_spans import random_sets  # noqa: E402


def run(L, args):
    rng = np.random.default_rng(synth.SEED + L)
    A = args.attrs
    model = _native.Model.from_tables(rng.normal(0, 0.5, size=(A, L)), rng.normal(0, 0.5, size=(L, L)))
    seq_ptr, item_ptr, attr = synth.synth_contigs(rng, [args.length] * args.sequences, A)
    n = int(seq_ptr[-1])
    ones = np.ones(len(attr))
    contig = rng.integers(0, args.sequences, size=args.anchors).astype(np.int32)
    item = rng.integers(0, args.length, size=args.anchors).astype(np.int32)
    mask = random_sets(rng, args.anchors, L)
    mask[mask == (1 << L) - 1] = 1  # (proper subsets: a full set's walk has an empty complement)
    anchors = (contig, item, mask)
    closed = (contig, np.maximum(item - 2, 0).astype(np.int32), np.minimum(item + 3, args.length).astype(np.int32), mask)
    reaches = [int(r) for r in args.reaches.split(",")]
    csr = (seq_ptr, item_ptr, attr)
    fns = {f"runs_reach_{r}": (lambda r=r: model.run_posteriors(*csr, anchors=anchors, reach=r, device=args.device)) for r in reaches}
    fns["runs_closed"] = lambda: model.run_posteriors(*csr, runs=closed, device=args.device)
    fns["pass_one_anchor"] = lambda: model.run_posteriors(*csr, anchors=(contig[:1], item[:1], mask[:1]), reach=0, device=args.device)
    fns["marginals_full"] = lambda: model.marginals_full(*csr, device=args.device)
    fns["marginals_full_any_l"] = lambda: model.marginals_full(*csr, device=args.device, values=ones)
    fns["sample_runs"] = lambda: model.sample_paths(*csr, args.samples, seed=1, device=args.device, runs=anchors, want_paths=False)
    exact = fns[f"runs_reach_{reaches[-1]}"]()
    drawn = fns["sample_runs"]()
    p = np.exp(exact["log_anchor"])
    share = (drawn[:, :, 0] >= 0).mean(axis=1)
    sigma = np.sqrt(np.maximum(p * (1.0 - p) / args.samples, 1.0 / args.samples))
    both = np.concatenate([exact["log_start"], exact["log_end"]], axis=1)
    out = {"tool": "bench_runs", "labels": L, "attrs": A, "items": n, "sequences": args.sequences, "entries": int(len(attr)),
           "anchors": args.anchors, "reaches": reaches, "samples": args.samples, "warmup": args.warmup, "evals_timed": args.evals,
           "finite_entries": int(np.isfinite(both).sum()), "min_finite_log_p": float(both[np.isfinite(both)].min()),
           "entries_below_1_over_samples": int((both[np.isfinite(both)] < -np.log(args.samples)).sum()),
           "sampled_vs_exact": {"max_abs_difference": float(np.abs(share - p).max()), "max_in_sigma": float((np.abs(share - p) / sigma).max())}}
    out.update(timed_in_turn(fns, args.warmup, args.evals))
    med = lambda name: out[name]["hip_event_us"][0]
    out["walks_us"] = {str(r): med(f"runs_reach_{r}") - med("pass_one_anchor") for r in reaches}
    out["walks_us"]["closed"] = med("runs_closed") - med("pass_one_anchor")
    out["runs_over_sample_runs"] = {str(r): med(f"runs_reach_{r}") / med("sample_runs") for r in reaches}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--anchors", type=int, default=1000)
    ap.add_argument("--reaches", default="16,64,200")
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--evals", type=int, default=30)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _native.device_count() < 1:
        raise SystemExit("bench_runs needs a HIP device")
    lines = [json.dumps(run(int(L), args)) for L in args.labels.split(",")]
    for line in lines:
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
