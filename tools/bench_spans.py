"""Region-posterior benchmark: ``Model.span_log_probabilities`` on 10 000 spans of mean length 20 against the two means there
were before it, on the equal set of tools/bench_constrained.py (1 000 sequences of 200 items).

    python tools/bench_spans.py [--sequences 1000] [--length 200] [--spans 10000] [--labels 2,8,32] [--out FILE]

Per label count one JSON line with the times of
  ``spans``               one ``span_log_probabilities`` call over the batch with all the spans (no marginals asked for);
  ``marginals_full``      the whole-sequence marginals of the same batch, the pass the new call contains -- as a caller gets
                          them (a 2-label model takes its own kernels there) and, ``marginals_full_any_l``, through the any-L
                          kernels the new call runs at every label count (every attribute value 1.0);
  ``log_likelihood_sets`` what ``SequenceCRF.log_likelihood`` with sets does for ``--old-spans`` (100) of the spans: a copy of
                          the span's sequence per span, the set inside the span and every label outside it, and two
                          whole-sequence passes over the copies (restricted and full lattice).  The packing on the Python side
                          is not timed.  The figure is for those 100 spans as measured; ``per_span_us`` divides by their number.
The calls are timed in turn, call by call, as in tools/bench_constrained.py (host clock and two HIP events on the null stream
around the synchronous call, which holds the plan, the upload, the launches and the download).  ``max_abs_difference`` is the
largest |difference| between the two routes on the 100 spans."""
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


def random_sets(rng, n, L):
    bits = rng.random((n, L)) < 0.5
    for i in np.flatnonzero(~bits.any(axis=1)):
        bits[i, int(rng.integers(0, L))] = True
    return (bits.astype(np.uint64) << np.arange(L, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def copies(seq_ptr, item_ptr, attr, contig, begin, end, mask, L):
    """The old route's batch: one copy of its sequence per span, with the masks of ``log_likelihood``'s sets."""
    c_ptr, i_ptr, ids, masks = [0], [0], [], []
    for c, b, e, m in zip(contig.tolist(), begin.tolist(), end.tolist(), mask.tolist()):
        g0, g1 = int(seq_ptr[c]), int(seq_ptr[c + 1])
        a0, a1 = int(item_ptr[g0]), int(item_ptr[g1])
        ids.append(attr[a0:a1])
        i_ptr.extend((item_ptr[g0 + 1:g1 + 1] - a0 + i_ptr[-1]).tolist())
        row = np.full(g1 - g0, (1 << L) - 1, dtype=np.uint32)
        row[b:e] = m
        masks.append(row)
        c_ptr.append(c_ptr[-1] + g1 - g0)
    return (np.array(c_ptr, dtype=np.int32), np.array(i_ptr, dtype=np.int32), np.concatenate(ids).astype(np.int32),
            np.concatenate(masks))


def run(L, args):
    rng = np.random.default_rng(synth.SEED + L)
    A = args.attrs
    model = _native.Model.from_tables(rng.normal(0, 0.5, size=(A, L)), rng.normal(0, 0.5, size=(L, L)))
    seq_ptr, item_ptr, attr = synth.synth_contigs(rng, [args.length] * args.sequences, A)
    n = int(seq_ptr[-1])
    ones = np.ones(len(attr))
    contig = rng.integers(0, args.sequences, size=args.spans).astype(np.int32)
    length = np.clip(rng.poisson(args.mean_length - 1, size=args.spans) + 1, 1, args.length).astype(np.int32)
    begin = (rng.random(args.spans) * (args.length - length + 1)).astype(np.int32)
    end = begin + length
    mask = random_sets(rng, args.spans, L)
    k = min(args.old_spans, args.spans)
    old = copies(seq_ptr, item_ptr, attr, contig[:k], begin[:k], end[:k], mask[:k], L)
    every = np.full(len(old[3]), (1 << L) - 1, dtype=np.uint32)

    def old_route():
        _, inside = model.marginals_full(*old[:3], device=args.device, allowed=old[3])
        _, free = model.marginals_full(*old[:3], device=args.device, allowed=every)
        return inside - free

    fns = {
        "spans": lambda: model.span_log_probabilities(seq_ptr, item_ptr, attr, contig, begin, end, mask, device=args.device),
        "marginals_full": lambda: model.marginals_full(seq_ptr, item_ptr, attr, device=args.device),
        "marginals_full_any_l": lambda: model.marginals_full(seq_ptr, item_ptr, attr, device=args.device, values=ones),
        "log_likelihood_sets": old_route,
    }
    new = fns["spans"]()
    diff = float(np.abs(new[:k] - old_route()).max())
    out = {"tool": "bench_spans", "labels": L, "attrs": A, "items": n, "sequences": args.sequences, "entries": int(len(attr)),
           "spans": args.spans, "mean_span_length": float(length.mean()), "old_route_spans": k, "old_route_items": int(old[0][-1]),
           "warmup": args.warmup, "evals_timed": args.evals, "max_abs_difference": diff,
           "finite": int(np.isfinite(new).sum()), "min_logp": float(new.min())}
    out.update(timed_in_turn(fns, args.warmup, args.evals))
    med = lambda name: out[name]["hip_event_us"][0]
    out["spans_over_marginals_full"] = med("spans") / med("marginals_full")
    out["spans_over_marginals_full_any_l"] = med("spans") / med("marginals_full_any_l")
    out["per_span_us"] = {"spans": med("spans") / args.spans, "log_likelihood_sets": med("log_likelihood_sets") / k}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--spans", type=int, default=10000)
    ap.add_argument("--mean-length", type=int, default=20)
    ap.add_argument("--old-spans", type=int, default=100)
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--evals", type=int, default=30)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _native.device_count() < 1:
        raise SystemExit("bench_spans needs a HIP device")
    lines = [json.dumps(run(int(L), args)) for L in args.labels.split(",")]
    for line in lines:
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
