"""Conditional-marginals benchmark: ``Model.span_conditionals`` on 1 000 spans of 10 items at reach 16 and 200 against the
route it replaces, on the equal set of tools/bench_constrained.py (1 000 sequences of 200 items).

    python tools/bench_conditionals.py [--sequences 1000] [--length 200] [--spans 1000] [--span-length 10] [--reaches 16,200]
                                       [--labels 2,8,32] [--out FILE]

Per label count and reach one JSON line with the times of
  ``conditionals``        one ``span_conditionals`` call over the batch with all the spans: the conditional marginals of every
                          row and the contributions of every gene and attribute occurrence of the rows;
  ``conditionals_rows``   the same call without the contributions (``want_contributions=False``);
  ``marginals_full_any_l`` the whole-sequence marginals of the same batch through the any-L kernels: the pass the call contains;
  ``spans``               ``span_log_probabilities`` on the same spans, which the call also contains;
  ``replicated``          the route the call replaces for the conditional marginals alone: ``marginals_full(allowed=...)`` on a
                          batch with one copy of its sequence per span, the set inside the span and every label outside it.  It
                          uses entries that this call leaves as they were, so the figure is the parent's.  The packing on the
                          Python side is not timed.  (The contributions have no replaced route short of one pass per gene and
                          occurrence.)
The calls are timed in turn, call by call, as in tools/bench_constrained.py (host clock and two HIP events on the null stream
around the synchronous call, which holds the plan, the upload, the launches and the download).  ``max_abs_difference`` is the
largest |difference| between the two routes' conditional marginals over the rows of the call."""
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
from tools.bench_spans import copies, random_sets  # noqa: E402


def run(L, reach, args):
    rng = np.random.default_rng(synth.SEED + L)
    A = args.attrs
    model = _native.Model.from_tables(rng.normal(0, 0.5, size=(A, L)), rng.normal(0, 0.5, size=(L, L)))
    seq_ptr, item_ptr, attr = synth.synth_contigs(rng, [args.length] * args.sequences, A)
    ones = np.ones(len(attr))
    contig = rng.integers(0, args.sequences, size=args.spans).astype(np.int32)
    begin = (rng.random(args.spans) * (args.length - args.span_length + 1)).astype(np.int32)
    end = (begin + args.span_length).astype(np.int32)
    mask = random_sets(rng, args.spans, L)
    old = copies(seq_ptr, item_ptr, attr, contig, begin, end, mask, L)
    call = lambda **kw: model.span_conditionals(seq_ptr, item_ptr, attr, contig, begin, end, mask, reach=reach, device=args.device, **kw)
    fns = {
        "conditionals": call,
        "conditionals_rows": lambda: call(want_contributions=False),
        "marginals_full_any_l": lambda: model.marginals_full(seq_ptr, item_ptr, attr, device=args.device, values=ones),
        "spans": lambda: model.span_log_probabilities(seq_ptr, item_ptr, attr, contig, begin, end, mask, device=args.device),
        "replicated": lambda: model.marginals_full(*old[:3], device=args.device, allowed=old[3]),
    }
    new = call()
    rep, _ = fns["replicated"]()
    diff = 0.0
    for q in range(args.spans):
        r0, r1 = int(new["row_ptr"][q]), int(new["row_ptr"][q + 1])
        if np.isfinite(new["logp"][q]):
            g = int(old[0][q]) + int(new["first"][q])
            diff = max(diff, float(np.abs(new["cond"][r0:r1] - rep[g:g + r1 - r0]).max()))
    out = {"tool": "bench_conditionals", "labels": L, "reach": reach, "attrs": A, "items": int(seq_ptr[-1]), "sequences": args.sequences,
           "entries": int(len(attr)), "spans": args.spans, "span_length": args.span_length, "rows": int(new["row_ptr"][-1]),
           "occurrences": int(new["occ_ptr"][-1]), "replicated_items": int(old[0][-1]), "warmup": args.warmup,
           "evals_timed": args.evals, "max_abs_difference": diff, "finite": int(np.isfinite(new["logp"]).sum())}
    out.update(timed_in_turn(fns, args.warmup, args.evals))
    med = lambda name: out[name]["hip_event_us"][0]
    out["conditionals_over_replicated"] = med("conditionals") / med("replicated")
    out["conditionals_rows_over_replicated"] = med("conditionals_rows") / med("replicated")
    out["conditionals_over_marginals_full_any_l"] = med("conditionals") / med("marginals_full_any_l")
    out["conditionals_over_spans"] = med("conditionals") / med("spans")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--spans", type=int, default=1000)
    ap.add_argument("--span-length", type=int, default=10)
    ap.add_argument("--reaches", default="16,200")
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--evals", type=int, default=15)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _native.device_count() < 1:
        raise SystemExit("bench_conditionals needs a HIP device")
    lines = []
    for L in args.labels.split(","):
        for reach in args.reaches.split(","):
            lines.append(json.dumps(run(int(L), int(reach), args)))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
