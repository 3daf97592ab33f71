"""Edge-posterior benchmark: the kernels of ``Model.edge_posteriors`` (``gl_edge_runs``, ``gl_edge_reduce``) beside the
forward-backward pass they follow, on 200 000 items as 1 000 sequences of 200, at 2, 8 and 32 labels.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_edges.py --trace-pass
    python tools/bench_edges.py --kernel-trace DIR [--out FILE]

``--trace-pass`` makes ``--trace-reps`` + 1 calls per configuration (the first is the warm-up) and nothing else, in a fixed
order; ``--kernel-trace DIR`` reads that run's ``*kernel_trace.csv`` and prints per configuration one JSON line with the
begin-to-end times in microseconds, per call, of the pass (every ``gecco::`` kernel in front of ``gl_edge_runs``: state scores
and the marginals recursion), of ``gl_edge_runs`` and of ``gl_edge_reduce``.  The runtime's copy kernels between two calls (the
outputs' way back) are not the pass and are left out.  The configurations: transition counts alone; with the entropy (the
default of a call without sets); with 1 set and with 32 sets; with 1 set and the pair table."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("transitions", None, False, False), ("transitions+entropy", None, False, True), ("1 set", 1, False, True),
           ("32 sets", 32, False, True), ("1 set + pair", 1, True, True)]


def trace_pass(args):
    from gecco_amd import _native, synth

    for L in (int(x) for x in args.labels.split(",")):
        rng = np.random.default_rng(synth.SEED + L)
        model = _native.Model.from_tables(rng.normal(0, 0.5, size=(args.attrs, L)), rng.normal(0, 0.5, size=(L, L)))
        csr = synth.synth_contigs(rng, [args.length] * args.sequences, args.attrs)
        for name, n_sets, pair, entropy in CONFIGS:
            sets = None if n_sets is None else rng.integers(1, 1 << L, size=n_sets, dtype=np.uint64).astype(np.uint32)
            for _ in range(args.trace_reps + 1):
                out = model.edge_posteriors(*csr, sets=sets, want_pair=pair, want_entropy=entropy)
            print(f"L={L} {name}: N[0].sum() = {out['transitions'][0].sum():.6g}", file=sys.stderr, flush=True)


def kernel_times(directory, args):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    calls, front = [], 0.0
    for start, end, name in sorted(rows):
        us = (end - start) / 1e3
        if "gl_edge_runs" in name:
            calls.append({"pass": front, "gl_edge_runs": us, "gl_edge_reduce": 0.0})
            front = 0.0
        elif "gl_edge_reduce" in name:
            calls[-1]["gl_edge_reduce"] = us
        elif "gecco::" in name:
            front += us
    per = args.trace_reps + 1
    labels = [int(x) for x in args.labels.split(",")]
    if len(calls) != per * len(labels) * len(CONFIGS):
        raise SystemExit(f"{len(calls)} traced calls, expected {per * len(labels) * len(CONFIGS)}")
    lines = []
    for k, (L, (name, n_sets, pair, entropy)) in enumerate((L, c) for L in labels for c in CONFIGS):
        timed = calls[k * per + 1:(k + 1) * per]
        lines.append(json.dumps({"labels": L, "configuration": name, "items": args.length * args.sequences,
                                 **{key: [round(c[key], 1) for c in timed] for key in ("pass", "gl_edge_runs", "gl_edge_reduce")}}))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--attrs", type=int, default=200)
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--trace-reps", type=int, default=3)
    ap.add_argument("--kernel-trace", default=None, metavar="DIR")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_pass:
        return trace_pass(args)
    if args.kernel_trace is None:
        ap.error("give --trace-pass (under rocprofv3) or --kernel-trace DIR")
    lines = kernel_times(args.kernel_trace, args)
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
