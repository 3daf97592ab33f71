"""Run-length potentials benchmark: the kernels of ``Model.viterbi_run_length`` and ``Model.marginals_run_length`` at a table of
M = 3 and 32 scores and 2, 8 and 32 labels on 200 000 items as 1 000 sequences of 200 (the batch of tools/bench_kbest.py), beside
the launches of ``viterbi_min_run`` / ``marginals_min_run`` at a minimum of M on the same input: the same slot count, so the
difference is the exit aggregate, the length scores and the counts.

    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/bench_runlength.py --trace-pass
    python tools/bench_runlength.py --kernel-db DIR [--out FILE]
    python tools/bench_runlength.py --fit [--out FILE]

``--trace-pass`` makes, per (label count, M), one warm-up call and ``--trace-reps`` calls each of ``viterbi_min_run`` with log Z_C,
``marginals_min_run``, ``viterbi_run_length`` with log Z_g and ``marginals_run_length`` with every output, and nothing else.  The
label set is every label but label 0; the table is a soft one (finite scores, a finite tail).  ``--kernel-db DIR`` reads that run's
rocpd database and prints one JSON line per (label count, M): the medians, in microseconds begin to end, of the max walk, the
backtrack, the sum walk, the storing forward walk and the backward walk of either family, and their ratios.  It needs no device.
``--fit`` times one ``SequenceCRF.fit_run_length_scores`` on that batch at 3 labels and M = 8 against planted labels: the number
of evaluations and the wall-clock time per evaluation (one native call each)."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("max", "backtrack", "sum", "store", "backward")


def kind(name):
    """(family, kernel) of a dispatch, or None."""
    for family, stem in (("min_run", "gl_minrun_"), ("run_length", "gl_runlen_")):
        if stem + "backtrack" in name:
            return family, "backtrack"
        if stem + "backward" in name:
            return family, "backward"
        if stem + "forward" in name:  # <LP, SUM, STORE>
            flags = re.search(r"<\s*\d+\s*,\s*(true|false)\s*(?:,\s*(true|false)\s*)?>", name)
            if flags:
                summed, stored = flags.group(1) == "true", flags.group(2) == "true"
            else:
                summed, stored = "Lb1E" in name, "Lb1ELb1E" in name
            return family, "store" if stored else ("sum" if summed else "max")
    return None


def soft_table(M):
    g = -0.5 * np.abs(np.arange(1, M + 1) - min(M, 6.0)) / max(M, 1)
    return g, -0.05


def trace_pass(args, configs):
    import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

    from gecco_amd import _native
    from tools.bench_kbest import setup

    if _native.device_count() < 1:
        raise SystemExit("bench_runlength needs a HIP device")
    for L, tables in configs:
        model, csr = setup(L, args)
        mask = ((1 << L) - 1) & ~1
        for M in tables:
            g, tau = soft_table(M)
            for call in (lambda: model.viterbi_min_run(*csr, mask, M, device=args.device),
                         lambda: model.marginals_min_run(*csr, mask, M, device=args.device),
                         lambda: model.viterbi_run_length(*csr, mask, g, tau, device=args.device),
                         lambda: model.marginals_run_length(*csr, mask, g, tau, device=args.device)):
                for _ in range(args.trace_reps + 1):
                    call()
            print(f"traced: {L} labels, M = {M}", flush=True)


def read_trace(args, configs):
    import glob
    import sqlite3

    rows = []
    for db in sorted(glob.glob(os.path.join(args.kernel_db, "**", "*.db"), recursive=True)):
        con = sqlite3.connect(db)
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')")]
        kt = [t for t in tabs if t.startswith("kernels")] or [t for t in tabs if "kernel_dispatch" in t]
        if not kt:
            continue
        cols = [c[1] for c in con.execute(f"pragma table_info({kt[0]})")]
        name = "name" if "name" in cols else "kernel_name"
        rows += list(con.execute(f"select {name}, start, end from {kt[0]}"))
    found = {(f, k): [] for f in ("min_run", "run_length") for k in KINDS}
    for n, s, e in sorted(rows, key=lambda r: r[1]):
        if kind(n):
            found[kind(n)].append((e - s) / 1e3)
    reps = args.trace_reps
    n_cfg = sum(len(t) for _, t in configs)
    for key, vals in found.items():
        # the viterbi entry launches max, backtrack, sum; the marginals entry store, backward
        if len(vals) != n_cfg * (reps + 1):
            raise SystemExit(f"{args.kernel_db}: {len(vals)} dispatches of {key}, expected {n_cfg * (reps + 1)}")
    lines, k = [], 0
    n = args.sequences * args.length
    for L, tables in configs:
        for M in tables:
            out = {"tool": "bench_runlength", "labels": L, "max_length": M, "items": n, "sequences": args.sequences,
                   "set": "every label but 0", "source": f"rocprofv3 --kernel-trace --stats, median of {reps} calls after one warm-up call",
                   "median_us": {}, "run_length_over_min_run": {}}
            for family in ("min_run", "run_length"):
                out["median_us"][family] = {name: float(np.median(found[(family, name)][k * (reps + 1) + 1:(k + 1) * (reps + 1)]))
                                            for name in KINDS}
            for name in KINDS:
                out["run_length_over_min_run"][name] = out["median_us"]["run_length"][name] / out["median_us"]["min_run"][name]
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
            k += 1
    return lines


def fit(args):
    import torch  # noqa: F401

    from gecco_amd.crfsuite_model import model_bytes
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(3)
    L, M, An = 3, 8, 4
    w = np.array([[1.1, 0.0, 0.0], [0.0, 1.1, 0.0], [0.0, 0.0, 1.1], [0.2, 0.1, 0.1]])
    trans = np.array([[0.2, -0.1, -0.1], [-0.1, 0.3, 0.0], [-0.1, 0.0, 0.3]])
    names, classes = [f"a{k}" for k in range(An)], [f"l{k}" for k in range(L)]
    blob = model_bytes(classes, names, np.repeat(np.arange(An), L), np.tile(np.arange(L), An), np.repeat(np.arange(L), L),
                       np.tile(np.arange(L), L), np.concatenate([w.ravel(), trans.ravel()]))
    crf = SequenceCRF.from_bytes(blob, window_size=None, device=args.device)
    X, Y = [], []
    for _ in range(args.sequences):
        y = []
        while len(y) < args.length:
            y.extend([0] * int(rng.integers(2, 12)))
            y.extend([int(rng.integers(1, L))] * int(rng.integers(3, 7)))
        y = y[:args.length]
        k = len(y)
        while k > 0 and y[k - 1] != 0:
            k -= 1
        if len(y) - k < 3:
            y[k:] = [0] * (len(y) - k)
        X.append([[names[lab if rng.random() < 0.75 else int(rng.integers(0, An))]] for lab in y])
        Y.append([classes[lab] for lab in y])
    crf.run_length_counts(X[:4], classes[1:], np.zeros(M))  # (warm-up)
    t0 = time.perf_counter()
    g, tau = crf.fit_run_length_scores(X, Y, classes[1:], M, c2=1.0)
    wall = time.perf_counter() - t0
    r = crf.fit_run_length_result_
    line = json.dumps({"tool": "bench_runlength --fit", "labels": L, "max_length": M, "items": args.sequences * args.length,
                       "sequences": args.sequences, "evaluations": r.n_eval, "iterations": r.n_iter, "status": r.status,
                       "wall_s": wall, "wall_ms_per_evaluation": 1e3 * wall / max(r.n_eval, 1),
                       "length_scores": g.tolist(), "tail": tau})
    print(line, flush=True)
    return [line]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--max-length", default="3,32")
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace-pass", action="store_true", help="the calls to be traced")
    ap.add_argument("--trace-reps", type=int, default=30)
    ap.add_argument("--kernel-db", default=None, help="directory of the rocprofv3 run of --trace-pass")
    ap.add_argument("--fit", action="store_true", help="time one fit_run_length_scores")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    configs = [(int(L), [int(m) for m in args.max_length.split(",")]) for L in args.labels.split(",")]
    if args.trace_pass:
        return trace_pass(args, configs)
    if args.fit:
        lines = fit(args)
    elif args.kernel_db:
        lines = read_trace(args, configs)
    else:
        raise SystemExit("bench_runlength: --trace-pass under rocprofv3, --kernel-db DIR, or --fit")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
