"""Run-count benchmark: the kernels of ``Model.run_counts`` at K = 2, 8 and 32 and 2, 8 and 32 labels on 200 000 items as 1 000
sequences of 200 (the batch of tools/bench_kbest.py and tools/bench_minrun.py), with the launches of ``Model.viterbi_min_run`` at
the same slot count beside them: a minimum of K + 1, or 32 where K + 1 is beyond that entry's range (K = 32: 33 slots against 32).

    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/bench_counts.py --trace-pass
    python tools/bench_counts.py --kernel-db DIR [--out FILE]

``--trace-pass`` makes, per label count and K, one warm-up call and ``--trace-reps`` calls of ``run_counts`` with ``log_mass``,
``score`` and ``y`` (the sum semiring's launch, the max semiring's, the backtrack), then as many of ``viterbi_min_run`` with
log Z_C, and nothing else.  The label set is every label but label 0.  ``--kernel-db DIR`` reads that run's rocpd database and
prints one JSON line per (label count, K): the begin-to-end times in microseconds of every traced call's ``gl_counts_forward`` in
either semiring, ``gl_counts_backtrack``, and ``gl_minrun_forward`` in either semiring, with their medians and the ratios of the
counts launches to their min-run siblings.  It needs no device; the warm-up calls are left out.  ``--out`` defaults to
profiles/counts_bench.jsonl."""
import argparse
import glob
import json
import os
import re
import sqlite3
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("counts_sum", "counts_max", "counts_backtrack", "minrun_max", "minrun_backtrack", "minrun_sum")


def configurations(args):
    return [(int(L), [int(k) for k in args.max_runs.split(",")]) for L in args.labels.split(",")]


def sibling_min_run(K):
    """The minimum at which ``viterbi_min_run`` has K + 1 slots, capped at that entry's range."""
    return min(K + 1, 32)


def kind(name):
    """Which of the six kernels a dispatch is, or None."""
    for family in ("counts", "minrun"):
        if f"gl_{family}_backtrack" in name:
            return f"{family}_backtrack"
        if f"gl_{family}_forward" in name:  # <LP, SUM[, STORE]>
            flags = re.search(r"<\s*\d+\s*,\s*(true|false)", name)
            summed = flags.group(1) == "true" if flags else "Lb1E" in name
            return f"{family}_sum" if summed else f"{family}_max"
    return None


def kernel_times(directory):
    """{kind: [microseconds of every dispatch, in start order]}."""
    rows = []
    for db in sorted(glob.glob(os.path.join(directory, "**", "*.db"), recursive=True)):
        con = sqlite3.connect(db)
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')")]
        kt = [t for t in tabs if t.startswith("kernels")] or [t for t in tabs if "kernel_dispatch" in t]
        if not kt:
            continue
        cols = [c[1] for c in con.execute(f"pragma table_info({kt[0]})")]
        name = "name" if "name" in cols else "kernel_name"
        rows += list(con.execute(f"select {name}, start, end from {kt[0]}"))
    found = {k: [] for k in KINDS}
    for n, s, e in sorted(rows, key=lambda r: r[1]):
        if kind(n):
            found[kind(n)].append((e - s) / 1e3)
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--max-runs", default="2,8,32")
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace-pass", action="store_true", help="the calls to be traced")
    ap.add_argument("--trace-reps", type=int, default=3)
    ap.add_argument("--kernel-db", default=None, help="directory of the rocprofv3 run of --trace-pass")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "counts_bench.jsonl"))
    args = ap.parse_args()
    configs = configurations(args)
    reps = args.trace_reps
    if args.trace_pass:
        import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

        from gecco_amd import _native
        from tools.bench_kbest import setup

        if _native.device_count() < 1:
            raise SystemExit("bench_counts needs a HIP device")
        for L, counts in configs:
            model, csr = setup(L, args)
            for K in counts:
                for _ in range(reps + 1):
                    model.run_counts(*csr, ((1 << L) - 1) & ~1, K, device=args.device)
                for _ in range(reps + 1):
                    model.viterbi_min_run(*csr, ((1 << L) - 1) & ~1, sibling_min_run(K), device=args.device)
        return
    if not args.kernel_db:
        raise SystemExit("bench_counts: --trace-pass under rocprofv3, or --kernel-db DIR (there is no untraced timing)")
    found = kernel_times(args.kernel_db)
    calls = sum(len(counts) for _, counts in configs) * (reps + 1)
    if {k: len(v) for k, v in found.items()} != {k: calls for k in KINDS}:
        raise SystemExit(f"{args.kernel_db}: dispatches {({k: len(v) for k, v in found.items()})}, expected {calls} of each")
    take = lambda name, k: found[name][k * (reps + 1) + 1:(k + 1) * (reps + 1)]  # (without the warm-up call)
    lines, k = [], 0
    n = args.sequences * args.length
    for L, counts in configs:
        for K in counts:
            out = {"tool": "bench_counts", "labels": L, "max_runs": K, "slots": K + 1, "min_run": sibling_min_run(K),
                   "min_run_slots": sibling_min_run(K), "items": n, "sequences": args.sequences, "set": "every label but 0",
                   "back_pointer_bytes": n * L * (K + 1),
                   "source": f"rocprofv3 --kernel-trace --stats, {reps} calls after one warm-up call", "kernel_us": {}}
            for name, key in (("gl_counts_forward_sum", "counts_sum"), ("gl_counts_forward_max", "counts_max"),
                              ("gl_counts_backtrack", "counts_backtrack"), ("gl_minrun_forward_sum", "minrun_sum"),
                              ("gl_minrun_forward_max", "minrun_max"), ("gl_minrun_backtrack", "minrun_backtrack")):
                vals = take(key, k)
                out["kernel_us"][name] = {"calls": vals, "median": float(np.median(vals))}
            med = lambda name: out["kernel_us"][name]["median"]
            out["sum_over_min_run_sum"] = med("gl_counts_forward_sum") / med("gl_minrun_forward_sum")
            out["max_over_min_run_max"] = med("gl_counts_forward_max") / med("gl_minrun_forward_max")
            out["forward_sum_ns_per_item"] = med("gl_counts_forward_sum") * 1e3 / n
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
            k += 1
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
