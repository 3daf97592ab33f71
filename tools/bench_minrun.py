"""Minimum-run decoding benchmark: the kernels of ``Model.viterbi_min_run`` at a minimum of 1, 3 and 32 and 2, 8 and 32 labels
on 200 000 items as 1 000 sequences of 200 (the batch of tools/bench_kbest.py), with ``gl_kbest_forward`` at K = 1 on the same
batch beside them for scale: the walk that exists without the new entry.

    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/bench_minrun.py --trace-pass
    python tools/bench_minrun.py --kernel-db DIR [--out FILE]

``--trace-pass`` makes, per label count, one warm-up call and ``--trace-reps`` calls of ``viterbi_kbest`` at K = 1, then per
minimum one warm-up call and ``--trace-reps`` calls of ``viterbi_min_run`` with log Z_C (both instantiations of the forward
kernel run, the max semiring's first) and nothing else.  The label set is every label but label 0.  ``--kernel-db DIR`` reads
that run's rocpd database and prints one JSON line per (label count, minimum): the begin-to-end times in microseconds of every
traced call's ``gl_minrun_forward`` in the max semiring, its backtrack, ``gl_minrun_forward`` in the sum semiring, and
``gl_kbest_forward`` at K = 1, with their medians.  It needs no device; the warm-up calls are left out.

``--marginals`` (with either of the two) is the mode of ``Model.marginals_min_run``, by default at a minimum of
1 and 3: per (label count, minimum) one warm-up call and ``--trace-reps`` calls of ``viterbi_min_run`` with log Z_C, then as
many of ``marginals_min_run`` with ``marg`` and ``inside``.  The JSON lines then hold the new call's two launches -- the sum
semiring's forward walk that keeps its values, and ``gl_minrun_backward`` -- beside the sum-semiring launch of ``viterbi_min_run``
(the parent commit's code path) and the whole-contig pass that every call runs first: the sum of the launches of a
``marginals_min_run`` call that are none of the min-run kernels."""
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


def configurations(args):
    return [(int(L), [int(m) for m in args.min_run.split(",")]) for L in args.labels.split(",")]


def kind(name):
    """Which of the four kernels a dispatch is, or None."""
    if "gl_kbest_forward" in name:
        return "kbest"
    if "gl_minrun_backtrack" in name:
        return "backtrack"
    if "gl_minrun_backward" in name:
        return "backward"
    if "gl_minrun_forward" in name:  # <LP, SUM, STORE>
        flags = re.search(r"<\s*\d+\s*,\s*(true|false)\s*(?:,\s*(true|false)\s*)?>", name)
        if flags:
            summed, stored = flags.group(1) == "true", flags.group(2) == "true"
        else:
            summed, stored = "Lb1E" in name, "Lb1ELb1E" in name
        return "store" if stored else ("sum" if summed else "max")
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
    found = {"kbest": [], "max": [], "backtrack": [], "sum": [], "store": [], "backward": [], "pass": []}
    before = 0.0  # the launches since the last min-run kernel: the pass of the call that the next one belongs to
    for n, s, e in sorted(rows, key=lambda r: r[1]):
        if kind(n):
            found[kind(n)].append((e - s) / 1e3)
            if kind(n) == "store":
                found["pass"].append(before)
            before = 0.0
        elif "gecco" in n:  # (the library's own kernels: not the runtime's copy kernels)
            before += (e - s) / 1e3
    return found


def marginals_lines(args, configs, reps, found):
    """The JSON lines of ``--marginals``: per (label count, minimum) the medians of the traced calls."""
    calls = sum(len(minima) for _, minima in configs) * (reps + 1)
    want = {"kbest": 0, "max": calls, "backtrack": calls, "sum": calls, "store": calls, "backward": calls, "pass": calls}
    if {k: len(v) for k, v in found.items()} != want:
        raise SystemExit(f"{args.kernel_db}: dispatches {({k: len(v) for k, v in found.items()})}, expected {want}")
    take = lambda name, k: found[name][k * (reps + 1) + 1:(k + 1) * (reps + 1)]  # (without the warm-up call)
    lines, k = [], 0
    n = args.sequences * args.length
    for L, minima in configs:
        for m in minima:
            out = {"tool": "bench_minrun --marginals", "labels": L, "min_run": m, "items": n, "sequences": args.sequences,
                   "set": "every label but 0", "forward_value_bytes": 8 * n * L * m,
                   "source": f"rocprofv3 --kernel-trace --stats, {reps} calls after one warm-up call", "kernel_us": {}}
            for name, key in (("gl_minrun_forward_sum_store", "store"), ("gl_minrun_backward", "backward"),
                              ("gl_minrun_forward_sum", "sum"), ("marginals_pass", "pass")):
                vals = take(key, k)
                out["kernel_us"][name] = {"calls": vals, "median": float(np.median(vals))}
            med = lambda name: out["kernel_us"][name]["median"]
            out["two_launches_us"] = med("gl_minrun_forward_sum_store") + med("gl_minrun_backward")
            out["two_launches_over_forward_sum"] = out["two_launches_us"] / med("gl_minrun_forward_sum")
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
            k += 1
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--min-run", default=None, help="default: 1,3,32; with --marginals 1,3")
    ap.add_argument("--marginals", action="store_true", help="the mode of Model.marginals_min_run")
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace-pass", action="store_true", help="the calls to be traced")
    ap.add_argument("--trace-reps", type=int, default=3)
    ap.add_argument("--kernel-db", default=None, help="directory of the rocprofv3 run of --trace-pass")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.min_run is None:
        args.min_run = "1,3" if args.marginals else "1,3,32"
    configs = configurations(args)
    reps = args.trace_reps
    if args.trace_pass:
        import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

        from gecco_amd import _native
        from tools.bench_kbest import setup

        if _native.device_count() < 1:
            raise SystemExit("bench_minrun needs a HIP device")
        for L, minima in configs:
            model, csr = setup(L, args)
            if args.marginals:
                for m in minima:
                    for _ in range(reps + 1):
                        model.viterbi_min_run(*csr, ((1 << L) - 1) & ~1, m, device=args.device)
                    for _ in range(reps + 1):
                        model.marginals_min_run(*csr, ((1 << L) - 1) & ~1, m, device=args.device)
                continue
            for _ in range(reps + 1):
                model.viterbi_kbest(*csr, 1, device=args.device)
            for m in minima:
                for _ in range(reps + 1):
                    model.viterbi_min_run(*csr, ((1 << L) - 1) & ~1, m, device=args.device)
        return
    if not args.kernel_db:
        raise SystemExit("bench_minrun: --trace-pass under rocprofv3, or --kernel-db DIR (there is no untraced timing)")
    found = kernel_times(args.kernel_db)
    if args.marginals:
        lines = marginals_lines(args, configs, reps, found)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    for name in ("store", "backward", "pass"):
        found.pop(name)
    calls = sum(len(minima) for _, minima in configs) * (reps + 1)
    want = {"kbest": len(configs) * (reps + 1), "max": calls, "backtrack": calls, "sum": calls}
    if {k: len(v) for k, v in found.items()} != want:
        raise SystemExit(f"{args.kernel_db}: dispatches {({k: len(v) for k, v in found.items()})}, expected {want}")
    take = lambda name, k: found[name][k * (reps + 1) + 1:(k + 1) * (reps + 1)]  # (without the warm-up call)
    lines, k = [], 0
    n = args.sequences * args.length
    for li, (L, minima) in enumerate(configs):
        for m in minima:
            out = {"tool": "bench_minrun", "labels": L, "min_run": m, "items": n, "sequences": args.sequences,
                   "set": "every label but 0", "back_pointer_bytes": n * L * m,
                   "source": f"rocprofv3 --kernel-trace --stats, {reps} calls after one warm-up call", "kernel_us": {}}
            for name, idx in (("gl_minrun_forward_max", ("max", k)), ("gl_minrun_backtrack", ("backtrack", k)),
                              ("gl_minrun_forward_sum", ("sum", k)), ("gl_kbest_forward_k1", ("kbest", li))):
                vals = take(*idx)
                out["kernel_us"][name] = {"calls": vals, "median": float(np.median(vals))}
            out["forward_max_ns_per_item"] = out["kernel_us"]["gl_minrun_forward_max"]["median"] * 1e3 / n
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
            k += 1
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
