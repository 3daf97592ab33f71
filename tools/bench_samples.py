"""Sampled-path benchmark: ``Model.sample_paths`` at 64, 256 and 1024 samples on the two batches of tools/bench_constrained.py
and tools/bench_spans.py -- 200 000 items as 1 000 sequences of 200, and one sequence of 20 000.

    python tools/bench_samples.py [--labels 2,8,32] [--samples 64,256,1024] [--kernel-db DIR] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/bench_samples.py --trace-pass

Per (batch, label count, sample count) one JSON line with the times of
  ``sample_paths``          one call that returns the paths (the download of n x N bytes is part of it);
  ``sample_runs``           one call with ``want_paths=False`` and one run query per sequence: the paths stay on the device;
  ``marginals_full_any_l``  the whole-sequence marginals through the any-L kernels, the pass the new call contains.
The calls are timed in turn, call by call, as in tools/bench_constrained.py (host clock and two HIP events on the null stream
around the synchronous call, which holds the plan, the upload, the launches and the download), after ``--warmup`` calls.

The kernels' own times come from a run of their own: ``--trace-pass`` makes ``--trace-reps`` ``sample_runs`` calls per
configuration, in the order of the timed run and nothing else, for ``rocprofv3 --kernel-trace --stats``; ``--kernel-db DIR`` then
reads that run's rocpd database and adds to every line the median begin-to-end time of ``gl_sample_paths``, of
``gl_sample_runs`` and the summed times of the kernels of the forward-backward pass in front of them, and
``paths_bytes_written_over_kernel_time`` = n x N bytes over the sampling kernel's time, with its share of the HBM peak (8 TB/s).
Without ``--kernel-db`` those fields say "not measured"."""
import argparse
import glob
import json
import os
import sqlite3
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes per second
SHAPES = {"1000x200": (1000, 200), "1x20000": (1, 20000)}


def configurations(args):
    return [(shape, int(L), int(N)) for shape in args.shapes.split(",") for L in args.labels.split(",") for N in args.samples.split(",")]


def setup(shape, L, args):
    from gecco_amd import _native, synth

    rng = np.random.default_rng(synth.SEED + L)
    sequences, length = SHAPES[shape]
    model = _native.Model.from_tables(rng.normal(0, 0.5, size=(args.attrs, L)), rng.normal(0, 0.5, size=(L, L)))
    seq_ptr, item_ptr, attr = synth.synth_contigs(rng, [length] * sequences, args.attrs)
    runs = (np.arange(sequences, dtype=np.int32), np.full(sequences, length // 2, dtype=np.int32),
            np.full(sequences, ((1 << L) - 1) & ~1, dtype=np.uint32))
    return model, (seq_ptr, item_ptr, attr), runs


def kernel_times(directory, configs, reps):
    """Per configuration the medians over its `reps` calls of (forward-backward kernels summed, gl_sample_paths, gl_sample_runs) in
    microseconds, from the dispatches of a --trace-pass run in start order."""
    calls = []
    for db in sorted(glob.glob(os.path.join(directory, "**", "*.db"), recursive=True)):
        con = sqlite3.connect(db)
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')")]
        kt = [t for t in tabs if t.startswith("kernels")] or [t for t in tabs if "kernel_dispatch" in t]
        if not kt:
            continue
        cols = [c[1] for c in con.execute(f"pragma table_info({kt[0]})")]
        name = "name" if "name" in cols else "kernel_name"
        front = 0.0
        for n, s, e in sorted(con.execute(f"select {name}, start, end from {kt[0]}"), key=lambda r: r[1]):
            if "gl_sample_paths" in n:
                calls.append([front, (e - s) / 1e3, 0.0])
                front = 0.0
            elif "gl_sample_runs" in n:
                calls[-1][2] = (e - s) / 1e3
            else:
                front += (e - s) / 1e3
    if len(calls) != len(configs) * reps:
        raise SystemExit(f"{directory}: {len(calls)} sampling launches, expected {len(configs)} configurations x {reps} calls")
    per = np.array(calls).reshape(len(configs), reps, 3)
    return {cfg: np.median(per[k], axis=0).tolist() for k, cfg in enumerate(configs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="1000x200,1x20000")
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--samples", default="64,256,1024")
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--evals", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace-pass", action="store_true", help="only the calls to be traced, untimed")
    ap.add_argument("--trace-reps", type=int, default=3)
    ap.add_argument("--kernel-db", default=None, help="directory of the rocprofv3 run of --trace-pass")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    configs = configurations(args)
    kernels = kernel_times(args.kernel_db, configs, args.trace_reps) if args.kernel_db else None
    import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

    from gecco_amd import _native

    if _native.device_count() < 1:
        raise SystemExit("bench_samples needs a HIP device")
    built, lines = {}, []
    for shape, L, N in configs:
        if (shape, L) not in built:
            built = {(shape, L): setup(shape, L, args)}  # (one batch at a time stays alive)
        model, csr, runs = built[(shape, L)]
        sample_runs = lambda: model.sample_paths(*csr, N, seed=args.seed, device=args.device, runs=runs, want_paths=False)
        if args.trace_pass:
            for _ in range(args.trace_reps):
                sample_runs()
            continue
        from tools.bench_constrained import timed_in_turn

        ones = np.ones(len(csr[2]))
        fns = {"sample_paths": lambda: model.sample_paths(*csr, N, seed=args.seed, device=args.device),
               "sample_runs": sample_runs,
               "marginals_full_any_l": lambda: model.marginals_full(*csr, device=args.device, values=ones)}
        n = int(csr[0][-1])
        found = sample_runs()
        out = {"tool": "bench_samples", "shape": shape, "labels": L, "samples": N, "items": n, "sequences": len(csr[0]) - 1,
               "attrs": args.attrs, "entries": int(len(csr[2])), "run_queries": len(runs[0]), "warmup": args.warmup,
               "evals_timed": args.evals, "paths_bytes": n * N, "runs_found_share": float((found[:, :, 0] >= 0).mean())}
        out.update(timed_in_turn(fns, args.warmup, args.evals))
        med = lambda name: out[name]["hip_event_us"][0]
        out["sample_runs_over_marginals_full_any_l"] = med("sample_runs") / med("marginals_full_any_l")
        if kernels is None:
            out["kernel_us"] = out["paths_bytes_written_over_kernel_time"] = "not measured"
        else:
            front, paths, tail = kernels[(shape, L, N)]
            rate = n * N / (paths * 1e-6)
            out["kernel_us"] = {"forward_backward_kernels_summed": front, "gl_sample_paths": paths, "gl_sample_runs": tail,
                                "source": f"rocprofv3 --kernel-trace --stats, median of {args.trace_reps} calls"}
            out["paths_bytes_written_over_kernel_time"] = {"bytes_per_s": rate, "share_of_hbm_peak": rate / HBM_PEAK}
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out and lines:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
