"""K-best benchmark: ``Model.viterbi_kbest`` at K = 1, 8 and 32 against ``Model.viterbi`` (``gecco_crf_viterbi``, the yardstick:
it exists without the new entry) on the same batch -- 200 000 items as 1 000 sequences of 200, at 2, 8 and 32 labels.

    python tools/bench_kbest.py [--labels 2,8,32] [--k 1,8,32] [--kernel-db DIR] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/bench_kbest.py --trace-pass

Per (label count, K) one JSON line with the times of
  ``viterbi_kbest``         one call: the plan, the upload, the forward-backward pass for log Z, the allocation of the
                            back-pointers (items x labels x K x 2 bytes), the list recursion, its backtrack and the download;
  ``viterbi``               the one best path of the same batch;
  ``marginals_full_any_l``  the whole-sequence marginals through the any-L kernels, the pass the new call contains.
The calls are timed in turn, call by call, as in tools/bench_constrained.py (host clock and two HIP events on the null stream
around the synchronous call), after ``--warmup`` calls.

The kernels' own times come from a run of their own: ``--trace-pass`` makes ``--trace-reps`` ``viterbi_kbest`` calls per
configuration, in the order of the timed run and nothing else, for ``rocprofv3 --kernel-trace --stats``; ``--kernel-db DIR`` then
reads that run's rocpd database and adds to every line the median begin-to-end time of ``gl_kbest_forward``, of
``gl_kbest_backtrack`` and the summed times of the kernels in front of them, and the forward kernel's time per item.  Without
``--kernel-db`` those fields say "not measured"."""
import argparse
import glob
import json
import os
import sqlite3
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def configurations(args):
    return [(int(L), int(K)) for L in args.labels.split(",") for K in args.k.split(",")]


def setup(L, args):
    from gecco_amd import _native, synth

    rng = np.random.default_rng(synth.SEED + L)
    model = _native.Model.from_tables(rng.normal(0, 0.5, size=(args.attrs, L)), rng.normal(0, 0.5, size=(L, L)))
    return model, synth.synth_contigs(rng, [args.length] * args.sequences, args.attrs)


def kernel_times(directory, configs, reps):
    """Per configuration the medians over its `reps` calls of (kernels in front summed, gl_kbest_forward, gl_kbest_backtrack) in
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
            if "gl_kbest_forward" in n:
                calls.append([front, (e - s) / 1e3, 0.0])
                front = 0.0
            elif "gl_kbest_backtrack" in n:
                calls[-1][2] = (e - s) / 1e3
            else:
                front += (e - s) / 1e3
    if len(calls) != len(configs) * reps:
        raise SystemExit(f"{directory}: {len(calls)} k-best launches, expected {len(configs)} configurations x {reps} calls")
    per = np.array(calls).reshape(len(configs), reps, 3)
    return {cfg: np.median(per[k], axis=0).tolist() for k, cfg in enumerate(configs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--k", default="1,8,32")
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--evals", type=int, default=10)
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
        raise SystemExit("bench_kbest needs a HIP device")
    built, lines = {}, []
    for L, K in configs:
        if L not in built:
            built = {L: setup(L, args)}  # (one batch at a time stays alive)
        model, csr = built[L]
        kbest = lambda: model.viterbi_kbest(*csr, K, device=args.device)
        if args.trace_pass:
            for _ in range(args.trace_reps):
                kbest()
            continue
        from tools.bench_constrained import timed_in_turn

        ones = np.ones(len(csr[2]))
        fns = {"viterbi_kbest": kbest, "viterbi": lambda: model.viterbi(*csr, device=args.device),
               "marginals_full_any_l": lambda: model.marginals_full(*csr, device=args.device, values=ones)}
        n = int(csr[0][-1])
        y, score, n_paths, _ = kbest()
        best, best_score = model.viterbi(*csr, device=args.device)
        out = {"tool": "bench_kbest", "labels": L, "k": K, "items": n, "sequences": len(csr[0]) - 1, "attrs": args.attrs,
               "entries": int(len(csr[2])), "warmup": args.warmup, "evals_timed": args.evals, "back_pointer_bytes": n * L * K * 2,
               "paths_bytes": n * K, "rank_0_is_viterbi": bool(np.array_equal(y[:, 0], best)),
               "ranks_filled_share": float(n_paths.mean() / K)}
        out.update(timed_in_turn(fns, args.warmup, args.evals))
        med = lambda name: out[name]["hip_event_us"][0]
        out["viterbi_kbest_over_viterbi"] = med("viterbi_kbest") / med("viterbi")
        if kernels is None:
            out["kernel_us"] = out["forward_ns_per_item"] = "not measured"
        else:
            front, forward, back = kernels[(L, K)]
            out["kernel_us"] = {"kernels_in_front_summed": front, "gl_kbest_forward": forward, "gl_kbest_backtrack": back,
                                "source": f"rocprofv3 --kernel-trace --stats, median of {args.trace_reps} calls"}
            out["forward_ns_per_item"] = forward * 1e3 / n
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out and lines:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
