"""Max-marginal benchmark: ``Model.max_marginals`` against the routes that exist without it, on the same batch -- 200 000 items
as 1 000 sequences of 200, one span of 10 items per sequence (1 000 spans), at 2, 8 and 32 labels.

    python tools/bench_maxmarg.py [--labels 2,8,32] [--kernel-db DIR] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/bench_maxmarg.py --trace-pass
    python <a checkout without the entry>/tools/bench_maxmarg.py       (this file copied there; the same box: the routes it replaces)

Per label count one JSON line with the times of
  ``max_marginals_best``       one call that returns ``best`` alone: the plan, the upload, gl_state, the two walks, the download;
  ``max_marginals_through``    the same with the epilogue and the download of ``through`` (items x labels x 8 bytes);
  ``viterbi_kbest_k1``         ``viterbi_kbest`` at K = 1, the max-semiring walk the library had: one forward walk with
                               back-pointers and a backtrack -- behind the forward-backward pass for log Z that this entry always
                               runs, which is why the launches are compared beside the calls;
  ``viterbi``                  the one best path of the same batch;
  ``span_scores``              ``max_marginals`` with the 1 000 spans and no ``through``: both span outputs of every span;
  ``viterbi_copy_per_span``    what that replaces: ``viterbi`` under ``allowed`` masks on one copy of the sequence per span, which
                               gives ``span_best`` alone -- ``span_broken`` would take one more copy per item of the span.
The calls are timed in turn, call by call, as in tools/bench_constrained.py (host clock and two HIP events on the null stream
around the synchronous call), after ``--warmup`` calls.  In a checkout whose library has no ``gecco_crf_max_marginals`` the tool
times the routes that exist there and says so in ``"library"``.

The launches' own times come from a run of their own: ``--trace-pass`` makes, per configuration, ``--trace-reps`` times the three
calls ``viterbi_copy_per_span``, ``max_marginals`` (through and spans) and ``viterbi_kbest_k1`` and nothing else, for ``rocprofv3
--kernel-trace --stats``; ``--kernel-db DIR`` then reads that run's rocpd database and adds to every line the median begin-to-end
time of every launch of the new call, of ``gl_kbest_forward`` and ``gl_kbest_backtrack``, and the summed launches of the
copy-per-span route.  Without ``--kernel-db`` those fields say "not measured"."""
import argparse
import glob
import json
import os
import sqlite3
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAUNCHES = ("gl_maxmarg_forward", "gl_maxmarg_backward", "gl_maxmarg_epilogue", "gl_maxmarg_spans", "gl_kbest_forward",
            "gl_kbest_backtrack")


def setup(L, args):
    """The model, the batch, the spans (one per sequence, ``--span`` items at a random place, a random proper label set) and the
    copy-per-span batch with its masks."""
    from gecco_amd import _native, synth

    rng = np.random.default_rng(synth.SEED + L)
    model = _native.Model.from_tables(rng.normal(0, 0.5, size=(args.attrs, L)), rng.normal(0, 0.5, size=(L, L)))
    csr = synth.synth_contigs(rng, [args.length] * args.sequences, args.attrs)
    n_spans = args.spans
    contig = (np.arange(n_spans) % args.sequences).astype(np.int32)
    begin = rng.integers(0, args.length - args.span + 1, size=n_spans).astype(np.int32)
    end = (begin + args.span).astype(np.int32)
    full = (1 << L) - 1
    mask = rng.integers(1, max(full, 2), size=n_spans).astype(np.uint32)  # (never the full set: a span that restricts nothing)
    cptr, gptr, attr = csr
    rows = np.concatenate([np.arange(cptr[c], cptr[c + 1]) for c in contig])
    deg = np.diff(gptr)[rows]
    copy_gptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    copy_attr = attr[np.repeat(gptr[rows], deg) + (np.arange(int(deg.sum())) - np.repeat(copy_gptr[:-1], deg))].astype(np.int32)
    copy_cptr = (np.arange(n_spans + 1) * args.length).astype(np.int32)
    allowed = np.full(len(rows), full, dtype=np.uint32)
    for q in range(n_spans):
        allowed[q * args.length + begin[q]:q * args.length + end[q]] = mask[q]
    return model, csr, (contig, begin, end, mask), (copy_cptr, copy_gptr, copy_attr), allowed


def kernel_times(directory, n_configs, reps):
    """Per configuration the medians over its `reps` repetitions, in microseconds, of every launch of LAUNCHES, of the gl_state in
    front of the walks, of the summed launches of the copy-per-span route and of the summed launches in front of gl_kbest_forward,
    from the dispatches of a --trace-pass run in start order."""
    reps_seen = []
    for db in sorted(glob.glob(os.path.join(directory, "**", "*.db"), recursive=True)):
        con = sqlite3.connect(db)
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')")]
        kt = [t for t in tabs if t.startswith("kernels")] or [t for t in tabs if "kernel_dispatch" in t]
        if not kt:
            continue
        cols = [c[1] for c in con.execute(f"pragma table_info({kt[0]})")]
        name = "name" if "name" in cols else "kernel_name"
        pending, cur = [], None
        for n, s, e in sorted(con.execute(f"select {name}, start, end from {kt[0]}"), key=lambda r: r[1]):
            us = (e - s) / 1e3
            hit = next((k for k in LAUNCHES if k in n), None)
            if hit == "gl_maxmarg_forward":  # the launch before it is the call's gl_state; what came earlier, the copy route
                cur = {"viterbi_copy_per_span_summed": sum(pending[:-1]), "gl_state": pending[-1] if pending else 0.0}
                pending = []
            if hit is None:
                pending.append(us)
                continue
            if cur is None:
                continue
            if hit == "gl_kbest_forward":
                cur["in_front_of_gl_kbest_forward_summed"] = sum(pending)
                pending = []
            cur[hit] = us
            if hit == "gl_kbest_backtrack":
                reps_seen.append(cur)
                cur, pending = None, []
    if len(reps_seen) != n_configs * reps:
        raise SystemExit(f"{directory}: {len(reps_seen)} traced repetitions, expected {n_configs} configurations x {reps}")
    out = []
    for k in range(n_configs):
        mine = reps_seen[k * reps:(k + 1) * reps]
        out.append({key: float(np.median([r.get(key, np.nan) for r in mine])) for key in mine[0]})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--spans", type=int, default=1000)
    ap.add_argument("--span", type=int, default=10, help="items of a span")
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--evals", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace-pass", action="store_true", help="only the calls to be traced, untimed")
    ap.add_argument("--trace-reps", type=int, default=3)
    ap.add_argument("--kernel-db", default=None, help="directory of the rocprofv3 run of --trace-pass")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    labels = [int(L) for L in args.labels.split(",")]
    kernels = kernel_times(args.kernel_db, len(labels), args.trace_reps) if args.kernel_db else None
    import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

    from gecco_amd import _native

    if _native.device_count() < 1:
        raise SystemExit("bench_maxmarg needs a HIP device")
    has_entry = hasattr(_native.load_library(), "gecco_crf_max_marginals")
    lines = []
    for k, L in enumerate(labels):
        model, csr, spans, copies, allowed = setup(L, args)
        dev = args.device
        fns = {"viterbi_copy_per_span": lambda: model.viterbi(*copies, device=dev, allowed=allowed),
               "viterbi_kbest_k1": lambda: model.viterbi_kbest(*csr, 1, device=dev),
               "viterbi": lambda: model.viterbi(*csr, device=dev)}
        if has_entry:
            fns.update({"max_marginals_best": lambda: model.max_marginals(*csr, device=dev, want_through=False),
                        "max_marginals_through": lambda: model.max_marginals(*csr, device=dev),
                        "span_scores": lambda: model.max_marginals(*csr, spans=spans, device=dev, want_through=False)})
        if args.trace_pass:
            for _ in range(args.trace_reps):
                fns["viterbi_copy_per_span"]()
                model.max_marginals(*csr, spans=spans, device=dev)
                fns["viterbi_kbest_k1"]()
            continue
        from tools.bench_constrained import timed_in_turn

        n = int(csr[0][-1])
        out = {"tool": "bench_maxmarg", "library": "with gecco_crf_max_marginals" if has_entry else "without gecco_crf_max_marginals",
               "labels": L, "items": n, "sequences": len(csr[0]) - 1, "spans": args.spans, "span_items": args.span, "attrs": args.attrs,
               "entries": int(len(csr[2])), "warmup": args.warmup, "evals_timed": args.evals, "workspace_bytes": 16 * n * L}
        _, copy_score = fns["viterbi_copy_per_span"]()
        if has_entry:
            got = model.max_marginals(*csr, spans=spans, device=dev)
            scale = np.maximum(1.0, np.abs(copy_score))
            out["span_best_against_copy_route_worst_relative"] = float(np.max(np.abs(got["span_best"] - copy_score) / scale))
            out["best_is_kbest_rank_0"] = bool(got["best"].tobytes() == np.ascontiguousarray(fns["viterbi_kbest_k1"]()[1][:, 0]).tobytes())
        out.update(timed_in_turn(fns, args.warmup, args.evals))
        med = lambda name: out[name]["hip_event_us"][0]  # noqa: E731
        if has_entry:
            out["max_marginals_best_over_viterbi_kbest_k1"] = med("max_marginals_best") / med("viterbi_kbest_k1")
            out["max_marginals_best_over_viterbi"] = med("max_marginals_best") / med("viterbi")
            out["span_scores_over_viterbi_copy_per_span"] = med("span_scores") / med("viterbi_copy_per_span")
        if kernels is None:
            out["kernel_us"] = "not measured"
        else:
            ku = dict(kernels[k], source=f"rocprofv3 --kernel-trace --stats, median of {args.trace_reps} repetitions")
            ku["two_walks_over_gl_kbest_forward"] = (ku["gl_maxmarg_forward"] + ku["gl_maxmarg_backward"]) / ku["gl_kbest_forward"]
            ku["walk_ns_per_item"] = [ku["gl_maxmarg_forward"] * 1e3 / n, ku["gl_maxmarg_backward"] * 1e3 / n]
            out["kernel_us"] = ku
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out and lines:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
