"""Circular-contig benchmark: ``Model.ring`` beside the chain calls at the same shape and against the route it replaces -- 200 000
items as 1 000 rings of 200, at 2, 8 and 32 labels.

    python tools/bench_ring.py [--labels 2,8,32] [--evals 30] [--kernel-db DIR] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/bench_ring.py --trace-pass
    python <a checkout without the entry>/tools/bench_ring.py      (this file copied there; the same box: the chain calls and the copies)

Per label count one JSON line with the times of
  ``ring_lognorm``             one call that returns log Z of the ring alone: the plan, the upload, gl_state, the sum forward walk;
  ``ring_marginals``           the same with the forward values kept, the backward walk and the download of the marginals;
  ``ring_path``                log Z and the two max-plus walks with the backtrack;
  ``ring``                     everything;
  ``marginals_full``, ``viterbi``   the chain calls of the same batch -- what a walk over the plain lattice costs;
  ``copies_marginals``, ``copies_viterbi``   the route the entry replaces: one chain of 201 items per ring and start label a, item 0
                               pinned to a through ``allowed`` and an appended item without attributes pinned to a, through
                               ``marginals_full`` and ``viterbi`` under masks; ``copies_host_reduction_us`` is the host's
                               log-sum-exp and mix of the L copies' tables on top (``--copy-evals`` calls: at 32 labels the batch
                               is 6.4 M items).
The differences ``ring_marginals - ring_lognorm`` (the stores, the backward walk and the download) and ``ring_path -
ring_lognorm`` (the two decode passes and the backtrack) are given beside the calls.  The calls are timed in turn, call by call,
as in tools/bench_constrained.py (host clock and two HIP events on the null stream around the synchronous call), after
``--warmup`` calls.  In a checkout whose library has no ``gecco_crf_ring`` the tool times the routes that exist there and says so
in ``"library"``.

The launches' own times come from a run of their own: ``--trace-pass`` makes, per label count, one warm-up and ``--trace-reps``
times the calls ``ring`` (everything), ``marginals_full`` and ``viterbi`` and nothing else, for ``rocprofv3 --kernel-trace
--stats``; ``--kernel-db DIR`` then reads that run's rocpd database and adds to every line the median begin-to-end time of every
launch of those calls, by kernel name, in the order the label counts were run.  (The library has no hook that would put HIP
events around a single launch of a call.)  Without ``--kernel-db`` the field says "not measured"."""
import argparse
import json
import glob
import os
import re
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def copies_of(csr, L, length):
    """The pinned chain copies of every ring: (CSR of n_rings * L chains of length + 1 items, masks)."""
    cptr, gptr, attr = csr
    n_rings = len(cptr) - 1
    deg = np.diff(gptr).reshape(n_rings, length)
    deg = np.concatenate([deg, np.zeros((n_rings, 1), dtype=deg.dtype)], axis=1)          # the appended item has no attributes
    deg = np.repeat(deg, L, axis=0).ravel()
    copy_gptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    per_ring = [attr[gptr[cptr[c]]:gptr[cptr[c + 1]]] for c in range(n_rings)]
    copy_attr = np.concatenate([a for a in per_ring for _ in range(L)]).astype(np.int32)
    copy_cptr = (np.arange(n_rings * L + 1) * (length + 1)).astype(np.int32)
    allowed = np.full((n_rings, L, length + 1), (1 << L) - 1, dtype=np.uint32)
    allowed[:, :, 0] = allowed[:, :, -1] = (np.uint32(1) << np.arange(L, dtype=np.uint32))[None, :]
    return (copy_cptr, copy_gptr, copy_attr), allowed.ravel()


def kernel_times(directory, n_configs, reps):
    """Per label count {kernel: median microseconds over the traced repetitions}, from the dispatches of a --trace-pass run in
    start order: a configuration is 1 + reps blocks, each opened by the ring call's gl_state and closed by viterbi's last launch;
    the first block of every configuration (the warm-up) is dropped."""
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
    rows.sort(key=lambda r: r[1])
    def short(n):
        m = re.search(r"gl_\w+(<[^>]*>)?", n)
        return m.group(0) if m else n[:60]

    blocks, cur = [], None
    for n, s, e in rows:
        if "gl_ring_forward" in n and (cur is None or any("gl_ring_backtrack" in k for k, _ in cur)):
            # the launch before the first ring walk is the call's gl_state
            head = [cur.pop()] if cur else []
            cur = head
            blocks.append(cur)
        if cur is not None:
            cur.append((n, (e - s) / 1e3))
    if len(blocks) != n_configs * (reps + 1):
        raise SystemExit(f"{directory}: {len(blocks)} traced repetitions, expected {n_configs} configurations x (1 + {reps})")
    out = []
    for k in range(n_configs):
        acc = {}
        for block in blocks[k * (reps + 1) + 1:(k + 1) * (reps + 1)]:
            seen = {}
            for n, us in block:
                key = short(n)
                seen[key] = seen.get(key, 0.0) + us  # (a kernel launched twice in a block: summed)
            for key, us in seen.items():
                acc.setdefault(key, []).append(us)
        out.append({key: float(np.median(v)) for key, v in acc.items()})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--evals", type=int, default=30)
    ap.add_argument("--copy-evals", type=int, default=5)
    ap.add_argument("--no-copies", action="store_true", help="leave the copy route out")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace-pass", action="store_true", help="only the calls to be traced, untimed")
    ap.add_argument("--trace-reps", type=int, default=30)
    ap.add_argument("--kernel-db", default=None, help="directory of the rocprofv3 run of --trace-pass")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n_labels = len(args.labels.split(","))
    kernels = kernel_times(args.kernel_db, n_labels, args.trace_reps) if args.kernel_db else None
    import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

    from gecco_amd import _native, synth
    from tools.bench_constrained import timed_in_turn

    if _native.device_count() < 1:
        raise SystemExit("bench_ring needs a HIP device")
    has_entry = hasattr(_native.load_library(), "gecco_crf_ring")
    lines = []
    for k, L in enumerate(int(x) for x in args.labels.split(",")):
        rng = np.random.default_rng(synth.SEED + L)
        model = _native.Model.from_tables(rng.normal(0, 0.5, size=(args.attrs, L)), rng.normal(0, 0.5, size=(L, L)))
        csr = synth.synth_contigs(rng, [args.length] * args.sequences, args.attrs)
        dev, n = args.device, int(csr[0][-1])
        fns = {"marginals_full": lambda: model.marginals_full(*csr, device=dev), "viterbi": lambda: model.viterbi(*csr, device=dev)}
        if has_entry:
            fns.update({"ring_lognorm": lambda: model.ring(*csr, device=dev, want_path=False, want_marginals=False),
                        "ring_marginals": lambda: model.ring(*csr, device=dev, want_path=False),
                        "ring_path": lambda: model.ring(*csr, device=dev, want_marginals=False),
                        "ring": lambda: model.ring(*csr, device=dev)})
        if args.trace_pass:
            for _ in range(args.trace_reps + 1):
                model.ring(*csr, device=dev)
                model.marginals_full(*csr, device=dev)
                model.viterbi(*csr, device=dev)
            continue
        out = {"tool": "bench_ring", "library": "with gecco_crf_ring" if has_entry else "without gecco_crf_ring", "labels": L, "items": n,
               "sequences": args.sequences, "attrs": args.attrs, "entries": int(len(csr[2])), "warmup": args.warmup,
               "evals_timed": args.evals, "workspace_bytes": 8 * (n * L * L + n + args.sequences) + n * L}
        out.update(timed_in_turn(fns, args.warmup, args.evals))
        med = lambda name: out[name]["hip_event_us"][0]  # noqa: E731
        if has_entry:
            out["backward_stores_and_download_us"] = med("ring_marginals") - med("ring_lognorm")
            out["decode_passes_us"] = med("ring_path") - med("ring_lognorm")
            out["ring_lognorm_over_marginals_full"] = med("ring_lognorm") / med("marginals_full")
            out["ring_path_over_viterbi"] = med("ring_path") / med("viterbi")
        if not args.no_copies:
            copies, allowed = copies_of(csr, L, args.length)
            route = {"copies_marginals": lambda: model.marginals_full(*copies, device=dev, allowed=allowed),
                     "copies_viterbi": lambda: model.viterbi(*copies, device=dev, allowed=allowed)}
            out.update(timed_in_turn(route, 1, args.copy_evals))
            marg, lognorm = route["copies_marginals"]()
            t0 = time.perf_counter()
            ln = lognorm.reshape(args.sequences, L)
            top = ln.max(axis=1)
            total = top + np.log(np.exp(ln - top[:, None]).sum(axis=1))
            weight = np.exp(ln - total[:, None])
            mix = (marg.reshape(args.sequences, L, args.length + 1, L)[:, :, :args.length, :] * weight[:, :, None, None]).sum(axis=1)
            out["copies_host_reduction_us"] = (time.perf_counter() - t0) * 1e6
            out["copies_evals_timed"] = args.copy_evals
            if has_entry:
                got = model.ring(*csr, device=dev, want_path=False)
                out["lognorm_against_copies_worst"] = float(np.abs(got["lognorm"] - total).max())
                out["marginals_against_copies_worst"] = float(np.abs(got["marginals"] - mix.reshape(n, L)).max())
                out["ring_over_copy_route"] = med("ring") / (med("copies_marginals") + med("copies_viterbi") + out["copies_host_reduction_us"])
        out["kernel_us"] = "not measured" if kernels is None else dict(
            kernels[k], source=f"rocprofv3 --kernel-trace --stats, median of {args.trace_reps} repetitions")
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out and lines:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
