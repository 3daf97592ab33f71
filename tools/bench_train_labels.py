"""Training benchmark by label count (a sibling of tools/bench_train.py): one objective + gradient evaluation of
gecco_crf_trainer_general_eval on a synthetic labelled set, per label count, against the single-thread numpy
yardstick of the tests and, at two labels, against gecco_crf_trainer_eval on the same set.

    python tools/bench_train_labels.py [--items 200000] [--window 20] [--labels 2,8,32] [--out FILE]

Per label count it prints one JSON line: microseconds per evaluation, the scratch bytes of the problem, the numpy
yardstick's time (on a prefix of the set, scaled by window count) and, at L = 2, the ratio to the 2-label trainer.

The clock is the host's around the synchronous call, as in tools/bench_train.py, so the two tools compare: a time
holds the Python marshalling, the gather of the weights into the dense tables, the upload, the six launches, the
download and the scatter into g, and ends in the library's stream synchronise.  The library runs on a stream of its own
and exposes no events; the kernels' own times come from a kernel trace of this tool in a run of its own
(``rocprofv3 --kernel-trace --stats -- python tools/bench_train_labels.py --no-cpu ...``)."""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):  # the CPU yardstick runs on one thread
    os.environ.setdefault(_v, "1")

import argparse
import json
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gecco_amd import _native, synth  # noqa: E402
from tests.train_objective_labels import objective as numpy_objective  # noqa: E402


def labelled_set(rng, n_items, W, A, L, stay=0.95):
    """Sequences with synth's contig-length law, labels from a Markov chain over L labels, and synth's attributes moved
    by label so that the labels can be learned."""
    lengths = np.maximum(synth.contig_lengths(rng, max(1, n_items // 200), total_genes=n_items), W)
    seq_ptr, item_ptr, attr = synth.synth_contigs(rng, lengths, A)
    n = int(seq_ptr[-1])
    jump = rng.random(n) >= stay
    jump[0] = True
    drawn = rng.integers(0, L, size=n)
    labels = drawn[np.maximum.accumulate(np.where(jump, np.arange(n), 0))].astype(np.int32)
    owner = np.repeat(np.arange(n), np.diff(item_ptr))
    attr = ((attr + labels[owner].astype(np.int64) * A // L) % A).astype(np.int32)
    return seq_ptr, item_ptr, attr, labels


def timed(fn, warmup, evals):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(evals):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(min(times)), float(max(times))


def run(L, args):
    rng = np.random.default_rng(synth.SEED + L)
    W, A = args.window, args.attrs
    seq_ptr, item_ptr, attr_id, labels = labelled_set(rng, args.items, W, A, L)
    K = A * L + L * L
    sfid, tfid = np.arange(A * L, dtype=np.int32), A * L + np.arange(L * L, dtype=np.int32)
    tr = _native.TrainerGeneral([(seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K, W, 1)])
    w = rng.normal(0, 0.5, size=K)
    med, lo, hi = timed(lambda: tr.eval([w]), args.warmup, args.evals)
    n_win = tr.num_windows(0)
    out = {"tool": "bench_train_labels", "labels": L, "window": W, "items": int(seq_ptr[-1]), "attrs": A,
           "nnz": int(item_ptr[-1]), "windows": n_win, "features": K, "eval_us": med * 1e6, "eval_us_min": lo * 1e6,
           "eval_us_max": hi * 1e6, "evals_timed": args.evals, "ns_per_window_position": med * 1e9 / (n_win * W),
           "scratch_bytes": tr.scratch_bytes(0), "scratch_bytes_per_window": tr.scratch_bytes(0) / n_win,
           "one_block_per_window_bytes": 8 * L * L * n_win}
    if L == 2:
        two = _native.Trainer(seq_ptr, item_ptr, attr_id, labels, A, W, 1, sfid, tfid, K)
        # alternate the two trainers so that both see the same neighbours on the machine
        a, b = [], []
        for _ in range(args.warmup):
            two.eval(w), tr.eval([w])
        for _ in range(args.evals):
            t0 = time.perf_counter()
            f2, g2 = two.eval(w)
            t1 = time.perf_counter()
            f, g = tr.eval([w])
            t2 = time.perf_counter()
            a.append(t1 - t0)
            b.append(t2 - t1)
        out["two_label_trainer"] = {"eval_us": float(np.median(a)) * 1e6, "general_eval_us": float(np.median(b)) * 1e6,
                                    "general_over_two_label": float(np.median(b) / np.median(a)),
                                    "rel_diff_f": abs(f[0] - f2) / abs(f2),
                                    "max_diff_g": float(np.max(np.abs(g[0] - g2) / (1 + np.abs(g2))))}
    if args.no_cpu:
        return out
    ns = int(np.searchsorted(seq_ptr, min(args.cpu_items, int(seq_ptr[-1])), side="right"))
    ns = max(1, min(ns, len(seq_ptr) - 1))
    sp = seq_ptr[:ns + 1]
    ip = item_ptr[:int(sp[-1]) + 1]
    t0 = time.perf_counter()
    fc, gc, nw_cpu = numpy_objective(sp, ip, attr_id[:int(ip[-1])], labels[:int(sp[-1])], A, L, W, 1, sfid, tfid, w)
    t_cpu = time.perf_counter() - t0
    out["cpu_baseline"] = {"kind": "single-thread numpy yardstick (tests/train_objective_labels.py)", "items": int(sp[-1]),
                           "windows": nw_cpu, "eval_s": t_cpu, "eval_s_scaled_to_set": t_cpu * n_win / max(nw_cpu, 1),
                           "speedup_vs_device": t_cpu * n_win / max(nw_cpu, 1) / med}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--items", type=int, default=200_000)
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--evals", type=int, default=30)
    ap.add_argument("--cpu-items", type=int, default=10_000)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy yardstick (for a run under a profiler)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    for L in [int(x) for x in args.labels.split(",")]:
        line = json.dumps(run(L, args))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
