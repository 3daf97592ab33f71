"""Training benchmark (not bench.py): objective + gradient evaluations of gecco_crf_trainer_eval and a whole L-BFGS /
OWL-QN fit on a synthetic labelled set from gecco_amd.synth, against a single-thread numpy port of the same objective.

    python tools/bench_train.py [--items 1000000] [--windows 20,5] [--c1 0.15] [--c2 0.15] [--out FILE]

Per window size it prints one JSON line: microseconds per evaluation (weights up, f and g down, synchronous), window
positions per second, the bytes an evaluation has to move at least and the share of the HBM peak that makes, the
fit's iterations / evaluations / wall time, and the numpy port's time per evaluation (on a prefix of the set, scaled to
the whole of it by window count)."""
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

from benchkit.train_objective import objective as numpy_objective  # noqa: E402
from gecco_amd import _native, synth, train  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E peak


def min_bytes(n_items, nnz, n_win, W, A):
    """Traffic an evaluation cannot avoid with this kernel layout: CSR + scores, window starts and labels, the per-window
    node marginals written and read back, the window rows, the transpose and the item marginals it gathers."""
    return (4 * (n_items + 1) + 4 * nnz + 16 * n_items          # item scores
            + 16 * n_items + 4 * n_items + 4 * n_win             # windows: scores, labels, starts
            + 16 * n_win * W + 40 * n_win                        # node marginals + rows written
            + 16 * n_win * W + 12 * n_items + 16 * n_items       # item marginals
            + 4 * (A + 1) + 4 * nnz + 16 * nnz + 16 * A          # attribute counts
            + 40 * n_win)                                        # row sums


def run(W, args):
    rng = np.random.default_rng(synth.SEED + W)
    lengths = synth.contig_lengths(rng, max(1, args.items // 200), total_genes=args.items)
    lengths = np.maximum(lengths, W)
    seq_ptr, item_ptr, attr_id, labels = synth.synth_training_set(rng, lengths, args.attrs)
    A, K = args.attrs, 2 * args.attrs + 4
    sfid, tfid = np.arange(2 * A, dtype=np.int32), 2 * A + np.arange(4, dtype=np.int32)
    t0 = time.perf_counter()
    tr = _native.Trainer(seq_ptr, item_ptr, attr_id, labels, A, W, 1, sfid, tfid, K)
    t_create = time.perf_counter() - t0
    n_win = tr.num_windows
    w = rng.normal(0, 0.5, size=K)
    for _ in range(3):
        tr.eval(w)
    times = []
    for _ in range(args.evals):
        t0 = time.perf_counter()
        f, g = tr.eval(w)
        times.append(time.perf_counter() - t0)
    t_eval = float(np.median(times))
    nbytes = min_bytes(int(seq_ptr[-1]), int(item_ptr[-1]), n_win, W, A)

    # whole fit from w = 0 (c1 > 0: OWL-QN), the trainer's defaults otherwise
    params = train.trainer_params({"c1": args.c1, "c2": args.c2, "max_iterations": args.max_iterations})
    c2 = float(params["c2"])

    def fg(x):
        fv, gv = tr.eval(x)
        return fv + c2 * float(x @ x), gv + 2 * c2 * x

    t0 = time.perf_counter()
    res = train.minimize(fg, np.zeros(K), c1=float(params["c1"]), num_memories=int(params["num_memories"]),
                         epsilon=float(params["epsilon"]), period=int(params["period"]), delta=float(params["delta"]),
                         max_iterations=params["max_iterations"])
    t_fit = time.perf_counter() - t0

    # CPU yardstick on a prefix of the sequences (about args.cpu_items items), scaled by windows
    ns = int(np.searchsorted(seq_ptr, min(args.cpu_items, int(seq_ptr[-1])), side="right"))
    ns = max(1, min(ns, len(seq_ptr) - 1))
    sp = seq_ptr[:ns + 1]
    ip = item_ptr[:int(sp[-1]) + 1]
    t0 = time.perf_counter()
    fc, gc, nw_cpu = numpy_objective(sp, ip, attr_id[:int(ip[-1])], labels[:int(sp[-1])], A, W, 1, sfid, tfid, w)
    t_cpu = time.perf_counter() - t0
    # the device's objective on the same prefix, for a check of the port
    tr_small = _native.Trainer(sp, ip, attr_id[:int(ip[-1])], labels[:int(sp[-1])], A, W, 1, sfid, tfid, K)
    fd, gd = tr_small.eval(w)
    return {
        "tool": "bench_train", "window": W, "items": int(seq_ptr[-1]), "attrs": A, "nnz": int(item_ptr[-1]),
        "windows": n_win, "features": K, "create_s": t_create,
        "eval_us": t_eval * 1e6, "eval_us_min": min(times) * 1e6, "evals_timed": args.evals,
        "window_positions_per_s": n_win * W / t_eval,
        "min_bytes_per_eval": nbytes, "achieved_GBps": nbytes / t_eval / 1e9, "hbm_peak_GBps": HBM_PEAK_GBPS,
        "hbm_frac": nbytes / t_eval / 1e9 / HBM_PEAK_GBPS,
        "fit": {"c1": args.c1, "c2": args.c2, "iterations": res.n_iter, "evaluations": res.n_eval, "status": res.status,
                "wall_s": t_fit, "objective": res.f, "nonzero_weights": int(np.count_nonzero(res.x))},
        "cpu_baseline": {"kind": "single-thread numpy port of the objective (not CRFsuite)", "items": int(sp[-1]),
                         "windows": nw_cpu, "eval_s": t_cpu,
                         "eval_s_scaled_to_set": t_cpu * n_win / max(nw_cpu, 1),
                         "speedup_vs_device": t_cpu * n_win / max(nw_cpu, 1) / t_eval,
                         "rel_diff_f_vs_device": abs(fc - fd) / abs(fc),
                         "max_diff_g_vs_device": float(np.max(np.abs(gc - gd) / (1 + np.abs(gc))))},
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--windows", default="20,5")
    ap.add_argument("--c1", type=float, default=0.15)
    ap.add_argument("--c2", type=float, default=0.15)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--max-iterations", type=int, default=1000)
    ap.add_argument("--cpu-items", type=int, default=50_000)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    for W in [int(x) for x in args.windows.split(",")]:
        line = json.dumps(run(W, args))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
