"""Hyperparameter search benchmark (not bench.py): ``cv.grid_search`` over a c1 x c2 x window grid against a loop of
``cv.cross_validate`` over the same points, on labelled genes built from a synthetic training set
(``synth.synth_training_set``: one domain per item, named after its attribute id).

    python tools/bench_tune.py [--items 1000000] [--folds 5] [--max-iterations 100] [--out FILE]

Prints one JSON line: the wall time of both, the peak device memory of each above the start (the library allocates
outside torch's allocator, so the device's used memory is sampled: ``*_peak_used_gib``), and whether every
(point, fold)'s fit, probabilities and metrics are bitwise the loop's."""
import argparse
import json
import os
import random
import sys
import threading
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gecco_amd import cv, synth  # noqa: E402
from gecco_amd.crf import ClusterCRF  # noqa: E402
from gecco_amd.model import Domain, Gene, Protein, Source, Strand  # noqa: E402


def genes_of(seq_ptr, item_ptr, attr_id, labels):
    """Labelled genes: sequence s holds genes seq_ptr[s] .. seq_ptr[s + 1], gene i the domains of its attributes."""
    genes = []
    for s in range(len(seq_ptr) - 1):
        src = Source(f"seq{s:06d}")
        for i in range(int(seq_ptr[s]), int(seq_ptr[s + 1])):
            j = i - int(seq_ptr[s])
            doms = [Domain(f"PF{int(a):05d}", 10 * k, 10 * k + 9, "Pfam", 1e-5, 1e-6, probability=float(labels[i]))
                    for k, a in enumerate(attr_id[item_ptr[i]:item_ptr[i + 1]].tolist())]
            genes.append(Gene(src, 1000 * j + 1, 1000 * j + 900, Strand.Coding, Protein(f"{src.id}_g{j}", None, doms),
                              _probability=float(labels[i])))
    return genes


class PeakMemory:
    """Samples the device's used memory (torch.cuda.mem_get_info: total - free, all allocations of the device) every few
    ms on a thread: the peak over the run, in bytes."""

    def __init__(self):
        import torch

        self.torch = torch
        self.peak = 0
        self._stop = threading.Event()

    def used(self):
        free, total = self.torch.cuda.mem_get_info(0)
        return total - free

    def __enter__(self):
        self.base = self.used()
        self.peak = self.base

        def run():
            while not self._stop.is_set():
                self.peak = max(self.peak, self.used())
                time.sleep(0.002)

        self._t = threading.Thread(target=run, daemon=True)
        self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join()
        self.peak = max(self.peak, self.used())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--c1", default="0,0.4")
    ap.add_argument("--c2", default="0,1")
    ap.add_argument("--window-size", default="5,20")
    ap.add_argument("--max-iterations", type=int, default=100)
    ap.add_argument("--skip-loop", action="store_true", help="time grid_search only")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    os.environ["GECCO_AMD_FIT"] = "native"
    grid = {"c1": [float(x) for x in args.c1.split(",")], "c2": [float(x) for x in args.c2.split(",")],
            "window_size": [int(x) for x in args.window_size.split(",")]}
    rng = np.random.default_rng(synth.SEED + args.items)
    W = max(grid["window_size"])
    lengths = np.maximum(synth.contig_lengths(rng, max(1, args.items // 200), total_genes=args.items), W)
    t0 = time.perf_counter()
    genes = genes_of(*synth.synth_training_set(rng, lengths, args.attrs))
    t_genes = time.perf_counter() - t0
    print(f"genes: {len(genes)} in {t_genes:.1f} s", file=sys.stderr, flush=True)

    def template(c1=0.15, c2=0.15, w=5):
        return ClusterCRF("protein", window_size=w, window_step=1, c1=c1, c2=c2, max_iterations=args.max_iterations)

    warnings.simplefilter("ignore")
    cv.cross_validate(template(), genes[:5000], 2)  # (warm-up: library, device, code objects)
    random.seed(1)
    with PeakMemory() as mem_grid:
        t0 = time.perf_counter()
        res = cv.grid_search(template(), genes, args.folds, grid)
        t_grid = time.perf_counter() - t0
    print(f"grid_search: {t_grid:.1f} s", file=sys.stderr, flush=True)
    rec = {"bench": "tune_grid", "items": len(genes), "folds": args.folds, "grid": grid, "points": len(res.points),
           "max_iterations": args.max_iterations, "genes_build_s": t_genes, "grid_search_s": t_grid,
           "grid_peak_used_gib": (mem_grid.peak - mem_grid.base) / 2**30,
           "best": res.best_point, "mean_aupr": res.mean_aupr}
    if not args.skip_loop:
        same = True
        t_loop = 0.0
        with PeakMemory() as mem_loop:
            for p, pt in enumerate(res.points):
                random.seed(1)
                t0 = time.perf_counter()
                alone = cv.cross_validate(template(pt["c1"], pt["c2"], pt["window_size"]), genes, args.folds)
                t_loop += time.perf_counter() - t0
                print(f"cross_validate point {p + 1}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
                for fold, ref in zip(res.folds[p], alone.folds):
                    probs = np.array([g.average_probability for g in ref.predicted])
                    same &= (fold.crf.training_result_.x.tobytes() == ref.crf.training_result_.x.tobytes()
                             and fold.probabilities.tobytes() == probs.tobytes()
                             and np.float64(fold.aupr).tobytes() == np.float64(ref.aupr).tobytes())
        rec.update({"cross_validate_loop_s": t_loop, "speedup": t_loop / t_grid,
                    "loop_peak_used_gib": (mem_loop.peak - mem_loop.base) / 2**30, "bitwise_equal": bool(same)})
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
