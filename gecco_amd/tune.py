"""Hyperparameter search for the CRF: a cross-validated grid over ``c1``, ``c2`` and the window size (``cv.grid_search``).

Every (point, fold) is what ``python -m gecco_amd.cv`` gives for that point with the same options and seed, but the
work shared between points is done once and all fits run together on the device (``train.fit_grid``).

    python -m gecco_amd.tune --genes G.tsv --features F.tsv --clusters C.tsv --c1 0 0.4 --c2 0 1 --window-size 5 20

It writes one row per (point, fold) to ``-o`` (``tune.tsv``) and one row per point to ``--summary``
(``tune.summary.tsv``), and prints the winning options as ``python -m gecco_amd.train`` takes them.
"""
import argparse
import random
import sys
from typing import List, Optional

import numpy as np

from . import cv, tables


def _values(kind):
    """argparse type of one list entry: a number, or several separated by commas."""
    def parse(text: str):
        try:
            return [kind(x) for x in text.split(",") if x.strip() != ""]
        except ValueError:
            raise argparse.ArgumentTypeError(f"invalid {kind.__name__} value: {text!r}") from None
    return parse


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m gecco_amd.tune", description=(
        "Cross-validate a grid of CRF hyperparameters (c1, c2, window size) on labelled tables, every fit on the device."))
    ap.add_argument("--genes", required=True, help="genes table (TSV)")
    ap.add_argument("--features", required=True, nargs="+", help="features table(s) (TSV)")
    ap.add_argument("--clusters", required=True, help="clusters table (TSV): the genes overlapping a cluster are positive")
    ap.add_argument("--e-filter", type=float, default=None,
                    help="accepted as gecco cv accepts it, and ignored as gecco cv ignores it")
    ap.add_argument("--p-filter", type=float, default=1e-9,
                    help="accepted as gecco cv accepts it, and ignored as gecco cv ignores it")
    ap.add_argument("--no-shuffle", dest="shuffle", action="store_false", help="do not shuffle the sequences")
    ap.add_argument("--seed", type=int, default=42, help="seed of random and numpy.random")
    ap.add_argument("--feature-type", choices=("protein", "domain"), default="protein")
    ap.add_argument("--window-step", type=int, default=1)
    ap.add_argument("--c1", type=_values(float), nargs="+", default=[[0.15]], help="values of c1 (L1 strength)")
    ap.add_argument("--c2", type=_values(float), nargs="+", default=[[0.15]], help="values of c2 (L2 strength)")
    ap.add_argument("--window-size", type=_values(int), nargs="+", default=[[5]], help="window sizes (1 to 32)")
    ap.add_argument("--miss-cost", type=_values(float), nargs="+", default=None,
                    help="values of the training cost of a missed cluster gene (an axis of the grid; 0: no cost)")
    ap.add_argument("--select", type=float, default=None, help="fraction of domains kept by Fisher selection")
    ap.add_argument("--correction", default=None, help="multiple-testing correction of the selection p-values")
    ap.add_argument("--loto", action="store_true", help="leave-one-type-out instead of K-fold cross-validation")
    ap.add_argument("--splits", type=int, default=10, help="number of folds (K-fold)")
    ap.add_argument("--metric", choices=cv.METRICS, default="aupr", help="what ranks the points (then the other metric)")
    ap.add_argument("-o", "--output", default="tune.tsv", help="one row per (point, fold)")
    ap.add_argument("--summary", default="tune.summary.tsv", help="one row per point")
    return ap


def parse_args(argv: Optional[List[str]] = None):
    """The options, and the grid they give (``cv.grid_points``); argument errors exit as argparse does."""
    ap = parser()
    args = ap.parse_args(argv)
    grid = {"c1": [v for vs in args.c1 for v in vs], "c2": [v for vs in args.c2 for v in vs],
            "window_size": [v for vs in args.window_size for v in vs]}
    if args.miss_cost is not None:
        grid[cv.COST_KEY] = [v for vs in args.miss_cost for v in vs]
    try:
        points = cv.grid_points(grid)
    except ValueError as err:
        ap.error(str(err))
    if args.window_step < 1 or args.window_step > min(grid["window_size"]):
        ap.error(f"--window-step {args.window_step} must be in 1 .. the smallest window size ({min(grid['window_size'])})")
    if args.select is not None and not 0 < args.select <= 1:
        ap.error(f"--select {args.select} must be in (0, 1]")
    return args, grid, points


def train_command(args, point) -> str:
    """The winning options as ``python -m gecco_amd.train`` takes them."""
    words = ["python -m gecco_amd.train", "--feature-type", args.feature_type, "--window-size", str(point["window_size"]),
             "--window-step", str(args.window_step), "--c1", repr(float(point["c1"])), "--c2", repr(float(point["c2"]))]
    if point.get(cv.COST_KEY):
        words += ["--miss-cost", repr(float(point[cv.COST_KEY]))]
    if args.select is not None:
        words += ["--select", repr(args.select)]
    if args.correction is not None:
        words += ["--correction", args.correction]
    if not args.shuffle:
        words.append("--no-shuffle")
    return " ".join(words)


def main(argv: Optional[List[str]] = None) -> int:
    from .crf import ClusterCRF

    args, grid, points = parse_args(argv)
    random.seed(args.seed)
    np.random.seed(args.seed)
    genes = tables.GeneTable.load(args.genes).to_genes()
    for path in args.features:
        genes = cv.annotate_genes(genes, tables.FeatureTable.load(path))
    clusters = tables.ClusterTable.load(args.clusters)
    genes = cv.label_genes(genes, clusters)

    crf = ClusterCRF(args.feature_type, algorithm="lbfgs", window_size=points[0]["window_size"],
                     window_step=args.window_step, c1=points[0]["c1"], c2=points[0]["c2"])
    if args.loto:
        def splits(seqs):
            return list(cv.LeaveOneGroupOut().split(seqs, groups=cv.loto_groups(seqs, clusters)))
    else:
        splits = args.splits
    result = cv.grid_search(crf, genes, splits, grid, shuffle=args.shuffle, select=args.select,
                            correction_method=args.correction, metric=args.metric)
    for p, pt in enumerate(result.points):
        print(f"c1={pt['c1']} c2={pt['c2']} window_size={pt['window_size']}"
              f"{' miss_cost=%s' % pt[cv.COST_KEY] if cv.COST_KEY in pt else ''}: mean AUROC={result.mean_auroc[p]:.3f} "
              f"mean AUPR={result.mean_aupr[p]:.3f}", file=sys.stderr)
    with open(args.output, "wb") as out:
        out.write(result.table())
    with open(args.summary, "wb") as out:
        out.write(result.summary())
    print(train_command(args, result.best_point))
    return 0


if __name__ == "__main__":
    sys.exit(main())
