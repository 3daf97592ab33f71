"""The hyperparameter search on the host: grid parsing, ranking and its tie-breaks, the two TSV layouts and the front
end's argument errors (gecco_amd/cv.py, gecco_amd/tune.py)."""
import math
import subprocess
import sys

import numpy as np
import pytest

from gecco_amd import cv, tune

ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))


def test_grid_points_are_the_product_in_grid_order():
    pts = cv.grid_points({"c1": [0, 0.4], "c2": [0.0, 1], "window_size": [5, 8]})
    assert [(p["c1"], p["c2"], p["window_size"]) for p in pts] == [
        (0, 0.0, 5), (0, 0.0, 8), (0, 1, 5), (0, 1, 8), (0.4, 0.0, 5), (0.4, 0.0, 8), (0.4, 1, 5), (0.4, 1, 8)]
    # values are kept as given (they are stored with the model's options); window sizes become ints
    assert type(pts[0]["c1"]) is int and type(pts[-1]["window_size"]) is int


def test_grid_points_fill_missing_keys_from_the_template():
    from gecco_amd.crf import ClusterCRF

    crf = ClusterCRF("protein", window_size=7, window_step=1, c1=0.25)
    pts = cv.grid_points({"c2": [0, 2]}, crf)
    assert pts == [{"c1": 0.25, "c2": 0, "window_size": 7}, {"c1": 0.25, "c2": 2, "window_size": 7}]
    # no c2 in the template: the trainer's default
    assert cv.grid_points({}, ClusterCRF("protein")) == [{"c1": 0.0, "c2": 1.0, "window_size": 5}]


@pytest.mark.parametrize("grid,match", [
    ({"c1": [], "c2": [0], "window_size": [5]}, "empty list of values for 'c1'"),
    ({"c1": [0], "c2": [0], "window_size": []}, "empty list of values for 'window_size'"),
    ({"c1": [0], "c2": [0], "window_size": [33]}, "window_size 33 is not an integer in 1 .. 32"),
    ({"c1": [0], "c2": [0], "window_size": [0]}, "window_size 0"),
    ({"c1": [0], "c2": [0], "window_size": [4.5]}, "window_size 4.5"),
    ({"c1": [-0.1], "c2": [0], "window_size": [5]}, "c1 -0.1 is not a finite value >= 0"),
    ({"c1": [0], "c2": [math.inf], "window_size": [5]}, "c2 inf"),
    ({"c1": [0], "c2": [0], "window_size": [5], "c3": [1]}, "unknown parameter"),
    ({"c2": [0], "window_size": [5]}, "no values for 'c1'"),
])
def test_grid_points_refuse_bad_grids(grid, match):
    with pytest.raises(ValueError, match=match):
        cv.grid_points(grid)


def test_ranking_by_metric_then_the_other_then_grid_order():
    auroc = [0.8, 0.9, 0.9, math.nan, 0.7]
    aupr = [0.5, 0.5, 0.5, 0.9, math.nan]
    # aupr first: point 3 (0.9); then 0.5 ties broken by auroc (1 and 2 tie again: grid order), then 0; NaN last
    assert cv.rank_points(auroc, aupr) == [3, 1, 2, 0, 4]
    assert cv.rank_points(auroc, aupr, "auroc") == [1, 2, 0, 4, 3]
    assert cv.rank_points([0.5, 0.5], [0.5, 0.5]) == [0, 1]
    with pytest.raises(ValueError, match="metric must be one of"):
        cv.rank_points(auroc, aupr, "f1")


def _fold(index, auroc, aupr, probs, truth, n_train=3, n_test=1):
    return cv.GridFold(index=index, train=np.arange(n_train), test=np.arange(n_test), crf=None,
                       keys=[("s", f"g{i}", i, i) for i in range(len(probs))], probabilities=np.asarray(probs, dtype=float),
                       truth=list(truth), auroc=auroc, aupr=aupr)


def _search():
    points = cv.grid_points({"c1": [0, 0.4], "c2": [1], "window_size": [5]})
    folds = [[_fold(1, 0.75, 0.5, [0.1, 0.9], [False, True]), _fold(2, math.nan, 0.25, [0.2, 0.3], [False, False])],
             [_fold(1, 0.5, 0.5, [0.6, 0.4], [False, True]), _fold(2, 1.0, 1.0, [0.1, 0.8], [False, True])]]
    return cv.GridSearch(points, folds, "aupr")


def test_search_means_skip_nan_folds_and_pool_like_cross_validation():
    res = _search()
    assert res.mean_auroc == [0.75, 0.75] and res.mean_aupr == [0.375, 0.75]
    labels = [False, True, False, False]
    assert res.auroc[0] == cv.roc_auc(labels, [0.1, 0.9, 0.2, 0.3])
    assert res.aupr[0] == cv.average_precision(labels, [0.1, 0.9, 0.2, 0.3])
    assert res.ranking == [1, 0] and res.best == 1 and res.best_point == {"c1": 0.4, "c2": 1, "window_size": 5}


def test_tsv_layouts():
    res = _search()
    rows = [r.split("\t") for r in res.table().decode().splitlines()]
    assert rows[0] == ["point", "c1", "c2", "window_size", "fold", "n_train", "n_test", "auroc", "aupr"]
    assert rows[1:] == [["1", "0.0", "1.0", "5", "1", "3", "1", "0.75", "0.5"],
                        ["1", "0.0", "1.0", "5", "2", "3", "1", "nan", "0.25"],
                        ["2", "0.4", "1.0", "5", "1", "3", "1", "0.5", "0.5"],
                        ["2", "0.4", "1.0", "5", "2", "3", "1", "1.0", "1.0"]]
    rows = [r.split("\t") for r in res.summary().decode().splitlines()]
    assert rows[0] == ["point", "c1", "c2", "window_size", "mean_auroc", "mean_aupr", "auroc", "aupr", "rank"]
    assert [r[0] for r in rows[1:]] == ["1", "2"] and [r[-1] for r in rows[1:]] == ["2", "1"]
    assert rows[2][4:6] == ["0.75", "0.75"]
    assert rows[1][6] == repr(res.auroc[0])


def test_front_end_parses_lists_and_prints_the_train_options():
    args, grid, points = tune.parse_args(["--genes", "g", "--features", "f", "--clusters", "c", "--c1", "0", "0.4",
                                          "--c2", "0,1", "--window-size", "5", "8", "--select", "0.5"])
    assert grid == {"c1": [0.0, 0.4], "c2": [0.0, 1.0], "window_size": [5, 8]} and len(points) == 8
    assert args.splits == 10 and args.seed == 42 and args.metric == "aupr" and args.shuffle
    assert tune.train_command(args, points[-1]) == ("python -m gecco_amd.train --feature-type protein --window-size 8 "
                                                    "--window-step 1 --c1 0.4 --c2 1.0 --select 0.5")
    _, grid, points = tune.parse_args(["--genes", "g", "--features", "f", "--clusters", "c"])
    assert grid == {"c1": [0.15], "c2": [0.15], "window_size": [5]}  # (cv's defaults: one point)


@pytest.mark.parametrize("extra,match", [
    (["--window-size", "40"], "window_size 40 is not an integer in 1 .. 32"),
    (["--c1", "-1"], "c1 -1.0 is not a finite value >= 0"),
    (["--c2", "x"], "invalid float value"),
    (["--window-size", "5", "--window-step", "6"], "--window-step 6"),
    (["--select", "0"], "--select 0.0"),
    (["--metric", "f1"], "invalid choice"),
])
def test_front_end_argument_errors(extra, match):
    cmd = [sys.executable, "-m", "gecco_amd.tune", "--genes", "g", "--features", "f", "--clusters", "c"] + extra
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 2 and match in proc.stderr, proc.stderr
