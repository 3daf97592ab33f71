"""The hyperparameter search on the device: the grid trainer (gecco_crf_trainer_grid_*) is bitwise the lone trainer of
each problem's set, whatever shares the launch; ``cv.grid_search`` is bitwise ``cross_validate`` run alone for every
point; ``python -m gecco_amd.tune`` writes what the API computes."""
import os
import random
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests.helpers import lone_trainer, same_bits, training_set
from tests.test_gpu_cv import _dataset, _model_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = {"c1": [0.0, 0.4], "c2": [0.0, 1.0], "window_size": [5, 8]}


def _sets(seed):
    """Mixed windows and steps, one set with more than 256 x 64 windows."""
    rng = np.random.default_rng(seed)
    return [training_set(rng, 5, 1, 90, 300, max_extra=120), training_set(rng, 20, 3, 40, 30), training_set(rng, 32, 1, 7, 3),
            training_set(rng, 1, 1, 60, 20), training_set(rng, 8, 2, 113, 25, drop=0.5)]


def test_grid_trainer_is_bitwise_the_lone_trainers():
    from gecco_amd import _native

    sets = _sets(4100)
    lone = [lone_trainer(s) for s in sets]
    # 10 problems on set 0 (more than one item group of 8), 3 on set 1, one on each other set, interleaved
    problem_set = [0, 1, 0, 2, 0, 0, 1, 3, 0, 0, 0, 4, 0, 1, 0]
    rng = np.random.default_rng(7)
    ws = [rng.normal(0, 1.5, size=sets[s][7]) for s in problem_set]
    masks = [np.ones(len(problem_set), dtype=bool)] + [rng.random(len(problem_set)) < 0.6 for _ in range(3)]
    sizes = None
    for budget in ("none", "third", "smallest"):
        if sizes is None:
            grid = _native.TrainerGrid(sets, problem_set, 0)
            sizes = [grid.scratch_bytes(k) for k in range(len(grid))]
        else:  # a third of all problems' scratch (several groups), or 1 byte (every problem capped at the largest one)
            grid = _native.TrainerGrid(sets, problem_set, sum(sizes) // 3 if budget == "third" else 1)
        assert len(grid) == len(problem_set)
        assert [grid.num_windows(k) for k in range(len(grid))] == [lone[s].num_windows for s in problem_set]
        assert [grid.scratch_bytes(k) for k in range(len(grid))] == sizes
        assert grid.scratch_bytes() == {"none": sum(sizes), "third": max(sum(sizes) // 3, max(sizes)),
                                        "smallest": max(sizes)}[budget]
        for mask in masks:
            f = np.full(len(problem_set), 12345.0)
            g = [np.full(sets[s][7], -7.0) for s in problem_set]
            grid.eval([w if m else None for w, m in zip(ws, mask)], mask, f, g)
            for k, s in enumerate(problem_set):
                if mask[k]:
                    ef, eg = lone[s].eval(ws[k])
                    assert same_bits(f[k], g[k], ef, eg), (budget, k)
                else:
                    assert f[k] == 12345.0 and np.all(g[k] == -7.0)


def test_extreme_problems_change_no_other():
    from gecco_amd import _native

    sets = _sets(4200)
    problem_set = [0, 0, 0, 1, 1, 4, 0]
    lone = [lone_trainer(s) for s in sets]
    rng = np.random.default_rng(3)
    for budget in (0, 1):
        grid = _native.TrainerGrid(sets, problem_set, budget)
        ws = [rng.normal(0, 1.5, size=sets[s][7]) for s in problem_set]
        for hot in (1, 3):  # transitions 720 / -800 apart: every window of that problem in log space
            tfid = sets[problem_set[hot]][6]
            for j, v in zip(range(4), (720.0, -800.0, 0.0, 720.0)):
                if tfid[j] >= 0:
                    ws[hot][tfid[j]] = v
        ws[2] = np.full_like(ws[2], np.nan)
        ws[5] = np.full_like(ws[5], np.inf)
        f, g = grid.eval(ws)
        assert not np.isfinite(f[2])
        for k, s in enumerate(problem_set):
            if k in (2, 5):
                continue
            ef, eg = lone[s].eval(ws[k])
            assert same_bits(f[k], g[k], ef, eg), (budget, k)


def test_grid_argument_errors_name_the_set_or_problem():
    from gecco_amd import _native

    sets = _sets(4300)
    bad = list(sets)
    bad[1] = sets[1][:8] + (33, 1)
    with pytest.raises(_native.NativeError, match="trainer grid: set 1: trainer: window of 33 items; windows of 1 to 32") \
            as err:
        _native.TrainerGrid(bad, [0, 1])
    assert err.value.code == _native.EUNSUPPORTED
    bad = list(sets)
    bad[3] = sets[3][:8] + (2, 1)  # longer than set 3's first sequence (1 item)
    with pytest.raises(ValueError, match="trainer grid: set 3: trainer: sequence 0 has fewer items than the window"):
        _native.TrainerGrid(bad, [3])
    with pytest.raises(ValueError, match="trainer grid: problem 1: set 7 out of range"):
        _native.TrainerGrid(sets, [0, 7])
    with pytest.raises(ValueError, match="trainer grid: at least one problem is needed"):
        _native.TrainerGrid(sets, [])

    from gecco_amd import cv
    from gecco_amd.crf import ClusterCRF

    genes, _ = _dataset()
    crf = ClusterCRF("protein", window_size=5, window_step=1, c1=0.15, c2=0.15)
    with pytest.raises(ValueError, match="empty list of values for 'c2'"):
        cv.grid_search(crf, genes, 3, {"c1": [0.1], "c2": [], "window_size": [5]})
    with pytest.raises(ValueError, match="window_size 33"):
        cv.grid_search(crf, genes, 3, {"c1": [0.1], "c2": [1.0], "window_size": [5, 33]})
    # a sequence shorter than the largest window: the reference's message, as cross_validate gives it for that point
    with pytest.raises(ValueError, match=r"not enough observations \(\d+\) for requested window size \(32\)"):
        cv.grid_search(crf, genes, 3, {"c1": [0.1], "c2": [1.0], "window_size": [5, 32]})


def test_fit_grid_is_fit_training_set_per_problem():
    from gecco_amd import train
    from gecco_amd.crf import ClusterCRF

    genes, _ = _dataset(seed=41)
    sets = []
    for W in (5, 8):
        random.seed(3)
        ts, _ = ClusterCRF("protein", window_size=W, window_step=1)._training_set(genes)
        sets.append(ts)
    problems = [(1, train.trainer_params({"c1": 0.4, "c2": 0.0})), (0, train.trainer_params({"c1": 0.0, "c2": 1.0})),
                (1, train.trainer_params({"c1": 0.0, "c2": 0.0, "max_iterations": 7})),
                (0, train.trainer_params({"c1": 0.4, "c2": 1.0}))]
    got = train.fit_grid(sets, problems, scratch_budget_bytes=1)
    for (s, params), r in zip(problems, got):
        e = train.fit_training_set(sets[s], params)
        assert (r.n_iter, r.n_eval, r.status) == (e.n_iter, e.n_eval, e.status) and r.n_iter > 0
        assert r.x.tobytes() == e.x.tobytes() and np.float64(r.f).tobytes() == np.float64(e.f).tobytes()
    with pytest.raises(ValueError, match="problem 0 names set 2"):
        train.fit_grid(sets, [(2, problems[0][1])])


def _nan_equal(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


@pytest.mark.parametrize("feature_type,select", [("protein", None), ("protein", 0.5), ("domain", None)])
def test_grid_search_is_cross_validate_per_point(tmp_path, monkeypatch, feature_type, select):
    from gecco_amd import cv
    from gecco_amd.crf import ClusterCRF

    monkeypatch.setenv("GECCO_AMD_FIT", "native")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        genes, _ = _dataset()
        random.seed(5)
        res = cv.grid_search(ClusterCRF(feature_type, window_size=5, window_step=1, c1=0.15, c2=0.15), genes, 3, GRID,
                             select=select)
        state = random.getstate()
        assert len(res.points) == 8 and all(len(fs) == 3 for fs in res.folds)
        for p, pt in enumerate(res.points):
            genes, _ = _dataset()
            random.seed(5)
            alone = cv.cross_validate(ClusterCRF(feature_type, window_size=pt["window_size"], window_step=1, c1=pt["c1"],
                                                 c2=pt["c2"]), genes, 3, select=select)
            assert random.getstate() == state
            for fold, ref in zip(res.folds[p], alone.folds):
                a, b = fold.crf.training_result_, ref.crf.training_result_
                assert (a.n_iter, a.n_eval, a.status) == (b.n_iter, b.n_eval, b.status) and a.n_iter > 0
                assert a.x.tobytes() == b.x.tobytes()
                assert fold.crf.significant_features == ref.crf.significant_features
                assert (_model_bytes(fold.crf, str(tmp_path / f"a{p}_{fold.index}"))
                        == _model_bytes(ref.crf, str(tmp_path / f"b{p}_{fold.index}")))
                assert fold.keys == [cv._gene_key(g) for g in ref.predicted]
                expected = np.array([g.average_probability for g in ref.predicted], dtype=np.float64)
                assert fold.probabilities.tobytes() == expected.tobytes()
                assert fold.truth == ref.truth
                assert _nan_equal(fold.auroc, ref.auroc) and _nan_equal(fold.aupr, ref.aupr)
            assert _nan_equal(res.auroc[p], alone.auroc) and _nan_equal(res.aupr[p], alone.aupr)
    if feature_type == "protein":  # the points differ: the search has something to rank
        assert len(set(res.mean_aupr)) > 1
    assert res.ranking == cv.rank_points(res.mean_auroc, res.mean_aupr, "aupr")


def test_front_end_writes_what_the_api_computes(tmp_path):
    from gecco_amd import cv, tables
    from gecco_amd.crf import ClusterCRF

    genes, clusters = _dataset(seed=31)
    gpath, fpath, cpath = tmp_path / "g.tsv", tmp_path / "f.tsv", tmp_path / "c.tsv"
    tables.GeneTable.from_genes(genes).dump(str(gpath))
    tables.FeatureTable.from_genes(genes).dump(str(fpath))
    clusters.dump(str(cpath))
    out, summary = tmp_path / "tune.tsv", tmp_path / "tune.summary.tsv"
    cmd = [sys.executable, "-m", "gecco_amd.tune", "--genes", str(gpath), "--features", str(fpath), "--clusters",
           str(cpath), "--splits", "3", "--seed", "7", "--c1", "0", "0.4", "--c2", "0,1", "--window-size", "5", "8",
           "--metric", "auroc", "-o", str(out), "--summary", str(summary)]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900,
                          env={**os.environ, "GECCO_AMD_FIT": "native"})
    assert proc.returncode == 0, proc.stderr

    random.seed(7)
    np.random.seed(7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded = cv.label_genes(cv.annotate_genes(tables.GeneTable.load(str(gpath)).to_genes(),
                                                  tables.FeatureTable.load(str(fpath))), tables.ClusterTable.load(str(cpath)))
        res = cv.grid_search(ClusterCRF("protein", window_size=5, window_step=1, c1=0.0, c2=0.0), loaded, 3, GRID,
                             metric="auroc")
    assert out.read_bytes() == res.table() and summary.read_bytes() == res.summary()
    assert len(out.read_bytes().decode().splitlines()) == 1 + 8 * 3
    best = res.best_point
    assert proc.stdout.strip() == (f"python -m gecco_amd.train --feature-type protein --window-size {best['window_size']} "
                                   f"--window-step 1 --c1 {float(best['c1'])!r} --c2 {float(best['c2'])!r}")
