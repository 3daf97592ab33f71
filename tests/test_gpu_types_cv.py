"""Several forests in one launch (gecco_crf_forest_fit_batch / _predict_batch) and the type classifier's cross-validation
built on them (gecco_amd.types.cross_validate, python -m gecco_amd.types_cv).  Every comparison is of bits or digests: a
forest of a batch against the same problem fitted alone -- whatever the other problems are, in either order, twice -- and
against the trees sklearn 1.7.2 recorded per fold (tests/golden/types/forest_cv.json.gz <- tools/gen_type_cv_fixtures.py).
The sets come from tests/types_cv_sets.py, each at the smallest shape at which its way of going wrong can show."""
import gzip
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before libgecco_crf.so: the wheel's own HIP runtime has to be the first one loaded)

from gecco_amd import _native, types  # noqa: E402
from tests import types_cv_sets as sets  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = os.path.join(ROOT, "tests", "golden", "types")
ARRAYS = ("children_left", "children_right", "feature", "threshold", "impurity", "n_node_samples", "weighted_n_node_samples",
          "value")
DTYPES = dict(zip(ARRAYS, (np.int64, np.int64, np.int64, np.float64, np.float64, np.int64, np.float64, np.float64)))


@pytest.fixture(scope="module")
def ref():
    with gzip.open(os.path.join(TYPES, "forest_cv.json.gz")) as fh:
        doc = json.load(fh)
    assert doc["tree_arrays"] == list(ARRAYS)
    doc["by_name"] = {r["name"]: r for r in doc["cases"]}
    return doc


def _lone(X, y, **kw):
    return types.DeviceForest(**kw).fit(X, y)


def _assert_same_forest(got, exp, what):
    """Every exported array of every tree, bit for bit."""
    a, b = got.forest, exp.forest
    assert (a.n_trees, a.n_outputs, a.max_n_classes) == (b.n_trees, b.n_outputs, b.max_n_classes), what
    assert a.node_count.tolist() == b.node_count.tolist() and a.max_depth.tolist() == b.max_depth.tolist(), what
    assert got.seeds.tolist() == exp.seeds.tolist(), what
    for t in range(a.n_trees):
        x, y = got.export(t), exp.export(t)
        for name in ARRAYS:
            assert x[name].dtype == y[name].dtype and x[name].tobytes() == y[name].tobytes(), (what, t, name)


def _folds_of(case):
    fl = types.type_folds(len(case["labels"]), case["splits"], True, case["seed"])
    return fl, [case["X"][train] for train, _ in fl], [case["y"][train] for train, _ in fl]


def _kw(case):
    return dict(n_estimators=case["n_estimators"], random_state=case["random_state"])


def _cross_validate(case):
    return types.cross_validate(case["X"], case["labels"], classes=case["classes"], splits=case["splits"], seed=case["seed"], **_kw(case))


def _assert_cv_equals_lone_fits(case):
    """cross_validate's folds against each fold fitted and scored alone; returns the result."""
    res = _cross_validate(case)
    fl, Xs, ys = _folds_of(case)
    assert len(res.models) == len(fl)
    for i, ((train, test), X, y) in enumerate(zip(fl, Xs, ys)):
        assert res.folds[i][0].tolist() == train.tolist() and res.folds[i][1].tolist() == test.tolist()
        lone = _lone(X, y, **_kw(case))
        _assert_same_forest(res.models[i], lone, (case["name"], i))
        assert res.posit[test].tobytes() == lone.predict_posit(case["X"][test]).tobytes(), (case["name"], i)
        assert (res.fold[test] == i).all()
    return res


@pytest.fixture(scope="module")
def unequal():
    case = sets.build("unequal_61")
    fl, Xs, ys = _folds_of(case)
    return case, fl, Xs, ys, types.DeviceForest.fit_many(Xs, ys, **_kw(case))


def test_batch_of_one_equals_the_lone_fit():
    X, y = sets.training_set("small_12")
    assert X.shape == (12, 5) and y.shape == (12, 2)
    (one,) = types.DeviceForest.fit_many([X], [y], random_state=0)
    lone = _lone(X, y, random_state=0)
    _assert_same_forest(one, lone, "small_12")
    rows = np.concatenate([X, sets.threshold_rows(np.random.default_rng(1), [lone.export(t) for t in range(10)], 5, 24)])
    (got,) = _native.predict_forests([one.forest], [rows])
    assert got.tobytes() == lone.predict_posit(rows).tobytes() == one.predict_posit(rows).tobytes()


def test_three_unequal_problems_equal_their_lone_fits(unequal):
    case, fl, Xs, ys, batch = unequal
    assert [len(X) for X in Xs] == [40, 41, 41] and len(batch) * case["n_estimators"] == 300  # more workgroups than CUs
    for i, (X, y) in enumerate(zip(Xs, ys)):
        _assert_same_forest(batch[i], _lone(X, y, **_kw(case)), ("unequal_61", i))


def test_unequal_problems_in_reverse_order_and_again(unequal):
    case, fl, Xs, ys, batch = unequal
    rev = types.DeviceForest.fit_many(Xs[::-1], ys[::-1], **_kw(case))[::-1]
    again = types.DeviceForest.fit_many(Xs, ys, **_kw(case))
    for i in range(3):
        _assert_same_forest(rev[i], batch[i], ("reverse", i))
        _assert_same_forest(again[i], batch[i], ("again", i))


def test_mixed_class_counts_in_one_launch():
    res = _assert_cv_equals_lone_fits(sets.build("rare_type_one_fold"))
    k = res.classes.index("Rare")
    assert (res.posit[res.fold == 1][:, k] == 0.0).all()  # the fold that never saw the type gives it probability 0
    assert res.truth[res.fold == 1][:, k].sum() == 2
    res = _assert_cv_equals_lone_fits(sets.build("type_in_every_training_cluster"))
    assert (res.posit[res.fold == 2][:, 0] == 0.0).all()  # sklearn's 1 - proba[:, 0] of an output whose only class is "present"
    # every output one-class in one problem only: max_n_classes, hence the layout of `value`, differs within the launch
    case = sets.build("rare_type_one_fold")
    _, Xs, ys = _folds_of(case)
    ys = [np.zeros_like(ys[0])] + ys[1:]
    batch = types.DeviceForest.fit_many(Xs, ys, **_kw(case))
    assert [m.forest.max_n_classes for m in batch] == [1, 2, 2]
    for i, (X, y) in enumerate(zip(Xs, ys)):
        _assert_same_forest(batch[i], _lone(X, y, **_kw(case)), ("mixed max_n_classes", i))
    assert batch[0].forest.node_count.tolist() == [1] * case["n_estimators"]


def test_columns_empty_in_one_fold_only():
    _assert_cv_equals_lone_fits(sets.build("column_empty_in_one_fold"))


def test_smallest_n_is_a_root_leaf_per_fold():
    res = _assert_cv_equals_lone_fits(sets.build("smallest_n"))
    for m in res.models:  # one training sample: the smallest set the fit accepts
        assert m.forest.node_count.tolist() == [1] * 25 and m.forest.max_depth.tolist() == [0] * 25
    # each fold knows its one cluster's types as the only class of every output: "present" scores 0, like sklearn
    assert res.posit.tolist() == [[0.0, 0.0], [0.0, 0.0]]


def test_a_problem_at_the_sample_limit_beside_a_small_one():
    big, small = sets.training_set("limit_4096"), sets.training_set("small_12")
    assert len(big[0]) == 4096  # kForestMaxSamples (include/gecco_crf.h: n_samples <= 4096)
    Xs = [big[0], np.pad(small[0], ((0, 0), (0, big[0].shape[1] - small[0].shape[1])))]
    ys = [big[1], small[1]]
    batch = types.DeviceForest.fit_many(Xs, ys, n_estimators=4, random_state=0)
    assert batch[0].forest.node_count.min() > 100
    for i, (X, y) in enumerate(zip(Xs, ys)):
        _assert_same_forest(batch[i], _lone(X, y, n_estimators=4, random_state=0), ("limit", i))


def test_predict_batch_equals_the_lone_predict(unequal):
    case, fl, Xs, ys, batch = unequal
    rng = np.random.default_rng(7)
    n_rows = [37, 0, 300]  # unequal blocks, an empty one, one of more than a workgroup's cells (300 x 3 > 256)
    blocks = [sets.threshold_rows(rng, [m.export(t) for t in range(10)], 40, n) for m, n in zip(batch, n_rows)]
    for X, b in zip(Xs, blocks):
        k = min(len(b[::7]), len(X))
        b[:7 * k:7] = X[:k]  # and training rows among the planted ones
    got = _native.predict_forests([m.forest for m in batch], blocks)
    for i, (m, b) in enumerate(zip(batch, blocks)):
        assert got[i].shape == (n_rows[i], 3)
        assert got[i].tobytes() == m.forest.predict(b).tobytes(), i
    assert len(np.unique(got[2])) > 10
    # all blocks empty: nothing to do; forests in another order score their own blocks
    assert [g.shape for g in _native.predict_forests([m.forest for m in batch], [np.zeros((0, 40))] * 3)] == [(0, 3)] * 3
    back = _native.predict_forests([m.forest for m in batch[::-1]], blocks[::-1])[::-1]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(back, got))
    with pytest.raises(ValueError):
        _native.predict_forests([m.forest for m in batch], [np.zeros((1, 39))] * 3)


def _tree_digest(tree) -> str:
    h = hashlib.sha256()
    for name in ARRAYS:
        h.update(np.ascontiguousarray(tree[name]).tobytes())
    return h.hexdigest()


def _embedded_inputs():
    comp, _, ids, labels = types.read_training_data(TYPES)
    return comp, ids, labels


@pytest.fixture(scope="module")
def embedded_cv():
    comp, _, labels = _embedded_inputs()
    return types.cross_validate(comp, labels, splits=3, seed=42)


@pytest.mark.parametrize("name", ["embedded"] + sets.NAMES)
def test_cross_validate_reproduces_sklearns_recorded_folds(ref, embedded_cv, name):
    rec = ref["by_name"][name]
    if name == "embedded":
        res = embedded_cv
    else:
        case = sets.build(name)
        assert sets.digest(case) == rec["input_sha256"]
        res = _cross_validate(case)
    assert res.classes == rec["classes"] and len(res.folds) == len(rec["folds"])
    bad = []
    for i, (f, model) in enumerate(zip(rec["folds"], res.models)):
        assert res.folds[i][0].tolist() == f["train"] and res.folds[i][1].tolist() == f["test"]
        assert model.forest.n_trees == len(f["trees"]) == rec["n_estimators"]
        for t, (node_count, max_depth, digest) in enumerate(f["trees"]):
            if (int(model.forest.node_count[t]), int(model.forest.max_depth[t])) != (node_count, max_depth):
                bad.append((i, t, "node_count/max_depth"))
            elif _tree_digest(model.export(t)) != digest:
                bad.append((i, t, "digest"))
        exp = np.asarray(f["posit"], dtype=np.uint64).view(np.float64).reshape(len(f["test"]), len(rec["classes"]))
        assert res.posit[f["test"]].tobytes() == exp.tobytes(), (name, i, int((res.posit[f["test"]] != exp).sum()))
    assert not bad, f"{len(bad)} trees differ, first: {bad[:5]}"


def test_cross_validate_equals_live_sklearn(ref):
    sklearn = pytest.importorskip("sklearn")
    sparse = pytest.importorskip("scipy.sparse")
    if sklearn.__version__ != ref["sklearn"]:
        pytest.skip(f"the installed sklearn is {sklearn.__version__}, the forest is pinned to {ref['sklearn']}")
    from sklearn.base import clone
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import KFold

    for name in sets.NAMES:  # another random_state than the fixture's: these trees are recorded nowhere
        case = dict(sets.build(name), random_state=7)
        res = _cross_validate(case)
        X = sparse.csr_matrix(case["X"])
        base = RandomForestClassifier(n_estimators=case["n_estimators"], random_state=7)
        for i, (train, test) in enumerate(KFold(case["splits"], shuffle=True, random_state=case["seed"]).split(case["X"])):
            rf = clone(base).fit(X[train], case["y"][train])
            for t, est in enumerate(rf.estimators_):
                exp = {n: np.ascontiguousarray(getattr(est.tree_, n), dtype=DTYPES[n]) for n in ARRAYS}
                assert _tree_digest(res.models[i].export(t)) == _tree_digest(exp), (name, i, t)
            exp = np.stack([1 - p[:, 0] for p in rf.predict_proba(X[test])], axis=1)
            assert res.posit[test].tobytes() == exp.tobytes(), (name, i)


def test_command_line_end_to_end(tmp_path, embedded_cv):
    out = tmp_path / "types_cv.tsv"
    proc = subprocess.run([sys.executable, "-m", "gecco_amd.types_cv", "--model", TYPES, "--splits", "3", "-o", str(out)], cwd=ROOT,
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr
    _, ids, labels = _embedded_inputs()
    lines = out.read_text().splitlines()
    header = lines[0].split("\t")
    assert header == ["cluster_id", "fold", "type", "predicted_type"] + types.probability_columns(embedded_cv.classes)
    cells = [line.split("\t") for line in lines[1:]]
    assert [c[0] for c in cells] == ids and len(cells) == 1870
    assert [int(c[1]) for c in cells] == embedded_cv.fold.tolist()
    assert [c[2] for c in cells] == [types.type_string(n) for n in labels]
    assert [c[3] for c in cells] == [types.type_string(n) for n in embedded_cv.predicted]
    order = [embedded_cv.classes.index(n) for n in sorted(embedded_cv.classes, key=str.casefold)]
    back = np.array([[float(v) for v in c[4:]] for c in cells])
    assert back.tobytes() == np.ascontiguousarray(embedded_cv.posit[:, order]).tobytes()  # repr digits: the bits round-trip
    err = proc.stderr
    assert all(f"fold {i}: n=" in err for i in range(3)) and "pooled: n=1870" in err
    assert all(f"  {c}: auroc=" in err for c in embedded_cv.classes) and "micro_aupr=" in err and "subset_accuracy=" in err
