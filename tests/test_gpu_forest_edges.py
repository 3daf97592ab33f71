"""The device forest (gecco_amd/csrc/crf_forest.hip) on the edge sets of tests/forest_edge_sets.py, against what sklearn
1.7.2 recorded for them (tests/golden/types/forest_edges.json.gz <- tools/gen_forest_edge_fixtures.py): near-equal feature
values (the build's effective FEATURE_THRESHOLD is 0: a position is valid when Xf[p] > Xf[p-1]), the negative / zero /
positive layout, ties in the argmax and between features, and the size limits (2n - 1 nodes, n + 1 stack records, 4096
samples, 8192 features, 64 outputs, a total weight of 2^24 - 1).  Every comparison is equality of bits.  Fixture only;
where sklearn is installed a second test fits fresh seeds of the near-equal families live."""
import gzip
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before libgecco_crf.so: the wheel's own HIP runtime has to be the first one loaded)

from gecco_amd import _native, types  # noqa: E402
from tests import forest_edge_sets as sets  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "types", "forest_edges.json.gz")


@pytest.fixture(scope="module")
def ref():
    with gzip.open(FIXTURE) as fh:
        doc = json.load(fh)
    doc["by_name"] = {r["name"]: r for r in doc["sets"]}
    return doc


def fit_device(s):
    """The set's forest on the device, entered the way the set says: `_native.Forest` with planted counts and the
    splitter states of the seeds, or `types.DeviceForest` with its bootstrap."""
    if s["mode"] == "forest":
        model = types.DeviceForest(n_estimators=s["n_estimators"], random_state=s["random_state"], max_features=s["max_features"])
        return model.fit(sets.coo(s), s["y"]).forest
    codes = np.zeros(s["y"].shape, dtype=np.uint8)
    n_classes = np.zeros(s["y"].shape[1], dtype=np.uint8)
    for k in range(s["y"].shape[1]):
        cls, inv = np.unique(s["y"][:, k], return_inverse=True)
        codes[:, k], n_classes[k] = inv, len(cls)
    counts = np.tile(s["counts"], (len(s["seeds"]), 1))
    states = np.array([types.splitter_state(seed) for seed in s["seeds"]], dtype=np.uint32)
    return _native.Forest(s["indptr"], s["indices"], s["data"], s["n"], codes, n_classes, counts, states, s["max_features"])


def first_mismatch(forest, expected, arrays):
    """None, or a description of the first tree that differs from the recorded one: the counts, else the first array."""
    for t, rec in enumerate(expected):
        got = (int(forest.node_count[t]), int(forest.max_depth[t]))
        if got != (rec["node_count"], rec["max_depth"]):
            return f"tree {t}: (node_count, max_depth) = {got}, sklearn has {(rec['node_count'], rec['max_depth'])}"
        ex = forest.export(t)
        for name in arrays:
            if hashlib.sha256(np.ascontiguousarray(ex[name]).tobytes()).hexdigest() != rec[name]:
                return f"tree {t} ({got[0]} nodes): `{name}` differs; device root = feature {ex['feature'][0]}, threshold {ex['threshold'][0]!r}"
    return None


def test_fixture_lists_every_set(ref):
    assert [r["name"] for r in ref["sets"]] == sets.NAMES


@pytest.mark.parametrize("name", sets.NAMES)
def test_edge_set(ref, name):
    rec = ref["by_name"][name]
    s = sets.build(name)
    assert sets.digest(s) == rec["input_sha256"], "the set builder drifted from the fixture"
    forest = fit_device(s)
    assert forest.n_trees == len(rec["trees"])
    bad = first_mismatch(forest, rec["trees"], ref["tree_arrays"])
    assert bad is None, f"{name} [{sets.PATHS[name]}]: {bad}"
    rows = sets.planted_rows(s, sets.split_nodes([forest.export(t) for t in range(forest.n_trees)]))
    assert list(rows.shape) == rec["rows_shape"] and hashlib.sha256(rows.tobytes()).hexdigest() == rec["rows_sha256"]
    got = forest.predict(rows)
    exp = np.asarray(rec["posit"], dtype=np.uint64).view(np.float64).reshape(got.shape)
    diff = np.argwhere(got.view(np.uint64) != exp.view(np.uint64))
    assert len(diff) == 0, (f"{name}: {len(diff)} posit cells differ, first at row {diff[0][0]} output {diff[0][1]}: "
                            f"{got[tuple(diff[0])]!r} != {exp[tuple(diff[0])]!r}, row = {rows[diff[0][0]][np.nonzero(rows[diff[0][0]])]!r}")


def _live_cases():
    cases = []
    for i, (base, k) in enumerate(((0.2, 1), (0.1, 3), (0.75, 1), (1.5, 2), (3e-8, 1), (-0.4, 5), (-0.4, 9), (100.0, 1))):
        cases.append((f"ulp{k}_at_{base:g}", sets.ulp_pair, (base, k, 7000 + i)))
    for i, (v, far) in enumerate(((sets.DENORM, True), (-sets.DENORM, False), (3e-9, False), (-3e-9, True), (5e-8, True), (-5e-8, False))):
        cases.append((f"zero_vs_{v:g}" + ("_far" if far else ""), sets.zero_block, (v, far, 7100 + i)))
    for i, (base, zb) in enumerate(((0.3, False), (-0.3, False), (2e-8, True), (0.0, True))):
        cases.append((f"chain_at_{base:g}", sets.chain, (base, zb, 7200 + i)))
    return cases


def test_near_equal_families_live(ref):
    """Fresh seeds of the three near-equal families, fitted by the installed sklearn now and compared array for array."""
    sklearn = pytest.importorskip("sklearn", reason="sklearn is not installed: the live near-equal comparison did not run")
    pytest.importorskip("scipy", reason="scipy is not installed: the live near-equal comparison did not run")
    if sklearn.__version__ != ref["sklearn"]:
        pytest.skip(f"the installed sklearn is {sklearn.__version__}, the fixture records {ref['sklearn']}: the forest targets the "
                    "recorded build's behaviour, so the live comparison did not run")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_forest_edge_fixtures as gen
    finally:
        sys.path.pop(0)
    for label, fn, args in _live_cases():
        s = fn(*args)
        s["name"] = label
        trees = gen.fit_sklearn(s)
        forest = fit_device(s)
        for t, est in enumerate(trees):
            exp = gen.tree_arrays(est)
            assert int(forest.node_count[t]) == len(exp["feature"]), f"{label}: tree {t}: node_count"
            got = forest.export(t)
            for name in ref["tree_arrays"]:
                assert np.ascontiguousarray(got[name]).tobytes() == exp[name].tobytes(), f"{label}: tree {t}: `{name}` differs"
        rows = sets.planted_rows(s, sets.split_nodes([gen.tree_arrays(e) for e in trees]))
        assert forest.predict(rows).tobytes() == gen.posit(trees, rows, s["y"].shape[1]).tobytes(), f"{label}: posit"


def test_size_limits_are_refused_on_the_host():
    """Only the host check runs: nothing here reaches the device."""
    def fit(n, F, counts):
        return _native.Forest(np.zeros(F + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), n,
                              np.zeros((n, 1), np.uint8), np.array([1], np.uint8), counts, np.array([5], np.uint32), 1)

    n, F = sets.MAX_SAMPLES, sets.MAX_FEATURES
    with pytest.raises(ValueError):
        fit(n + 1, 4, np.ones((1, n + 1), np.int32))
    with pytest.raises(ValueError):
        fit(8, F + 1, np.ones((1, 8), np.int32))
    with pytest.raises(ValueError):  # a total weight of 2^24
        fit(n, 4, np.full((1, n), n, np.int32))
    with pytest.raises(ValueError):  # a count above n_samples
        fit(8, 4, np.array([[9, 1, 1, 1, 1, 1, 1, 1]], np.int32))
    fit(8, 4, np.ones((1, 8), np.int32))  # in range: fits (every feature constant: one leaf)
