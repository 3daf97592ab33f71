"""Host side of the forest edge sets (tests/forest_edge_sets.py), no device needed: the builder reproduces the digests
recorded in tests/golden/types/forest_edges.json.gz; where sklearn is installed, the generator rewrites the fixture byte
for byte and every limit set reaches the edge it is for under sklearn (a set that does not is a broken set)."""
import gzip
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import forest_edge_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = os.path.join(ROOT, "tests", "golden", "types")
FIXTURE = os.path.join(TYPES, "forest_edges.json.gz")


@pytest.fixture(scope="module")
def ref():
    with gzip.open(FIXTURE) as fh:
        doc = json.load(fh)
    doc["by_name"] = {r["name"]: r for r in doc["sets"]}
    return doc


def test_builder_digests_match_the_fixture(ref):
    assert [r["name"] for r in ref["sets"]] == sets.NAMES
    for name in sets.NAMES:
        assert sets.digest(sets.build(name)) == ref["by_name"][name]["input_sha256"], name


def test_fixture_is_smaller_than_the_forest_fixture():
    assert os.path.getsize(FIXTURE) < os.path.getsize(os.path.join(TYPES, "ref_forest.json.gz"))


def test_sets_are_within_the_kernels_range():
    for name in sets.NAMES:
        s = sets.build(name)
        assert 1 <= s["n"] <= sets.MAX_SAMPLES and 1 <= s["F"] <= sets.MAX_FEATURES and 1 <= s["y"].shape[1] <= sets.MAX_OUTPUTS
        assert s["indptr"][0] == 0 and s["indptr"][-1] == len(s["indices"]) == len(s["data"]) and np.isfinite(s["data"]).all()
        for f in range(s["F"]):
            r = s["indices"][s["indptr"][f]:s["indptr"][f + 1]]
            assert (np.diff(r) > 0).all() and (len(r) == 0 or (0 <= r[0] and r[-1] < s["n"]))
        if s["mode"] == "tree":
            assert (0 <= s["counts"]).all() and (s["counts"] <= s["n"]).all() and 1 <= int(s["counts"].sum()) < 2 ** 24
    s = sets.build("total_weight_2p24_minus_1")
    assert int(s["counts"].astype(np.int64).sum()) == 2 ** 24 - 1
    s = sets.build("wide_4096x8192_64out")
    assert (s["n"], s["F"], s["y"].shape[1]) == (4096, 8192, 64) and not s["y"][:, 0].any() and not s["y"][:, 63].any()
    assert sets.build("outputs_64_two_class")["y"][:, 63].any()
    s = sets.build("stored_zeros")
    col0 = s["data"][:s["indptr"][1]]
    assert (col0 == 0).any() and np.signbit(col0[col0 == 0]).any()  # explicit +0.0 and -0.0 entries


def test_near_equal_sets_sit_between_the_three_rules():
    """The planted pairs are where `>`, `> + 1e-7f` in float32 and `> + 1e-7` in double give different answers."""
    f32 = np.float32

    def rules(a, b):
        return (bool(b > a), bool(b > f32(a + f32(1e-7))), bool(float(b) > float(a) + 1e-7))

    expect = {(0.2, 1): (True, False, False), (0.75, 1): (True, False, False), (1e-8, 1): (True, False, False),
              (0.2, 6): (True, False, False), (-0.2, 6): (True, False, False),  # 8.9e-8: below 1e-7 either way
              (1.0, 1): (True, False, True), (0.75, 2): (True, False, True),    # 1.19e-7: the float32 sum rounds up to b
              (0.2, 7): (True, False, True), (-0.2, 7): (True, False, True),    # 1.04e-7: likewise
              (3.0, 1): (True, True, True)}                                     # 2.4e-7: far enough for all three
    for (base, k), want in expect.items():
        assert f"ulp{k}_at_{base:g}" in sets.NAMES
        assert rules(f32(base), sets.ulps(base, k)) == want, (base, k)
    for v in (sets.DENORM, 1e-8, 9e-8):
        assert rules(f32(0), f32(v)) == (True, False, False) and rules(f32(-v), f32(0)) == (True, False, False)


@pytest.mark.parametrize("name", list(sets.MIRRORED))
def test_mirrored_proxies_tie_where_the_set_says(name):
    """Exact arithmetic (Fractions): positions j and N - j hold the maximal proxy, alone; the float64 proxies computed
    with sklearn's operations are equal bit for bit; and the pair lands where block_argmax is to be exercised."""
    N, want, _, _ = sets.MIRRORED[name]
    s = sets.build(name)
    y = s["y"][:, 0]
    assert (y == y[::-1]).all() and s["data"].tolist() == list(range(1, N + 1))
    pair = sets.tied_best(y)
    assert pair is not None and pair[0] < pair[1] == N - pair[0]
    assert sets.landing(N, pair) == want
    C = -(-N // sets.THREADS)
    ta, tb = pair[0] // C, pair[1] // C
    assert {"one_chunk": ta == tb, "two_lanes": ta != tb and ta // 64 == tb // 64, "two_waves": ta // 64 != tb // 64}[want]

    def proxy64(j):  # Gini.children_impurity + proxy_impurity_improvement, one output
        l1 = float(y[:j].sum())
        r1 = float(y[j:].sum())
        wl, wr = float(j), float(N - j)
        sql = (wl - l1) * (wl - l1) + l1 * l1
        sqr = (wr - r1) * (wr - r1) + r1 * r1
        return -wr * ((1.0 - sqr / (wr * wr)) / 1) - wl * ((1.0 - sql / (wl * wl)) / 1)

    p = np.array([proxy64(j) for j in range(1, N)])
    assert p[pair[0] - 1] == p[pair[1] - 1] == p.max() and int(np.argmax(p)) == pair[0] - 1 and (p == p.max()).sum() == 2


def _gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_forest_edge_fixtures as gen
    finally:
        sys.path.pop(0)
    return gen


def _needs_recorded_sklearn(ref):
    sklearn = pytest.importorskip("sklearn")
    pytest.importorskip("scipy")
    if sklearn.__version__ != ref["sklearn"]:
        pytest.skip(f"the installed sklearn is {sklearn.__version__}, the fixture records {ref['sklearn']}")


def test_generator_reproduces_the_fixture(tmp_path, ref):
    _needs_recorded_sklearn(ref)
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_forest_edge_fixtures.py"), "--out", str(tmp_path)],
                          stdout=subprocess.DEVNULL)
    new = (tmp_path / "forest_edges.json.gz").read_bytes()
    assert hashlib.sha256(new).hexdigest() == hashlib.sha256(open(FIXTURE, "rb").read()).hexdigest()


def test_sets_reach_their_edges_under_sklearn(ref):
    _needs_recorded_sklearn(ref)
    gen = _gen()

    def trees(name):
        return [e.tree_ for e in gen.fit_sklearn(sets.build(name))]

    n = sets.MAX_SAMPLES
    (t,) = trees("node_cap_4096")
    assert t.node_count == 2 * n - 1                       # every node slot of the tree
    (t,) = trees("stack_cap_4096")
    assert t.node_count == 2 * n - 1 and t.max_depth == n - 1  # n + 1 stack records
    for name, (N, _, _, _) in sets.MIRRORED.items():       # sklearn keeps the first of the tied pair
        (t,) = trees(name)
        pair = sets.tied_best(sets.build(name)["y"][:, 0])
        assert t.feature[0] == 0 and t.threshold[0] == pair[0] + 0.5, name
    for m in (255, 256, 257, 1023, 1025):                  # the root's column holds exactly m nonzeros
        s = sets.build(f"bitonic_{m}")
        assert int((s["data"][:s["indptr"][1]] != 0).sum()) == m and s["n"] > m
    for t in trees("constant_root") + trees("one_sample"):
        assert t.node_count == 1
    assert trees("constant_root")[0].impurity[0] > 0       # an impure leaf: no feature could split it
    for t in trees("symmetric_pm_a"):                      # the midpoint of -a and +a
        assert t.threshold[0] == 0.0 and not np.signbit(t.threshold[0])
    assert any(-1e-30 < th < 0 for t in trees("threshold_below_zero") for th in t.threshold[t.feature == 0])
    assert any(th == -sets.DENORM / 2 for t in trees("denormal_below_zero") for th in t.threshold[t.feature == 0])
    # the near-equal families: the recorded build splits every planted pair (FEATURE_THRESHOLD acts as 0)
    for name in sets.NEAR_EQUAL:
        if name.startswith("ulp") or name.startswith("zero_vs_"):
            for t in trees(name):
                th = t.threshold[t.feature == 0]
                assert len(th) > 0, name
    assert any(th == sets.DENORM / 2 for t in trees("zero_vs_1.4013e-45") for th in t.threshold)
    for name in ("chain_300_at_0.2", "chain_300_at_1e-8", "chain_300_denormals"):
        assert all(t.node_count > 100 for t in trees(name)), name
    for t in trees("const_equal_nonzeros"):
        assert not (t.feature == 0).any()                  # the equal column never splits
    assert any((t.feature == 0).any() for t in trees("const_one_ulp_off"))
