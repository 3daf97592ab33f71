"""Run-count posteriors without a device: the yardstick's recursion against path enumeration (tests/counts_reference.py) in both
semirings, its identities where the tail slot is empty, the host refusals of ``gecco_crf_run_counts``, the header and the
signatures of ABI 2.23.0, and the argument checks of ``SequenceCRF.run_count_log_probability`` / ``predict_run_counts`` and
``TypedClusterCRF.predict_cluster_counts`` / ``predict_count_clusters``, which come before any device call."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import counts_reference as cn
from tests import edges_reference as er
from tests import runs_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the yardstick
def _lattice(rng, L, n, masked, integer):
    if integer:
        score, trans = rng.integers(-2, 3, size=(n, L)).astype(float), rng.integers(-2, 3, size=(L, L)).astype(float)
    else:
        score, trans = rng.normal(0.0, 1.0, size=(n, L)), rng.normal(0.0, 1.5, size=(L, L))
    if masked:
        out = rng.random((n, L)) < 0.3
        out[np.arange(n), rng.integers(0, L, size=n)] = False  # (every item allows a label)
        score[out] = -np.inf
    return score, trans


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("L,longest", [(2, 8), (3, 6)])
def test_the_recursion_equals_enumeration(L, longest, integer, masked):
    rng = np.random.default_rng(2000 * L + 10 * integer + masked)
    cases = empty = 0
    worst = 0.0
    for n in range(1, longest + 1):
        score, trans = _lattice(rng, L, n, masked, integer)
        for K in (1, 2, 3, 4):
            for mask in range(1, 1 << L):  # every mask
                best, arg, logz, count = cn.enumerate_paths(score, trans, mask, K)
                paths, got = cn.recursion(score, trans, mask, K)
                z, largest = cn.recursion(score, trans, mask, K, "sum")
                assert len(paths) == K + 1 and got.shape == z.shape == (K + 1,) and not np.isnan(z.astype(float)).any()
                for k in range(K + 1):
                    cases += 1
                    where = (L, n, K, mask, k)
                    if count[k] == 0:
                        empty += 1
                        assert paths[k] is None and got[k] == -np.inf and z[k] == -np.inf, where
                        continue
                    runs = cn.n_runs(paths[k], mask)
                    assert (runs >= K if k == K else runs == k) and cn.path_score(score, trans, paths[k]) == got[k], where
                    # (rounding is monotone, so a maximum of rounded sums is the rounded sum of a maximum: equal bits, integer or not)
                    assert got[k] == best[k] and tuple(paths[k].tolist()) in arg[k], where
                    err = abs(float(z[k] - logz[k]))
                    worst = max(worst, err / cn.lognorm_bound(n, L, largest))
                    assert err <= cn.lognorm_bound(n, L, largest), (where, err)
    print(f"L={L} integer={integer} masked={masked}: {cases} slots, {empty} without a path, worst |log Z_k - enumeration| / bound = {worst:.3g}")
    assert empty > 0 and cases > 4 * empty // 3


def test_run_counting():
    assert cn.n_runs([], 2) == 0 and cn.n_runs([0, 0], 2) == 0 and cn.n_runs([1], 2) == 1
    assert cn.n_runs([1, 0, 1], 2) == 2 and cn.n_runs([1, 2, 0, 2, 2, 0], 6) == 2  # (labels inside a run may differ)
    assert cn.n_runs([0, 1, 1, 0], 2) == 1 and cn.n_runs([1, 0, 0, 1], 2) == 2     # (runs at the ends count)


def test_a_sequence_without_items():
    paths, scores = cn.recursion(np.zeros((0, 3)), np.zeros((3, 3)), 6, 2)
    assert paths[0].tolist() == [] and paths[1:] == [None, None] and scores.tolist() == [0.0, -np.inf, -np.inf]
    z, largest = cn.recursion(np.zeros((0, 3)), np.zeros((3, 3)), 6, 2, "sum")
    assert z.tolist() == [0.0, -np.inf, -np.inf] and largest == 0.0


@pytest.mark.parametrize("L", [2, 3, 5])
def test_identities_where_the_tail_slot_is_empty(L):
    """K > ceil(n / 2): no path has K runs, the tail slot is exactly -inf, and the slots are the whole distribution."""
    rng = np.random.default_rng(70 + L)
    every = (1 << L) - 1
    for n in (1, 2, 5, 8):
        K = (n + 1) // 2 + 1
        for masked in (False, True):
            score, trans = _lattice(rng, L, n, masked, False)
            xi, marg, _ = er.edges_one(score, trans)
            for mask in (1, every & ~1, int(rng.integers(1, every + 1)), every):
                z, largest = cn.recursion(score, trans, mask, K, "sum")
                assert z[K] == -np.inf
                total = z.max() + np.log(np.exp(z - z.max()).sum())
                tol = (K + 2) * cn.lognorm_bound(n, L, largest) + 1e-12
                assert abs(float(total) - rr.log_z(score, trans)) <= tol
                p = np.exp((z - total).astype(np.float64))
                assert abs(p.sum() - 1.0) <= tol
                # the mean of the distribution is the expected number of runs
                want = er.expected_runs(marg[0], xi.sum(axis=0), mask)
                assert abs(float((np.arange(K + 1) * p).sum()) - want) <= K * tol + 1e-12
                # no run at all: the whole sequence stays in the complement of the set
                outside = score.copy()
                outside[:, cn.inside_labels(mask, L)] = -np.inf
                span = rr.log_z(outside, trans) - rr.log_z(score, trans)
                if mask == every:
                    assert z[0] == -np.inf and abs(p[1] - 1.0) <= tol  # (every label inside: exactly one run)
                else:
                    assert (z[0] == -np.inf and span == -np.inf) or abs(float(z[0] - total) - span) <= tol


# ---------------------------------------------------------------- the entry's host refusals
L3 = 3


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    return _native


@pytest.fixture(scope="module")
def model3(nat):
    rng = np.random.default_rng(5)
    return nat.Model.from_tables(rng.normal(size=(7, L3)), rng.normal(size=(L3, L3)))


NAMES = ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "set_mask", "max_runs", "log_mass", "score", "y",
         "lognorm")


def _call(nat, model, device=99, **change):
    """A valid batch of two contigs (2 and 3 genes), the set {1, 2} and K = 2, on a device that does not exist, with `change`
    applied."""
    a = {"contig_ptr": np.array([0, 2, 5], dtype=np.int32), "n_contigs": 2, "gene_ptr": np.arange(0, 12, 2, dtype=np.int32),
         "attr_id": (np.arange(10, dtype=np.int32) * 3) % 7, "attr_value": None, "allowed": None, "set_mask": 6, "max_runs": 2,
         "log_mass": np.zeros((2, 3)), "score": np.zeros((2, 3)), "y": np.zeros((3, 5), dtype=np.int8), "lognorm": np.zeros(2)}
    a.update(change)
    fn = nat.load_library().gecco_crf_run_counts
    args = [a[n].ctypes.data_as(t) if isinstance(a[n], np.ndarray) else a[n] for n, t in zip(NAMES, fn.argtypes[2:])]
    rc = fn(model._h, device, *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


def test_host_refusals_come_before_the_device(nat, model3):
    call = lambda **kw: _call(nat, model3, **kw)
    # a valid call gets past the host checks: what stops it is the device that does not exist
    assert call()[0] not in (nat.OK, nat.EINVAL)
    assert call(lognorm=None, log_mass=None)[0] not in (nat.OK, nat.EINVAL)
    assert call(score=None, y=None)[0] not in (nat.OK, nat.EINVAL) and call(y=None)[0] not in (nat.OK, nat.EINVAL)
    assert call(max_runs=1, set_mask=7, log_mass=np.zeros((2, 2)), score=np.zeros((2, 2)))[0] not in (nat.OK, nat.EINVAL)
    assert call(max_runs=32, set_mask=1, log_mass=np.zeros((2, 33)), score=None, y=None)[0] not in (nat.OK, nat.EINVAL)
    # an argument error together with a device that does not exist reports the argument
    for bad in (0, -1, 33, 1 << 20):
        assert call(max_runs=bad) == (nat.EINVAL, f"run_counts: max_runs = {bad} is outside 1 .. 32")
    rc, msg = call(set_mask=0)
    assert rc == nat.EINVAL and msg.startswith("run_counts: set_mask") and "empty" in msg
    for bad in (8, 9, 1 << 31):
        rc, msg = call(set_mask=bad)
        assert rc == nat.EINVAL and msg.startswith("run_counts: set_mask") and f"at or above num_labels = 3 (mask {bad})" in msg
    assert call(score=None) == (nat.EINVAL, "run_counts: y is given without score")
    assert call(log_mass=None, score=None, y=None) == (nat.EINVAL, "run_counts: log_mass, score and y are all NULL")
    # the checks of the _valued and _constrained entries
    v = np.ones(10)
    v[3] = np.inf
    assert call(attr_value=v) == (nat.EINVAL, "attribute value 3 is not finite (NaN or infinite)")
    assert call(allowed=np.array([7, 1, 0, 4, 3], dtype=np.uint32)) == (nat.EINVAL, "constrained: gene 2 allows no label (a mask of 0)")
    assert call(allowed=np.array([7, 1, 6, 4, 9], dtype=np.uint32)) == \
        (nat.EINVAL, "constrained: gene 4 allows a label at or above num_labels = 3 (mask 9)")
    assert call(contig_ptr=None)[0] == nat.EINVAL and call(n_contigs=-1)[0] == nat.EINVAL
    assert call(gene_ptr=None) == (nat.EINVAL, "null buffer")


def test_a_batch_without_genes_needs_no_argument_complaint(nat, model3):
    rc, msg = _call(nat, model3, contig_ptr=np.zeros(4, dtype=np.int32), n_contigs=3, log_mass=np.full((3, 3), 7.0),
                    score=np.full((3, 3), 7.0), lognorm=np.full(3, 7.0), y=None)
    assert rc != nat.EINVAL, msg  # (ENODEV from the device that does not exist, or OK: never a complaint about an argument)


def test_the_native_wrapper_checks_its_arrays(nat, model3):
    cptr, gptr, attr = np.array([0, 2, 5], dtype=np.int32), np.arange(0, 12, 2, dtype=np.int32), (np.arange(10, dtype=np.int32) * 3) % 7
    with pytest.raises(ValueError, match="values holds 3 entries"):
        model3.run_counts(cptr, gptr, attr, 6, 2, values=np.ones(3))
    with pytest.raises(ValueError, match="allowed holds 2 masks for 5 genes"):
        model3.run_counts(cptr, gptr, attr, 6, 2, allowed=[1, 1])
    for bad in (0, 33):
        with pytest.raises(ValueError, match=rf"run_counts: max_runs = {bad} is outside 1 \.\. 32"):
            model3.run_counts(cptr, gptr, attr, 6, bad, device=99)
    with pytest.raises(ValueError, match="set_mask"):
        model3.run_counts(cptr, gptr, attr, 0, 2, device=99)
    with pytest.raises(ValueError, match="set_mask"):
        model3.run_counts(cptr, gptr, attr, -1, 2)
    with pytest.raises(ValueError, match="all NULL"):
        model3.run_counts(cptr, gptr, attr, 6, 2, device=99, want_log_mass=False, want_paths=False)
    with pytest.raises(TypeError):
        model3.run_counts(cptr, gptr, attr, 6, 2.5)


def test_the_header_declares_the_entry_and_the_library_exports_it(nat):
    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    assert "ABI 2.23.0" in header and "ABI 2.23.0 gecco_crf_run_counts" in re.sub(r"\s*\n \*\s*", " ", header)
    for words in ("The tie rule is operational", "Infeasible counts", "Max semiring", "Sum semiring", "saturating tail slot",
                  "runs only when log_mass is given", "y given without score"):
        assert words in header, words
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+gecco_crf_run_counts\s*\(([^;]*)\)\s*;", code)
    assert m, "gecco_crf_run_counts is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["m", "device"] + list(NAMES)
    lib = nat.load_library()
    assert hasattr(lib, "gecco_crf_run_counts")
    assert len(nat.SIGNATURES["gecco_crf_run_counts"][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    sig = inspect.signature(nat.Model.run_counts)
    assert list(sig.parameters) == ["self", "contig_ptr", "gene_ptr", "attr_id", "set_mask", "max_runs", "device", "values", "allowed",
                                    "want_log_mass", "want_paths", "want_lognorm"]
    assert sig.parameters["device"].default == 0 and sig.parameters["want_paths"].default is True


def test_the_kernel_file_is_built_without_contraction():
    from gecco_amd import build

    at = build.SOURCES.index("crf_minrun.hip")
    assert build.SOURCES[at + 1] == "crf_counts.hip" and build.EXTRA_FLAGS["crf_counts.hip"] == ["-ffp-contract=off"]
    assert os.path.exists(os.path.join(build.CSRC, "crf_counts.hip"))


# ---------------------------------------------------------------- SequenceCRF
@pytest.fixture()
def crf(monkeypatch):
    from gecco_amd import _native
    from gecco_amd.crfsuite_model import model_bytes
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(5)
    An, L = 4, 3
    names, classes = [f"a{k}" for k in range(An)], ["x", "y", "z"]
    w = rng.normal(0.0, 1.0, size=An * L + L * L)
    blob = model_bytes(classes, names, np.repeat(np.arange(An), L), np.tile(np.arange(L), An), np.repeat(np.arange(L), L),
                       np.tile(np.arange(L), L), w)
    crf = SequenceCRF.from_bytes(blob, window_size=None)

    def no_device(*args, **kwargs):
        raise AssertionError("the native call was reached")

    for name in ("run_counts", "viterbi_min_run", "viterbi_kbest", "marginals_full", "viterbi"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [], [["a0", "a3"]]]


@pytest.mark.parametrize("method", ["run_count_log_probability", "run_count_probability", "predict_run_counts"])
def test_bad_sets_and_counts_are_refused_before_any_device_call(crf, method):
    fn = getattr(crf, method)
    for bad in (0, -3, 33):
        with pytest.raises(ValueError, match=rf"max_runs = {bad} is outside 1 \.\. 32"):
            fn(X, ["y"], bad)
    for bad in (2.5, "3", None):
        with pytest.raises(ValueError, match="max_runs is an integer"):
            fn(X, ["y"], bad)
    with pytest.raises(ValueError, match="unknown label"):
        fn(X, ["y", "q"], 2)
    with pytest.raises(ValueError, match="empty"):
        fn(X, [], 2)
    with pytest.raises(ValueError, match="unknown label"):
        fn(X, ["y"], 2, allowed=[["x", "q", None], [], [None]])
    assert method in type(crf).__dict__ and "max_runs" in getattr(type(crf), method).__doc__


def test_no_item_needs_no_device(crf):
    lp = crf.run_count_log_probability([[], []], ["y", "z"], 3)
    assert lp.dtype == np.float64 and lp.tolist() == [[0.0, -np.inf, -np.inf, -np.inf]] * 2
    assert crf.run_count_probability([[], []], ["y", "z"], 3).tolist() == [[1.0, 0.0, 0.0, 0.0]] * 2
    assert crf.run_count_log_probability([], ["y"], 3).shape == (0, 4)
    out = crf.predict_run_counts([[]], ["y"], 2)
    assert len(out) == 1 and out[0]["paths"] == [[], None, None]
    assert out[0]["scores"].tolist() == [0.0, -np.inf, -np.inf] and out[0]["log_probabilities"].tolist() == [0.0, -np.inf, -np.inf]
    assert crf.predict_run_counts([], ["y"], 2) == []


def test_an_unfitted_model_is_refused():
    from gecco_amd.sequence import SequenceCRF

    for method in ("run_count_log_probability", "run_count_probability", "predict_run_counts"):
        with pytest.raises(ValueError, match="not fitted"):
            getattr(SequenceCRF(window_size=None), method)(X, ["y"], 2)


# ---------------------------------------------------------------- the typed front end
def test_the_typed_front_end_takes_the_arguments():
    from gecco_amd import typed

    params = inspect.signature(typed.TypedClusterCRF.predict_cluster_counts).parameters
    assert params["max_clusters"].default == 8 and params["known"].default is None
    params = inspect.signature(typed.TypedClusterCRF.predict_count_clusters).parameters
    assert params["n_clusters"].default == 1 and params["known"].default is None
    base = ["predict", "--model", "m", "-f", "f", "-g", "g"]
    args = typed.build_parser().parse_args(base)
    assert args.cluster_counts is None and args.exact_clusters is None
    args = typed.build_parser().parse_args(base + ["--cluster-counts", "4", "--exact-clusters", "1"])
    assert args.cluster_counts == 4 and args.exact_clusters == 1
    assert typed.count_columns(3) == ("sequence_id", "genes", "p_0", "p_1", "p_2", "p_ge_3", "map_clusters")
    assert typed.TypedClusterCRF.SEQUENCE_COLUMNS == ("sequence_id", "genes", "log_z", "entropy", "expected_clusters")


def test_the_typed_front_end_checks_the_arguments_first():
    """Before the model is looked at: an unfitted one never gets to say so."""
    from gecco_amd import typed

    crf = typed.TypedClusterCRF()
    for bad, words in ((0, "max_clusters = 0 is outside 1 .. 32"), (33, "max_clusters = 33 is outside"), (1.5, "max_clusters is an integer")):
        with pytest.raises(ValueError, match=words):
            crf.predict_cluster_counts([], max_clusters=bad)
    for bad, words in ((-1, "n_clusters = -1 is outside 0 .. 31"), (32, "n_clusters = 32 is outside"), (1.5, "n_clusters is an integer")):
        with pytest.raises(ValueError, match=words):
            crf.predict_count_clusters([], n_clusters=bad)
    with pytest.raises(ValueError, match="not fitted"):
        crf.predict_cluster_counts([], max_clusters=3)
    with pytest.raises(ValueError, match="not fitted"):
        crf.predict_count_clusters([], n_clusters=1)


def test_cluster_counts_table(tmp_path):
    from gecco_amd import typed

    rows = {"sequence_id": ["s1", "s2"], "genes": [7, 0], "p_0": [0.25, 1.0], "p_1": [0.5, 0.0], "p_ge_2": [0.25, 0.0], "map_clusters": [1, 0]}
    path = os.path.join(str(tmp_path), "cluster_counts.tsv")
    typed.write_cluster_counts(path, rows)
    got = [line.rstrip("\n").split("\t") for line in open(path)]
    assert got == [["sequence_id", "genes", "p_0", "p_1", "p_ge_2", "map_clusters"], ["s1", "7", "0.25", "0.5", "0.25", "1"],
                   ["s2", "0", "1.0", "0.0", "0.0", "0"]]
