"""The K best label paths without a device: the yardstick's three forms against each other (tests/kbest_reference.py: the list
recursion equals path enumeration), how many ranks the device tests' seeds leave unseparated, the host refusals of
``gecco_crf_viterbi_kbest``, the header and the signatures of ABI 2.18.0, and the argument checks of
``SequenceCRF.predict_kbest`` and of the typed front end's ``alternatives``, which come before any device call."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests import kbest_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the yardstick
def _lattice(rng, L, T, masked, integer=False):
    if integer:
        score, trans = rng.integers(-2, 3, size=(T, L)).astype(float), rng.integers(-2, 3, size=(L, L)).astype(float)
    else:
        score, trans = rng.normal(0.0, 1.0, size=(T, L)), rng.normal(0.0, 1.5, size=(L, L))
    if masked:
        out = rng.random((T, L)) < 0.4
        out[np.arange(T), rng.integers(0, L, size=T)] = False  # (every item allows a label)
        score[out] = -np.inf
    return score, trans


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("L", [2, 3, 5])
def test_the_list_recursion_equals_enumeration(L, T, masked):
    rng = np.random.default_rng(100 * L + 10 * T + masked)
    for integer in (False, True):  # (integer weights: ties at every turn, the order decides)
        score, trans = _lattice(rng, L, T, masked, integer)
        total = int(np.prod((score != -np.inf).sum(axis=1)))
        for k in (1, 2, 7, 33):
            want = kr.enumerate_kbest(score, trans, k)
            assert len(want) == min(k, total)
            assert kr.list_dp(score, trans, k) == want
            paths, scores = kr.list_dp_numpy(score, trans, k)
            assert [tuple(p) for p in paths.tolist()] == [p for p, _ in want] and scores.tolist() == [s for _, s in want]
            paths, scores = kr.kbest(score, trans, k)
            assert [tuple(p) for p in paths.tolist()] == [p for p, _ in want] and scores.tolist() == [s for _, s in want]
        # the order: score descending, then the reversed path ascending; rank 0 is the Viterbi recursion's path
        every = kr.enumerate_kbest(score, trans, L ** T)
        keys = [(-s, p[::-1]) for p, s in every]
        assert keys == sorted(keys) and all(s > -np.inf for _, s in every)
        from tests.constrained_reference import viterbi_one

        y, best = viterbi_one(score, trans)
        assert tuple(y.tolist()) == every[0][0] and best == every[0][1]


def test_the_numpy_recursion_equals_the_list_recursion_on_longer_sequences():
    rng = np.random.default_rng(7)
    for L, T, masked in ((4, 40, False), (9, 25, True), (17, 12, False)):
        score, trans = _lattice(rng, L, T, masked)
        want = kr.list_dp(score, trans, 6)
        paths, scores = kr.list_dp_numpy(score, trans, 6)
        assert [tuple(p) for p in paths.tolist()] == [p for p, _ in want] and scores.tolist() == [s for _, s in want]
        assert all(kr.path_score(score, trans, p) == s for p, s in want), "a score is the left-to-right sum along its path"


def test_the_seeds_of_the_device_tests_leave_at_most_one_rank_in_a_hundred_unseparated():
    """The cap the device tests assert, counted here with the yardstick alone (random normal weights: none at all)."""
    from tests import test_gpu_kbest as gk

    def count(ref):
        ranks = unseparated = 0
        for r in ref:
            if r is not None:
                sep = r[3][:gk.KMAX]
                ranks += len(sep)
                unseparated += int((~sep).sum())
        return ranks, unseparated

    cases = [(f"enumeration L={L} values={v}", gk.reference(gk.enumeration_batch(L), v, False, enumerate_all=True))
             for L in (2, 3, 5) for v in (False, True)]
    cases += [(f"seams L={L}", gk.reference(gk.seam_batch(L), True, False)) for L in (2, 8, 17)]
    cases += [(f"masks L={L}", gk.reference(gk.seam_batch(L), True, True)) for L in (2, 8, 17)]
    for tag, ref in cases:
        ranks, unseparated = count(ref)
        print(f"{tag}: {unseparated} of {ranks} ranks unseparated")
        assert ranks > 0 and unseparated <= 0.01 * ranks, tag


def test_the_bound_and_the_separation_flags():
    score = np.array([[1.0, -2.0], [0.5, 4.0]])
    trans = np.array([[0.25, -1.0], [2.0, 0.0]])
    assert kr.bound(np.array([0, 1]), np.abs(score), np.abs(trans)) == 4.0 * 2 * kr.EPS * (1.0 + 4.0 + 1.0)
    assert kr.bound(np.array([1]), np.abs(score[:1]), np.abs(trans)) == 4.0 * kr.EPS * 2.0
    flags = kr.separated(np.array([3.0, 2.0, 2.0 - 1e-15, 1.0]), np.full(4, 1e-15))
    assert flags.tolist() == [True, False, False, True]


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


def _call(nat, model, **change):
    """A valid batch of two contigs (2 and 3 genes), k = 4, on a device that does not exist, with `change` applied."""
    a = {"contig_ptr": np.array([0, 2, 5], dtype=np.int32), "n_contigs": 2, "gene_ptr": np.arange(0, 12, 2, dtype=np.int32),
         "attr_id": (np.arange(10, dtype=np.int32) * 3) % 7, "attr_value": None, "allowed": None, "k": 4,
         "y": np.zeros(5 * 32, dtype=np.int8), "score": np.zeros(2 * 32), "n_paths": np.zeros(2, dtype=np.int32),
         "lognorm": np.zeros(2)}
    a.update(change)
    fn = nat.load_library().gecco_crf_viterbi_kbest
    names = ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "k", "y", "score", "n_paths", "lognorm")
    args = [a[n].ctypes.data_as(t) if isinstance(a[n], np.ndarray) else a[n] for n, t in zip(names, fn.argtypes[2:])]
    rc = fn(model._h, 99, *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


def test_host_refusals_come_before_the_device(nat, model3):
    call = lambda **kw: _call(nat, model3, **kw)
    # a valid call gets past the host checks: what stops it is the device that does not exist
    assert call()[0] not in (nat.OK, nat.EINVAL)
    assert call(lognorm=None)[0] not in (nat.OK, nat.EINVAL)
    assert call(k=1)[0] not in (nat.OK, nat.EINVAL) and call(k=32)[0] not in (nat.OK, nat.EINVAL)
    for bad in (0, -1, 33, 1 << 20):
        assert call(k=bad) == (nat.EINVAL, f"viterbi_kbest: k = {bad} is outside 1 .. 32")
    assert call(y=None) == (nat.EINVAL, "null buffer")
    assert call(score=None) == (nat.EINVAL, "null buffer") and call(n_paths=None) == (nat.EINVAL, "null buffer")
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
    rc, msg = _call(nat, model3, contig_ptr=np.zeros(4, dtype=np.int32), n_contigs=3, score=np.zeros(3 * 4),
                    n_paths=np.full(3, 9, dtype=np.int32), lognorm=np.full(3, 7.0), y=None)
    assert rc != nat.EINVAL, msg  # (ENODEV from the device that does not exist, or OK: never a complaint about an argument)


def test_the_native_wrapper_checks_its_arrays(nat, model3):
    cptr, gptr, attr = np.array([0, 2, 5], dtype=np.int32), np.arange(0, 12, 2, dtype=np.int32), (np.arange(10, dtype=np.int32) * 3) % 7
    with pytest.raises(ValueError, match="values holds 3 entries"):
        model3.viterbi_kbest(cptr, gptr, attr, 4, values=np.ones(3))
    with pytest.raises(ValueError, match="allowed holds 2 masks for 5 genes"):
        model3.viterbi_kbest(cptr, gptr, attr, 4, allowed=[1, 1])
    for bad in (0, 33):
        with pytest.raises(ValueError, match=rf"viterbi_kbest: k = {bad} is outside 1 \.\. 32"):
            model3.viterbi_kbest(cptr, gptr, attr, bad)
    with pytest.raises(TypeError):
        model3.viterbi_kbest(cptr, gptr, attr, 2.5)


def test_the_header_declares_the_entry_and_the_library_exports_it(nat):
    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    assert "ABI 2.18.0" in header
    for words in ("prefix property", "Empty ranks", "The order is total", "L-way merge"):
        assert words in header, words
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+gecco_crf_viterbi_kbest\s*\(([^;]*)\)\s*;", code)
    assert m, "gecco_crf_viterbi_kbest is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "m", "device", "contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "k", "y", "score", "n_paths", "lognorm"]
    lib = nat.load_library()
    assert hasattr(lib, "gecco_crf_viterbi_kbest")
    assert len(nat.SIGNATURES["gecco_crf_viterbi_kbest"][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    sig = inspect.signature(nat.Model.viterbi_kbest)
    assert list(sig.parameters) == ["self", "contig_ptr", "gene_ptr", "attr_id", "k", "device", "values", "allowed"]
    assert sig.parameters["device"].default == 0 and sig.parameters["values"].default is None and sig.parameters["allowed"].default is None


def test_the_kernel_file_is_built_without_contraction():
    from gecco_amd import build

    assert "crf_kbest.hip" in build.SOURCES and build.SOURCES.index("crf_kbest.hip") == build.SOURCES.index("crf_sample.hip") + 1
    assert build.EXTRA_FLAGS["crf_kbest.hip"] == ["-ffp-contract=off"]


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

    for name in ("viterbi_kbest", "sample_paths", "marginals_full", "viterbi"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [], [["a0", "a3"]]]


def test_bad_counts_and_sets_are_refused_before_any_device_call(crf):
    for bad in (0, -3, 33):
        with pytest.raises(ValueError, match=rf"k = {bad} is outside 1 \.\. 32"):
            crf.predict_kbest(X, bad)
    for bad in (2.5, "3", None):
        with pytest.raises(ValueError, match="k is an integer"):
            crf.predict_kbest(X, bad)
    with pytest.raises(ValueError, match="unknown label"):
        crf.predict_kbest(X, 4, allowed=[["x", "q", None], [], [None]])
    with pytest.raises(ValueError, match="items but"):
        crf.predict_kbest(X, 4, allowed=[["x", None], [], [None]])
    assert "predict_kbest" in type(crf).__dict__ and "log_probabilities" in type(crf).predict_kbest.__doc__


def test_no_item_needs_no_device(crf):
    out = crf.predict_kbest([[], []], 5)
    assert len(out) == 2 and all(o["paths"] == [] and o["scores"].shape == (0,) and o["log_probabilities"].shape == (0,) for o in out)
    assert crf.predict_kbest([], 3) == []


def test_an_unfitted_model_is_refused():
    from gecco_amd.sequence import SequenceCRF

    with pytest.raises(ValueError, match="not fitted"):
        SequenceCRF(window_size=None).predict_kbest(X, 4)


# ---------------------------------------------------------------- the typed front end
def test_the_typed_front_end_takes_the_arguments():
    from gecco_amd import typed

    for name in ("predict_clusters", "predict_genes_and_clusters"):
        params = inspect.signature(getattr(typed.TypedClusterCRF, name)).parameters
        assert params["alternatives"].default == 0 and params["alternatives_margin"].default == 10
    base = ["predict", "--model", "m", "-f", "f", "-g", "g"]
    args = typed.build_parser().parse_args(base)
    assert args.alternatives == 0 and args.alternatives_margin == 10
    args = typed.build_parser().parse_args(base + ["--alternatives", "4", "--alternatives-margin", "3"])
    assert args.alternatives == 4 and args.alternatives_margin == 3


def test_the_typed_front_end_checks_the_arguments_first():
    """Before the model is looked at: an unfitted one never gets to say so."""
    from gecco_amd import typed

    crf = typed.TypedClusterCRF()
    for kw, words in ((dict(alternatives=-1), "alternatives = -1 is outside 0 .. 32"), (dict(alternatives=33), "alternatives = 33 is outside"),
                      (dict(alternatives=1.5), "integers"), (dict(alternatives=4, alternatives_margin=-1), "alternatives_margin = -1 is negative"),
                      (dict(alternatives=4, alternatives_margin=0.5), "integers")):
        for method in (crf.predict_clusters, crf.predict_genes_and_clusters):
            with pytest.raises(ValueError, match=words):
                method([], **kw)
    with pytest.raises(ValueError, match="not fitted"):
        crf.predict_clusters([], alternatives=4)


def test_alternatives_table(tmp_path):
    from types import SimpleNamespace

    from gecco_amd import typed

    clusters = [SimpleNamespace(id="c_1", alternatives=[
        {"rank": 0, "run": (2, 5), "start": 100, "end": 900, "type": "Beta", "log_p": -0.25},
        {"rank": 1, "run": None, "start": None, "end": None, "type": None, "log_p": -3.0}]), SimpleNamespace(id="c_2")]
    path = os.path.join(str(tmp_path), "alternatives.tsv")
    typed.write_alternatives(path, clusters)
    rows = [line.rstrip("\n").split("\t") for line in open(path)]
    assert rows == [["cluster_id", "rank", "start", "end", "type", "log_p", "p"],
                    ["c_1", "0", "100", "900", "Beta", "-0.25", repr(math.exp(-0.25))],
                    ["c_1", "1", "", "", "", "-3.0", repr(math.exp(-3.0))]]
