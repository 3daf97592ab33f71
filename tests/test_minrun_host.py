"""Decoding under a minimum run length without a device: the yardstick's recursion against path enumeration
(tests/minrun_reference.py), a minimum of 1 against the plain Viterbi recursion, the host refusals of
``gecco_crf_viterbi_min_run``, the header and the signatures of ABI 2.20.0, and the argument checks of
``SequenceCRF.predict_min_run`` and ``TypedClusterCRF.predict_path_clusters``, which come before any device call."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import minrun_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the yardstick
def _lattice(rng, L, T, masked, integer):
    if integer:
        score, trans = rng.integers(-2, 3, size=(T, L)).astype(float), rng.integers(-2, 3, size=(L, L)).astype(float)
    else:
        score, trans = rng.normal(0.0, 1.0, size=(T, L)), rng.normal(0.0, 1.5, size=(L, L))
    if masked:
        out = rng.random((T, L)) < 0.3
        out[np.arange(T), rng.integers(0, L, size=T)] = False  # (every item allows a label)
        score[out] = -np.inf
    return score, trans


def _sets(rng, L):
    """The set of every label, and a random one that is not empty."""
    every = (1 << L) - 1
    return [every, int(rng.integers(1, every + 1))]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("L,longest", [(2, 10), (3, 7), (4, 5)])
def test_the_recursion_equals_enumeration(L, longest, integer, masked):
    rng = np.random.default_rng(1000 * L + 10 * integer + masked)
    cases = infeasible = differs = 0
    worst = 0.0
    for T in range(1, longest + 1):
        score, trans = _lattice(rng, L, T, masked, integer)
        free, _ = cr.viterbi_one(score, trans)
        for m in (1, 2, 3, 4):
            for mask in _sets(rng, L):
                best, arg, logz, count = mr.enumerate_paths(score, trans, mask, m)
                path, got = mr.recursion(score, trans, mask, m)
                cases += 1
                if count == 0:
                    infeasible += 1
                    assert path is None and got == -np.inf
                    assert mr.recursion(score, trans, mask, m, "sum")[0] == -np.inf
                    continue
                assert mr.feasible(path, mask, m) and mr.path_score(score, trans, path) == got
                # (rounding is monotone, so a maximum of rounded sums is the rounded sum of a maximum: equal bits, integer or not)
                assert got == best and tuple(path.tolist()) in arg, (L, T, m, mask)
                differs += m > 1 and path.tolist() != free.tolist()
                z, largest = mr.recursion(score, trans, mask, m, "sum")
                err = abs(float(z - logz))
                worst = max(worst, err)
                assert err <= 8e-15 * max(1.0, largest), (L, T, m, mask, err)
    print(f"L={L} integer={integer} masked={masked}: {cases} cases, {infeasible} without a feasible path, {differs} where the "
          f"constrained path is not the free one, worst |log Z_C - enumeration| = {worst:.3g}")
    assert differs > 0 and infeasible > 0


def test_short_sequences_under_the_full_set_have_no_path():
    score, trans = np.zeros((2, 3)), np.zeros((3, 3))
    assert mr.recursion(score, trans, 7, 3) == (None, -np.inf)
    assert mr.recursion(score, trans, 7, 3, "sum")[0] == -np.inf
    path, best = mr.recursion(score, trans, 6, 3)  # (label 0 is outside: the all-background path)
    assert path.tolist() == [0, 0] and best == 0.0
    assert not mr.feasible([1, 1, 0, 2], 6, 2) and mr.feasible([1, 2, 0, 0], 6, 2) and mr.feasible([0, 0], 6, 2)
    assert not mr.feasible([1, 0, 0], 6, 2) and not mr.feasible([0, 0, 1], 6, 2)  # (runs at the ends count)


@pytest.mark.parametrize("L", [2, 3, 5, 9])
def test_a_minimum_of_one_is_the_plain_viterbi_recursion(L):
    rng = np.random.default_rng(40 + L)
    for T in (1, 2, 7, 30):
        for integer in (False, True):
            for masked in (False, True):
                score, trans = _lattice(rng, L, T, masked, integer)
                y, best = cr.viterbi_one(score, trans)
                for mask in _sets(rng, L):
                    path, got = mr.recursion(score, trans, mask, 1)
                    assert path.tolist() == y.tolist() and np.float64(got).tobytes() == np.float64(best).tobytes()


def test_the_sum_semiring_of_a_minimum_of_one_is_log_z():
    rng = np.random.default_rng(3)
    score, trans = _lattice(rng, 3, 6, False, False)
    terms = np.array([mr.path_score(score, trans, p, np.longdouble) for p in np.ndindex(*(3,) * 6)])
    z, _ = mr.recursion(score, trans, 5, 1, "sum")
    assert abs(float(z - (terms.max() + np.log(np.exp(terms - terms.max()).sum())))) <= 1e-15 * 10


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


def _call(nat, model, device=99, **change):
    """A valid batch of two contigs (2 and 3 genes), the set {1, 2} and a minimum of 2, on a device that does not exist, with
    `change` applied."""
    a = {"contig_ptr": np.array([0, 2, 5], dtype=np.int32), "n_contigs": 2, "gene_ptr": np.arange(0, 12, 2, dtype=np.int32),
         "attr_id": (np.arange(10, dtype=np.int32) * 3) % 7, "attr_value": None, "allowed": None, "set_mask": 6, "min_run": 2,
         "y": np.zeros(5, dtype=np.int8), "score": np.zeros(2), "lognorm_min_run": np.zeros(2), "lognorm": np.zeros(2)}
    a.update(change)
    fn = nat.load_library().gecco_crf_viterbi_min_run
    names = ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "set_mask", "min_run", "y", "score",
             "lognorm_min_run", "lognorm")
    args = [a[n].ctypes.data_as(t) if isinstance(a[n], np.ndarray) else a[n] for n, t in zip(names, fn.argtypes[2:])]
    rc = fn(model._h, device, *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


def test_host_refusals_come_before_the_device(nat, model3):
    call = lambda **kw: _call(nat, model3, **kw)
    # a valid call gets past the host checks: what stops it is the device that does not exist
    assert call()[0] not in (nat.OK, nat.EINVAL)
    assert call(lognorm=None, lognorm_min_run=None)[0] not in (nat.OK, nat.EINVAL)
    assert call(min_run=1, set_mask=7)[0] not in (nat.OK, nat.EINVAL) and call(min_run=32, set_mask=1)[0] not in (nat.OK, nat.EINVAL)
    # an argument error together with a device that does not exist reports the argument
    for bad in (0, -1, 33, 1 << 20):
        assert call(min_run=bad) == (nat.EINVAL, f"viterbi_min_run: min_run = {bad} is outside 1 .. 32")
    rc, msg = call(set_mask=0)
    assert rc == nat.EINVAL and "set_mask" in msg and "empty" in msg
    for bad in (8, 9, 1 << 31):
        rc, msg = call(set_mask=bad)
        assert rc == nat.EINVAL and "set_mask" in msg and f"at or above num_labels = 3 (mask {bad})" in msg
    assert call(y=None) == (nat.EINVAL, "null buffer") and call(score=None) == (nat.EINVAL, "null buffer")
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
    rc, msg = _call(nat, model3, contig_ptr=np.zeros(4, dtype=np.int32), n_contigs=3, score=np.zeros(3),
                    lognorm_min_run=np.full(3, 7.0), lognorm=np.full(3, 7.0), y=None)
    assert rc != nat.EINVAL, msg  # (ENODEV from the device that does not exist, or OK: never a complaint about an argument)


def test_the_native_wrapper_checks_its_arrays(nat, model3):
    cptr, gptr, attr = np.array([0, 2, 5], dtype=np.int32), np.arange(0, 12, 2, dtype=np.int32), (np.arange(10, dtype=np.int32) * 3) % 7
    with pytest.raises(ValueError, match="values holds 3 entries"):
        model3.viterbi_min_run(cptr, gptr, attr, 6, 2, values=np.ones(3))
    with pytest.raises(ValueError, match="allowed holds 2 masks for 5 genes"):
        model3.viterbi_min_run(cptr, gptr, attr, 6, 2, allowed=[1, 1])
    for bad in (0, 33):
        with pytest.raises(ValueError, match=rf"viterbi_min_run: min_run = {bad} is outside 1 \.\. 32"):
            model3.viterbi_min_run(cptr, gptr, attr, 6, bad, device=99)
    with pytest.raises(ValueError, match="set_mask"):
        model3.viterbi_min_run(cptr, gptr, attr, 0, 2, device=99)
    with pytest.raises(ValueError, match="set_mask"):
        model3.viterbi_min_run(cptr, gptr, attr, -1, 2)
    with pytest.raises(TypeError):
        model3.viterbi_min_run(cptr, gptr, attr, 6, 2.5)


def test_the_header_declares_the_entry_and_the_library_exports_it(nat):
    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    assert "ABI 2.20.0" in header
    for words in ("The tie rule is operational", "No feasible path", "Max semiring", "Sum semiring", "runs only when lognorm_min_run is given"):
        assert words in header, words
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+gecco_crf_viterbi_min_run\s*\(([^;]*)\)\s*;", code)
    assert m, "gecco_crf_viterbi_min_run is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "m", "device", "contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "set_mask", "min_run", "y", "score",
        "lognorm_min_run", "lognorm"]
    lib = nat.load_library()
    assert hasattr(lib, "gecco_crf_viterbi_min_run")
    assert len(nat.SIGNATURES["gecco_crf_viterbi_min_run"][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    sig = inspect.signature(nat.Model.viterbi_min_run)
    assert list(sig.parameters) == ["self", "contig_ptr", "gene_ptr", "attr_id", "set_mask", "min_run", "device", "values", "allowed",
                                    "want_lognorm"]
    assert sig.parameters["device"].default == 0 and sig.parameters["want_lognorm"].default is True


def test_the_kernel_file_is_built_without_contraction():
    from gecco_amd import build

    assert "crf_minrun.hip" in build.SOURCES and build.EXTRA_FLAGS["crf_minrun.hip"] == ["-ffp-contract=off"]


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

    for name in ("viterbi_min_run", "viterbi_kbest", "marginals_full", "viterbi"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [], [["a0", "a3"]]]


def test_bad_sets_and_minima_are_refused_before_any_device_call(crf):
    for bad in (0, -3, 33):
        with pytest.raises(ValueError, match=rf"min_run = {bad} is outside 1 \.\. 32"):
            crf.predict_min_run(X, ["y"], bad)
    for bad in (2.5, "3", None):
        with pytest.raises(ValueError, match="min_run is an integer"):
            crf.predict_min_run(X, ["y"], bad)
    with pytest.raises(ValueError, match="unknown label"):
        crf.predict_min_run(X, ["y", "q"], 2)
    with pytest.raises(ValueError, match="empty"):
        crf.predict_min_run(X, [], 2)
    with pytest.raises(ValueError, match="unknown label"):
        crf.predict_min_run(X, ["y"], 2, allowed=[["x", "q", None], [], [None]])
    assert "predict_min_run" in type(crf).__dict__ and "constraint_log_probability" in type(crf).predict_min_run.__doc__


def test_no_item_needs_no_device(crf):
    out = crf.predict_min_run([[], []], ["y", "z"], 3)
    assert out == [{"labels": [], "score": 0.0, "log_probability": 0.0, "constraint_log_probability": 0.0}] * 2
    assert crf.predict_min_run([], ["y"], 3) == []


def test_an_unfitted_model_is_refused():
    from gecco_amd.sequence import SequenceCRF

    with pytest.raises(ValueError, match="not fitted"):
        SequenceCRF(window_size=None).predict_min_run(X, ["y"], 2)


# ---------------------------------------------------------------- the typed front end
def test_the_typed_front_end_takes_the_arguments():
    from gecco_amd import typed

    params = inspect.signature(typed.TypedClusterCRF.predict_path_clusters).parameters
    assert params["min_run"].default == 3 and params["min_run"].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["known"].default is None
    assert "not annotated genes" in typed.TypedClusterCRF.predict_path_clusters.__doc__
    base = ["predict", "--model", "m", "-f", "f", "-g", "g"]
    assert typed.build_parser().parse_args(base).path_clusters is None
    assert typed.build_parser().parse_args(base + ["--path-clusters", "4"]).path_clusters == 4


def test_the_typed_front_end_checks_the_arguments_first():
    """Before the model is looked at: an unfitted one never gets to say so."""
    from gecco_amd import typed

    crf = typed.TypedClusterCRF()
    for bad, words in ((0, "min_run = 0 is outside 1 .. 32"), (33, "min_run = 33 is outside"), (1.5, "min_run is an integer")):
        with pytest.raises(ValueError, match=words):
            crf.predict_path_clusters([], min_run=bad)
    with pytest.raises(ValueError, match="not fitted"):
        crf.predict_path_clusters([], min_run=3)


def test_paths_table(tmp_path):
    from gecco_amd import typed

    rows = [{"sequence_id": "s1", "genes": 7, "log_z": 1.5, "score": 0.25, "log_p": -1.25, "constraint_log_p": -0.5, "clusters": 2},
            {"sequence_id": "s2", "genes": 1, "log_z": 0.5, "score": float("-inf"), "log_p": float("-inf"),
             "constraint_log_p": float("-inf"), "clusters": 0}]
    path = os.path.join(str(tmp_path), "paths.tsv")
    typed.write_paths(path, rows)
    got = [line.rstrip("\n").split("\t") for line in open(path)]
    assert got == [["sequence_id", "genes", "log_z", "score", "log_p", "constraint_log_p", "clusters"],
                   ["s1", "7", "1.5", "0.25", "-1.25", "-0.5", "2"], ["s2", "1", "0.5", "-inf", "-inf", "-inf", "0"]]
