"""Max-marginals without a device: the yardstick's two forms against each other (tests/maxmarg_reference.py: the max-plus
forward/backward and its masked-Viterbi walks equal path enumeration), the identities of exact max-marginals under integer
weights, the bound's constant, the host refusals of ``gecco_crf_max_marginals``, the header and the signatures of ABI 2.25.0,
and the argument checks of ``SequenceCRF.predict_max_marginals`` / ``span_best_scores`` and of the typed front end's
``margins`` plumbing, which come before any device call."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import maxmarg_reference as mr
from tests.test_gpu_kbest import enumeration_batch, tables
from tests.test_kbest_host import _lattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _queries(rng, L, T):
    full = (1 << L) - 1
    sets = [full] + [int(rng.integers(1, full + 1)) for _ in range(3)]
    spans = [(0, T, full), (0, 1, int(rng.integers(1, full + 1))), (T - 1, T, int(rng.integers(1, full + 1)))]
    for _ in range(4):
        lo = int(rng.integers(0, T))
        spans.append((lo, int(rng.integers(lo + 1, T + 1)), int(rng.integers(1, full + 1))))
    return sets, spans


def _same(a, b, exact):
    for name in ("best", "through", "inside", "outside", "span_best", "span_broken"):
        x, y = np.asarray(a[name], dtype=np.float64), np.asarray(b[name], dtype=np.float64)
        assert x.shape == y.shape and not np.isnan(x).any() and not np.isnan(y).any(), name
        assert np.array_equal(np.isneginf(x), np.isneginf(y)), f"{name}: -inf in other places"
        fin = np.isfinite(x)
        if exact:
            assert np.array_equal(x[fin], y[fin]), name
        else:
            assert np.all(np.abs(x[fin] - y[fin]) <= 1e-12 * np.maximum(1.0, np.abs(x[fin]))), name


# ---------------------------------------------------------------- the yardstick: (b) equals (a)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("L", [2, 3, 5])
def test_forward_backward_equals_enumeration(L, T, masked):
    rng = np.random.default_rng(300 * L + 10 * T + masked)
    for integer in (False, True):
        score, trans = _lattice(rng, L, T, masked, integer)
        sets, spans = _queries(rng, L, T)
        want = mr.enumerate_all(score, trans, sets, spans)
        got = mr.all_quantities(score, trans, sets, spans)
        _same(got, want, exact=integer)
        by_items = [mr.span_broken_by_items(score, trans, b, e, m) for b, e, m in spans]
        _same(dict(got, span_broken=np.array(by_items)), want, exact=integer)


@pytest.mark.parametrize("L", [2, 4, 8])
def test_forward_backward_equals_enumeration_on_the_enumeration_batches(L):
    """The batches of the device tests, each plain, valued, masked, and valued plus masked; the sequences short enough to list."""
    b = enumeration_batch(L)
    rng = np.random.default_rng(L)
    done = 0
    for valued, masked in ((False, False), (True, False), (False, True), (True, True)):
        score, _ = tables(b, valued, masked)
        for c in range(len(b["cptr"]) - 1):
            g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
            if g1 == g0 or L ** (g1 - g0) > 4096:
                continue
            sets, spans = _queries(rng, L, g1 - g0)
            _same(mr.all_quantities(score[g0:g1], b["trans"], sets, spans), mr.enumerate_all(score[g0:g1], b["trans"], sets, spans), False)
            done += 1
    assert done >= 100


# ---------------------------------------------------------------- exact arithmetic: the identities
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("L,T", [(2, 1), (2, 9), (3, 30), (5, 64), (17, 33), (32, 12)])
def test_identities_hold_exactly_with_integer_weights(L, T, masked):
    rng = np.random.default_rng(17 * L + T + masked)
    score, trans = _lattice(rng, L, T, masked, integer=True)
    full = (1 << L) - 1
    th = mr.through(score, trans)
    best = mr.viterbi_score(score, trans)
    y = mr.viterbi_path(score, trans)
    assert mr.path_score(score, trans, y) == best
    assert np.all(th.max(axis=1) == best), "max_l through_t(l) = best at every t"
    assert np.all(th[np.arange(T), y] == best), "through_t(y*_t) = best"
    contained = left = 0
    for _ in range(40):
        lo = int(rng.integers(0, T))
        hi = int(rng.integers(lo + 1, T + 1))
        mask = int(rng.integers(1, full + 1))
        inside, broken = mr.span_best(score, trans, lo, hi, mask), mr.span_broken(th, lo, hi, mask)
        assert broken == mr.span_broken_by_items(score, trans, lo, hi, mask)
        assert mr.span_best(score, trans, lo, hi, full) == best and mr.span_broken(th, lo, hi, full) == -np.inf
        assert max(inside, broken) == best, "max(span_best, span_broken) = best"
        stays = all((mask >> lab) & 1 for lab in y[lo:hi])
        if stays:
            contained += 1
            assert best - inside == 0.0, "margin_present = 0 when the Viterbi path lies in the set on the span"
        else:
            left += 1
            assert broken == best and best - inside >= 0.0
            # (0 here only through a tie: another best path that does stay inside)
            if best - inside == 0.0:
                masked_table = score.copy()
                masked_table[lo:hi, ~mr.members(mask, L)] = -np.inf
                other = mr.viterbi_path(masked_table, trans)
                assert other != y and mr.path_score(score, trans, other) == best
    assert contained or left


def test_the_bound_is_the_derived_one():
    abs_score = np.array([[1.0, 2.0], [0.5, 0.25], [3.0, 1.0]])
    abs_T = np.array([[0.5, 1.5], [1.0, 0.0]])
    assert mr.bound(abs_score, abs_T) == 4.0 * 3 * mr.EPS * ((2.0 + 0.5 + 3.0) + 2 * 1.5)
    assert mr.bound(abs_score[:1], abs_T) == 4.0 * mr.EPS * 2.0
    for T in range(1, 400):  # the additions on a path through a and b, and an item's own, under the constant
        assert 2 * T - 1 + 3 <= 4 * T
    with pytest.raises(ValueError):
        mr.bound(abs_score, abs_T, max_terms=4)


# ---------------------------------------------------------------- the C entry: refusals before the device, header, signatures
L3 = 3


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    return _native


@pytest.fixture(scope="module")
def model3(nat):
    rng = np.random.default_rng(5)
    return nat.Model.from_tables(rng.normal(size=(7, L3)), rng.normal(size=(L3, L3)))


NAMES = ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "set_mask", "n_sets", "span_contig", "span_begin",
         "span_end", "span_mask", "n_spans", "through", "inside", "outside", "span_best", "span_broken", "best", "lognorm")


def _call(nat, model, **change):
    """A valid batch of two contigs (2 and 3 genes), two sets and two spans, on a device that does not exist, with `change`."""
    i32, u32 = (lambda *x: np.array(x, dtype=np.int32)), (lambda *x: np.array(x, dtype=np.uint32))
    a = {"contig_ptr": i32(0, 2, 5), "n_contigs": 2, "gene_ptr": np.arange(0, 12, 2, dtype=np.int32),
         "attr_id": (np.arange(10, dtype=np.int32) * 3) % 7, "attr_value": None, "allowed": None, "set_mask": u32(7, 2), "n_sets": 2,
         "span_contig": i32(0, 1), "span_begin": i32(0, 1), "span_end": i32(2, 3), "span_mask": u32(1, 6), "n_spans": 2,
         "through": np.zeros(5 * 3), "inside": np.zeros(5 * 2), "outside": np.zeros(5 * 2), "span_best": np.zeros(2),
         "span_broken": np.zeros(2), "best": np.zeros(2), "lognorm": np.zeros(2)}
    a.update(change)
    fn = nat.load_library().gecco_crf_max_marginals
    args = [a[n].ctypes.data_as(t) if isinstance(a[n], np.ndarray) else a[n] for n, t in zip(NAMES, fn.argtypes[2:])]
    rc = fn(model._h, 99, *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


def test_host_refusals_come_before_the_device(nat, model3):
    call = lambda **kw: _call(nat, model3, **kw)  # noqa: E731
    i32, u32 = (lambda *x: np.array(x, dtype=np.int32)), (lambda *x: np.array(x, dtype=np.uint32))
    # a valid call gets past the host checks: what stops it is the device that does not exist
    assert call()[0] not in (nat.OK, nat.EINVAL)
    for name in ("through", "inside", "outside", "span_best", "span_broken", "lognorm"):
        assert call(**{name: None})[0] not in (nat.OK, nat.EINVAL), name
    assert call(n_sets=0, set_mask=None, inside=None, outside=None)[0] not in (nat.OK, nat.EINVAL)
    assert call(n_spans=0, span_best=None, span_broken=None)[0] not in (nat.OK, nat.EINVAL)
    assert call(set_mask=np.full(32, 5, dtype=np.uint32), n_sets=32, inside=np.zeros(160), outside=np.zeros(160))[0] not in (nat.OK, nat.EINVAL)
    for bad in (-1, 33, 1 << 20):
        assert call(n_sets=bad) == (nat.EINVAL, f"max_marginals: n_sets = {bad} is outside 0 .. 32")
    assert call(set_mask=u32(7, 0)) == (nat.EINVAL, "max_marginals: set 1: the label set is empty (a mask of 0)")
    assert call(set_mask=u32(9, 1)) == (nat.EINVAL, "max_marginals: set 0: the set holds a label at or above num_labels = 3 (mask 9)")
    for keep in ("inside", "outside"):
        other = "outside" if keep == "inside" else "inside"
        assert call(n_sets=0, **{other: None}) == (nat.EINVAL, "max_marginals: inside or outside given without a label set")
    for keep in ("span_best", "span_broken"):
        other = "span_broken" if keep == "span_best" else "span_best"
        assert call(n_spans=0, **{other: None}) == (nat.EINVAL, "max_marginals: span_best or span_broken given without spans")
    assert call(n_spans=-1) == (nat.EINVAL, "max_marginals: negative number of spans")
    # the span checks of gecco_crf_span_probabilities
    assert call(span_contig=i32(0, 2)) == (nat.EINVAL, "max_marginals: span 1: contig 2 out of range (the batch has 2)")
    assert call(span_contig=i32(-1, 1))[1].startswith("max_marginals: span 0: contig -1 out of range")
    assert call(span_end=i32(3, 3)) == (nat.EINVAL, "max_marginals: span 0: [0, 3) is not a non-empty range inside contig 0 of 2 genes")
    assert call(span_begin=i32(0, 3))[1].startswith("max_marginals: span 1: [3, 3) is not a non-empty range")
    assert call(span_begin=i32(-1, 1))[1].startswith("max_marginals: span 0: [-1, 2) is not a non-empty range")
    assert call(span_mask=u32(1, 0)) == (nat.EINVAL, "max_marginals: span 1: the label set is empty (a mask of 0)")
    assert call(span_mask=u32(8, 1))[1].startswith("max_marginals: span 0: the set holds a label at or above num_labels = 3")
    assert call(span_mask=None)[0] == nat.EINVAL and call(set_mask=None)[0] == nat.EINVAL and call(best=None)[0] == nat.EINVAL
    # the checks of the _valued and _constrained entries
    v = np.ones(10)
    v[3] = np.inf
    assert call(attr_value=v) == (nat.EINVAL, "attribute value 3 is not finite (NaN or infinite)")
    assert call(allowed=u32(7, 1, 0, 4, 3)) == (nat.EINVAL, "constrained: gene 2 allows no label (a mask of 0)")
    assert call(allowed=u32(7, 1, 6, 4, 9)) == (nat.EINVAL, "constrained: gene 4 allows a label at or above num_labels = 3 (mask 9)")
    assert call(contig_ptr=None)[0] == nat.EINVAL and call(n_contigs=-1)[0] == nat.EINVAL
    assert call(gene_ptr=None) == (nat.EINVAL, "null buffer")


def test_a_batch_without_genes_needs_no_device(nat, model3):
    best, lognorm = np.full(3, 9.0), np.full(3, 7.0)
    rc, msg = _call(nat, model3, contig_ptr=np.zeros(4, dtype=np.int32), n_contigs=3, n_spans=0, span_best=None, span_broken=None,
                    best=best, lognorm=lognorm)
    assert rc != nat.EINVAL, msg  # (ENODEV from the device that does not exist, or OK: never a complaint about an argument)
    if rc == nat.OK:
        assert np.all(best == 0.0) and np.all(lognorm == 0.0)


def test_the_header_declares_the_entry_and_the_library_exports_it(nat):
    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    assert "ABI 2.25.0" in header and "ABI 2.25.0 gecco_crf_max_marginals" in flat
    for words in ("not clamped", "span_broken[q]", "never NaN", "0 <= n_sets <= 32", "not posteriors", "16 * n_genes * L bytes"):
        assert words in flat, words
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+gecco_crf_max_marginals\s*\(([^;]*)\)\s*;", code)
    assert m, "gecco_crf_max_marginals is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["m", "device", *NAMES]
    lib = nat.load_library()
    assert hasattr(lib, "gecco_crf_max_marginals")
    assert len(nat.SIGNATURES["gecco_crf_max_marginals"][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    sig = inspect.signature(nat.Model.max_marginals)
    assert list(sig.parameters)[:9] == ["self", "contig_ptr", "gene_ptr", "attr_id", "sets", "spans", "device", "values", "allowed"]
    assert sig.parameters["want_lognorm"].default is False and sig.parameters["want_through"].default is True


def test_the_kernel_file_is_built_without_contraction():
    from gecco_amd import build

    assert "crf_maxmarg.hip" in build.SOURCES and build.EXTRA_FLAGS["crf_maxmarg.hip"] == ["-ffp-contract=off"]
    text = open(os.path.join(ROOT, "gecco_amd", "csrc", "crf_maxmarg.hip")).read()
    assert '#include "crf_contig_walk.hpp"' in text and "load_trans<true>" in text and "max_plus(" in text
    assert "atomic" not in text.replace("No atomics", "")


def test_the_native_wrapper_checks_its_arrays(nat, model3):
    cptr, gptr, attr = np.array([0, 2, 5], dtype=np.int32), np.arange(0, 12, 2, dtype=np.int32), (np.arange(10, dtype=np.int32) * 3) % 7
    with pytest.raises(ValueError, match="values holds 3 entries"):
        model3.max_marginals(cptr, gptr, attr, values=np.ones(3))
    with pytest.raises(ValueError, match="allowed holds 2 masks for 5 genes"):
        model3.max_marginals(cptr, gptr, attr, allowed=[1, 1])
    with pytest.raises(ValueError, match="the span arrays differ in length"):
        model3.max_marginals(cptr, gptr, attr, spans=([0], [0, 1], [1], [1]))
    with pytest.raises(ValueError, match=r"max_marginals: n_sets = 33 is outside 0 \.\. 32"):
        model3.max_marginals(cptr, gptr, attr, sets=[1] * 33)
    with pytest.raises(ValueError, match="max_marginals: set 0: the label set is empty"):
        model3.max_marginals(cptr, gptr, attr, sets=[0])


# ---------------------------------------------------------------- SequenceCRF and the typed front end
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

    for name in ("max_marginals", "marginals_full", "viterbi", "span_log_probabilities"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [], [["a0", "a3"]]]


def test_unknown_labels_and_empty_sets_are_refused_before_any_device_call(crf):
    with pytest.raises(ValueError, match="set 1: unknown label 'w'"):
        crf.predict_max_marginals(X, sets=["x", "w"])
    with pytest.raises(ValueError, match="set 0: an empty set holds no label"):
        crf.predict_max_marginals(X, sets=[set()])
    with pytest.raises(ValueError, match="sets is a list of label sets"):
        crf.predict_max_marginals(X, sets=5)
    with pytest.raises(ValueError, match="unknown label 'w'"):
        crf.predict_max_marginals(X, allowed=[["x", "w", None], [], [None]])
    for spans, text in (([(0, 0, 2, "w")], "span 0: unknown label 'w'"), ([(0, 0, 2, [])], "span 0: an empty set holds no label"),
                        ([(0, 0, 1, "x"), (3, 0, 1, "x")], "span 1: sequence index 3 out of range"),
                        ([(0, 2, 2, "x")], r"span 0: \[2, 2\) is not a non-empty range"), ([(0, -1, 2, "x")], r"span 0: \[-1, 2\)"),
                        ([(2, 0, 2, "x")], "span 0: stop 2 lies beyond sequence 2 of 1 items"),
                        ([(1, 0, 1, "x")], "span 0: stop 1 lies beyond sequence 1 of 0 items"), ([(0, 1)], "span 0: expected")):
        with pytest.raises(ValueError, match=text):
            crf.span_best_scores(X, spans)
    # nothing to ask: no device either
    assert all(v.shape == (0,) for v in crf.span_best_scores(X, []).values())
    empty = crf.predict_max_marginals([[], []], sets=["x"])
    assert len(empty) == 2 and empty[0]["through"].shape == (0, 3) and empty[0]["best"] == 0.0 and empty[1]["inside"].shape == (0, 1)


def test_the_docstrings_say_what_the_numbers_are():
    from gecco_amd import typed
    from gecco_amd.sequence import SequenceCRF

    for doc in (SequenceCRF.predict_max_marginals.__doc__, SequenceCRF.span_best_scores.__doc__, typed.TypedClusterCRF._margins.__doc__):
        flat = re.sub(r"\s+", " ", doc)
        assert "score differences" in flat or "difference of two path scores" in flat
        assert "ratio of the probabilities of two single" in flat and "not posteriors" in flat or "not a posterior" in flat
        assert "not a windowed one" in flat or "not of the windowed one" in flat


def test_the_typed_front_end_takes_the_option():
    from gecco_amd import typed

    for fn in (typed.TypedClusterCRF.predict_clusters, typed.TypedClusterCRF.predict_genes_and_clusters):
        assert inspect.signature(fn).parameters["margins"].default is False
    args = typed.build_parser().parse_args(["predict", "--model", "m", "--genes", "g", "--features", "f", "--margins"])
    assert args.margins is True
    assert typed.build_parser().parse_args(["predict", "--model", "m", "--genes", "g", "--features", "f"]).margins is False
