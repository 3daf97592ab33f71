"""Marginals given a region and knock-out attributions, host side (no device): the numpy yardstick
(tests/conditionals_reference.py) pinned on path enumeration; the identity the product uses against scoring the changed input
again; the refusals of ``gecco_crf_span_conditionals``, ``SequenceCRF.predict_marginals_given_span`` and ``span_attributions``
before any device call; the header, the export and the typed command line's flags."""
import functools
import os
import re

import numpy as np
import pytest

from tests import conditionals_reference as cd
from tests import constrained_reference as cr
from tests import train_objective_partial as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 30
I32, U32, I64 = np.int32, np.uint32, np.int64


# ---------------------------------------------------------------- 1. the yardstick on path enumeration
def test_the_yardstick_on_path_enumeration_of_every_span_and_set():
    L = 3
    rng = np.random.default_rng(9100)
    w, trans = rng.normal(0.0, 1.5, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    lengths = [1, 2, 3, 4, 5, 6]
    cptr = np.concatenate([[0], np.cumsum(lengths)])
    deg = rng.integers(0, 5, size=int(cptr[-1]))
    gptr = np.concatenate([[0], np.cumsum(deg)]).astype(I32)
    attr = rng.integers(0, A, size=int(gptr[-1])).astype(I32)
    n = int(cptr[-1])
    worst_c = worst_p = 0.0
    count = 0
    for masked in (False, True):
        allowed = tp.full_masks(n, L)
        if masked:
            bits = rng.random((n, L)) < 0.7
            bits[~bits.any(axis=1), 0] = True
            allowed = (bits.astype(np.uint64) << np.arange(L, dtype=np.uint64)[None, :]).sum(axis=1).astype(U32)
        score = cr.masked_scores(gptr, attr, None, w, allowed)
        for c, T in enumerate(lengths):
            sc = score[cptr[c]:cptr[c + 1]]
            for b in range(T):
                for e in range(b + 1, T + 1):
                    for m in range(1, 8):
                        want, want_logp = cd.enumerate_region(sc, trans, b, e, m)
                        got, logze, logz = cd.region(sc, trans, b, e, m)
                        count += 1
                        assert np.isfinite(want_logp) == np.isfinite(logze)
                        if not np.isfinite(logze):
                            assert not got.any() and not want.any()
                            continue
                        worst_c = max(worst_c, float(np.abs(got - want).max()))
                        worst_p = max(worst_p, abs((logze - logz) - want_logp) / cd.bound_of(logze, logz))
                        assert np.all(np.abs(got - want) <= 1e-12)
                        assert abs((logze - logz) - want_logp) <= cd.bound_of(logze, logz)
                        assert np.all(got[b:e][:, [(m >> l) & 1 == 0 for l in range(L)]] == 0.0)
                        assert np.all(np.abs(got.sum(axis=1) - 1.0) <= 1e-12)
    print(f"{count} regions: worst |cond - enumeration| = {worst_c:.3g}, worst |logp - enumeration| / bound = {worst_p:.3g}")


# ---------------------------------------------------------------- 2. the identity against scoring again
def _lengths(rng):
    return [1, 2, 3] + [int(x) for x in rng.integers(1, 61, size=9)] + [300]


@functools.lru_cache(maxsize=None)
def _batch(L):
    rng = np.random.default_rng(7100 + L)
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    cptr = np.concatenate([[0], np.cumsum(_lengths(rng))]).astype(I32)
    deg = rng.integers(0, 5, size=int(cptr[-1]))
    gptr = np.concatenate([[0], np.cumsum(deg)]).astype(I32)
    attr = rng.integers(0, A, size=int(gptr[-1])).astype(I32)
    v = rng.normal(0.0, 1.0, size=len(attr))
    bits = rng.random((int(cptr[-1]), L)) < 0.8
    for i in np.flatnonzero(~bits.any(axis=1)):
        bits[i, int(rng.integers(0, L))] = True
    allowed = (bits.astype(np.uint64) << np.arange(L, dtype=np.uint64)[None, :]).sum(axis=1).astype(U32)
    return dict(L=L, w=w, trans=trans, cptr=cptr, gptr=gptr, attr=attr, v=v, allowed=allowed)


@pytest.mark.parametrize("valued,masked", [(False, False), (True, True)])
@pytest.mark.parametrize("L", [2, 3, 8, 17, 32])
def test_the_identity_against_scoring_the_changed_input_again(L, valued, masked):
    """log sum marg e^delta - log sum cond e^delta, from the yardstick's own two rows, against the region's log-probability
    before and after the change: within b1 + b2, the two log-probabilities' own bounds."""
    b = _batch(L)
    rng = np.random.default_rng(7200 + L)
    cptr, gptr, attr = b["cptr"], b["gptr"], b["attr"]
    every = tp.full_masks(int(cptr[-1]), L)
    score = cr.masked_scores(gptr, attr, b["v"] if valued else None, b["w"], b["allowed"] if masked else every)
    worst, cases, possible = 0.0, 0, 0
    for c in range(len(cptr) - 1):
        g0, T = int(cptr[c]), int(cptr[c + 1] - cptr[c])
        sc = score[g0:g0 + T]
        marg, _ = cr.marginals(np.array([0, T]), sc, b["trans"])
        for _ in range(2):
            lo = int(rng.integers(0, T))
            hi = int(rng.integers(lo + 1, T + 1))
            m = int(rng.integers(1, 1 << min(L, 31))) | ((1 << 31) if L == 32 and rng.random() < 0.5 else 0)
            cond, logze, logz = cd.region(sc, b["trans"], lo, hi, m)
            if not np.isfinite(logze):
                continue
            possible += 1
            for t in sorted({lo, hi - 1, max(lo - 1, 0), min(hi, T - 1), int(rng.integers(0, T))}):
                deltas = [None] + [-(b["v"][k] if valued else 1.0) * b["w"][attr[k]] for k in range(gptr[g0 + t], gptr[g0 + t + 1])]
                for delta in deltas:
                    want, bound = cd.contribution(sc, b["trans"], lo, hi, m, t, delta, base=(logze, logz))
                    d = np.where(np.isfinite(sc[t]), -sc[t], 0.0) if delta is None else delta
                    got = cd.identity(marg[t], cond[t], d)
                    worst = max(worst, abs(got - want) / bound)
                    cases += 1
                    assert abs(got - want) <= bound, (c, lo, hi, m, t)
    assert possible >= 8 and cases >= 50
    print(f"L={L} values={valued} allowed={masked}: {cases} knock-outs, worst |identity - scoring again| / bound = {worst:.3g}")


# ---------------------------------------------------------------- 3. refusals before any device call
ARGS = ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "span_contig", "span_begin", "span_end",
        "span_mask", "n_spans", "reach", "row_ptr", "occ_ptr", "logp", "cond", "item_contribution", "attr_contribution", "marg",
        "lognorm")


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    return _native


@pytest.fixture(scope="module")
def model3(nat):
    rng = np.random.default_rng(5)
    return nat.Model.from_tables(rng.normal(size=(7, 3)), rng.normal(size=(3, 3)))


def _call(nat, model, entry="gecco_crf_span_conditionals", **change):
    """A valid call on two contigs (2 and 3 genes, two attribute occurrences each), spans [0, 2) of contig 0 and [1, 3) of contig
    1 at reach 1, on a device that does not exist, with `change` applied."""
    a = {"contig_ptr": np.array([0, 2, 5], dtype=I32), "n_contigs": 2, "gene_ptr": np.arange(0, 12, 2, dtype=I32),
         "attr_id": (np.arange(10, dtype=I32) * 3) % 7, "attr_value": None, "allowed": None,
         "span_contig": np.array([0, 1], dtype=I32), "span_begin": np.array([0, 1], dtype=I32), "span_end": np.array([2, 3], dtype=I32),
         "span_mask": np.array([5, 2], dtype=U32), "n_spans": 2, "reach": 1, "row_ptr": np.array([0, 2, 5], dtype=I64),
         "occ_ptr": np.arange(0, 12, 2, dtype=I64), "logp": np.zeros(2), "cond": np.zeros(5 * 3), "item_contribution": np.zeros(5),
         "attr_contribution": np.zeros(10), "marg": np.zeros(5 * 3), "lognorm": np.zeros(2)}
    a.update(change)
    fn = getattr(nat.load_library(), entry)
    names = ARGS if entry == "gecco_crf_span_conditionals" else [n for n in ARGS if n not in (
        "reach", "row_ptr", "occ_ptr", "cond", "item_contribution", "attr_contribution")]
    args = [a[n].ctypes.data_as(t) if isinstance(a[n], np.ndarray) else a[n] for n, t in zip(names, fn.argtypes[2:])]
    rc = fn(model._h, 99, *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


def test_the_library_refuses_on_the_host_in_the_span_entrys_words(nat, model3):
    call = lambda **kw: _call(nat, model3, **kw)
    # a valid call gets past the host checks: what stops it is the device that does not exist
    assert call()[0] not in (nat.OK, nat.EINVAL)
    assert call(occ_ptr=None, attr_contribution=None, item_contribution=None)[0] not in (nat.OK, nat.EINVAL)
    for change in (dict(span_mask=np.array([5, 0], dtype=U32)), dict(span_mask=np.array([5, 9], dtype=U32)),
                   dict(span_contig=np.array([2, 0], dtype=I32)), dict(span_end=np.array([2, 4], dtype=I32)),
                   dict(span_begin=np.array([0, 3], dtype=I32)), dict(span_begin=np.array([-1, 1], dtype=I32)),
                   dict(contig_ptr=None)):
        got = call(**change)
        assert got[0] == nat.EINVAL and got == _call(nat, model3, "gecco_crf_span_probabilities", **change), change
        assert change.get("contig_ptr", 0) is None or got[1].startswith("span ")
    rc, msg = call(reach=-1)
    assert rc == nat.EINVAL and "reach = -1" in msg
    rc, msg = call(row_ptr=np.array([0, 2, 4], dtype=I64))
    assert rc == nat.EINVAL and msg.startswith("span 1: row_ptr[2] = 4, expected 5")
    rc, msg = call(row_ptr=np.array([1, 2, 5], dtype=I64))
    assert rc == nat.EINVAL and msg.startswith("span 0: row_ptr[0] = 1")
    rc, msg = call(reach=0)  # (the same tables at another reach: span 0 keeps its two rows, span 1 has two, not three)
    assert rc == nat.EINVAL and msg.startswith("span 1: row_ptr[2] = 5, expected 4")
    rc, msg = call(occ_ptr=np.array([0, 2, 4, 6, 9, 10], dtype=I64))
    assert rc == nat.EINVAL and msg.startswith("span 1: occ_ptr[4] = 9, expected 8")
    rc, msg = call(occ_ptr=None)
    assert rc == nat.EINVAL and "attr_contribution without occ_ptr" in msg
    assert call(cond=None) == (nat.EINVAL, "null buffer") and call(row_ptr=None) == (nat.EINVAL, "null buffer")


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

    for name in ("span_conditionals", "span_log_probabilities", "marginals_full", "viterbi", "windowed_marginals",
                 "windowed_marginals_all"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [], [["a0", "a3"]]]


@pytest.mark.parametrize("span,words", [
    ((0, 0, 2, "w"), "unknown label 'w'"),
    ((0, 0, 2, set()), "empty set"),
    ((3, 0, 1, "x"), "sequence index 3 out of range"),
    ((0, 2, 2, "x"), "start >= stop"),
    ((0, -1, 2, "x"), "start < 0"),
    ((0, 0, 4, "x"), "stop 4 lies beyond sequence 0 of 3 items"),
    ((1, 0, 1, "x"), "stop 1 lies beyond sequence 1 of 0 items"),
    ((0, 0, 2), "expected (sequence_index, start, stop, labels)"),
])
def test_bad_spans_are_refused_before_any_device_call_in_span_log_probabilitys_words(crf, span, words):
    good = (0, 0, 3, {"x", "y"})
    with pytest.raises(ValueError) as base:
        crf.span_log_probability(X, [good, span])
    for method in (crf.predict_marginals_given_span, crf.span_attributions):
        with pytest.raises(ValueError) as err:
            method(X, [good, span], reach=2)
        assert "span 1" in str(err.value) and words in str(err.value) and str(err.value) == str(base.value)


def test_a_bad_reach_is_refused_before_any_device_call(crf):
    for method in (crf.predict_marginals_given_span, crf.span_attributions):
        with pytest.raises(ValueError, match="reach = -1 is negative"):
            method(X, [(0, 0, 1, "x")], reach=-1)
        with pytest.raises(ValueError, match="not an integer"):
            method(X, [(0, 0, 1, "x")], reach=1.5)
        assert method(X, []) == []


# ---------------------------------------------------------------- 4. the header, the export, the command line
def test_the_header_declares_the_entry_and_the_library_exports_it():
    from gecco_amd import _native as nat

    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    assert "ABI 2.24.0" in header and "ABI 2.24.0 gecco_crf_span_conditionals" in re.sub(r"\s*\n \*\s*", " ", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+gecco_crf_span_conditionals\s*\(([^;]*)\)\s*;", code)
    assert m, "gecco_crf_span_conditionals is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["m", "device"] + list(ARGS)
    lib = nat.load_library()
    assert hasattr(lib, "gecco_crf_span_conditionals")
    assert len(nat.SIGNATURES["gecco_crf_span_conditionals"][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    assert callable(nat.Model.span_conditionals)
    from gecco_amd import build

    assert "crf_conditionals.hip" in build.SOURCES and build.EXTRA_FLAGS["crf_conditionals.hip"] == ["-ffp-contract=off"]


def test_the_typed_front_end_takes_the_flags():
    import inspect

    from gecco_amd import typed

    for name in ("predict_clusters", "predict_genes_and_clusters"):
        sig = inspect.signature(getattr(typed.TypedClusterCRF, name)).parameters
        assert sig["attributions"].default is False and sig["attribution_reach"].default == 10
    base = ["predict", "--model", "m", "-f", "f", "-g", "g"]
    args = typed.build_parser().parse_args(base)
    assert args.attributions is False and args.attribution_reach == 10
    args = typed.build_parser().parse_args(base + ["--attributions", "--attribution-reach", "3"])
    assert args.attributions is True and args.attribution_reach == 3
