"""The whole-contig sum-product pass at its transition-range guards, and beyond them: ``marginals_full`` and the two queries
whose range argument leans on it (``edge_posteriors``, ``span_log_probabilities``) through every whole-contig arrangement, on the
planted transition families of tests/lattice_range_families.py, against the log-space yardsticks that
tests/test_lattice_range_host.py pins on path enumeration on these very inputs (``constrained_reference.marginals``,
``edges_reference.edge_posteriors``, the ``_yardstick`` of tests/test_gpu_spans.py).  ``oracle.crf_oracle.full_marginals`` is not
used: it is a scaled linear-space recursion with the same exp(trans) in it.

The guards read the transition weights alone (crf_plan.cpp): ``rows_rescale_period`` (4 max|trans| < 600: family a stands one
grid step under and exactly at max|trans| = 150, on both signs), ``raw_fold`` (8 (max - min) < 600: family b at a spread of 74.9
and 75.1) and the range of exp(trans) on the any-L route (family e, shifts of +-800).  Every arrangement is forced by its
switch, so each is run at period 4 and 1, and the 2-label scan with raw_fold 1 and 0.

Tolerances are the ones tests/test_gpu_general.py holds these kernels to at ordinary weights: marginals within 1e-12 of the
yardstick, rows summing to 1 within 1e-13, log Z within 1e-10 max(1, |log Z|); the queries under the bounds of the ``_check``
functions of tests/test_gpu_edges.py and tests/test_gpu_spans.py, imported.  Every family meets every arrangement in full: the
yardstick of a (label count, model) is computed once and shared by the arrangements of that label count, which is what keeps a
case at a second or two.  Every case prints its worst |error| and worst error / bound."""
import functools

import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import edges_reference as er
from tests import lattice_range_families as fam
from tests import test_gpu_edges as ge
from tests import test_gpu_spans as gs
from tests import train_objective_partial as tp

pytestmark = pytest.mark.gpu

FORCE, CHUNKED, MARGINALS = "GECCO_CRF_FORCE_GENERAL", "GECCO_CRF_GENERAL_CHUNKED", "GECCO_CRF_GENERAL_MARGINALS"
# (id, labels, the switches): the 2-label scan, and the five any-L arrangements
ARRANGEMENTS = ([("L2-scan", 2, ()), ("L2-general", 2, ((FORCE, "1"),))] +
                [(f"L{L}-chunked", L, ()) for L in (3, 8)] + [(f"L{L}-sequential", L, ((CHUNKED, "0"),)) for L in (3, 8)] +
                [(f"L{L}-{mode}", L, ((MARGINALS, mode),)) for L in (9, 17, 32) for mode in ("wave", "chunked", "split")])
QUERY_ARRANGEMENTS = [a for a in ARRANGEMENTS if a[1] > 2 and not (a[2] and a[2][0][0] == CHUNKED)]
ARR_IDS = [a[0] for a in ARRANGEMENTS]
FAMILIES = {"a": fam.SHIFTS_A, "b": fam.FAR_B, "c": fam.FORBID_C, "d": fam.LEADERS_D}
REFUSAL = "transition weight"


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


def _switch(monkeypatch, switches):
    for name in (FORCE, CHUNKED, MARGINALS):
        monkeypatch.delenv(name, raising=False)
    for name, value in switches:
        monkeypatch.setenv(name, value)


# ---------------------------------------------------------------- the yardstick, computed once per (label count, model)
@functools.lru_cache(maxsize=None)
def _score(L, leaders, lengths):
    cptr, gptr, attr = fam.batch(L, lengths, leaders)
    w = fam.leader_weights(L) if leaders else fam.base(L)[0]
    score = cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L))
    score.setflags(write=False)
    return score


@functools.lru_cache(maxsize=None)
def _reference(L, family, key, lengths=fam.LENGTHS):
    """(marginals, log Z) of a planted model over the batch, read only."""
    _, trans, leaders = fam.model_of(L, family, key)
    marg, logz = cr.marginals(fam.batch(L, lengths, leaders)[0], _score(L, leaders, lengths), trans)
    marg.setflags(write=False)
    logz.setflags(write=False)
    return marg, logz


def _judge(tag, marg, logz, ref_marg, ref_logz):
    """marginals_full's outputs against a yardstick under the module's tolerances: (worst |marginal error|, worst log Z
    error / bound), printed before anything is asserted."""
    assert marg.shape == ref_marg.shape and logz.shape == ref_logz.shape
    finite = bool(np.all(np.isfinite(marg)) and np.all(np.isfinite(logz)))
    with np.errstate(invalid="ignore"):
        dm = float(np.abs(marg - ref_marg).max(initial=0.0))
        ds = float(np.abs(marg.sum(axis=1) - 1.0).max(initial=0.0))
        dz = float((np.abs(logz - ref_logz) / (1e-10 * np.maximum(1.0, np.abs(ref_logz)))).max(initial=0.0))
    print(f"{tag}: worst |marginal error| = {dm:.3g} (x{dm / 1e-12:.3g} of 1e-12), worst |row sum - 1| = {ds:.3g}, "
          f"worst |log Z error| / bound = {dz:.3g}" + ("" if finite else "  NOT FINITE"))
    assert finite, f"{tag}: NaN or infinity with a clean status"
    assert marg.min(initial=0.0) >= 0.0 and marg.max(initial=0.0) <= 1.0, f"{tag}: a marginal outside [0, 1]"
    assert dm <= 1e-12, f"{tag}: marginals off by {dm:.3g}"
    assert ds <= 1e-13, f"{tag}: a row sums to 1 +- {ds:.3g}"
    assert dz <= 1.0, f"{tag}: log Z off by {dz:.3g} of its bound"
    return dm, dz


def _dead_pairs(L, what, lengths=fam.LENGTHS):
    dead = fam.forbidden(L, what)[1]
    return np.concatenate([dead(T) for T in lengths], axis=0)


# ---------------------------------------------------------------- 1. marginals_full, every family, every arrangement
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("name,L,switches", ARRANGEMENTS, ids=ARR_IDS)
def test_marginals_on_every_family_through_every_arrangement(nat, monkeypatch, name, L, switches, family):
    _switch(monkeypatch, switches)
    sides, failed = set(), []
    for key in FAMILIES[family]:
        w, trans, leaders = fam.model_of(L, family, key)
        fig = fam.figures(trans)
        assert fig["in_range"]
        sides.add((fig["period"], fig["raw_fold"]))
        csr = fam.batch(L, fam.LENGTHS, leaders)
        model = nat.Model.from_tables(w, trans)
        marg, logz = model.marginals_full(*csr)
        tag = f"{name} family {family} {key} (period {fig['period']}, raw_fold {fig['raw_fold']})"
        try:  # (every model of the family is run and printed before the case fails)
            _judge(tag, marg, logz, *_reference(L, family, key))
            assert logz[fam.LENGTHS.index(0)] == 0.0, f"{tag}: a contig without items has log Z 0"
            if family == "c":  # a pair that no path goes through: below 1e-300 or an exact 0
                dead = _dead_pairs(L, key)
                assert (key == "diagonal") != bool(dead.any())
                assert np.all(marg[dead] < 1e-300), f"{tag}: mass {marg[dead].max():.3g} on a forbidden (item, label) pair"
        except AssertionError as miss:
            failed.append(str(miss).splitlines()[0])
    assert not failed, "\n".join(failed)
    if family == "a":
        assert {p for p, _ in sides} == {1, 4}, "rows_rescale_period 4 and 1 are both visited"
    if family == "b":
        assert {f for _, f in sides} == {0, 1} and {p for p, _ in sides} == {1, 4}, "raw_fold 1 and 0 are both visited"
    if family == "d":
        assert {f for _, f in sides} == {0, 1}


@pytest.mark.parametrize("name,L,switches", [("L3-chunked", 3, ()), ("L17-chunked", 17, ((MARGINALS, "chunked"),))], ids=["L3", "L17"])
def test_a_contig_past_the_long_contig_threshold(nat, monkeypatch, name, L, switches):
    """2049 items: chunks of 64 genes (kGenLongContig), 33 of them on one chunk walk, at max|trans| = 150 on both signs."""
    _switch(monkeypatch, switches)
    assert fam.LONG_LENGTHS[0] == 2049
    for key in ("at+", "at-"):
        w, trans, _ = fam.model_of(L, "a", key)
        assert np.abs(trans).max() == 150.0 and fam.figures(trans)["period"] == 1
        marg, logz = nat.Model.from_tables(w, trans).marginals_full(*fam.batch(L, fam.LONG_LENGTHS))
        _judge(f"{name} 2049 items, family a {key}", marg, logz, *_reference(L, "a", key, fam.LONG_LENGTHS))


# ---------------------------------------------------------------- 2. shift invariance on the device
@pytest.mark.parametrize("name,L,switches", ARRANGEMENTS, ids=ARR_IDS)
def test_a_uniform_shift_changes_log_z_by_its_multiple_and_nothing_else(nat, monkeypatch, name, L, switches):
    """trans + c is the base model's distribution (exactly: the family's grid), so ONE yardstick, the base model's, judges the
    base model and every shifted one, and the two log Z differ by (T - 1) c.  A wrong rescaling period or a dropped scale
    factor fails here, and a wrong reference cannot: tests/test_lattice_range_host.py holds the yardstick to this identity."""
    _switch(monkeypatch, switches)
    w, trans = fam.base(L)
    csr = fam.batch(L)
    steps = np.maximum(np.diff(csr[0]).astype(np.float64) - 1.0, 0.0)
    ref_marg, ref_logz = _reference(L, "base", None)
    marg0, logz0 = nat.Model.from_tables(w, trans).marginals_full(*csr)
    _judge(f"{name} base model", marg0, logz0, ref_marg, ref_logz)
    failed = []
    for which in fam.SHIFTS_A:
        moved, c = fam.shifted(L, which)
        marg, logz = nat.Model.from_tables(w, moved).marginals_full(*csr)
        try:  # (every shift is run and printed before the case fails)
            _judge(f"{name} shift {which} against the base model's yardstick", marg, logz, ref_marg, ref_logz + steps * c)
            gap = np.abs((logz - logz0) - steps * c)
            bound = 1e-10 * (np.maximum(1.0, np.abs(logz)) + np.maximum(1.0, np.abs(logz0)))  # (each of the two within its own)
            print(f"{name} shift {which}: worst |(log Z' - log Z) - (T - 1) c| / bound = {float((gap / bound).max()):.3g}")
            assert np.all(gap <= bound), f"{name} shift {which}: log Z' - log Z is not (T - 1) c"
        except AssertionError as miss:
            failed.append(str(miss).splitlines()[0])
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------- 3. the queries behind the pass
QUERY_MODELS = [("a", "under+"), ("a", "at+"), ("a", "under-"), ("a", "at-"), ("b", 151.0)]


def _sets(L):
    """Two sets for enter / leave: the even labels, and the last label alone."""
    return (sum(1 << y for y in range(0, L, 2)), 1 << (L - 1))


@functools.lru_cache(maxsize=None)
def _phase_spans(L):
    """Spans whose first item is = 0, 1, 2, 3 (mod 4) and whose last item is = 0, 1, 2, 3 (mod 4), all sixteen pairs on each of
    the contigs of 9, 33, 65 and 129 items, so that every phase of the period-4 rescaling borders a span on both sides; the
    whole 300-item contig under the full set (exactly 0.0) and three more spans of it."""
    rng = np.random.default_rng(7500 + L)
    spans = []
    for T in (9, 33, 65, 129):
        c = fam.LENGTHS.index(T)
        for rb in range(4):
            for re in range(4):
                b = rb + (4 * ((rb + re) % 2) if T > 9 else 0)
                lasts = [x for x in range(b, T) if x % 4 == re]
                last = lasts[-1] if (rb + re) % 2 else lasts[len(lasts) // 2]
                spans.append((c, b, last + 1, gs._set_mask(rng, L, "random")))
    c300 = fam.LENGTHS.index(300)
    spans += [(c300, 0, 300, (1 << L) - 1), (c300, 0, 300, gs._set_mask(rng, L, "random")), (c300, 63, 298, gs._set_mask(rng, L, "random")),
              (c300, 2, 65, gs._set_mask(rng, L, "singleton"))]
    assert {(s[1] % 4, (s[2] - 1) % 4) for s in spans} >= {(x, y) for x in range(4) for y in range(4)}
    return tuple(spans)


@functools.lru_cache(maxsize=None)
def _query_reference(L, family, key):
    """(edge posteriors, (span log-probabilities, bounds)) of a planted model, read only."""
    _, trans, leaders = fam.model_of(L, family, key)
    cptr, score = fam.batch(L, fam.LENGTHS, leaders)[0], _score(L, leaders, fam.LENGTHS)
    return er.edge_posteriors(cptr, score, trans, _sets(L)), gs._yardstick(cptr, score, trans, list(_phase_spans(L)))


@pytest.mark.parametrize("family,key", QUERY_MODELS, ids=[f"{f}-{k}" for f, k in QUERY_MODELS])
@pytest.mark.parametrize("name,L,switches", QUERY_ARRANGEMENTS, ids=[a[0] for a in QUERY_ARRANGEMENTS])
def test_the_queries_read_directions_whatever_the_scaling(nat, monkeypatch, name, L, switches, family, key):
    _switch(monkeypatch, switches)
    w, trans, leaders = fam.model_of(L, family, key)
    fig = fam.figures(trans)
    csr = fam.batch(L, fam.LENGTHS, leaders)
    sets, spans = _sets(L), list(_phase_spans(L))
    ref_edges, (ref_spans, bound) = _query_reference(L, family, key)
    tag = f"{name} family {family} {key} (period {fig['period']})"
    model = nat.Model.from_tables(w, trans)
    emarg, elogz = model.marginals_full(*csr)
    out = model.edge_posteriors(*csr, sets=np.array(sets, dtype=np.uint32), want_pair=True, want_marginals=True)
    ge._check(f"{tag} edges", out, ref_edges, csr[0], L, sets)
    assert out["marginals"].tobytes() == emarg.tobytes() and out["lognorm"].tobytes() == elogz.tobytes(), "marginals_full's bytes"
    logp, marg, logz = model.span_log_probabilities(*csr, *gs._arrays(spans), want_marginals=True)
    assert np.isfinite(ref_spans).all()
    gs._check(f"{tag} spans", logp, ref_spans, bound, spans, L)
    assert marg.tobytes() == emarg.tobytes() and logz.tobytes() == elogz.tobytes(), "marginals_full's bytes"


# ---------------------------------------------------------------- 4. outside exp's range
def _correct_or_refused(tag, call, judge, must_answer=False):
    """The disjunction of family e: the call returns and is right under `judge`, or it raises the binding's exception for
    GECCO_CRF_EINVAL with a message that names the transition weights.  Never NaN, infinities or wrong numbers with a clean
    status.  `must_answer`: refusing is not an option (the 2-label scan, whose constants are ratios of transitions)."""
    try:
        got = call()
    except ValueError as refusal:
        print(f"{tag}: refused -- {refusal}")
        assert not must_answer, f"{tag}: refused a model it can run"
        assert REFUSAL in str(refusal) and "700" in str(refusal), f"{tag}: the refusal does not name the transition weights"
        return "refused"
    judge(got)
    return "answered"


@pytest.mark.parametrize("c", fam.SHIFTS_E)
@pytest.mark.parametrize("name,L,switches", ARRANGEMENTS, ids=ARR_IDS)
def test_transition_weights_outside_the_range_of_exp(nat, monkeypatch, name, L, switches, c):
    _switch(monkeypatch, switches)
    w = fam.base(L)[0]
    moved, shift = fam.shifted(L, c)
    assert shift == c and not fam.figures(moved)["in_range"] and np.all(np.isfinite(moved))
    csr = fam.batch(L)
    steps = np.maximum(np.diff(csr[0]).astype(np.float64) - 1.0, 0.0)
    ref_marg, ref_logz = _reference(L, "base", None)
    model = nat.Model.from_tables(w, moved)
    tag = f"{name} shift {c:+g}"
    end = _correct_or_refused(tag, lambda: model.marginals_full(*csr),
                              lambda got: _judge(tag, got[0], got[1], ref_marg, ref_logz + steps * c), must_answer=name == "L2-scan")
    if L > 2 and not (switches and switches[0][0] == CHUNKED):  # the queries run the same pass first: the same disjunction
        spans = list(_phase_spans(L))
        ref_edges, (ref_spans, bound) = _query_reference(L, "a", "under+")  # (a shift of the same base model: the same distribution)
        assert _correct_or_refused(f"{tag} edges", lambda: model.edge_posteriors(*csr, sets=np.array(_sets(L), dtype=np.uint32),
                                                                                want_pair=True, want_marginals=True),
                                   lambda out: ge._check(f"{tag} edges", out, ref_edges, csr[0], L, _sets(L))) == end
        assert _correct_or_refused(f"{tag} spans", lambda: model.span_log_probabilities(*csr, *gs._arrays(spans)),
                                   lambda logp: gs._check(f"{tag} spans", logp, ref_spans, bound, spans, L)) == end


@pytest.mark.parametrize("L", [2, 3, 17])
def test_outside_the_range_viterbi_decodes_and_the_windows_answer_or_refuse(nat, monkeypatch, L):
    """Viterbi reads the raw transition weights: no exp, no refusal, and the best path's score moves by (T - 1) c.  The any-L
    window kernels read exp(trans) and stand under the same disjunction as the whole-contig pass."""
    _switch(monkeypatch, ())
    w, trans = fam.base(L)
    csr = fam.batch(L)
    cptr, gptr, attr = csr
    steps = np.maximum(np.diff(cptr).astype(np.float64) - 1.0, 0.0)
    score = _score(L, False, fam.LENGTHS)
    _, base_sc = cr.viterbi(cptr, score, trans)
    W = 5
    ref_all, ref_any = cr.windowed(cptr, score, trans, W, 1, 0, True)
    for c in fam.SHIFTS_E:
        model = nat.Model.from_tables(w, fam.shifted(L, c)[0])
        y, sc = model.viterbi(*csr)
        bound = 1e-10 * np.maximum(1.0, np.abs(base_sc + steps * c))
        print(f"L={L} shift {c:+g}: Viterbi worst |score - (base + (T - 1) c)| / bound = {float((np.abs(sc - base_sc - steps * c) / bound).max()):.3g}")
        assert y.shape == (int(cptr[-1]),) and np.all((y >= 0) & (y < L)) and np.all(np.abs(sc - base_sc - steps * c) <= bound)

        def judge(got):
            p_all, p_any = got
            dm = max(float(np.abs(p_all - ref_all).max()), float(np.abs(p_any - ref_any).max()))
            print(f"L={L} shift {c:+g}: windowed worst |error| = {dm:.3g}")
            assert np.all(np.isfinite(p_all)) and np.all(np.isfinite(p_any)) and dm <= 1e-12

        if L > 2:
            _correct_or_refused(f"L={L} shift {c:+g} windowed", lambda: model.windowed_marginals_all(*csr, W, 1, 0, True), judge)
