"""What tests/test_gpu_query_range.py rests on, shown without a device: the planted figures of the query families
(tests/lattice_range_families.py), the conditions of the floor rule on the yardsticks (tests/query_range_reference.py), the
yardsticks against path enumeration in log space on these very models, and the claim that a uniform shift of the transitions
leaves every yardstick value where it was."""
import itertools

import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import edges_reference as er
from tests import lattice_range_families as fam
from tests import query_range_reference as qr
from tests import runs_reference as rr
from tests import sampling_reference as sr

LOG_QUERIES = ("spans", "runs", "conditionals")
ENUM_LENGTHS = (1, 2, 3, 4, 6, 7)  # (7: the shortest contig that carries family m's leader)
ALL_MODELS = [(f, k) for f in sorted(fam.QUERY_FAMILIES) for k in fam.QUERY_FAMILIES[f]]


def _entries(L, family, key, query):
    """Every log-valued yardstick entry of one query on one model, flat, with its bound."""
    if query == "runs":
        (val, bnd), (rval, rbnd) = qr.runs_reference(L, family, key)
        return (np.concatenate([val[k].ravel() for k in qr.KEYS] + [rval]), np.concatenate([bnd[k].ravel() for k in qr.KEYS] + [rbnd]))
    return qr.span_reference(L, family, key)  # (the conditionals' logp are the spans' on the same list)


# ---------------------------------------------------------------- 1. the planted figures
@pytest.mark.parametrize("L", fam.QUERY_LABELS)
def test_planted_figures(L):
    w, trans = fam.base(L)
    spread = float(trans.max() - trans.min())
    assert 3.5 <= spread <= 7.03, "the base spreads are 3.5 to 7.02"
    for key, side in zip(fam.GUARD_G, (700.0, -700.0)):
        moved, c = fam.shift_any(L, key)
        assert float(moved.max()) == side and fam.figures(moved)["in_range"], "family g: max trans at the guard's own figure, accepted"
        assert np.array_equal(moved - c, trans)
    for key, side in zip(fam.BEYOND_G, (700.0, -700.0)):
        moved, _ = fam.shift_any(L, key)
        assert abs(float(moved.max()) - side) == fam.GRID and abs(float(moved.max())) > 700.0 and not fam.figures(moved)["in_range"]
    low = np.exp(fam.shift_any(L, "at-700")[0])
    assert low.min() >= np.finfo(np.float64).tiny, "at -700 every exp(trans) is still a normal double"
    if L == 32:
        assert 8.8e-308 < low.min() < 8.9e-308
    assert np.isfinite(np.exp(fam.shift_any(L, "at+700")[0]) * L).all()
    # no planted matrix holds an entry whose exp is subnormal and not zero; exp_zero marks exactly the -2000 entries
    for family, key in ALL_MODELS:
        _, t, _ = fam.query_model(L, family, key)
        e = np.exp(t)
        assert np.all((e == 0.0) | (e >= np.finfo(np.float64).tiny)), (family, key)
        assert np.array_equal(np.isneginf(fam.exp_zero(t)), t <= -1500.0) and np.array_equal(fam.exp_zero(t)[t > -1500.0], t[t > -1500.0])
        assert fam.figures(t)["in_range"]
    assert any((fam.query_model(L, "c", k)[1] <= -1500.0).any() for k in fam.FORBID_C) and (fam.query_model(L, "b", 2000.0)[1] <= -1500).sum() == 1
    # the leads
    for leaders, lead in (("m", fam.MID_LEAD), ("d", 800.0)):
        score = qr.scores(L, leaders)
        csr = fam.query_batch(L, leaders)
        marked = fam.leader_of(csr)
        assert (marked >= 0).sum() > 0
        for g in np.flatnonzero(marked >= 0):
            assert score[g, marked[g]] - np.delete(score[g], marked[g]).max() >= lead, (leaders, g)
        plain = qr.scores(L, None)
        assert np.array_equal(score[marked < 0], plain[marked < 0]), "no other item is touched"
    # the side of run_posteriors' own range every model stands on: the far shifts are refused, max|trans| = 150 is taken
    taken = {(f, k) for f, k in ALL_MODELS if fam.runs_in_range(fam.query_model(L, f, k)[1])}
    assert {(f, k) for f, k in ALL_MODELS} - taken == {("a", "+600"), ("a", "-600"), ("g", "at+700"), ("g", "at-700"), ("d'", "+600"), ("d'", "-600"),
                                                        ("m", "+600"), ("m", "-600"), ("m", "at+700"), ("m", "at-700")}
    assert np.abs(fam.query_model(L, "m", "at+")[1]).max() == 150.0 and np.abs(fam.query_model(L, "m", "at-")[1]).max() == 150.0
    cptr = fam.query_batch(L, "m")[0]
    marked = fam.leader_of(fam.query_batch(L, "m"))
    for c, T in enumerate(fam.QUERY_LENGTHS):
        mine = np.flatnonzero(marked[int(cptr[c]):int(cptr[c + 1])] >= 0)
        assert mine.tolist() == ([T // 2] if T >= 7 else []) and (T < 7 or 0 < T // 2 < T - 1), "one interior item of every contig of 7 or more"


# ---------------------------------------------------------------- 2. the conditions of the floor rule
@pytest.mark.parametrize("query", LOG_QUERIES)
@pytest.mark.parametrize("L", fam.QUERY_LABELS)
def test_the_floor_rule_has_what_it_needs(L, query):
    """Conditions, not measurements: the gap [-790, -700) is empty in every yardstick; under d' at least 100 ordinary finite and
    100 deep entries; under every family-c model at least 20 entries that are -inf only because of the forbidden transition;
    under m, a, b, g (and c) every finite entry is ordinary, so nothing there can hide behind the disjunction."""
    plain, _ = _entries(L, "a", "base", query)
    for family, key in sorted({qr.canon(f, k) for f, k in ALL_MODELS}, key=str):
        ref, bound = _entries(L, family, key, query)
        ordinary, deep = qr.classes(ref)  # (asserts the empty gap)
        fin = np.isfinite(ref)
        n_ord, n_deep = int((ordinary & fin).sum()), int(deep.sum())
        print(f"L={L} {query} family {family} {key}: {n_ord} ordinary finite, {n_deep} deep, {int(np.isneginf(ref).sum())} -inf")
        assert np.all(bound > 0.0)
        if family == "d'":
            assert n_ord >= 100 and n_deep >= 100
        else:
            assert n_deep == 0 and n_ord >= 50  # (every finite entry is ordinary, and there are enough of them to judge)
        if family == "c":
            only = int((np.isneginf(ref) & np.isfinite(plain)).sum())
            print(f"    {only} entries are -inf only because of the forbidden transition")
            assert only >= 20
        if family in ("a", "m") or (family == "b" and key < 2000.0):
            assert np.array_equal(np.isneginf(ref), np.isneginf(plain))


# ---------------------------------------------------------------- 3. the yardsticks against enumeration in log space
def _lse(v):
    return rr._lse(np.asarray(v, dtype=np.float64))


def _paths(X, trans):
    """Every path of one short sequence and its score in log space, -inf where a transition or a pair does not exist."""
    T, L = X.shape
    P = np.array(list(itertools.product(range(L), repeat=T)), dtype=np.int64)
    s = X[0, P[:, 0]].copy()
    for t in range(1, T):
        s = s + trans[P[:, t - 1], P[:, t]] + X[t, P[:, t]]
    return P, s


def _extents(inside):
    """Per path and item the first and last item of the maximal run of `inside` through it (garbage where not inside)."""
    N, T = inside.shape
    left, right = np.zeros((N, T), dtype=np.int64), np.zeros((N, T), dtype=np.int64)
    for t in range(T):
        left[:, t] = np.where(inside[:, t], (left[:, t - 1] if t else 0) + 1, 0)
    for t in range(T - 1, -1, -1):
        right[:, t] = np.where(inside[:, t], (right[:, t + 1] if t < T - 1 else 0) + 1, 0)
    at = np.arange(T)[None, :]
    return at - left + 1, at + right - 1


def _close(tag, got, want, logz=0.0):
    """Within 1e-12 (of the value, where it is large), with equal -inf patterns.  Both sides are differences of two log Z: at
    shifts of 600 and leads of 800 per item those are of the order of 10^4, and one unit in their last place is 1.8e-12 -- so
    eight units of `logz` are allowed on top, which is nothing at ordinary weights."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and not np.isnan(got).any() and not np.isnan(want).any(), tag
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), f"{tag}: the -inf patterns differ"
    fin = np.isfinite(want)
    tol = 1e-12 * np.maximum(1.0, np.abs(want[fin])) + 8.0 * np.finfo(np.float64).eps * abs(logz)
    worst = float((np.abs(got[fin] - want[fin]) / tol).max(initial=0.0))
    assert worst <= 1.0, f"{tag}: {worst:.3g} of the tolerance"
    return worst


@pytest.mark.parametrize("family,key", ALL_MODELS, ids=[f"{f}-{k}" for f, k in ALL_MODELS])
@pytest.mark.parametrize("L", [2, 3])
def test_the_yardsticks_are_enumerations(L, family, key):
    w, raw, leaders = fam.query_model(L, family, key)
    tz = fam.exp_zero(raw)
    csr = fam.query_batch(L, leaders, ENUM_LENGTHS)
    cptr = csr[0]
    score = qr.scores(L, leaders, ENUM_LENGTHS)
    sets = qr.label_sets(L) + [(1 << L) - 1]
    worst = 0.0
    edges = er.edge_posteriors(cptr, score, raw, qr.edge_sets(L))
    marg, logz_all = cr.marginals(cptr, score, raw)
    yard = qr.Regions(csr, w, score, tz, raw)
    la = sr.log_forward(cptr, score, raw)
    for c, T in enumerate(ENUM_LENGTHS):
        g0 = int(cptr[c])
        X = score[g0:g0 + T]
        P, s = _paths(X, tz)
        logz = _lse(s)
        assert np.isfinite(logz)
        worst = max(worst, _close("log Z", [qr.log_z(X, tz), logz_all[c]], [logz, logz], logz))
        tol = 1e-12 + 8.0 * np.finfo(np.float64).eps * abs(logz)  # (a probability from enumeration is exp of a difference of logs of that size)
        # the probability-valued yardsticks, formed on the raw matrix, against enumeration on exp_zero
        xi, H, _ = er.enumerate_edges(X, tz, qr.edge_sets(L))
        assert np.abs(edges["pair"][g0:g0 + T] - xi).max() <= tol and abs(edges["entropy"][c] - H) <= 1e-12 * max(1.0, T)
        m_enum = np.array([[np.exp(_lse(s[P[:, t] == l]) - logz) for l in range(L)] for t in range(T)])
        assert np.abs(marg[g0:g0 + T] - m_enum).max() <= tol
        for nxt in np.flatnonzero(np.isfinite(tz).any(axis=0)):  # the sampler's weights: a term of e^-2000 is an exact 0.0
            pick = np.full((T, 1), nxt)
            last = np.zeros(T, dtype=bool)
            assert np.array_equal(sr._weights(la[g0:g0 + T], raw, pick, last), sr._weights(la[g0:g0 + T], tz, pick, last))
        for mask in sets:
            inside = rr.inside_of(mask, L)[P]
            first, final = _extents(inside)
            # spans and regions
            spans = [(c, b, e, mask) for b in range(T) for e in range(b + 1, T + 1)]
            want = [_lse(s[inside[:, b:e].all(axis=1)]) - logz for _, b, e, _ in spans]
            worst = max(worst, _close("spans", qr.span_yardstick(cptr, score, tz, spans)[0], want, logz))
            for (_, b, e, _), lp in list(zip(spans, want))[::3]:
                cond, logze, lz = yard.region(c, b, e, mask)
                worst = max(worst, _close("region logp", [logze - lz], [lp], logz))
                keep = inside[:, b:e].all(axis=1)
                if np.isfinite(lp):
                    c_enum = np.array([[np.exp(_lse(s[keep & (P[:, t] == l)]) - (lp + logz)) for l in range(L)] for t in range(T)])
                    assert np.abs(cond - c_enum).max() <= tol and np.all(cond[np.isneginf(qr.restricted(X, b, e, mask))] == 0.0)
                    t = (b + e) // 2  # the item's knock-out, scored again by enumeration
                    X2 = X.copy()
                    X2[t] = 0.0
                    P2, s2 = _paths(X2, tz)
                    want_ko = lp - (_lse(s2[keep]) - _lse(s2))
                    got_ko, bound = yard.knock_out(c, b, e, mask, t)
                    assert abs(got_ko - want_ko) <= tol * max(1.0, abs(want_ko), abs(lp)) and bound > 0.0
                else:
                    assert not cond.any()
            if mask == (1 << L) - 1:
                continue
            # anchors at a reach inside the contig and beyond it, and closed runs
            anchors = [(c, a, mask) for a in range(T)]
            for reach in (1, T):
                val, _ = qr.anchor_yardstick(cptr, score, tz, anchors, reach)
                for a in range(T):
                    on = inside[:, a]
                    worst = max(worst, _close("anchor", [val["log_anchor"][a]], [_lse(s[on]) - logz], logz))
                    starts = [_lse(s[on & (first[:, a] == a - r)]) - logz if a - r >= 0 else -np.inf for r in range(reach + 1)]
                    ends = [_lse(s[on & (final[:, a] == a + r)]) - logz if a + r < T else -np.inf for r in range(reach + 1)]
                    worst = max(worst, _close("starts", val["log_start"][a], starts, logz), _close("ends", val["log_end"][a], ends, logz))
                    worst = max(worst, _close("beyond", [val["log_start_beyond"][a], val["log_end_beyond"][a]],
                                              [_lse(s[on & (first[:, a] < a - reach)]) - logz, _lse(s[on & (final[:, a] > a + reach)]) - logz], logz))
            runs = [(c, b, e, mask) for b in range(T) for e in range(b + 1, T + 1)]
            want = [_lse(s[inside[:, b] & (first[:, b] == b) & (final[:, b] == e - 1)]) - logz for _, b, e, _ in runs]
            worst = max(worst, _close("closed runs", qr.run_yardstick(cptr, score, tz, runs)[0], want, logz))
    print(f"L={L} family {family} {key}: worst |yardstick - enumeration| / tolerance = {worst:.3g}")


# ---------------------------------------------------------------- 4. a uniform shift leaves every yardstick value where it was
@pytest.mark.parametrize("L", fam.QUERY_LABELS)
def test_a_uniform_shift_moves_no_yardstick_value(L):
    """trans + c is the unshifted model's distribution exactly (the families' grid): the shifted model's own yardstick agrees with
    the one tests/test_gpu_query_range.py judges it by within twice the query's bound, with equal -inf patterns."""
    shifted = [(f, k) for f, k in ALL_MODELS if qr.canon(f, k) != (f, k)]
    assert len(shifted) == 6 + 2 + 2 + 6
    for family, key in shifted:
        dist = qr.canon(family, key)
        assert fam.query_shift(L, family, key) != 0.0
        worst = 0.0
        for query in ("spans", "runs"):
            mine, _ = _entries(L, family, key, query)
            ref, bound = _entries(L, *dist, query)
            assert np.array_equal(np.isneginf(mine), np.isneginf(ref)), (family, key, query)
            fin = np.isfinite(ref)
            worst = max(worst, float((np.abs(mine[fin] - ref[fin]) / (2.0 * bound[fin])).max()))
        a, b = qr.regions(L, family, key), qr.regions(L, *dist)
        for c, lo, hi, m in qr.spans(L)[::8]:
            ca, cb = a.region(c, lo, hi, m)[0], b.region(c, lo, hi, m)[0]
            worst = max(worst, float(np.abs(ca - cb).max()) / 2e-12)
        ma, mb = qr.marginal_reference(L, family, key)[0], qr.marginal_reference(L, *dist)[0]
        worst = max(worst, float(np.abs(ma - mb).max()) / 2e-12)
        ea, eb = qr.edge_reference(L, family, key), qr.edge_reference(L, *dist)
        worst = max(worst, float(np.abs(ea["pair"] - eb["pair"]).max()) / 2e-12)
        print(f"L={L} family {family} {key}: worst |own yardstick - the unshifted model's| / twice the bound = {worst:.3g}")
        assert worst <= 1.0
