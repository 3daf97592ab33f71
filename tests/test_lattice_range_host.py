"""The yardstick of tests/test_gpu_lattice_range.py on that file's own inputs, without a device: the log-space references
(tests/constrained_reference.py, tests/edges_reference.py) on the planted transition families of
tests/lattice_range_families.py.  Three things make a failure of the device test the kernel's and not the reference's:

1. shift invariance: ``trans + c`` describes the distribution of ``trans`` -- the yardstick's marginals agree to 1e-13 and its
   log Z differs by (T - 1) c to 1e-10 max(1, |log Z|), for every uniform shift the device tests use (up to +-800);
2. on every planted family at 3 labels and contigs of 1 to 6 items the yardstick is path enumeration's: marginals and pair
   marginals to 1e-12 (enumeration adds up path scores of up to 6 x 800, whose ulp is 9e-13: its own weights carry a relative
   error of that order at the largest shifts, and 1e-16 elsewhere), log Z to 1e-10 max(1, |log Z|);
3. the planted models have the figures the device tests rely on: both sides of ``4 max|trans| < 600`` (rows_rescale_period),
   both sides of ``8 (max - min) < 600`` (raw_fold), and both sides of -700 <= max trans <= 700 (the any-L route's range)."""
import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import edges_reference as er
from tests import lattice_range_families as fam
from tests import train_objective_partial as tp


def _scores(L, w, csr):
    cptr, gptr, attr = csr
    return cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L))


# ---------------------------------------------------------------- 1. shift invariance
@pytest.mark.parametrize("L", fam.LABELS)
def test_a_uniform_shift_leaves_the_yardstick_where_it_was(L):
    w, trans = fam.base(L)
    csr = fam.batch(L)
    cptr = csr[0]
    T = np.diff(cptr).astype(np.float64)
    score = _scores(L, w, csr)
    marg0, logz0 = cr.marginals(cptr, score, trans)
    assert np.all(np.isfinite(marg0)) and np.abs(marg0.sum(axis=1) - 1.0).max() <= 1e-13
    for which in fam.SHIFTS_A + fam.SHIFTS_E:
        moved, c = fam.shifted(L, which)
        marg, logz = cr.marginals(cptr, score, moved)
        want = logz0 + np.maximum(T - 1.0, 0.0) * c
        dm = float(np.abs(marg - marg0).max())
        dz = float((np.abs(logz - want) / (1e-10 * np.maximum(1.0, np.abs(want)))).max())
        print(f"L={L} shift {which} (c = {c!r}): worst |marginal difference| = {dm:.3g}, worst |log Z difference| / bound = {dz:.3g}")
        assert np.all(np.isfinite(marg)) and np.all(np.isfinite(logz))
        assert dm <= 1e-13 and dz <= 1.0, which


# ---------------------------------------------------------------- 2. path enumeration
def _planted():
    return ([("a", k) for k in fam.SHIFTS_A] + [("b", s) for s in fam.FAR_B] + [("c", k) for k in fam.FORBID_C] +
            [("d", s) for s in fam.LEADERS_D] + [("e", c) for c in fam.SHIFTS_E])


@pytest.mark.parametrize("family,key", _planted(), ids=[f"{f}-{k}" for f, k in _planted()])
def test_the_yardstick_is_path_enumeration_on_every_family(family, key):
    L, lengths = 3, (1, 2, 3, 4, 5, 6)
    w, trans, leaders = fam.model_of(L, family, key)
    csr = fam.batch(L, lengths, leaders)
    cptr = csr[0]
    score = _scores(L, w, csr)
    sets = (0b011, 0b100)
    marg, logz = cr.marginals(cptr, score, trans)
    edges = er.edge_posteriors(cptr, score, trans, sets)
    assert np.abs(edges["marg"] - marg).max() <= 1e-13, "the two references agree on the marginals"
    worst = [0.0, 0.0, 0.0]
    for s, (g0, g1) in enumerate(zip(cptr[:-1].tolist(), cptr[1:].tolist())):
        X = score[g0:g1]
        elogz, emarg, _, _ = cr.enumerate_paths(X, trans)
        exi, eH, _ = er.enumerate_edges(X, trans, sets)
        worst[0] = max(worst[0], float(np.abs(marg[g0:g1] - emarg).max()))
        worst[1] = max(worst[1], abs(logz[s] - elogz) / (1e-10 * max(1.0, abs(elogz))))
        worst[2] = max(worst[2], float(np.abs(edges["pair"][g0:g1] - exi).max()))
        assert abs(edges["entropy"][s] - eH) <= 1e-12 * (g1 - g0)
        if family == "c":  # the pairs that no path goes through: exact zeros in both
            dead = fam.forbidden(L, key)[1](g1 - g0)
            assert np.all(emarg[dead] == 0.0) and np.all(marg[g0:g1][dead] == 0.0)
    print(f"{family} {key}: worst |marginal - enumeration| = {worst[0]:.3g}, |log Z - enumeration| / bound = {worst[1]:.3g}, "
          f"|pair marginal - enumeration| = {worst[2]:.3g}")
    assert worst[0] <= 1e-12 and worst[1] <= 1.0 and worst[2] <= 1e-12
    if family == "d":  # the leaders lead: every item of these contigs has a label at 1 to rounding
        assert np.all(marg.max(axis=1) >= 1.0 - 1e-12)
        assert np.all(np.sort(score, axis=1)[:, -1] - np.sort(score, axis=1)[:, -2] >= 800.0)


# ---------------------------------------------------------------- 3. the planted figures
@pytest.mark.parametrize("L", fam.LABELS)
def test_the_planted_models_stand_on_both_sides_of_every_guard(L):
    _, trans = fam.base(L)
    assert np.array_equal(np.round(trans / fam.GRID) * fam.GRID, trans) and np.abs(trans).max() < 6.0
    fig = fam.figures(trans)
    assert 4 * np.abs(trans).max() < 600 and fig["period"] == 4 and fig["raw_fold"] == 1 and fig["in_range"]
    # family a: max|trans| one grid step under 150 and at 150, on both signs; then 600
    for sign, under, at in ((1.0, "under+", "at+"), (-1.0, "under-", "at-")):
        lo, hi = fam.shifted(L, under)[0], fam.shifted(L, at)[0]
        assert np.abs(lo).max() == 150.0 - fam.GRID and 4 * np.abs(lo).max() < 600 and fam.figures(lo)["period"] == 4
        assert np.abs(hi).max() == 150.0 and 4 * np.abs(hi).max() >= 600 and fam.figures(hi)["period"] == 1
        edge = lo.max() if sign > 0 else lo.min()
        assert abs(edge) == np.abs(lo).max() and np.sign(edge) == sign  # (the planted sign holds the maximum)
        assert fam.figures(lo)["raw_fold"] == 1 and fam.figures(hi)["raw_fold"] == 1  # (a shift leaves the spread alone)
    for which in ("+600", "-600"):
        far = fam.shifted(L, which)[0]
        assert 594.0 < np.abs(far).max() < 606.0 and fam.figures(far)["period"] == 1 and fam.figures(far)["in_range"]
    # family b: the spread is s; 74.9 and 75.1 stand on the two sides of raw_fold, and max|trans| = s - max trans
    for s in fam.FAR_B:
        far = fam.far_entry(L, s)
        i, j = fam.far_cell(L)
        assert i != j and far.max() == trans.max() and far.min() == far[i, j] and (far != trans).sum() == 1
        assert abs((far.max() - far.min()) - s) <= 1e-12 and abs(np.abs(far).max() - (s - trans.max())) <= 1e-12
        assert fam.figures(far)["in_range"]
    assert 8 * fam.figures(fam.far_entry(L, 74.9))["spread"] < 600 and fam.figures(fam.far_entry(L, 74.9))["raw_fold"] == 1
    assert 8 * fam.figures(fam.far_entry(L, 75.1))["spread"] >= 600 and fam.figures(fam.far_entry(L, 75.1))["raw_fold"] == 0
    for s in (74.9, 75.1, 149.0):
        assert 4 * np.abs(fam.far_entry(L, s)).max() < 600 and fam.figures(fam.far_entry(L, s))["period"] == 4
    for s in (600.0, 2000.0):
        assert 4 * np.abs(fam.far_entry(L, s)).max() >= 600 and fam.figures(fam.far_entry(L, s))["period"] == 1
    # (s = 151 puts max|trans| at 151 - max trans: under 150 where the base maximum is above 1.  Family a is what brackets 150.)
    assert fam.figures(fam.far_entry(L, 151.0))["period"] == (4 if trans.max() > 1.0 else 1)
    # family c: -2000 where it is planted and nowhere else; exp(-2000) is an exact 0; period 1, raw_fold 0
    for what in fam.FORBID_C:
        hard, dead = fam.forbidden(L, what)
        under = fam.shifted(L, "under-")[0] if what == "row-150" else trans  # ("row-150": the row in the shifted matrix)
        assert (hard == fam.FORBIDDEN).sum() == L and np.exp(fam.FORBIDDEN) == 0.0 and np.array_equal(hard[hard != fam.FORBIDDEN], under[hard != fam.FORBIDDEN])
        assert what != "row-150" or hard[hard != fam.FORBIDDEN].max() < -140.0
        assert fam.figures(hard)["period"] == 1 and fam.figures(hard)["raw_fold"] == 0 and fam.figures(hard)["in_range"]
        assert dead(1).sum() == 0 and dead(5).sum() == (0 if what == "diagonal" else 4)
    # family d: runs of at least 16 alternating leaders on every contig that has 16 items
    for T in fam.LENGTHS:
        runs = fam.leader_runs(T)
        assert all(0 <= b < e <= T for b, e in runs) or T == 0
        assert T < 16 or all(e - b >= 16 for b, e in runs)
    cptr, gptr, attr = fam.batch(L, fam.LENGTHS, True)
    lead = np.array([[(attr[gptr[g]:gptr[g + 1]] == a).any() for a in (fam.LEAD0, fam.LEAD1)] for g in range(int(cptr[-1]))])
    assert not np.any(lead.all(axis=1))
    g0 = int(cptr[fam.LENGTHS.index(300)])
    for b, e in fam.leader_runs(300):
        assert np.array_equal(lead[g0 + b:g0 + e, 0], np.arange(e - b) % 2 == 0) and np.array_equal(lead[g0 + b:g0 + e, 1], np.arange(e - b) % 2 == 1)
    assert not np.any(fam.batch(L)[2] >= fam.LEAD0), "no leader attribute outside family d"
    for s, fold in ((74.9, 1), (75.1, 0)):
        assert fam.figures(fam.model_of(L, "d", s)[1])["raw_fold"] == fold
    # family e: the largest weight outside [-700, 700], every weight finite
    for c in fam.SHIFTS_E:
        out = fam.shifted(L, c)[0]
        assert np.all(np.isfinite(out)) and not fam.figures(out)["in_range"] and (out.max() > 700 if c > 0 else out.max() < -700)
        with np.errstate(over="ignore", under="ignore"):
            assert np.all(np.isinf(np.exp(out))) if c > 0 else np.all(np.exp(out) == 0.0)
    # the contig lengths straddle the chunks (32, 64), the lane fold and the wave's staging (8) and the period-4 phase
    assert {0, 1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129, 300} == set(fam.LENGTHS) and fam.LONG_LENGTHS[0] > 2048
