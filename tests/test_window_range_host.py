"""The yardstick of tests/test_gpu_window_range.py on that file's own inputs, without a device.  Five things make a failure of
the device test the kernel's and not the reference's:

1. on windows small enough to enumerate (up to 3 labels and 4 items, with and without allowed-label sets, padded contigs
   included) ``window_range_reference.windowed`` is ``constrained_reference.enumerate_paths`` applied per window, for p_all and
   for p_any;
2. on every planted input of the device tests its float64 run agrees with its own ``np.longdouble`` run within 1e-13, a tenth of
   the device tolerance (where long double carries a 64-bit significand);
3. shift invariance: ``trans + c`` leaves every window marginal where it was, within 1e-13, for the shifts of family a;
4. the planted models have the figures the device tests rely on: the spreads stand on the side of ``spread (W - 1) < 600`` they
   claim, to the grid step, and the leaders lead by at least 800;
5. ``constrained_reference.windowed``, whose vectors are not shifted, misses this yardstick by more than 1e-12 on family d at
   W = 20: it cannot judge these inputs at the device tolerance, which is why the device tests do not use it."""
import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import lattice_range_families as fam
from tests import test_gpu_window_range as gw
from tests import train_objective_partial as tp
from tests import window_range_reference as wr

EXTENDED = np.finfo(np.longdouble).nmant >= 63


# ---------------------------------------------------------------- 1. path enumeration
def _enumerated(cptr, score, trans, W, step, background, pad):
    """constrained_reference.enumerate_paths per window, under windowed's contract."""
    n, L = score.shape
    p_all, p_any = np.zeros((n, L)), np.zeros(n)
    for b, e in zip(cptr[:-1].tolist(), cptr[1:].tolist()):
        m = e - b
        if m == 0:
            continue
        if m < W and not pad:
            p_all[b:e], p_any[b:e] = np.nan, np.nan
            continue
        front = (W - m) // 2 if m < W else 0
        X = np.zeros((max(m, W), L))
        X[front:front + m] = score[b:e]
        full, anyp = np.zeros_like(X), np.zeros(len(X))
        for s0 in range(0, len(X) - W + 1, step):
            marg = cr.enumerate_paths(X[s0:s0 + W], trans)[1]
            full[s0:s0 + W] = np.maximum(full[s0:s0 + W], marg)
            anyp[s0:s0 + W] = np.maximum(anyp[s0:s0 + W], np.delete(marg, background, axis=1).sum(axis=1))
        p_all[b:e], p_any[b:e] = full[front:front + m], anyp[front:front + m]
    return p_all, p_any


ENUMERATED = [("base", None), ("a", "at-"), ("b", 600.0), ("c", "row"), ("c", "column"), ("c", "diagonal"), ("d", 75.1),
              ("edge", "sticky", 4, 0, True), ("edge", "restless", 4, 1, False), ("edge", "column", 2, 0, True)]


@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("key", ENUMERATED, ids=[str(k) for k in ENUMERATED])
def test_the_yardstick_is_path_enumeration_per_window(key, masked):
    lengths = (0, 1, 2, 3, 4, 5, 9, 0)
    worst = 0.0
    for L in (2, 3):
        w, trans, leaders = fam.window_model(L, key)
        cptr, gptr, attr = fam.batch(L, lengths, leaders, whole=leaders)
        n = int(cptr[-1])
        allowed = tp.random_masks(np.random.default_rng(7700 + L), n, L) if masked else tp.full_masks(n, L)
        score = cr.masked_scores(gptr, attr, None, w, allowed)
        for W, step, pad in ((1, 1, True), (2, 1, True), (3, 2, True), (4, 1, True), (4, 3, False), (3, 1, False)):
            for bg in (0, L - 1):
                p_all, p_any = wr.windowed(cptr, score, trans, W, step, bg, pad)
                e_all, e_any = _enumerated(cptr, score, trans, W, step, bg, pad)
                assert np.array_equal(np.isnan(p_all), np.isnan(e_all)) and np.array_equal(np.isnan(p_any), np.isnan(e_any))
                ok = ~np.isnan(e_any)
                worst = max(worst, float(np.abs(p_all[ok] - e_all[ok]).max(initial=0.0)), float(np.abs(p_any[ok] - e_any[ok]).max(initial=0.0)))
                assert np.array_equal(wr.windowed(cptr, score, trans, W, step, None, pad)[0], p_all, equal_nan=True)
    print(f"{key} {'masked' if masked else 'free'}: worst |yardstick - enumeration| = {worst:.3g}")
    # (enumeration adds up path scores of up to 4 x 800, whose ulp is 4.5e-13: its weights carry that relative error under leaders)
    assert worst <= 1e-12


# ---------------------------------------------------------------- 2. the yardstick against its own extended-precision run
INPUTS = gw.planted_inputs()
INPUT_GROUPS = sorted({(L, W) for L, _, W, _, _, _ in INPUTS})


@pytest.mark.skipif(not EXTENDED, reason="long double carries no 64-bit significand here")
@pytest.mark.parametrize("L,W", INPUT_GROUPS, ids=[f"L{L}-W{W}" for L, W in INPUT_GROUPS])
def test_float64_is_within_a_tenth_of_the_device_tolerance_of_extended_precision(L, W):
    worst, where = 0.0, None
    for inp in INPUTS:
        if (inp[0], inp[2]) != (L, W):
            continue
        p_all, p_any = gw.compute_reference(*inp)
        x_all, x_any = gw.compute_reference(*inp, dtype=np.longdouble)
        assert p_all.dtype == np.float64 and x_all.dtype == np.longdouble
        err = 0.0
        for got, ext in [(p_all, x_all)] + [(p_any[bg], x_any[bg]) for bg in p_any]:
            assert np.array_equal(np.isnan(got), np.isnan(ext))
            ok = ~np.isnan(got)
            err = max(err, float(np.abs(got[ok] - ext[ok]).max(initial=0.0)))
        if err >= worst:
            worst, where = err, inp
        assert err <= 1e-13, (inp, err)
    print(f"L={L} W={W}: worst |float64 yardstick - long double yardstick| = {worst:.3g} at {where}")


# ---------------------------------------------------------------- 3. shift invariance
@pytest.mark.parametrize("L", (2, 3, 8, 17, 32))
def test_a_uniform_shift_leaves_every_window_marginal_where_it_was(L):
    W = 20
    score = gw.score_of(L, W, False, None)
    cptr = fam.window_batch(L, W)[0]
    base_all, base_any = wr.windowed(cptr, score, fam.base(L)[1], W, 1, 0, True)
    for which in fam.SHIFTS_A:
        moved, c = fam.shifted(L, which)
        p_all, p_any = wr.windowed(cptr, score, moved, W, 1, 0, True)
        d = max(float(np.abs(p_all - base_all).max()), float(np.abs(p_any - base_any).max()))
        print(f"L={L} shift {which} (c = {c!r}): worst |window marginal difference| = {d:.3g}")
        assert d <= 1e-13, which


# ---------------------------------------------------------------- 4. the planted figures
def test_the_guard_spreads_stand_where_they_claim():
    assert fam.guard_spread(2) == 600.0 - fam.GRID and fam.guard_spread(5) == 150.0 - fam.GRID
    for W in fam.WINDOWS + (21,):
        s = fam.guard_spread(W)
        assert s == np.round(s / fam.GRID) * fam.GRID and s * (W - 1) < 600.0 and not (s + fam.GRID) * (W - 1) < 600.0
        assert abs(s - 600.0 / (W - 1)) <= fam.GRID
    assert abs(fam.guard_spread(20) - 31.578947) < 1e-5 and abs(fam.guard_spread(32) - 19.354838) < 1e-5


@pytest.mark.parametrize("L", (2, 3, 4, 8, 9, 17, 32))
def test_the_spread_shapes_and_the_leaders_are_what_the_device_tests_rely_on(L):
    _, trans = fam.base(L)
    hi = trans.max()
    diag, off = np.eye(L, dtype=bool), ~np.eye(L, dtype=bool)
    for W in fam.WINDOWS:
        for side in (0, 1):
            s = fam.guard_spread(W) + side * fam.GRID
            for shape in fam.SPREAD_SHAPES:
                out = fam.spread_model(L, shape, s)
                assert out.max() == hi and out.min() == hi - s and out.max() - out.min() == s
                assert np.array_equal(np.round(out / fam.GRID) * fam.GRID, out), "on the grid"
                assert ((out.max() - out.min()) * float(W - 1) < 600.0) == (side == 0)
                assert fam.small_tier_ok(L, W, out) == (side == 0 and (W <= 20 or L <= 4 or L > 8))
                assert fam.small_tier_ok(L, W, out, True) == (side == 0 and L <= 8 and (W <= 20 or L <= 4))
                low = out == hi - s
                if shape == "one":
                    assert low.sum() == 1 and low[fam.far_cell(L)] and np.array_equal(out[~low], trans[~low])
                elif shape == "sticky":
                    assert np.all(out[diag] == hi) and np.all(low[off])
                elif shape == "restless":
                    assert np.all(low[diag]) and (L == 2 or low.sum() == L)
                else:
                    assert np.all(low[:, 0]) and low.sum() == L
    # the leaders: one on every item of every contig, alternating from the contig's first item, leading by at least 800
    for W in fam.WINDOWS:
        assert fam.window_lengths(W) == (0, 1, W - 1, W, W + 1, 2 * W + 3, 65, 300, 0)
        csr = fam.window_batch(L, W, True)
        lead = fam.leader_of(csr)
        assert np.all(fam.leader_of(fam.window_batch(L, W)) == -1)
        want = np.concatenate([np.arange(m) % 2 for m in fam.window_lengths(W)])
        assert np.array_equal(lead, want)
        score = gw.score_of(L, W, True, None)
        top = score[np.arange(len(lead)), lead]
        rest = np.where(np.arange(L)[None, :] == lead[:, None], -np.inf, score).max(axis=1)
        assert np.all(top - rest >= 800.0)
        forbid = fam.forbid_the_leader(L, csr)
        assert np.all((forbid >> lead.astype(np.uint32)) & 1 == 0) and np.all(forbid | (1 << lead.astype(np.uint32)) == (1 << L) - 1)
        assert np.all(forbid != 0)


# ---------------------------------------------------------------- 5. the unshifted yardstick cannot judge these inputs
def test_the_unshifted_window_reference_misses_the_device_tolerance_under_leaders():
    """Family d at W = 20: ``constrained_reference.windowed`` forms la + lb - lz from numbers near 20 x 800 and misses this
    yardstick by more than the device tolerance; where long double carries a 64-bit significand, that run says which of the
    two is off.  Do not swap the yardsticks back."""
    for L in (3, 8, 17, 32):
        key, W = ("d", fam.LEADERS_D[1]), 20
        _, trans, leaders = fam.window_model(L, key)
        cptr, score = fam.window_batch(L, W, leaders)[0], gw.score_of(L, W, leaders, None)
        old_all, _ = cr.windowed(cptr, score, trans, W, 1, 0, True)
        new_all, _ = wr.windowed(cptr, score, trans, W, 1, 0, True)
        gap = float(np.abs(old_all - new_all).max())
        print(f"L={L}: |constrained_reference.windowed - window_range_reference.windowed| = {gap:.3g}")
        assert gap > 1e-12
        if EXTENDED:
            x_all, _ = wr.windowed(cptr, score, trans, W, 1, 0, True, dtype=np.longdouble)
            off_old, off_new = float(np.abs(old_all - x_all).max()), float(np.abs(new_all - x_all).max())
            print(f"L={L}: against long double: constrained_reference.windowed {off_old:.3g}, window_range_reference.windowed {off_new:.3g}")
            assert off_old > 1e-12 and off_new <= 1e-13
