"""The window kernels at their range guard, and beyond it: ``windowed_marginals`` and ``windowed_marginals_all`` through every
window tier (csrc/crf_general_windowed.hip: the un-normalised ``gl_windowed_small`` / ``gl_all_small`` and ``gl_windowed_mfma``, the
scaled lane-group ``gl_windowed`` / ``gl_all_groups``; csrc/crf_kernels.hip: the 2-label kernels) on the planted transition
families of tests/lattice_range_families.py, against the conditioned yardstick of tests/window_range_reference.py, which
tests/test_window_range_host.py pins on path enumeration and on its own extended-precision run on these very inputs.

The guard reads the transition weights alone (``gen_small_ok``): the un-normalised tiers run while
``(max trans - min trans) (W - 1) < 600``.  Every spread shape stands at ``guard_spread(W)``, the last grid value inside, and one
grid step beyond, for W = 2, 5, 20 and 32: the first is the un-normalised tier's worst admitted model (Z of a window near e^-600
where nearly every path pays the spread per step), the second falls to the lane-group tier, which reads the raw exp(trans).
Every arrangement is forced by its switch and confirmed through the plan's kernel name before anything is compared.

Every case asserts: no infinity, the yardstick's NaN pattern (skipped contigs), every value in [0, 1] -- exactly 1 at most, for
p, p_all and p_any -- and |p - yardstick| <= 1e-12, the tolerance tests/test_gpu_general.py, tests/test_gpu_windowed_all.py and
tests/test_gpu_windowed.py hold these kernels to at ordinary weights.  Rows of p_all are maxima over windows and need not sum to
1.  The yardstick of a (label count, model, W, step, pad, masks) is computed once and shared by the arrangements of that label
count.  Every case prints its worst |error| and worst error / tolerance per model, and runs every model before it fails."""
import functools

import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import lattice_range_families as fam
from tests import train_objective_partial as tp
from tests import window_range_reference as wr

pytestmark = pytest.mark.gpu

TOL = 1e-12
GROUPS, FORCE, GENERIC = "GECCO_CRF_GENERAL_GROUPS", "GECCO_CRF_FORCE_GENERAL", "GECCO_CRF_FORCE_GENERIC"
# (id, labels, the switches, the un-normalised tier's name or None, the name of the kernel that takes everything else)
SINGLE = ([(f"L{L}-small", L, (), "gl_windowed_small", "gl_windowed") for L in (3, 4, 8)] +
          [(f"L{L}-mfma", L, (), "gl_windowed_mfma", "gl_windowed") for L in (9, 17, 32)] +
          [(f"L{L}-groups", L, ((GROUPS, "1"),), None, "gl_windowed") for L in (3, 4, 8, 9, 17, 32)])
# the 2-label kernels ("crf_windowed_": the register-resident kernel or, where its own guard turns the model away, the generic
# one); the forced any-label route runs a 2-label model's single-label call on the lane-group tier (crf_plan.cpp: the
# lane-per-window tier from 3 labels; its 2-label form is the all-label call's, L2-all-small below)
TWO = [("L2-fast", 2, (), None, "crf_windowed_"), ("L2-generic", 2, ((GENERIC, "1"),), None, "crf_windowed_generic_l2"),
       ("L2-general", 2, ((FORCE, "1"),), None, "gl_windowed"), ("L2-general-groups", 2, ((FORCE, "1"), (GROUPS, "1")), None, "gl_windowed")]
ALL = ([(f"L{L}-all-small", L, (), "gl_all_small", "gl_all_groups") for L in (2, 3, 4, 8)] +
       [(f"L{L}-all-groups", L, ((GROUPS, "1"),), None, "gl_all_groups") for L in (3, 8, 9, 17, 32)])
BEYOND = {"a": fam.SHIFTS_A, "b": (149.0, 151.0, 600.0, 2000.0), "c": fam.FORBID_C, "d": fam.LEADERS_D}
GEOMETRY = ((20, 1, False), (20, 7, True), (5, 4, False))
MASK_LABELS, MASK_KINDS = (2, 3, 17), ("random", "leader")


def single_windows(L):
    """The guard-edge windows of the single-label call: 32 items where the un-normalised tier takes them."""
    return (2, 5, 20) + ((32,) if L <= 4 or L >= 9 else ())


def all_windows(L):
    return (2, 5, 20) + ((32,) if L <= 4 else ())


def edge_keys(W, shapes=fam.SPREAD_SHAPES, leaders=(False, True)):
    return [("edge", shape, W, side, lead) for shape in shapes for side in (0, 1) for lead in leaders]


def beyond_keys(family):
    return [(family, key) for key in BEYOND[family]]


def mask_keys(W):
    return [("edge", "sticky", W, 0, True), ("d", fam.LEADERS_D[1])]


def queried(L):
    return tuple(range(L)) if L <= 4 else (0, L // 2, L - 1)


def is_all(arrangement):
    return arrangement[4].startswith("gl_all")


def planted_inputs():
    """Every (labels, model key, W, step, pad, masks) the cases below run, for tests/test_window_range_host.py."""
    out = []
    for arr in SINGLE + TWO + ALL:
        L = arr[1]
        for W in (all_windows(L) if is_all(arr) else single_windows(L)):
            out += [(L, key, W, 1, True, None) for key in edge_keys(W)]
        for W in (5, 20):
            if arr[3] is None and arr[4].startswith("gl_"):
                out += [(L, key, W, 1, True, None) for family in sorted(BEYOND) for key in beyond_keys(family)]
        for W, step, pad in GEOMETRY:
            out += [(L, key, W, step, pad, None) for key in edge_keys(W, ("sticky",), (False,))]
    out += [(8, key, 21, 1, True, None) for key in edge_keys(21, ("sticky",))]
    for L in MASK_LABELS:
        out += [(L, key, W, 1, True, kind) for W in (5, 20) for key in mask_keys(W) for kind in MASK_KINDS]
    return sorted(set(out), key=repr)


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


def _switch(monkeypatch, switches):
    for name in (GROUPS, FORCE, GENERIC):
        monkeypatch.delenv(name, raising=False)
    for name, value in switches:
        monkeypatch.setenv(name, value)


# ---------------------------------------------------------------- the yardstick, computed once per input
@functools.lru_cache(maxsize=None)
def masks_of(L, W, leaders, kind):
    """None, random non-empty sets, or every label but the one that leads on the item (the trainers' uint32 masks)."""
    if kind is None:
        return None
    csr = fam.window_batch(L, W, leaders)
    n = int(csr[0][-1])
    out = tp.random_masks(np.random.default_rng(7600 + 40 * L + W), n, L) if kind == "random" else fam.forbid_the_leader(L, csr)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def score_of(L, W, leaders, kind):
    cptr, gptr, attr = fam.window_batch(L, W, leaders)
    w = fam.leader_weights(L) if leaders else fam.base(L)[0]
    allowed = masks_of(L, W, leaders, kind)
    score = cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L) if allowed is None else allowed)
    score.setflags(write=False)
    return score


def compute_reference(L, key, W, step, pad, kind, dtype=np.float64):
    """(p_all, {background: p_any} for the backgrounds 0 and L - 1) of a planted input."""
    _, trans, leaders = fam.window_model(L, key)
    cptr = fam.window_batch(L, W, leaders)[0]
    p_all, p_any = wr.windowed_backgrounds(cptr, score_of(L, W, leaders, kind), trans, W, step, (0, L - 1), pad, dtype)
    return p_all, {0: p_any[0], L - 1: p_any[1]}


@functools.lru_cache(maxsize=None)
def _reference(L, key, W, step=1, pad=True, kind=None):
    p_all, p_any = compute_reference(L, key, W, step, pad, kind)
    for x in (p_all, *p_any.values()):
        x.setflags(write=False)
    return p_all, p_any


def _judge(tag, got, ref, failed):
    """One output against the yardstick: its worst |error| (NaN where the patterns differ); what it misses goes to `failed`."""
    got = np.asarray(got)
    assert got.shape == ref.shape, tag
    here = ~np.isnan(ref)
    err = float(np.abs(got[here] - ref[here]).max(initial=0.0)) if np.array_equal(np.isnan(got), ~here) else float("nan")
    if np.isinf(got).any():
        failed.append(f"{tag}: an infinity")
    if np.isnan(err):
        failed.append(f"{tag}: {int((np.isnan(got) != ~here).sum())} values differ from the yardstick's NaN pattern")
    else:
        if got[here].size and not (got[here].min() >= 0.0 and got[here].max() <= 1.0):
            failed.append(f"{tag}: outside [0, 1]: min {got[here].min()!r}, max - 1 = {got[here].max() - 1.0:.3g}")
        if not err <= TOL:
            failed.append(f"{tag}: off by {err:.3g} (x{err / TOL:.3g} of the tolerance)")
    return err


def _run(nat, arrangement, L, key, W, step=1, pad=True, kind=None, failed=None):
    """One planted input through one arrangement: asserts the tier, judges every queried output, prints the worst figure.
    Returns (kernel name, worst |error|)."""
    name, _, _, small, other = arrangement
    w, trans, leaders = fam.window_model(L, key)
    csr = fam.window_batch(L, W, leaders)
    allowed = masks_of(L, W, leaders, kind)
    model = nat.Model.from_tables(w, trans)
    plan = nat.Plan(model, csr[0], W, step, pad, device=-1)
    everything = is_all(arrangement)
    kernel = plan.all_kernel_name if everything else plan.kernel_name
    expect = small if small is not None and fam.small_tier_ok(L, W, trans, everything) else other
    assert kernel.startswith(expect) if expect.endswith("_") else kernel == expect, f"{name} {key} W={W}: {kernel}, not {expect}"
    if kind and not kernel.startswith("gl_"):  # (allowed-label sets exist on the any-label route alone: crf_plan.cpp)
        kernel = "the any-label route"
    tag = f"{name} {key} W={W} step={step} pad={int(pad)}" + (f" masks={kind}" if kind else "") + f" [{kernel}]"
    ref_all, ref_any = _reference(L, key, W, step, pad, kind)
    mine, worst = [], 0.0
    if everything:
        for bg in (0, L - 1):
            p_all, p_any = model.windowed_marginals_all(*csr, W, step, background=bg, pad=pad, allowed=allowed)
            errs = (_judge(f"{tag} p_all (background {bg})", p_all, ref_all, mine), _judge(f"{tag} p_any (background {bg})", p_any, ref_any[bg], mine))
            worst = max(worst, *errs) if not np.isnan(errs).any() else float("nan")
            if L == 2 and not np.array_equal(p_any.view(np.uint64), p_all[:, 1 - bg].copy().view(np.uint64)):
                mine.append(f"{tag}: with two labels p_any is not the other column bit for bit")
    else:
        for label in queried(L):
            p = model.windowed_marginals(*csr, W, step, label, pad, allowed=allowed)
            err = _judge(f"{tag} label {label}", p, ref_all[:, label], mine)
            worst = max(worst, err) if not np.isnan(err) else float("nan")
    print(f"{tag}: worst |error| = {worst:.3g} (x{worst / TOL:.3g} of {TOL:g})" + ("" if not mine else "  MISSES"))
    if failed is None:
        assert not mine, "\n".join(mine)
    else:
        failed += mine
    return kernel, worst


def _ids(arrangements):
    return [a[0] for a in arrangements]


# ---------------------------------------------------------------- 1. the guard edge
EDGE_CASES = [(a, W) for a in SINGLE + TWO + ALL for W in (all_windows(a[1]) if is_all(a) else single_windows(a[1]))]


@pytest.mark.parametrize("arrangement,W", EDGE_CASES, ids=[f"{a[0]}-W{W}" for a, W in EDGE_CASES])
def test_both_sides_of_the_guard(nat, monkeypatch, arrangement, W):
    """Four shapes of the spread at the last grid value inside ``spread (W - 1) < 600`` and at the first beyond it, plain and
    with the leaders: the un-normalised tier takes the first, the lane-group tier the second, both are the yardstick's."""
    name, L, switches, small, other = arrangement
    _switch(monkeypatch, switches)
    failed, tiers = [], set()
    for key in edge_keys(W):
        trans = fam.window_model(L, key)[1]
        s = float(trans.max() - trans.min())
        assert (s * (W - 1) < 600.0) == (key[3] == 0) and s == fam.guard_spread(W) + key[3] * fam.GRID
        kernel, _ = _run(nat, arrangement, L, key, W, failed=failed)
        tiers.add((key[3], kernel))
    if small is not None:
        assert tiers == {(0, small), (1, other)}, f"{name} W={W}: the two sides land on {sorted(tiers)}"
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("arrangement", [a for a in SINGLE + ALL if a[1] == 8 and a[3]], ids=["single", "all"])
def test_a_window_past_the_tier_s_limit_at_the_guard(nat, monkeypatch, arrangement):
    """21 items at 5 to 8 labels: the lane-group tier by the window limit, whatever the spread."""
    _switch(monkeypatch, arrangement[2])
    failed = []
    for key in edge_keys(21, ("sticky",)):
        kernel, _ = _run(nat, arrangement, 8, key, 21, failed=failed)
        assert kernel == arrangement[4]
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------- 2. beyond the guard: the lane-group tier
GROUP_ARRANGEMENTS = [a for a in SINGLE + TWO + ALL if a[3] is None and a[4].startswith("gl_")]


def _unreached(L, what, W):
    """[n, L] bool: the (item, label) pairs of family c that no path of any covering window reaches, at step 1 with padding.
    "row": label L - 1 is followed by nothing, so it is legal at a window's last item only; "column": label 0 follows nothing,
    so it is legal at a window's first item only.  A padding item is an item of the window like any other."""
    out = []
    for m in fam.window_lengths(W):
        n, front = max(m, W), ((W - m) // 2 if m < W else 0)
        pos = front + np.arange(m)
        starts = np.arange(0, n - W + 1)
        dead = np.zeros((m, L), dtype=bool)
        if what.startswith("row"):
            dead[:, L - 1] = ~np.isin(pos - (W - 1), starts)
        elif what == "column":
            dead[:, 0] = ~np.isin(pos, starts)
        out.append(dead)
    return np.concatenate(out, axis=0)


@pytest.mark.parametrize("family", sorted(BEYOND))
@pytest.mark.parametrize("arrangement", GROUP_ARRANGEMENTS, ids=_ids(GROUP_ARRANGEMENTS))
def test_the_lane_group_tier_beyond_the_guard(nat, monkeypatch, arrangement, family):
    """What the guard turns away, and what the tier's switch sends there: uniform shifts to |trans| of 150 and 600 (family a),
    one entry 149 to 2000 below the maximum (b), a forbidden row, column or diagonal at -2000 (c), labels that lead by 800 (d)."""
    name, L, switches, _, other = arrangement
    _switch(monkeypatch, switches)
    failed = []
    for W in (5, 20):
        for key in beyond_keys(family):
            kernel, _ = _run(nat, arrangement, L, key, W, failed=failed)
            assert kernel == other
            if family == "c" and is_all(arrangement):
                dead = _unreached(L, key[1], W)
                assert (key[1] == "diagonal") != bool(dead.any())
                w, trans, leaders = fam.window_model(L, key)
                p_all, _ = nat.Model.from_tables(w, trans).windowed_marginals_all(*fam.window_batch(L, W, leaders), W, 1, background=0, pad=True)
                assert np.all(_reference(L, key, W)[0][dead] < 1e-300), "the yardstick's own dead pairs"
                if not np.all(p_all[dead] < 1e-300):
                    failed.append(f"{name} {key} W={W}: mass {p_all[dead].max():.3g} on a pair no window's path reaches")
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------- 3. geometry at the edge
@pytest.mark.parametrize("W,step,pad", GEOMETRY, ids=[f"W{W}-step{s}-pad{int(p)}" for W, s, p in GEOMETRY])
@pytest.mark.parametrize("arrangement", SINGLE + TWO + ALL, ids=_ids(SINGLE + TWO + ALL))
def test_steps_and_skipped_contigs_at_the_guard(nat, monkeypatch, arrangement, W, step, pad):
    """Skipped contigs hold NaN, items that no window covers hold exactly 0, on both sides of the guard."""
    name, L, switches, _, _ = arrangement
    _switch(monkeypatch, switches)
    cptr = fam.window_batch(L, W)[0]
    failed = []
    for key in edge_keys(W, ("sticky",), (False,)):
        ref_all, _ = _reference(L, key, W, step, pad)
        short = np.concatenate([np.full(m, 0 < m < W and not pad) for m in np.diff(cptr)])
        assert np.array_equal(np.isnan(ref_all).any(axis=1), short) and short.any() == (not pad)
        bare = (ref_all == 0.0).all(axis=1)
        assert bare.any() == (step > 1), "the yardstick leaves items uncovered where the step does"
        _run(nat, arrangement, L, key, W, step, pad, failed=failed)  # (an exact 0 in the yardstick and |error| <= 1e-12 ...)
        w, trans, _ = fam.window_model(L, key)
        model = nat.Model.from_tables(w, trans)
        if is_all(arrangement):
            p_all, p_any = model.windowed_marginals_all(*fam.window_batch(L, W), W, step, background=0, pad=pad)
            exact = np.all(p_all[bare] == 0.0) and np.all(p_any[bare] == 0.0)
        else:
            exact = np.all(model.windowed_marginals(*fam.window_batch(L, W), W, step, 0, pad)[bare] == 0.0)
        if not exact:  # (... is not yet an exact 0 on the device)
            failed.append(f"{name} {key}: an item that no window covers does not hold an exact 0")
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------- 4. masks
MASK_ARRANGEMENTS = [a for a in SINGLE + TWO + ALL if a[1] in MASK_LABELS and (a[3] or a[0] == "L2-fast" or a[0] == "L17-all-groups")]


@pytest.mark.parametrize("kind", MASK_KINDS)
@pytest.mark.parametrize("arrangement", MASK_ARRANGEMENTS, ids=_ids(MASK_ARRANGEMENTS))
def test_allowed_label_sets_at_the_guard_and_under_leaders(nat, monkeypatch, arrangement, kind):
    """``allowed=`` on the "sticky" guard-edge model and on family d, both with a leader on every item: random sets, and sets
    that forbid the leader wherever it leads (every allowed label then trails the forbidden one by 800)."""
    name, L, switches, _, _ = arrangement
    _switch(monkeypatch, switches)
    failed = []
    for W in (5, 20):
        for key in mask_keys(W):
            allowed = masks_of(L, W, True, kind)
            assert np.all(allowed != 0) and np.any(allowed != (1 << L) - 1)
            _run(nat, arrangement, L, key, W, kind=kind, failed=failed)
    assert not failed, "\n".join(failed)
