"""Every label's windowed marginal in one device pass (csrc/crf_general_windowed.hip: `gl_all_small`, one lane per window
for 2 to 8 labels; `gl_all_groups`, one group of lanes per window for everything else) against the numpy yardstick
(tests/typed_yardstick.py) and against the single-label entry on the device.  Tolerances: 1e-12 against the yardstick,
as tests/test_gpu_general.py holds the single-label kernels to; 2e-12 between two device results that are each within
1e-12 of one oracle."""
import numpy as np
import pytest

from tests import typed_yardstick as ty
from tests.helpers import synth_contigs, synth_model

pytestmark = pytest.mark.gpu

LABEL_COUNTS = [1, 2, 3, 5, 8, 9, 16, 17, 32]
WINDOWS = [1, 2, 5, 20, 32]
A = 300


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    assert _native.device_count() >= 1
    return _native


def _lengths(W):
    # 300 and 600 cross a 256-slot tile once and twice; empty contigs at both ends
    return [0, 1, W - 1, W, W + 1, 2 * W + 3, 300, 600, 0]


def _steps(W):
    return sorted({s for s in (1, 2, W) if s <= W})


def _check(got, exp, tol, what):
    assert got.shape == exp.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(exp)), what
    ok = ~np.isnan(exp)
    if ok.any():
        err = np.abs(got[ok] - exp[ok]).max()
        assert err <= tol, (what, err)


@pytest.mark.parametrize("L", LABEL_COUNTS)
def test_all_labels_against_yardstick_and_single_label_entry(nat, L):
    rng = np.random.default_rng(4100 + L)
    w, trans = synth_model(A, rng, L=L)
    model = nat.Model.from_tables(w, trans)
    for W in WINDOWS:
        cptr, gptr, attr = synth_contigs(rng, _lengths(W), A)
        for step in _steps(W):
            for pad in (True, False):
                bg = (W + step) % L
                p_all, p_any = model.windowed_marginals_all(cptr, gptr, attr, W, step, background=bg, pad=pad)
                e_all, e_any = ty.windowed_all(w, trans, cptr, gptr, attr, W, step, bg, pad)
                _check(p_all, e_all, 1e-12, (L, W, step, pad, "p_all"))
                _check(p_any, e_any, 1e-12, (L, W, step, pad, "p_any"))
                for l in range(L):
                    single = model.windowed_marginals(cptr, gptr, attr, W, step, l, pad)
                    _check(p_all[:, l], single, 2e-12, (L, W, step, pad, l))
                    assert np.array_equal(np.isnan(p_any), np.isnan(single))
                only_all, none = model.windowed_marginals_all(cptr, gptr, attr, W, step, background=None, pad=pad)
                assert none is None  # (background = -1 with p_any = NULL)
                assert np.array_equal(only_all, p_all, equal_nan=True)


def test_two_labels_p_any_is_the_other_column_bit_for_bit(nat):
    rng = np.random.default_rng(4202)
    w, trans = synth_model(A, rng, L=2)
    model = nat.Model.from_tables(w, trans)
    for W in WINDOWS:
        cptr, gptr, attr = synth_contigs(rng, _lengths(W), A)
        for step in _steps(W):
            for pad in (True, False):
                p_all, p_any = model.windowed_marginals_all(cptr, gptr, attr, W, step, background=0, pad=pad)
                assert np.array_equal(p_any.view(np.uint64), p_all[:, 1].copy().view(np.uint64))
                p_all, p_any = model.windowed_marginals_all(cptr, gptr, attr, W, step, background=1, pad=pad)
                assert np.array_equal(p_any.view(np.uint64), p_all[:, 0].copy().view(np.uint64))


def test_two_labels_bitwise_in_the_lane_group_tier(nat, monkeypatch):
    rng = np.random.default_rng(4203)
    w, trans = synth_model(A, rng, L=2)
    model = nat.Model.from_tables(w, trans)
    cptr, gptr, attr = synth_contigs(rng, _lengths(20), A)
    monkeypatch.setenv("GECCO_CRF_GENERAL_GROUPS", "1")
    assert nat.Plan(model, cptr, 20, 1, True, device=0).all_kernel_name == "gl_all_groups"
    for bg in (0, 1):
        p_all, p_any = model.windowed_marginals_all(cptr, gptr, attr, 20, 1, background=bg, pad=False)
        assert np.array_equal(p_any.view(np.uint64), p_all[:, 1 - bg].copy().view(np.uint64))


def test_one_label(nat):
    rng = np.random.default_rng(4201)
    w, trans = synth_model(A, rng, L=1)
    model = nat.Model.from_tables(w, trans)
    cptr, gptr, attr = synth_contigs(rng, _lengths(5), A)
    p_all, p_any = model.windowed_marginals_all(cptr, gptr, attr, 5, 2, background=0, pad=False)
    single = model.windowed_marginals(cptr, gptr, attr, 5, 2, 0, False)
    scored = ~np.isnan(single) & (single != 0.0)
    assert scored.any() and np.array_equal(np.isnan(p_all[:, 0]), np.isnan(single))
    assert np.array_equal(p_all[scored, 0], np.ones(int(scored.sum())))
    assert np.array_equal(p_any[~np.isnan(single)], np.zeros(int((~np.isnan(single)).sum())))


def test_argument_errors(nat):
    model = nat.Model.from_tables(np.zeros((4, 3)), np.zeros((3, 3)))
    lib = nat.load_library()
    cptr, gptr, attr = (np.array(v, dtype=np.int32) for v in ([0, 2], [0, 1, 2], [0, 1]))
    p_all, p_any = np.zeros((2, 3)), np.zeros(2)
    P = nat._ptr
    args = (model._h, 0, P(cptr, nat._c_i32p), 1, P(gptr, nat._c_i32p), P(attr, nat._c_i32p), 2, 1)
    assert lib.gecco_crf_windowed_marginals_all(*args, -1, 1, P(p_all, nat._c_f64p), None) == 0
    assert lib.gecco_crf_windowed_marginals_all(*args, -1, 1, P(p_all, nat._c_f64p), P(p_any, nat._c_f64p)) == -1  # GECCO_CRF_EINVAL
    assert lib.gecco_crf_last_error()
    assert lib.gecco_crf_windowed_marginals_all(*args, 3, 1, P(p_all, nat._c_f64p), P(p_any, nat._c_f64p)) == -1
    assert b"background" in lib.gecco_crf_last_error()
    plan = nat.Plan(model, cptr, 2, 1, True, device=0)
    with pytest.raises(ValueError, match="background"):
        plan.run_windowed_all(1, 1, 1, d_p_any=1, background=3)
    with pytest.raises(ValueError, match="p_any"):
        plan.run_windowed_all(1, 1, 1, d_p_any=1, background=None)


@pytest.mark.parametrize("L,W", [(3, 5), (3, 20), (8, 20), (2, 32), (17, 5), (17, 20)])
def test_cut_invariance(nat, L, W):
    """A contig scored alone has the bits it has inside a batch (here the batch in reversed contig order)."""
    rng = np.random.default_rng(4300 + 40 * L + W)
    w, trans = synth_model(A, rng, L=L)
    model = nat.Model.from_tables(w, trans)
    lengths = _lengths(W)
    contigs = [synth_contigs(rng, [n], A) for n in lengths]
    rev = list(reversed(contigs))
    cptr = np.concatenate([[0], np.cumsum([c[0][-1] for c in rev])]).astype(np.int32)
    gptr = np.concatenate([[0]] + [c[1][1:] + off for c, off in zip(rev, np.cumsum([0] + [c[1][-1] for c in rev])[:-1])]).astype(np.int32)
    attr = np.concatenate([c[2] for c in rev]).astype(np.int32)
    for step, pad in ((1, True), (2, False), (W, True)):
        if step > W:
            continue
        b_all, b_any = model.windowed_marginals_all(cptr, gptr, attr, W, step, background=0, pad=pad)
        for k, (c1, g1, a1) in enumerate(rev):
            if c1[-1] == 0:
                continue
            one_all, one_any = model.windowed_marginals_all(c1, g1, a1, W, step, background=0, pad=pad)
            sl = slice(int(cptr[k]), int(cptr[k + 1]))
            assert np.array_equal(one_all.view(np.uint64), b_all[sl].copy().view(np.uint64)), (L, W, step, pad, k)
            assert np.array_equal(one_any.view(np.uint64), b_any[sl].view(np.uint64)), (L, W, step, pad, k)


@pytest.mark.parametrize("L", [2, 3, 4, 5, 6, 7, 8])
def test_lane_per_window_tier(nat, L, monkeypatch):
    """2 to 8 labels take `gl_all_small`; GECCO_CRF_GENERAL_GROUPS=1 sends the same model to `gl_all_groups`: both
    against the yardstick, on tiles with padded, skipped and long contigs."""
    rng = np.random.default_rng(4400 + L)
    w, trans = synth_model(200, rng, L=L)
    model = nat.Model.from_tables(w, trans)
    lengths = [1, 2, 3, 19, 20, 21, 40, 63, 64, 65, 200, 237, 238, 474, 475, 0, 1500] + list(rng.integers(1, 60, size=20))
    cptr, gptr, attr = synth_contigs(rng, lengths, 200)
    cases = [(20, 1, True), (20, 7, False), (5, 4, False)] + ([(32, 1, True), (32, 5, False)] if L <= 4 else [(19, 1, False)])
    for W, step, pad in cases:
        bg = L - 1
        e_all, e_any = ty.windowed_all(w, trans, cptr, gptr, attr, W, step, bg, pad)
        assert nat.Plan(model, cptr, W, step, pad, device=0).all_kernel_name == "gl_all_small"
        p_all, p_any = model.windowed_marginals_all(cptr, gptr, attr, W, step, background=bg, pad=pad)
        _check(p_all, e_all, 1e-12, (L, W, step, pad, "small p_all"))
        _check(p_any, e_any, 1e-12, (L, W, step, pad, "small p_any"))
        monkeypatch.setenv("GECCO_CRF_GENERAL_GROUPS", "1")
        assert nat.Plan(model, cptr, W, step, pad, device=0).all_kernel_name == "gl_all_groups"
        g_all, g_any = model.windowed_marginals_all(cptr, gptr, attr, W, step, background=bg, pad=pad)
        monkeypatch.delenv("GECCO_CRF_GENERAL_GROUPS")
        _check(g_all, e_all, 1e-12, (L, W, step, pad, "groups p_all"))
        _check(g_any, e_any, 1e-12, (L, W, step, pad, "groups p_any"))
    if L >= 5:  # windows beyond the tier's 20 genes go to the lane-group tier
        assert nat.Plan(model, cptr, 21, 1, True, device=0).all_kernel_name == "gl_all_groups"


@pytest.mark.parametrize("L", [1, 9, 13, 32])
def test_lane_group_tier_by_model_choice(nat, L):
    rng = np.random.default_rng(4500 + L)
    w, trans = synth_model(200, rng, L=L)
    model = nat.Model.from_tables(w, trans)
    cptr, gptr, attr = synth_contigs(rng, [1, 19, 20, 21, 64, 237, 0, 500, 47, 48, 49], 200)
    for W, step, pad in ((20, 1, True), (48, 7, True), (48, 1, False)):
        assert nat.Plan(model, cptr, W, step, pad, device=0).all_kernel_name == "gl_all_groups"
        bg = L // 2
        p_all, p_any = model.windowed_marginals_all(cptr, gptr, attr, W, step, background=bg, pad=pad)
        e_all, e_any = ty.windowed_all(w, trans, cptr, gptr, attr, W, step, bg, pad)
        _check(p_all, e_all, 1e-12, (L, W, step, pad, "p_all"))
        _check(p_any, e_any, 1e-12, (L, W, step, pad, "p_any"))


def test_lane_per_window_tier_range_guard(nat):
    """The construction of test_gpu_general.test_lane_per_window_kernel_range_guard: the un-normalised tier up to a
    transition spread of 600 / (W - 1), the scaled lane-group tier beyond; the caller sees no difference."""
    rng = np.random.default_rng(77)
    A_, L, W = 60, 3, 20
    w = np.clip(rng.laplace(0.0, 6.0, size=(A_, L)), -40.0, 40.0)
    cptr, gptr, attr = synth_contigs(rng, [19, 20, 21, 300, 1000], A_)
    for spread, kernel in ((31.5, "gl_all_small"), (31.6, "gl_all_groups"), (80.0, "gl_all_groups")):
        trans = rng.uniform(-1.0, 1.0, size=(L, L))
        trans[1, 2] = trans.max() - spread  # (W - 1) * 31.5 = 598.5
        trans[trans < trans[1, 2]] = trans[1, 2]
        model = nat.Model.from_tables(w, trans)
        assert nat.Plan(model, cptr, W, 1, True, device=0).all_kernel_name == kernel
        p_all, p_any = model.windowed_marginals_all(cptr, gptr, attr, W, 1, background=0, pad=True)
        e_all, e_any = ty.windowed_all(w, trans, cptr, gptr, attr, W, 1, 0, True)
        _check(p_all, e_all, 1e-12, (spread, "p_all"))
        _check(p_any, e_any, 1e-12, (spread, "p_any"))


def test_extreme_state_weights(nat, monkeypatch):
    rng = np.random.default_rng(4600)
    L, W = 5, 20
    w = 50.0 * rng.normal(0, 1, size=(A, L))
    trans = rng.normal(0, 1.5, size=(L, L))
    model = nat.Model.from_tables(w, trans)
    cptr, gptr, attr = synth_contigs(rng, _lengths(W), A)
    e_all, e_any = ty.windowed_all(w, trans, cptr, gptr, attr, W, 1, 0, True)
    for groups in (False, True):
        if groups:
            monkeypatch.setenv("GECCO_CRF_GENERAL_GROUPS", "1")
        p_all, p_any = model.windowed_marginals_all(cptr, gptr, attr, W, 1, background=0, pad=True)
        assert np.isfinite(p_all).all() and np.isfinite(p_any).all()
        assert p_all.min() >= 0.0 and p_all.max() <= 1.0 and p_any.min() >= 0.0 and p_any.max() <= 1.0
        _check(p_all, e_all, 1e-12, ("extreme", groups))
        _check(p_any, e_any, 1e-12, ("extreme p_any", groups))


def test_sequence_crf_predict_windowed_all(nat):
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(4700)
    names = [f"a{k}" for k in range(12)]
    X, y = [], []
    for _ in range(6):
        n = int(rng.integers(8, 30))
        labs = [str(v) for v in (np.arange(n) // 4 + int(rng.integers(0, 3))) % 3]
        X.append([[names[(4 * int(lab) + int(rng.integers(0, 4))) % 12]] for lab in labs])
        y.append(labs)
    crf = SequenceCRF(window_size=5, c1=0.1, c2=0.1).fit(X, y)
    Xp = X + [[["a1"], ["a5"]]]
    cols, anys = crf.predict_windowed_all(Xp, background=crf.classes_[0])
    only = crf.predict_windowed_all(Xp)
    assert len(cols) == len(anys) == len(only) == len(Xp)
    for k, label in enumerate(crf.classes_):
        single = crf.predict_windowed(Xp, label)
        for a, b in zip(cols, single):
            assert a.shape == (len(b), len(crf.classes_)) and np.abs(a[:, k] - b).max() <= 2e-12
    for a, b, c in zip(cols, only, anys):
        assert np.array_equal(a, b) and c.shape == (len(a),) and (c <= a[:, 1:].sum(axis=1) + 1e-12).all()
    with pytest.raises(ValueError, match="unknown label"):
        crf.predict_windowed_all(Xp, background="nope")


@pytest.mark.parametrize("L,pad", [(2, True), (2, False), (3, False)])
def test_plan_after_a_whole_contig_pass(nat, L, pad, monkeypatch):
    """The lane-per-window tier's tile table is built on the first `run_windowed_all` of a plan whose own table has
    another geometry (2-label plans; plans built under GECCO_CRF_GENERAL_GROUPS): a whole-contig pass on the plan in
    between must not change it.  Padded (pad) or skipped (no pad) short contigs make the tiles irregular."""
    import torch

    rng = np.random.default_rng(4800 + L)
    w, trans = synth_model(A, rng, L=L)
    model = nat.Model.from_tables(w, trans)
    W = 20
    cptr, gptr, attr = synth_contigs(rng, [3, 300, 0, 7, 19, 600, 12, 45, 1, 260, 5], A)
    n = int(cptr[-1])
    if L != 2:
        monkeypatch.setenv("GECCO_CRF_GENERAL_GROUPS", "1")
    plan = nat.Plan(model, cptr, W, 1, pad, device=0)
    monkeypatch.delenv("GECCO_CRF_GENERAL_GROUPS", raising=False)
    assert plan.all_kernel_name == "gl_all_small" and plan.kernel_name != "gl_windowed_small"
    dev = torch.device("cuda:0")
    d_gp, d_at = torch.from_numpy(gptr).to(dev), torch.from_numpy(attr).to(dev)
    y = torch.zeros(n, dtype=torch.int8, device=dev)
    p_all = torch.full((n, L), -1.0, dtype=torch.float64, device=dev)
    p_any = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    plan.run_viterbi(d_gp.data_ptr(), d_at.data_ptr(), y.data_ptr())
    plan.run_windowed_all(d_gp.data_ptr(), d_at.data_ptr(), p_all.data_ptr(), p_any.data_ptr(), background=0)
    torch.cuda.synchronize()
    e_all, e_any = ty.windowed_all(w, trans, cptr, gptr, attr, W, 1, 0, pad)
    _check(p_all.cpu().numpy(), e_all, 1e-12, (L, pad, "p_all"))
    _check(p_any.cpu().numpy(), e_any, 1e-12, (L, pad, "p_any"))
    # and again, now that the table exists, after another whole-contig pass
    marg = torch.zeros(n, L, dtype=torch.float64, device=dev)
    plan.run_marginals_full(d_gp.data_ptr(), d_at.data_ptr(), marg.data_ptr())
    p_all.fill_(-1.0)
    plan.run_windowed_all(d_gp.data_ptr(), d_at.data_ptr(), p_all.data_ptr(), p_any.data_ptr(), background=0)
    torch.cuda.synchronize()
    _check(p_all.cpu().numpy(), e_all, 1e-12, (L, pad, "p_all again"))
