"""The device training objective (gecco_crf_trainer_eval) where it can go wrong: weights far from the origin (score and
transition gaps beyond fp64's exp range, the scaled forward-backward's underflow and its log-space recomputation), the
closed form at w = 0, a set large enough for every strided loop to run more than once, window edges, and reuse of one
trainer across weight vectors.  Results are compared with benchkit.train_objective (numpy, log space) within bounds
derived from the magnitudes involved (tests.helpers.objective_tolerances), or with a closed form."""
import math
import zlib

import numpy as np
import pytest

from benchkit.train_objective import objective
from tests.helpers import objective_tolerances, random_problem

pytestmark = pytest.mark.gpu


def _trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K):
    from gecco_amd import _native

    return _native.Trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)


def check_against_numpy(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, w, strict=False):
    """Device f, g finite and within the derived bounds of the log-space reference; `strict` (weights of order 1) also
    within 1e-12 |f| and 1e-9 (1 + |g|), the bounds of tests/test_gpu_train.py.  Returns the device (f, g)."""
    f, g = tr.eval(w)
    ef, eg, nw, d = objective(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, w, details=True)
    assert tr.num_windows == nw
    assert np.isfinite(ef) and np.all(np.isfinite(eg))  # (the yardstick itself is finite at every point used here)
    assert np.isfinite(f) and np.all(np.isfinite(g)), (f, int(np.count_nonzero(~np.isfinite(g))))
    tol_f, tol_g = objective_tolerances(seq_ptr, item_ptr, attr_id, W, step, sfid, tfid, w, d)
    if strict:
        tol_f = min(tol_f, 1e-12 * abs(ef))
        tol_g = np.minimum(tol_g, 1e-9 * (1 + np.abs(eg)))
    assert abs(f - ef) <= tol_f, (f, ef, abs(f - ef), tol_f)
    err = np.abs(g - eg)
    assert np.all(err <= tol_g), (int(np.argmax(err / np.maximum(tol_g, 1e-300))), float(err.max()))
    return f, g


# ---------------------------------------------------------------- weights far from the origin
SHAPES = [(2, 1), (2, 3), (5, 1), (5, 3), (20, 1), (20, 3), (32, 1), (32, 3)]
SHAPES = [(W, s) for W, s in SHAPES if s <= W]


@pytest.mark.parametrize("scale", [0.1, 1.0, 10.0, 100.0, 150.0, 300.0, 1000.0])
@pytest.mark.parametrize("W,step", SHAPES)
def test_weight_scale_sweep(W, step, scale):
    rng = np.random.default_rng(7000 + 37 * W + step)
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K, w0 = random_problem(rng, W, step)
    tr = _trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)
    check_against_numpy(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, scale * w0, strict=scale <= 1)


@pytest.mark.parametrize("step", [1, 3])
def test_underflow_at_150x_with_every_exp_in_range(step):
    """Weights 150 x N(0, 1.5) on a problem (seed 17) whose transition weights (about -603 to 251) keep every exp(t)
    finite and normal, but where the scaled products underflow inside a third of the windows: labels lose their alpha
    while their paths dominate later in the window (log Z off by hundreds of nats, NaN marginals without the
    log-space recomputation)."""
    W = 20
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K, w0 = random_problem(np.random.default_rng(17), W, step)
    tr = _trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)
    check_against_numpy(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, 150.0 * w0)


def _blocks_problem(blocks, W, step, n_copies=3):
    """Sequences made of blocks (attribute, label, length): attribute a on every item of its block, one feature for
    every (attribute, label) and label pair (state feature 2a + y, transition 2A + 2i + j).  The copies are shifted by
    one item each, so the windows see the block edges at every offset."""
    A = 1 + max(a for a, _, _ in blocks)
    seq_ptr, item_ptr, attr_id, labels = [0], [0], [], []
    for c in range(n_copies):
        for a, y, n in ([(blocks[0][0], blocks[0][1], c)] if c else []) + list(blocks):
            for _ in range(n):
                attr_id.append(a)
                item_ptr.append(len(attr_id))
                labels.append(y)
        seq_ptr.append(len(labels))
    sfid = np.arange(2 * A, dtype=np.int32)
    tfid = 2 * A + np.arange(4, dtype=np.int32)
    return (np.array(seq_ptr, dtype=np.int32), np.array(item_ptr, dtype=np.int32), np.array(attr_id, dtype=np.int32),
            np.array(labels, dtype=np.int32), A, sfid, tfid, 2 * A + 4)


def _weights(A, state, trans):
    """state {(a, y): weight}, trans (t00, t01, t10, t11) -> the weight vector of _blocks_problem's features."""
    w = np.zeros(2 * A + 4)
    for (a, y), v in state.items():
        w[2 * a + y] = v
    w[2 * A:] = trans
    return w


# (blocks, state weights, transition weights) at W = 20; every case leaves the range of the scaled form on purpose
HAND_CASES = {
    # exp(720) overflows: the scaled form needs the max-shifted transitions
    "transition_plus_720": ([(0, 0, 12), (1, 1, 14), (0, 0, 10)], {(0, 0): 2.0, (1, 1): 1.5}, (720.0, -1.0, 0.5, 3.0)),
    # exp(-800) underflows, and the gold path needs that transition: 1000-nat states on both sides of the 0 -> 1 edge
    "transition_minus_800": ([(0, 0, 15), (1, 1, 15)], {(0, 0): 1000.0, (1, 1): 1000.0}, (0.0, -800.0, 0.0, 0.0)),
    # a state gap of 760 nats; the gold path runs through the improbable label on the middle block
    "state_gap_760_gold_improbable": ([(0, 0, 8), (1, 1, 6), (0, 0, 12)], {(1, 0): 760.0}, (0.5, -0.5, -0.5, 0.5)),
    # an 800-nat gap that flips sign halfway: label 1's alpha underflows, then label 1's paths dominate
    "gap_flips_sign_path_loss": ([(0, 0, 10), (1, 1, 10), (0, 0, 5)], {(0, 0): 800.0, (1, 1): 800.0},
                                 (-524.0, 0.0, 0.0, 114.0)),
}


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("case", sorted(HAND_CASES))
def test_hand_set_extremes(case, step):
    blocks, state, trans = HAND_CASES[case]
    W = 20
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K = _blocks_problem(blocks, W, step)
    tr = _trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)
    w = _weights(A, state, trans)
    check_against_numpy(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, w)
    # the same data with ordinary weights stays on the tight bounds (the flagging leaves the other windows alone)
    check_against_numpy(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, np.sign(w) * 0.7, strict=True)


# ---------------------------------------------------------------- closed form at w = 0
def _closed_form_at_zero(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K):
    """At w = 0 every label path of a window is equally likely: log Z = W ln 2, gold = 0, node marginals 1/2, pairwise
    marginals 1/4.  So f = n_windows W ln 2, g(a, y) = (window-occurrences of a) / 2 - empirical, g(i, j) =
    n_windows (W - 1) / 4 - empirical.  Empirical counts by plain loops over the windows."""
    occ = np.zeros(A)
    emp_s = np.zeros((A, 2))
    emp_t = np.zeros((2, 2))
    nw = 0
    for s in range(len(seq_ptr) - 1):
        for i0 in range(int(seq_ptr[s]), int(seq_ptr[s + 1]) - W + 1, step):
            nw += 1
            for i in range(i0, i0 + W):
                for a in attr_id[item_ptr[i]:item_ptr[i + 1]]:
                    occ[a] += 1
                    emp_s[a, labels[i]] += 1
                if i > i0:
                    emp_t[labels[i - 1], labels[i]] += 1
    g = np.zeros(K)
    sfid, tfid = np.asarray(sfid).reshape(A, 2), np.asarray(tfid).reshape(2, 2)
    for a in range(A):
        for y in range(2):
            if sfid[a, y] >= 0:
                g[sfid[a, y]] += occ[a] / 2 - emp_s[a, y]
    for i in range(2):
        for j in range(2):
            if tfid[i, j] >= 0:
                g[tfid[i, j]] += nw * (W - 1) / 4 - emp_t[i, j]
    return nw * W * math.log(2.0), g, nw


def check_closed_form(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K):
    ef, eg, nw = _closed_form_at_zero(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)
    f, g = tr.eval(np.zeros(K))
    assert tr.num_windows == nw
    # every marginal is exactly 1/2 or 1/4 in the scaled form (c = 2, alpha = 1/2, u = 1/2, beta = 1), so the counts
    # are sums of exact binary fractions: g is exact.  f rounds ln 2 once per window position and then sums n_windows
    # rows: 4 eps (W + log2 n_windows) f.
    np.testing.assert_array_equal(g, eg)
    assert abs(f - ef) <= 4 * np.finfo(np.float64).eps * (W + math.log2(nw + 1)) * ef, (f, ef)
    return nw


# ---------------------------------------------------------------- window edges
def _edge_case(name):
    """(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K, tail_attr) for the named window-edge case;
    tail_attr is an attribute that only uncovered tail items carry (None if there is none)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    tail_attr = None
    W, step, A = {"step_eq_W_5": (5, 5, 12), "step_eq_W_32": (32, 32, 12), "uncovered_tail": (5, 3, 12),
                  "exactly_W": (7, 2, 12), "empty_items_and_windows": (4, 1, 12), "all_labels_0": (6, 2, 12),
                  "all_labels_1": (6, 2, 12), "one_attribute": (5, 1, 1), "no_sequences": (5, 1, 4)}[name]
    if name == "no_sequences":
        lengths = []
    elif name == "exactly_W":
        lengths = [W] * 6
    elif name == "uncovered_tail":
        lengths = [W + 2 * step + r for r in (0, 1, 2, 1, 2)]  # tails of 0 to step - 1 items no window reaches
    else:
        lengths = [W, 2 * W + 1] + list(rng.integers(W, 3 * W + 7, size=5))
    seq_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(seq_ptr[-1])
    y = (np.cumsum(rng.random(n) < 0.2) & 1).astype(np.int32)
    if name == "all_labels_0":
        y[:] = 0
    if name == "all_labels_1":
        y[:] = 1
    items = [list(rng.integers(0, A, size=int(rng.integers(0, 4)))) for _ in range(n)]
    if name == "empty_items_and_windows":
        for i in range(n):
            if rng.random() < 0.3:
                items[i] = []
        for i in range(int(seq_ptr[1])):  # the first sequence holds no attribute at all
            items[i] = []
    if name == "uncovered_tail":
        A += 1
        tail_attr = A - 1
        for s in range(len(lengths)):
            b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
            covered = b + (e - b - W) // step * step + W
            for i in range(covered, e):
                items[i] = items[i] + [tail_attr]
        assert sum(tail_attr in it for it in items) > 0
    item_ptr = np.concatenate([[0], np.cumsum([len(it) for it in items])]).astype(np.int32)
    attr_id = np.array([a for it in items for a in it], dtype=np.int32)
    sfid = np.arange(2 * A, dtype=np.int32)
    tfid = 2 * A + np.arange(4, dtype=np.int32)
    return seq_ptr, item_ptr, attr_id, y, A, W, step, sfid, tfid, 2 * A + 4, tail_attr


EDGE_CASES = ["step_eq_W_5", "step_eq_W_32", "uncovered_tail", "exactly_W", "empty_items_and_windows", "all_labels_0",
              "all_labels_1", "one_attribute", "no_sequences"]


@pytest.mark.parametrize("name", EDGE_CASES)
def test_window_edges(name):
    seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K, tail_attr = _edge_case(name)
    tr = _trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)
    nw = check_closed_form(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)
    w = np.random.default_rng(3).normal(0, 1.5, size=K)
    if name == "no_sequences":
        assert nw == 0
        f, g = tr.eval(w)
        assert f == 0.0 and np.all(g == 0.0) and g.shape == (K,)
        return
    assert nw > 0
    f, g = check_against_numpy(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, w, strict=True)
    check_against_numpy(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, 300 * w)
    if tail_attr is not None:  # an attribute no window sees has no expected and no empirical count
        assert g[sfid[2 * tail_attr]] == 0.0 and g[sfid[2 * tail_attr + 1]] == 0.0


@pytest.mark.parametrize("W,step", SHAPES + [(1, 1)])
def test_closed_form_without_features(W, step):
    """K = 0: eval of the empty weight vector is f = n_windows W ln 2 and an empty gradient."""
    rng = np.random.default_rng(W + 100 * step)
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K, _ = random_problem(rng, W, step)
    tr = _trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, np.full(2 * A, -1), np.full(4, -1), 0)
    check_closed_form(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, np.full(2 * A, -1), np.full(4, -1), 0)
    tr = _trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)
    check_closed_form(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)


# ---------------------------------------------------------------- scale: every strided loop more than once
def test_scale_300k_items_zipf_attributes():
    """~300 k items at W = 20: more than 65 536 windows (train_reduce_rows' rows per thread > 1), thousands of
    attributes with a Zipf skew (train_attr_counts' lane-strided loop: many attributes over 256 items, one over
    65 536), and one attribute on every item."""
    rng = np.random.default_rng(300_000)
    W, step, A = 20, 1, 3000
    lengths = rng.integers(W, 400, size=1500)
    seq_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(seq_ptr[-1])
    assert n > 250_000
    deg = rng.integers(0, 4, size=n)
    zipf = np.minimum(rng.zipf(1.4, size=int(deg.sum())), A - 1) - 1  # attribute 0 the most frequent
    every = A - 1  # on every item, after its Zipf attributes
    item_ptr = np.concatenate([[0], np.cumsum(deg + 1)]).astype(np.int32)
    attr_id = np.empty(int(item_ptr[-1]), dtype=np.int32)
    last = item_ptr[1:] - 1
    mask = np.ones(len(attr_id), dtype=bool)
    mask[last] = False
    attr_id[mask] = zipf
    attr_id[last] = every
    labels = (np.cumsum(rng.random(n) < 0.05) & 1).astype(np.int32)
    counts = np.bincount(attr_id, minlength=A)
    assert counts[every] == n and counts.max() > 65_536 and np.count_nonzero(counts > 256) >= 5
    sfid = np.arange(2 * A, dtype=np.int32)
    sfid[rng.random(2 * A) < 0.05] = -1
    keep = sfid >= 0
    sfid[keep] = np.arange(int(keep.sum()))
    tfid = int(keep.sum()) + np.arange(4, dtype=np.int32)
    K = int(keep.sum()) + 4
    tr = _trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)
    assert tr.num_windows > 65_536
    w = rng.normal(0, 0.5, size=K)
    w[sfid[2 * every:2 * every + 2]] = (0.3, -0.2)
    check_against_numpy(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, w, strict=True)


# ---------------------------------------------------------------- determinism and no stale state
def test_reuse_across_weight_vectors_is_bit_exact():
    """eval(w1), eval(w2), eval(w1): the third result carries the bits of the first, with w2 sending some windows to
    the log-space recomputation (and some not); two trainers of the same data give the same bits."""
    W, step = 20, 3
    rng = np.random.default_rng(424242)
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K, w1 = random_problem(rng, W, step)
    w2 = 150.0 * w1
    tr = _trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)
    tr2 = _trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)
    f1, g1 = check_against_numpy(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, w1, strict=True)
    f2, g2 = check_against_numpy(tr, seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, w2)
    f3, g3 = tr.eval(w1)
    assert np.float64(f3).tobytes() == np.float64(f1).tobytes() and g3.tobytes() == g1.tobytes()
    for w, (f, g) in ((w2, (f2, g2)), (w1, (f1, g1)), (np.zeros(K), tr.eval(np.zeros(K)))):
        fo, go = tr2.eval(w)
        assert np.float64(fo).tobytes() == np.float64(f).tobytes() and go.tobytes() == g.tobytes()
    f4, g4 = tr.eval(w2)
    assert np.float64(f4).tobytes() == np.float64(f2).tobytes() and g4.tobytes() == g2.tobytes()
