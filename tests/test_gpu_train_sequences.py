"""Training on whole sequences on the device: ``gecco_crf_trainer_sequences_eval`` against the independent numpy yardstick
(tests/train_objective_sequences.py), the kernel's geometry edges and length extremes, its bit contracts and refusals,
its agreement with the window trainers where every sequence is one window, the fits through it against scipy's optimum
of the yardstick, and ``SequenceCRF(window_size=None)`` end to end."""
import ctypes

import numpy as np
import pytest

from tests.train_objective_labels import labelled_sequences, same_bits
from tests.train_objective_sequences import objective_sequences, objective_sequences_tolerances, sequences_problem

pytestmark = pytest.mark.gpu

# the sequence kernel's geometry (csrc/crf_train_general.hip): 256 threads as groups of G = next power of two >= L
# lanes; a workgroup owns the 256 / G sequences it runs side by side, and the first stage of the block sums has
# kTrainGenReduceSlabs slabs
THREADS = 256
REDUCE_SLABS = 32


def _group(L):
    G = 2
    while G < L:
        G *= 2
    return G


def _trainer(*problems):
    from gecco_amd import _native

    return _native.TrainerSequences(list(problems))


def _labels_of(s):
    return np.asarray(s[5]).size // s[4]


def _reference(s, w):
    return objective_sequences(*s[:5], _labels_of(s), s[5], s[6], w)


def check_strict(tr, k, s, w, ws=None, active=None):
    """Problem k of `tr` at `w` within the project's bounds of the yardstick (tests/test_gpu_train_general.py), and the
    same bytes from a second evaluation.  Returns (f, g)."""
    n = len(tr)
    ws = [w if j == k else None for j in range(n)] if ws is None else ws
    active = [j == k for j in range(n)] if active is None else active
    f, g = tr.eval(ws, active)
    ef, eg, n_seqs = _reference(s, w)
    assert tr.num_sequences(k) == n_seqs
    print(f"L={_labels_of(s)} sequences={n_seqs}: |f - ref| / |ref| = {abs(f[k] - ef) / max(abs(ef), 1e-300):.3g}, "
          f"max |g - ref| / (1 + |ref|) = {(np.abs(g[k] - eg) / (1 + np.abs(eg))).max() if len(eg) else 0.0:.3g}")
    assert abs(f[k] - ef) <= 1e-12 * abs(ef), (f[k], ef)
    assert np.all(np.abs(g[k] - eg) <= 1e-9 * (1 + np.abs(eg))), np.abs(g[k] - eg).max()
    f2, g2 = tr.eval(ws, active)
    assert same_bits(f[k], g[k], f2[k], g2[k])
    return f[k], g[k]


def check_bounds(tr, k, s, w):
    """Problem k at `w` finite and within the derived bounds of the yardstick (weights far from the origin)."""
    n = len(tr)
    f, g = tr.eval([w if j == k else None for j in range(n)], [j == k for j in range(n)])
    ef, eg, _ = _reference(s, w)
    assert np.isfinite(ef) and np.all(np.isfinite(eg))
    assert np.isfinite(f[k]) and np.all(np.isfinite(g[k])), (f[k], int(np.count_nonzero(~np.isfinite(g[k]))))
    tol_f, tol_g = objective_sequences_tolerances(*s[:5], _labels_of(s), s[5], s[6], w)
    err = np.abs(g[k] - eg)
    print(f"L={_labels_of(s)}: |f - ref| = {abs(f[k] - ef):.3g} (bound {tol_f:.3g}), "
          f"max |g - ref| / bound = {(err / np.maximum(tol_g, 1e-300)).max():.3g}")
    assert abs(f[k] - ef) <= tol_f, (f[k], ef, abs(f[k] - ef), tol_f)
    assert np.all(err <= tol_g), (int(np.argmax(err / np.maximum(tol_g, 1e-300))), float(err.max()))


# ---------------------------------------------------------------- objective and gradient against the yardstick
FIXED_LENGTHS = [1, 1, 2, 3, 7, 40, 41, 300]


@pytest.mark.parametrize("L", [2, 3, 5, 8, 17, 32])
def test_eval_matches_the_yardstick(L):
    """Every G (2, 4, 8, 8, 32, 32), with L = G and L < G; 20 attributes, a tenth of the pairs without a feature."""
    rng = np.random.default_rng(7000 + L)
    lengths = FIXED_LENGTHS + [int(x) for x in rng.integers(1, 61, size=30)]
    s = sequences_problem(rng, L, lengths)
    assert np.any(np.diff(s[1]) == 0) and np.any(s[5] < 0) and np.any(s[6] < 0)
    tr = _trainer(s)
    assert len(tr) == 1 and tr.num_sequences(0) == len(lengths)
    check_strict(tr, 0, s, rng.normal(0, 1.5, size=s[7]))
    check_strict(tr, 0, s, np.zeros(s[7]))


# ---------------------------------------------------------------- geometry edges
def _with_sequences(rng, L, n_seqs, lo=1, hi=12, A=20):
    lengths = [int(x) for x in rng.integers(lo, hi + 1, size=n_seqs)]
    return sequences_problem(rng, L, lengths, A=A, drop=0.0, stay=0.8)


@pytest.mark.parametrize("L", [2, 3, 9, 32])
def test_sequence_count_edges(L):
    """A single sequence; one below, at and one above a workgroup's sequences (256 / G, all side by side: a round is
    a workgroup), and the same around two workgroups."""
    rng = np.random.default_rng(600 + L)
    side = THREADS // _group(L)
    for n_seqs in (1, side - 1, side, side + 1, 2 * side - 1, 2 * side, 2 * side + 1):
        s = _with_sequences(rng, L, n_seqs)
        tr = _trainer(s)
        assert tr.num_sequences(0) == n_seqs
        check_strict(tr, 0, s, rng.normal(0, 1.5, size=s[7]))


@pytest.mark.parametrize("n_workgroups", [REDUCE_SLABS - 1, REDUCE_SLABS, REDUCE_SLABS + 1, REDUCE_SLABS + 7])
def test_workgroups_around_the_reduce_slabs(n_workgroups):
    """One below, exactly, one above and several above kTrainGenReduceSlabs workgroups (the last one not full): slabs of
    one block, of two blocks, and empty slabs.  Two labels (128 sequences per workgroup) and 1 to 3 items keep the
    thousands of sequences small."""
    rng = np.random.default_rng(77 + n_workgroups)
    s = _with_sequences(rng, 2, THREADS // _group(2) * (n_workgroups - 1) + 5, hi=3)
    check_strict(_trainer(s), 0, s, rng.normal(0, 1.5, size=s[7]))


def _empty(A=4, L=3):
    return (np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32),
            A, np.arange(A * L, dtype=np.int32), A * L + np.arange(L * L, dtype=np.int32), A * L + L * L)


def test_problem_without_sequences_beside_a_normal_one():
    rng = np.random.default_rng(8)
    s = _with_sequences(rng, 5, 40)
    empty = _empty()
    w = rng.normal(0, 1.5, size=s[7])
    f0, g0 = _trainer(s).eval([w])
    for problems, k in (((empty, s), 1), ((s, empty), 0)):
        tr = _trainer(*problems)
        assert tr.num_sequences(1 - k) == 0 and tr.num_sequences(k) == 40
        ws = [None, None]
        ws[k], ws[1 - k] = w, rng.normal(0, 1.5, size=empty[7])
        f, g = tr.eval(ws)
        assert f[1 - k] == 0.0 and np.all(g[1 - k] == 0.0) and g[1 - k].shape == (empty[7],)
        assert same_bits(f[k], g[k], f0[0], g0[0])
    f, g = _trainer(empty).eval([np.ones(empty[7])])
    assert f[0] == 0.0 and np.all(g[0] == 0.0)


# ---------------------------------------------------------------- length extremes
@pytest.mark.parametrize("L", [2, 5, 32])
def test_only_sequences_of_one_item(L):
    """No transitions: f is a sum of per-item log-sum-exps and the expected transition counts are exactly 0."""
    rng = np.random.default_rng(900 + L)
    s = sequences_problem(rng, L, [1] * 300, drop=0.0)
    tr = _trainer(s)
    w = rng.normal(0, 1.5, size=s[7])
    _, g = check_strict(tr, 0, s, w)
    assert np.all(g[np.asarray(s[6])] == 0.0)


@pytest.mark.parametrize("L", [2, 32])
def test_one_long_sequence_beside_many_short_ones(L):
    """3 000 items in one sequence and 200 sequences of one item: the first workgroup waits for the long sequence while
    its other groups have long left their loops (two workgroups at two labels, 26 at 32)."""
    rng = np.random.default_rng(3000 + L)
    lengths = [1] * 120 + [3000] + [1] * 80
    s = sequences_problem(rng, L, lengths)
    check_strict(_trainer(s), 0, s, rng.normal(0, 1.5, size=s[7]))


# ---------------------------------------------------------------- weights far from the origin
def _plant(s, w, rng):
    """w with one transition at -800 and one at +720 (two pairs that have a feature)."""
    L = _labels_of(s)
    tfid = np.asarray(s[6]).reshape(L, L)
    pairs = [(i, j) for i in range(L) for j in range(L) if tfid[i, j] >= 0]
    a, b = (pairs[k] for k in rng.choice(len(pairs), size=2, replace=False))
    w = w.copy()
    w[tfid[a]], w[tfid[b]] = -800.0, 720.0
    return w


@pytest.mark.parametrize("L", [3, 9])
def test_extreme_weights(L):
    rng = np.random.default_rng(9000 + L)
    s = sequences_problem(rng, L, [1, 2, 5, 20, 41, 150] + [int(x) for x in rng.integers(1, 61, size=20)])
    tr = _trainer(s)
    w = 1000.0 * rng.normal(0, 1.5, size=s[7])
    check_bounds(tr, 0, s, w)
    check_bounds(tr, 0, s, _plant(s, w, rng))
    check_bounds(tr, 0, s, _plant(s, rng.normal(0, 1.5, size=s[7]), rng))


@pytest.mark.parametrize("L", [3, 9])
def test_state_gap_flips_sign_inside_a_sequence(L):
    """Blocks of 11 items, block b with attribute b on every item and label b % L: attribute 0 weighs +800 on label 0
    and attribute 1 +800 on label 1, so across their edge label 1 is 800 nats down and then 800 nats up; the transition
    the gold path takes there weighs -800, another one +720.  The six blocks are one sequence of 66 items, and again two
    of 25 and 41 (cut inside blocks)."""
    n_blocks, blen = 6, 11
    A = n_blocks
    attr_id = np.tile(np.repeat(np.arange(n_blocks), blen), 2).astype(np.int32)
    n = len(attr_id)
    labels = (attr_id % L).astype(np.int32)
    s = (np.array([0, 66, 91, 132], dtype=np.int32), np.arange(n + 1, dtype=np.int32), attr_id, labels, A,
         np.arange(A * L, dtype=np.int32), A * L + np.arange(L * L, dtype=np.int32), A * L + L * L)
    rng = np.random.default_rng(20 * L)
    w = rng.normal(0, 0.5, size=s[7])
    w[0 * L + 0] = 800.0
    w[1 * L + 1] = 800.0
    w[A * L + 0 * L + 1] = -800.0
    w[A * L + 2 * L + 0] = 720.0
    tr = _trainer(s)
    check_bounds(tr, 0, s, w)
    check_strict(tr, 0, s, np.sign(w) * 0.7)


# ---------------------------------------------------------------- sequences that are one window each
@pytest.mark.parametrize("L,W", [(4, 5), (2, 20)])
def test_agrees_with_the_window_trainers(L, W):
    """Every sequence holds exactly W items, so the windowed objective at (W, step 1) is the whole-sequence one:
    ``TrainerGeneral`` at four labels, the 2-label ``Trainer`` at two."""
    from gecco_amd import _native

    rng = np.random.default_rng(50 + L)
    s = sequences_problem(rng, L, [W] * 300)
    w = rng.normal(0, 1.5, size=s[7])
    f, g = _trainer(s).eval([w])
    if L == 2:
        f2, g2 = _native.Trainer(s[0], s[1], s[2], s[3], s[4], W, 1, s[5], s[6], s[7]).eval(w)
    else:
        fs, gs = _native.TrainerGeneral([s + (W, 1)]).eval([w])
        f2, g2 = fs[0], gs[0]
    print(f"L={L} W={W}: |f - windowed| / |f| = {abs(f[0] - f2) / abs(f2):.3g}, "
          f"max |g - windowed| / (1 + |g|) = {(np.abs(g[0] - g2) / (1 + np.abs(g2))).max():.3g}")
    assert abs(f[0] - f2) <= 1e-12 * abs(f2)
    assert np.all(np.abs(g[0] - g2) <= 1e-9 * (1 + np.abs(g2)))


# ---------------------------------------------------------------- several problems at once
def test_masks_and_lone_bits():
    rng = np.random.default_rng(31)
    sets = [sequences_problem(rng, L, [int(x) for x in rng.integers(1, hi, size=n)]) for L, hi, n in
            ((2, 40, 300), (32, 25, 30), (5, 60, 70))]
    ws = [rng.normal(0, 1.5, size=s[7]) for s in sets]
    lone = []
    for s, w in zip(sets, ws):
        f, g = _trainer(s).eval([w])
        lone.append((f[0], g[0]))
    tr = _trainer(*sets)
    assert len(tr) == 3 and [tr.num_sequences(k) for k in range(3)] == [300, 30, 70]
    assert tr.num_sequences(3) == -1 and tr.scratch_bytes(3) == -1
    assert tr.scratch_bytes(-1) == sum(tr.scratch_bytes(k) for k in range(3))
    for mask in ([True] * 3, [False] * 3, [True, False, True], [False, True, False], [False, False, True], [True, True, False]):
        f = np.full(3, -7.25)
        g = [np.full(s[7], -3.5) for s in sets]
        tr.eval([w if m else None for w, m in zip(ws, mask)], mask, f, g)
        for k, m in enumerate(mask):
            if m:
                assert same_bits(f[k], g[k], *lone[k]), (mask, k)
            else:
                assert f[k] == -7.25 and np.all(g[k] == -3.5), (mask, k)
    for k, s in enumerate(sets):
        check_strict(tr, k, s, ws[k])


# ---------------------------------------------------------------- refusals
def _tiny(L, label=0, lengths=(3, 1, 2), A=2):
    n = sum(lengths)
    return (np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), np.zeros(n + 1, dtype=np.int32), [],
            np.full(n, label, dtype=np.int32), A, [-1] * (A * L), [-1] * (L * L), 0)


def test_refusals():
    from gecco_amd import _native

    for L in (1, 33):
        with pytest.raises(_native.NativeError, match="trainer sequences: problem 0: .*models of 2 to 32 labels") as e:
            _trainer(_tiny(L))
        assert e.value.code == _native.EUNSUPPORTED
    with pytest.raises(ValueError, match="trainer sequences: problem 1: trainer: sequence 1 has no items"):
        _trainer(_tiny(3), _tiny(3, lengths=(3, 0, 2)))
    with pytest.raises(ValueError, match=r"trainer sequences: problem 0: trainer: labels must lie in \[0, num_labels\)"):
        _trainer(_tiny(3, label=3))
    _trainer(_tiny(3, label=2))
    bad = list(_tiny(3))
    bad[0] = np.array([0, 4, 3, 6], dtype=np.int32)
    with pytest.raises(ValueError, match="problem 0: trainer: seq_ptr is not monotone"):
        _trainer(tuple(bad))
    bad = list(_tiny(3))
    bad[1], bad[2] = np.array([0, 1, 2, 3, 4, 5, 6], dtype=np.int32), np.array([0, 1, 2, 1, 0, 1], dtype=np.int32)
    with pytest.raises(ValueError, match="problem 0: trainer: attribute id out of range"):
        _trainer(tuple(bad))
    with pytest.raises(ValueError, match="8 entries"):
        _trainer(_tiny(3) + (5, 1))

    # a null weight vector for an active problem, past the Python layer's own checks
    rng = np.random.default_rng(4)
    s = sequences_problem(rng, 3, [4, 2])
    tr = _trainer(_tiny(3), s)
    f = np.zeros(2)
    g = [np.zeros(1), np.zeros(s[7])]
    vp = ctypes.c_void_p
    w_ptr, g_ptr = (vp * 2)(None, None), (vp * 2)(g[0].ctypes.data, g[1].ctypes.data)
    rc = tr._c("eval")(tr._h, (ctypes.c_uint8 * 2)(1, 1), w_ptr, f.ctypes.data, g_ptr)
    assert rc == _native.EINVAL
    assert tr._lib.gecco_crf_last_error().decode() == "trainer_sequences_eval: null argument for problem 1"
    # (problem 0 has no features: its weight vector may be null)
    w1 = rng.normal(size=s[7])
    w_ptr[1] = w1.ctypes.data
    assert tr._c("eval")(tr._h, (ctypes.c_uint8 * 2)(1, 1), w_ptr, f.ctypes.data, g_ptr) == 0
    assert same_bits(f[1], g[1], *(v[0] for v in _trainer(s).eval([w1])))


@pytest.mark.parametrize("L,n_seqs", [(2, 1), (3, 256), (32, 257), (7, 600)])
def test_scratch_bytes_is_the_formula(L, n_seqs):
    from gecco_amd import train

    rng = np.random.default_rng(L)
    s = _with_sequences(rng, L, n_seqs, hi=4)
    n_items = int(s[0][-1])
    expect = 8 * (2 * n_items * L + (-(-n_seqs // (THREADS // _group(L))) + REDUCE_SLABS) * (1 + L * L))
    tr = _trainer(s)
    assert tr.scratch_bytes(0) == tr.scratch_bytes(-1) == expect
    ts = train.TrainingSet(seq_ptr=s[0], labels_=list(range(L)), window=None)
    assert train._sequences_scratch_bytes(ts) == expect


# ---------------------------------------------------------------- fits
def _named(rng, L, n_seqs, A=20, lo=3, hi=30, stay=0.9, first=()):
    lengths = list(first) + [int(x) for x in rng.integers(lo, hi + 1, size=n_seqs - len(first))]
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, lengths, A, L, stay=stay)
    X, y = [], []
    for s in range(len(seq_ptr) - 1):
        X.append([[f"a{a}" for a in attr_id[item_ptr[i]:item_ptr[i + 1]]] for i in range(seq_ptr[s], seq_ptr[s + 1])])
        y.append([f"type{v}" for v in labels[seq_ptr[s]:seq_ptr[s + 1]]])
    return X, y


def _fit_set(seed, L=3, n_seqs=40, window=None):
    from gecco_amd import train

    X, y = _named(np.random.default_rng(seed), L, n_seqs)
    ts = train.build_training_set(X, y, window, None if window is None else 1, max_labels=max(L, 2))
    assert ts.num_labels == L
    return ts


def _np_fg(ts, c2):
    A, L = len(ts.attrs_), ts.num_labels

    def fg(w):
        f, g, _ = objective_sequences(ts.seq_ptr, ts.item_ptr, ts.attr_id, ts.labels, A, L, ts.state_fid.ravel(),
                                      ts.trans_fid.ravel(), w)
        return f + c2 * float(w @ w), g + 2 * c2 * w

    return fg


def test_fit_l2_reaches_the_scipy_optimum():
    import scipy.optimize
    from gecco_amd import train

    ts = _fit_set(11)
    assert ts.window is None
    params = train.trainer_params({"c1": 0.0, "c2": 0.15, "epsilon": 1e-10, "delta": 0.0})
    res = train.fit_training_set(ts, params)
    fg = _np_fg(ts, 0.15)
    ref = scipy.optimize.minimize(fg, np.zeros(ts.num_features), jac=True, method="L-BFGS-B",
                                  options={"ftol": 1e-15, "gtol": 1e-10, "maxiter": 10000})
    f_ours = fg(res.x)[0]
    print(f"f = {f_ours!r}, scipy {ref.fun!r} after {ref.nfev} evaluations; max |x - scipy| = {np.abs(res.x - ref.x).max():.3g}")
    assert abs(f_ours - ref.fun) <= 1e-8 * abs(ref.fun), (f_ours, ref.fun, res)
    assert np.abs(res.x - ref.x).max() <= 1e-4


def test_fit_l1_satisfies_kkt():
    from gecco_amd import train

    ts = _fit_set(12)
    c1 = 0.5
    params = train.trainer_params({"c1": c1, "c2": 0.0, "epsilon": 1e-10, "delta": 0.0})
    res = train.fit_training_set(ts, params)
    _, g = _np_fg(ts, 0.0)(res.x)
    w = res.x
    nz = w != 0
    assert nz.any() and (~nz).any()
    print(f"KKT: max |g + c1 sign(w)| = {np.abs(g[nz] + c1 * np.sign(w[nz])).max():.3g}, max |g| at 0 = {np.abs(g[~nz]).max():.3g}")
    assert np.abs(g[nz] + c1 * np.sign(w[nz])).max() <= 1e-5
    assert np.abs(g[~nz]).max() <= c1 + 1e-5


def test_fit_training_sets_and_grid_return_the_lone_fits(monkeypatch):
    """Whole-sequence sets of three, two and three labels, in ``fit_grid`` with a windowed 2-label set between them:
    every result is the lone fit's, bit for bit, also when a scratch budget splits the whole-sequence fits in groups."""
    from gecco_amd import _native, train

    sets = [_fit_set(21), _fit_set(22, L=2), _fit_set(23, L=2, window=3), _fit_set(24)]
    whole = [0, 1, 3]
    params = train.trainer_params({"c1": 0.05, "c2": 0.1, "max_iterations": 25})
    lone = [train.fit_training_set(ts, params) for ts in sets]
    need = [train._sequences_scratch_bytes(sets[k]) for k in whole]
    assert need == [_native.TrainerSequences([sets[k].native_args()]).scratch_bytes(0) for k in whole]
    created = []

    class Counting(_native.TrainerSequences):
        def __init__(self, problems, device=0):
            created.append(len(problems))
            super().__init__(problems, device=device)

    monkeypatch.setattr(_native, "TrainerSequences", Counting)
    grid = [(k, params) for k in range(4)]
    with pytest.raises(ValueError, match="same window and step"):
        train.fit_training_sets(sets, params)
    for fit, expect, groups in (
            (lambda: train.fit_training_sets([sets[k] for k in whole], params), [lone[k] for k in whole], [3]),
            (lambda: train.fit_grid(sets, grid), lone, [3]),
            (lambda: train.fit_grid(sets, grid, scratch_budget_bytes=need[0] + need[1]), lone, [2, 1]),
            (lambda: train.fit_grid(sets, grid, scratch_budget_bytes=1), lone, [1, 1, 1])):
        res = fit()
        assert created == groups
        del created[:]
        assert len(res) == len(expect)
        for a, b in zip(res, expect):
            assert a.x.tobytes() == b.x.tobytes() and a.n_iter == b.n_iter and a.status == b.status
            assert np.float64(a.f).tobytes() == np.float64(b.f).tobytes()
    assert all(r.n_iter > 0 for r in lone)


# ---------------------------------------------------------------- the estimator end to end
def test_sequence_crf_without_a_window_end_to_end(tmp_path):
    from oracle import crf_oracle as orc
    from oracle import lcrf
    from gecco_amd import _native, train
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(808)
    X, y = _named(rng, 4, 40, lo=1, hi=30, stay=0.85, first=(3, 1, 4, 2))
    assert sum(len(xs) < 5 for xs in X) >= 4
    X[0][0] = X[0][0] + X[0][0][:1]  # a duplicate attribute collapses
    crf = SequenceCRF(window_size=None, c1=0.05, c2=0.1, max_iterations=40).fit(X, y)
    ts = train.build_training_set([[list(dict.fromkeys(it)) for it in xs] for xs in X], y, None, None, max_labels=32)
    assert crf.classes_ == ts.labels_ and len(crf.classes_) == 4
    x = crf.training_result_.x
    assert crf.training_result_.n_iter > 0 and len(x) == ts.num_features
    S = len(ts.state_attr)
    exp_state = {(ts.attrs_[a], ts.labels_[l]): x[k] for k, (a, l) in enumerate(zip(ts.state_attr, ts.state_label)) if x[k] != 0}
    exp_trans = {(ts.labels_[i], ts.labels_[j]): x[S + k] for k, (i, j) in enumerate(zip(ts.trans_src, ts.trans_dst))
                 if x[S + k] != 0}
    assert len(exp_state) > 0 and len(exp_trans) > 0
    assert crf.state_features_ == exp_state and crf.transition_features_ == exp_trans

    blob = crf.to_bytes()
    crf.save(tmp_path / "model.crfsuite")
    for other in (SequenceCRF.from_bytes(blob, window_size=None), SequenceCRF.load(tmp_path / "model.crfsuite", window_size=None)):
        assert other.window_size is None and other.classes_ == crf.classes_ and other.attributes_ == crf.attributes_
        assert other.state_features_ == crf.state_features_ and other.transition_features_ == crf.transition_features_
        assert other.to_bytes() == blob
    loaded = SequenceCRF.from_bytes(blob, window_size=None)
    m = lcrf.parse_lcrf(blob)
    assert m["labels"] == crf.classes_ and m["attrs"] == crf.attributes_

    Xt, _ = _named(np.random.default_rng(909), 4, 8, lo=1, hi=40, first=(1, 2))
    Xt[1][0] = Xt[1][0] + ["never seen"]  # unknown names are dropped
    index = {a: i for i, a in enumerate(m["attrs"])}
    seq_ptr, item_ptr, attr = [0], [0], []
    for xs in Xt:
        for it in xs:
            attr.extend(index[a] for a in dict.fromkeys(it) if a in index)
            item_ptr.append(len(attr))
        seq_ptr.append(len(item_ptr) - 1)
    seq_ptr, item_ptr, attr = (np.array(v, dtype=np.int32) for v in (seq_ptr, item_ptr, attr))
    exp_marg, _ = orc.full_marginals(m["state"], m["trans"], seq_ptr, item_ptr, attr)
    exp_y, _ = orc.viterbi(m["state"], m["trans"], seq_ptr, item_ptr, attr)
    marg = loaded.predict_marginals(Xt)
    assert [len(a) for a in marg] == [len(xs) for xs in Xt] and all(a.shape[1] == 4 for a in marg)
    assert np.abs(np.concatenate(marg) - exp_marg).max() <= 1e-12
    got_y = loaded.predict(Xt)
    assert [lab for ys in got_y for lab in ys] == [m["labels"][k] for k in exp_y.tolist()]
    with pytest.raises(ValueError, match="has no window"):
        loaded.predict_windowed(Xt, crf.classes_[0])

    # the log-space training kernel against the scaled-scan inference kernels: the likelihood of the training data
    ll = loaded.log_likelihood(X, y)
    assert ll.shape == (len(X),) and np.all(ll < 0)
    f, _ = _native.TrainerSequences([ts.native_args()]).eval([x])
    tol_f, _ = objective_sequences_tolerances(ts.seq_ptr, ts.item_ptr, ts.attr_id, ts.labels, len(ts.attrs_), 4,
                                              ts.state_fid.ravel(), ts.trans_fid.ravel(), x)
    print(f"-sum(log_likelihood) = {-ll.sum()!r}, trainer f = {f[0]!r}: difference {abs(-ll.sum() - f[0]):.3g} (bound {tol_f:.3g})")
    assert abs(-ll.sum() - f[0]) <= tol_f
    # per sequence, and with an empty sequence and an unknown attribute in between
    one = loaded.log_likelihood([X[3], [], [it + ["never seen"] for it in X[5]]], [y[3], [], y[5]])
    assert one[1] == 0.0 and abs(one[0] - ll[3]) <= 1e-12 * abs(ll[3]) and abs(one[2] - ll[5]) <= 1e-12 * abs(ll[5])
    with pytest.raises(ValueError, match="unknown label"):
        loaded.log_likelihood([X[3]], [["no such type"] * len(X[3])])
    # a windowed model has the same method
    assert np.allclose(SequenceCRF.from_bytes(blob, window_size=5).log_likelihood(X[:4], y[:4]), ll[:4], rtol=1e-12, atol=0)
