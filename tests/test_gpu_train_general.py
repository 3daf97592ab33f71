"""Training with 2 to 32 labels on the device: ``gecco_crf_trainer_general_eval`` against the independent numpy
yardstick (tests/train_objective_labels.py), its bit contracts, its refusals, the fits through it against scipy's
optimum of the yardstick, and ``SequenceCRF`` end to end."""
import numpy as np
import pytest

from tests.train_objective_labels import (count_windows, labelled_sequences, objective, objective_tolerances, same_bits,
                                          training_set, window_starts)

pytestmark = pytest.mark.gpu

# the window kernel's geometry (csrc/crf_train_general.hip): 256 threads as groups of G = next power of two >= L
# lanes, 256 / G windows side by side; a workgroup owns kTrainGenWindowsPerBlock windows, and the first stage of the
# block sums has kTrainGenReduceSlabs slabs
THREADS = 256
WINDOWS_PER_WORKGROUP = 128
REDUCE_SLABS = 32


def _group(L):
    G = 2
    while G < L:
        G *= 2
    return G


def _general(*problems):
    from gecco_amd import _native

    return _native.TrainerGeneral(list(problems))


def _labels_of(s):
    return np.asarray(s[5]).size // s[4]


def _reference(s, w, details=False):
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K, W, step = s
    return objective(seq_ptr, item_ptr, attr_id, labels, A, _labels_of(s), W, step, sfid, tfid, w, details=details)


def check_strict(tr, k, s, w, ws=None, active=None):
    """Problem k of `tr` at `w` within the project's bounds of the yardstick (tests/test_gpu_train.py), and the same
    bytes from a second evaluation.  Returns (f, g)."""
    n = len(tr)
    ws = [w if j == k else None for j in range(n)] if ws is None else ws
    active = [j == k for j in range(n)] if active is None else active
    f, g = tr.eval(ws, active)
    ef, eg, nw = _reference(s, w)
    assert tr.num_windows(k) == nw
    print(f"L={_labels_of(s)} W={s[8]} step={s[9]}: |f - ref| / |ref| = {abs(f[k] - ef) / max(abs(ef), 1e-300):.3g}, "
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
    ef, eg, nw, d = _reference(s, w, details=True)
    assert np.isfinite(ef) and np.all(np.isfinite(eg))
    assert np.isfinite(f[k]) and np.all(np.isfinite(g[k])), (f[k], int(np.count_nonzero(~np.isfinite(g[k]))))
    tol_f, tol_g = objective_tolerances(s[0], s[1], s[2], _labels_of(s), s[8], s[9], s[5], s[6], w, d)
    err = np.abs(g[k] - eg)
    print(f"L={_labels_of(s)} W={s[8]}: |f - ref| = {abs(f[k] - ef):.3g} (bound {tol_f:.3g}), "
          f"max |g - ref| / bound = {(err / np.maximum(tol_g, 1e-300)).max():.3g}")
    assert abs(f[k] - ef) <= tol_f, (f[k], ef, abs(f[k] - ef), tol_f)
    assert np.all(err <= tol_g), (int(np.argmax(err / np.maximum(tol_g, 1e-300))), float(err.max()))


# ---------------------------------------------------------------- objective and gradient against the yardstick
@pytest.mark.parametrize("W,step", [(1, 1), (2, 1), (5, 3), (20, 1), (32, 1), (32, 3)])
@pytest.mark.parametrize("L", [2, 3, 5, 8, 9, 16, 17, 32])
def test_eval_matches_the_yardstick(L, W, step):
    rng = np.random.default_rng(5000 + 101 * L + 37 * W + step)
    s = training_set(rng, L, W, step)  # 60 attributes, 25 + 3 sequences, a tenth of the pairs without a feature
    seq_ptr, item_ptr, labels = s[0], s[1], s[3]
    assert np.any(np.diff(item_ptr) == 0) and np.any(s[5] < 0) and np.any(s[6] < 0)
    assert any(len(set(labels[i0:i0 + W].tolist())) < L for i0 in window_starts(seq_ptr, W, step))  # a label is absent
    tr = _general(s)
    assert len(tr) == 1 and tr.num_windows(0) == count_windows(seq_ptr, W, step)
    check_strict(tr, 0, s, rng.normal(0, 1.5, size=s[7]))
    check_strict(tr, 0, s, np.zeros(s[7]))


# ---------------------------------------------------------------- window-count edges
def _with_windows(rng, L, W, n_win, A=20):
    """A problem of exactly n_win windows (step 1): one sequence of W + n_win - 1 items."""
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, [W + n_win - 1], A, L, stay=0.8)
    K = A * L + L * L
    return (seq_ptr, item_ptr, attr_id, labels, A, np.arange(A * L, dtype=np.int32),
            A * L + np.arange(L * L, dtype=np.int32), K, W, 1)


@pytest.mark.parametrize("L", [2, 3, 9, 32])
def test_window_count_edges(L):
    """1 window; one more than the windows side by side in a workgroup (256 / G); exactly and one more than a
    workgroup's windows."""
    rng = np.random.default_rng(600 + L)
    for n_win in (1, THREADS // _group(L) + 1, WINDOWS_PER_WORKGROUP, WINDOWS_PER_WORKGROUP + 1):
        s = _with_windows(rng, L, 4, n_win)
        tr = _general(s)
        assert tr.num_windows(0) == n_win
        check_strict(tr, 0, s, rng.normal(0, 1.5, size=s[7]))


def test_more_workgroups_than_slabs():
    """More than kTrainGenReduceSlabs workgroups, not a multiple of it: slabs of several blocks and empty slabs."""
    rng = np.random.default_rng(77)
    n_win = WINDOWS_PER_WORKGROUP * (2 * REDUCE_SLABS + 7) + 5
    s = _with_windows(rng, 3, 5, n_win)
    check_strict(_general(s), 0, s, rng.normal(0, 1.5, size=s[7]))


def test_problem_without_sequences_beside_a_normal_one():
    rng = np.random.default_rng(8)
    s = training_set(rng, 5, 6, 2)
    A, L = 4, 3
    empty = (np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32),
             np.zeros(0, dtype=np.int32), A, np.arange(A * L, dtype=np.int32), A * L + np.arange(L * L, dtype=np.int32),
             A * L + L * L, 5, 1)
    w = rng.normal(0, 1.5, size=s[7])
    lone = _general(s)
    f0, g0 = lone.eval([w])
    for problems, k in (((empty, s), 1), ((s, empty), 0)):
        tr = _general(*problems)
        assert tr.num_windows(1 - k) == 0
        ws = [None, None]
        ws[k], ws[1 - k] = w, rng.normal(0, 1.5, size=empty[7])
        f, g = tr.eval(ws)
        assert f[1 - k] == 0.0 and np.all(g[1 - k] == 0.0) and g[1 - k].shape == (empty[7],)
        assert same_bits(f[k], g[k], f0[0], g0[0])
    f, g = _general(empty).eval([np.ones(empty[7])])
    assert f[0] == 0.0 and np.all(g[0] == 0.0)


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


@pytest.mark.parametrize("scale", [100.0, 1000.0])
@pytest.mark.parametrize("W", [5, 20])
@pytest.mark.parametrize("L", [3, 9])
def test_extreme_weights(L, W, scale):
    rng = np.random.default_rng(9000 + 10 * L + W)
    s = training_set(rng, L, W, 1)
    tr = _general(s)
    w = scale * rng.normal(0, 1.5, size=s[7])
    check_bounds(tr, 0, s, w)
    check_bounds(tr, 0, s, _plant(s, w, rng))
    check_bounds(tr, 0, s, _plant(s, rng.normal(0, 1.5, size=s[7]), rng))


@pytest.mark.parametrize("W", [5, 20])
@pytest.mark.parametrize("L", [3, 9])
def test_state_gap_flips_sign_inside_a_window(L, W):
    """Blocks of W / 2 + 1 items, block b with attribute b on every item and label b % L: attribute 0 weighs +800 on
    label 0 and attribute 1 +800 on label 1, so in the windows across their edge label 1 is 800 nats down and then
    800 nats up; the transition the gold path takes there weighs -800, another one +720."""
    n_blocks, blen = 6, W // 2 + 1
    A = n_blocks
    attr_id = np.repeat(np.arange(n_blocks), blen).astype(np.int32)
    n = len(attr_id)
    labels = (attr_id % L).astype(np.int32)
    s = (np.array([0, n], dtype=np.int32), np.arange(n + 1, dtype=np.int32), attr_id, labels, A,
         np.arange(A * L, dtype=np.int32), A * L + np.arange(L * L, dtype=np.int32), A * L + L * L, W, 1)
    rng = np.random.default_rng(L * W)
    w = rng.normal(0, 0.5, size=s[7])
    w[0 * L + 0] = 800.0
    w[1 * L + 1] = 800.0
    w[A * L + 0 * L + 1] = -800.0
    w[A * L + 2 * L + 0] = 720.0
    tr = _general(s)
    check_bounds(tr, 0, s, w)
    check_strict(tr, 0, s, np.sign(w) * 0.7)


# ---------------------------------------------------------------- several problems at once
BATCH = [(2, 20, 1, 25), (3, 5, 3, 8), (8, 32, 3, 12), (9, 2, 1, 30), (32, 20, 1, 5)]  # (L, W, step, sequences)


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(31)
    sets = [training_set(rng, L, W, step, n_seqs=n) for L, W, step, n in BATCH]
    ws = [rng.normal(0, 1.5, size=s[7]) for s in sets]
    lone = []
    for s, w in zip(sets, ws):
        f, g = _general(s).eval([w])
        lone.append((f[0], g[0]))
    return sets, ws, lone


def test_batch_masks_and_lone_bits(batch):
    sets, ws, lone = batch
    tr = _general(*sets)
    assert len(tr) == 5
    assert [tr.num_windows(k) for k in range(5)] == [count_windows(s[0], s[8], s[9]) for s in sets]
    assert tr.num_windows(5) == -1 and tr.scratch_bytes(5) == -1
    assert tr.scratch_bytes(-1) == sum(tr.scratch_bytes(k) for k in range(5))
    masks = [[True] * 5, [False] * 5, [True, False, True, False, True], [False, True, False, True, False],
             [False, False, False, False, True], [True, False, False, False, False], [False, True, True, True, False]]
    for mask in masks:
        f = np.full(5, -7.25)
        g = [np.full(s[7], -3.5) for s in sets]
        tr.eval([w if m else None for w, m in zip(ws, mask)], mask, f, g)
        for k, m in enumerate(mask):
            if m:
                assert same_bits(f[k], g[k], *lone[k]), (mask, k)
            else:
                assert f[k] == -7.25 and np.all(g[k] == -3.5), (mask, k)
    for k, s in enumerate(sets):
        check_strict(tr, k, s, ws[k])


def test_two_labels_agree_with_the_two_label_trainer(batch):
    from gecco_amd import _native

    sets, ws, lone = batch
    s = sets[0]
    f2, g2 = _native.Trainer(s[0], s[1], s[2], s[3], s[4], s[8], s[9], s[5], s[6], s[7]).eval(ws[0])
    f, g = lone[0]
    assert abs(f - f2) <= 1e-12 * abs(f2)
    assert np.all(np.abs(g - g2) <= 1e-9 * (1 + np.abs(g2)))


# ---------------------------------------------------------------- refusals
def _tiny(L, W=3, label=0, n=6, A=2):
    return ([0, n], np.zeros(n + 1, dtype=np.int32), [], np.full(n, label, dtype=np.int32), A, [-1] * (A * L), [-1] * (L * L), 0, W,
            1)


def test_refusals():
    from gecco_amd import _native

    for L in (1, 33):
        with pytest.raises(_native.NativeError, match="models of 2 to 32 labels") as e:
            _general(_tiny(L))
        assert e.value.code == _native.EUNSUPPORTED and "problem 0" in str(e.value)
    with pytest.raises(_native.NativeError, match="problem 1: .*windows of 1 to 32") as e:
        _general(_tiny(3), _tiny(3, W=33, n=40))
    assert e.value.code == _native.EUNSUPPORTED
    with pytest.raises(ValueError, match=r"problem 0: trainer: labels must lie in \[0, num_labels\)"):
        _general(_tiny(3, label=3))
    _general(_tiny(3, label=2))
    bad = list(_tiny(3))
    bad[6] = [-1] * 4
    with pytest.raises(ValueError, match="trans_fid must have L \\* L = 9 entries"):
        _general(tuple(bad))
    with pytest.raises(ValueError, match="fewer items than the window"):
        _general(_tiny(3, W=7))
    with pytest.raises(ValueError, match="window and a step"):
        _general(_tiny(3)[:8])


def test_scratch_stays_below_one_block_per_window():
    s = training_set(np.random.default_rng(3220), 32, 20, 1)
    tr = _general(s)
    nw = tr.num_windows(0)
    assert nw > 0 and 0 < tr.scratch_bytes(0) < 8 * 32 * 32 * nw


# ---------------------------------------------------------------- fits
def _fit_set(seed, L=4, W=5, A=40, n_items=1200):
    from gecco_amd import train

    rng = np.random.default_rng(seed)
    lengths = [int(x) for x in rng.integers(W + 5, 70, size=n_items // 37)]
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, lengths, A, L, stay=0.9)
    seqs, labs = [], []
    for s in range(len(seq_ptr) - 1):
        seqs.append([[f"a{a}" for a in attr_id[item_ptr[i]:item_ptr[i + 1]]] for i in range(seq_ptr[s], seq_ptr[s + 1])])
        labs.append([f"y{y}" for y in labels[seq_ptr[s]:seq_ptr[s + 1]]])
    ts = train.build_training_set(seqs, labs, W, 1, max_labels=max(L, 2))
    assert ts.num_labels == L
    return ts


def _np_fg(ts, c2):
    A, L = len(ts.attrs_), ts.num_labels

    def fg(w):
        f, g, _ = objective(ts.seq_ptr, ts.item_ptr, ts.attr_id, ts.labels, A, L, ts.window, ts.step, ts.state_fid.ravel(),
                            ts.trans_fid.ravel(), w)
        return f + c2 * float(w @ w), g + 2 * c2 * w

    return fg


def test_fit_l2_reaches_the_scipy_optimum():
    import scipy.optimize
    from gecco_amd import train

    ts = _fit_set(11)
    params = train.trainer_params({"c1": 0.0, "c2": 0.15, "epsilon": 1e-10, "delta": 0.0})
    res = train.fit_training_set(ts, params)
    fg = _np_fg(ts, 0.15)
    ref = scipy.optimize.minimize(fg, np.zeros(ts.num_features), jac=True, method="L-BFGS-B",
                                  options={"ftol": 1e-15, "gtol": 1e-10, "maxiter": 10000})
    f_ours = fg(res.x)[0]
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
    assert np.abs(g[nz] + c1 * np.sign(w[nz])).max() <= 1e-5
    assert np.abs(g[~nz]).max() <= c1 + 1e-5


def test_fit_training_sets_and_grid_return_the_lone_fits(monkeypatch):
    """Three 4-label sets and a 2-label one between them: every result is the lone fit's, bit for bit, also when a
    scratch budget makes ``fit_grid`` run the many-label fits in groups (here of two and of one)."""
    from gecco_amd import _native, train

    sets = [_fit_set(21), _fit_set(22, L=2), _fit_set(23), _fit_set(24)]
    params = train.trainer_params({"c1": 0.05, "c2": 0.1, "max_iterations": 25})
    lone = [train.fit_training_set(ts, params) for ts in sets]
    need = [train._general_scratch_bytes(sets[k]) for k in (0, 2, 3)]
    assert need == [_native.TrainerGeneral([sets[k].native_args()]).scratch_bytes(0) for k in (0, 2, 3)]
    created = []

    class Counting(_native.TrainerGeneral):
        def __init__(self, problems, device=0):
            created.append(len(problems))
            super().__init__(problems, device=device)

    monkeypatch.setattr(_native, "TrainerGeneral", Counting)
    grid = [(k, params) for k in range(4)]
    for fit, groups in ((lambda: train.fit_training_sets(sets, params), [3]), (lambda: train.fit_grid(sets, grid), [3]),
                        (lambda: train.fit_grid(sets, grid, scratch_budget_bytes=need[0] + need[1]), [2, 1]),
                        (lambda: train.fit_grid(sets, grid, scratch_budget_bytes=1), [1, 1, 1])):
        res = fit()
        assert created == groups
        del created[:]
        for a, b in zip(res, lone):
            assert a.x.tobytes() == b.x.tobytes() and a.n_iter == b.n_iter and a.status == b.status
            assert np.float64(a.f).tobytes() == np.float64(b.f).tobytes()
    assert lone[0].n_iter > 0


# ---------------------------------------------------------------- the estimator end to end
def _named(rng, L, n_seqs, A=30, lo=12, hi=50):
    lengths = [int(x) for x in rng.integers(lo, hi, size=n_seqs)]
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, lengths, A, L, stay=0.85)
    X, y = [], []
    for s in range(len(seq_ptr) - 1):
        X.append([[f"a{a}" for a in attr_id[item_ptr[i]:item_ptr[i + 1]]] for i in range(seq_ptr[s], seq_ptr[s + 1])])
        y.append([f"type{v}" for v in labels[seq_ptr[s]:seq_ptr[s + 1]]])
    return X, y


def test_sequence_crf_end_to_end(tmp_path):
    from oracle import crf_oracle as orc
    from oracle import lcrf
    from gecco_amd import _native, train
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(808)
    X, y = _named(rng, 8, 40)
    X[0][0] = X[0][0] + X[0][0][:1]  # a duplicate attribute collapses
    crf = SequenceCRF(window_size=5, c1=0.05, c2=0.1, max_iterations=40).fit(X, y)
    ts = train.build_training_set([[list(dict.fromkeys(it)) for it in xs] for xs in X], y, 5, 1, max_labels=32)
    assert crf.classes_ == ts.labels_ and len(crf.classes_) == 8
    x = crf.training_result_.x
    assert crf.training_result_.n_iter > 0 and len(x) == ts.num_features
    S = len(ts.state_attr)
    exp_state = {(ts.attrs_[a], ts.labels_[l]): x[k] for k, (a, l) in enumerate(zip(ts.state_attr, ts.state_label)) if x[k] != 0}
    exp_trans = {(ts.labels_[i], ts.labels_[j]): x[S + k] for k, (i, j) in enumerate(zip(ts.trans_src, ts.trans_dst))
                 if x[S + k] != 0}
    assert len(exp_state) > 0 and len(exp_trans) > 0
    assert crf.state_features_ == exp_state and crf.transition_features_ == exp_trans
    assert set(crf.attributes_) == {a for a, _ in exp_state}

    blob = crf.to_bytes()
    crf.save(tmp_path / "model.crfsuite")
    for other in (SequenceCRF.from_bytes(blob, window_size=5), SequenceCRF.load(tmp_path / "model.crfsuite", window_size=5)):
        assert other.classes_ == crf.classes_ and other.attributes_ == crf.attributes_
        assert other.state_features_ == crf.state_features_ and other.transition_features_ == crf.transition_features_
        assert other.to_bytes() == blob
    loaded = SequenceCRF.from_bytes(blob, window_size=5)
    m = lcrf.parse_lcrf(blob)
    native = _native.Model.from_lcrf(blob)
    assert m["labels"] == crf.classes_ == native.labels() and m["attrs"] == crf.attributes_ == native.attrs()

    Xt, _ = _named(np.random.default_rng(909), 8, 6, lo=3, hi=40)
    Xt[1][2] = Xt[1][2] + ["never seen"]  # unknown names are dropped
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
    assert [len(a) for a in marg] == [len(xs) for xs in Xt] and all(a.shape[1] == 8 for a in marg)
    assert np.abs(np.concatenate(marg) - exp_marg).max() <= 1e-12
    got_y = loaded.predict(Xt)
    assert [lab for ys in got_y for lab in ys] == [m["labels"][k] for k in exp_y.tolist()]
    label = crf.classes_[3]
    exp_p = orc.windowed_marginals(m["state"], m["trans"], seq_ptr, item_ptr, attr, 5, 1, 3, True)
    assert np.abs(np.concatenate(loaded.predict_windowed(Xt, label)) - exp_p).max() <= 1e-12
    with pytest.raises(ValueError, match="unknown label"):
        loaded.predict_windowed(Xt, "no such type")


def test_sequence_crf_with_two_labels_takes_the_two_label_path():
    from gecco_amd import train
    from gecco_amd.sequence import SequenceCRF

    X, y = _named(np.random.default_rng(202), 2, 25)
    crf = SequenceCRF(window_size=5, c2=0.2, max_iterations=30).fit(X, y)
    ts = train.build_training_set(X, y, 5, 1)
    res = train.fit_training_set(ts, train.trainer_params({"c2": 0.2, "max_iterations": 30}))
    assert crf.training_result_.x.tobytes() == res.x.tobytes() and crf.training_result_.n_iter == res.n_iter > 0
    assert crf.to_bytes() == train.model_blob(ts, res.x)
