"""Cost-sensitive training on the device: the ``*_create_weighted`` trainers (sequence weights and a label-cost matrix)
against the independent numpy yardstick (tests/train_objective_weighted.py), their exact-scaling, zero-weight and bit
contracts, their refusals, and the fits and front ends through them."""
import numpy as np
import pytest

from tests.train_objective_labels import labelled_sequences, same_bits, training_set
from tests.train_objective_sequences import sequences_problem, subproblem
from tests.train_objective_weighted import augmented, label_count, objective_weighted, weighted_tolerances

pytestmark = pytest.mark.gpu

THREADS = 256
WINDOWS_PER_WORKGROUP = 128
REDUCE_SLABS = 32


def _group(L):
    G = 2
    while G < L:
        G *= 2
    return G


def _trainer(problems, **kw):
    from gecco_amd import _native

    whole = len(problems[0]) == 8
    return (_native.TrainerSequences if whole else _native.TrainerGeneral)(list(problems), **kw)


def _costs(rng, L):
    """Asymmetric, entries in [0, 2], zero diagonal."""
    C = rng.uniform(0.0, 2.0, size=(L, L))
    C[np.arange(L), np.arange(L)] = 0.0
    return C


def _weights(rng, n, lo=0.25, hi=4.0):
    wts = rng.uniform(lo, hi, size=n)
    assert len(set(wts.tolist())) == n
    return wts


def check_strict(tr, k, s, wts, C, w):
    """Problem k at `w` within the project's strict bounds of the yardstick (`check_strict` of
    tests/test_gpu_train_general.py), and the same bytes from a second evaluation."""
    n = len(tr)
    ws, active = [w if j == k else None for j in range(n)], [j == k for j in range(n)]
    f, g = tr.eval(ws, active)
    ef, eg, ni = objective_weighted(s, wts, C, w)
    assert tr.num_windows(k) == ni
    print(f"L={label_count(s)} {'W=%d step=%d' % (s[8], s[9]) if len(s) == 10 else 'whole'}: |f - ref| / |ref| = "
          f"{abs(f[k] - ef) / max(abs(ef), 1e-300):.3g}, max |g - ref| / (1 + |ref|) = "
          f"{(np.abs(g[k] - eg) / (1 + np.abs(eg))).max() if len(eg) else 0.0:.3g}")
    assert abs(f[k] - ef) <= 1e-12 * abs(ef), (f[k], ef)
    assert np.all(np.abs(g[k] - eg) <= 1e-9 * (1 + np.abs(eg))), np.abs(g[k] - eg).max()
    f2, g2 = tr.eval(ws, active)
    assert same_bits(f[k], g[k], f2[k], g2[k])
    return f[k], g[k]


def check_bounds(tr, s, wts, C, w):
    f, g = tr.eval([w])
    ef, eg, _ = objective_weighted(s, wts, C, w)
    assert np.isfinite(ef) and np.all(np.isfinite(eg)) and np.isfinite(f[0]) and np.all(np.isfinite(g[0]))
    tol_f, tol_g = weighted_tolerances(s, wts, C, w)
    err = np.abs(g[0] - eg)
    print(f"L={label_count(s)}: |f - ref| = {abs(f[0] - ef):.3g} (bound {tol_f:.3g}), max |g - ref| / bound = "
          f"{(err / np.maximum(tol_g, 1e-300)).max():.3g}")
    assert abs(f[0] - ef) <= tol_f, (f[0], ef, tol_f)
    assert np.all(err <= tol_g), (int(np.argmax(err / np.maximum(tol_g, 1e-300))), float(err.max()))


# ---------------------------------------------------------------- 1. against the yardstick
@pytest.mark.parametrize("W,step", [(1, 1), (2, 1), (5, 3), (32, 1)])
@pytest.mark.parametrize("L", [2, 3, 5, 32])
def test_windows_match_the_yardstick(L, W, step):
    rng = np.random.default_rng(7000 + 101 * L + 37 * W + step)
    s = training_set(rng, L, W, step)
    wts, C = _weights(rng, len(s[0]) - 1), _costs(rng, L)
    tr = _trainer([s], weights=[wts], costs=[C])
    check_strict(tr, 0, s, wts, C, rng.normal(0, 1.5, size=s[7]))
    check_strict(tr, 0, s, wts, C, np.zeros(s[7]))
    # weights alone, and costs alone (weights of 1)
    check_strict(_trainer([s], weights=[wts]), 0, s, wts, None, rng.normal(0, 1.5, size=s[7]))
    check_strict(_trainer([s], costs=[C]), 0, s, None, C, rng.normal(0, 1.5, size=s[7]))


def _shuffled_lengths(rng, L):
    """256 / G + 1 sequences (a second workgroup), lengths 1 and 2 among them, in a shuffled length order."""
    n = THREADS // _group(L) + 1
    lengths = [1, 2, 1, 2] + [int(x) for x in rng.integers(1, 40, size=n - 4)]
    rng.shuffle(lengths)
    assert lengths != sorted(lengths, reverse=True)
    return lengths


@pytest.mark.parametrize("L", [2, 3, 5, 32])
def test_whole_sequences_match_the_yardstick(L):
    rng = np.random.default_rng(7100 + L)
    s = sequences_problem(rng, L, _shuffled_lengths(rng, L))
    wts, C = _weights(rng, len(s[0]) - 1), _costs(rng, L)
    tr = _trainer([s], weights=[wts], costs=[C])
    check_strict(tr, 0, s, wts, C, rng.normal(0, 1.5, size=s[7]))
    check_strict(tr, 0, s, wts, C, np.zeros(s[7]))


@pytest.mark.parametrize("L", [3, 32])
def test_extreme_weights(L):
    """Model weights scaled by 40 (the pattern of test_extreme_weights of tests/test_gpu_train_general.py), within the
    restated derived bounds."""
    rng = np.random.default_rng(7200 + L)
    s = training_set(rng, L, 5, 1)
    wts, C = _weights(rng, len(s[0]) - 1), _costs(rng, L)
    check_bounds(_trainer([s], weights=[wts], costs=[C]), s, wts, C, 40.0 * rng.normal(0, 1.5, size=s[7]))
    q = sequences_problem(rng, L, _shuffled_lengths(rng, L))
    wq = _weights(rng, len(q[0]) - 1)
    check_bounds(_trainer([q], weights=[wq], costs=[C]), q, wq, C, 40.0 * rng.normal(0, 1.5, size=q[7]))


# ---------------------------------------------------------------- 2. workgroup edges
def _full_features(seq_ptr, item_ptr, attr_id, labels, A, L, *ws):
    return (seq_ptr, item_ptr, attr_id, labels, A, np.arange(A * L, dtype=np.int32), A * L + np.arange(L * L, dtype=np.int32),
            A * L + L * L, *ws)


@pytest.mark.parametrize("L", [2, 32])
def test_workgroup_edges(L):
    """One sequence of 129 windows (W = 4); two sequences of different weights whose windows straddle window 128."""
    rng = np.random.default_rng(7300 + L)
    W, A = 4, 20
    C = _costs(rng, L)
    for lengths, wts in (([W + 128], [1.75]), ([W + 99, W + 59], [0.5, 3.25]), ([W + 127, W], [2.5, 0.75])):
        s = _full_features(*labelled_sequences(rng, lengths, A, L, stay=0.8), A, L, W, 1)
        wts = np.array(wts)
        tr = _trainer([s], weights=[wts], costs=[C])
        assert tr.num_windows(0) == sum(n - W + 1 for n in lengths) > WINDOWS_PER_WORKGROUP
        check_strict(tr, 0, s, wts, C, rng.normal(0, 1.5, size=s[7]))


# ---------------------------------------------------------------- 3. exact scaling
@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("L", [2, 3, 32])
def test_a_power_of_two_weight_scales_every_bit(L, whole):
    """Every weight 2.0 (0.5), no costs: f and every entry of g are bit for bit 2x (0.5x) the unweighted trainer's, since
    every term of every fixed-order sum scales by a power of two.  A weight applied twice, or not at all, somewhere
    fails this."""
    rng = np.random.default_rng(7400 + L)
    s = sequences_problem(rng, L, _shuffled_lengths(rng, L)) if whole else training_set(rng, L, 5, 2)
    w = rng.normal(0, 1.5, size=s[7])
    f0, g0 = _trainer([s]).eval([w])
    for scale in (2.0, 0.5):
        f, g = _trainer([s], weights=[np.full(len(s[0]) - 1, scale)]).eval([w])
        assert same_bits(f[0], g[0], scale * f0[0], scale * g0[0]), scale
    assert f0[0] > 0 and np.count_nonzero(g0[0]) > 0


# ---------------------------------------------------------------- 4. zero weights
@pytest.mark.parametrize("whole", [False, True])
def test_zero_weights_drop_their_sequences(whole):
    rng = np.random.default_rng(7500 + whole)
    L, A = 3, 20
    lengths = [int(x) for x in rng.integers(6, 30, size=12)]
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, lengths, A, L)
    # attribute A (one more) sits on the items of the zero-weight sequences only
    zero = [2, 5, 11]
    item_ptr64 = item_ptr.astype(np.int64)
    attr, ptr = [], [0]
    for q in range(len(lengths)):
        for i in range(seq_ptr[q], seq_ptr[q + 1]):
            attr.extend(attr_id[item_ptr64[i]:item_ptr64[i + 1]].tolist() + ([A] if q in zero else []))
            ptr.append(len(attr))
    ws = () if whole else (5, 2)
    s = _full_features(seq_ptr, np.array(ptr, dtype=np.int32), np.array(attr, dtype=np.int32), labels, A + 1, L, *ws)
    wts = _weights(rng, len(lengths))
    wts[zero] = 0.0
    C = _costs(rng, L)
    w = rng.normal(0, 1.5, size=s[7])
    f, g = _trainer([s], weights=[wts], costs=[C]).eval([w])
    only = np.asarray(s[5]).reshape(A + 1, L)[A]
    assert np.all(g[0][only] == 0.0)
    keep = [q for q in range(len(lengths)) if q not in zero]
    sub = subproblem(s[0], s[1], s[2], s[3], keep)
    f1, g1 = _trainer([(*sub, *s[4:])], weights=[wts[keep]], costs=[C]).eval([w])
    assert abs(f[0] - f1[0]) <= 1e-12 * abs(f1[0])
    assert np.all(np.abs(g[0] - g1[0]) <= 1e-9 * (1 + np.abs(g1[0])))


# ---------------------------------------------------------------- 5. device cross-check of the costs
@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("L", [2, 5, 32])
def test_costs_are_the_gold_attribute_set_on_the_unweighted_trainer(L, whole):
    rng = np.random.default_rng(7600 + L)
    s = sequences_problem(rng, L, _shuffled_lengths(rng, L)) if whole else training_set(rng, L, 5, 3)
    C = _costs(rng, L)
    w = rng.normal(0, 1.5, size=s[7])
    f, g = _trainer([s], costs=[C]).eval([w])
    aug, tail = augmented(s, C)
    fa, ga = _trainer([aug]).eval([np.concatenate([w, tail])])
    assert abs(f[0] - fa[0]) <= 1e-12 * abs(fa[0])
    assert np.all(np.abs(g[0] - ga[0][:s[7]]) <= 1e-9 * (1 + np.abs(ga[0][:s[7]])))


# ---------------------------------------------------------------- 6. partial sets
@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("L", [2, 5, 32])
def test_weights_on_a_partial_problem(L, whole):
    from tests.train_objective_partial import hide_labels, objective_partial, partial_tolerances

    rng = np.random.default_rng(7700 + L)
    s = sequences_problem(rng, L, _shuffled_lengths(rng, L)) if whole else training_set(rng, L, 5, 3)
    masks, _ = hide_labels(rng, s[3], L)
    wts = _weights(rng, len(s[0]) - 1)
    w = rng.normal(0, 1.5, size=s[7])
    W, step = (None, None) if whole else (s[8], s[9])
    ef, eg = 0.0, np.zeros(s[7])
    for q in range(len(s[0]) - 1):  # the partial yardstick sequence by sequence, scaled
        b, e = int(s[0][q]), int(s[0][q + 1])
        sub = subproblem(s[0], s[1], s[2], s[3], [q])
        fq, gq, _ = objective_partial(sub[0], sub[1], sub[2], masks[b:e], s[4], L, W, step, s[5], s[6], w)
        ef, eg = ef + wts[q] * fq, eg + wts[q] * gq
    # the bounds: that yardstick's own for the whole problem (sums of per-instance terms that are not negative), every
    # instance's term scaled by its weight, so by at most the largest; the multiplication is one more rounded term of a row
    # of 2n + 2 and of a marginal's 5n, n >= 1: a factor of at most 5 / 4
    _, _, _, groups = objective_partial(s[0], s[1], s[2], masks, s[4], L, W, step, s[5], s[6], w, details=True)
    tol_f, tol_g = (1.25 * float(wts.max()) * t for t in partial_tolerances(L, groups))
    tr = _trainer([s], allowed=[masks], weights=[wts])
    f, g = tr.eval([w])
    print(f"L={L}: |f - ref| = {abs(f[0] - ef):.3g} (bound {tol_f:.3g}), max |g - ref| / bound = "
          f"{(np.abs(g[0] - eg) / np.maximum(tol_g, 1e-300)).max():.3g}")
    assert abs(f[0] - ef) <= tol_f, (f[0], ef, tol_f)
    assert np.all(np.abs(g[0] - eg) <= tol_g)
    f2, g2 = tr.eval([w])
    assert same_bits(f[0], g[0], f2[0], g2[0])
    # exact scaling against the unweighted partial trainer
    f0, g0 = _trainer([s], allowed=[masks]).eval([w])
    fs, gs = _trainer([s], allowed=[masks], weights=[np.full(len(s[0]) - 1, 2.0)]).eval([w])
    assert same_bits(fs[0], gs[0], 2.0 * f0[0], 2.0 * g0[0])
    with pytest.raises(ValueError, match="problem 0: label costs on a problem with allowed-label masks"):  # (GECCO_CRF_EINVAL)
        _trainer([s], allowed=[masks], costs=[_costs(rng, L)])


# ---------------------------------------------------------------- 7. contracts
BATCH = [(2, 20, 1, 25), (3, 5, 3, 8), (32, 20, 1, 5), (5, 2, 1, 30)]  # (L, W, step, sequences)


def _scratch_formula(s, weighted, costs, masked=False):
    L = label_count(s)
    n_items, n_seqs = int(s[0][-1]), len(s[0]) - 1
    if len(s) == 10:
        W, step = s[8], s[9]
        inst = sum((int(n) - W) // step + 1 for n in np.diff(s[0]))
        base = 2 * n_items * L + inst * W * L + (-(-inst // WINDOWS_PER_WORKGROUP) + REDUCE_SLABS) * (1 + L * L)
        base += inst * W * L if masked else 0
    else:
        inst = n_seqs
        base = 2 * n_items * L + (-(-inst // (THREADS // _group(L))) + REDUCE_SLABS) * (1 + L * L)
        base += n_items * L if masked else 0
    return 8 * (base + (inst if weighted or costs else 0) + (L * L if costs else 0))


def test_batch_masks_lone_bits_and_scratch():
    rng = np.random.default_rng(7800)
    sets = [training_set(rng, L, W, step, n_seqs=n) for L, W, step, n in BATCH]
    ws = [rng.normal(0, 1.5, size=s[7]) for s in sets]
    weights = [_weights(rng, len(sets[0][0]) - 1), None, _weights(rng, len(sets[2][0]) - 1), None]
    costs = [_costs(rng, 2), None, None, _costs(rng, 5)]
    lone = []
    for k, (s, w) in enumerate(zip(sets, ws)):
        kw = {} if weights[k] is None and costs[k] is None else {"weights": [weights[k]], "costs": [costs[k]]}
        t = _trainer([s], **kw)
        f, g = t.eval([w])
        lone.append((f[0], g[0]))
        assert t.scratch_bytes(0) == _scratch_formula(s, weights[k] is not None, costs[k] is not None)
    tr = _trainer(sets, weights=weights, costs=costs)
    assert [tr.scratch_bytes(k) for k in range(4)] == [_scratch_formula(s, weights[k] is not None, costs[k] is not None)
                                                       for k, s in enumerate(sets)]
    assert tr.scratch_bytes(-1) == sum(tr.scratch_bytes(k) for k in range(4))
    # problem 1 has neither: the bytes of the lone unweighted trainer (computed above without a keyword)
    for mask in ([True] * 4, [False] * 4, [True, False, True, False], [False, True, False, True], [False, False, False, True],
                 [True, False, False, False], [False, True, True, False]):
        f = np.full(4, -7.25)
        g = [np.full(s[7], -3.5) for s in sets]
        tr.eval([w if m else None for w, m in zip(ws, mask)], mask, f, g)
        for k, m in enumerate(mask):
            if m:
                assert same_bits(f[k], g[k], *lone[k]), (mask, k)
            else:
                assert f[k] == -7.25 and np.all(g[k] == -3.5), (mask, k)
    check_strict(tr, 0, sets[0], weights[0], costs[0], ws[0])
    check_strict(tr, 3, sets[3], None, costs[3], ws[3])
    # whole sequences and a partial problem: the formula
    q = sequences_problem(rng, 5, [3, 9, 1, 4])
    assert _trainer([q], weights=[np.ones(4)]).scratch_bytes(0) == _scratch_formula(q, True, False)
    assert _trainer([q], costs=[_costs(rng, 5)]).scratch_bytes(0) == _scratch_formula(q, False, True)
    from tests.train_objective_partial import full_masks
    assert (_trainer([q], allowed=[full_masks(int(q[0][-1]), 5)], weights=[np.ones(4)]).scratch_bytes(0)
            == _scratch_formula(q, True, False, masked=True))


def test_the_restated_scratch_formulas_of_train():
    from gecco_amd import train
    from tests.test_gpu_train_general import _fit_set

    ts = _fit_set(31, L=3)
    ts.seq_weight = np.linspace(0.5, 2.0, len(ts.seq_ptr) - 1)
    params = train.trainer_params({"label_costs": {("y0", "y1"): 1.5}})
    C = train._cost_matrix(ts, params)
    tr = _trainer([ts.native_args()], weights=[ts.seq_weight], costs=[C])
    assert tr.scratch_bytes(0) == train._general_scratch_bytes(ts, params)
    assert _trainer([ts.native_args()], weights=[ts.seq_weight]).scratch_bytes(0) == train._general_scratch_bytes(ts)
    whole = train.TrainingSet(**{**ts.__dict__, "window": None, "step": None})
    tq = _trainer([whole.native_args()], weights=[ts.seq_weight], costs=[C])
    assert tq.scratch_bytes(0) == train._sequences_scratch_bytes(whole, params)


@pytest.mark.parametrize("whole", [False, True])
def test_refusals_come_before_the_device(whole):
    """Each refusal with its message and code, on a device that does not exist: found on the host."""
    from gecco_amd import _native

    rng = np.random.default_rng(7900)
    s = sequences_problem(rng, 3, [4, 2, 6]) if whole else training_set(rng, 3, 3, 1, n_seqs=2, fixed=1)
    n = len(s[0]) - 1
    family = "trainer sequences" if whole else "trainer general"
    good = np.zeros((3, 3))
    good[1, 2] = 0.5

    def refused(match, problems=None, **kw):
        with pytest.raises(ValueError, match=match) as err:  # (GECCO_CRF_EINVAL is a ValueError, any other code a NativeError)
            _trainer(problems or [s], device=10 ** 6, **kw)
        assert not isinstance(err.value, _native.NativeError) and family in str(err.value)

    for bad in (-0.5, float("nan"), float("inf")):
        wts = np.ones(n)
        wts[1] = bad
        refused("problem 0: weight of sequence 1 is negative or not finite", weights=[wts])
        C = good.copy()
        C[2, 0] = bad
        refused(r"problem 0: cost \[2\]\[0\] is negative or not finite", costs=[C])
    C = good.copy()
    C[1, 1] = 0.25
    refused(r"problem 1: cost \[1\]\[1\] is on the diagonal and not 0", problems=[s, s], costs=[None, C])
    from tests.train_objective_partial import full_masks
    refused("problem 0: label costs on a problem with allowed-label masks", allowed=[full_masks(int(s[0][-1]), 3)], costs=[good])
    with pytest.raises(ValueError, match="weights of a problem hold 2 entries"):
        _trainer([s], weights=[np.ones(2)] if n != 2 else [np.ones(5)])
    # legal: a weight of 0, a table of zeros (only the missing device is left to refuse)
    with pytest.raises(_native.NativeError) as err:
        _trainer([s], device=10 ** 6, weights=[np.zeros(n)], costs=[np.zeros((3, 3))])
    assert err.value.code in (_native.ENODEV, _native.EHIP, _native.EINVAL) and "weight" not in str(err.value) and "cost" not in str(err.value)


# ---------------------------------------------------------------- 8. fits
def _weighted_fit_set(seed, L=4):
    from tests.test_gpu_train_general import _fit_set

    ts = _fit_set(seed, L=L)
    rng = np.random.default_rng(seed)
    # distinct weights in [0.25, 4] scaled to a mean of 1, as class weights have: the tolerances of the two fit tests below are
    # absolute, on an objective and a gradient that scale with the weights, and c1 / c2 keep their meaning
    wts = _weights(rng, len(ts.seq_ptr) - 1)
    ts.seq_weight = wts / wts.mean()
    costs = {(f"y{a}", f"y{b}"): float(rng.uniform(0, 2)) for a in range(L) for b in range(L) if a != b}
    return ts, costs


def _np_fg(ts, C, c2):
    def fg(w):
        f, g, _ = objective_weighted(ts.native_args(), ts.seq_weight, C, w)
        return f + c2 * float(w @ w), g + 2 * c2 * w

    return fg


def test_fit_l2_reaches_the_scipy_optimum():
    import scipy.optimize
    from gecco_amd import train

    ts, costs = _weighted_fit_set(41)
    params = train.trainer_params({"c1": 0.0, "c2": 0.15, "epsilon": 1e-10, "delta": 0.0, "label_costs": costs})
    res = train.fit_training_set(ts, params)
    fg = _np_fg(ts, train._cost_matrix(ts, params), 0.15)
    ref = scipy.optimize.minimize(fg, np.zeros(ts.num_features), jac=True, method="L-BFGS-B",
                                  options={"ftol": 1e-15, "gtol": 1e-10, "maxiter": 10000})
    f_ours = fg(res.x)[0]
    assert abs(f_ours - ref.fun) <= 1e-8 * abs(ref.fun), (f_ours, ref.fun, res)
    assert np.abs(res.x - ref.x).max() <= 1e-4


def test_fit_l1_satisfies_kkt():
    """The set is that of test_fit_l1_satisfies_kkt of tests/test_gpu_train_general.py (seed 12), whose conditions these are,
    with weights and costs on it: OWL-QN's backtracking search ends every one of these fits with "line search failed", at a
    gradient residual that depends on the set (measured on the device: 4.2e-6 on that set as it is, 7.9e-6 with these
    weights; on the set of seed 42 with weights and costs 2.5e-5, which is above the bound)."""
    from gecco_amd import train

    ts, costs = _weighted_fit_set(12)
    c1 = 0.5
    params = train.trainer_params({"c1": c1, "c2": 0.0, "epsilon": 1e-10, "delta": 0.0, "label_costs": costs})
    res = train.fit_training_set(ts, params)
    _, g = _np_fg(ts, train._cost_matrix(ts, params), 0.0)(res.x)
    w = res.x
    nz = w != 0
    assert nz.any() and (~nz).any()
    print(f"{res!r}: max KKT residual on the support {np.abs(g[nz] + c1 * np.sign(w[nz])).max():.3g}, "
          f"max |g| off it {np.abs(g[~nz]).max():.6g}")
    assert np.abs(g[nz] + c1 * np.sign(w[nz])).max() <= 1e-5
    assert np.abs(g[~nz]).max() <= c1 + 1e-5


def _same_result(a, b):
    return (a.x.tobytes() == b.x.tobytes() and a.n_iter == b.n_iter and a.status == b.status
            and np.float64(a.f).tobytes() == np.float64(b.f).tobytes())


def test_batch_and_grid_fits_return_the_lone_fits():
    """Sets with and without weights, 2 labels among them, and a grid whose problems differ in their costs, under a
    scratch budget that splits the groups: every result is the lone fit's, bit for bit; the sets without weights keep the
    bits of their lone unweighted fits."""
    from gecco_amd import train
    from tests.test_gpu_train_general import _fit_set

    weighted4, costs4 = _weighted_fit_set(51)
    weighted2, _ = _weighted_fit_set(52, L=2)
    sets = [weighted4, _fit_set(53, L=2), weighted2, _fit_set(54)]
    base = {"c1": 0.05, "c2": 0.1, "max_iterations": 20}
    params = train.trainer_params(base)
    lone = [train.fit_training_set(ts, params) for ts in sets]
    for a, b in zip(train.fit_training_sets(sets, params), lone):
        assert _same_result(a, b)
    grid = [(0, train.trainer_params({**base, "label_costs": costs4})), (1, params),
            (1, train.trainer_params({**base, "label_costs": {("y1", "y0"): 2.0}})),
            (1, train.trainer_params({**base, "label_costs": {("y1", "y0"): 0.5, ("y0", "y1"): 0.25}})),
            (2, params), (3, params), (3, train.trainer_params({**base, "label_costs": {("y2", "y0"): 1.0}}))]
    lone_grid = [train.fit_training_set(sets[s], p) for s, p in grid]
    assert _same_result(lone_grid[1], lone[1]) and _same_result(lone_grid[5], lone[3])
    assert not _same_result(lone_grid[2], lone_grid[3]) and not _same_result(lone_grid[2], lone[1])
    need = train._general_scratch_bytes(sets[0], grid[0][1]) + train._general_scratch_bytes(sets[1], grid[2][1])
    for budget in (train.GRID_SCRATCH_BUDGET, need, 1):
        for a, b in zip(train.fit_grid(sets, grid, scratch_budget_bytes=budget), lone_grid):
            assert _same_result(a, b), budget
    assert lone[0].n_iter > 0


# ---------------------------------------------------------------- 9. front ends
def _named(rng, L, n_seqs, A=30, lo=12, hi=50):
    from tests.test_gpu_train_general import _named as named

    return named(rng, L, n_seqs, A=A, lo=lo, hi=hi)


def test_sequence_crf_with_weights_and_costs(tmp_path):
    from gecco_amd import train
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(8100)
    X, y = _named(rng, 3, 20)
    wts = _weights(rng, len(X))
    costs = {("type1", "type0"): 1.5, ("type0", "type2"): 0.5}
    crf = SequenceCRF(window_size=5, c2=0.2, max_iterations=25, label_costs=costs).fit(X, y, sample_weight=wts)
    ts = train.build_training_set(X, y, 5, 1, max_labels=32, sample_weight=wts)
    res = train.fit_training_set(ts, train.trainer_params({"c2": 0.2, "max_iterations": 25, "label_costs": costs}))
    assert crf.training_result_.x.tobytes() == res.x.tobytes() and crf.training_result_.n_iter == res.n_iter > 0
    plain = SequenceCRF(window_size=5, c2=0.2, max_iterations=25).fit(X, y)
    assert plain.training_result_.x.tobytes() != res.x.tobytes()
    crf.save(tmp_path / "m.crfsuite")
    other = SequenceCRF.load(tmp_path / "m.crfsuite", window_size=5)
    assert other.to_bytes() == crf.to_bytes() == train.model_blob(ts, res.x)
    with pytest.raises(ValueError, match="partially labelled"):
        SequenceCRF(window_size=5, label_costs=costs).fit(X, [[{"type0", "type1"}] + ys[1:] for ys in y])


def test_cluster_crf_with_label_costs_fits_saves_and_loads(tmp_path, monkeypatch):
    import random
    import warnings

    from gecco_amd import pickle_model
    from gecco_amd.crf import ClusterCRF
    from tests.test_gpu_train import _genes

    monkeypatch.delenv("GECCO_AMD_FIT", raising=False)
    costs = {("1", "0"): 2.0, ("0", "1"): 0.25}
    fits = []
    for options in ({"label_costs": costs}, {}):
        random.seed(3)
        crf = ClusterCRF("protein", window_size=5, window_step=1, c1=0.1, c2=0.05, **options)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            crf.fit(_genes(np.random.default_rng(5)))
        fits.append(crf)
    crf, plain = fits
    assert crf.training_result_.n_iter > 0 and crf.training_result_.x.tobytes() != plain.training_result_.x.tobytes()
    crf.save(tmp_path)
    loaded = ClusterCRF.trained(tmp_path)
    assert loaded._options["label_costs"] == costs and loaded._options["c1"] == 0.1
    assert pickle_model.load_model_dir(tmp_path).state["_options"]["label_costs"] == costs
    genes = _genes(np.random.default_rng(6), n_contigs=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = [g.average_probability for g in crf.predict_probabilities(genes)]
        b = [g.average_probability for g in loaded.predict_probabilities(_genes(np.random.default_rng(6), n_contigs=3))]
    assert a == b


def test_typed_class_weight_balanced(monkeypatch):
    from gecco_amd import train, typed
    from tests.typed_planted import C, W, cluster_table, planted_set

    genes, rows = planted_set(11, 6, "train", composite=True)
    captured = []
    fit = train.fit_training_set
    monkeypatch.setattr(train, "fit_training_set", lambda ts, params, device=0: captured.append((ts, params)) or fit(ts, params, device=device))
    crf = typed.TypedClusterCRF(W, 1, c1=C, c2=C, class_weight="balanced", max_iterations=30)
    crf.fit(genes, cluster_table(rows), shuffle=False)
    # by hand: 12 clusters; contig c holds two of type TYPES[c % 3], but the second of contig 0 is Alpha;Beta
    counts = {"Alpha": 3, "Alpha;Beta": 1, "Beta": 4, "Gamma": 4}
    expected = {label: 12 / (4 * c) for label, c in counts.items()}
    assert crf.class_weight_ == expected
    by_contig = [(expected["Alpha"] + expected["Alpha;Beta"]) / 2, expected["Beta"], expected["Gamma"], expected["Alpha"],
                 expected["Beta"], expected["Gamma"]]  # (shuffle=False: the sequences in sorted order of their ids)
    ts, params = captured[0]
    assert ts.seq_weight.tolist() == by_contig
    monkeypatch.undo()
    again = train.TrainingSet(**{**ts.__dict__, "seq_weight": np.array(by_contig)})
    res = train.fit_training_set(again, params)
    assert res.x.tobytes() == crf.training_result_.x.tobytes() and res.n_iter > 0
    plain = typed.TypedClusterCRF(W, 1, c1=C, c2=C, max_iterations=30).fit(genes, cluster_table(rows), shuffle=False)
    assert plain.class_weight_ is None and plain.training_result_.x.tobytes() != res.x.tobytes()


def _write_tables(directory, genes, clusters):
    import os

    from gecco_amd import tables

    os.makedirs(directory, exist_ok=True)
    paths = [os.path.join(directory, name) for name in ("genes.tsv", "features.tsv", "clusters.tsv")]
    tables.GeneTable.from_genes(genes).dump(paths[0])
    tables.FeatureTable.from_genes(genes).dump(paths[1])
    clusters.dump(paths[2])
    return paths


def test_command_lines_run_end_to_end(tmp_path, monkeypatch):
    """``train``, ``typed train`` and ``cv`` with their cost options, in process, on the small tables of the existing
    command-line tests; a cost changes the model."""
    import os
    import warnings

    from gecco_amd import cv, train_cli, typed
    from tests.test_gpu_train_cli import _synthetic_inputs
    from tests.typed_planted import cluster_table, planted_set

    monkeypatch.setenv("GECCO_AMD_FIT", "native")
    g, (f,), c = _synthetic_inputs(tmp_path)  # (domains below the command lines' default p-value filter)
    common = ["--genes", g, "--features", f, "--clusters", c]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert train_cli.main(common + ["--miss-cost", "2", "--false-cost", "0.5", "-o", str(tmp_path / "m_cost")]) == 0
        assert train_cli.main(common + ["-o", str(tmp_path / "m_plain")]) == 0
        assert cv.main(common + ["--splits", "3", "--miss-cost", "2", "-o", str(tmp_path / "cv_cost.tsv")]) == 0
        assert cv.main(common + ["--splits", "3", "-o", str(tmp_path / "cv_plain.tsv")]) == 0
    models = [open(os.path.join(str(tmp_path / d), "model.pkl"), "rb").read() for d in ("m_cost", "m_plain")]
    assert models[0] != models[1]
    assert (tmp_path / "cv_cost.tsv").read_bytes() != (tmp_path / "cv_plain.tsv").read_bytes()
    tg, rows = planted_set(11, 6, "train", composite=False)
    g, f, c = _write_tables(str(tmp_path / "typed"), tg, cluster_table(rows))
    common = ["train", "--genes", g, "--features", f, "--clusters", c]
    assert typed.main(common + ["--class-weight", "balanced", "--miss-cost", "1.5", "--false-cost", "0.5", "-o",
                                str(tmp_path / "t_cost")]) == 0
    assert typed.main(common + ["-o", str(tmp_path / "t_plain")]) == 0
    blobs = [open(os.path.join(str(tmp_path / d), "typed_model.crfsuite"), "rb").read() for d in ("t_cost", "t_plain")]
    assert blobs[0] != blobs[1]


def test_grid_search_with_a_miss_cost_axis_is_cross_validate_per_point(monkeypatch):
    import random
    import warnings

    from gecco_amd import cv
    from gecco_amd.crf import ClusterCRF
    from tests.test_gpu_cv import _dataset

    monkeypatch.setenv("GECCO_AMD_FIT", "native")
    grid = {"c1": [0.15], "c2": [0.15], "window_size": [5], "miss_cost": [0.0, 2.0]}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        genes, _ = _dataset()
        random.seed(5)
        res = cv.grid_search(ClusterCRF("protein", window_size=5, window_step=1, c1=0.15, c2=0.15), genes, 3, grid)
        assert [pt["miss_cost"] for pt in res.points] == [0.0, 2.0] and b"miss_cost" in res.table() and b"miss_cost" in res.summary()
        for p, pt in enumerate(res.points):
            genes, _ = _dataset()
            random.seed(5)
            alone = cv.cross_validate(ClusterCRF("protein", window_size=5, window_step=1, c1=0.15, c2=0.15,
                                                 **cv.cost_options(pt["miss_cost"], 0.0)), genes, 3)
            for fold, ref in zip(res.folds[p], alone.folds):
                a, b = fold.crf.training_result_, ref.crf.training_result_
                assert (a.n_iter, a.n_eval, a.status) == (b.n_iter, b.n_eval, b.status) and a.n_iter > 0
                assert a.x.tobytes() == b.x.tobytes()
                expected = np.array([g.average_probability for g in ref.predicted], dtype=np.float64)
                assert fold.probabilities.tobytes() == expected.tobytes()
    assert res.folds[0][0].crf.training_result_.x.tobytes() != res.folds[1][0].crf.training_result_.x.tobytes()


def test_recall_of_the_cluster_label_under_a_miss_cost():
    """Printed, not asserted: the training-set recall of label '1' at miss cost 0 and 2 on a planted imbalanced set (a
    tenth of the items are '1', and their attributes overlap the background's).  The direction is expected, and not
    guaranteed by the objective."""
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(8200)
    X, y = [], []
    for _ in range(30):
        n = int(rng.integers(30, 60))
        lab = np.zeros(n, dtype=int)
        start = int(rng.integers(0, n - 6))
        lab[start:start + int(rng.integers(3, 6))] = 1
        X.append([[f"a{int(a)}" for a in rng.integers(0, 12, size=2) + (4 if v else 0)] for v in lab])
        y.append([str(v) for v in lab])
    for cost in (0.0, 2.0):
        options = {"label_costs": {("1", "0"): cost}} if cost else {}
        crf = SequenceCRF(window_size=5, c1=0.1, c2=0.1, max_iterations=60, **options).fit(X, y)
        pred = crf.predict(X)
        hit = sum(p == "1" for ps, ys in zip(pred, y) for p, t in zip(ps, ys) if t == "1")
        called = sum(p == "1" for ps in pred for p in ps)
        total = sum(t == "1" for ys in y for t in ys)
        print(f"miss cost {cost}: recall of '1' = {hit / total:.3f} ({hit} of {total}), precision = {hit / max(called, 1):.3f}")
