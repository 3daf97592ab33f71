"""Training with real-valued attributes on the device: ``gecco_crf_trainer_general_create_valued`` and
``gecco_crf_trainer_sequences_create_valued`` against the independent numpy yardstick (tests/train_objective_valued.py),
the geometry edges of the kernels that read values (item scores, the attribute -> items transpose), the bit contracts
(all values 1.0 are the unvalued trainer; a valued problem beside an unvalued and an inactive one), the refusals, and
``SequenceCRF`` fitted on dict items against scipy's optimum of the yardstick."""
import numpy as np
import pytest

from tests import train_objective_valued as tv
from tests.train_objective_labels import same_bits
from tests.train_objective_sequences import sequences_problem

pytestmark = pytest.mark.gpu

THREADS = 256
LABELS = [2, 3, 5, 8, 17, 32]  # every G (2, 4, 8, 8, 32, 32), with L = G and L < G
FIXED_LENGTHS = [1, 1, 2, 3, 7, 40, 41, 300]
WINDOWS = [(1, 1), (5, 2), (20, 1), (32, 1)]


def _group(L):
    G = 2
    while G < L:
        G *= 2
    return G


def _labels_of(s):
    return np.asarray(s[5]).size // s[4]


def _problem(rng, L, window=None, A=20, lengths=None, drop=0.1):
    """(problem tuple, values): a seeded problem as ``sequences_problem`` builds it (a tenth of the pairs without a
    feature, some empty items), for a windowed problem with (W, step) appended and every sequence at least W long, and one
    value per attribute entry from the mix N(0, 1), 0, 1, +-2^10, 2^-10."""
    if lengths is None:
        lengths = FIXED_LENGTHS + [int(x) for x in rng.integers(1, 61, size=30)]
    if window is not None:
        lengths = [max(n, window[0]) for n in lengths]
    s = sequences_problem(rng, L, lengths, A=A, drop=drop)
    if window is not None:
        s = s + tuple(window)
    return s, tv.mixed_values(rng, len(s[2]))


def _trainer(problems, values):
    from gecco_amd import _native

    family = _native.TrainerSequences if len(problems[0]) == 8 else _native.TrainerGeneral
    return family(list(problems), values=list(values))


def _reference(s, v, w, details=False):
    L = _labels_of(s)
    if len(s) == 8:
        return tv.objective_sequences(*s[:5], L, s[5], s[6], w, v, details=details)
    return tv.objective(*s[:5], L, s[8], s[9], s[5], s[6], w, v, details=details)


def _tolerances(s, v, w):
    L = _labels_of(s)
    if len(s) == 8:
        return tv.objective_sequences_tolerances(*s[:5], L, s[5], s[6], w, v)
    return tv.objective_tolerances(*s[:5], L, s[8], s[9], s[5], s[6], w, v)


def check_strict(tr, k, s, v, w):
    """Problem k of `tr` at `w` within the project's strict bounds of the yardstick (tests/test_gpu_train_sequences.py's
    check_strict), and the same bytes from a second evaluation.  Returns (f, g)."""
    n = len(tr)
    ws, active = [w if j == k else None for j in range(n)], [j == k for j in range(n)]
    f, g = tr.eval(ws, active)
    ef, eg, n_inst = _reference(s, v, w)
    assert tr.num_windows(k) == n_inst
    print(f"L={_labels_of(s)} instances={n_inst}: |f - ref| / |ref| = {abs(f[k] - ef) / max(abs(ef), 1e-300):.3g}, "
          f"max |g - ref| / (1 + |ref|) = {(np.abs(g[k] - eg) / (1 + np.abs(eg))).max() if len(eg) else 0.0:.3g}")
    assert abs(f[k] - ef) <= 1e-12 * abs(ef), (f[k], ef)
    assert np.all(np.abs(g[k] - eg) <= 1e-9 * (1 + np.abs(eg))), np.abs(g[k] - eg).max()
    f2, g2 = tr.eval(ws, active)
    assert same_bits(f[k], g[k], f2[k], g2[k])
    return f[k], g[k]


def check_bounds(tr, k, s, v, w):
    """Problem k at `w` finite and within the derived bounds of the yardstick (weights far from the origin)."""
    n = len(tr)
    f, g = tr.eval([w if j == k else None for j in range(n)], [j == k for j in range(n)])
    ef, eg, _ = _reference(s, v, w)
    assert np.isfinite(ef) and np.all(np.isfinite(eg))
    assert np.isfinite(f[k]) and np.all(np.isfinite(g[k])), (f[k], int(np.count_nonzero(~np.isfinite(g[k]))))
    tol_f, tol_g = _tolerances(s, v, w)
    err = np.abs(g[k] - eg)
    print(f"L={_labels_of(s)}: |f - ref| = {abs(f[k] - ef):.3g} (bound {tol_f:.3g}), "
          f"max |g - ref| / bound = {(err / np.maximum(tol_g, 1e-300)).max():.3g}")
    assert abs(f[k] - ef) <= tol_f, (f[k], ef, abs(f[k] - ef), tol_f)
    assert np.all(err <= tol_g), (int(np.argmax(err / np.maximum(tol_g, 1e-300))), float(err.max()))


# ---------------------------------------------------------------- against the yardstick
@pytest.mark.parametrize("window", [None] + WINDOWS, ids=lambda w: "whole" if w is None else f"W{w[0]}s{w[1]}")
@pytest.mark.parametrize("L", LABELS)
def test_eval_matches_the_yardstick(L, window):
    rng = np.random.default_rng(4100 + 10 * L + (0 if window is None else window[0]))
    s, v = _problem(rng, L, window, A=20 if window is None else 60)
    assert np.any(np.diff(s[1]) == 0) and np.any(s[5] < 0) and np.any(s[6] < 0)
    assert {0.0, 1.0, 1024.0, -1024.0, 2.0 ** -10} <= set(v.tolist())
    tr = _trainer([s], [v])
    assert len(tr) == 1
    check_strict(tr, 0, s, v, np.zeros(s[7]))
    check_strict(tr, 0, s, v, rng.normal(0, 1.5, size=s[7]))


def _plant(s, w, rng):
    """w with one transition at -800 and one at +720 (two pairs that have a feature): §4.9b's plants."""
    L = _labels_of(s)
    tfid = np.asarray(s[6]).reshape(L, L)
    pairs = [(i, j) for i in range(L) for j in range(L) if tfid[i, j] >= 0]
    a, b = (pairs[k] for k in rng.choice(len(pairs), size=2, replace=False))
    w = w.copy()
    w[tfid[a]], w[tfid[b]] = -800.0, 720.0
    return w


@pytest.mark.parametrize("window", [None, (5, 1), (20, 1)], ids=lambda w: "whole" if w is None else f"W{w[0]}")
@pytest.mark.parametrize("L", [3, 9])
def test_extreme_weights_under_large_values(L, window):
    """Weights a thousand times N(0, 1.5), transitions planted at -800 and +720, and |v| = 2^10 on top: state scores of
    millions of nats.  Finite, and within the derived bounds."""
    rng = np.random.default_rng(9100 + L + (0 if window is None else window[0]))
    s, v = _problem(rng, L, window, lengths=[1, 2, 5, 20, 41, 150] + [int(x) for x in rng.integers(1, 61, size=20)])
    assert np.abs(v).max() == 1024.0
    tr = _trainer([s], [v])
    w = 1000.0 * rng.normal(0, 1.5, size=s[7])
    check_bounds(tr, 0, s, v, w)
    check_bounds(tr, 0, s, v, _plant(s, w, rng))
    check_bounds(tr, 0, s, v, _plant(s, rng.normal(0, 1.5, size=s[7]), rng))


# ---------------------------------------------------------------- geometry edges of what changed
def _with_attribute_lists(s, v, counts, rng):
    """The problem with len(counts) new attributes in front of the others, attribute k on the first counts[k] items (one
    more entry at the end of the item's list, with a value of its own), every pair with a feature."""
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K = s[:8]
    n, L, extra = len(labels), _labels_of(s), len(counts)
    assert max(counts) <= n
    new_ptr, new_attr, new_val = [0], [], []
    for i in range(n):
        new_attr.extend(int(a) + extra for a in attr_id[item_ptr[i]:item_ptr[i + 1]])
        new_val.extend(v[item_ptr[i]:item_ptr[i + 1]].tolist())
        for k, c in enumerate(counts):
            if i < c:
                new_attr.append(k)
                new_val.append(float(rng.normal()))
        new_ptr.append(len(new_attr))
    A2 = A + extra
    K2 = A2 * L + L * L
    out = (seq_ptr, np.array(new_ptr, dtype=np.int32), np.array(new_attr, dtype=np.int32), labels, A2,
           np.arange(A2 * L, dtype=np.int32), A2 * L + np.arange(L * L, dtype=np.int32), K2) + tuple(s[8:])
    return out, np.array(new_val)


@pytest.mark.parametrize("whole", [True, False], ids=["whole", "windowed"])
@pytest.mark.parametrize("L", [2, 3, 32])
def test_attribute_list_lengths_around_the_rows(L, whole):
    """gen_attr_counts sums an attribute's items in 256 / G strided rows: lists of 0, 1, rows - 1, rows, rows + 1 and
    3 rows + 1 items (a row with no item, one, and four)."""
    rows = THREADS // _group(L)
    counts = [0, 1, rows - 1, rows, rows + 1, 3 * rows + 1]
    rng = np.random.default_rng(300 + L)
    s, v = _problem(rng, L, None if whole else (5, 2), lengths=[3 * rows + 1 + 7, 9, 5, 30], drop=0.0)
    s, v = _with_attribute_lists(s, v, counts, rng)
    assert np.bincount(s[2], minlength=s[4])[:6].tolist() == counts
    tr = _trainer([s], [v])
    _, g = check_strict(tr, 0, s, v, rng.normal(0, 1.5, size=s[7]))
    assert np.all(g[:L] == 0.0)  # the attribute no item holds: no expected and no empirical count


@pytest.mark.parametrize("n_win", [127, 128, 129])
def test_window_counts_around_a_workgroup(n_win):
    rng = np.random.default_rng(n_win)
    for L in (3, 17):
        s, v = _problem(rng, L, (5, 1), lengths=[5 + 99, 5 + n_win - 100 - 1])
        tr = _trainer([s], [v])
        assert tr.num_windows(0) == n_win
        check_strict(tr, 0, s, v, rng.normal(0, 1.5, size=s[7]))


@pytest.mark.parametrize("L", [2, 5, 32])
def test_sequence_counts_around_a_workgroup(L):
    rng = np.random.default_rng(70 + L)
    side = THREADS // _group(L)
    for n_seqs in (side - 1, side, side + 1):
        s, v = _problem(rng, L, lengths=[int(x) for x in rng.integers(1, 9, size=n_seqs)])
        tr = _trainer([s], [v])
        assert tr.num_windows(0) == n_seqs
        check_strict(tr, 0, s, v, rng.normal(0, 1.5, size=s[7]))


@pytest.mark.parametrize("whole", [True, False], ids=["whole", "windowed"])
def test_items_with_no_and_with_forty_attributes(whole):
    rng = np.random.default_rng(40)
    L, A = 5, 60
    s, v = _problem(rng, L, None if whole else (5, 1), A=A, lengths=[9, 12, 6])
    item_ptr, attr_id = s[1], s[2]
    target = int(np.flatnonzero(np.diff(item_ptr) > 0)[3])
    forty = rng.choice(A, size=40, replace=False).astype(np.int32)
    attr = np.concatenate([attr_id[:item_ptr[target]], forty, attr_id[item_ptr[target + 1]:]])
    vals = np.concatenate([v[:item_ptr[target]], tv.mixed_values(rng, 40), v[item_ptr[target + 1]:]])
    ptr = item_ptr.copy()
    ptr[target + 1:] += 40 - (item_ptr[target + 1] - item_ptr[target])
    s = s[:1] + (ptr.astype(np.int32), attr.astype(np.int32)) + s[3:]
    assert 40 in np.diff(s[1]) and 0 in np.diff(s[1])
    check_strict(_trainer([s], [vals]), 0, s, vals, rng.normal(0, 1.5, size=s[7]))


# ---------------------------------------------------------------- bit contracts
@pytest.mark.parametrize("window", [None, (5, 2)], ids=["whole", "windowed"])
@pytest.mark.parametrize("L", LABELS)
def test_all_ones_are_the_unvalued_trainer(L, window):
    from gecco_amd import _native

    rng = np.random.default_rng(500 + L)
    s, _ = _problem(rng, L, window)
    w = rng.normal(0, 1.5, size=s[7])
    family = _native.TrainerSequences if window is None else _native.TrainerGeneral
    plain = family([s])
    f0, g0 = plain.eval([w])
    valued = _trainer([s], [np.ones(len(s[2]))])
    f1, g1 = valued.eval([w])
    assert same_bits(f0[0], g0[0], f1[0], g1[0])
    assert valued.scratch_bytes(0) == plain.scratch_bytes(0) + 8 * len(s[2])


@pytest.mark.parametrize("window", [None, (5, 2)], ids=["whole", "windowed"])
def test_valued_problem_beside_an_unvalued_and_an_inactive_one(window):
    from gecco_amd import _native

    rng = np.random.default_rng(61)
    (s0, v0), (s1, _), (s2, v2) = (_problem(rng, L, window) for L in (5, 3, 17))
    ws = [rng.normal(0, 1.5, size=s[7]) for s in (s0, s1, s2)]
    family = _native.TrainerSequences if window is None else _native.TrainerGeneral
    lone_valued = _trainer([s0], [v0]).eval([ws[0]])
    lone_plain = family([s1]).eval([ws[1]])  # the unvalued create
    tr = _trainer([s0, s1, s2], [v0, None, v2])
    f = np.full(3, -7.25)
    g = [np.full(s[7], -3.5) for s in (s0, s1, s2)]
    tr.eval([ws[0], ws[1], None], [True, True, False], f, g)
    assert same_bits(f[0], g[0], lone_valued[0][0], lone_valued[1][0])
    assert same_bits(f[1], g[1], lone_plain[0][0], lone_plain[1][0])
    assert f[2] == -7.25 and np.all(g[2] == -3.5)
    assert tr.scratch_bytes(1) == family([s1]).scratch_bytes(0)
    assert tr.scratch_bytes(-1) == sum(tr.scratch_bytes(k) for k in range(3))
    check_strict(tr, 2, s2, v2, ws[2])


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("window", [None, (5, 1)], ids=["whole", "windowed"])
def test_non_finite_values_are_refused(bad, window):
    from gecco_amd import _native

    rng = np.random.default_rng(2)
    s, v = _problem(rng, 3, window, lengths=[6, 9])
    good, _ = _problem(rng, 4, window, lengths=[7])
    v = v.copy()
    v[4] = bad
    family = "sequences" if window is None else "general"
    with pytest.raises(ValueError, match=f"trainer {family}: problem 1: trainer: attribute value 4 is not finite"):
        _trainer([good, s], [None, v])
    lib = _native.load_library()
    assert lib.gecco_crf_last_error().decode() == f"trainer {family}: problem 1: trainer: attribute value 4 is not finite (NaN or infinite)"


# ---------------------------------------------------------------- a fit on dict items
def _scored_data(rng, n_seqs=40, lo=8, hi=25):
    """Three labels; "kind" tells c from the other two, and the real-valued "score" alone tells a (positive) from b
    (negative): as a plain name it sits on every item alike."""
    X, y = [], []
    for _ in range(n_seqs):
        n = int(rng.integers(lo, hi + 1))
        labs = [str(rng.choice(["a", "b", "c"])) for _ in range(n)]  # (independent labels: transitions tell nothing)
        xs = []
        for lab in labs:
            score = {"a": 1.0, "b": -1.0, "c": 0.0}[lab] + float(rng.normal(0, 0.4))
            xs.append({"bias": 1.0, "kind": "c" if lab == "c" else "ab", "score": score, "odd": bool(rng.integers(0, 2))})
        X.append(xs)
        y.append(labs)
    return X, y


def _accuracy_ab(crf, X, y):
    pred = crf.predict(X)
    hits = [p == t for ps, ts in zip(pred, y) for p, t in zip(ps, ts) if t in ("a", "b")]
    return sum(hits) / len(hits)


@pytest.mark.parametrize("window", [5, None], ids=["windowed", "whole"])
def test_sequence_crf_fits_dict_items(window):
    import scipy.optimize
    from gecco_amd import _native, train
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(77)
    X, y = _scored_data(rng)
    options = {"c1": 0.0, "c2": 0.15, "epsilon": 1e-10, "delta": 0.0}
    crf = SequenceCRF(window_size=window, **options).fit(X, y)
    assert sorted(crf.classes_) == ["a", "b", "c"]
    assert {"bias", "kind:ab", "kind:c", "score", "odd"} == set(crf.attributes_)
    pairs = [[list(zip(*train.item_attributes(item))) for item in xs] for xs in X]
    ts = train.build_training_set(pairs, y, window, None if window is None else 1, max_labels=32)
    assert ts.attr_value is not None and crf.classes_ == ts.labels_
    A, L = len(ts.attrs_), ts.num_labels

    def fg(w):
        if window is None:
            f, g, _ = tv.objective_sequences(ts.seq_ptr, ts.item_ptr, ts.attr_id, ts.labels, A, L, ts.state_fid.ravel(),
                                             ts.trans_fid.ravel(), w, ts.attr_value)
        else:
            f, g, _ = tv.objective(ts.seq_ptr, ts.item_ptr, ts.attr_id, ts.labels, A, L, window, 1, ts.state_fid.ravel(),
                                   ts.trans_fid.ravel(), w, ts.attr_value)
        return f + 0.15 * float(w @ w), g + 2 * 0.15 * w

    x = crf.training_result_.x
    ref = scipy.optimize.minimize(fg, np.zeros(ts.num_features), jac=True, method="L-BFGS-B",
                                  options={"ftol": 1e-15, "gtol": 1e-10, "maxiter": 10000})
    f_ours = fg(x)[0]
    print(f"f = {f_ours!r}, scipy {ref.fun!r}; max |x - scipy| = {np.abs(x - ref.x).max():.3g}")
    assert abs(f_ours - ref.fun) <= 1e-8 * abs(ref.fun), (f_ours, ref.fun, crf.training_result_)
    assert np.abs(x - ref.x).max() <= 1e-4
    # the score separates a from b; the same data with the score as a plain name cannot
    Xt, yt = _scored_data(np.random.default_rng(78), n_seqs=15)
    acc = _accuracy_ab(crf, Xt, yt)
    strip = lambda data: [[["bias", "kind:" + it["kind"], "score"] + (["odd"] if it["odd"] else []) for it in xs] for xs in data]
    blind = SequenceCRF(window_size=window, **options).fit(strip(X), y)
    acc_blind = _accuracy_ab(blind, strip(Xt), yt)
    print(f"a-or-b items labelled right: {acc:.3f} with values, {acc_blind:.3f} with the score as a plain name")
    assert acc >= 0.95 and acc_blind <= 0.65
    if window is None:
        # the log-space training kernels against the scaled-scan inference kernels: the likelihood of the training data
        ll = crf.log_likelihood(X, y)
        f, _ = _native.TrainerSequences([ts.native_args()], values=[ts.attr_value]).eval([x])
        tol_f, _ = tv.objective_sequences_tolerances(ts.seq_ptr, ts.item_ptr, ts.attr_id, ts.labels, A, L,
                                                     ts.state_fid.ravel(), ts.trans_fid.ravel(), x, ts.attr_value)
        print(f"-sum(log_likelihood) = {-ll.sum()!r}, trainer f = {f[0]!r}: difference {abs(-ll.sum() - f[0]):.3g} (bound {tol_f:.3g})")
        assert np.all(ll < 0) and abs(-ll.sum() - f[0]) <= tol_f


def test_valued_sets_route_to_the_general_kernels(monkeypatch):
    """``fit_training_set``, ``fit_training_sets`` and ``fit_grid``: a valued windowed set of two labels takes
    ``TrainerGeneral``, a valued whole-sequence set ``TrainerSequences``, each with its values, and every result is the lone
    fit's; an unvalued set beside them routes as before."""
    from gecco_amd import _native, train

    rng = np.random.default_rng(5)
    X, y = _scored_data(rng, n_seqs=12)
    two = [[lab if lab != "c" else "a" for lab in ls] for ls in y]
    pairs = [[list(zip(*train.item_attributes(item))) for item in xs] for xs in X]
    names = [[[nm for nm, _ in item] for item in xs] for xs in pairs]
    sets = [train.build_training_set(pairs, two, 5, 1), train.build_training_set(names, two, 5, 1),
            train.build_training_set(pairs, y, 5, 1, max_labels=3)]
    whole = [train.build_training_set(pairs, two, None, None), train.build_training_set(names, y, None, None, max_labels=3)]
    assert [ts.attr_value is None for ts in sets] == [False, True, False]
    made = []
    for family in ("Trainer", "TrainerBatch", "TrainerGrid", "TrainerGeneral", "TrainerSequences"):
        base = getattr(_native, family)

        def init(self, *a, _base=base, _family=family, **kw):
            made.append((_family, [v is not None for v in kw.get("values") or []]))
            _base.__init__(self, *a, **kw)

        monkeypatch.setattr(_native, family, type(family, (base,), {"__init__": init}))
    params = train.trainer_params({"c1": 0.05, "c2": 0.1, "max_iterations": 15})
    lone = [train.fit_training_set(ts, params) for ts in sets]
    assert made == [("TrainerGeneral", [True]), ("Trainer", []), ("TrainerGeneral", [True])]
    del made[:]
    lone_whole = [train.fit_training_set(ts, params) for ts in whole]
    assert made == [("TrainerSequences", [True]), ("TrainerSequences", [])]
    del made[:]
    same = lambda a, b: a.x.tobytes() == b.x.tobytes() and a.n_iter == b.n_iter and a.status == b.status
    res = train.fit_training_sets(sets, params)
    assert sorted(made) == [("TrainerBatch", []), ("TrainerGeneral", [True, True])] and all(map(same, res, lone))
    del made[:]
    res = train.fit_grid(sets + whole, [(k, params) for k in range(5)])
    assert sorted(made) == [("TrainerGeneral", [True, True]), ("TrainerGrid", []), ("TrainerSequences", [True, False])]
    assert all(map(same, res, lone + lone_whole))
    assert all(r.n_iter > 0 for r in lone + lone_whole)
