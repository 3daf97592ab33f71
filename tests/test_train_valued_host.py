"""Real-valued attributes on the host: the valued yardstick (tests/train_objective_valued.py) against enumeration of every
label path and against the unvalued yardstick on the CSR that lists an attribute of value k k times; the training-set
builder's frequencies, ``min_freq`` and refusals with values; python-crfsuite's dict conversion case by case."""
import itertools

import numpy as np
import pytest

from tests import train_objective_valued as tv
from tests.train_objective_labels import labelled_sequences, objective as objective_unvalued
from tests.train_objective_labels import objective_tolerances as tolerances_unvalued
from tests.train_objective_sequences import objective_sequences as objective_sequences_unvalued
from tests.train_objective_sequences import objective_sequences_tolerances as sequences_tolerances_unvalued


# ---------------------------------------------------------------- enumeration of every label path
def _enumerate(score, labels, T, instances):
    """f, per-item expected label counts [n, L] and expected transition counts by summing over every path of every
    instance (a list of item index lists)."""
    n, L = score.shape
    f, item, dT = 0.0, np.zeros((n, L)), np.zeros((L, L))
    for items in instances:
        paths = list(itertools.product(range(L), repeat=len(items)))
        sc = np.array([sum(score[i, y] for i, y in zip(items, p)) + sum(T[a, b] for a, b in zip(p[:-1], p[1:])) for p in paths])
        mx = sc.max()
        logz = mx + np.log(np.exp(sc - mx).sum())
        prob = np.exp(sc - logz)
        gold = tuple(int(labels[i]) for i in items)
        f += logz - sc[paths.index(gold)]
        for p, pr in zip(paths, prob):
            for i, y in zip(items, p):
                item[i, y] += pr
            for a, b in zip(p[:-1], p[1:]):
                dT[a, b] += pr
    return f, item, dT


def _tiny(rng, L, lengths, A=5):
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, lengths, A, L, stay=0.6)
    values = rng.normal(0.0, 1.0, size=len(attr_id))
    values[::3] = -0.75   # a negative
    values[1::4] = 0.0    # an exact zero
    values[2::5] = 0.3125  # a fraction
    fid = np.arange(A * L + L * L, dtype=np.int32)
    fid[[1, A * L + 1]] = -1
    keep = fid >= 0
    fid[keep] = np.arange(int(keep.sum()))
    return seq_ptr, item_ptr, attr_id, labels, A, fid[:A * L], fid[A * L:], int(keep.sum()), values


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("whole", [False, True])
def test_yardstick_against_path_enumeration(L, whole):
    rng = np.random.default_rng(100 * L + whole)
    lengths = [1, 2, 3, 4, 4, 3, 2, 1] if whole else [2, 3, 4, 4, 2]
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K, values = _tiny(rng, L, lengths)
    assert (values < 0).any() and (values == 0).any() and len(attr_id) > 10
    w = rng.normal(0.0, 1.5, size=K)
    _, _, S, T = tv.dense_tables(A, L, sfid, tfid, w)
    score = np.zeros((len(labels), L))
    for i in range(len(labels)):
        for k in range(item_ptr[i], item_ptr[i + 1]):
            score[i] += values[k] * S[attr_id[k]]
    for W, step in ((None, None),) if whole else ((1, 1), (2, 1), (2, 2)):
        if whole:
            instances = [list(range(seq_ptr[s], seq_ptr[s + 1])) for s in range(len(lengths))]
            f, g, n_inst = tv.objective_sequences(seq_ptr, item_ptr, attr_id, labels, A, L, sfid, tfid, w, values)
        else:
            instances = [list(range(b, b + W)) for s in range(len(lengths)) for b in range(seq_ptr[s], seq_ptr[s + 1] - W + 1, step)]
            f, g, n_inst = tv.objective(seq_ptr, item_ptr, attr_id, labels, A, L, W, step, sfid, tfid, w, values)
        assert n_inst == len(instances)
        ef, item, dT = _enumerate(score, labels, T, instances)
        eg = np.zeros(K)
        cover = np.zeros(len(labels))
        for items in instances:
            for i in items:
                cover[i] += 1
            for a, b in zip(items[:-1], items[1:]):
                if tfid[labels[a] * L + labels[b]] >= 0:
                    eg[tfid[labels[a] * L + labels[b]]] -= 1.0
        for i in range(len(labels)):
            for k in range(item_ptr[i], item_ptr[i + 1]):
                for y in range(L):
                    fid = sfid[attr_id[k] * L + y]
                    if fid >= 0:
                        eg[fid] += values[k] * item[i, y] - values[k] * cover[i] * (labels[i] == y)
        for a in range(L):
            for b in range(L):
                if tfid[a * L + b] >= 0:
                    eg[tfid[a * L + b]] += dT[a, b]
        assert abs(f - ef) <= 1e-12 * max(1.0, abs(ef)), (f, ef)
        assert np.abs(g - eg).max() <= 1e-12 * (1 + np.abs(eg).max())


def test_inference_yardstick_against_path_enumeration():
    rng = np.random.default_rng(5)
    L, A = 3, 4
    seq_ptr = np.array([0, 4, 4, 5, 8])
    item_ptr = np.array([0, 2, 2, 3, 5, 6, 8, 9, 10])
    attr_id = rng.integers(0, A, size=10)
    attr_id[3] = A + 2  # an unknown id carries no weight
    values = rng.normal(size=10)
    values[3] = 1e6
    S, T = rng.normal(size=(A, L)), rng.normal(size=(L, L))
    score = tv.item_scores(item_ptr, attr_id, values, S)
    assert np.all(score[1] == 0.0) and np.allclose(score[2], values[2] * S[attr_id[2]])
    marg, logz = tv.marginals_sequences(seq_ptr, item_ptr, attr_id, values, S, T)
    y, sc = tv.viterbi(seq_ptr, item_ptr, attr_id, values, S, T)
    assert logz[1] == 0.0 and sc[1] == 0.0
    for s in (0, 2, 3):
        items = list(range(seq_ptr[s], seq_ptr[s + 1]))
        ef, item, _ = _enumerate(score, np.zeros(len(score), dtype=int), T, [items])
        assert np.abs(marg[items] - item[items]).max() <= 1e-13
        paths = list(itertools.product(range(L), repeat=len(items)))
        best = max(paths, key=lambda p: tv.path_score(score[items], T, p))
        assert tuple(y[items]) == best and sc[s] == tv.path_score(score[items], T, best)
    # windows of 3 at step 2 over a sequence of 4 (item 3 uncovered), of 1 (padded, one item in front), of 3 (one window)
    p_all, p_any = tv.windowed(seq_ptr, item_ptr, attr_id, values, S, T, 3, 2, background=0)
    _, item, _ = _enumerate(score, np.zeros(len(score), dtype=int), T, [[0, 1, 2]])
    assert np.abs(p_all[:3] - item[:3]).max() <= 1e-13 and np.all(p_all[3] == 0.0) and p_any[3] == 0.0
    assert np.abs(p_any[:3] - (item[:3, 1] + item[:3, 2])).max() <= 1e-13
    pad = np.vstack([np.zeros(L), score[4], np.zeros(L)])
    _, item, _ = _enumerate(pad, np.zeros(3, dtype=int), T, [[0, 1, 2]])
    assert np.abs(p_all[4] - item[1]).max() <= 1e-13
    p_all, p_any = tv.windowed(seq_ptr, item_ptr, attr_id, values, S, T, 3, 1, background=1, pad=False)
    assert np.all(np.isnan(p_all[4])) and np.isnan(p_any[4]) and np.all(np.isfinite(p_all[:4]))
    # a strict `<` update keeps the first of tied labels
    y, _ = tv.viterbi_scores(np.zeros((4, 3)), np.zeros((3, 3)))
    assert y.tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------- the duplication identity
@pytest.mark.parametrize("L,W,step", [(2, 5, 2), (3, 1, 1), (5, 20, 1), (8, None, None)])
def test_integer_values_are_repeated_attributes(L, W, step):
    """Values in {1, 2, 3}: the valued yardstick equals the unvalued one (its np.add.at scatter sums duplicates) on the CSR
    that lists an attribute of value k k times, within the unvalued bounds."""
    rng = np.random.default_rng(40 + L)
    A = 12
    lengths = [int(x) for x in rng.integers(W or 1, 30, size=12)]
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, lengths, A, L)
    values = rng.integers(1, 4, size=len(attr_id)).astype(np.float64)
    deg = np.diff(item_ptr)
    owner = np.repeat(np.arange(len(labels)), deg)
    rep = values.astype(np.int64)
    dup_attr = np.repeat(attr_id, rep)
    dup_deg = np.zeros(len(labels), dtype=np.int64)
    np.add.at(dup_deg, owner, rep)
    dup_ptr = np.concatenate([[0], np.cumsum(dup_deg)]).astype(np.int32)
    K = A * L + L * L
    sfid, tfid = np.arange(A * L), A * L + np.arange(L * L)
    w = rng.normal(0.0, 1.5, size=K)
    if W is None:
        f, g, _ = tv.objective_sequences(seq_ptr, item_ptr, attr_id, labels, A, L, sfid, tfid, w, values)
        ef, eg, _ = objective_sequences_unvalued(seq_ptr, dup_ptr, dup_attr, labels, A, L, sfid, tfid, w)
        tol_f, tol_g = sequences_tolerances_unvalued(seq_ptr, dup_ptr, dup_attr, labels, A, L, sfid, tfid, w)
        assert abs(f - ef) <= tol_f and np.all(np.abs(g - eg) <= tol_g)
        return
    f, g, nw = tv.objective(seq_ptr, item_ptr, attr_id, labels, A, L, W, step, sfid, tfid, w, values)
    ef, eg, enw, details = objective_unvalued(seq_ptr, dup_ptr, dup_attr, labels, A, L, W, step, sfid, tfid, w, details=True)
    tol_f, tol_g = tolerances_unvalued(seq_ptr, dup_ptr, dup_attr, L, W, step, sfid, tfid, w, details)
    assert nw == enw and abs(f - ef) <= tol_f and np.all(np.abs(g - eg) <= tol_g)
    # and the valued bounds are no tighter than a rounding of the values they bound
    vf, vg = tv.objective_tolerances(seq_ptr, item_ptr, attr_id, labels, A, L, W, step, sfid, tfid, w, values)
    assert vf > 0 and np.all(vg > 0) and abs(f - ef) <= vf and np.all(np.abs(g - eg) <= vg)


# ---------------------------------------------------------------- the training-set builder
def _named(rng, n_seqs=6, L=3, A=8, lo=5, hi=12):
    lengths = [int(x) for x in rng.integers(lo, hi + 1, size=n_seqs)]
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, lengths, A, L, stay=0.7)
    X, y = [], []
    for s in range(n_seqs):
        X.append([[f"a{a}" for a in attr_id[item_ptr[i]:item_ptr[i + 1]]] for i in range(seq_ptr[s], seq_ptr[s + 1])])
        y.append([f"t{v}" for v in labels[seq_ptr[s]:seq_ptr[s + 1]]])
    return X, y


@pytest.mark.parametrize("window,step", [(None, None), (3, 1), (4, 3)])
def test_build_training_set_with_values(window, step):
    from gecco_amd import train

    rng = np.random.default_rng(9)
    X, y = _named(rng)
    plain = train.build_training_set(X, y, window, step, max_labels=8)
    assert plain.attr_value is None and len(plain.native_args()) == (8 if window is None else 10)
    vals = iter(tv.mixed_values(rng, 10000).tolist())
    Xv = [[[(a, next(vals)) for a in item] for item in xs] for xs in X]
    Xv[0][0] = list(Xv[0][0]) + [("only zero", 0.0)]
    ts = train.build_training_set(Xv, y, window, step, max_labels=8)
    assert ts.attr_value is not None and ts.attr_value.dtype == np.float64 and len(ts.attr_value) == len(ts.attr_id)
    assert ts.native_args()[2] is ts.attr_id and len(ts.native_args()) == len(plain.native_args())
    # a pair seen only with value 0 keeps its feature (frequency 0 >= min_freq 0)
    a0 = ts.attrs_.index("only zero")
    lab0 = ts.labels[0]
    cov0 = 1 if window is None else int(train._coverage(len(X[0]), window, step)[0])
    assert (ts.state_fid[a0, lab0] >= 0) == (cov0 > 0)
    # frequencies are sums of value x coverage, and min_freq compares the sums
    A, L = len(ts.attrs_), ts.num_labels
    freq = np.zeros((A, L))
    seen = np.zeros((A, L), dtype=bool)
    for s, xs in enumerate(Xv):
        cov = np.ones(len(xs), dtype=int) if window is None else train._coverage(len(xs), window, step)
        for i, item in enumerate(xs):
            lab = ts.labels[ts.seq_ptr[s] + i]
            for name, v in item:
                if cov[i] > 0:
                    freq[ts.attrs_.index(name), lab] += v * cov[i]
                    seen[ts.attrs_.index(name), lab] = True
    # (CRFsuite keeps a feature whose frequency is at least min_freq: at the default 0 a negative sum is dropped, a zero kept)
    assert np.array_equal(ts.state_fid >= 0, seen & (freq >= 0.0)) and (seen & (freq < 0.0)).any()
    for min_freq in (0.5, 3.0):
        cut = train.build_training_set(Xv, y, window, step, min_freq=min_freq, max_labels=8)
        assert np.array_equal(cut.state_fid >= 0, seen & (freq >= min_freq)), min_freq
        assert (cut.state_fid >= 0).sum() < seen.sum()
    # mappings are the same items
    as_dict = train.build_training_set([[dict(item) for item in xs] for xs in Xv], y, window, step, max_labels=8)
    for name in ("attr_id", "attr_value", "item_ptr", "state_fid", "trans_fid"):
        assert np.array_equal(getattr(as_dict, name), getattr(ts, name)), name


def test_build_training_set_plain_names_are_what_they_were():
    """Every field of a plain-name set against a restatement of the unvalued builder's outputs: all values 1.0 give the
    same ids, pointers and features, and the plain set has no values."""
    from gecco_amd import train

    X, y = _named(np.random.default_rng(3))
    for window, step in ((None, None), (3, 2)):
        plain = train.build_training_set(X, y, window, step, min_freq=2.0, max_labels=8)
        ones = train.build_training_set([[[(a, 1.0) for a in item] for item in xs] for xs in X], y, window, step, min_freq=2.0,
                                        max_labels=8)
        assert plain.attr_value is None and np.all(ones.attr_value == 1.0)
        for name, value in plain.__dict__.items():
            if name == "attr_value":
                continue
            other = getattr(ones, name)
            if isinstance(value, np.ndarray):
                assert value.dtype == other.dtype and np.array_equal(value, other), name
            else:
                assert value == other, name
        # first-appearance ids and CSR
        names = []
        for s, xs in enumerate(X):
            cov = np.ones(len(xs), dtype=int) if window is None else train._coverage(len(xs), window, step)
            for item, c in zip(xs, cov):
                names.extend(a for a in item if c > 0 and a not in names)
        assert plain.attrs_ == names
        flat = [a for xs in X for item in xs for a in item if a in names]
        assert [plain.attrs_[k] for k in plain.attr_id] == flat
        assert plain.attr_id.dtype == np.int32 and plain.item_ptr.dtype == np.int32 and plain.seq_ptr.dtype == np.int32


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_values_are_refused(bad):
    from gecco_amd import train

    X, y = _named(np.random.default_rng(1))
    Xv = [[[(a, 1.0) for a in item] for item in xs] for xs in X]
    Xv[2][1] = [("a0", bad)]
    with pytest.raises(ValueError, match="finite"):
        train.build_training_set(Xv, y, None, None, max_labels=8)
    with pytest.raises(ValueError, match="finite"):
        train.item_attributes({"score": bad})


def test_dict_conversion():
    """python-crfsuite's ItemSequence conversion, case by case."""
    from gecco_amd.train import item_attributes

    assert item_attributes({"score": 0.37, "count": 3}) == (["score", "count"], [0.37, 3.0])
    assert item_attributes({"upper": True, "digit": False}) == (["upper", "digit"], [1.0, 0.0])
    assert item_attributes({"word": "x"}) == (["word:x"], [1.0])
    assert item_attributes({"tags": ["s1", "s2"]}) == (["tags:s1", "tags:s2"], [1.0, 1.0])
    names, values = item_attributes({"tags": {"s1"}})
    assert (names, values) == (["tags:s1"], [1.0])
    assert item_attributes({"k": {"inner": 2.5, "deep": {"w": "x", "b": True}}}) == (["k:inner", "k:deep:w:x", "k:deep:b"], [2.5, 1.0, 1.0])
    assert item_attributes({"bias": 1.0, "neg": -2.0, "zero": 0}) == (["bias", "neg", "zero"], [1.0, -2.0, 0.0])
    assert item_attributes({"np": np.float32(0.5), "flag": np.bool_(True)}) == (["np", "flag"], [0.5, 1.0])
    # a list of names stays what it is; pairs carry their values, a bare name among them weighs 1
    assert item_attributes(["a", "b", "a"]) == (["a", "b", "a"], None)
    assert item_attributes([]) == ([], None)
    assert item_attributes([("a", 2.0), "b"]) == (["a", "b"], [2.0, 1.0])
    assert item_attributes({}) == ([], [])
    with pytest.raises(ValueError, match="not a string"):
        item_attributes("abc")
    with pytest.raises(ValueError, match="a value is"):
        item_attributes({"k": object()})


def test_sequence_crf_items_helper():
    """Plain names keep the unvalued path (values None, duplicates collapsed); one dict item gives the whole sequence
    values, 1.0 for the attributes of its plain items."""
    from gecco_amd.sequence import _items

    assert _items([["a", "b", "a"], []]) == ([["a", "b"], []], None)
    assert _items([["a", "a"], {"s": 0.5, "w": "x"}]) == ([["a"], ["s", "w:x"]], [[1.0], [0.5, 1.0]])
    assert _items([[("a", 2.0), ("a", 3.0)]]) == ([["a", "a"]], [[2.0, 3.0]])
    with pytest.raises(ValueError, match="not a string"):
        _items(["abc"])


def test_scratch_restatements_grow_by_the_transpose():
    from gecco_amd import train

    X, y = _named(np.random.default_rng(2))
    Xv = [[[(a, 0.5) for a in item] for item in xs] for xs in X]
    for window, step, scratch in ((None, None, train._sequences_scratch_bytes), (3, 1, train._general_scratch_bytes)):
        plain = train.build_training_set(X, y, window, step, max_labels=8)
        valued = train.build_training_set(Xv, y, window, step, max_labels=8)
        assert scratch(valued) == scratch(plain) + 8 * len(valued.attr_id)
