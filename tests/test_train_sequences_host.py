"""Whole-sequence training, the parts that need no GPU: the numpy yardstick (tests/train_objective_sequences.py) against
path enumeration, ``build_training_set(window=None)``, and the argument handling of ``SequenceCRF(window_size=None)``
and ``SequenceCRF.log_likelihood``."""
import itertools

import numpy as np
import pytest

from tests.train_objective_sequences import (length_groups, objective_sequences, objective_sequences_tolerances,
                                             sequences_problem, subproblem)


# ---------------------------------------------------------------- the yardstick against the definition
def _enumerate(seq_ptr, item_ptr, attr_id, labels, A, L, sfid, tfid, w):
    """f and g by listing all L^n label paths of every sequence (fp64, no recursion and no log-sum-exp beyond the one
    over the paths)."""
    sfid, tfid = np.asarray(sfid).reshape(A, L), np.asarray(tfid).reshape(L, L)
    S = np.where(sfid >= 0, w[np.maximum(sfid, 0)], 0.0)
    T = np.where(tfid >= 0, w[np.maximum(tfid, 0)], 0.0)
    f, g = 0.0, np.zeros(len(w))
    for s in range(len(seq_ptr) - 1):
        b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        attrs = [attr_id[item_ptr[i]:item_ptr[i + 1]] for i in range(b, e)]
        paths = list(itertools.product(range(L), repeat=e - b))
        sc = np.array([sum(S[a, y[t]] for t in range(e - b) for a in attrs[t]) + sum(T[y[t - 1], y[t]] for t in range(1, e - b))
                       for y in paths])
        top = sc.max()
        p = np.exp(sc - top)
        z = p.sum()
        gold = tuple(int(v) for v in labels[b:e])
        f += top + np.log(z) - sc[paths.index(gold)]
        for y, q in zip(paths, p / z):
            q -= 1.0 if y == gold else 0.0  # expected - empirical
            for t in range(e - b):
                for a in attrs[t]:
                    if sfid[a, y[t]] >= 0:
                        g[sfid[a, y[t]]] += q
                if t > 0 and tfid[y[t - 1], y[t]] >= 0:
                    g[tfid[y[t - 1], y[t]]] += q
    return f, g


@pytest.mark.parametrize("L,lengths", [(3, [1, 2, 4, 1, 3, 5, 2]), (2, [5, 1, 1, 3]), (3, [1]), (2, [2, 2, 4, 5, 3])])
def test_yardstick_matches_path_enumeration(L, lengths):
    """At unit-scale weights both sides are sums of at most 3^5 = 243 positive terms and a handful of scores of size
    about 10, each rounded to eps = 2.2e-16: f to 1e-13 relative and g to 1e-12 (1 + |g|) leave two orders of margin
    over 243 eps and fail on any wrong term (a missing transition moves f by about 1)."""
    rng = np.random.default_rng(40 + L + len(lengths))
    p = sequences_problem(rng, L, lengths, A=6)
    w = rng.normal(0, 1.5, size=p[7])
    f, g, n = objective_sequences(*p[:5], L, p[5], p[6], w)
    ef, eg = _enumerate(*p[:5], L, p[5], p[6], w)
    assert n == len(lengths)
    print(f"L={L} lengths={lengths}: |f - enum| = {abs(f - ef):.3g}, max |g - enum| = {np.abs(g - eg).max():.3g}")
    assert abs(f - ef) <= 1e-13 * abs(ef), (f, ef)
    assert np.all(np.abs(g - eg) <= 1e-12 * (1 + np.abs(eg)))


def test_subproblems_and_tolerances():
    rng = np.random.default_rng(3)
    p = sequences_problem(rng, 3, [2, 5, 2, 1, 5, 5], A=6)
    assert length_groups(p[0]) == {2: [0, 2], 5: [1, 4, 5], 1: [3]}
    seq_ptr, item_ptr, attr_id, labels = subproblem(*p[:4], [4, 0])
    assert seq_ptr.tolist() == [0, 5, 7]
    assert labels.tolist() == p[3][10:15].tolist() + p[3][0:2].tolist()
    assert attr_id.tolist() == p[2][p[1][10]:p[1][15]].tolist() + p[2][p[1][0]:p[1][2]].tolist()
    assert item_ptr[-1] == len(attr_id) and np.all(np.diff(item_ptr) >= 0)
    w = rng.normal(0, 1.5, size=p[7])
    tol_f, tol_g = objective_sequences_tolerances(*p[:5], 3, p[5], p[6], w)
    assert 0 < tol_f < 1e-9 and tol_g.shape == (p[7],) and np.all(tol_g > 0) and np.all(tol_g < 1e-9)


# ---------------------------------------------------------------- feature generation over whole sequences
X = [[["a", "b"], ["b"], [], ["c"]], [["b", "d"]], [["a"], ["a", "c"]]]
Y = [["x", "x", "y", "x"], ["z"], ["y", "y"]]


def test_build_training_set_whole_sequences():
    from gecco_amd import train

    ts = train.build_training_set(X, Y, None, None, max_labels=3)
    assert ts.window is None and ts.step is None
    assert ts.labels_ == ["x", "y", "z"] and ts.attrs_ == ["a", "b", "c", "d"]  # first appearance; a name before its item's label
    assert ts.seq_ptr.tolist() == [0, 4, 5, 7] and ts.item_ptr.tolist() == [0, 2, 3, 3, 4, 6, 7, 9]
    assert ts.attr_id.tolist() == [0, 1, 1, 2, 1, 3, 0, 0, 2] and ts.labels.tolist() == [0, 0, 1, 0, 2, 1, 1]
    # observed pairs, (attribute, label) order: a/x a/y b/x b/z c/x c/y d/z; then x>x x>y y>x y>y (1 + 1 + 1 + 1)
    assert list(zip(ts.state_attr.tolist(), ts.state_label.tolist())) == [(0, 0), (0, 1), (1, 0), (1, 2), (2, 0), (2, 1), (3, 2)]
    assert list(zip(ts.trans_src.tolist(), ts.trans_dst.tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert ts.state_fid[0].tolist() == [0, 1, -1] and ts.trans_fid.tolist() == [[7, 8, -1], [9, 10, -1], [-1, -1, -1]]
    assert len(ts.native_args()) == 8 and ts.native_args()[7] == ts.num_features == 11
    assert train.build_training_set(X, Y, max_labels=3).state_fid.tolist() == ts.state_fid.tolist()  # (the default)

    # min_freq on plain counts: a/y (a appears twice beside y) and b/x (twice) stay, no transition does
    ts2 = train.build_training_set(X, Y, None, None, min_freq=2, max_labels=3)
    assert list(zip(ts2.state_attr.tolist(), ts2.state_label.tolist())) == [(0, 1), (1, 0)] and len(ts2.trans_src) == 0
    ts3 = train.build_training_set(X, Y, None, None, all_possible_states=True, all_possible_transitions=True, max_labels=3)
    assert len(ts3.state_attr) == 12 and len(ts3.trans_src) == 9
    ts4 = train.build_training_set(X, Y, None, None, min_freq=1, all_possible_transitions=True, max_labels=3)
    assert len(ts4.trans_src) == 4  # (possible but unobserved transitions have frequency 0)


def test_whole_sequences_of_equal_length_are_one_window_each():
    from gecco_amd import train

    rng = np.random.default_rng(17)
    n = 6
    seqs = [[[f"a{a}" for a in rng.integers(0, 9, size=int(rng.integers(0, 3)))] for _ in range(n)] for _ in range(12)]
    seqs = [[list(dict.fromkeys(it)) for it in xs] for xs in seqs]
    labs = [[f"y{int(v)}" for v in rng.integers(0, 3, size=n)] for _ in range(12)]
    for kw in ({}, {"min_freq": 2.0}, {"all_possible_states": True}, {"all_possible_transitions": True, "min_freq": 1.0}):
        whole = train.build_training_set(seqs, labs, None, None, max_labels=4, **kw)
        windowed = train.build_training_set(seqs, labs, n, 1, max_labels=4, **kw)
        assert whole.labels_ == windowed.labels_ and whole.attrs_ == windowed.attrs_
        for name in ("seq_ptr", "item_ptr", "attr_id", "labels", "state_attr", "state_label", "trans_src", "trans_dst",
                     "state_fid", "trans_fid"):
            a, b = getattr(whole, name), getattr(windowed, name)
            assert a.dtype == b.dtype and a.tolist() == b.tolist(), (kw, name)
        assert whole.window is None and windowed.window == n


def test_build_training_set_refuses_an_empty_sequence():
    from gecco_amd import train

    with pytest.raises(ValueError, match="sequence 1 has no items"):
        train.build_training_set([X[0], [], X[2]], [Y[0], [], Y[2]], None, None, max_labels=3)
    with pytest.raises(ValueError, match="exactly 2 labels"):
        train.build_training_set(X, Y, None, None)


# ---------------------------------------------------------------- the estimator's arguments
def _model_bytes():
    from gecco_amd import crfsuite_model

    # attributes a, b; labels x, y: every state pair and transition has a weight
    return crfsuite_model.model_bytes(["x", "y"], ["a", "b"], [0, 0, 1, 1], [0, 1, 0, 1], [0, 0, 1, 1], [0, 1, 0, 1],
                                      np.array([1.0, -1.0, -0.5, 0.5, 0.25, -0.25, -0.75, 0.75]))


def test_sequence_crf_without_a_window(tmp_path):
    from gecco_amd.sequence import SequenceCRF

    crf = SequenceCRF(window_size=None, window_step=7, c2=0.5)
    assert crf.window_size is None and crf.window_step == 1 and crf.params["c2"] == 0.5
    for bad in (0, 33):  # (the window's own limits stay)
        with pytest.raises(ValueError, match="window_size must lie in 1..32"):
            SequenceCRF(window_size=bad)
    with pytest.raises(ValueError, match="not fitted"):
        crf.predict_windowed([[["a"]]], "x")
    with pytest.raises(ValueError, match="sequence 1: 1 items but 2 labels"):
        crf.fit([[["a"]], [["a"]]], [["x"], ["x", "y"]])
    with pytest.raises(ValueError, match="sequence 1 has no items"):
        crf.fit([[["a"], ["b"]], []], [["x", "y"], []])

    blob = _model_bytes()
    (tmp_path / "m.crfsuite").write_bytes(blob)
    for loaded in (SequenceCRF.from_bytes(blob, window_size=None, window_step=3),
                   SequenceCRF.load(tmp_path / "m.crfsuite", window_size=None)):
        assert loaded.window_size is None and loaded.window_step == 1
        assert loaded.classes_ == ["x", "y"] and loaded.to_bytes() == blob
        with pytest.raises(ValueError, match="has no window"):
            loaded.predict_windowed([[["a"]]], "x")
        with pytest.raises(ValueError, match="has no window"):
            loaded.predict_windowed_all([[["a"]]])
        with pytest.raises(ValueError, match="has no window"):
            loaded.predict_windowed_all([[["a"]]], background="x")


def test_log_likelihood_arguments():
    from gecco_amd.sequence import SequenceCRF

    with pytest.raises(ValueError, match="not fitted"):
        SequenceCRF(window_size=None).log_likelihood([[["a"]]], [["x"]])
    for crf in (SequenceCRF.from_bytes(_model_bytes(), window_size=None), SequenceCRF.from_bytes(_model_bytes(), window_size=5)):
        with pytest.raises(ValueError, match="unknown label 'z'"):
            crf.log_likelihood([[["a"], ["b"]]], [["x", "z"]])
        with pytest.raises(ValueError, match="X holds 1 sequences and y 2"):
            crf.log_likelihood([[["a"]]], [["x"], ["y"]])
        with pytest.raises(ValueError, match="sequence 0: 2 items but 1 labels"):
            crf.log_likelihood([[["a"], ["b"]]], [["x"]])
        out = crf.log_likelihood([], [])
        assert isinstance(out, np.ndarray) and out.shape == (0,) and out.dtype == np.float64
        assert crf.log_likelihood([[], []], [[], []]).tolist() == [0.0, 0.0]  # (no device work)
