"""Host side of training with more than two labels: ``build_training_set(max_labels=...)`` on a toy set counted by hand,
the argument checks of ``SequenceCRF``, and the model writer's round trip for three labels."""
import numpy as np
import pytest

from gecco_amd import train

# window 2, step 1.  Coverage: [1, 2, 1] and [1, 1].  Labels X, Y, Z and attributes a, b, c in order of appearance.
SEQS = [[["a"], ["a", "b"], ["b"]], [["a"], ["c"]]]
LABS = [["X", "Y", "Z"], ["X", "X"]]
# state features seen, with their frequencies (once per window holding the item):
#   (a, X) 2   (a, Y) 2   (b, Y) 2   (b, Z) 1   (c, X) 1;   transitions: (X, X) 1   (X, Y) 1   (Y, Z) 1


def test_three_labels_counted_by_hand():
    ts = train.build_training_set(SEQS, LABS, 2, 1, max_labels=3)
    assert ts.labels_ == ["X", "Y", "Z"] and ts.attrs_ == ["a", "b", "c"] and ts.num_labels == 3
    assert ts.labels.tolist() == [0, 1, 2, 0, 0]
    assert ts.seq_ptr.tolist() == [0, 3, 5] and ts.item_ptr.tolist() == [0, 1, 3, 4, 5, 6]
    assert ts.attr_id.tolist() == [0, 0, 1, 1, 0, 2]
    assert ts.state_fid.shape == (3, 3) and ts.trans_fid.shape == (3, 3)
    assert ts.state_fid.tolist() == [[0, 1, -1], [-1, 2, 3], [4, -1, -1]]
    assert ts.trans_fid.tolist() == [[5, 6, -1], [-1, -1, 7], [-1, -1, -1]]
    assert ts.num_features == 8
    assert ts.state_attr.tolist() == [0, 0, 1, 1, 2] and ts.state_label.tolist() == [0, 1, 1, 2, 0]
    assert ts.trans_src.tolist() == [0, 0, 1] and ts.trans_dst.tolist() == [0, 1, 2]
    assert ts.native_args()[5].shape == (3, 3)


def test_min_freq_and_all_possible_switches():
    ts = train.build_training_set(SEQS, LABS, 2, 1, min_freq=2, max_labels=8)
    assert ts.state_fid.tolist() == [[0, 1, -1], [-1, 2, -1], [-1, -1, -1]]
    assert (ts.trans_fid == -1).all() and ts.num_features == 3
    ts = train.build_training_set(SEQS, LABS, 2, 1, all_possible_states=True, max_labels=3)
    assert ts.state_fid.tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    assert ts.trans_fid.tolist() == [[9, 10, -1], [-1, -1, 11], [-1, -1, -1]]
    ts = train.build_training_set(SEQS, LABS, 2, 1, all_possible_transitions=True, max_labels=3)
    assert ts.trans_fid.tolist() == [[5, 6, 7], [8, 9, 10], [11, 12, 13]] and ts.num_features == 14
    # (with min_freq, the unobserved pairs the switches add have frequency 0 and go again)
    ts = train.build_training_set(SEQS, LABS, 2, 1, min_freq=1, all_possible_states=True, all_possible_transitions=True,
                                  max_labels=3)
    assert ts.num_features == 8


def test_label_count_limits():
    with pytest.raises(ValueError, match="training needs exactly 2 labels, found 3"):
        train.build_training_set(SEQS, LABS, 2, 1)
    with pytest.raises(ValueError, match="training needs exactly 2 labels"):
        train.build_training_set(SEQS, LABS, 2, 1, max_labels=2)
    for bad in (1, 33, 0):
        with pytest.raises(ValueError, match="max_labels must lie in 2..32"):
            train.build_training_set(SEQS, LABS, 2, 1, max_labels=bad)
    one = [["X", "X", "X"], ["X", "X"]]
    with pytest.raises(ValueError, match="training needs 2 to 5 labels, found 1"):
        train.build_training_set(SEQS, one, 2, 1, max_labels=5)
    many = [[[f"a{i}"] for i in range(40)]]
    with pytest.raises(ValueError, match="training needs 2 to 32 labels, found 40"):
        train.build_training_set(many, [[f"y{i}" for i in range(40)]], 2, 1, max_labels=32)
    # a two-label set is the same set with or without the limit raised
    two = [["X", "Y", "Y"], ["X", "X"]]
    a, b = train.build_training_set(SEQS, two, 2, 1), train.build_training_set(SEQS, two, 2, 1, max_labels=32)
    assert a.state_fid.tolist() == b.state_fid.tolist() and a.trans_fid.tolist() == b.trans_fid.tolist()
    assert a.labels_ == b.labels_ and a.labels.tolist() == b.labels.tolist()


def test_sequence_crf_argument_errors():
    from gecco_amd.sequence import SequenceCRF

    with pytest.raises(ValueError, match="window_size must lie in 1..32"):
        SequenceCRF(window_size=33)
    with pytest.raises(ValueError, match="window_size must lie in 1..32"):
        SequenceCRF(window_size=0)
    with pytest.raises(ValueError, match="Window step"):
        SequenceCRF(window_size=5, window_step=6)
    with pytest.raises(ValueError, match="unsupported trainer option 'gamma'"):
        SequenceCRF(gamma=1.0)
    with pytest.raises(ValueError, match="invalid value for c2"):
        SequenceCRF(c2=-1.0)
    with pytest.raises(ValueError, match="unsupported training algorithm"):
        SequenceCRF(algorithm="l2sgd")
    crf = SequenceCRF(window_size=2, c1=0.1)
    assert crf.params["c1"] == 0.1 and crf.params["c2"] == 1.0 and crf.window_step == 1
    with pytest.raises(ValueError, match="X holds 2 sequences and y 1"):
        crf.fit(SEQS, LABS[:1])
    with pytest.raises(ValueError, match="sequence 1: 2 items but 3 labels"):
        crf.fit(SEQS, [LABS[0], ["X", "X", "X"]])
    with pytest.raises(ValueError, match="sequence 1 has 2 items, fewer than the window of 3"):
        SequenceCRF(window_size=3).fit(SEQS, LABS)
    with pytest.raises(ValueError, match="not a string"):
        crf.fit([["ab", "c"]], [["X", "Y"]])
    with pytest.raises(ValueError, match="training needs 2 to 32 labels, found 1"):
        crf.fit(SEQS, [["X", "X", "X"], ["X", "X"]])
    for call in (crf.to_bytes, lambda: crf.predict(SEQS), lambda: crf.predict_marginals(SEQS),
                 lambda: crf.predict_windowed(SEQS, "X")):
        with pytest.raises(ValueError, match="not fitted"):
            call()


def test_model_writer_round_trip_three_labels():
    from oracle import lcrf

    ts = train.build_training_set(SEQS, LABS, 2, 1, max_labels=3)
    w = np.array([0.5, -1.25, 0.0, 2.0, 3.5, -0.75, 0.0, 1.5])  # (b, Y) and (X, Y) weigh 0 and are dropped
    m = lcrf.parse_lcrf(train.model_blob(ts, w))
    assert m["labels"] == ["X", "Y", "Z"] and m["attrs"] == ["a", "b", "c"]
    assert m["header"][5] == 3 and m["n_feat"] == 6
    state = np.zeros((3, 3))
    state[0, 0], state[0, 1], state[1, 2], state[2, 0] = 0.5, -1.25, 2.0, 3.5
    trans = np.zeros((3, 3))
    trans[0, 0], trans[1, 2] = -0.75, 1.5
    np.testing.assert_array_equal(m["state"], state)
    np.testing.assert_array_equal(m["trans"], trans)
    np.testing.assert_array_equal(m["state_mask"], state != 0)
    np.testing.assert_array_equal(m["trans_mask"], trans != 0)
