"""The whole-sequence CRF training objective (one instance per sequence, of that sequence's length) in numpy: the
independent yardstick of ``gecco_crf_trainer_sequences_eval`` (tests/test_gpu_train_sequences.py), pinned on path
enumeration by tests/test_train_sequences_host.py.  It is tests/train_objective_labels.py's windowed yardstick called on
every sequence alone with W = its length and step = 1, summed in sequence order; it shares no code with the product.
Also here: the error bounds between two fp64 evaluations (that module's bounds per length group, added) and seeded
problems with sequences of given lengths."""
import numpy as np

from tests.train_objective_labels import labelled_sequences, objective, objective_tolerances


def subproblem(seq_ptr, item_ptr, attr_id, labels, members):
    """(seq_ptr, item_ptr, attr_id, labels) of the sequences `members` alone, in that order."""
    seq_ptr, item_ptr = np.asarray(seq_ptr, dtype=np.int64), np.asarray(item_ptr, dtype=np.int64)
    attr_id, labels = np.asarray(attr_id), np.asarray(labels)
    items = np.concatenate([np.arange(seq_ptr[s], seq_ptr[s + 1]) for s in members] + [np.zeros(0, dtype=np.int64)])
    sub_seq = np.concatenate([[0], np.cumsum([seq_ptr[s + 1] - seq_ptr[s] for s in members])]).astype(np.int32)
    deg = item_ptr[items + 1] - item_ptr[items]
    sub_item = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    sub_attr = np.concatenate([attr_id[item_ptr[i]:item_ptr[i + 1]] for i in items] + [np.zeros(0, dtype=np.int32)])
    return sub_seq, sub_item, sub_attr.astype(np.int32), labels[items].astype(np.int32)


def objective_sequences(seq_ptr, item_ptr, attr_id, labels, A, L, state_fid, trans_fid, w):
    """Sum over the sequences of -log p(y | x) of the whole sequence, and its gradient over the features ``w``: returns
    (f, g, number of sequences).  Every sequence must hold at least one item."""
    f, g = 0.0, np.zeros(len(w))
    n_seqs = len(seq_ptr) - 1
    for s in range(n_seqs):
        sub = subproblem(seq_ptr, item_ptr, attr_id, labels, [s])
        fs, gs, nw = objective(*sub, A, L, int(sub[0][1]), 1, state_fid, trans_fid, w)
        assert nw == 1
        f += fs
        g += gs
    return f, g, n_seqs


def length_groups(seq_ptr):
    """{length: the sequences of that length, ascending}."""
    groups = {}
    for s, n in enumerate(np.diff(np.asarray(seq_ptr)).tolist()):
        groups.setdefault(int(n), []).append(s)
    return groups


def objective_sequences_tolerances(seq_ptr, item_ptr, attr_id, labels, A, L, state_fid, trans_fid, w):
    """Bounds (tol_f, tol_g [K]) on |f - f_ref| and |g - g_ref| between two fp64 evaluations of the whole-sequence
    objective: the sequences of one length n are a windowed problem with W = n and step = 1 whose every sequence is one
    window, so tests.train_objective_labels.objective_tolerances bounds that group's share of f and g; the objective is
    the sum of the groups' shares, and so is the bound (adding the shares rounds by eps of a sum the bounds exceed)."""
    tol_f, tol_g = 0.0, np.zeros(len(w))
    for n, members in length_groups(seq_ptr).items():
        sub = subproblem(seq_ptr, item_ptr, attr_id, labels, members)
        _, _, _, details = objective(*sub, A, L, n, 1, state_fid, trans_fid, w, details=True)
        tf, tg = objective_tolerances(sub[0], sub[1], sub[2], L, n, 1, state_fid, trans_fid, w, details)
        tol_f += tf
        tol_g += tg
    return tol_f, tol_g


def sequences_problem(rng, L, lengths, A=20, drop=0.1, stay=0.9):
    """A seeded problem as ``_native.TrainerSequences`` takes it, ``(seq_ptr, item_ptr, attr_id, labels, A, state_fid,
    trans_fid, K)``, with sequences of the given lengths; a share ``drop`` of the (attribute, label) and transition
    pairs, and with a positive ``drop`` at least one of each, has no feature (as ``training_set`` there)."""
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, lengths, A, L, stay=stay)
    fid = np.arange(A * L + L * L, dtype=np.int32)
    fid[rng.random(len(fid)) < drop] = -1
    if drop > 0:
        fid[[int(rng.integers(0, A * L)), A * L + int(rng.integers(0, L * L))]] = -1
    keep = fid >= 0
    fid[keep] = np.arange(int(keep.sum()))
    return (seq_ptr, item_ptr, attr_id, labels, A, fid[:A * L], fid[A * L:], int(keep.sum()))
