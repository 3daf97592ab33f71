"""The CRF training objective for any number of labels in numpy, log space: the independent yardstick of
``gecco_crf_trainer_general_eval`` (tests/test_gpu_train_general.py), pinned on path enumeration by
tests/test_train_objective_labels.py.  It shares no code with the product: log-sum-exp recursions vectorised over the
windows, nothing scaled.  Also here: seeded training sets with L labels and the error bounds between two fp64
evaluations of the objective."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
TINY = float(np.finfo(np.float64).tiny)


def _lse(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def _tables(A, L, state_fid, trans_fid, w):
    w = np.asarray(w, dtype=np.float64)
    sfid, tfid = np.asarray(state_fid).reshape(A, L), np.asarray(trans_fid).reshape(L, L)
    S = np.where(sfid >= 0, w[np.maximum(sfid, 0)] if len(w) else 0.0, 0.0)
    T = np.where(tfid >= 0, w[np.maximum(tfid, 0)] if len(w) else 0.0, 0.0)
    return sfid, tfid, S, T


def window_starts(seq_ptr, W, step):
    starts = [np.arange(seq_ptr[s], seq_ptr[s + 1] - W + 1, step) for s in range(len(seq_ptr) - 1)]
    return np.concatenate(starts + [np.zeros(0, dtype=np.int64)]).astype(np.int64)


def objective(seq_ptr, item_ptr, attr_id, labels, A, L, W, step, state_fid, trans_fid, w, details=False):
    """Sum over every window (`W` items, `step` apart, no padding) of -log p(y | x) and its gradient over the features
    ``w`` (state_fid[a*L + y] / trans_fid[i*L + j] = feature id or -1).  Returns (f, g, number of windows), and with
    ``details`` a fourth item: per window ``logz`` and ``gold``, per feature ``expected`` and ``empirical`` counts."""
    seq_ptr, item_ptr = np.asarray(seq_ptr), np.asarray(item_ptr)
    attr_id, labels = np.asarray(attr_id), np.asarray(labels)
    K = len(w)
    sfid, tfid, S, T = _tables(A, L, state_fid, trans_fid, w)
    n = len(labels)
    owner = np.repeat(np.arange(n), np.diff(item_ptr))
    score = np.zeros((n, L))
    np.add.at(score, owner, S[attr_id])
    starts = window_starts(seq_ptr, W, step)
    idx = starts[:, None] + np.arange(W)[None, :]
    X, Y = score[idx], labels[idx]  # (windows, W, L), (windows, W)
    nw = len(starts)
    la, lb = np.zeros((nw, W, L)), np.zeros((nw, W, L))
    la[:, 0] = X[:, 0]
    for t in range(1, W):
        la[:, t] = _lse(la[:, t - 1, :, None] + T[None], axis=1) + X[:, t]
    for t in range(W - 2, -1, -1):
        lb[:, t] = _lse(T[None] + (X[:, t + 1] + lb[:, t + 1])[:, None, :], axis=2)
    logz = _lse(la[:, -1], axis=1)
    gold = X[np.arange(nw)[:, None], np.arange(W)[None], Y].sum(axis=1) + T[Y[:, :-1], Y[:, 1:]].sum(axis=1)
    f = float(np.sum(logz - gold))
    marg = np.exp(la + lb - logz[:, None, None])
    item, emp_item = np.zeros((n, L)), np.zeros((n, L))
    np.add.at(item, idx.ravel(), marg.reshape(-1, L))
    np.add.at(emp_item, idx.ravel(), np.eye(L)[Y.ravel()])
    dS, eS = np.zeros((A, L)), np.zeros((A, L))
    np.add.at(dS, attr_id, item[owner])
    np.add.at(eS, attr_id, emp_item[owner])
    dT, eT = np.zeros((L, L)), np.zeros((L, L))
    for t in range(1, W):  # (position by position: [windows, L, L] at a time)
        dT += np.exp(la[:, t - 1, :, None] + T[None] + (X[:, t] + lb[:, t])[:, None, :] - logz[:, None, None]).sum(axis=0)
        np.add.at(eT, (Y[:, t - 1], Y[:, t]), 1.0)
    expected, empirical = np.zeros(K), np.zeros(K)
    m = sfid >= 0
    expected[sfid[m]] += dS[m]
    empirical[sfid[m]] += eS[m]
    m = tfid >= 0
    expected[tfid[m]] += dT[m]
    empirical[tfid[m]] += eT[m]
    g = expected - empirical
    if details:
        return f, g, nw, {"logz": logz, "gold": gold, "expected": expected, "empirical": empirical}
    return f, g, nw


def objective_tolerances(seq_ptr, item_ptr, attr_id, L, W, step, state_fid, trans_fid, w, details):
    """Bounds (tol_f, tol_g [K]) on |f - f_ref| and |g - g_ref| between two fp64 evaluations of the objective with L
    labels: tests.helpers.objective_tolerances (derived there for two labels) restated.

    Every log-space quantity of a window is bounded by M_w = sum_t max_y |s_t[y]| + (W - 1) max |t| + W ln L (W ln L
    where two labels have W ln 2: log Z exceeds the best path's score by at most that).  A window's row (log Z - gold)
    is a sum of at most 2W + 2 such terms, each rounded by at most eps M_w on each side.  New with L labels: every
    log-sum-exp adds L positive terms, a relative error of about log2 L eps in the sum (pairwise; up to (L - 1) eps in
    sequence), which the log turns into an absolute error of that size, far below eps M_w; it is counted as log2 L
    further terms of the row.  The rows are then summed in a tree or pairwise of depth log2(n_windows):
        tol_f = 2 eps sum_w (2W + 2 + log2 L + 2 log2(n_windows + 1)) M_w.
    A node or pairwise marginal is exp of a sum of about four terms bounded by M = max_w M_w, times at most one
    quotient of an L-term sum: relative error <= eps (4W + 4 M + log2 L).  Expected counts sum at most W window
    marginals per item and then the items in a tree; the empirical count is an exact integer; a marginal below DBL_MIN
    may be flushed to 0 by either side:
        tol_g = 2 eps ((5W + 4 M + log2 L + log2(n_items + 1)) expected + empirical) + (n_items + W n_windows) DBL_MIN.
    Both are the sum of the two sides' worst cases."""
    seq_ptr, item_ptr = np.asarray(seq_ptr), np.asarray(item_ptr)
    n = int(seq_ptr[-1])
    A = np.asarray(state_fid).size // L
    _, _, S, T = _tables(A, L, state_fid, trans_fid, w)
    score = np.zeros((n, L))
    np.add.at(score, np.repeat(np.arange(n), np.diff(item_ptr)), S[np.asarray(attr_id)])
    smag = np.abs(score).max(axis=1) if n else np.zeros(0)
    starts = window_starts(seq_ptr, W, step)
    csum = np.concatenate([[0.0], np.cumsum(smag)])
    Mw = csum[starts + W] - csum[starts] + (W - 1) * float(np.abs(T).max()) + W * np.log(float(L))
    nw = len(starts)
    tol_f = 2 * EPS * (2 * W + 2 + np.log2(L) + 2 * np.log2(nw + 1)) * float(Mw.sum())
    M = float(Mw.max()) if nw else 0.0
    tol_g = (2 * EPS * ((5 * W + 4 * M + np.log2(L) + np.log2(n + 1)) * details["expected"] + details["empirical"])
             + (n + W * nw) * TINY)
    return tol_f, tol_g


# ---------------------------------------------------------------- seeded training sets
def labelled_sequences(rng, lengths, A, L, stay=0.9, max_attrs=3):
    """(seq_ptr, item_ptr, attr_id, labels), int32: labels from a Markov chain over L labels that keeps its label with
    probability `stay` (and jumps to any label otherwise); an item holds 0 to max_attrs distinct attributes, drawn
    from a range of the attribute ids that moves with its label (so the labels can be learned)."""
    seq_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(seq_ptr[-1])
    labels = np.zeros(n, dtype=np.int32)
    y = int(rng.integers(0, L))
    for i in range(n):
        if rng.random() >= stay:
            y = int(rng.integers(0, L))
        labels[i] = y
    span = max(A // 2, 1)
    item_ptr, attr = [0], []
    for i in range(n):
        k = int(rng.integers(0, max_attrs + 1))
        base = int(labels[i]) * A // L
        attr.extend(sorted({(base + int(a)) % A for a in rng.integers(0, span, size=k)}))
        item_ptr.append(len(attr))
    return seq_ptr, np.array(item_ptr, dtype=np.int32), np.array(attr, dtype=np.int32), labels


def training_set(rng, L, W, step, A=60, n_seqs=25, fixed=3, drop=0.1, max_extra=60):
    """A seeded problem as ``_native.TrainerGeneral`` takes it, ``(seq_ptr, item_ptr, attr_id, labels, A, state_fid,
    trans_fid, K, W, step)``: ``fixed`` sequences of exactly W items and ``n_seqs`` of W to W + max_extra - 1; a share
    ``drop`` of the (attribute, label) and transition pairs, and at least one of each, has no feature."""
    lengths = [W] * fixed + [int(x) for x in rng.integers(W, W + max_extra, size=n_seqs)]
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, lengths, A, L)
    fid = np.arange(A * L + L * L, dtype=np.int32)
    fid[rng.random(len(fid)) < drop] = -1
    if drop > 0:
        fid[[int(rng.integers(0, A * L)), A * L + int(rng.integers(0, L * L))]] = -1
    keep = fid >= 0
    fid[keep] = np.arange(int(keep.sum()))
    return (seq_ptr, item_ptr, attr_id, labels, A, fid[:A * L], fid[A * L:], int(keep.sum()), W, step)


def count_windows(seq_ptr, W, step):
    return sum((int(seq_ptr[s + 1] - seq_ptr[s]) - W) // step + 1 for s in range(len(seq_ptr) - 1))


def same_bits(f_a, g_a, f_b, g_b):
    return np.float64(f_a).tobytes() == np.float64(f_b).tobytes() and np.asarray(g_a).tobytes() == np.asarray(g_b).tobytes()
