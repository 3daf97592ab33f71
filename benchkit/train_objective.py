"""The CRF training objective in numpy, log space: the independent yardstick of `gecco_crf_trainer_eval`.

One definition serves the GPU tests (tests/test_gpu_train.py: accuracy of the device objective, scipy's optimum) and
tools/bench_train.py (the single-thread CPU baseline).  It shares no code with the product: no scaling, no normaliser
bookkeeping, logsumexp recursions vectorised over windows."""
import numpy as np


def _lse(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def objective(seq_ptr, item_ptr, attr_id, labels, A, W, step, state_fid, trans_fid, w, details=False):
    """Sum over every window (`W` items, `step` apart, no padding) of -log p(y | x) and its gradient over the features
    ``w`` (state_fid[a*2 + y] / trans_fid[i*2 + j] = feature id or -1, 2 labels).  Returns (f, g, number of windows),
    and with ``details`` a fourth item: a dict of the terms f and g are made of -- per window ``logz`` and ``gold``
    (score of the gold path), per feature ``expected`` and ``empirical`` counts (g = expected - empirical)."""
    w = np.asarray(w, dtype=np.float64)
    seq_ptr, item_ptr = np.asarray(seq_ptr), np.asarray(item_ptr)
    attr_id, labels = np.asarray(attr_id), np.asarray(labels)
    K = len(w)
    state_fid, trans_fid = np.asarray(state_fid).reshape(A, 2), np.asarray(trans_fid).reshape(2, 2)
    S = np.where(state_fid >= 0, w[np.maximum(state_fid, 0)] if K else 0.0, 0.0)
    T = np.where(trans_fid >= 0, w[np.maximum(trans_fid, 0)] if K else 0.0, 0.0)
    n = len(labels)
    owner = np.repeat(np.arange(n), np.diff(item_ptr))
    score = np.zeros((n, 2))
    np.add.at(score, owner, S[attr_id])
    starts = np.concatenate([np.arange(seq_ptr[s], seq_ptr[s + 1] - W + 1, step) for s in range(len(seq_ptr) - 1)]
                            + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    idx = starts[:, None] + np.arange(W)[None, :]
    X, Y = score[idx], labels[idx]  # (windows, W, 2), (windows, W)
    nw = len(starts)
    la, lb = np.zeros((nw, W, 2)), np.zeros((nw, W, 2))
    la[:, 0] = X[:, 0]
    for t in range(1, W):
        la[:, t] = _lse(la[:, t - 1, :, None] + T[None], axis=1) + X[:, t]
    for t in range(W - 2, -1, -1):
        lb[:, t] = _lse(T[None] + (X[:, t + 1] + lb[:, t + 1])[:, None, :], axis=2)
    logz = _lse(la[:, -1], axis=1)
    gold = X[np.arange(nw)[:, None], np.arange(W)[None], Y].sum(axis=1) + T[Y[:, :-1], Y[:, 1:]].sum(axis=1)
    f = float(np.sum(logz - gold))
    marg = np.exp(la + lb - logz[:, None, None])
    item, emp_item = np.zeros((n, 2)), np.zeros((n, 2))
    np.add.at(item, idx.ravel(), marg.reshape(-1, 2))
    np.add.at(emp_item, idx.ravel(), np.eye(2)[Y.ravel()])
    dS, eS = np.zeros((A, 2)), np.zeros((A, 2))
    np.add.at(dS, attr_id, item[owner])
    np.add.at(eS, attr_id, emp_item[owner])
    dT, eT = np.zeros((2, 2)), np.zeros((2, 2))
    if W > 1:
        dT += np.exp(la[:, :-1, :, None] + T[None, None] + (X[:, 1:] + lb[:, 1:])[:, :, None, :]
                     - logz[:, None, None, None]).sum(axis=(0, 1))
        np.add.at(eT, (Y[:, :-1].ravel(), Y[:, 1:].ravel()), 1.0)
    expected, empirical = np.zeros(K), np.zeros(K)
    m = state_fid >= 0
    expected[state_fid[m]] += dS[m]
    empirical[state_fid[m]] += eS[m]
    m = trans_fid >= 0
    expected[trans_fid[m]] += dT[m]
    empirical[trans_fid[m]] += eT[m]
    g = expected - empirical
    if details:
        return f, g, nw, {"logz": logz, "gold": gold, "expected": expected, "empirical": empirical}
    return f, g, nw
