"""Inference under allowed-label sets in numpy, log space: the independent yardstick of the ``*_constrained`` one-shots
(tests/test_gpu_constrained.py), pinned on path enumeration by tests/test_constrained_host.py.  Every item carries a uint32
mask with bit y set when label y is allowed (the trainers' masks, tests/train_objective_partial.py); a constrained quantity
is the unconstrained one on the table of item scores with ``-np.inf`` at every disallowed (item, label) pair.  Every sum
over labels is a log-sum-exp whose maximum is finite (every item allows a label), so an excluded term is an exact zero and
nothing invalid is formed.  It shares no code with the product."""
import itertools

import numpy as np

from tests.train_objective_partial import mask_matrix
from tests.train_objective_valued import forward_backward, item_scores, lse


def masked_scores(item_ptr, attr_id, values, S, allowed):
    """[n, L] item scores (value x weight in CSR order; ``values`` None: every value 1), ``-inf`` where disallowed."""
    attr_id = np.asarray(attr_id)
    score = item_scores(item_ptr, attr_id, np.ones(len(attr_id)) if values is None else values, S)
    return np.where(mask_matrix(allowed, S.shape[1]), score, -np.inf)


def marginals(seq_ptr, score, T):
    """Whole-sequence marginals [n, L] given that the path lies inside the sets, and log Z_A per sequence (0 for a sequence
    without items).  Every forward and backward vector is shifted by its own log-sum-exp, so that a long sequence's vectors
    stay of order 1 (tests.train_objective_valued.marginals_sequences explains why).  A disallowed entry is exp(-inf) = 0."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    marg, logz = np.zeros_like(score), np.zeros(len(seq_ptr) - 1)
    for s in range(len(seq_ptr) - 1):
        b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        if e == b:
            continue
        X, n = score[b:e], e - b
        la, lb = np.zeros_like(X), np.zeros_like(X)
        la[0] = X[0]
        total = lse(la[0], 0)
        la[0] = la[0] - total
        for t in range(1, n):
            la[t] = lse(la[t - 1][:, None] + T, axis=0) + X[t]
            shift = lse(la[t], 0)
            la[t] = la[t] - shift
            total += shift
        for t in range(n - 2, -1, -1):
            lb[t] = lse(T + (X[t + 1] + lb[t + 1])[None, :], axis=1)
            lb[t] = lb[t] - lse(lb[t], 0)
        q = la + lb
        marg[b:e] = np.exp(q - lse(q, axis=1)[:, None])
        logz[s] = total
    return marg, logz


def viterbi_one(score, T):
    """CRFsuite's recursion over one sequence of item scores [n, L] that may hold -inf: per target label the maximum over the
    source label with a strict `<` update in index order -- the FIRST source that attains it, which is numpy's argmax --
    and the first arg max at the end.  Returns (labels, score).  tests/test_constrained_host.py holds it to the loop form
    (tests.train_objective_valued.viterbi_scores) and to enumeration."""
    n, L = score.shape
    back = np.zeros((n, L), dtype=np.int64)
    d = score[0].copy()
    for t in range(1, n):
        cand = d[:, None] + T
        back[t] = np.argmax(cand, axis=0)
        d = cand[back[t], np.arange(L)] + score[t]
    y = np.zeros(n, dtype=np.int64)
    y[-1] = int(np.argmax(d))
    for t in range(n - 1, 0, -1):
        y[t - 1] = back[t, y[t]]
    return y, float(d[y[-1]])


def viterbi(seq_ptr, score, T):
    """Labels [n] and path score per sequence (0 for a sequence without items)."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    y, sc = np.zeros(len(score), dtype=np.int64), np.zeros(len(seq_ptr) - 1)
    for s in range(len(seq_ptr) - 1):
        b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        if e > b:
            y[b:e], sc[s] = viterbi_one(score[b:e], T)
    return y, sc


def windowed(seq_ptr, score, T, W, step, background=None, pad=True):
    """GECCO's windowed probabilities on the restricted lattice: p_all [n, L] and p_any [n] (or None) as
    tests.train_objective_valued.windowed defines them, every window an independent forward-backward over the masked
    scores.  Padding items have score 0 under every label: they allow every label."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    n, L = score.shape
    p_all = np.zeros((n, L))
    p_any = None if background is None else np.zeros(n)
    others = [l for l in range(L) if l != background]
    for s in range(len(seq_ptr) - 1):
        b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        m = e - b
        if m == 0:
            continue
        if m < W and not pad:
            p_all[b:e] = np.nan
            if p_any is not None:
                p_any[b:e] = np.nan
            continue
        front = (W - m) // 2 if m < W else 0
        X = np.zeros((max(m, W), L))
        X[front:front + m] = score[b:e]
        starts = np.arange(0, len(X) - W + 1, step)
        idx = starts[:, None] + np.arange(W)[None, :]
        la, lb, lz = forward_backward(X[idx], T)
        marg = np.exp(la + lb - lz[:, None, None])
        full = np.zeros((len(X), L))
        np.maximum.at(full, idx.ravel(), marg.reshape(-1, L))
        p_all[b:e] = full[front:front + m]
        if p_any is not None:
            tot = np.zeros(marg.shape[:2])
            for l in others:
                tot = tot + marg[:, :, l]
            anyp = np.zeros(len(X))
            np.maximum.at(anyp, idx.ravel(), tot.ravel())
            p_any[b:e] = anyp[front:front + m]
    return p_all, p_any


def enumerate_paths(score, T):
    """Every path through one short sequence of masked scores: (log Z_A, marginals [n, L], the best score, the set of the
    paths that attain it).  A path through a disallowed pair has score -inf and weight 0."""
    n, L = score.shape
    paths = list(itertools.product(range(L), repeat=n))
    s = np.array([score[0, p[0]] + sum(T[p[t - 1], p[t]] + score[t, p[t]] for t in range(1, n)) for p in paths])
    logz = float(lse(s, 0))
    w = np.exp(s - logz)
    marg = np.zeros((n, L))
    for p, wp in zip(paths, w):
        for t, l in enumerate(p):
            marg[t, l] += wp
    best = float(s.max())
    return logz, marg, best, {p for p, sp in zip(paths, s) if sp == best}
