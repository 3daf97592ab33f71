"""Edge posteriors in numpy, log space: the independent yardstick of ``gecco_crf_edge_posteriors`` (tests/test_gpu_edges.py),
pinned on path enumeration by tests/test_edges_host.py.  The lattice is a table of item scores with ``-np.inf`` at every
disallowed (item, label) pair (``tests.constrained_reference.masked_scores``).  Every forward and backward vector is shifted by
its own log-sum-exp, as in ``tests.constrained_reference.marginals``, so that a long sequence's vectors stay of order 1; every
sum over labels is a log-sum-exp whose maximum is finite (every item allows a label), so an excluded term is an exact zero.  It
shares no code with the product."""
import itertools

import numpy as np


def lse(a, axis=None):
    m = np.max(a, axis=axis, keepdims=True)
    out = m + np.log(np.sum(np.exp(a - m), axis=axis, keepdims=True))
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def plogp(logc):
    """-c log c elementwise from log c, with 0 log 0 = 0."""
    c = np.exp(logc)
    with np.errstate(invalid="ignore"):
        return np.where(c > 0.0, -c * logc, 0.0)


def edges_one(X, T):
    """One sequence of masked item scores X [n, L], n >= 1: ``(xi [n, L, L], marg [n, L], H)``.  xi[t] is the pairwise
    marginal of the edge entering item t (zeros at t = 0); H the entropy of the path distribution by the chain rule:
    H(marg_0) + sum_t sum_i marg_{t-1}(i) H(c_t(. | i)) with log c_t(j | i) = T[i, j] + X[t, j] + log beta_t(j) - log-sum-exp."""
    n, L = X.shape
    la, lb = np.zeros((n, L)), np.zeros((n, L))
    la[0] = X[0] - lse(X[0])
    for t in range(1, n):
        la[t] = lse(la[t - 1][:, None] + T, axis=0) + X[t]
        la[t] = la[t] - lse(la[t])
    for t in range(n - 2, -1, -1):
        lb[t] = lse(T + (X[t + 1] + lb[t + 1])[None, :], axis=1)
        lb[t] = lb[t] - lse(lb[t])
    q = la + lb
    lmarg = q - lse(q, axis=1)[:, None]
    marg = np.exp(lmarg)
    xi = np.zeros((n, L, L))
    H = float(plogp(lmarg[0]).sum())
    for t in range(1, n):
        out = T + (X[t] + lb[t])[None, :]  # [i, j]: what leaves label i for label j, up to a factor per row
        u = la[t - 1][:, None] + out
        xi[t] = np.exp(u - lse(u))
        alive = np.isfinite(lmarg[t - 1])  # (a row with no mass has no conditional distribution, and no weight)
        logc = out[alive] - lse(out[alive], axis=1)[:, None]
        H += float((marg[t - 1][alive] * plogp(logc).sum(axis=1)).sum())
    return xi, marg, H


def edge_posteriors(seq_ptr, score, T, set_masks=()):
    """Over a batch: ``dict(pair [n, L, L], marg [n, L], enter [n, n_sets], leave [n, n_sets], transitions [n_seqs, L, L],
    entropy [n_seqs])`` -- enter / leave and the transition counts are sums of entries of xi."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    n, L = score.shape
    n_seqs, n_sets = len(seq_ptr) - 1, len(set_masks)
    inside = np.array([[(int(m) >> y) & 1 for y in range(L)] for m in set_masks], dtype=bool).reshape(n_sets, L)
    out = dict(pair=np.zeros((n, L, L)), marg=np.zeros((n, L)), enter=np.zeros((n, n_sets)), leave=np.zeros((n, n_sets)),
               transitions=np.zeros((n_seqs, L, L)), entropy=np.zeros(n_seqs))
    for s in range(n_seqs):
        b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        if e == b:
            continue
        xi, marg, H = edges_one(score[b:e], T)
        out["pair"][b:e], out["marg"][b:e], out["entropy"][s] = xi, marg, H
        out["transitions"][s] = xi.sum(axis=0)
        for k in range(n_sets):
            S = inside[k]
            out["enter"][b, k] = marg[0][S].sum()
            out["leave"][e - 1, k] = marg[-1][S].sum()
            if e - b > 1:
                out["enter"][b + 1:e, k] = xi[1:][:, ~S][:, :, S].sum(axis=(1, 2))
                out["leave"][b:e - 1, k] = xi[1:][:, S][:, :, ~S].sum(axis=(1, 2))
    return out


def expected_runs(first_marg, transitions, set_mask):
    """The host formula of ``SequenceCRF.expected_runs`` for one sequence: P(y_0 in S) + sum over i outside S, j inside S of N(i, j)."""
    L = len(first_marg)
    S = np.array([(int(set_mask) >> y) & 1 for y in range(L)], dtype=bool)
    return float(first_marg[S].sum() + transitions[~S][:, S].sum())


def enumerate_edges(X, T, set_masks=()):
    """Every path through one short sequence of masked scores: ``(xi [n, L, L], H = -sum p log p, runs [n_sets])``, runs[k] the
    expected number of maximal runs of labels of set k.  A path through a disallowed pair has weight 0."""
    n, L = X.shape
    paths = list(itertools.product(range(L), repeat=n))
    s = np.array([X[0, p[0]] + sum(T[p[t - 1], p[t]] + X[t, p[t]] for t in range(1, n)) for p in paths])
    logp = s - lse(s)
    w = np.exp(logp)
    xi = np.zeros((n, L, L))
    runs = np.zeros(len(set_masks))
    for p, wp in zip(paths, w):
        for t in range(1, n):
            xi[t, p[t - 1], p[t]] += wp
        for k, m in enumerate(set_masks):
            inside = [(int(m) >> y) & 1 for y in p]
            runs[k] += wp * sum(1 for t in range(n) if inside[t] and (t == 0 or not inside[t - 1]))
    return xi, float(plogp(logp).sum()), runs
