"""GECCO's windowed probabilities in numpy and log space with every vector conditioned: the yardstick of
tests/test_gpu_window_range.py, pinned on path enumeration and on its own extended-precision run by
tests/test_window_range_host.py.

``constrained_reference.windowed`` (and ``train_objective_valued.windowed``, which it restates) runs a log-space
forward-backward whose vectors are not shifted: with item scores of 800 over a 20-item window, ``la + lb - lz`` cancels numbers
near 1.6e4, whose ulp is 1.8e-12 -- the whole tolerance the device is held to.  Here every forward and every backward vector of
every window is shifted by its own log-sum-exp, as ``constrained_reference.marginals`` does for a whole sequence: the vectors
stay of order 1 whatever the scores, and a marginal is ``exp(q - lse(q))`` with ``q = la + lb`` rounded at that size.  The
windows of a contig run side by side.  It shares no code with the product."""
import numpy as np


def _lse(a, axis):
    """log-sum-exp along `axis` in a's own dtype; a slice that holds only -inf gives -inf (and no NaN)."""
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def window_marginals(X, T):
    """Marginals [m, W, L] of m windows of W items with the item scores X [m, W, L] (-inf: the pair is disallowed; every
    item allows a label) and the transitions T [L, L], in X's dtype."""
    m, W, L = X.shape
    la, lb = np.zeros_like(X), np.zeros_like(X)
    la[:, 0] = X[:, 0] - _lse(X[:, 0], 1)[:, None]
    for t in range(1, W):
        v = _lse(la[:, t - 1, :, None] + T[None], axis=1) + X[:, t]
        la[:, t] = v - _lse(v, 1)[:, None]
    for t in range(W - 2, -1, -1):
        v = _lse(T[None] + (X[:, t + 1] + lb[:, t + 1])[:, None, :], axis=2)
        lb[:, t] = v - _lse(v, 1)[:, None]
    q = la + lb
    return np.exp(q - _lse(q, 2)[:, :, None])


def windowed_backgrounds(seq_ptr, score, T, W, step, backgrounds=(), pad=True, dtype=np.float64):
    """``windowed`` for several backgrounds over one forward-backward: (p_all [n, L], [p_any [n] per background])."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    score, T = np.asarray(score).astype(dtype), np.asarray(T).astype(dtype)
    n, L = score.shape
    assert all(0 <= bg < L for bg in backgrounds)
    p_all = np.zeros((n, L), dtype=dtype)
    p_any = [np.zeros(n, dtype=dtype) for _ in backgrounds]
    for s in range(len(seq_ptr) - 1):
        b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        m = e - b
        if m == 0:
            continue
        if m < W and not pad:
            p_all[b:e] = np.nan
            for p in p_any:
                p[b:e] = np.nan
            continue
        front = (W - m) // 2 if m < W else 0
        X = np.zeros((max(m, W), L), dtype=dtype)
        X[front:front + m] = score[b:e]
        starts = np.arange(0, len(X) - W + 1, step)
        idx = starts[:, None] + np.arange(W)[None, :]
        marg = window_marginals(X[idx], T)
        full = np.zeros((len(X), L), dtype=dtype)
        np.maximum.at(full, idx.ravel(), marg.reshape(-1, L))
        p_all[b:e] = full[front:front + m]
        for p, bg in zip(p_any, backgrounds):
            tot = np.zeros(marg.shape[:2], dtype=dtype)
            for l in range(L):
                if l != bg:
                    tot = tot + marg[:, :, l]
            anyp = np.zeros(len(X), dtype=dtype)
            np.maximum.at(anyp, idx.ravel(), tot.ravel())
            p[b:e] = anyp[front:front + m]
    return p_all, p_any


def windowed(seq_ptr, score, T, W, step, background=None, pad=True, dtype=np.float64):
    """p_all [n, L] and p_any [n] (None without a background) under the contract of ``constrained_reference.windowed``:
    `score` is the masked score table (-inf at disallowed pairs), a padding item scores 0 under every label, a contig shorter
    than W without ``pad`` holds NaN, an item that no window covers holds 0.  p_all[g, l] is the maximum over the windows
    that cover item g of P_w(y_g = l), p_any[g] the maximum over the same windows of the sum over l != background (in label
    order) of P_w(y_g = l).  One label's windowed probability is its column.  ``dtype``: the arithmetic's (np.longdouble:
    the run the float64 one is checked against)."""
    p_all, p_any = windowed_backgrounds(seq_ptr, score, T, W, step, () if background is None else (background,), pad, dtype)
    return p_all, (p_any[0] if p_any else None)
