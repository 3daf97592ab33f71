"""Marginals under a minimum run length in plain numpy: the independent yardstick of ``gecco_crf_marginals_min_run``
(tests/test_gpu_minrun_marginals.py), pinned on path enumeration by tests/test_minrun_marginals_host.py.  It shares no code with
the product, and of tests/minrun_reference.py it takes the definitions only: ``feasible`` and ``path_score``.

A sequence is a table of item scores ``score [n, L]`` (``-inf`` at a disallowed (item, label) pair) and transition weights
``T [L, L]``; a label set is a bit mask, and a path is feasible under (mask, m) when every maximal run of consecutive items with
labels inside the set has at least m items (tests/minrun_reference.py).  The marginal of (item t, label j) under the constraint
is the mass of the feasible paths with label j at item t over the mass of all feasible paths, exp(log Z_C).

``forward_backward`` works on the EXPLICIT list of expanded states -- a label outside the set has one state ``(j, 0)``, a label
inside the states ``(j, d)``, d = 1 .. m, d = min(run length so far, m), ordered by label, then by d -- and on a DENSE table of
expanded transitions ``E [S, S]``, ``-inf`` at a forbidden pair.  Nothing of the structure is used beyond that table (a
forbidden pair adds exp(-inf) = 0 to a sum and is left out of it, which is what keeps the yardstick at seconds): the
recursions are alpha_t(s') = LSE_s(alpha_{t-1}(s) + E[s, s']) + score[t, label(s')] and beta_t(s) = LSE_s'(E[s, s'] +
score[t + 1, label(s')] + beta_{t+1}(s')), every LSE shifted by its own maximum, in the ``dtype`` given; ``numpy.longdouble`` is
the yardstick.  ``enumerate_marginals`` walks all L**n paths -- short sequences only."""
import itertools

import numpy as np

from tests import minrun_reference as mr


def expanded_states(mask, m, L):
    """[(label, d)]: d = 0 for a label outside the set, d = 1 .. m inside; by label, then by d."""
    states = []
    for j in range(L):
        if (int(mask) >> j) & 1:
            states.extend((j, d) for d in range(1, m + 1))
        else:
            states.append((j, 0))
    return states


def allowed_step(src, dst, m):
    """May expanded state ``dst`` at item t follow ``src`` at item t - 1?"""
    (_, ds), (_, dd) = src, dst
    if dd == 0:                      # a run may end only when it is long enough (or there is none)
        return ds == 0 or ds == m
    if ds == 0:                      # a run starts
        return dd == 1
    return dd == min(ds + 1, m)      # a run goes on


def expanded_table(T, mask, m, dtype=np.longdouble):
    """(states, E [S, S] in ``dtype`` with -inf at forbidden pairs, start [S] bool, end [S] bool)."""
    L = T.shape[0]
    states = expanded_states(mask, m, L)
    S = len(states)
    E = np.full((S, S), -np.inf, dtype=dtype)
    for a, src in enumerate(states):
        for b, dst in enumerate(states):
            if allowed_step(src, dst, m):
                E[a, b] = dtype(T[src[0], dst[0]])
    start = np.array([d <= 1 for _, d in states], dtype=bool)
    end = np.array([d == 0 or d == m for _, d in states], dtype=bool)
    return states, E, start, end


def lse(c, axis):
    """Max-shifted log-sum-exp in c's dtype; -inf where every entry is -inf."""
    mx = c.max(axis=axis)
    shift = np.where(mx == -np.inf, 0, mx).astype(c.dtype)
    with np.errstate(divide="ignore"):
        total = np.exp(c - np.expand_dims(shift, axis)).sum(axis=axis)
        return np.where(mx == -np.inf, -np.inf, shift + np.log(total)).astype(c.dtype)


class _Grouped:
    """The finite entries of a dense table grouped by column (``by = 1``: a destination's sources) or by row (``by = 0``: a
    source's successors), for a log-sum-exp per group, every group shifted by its own maximum."""

    def __init__(self, E, by):
        rows, cols = np.nonzero(E > -np.inf)
        key = cols if by == 1 else rows
        order = np.argsort(key, kind="stable")
        self.rows, self.cols, key = rows[order], cols[order], key[order]
        self.weight = E[self.rows, self.cols]
        self.owners, self.starts = np.unique(key, return_index=True)
        self.group = np.searchsorted(self.owners, key)
        self.size = E.shape[0]

    def lse(self, c):
        """c: one term per finite entry, in this object's order; [S], -inf for a group without a finite term (or entry)."""
        out = np.full(self.size, -np.inf, dtype=c.dtype)
        if c.size == 0:
            return out
        mx = np.maximum.reduceat(c, self.starts)
        shift = np.where(mx == -np.inf, 0, mx).astype(c.dtype)
        with np.errstate(divide="ignore"):
            total = np.add.reduceat(np.exp(c - shift[self.group]), self.starts)
            out[self.owners] = np.where(mx == -np.inf, -np.inf, shift + np.log(total))
        return out


def forward_backward(score, T, mask, m, dtype=np.longdouble):
    """(marginals [n, L] in ``dtype``, log Z_C, the largest finite |alpha or beta| met).  Without a feasible path the marginals
    are zeros and log Z_C is -inf."""
    n, L = score.shape
    score = np.asarray(score).astype(dtype)
    states, E, start, end = expanded_table(np.asarray(T), mask, m, dtype)
    label = np.array([j for j, _ in states], dtype=np.int64)
    S = len(states)
    ninf = dtype(-np.inf)
    alpha = np.full((n, S), ninf, dtype=dtype)
    beta = np.full((n, S), ninf, dtype=dtype)
    alpha[0] = np.where(start, score[0][label], ninf)
    into, out_of = _Grouped(E, 1), _Grouped(E, 0)
    for t in range(1, n):
        alpha[t] = into.lse(alpha[t - 1][into.rows] + into.weight) + score[t][label]
    beta[n - 1] = np.where(end, dtype(0), ninf)
    for t in range(n - 2, -1, -1):
        beta[t] = out_of.lse(out_of.weight + (score[t + 1][label] + beta[t + 1])[out_of.cols])
    logz = lse(np.where(end, alpha[n - 1], ninf), 0)[()]
    both = np.concatenate([alpha.ravel(), beta.ravel()])
    fin = both[np.isfinite(both)]
    largest = float(np.abs(fin).max()) if fin.size else 0.0
    marg = np.zeros((n, L), dtype=dtype)
    if logz == -np.inf:
        return marg, logz, largest
    ab = alpha + beta
    with np.errstate(invalid="ignore"):
        p = np.where(ab == -np.inf, dtype(0), np.exp(ab - logz)).astype(dtype)
    for s in range(S):  # (ascending d within a label)
        marg[:, label[s]] += p[:, s]
    return marg, logz, largest


def enumerate_marginals(score, T, mask, m):
    """(marginals [n, L], log Z_C) in longdouble by enumeration of all L**n paths; zeros and -inf when none is feasible."""
    n, L = score.shape
    paths, terms = [], []
    for p in itertools.product(range(L), repeat=n):
        if not mr.feasible(p, mask, m):
            continue
        s = mr.path_score(score, T, p, np.longdouble)
        if s == -np.inf:
            continue
        paths.append(p)
        terms.append(s)
    marg = np.zeros((n, L), dtype=np.longdouble)
    if not terms:
        return marg, np.longdouble(-np.inf)
    terms = np.array(terms, dtype=np.longdouble)
    mx = terms.max()
    logz = mx + np.log(np.exp(terms - mx).sum())
    w = np.exp(terms - logz)
    for p, wp in zip(paths, w):
        marg[np.arange(n), list(p)] += wp
    return marg, logz
