"""Circular sequences in plain numpy: the independent yardstick of ``gecco_crf_ring`` (tests/test_gpu_ring.py), pinned on path
enumeration by tests/test_ring_host.py.  It shares no code with the product.

A ring is a table of item scores ``score [n, L]`` (``-inf`` at a disallowed (item, label) pair, as
tests.constrained_reference.masked_scores builds it) and transition weights ``T [L, L]``.  It has n edges, t -> (t + 1) mod n:
the last item has a transition into the first.  A path's score is the left-to-right sum of the chain and then the closing edge,
``(((score[0, y0] + T[y0, y1]) + score[1, y1]) + ... + score[n-1, y_{n-1}]) + T[y_{n-1}, y0]``; a ring of one item has the
self-edge ``T[y0, y0]``, a ring of two both ``T[y0, y1]`` and ``T[y1, y0]``.  A path of score ``-inf`` does not exist.

Two forms of every quantity:
  (a) ``enumerate_ring``: every one of the L**n paths, scored one by one -- short rings only;
  (b) ``sum_walks`` and ``best_path``: the recursions conditioned on the start label a = y0,
        F_0[a][j] = score[0, a] if j = a else -inf,   F_t[a][j] = R_i(F_{t-1}[a][i] + T[i, j]) + score[t, j],
        closed[a] = R_j(F_{n-1}[a][j] + T[j, a]),
        B_{n-1}[a][i] = T[i, a],                      B_t[a][i] = LSE_k(T[i, k] + score[t+1, k] + B_{t+1}[a][k]),
      with R a log-sum-exp (``numpy.longdouble``, max-shifted) or a max (float64, the operation order above, so that the score
      of the best path has the bits of the best enumerated path's).

The tie rule.  Among equal closed[a] the smaller start label wins; inside the conditioned walk a destination scans its sources in
ascending label order with a strict ``>`` (``numpy.argmax``: the first maximum), and the last label is the first arg max of
``V_{n-1}[a*][j] + T[j, a*]``.  In exact arithmetic (integer weights) that picks, among the best paths, the one that is smallest
in the order of the keys ``(y0, y_{n-1}, y_{n-2}, ..., y1)``, which is how ``enumerate_ring`` breaks ties.

``lognorm_bound``: tests.minrun_reference.lognorm_bound carries over.  Every one of the L conditioned chains is that module's
recursion at m = 1: per item a log-sum-exp over L sources -- at most 2 L exponentials and positive additions, one logarithm and
three additions at magnitude <= M.  The ring adds two reductions of the same shape: the closing edge (a log-sum-exp over the L end
labels) and the log-sum-exp over the L start labels.  The chains do not mix before the closure, so errors do not add up across
them: log Z_ring is off by what a chain of n + 2 items would be, ``minrun_reference.lognorm_bound(n + 1, L, M)`` =
(n + 2)(2 L + 8) eps max(1, M).

``bound``: the max semiring's, in the form of tests.maxmarg_reference.bound and by its derivation.  A ring path has n item
scores and n transitions, 2 n - 1 additions between them -- the count of that module's ``through`` -- and an item score of d <= 3
products adds d roundings: no term passes through more than 2 n - 1 + d <= 4 n roundings.  S, the sum of the absolute values of
the worst path's terms, is at most sum_t max_l |terms of score[t, l]| + n max|T| (n transitions, not n - 1)."""
import itertools

import numpy as np

from tests import minrun_reference as mr

EPS = float(np.finfo(np.float64).eps)
NINF = -np.inf


def ring_score(score, T, path, dtype=np.float64):
    s = dtype(score[0, path[0]])
    for t in range(1, len(path)):
        s = (s + dtype(T[path[t - 1], path[t]])) + dtype(score[t, path[t]])
    s = s + dtype(T[path[-1], path[0]])
    return s if dtype is not np.float64 else float(s)


def tie_key(path):
    """The order in which the device's rule prefers equal paths: the start label, then the labels from the last item backwards."""
    return (path[0],) + tuple(reversed(path[1:]))


def _lse(c, axis):
    """Max-shifted, in c's dtype; -inf where every entry is -inf."""
    mx = c.max(axis=axis)
    shift = np.where(mx == NINF, 0, mx).astype(c.dtype)
    with np.errstate(divide="ignore"):
        return np.where(mx == NINF, NINF, shift + np.log(np.exp(c - np.expand_dims(shift, axis)).sum(axis=axis))).astype(c.dtype)


# ---------------------------------------------------------------- (a) enumeration
def enumerate_ring(score, T):
    """Every quantity by enumeration of all L**n paths: a dict with ``lognorm`` (longdouble; -inf without a path), ``marginals``
    ``[n, L]`` (zeros without a path), ``score`` (float64) and ``path`` (a tuple, or None) of the best path under the tie rule."""
    n, L = score.shape
    assert n >= 1 and L ** n <= 50000
    best, arg, paths, terms = NINF, None, [], []
    for p in itertools.product(range(L), repeat=n):
        s = ring_score(score, T, p)
        if s == NINF:
            continue
        paths.append(p)
        terms.append(ring_score(score, T, p, np.longdouble))
        if s > best or (s == best and tie_key(p) < tie_key(arg)):
            best, arg = s, p
    marg = np.zeros((n, L))
    if not paths:
        return dict(lognorm=np.longdouble(NINF), marginals=marg, score=NINF, path=None)
    terms = np.array(terms, dtype=np.longdouble)
    mx = terms.max()
    mass = np.exp(terms - mx)
    total = mass.sum()
    acc = np.zeros((n, L), dtype=np.longdouble)
    for p, w in zip(paths, mass):
        acc[np.arange(n), list(p)] += w
    return dict(lognorm=mx + np.log(total), marginals=(acc / total).astype(np.float64), score=best, path=arg)


# ---------------------------------------------------------------- (b) the conditioned walks
def sum_walks(score, T, dtype=np.longdouble):
    """``(log Z_ring, marginals [n, L] float64, largest finite |forward value|)`` by the conditioned forward and backward walks."""
    n, L = score.shape
    score, T = score.astype(dtype), T.astype(dtype)
    F = np.full((n, L, L), NINF, dtype=dtype)  # [item, start label, label]
    F[0][np.arange(L), np.arange(L)] = score[0]
    for t in range(1, n):
        F[t] = _lse(F[t - 1][:, :, None] + T[None, :, :], 1) + score[t][None, :]
    closed = _lse(F[n - 1] + T.T, 1)  # [a]: over the end label j, F[a][j] + T[j, a]
    lognorm = _lse(closed, 0)[()]
    fin = F[np.isfinite(F)]
    largest = float(np.abs(fin).max()) if fin.size else 0.0
    marg = np.zeros((n, L))
    if lognorm == NINF:
        return lognorm, marg, largest
    B = np.full((n, L, L), NINF, dtype=dtype)  # [item, start label, label]
    B[n - 1] = T.T
    for t in range(n - 2, -1, -1):
        B[t] = _lse(T[None, :, :] + (score[t + 1][None, :] + B[t + 1])[:, None, :], 2)
    with np.errstate(invalid="ignore"):
        ab = F + B
    ab = np.where(np.isnan(ab), NINF, ab)
    marg = np.exp(ab - lognorm).sum(axis=1).astype(np.float64)
    return lognorm, marg, largest


def best_path(score, T):
    """``(path int64 [n] or None, score)``: the two max-plus passes in float64, the kernel's operation order and tie rule."""
    n, L = score.shape
    V = np.full((L, L), NINF)
    V[np.arange(L), np.arange(L)] = score[0]
    for t in range(1, n):
        V = (V[:, :, None] + T[None, :, :]).max(axis=1) + score[t][None, :]
    closed = (V + T.T).max(axis=1)
    a = int(closed.argmax())
    if closed[a] == NINF:
        return None, NINF
    v = np.full(L, NINF)
    v[a] = score[0, a]
    back = []
    for t in range(1, n):
        cand = v[:, None] + T
        back.append(cand.argmax(axis=0))
        v = cand.max(axis=0) + score[t]
    j = int((v + T[:, a]).argmax())
    path = np.zeros(n, dtype=np.int64)
    for t in range(n - 1, -1, -1):
        path[t] = j
        if t:
            j = int(back[t - 1][j])
    return path, float(closed[a])


# ---------------------------------------------------------------- bounds
def lognorm_bound(T, L, largest):
    """(T + 2)(2 L + 8) eps max(1, M) for a ring of T items: tests.minrun_reference.lognorm_bound at T + 1 (module docstring)."""
    return mr.lognorm_bound(T + 1, L, largest)


def bound(abs_score, abs_T, max_terms=3):
    """B = 4 n eps (sum_t max_l abs_score[t, l] + n max abs_T): ``abs_score [n, L]`` holds per (item, label) the sum of the
    absolute values of the products that make up the item score (at most ``max_terms`` of them, and the constant 4 is derived
    for max_terms <= 3: the module docstring)."""
    if max_terms > 3:
        raise ValueError("c = 4 is derived for item scores of at most 3 terms")
    n = abs_score.shape[0]
    total = float(abs_score.max(axis=1).sum()) + n * float(np.max(abs_T))
    return 4.0 * n * EPS * total
