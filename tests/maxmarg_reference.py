"""Max-marginals in plain Python and numpy: the independent yardstick of ``gecco_crf_max_marginals``
(tests/test_gpu_maxmarg.py), pinned on path enumeration by tests/test_maxmarg_host.py.  It shares no code with the product.

A sequence is a table of item scores ``score [n, L]`` (``-inf`` at a disallowed (item, label) pair, as
tests.constrained_reference.masked_scores builds it) and transition weights ``T [L, L]``.  A path's score is the left-to-right
sum ``((score[0, y0] + T[y0, y1]) + score[1, y1]) + T[y1, y2]) + ...``.  A path of score ``-inf`` does not exist.

Two forms of every quantity:
  (a) ``enumerate_all``: every one of the L**n paths, scored one by one; a quantity is the maximum over the paths that qualify
      -- short sequences only (n <= 6);
  (b) ``forward`` / ``backward`` / ``through`` and the restricted walks.  No logarithm or exponential anywhere (max-plus needs
      none).  The restricted quantities are NOT computed the way the kernel walks them: ``span_best`` masks the score table
      (labels outside the set get ``-inf`` on the span) and runs plain Viterbi over the whole sequence; ``span_broken_by_items``
      forbids the set at one item of the span at a time and takes the best of those Viterbi scores; ``span_broken`` reads the
      same number off ``through``.

``bound``: how far a device value may lie from the yardstick's.  Derivation.  Flatten a value into its terms: every value x
weight product of the item scores on a path and every transition weight on it.  ``through_t(l) = a_t(l) + b_t(l)``: a_t is a
left-to-right sum of t + 1 item scores and t transitions (2 t additions between them), b_t a sum of T - 1 - t item scores and as
many transitions (2 (T - 1 - t) - 1 additions between them, its first term being added to an exact 0), and one addition joins
the two: at most 2 T - 1 additions between item scores and transitions, whatever t -- and the same count for ``span_best``, whose
walk replaces a stretch of a, and for ``best`` (2 T - 2).  An item score is itself a sum of d products, d roundings (a fused
multiply-add, or an addition).  So no term passes through more than 2 T - 1 + d roundings, each of relative size u = eps / 2,
and to first order a computed value is off from the exact one by at most (2 T - 1 + d) u S, S the sum of the absolute values of
the path's terms.  Device and yardstick may each be off by that much, in any order of their additions: they differ by at most
(2 T - 1 + d) eps S.  The two may also pick different paths for a maximum; |max_i x_i - max_i x'_i| <= max_i |x_i - x'_i|, so the
bound holds with S taken over the worst path: S <= sum_t max_l |terms of s_t(l)| + (T - 1) max|A|.  The test batches give an
item at most d = 3 attributes, and 2 T - 1 + 3 <= 4 T for every T >= 1: c = 4, the constant of kbest_reference.bound, with
room for the second-order terms (at T = 300, 4 T u is 1e-13)."""
import itertools

import numpy as np

EPS = float(np.finfo(np.float64).eps)
NINF = -np.inf


def path_score(score, T, path):
    s = score[0, path[0]]
    for t in range(1, len(path)):
        s = (s + T[path[t - 1], path[t]]) + score[t, path[t]]
    return float(s)


def members(mask, L):
    """Boolean [L]: label y is in the set when bit y of ``mask`` is set."""
    return ((int(mask) >> np.arange(L)) & 1).astype(bool)


# ---------------------------------------------------------------- (a) enumeration
def enumerate_all(score, T, sets=(), spans=()):
    """Every quantity by enumeration of all L**n paths: a dict with ``best``, ``through [n, L]``, ``inside`` / ``outside``
    ``[n, n_sets]``, ``span_best`` / ``span_broken`` ``[n_spans]`` for ``spans`` = [(begin, end, mask)]."""
    n, L = score.shape
    assert n >= 1 and L ** n <= 50000
    best = NINF
    through = np.full((n, L), NINF)
    inside = np.full((n, len(sets)), NINF)
    outside = np.full((n, len(sets)), NINF)
    sbest = np.full(len(spans), NINF)
    sbroken = np.full(len(spans), NINF)
    inset = [members(m, L) for m in sets]
    inspan = [members(m, L) for _, _, m in spans]
    for p in itertools.product(range(L), repeat=n):
        s = path_score(score, T, p)
        if s == NINF:
            continue
        best = max(best, s)
        for t, y in enumerate(p):
            through[t, y] = max(through[t, y], s)
            for k, mem in enumerate(inset):
                if mem[y]:
                    inside[t, k] = max(inside[t, k], s)
                else:
                    outside[t, k] = max(outside[t, k], s)
        for q, (b, e, _) in enumerate(spans):
            if all(inspan[q][y] for y in p[b:e]):
                sbest[q] = max(sbest[q], s)
            else:
                sbroken[q] = max(sbroken[q], s)
    return dict(best=float(best), through=through, inside=inside, outside=outside, span_best=sbest, span_broken=sbroken)


# ---------------------------------------------------------------- (b) max-plus forward / backward
def forward(score, T):
    """a [n, L]: a_0 = score[0], a_t(j) = max_i (a_{t-1}(i) + T[i, j]) + score[t, j]."""
    n, L = score.shape
    a = np.empty((n, L))
    a[0] = score[0]
    for t in range(1, n):
        a[t] = (a[t - 1][:, None] + T).max(axis=0) + score[t]
    return a


def backward(score, T):
    """b [n, L]: b_{n-1} = 0, b_t(i) = max_j (T[i, j] + (score[t+1, j] + b_{t+1}(j)))."""
    n, L = score.shape
    b = np.zeros((n, L))
    for t in range(n - 2, -1, -1):
        b[t] = (T + (score[t + 1] + b[t + 1])[None, :]).max(axis=1)
    return b


def viterbi_score(score, T):
    return float(forward(score, T)[-1].max())


def through(score, T):
    return forward(score, T) + backward(score, T)


def split_by_sets(th, sets):
    """(inside, outside) [n, n_sets]: the maxima of ``th`` over the labels in / not in every set (-inf over nothing)."""
    n, L = th.shape
    inside = np.full((n, len(sets)), NINF)
    outside = np.full((n, len(sets)), NINF)
    for k, m in enumerate(sets):
        mem = members(m, L)
        if mem.any():
            inside[:, k] = th[:, mem].max(axis=1)
        if (~mem).any():
            outside[:, k] = th[:, ~mem].max(axis=1)
    return inside, outside


def span_best(score, T, begin, end, mask):
    """Plain Viterbi on the table with the labels outside the set struck out on the span."""
    masked = score.copy()
    masked[begin:end, ~members(mask, score.shape[1])] = NINF
    return viterbi_score(masked, T)


def span_broken_by_items(score, T, begin, end, mask):
    """The best over the span's items of plain Viterbi with the set struck out at that one item."""
    mem = members(mask, score.shape[1])
    out = NINF
    for t in range(begin, end):
        masked = score.copy()
        masked[t, mem] = NINF
        out = max(out, viterbi_score(masked, T))
    return out


def span_broken(th, begin, end, mask):
    mem = members(mask, th.shape[1])
    return float(th[begin:end, ~mem].max()) if (~mem).any() else NINF


def all_quantities(score, T, sets=(), spans=()):
    """The dict of ``enumerate_all`` by form (b)."""
    th = through(score, T)
    inside, outside = split_by_sets(th, sets)
    return dict(best=viterbi_score(score, T), through=th, inside=inside, outside=outside,
                span_best=np.array([span_best(score, T, b, e, m) for b, e, m in spans], dtype=np.float64),
                span_broken=np.array([span_broken(th, b, e, m) for b, e, m in spans], dtype=np.float64))


def viterbi_path(score, T):
    """The first-arg-max Viterbi path (strict ``<`` update, smaller label on a tie), as a list."""
    n, L = score.shape
    a = score[0].copy()
    back = []
    for t in range(1, n):
        cand = a[:, None] + T
        back.append(cand.argmax(axis=0))
        a = cand.max(axis=0) + score[t]
    y = [int(a.argmax())]
    for bp in reversed(back):
        y.append(int(bp[y[-1]]))
    return y[::-1]


# ---------------------------------------------------------------- the bound
def bound(abs_score, abs_T, max_terms=3):
    """B = 4 n eps (sum_t max_l abs_score[t, l] + (n - 1) max abs_T): ``abs_score [n, L]`` holds per (item, label) the sum of the
    absolute values of the products that make up the item score (at most ``max_terms`` of them, and the constant 4 is derived
    for max_terms <= 3: the module docstring)."""
    if max_terms > 3:
        raise ValueError("c = 4 is derived for item scores of at most 3 terms")
    n = abs_score.shape[0]
    total = float(abs_score.max(axis=1).sum()) + (n - 1) * (float(np.max(abs_T)) if n > 1 else 0.0)
    return 4.0 * n * EPS * total
