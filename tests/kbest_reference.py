"""The K best label paths in plain Python and numpy: the independent yardstick of ``gecco_crf_viterbi_kbest``
(tests/test_gpu_kbest.py), pinned on path enumeration by tests/test_kbest_host.py.  It shares no code with the product.

A sequence is a table of item scores ``score [n, L]`` (``-inf`` at a disallowed (item, label) pair, as
tests.constrained_reference.masked_scores builds it) and transition weights ``T [L, L]``.  A path's score is the left-to-right
sum ``((score[0, y0] + T[y0, y1]) + score[1, y1]) + T[y1, y2]) + ...``, the operation order of
tests.constrained_reference.viterbi_one.  The order of the paths is total: score descending, then the reversed path
``(y_{n-1}, ..., y_0)`` ascending.  A path of score ``-inf`` does not exist.

Three forms of the same rule:
  * ``enumerate_kbest``: every one of the L**n paths, scored and sorted -- short sequences only;
  * ``list_dp``: the list recursion with Python lists, per (item, label) the K best prefixes, candidates in (source label,
    source rank) order under a stable sort;
  * ``list_dp_numpy``: the same recursion with numpy's stable sort, for the longer sequences of the device tests.

The separation rule of the device tests lives here too (``bound``, ``separated``), so that the CPU test can count, with the
yardstick alone, how many ranks a seed leaves unseparated."""
import itertools

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def path_score(score, T, path):
    s = score[0, path[0]]
    for t in range(1, len(path)):
        s = (s + T[path[t - 1], path[t]]) + score[t, path[t]]
    return float(s)


def enumerate_kbest(score, T, k):
    """[(path tuple, score)] of the k best paths, by enumeration of all L**n."""
    n, L = score.shape
    found = []
    for p in itertools.product(range(L), repeat=n):
        s = path_score(score, T, p)
        if s != -np.inf:
            found.append((-s, p[::-1]))
    found.sort()
    return [(rev[::-1], -neg) for neg, rev in found[:k]]


def list_dp(score, T, k):
    """[(path tuple, score)] of the k best paths by the list recursion, Python lists throughout."""
    n, L = score.shape
    # lists[j] = [(score, back)] best first; back = (source label, source rank) or None at item 0
    lists = [[(float(score[0, j]), None)] if score[0, j] != -np.inf else [] for j in range(L)]
    history = [lists]
    for t in range(1, n):
        new = []
        for j in range(L):
            cand = []
            for i in range(L):
                for r, (s, _) in enumerate(lists[i]):
                    v = float((s + T[i, j]) + score[t, j])
                    if v != -np.inf:
                        cand.append((v, (i, r)))
            cand.sort(key=lambda c: -c[0])  # (stable: equal scores stay in (i, r) order)
            new.append(cand[:k])
        lists = new
        history.append(lists)
    last = [(s, (j, r)) for j in range(L) for r, (s, _) in enumerate(lists[j])]
    last.sort(key=lambda c: -c[0])
    out = []
    for s, (j, r) in last[:k]:
        path = []
        for t in range(n - 1, -1, -1):
            path.append(j)
            back = history[t][j][r][1]
            if back is not None:
                j, r = back
        out.append((tuple(path[::-1]), s))
    return out


def list_dp_numpy(score, T, k):
    """``list_dp`` with numpy's stable sort: (paths int64 [m, n], scores [m]), m <= k the number of paths that exist."""
    n, L = score.shape
    D = np.full((L, k), -np.inf)
    D[:, 0] = score[0]
    backs = []
    cols = np.arange(L)
    for t in range(1, n):
        cand = ((D[:, :, None] + T[:, None, :]).reshape(L * k, L)) + score[t][None, :]  # rows in (i, r) order
        order = np.argsort(-cand, axis=0, kind="stable")[:k]                              # [k, L]
        D = cand[order, cols[None, :]].T.copy()
        backs.append(order.T)  # [L, k]: i * k + r
    flat = D.reshape(-1)       # (j, r) order
    order = np.argsort(-flat, kind="stable")[:k]
    order = order[flat[order] != -np.inf]
    paths = np.zeros((len(order), n), dtype=np.int64)
    for m, o in enumerate(order.tolist()):
        j, r = divmod(o, k)
        for t in range(n - 1, -1, -1):
            paths[m, t] = j
            if t:
                j, r = divmod(int(backs[t - 1][j, r]), k)
    return paths, flat[order]


def kbest(score, T, k):
    """(paths [m, n], scores [m]) by enumeration where the lattice is small, else by the numpy list recursion."""
    n, L = score.shape
    if L ** n <= 4096:
        found = enumerate_kbest(score, T, k)
        return (np.array([p for p, _ in found], dtype=np.int64).reshape(len(found), n), np.array([s for _, s in found]))
    return list_dp_numpy(score, T, k)


def bound(path, abs_score, abs_T):
    """B = 4 n eps (sum of |terms of the path|): ``abs_score [n, L]`` holds per (item, label) the sum of the absolute values of
    the products that make up the item score, ``abs_T = |T|``.  A left-to-right sum of m terms is off by at most (m - 1) eps
    times the sum of their absolute values, to first order; a path has n item scores (each a short sum of its own) and n - 1
    transitions, so 4 n covers it with room."""
    n = len(path)
    total = float(abs_score[np.arange(n), path].sum())
    if n > 1:
        total += float(abs_T[path[:-1], path[1:]].sum())
    return 4.0 * n * EPS * total


def separated(scores, bounds):
    """Per rank of a reference list computed with ONE RANK MORE than the call under test (so that the last rank tested has a
    neighbour behind it where a further path exists): True where the score is more than 2 B from both neighbours, B the
    larger of the two paths' bounds.  One flag per rank given; the caller slices to the ranks it tests."""
    m = len(scores)
    ok = np.ones(m, dtype=bool)
    for r in range(m):
        for o in (r - 1, r + 1):
            if 0 <= o < m and abs(scores[r] - scores[o]) <= 2.0 * max(bounds[r], bounds[o]):
                ok[r] = False
    return ok
