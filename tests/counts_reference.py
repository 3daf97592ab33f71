"""Run-count posteriors in plain numpy: the independent yardstick of ``gecco_crf_run_counts`` (tests/test_gpu_counts.py), pinned on
path enumeration by tests/test_counts_host.py.  It shares no code with the product.

A sequence is a table of item scores ``score [n, L]`` (``-inf`` at a disallowed (item, label) pair, as
tests.constrained_reference.masked_scores builds it) and transition weights ``T [L, L]``.  A label set is a bit mask (bit y set:
label y is inside); ``n_runs(path, mask)`` is the number of maximal runs of consecutive items with labels inside the set, runs at
either end of the sequence included.  With K = max_runs, slot k < K holds the paths with exactly k runs and slot K those with at
least K.  A path's score is the left-to-right sum ``((score[0, y0] + T[y0, y1]) + score[1, y1]) + T[y1, y2]) + ...``; a path of
score ``-inf`` does not exist.

Three parts:
  * ``recursion``: the recursion over states expanded by a saturating run counter, in the max semiring (float64, the kernel's
    source order and strict ``>`` update, so that integer weights give the kernel's paths and score bits) and in the sum semiring
    (``numpy.longdouble``; the same sources, summed in the linear domain under a shift per item);
  * ``enumerate_paths``: every one of the L**n paths, sorted into the slots -- short sequences only;
  * ``path_score``, ``n_runs``, ``lognorm_bound``.

The expanded states are a table ``D [L, K + 1]``: ``D[j, c]`` is state (j, c), c = min(runs begun up to and including this item,
K), with ``-inf`` at (j inside, 0), which does not exist.  A destination's candidates are ``D[source] + T[i, j]``, scanned in
ascending (source label, source slot) order; the first maximum wins (``numpy.argmax``), and the item score is added to the
winner.  A label outside the set takes (i, c) of every label; a label inside takes (i, c) of the labels inside, (i, c - 1) of the
labels outside, and at c = K also (i, K) of the labels outside.  At the end every state is admissible; slot k takes the first
maximum over labels of ``D[:, k]``.  This tie rule is operational -- a rule on expanded states, not an order on paths."""
import itertools

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def path_score(score, T, path, dtype=np.float64):
    s = dtype(score[0, path[0]])
    for t in range(1, len(path)):
        s = (s + dtype(T[path[t - 1], path[t]])) + dtype(score[t, path[t]])
    return s if dtype is not np.float64 else float(s)


def inside_labels(mask, L):
    return np.array([(int(mask) >> y) & 1 for y in range(L)], dtype=bool)


def n_runs(path, mask):
    """The number of maximal runs of labels inside the set."""
    runs, before = 0, False
    for y in path:
        now = bool((int(mask) >> int(y)) & 1)
        runs += now and not before
        before = now
    return runs


def _lowered(D, ins):
    """What label i offers an inside destination at slot c: (i, c) if i is inside, (i, c - 1) if outside (nothing at c = 0)."""
    low = np.full_like(D, -np.inf)
    low[:, 1:] = D[:, :-1]
    return np.where(ins[:, None], D, low)


def _max_step(D, ins, T, K):
    """One item of the max semiring without the item score: (values [L, K + 1], back-pointers)."""
    L = len(ins)
    plain = D[:, None, :] + T[:, :, None]                      # [i, j, c]: -> (j outside, c)
    low = _lowered(D, ins)
    begun = low[:, None, :] + T[:, :, None]                    # [i, j, c]: -> (j inside, c), one source per label
    tail = np.empty((2 * L, L))                                # -> (j inside, K): (i, K - 1) then (i, K) of an outside label
    tail[0::2] = low[:, K, None] + T
    tail[1::2] = np.where(ins, -np.inf, D[:, K])[:, None] + T
    new = np.where(ins[:, None], begun.max(axis=0), plain.max(axis=0))
    new[ins, 0] = -np.inf
    new[ins, K] = tail.max(axis=0)[ins]
    return new, (plain.argmax(axis=0), begun.argmax(axis=0), tail.argmax(axis=0))


REACH = 11000.0  # what one shift holds in longdouble: exp(-11356) is its smallest normal number


def _sum_step(D, ins, T, K):
    """_sum_step_once on the states within one shift's reach of the item's largest, and again on their own on those further
    below, whose exp under that shift is 0 or subnormal; the two parts are disjoint sets of sources and add up (log-add-exp).
    Under a label that leads by 800 per item a count's mass lies 12000 below another's after 15 items and is not -inf.
    Without states that far below, this is _sum_step_once and its bits."""
    top = D.max()
    reach = max(REACH - float(T.max() - T[np.isfinite(T)].min()), 1000.0)  # (a product with the smallest exp(T - max T) has to fit as well)
    low = D < top - reach
    if top == -np.inf or not (low & (D > -np.inf)).any():
        return _sum_step_once(D, ins, T, K)
    ninf = D.dtype.type(-np.inf)
    return np.logaddexp(_sum_step_once(np.where(low, ninf, D), ins, T, K), _sum_step(np.where(low, D, ninf), ins, T, K))


def _sum_step_once(D, ins, T, K):
    """One item of the sum semiring without the item score: sums of products in the linear domain under one shift for the item
    (the largest finite forward value) and one for T -- in longdouble, whose exponent range holds exp of differences of ten
    thousand."""
    new = np.full_like(D, -np.inf)
    top = D.max()
    if top == -np.inf:
        return new
    t_top = T.max()
    ET, E = np.exp(T - t_top), np.exp(D - top)
    low = np.exp(_lowered(D, ins) - top)
    lin = np.where(ins[:, None], ET.T @ low, ET.T @ E)          # [j, c]
    lin[ins, 0] = 0
    lin[ins, K] += (ET.T @ np.where(ins, 0, E[:, K]))[ins]
    with np.errstate(divide="ignore"):
        return ((top + t_top) + np.log(lin)).astype(D.dtype)


def recursion(score, T, mask, K, semiring="max"):
    """max: (paths: K + 1 int64 arrays [n] or None, scores float64 [K + 1]); sum: (log Z_k longdouble [K + 1], the largest finite
    |forward value|).  A sequence without items: the empty path in slot 0, score and log-mass 0."""
    n, L = score.shape
    best_of = semiring == "max"
    dtype = np.float64 if best_of else np.longdouble
    ninf = dtype(-np.inf)
    if n == 0:
        first = np.full(K + 1, ninf, dtype=dtype)
        first[0] = 0
        return ([np.zeros(0, dtype=np.int64)] + [None] * K, first) if best_of else (first, 0.0)
    score, T = score.astype(dtype), T.astype(dtype)
    ins = inside_labels(mask, L)
    D = np.full((L, K + 1), ninf, dtype=dtype)
    D[~ins, 0] = score[0][~ins]
    D[ins, 1] = score[0][ins]
    backs = []
    largest = 0.0

    def note(a):
        nonlocal largest
        fin = a[np.isfinite(a)]
        if fin.size:
            largest = max(largest, float(np.abs(fin).max()))

    note(D)
    for t in range(1, n):
        if best_of:
            D, bk = _max_step(D, ins, T, K)
            backs.append(bk)
        else:
            D = _sum_step(D, ins, T, K)
        D = (D + score[t][:, None]).astype(dtype)
        note(D)
    if not best_of:
        mx = D.max(axis=0)
        shift = np.where(mx == -np.inf, 0, mx).astype(dtype)
        with np.errstate(divide="ignore"):
            logz = np.where(mx == -np.inf, ninf, shift + np.log(np.exp(D - shift[None, :]).sum(axis=0))).astype(dtype)
        return logz, largest
    paths, scores = [], np.full(K + 1, -np.inf)
    for k in range(K + 1):
        j = int(D[:, k].argmax())
        if D[j, k] == -np.inf:
            paths.append(None)
            continue
        scores[k] = D[j, k]
        path = np.zeros(n, dtype=np.int64)
        c = k
        for t in range(n - 1, -1, -1):
            path[t] = j
            if t == 0:
                break
            plain, begun, tail = backs[t - 1]
            if not ins[j]:
                i = int(plain[j, c])
            elif c < K:
                i = int(begun[j, c])
                c = c if ins[i] else c - 1
            else:
                i, full = divmod(int(tail[j]), 2)
                c = K if ins[i] or full else K - 1
            j = i
        paths.append(path)
    return paths, scores


def enumerate_paths(score, T, mask, K):
    """Per slot, by enumeration of all L**n: (best scores float64 [K + 1], [the paths of that score] per slot, log Z_k longdouble
    [K + 1], the number of paths that exist per slot); -inf, [], -inf, 0 in a slot without a path."""
    n, L = score.shape
    best, arg = np.full(K + 1, -np.inf), [[] for _ in range(K + 1)]
    terms = [[] for _ in range(K + 1)]
    for p in itertools.product(range(L), repeat=n):
        s = path_score(score, T, p) if n else 0.0
        if s == -np.inf:
            continue
        k = min(n_runs(p, mask), K)
        terms[k].append(path_score(score, T, p, np.longdouble) if n else np.longdouble(0))
        if s > best[k]:
            best[k], arg[k] = s, [p]
        elif s == best[k]:
            arg[k].append(p)
    logz = np.full(K + 1, -np.inf, dtype=np.longdouble)
    for k, v in enumerate(terms):
        if v:
            v = np.array(v, dtype=np.longdouble)
            logz[k] = v.max() + np.log(np.exp(v - v.max()).sum())
    return best, arg, logz, [len(v) for v in terms]


def lognorm_bound(n, L, largest):
    """(n + 1)(2 L + 8) eps max(1, M).  No destination has more than 2 L sources (slot K of an inside label: L at most at K, plus
    the outside labels at K - 1 and at K), so per item there are at most 2 L exponentials and positive additions, one logarithm
    and three additions at magnitude <= M, the largest finite |forward value| of the reference on the sequence; the final
    per-slot log-sum-exp over L labels is the "+ 1"."""
    return (n + 1) * (2 * L + 8) * EPS * max(1.0, largest)
