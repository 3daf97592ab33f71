"""Decoding under a minimum run length in plain numpy: the independent yardstick of ``gecco_crf_viterbi_min_run``
(tests/test_gpu_minrun.py), pinned on path enumeration by tests/test_minrun_host.py.  It shares no code with the product.

A sequence is a table of item scores ``score [n, L]`` (``-inf`` at a disallowed (item, label) pair, as
tests.constrained_reference.masked_scores builds it) and transition weights ``T [L, L]``.  A label set is a bit mask (bit y set:
label y is inside); a path is feasible under (mask, m) when every maximal run of consecutive items with labels inside the set has
at least m items, runs at either end of the sequence included.  A path's score is the left-to-right sum
``((score[0, y0] + T[y0, y1]) + score[1, y1]) + T[y1, y2]) + ...``; a path of score ``-inf`` does not exist.

Three parts:
  * ``recursion``: the recursion over states expanded by a run counter, in the max semiring (float64, the kernel's source order
    and strict ``>`` update, so that integer weights give the kernel's path and score bits) and in the sum semiring
    (``numpy.longdouble`` by default; the same sources, summed in the linear domain under a shift per item);
  * ``enumerate_paths``: every one of the L**n paths with the feasibility predicate -- short sequences only;
  * ``path_score``, ``feasible``.

The expanded states.  A label outside the set has one state; a label j inside has (j, d), d = 1 .. m, d = min(run length so
far, m).  Here the outside states are a vector ``out [L]`` and the inside states a table ``run [L, m]`` (``run[j, d - 1]``), with
``-inf`` where a label is of the other kind.  A destination's candidates are ``delta[source] + T[i, j]``, scanned in ascending
(source label, source d) order; the first maximum wins (``numpy.argmax``), and the item score is added to the winner: the
operation order of tests.constrained_reference.viterbi_one.  At the end the outside states and the states (j, m) are admissible,
one per label, and the first maximum in label order wins.  This tie rule is operational -- a rule on expanded states, not an
order on paths."""
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


def feasible(path, mask, m):
    """Every maximal run of labels inside the set has at least m items."""
    run = 0
    for y in path:
        if (int(mask) >> int(y)) & 1:
            run += 1
        else:
            if 0 < run < m:
                return False
            run = 0
    return not 0 < run < m


def _logsumexp(c, axis):
    """Max-shifted, in c's dtype; -inf where every entry is -inf."""
    mx = c.max(axis=axis)
    shift = np.where(mx == -np.inf, 0, mx).astype(c.dtype)
    with np.errstate(divide="ignore"):
        return np.where(mx == -np.inf, -np.inf, shift + np.log(np.exp(c - np.expand_dims(shift, axis)).sum(axis=axis))).astype(c.dtype)


REACH = 11000.0  # what one shift holds in longdouble: exp(-11356) is its smallest normal number


def _sum_step(out, run, ins, T, m):
    """_sum_step_once on the states within one shift's reach of the item's largest, and again on their own on those further
    below, whose exp under that shift is 0 or subnormal; the two parts are disjoint sets of sources and add up (log-add-exp).
    A sequence whose only feasible paths cross six transitions of weight -2000, next to infeasible states of ordinary size,
    has log Z_C = -12000, not -inf.  Without states that far below, this is _sum_step_once and its bits."""
    top = max(out.max(), run.max())
    reach = max(REACH - float(T.max() - T[np.isfinite(T)].min()), 1000.0)  # (a product with the smallest exp(T - max T) has to fit as well)
    low_o, low_r = out < top - reach, run < top - reach
    if top == -np.inf or not ((low_o & (out > -np.inf)).any() or (low_r & (run > -np.inf)).any()):
        return _sum_step_once(out, run, ins, T, m)
    ninf = out.dtype.type(-np.inf)
    near = _sum_step_once(np.where(low_o, ninf, out), np.where(low_r, ninf, run), ins, T, m)
    far = _sum_step(np.where(low_o, out, ninf), np.where(low_r, run, ninf), ins, T, m)
    return np.logaddexp(near[0], far[0]), np.logaddexp(near[1], far[1])


def _sum_step_once(out, run, ins, T, m):
    """One item of the sum semiring without the item score: log-sum-exp over every destination's sources, as sums of products
    in the linear domain under one shift for the item (the largest finite forward value) and one for T -- in longdouble, whose
    exponent range holds exp of differences of ten thousand, the log-sum-exp itself to rounding."""
    dtype = out.dtype
    L = len(out)
    new_out, new_run = np.full(L, -np.inf, dtype=dtype), np.full((L, m), -np.inf, dtype=dtype)
    top = max(out.max(), run.max())
    if top == -np.inf:
        return new_out, new_run
    t_top = T.max()
    ET = np.exp(T - t_top)
    Eo, Er = np.exp(out - top), np.exp(run - top)
    with np.errstate(divide="ignore"):
        back = lambda v: (top + t_top) + np.log(v)
        new_out = back(np.where(ins, Er[:, m - 1], Eo) @ ET)
        if m == 1:
            new_run[:, 0] = new_out
        else:
            new_run[:, 0] = back(Eo @ ET)
            if m > 2:
                new_run[:, 1:m - 1] = back(Er[:, :m - 2].T @ ET).T
            new_run[:, m - 1] = back((Er[:, m - 2] + Er[:, m - 1]) @ ET)
    return new_out.astype(dtype), new_run.astype(dtype)


def recursion(score, T, mask, m, semiring="max", dtype=None):
    """max: (path int64 [n] or None, best score); sum: (log Z_C, largest finite |forward value|) in ``dtype``."""
    n, L = score.shape
    best_of = semiring == "max"
    dtype = np.float64 if best_of else (dtype or np.longdouble)
    score, T = score.astype(dtype), T.astype(dtype)
    ins = inside_labels(mask, L)
    ninf = dtype(-np.inf)
    out = np.where(ins, ninf, score[0]).astype(dtype)
    run = np.full((L, m), ninf, dtype=dtype)
    run[ins, 0] = score[0][ins]
    backs = []
    largest = 0.0

    def note(*arrays):
        nonlocal largest
        for a in arrays:
            fin = a[np.isfinite(a)]
            if fin.size:
                largest = max(largest, float(np.abs(fin).max()))

    note(out, run)
    for t in range(1, n):
        closing = np.where(ins, run[:, m - 1], out)                 # what a label offers a destination that ends a run
        # candidates [source, destination], sources in ascending (label, d) order
        cand_out = closing[:, None] + T                              # -> j outside (and, with m = 1, -> (j, 1))
        if m > 1 and best_of:
            cand_first = out[:, None] + T                            # -> (j, 1): from outside labels only
            cand_mid = run[:, :m - 2, None] + T[:, None, :]          # -> (j, d), 1 < d < m: [i, d - 2, j]
            cand_full = (run[:, m - 2:, None] + T[:, None, :]).reshape(2 * L, L)  # -> (j, m): (i, m - 1), (i, m) interleaved
        new_run = np.full((L, m), ninf, dtype=dtype)
        if best_of:
            pick = lambda c: (c.max(axis=0), c.argmax(axis=0))
            v, a = pick(cand_out)
            new_out = v + score[t]
            bk = {"out": a}
            if m == 1:
                new_run[:, 0] = new_out
                bk["run"] = a[:, None]
            else:
                v, a = pick(cand_first)
                new_run[:, 0] = v + score[t]
                arg = np.zeros((L, m), dtype=np.int64)   # source label; at d = m: 2 * label + (1 if from (i, m))
                arg[:, 0] = a
                if m > 2:
                    new_run[:, 1:m - 1] = (cand_mid.max(axis=0) + score[t][None, :]).T
                    arg[:, 1:m - 1] = cand_mid.argmax(axis=0).T
                v, a = pick(cand_full)
                new_run[:, m - 1] = v + score[t]
                arg[:, m - 1] = a
                bk["run"] = arg
            backs.append(bk)
        else:
            new_out, new_run = _sum_step(out, run, ins, T, m)
            new_out, new_run = new_out + score[t], new_run + score[t][:, None]
        out = np.where(ins, ninf, new_out).astype(dtype)
        run = np.where(ins[:, None], new_run, ninf).astype(dtype)
        note(out, run)
    final = np.where(ins, run[:, m - 1], out)
    if not best_of:
        return _logsumexp(final, 0)[()], largest
    j = int(final.argmax())
    if final[j] == -np.inf:
        return None, -np.inf
    path = np.zeros(n, dtype=np.int64)
    d = m if ins[j] else 0  # (0: an outside state)
    for t in range(n - 1, -1, -1):
        path[t] = j
        if t == 0:
            break
        bk = backs[t - 1]
        if d == 0 or m == 1:
            i = int(bk["out"][j] if d == 0 else bk["run"][j, 0])
            d = m if ins[i] else 0
        elif d == 1:
            i, d = int(bk["run"][j, 0]), 0
        elif d < m:
            i, d = int(bk["run"][j, d - 1]), d - 1
        else:
            i, full = divmod(int(bk["run"][j, m - 1]), 2)
            d = m if full else m - 1
        j = i
    return path, float(final[path[-1]])


def enumerate_paths(score, T, mask, m):
    """(best score, [the feasible paths of that score], log Z_C in longdouble, number of feasible paths that exist), by
    enumeration of all L**n; (-inf, [], -inf, 0) when there is none."""
    n, L = score.shape
    best, arg, terms = -np.inf, [], []
    for p in itertools.product(range(L), repeat=n):
        if not feasible(p, mask, m):
            continue
        s = path_score(score, T, p)
        if s == -np.inf:
            continue
        terms.append(path_score(score, T, p, np.longdouble))
        if s > best:
            best, arg = s, [p]
        elif s == best:
            arg.append(p)
    if not terms:
        return -np.inf, [], np.longdouble(-np.inf), 0
    terms = np.array(terms, dtype=np.longdouble)
    mx = terms.max()
    return best, arg, mx + np.log(np.exp(terms - mx).sum()), len(terms)


def lognorm_bound(n, L, largest):
    """(n + 1)(2 L + 8) eps max(1, M): per item at most 2 L exponentials and positive additions, one logarithm and three
    additions at magnitude <= M, the largest finite |forward value| of the reference on the sequence."""
    return (n + 1) * (2 * L + 8) * EPS * max(1.0, largest)
