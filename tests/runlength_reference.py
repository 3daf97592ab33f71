"""Run-length potentials in plain numpy: the independent yardstick of ``gecco_crf_viterbi_run_length`` and
``gecco_crf_marginals_run_length`` (tests/test_gpu_runlength.py), pinned on path enumeration by tests/test_runlength_host.py.  It
shares no code with the product.

A sequence is a table of item scores ``score [n, L]`` (``-inf`` at a disallowed (item, label) pair) and transition weights
``T [L, L]``; a label set is a bit mask.  A run is a maximal stretch of consecutive items with labels inside the set, runs at
either end of the sequence included.  The length model is a table ``g`` of M scores and a tail score ``tau``, each finite or
``-inf``; a path whose runs have n_r items has

    score_g(y) = score(y) + sum over runs of ( g[min(n_r, M) - 1] + tau * max(n_r - M, 0) )

(``g`` is 0-based here: ``g[d - 1]`` scores min(length, M) = d), and a term of ``-inf`` makes the path infeasible.

Four parts:
  * ``enumerate_all``: every one of the L**n paths with ``score_g`` straight from the definition -- short sequences only;
  * ``forward_backward``: the recursion over the EXPLICIT list of expanded states (a label outside the set has one state
    ``(j, 0)``, a label inside the states ``(j, d)``, d = 1 .. M, d = min(run length so far, M); by label, then by d) and a DENSE
    table of expanded transitions with the length scores on the edges that end a run or extend one beyond M, and an end vector
    for the run that reaches the last item; ``numpy.longdouble`` is the yardstick.  The counts are edge posteriors of that
    table -- not the product's exit continuation;
  * ``max_recursion``: the max semiring in float64 with the product's stated operation order ``((delta + g or tau) + trans) +
    state`` and its operational tie rule (sources in ascending label order, a label's tau source behind its other one, a strict
    ``>``; the aggregate with d ascending; the smaller label at the end), so that integer weights give the product's path and
    score bits.  It also says whether any maximum it took was tied;
  * ``path_score_g``: one path's score in that operation order, and ``observed_counts``: a path's run-length counts."""
import itertools

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def inside_labels(mask, L):
    return np.array([(int(mask) >> y) & 1 for y in range(L)], dtype=bool)


def runs_of(path, mask):
    """The lengths of the maximal runs of labels inside the set, left to right."""
    out, run = [], 0
    for y in path:
        if (int(mask) >> int(y)) & 1:
            run += 1
        else:
            if run:
                out.append(run)
            run = 0
    if run:
        out.append(run)
    return out


def observed_counts(path, mask, M):
    """[M + 1]: entry d - 1 the number of runs with min(length, M) = d, the last entry the number of items beyond the M-th."""
    out = np.zeros(M + 1)
    for n in runs_of(path, mask):
        out[min(n, M) - 1] += 1
        out[M] += max(n - M, 0)
    return out


def length_terms(path, mask, g, tau, dtype=np.longdouble):
    """The sum of the length scores of the path's runs; -inf when one of them is."""
    M = len(g)
    total = dtype(0)
    for n in runs_of(path, mask):
        total = total + dtype(g[min(n, M) - 1])
        if n > M:  # (no 0 * -inf)
            total = total + dtype(tau) * dtype(n - M)
    return total


def plain_score(score, T, path, dtype=np.longdouble):
    s = dtype(score[0, path[0]])
    for t in range(1, len(path)):
        s = (s + dtype(T[path[t - 1], path[t]])) + dtype(score[t, path[t]])
    return s


def path_score_g(score, T, path, mask, g, tau):
    """score_g of one path in float64, in the product's operation order: ((delta + g or tau) + trans) + state along the path,
    and + g for a run that reaches the last item."""
    M = len(g)
    ins = inside_labels(mask, score.shape[1])
    s = np.float64(score[0, path[0]])
    run = 1 if ins[path[0]] else 0
    for t in range(1, len(path)):
        i, j = path[t - 1], path[t]
        if run and not ins[j]:
            s = s + np.float64(g[min(run, M) - 1])
        elif run >= M and ins[j]:
            s = s + np.float64(tau)
        s = (s + np.float64(T[i, j])) + np.float64(score[t, j])
        run = run + 1 if ins[j] else 0
    if run:
        s = s + np.float64(g[min(run, M) - 1])
    return float(s)


def enumerate_all(score, T, mask, g, tau):
    """By enumeration of all L**n paths, score_g straight from the definition in longdouble: a dict with ``best`` (float, -inf
    without a feasible path), ``paths`` (the feasible paths of that score), ``logz`` (longdouble), ``marg`` [n, L] and ``counts``
    [M + 1] (zeros without a feasible path)."""
    n, L = score.shape
    M = len(g)
    paths, terms = [], []
    for p in itertools.product(range(L), repeat=n):
        s = plain_score(score, T, p)
        if s == -np.inf:
            continue
        s = s + length_terms(p, mask, g, tau)
        if s == -np.inf:
            continue
        paths.append(p)
        terms.append(s)
    out = dict(best=-np.inf, paths=[], logz=np.longdouble(-np.inf), marg=np.zeros((n, L), dtype=np.longdouble),
               counts=np.zeros(M + 1, dtype=np.longdouble))
    if not terms:
        return out
    terms = np.array(terms, dtype=np.longdouble)
    mx = terms.max()
    out["best"] = float(mx)
    out["paths"] = [p for p, s in zip(paths, terms) if s == mx]
    out["logz"] = mx + np.log(np.exp(terms - mx).sum())
    w = np.exp(terms - out["logz"])
    for p, wp in zip(paths, w):
        out["marg"][np.arange(n), list(p)] += wp
        out["counts"] += wp * observed_counts(p, mask, M)
    return out


# ---------------------------------------------------------------- the sum semiring over the explicit state list
def expanded_states(mask, M, L):
    states = []
    for j in range(L):
        if (int(mask) >> j) & 1:
            states.extend((j, d) for d in range(1, M + 1))
        else:
            states.append((j, 0))
    return states


def edge_score(src, dst, M, g, tau):
    """What the step src -> dst adds beyond trans, or None when dst may not follow src."""
    (_, ds), (_, dd) = src, dst
    if dd == 0:                       # to an outside state: a run that ends pays its length score
        return 0.0 if ds == 0 else g[ds - 1]
    if ds == 0:                       # a run starts
        return 0.0 if dd == 1 else None
    if dd != min(ds + 1, M):          # a run goes on: the counter moves on, or stays at M
        return None
    return tau if ds == M else 0.0    # an item beyond the M-th pays the tail score


def expanded_table(T, mask, g, tau, dtype=np.longdouble):
    """(states, E [S, S] with -inf at forbidden pairs, start [S] bool, end [S]: the score of stopping in a state,
    ends [S, S] / tails [S, S] bool: the edges that end a run / that are tail steps)."""
    L, M = T.shape[0], len(g)
    states = expanded_states(mask, M, L)
    S = len(states)
    E = np.full((S, S), -np.inf, dtype=dtype)
    ends, tails = np.zeros((S, S), dtype=bool), np.zeros((S, S), dtype=bool)
    for a, src in enumerate(states):
        for b, dst in enumerate(states):
            extra = edge_score(src, dst, M, g, tau)
            if extra is not None:
                E[a, b] = dtype(T[src[0], dst[0]]) + dtype(extra)
                ends[a, b] = src[1] > 0 and dst[1] == 0
                tails[a, b] = src[1] == M and dst[1] == M
    start = np.array([d <= 1 for _, d in states], dtype=bool)
    end = np.array([0.0 if d == 0 else g[d - 1] for _, d in states], dtype=dtype)
    return states, E, start, end, ends, tails


def lse(c, axis=None):
    """Max-shifted log-sum-exp in c's dtype; -inf where every entry is -inf."""
    mx = c.max(axis=axis)
    shift = np.where(mx == -np.inf, 0, mx).astype(c.dtype)
    with np.errstate(divide="ignore"):
        total = np.exp(c - (shift if axis is None else np.expand_dims(shift, axis))).sum(axis=axis)
        return np.where(mx == -np.inf, -np.inf, shift + np.log(total)).astype(c.dtype)


def forward_backward(score, T, mask, g, tau, dtype=np.longdouble):
    """A dict: ``marg`` [n, L], ``logz``, ``counts`` [M + 1] and ``largest``, the largest finite |alpha, beta or alpha + end| met.
    Without a feasible path the marginals and counts are zeros and ``logz`` is -inf."""
    n, L = score.shape
    M = len(g)
    score = np.asarray(score).astype(dtype)
    states, E, start, end, ends, tails = expanded_table(np.asarray(T), mask, g, tau, dtype)
    label = np.array([j for j, _ in states], dtype=np.int64)
    depth = np.array([d for _, d in states], dtype=np.int64)
    S = len(states)
    ninf = dtype(-np.inf)
    alpha = np.full((n, S), ninf, dtype=dtype)
    beta = np.full((n, S), ninf, dtype=dtype)
    alpha[0] = np.where(start, score[0][label], ninf)
    for t in range(1, n):
        alpha[t] = lse(alpha[t - 1][:, None] + E, axis=0) + score[t][label]
    beta[n - 1] = end
    for t in range(n - 2, -1, -1):
        beta[t] = lse(E + (score[t + 1][label] + beta[t + 1])[None, :], axis=1)
    last = alpha[n - 1] + end
    logz = lse(last)[()]
    both = np.concatenate([alpha.ravel(), beta.ravel(), last])
    fin = both[np.isfinite(both)]
    out = dict(marg=np.zeros((n, L), dtype=dtype), logz=logz, counts=np.zeros(M + 1, dtype=dtype),
               largest=float(np.abs(fin).max()) if fin.size else 0.0)
    if logz == -np.inf:
        return out
    ab = alpha + beta
    p = np.where(ab == -np.inf, dtype(0), np.exp(ab - logz)).astype(dtype)
    for s in range(S):  # (ascending d within a label)
        out["marg"][:, label[s]] += p[:, s]
    # the counts: posteriors of the edges that end a run, by the source's d, and of the tail steps; a run that reaches the last item
    runs = np.flatnonzero(depth > 0)
    for t in range(n - 1):
        xi = (alpha[t][:, None] + E) + (score[t + 1][label] + beta[t + 1])[None, :]
        w = np.where(xi == -np.inf, dtype(0), np.exp(xi - logz))
        np.add.at(out["counts"], depth[runs] - 1, np.where(ends, w, 0).sum(axis=1)[runs])
        out["counts"][M] += np.where(tails, w, 0).sum()
    w = np.where(last == -np.inf, dtype(0), np.exp(last - logz))
    np.add.at(out["counts"], depth[runs] - 1, w[runs])
    return out


# ---------------------------------------------------------------- the max semiring in the product's order and tie rule
def _first_max(cand):
    """Column-wise over cand [sources, destinations]: (max, index of the first maximum, is any finite maximum tied)."""
    best = cand.max(axis=0)
    arg = cand.argmax(axis=0)
    tied = bool((((cand == best[None, :]).sum(axis=0) > 1) & (best > -np.inf)).any())
    return best, arg, tied


def max_recursion(score, T, mask, g, tau):
    """(path int64 [n] or None, best score_g as a float, tie_free).  float64 throughout; delta[i, d - 1] is state (i, d), an
    outside label's one state sits at slot M - 1, as in the product."""
    n, L = score.shape
    M = len(g)
    score, T = np.asarray(score, dtype=np.float64), np.asarray(T, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    tau = np.float64(tau)
    ins = inside_labels(mask, L)
    top = M - 1
    ninf = -np.inf
    delta = np.full((L, M), ninf)
    delta[np.arange(L), np.where(ins, 0, top)] = score[0]
    tie = False

    def aggregate(delta):
        nonlocal tie
        v = np.where(ins[:, None], delta + g[None, :], ninf)
        best, arg, tied = _first_max(v.T)
        tie = tie or tied
        return np.where(ins, best, delta[:, top]), arg

    A, argd = aggregate(delta)
    backs, exits = [], [argd]
    for t in range(1, n):
        new = np.full((L, M), ninf)
        bk = np.zeros((L, M, 2), dtype=np.int64)  # (source label, 1 if the tau source)
        # the tau sources of the last slot: (i, M), i inside
        second = np.where(ins[:, None], (delta[:, top][:, None] + tau) + T, ninf)
        for d in range(M):
            if d == 0:
                first_in = np.where(~ins[:, None], A[:, None] + T, ninf)
            else:
                first_in = np.where(ins[:, None], delta[:, d - 1][:, None] + T, ninf)
            if d == top:
                cand = np.stack([first_in, second], axis=1).reshape(2 * L, L)  # (i first, i second) interleaved
                best, arg, tied = _first_max(cand)
                src, sec = arg // 2, arg % 2
            else:
                best, arg, tied = _first_max(first_in)
                src, sec = arg, np.zeros(L, dtype=np.int64)
            tie = tie or (tied and bool(ins.any()))
            new[ins, d] = (best + score[t])[ins]
            bk[ins, d, 0], bk[ins, d, 1] = src[ins], sec[ins]
        best, arg, tied = _first_max(A[:, None] + T)   # an outside destination: every label's aggregate
        tie = tie or (tied and bool((~ins).any()))
        new[~ins, top] = (best + score[t])[~ins]
        bk[~ins, top, 0] = arg[~ins]
        delta = new
        A, argd = aggregate(delta)
        backs.append(bk)
        exits.append(argd)
    final = A.max()
    if final == -np.inf:
        return None, -np.inf, not tie
    tie = tie or int((A == final).sum()) > 1
    j = int(A.argmax())  # (the smaller label among equal aggregates)
    slot = int(exits[n - 1][j]) if ins[j] else top
    path = np.zeros(n, dtype=np.int64)
    for t in range(n - 1, -1, -1):
        path[t] = j
        if t == 0:
            break
        i, sec = (int(x) for x in backs[t - 1][j, slot])
        if not ins[j]:
            slot = int(exits[t - 1][i]) if ins[i] else top
        elif sec:
            slot = top
        elif slot == 0:
            slot = top
        else:
            slot -= 1
        j = i
    return path, float(final), not tie


# ---------------------------------------------------------------- the bounds of the device tests, derived
def log_bound(n, L, M, largest):
    """A log-quantity of the device (a forward value, a backward value, log Z_g) against its exact value: per item at most 2 L
    exponentials and positive additions, one logarithm and three additions (the min-run bound of
    tests/minrun_reference.lognorm_bound), and the aggregate's (or the backward walk's exit and stay combination's) M + 2
    operations more, each at magnitude <= ``largest``: (n + 1)(2 L + 8 + M + 2) eps max(1, largest)."""
    return (n + 1) * (2 * L + 8 + M + 2) * EPS * max(1.0, largest)


def marginal_bound(n, L, M, largest):
    """Relative, where the yardstick's value is >= 1e-280: three log-quantities per term (alpha, beta, log Z_g) and the sum over
    the run counter, (M + 4) eps."""
    return float(np.expm1(3.0 * log_bound(n, L, M, largest) + (M + 4) * EPS))


def count_bound(n, L, M, largest):
    """Relative: a count is a sum of at most n L non-negative terms, each exp of three log-quantities (alpha + g, the
    continuation, log Z_g) and two additions; the sum itself adds (n L + L) eps."""
    return float(np.expm1(3.0 * log_bound(n, L, M, largest) + (n * L + L + 4) * EPS))
