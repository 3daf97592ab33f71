"""Run posteriors in numpy, log space: the independent yardstick of ``gecco_crf_run_posteriors`` (tests/test_gpu_runs.py),
pinned on path enumeration by tests/test_runs_host.py.  It shares no code with the product.

Fix a sequence of masked item scores ``X`` [T, L] (``cr.masked_scores``: ``-inf`` at a disallowed pair), the transition weights,
an anchor item ``a`` and a label set ``S`` (a uint32 mask).  The run through ``a`` is the maximal stretch of items around ``a``
whose labels all lie in ``S``.

(a) By definition.  Every quantity is ``log Z_A' - log Z_A``, both from ``cr.marginals``: A the lattice of ``X``, A' the same
    with ``-inf`` written over the labels outside ``S`` on the run's items and over the labels inside ``S`` on the neighbour that
    has to end the run.  An item left without a label makes the result ``-inf`` outright.  One forward-backward per entry: slow,
    for single entries and samples of them.
(b) A direct log-space recursion that gives a whole distribution in one walk away from the anchor, on unscaled log forward and
    backward vectors (log space has the range).  tests/test_runs_host.py holds (a), (b) and enumeration within 1e-12 of each
    other with equal ``-inf`` patterns.

Every function returns, beside the log-probabilities, ``inner`` = log Z_A' of every entry (``-inf`` where there is no path): the
tolerance of a log-ratio is ``1e-10 (max(1, |log Z_A'|) + max(1, |log Z_A|))`` (``bound``)."""
import itertools

import numpy as np

from tests import constrained_reference as cr
from tests.train_objective_partial import mask_matrix

NINF = -np.inf


def inside_of(mask, L):
    return mask_matrix(np.array([mask], dtype=np.uint32), L)[0]


def bound(inner, logz):
    inner = np.asarray(inner, dtype=np.float64)
    return 1e-10 * (np.where(np.isfinite(inner), np.maximum(1.0, np.abs(inner)), 1.0) + max(1.0, abs(logz)))


# ---------------------------------------------------------------- (a) by definition
def log_z(X, trans):
    """log Z of one sequence of masked scores; -inf outright when an item is left without a label."""
    if np.any(np.all(np.isneginf(X), axis=1)):
        return NINF
    return float(cr.marginals(np.array([0, len(X)]), X, trans)[1][0])


def restricted(X, inside, first, last, closed_left, closed_right):
    """X with the items first .. last held inside the set, and the neighbour on a closed side held outside it (a closed side at
    the sequence's edge needs nothing)."""
    Y = X.copy()
    Y[first:last + 1, ~inside] = NINF
    if closed_left and first > 0:
        Y[first - 1, inside] = NINF
    if closed_right and last + 1 < len(X):
        Y[last + 1, inside] = NINF
    return Y


def run_by_definition(X, trans, begin, end, mask):
    """(log P(the run is exactly [begin, end)), log Z_A', log Z_A)."""
    inner = log_z(restricted(X, inside_of(mask, X.shape[1]), begin, end - 1, True, True), trans)
    logz = log_z(X, trans)
    return inner - logz, inner, logz


def anchor_entry_by_definition(X, trans, a, mask, what, r=0, reach=0):
    """One entry of an anchor query, (value, log Z_A', log Z_A): what = "anchor", "start" (entry r), "start_beyond" (at
    `reach`), "end", "end_beyond"."""
    T, inside = len(X), inside_of(mask, X.shape[1])
    logz = log_z(X, trans)
    if what == "anchor":
        first, last, cl, cr_ = a, a, False, False
    elif what == "start":
        first, last, cl, cr_ = a - r, a, True, False
    elif what == "start_beyond":
        first, last, cl, cr_ = a - reach - 1, a, False, False
    elif what == "end":
        first, last, cl, cr_ = a, a + r, False, True
    else:
        first, last, cl, cr_ = a, a + reach + 1, False, False
    if first < 0 or last >= T:
        return NINF, NINF, logz
    inner = log_z(restricted(X, inside, first, last, cl, cr_), trans)
    return inner - logz, inner, logz


def anchor_by_definition(X, trans, a, mask, reach):
    """The whole anchor query by (a): a dict of values and a dict of log Z_A' under the keys of the product, and log Z_A."""
    val, inn = {}, {}
    for key, what in (("log_anchor", "anchor"), ("log_start_beyond", "start_beyond"), ("log_end_beyond", "end_beyond")):
        val[key], inn[key], logz = anchor_entry_by_definition(X, trans, a, mask, what, reach=reach)
    for key, what in (("log_start", "start"), ("log_end", "end")):
        rows = [anchor_entry_by_definition(X, trans, a, mask, what, r=r) for r in range(reach + 1)]
        val[key], inn[key] = np.array([x[0] for x in rows]), np.array([x[1] for x in rows])
    return val, inn, logz


# ---------------------------------------------------------------- (b) the direct recursion
def _lse(v):
    """log-sum-exp of a vector that may be empty or all -inf (then -inf)."""
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return NINF
    m = float(np.max(v))
    if m == NINF:
        return NINF
    return m + float(np.log(np.sum(np.exp(v - m))))


def _lse_rows(Mx):
    """log-sum-exp along axis 1 of a matrix that may hold all -inf rows."""
    m = np.max(Mx, axis=1)
    safe = np.where(np.isneginf(m), 0.0, m)
    with np.errstate(divide="ignore"):
        return np.where(np.isneginf(m), NINF, safe + np.log(np.sum(np.exp(Mx - safe[:, None]), axis=1)))


def forward_backward(X, trans):
    """Unscaled log alpha [T, L], log beta [T, L] and log Z."""
    T, L = X.shape
    la, lb = np.full((T, L), NINF), np.zeros((T, L))
    la[0] = X[0]
    for t in range(1, T):
        la[t] = _lse_rows((la[t - 1][:, None] + trans).T) + X[t]
    for t in range(T - 2, -1, -1):
        lb[t] = _lse_rows(trans + (X[t + 1] + lb[t + 1])[None, :])
    return la, lb, _lse(la[-1])


def anchor_direct(X, trans, a, mask, reach, fb=None):
    """The whole anchor query by (b): (values, log Z_A' of every entry, log Z_A), dicts under the keys of the product."""
    T, L = X.shape
    inside = inside_of(mask, L)
    la, lb, logz = fb if fb is not None else forward_backward(X, trans)
    tot = {"log_start": np.full(reach + 1, NINF), "log_end": np.full(reach + 1, NINF), "log_start_beyond": NINF,
           "log_end_beyond": NINF}
    # leftwards: c_t(j) = [j in S] psi_t(j) sum_k M(j, k) c_{t+1}(k), c_a = [S] psi_a beta_a
    c = np.where(inside, X[a] + lb[a], NINF)
    tot["log_anchor"] = _lse((la[a] + lb[a])[inside])
    for r in range(reach + 2):
        t = a - r
        if t < 0:
            break
        if r == reach + 1:
            # P(y_t .. y_a in S): the masked vector with every way into item t
            if t == 0:
                tot["log_start_beyond"] = _lse(c)
            else:
                d = _lse_rows(trans + c[None, :])
                tot["log_start_beyond"] = _lse(la[t - 1] + d)
            break
        if t == 0:
            tot["log_start"][r] = _lse(c)
            break
        d = _lse_rows(trans + c[None, :])
        tot["log_start"][r] = _lse((la[t - 1] + d)[~inside])
        c = np.where(inside, X[t - 1] + d, NINF)
    # rightwards: c_t(j) = [j in S] psi_t(j) sum_i c_{t-1}(i) M(i, j), c_a = [S] alpha_a
    c = np.where(inside, la[a], NINF)
    for r in range(reach + 2):
        t = a + r
        if t >= T:
            break
        if r == reach + 1:
            tot["log_end_beyond"] = _lse(c + lb[t])
            break
        if t == T - 1:
            tot["log_end"][r] = _lse(c)
            break
        d = _lse_rows((c[:, None] + trans).T)
        tot["log_end"][r] = _lse((d + X[t + 1] + lb[t + 1])[~inside])
        c = np.where(inside, X[t + 1] + d, NINF)
    val = {k: (v - logz if np.ndim(v) else float(v - logz)) for k, v in tot.items()}
    return val, tot, logz


def joint_row_direct(X, trans, s, mask, fb=None):
    """log P(a run starts at s and its last item is e) for every e >= s, by (b): (values [T - s], log Z_A' [T - s], log Z_A)."""
    T, L = X.shape
    inside = inside_of(mask, L)
    la, lb, logz = fb if fb is not None else forward_backward(X, trans)
    if s == 0:
        c = np.where(inside, X[0], NINF)
    else:
        c = np.where(inside, _lse_rows((np.where(inside, NINF, la[s - 1])[:, None] + trans).T) + X[s], NINF)
    tot = np.full(T - s, NINF)
    for e in range(s, T):
        if e == T - 1:
            tot[e - s] = _lse(c)
            break
        d = _lse_rows((c[:, None] + trans).T)
        tot[e - s] = _lse((d + X[e + 1] + lb[e + 1])[~inside])
        c = np.where(inside, X[e + 1] + d, NINF)
    return tot - logz, tot, logz


# ---------------------------------------------------------------- enumeration (short sequences)
def enumerate_runs(X, trans, mask):
    """Every path through one short sequence.  Returns (log Z, anchor [T], start [T, T], end [T, T], joint [T, T + 1]) in log
    space: anchor[a] = log P(y_a in S); start[a, s] = log P(the run through a starts at s); end[a, e] = log P(its last item is
    e); joint[b, e] = log P(a run is exactly [b, e))."""
    T, L = X.shape
    inside = inside_of(mask, L)
    paths = list(itertools.product(range(L), repeat=T))
    sc = np.array([X[0, p[0]] + sum(trans[p[t - 1], p[t]] + X[t, p[t]] for t in range(1, T)) for p in paths])
    m = sc.max()
    logz = m + np.log(np.sum(np.exp(sc - m)))
    w = np.exp(sc - logz)
    anchor, start, end, joint = np.zeros(T), np.zeros((T, T)), np.zeros((T, T)), np.zeros((T, T + 1))
    for p, wp in zip(paths, w):
        t = 0
        while t < T:
            if not inside[p[t]]:
                t += 1
                continue
            b = t
            while t < T and inside[p[t]]:
                t += 1
            joint[b, t] += wp
            for a in range(b, t):
                anchor[a] += wp
                start[a, b] += wp
                end[a, t - 1] += wp
    with np.errstate(divide="ignore"):
        return float(logz), np.log(anchor), np.log(start), np.log(end), np.log(joint)
