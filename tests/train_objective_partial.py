"""The partial-label ("constrained-lattice") CRF training objective in numpy, log space: the independent yardstick of the
``*_create_partial`` trainers (tests/test_gpu_train_partial.py), pinned on path enumeration by
tests/test_train_partial_host.py.  Every item carries a set of allowed labels, as a uint32 mask with bit y set when label y
is allowed, and

    f(w) = sum over instances of (log Z - log Z_A),    g(w) = E[feature counts] - E_A[feature counts],

Z_A and E_A over the paths with y_t in A_t for every t.  The instances are sliding windows (``W``, ``step``) or, with
``W=None``, the whole sequences.  It shares no code with the product and follows tests/train_objective_labels.py's
conventions: a disallowed label's score is ``-np.inf``, every sum over labels is a log-sum-exp whose maximum is finite
(every item allows a label), so the excluded terms are exact zeros and nothing invalid is ever formed.  Also here: the error
bounds between two fp64 evaluations, and seeded masks."""
import numpy as np

from tests.train_objective_labels import EPS, TINY, _lse, _tables, window_starts


def mask_matrix(allowed, L):
    """[n_items, L] bool: label y allowed on item i.  The masks are unsigned: bit 31 is a label like any other."""
    allowed = np.asarray(allowed, dtype=np.uint64)
    return ((allowed[:, None] >> np.arange(L, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def _forward_backward(X, T):
    """(log Z [m], node marginals [m, n, L], summed pairwise marginals [L, L]) of m instances of n items with the item
    scores X [m, n, L], which may hold -inf (every item with a finite entry)."""
    m, n, L = X.shape
    la, lb = np.zeros((m, n, L)), np.zeros((m, n, L))
    la[:, 0] = X[:, 0]
    for t in range(1, n):
        la[:, t] = _lse(la[:, t - 1, :, None] + T[None], axis=1) + X[:, t]
    for t in range(n - 2, -1, -1):
        lb[:, t] = _lse(T[None] + (X[:, t + 1] + lb[:, t + 1])[:, None, :], axis=2)
    logz = _lse(la[:, -1], axis=1)
    marg = np.exp(la + lb - logz[:, None, None])
    dT = np.zeros((L, L))
    for t in range(1, n):
        dT += np.exp(la[:, t - 1, :, None] + T[None] + (X[:, t] + lb[:, t])[:, None, :] - logz[:, None, None]).sum(axis=0)
    return logz, marg, dT


def instance_groups(seq_ptr, W, step):
    """[(n, starts)]: the instances by length, each group's first items ascending.  Windows: one group of length W; whole
    sequences (``W is None``): one group per distinct length."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    if W is not None:
        return [(int(W), window_starts(seq_ptr, W, step))]
    lengths = np.diff(seq_ptr)
    return [(int(n), seq_ptr[:-1][lengths == n]) for n in sorted(set(lengths.tolist()))]


def objective_partial(seq_ptr, item_ptr, attr_id, allowed, A, L, W, step, state_fid, trans_fid, w, details=False):
    """(f, g, number of instances) of the objective above; with ``details`` a fourth item, per instance group what
    ``partial_tolerances`` needs: n, the instance and item counts, sum and maximum of the magnitude bound M_w, and the
    group's expected counts of the free and of the restricted pass."""
    item_ptr, attr_id = np.asarray(item_ptr), np.asarray(attr_id)
    K = len(w)
    sfid, tfid, S, T = _tables(A, L, state_fid, trans_fid, w)
    n_items = len(item_ptr) - 1
    owner = np.repeat(np.arange(n_items), np.diff(item_ptr))
    score = np.zeros((n_items, L))
    np.add.at(score, owner, S[attr_id])
    ok = mask_matrix(allowed, L)
    if len(ok) != n_items or not ok.any(axis=1).all():
        raise ValueError("every item needs one mask with at least one allowed label")
    masked = np.where(ok, score, -np.inf)
    smag = np.abs(score).max(axis=1) if n_items else np.zeros(0)
    tmag = float(np.abs(T).max())
    f, g, count, groups = 0.0, np.zeros(K), 0, []
    for n, starts in instance_groups(seq_ptr, W, step):
        if len(starts) == 0:
            continue
        idx = starts[:, None] + np.arange(n)[None, :]
        expected = []
        logzs = []
        for X in (score[idx], masked[idx]):
            logz, marg, dT = _forward_backward(X, T)
            item = np.zeros((n_items, L))
            np.add.at(item, idx.ravel(), marg.reshape(-1, L))
            dS = np.zeros((A, L))
            np.add.at(dS, attr_id, item[owner])
            e = np.zeros(K)
            e[sfid[sfid >= 0]] += dS[sfid >= 0]
            e[tfid[tfid >= 0]] += dT[tfid >= 0]
            expected.append(e)
            logzs.append(logz)
        f += float(np.sum(logzs[0] - logzs[1]))
        g += expected[0] - expected[1]
        count += len(starts)
        Mw = smag[idx].sum(axis=1) + (n - 1) * tmag + n * np.log(float(L))
        groups.append({"n": n, "instances": len(starts), "items": len(np.unique(idx)) if W is None else n_items,
                       "M_sum": float(Mw.sum()), "M_max": float(Mw.max()), "expected_free": expected[0],
                       "expected_restricted": expected[1]})
    return (f, g, count, groups) if details else (f, g, count)


def partial_tolerances(L, groups):
    """Bounds (tol_f, tol_g [K]) on |f - f_ref| and |g - g_ref| between two fp64 evaluations of the partial objective,
    from ``objective_partial``'s details.  They are tests.train_objective_labels.objective_tolerances' bounds, taken once
    for the free and once for the restricted pass and added, per instance group (a group of one length n is a windowed
    problem with W = n; the groups' shares of f and g add, and so do their bounds, as in
    tests.train_objective_sequences.objective_sequences_tolerances):

    * f: an instance's row is log Z - log Z_A.  Either term is a log-space quantity bounded by the same M_w = sum_t max_y
      |s_t[y]| + (n - 1) max |t| + n ln L (the restricted lattice is a sub-lattice: its best path scores no more than the
      free one's and no less than -M_w), and where the labelled row subtracts the gold path's score of 2n - 1 terms the
      restricted pass has a second recursion of the same form, so each pass takes the labelled row's whole bound:
          tol_f = 2 * 2 eps sum_w (2n + 2 + log2 L + 2 log2(instances + 1)) M_w.
      An excluded term adds an exact 0 to a sum and no rounding.
    * g: the labelled bound's relative error of an expected count, eps (5n + 4M + log2 L + log2(items + 1)), M = max_w M_w,
      holds for either pass's count (a restricted marginal is the same exp of a sum of four bounded terms; one that is
      exactly 0 has no error).  The exact integer empirical count is replaced by 0: the second term of the labelled bound is
      instead the restricted pass's expected count under the same relative error.  A marginal below DBL_MIN may be flushed
      to 0 by either side, in either pass:
          tol_g = 2 eps (5n + 4M + log2 L + log2(items + 1)) (expected_free + expected_restricted)
                  + 2 (items + n instances) DBL_MIN.
    Both are the sum of the two sides' worst cases, as there."""
    tol_f, tol_g = 0.0, 0.0
    for gr in groups:
        n, m, items = gr["n"], gr["instances"], gr["items"]
        tol_f += 2 * 2 * EPS * (2 * n + 2 + np.log2(L) + 2 * np.log2(m + 1)) * gr["M_sum"]
        rel = 2 * EPS * (5 * n + 4 * gr["M_max"] + np.log2(L) + np.log2(items + 1))
        tol_g = tol_g + rel * (gr["expected_free"] + gr["expected_restricted"]) + 2 * (items + n * m) * TINY
    return tol_f, tol_g


# ---------------------------------------------------------------- seeded masks
def singleton_masks(labels):
    return (np.uint64(1) << np.asarray(labels, dtype=np.uint64)).astype(np.uint32)


def full_masks(n_items, L):
    return np.full(n_items, (1 << L) - 1, dtype=np.uint32)


def random_masks(rng, n_items, L):
    """Random non-empty subsets of the L labels, one per item: every label in with probability 1/2, and an empty draw
    given one label at random."""
    bits = rng.random((n_items, L)) < 0.5
    for i in np.flatnonzero(~bits.any(axis=1)):
        bits[i, int(rng.integers(0, L))] = True
    return (bits.astype(np.uint64) << np.arange(L, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def hide_labels(rng, labels, L, share=0.5):
    """Masks of a labelled set in which a seeded share of the items is hidden as {truth, one other label}; returns
    (masks, hidden [n_items] bool)."""
    labels = np.asarray(labels, dtype=np.int64)
    hidden = rng.random(len(labels)) < share
    other = (labels + rng.integers(1, L, size=len(labels))) % L
    masks = np.uint64(1) << labels.astype(np.uint64)
    masks = np.where(hidden, masks | (np.uint64(1) << other.astype(np.uint64)), masks)
    return masks.astype(np.uint32), hidden
