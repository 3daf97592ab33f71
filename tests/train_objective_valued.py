"""A linear-chain CRF over items whose attributes carry real values (CRFsuite's name:value items), in numpy and log space:
the independent yardstick of the ``*_valued`` entries (tests/test_gpu_train_valued.py, tests/test_gpu_sequence_valued.py),
pinned on path enumeration and on the unvalued yardstick by tests/test_train_valued_host.py.  It shares no code with the
product, and none with tests/train_objective_labels.py (which pins it through the duplication identity).

    state score   s_t[y] = sum over the item's entries of v * w[a][y]          (CSR order)
    objective     f = sum over instances of (log Z - score(gold)),  instances = sliding windows, or whole sequences
    gradient      state (a, y): sum over instances and entries of a of v * P(y_t = y)  -  sum of v * [y_t = y]
                  transition (i, j): expected minus observed count, as without values

Also here: whole-sequence marginals with log Z, CRFsuite's sequential Viterbi, GECCO's windowed maxima (one label, every
label, any label but a background), and the error bounds between two fp64 evaluations of the objective."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
TINY = float(np.finfo(np.float64).tiny)


def lse(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def dense_tables(A, L, state_fid, trans_fid, w):
    """(sfid [A, L], tfid [L, L], S [A, L], T [L, L]): the weights of `w` in their dense slots, 0 where there is no feature."""
    w = np.asarray(w, dtype=np.float64)
    sfid, tfid = np.asarray(state_fid).reshape(A, L), np.asarray(trans_fid).reshape(L, L)
    pick = lambda fid: np.where(fid >= 0, w[np.maximum(fid, 0)], 0.0) if len(w) else np.zeros(fid.shape)
    return sfid, tfid, pick(sfid), pick(tfid)


def item_scores(item_ptr, attr_id, values, S):
    """[n, L]: every entry's value x weight row, added entry by entry in CSR order (np.add.at is unbuffered and in index
    order); ids outside S's rows carry no weight."""
    item_ptr, attr_id = np.asarray(item_ptr, dtype=np.int64), np.asarray(attr_id, dtype=np.int64)
    values = np.asarray(values, dtype=np.float64)
    n, A = len(item_ptr) - 1, S.shape[0]
    owner = np.repeat(np.arange(n), np.diff(item_ptr))
    known = (attr_id >= 0) & (attr_id < A)
    score = np.zeros((n, S.shape[1]))
    np.add.at(score, owner[known], values[known, None] * S[attr_id[known]])
    return score


def forward_backward(X, T):
    """Instances of one length side by side: X [m, n, L] state scores, T [L, L].  Returns (log alpha, log beta, log Z [m])."""
    m, n, L = X.shape
    la, lb = np.zeros((m, n, L)), np.zeros((m, n, L))
    la[:, 0] = X[:, 0]
    for t in range(1, n):
        la[:, t] = lse(la[:, t - 1, :, None] + T[None], axis=1) + X[:, t]
    for t in range(n - 2, -1, -1):
        lb[:, t] = lse(T[None] + (X[:, t + 1] + lb[:, t + 1])[:, None, :], axis=2)
    return la, lb, lse(la[:, -1], axis=1)


def _instances(score, labels, T, idx):
    """The instances whose items are the rows of idx [m, n]: (sum of log Z - gold, node marginals [m, n, L], expected
    transition counts [L, L], per-instance (logz, gold))."""
    X, Y = score[idx], labels[idx]
    m, n = idx.shape
    la, lb, logz = forward_backward(X, T)
    gold = X[np.arange(m)[:, None], np.arange(n)[None], Y].sum(axis=1) + T[Y[:, :-1], Y[:, 1:]].sum(axis=1)
    marg = np.exp(la + lb - logz[:, None, None])
    dT = np.zeros_like(T)
    for t in range(1, n):
        dT += np.exp(la[:, t - 1, :, None] + T[None] + (X[:, t] + lb[:, t])[:, None, :] - logz[:, None, None]).sum(axis=0)
    return float(np.sum(logz - gold)), marg, dT, logz, gold


def _objective(instance_groups, item_ptr, attr_id, labels, A, L, state_fid, trans_fid, w, values):
    """f, g and details over instance groups (each an index array [m, n] of instances of n items)."""
    item_ptr, attr_id = np.asarray(item_ptr, dtype=np.int64), np.asarray(attr_id, dtype=np.int64)
    labels, values = np.asarray(labels, dtype=np.int64), np.asarray(values, dtype=np.float64)
    K = len(w)
    sfid, tfid, S, T = dense_tables(A, L, state_fid, trans_fid, w)
    n = len(labels)
    owner = np.repeat(np.arange(n), np.diff(item_ptr))
    score = item_scores(item_ptr, attr_id, values, S)
    f, n_inst = 0.0, 0
    item, cover = np.zeros((n, L)), np.zeros(n)
    dT, eT = np.zeros((L, L)), np.zeros((L, L))
    logz_all, gold_all = [], []
    for idx in instance_groups:
        if idx.shape[0] == 0:
            continue
        fi, marg, dTi, logz, gold = _instances(score, labels, T, idx)
        f += fi
        n_inst += idx.shape[0]
        np.add.at(item, idx.ravel(), marg.reshape(-1, L))
        np.add.at(cover, idx.ravel(), 1.0)
        dT += dTi
        Y = labels[idx]
        np.add.at(eT, (Y[:, :-1].ravel(), Y[:, 1:].ravel()), 1.0)
        logz_all.append(logz)
        gold_all.append(gold)
    dS, eS = np.zeros((A, L)), np.zeros((A, L))
    np.add.at(dS, attr_id, values[:, None] * item[owner])
    np.add.at(eS, (attr_id, labels[owner]), values * cover[owner])
    expected, empirical = np.zeros(K), np.zeros(K)
    m = sfid >= 0
    expected[sfid[m]] += dS[m]
    empirical[sfid[m]] += eS[m]
    m = tfid >= 0
    expected[tfid[m]] += dT[m]
    empirical[tfid[m]] += eT[m]
    # what the error bound of a state feature's sums needs: the sums of |v| x marginal and of |v| x coverage
    aS, bS = np.zeros((A, L)), np.zeros((A, L))
    np.add.at(aS, attr_id, np.abs(values)[:, None] * item[owner])
    np.add.at(bS, (attr_id, labels[owner]), np.abs(values) * cover[owner])
    abs_expected, abs_empirical = expected.copy(), empirical.copy()
    m = sfid >= 0
    abs_expected[sfid[m]] = aS[m]
    abs_empirical[sfid[m]] = bS[m]
    details = {"logz": np.concatenate(logz_all + [np.zeros(0)]), "gold": np.concatenate(gold_all + [np.zeros(0)]),
               "expected": expected, "empirical": empirical, "abs_expected": abs_expected, "abs_empirical": abs_empirical,
               "score": score, "T": T}
    return f, expected - empirical, n_inst, details


def window_index(seq_ptr, W, step):
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    starts = [np.arange(seq_ptr[s], seq_ptr[s + 1] - W + 1, step) for s in range(len(seq_ptr) - 1)]
    starts = np.concatenate(starts + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return starts[:, None] + np.arange(W)[None, :]


def objective(seq_ptr, item_ptr, attr_id, labels, A, L, W, step, state_fid, trans_fid, w, values, details=False):
    """The windowed objective with values: (f, g, number of windows), and with ``details`` a fourth item."""
    out = _objective([window_index(seq_ptr, W, step)], item_ptr, attr_id, labels, A, L, state_fid, trans_fid, w, values)
    return out if details else out[:3]


def sequence_index_groups(seq_ptr):
    """Per length, the index array [m, n] of the sequences of that length (ascending)."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    by_len = {}
    for s in range(len(seq_ptr) - 1):
        by_len.setdefault(int(seq_ptr[s + 1] - seq_ptr[s]), []).append(int(seq_ptr[s]))
    return {n: np.array(b, dtype=np.int64)[:, None] + np.arange(n)[None, :] for n, b in sorted(by_len.items())}


def objective_sequences(seq_ptr, item_ptr, attr_id, labels, A, L, state_fid, trans_fid, w, values, details=False):
    """The whole-sequence objective with values: (f, g, number of sequences).  Every sequence holds at least one item."""
    out = _objective(list(sequence_index_groups(seq_ptr).values()), item_ptr, attr_id, labels, A, L, state_fid, trans_fid, w,
                     values)
    return out if details else out[:3]


# ---------------------------------------------------------------- error bounds between two fp64 evaluations
def _tolerances(groups, n_items, L, details):
    """tests/train_objective_labels.py's objective_tolerances restated for valued item scores, per group of instances of one
    length W (the bounds of the groups add).  The derivation there holds with s_t[y] = sum of v w in place of the sum of
    w: M_w = sum_t max_y |s_t[y]| + (W - 1) max|t| + W ln L bounds every log-space quantity of an instance,
        tol_f = 2 eps sum_w (2W + 2 + log2 L + 2 log2(n_instances + 1)) M_w.
    Two things are new.  The item scores themselves: an item score of d entries is a sum of d rounded products, off by at
    most (d + 1) eps sum |v w| <= (d + 1) eps times a bound B_t on sum_a |v||w|; both evaluations carry that error into
    log Z and gold (each 1-Lipschitz in the scores), so f gains 2 * 2 eps sum over instances and positions of (d_t + 1) B_t.
    (Without values the same term exists and is covered there by the margin of M_w; with |v| = 2^10 next to cancelling
    signs it is not.)  And a state feature's expected count is a sum of v x marginal whose terms may cancel: the relative
    bound applies to sum |v| x marginal (abs_expected), and the empirical count, no longer an exact integer, is a sum of
    up to n_items rounded products: (log2(n_items + 1) + 2) eps sum |v| x coverage (abs_empirical) on each side.
        tol_g = 2 eps ((5W + 4M + log2 L + log2(n_items + 1)) abs_expected + (log2(n_items + 1) + 2) abs_empirical)
                + (n_items + W n_instances) DBL_MIN,
    with M = max_w M_w enlarged by the item-score term above (a marginal is the exponential of such quantities)."""
    score, T = details["score"], details["T"]
    smag = np.abs(score).max(axis=1) if n_items else np.zeros(0)
    tmax = float(np.abs(T).max())
    slack = details["score_slack"]  # per item: (d + 1) B_t, in units of eps
    tol_f, M, total = 0.0, 0.0, 0
    for W, idx in groups:
        if idx.shape[0] == 0:
            continue
        Mw = smag[idx].sum(axis=1) + (W - 1) * tmax + W * np.log(float(L))
        nw = idx.shape[0]
        tol_f += 2 * EPS * (2 * W + 2 + np.log2(L) + 2 * np.log2(nw + 1)) * float(Mw.sum()) + 4 * EPS * float(slack[idx].sum())
        M = max(M, float(Mw.max()) + 2 * EPS * float(slack[idx].sum(axis=1).max()))
        total += W * nw
    Wmax = max([W for W, idx in groups if idx.shape[0]] + [1])
    lg = np.log2(n_items + 1)
    tol_g = (2 * EPS * ((5 * Wmax + 4 * M + np.log2(L) + lg) * details["abs_expected"] + (lg + 2) * details["abs_empirical"])
             + (n_items + total) * TINY)
    return tol_f, tol_g


def _score_slack(item_ptr, attr_id, values, S):
    item_ptr, attr_id = np.asarray(item_ptr, dtype=np.int64), np.asarray(attr_id, dtype=np.int64)
    n = len(item_ptr) - 1
    deg = np.diff(item_ptr)
    owner = np.repeat(np.arange(n), deg)
    B = np.zeros(n)
    np.add.at(B, owner, np.abs(np.asarray(values, dtype=np.float64)) * np.abs(S[attr_id]).max(axis=1))
    return (deg + 1) * B


def objective_tolerances(seq_ptr, item_ptr, attr_id, labels, A, L, W, step, state_fid, trans_fid, w, values):
    """(tol_f, tol_g [K]) for the windowed objective."""
    _, _, _, d = objective(seq_ptr, item_ptr, attr_id, labels, A, L, W, step, state_fid, trans_fid, w, values, details=True)
    d["score_slack"] = _score_slack(item_ptr, attr_id, values, dense_tables(A, L, state_fid, trans_fid, w)[2])
    return _tolerances([(W, window_index(seq_ptr, W, step))], int(np.asarray(seq_ptr)[-1]), L, d)


def objective_sequences_tolerances(seq_ptr, item_ptr, attr_id, labels, A, L, state_fid, trans_fid, w, values):
    """(tol_f, tol_g [K]) for the whole-sequence objective: the sequences of one length are one group."""
    _, _, _, d = objective_sequences(seq_ptr, item_ptr, attr_id, labels, A, L, state_fid, trans_fid, w, values, details=True)
    d["score_slack"] = _score_slack(item_ptr, attr_id, values, dense_tables(A, L, state_fid, trans_fid, w)[2])
    return _tolerances(list(sequence_index_groups(seq_ptr).items()), int(np.asarray(seq_ptr)[-1]), L, d)


# ---------------------------------------------------------------- inference
def marginals_sequences(seq_ptr, item_ptr, attr_id, values, S, T):
    """Whole-sequence marginals [n, L] and log Z per sequence (0 for a sequence without items).  Log space with every
    forward and backward vector shifted by its own log-sum-exp (the shifts add up to log Z), so that a long sequence's
    vectors stay of order 1 and an item's marginal, softmax(log alpha + log beta), is rounded at that size: the plain
    recursion carries log alpha of the size of log Z, whose ulp at 300 items is of the order of the 1e-12 the device is
    held to."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    score = item_scores(item_ptr, attr_id, values, S)
    marg, logz = np.zeros_like(score), np.zeros(len(seq_ptr) - 1)
    for s in range(len(seq_ptr) - 1):
        b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        if e == b:
            continue
        X, n = score[b:e], e - b
        la, lb = np.zeros_like(X), np.zeros_like(X)
        la[0] = X[0]
        total = lse(la[0], 0)
        la[0] -= total
        for t in range(1, n):
            la[t] = lse(la[t - 1][:, None] + T, axis=0) + X[t]
            shift = lse(la[t], 0)
            la[t] -= shift
            total += shift
        for t in range(n - 2, -1, -1):
            lb[t] = lse(T + (X[t + 1] + lb[t + 1])[None, :], axis=1)
            lb[t] -= lse(lb[t], 0)
        q = la + lb
        marg[b:e] = np.exp(q - lse(q, axis=1)[:, None])
        logz[s] = total
    return marg, logz


def viterbi_scores(score, T):
    """CRFsuite's recursion ([EXT] crf1dc_viterbi) over one sequence of state scores [n, L]: the maximum over the source
    label in index order with a strict `<` update, the first arg max at the end.  Returns (labels, score)."""
    n, L = score.shape
    back = np.zeros((n, L), dtype=np.int64)
    d = score[0].copy()
    for t in range(1, n):
        nd = np.empty(L)
        for j in range(L):
            best, arg = -np.inf, 0
            for i in range(L):
                c = d[i] + T[i, j]
                if best < c:
                    best, arg = c, i
            back[t, j] = arg
            nd[j] = best + score[t, j]
        d = nd
    y = np.zeros(n, dtype=np.int64)
    best, arg = -np.inf, 0
    for j in range(L):
        if best < d[j]:
            best, arg = d[j], j
    y[-1] = arg
    for t in range(n - 1, 0, -1):
        y[t - 1] = back[t, y[t]]
    return y, float(best)


def viterbi(seq_ptr, item_ptr, attr_id, values, S, T):
    """Labels [n] and path score per sequence (0 for a sequence without items)."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    score = item_scores(item_ptr, attr_id, values, S)
    y, sc = np.zeros(len(score), dtype=np.int64), np.zeros(len(seq_ptr) - 1)
    for s in range(len(seq_ptr) - 1):
        b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        if e > b:
            y[b:e], sc[s] = viterbi_scores(score[b:e], T)
    return y, sc


def path_score(score, T, y):
    """The score of the path y through one sequence, added in CRFsuite's order (state, then transition and state)."""
    s = score[0, y[0]]
    for t in range(1, len(y)):
        s = (s + T[y[t - 1], y[t]]) + score[t, y[t]]
    return float(s)


def windowed(seq_ptr, item_ptr, attr_id, values, S, T, W, step, background=None, pad=True):
    """GECCO's windowed probabilities: p_all [n, L], per item and label the maximum over the windows covering the item
    (W items, `step` apart from the sequence's first) of the label's marginal inside the window, and p_any [n], the
    maximum over the same windows of the sum of the marginals of every label but `background` (label-index order), or
    None.  A sequence shorter than W is padded to W with empty items, (W - n) // 2 of them in front (``pad``), or holds
    NaN everywhere; an item no window covers holds 0.0.  One label's windowed probability is its column."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    score = item_scores(item_ptr, attr_id, values, S)
    n, L = score.shape
    p_all = np.zeros((n, L))
    p_any = None if background is None else np.zeros(n)
    others = [l for l in range(L) if l != background]
    for s in range(len(seq_ptr) - 1):
        b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        m = e - b
        if m == 0:
            continue
        if m < W and not pad:
            p_all[b:e] = np.nan
            if p_any is not None:
                p_any[b:e] = np.nan
            continue
        front = (W - m) // 2 if m < W else 0
        X = np.zeros((max(m, W), L))
        X[front:front + m] = score[b:e]
        starts = np.arange(0, len(X) - W + 1, step)
        idx = starts[:, None] + np.arange(W)[None, :]
        la, lb, lz = forward_backward(X[idx], T)
        marg = np.exp(la + lb - lz[:, None, None])
        full = np.zeros((len(X), L))
        np.maximum.at(full, idx.ravel(), marg.reshape(-1, L))
        p_all[b:e] = full[front:front + m]
        if p_any is not None:
            tot = np.zeros(marg.shape[:2])
            for l in others:
                tot = tot + marg[:, :, l]
            anyp = np.zeros(len(X))
            np.maximum.at(anyp, idx.ravel(), tot.ravel())
            p_any[b:e] = anyp[front:front + m]
    return p_all, p_any


# ---------------------------------------------------------------- seeded problems
def mixed_values(rng, n):
    """One value per entry from the mix the valued tests use: N(0, 1), exact 0, exact 1, +-2^10 and 2^-10."""
    kind = rng.integers(0, 8, size=n)
    v = rng.normal(0.0, 1.0, size=n)
    v[kind == 3] = 0.0
    v[kind == 4] = 1.0
    v[kind == 5] = 1024.0
    v[kind == 6] = -1024.0
    v[kind == 7] = 2.0 ** -10
    return v
