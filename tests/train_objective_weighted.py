"""The weighted, cost-augmented CRF training objective in numpy: the independent yardstick of the ``*_create_weighted``
trainers (tests/test_gpu_train_weighted.py), pinned on path enumeration by tests/test_train_objective_weighted.py.

    f(w) = sum over sequences q of omega(q) * sum over the instances of q of
               (log sum_y' exp(score(y') + sum_t C[y_t][y'_t]) - score(y))

It shares no code with the product.  It is the unweighted yardstick (tests/train_objective_labels.py) evaluated on an
*augmented* set: every item gets one extra attribute named by its gold label, attribute ``A + y`` carries the fixed
state weights ``C[y][.]`` on feature ids appended after the real ones, the set is evaluated sequence by sequence at
``w' = (w, C)``, every sequence's f and g are multiplied by its weight, and the first K gradient entries are kept.  The
gold path's score gains ``C[y][y] = 0`` per item, so the augmented f is the cost-augmented one.  Also here: that
module's error bounds restated for weights and costs."""
import numpy as np

from tests.train_objective_labels import EPS, TINY, _tables, objective, window_starts
from tests.train_objective_sequences import length_groups, subproblem


def label_count(problem):
    return np.asarray(problem[5]).size // int(problem[4])


def augmented(problem, C):
    """``(problem', w_tail)``: the problem with the gold-label attributes and their features (ids K .. K + L*L - 1,
    attribute ``A + y`` on label j: ``K + y * L + j``), and the weights ``C.ravel()`` to append to w."""
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K, *rest = problem
    L = label_count(problem)
    C = np.zeros((L, L)) if C is None else np.asarray(C, dtype=np.float64).reshape(L, L)
    item_ptr, attr_id, labels = np.asarray(item_ptr, dtype=np.int64), np.asarray(attr_id), np.asarray(labels)
    n = len(labels)
    new_attr, new_ptr = [], [0]
    for i in range(n):
        new_attr.extend(attr_id[item_ptr[i]:item_ptr[i + 1]].tolist())
        new_attr.append(A + int(labels[i]))
        new_ptr.append(len(new_attr))
    sfid2 = np.concatenate([np.asarray(sfid, dtype=np.int32).ravel(), (K + np.arange(L * L)).astype(np.int32)])
    return ((np.asarray(seq_ptr, dtype=np.int32), np.array(new_ptr, dtype=np.int32), np.array(new_attr, dtype=np.int32),
             labels.astype(np.int32), A + L, sfid2, np.asarray(tfid, dtype=np.int32).ravel(), K + L * L, *rest), C.ravel().copy())


def _per_sequence(problem, C, w):
    """Per sequence (f, g', details, n_instances) of the unweighted yardstick on the augmented set at (w, C); a windowed
    problem has 10 entries, one of whole sequences 8."""
    aug, tail = augmented(problem, C)
    seq_ptr, item_ptr, attr_id, labels, A2, sfid2, tfid, K2, *ws = aug
    L = label_count(problem)
    w2 = np.concatenate([np.asarray(w, dtype=np.float64), tail])
    out = []
    for s in range(len(seq_ptr) - 1):
        sub = subproblem(seq_ptr, item_ptr, attr_id, labels, [s])
        W, step = (int(ws[0]), int(ws[1])) if ws else (int(sub[0][1]), 1)
        f, g, nw, d = objective(*sub, A2, L, W, step, sfid2, tfid, w2, details=True)
        out.append((f, g, d, nw))
    return out


def objective_weighted(problem, weights, C, w):
    """(f, g [K], number of instances) of the weighted cost-augmented objective.  ``weights``: one per sequence, or None
    (all 1); ``C``: [L, L] with row = gold, or None (no costs)."""
    K = len(w)
    n_seqs = len(problem[0]) - 1
    weights = np.ones(n_seqs) if weights is None else np.asarray(weights, dtype=np.float64)
    f, g, n = 0.0, np.zeros(K), 0
    for omega, (fs, gs, _, nw) in zip(weights, _per_sequence(problem, C, w)):
        f += omega * fs
        g += omega * gs[:K]
        n += nw
    return f, g, n


def _group_bound(aug, members, weights, L, W, step, w2, K, expected, empirical):
    """tests.train_objective_labels.objective_tolerances restated for the instances of the sequences `members` of the
    augmented set: the score magnitudes are those of the augmented scores s_t[y'] + C[y_t][y'] (at most max C above the
    plain ones), a window's row is scaled by its sequence's weight (one more rounding: 2W + 3 terms where that bound has
    2W + 2), and so is every marginal (5W + 1 where it has 5W); `expected` / `empirical` are the weighted counts (the
    rounding of the empirical sum itself is added by the caller, over the whole problem)."""
    seq_ptr, item_ptr, attr_id, labels = subproblem(aug[0], aug[1], aug[2], aug[3], members)
    n = int(seq_ptr[-1])
    _, _, S, T = _tables(aug[4], L, aug[5], aug[6], w2)
    score = np.zeros((n, L))
    np.add.at(score, np.repeat(np.arange(n), np.diff(item_ptr)), S[attr_id])
    smag = np.abs(score).max(axis=1) if n else np.zeros(0)
    starts = window_starts(seq_ptr, W, step)
    omega = np.concatenate([np.full(len(np.arange(seq_ptr[k], seq_ptr[k + 1] - W + 1, step)), weights[s])
                            for k, s in enumerate(members)] + [np.zeros(0)])
    csum = np.concatenate([[0.0], np.cumsum(smag)])
    Mw = csum[starts + W] - csum[starts] + (W - 1) * float(np.abs(T).max()) + W * np.log(float(L))
    nw = len(starts)
    tol_f = 2 * EPS * (2 * W + 3 + np.log2(L) + 2 * np.log2(nw + 1)) * float((omega * Mw).sum())
    M = float(Mw.max()) if nw else 0.0
    tol_g = (2 * EPS * ((5 * W + 1 + 4 * M + np.log2(L) + np.log2(n + 1)) * expected + empirical)
             + (n + W * nw) * TINY * max(1.0, float(omega.max()) if nw else 1.0))
    return tol_f, tol_g[:K]


def weighted_tolerances(problem, weights, C, w):
    """Bounds (tol_f, tol_g [K]) on |f - f_ref| and |g - g_ref| between two fp64 evaluations of the weighted
    cost-augmented objective.  Windows: one group, every sequence.  Whole sequences: one group per length, the bounds
    added (tests.train_objective_sequences.objective_sequences_tolerances).

    The empirical count is an exact integer in those bounds; here it is a sum of weights that either side rounds as it
    adds them: one side adds a feature's occurrences one by one (at most N = max(instances * longest instance, attribute
    entries) terms: an error of at most (N - 1) eps of the sum), the other one product per sequence (S terms, each
    rounded once more): (N + S) eps of the weighted empirical count is added."""
    K = len(w)
    n_seqs = len(problem[0]) - 1
    weights = np.ones(n_seqs) if weights is None else np.asarray(weights, dtype=np.float64)
    aug, tail = augmented(problem, C)
    L = label_count(problem)
    w2 = np.concatenate([np.asarray(w, dtype=np.float64), tail])
    per = _per_sequence(problem, C, w)
    windowed = len(problem) == 10
    groups = {int(problem[8]): list(range(n_seqs))} if windowed else length_groups(problem[0])
    tol_f, tol_g = 0.0, np.zeros(K)
    for W, members in groups.items():
        expected = sum(weights[s] * per[s][2]["expected"] for s in members)
        empirical = sum(weights[s] * per[s][2]["empirical"] for s in members)
        tf, tg = _group_bound(aug, members, weights, L, W, int(problem[9]) if windowed else 1, w2, K, expected, empirical)
        tol_f += tf
        tol_g += tg
    instances = sum(p[3] for p in per)
    terms = max(instances * max(groups), len(aug[2])) + n_seqs
    tol_g += EPS * terms * sum(weights[s] * per[s][2]["empirical"] for s in range(n_seqs))[:K]
    return tol_f, tol_g
