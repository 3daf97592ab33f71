"""The weighted cost-augmented yardstick (tests/train_objective_weighted.py) against path enumeration: every label path of
every instance is scored on its own, cost included, and f and g are formed from those sums directly."""
import itertools

import numpy as np
import pytest

from tests.train_objective_labels import training_set
from tests.train_objective_sequences import sequences_problem
from tests.train_objective_weighted import label_count, objective_weighted, weighted_tolerances


def _enumerated(problem, weights, C, w):
    """f and g by enumeration: per instance every path y' with score(y') + sum_t C[y_t][y'_t], its feature counts, and the
    gold path's."""
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K, *ws = problem
    L = label_count(problem)
    sfid, tfid = np.asarray(sfid).reshape(A, L), np.asarray(tfid).reshape(L, L)
    f, g = 0.0, np.zeros(K)

    def path(i0, ys):
        score, counts = 0.0, np.zeros(K)
        for t, y in enumerate(ys):
            for a in attr_id[item_ptr[i0 + t]:item_ptr[i0 + t + 1]]:
                if sfid[a, y] >= 0:
                    score += w[sfid[a, y]]
                    counts[sfid[a, y]] += 1
            if t and tfid[ys[t - 1], y] >= 0:
                score += w[tfid[ys[t - 1], y]]
                counts[tfid[ys[t - 1], y]] += 1
        return score, counts

    for s in range(len(seq_ptr) - 1):
        b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        starts = range(b, e - ws[0] + 1, ws[1]) if ws else [b]
        n = ws[0] if ws else e - b
        for i0 in starts:
            gold = [int(y) for y in labels[i0:i0 + n]]
            gold_score, gold_counts = path(i0, gold)
            terms, counts = [], []
            for ys in itertools.product(range(L), repeat=n):
                sc, cn = path(i0, ys)
                terms.append(sc + sum(C[y, yp] for y, yp in zip(gold, ys)))
                counts.append(cn)
            terms = np.array(terms)
            m = terms.max()
            p = np.exp(terms - m)
            f += weights[s] * (m + np.log(p.sum()) - gold_score)
            g += weights[s] * ((p[:, None] * np.array(counts)).sum(axis=0) / p.sum() - gold_counts)
    return f, g


def _costs(rng, L):
    C = rng.uniform(0.0, 2.0, size=(L, L))
    C[np.arange(L), np.arange(L)] = 0.0
    assert np.abs(C - C.T).max() > 0.1  # (asymmetric: a transposed table fails)
    return C


def _weights(rng, n):
    wts = rng.uniform(0.25, 4.0, size=n)
    wts[n // 2] = 0.0
    assert len(set(wts.tolist())) == n
    return wts


@pytest.mark.parametrize("W,step", [(1, 1), (2, 1), (4, 2), (5, 3)])
@pytest.mark.parametrize("L", [2, 3])
def test_windows_match_enumeration(L, W, step):
    rng = np.random.default_rng(100 * L + 10 * W + step)
    p = training_set(rng, L, W, step, A=7, n_seqs=4, fixed=1, max_extra=5)
    C, wts = _costs(rng, L), _weights(rng, len(p[0]) - 1)
    w = rng.normal(0, 1.5, size=p[7])
    f, g, n = objective_weighted(p, wts, C, w)
    ef, eg = _enumerated(p, wts, C, w)
    assert n > 0 and abs(f - ef) <= 1e-12 * abs(ef) and np.abs(g - eg).max() <= 1e-12 * (1 + np.abs(eg).max())
    # the transposed table is another objective, and so is the unweighted one
    ft, gt, _ = objective_weighted(p, wts, C.T, w)
    assert abs(ft - ef) > 1e-6 * abs(ef)
    fu, _, _ = objective_weighted(p, None, C, w)
    assert abs(fu - ef) > 1e-6 * abs(ef)
    tol_f, tol_g = weighted_tolerances(p, wts, C, w)
    assert abs(f - ef) <= tol_f and np.all(np.abs(g - eg) <= tol_g) and tol_f < 1e-10 * abs(ef)


@pytest.mark.parametrize("L", [2, 3])
def test_whole_sequences_match_enumeration(L):
    rng = np.random.default_rng(7 + L)
    p = sequences_problem(rng, L, [3, 1, 5, 2, 4, 1], A=6, stay=0.6)
    C, wts = _costs(rng, L), _weights(rng, 6)
    w = rng.normal(0, 1.5, size=p[7])
    f, g, n = objective_weighted(p, wts, C, w)
    ef, eg = _enumerated(p, wts, C, w)
    assert n == 6 and abs(f - ef) <= 1e-12 * abs(ef) and np.abs(g - eg).max() <= 1e-12 * (1 + np.abs(eg).max())
    ft, _, _ = objective_weighted(p, wts, C.T, w)
    assert abs(ft - ef) > 1e-6 * abs(ef)
    tol_f, tol_g = weighted_tolerances(p, wts, C, w)
    assert abs(f - ef) <= tol_f and np.all(np.abs(g - eg) <= tol_g)


def test_no_weights_and_no_costs_is_the_unweighted_yardstick():
    from tests.train_objective_labels import objective

    rng = np.random.default_rng(3)
    p = training_set(rng, 3, 4, 2, A=9, n_seqs=5)
    w = rng.normal(0, 1.5, size=p[7])
    f, g, n = objective_weighted(p, None, None, w)
    ef, eg, en = objective(*p[:5], 3, 4, 2, p[5], p[6], w)
    assert n == en and abs(f - ef) <= 1e-12 * abs(ef) and np.abs(g - eg).max() <= 1e-11
