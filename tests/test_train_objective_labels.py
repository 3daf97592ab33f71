"""The many-label yardstick of the device objective (tests/train_objective_labels.py) against the definition: all L^W
label paths of every window in 50-digit arithmetic, as tests/test_train_host.py pins the 2-label yardstick."""
import itertools

import numpy as np
import pytest

from tests.train_objective_labels import objective

# (L, W, step, weight scale)
CASES = [(3, 5, 1, 1.5), (3, 7, 2, 1.5), (4, 5, 1, 1.5), (9, 3, 1, 1.5), (5, 4, 1, 150.0), (3, 6, 1, 1500.0), (2, 8, 1, 1.5)]


def _problem(L, W, step, sigma):
    rng = np.random.default_rng(1000 * L + 10 * W + step)
    A = 12
    lengths = [int(x) for x in rng.integers(W, W + 6, size=3)]
    seq_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(seq_ptr[-1])
    labels = rng.integers(0, L, size=n).astype(np.int32)
    items = [sorted(set(rng.integers(0, A, size=int(rng.integers(0, 4))).tolist())) for _ in range(n)]
    item_ptr = np.concatenate([[0], np.cumsum([len(it) for it in items])]).astype(np.int32)
    attr_id = np.array([a for it in items for a in it], dtype=np.int32)
    fid = np.arange(A * L + L * L, dtype=np.int32)
    fid[[3, A * L + 1]] = -1  # a state and a transition pair without a feature
    keep = fid >= 0
    fid[keep] = np.arange(int(keep.sum()))
    w = rng.normal(0, sigma, size=int(keep.sum()))
    return seq_ptr, item_ptr, attr_id, labels, A, fid[:A * L], fid[A * L:], w


def _mp_objective(seq_ptr, item_ptr, attr_id, labels, A, L, W, step, sfid, tfid, w):
    """f and g [K] by enumerating all L^W label paths of every window in 50-digit arithmetic: no recursion, no
    log-sum-exp.  The path probabilities are gathered per (position, label) and (position, label, label) and then
    handed to the features."""
    import mpmath

    with mpmath.workdps(50):
        K = len(w)
        wm = [mpmath.mpf(float(x)) for x in w]
        zero = mpmath.mpf(0)
        sfid, tfid = np.asarray(sfid).reshape(A, L), np.asarray(tfid).reshape(L, L)
        n = int(seq_ptr[-1])
        feats = [[[int(sfid[a, y]) for a in attr_id[item_ptr[i]:item_ptr[i + 1]] if sfid[a, y] >= 0] for y in range(L)]
                 for i in range(n)]
        score = [[mpmath.fsum(wm[k] for k in feats[i][y]) for y in range(L)] for i in range(n)]
        tw = [[wm[tfid[i, j]] if tfid[i, j] >= 0 else zero for j in range(L)] for i in range(L)]
        paths = list(itertools.product(range(L), repeat=W))
        f = zero
        g = [zero] * K
        n_win = 0
        for s in range(len(seq_ptr) - 1):
            for i0 in range(int(seq_ptr[s]), int(seq_ptr[s + 1]) - W + 1, step):
                n_win += 1
                sc = [mpmath.fsum([score[i0 + t][y[t]] for t in range(W)] + [tw[y[t - 1]][y[t]] for t in range(1, W)])
                      for y in paths]
                top = max(sc)
                ex = [mpmath.exp(v - top) for v in sc]
                z = mpmath.fsum(ex)
                gold = tuple(int(v) for v in labels[i0:i0 + W])
                f += top + mpmath.log(z) - sc[paths.index(gold)]
                node = [[zero] * L for _ in range(W)]
                pair = [[[zero] * L for _ in range(L)] for _ in range(W)]
                for y, e in zip(paths, ex):
                    p = e / z - (1 if y == gold else 0)  # expected - empirical
                    for t in range(W):
                        node[t][y[t]] += p
                        if t > 0:
                            pair[t][y[t - 1]][y[t]] += p
                for t in range(W):
                    for y in range(L):
                        for k in feats[i0 + t][y]:
                            g[k] += node[t][y]
                        if t > 0:
                            for yp in range(L):
                                if tfid[yp, y] >= 0:
                                    g[tfid[yp, y]] += pair[t][yp][y]
        return float(f), np.array([float(v) for v in g]), n_win


@pytest.mark.parametrize("L,W,step,sigma", CASES)
def test_yardstick_matches_path_enumeration(L, W, step, sigma):
    """f to 1e-14 relative and g to 1e-11 (1 + |g|): about five times the worst differences seen between the yardstick
    and the enumeration on these cases (1.4e-16 and 1.9e-12, the latter at sigma = 1500)."""
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, w = _problem(L, W, step, sigma)
    f, g, nw = objective(seq_ptr, item_ptr, attr_id, labels, A, L, W, step, sfid, tfid, w)
    mf, mg, mnw = _mp_objective(seq_ptr, item_ptr, attr_id, labels, A, L, W, step, sfid, tfid, w)
    assert nw == mnw > 0
    print(f"L={L} W={W} sigma={sigma}: |f - mp| / |mp| = {abs(f - mf) / abs(mf):.3g}, "
          f"max |g - mp| / (1 + |g|) = {(np.abs(g - mg) / (1 + np.abs(mg))).max():.3g}")
    assert abs(f - mf) <= 1e-14 * abs(mf), (f, mf)
    assert np.all(np.abs(g - mg) <= 1e-11 * (1 + np.abs(mg))), np.abs(g - mg).max()


def test_yardstick_matches_the_two_label_yardstick():
    from benchkit.train_objective import objective as objective2

    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, w = _problem(2, 8, 1, 1.5)
    f, g, nw = objective(seq_ptr, item_ptr, attr_id, labels, A, 2, 8, 1, sfid, tfid, w)
    f2, g2, nw2 = objective2(seq_ptr, item_ptr, attr_id, labels, A, 8, 1, sfid, tfid, w)
    assert nw == nw2
    assert abs(f - f2) <= 1e-13 * (1 + abs(f2))
    assert np.all(np.abs(g - g2) <= 1e-13 * (1 + np.abs(g2)))
