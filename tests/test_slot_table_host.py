"""CPU: the per-attribute factor table behind the W = 20 window kernels' slot constants (gecco_crf_model_slot_table) and the
bound that lets the Viterbi margin absorb score differences summed attribute by attribute.

The table holds (delta_a, exp(delta_a)), not (delta_a, expm1(delta_a)): 1 + fl(expm1(delta)) carries an absolute error of
half an ulp of 1, which is a relative error of 2^-53 exp(-delta) in the factor -- 3e-8 at delta = -20 -- and a gene with a
strongly negative and a compensating positive attribute keeps all of it.  The same one-ulp bound is asked of exp."""
import numpy as np

from gecco_amd import _native as nat


def _ulp_distance(a, b):
    ia, ib = np.asarray(a).view(np.int64), np.asarray(b).view(np.int64)
    return np.abs(ia - ib)


def test_table_against_numpy():
    rng = np.random.default_rng(2024)
    A = 5000
    w = rng.laplace(-0.4, 1.7, size=(A, 2))
    w[:50] = rng.integers(-30, 31, size=(50, 2))           # integer weights: exact differences
    w[50:60, 1] = w[50:60, 0] + rng.uniform(-700, 700, 10)  # the far ends of the range
    w[60] = (3.25, 3.25)                                     # delta = 0
    trans = rng.normal(size=(2, 2))
    m = nat.Model.from_tables(w, trans)
    for label in (0, 1):
        pairs, dmax, cnt = m.slot_table(label)
        assert pairs.shape == (A + 1, 2)
        delta = w[:, label] - w[:, 1 - label]
        assert np.array_equal(pairs[:A, 0], delta)  # one IEEE subtraction, exact for the integer rows
        want = np.exp(delta)
        print("largest distance to numpy.exp in ulps:", int(_ulp_distance(pairs[:A, 1], want).max()))
        assert _ulp_distance(pairs[:A, 1], want).max() <= 1
        assert pairs[60, 1] == 1.0
        # the neutral entry that attribute ids outside the dictionary are clamped to: leaves sum and product unchanged
        assert pairs[A, 0] == 0.0 and pairs[A, 1] == 1.0 and not np.signbit(pairs[A, 0])
        assert dmax == np.abs(delta).max()
        assert cnt == (0 if dmax >= 700 else int(np.floor(700.0 / dmax)))
    # the other label's table is the mirror image
    p1, p0 = m.slot_table(1)[0], m.slot_table(0)[0]
    assert np.array_equal(p1[:A, 0], -p0[:A, 0])


def test_prod_max_cnt_rule():
    f = nat.load_library().gecco_crf_slot_prod_max_cnt
    assert f(0.0) == 2 ** 31 - 1   # no attribute can move the product
    assert f(25.4) == 27
    assert f(699.0) == 1
    assert f(701.0) == 0
    assert f(700.0) == 0
    assert f(float("inf")) == 0 and f(float("nan")) == 0
    # through a model: dmax is the largest |difference|, whichever its sign
    w = np.zeros((4, 2))
    w[1] = (0.0, 12.7)
    w[2] = (12.7, -12.7)
    m = nat.Model.from_tables(w, np.zeros((2, 2)))
    assert m.slot_table(1)[1:] == (25.4, 27) and m.slot_table(0)[1:] == (25.4, 27)
    assert nat.Model.from_tables(np.zeros((3, 2)), np.zeros((2, 2))).slot_table(1)[1:] == (0.0, 2 ** 31 - 1)


def test_margin_absorbs_the_summation_order():
    """over a contig, sum_g |sum_a delta_a - (s1 - s0)| stays below ulp(M) = M 2^-52 with
    M = nnz * 2 max|w| + (n + 2) max|trans| (vd_bound), the term vd_margin is widened by.  Sequential fp64 sums in CSR order on
    both sides, as the kernels add them."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for trial in range(40):
        A = 300
        scale = (0.01, 1.7, 40.0)[trial % 3]
        w = rng.laplace(0.0, scale, size=(A, 2))
        tmax = 1.0
        wmax = np.abs(w).max()
        n = int(rng.integers(1, 400))
        k = rng.integers(0, 30, size=n)
        nnz = int(k.sum())
        total = 0.0
        for g in range(n):
            ids = rng.integers(0, A, size=k[g])
            s0 = s1 = d = 0.0
            for a in ids:
                s0 += w[a, 0]
                s1 += w[a, 1]
                d += w[a, 1] - w[a, 0]
            total += abs(d - (s1 - s0))
        ulp_m = (nnz * 2.0 * wmax + (n + 2.0) * tmax) * 2.0 ** -52
        worst = max(worst, total / ulp_m)
        assert total < ulp_m, (trial, total, ulp_m)
    print("largest sum of differences, in ulp(M):", worst)
