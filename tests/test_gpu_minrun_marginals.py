"""Marginals under a minimum run length on the device: ``gecco_crf_marginals_min_run`` against the independent yardstick
(tests/minrun_marginals_reference.py: a forward-backward over the explicit expanded state list in ``numpy.longdouble``, and path
enumeration), up through ``SequenceCRF.predict_marginals_min_run`` and ``TypedClusterCRF.predict_path_clusters(marginals=True)``.

The tolerance is derived, not measured.  A log-marginal is alpha + beta - log Z_C; each of the three is within
``minrun_reference.lognorm_bound(T, L, M)`` of its exact value, M the yardstick's largest finite |alpha or beta| on the sequence
(per gene at most 2 L exponentials and positive additions, one logarithm and three additions at magnitude <= M), and the sum over
the run counter adds (m + 4) eps.  So wherever the yardstick's p >= 1e-280 the relative error of p is at most
``expm1(3 lognorm_bound(T, L, M) + (m + 4) eps)``, the device's value is <= 1e-279 where the yardstick's is smaller, and
|sum_j marg - 1| is within the same bound on a feasible sequence.  A wrong source set or a dropped slot misses this by many
orders of magnitude.

The seam grid runs every label count against every minimum, the three label sets and the two weight families; the largest case
(8 labels at a minimum of 32) takes about a second, most of it the longdouble yardstick.  A yardstick is computed once per
(batch, set, minimum) and shared."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import minrun_marginals_reference as mm
from tests import minrun_reference as mr
from tests import test_gpu_kbest as gk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = mr.EPS
CASES = [(L, m) for L in (2, 3, 5, 8, 32) for m in (1, 2, 3, 32) if (m < 32 or L <= 8) and (L < 32 or m <= 5)]
FAMILIES = {"unit": (1.0, 1.5), "wide": (30.0, 10.0)}  # the deviations of the state scores and of the transitions
WORST = {"ratio": 0.0}  # the largest error / bound seen by this module's tests, printed by each


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


# ---------------------------------------------------------------- batches, the yardstick, the acceptance
def seam_lengths(m):
    """The lengths the issue names, in one batch: 15 contigs, no multiple of any 64 / LP."""
    return [0, 1, m - 1, m, m + 1, 2 * m, 2 * m + 1, 7, 8, 9, 16, 17, 63, 64, 65]


def direct_batch(seed, L, lengths, family="unit"):
    """A batch whose state scores are a table of its own: every gene has one private attribute, so the model's weights are
    the scores.  (score [n, L], trans [L, L], the CSR arrays)."""
    rng = np.random.default_rng(seed)
    s_state, s_trans = FAMILIES[family]
    cptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(cptr[-1])
    score, trans = rng.normal(0.0, s_state, size=(n, L)), rng.normal(0.0, s_trans, size=(L, L))
    return dict(L=L, score=score, trans=trans, cptr=cptr, csr=(cptr, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)))


@functools.lru_cache(maxsize=None)
def seam_batch(L, m, family):
    return direct_batch(9700 + 40 * L + m + (5000 if family == "wide" else 0), L, seam_lengths(m), family)


def label_sets(L):
    """The last label; every label but 0; every label."""
    return [1 << (L - 1), ((1 << L) - 1) & ~1, (1 << L) - 1]


def bound(T, L, M, m):
    return math.expm1(3.0 * mr.lognorm_bound(T, L, M) + (m + 4) * EPS)


def yardstick(b, score, mask, m):
    """Per contig (marginals, log Z_C, M) or None for one without genes; kept on the batch and left unchanged."""
    key = ("yard", mask, m)
    if key not in b:
        out = []
        for g0, g1 in zip(b["cptr"][:-1].tolist(), b["cptr"][1:].tolist()):
            out.append(mm.forward_backward(score[g0:g1], b["trans"], mask, m) if g1 > g0 else None)
        b[key] = out
    return b[key]


def judge(tag, b, score, mask, m, got):
    """One call against the yardstick, contig by contig; returns the worst error / bound."""
    marg, inside, lzc, lz = got
    L = b["L"]
    cptr = b["cptr"]
    n, nc = int(cptr[-1]), len(cptr) - 1
    assert marg.shape == (n, L) and marg.dtype == np.float64 and inside.shape == (n,) and lzc.shape == lz.shape == (nc,)
    assert not np.isnan(marg).any() and not np.isnan(inside).any() and not np.isnan(lzc).any()
    assert np.all(marg[score == -np.inf] == 0.0), f"{tag}: a disallowed pair is not exactly 0.0"
    cols = [j for j in range(L) if (mask >> j) & 1]
    worst = 0.0
    for c, ref in enumerate(yardstick(b, score, mask, m)):
        g0, g1 = int(cptr[c]), int(cptr[c + 1])
        T = g1 - g0
        where = f"{tag} contig {c} (T={T})"
        if ref is None:
            assert lzc[c] == 0.0 and lz[c] == 0.0, f"{where}: a contig without genes has 0 for both log Z"
            continue
        want, z, M = ref
        mine = marg[g0:g1]
        if z == -np.inf:
            assert lzc[c] == -np.inf and not mine.any() and not inside[g0:g1].any(), f"{where}: no feasible path is -inf and zeros"
            continue
        zb = mr.lognorm_bound(T, L, M)
        assert np.isfinite(lzc[c]) and abs(float(np.longdouble(lzc[c]) - z)) <= zb, f"{where}: log Z_C off by {float(lzc[c] - z):.3g}, bound {zb:.3g}"
        B = bound(T, L, M, m)
        big = want >= 1e-280
        rel = np.abs((mine.astype(np.longdouble)[big] - want[big]) / want[big]).astype(np.float64)
        ratio = float(rel.max()) / B
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{where}: relative error {float(rel.max()):.3g}, bound {B:.3g} (L={L}, m={m}, M={M:.3g})"
        assert np.all(mine[~big] <= 1e-279), f"{where}: mass where the yardstick has none"
        total = np.abs(mine.sum(axis=1) - 1.0).max()
        assert total <= B, f"{where}: |sum of a gene's marginals - 1| = {total:.3g}, bound {B:.3g}"
        # inside is the sum of the set's columns, in the kernel's order of additions
        assert np.abs(inside[g0:g1] - mine[:, cols].sum(axis=1)).max() <= L * EPS, f"{where}: inside is not the sum of the set's columns"
    WORST["ratio"] = max(WORST["ratio"], worst)
    return worst


def same_bytes(a, b):
    return all((x is None and z is None) or x.tobytes() == z.tobytes() for x, z in zip(a, b))


def alone(b, c):
    """Contig c of a direct batch as a batch of its own."""
    g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
    T = g1 - g0
    return (np.array([0, T], dtype=np.int32), np.arange(T + 1, dtype=np.int32), np.arange(g0, g1, dtype=np.int32)), g0, g1


# ---------------------------------------------------------------- 1. the seams
@pytest.mark.parametrize("L,m", CASES)
def test_seams(nat, L, m):
    turn = CASES.index((L, m))
    assert (len(seam_lengths(m)) % (64 // max(2, 1 << (L - 1).bit_length()))) != 0
    for s, (mask, family) in enumerate((mask, family) for mask in label_sets(L) for family in FAMILIES):
        b = seam_batch(L, m, family)
        model = nat.Model.from_tables(b["score"], b["trans"])
        tag = f"L={L} m={m} set={mask:#x} {family}"
        got = model.marginals_min_run(*b["csr"], mask, m)
        worst = judge(tag, b, b["score"], mask, m, got)
        print(f"{tag}: worst error / bound = {worst:.3g}")
        # log Z_C has the decoder's bits, log Z the marginals entry's
        _, _, vlzc, vlz = model.viterbi_min_run(*b["csr"], mask, m)
        assert got[2].tobytes() == vlzc.tobytes(), f"{tag}: lognorm_min_run is not viterbi_min_run's"
        free, elogz = model.marginals_full(*b["csr"])
        assert got[3].tobytes() == vlz.tobytes() == elogz.tobytes(), f"{tag}: lognorm is not the marginals entry's"
        # equal calls, equal bytes; without marg, inside keeps its bytes; without inside, marg keeps its own
        assert same_bytes(model.marginals_min_run(*b["csr"], mask, m), got), f"{tag}: equal calls, other bytes"
        bare = model.marginals_min_run(*b["csr"], mask, m, want_marginals=False)
        assert bare[0] is None and same_bytes(bare[1:], got[1:]), f"{tag}: inside changes with marg NULL"
        bare = model.marginals_min_run(*b["csr"], mask, m, want_inside=False)
        assert bare[1] is None and bare[0].tobytes() == got[0].tobytes(), f"{tag}: marg changes with inside NULL"
        if m == 1:  # the expanded lattice is the plain one
            for c, ref in enumerate(yardstick(b, b["score"], mask, m)):
                if ref is None:
                    continue
                g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
                want, _, M = ref
                B, big = bound(g1 - g0, L, M, m), ref[0] >= 1e-280
                diff = np.abs(got[0][g0:g1][big] - free[g0:g1][big]) / want[big].astype(np.float64)
                assert diff.max() <= B, f"{tag} contig {c}: m = 1 is not marginals_full ({diff.max():.3g}, bound {B:.3g})"
                assert abs(got[2][c] - got[3][c]) <= mr.lognorm_bound(g1 - g0, L, max(M, abs(got[3][c]))), f"{tag} contig {c}: log Z_C is not log Z"
        if s == turn % 6:  # every contig alone has the bytes it has inside the batch
            for c in range(len(b["cptr"]) - 1):
                csr, g0, g1 = alone(b, c)
                if g1 == g0:
                    continue
                am, ai, alzc, alz = model.marginals_min_run(*csr, mask, m)
                assert am.tobytes() == got[0][g0:g1].tobytes() and ai.tobytes() == got[1][g0:g1].tobytes(), f"{tag} contig {c}: alone, other bytes"
                assert alzc[0] == got[2][c] or (np.isinf(alzc[0]) and np.isinf(got[2][c]))
    print(f"largest error / bound so far: {WORST['ratio']:.3g}")


# ---------------------------------------------------------------- 2. enumeration on small shapes
@pytest.mark.parametrize("L,longest", [(2, 8), (3, 6)])
def test_enumeration(nat, L, longest):
    lengths = list(range(1, longest + 1)) * 2 + [0]
    b = direct_batch(9800 + L, L, lengths)
    model = nat.Model.from_tables(b["score"], b["trans"])
    cptr = b["cptr"]
    worst = 0.0
    for m in (1, 2, 3, 4):
        for mask in range(1, 1 << L):
            marg, inside, lzc, lz = model.marginals_min_run(*b["csr"], mask, m)
            for c in range(len(cptr) - 1):
                g0, g1 = int(cptr[c]), int(cptr[c + 1])
                if g1 == g0:
                    continue
                where = f"L={L} m={m} set={mask:#x} contig {c}"
                want, logz = mm.enumerate_marginals(b["score"][g0:g1], b["trans"], mask, m)
                if logz == -np.inf:
                    assert lzc[c] == -np.inf and not marg[g0:g1].any() and not inside[g0:g1].any(), where
                    continue
                M = mm.forward_backward(b["score"][g0:g1], b["trans"], mask, m)[2]
                B = bound(g1 - g0, L, M, m)
                big = want >= 1e-280
                rel = np.abs((marg[g0:g1].astype(np.longdouble)[big] - want[big]) / want[big]).astype(np.float64)
                assert rel.max() <= B and np.all(marg[g0:g1][~big] <= 1e-279), f"{where}: {rel.max():.3g}, bound {B:.3g}"
                assert abs(float(np.longdouble(lzc[c]) - logz)) <= mr.lognorm_bound(g1 - g0, L, M), where
                worst = max(worst, float(rel.max()) / B)
    print(f"L={L}: worst error / bound against enumeration = {worst:.3g}")


# ---------------------------------------------------------------- 3. structure
def test_contigs_shorter_than_the_minimum(nat):
    b = direct_batch(9900, 3, [1, 2, 3, 0, 5, 2])
    model = nat.Model.from_tables(b["score"], b["trans"])
    short = np.concatenate([np.full(T, T < 3) for T in np.diff(b["cptr"]).tolist()])
    # the set is not every label: a short contig stays outside -- the set's columns are exactly 0.0
    got = model.marginals_min_run(*b["csr"], 6, 3)
    judge("short, set {1, 2}", b, b["score"], 6, 3, got)
    assert np.all(got[0][short][:, 1:] == 0.0) and np.all(np.abs(got[0][short][:, 0] - 1.0) <= 1e-12) and np.all(got[1][short] == 0.0)
    assert np.all(np.isfinite(got[2][np.diff(b["cptr"]) > 0]))
    # every label in the set: a short contig has no path
    marg, inside, lzc, lz = model.marginals_min_run(*b["csr"], 7, 3)
    judge("short, every label", b, b["score"], 7, 3, (marg, inside, lzc, lz))
    lengths = np.diff(b["cptr"])
    assert not marg[short].any() and not inside[short].any() and np.all(lzc[(lengths > 0) & (lengths < 3)] == -np.inf)
    assert not np.isnan(marg).any() and not np.isnan(inside).any() and not np.isnan(lzc).any() and np.all(np.isfinite(lz))
    assert np.all(np.abs(inside[~short] - 1.0) <= 1e-12)


def test_a_contig_of_exactly_the_minimum_is_all_or_nothing(nat):
    for m in (2, 3, 7, 32):
        b = direct_batch(9910 + m, 2, [m])
        model = nat.Model.from_tables(b["score"], b["trans"])
        got = model.marginals_min_run(*b["csr"], 2, m)
        judge(f"T = m = {m}", b, b["score"], 2, m, got)
        col = got[0][:, 1]
        _, _, M = yardstick(b, b["score"], 2, m)[0]
        assert np.abs(col - col[0]).max() <= bound(m, 2, M, m) * col[0], f"m={m}: the run is there at every gene or at none"


def test_a_planted_lone_gene(nat):
    """+30 for label 1 at one gene of a background of -3, m = 3: the free marginal there is above 0.9, the constrained one
    follows the yardstick -- the two differ where it matters."""
    T = 9
    score = np.stack([np.zeros(T), np.full(T, -3.0)], axis=1)
    score[4, 1] = 30.0
    b = dict(L=2, score=score, trans=np.array([[0.5, -1.0], [-1.0, 0.5]]), cptr=np.array([0, T], dtype=np.int32),
             csr=(np.array([0, T], dtype=np.int32), np.arange(T + 1, dtype=np.int32), np.arange(T, dtype=np.int32)))
    model = nat.Model.from_tables(b["score"], b["trans"])
    free, _ = model.marginals_full(*b["csr"])
    got = model.marginals_min_run(*b["csr"], 2, 3)
    judge("planted", b, score, 2, 3, got)
    want = yardstick(b, score, 2, 3)[0][0]
    assert free[4, 1] > 0.9 and free[3, 1] < 0.1 and free[5, 1] < 0.1
    assert abs(got[1][4] - float(want[4, 1])) <= 1e-12 and max(got[1][3], got[1][5]) > 5.0 * max(free[3, 1], free[5, 1])
    print(f"gene 4: free {free[4, 1]:.6g}, constrained {got[1][4]:.6g}; its neighbours: free {free[3, 1]:.3g} / {free[5, 1]:.3g}, "
          f"constrained {got[1][3]:.3g} / {got[1][5]:.3g}")


def test_state_scores_of_700_per_item(nat):
    """exp(700 T) overflows and exp(-700 T) underflows: everything stays finite and within the bound."""
    T = 64
    rng = np.random.default_rng(17)
    for L, mask, m in ((2, 2, 1), (3, 6, 3), (3, 7, 5)):
        for sign in (1.0, -1.0):
            score = sign * 700.0 + rng.normal(0.0, 1.0, size=(T, L))
            score[::3] *= -1.0  # (and a mix of both)
            b = dict(L=L, score=score, trans=rng.normal(0.0, 1.5, size=(L, L)), cptr=np.array([0, T], dtype=np.int32),
                     csr=(np.array([0, T], dtype=np.int32), np.arange(T + 1, dtype=np.int32), np.arange(T, dtype=np.int32)))
            model = nat.Model.from_tables(b["score"], b["trans"])
            got = model.marginals_min_run(*b["csr"], mask, m)
            assert np.isfinite(got[2][0]) and np.all(np.isfinite(got[0]))
            ratio = judge(f"700: L={L} set={mask} m={m} sign={sign}", b, score, mask, m, got)
            print(f"L={L} set={mask} m={m} sign={sign}: log Z_C {got[2][0]!r}, error / bound = {ratio:.3g}")


# ---------------------------------------------------------------- 4. values and masks
@pytest.mark.parametrize("valued,masked", [(True, False), (False, True)])
def test_values_and_allowed(nat, valued, masked):
    L, m, mask = 5, 3, 0b11100
    b = gk.make_batch(9950 + valued, L, [0, 1, 2, 3, 4, 7, 9, 17, 40, 65, 3])
    b["score"], _ = gk.tables(b, valued, masked)
    model = nat.Model.from_tables(b["w"], b["trans"])
    got = model.marginals_min_run(*b["csr"], mask, m, **gk.kw(b, valued, masked))
    worst = judge(f"values={valued} allowed={masked}", b, b["score"], mask, m, got)
    if masked:
        assert (b["score"] == -np.inf).any() and np.all(got[0][b["score"] == -np.inf] == 0.0)
        _, elogz = model.marginals_full(*b["csr"], **gk.kw(b, valued, masked))
        assert got[3].tobytes() == elogz.tobytes()
    print(f"values={valued} allowed={masked}: worst error / bound = {worst:.3g}")


def test_refusals_reach_the_caller(nat):
    b = direct_batch(9960, 3, [3, 2])
    model = nat.Model.from_tables(b["score"], b["trans"])
    for bad in (0, -1, 33):
        with pytest.raises(Exception, match=rf"marginals_min_run: min_run = {bad} is outside 1 \.\. 32"):
            model.marginals_min_run(*b["csr"], 6, bad)
    for bad in (0, 8):
        with pytest.raises(Exception, match="marginals_min_run: set_mask"):
            model.marginals_min_run(*b["csr"], bad, 2)


# ---------------------------------------------------------------- 5. SequenceCRF
def test_predict_marginals_min_run(nat):
    L = 5
    b = gk.make_batch(9970, L, [1, 2, 0, 9, 31, 64, 3])
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = gk.sequence_crf(w, b["trans"])
    cptr, gptr, attr = b["csr"]
    X = [[[names[a] for a in dict.fromkeys(attr[gptr[i]:gptr[i + 1]].tolist())] for i in range(cptr[s], cptr[s + 1])]
         for s in range(len(cptr) - 1)]
    seq_ptr, item_ptr, ids, values = crf._pack(X)
    inside = classes[1:]
    marg, ins, lzc, lz = crf._model.marginals_min_run(seq_ptr, item_ptr, ids, (1 << L) - 2, 3, values=values)
    out = crf.predict_marginals_min_run(X, inside, 3)
    assert len(out) == len(X) and all(sorted(o) == ["constraint_log_probability", "inside", "marginals"] for o in out)
    again = crf.predict_min_run(X, inside, 3)
    for s, o in enumerate(out):
        g0, g1 = int(seq_ptr[s]), int(seq_ptr[s + 1])
        if g1 == g0:
            assert o["marginals"].shape == (0, L) and o["inside"].shape == (0,) and o["constraint_log_probability"] == 0.0
            continue
        assert o["marginals"].tobytes() == marg[g0:g1].tobytes() and o["inside"].tobytes() == ins[g0:g1].tobytes()
        assert o["constraint_log_probability"] == float(lzc[s] - lz[s]) == again[s]["constraint_log_probability"]
        assert np.abs(o["marginals"].sum(axis=1) - 1.0).max() <= 1e-12
    # columns in predict_marginals' order: at a minimum of 1 these are its numbers
    for o, free in zip(crf.predict_marginals_min_run(X, inside, 1), crf.predict_marginals(X)):
        assert o["marginals"].shape == free.shape and (free.size == 0 or np.abs(o["marginals"] - free).max() <= 1e-12)
    # every label in the set: the short sequences have no path
    short = crf.predict_marginals_min_run(X, classes, 3)
    assert short[0]["marginals"] is None and short[0]["inside"] is None and short[0]["constraint_log_probability"] == -np.inf
    assert short[1]["marginals"] is None and short[3]["marginals"] is not None and short[2]["marginals"].shape == (0, L)
    # with allowed sets the mass stays inside them
    allowed = [[{classes[0], classes[-1]} if t % 2 else None for t in range(T)] for T in np.diff(cptr).tolist()]
    for o, sets in zip(crf.predict_marginals_min_run(X, inside, 2, allowed=allowed), allowed):
        if o["marginals"] is not None:
            for row, a in zip(o["marginals"], sets):
                assert a is None or all(row[k] == 0.0 for k, name in enumerate(classes) if name not in a)


# ---------------------------------------------------------------- 6. the typed front end
def test_typed_front_end_path_marginals(nat, tmp_path):
    import itertools
    import operator
    import random

    from gecco_amd import packing, tables, typed
    from tests import test_gpu_spans as gs
    from tests.typed_planted import C, W, planted_set

    train_genes, train_rows = planted_set(11, 12, "train", composite=True)
    fresh_genes, _ = planted_set(12, 2, "fresh", composite=False)
    base = str(tmp_path)
    gs._write_tables(os.path.join(base, "train"), train_genes, train_rows)
    gs._write_tables(os.path.join(base, "fresh"), fresh_genes)
    random.seed(42)
    np.random.seed(42)
    crf = typed.TypedClusterCRF(W, 1, c1=C, c2=C)
    crf.fit(gs._load(os.path.join(base, "train")), tables.ClusterTable.load(os.path.join(base, "train", "clusters.tsv")))
    genes = gs._load(os.path.join(base, "fresh"))
    L, bg, M = len(crf.classes_), crf.classes_.index("0"), 4
    ordered = sorted(genes, key=operator.attrgetter("source.id", "start"))
    contigs = [list(g) for _, g in itertools.groupby(ordered, key=operator.attrgetter("source.id"))]
    batch = packing.pack_contigs(contigs, crf._attr_index, "protein")
    cptr, gptr, attr = batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id
    model = nat.Model.from_lcrf(crf._blob)
    mask = ((1 << L) - 1) & ~(1 << bg)
    marg, inside, lzc, lz = model.marginals_min_run(cptr, gptr, attr, mask, M)
    y = model.viterbi_min_run(cptr, gptr, attr, mask, M)[0]
    plain = crf.predict_path_clusters(genes, min_run=M)
    assert plain and not any(hasattr(c, "average_p") for c in plain) and not hasattr(crf, "path_gene_probabilities_")
    rows = dict(crf.path_posteriors_)
    found = crf.predict_path_clusters(genes, min_run=M, marginals=True)
    assert [c.id for c in found] == [c.id for c in plain] and crf.path_posteriors_ == rows
    assert crf.path_gene_probabilities_.tobytes() == inside.tobytes()
    ids = [g.id for g in ordered]
    for c in found:
        first, last = ids.index(c.genes[0].id), ids.index(c.genes[-1].id) + 1
        ps = inside[first:last]
        assert (c.average_p, c.max_p, c.min_p) == (float(np.mean(ps)), float(ps.max()), float(ps.min()))
        assert 0.0 <= c.min_p <= c.average_p <= c.max_p <= 1.0 + 1e-12
    pg = crf.path_genes_
    assert sorted(pg) == sorted(crf.PATH_GENE_COLUMNS) and pg["p"] == inside.tolist()
    assert pg["sequence_id"] == [g.source.id for g in ordered] and pg["protein_id"] == [g.protein.id for g in ordered]
    assert pg["path_label"] == [crf.classes_[k] for k in y.tolist()]
    # the constrained probabilities are not the free ones
    free, _ = model.marginals_full(cptr, gptr, attr)
    assert np.abs(inside - (1.0 - free[:, bg])).max() > 1e-6
    # the command line: today's tables without the flag, three columns and a table more with it
    crf.save(os.path.join(base, "model"))
    common = [sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
              os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv")]
    for flags, out in ((["--path-clusters", str(M)], "plain"), (["--path-clusters", str(M), "--path-marginals"], "cli")):
        done = subprocess.run(common + flags + ["-o", os.path.join(base, out)], cwd=ROOT, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
    done = subprocess.run(common + ["--path-marginals", "-o", os.path.join(base, "bad")], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode != 0 and "--path-marginals needs --path-clusters" in done.stderr
    for name in sorted(os.listdir(os.path.join(base, "plain"))):
        if name != "path_clusters.tsv":
            assert open(os.path.join(base, "plain", name), "rb").read() == open(os.path.join(base, "cli", name), "rb").read(), name
    assert sorted(set(os.listdir(os.path.join(base, "cli"))) - set(os.listdir(os.path.join(base, "plain")))) == ["path_genes.tsv"]
    read = lambda *p: [line.rstrip("\n").split("\t") for line in open(os.path.join(base, *p))]
    today, more = read("plain", "path_clusters.tsv"), read("cli", "path_clusters.tsv")
    assert today[0] == ["sequence_id", "cluster_id", "start", "end", "genes", "type"]
    assert more[0] == today[0] + ["average_p", "max_p", "min_p"] and [row[:6] for row in more] == today
    assert [[float(v) for v in row[6:]] for row in more[1:]] == [[c.average_p, c.max_p, c.min_p] for c in found]
    lines = read("cli", "path_genes.tsv")
    assert lines[0] == list(crf.PATH_GENE_COLUMNS) and [row[1] for row in lines[1:]] == pg["protein_id"]
    assert [float(row[3]) for row in lines[1:]] == pg["p"] and [row[2] for row in lines[1:]] == pg["path_label"]
