"""Decoding under a minimum run length on the device: ``gecco_crf_viterbi_min_run`` against the independent yardstick
(tests/minrun_reference.py: the run-counter recursion and path enumeration), up through ``SequenceCRF.predict_min_run`` and the
typed front end's ``predict_path_clusters``.

Two tiers.  Exact (integer weights in -2 .. 2: every sum is exact and ties abound): labels identical to the reference recursion
and scores bit-equal, nothing excused -- the kernel scans its sources in the reference's order.  Rounded (normal weights): the
device's OWN path is judged, so a near-tie is harmless and nothing is excused either: the path is feasible, the device score is
within B = 4 T eps (sum of |terms of the path|) of the left-to-right sum along it (kbest_reference.bound), and it is no more
than 2 B below the reference's best.  log Z_C is compared with the reference recursion in ``numpy.longdouble`` under
(T + 1)(2 L + 8) eps max(1, M), M the largest finite |forward value| of the reference on the contig: per gene at most 2 L
exponentials and positive additions, one logarithm and three additions at magnitude <= M.

The seam grid runs every label count against every minimum.  A (label count, minimum) case takes the four label sets and the
four kinds of batch (plain, valued, masked, valued and masked) as a Latin square rotated by the case's position in the grid, so
that every set meets every kind at every label count and at every minimum, and a case stays at a second or two: the numpy
yardstick is what costs the time."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import kbest_reference as kr
from tests import minrun_reference as mr
from tests import test_gpu_kbest as gk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = [2, 3, 4, 8, 9, 16, 17, 32]
MINIMA = [1, 2, 3, 5, 16, 32]
KINDS = ((False, False), (True, False), (False, True), (True, True))  # (valued, masked)
WORST = {"ratio": 0.0}  # the largest |log Z_C - reference| / bound seen by this module's tests, printed by each


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


# ---------------------------------------------------------------- batches and the yardstick
def seam_lengths(L, m):
    """The lengths at the kernel's seams, mixed so that the lane groups of a wave end at different steps: every seam length, and
    as many more as two waves and a half hold at this label count.  A leading sequence of 3 items stays outside the batch
    (``contig_ptr[0] > 0``)."""
    rng = np.random.default_rng(90 + 40 * L + m)
    seams = sorted({0, 1, max(m - 1, 0), m, m + 1, 7, 8, 9, 64, 65, 300})
    groups = 64 // max(2, 1 << (L - 1).bit_length())
    more = max(0, 2 * groups + groups // 2 - len(seams))
    lengths = seams + [int(x) for x in rng.choice(seams[:-1], size=more)]
    rng.shuffle(lengths)
    return [3] + lengths


@functools.lru_cache(maxsize=None)
def seam_batch(L, m, integer):
    return gk.make_batch(9200 + 40 * L + m + 5000 * integer, L, seam_lengths(L, m), integer=integer)


def label_sets(L):
    """One label; all but label 0; the top labels only; every label."""
    return [1 << (L // 2), ((1 << L) - 1) & ~1, ((1 << L) - 1) & ~((1 << (L - (L + 1) // 2)) - 1), (1 << L) - 1]


def call(model, b, mask, m, valued, masked, first=1, **more):
    """The batch from sequence `first` on: contig_ptr[0] > 0 where first > 0."""
    return model.viterbi_min_run(b["cptr"][first:], b["gptr"], b["attr"], mask, m, **gk.kw(b, valued, masked), **more)


def rebased(b, valued, masked, first=1):
    """The same sequences as a batch of its own that starts at item 0, for the entries that take no other: (csr, keywords)."""
    cptr, gptr, attr = b["csr"]
    g0 = int(cptr[first])
    a0 = int(gptr[g0])
    return ((cptr[first:] - g0, gptr[g0:] - a0, attr[a0:]),
            dict(values=b["v"][a0:] if valued else None, allowed=b["allowed"][g0:] if masked else None))


def sequences(b, first=1):
    cptr = b["cptr"]
    return [(c - first, int(cptr[c]), int(cptr[c + 1])) for c in range(first, len(cptr) - 1)]


def check_lognorm(tag, got, want, largest, T, L):
    """|log Z_C - reference| under the derived bound; returns the ratio."""
    if want == -np.inf:
        assert got == -np.inf, f"{tag}: log Z_C {got!r}, expected -inf"
        return 0.0
    bound = mr.lognorm_bound(T, L, largest)
    err = abs(float(np.longdouble(got) - want))
    assert np.isfinite(got) and err <= bound, f"{tag}: log Z_C off by {err:.3g}, bound {bound:.3g} (T={T}, L={L}, M={largest:.3g})"
    WORST["ratio"] = max(WORST["ratio"], err / bound)
    return err / bound


def judge(tag, b, mask, m, valued, masked, got, exact, base=1):
    """The acceptance of one call against the yardstick, sequence by sequence; `base`: the first sequence of the call."""
    y, sc, lzc, lz = got
    L = b["L"]
    score, absolute = gk.tables(b, valued, masked)
    absT = np.abs(b["trans"])
    g_base = int(b["cptr"][base])
    assert y.dtype == np.int8 and y.shape == (int(b["cptr"][-1]) - g_base,) and sc.shape == lzc.shape == lz.shape == (len(b["cptr"]) - 1 - base,)
    assert not np.isnan(sc).any() and not np.isnan(lzc).any()
    worst_b = worst_z = 0.0
    for c, g0, g1 in sequences(b, base):
        T = g1 - g0
        where = f"{tag} sequence {c} (T={T})"
        if T == 0:
            assert sc[c] == 0.0 and lzc[c] == 0.0 and lz[c] == 0.0, f"{where}: an empty sequence has score 0 and log Z 0"
            continue
        mine = y[g0 - g_base:g1 - g_base].astype(np.int64)
        path, best = mr.recursion(score[g0:g1], b["trans"], mask, m)
        z, largest = mr.recursion(score[g0:g1], b["trans"], mask, m, "sum")
        if path is None:
            assert np.all(mine == -1) and sc[c] == -np.inf and lzc[c] == -np.inf, f"{where}: no feasible path is -1 / -inf / -inf"
            continue
        assert np.all(mine >= 0) and mr.feasible(mine, mask, m), f"{where}: the device's path has a short run"
        if exact:
            assert mine.tolist() == path.tolist(), f"{where}: another path than the reference recursion's"
            assert sc[c] == best, f"{where}: score {sc[c]!r}, expected {best!r}"
            if L ** T <= 4096:
                assert mr.enumerate_paths(score[g0:g1], b["trans"], mask, m)[0] == best, f"{where}: the reference is not enumeration's"
        else:
            B = kr.bound(mine, absolute[g0:g1], absT)
            along = kr.path_score(score[g0:g1], b["trans"], mine)
            assert abs(sc[c] - along) <= B, f"{where}: score off its own path's sum by {abs(sc[c] - along):.3g}, B = {B:.3g}"
            assert sc[c] >= best - 2.0 * B, f"{where}: score {sc[c]!r} is more than 2 B below the reference's best {best!r}"
            worst_b = max(worst_b, abs(sc[c] - along) / B if B > 0 else 0.0)
        worst_z = max(worst_z, check_lognorm(where, lzc[c], z, largest, T, L))
        assert lzc[c] <= lz[c] + mr.lognorm_bound(T, L, max(largest, abs(lz[c]))), f"{where}: log Z_C {lzc[c]!r} above log Z {lz[c]!r}"
        if m == 1:
            assert abs(lzc[c] - lz[c]) <= mr.lognorm_bound(T, L, max(largest, abs(lz[c]))), f"{where}: m = 1, log Z_C is not log Z"
    return worst_b, worst_z


def same_bytes(a, b):
    return all((x is None and z is None) or x.tobytes() == z.tobytes() for x, z in zip(a, b))


# ---------------------------------------------------------------- 1. the seams
@pytest.mark.parametrize("m", MINIMA)
@pytest.mark.parametrize("L", LABELS)
def test_seams(nat, L, m):
    turn = LABELS.index(L) + MINIMA.index(m)
    sets = label_sets(L)
    held = 0  # (sequences whose free Viterbi path is feasible: all of them at m = 1, whatever the seeds give otherwise)
    for exact in (True, False):
        b = seam_batch(L, m, exact)
        lengths = np.diff(b["cptr"])[1:].tolist()
        assert {0, 1, m, m + 1, 7, 8, 9, 64, 65, 300} <= set(lengths) and b["cptr"][1] > 0
        assert len(lengths) >= 2 * (64 // max(2, 1 << (L - 1).bit_length())) + 1
        model = nat.Model.from_tables(b["w"], b["trans"])
        for s, mask in enumerate(sets):
            valued, masked = KINDS[(s + turn) % 4]
            tag = f"L={L} m={m} set={mask:#x} values={valued} allowed={masked} exact={exact}"
            got = call(model, b, mask, m, valued, masked)
            worst_b, worst_z = judge(tag, b, mask, m, valued, masked, got, exact)
            print(f"{tag}: worst |score - own path| / B = {worst_b:.3g}, worst |log Z_C error| / bound = {worst_z:.3g}")
            # asking for log Z_C changes no byte of y and score; equal calls give equal bytes
            bare = call(model, b, mask, m, valued, masked, want_lognorm=False)
            assert bare[2] is None and bare[3] is None and same_bytes(bare[:2], got[:2]), f"{tag}: log Z_C changes y or score"
            assert same_bytes(call(model, b, mask, m, valued, masked), got), f"{tag}: equal calls, other bytes"
            # log Z is the marginals entry's
            csr0, kw0 = rebased(b, valued, masked)
            _, elogz = model.marginals_full(*csr0, **kw0)
            assert got[3].tobytes() == elogz.tobytes(), f"{tag}: lognorm is not the marginals entry's"
            # against the entries that exist: the free Viterbi path, where it is feasible
            vy, _ = model.viterbi(*csr0, **kw0)
            ky, ksc, _, _ = model.viterbi_kbest(*csr0, 1, **kw0)
            assert ky[:, 0].tobytes() == vy.tobytes()
            g_base = int(b["cptr"][1])
            for c, g0, g1 in sequences(b):
                if g1 == g0:
                    continue
                free = vy[g0 - g_base:g1 - g_base]
                if m == 1 or mr.feasible(free, mask, m):
                    held += 1
                    # (the best of all paths is the best of the feasible ones: the same left-to-right sum, the same bits)
                    assert got[1][c] == ksc[c, 0], f"{tag} sequence {c}: the free path is feasible, the score is not its score"
                    if m == 1 or not exact:  # (integer weights: a tie may go to another feasible path of that score)
                        assert got[0][g0 - g_base:g1 - g_base].tobytes() == free.tobytes(), f"{tag} sequence {c}: not the free path"
    assert held > 0 or m > 1
    print(f"{held} sequences whose free path is feasible; largest |log Z_C - reference| / bound so far: {WORST['ratio']:.3g}")


# ---------------------------------------------------------------- 2. enumeration on small shapes
@pytest.mark.parametrize("L,longest", [(2, 10), (3, 7), (4, 5)])
def test_enumeration(nat, L, longest):
    lengths = list(range(1, longest + 1)) * 2 + [0]
    rng = np.random.default_rng(60 + L)
    for integer in (True, False):
        b = gk.make_batch(9300 + L + 100 * integer, L, lengths, integer=integer)
        model = nat.Model.from_tables(b["w"], b["trans"])
        for m in (1, 2, 3, 4):
            for mask in ((1 << L) - 1, int(rng.integers(1, 1 << L))):
                valued, masked = KINDS[int(rng.integers(0, 4))]
                score, absolute = gk.tables(b, valued, masked)
                y, sc, lzc, lz = call(model, b, mask, m, valued, masked, first=0)
                for c, g0, g1 in sequences(b, 0):
                    if g1 == g0:
                        continue
                    best, arg, logz, count = mr.enumerate_paths(score[g0:g1], b["trans"], mask, m)
                    where = f"L={L} m={m} set={mask:#x} values={valued} allowed={masked} integer={integer} sequence {c}"
                    if count == 0:
                        assert np.all(y[g0:g1] == -1) and sc[c] == -np.inf and lzc[c] == -np.inf, where
                        continue
                    mine = y[g0:g1].astype(np.int64)
                    if integer:  # (every sum is exact: enumeration's best score, and one of the paths that have it)
                        assert sc[c] == best and tuple(mine.tolist()) in arg, where
                    else:        # (the device adds up an item's score in its own order: its own path is judged)
                        B = kr.bound(mine, absolute[g0:g1], np.abs(b["trans"]))
                        assert np.all(mine >= 0) and mr.feasible(mine, mask, m), where
                        assert abs(sc[c] - kr.path_score(score[g0:g1], b["trans"], mine)) <= B and sc[c] >= best - 2.0 * B, where
                    _, largest = mr.recursion(score[g0:g1], b["trans"], mask, m, "sum")
                    check_lognorm(where, lzc[c], logz, largest, g1 - g0, L)
    print(f"largest |log Z_C - reference| / bound so far: {WORST['ratio']:.3g}")


# ---------------------------------------------------------------- 3. planted cases
def planted_model(nat, score, trans):
    """A model whose item scores are `score`: one private attribute per item."""
    T = len(score)
    cptr, gptr, attr = np.array([0, T], dtype=np.int32), np.arange(T + 1, dtype=np.int32), np.arange(T, dtype=np.int32)
    return nat.Model.from_tables(np.asarray(score, dtype=float), np.asarray(trans, dtype=float)), (cptr, gptr, attr)


PLANTED = [  # (what, the score of label 1 per item, the free path, the constrained path): S = {1}, m = 3, label 0 scores 0
    ("a run of 1 at the last item is extended", [-3, -3, -3, -3, -0.4, -0.4, 4], [0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 1, 1, 1]),
    ("a run of 1 at the last item is dropped", [-3, -3, -3, -3, -3, -3, 4], [0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0]),
    ("a run of 1 at the first item is extended", [4, -0.4, -0.4, -3, -3, -3, -3], [1, 0, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0]),
    ("a run of 1 at the first item is dropped", [4, -3, -3, -3, -3, -3, -3], [1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0]),
    ("two runs of 2 are merged across a gap of 1", [-3, 3, 3, -3.5, 3, 3, -3, -3], [0, 1, 1, 0, 1, 1, 0, 0], [0, 1, 1, 1, 1, 1, 0, 0]),
]


@pytest.mark.parametrize("what,ones,free,want", PLANTED, ids=[p[0] for p in PLANTED])
def test_planted_short_runs(nat, what, ones, free, want):
    trans = np.array([[0.5, -1.0], [-1.0, 0.5]])
    score = np.stack([np.zeros(len(ones)), np.array(ones, dtype=float)], axis=1)
    model, csr = planted_model(nat, score, trans)
    assert model.viterbi(*csr)[0].tolist() == free and not mr.feasible(free, 2, 3)
    best, arg, logz, _ = mr.enumerate_paths(score, trans, 2, 3)
    assert arg == [tuple(want)], "the planted case is what enumeration says"
    y, sc, lzc, lz = model.viterbi_min_run(*csr, 2, 3)
    assert y.tolist() == want and sc[0] == best
    check_lognorm(what, lzc[0], logz, mr.recursion(score, trans, 2, 3, "sum")[1], len(ones), 2)
    assert lzc[0] < lz[0]


def test_no_feasible_path(nat):
    b = gk.make_batch(9400, 3, [1, 2, 3, 0, 5, 2])
    model = nat.Model.from_tables(b["w"], b["trans"])
    score, _ = gk.tables(b, False, False)
    # every label in the set and fewer items than the minimum
    y, sc, lzc, lz = model.viterbi_min_run(*b["csr"], 7, 3)
    for c, (g0, g1) in enumerate(zip(b["cptr"][:-1].tolist(), b["cptr"][1:].tolist())):
        if 0 < g1 - g0 < 3:
            assert np.all(y[g0:g1] == -1) and sc[c] == -np.inf and lzc[c] == -np.inf and np.isfinite(lz[c])
        elif g1 > g0:  # (every path is feasible: log Z_C is log Z)
            z, largest = mr.recursion(score[g0:g1], b["trans"], 7, 3, "sum")
            assert np.all(y[g0:g1] >= 0) and np.isfinite(sc[c])
            check_lognorm(f"sequence {c}", lzc[c], z, largest, g1 - g0, 3)
            assert abs(lzc[c] - lz[c]) <= mr.lognorm_bound(g1 - g0, 3, largest)
        else:
            assert sc[c] == 0.0 and lzc[c] == 0.0 and lz[c] == 0.0
    # masks: every second item allows label 0 alone and the others the set {1, 2} alone -- runs of 1 everywhere
    n = int(b["cptr"][-1])
    allowed = np.where(np.arange(n) % 2 == 0, 6, 1).astype(np.uint32)
    y, sc, lzc, lz = model.viterbi_min_run(*b["csr"], 6, 2, allowed=allowed)
    lengths = np.diff(b["cptr"])
    assert np.all(y == -1) and np.all(sc[lengths > 0] == -np.inf) and np.all(lzc[lengths > 0] == -np.inf)
    assert np.all(np.isfinite(lz)) and not np.isnan(lzc).any()
    # masks that allow no label of the set: the path stays outside, and log Z_C is log Z
    only0 = np.full(n, 1, dtype=np.uint32)
    y, sc, lzc, lz = model.viterbi_min_run(*b["csr"], 6, 2, allowed=only0)
    ky, ksc, _, _ = model.viterbi_kbest(*b["csr"], 1, allowed=only0)
    assert np.all(y == 0) and np.all(ky == 0) and np.array_equal(sc[lengths > 0], ksc[lengths > 0, 0])
    # (one path: its log-mass is its score, computed twice in other ways)
    for c in np.flatnonzero(lengths > 0).tolist():
        assert abs(lzc[c] - lz[c]) <= mr.lognorm_bound(int(lengths[c]), 3, abs(sc[c]))


def test_state_scores_of_700_per_item(nat):
    """exp(700 T) overflows and exp(-700 T) underflows: log Z_C is finite all the same, never NaN."""
    L, T = 3, 40
    rng = np.random.default_rng(17)
    for sign in (1.0, -1.0):
        score = sign * 700.0 + rng.normal(0.0, 1.0, size=(T, L))
        score[::3] *= -1.0  # (and a mix of both)
        trans = rng.normal(0.0, 1.5, size=(L, L))
        model, csr = planted_model(nat, score, trans)
        for mask, m in ((6, 3), (7, 5), (2, 32)):
            y, sc, lzc, lz = model.viterbi_min_run(*csr, mask, m)
            z, largest = mr.recursion(score, trans, mask, m, "sum")
            assert np.isfinite(lzc[0]) and np.isfinite(sc[0]) and mr.feasible(y, mask, m)
            ratio = check_lognorm(f"sign {sign} set {mask} m {m}", lzc[0], z, largest, T, L)
            print(f"sign {sign} set {mask} m {m}: log Z_C {lzc[0]!r}, |error| / bound = {ratio:.3g}")
            assert lzc[0] <= lz[0] + mr.lognorm_bound(T, L, largest)


def test_refusals_reach_the_caller(nat):
    b = gk.make_batch(9500, 3, [3, 2])
    model = nat.Model.from_tables(b["w"], b["trans"])
    for bad in (0, -1, 33):
        with pytest.raises(Exception, match=rf"viterbi_min_run: min_run = {bad} is outside 1 \.\. 32"):
            model.viterbi_min_run(*b["csr"], 6, bad)
    for bad in (0, 8):
        with pytest.raises(Exception, match="set_mask"):
            model.viterbi_min_run(*b["csr"], bad, 2)


# ---------------------------------------------------------------- 4. SequenceCRF
@pytest.mark.parametrize("L", [2, 5, 17])
def test_predict_min_run(nat, L):
    b = gk.make_batch(9600 + L, L, [1, 2, 0, 9, 31, 64, 65, 3])
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = gk.sequence_crf(w, b["trans"])
    cptr, gptr, attr = b["csr"]
    X = [[[names[a] for a in dict.fromkeys(attr[gptr[i]:gptr[i + 1]].tolist())] for i in range(cptr[s], cptr[s + 1])]
         for s in range(len(cptr) - 1)]
    inside = classes[1:]
    out = crf.predict_min_run(X, inside, 3)
    assert len(out) == len(X) and all(sorted(o) == ["constraint_log_probability", "labels", "log_probability", "score"] for o in out)
    assert out[2] == {"labels": [], "score": 0.0, "log_probability": 0.0, "constraint_log_probability": 0.0}
    best = crf.predict(X)
    for s, (o, T) in enumerate(zip(out, np.diff(cptr).tolist())):
        if T == 0:
            continue
        assert len(o["labels"]) == T and set(o["labels"]) <= set(classes)
        assert mr.feasible([classes.index(name) for name in o["labels"]], (1 << L) - 2, 3)
        assert o["log_probability"] <= o["constraint_log_probability"] + 1e-9 and o["constraint_log_probability"] <= 1e-9
        again = crf.log_likelihood([X[s]], [o["labels"]])[0]
        assert abs(again - o["log_probability"]) <= 1e-12 * max(1.0, abs(o["score"]))
        if mr.feasible([classes.index(name) for name in best[s]], (1 << L) - 2, 3):
            assert o["labels"] == best[s]
    # a minimum of 1 is predict's path; every label in the set leaves the short sequences without a path
    assert [o["labels"] for o in crf.predict_min_run(X, classes[0], 1)] == best
    short = crf.predict_min_run(X, classes, 3)
    assert short[0]["labels"] is None and short[0]["score"] == -np.inf and short[0]["constraint_log_probability"] == -np.inf
    assert short[1]["labels"] is None and short[3]["labels"] is not None and short[2]["labels"] == []
    # with allowed sets the path stays inside them
    allowed = [[{classes[0], classes[-1]} if t % 2 else None for t in range(T)] for T in np.diff(cptr).tolist()]
    for o, sets in zip(crf.predict_min_run(X, inside, 2, allowed=allowed), allowed):
        assert o["labels"] is None or all(a is None or lab in a for lab, a in zip(o["labels"], sets))


# ---------------------------------------------------------------- 5. the typed front end
def test_typed_front_end_calls_path_clusters(nat, tmp_path):
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
    y, sc, lzc, lz = model.viterbi_min_run(cptr, gptr, attr, ((1 << L) - 1) & ~(1 << bg), M)
    found = crf.predict_path_clusters(genes, min_run=M)
    assert found and all(len(c.genes) >= M for c in found)
    rows = crf.path_posteriors_
    assert sorted(rows) == sorted(crf.PATH_COLUMNS) and rows["sequence_id"] == [c[0].source.id for c in contigs]
    assert rows["genes"] == np.diff(cptr).tolist() and rows["log_z"] == lz.tolist() and rows["score"] == sc.tolist()
    assert rows["log_p"] == (sc - lz).tolist() and rows["constraint_log_p"] == (lzc - lz).tolist()
    assert sum(rows["clusters"]) == len(found) and all(p <= 1e-9 for p in rows["constraint_log_p"])
    # the clusters are the runs of the path
    ids = [g.id for g in ordered]
    seen = np.full(len(ordered), bg, dtype=np.int64)
    for ci, contig in enumerate(contigs):
        mine = [c for c in found if c.genes[0].source.id == contig[0].source.id]
        assert [c.id for c in mine] == [f"{contig[0].source.id}_cluster_{k + 1}" for k in range(len(mine))]
    for c in found:
        first, last = ids.index(c.genes[0].id), ids.index(c.genes[-1].id) + 1
        assert np.all(y[first:last] != bg) and (first == 0 or y[first - 1] == bg or first in cptr.tolist())
        seen[first:last] = y[first:last]
        major = int(np.argmax(np.bincount(y[first:last].astype(np.int64), minlength=L)))
        assert c.path_type == (";".join(crf.label_types_[major]) or "Unknown")
    assert np.array_equal(seen != bg, y != bg), "every run of the path is a cluster"
    # a known region: its genes cannot be background, so the constrained path holds a cluster that covers them
    assert "Beta" in crf.classes_ and ids[60].startswith("fresh00") and cptr[1] >= 70
    known = tables.ClusterTable({"sequence_id": ["fresh00"], "cluster_id": ["k1"], "start": [ordered[60].start],
                                 "end": [ordered[69].end], "type": ["Beta"]})
    k_found = crf.predict_path_clusters(genes, min_run=M, known=known)
    assert any(set(ids[60:70]) <= {g.id for g in c.genes} for c in k_found) and all(len(c.genes) >= M for c in k_found)
    assert crf.path_posteriors_["log_z"][0] <= rows["log_z"][0] and np.allclose(crf.path_posteriors_["log_z"][1:], rows["log_z"][1:], rtol=0, atol=1e-9)
    found = crf.predict_path_clusters(genes, min_run=M)
    assert crf.path_posteriors_ == rows
    # the command line: both files with the flag, clusters.tsv unchanged, and nothing new without it
    crf.save(os.path.join(base, "model"))
    common = [sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
              os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv")]
    for flags, out in (([], "plain"), (["--path-clusters", str(M)], "cli")):
        done = subprocess.run(common + flags + ["-o", os.path.join(base, out)], cwd=ROOT, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
    gs._same_tables(os.path.join(base, "plain"), os.path.join(base, "cli"))
    assert open(os.path.join(base, "plain", "clusters.tsv"), "rb").read() == open(os.path.join(base, "cli", "clusters.tsv"), "rb").read()
    assert not os.path.exists(os.path.join(base, "plain", "paths.tsv")) and not os.path.exists(os.path.join(base, "plain", "path_clusters.tsv"))
    with open(os.path.join(base, "cli", "paths.tsv")) as fh:
        lines = [line.rstrip("\n").split("\t") for line in fh]
    assert lines[0] == list(crf.PATH_COLUMNS) and len(lines) == 1 + len(contigs)
    assert [row[0] for row in lines[1:]] == rows["sequence_id"] and [int(row[6]) for row in lines[1:]] == rows["clusters"]
    assert all(abs(float(row[5]) - v) <= 1e-12 for row, v in zip(lines[1:], rows["constraint_log_p"]))
    with open(os.path.join(base, "cli", "path_clusters.tsv")) as fh:
        lines = [line.rstrip("\n").split("\t") for line in fh]
    assert lines[0] == ["sequence_id", "cluster_id", "start", "end", "genes", "type"]
    assert [row[1] for row in lines[1:]] == [c.id for c in found] and all(int(row[4]) >= M for row in lines[1:])
