"""The K best label paths on the device: ``gecco_crf_viterbi_kbest`` against the independent yardstick
(tests/kbest_reference.py: path enumeration and a list recursion), up through ``SequenceCRF.predict_kbest`` and the typed
front end's ``alternatives``.

The separation rule.  A device score must equal the reference's to within B = 4 T eps (sum of |terms of the path|), the terms
being every value x weight product of the path's item scores and every transition weight on it (kbest_reference.bound says
why 4 T covers a left-to-right sum).  Paths must be equal at every rank whose reference score is more than 2 B from both
neighbours -- the reference is computed with one rank more than the call, so the last rank has its neighbour.  At most 1 % of
the ranks of a test may be unseparated: asserted here, and counted for the same seeds with the reference alone by
tests/test_kbest_host.py (random normal weights leave none).  Where every sum is exact (integer weights) nothing is excused:
scores are bit-equal and paths identical at every rank, ties in the reversed-lexicographic order."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import kbest_reference as kr
from tests import train_objective_partial as tp

pytestmark = pytest.mark.gpu

A = 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMAX = 32
SEAM_LABELS = [2, 4, 8, 9, 16, 17, 32]
SEAM_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 33, 64, 65, 300)


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


# ---------------------------------------------------------------- batches and the yardstick
def enumeration_lengths():
    """About 40 sequences of 1, 2, 3 and 6 items, with an empty one in the middle."""
    lengths = [1, 2, 3] * 12 + [6] * 4
    return lengths[:20] + [0] + lengths[20:]


def seam_lengths(L):
    """The lengths at the kernel's seams, mixed so that the lane groups of a wave end at different steps: as many sequences as
    two waves hold at this label count and a half, in an order that puts the longest in the middle of a wave."""
    rng = np.random.default_rng(70 + L)
    groups = 64 // max(2, 1 << (L - 1).bit_length())
    lengths = list(SEAM_LENGTHS) + [int(x) for x in rng.choice(SEAM_LENGTHS[:-1], size=max(0, 2 * groups + groups // 2 - 11))]
    rng.shuffle(lengths)
    return lengths


def make_batch(seed, L, lengths, integer=False):
    """Weights, a CSR batch, values and wide masks.  Every item carries 0 to 2 of the A shared attributes and, first, one
    attribute that no other item has: two items with equal attribute sets have equal score rows, and without values such
    twins make whole families of paths tie by symmetry (swap the twins' labels), which is the business of the exact tests
    with integer weights, not of the ones that compare under rounding."""
    rng = np.random.default_rng(seed)
    cptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(cptr[-1])
    if integer:
        w, trans = rng.integers(-2, 3, size=(A + n, L)).astype(float), rng.integers(-2, 3, size=(L, L)).astype(float)
    else:
        w, trans = rng.normal(0.0, 1.0, size=(A + n, L)), rng.normal(0.0, 1.5, size=(L, L))
    deg = rng.integers(1, 4, size=n)
    gptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    attr = rng.integers(0, A, size=int(gptr[-1])).astype(np.int32)
    attr[gptr[:-1]] = A + np.arange(n, dtype=np.int32)
    bits = rng.random((n, L)) < 0.7
    for i in np.flatnonzero(~bits.any(axis=1)):
        bits[i, int(rng.integers(0, L))] = True
    allowed = (bits.astype(np.uint64) << np.arange(L, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
    return dict(L=L, w=w, trans=trans, cptr=cptr, gptr=gptr, attr=attr, csr=(cptr, gptr, attr), v=rng.normal(0.0, 1.0, size=len(attr)),
                allowed=allowed)


@functools.lru_cache(maxsize=None)
def enumeration_batch(L):
    return make_batch(8500 + L, L, enumeration_lengths())


@functools.lru_cache(maxsize=None)
def seam_batch(L):
    return make_batch(8600 + L, L, seam_lengths(L))


def tables(b, valued, masked):
    """(item scores [n, L] with -inf where disallowed, the sums of the absolute values of their terms)."""
    n = int(b["cptr"][-1])
    every = tp.full_masks(n, b["L"])
    score = cr.masked_scores(b["gptr"], b["attr"], b["v"] if valued else None, b["w"], b["allowed"] if masked else every)
    absolute = cr.masked_scores(b["gptr"], b["attr"], np.abs(b["v"]) if valued else None, np.abs(b["w"]), every)
    return score, absolute


def reference(b, valued, masked, enumerate_all=False):
    """Per sequence (paths [m, T], scores [m], bounds [m], separated [m]) for m <= KMAX + 1 ranks: computed once per batch
    and kind, shared by every K (the order is total: the list of a smaller K is a prefix) and left unchanged."""
    key = ("ref", valued, masked, enumerate_all)
    if key not in b:
        score, absolute = tables(b, valued, masked)
        absT = np.abs(b["trans"])
        out = []
        for c in range(len(b["cptr"]) - 1):
            g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
            if g1 == g0:
                out.append(None)
                continue
            if enumerate_all:
                found = kr.enumerate_kbest(score[g0:g1], b["trans"], KMAX + 1)
                paths = np.array([p for p, _ in found], dtype=np.int64).reshape(len(found), g1 - g0)
                scores = np.array([s for _, s in found])
            else:
                paths, scores = kr.kbest(score[g0:g1], b["trans"], KMAX + 1)
            bounds = np.array([kr.bound(p, absolute[g0:g1], absT) for p in paths])
            out.append((paths, scores, bounds, kr.separated(scores, bounds)))
        b[key] = out
    return b[key]


def kw(b, valued, masked):
    return dict(values=b["v"] if valued else None, allowed=b["allowed"] if masked else None)


def accept(tag, b, ref, K, got, exact=False):
    """The acceptance of tests 1 and 3: n_paths, the empty ranks, scores within B, paths equal at every separated rank (exact:
    scores bit-equal and paths equal at every rank), and at most 1 % of the ranks unseparated."""
    y, sc, npaths, _ = got
    cptr = b["cptr"]
    assert y.shape == (int(cptr[-1]), K) and y.dtype == np.int8 and sc.shape == (len(cptr) - 1, K) and npaths.dtype == np.int32
    ranks = unseparated = 0
    worst = 0.0
    for c, r in enumerate(ref):
        g0, g1 = int(cptr[c]), int(cptr[c + 1])
        if r is None:
            assert npaths[c] == 0 and np.all(sc[c] == -np.inf), f"{tag}: an empty sequence has no path"
            continue
        paths, scores, bounds, sep = r
        m = min(K, len(scores))
        assert npaths[c] == m, f"{tag} sequence {c}: n_paths {npaths[c]}, expected {m}"
        assert np.all(y[g0:g1, m:] == -1) and np.all(sc[c, m:] == -np.inf), f"{tag} sequence {c}: empty ranks are -1 / -inf"
        for k in range(m):
            if exact:
                assert sc[c, k] == scores[k], f"{tag} sequence {c} rank {k}: score {sc[c, k]!r}, expected {scores[k]!r}"
            else:
                err = abs(sc[c, k] - scores[k])
                worst = max(worst, err / bounds[k] if bounds[k] > 0 else (0.0 if err == 0 else np.inf))
                assert err <= bounds[k], f"{tag} sequence {c} rank {k}: score off by {err:.3g}, B = {bounds[k]:.3g}"
            ranks += 1
            if exact or sep[k]:
                assert y[g0:g1, k].tolist() == paths[k].tolist(), f"{tag} sequence {c} rank {k}: another path"
            else:
                unseparated += 1
    print(f"{tag}: {ranks} ranks, {unseparated} unseparated, worst |score error| / B = {worst:.3g}")
    assert unseparated <= 0.01 * ranks, f"{tag}: choose another seed -- {unseparated} of {ranks} ranks are unseparated"


# ---------------------------------------------------------------- 1. enumeration
@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("L", [2, 3, 5])
def test_enumeration(nat, L, valued):
    b = enumeration_batch(L)
    assert {1, 2, 3, 6} <= set(np.diff(b["cptr"]).tolist()) and np.diff(b["cptr"])[20] == 0
    model = nat.Model.from_tables(b["w"], b["trans"])
    ref = reference(b, valued, False, enumerate_all=True)
    for K in (1, 2, 7, 32):
        got = model.viterbi_kbest(*b["csr"], K, **kw(b, valued, False))
        for c, T in enumerate(np.diff(b["cptr"]).tolist()):
            assert got[2][c] == min(K, L ** T if T else 0)
        accept(f"L={L} values={valued} K={K}", b, ref, K, got)


# ---------------------------------------------------------------- 2. ties, exactly
@pytest.mark.parametrize("L", [2, 3, 5, 8, 17, 32])
def test_ties_in_exact_arithmetic(nat, L):
    """Integer weights in -2 .. 2: every sum is exact, ties abound, and nothing is excused."""
    lengths = [1, 2, 3, 4, 5, 6, 0, 20, 40, 3, 2, 1, 33, 9] if L > 5 else [1, 2, 3, 4, 5, 6, 0, 3, 2, 1, 6, 5, 4]
    b = make_batch(8700 + L, L, lengths, integer=True)
    model = nat.Model.from_tables(b["w"], b["trans"])
    ref = reference(b, False, False, enumerate_all=L <= 5)
    for K in (1, 5, 32):
        accept(f"integer weights L={L} K={K}", b, ref, K, model.viterbi_kbest(*b["csr"], K), exact=True)


def test_an_all_zero_model_lists_every_path_in_reversed_lexicographic_order(nat):
    L, T, K = 3, 3, 27
    model = nat.Model.from_tables(np.zeros((A, L)), np.zeros((L, L)))
    cptr, gptr, attr = np.array([0, T], dtype=np.int32), np.arange(T + 1, dtype=np.int32), np.zeros(T, dtype=np.int32)
    y, sc, npaths, logz = model.viterbi_kbest(cptr, gptr, attr, K)
    assert npaths[0] == 27 and np.all(sc == 0.0)
    found = kr.enumerate_kbest(np.zeros((T, L)), np.zeros((L, L)), K)
    assert [tuple(y[:, k].tolist()) for k in range(K)] == [p for p, _ in found]
    assert [tuple(y[::-1, k].tolist()) for k in range(K)] == sorted(tuple(y[::-1, k].tolist()) for k in range(K))
    assert abs(logz[0] - T * np.log(L)) <= 1e-12


# ---------------------------------------------------------------- 3. the list recursion at the kernel's seams
@pytest.mark.parametrize("L", SEAM_LABELS)
def test_list_recursion_at_the_seams(nat, L):
    b = seam_batch(L)
    assert set(SEAM_LENGTHS) <= set(np.diff(b["cptr"]).tolist())
    model = nat.Model.from_tables(b["w"], b["trans"])
    ref = reference(b, True, False)
    for K in (1, 5, 32):
        accept(f"seams L={L} K={K}", b, ref, K, model.viterbi_kbest(*b["csr"], K, **kw(b, True, False)))


# ---------------------------------------------------------------- 4. rank 0 is Viterbi   5. the prefix property
@pytest.mark.parametrize("L", SEAM_LABELS)
def test_rank_0_is_viterbi_and_smaller_calls_are_prefixes(nat, L):
    b = seam_batch(L)
    model = nat.Model.from_tables(b["w"], b["trans"])
    absT = np.abs(b["trans"])
    for valued, masked in ((False, False), (True, False), (False, True)):
        y, sc, npaths, _ = model.viterbi_kbest(*b["csr"], 32, **kw(b, valued, masked))
        vy, vsc = model.viterbi(*b["csr"], **kw(b, valued, masked))
        assert np.ascontiguousarray(y[:, 0]).tobytes() == vy.tobytes(), f"values={valued} allowed={masked}: rank 0 is not Viterbi's path"
        _, absolute = tables(b, valued, masked)
        for c in range(len(npaths)):
            g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
            assert abs(sc[c, 0] - vsc[c]) <= kr.bound(vy[g0:g1].astype(np.int64), absolute[g0:g1], absT)
        for small in (1, 5):
            ys, scs, nps, _ = model.viterbi_kbest(*b["csr"], small, **kw(b, valued, masked))
            assert ys.tobytes() == np.ascontiguousarray(y[:, :small]).tobytes(), f"K'={small}: the paths are no prefix"
            assert scs.tobytes() == np.ascontiguousarray(sc[:, :small]).tobytes(), f"K'={small}: the scores are no prefix"
            assert np.array_equal(nps, np.minimum(npaths, small))


# ---------------------------------------------------------------- 6. masks
@pytest.mark.parametrize("L", [2, 3, 8, 17, 32])
def test_masks(nat, L):
    b = seam_batch(L) if L in SEAM_LABELS else make_batch(8600 + L, L, seam_lengths(L))
    model = nat.Model.from_tables(b["w"], b["trans"])
    cptr, n = b["cptr"], int(b["cptr"][-1])
    K = 32
    got = model.viterbi_kbest(*b["csr"], K, **kw(b, True, True))
    accept(f"masks L={L} K={K}", b, reference(b, True, True), K, got)
    y, sc, npaths, _ = got
    exists = np.arange(K)[None, :] < np.repeat(npaths, np.diff(cptr))[:, None]
    assert np.all(y[exists] >= 0) and np.all(y[~exists] == -1)
    assert np.all(((b["allowed"][:, None] >> np.where(exists, y, 0).astype(np.uint32)) & 1)[exists]), "a path carries a disallowed label"
    count = np.array([bin(int(m)).count("1") for m in b["allowed"]], dtype=object)
    for c in range(len(npaths)):
        total = int(np.prod(count[cptr[c]:cptr[c + 1]]))
        assert npaths[c] == min(K, total), f"sequence {c}: n_paths {npaths[c]} of {total} allowed paths"
    # singleton masks everywhere: one path, the pinned one
    pins = np.random.default_rng(L).integers(0, L, size=n)
    y1, sc1, np1, _ = model.viterbi_kbest(*b["csr"], 5, values=b["v"], allowed=(np.uint32(1) << pins.astype(np.uint32)))
    assert np.all(np1 == 1) and np.array_equal(y1[:, 0], pins) and np.all(y1[:, 1:] == -1) and np.all(sc1[:, 1:] == -np.inf)
    # every mask full: the bytes of the call without masks
    full = tp.full_masks(n, L)
    a = model.viterbi_kbest(*b["csr"], K, values=b["v"], allowed=full)
    e = model.viterbi_kbest(*b["csr"], K, values=b["v"])
    assert all(x.tobytes() == z.tobytes() for x, z in zip(a, e)), "full masks change the bytes"
    if L == 2:  # (without values a 2-label model's log Z comes from kernels of its own: the any-L comparison carries values of 1)
        ones = np.ones(len(b["attr"]))
        a = model.viterbi_kbest(*b["csr"], K, allowed=full)
        e = model.viterbi_kbest(*b["csr"], K, values=ones)
        assert all(x.tobytes() == z.tobytes() for x, z in zip(a, e))
        plain = model.viterbi_kbest(*b["csr"], K)
        assert all(x.tobytes() == z.tobytes() for x, z in zip(a[:3], plain[:3]))


# ---------------------------------------------------------------- 7. probabilities
def test_every_path_of_a_small_lattice_sums_to_one(nat):
    L, T, K = 2, 4, 16
    b = make_batch(8800, L, [T] * 9)
    model = nat.Model.from_tables(b["w"], b["trans"])
    for valued, masked in ((False, False), (True, False)):
        _, sc, npaths, logz = model.viterbi_kbest(*b["csr"], K, **kw(b, valued, masked))
        assert np.all(npaths == 16)
        total = np.exp(sc - logz[:, None]).sum(axis=1)
        print(f"values={valued}: worst |sum of p - 1| = {np.abs(total - 1).max():.3g}")
        assert np.all(np.abs(total - 1.0) <= 1e-12)


@pytest.mark.parametrize("L", SEAM_LABELS)
def test_probabilities_never_exceed_one_and_lognorm_is_the_marginals(nat, L):
    b = seam_batch(L)
    model = nat.Model.from_tables(b["w"], b["trans"])
    for valued, masked in ((False, False), (True, False), (True, True)):
        _, sc, _, logz = model.viterbi_kbest(*b["csr"], 32, **kw(b, valued, masked))
        _, elogz = model.marginals_full(*b["csr"], **kw(b, valued, masked))
        assert logz.tobytes() == elogz.tobytes(), f"values={valued} allowed={masked}: lognorm is not the marginals entry's"
        assert np.all(np.exp(sc - logz[:, None]).sum(axis=1) <= 1.0 + 1e-12)


def sequence_crf(w, trans):
    from gecco_amd.crfsuite_model import model_bytes
    from gecco_amd.sequence import SequenceCRF

    An, L = w.shape
    names, classes = [f"a{k}" for k in range(An)], [f"l{k}" for k in range(L)]
    blob = model_bytes(classes, names, np.repeat(np.arange(An), L), np.tile(np.arange(L), An), np.repeat(np.arange(L), L),
                       np.tile(np.arange(L), L), np.concatenate([w.ravel(), trans.ravel()]))
    return SequenceCRF.from_bytes(blob, window_size=None), names, classes


@pytest.mark.parametrize("L", [2, 5, 17])
def test_predict_kbest(nat, L):
    b = make_batch(8900 + L, L, [1, 2, 0, 9, 31, 64, 65, 3])
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = sequence_crf(w, b["trans"])
    cptr, gptr, attr = b["csr"]
    X = [[[names[a] for a in dict.fromkeys(attr[gptr[i]:gptr[i + 1]].tolist())] for i in range(cptr[s], cptr[s + 1])]
         for s in range(len(cptr) - 1)]
    out = crf.predict_kbest(X, 7)
    best = crf.predict(X)
    ll = crf.log_likelihood(X, best)
    assert len(out) == len(X) and sorted(out[2]) == ["log_probabilities", "paths", "scores"] and out[2]["paths"] == []
    assert out[2]["scores"].size == 0 and out[2]["log_probabilities"].size == 0
    for s, (o, T) in enumerate(zip(out, np.diff(cptr).tolist())):
        if T == 0:
            continue
        m = min(7, L ** T)
        assert len(o["paths"]) == m and o["scores"].shape == (m,) and o["log_probabilities"].shape == (m,)
        assert o["paths"][0] == best[s], "rank 0 is predict's path"
        assert np.all(np.diff(o["scores"]) <= 0) and np.all(o["log_probabilities"] <= 1e-12)
        assert abs(o["log_probabilities"][0] - ll[s]) <= 1e-12 * max(1.0, abs(o["scores"][0])), (s, o["log_probabilities"][0], ll[s])
        again = crf.log_likelihood([X[s]] * m, o["paths"])
        assert np.all(np.abs(again - o["log_probabilities"]) <= 1e-12 * np.maximum(1.0, np.abs(o["scores"])))
        assert all(set(p) <= set(classes) and len(p) == T for p in o["paths"])
    # with allowed sets the paths stay inside them
    allowed = [[{classes[0], classes[-1]} if t % 2 else None for t in range(T)] for T in np.diff(cptr).tolist()]
    for o, sets in zip(crf.predict_kbest(X, 4, allowed=allowed), allowed):
        assert all(a is None or lab in a for p in o["paths"] for lab, a in zip(p, sets))


# ---------------------------------------------------------------- 8. a slice
@pytest.mark.parametrize("L", [2, 5, 12])
def test_a_slice_gives_the_bytes_of_the_rebased_batch(nat, L):
    b = make_batch(9000 + L, L, [4, 9, 3, 30, 1, 0, 70])
    model = nat.Model.from_tables(b["w"], b["trans"])
    cptr, gptr, attr = b["csr"]
    g0 = int(cptr[2])
    a0 = int(gptr[g0])
    assert g0 > 0 and a0 > 0
    allowed = b["allowed"].copy()
    allowed[:g0] = 0  # (masks of genes outside the batch are not looked at)
    for kw_slice, kw_alone in ((dict(values=b["v"], allowed=allowed), dict(values=b["v"][a0:], allowed=allowed[g0:])), (dict(), dict())):
        got = model.viterbi_kbest(cptr[2:], gptr, attr, 7, **kw_slice)
        alone = model.viterbi_kbest(cptr[2:] - g0, gptr[g0:] - a0, attr[a0:], 7, **kw_alone)
        for x, z in zip(got, alone):
            assert x.size and x.tobytes() == z.tobytes()
        assert got[0].shape == (int(cptr[-1]) - g0, 7) and got[2][3] == 0 and np.isfinite(got[1][:, 0]).sum() == 4


def test_refusals_reach_the_caller(nat):
    b = make_batch(9100, 3, [3, 2])
    model = nat.Model.from_tables(b["w"], b["trans"])
    for k in (0, -1, 33):
        with pytest.raises(Exception, match=rf"viterbi_kbest: k = {k} is outside 1 \.\. 32"):
            model.viterbi_kbest(*b["csr"], k)


# ---------------------------------------------------------------- 9. the typed front end
def test_typed_front_end_lists_alternatives(nat, tmp_path):
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
    L, bg, K, M = len(crf.classes_), crf.classes_.index("0"), 4, 3
    # without the option, and with 0: the tables of a call that omits the argument, byte for byte, and no attribute
    plain_genes, plain_clusters = crf.predict_genes_and_clusters(genes)
    off_genes, off_clusters = crf.predict_genes_and_clusters(genes, alternatives=0)
    gs._dump(os.path.join(base, "plain"), crf, plain_genes, plain_clusters)
    gs._dump(os.path.join(base, "off"), crf, off_genes, off_clusters)
    gs._same_tables(os.path.join(base, "plain"), os.path.join(base, "off"))
    assert not any(hasattr(c, "alternatives") for c in off_clusters)
    for bad, text in ((33, "alternatives = 33 is outside 0 .. 32"), (-1, "alternatives = -1 is outside 0 .. 32"), (1.5, "are integers")):
        with pytest.raises(ValueError, match=text):
            crf.predict_clusters(genes, alternatives=bad)
    with pytest.raises(ValueError, match="alternatives_margin = -2 is negative"):
        crf.predict_clusters(genes, alternatives=2, alternatives_margin=-2)
    # the batch as the front end packs it, and the yardstick's tables for whole-contig path scores
    ordered = sorted(genes, key=operator.attrgetter("source.id", "start"))
    ids = [g.id for g in ordered]
    contigs = [list(g) for _, g in itertools.groupby(ordered, key=operator.attrgetter("source.id"))]
    batch = packing.pack_contigs(contigs, crf._attr_index, "protein")
    cptr, gptr, attr = batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id
    model = nat.Model.from_lcrf(crf._blob)
    score = cr.masked_scores(gptr, attr, None, model.state_weights()[0], tp.full_masks(int(cptr[-1]), L))
    trans = model.trans_weights()[0]
    best = model.viterbi(cptr, gptr, attr)[0].astype(np.int64)
    for margin in (M, 10):
        annotated, found = crf.predict_genes_and_clusters(genes, alternatives=K, alternatives_margin=margin)
        assert found and [c.id for c in found] == [c.id for c in plain_clusters]
        gs._dump(os.path.join(base, f"on{margin}"), crf, annotated, found)
        gs._same_tables(os.path.join(base, "plain"), os.path.join(base, f"on{margin}"))  # (clusters.tsv is unchanged)
        p_any = np.array([g.average_probability for g in annotated])
        worst, several = 0.0, 0
        for cl in found:
            first, last = ids.index(cl.genes[0].id), ids.index(cl.genes[-1].id) + 1
            c = int(np.searchsorted(cptr, first, side="right")) - 1
            c0, c1 = int(cptr[c]), int(cptr[c + 1])
            lo, hi = max(c0, first - margin - 1), min(c1, last + margin + 1)
            anchor = first + int(np.argmax(p_any[first:last])) - c0
            alts = cl.alternatives
            assert 1 <= len(alts) <= K and [a["rank"] for a in alts] == list(range(len(alts)))
            several += len(alts) > 1
            assert all(a["window"] == (lo - c0, hi - c0) and len(a["labels"]) == hi - lo for a in alts)
            assert all(x["log_p"] >= y["log_p"] for x, y in zip(alts, alts[1:])) and alts[0]["log_p"] <= 1e-12
            whole_best = best[c0:c1]
            s_best = kr.path_score(score[c0:c1], trans, whole_best)
            for a in alts:
                labels = np.array([crf.classes_.index(name) for name in a["labels"]], dtype=np.int64)
                whole = whole_best.copy()
                whole[lo - c0:hi - c0] = labels
                if lo > c0:
                    assert whole[lo - c0] == whole_best[lo - c0], "a copied end gene is pinned to the Viterbi path's label"
                if hi < c1:
                    assert whole[hi - 1 - c0] == whole_best[hi - 1 - c0]
                # the stated exactness: the ratio of two paths' probabilities is that of the whole-contig paths
                want = kr.path_score(score[c0:c1], trans, whole) - s_best + alts[0]["log_p"]
                worst = max(worst, abs(a["log_p"] - want))
                assert abs(a["log_p"] - want) <= 1e-9, (cl.id, a["rank"], a["log_p"], want)
                # the run around the anchor on the spliced path
                if whole[anchor] == bg:
                    assert a["run"] is None and a["start"] is None and a["end"] is None and a["type"] is None
                    continue
                x = z = anchor
                while x > 0 and whole[x - 1] != bg:
                    x -= 1
                while z + 1 < c1 - c0 and whole[z + 1] != bg:
                    z += 1
                assert a["run"] == (x, z + 1) and (a["start"], a["end"]) == (ordered[c0 + x].start, ordered[c0 + z].end)
                major = int(np.argmax(np.bincount(whole[x:z + 1], minlength=L)))
                assert a["type"] == (";".join(crf.label_types_[major]) or "Unknown")
            # rank 0 is the Viterbi path's reading
            assert [crf.classes_.index(name) for name in alts[0]["labels"]] == whole_best[lo - c0:hi - c0].tolist()
        print(f"margin {margin}: {len(found)} clusters, {several} with more than one reading, worst |log_p - whole-contig| = {worst:.3g}")
        assert several
    # the command line writes alternatives.tsv next to an unchanged clusters.tsv
    crf.save(os.path.join(base, "model"))
    done = subprocess.run([sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
                           os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv"),
                           "--alternatives", str(K), "-o", os.path.join(base, "cli")], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    gs._same_tables(os.path.join(base, "plain"), os.path.join(base, "cli"))
    with open(os.path.join(base, "cli", "alternatives.tsv")) as fh:
        lines = [line.rstrip("\n").split("\t") for line in fh]
    assert lines[0] == ["cluster_id", "rank", "start", "end", "type", "log_p", "p"]
    want = [[str(c.id), str(a["rank"]), "" if a["run"] is None else str(a["start"]), "" if a["run"] is None else str(a["end"]),
             a["type"] or "", repr(a["log_p"]), repr(float(np.exp(a["log_p"])))] for c in found for a in c.alternatives]
    assert [row[:6] for row in lines[1:]] == [row[:6] for row in want]
    assert all(abs(float(row[6]) - float(w[6])) <= 1e-15 for row, w in zip(lines[1:], want))
