"""Run-count posteriors on the device: ``gecco_crf_run_counts`` against the independent yardstick (tests/counts_reference.py: the
recursion over the saturating run counter, pinned on path enumeration by tests/test_counts_host.py), up through
``SequenceCRF.run_count_log_probability`` / ``predict_run_counts`` and the typed front end's ``predict_cluster_counts`` /
``predict_count_clusters``.

Two tiers, as in tests/test_gpu_minrun.py.  Exact (integer weights in -2 .. 2: every sum is exact and ties abound): every plane's
labels identical to the reference recursion and scores bit-equal, nothing excused -- the kernel scans its sources in the
reference's order -- and the largest of a sequence's scores has the bits of ``viterbi_kbest``'s rank 0.  Rounded (normal weights):
the device's OWN path is judged, so a near-tie is harmless and nothing is excused either: plane k has exactly k runs (at least K
in plane K), the device score is within B = 4 T eps (sum of |terms of the path|) of the left-to-right sum along it
(kbest_reference.bound), and it is no more than 2 B below the reference's best for the slot.  Every finite log Z_k is compared
with the reference recursion in ``numpy.longdouble`` under (T + 1)(2 L + 8) eps max(1, M), M the largest finite |forward value| of
the reference on the sequence (counts_reference.lognorm_bound derives it); -inf exactly where the reference has -inf; no NaN.

The seam grid runs every label count against every K.  A (label count, K) case takes the four label sets and the four kinds of
batch (plain, valued, masked, valued and masked) as a Latin square rotated by the case's position in the grid, so that every set
meets every kind at every label count and at every K, and a case stays at a second or two: the numpy yardstick is what costs
the time."""
import functools
import os

import numpy as np
import pytest

from tests import counts_reference as cn
from tests import kbest_reference as kr
from tests import test_gpu_kbest as gk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = [2, 3, 4, 8, 9, 16, 17, 32]
COUNTS = [1, 2, 3, 5, 16, 32]
KINDS = ((False, False), (True, False), (False, True), (True, True))  # (valued, masked)
WORST = {"ratio": 0.0}  # the largest |log Z_k - reference| / bound seen by this module's tests, printed by each


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


# ---------------------------------------------------------------- batches and the yardstick
def seams(K):
    """2 K - 1 is the shortest sequence that holds K runs: slot K first becomes reachable there."""
    return sorted({0, 1, 2, 3, 7, 8, 9, 2 * K - 1, 2 * K, 2 * K + 1, 64, 65, 300})


def seam_lengths(L, K):
    """The lengths at the kernel's seams, mixed so that the lane groups of a wave end at different steps: every seam length, and
    as many more as two waves and a half hold at this label count.  A leading sequence of 3 items stays outside the batch
    (``contig_ptr[0] > 0``)."""
    rng = np.random.default_rng(170 + 40 * L + K)
    at = seams(K)
    groups = 64 // max(2, 1 << (L - 1).bit_length())
    more = max(0, 2 * groups + groups // 2 - len(at))
    lengths = at + [int(x) for x in rng.choice([v for v in at if v < 64], size=more)]
    rng.shuffle(lengths)
    return [3] + lengths


@functools.lru_cache(maxsize=None)
def seam_batch(L, K, integer):
    return gk.make_batch(9700 + 40 * L + K + 5000 * integer, L, seam_lengths(L, K), integer=integer)


def label_sets(L):
    """One label; all but label 0; the top labels only; every label."""
    return [1 << (L // 2), ((1 << L) - 1) & ~1, ((1 << L) - 1) & ~((1 << (L - (L + 1) // 2)) - 1), (1 << L) - 1]


def call(model, b, mask, K, valued, masked, first=1, **more):
    """The batch from sequence `first` on: contig_ptr[0] > 0 where first > 0."""
    return model.run_counts(b["cptr"][first:], b["gptr"], b["attr"], mask, K, **gk.kw(b, valued, masked), **more)


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


def lse(v):
    v = np.asarray(v)
    top = v.max()
    return top if top == -np.inf else top + np.log(np.exp(v - top).sum())


def check_mass(tag, got, want, largest, T, L):
    """Every slot of one sequence: |log Z_k - reference| under the derived bound, -inf exactly where the reference has it;
    returns the worst ratio."""
    assert not np.isnan(got).any(), f"{tag}: NaN in log_mass"
    bound = cn.lognorm_bound(T, L, largest)
    worst = 0.0
    for k in range(len(want)):
        if want[k] == -np.inf:
            assert got[k] == -np.inf, f"{tag} slot {k}: log Z_k {got[k]!r}, expected -inf"
            continue
        err = abs(float(np.longdouble(got[k]) - want[k]))
        assert np.isfinite(got[k]) and err <= bound, \
            f"{tag} slot {k}: log Z_k off by {err:.3g}, bound {bound:.3g} (T={T}, L={L}, M={largest:.3g})"
        worst = max(worst, err / bound)
    WORST["ratio"] = max(WORST["ratio"], worst)
    return worst


def judge(tag, b, mask, K, valued, masked, got, exact, base=1):
    """The acceptance of one call against the yardstick, sequence by sequence; `base`: the first sequence of the call."""
    mass, sc, y, lz = got
    L = b["L"]
    score, absolute = gk.tables(b, valued, masked)
    absT = np.abs(b["trans"])
    g_base = int(b["cptr"][base])
    nc = len(b["cptr"]) - 1 - base
    assert y.dtype == np.int8 and y.shape == (K + 1, int(b["cptr"][-1]) - g_base) and mass.shape == sc.shape == (nc, K + 1)
    assert lz.shape == (nc,) and not np.isnan(sc).any() and not np.isnan(mass).any()
    first = np.array([0.0] + [-np.inf] * K)
    worst_b = worst_z = 0.0
    for c, g0, g1 in sequences(b, base):
        T = g1 - g0
        where = f"{tag} sequence {c} (T={T})"
        if T == 0:
            assert np.array_equal(sc[c], first) and np.array_equal(mass[c], first) and lz[c] == 0.0, \
                f"{where}: an empty sequence has the empty path in slot 0 and nothing else"
            continue
        paths, best = cn.recursion(score[g0:g1], b["trans"], mask, K)
        z, largest = cn.recursion(score[g0:g1], b["trans"], mask, K, "sum")
        for k in range(K + 1):
            mine = y[k, g0 - g_base:g1 - g_base].astype(np.int64)
            if paths[k] is None:
                assert np.all(mine == -1) and sc[c, k] == -np.inf, f"{where} slot {k}: no path is -1 / -inf"
                continue
            runs = cn.n_runs(mine, mask) if np.all(mine >= 0) else -1
            assert runs >= K if k == K else runs == k, f"{where} slot {k}: the device's path has {runs} runs"
            if exact:
                assert mine.tolist() == paths[k].tolist(), f"{where} slot {k}: another path than the reference recursion's"
                assert sc[c, k] == best[k], f"{where} slot {k}: score {sc[c, k]!r}, expected {best[k]!r}"
            else:
                B = kr.bound(mine, absolute[g0:g1], absT)
                along = kr.path_score(score[g0:g1], b["trans"], mine)
                assert abs(sc[c, k] - along) <= B, f"{where} slot {k}: score off its own path's sum by {abs(sc[c, k] - along):.3g}, B = {B:.3g}"
                assert sc[c, k] >= best[k] - 2.0 * B, f"{where} slot {k}: score {sc[c, k]!r} is more than 2 B below the reference's {best[k]!r}"
                worst_b = max(worst_b, abs(sc[c, k] - along) / B if B > 0 else 0.0)
        worst_z = max(worst_z, check_mass(where, mass[c], z, largest, T, L))
        # the recursion's own total is log Z
        total = lse(mass[c])
        assert abs(total - lz[c]) <= (K + 2) * cn.lognorm_bound(T, L, max(largest, abs(lz[c]))), \
            f"{where}: the slots add up to {total!r}, log Z is {lz[c]!r}"
    return worst_b, worst_z


def close(a, b):
    """Equal up to the rounding of a log-sum-exp over a row, -inf where the other has -inf."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isneginf(a), np.isneginf(b)) and np.allclose(a, b, rtol=0, atol=1e-13)


def same_bytes(a, b):
    return all((x is None and z is None) or x.tobytes() == z.tobytes() for x, z in zip(a, b))


# ---------------------------------------------------------------- 1. the seams
@pytest.mark.parametrize("K", COUNTS)
@pytest.mark.parametrize("L", LABELS)
def test_seams(nat, L, K):
    turn = LABELS.index(L) + COUNTS.index(K)
    sets = label_sets(L)
    for exact in (True, False):
        b = seam_batch(L, K, exact)
        lengths = np.diff(b["cptr"])[1:].tolist()
        assert set(seams(K)) <= set(lengths) and b["cptr"][1] > 0
        assert len(lengths) >= 2 * (64 // max(2, 1 << (L - 1).bit_length())) + 1
        model = nat.Model.from_tables(b["w"], b["trans"])
        for s, mask in enumerate(sets):
            valued, masked = KINDS[(s + turn) % 4]
            tag = f"L={L} K={K} set={mask:#x} values={valued} allowed={masked} exact={exact}"
            got = call(model, b, mask, K, valued, masked)
            worst_b, worst_z = judge(tag, b, mask, K, valued, masked, got, exact)
            print(f"{tag}: worst |score - own path| / B = {worst_b:.3g}, worst |log Z_k error| / bound = {worst_z:.3g}")
            # asking for the log-masses changes no byte of score and y, and the reverse; equal calls give equal bytes
            bare = call(model, b, mask, K, valued, masked, want_log_mass=False)
            assert bare[0] is None and same_bytes(bare[1:], got[1:]), f"{tag}: log_mass changes score, y or lognorm"
            bare = call(model, b, mask, K, valued, masked, want_paths=False)
            assert bare[1] is None and bare[2] is None and same_bytes(bare[::3], got[::3]), f"{tag}: the paths change log_mass"
            assert same_bytes(call(model, b, mask, K, valued, masked), got), f"{tag}: equal calls, other bytes"
            # log Z is the marginals entry's
            csr0, kw0 = rebased(b, valued, masked)
            _, elogz = model.marginals_full(*csr0, **kw0)
            assert got[3].tobytes() == elogz.tobytes(), f"{tag}: lognorm is not the marginals entry's"
            # the best of all paths is the best of some slot: the same left-to-right sum, the same bits
            _, ksc, _, _ = model.viterbi_kbest(*csr0, 1, **kw0)
            full = np.diff(b["cptr"])[1:] > 0
            assert np.array_equal(got[1].max(axis=1)[full], ksc[full, 0]), f"{tag}: the largest score is not viterbi_kbest's rank 0"
    print(f"largest |log Z_k - reference| / bound so far: {WORST['ratio']:.3g}")


# ---------------------------------------------------------------- 2. enumeration on small shapes
@pytest.mark.parametrize("L,longest", [(2, 9), (3, 6)])
def test_enumeration(nat, L, longest):
    lengths = list(range(1, longest + 1)) * 2 + [0]
    rng = np.random.default_rng(80 + L)
    for integer in (True, False):
        b = gk.make_batch(9800 + L + 100 * integer, L, lengths, integer=integer)
        model = nat.Model.from_tables(b["w"], b["trans"])
        for K in (1, 2, 3, 4):
            for mask in ((1 << L) - 1, int(rng.integers(1, 1 << L))):
                valued, masked = KINDS[int(rng.integers(0, 4))]
                score, absolute = gk.tables(b, valued, masked)
                mass, sc, y, lz = call(model, b, mask, K, valued, masked, first=0)
                for c, g0, g1 in sequences(b, 0):
                    if g1 == g0:
                        continue
                    best, arg, logz, count = cn.enumerate_paths(score[g0:g1], b["trans"], mask, K)
                    where = f"L={L} K={K} set={mask:#x} values={valued} allowed={masked} integer={integer} sequence {c}"
                    _, largest = cn.recursion(score[g0:g1], b["trans"], mask, K, "sum")
                    check_mass(where, mass[c], logz, largest, g1 - g0, L)
                    for k in range(K + 1):
                        mine = y[k, g0:g1].astype(np.int64)
                        if count[k] == 0:
                            assert np.all(mine == -1) and sc[c, k] == -np.inf, (where, k)
                        elif integer:  # (every sum is exact: enumeration's best score, and one of the paths that have it)
                            assert sc[c, k] == best[k] and tuple(mine.tolist()) in arg[k], (where, k)
                        else:          # (the device adds up an item's score in its own order: its own path is judged)
                            B = kr.bound(mine, absolute[g0:g1], np.abs(b["trans"]))
                            runs = cn.n_runs(mine, mask)
                            assert np.all(mine >= 0) and (runs >= K if k == K else runs == k), (where, k)
                            assert abs(sc[c, k] - kr.path_score(score[g0:g1], b["trans"], mine)) <= B and sc[c, k] >= best[k] - 2.0 * B, (where, k)
    print(f"largest |log Z_k - reference| / bound so far: {WORST['ratio']:.3g}")


# ---------------------------------------------------------------- 3. planted cases
def planted_model(nat, score, trans):
    """A model whose item scores are `score`: one private attribute per item."""
    T = len(score)
    cptr, gptr, attr = np.array([0, T], dtype=np.int32), np.arange(T + 1, dtype=np.int32), np.arange(T, dtype=np.int32)
    return nat.Model.from_tables(np.asarray(score, dtype=float), np.asarray(trans, dtype=float)), (cptr, gptr, attr)


def test_the_best_path_with_one_run_is_not_the_free_path_pruned(nat):
    """Two strong runs across a weak gap: the best single run bridges the gap, where deleting the weaker run keeps one of the
    two only."""
    ones = [-3, 3, 3, -3.5, 3, 3, -3, -3]
    trans = np.array([[0.5, -1.0], [-1.0, 0.5]])
    score = np.stack([np.zeros(len(ones)), np.array(ones, dtype=float)], axis=1)
    model, csr = planted_model(nat, score, trans)
    assert model.viterbi(*csr)[0].tolist() == [0, 1, 1, 0, 1, 1, 0, 0]
    best, arg, logz, _ = cn.enumerate_paths(score, trans, 2, 2)
    assert arg[1] == [(0, 1, 1, 1, 1, 1, 0, 0)] and arg[2] == [(0, 1, 1, 0, 1, 1, 0, 0)] and arg[0] == [(0,) * 8]
    mass, sc, y, lz = model.run_counts(*csr, 2, 2)
    assert y.tolist() == [list(p[0]) for p in arg] and sc[0].tolist() == best.tolist()
    check_mass("planted", mass[0], logz, cn.recursion(score, trans, 2, 2, "sum")[1], len(ones), 2)
    assert abs(lse(mass[0]) - lz[0]) <= 1e-12


def test_infeasible_counts(nat):
    b = gk.make_batch(9900, 3, [1, 2, 3, 0, 5, 2])
    model = nat.Model.from_tables(b["w"], b["trans"])
    lengths = np.diff(b["cptr"])
    # every label in the set: exactly one run, whatever the length
    mass, sc, y, lz = model.run_counts(*b["csr"], 7, 3)
    for c, T in enumerate(lengths.tolist()):
        if T:
            assert np.all(np.isinf(mass[c, [0, 2, 3]])) and np.all(np.isinf(sc[c, [0, 2, 3]])) and abs(mass[c, 1] - lz[c]) <= 1e-12
            g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
            assert np.all(y[[0, 2, 3], g0:g1] == -1) and np.all(y[1, g0:g1] >= 0)
    # more runs than ceil(T / 2)
    mass, sc, y, lz = model.run_counts(*b["csr"], 2, 3)
    for c, T in enumerate(lengths.tolist()):
        for k in range(4):
            assert (mass[c, k] > -np.inf) == (sc[c, k] > -np.inf) == (k <= (T + 1) // 2), (c, T, k)
    # masks that allow no label of the set: no run, and slot 0 is all of log Z
    only0 = np.full(int(b["cptr"][-1]), 1, dtype=np.uint32)
    mass, sc, y, lz = model.run_counts(*b["csr"], 6, 2, allowed=only0)
    assert np.all(np.isinf(mass[:, 1:])) and np.all(y[0] == 0) and np.all(y[1:] == -1) and not np.isnan(mass).any()
    assert np.all(np.abs(mass[:, 0] - lz) <= 1e-12) and np.all(np.abs(sc[:, 0] - lz) <= 1e-12)  # (one path)


def test_state_scores_of_700_per_item(nat):
    """exp(700 T) overflows and exp(-700 T) underflows: every log Z_k that exists is finite all the same, never NaN."""
    L, T = 3, 40
    rng = np.random.default_rng(19)
    for sign in (1.0, -1.0):
        score = sign * 700.0 + rng.normal(0.0, 1.0, size=(T, L))
        score[::3] *= -1.0  # (and a mix of both)
        trans = rng.normal(0.0, 1.5, size=(L, L))
        model, csr = planted_model(nat, score, trans)
        for mask, K in ((6, 3), (7, 5), (2, 32)):
            mass, sc, y, lz = model.run_counts(*csr, mask, K)
            z, largest = cn.recursion(score, trans, mask, K, "sum")
            ratio = check_mass(f"sign {sign} set {mask} K {K}", mass[0], z, largest, T, L)
            print(f"sign {sign} set {mask} K {K}: |error| / bound = {ratio:.3g}")
            assert abs(lse(mass[0]) - lz[0]) <= (K + 2) * cn.lognorm_bound(T, L, largest)


def test_refusals_reach_the_caller(nat):
    b = gk.make_batch(9950, 3, [3, 2])
    model = nat.Model.from_tables(b["w"], b["trans"])
    for bad in (0, -1, 33):
        with pytest.raises(Exception, match=rf"run_counts: max_runs = {bad} is outside 1 \.\. 32"):
            model.run_counts(*b["csr"], 6, bad)
    for bad in (0, 8):
        with pytest.raises(Exception, match="set_mask"):
            model.run_counts(*b["csr"], bad, 2)
    with pytest.raises(Exception, match="all NULL"):
        model.run_counts(*b["csr"], 6, 2, want_log_mass=False, want_paths=False)


# ---------------------------------------------------------------- 4. SequenceCRF
@pytest.mark.parametrize("L", [2, 5, 17])
def test_sequence_front_end(nat, L):
    b = gk.make_batch(9960 + L, L, [1, 2, 0, 9, 31, 64, 65, 3])
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = gk.sequence_crf(w, b["trans"])
    cptr, gptr, attr = b["csr"]
    # dict items: every attribute with a value of its own
    X = [[{names[a]: float(b["v"][e]) for e, a in zip(range(gptr[i], gptr[i + 1]), attr[gptr[i]:gptr[i + 1]].tolist())}
          for i in range(cptr[s], cptr[s + 1])] for s in range(len(cptr) - 1)]
    inside, K = classes[1:], 4
    seq_ptr, item_ptr, ids, values = crf._pack(X)
    assert values is not None
    mass, sc, y, lz = crf._model.run_counts(seq_ptr, item_ptr, ids, (1 << L) - 2, K, values=values)
    lp = crf.run_count_log_probability(X, inside, K)
    assert lp.shape == (len(X), K + 1) and lp.dtype == np.float64
    want = mass - np.array([lse(row) for row in mass])[:, None]
    assert close(lp, want) and close(crf.run_count_probability(X, inside, K), np.exp(want))
    assert np.all(np.abs(np.exp(lp).sum(axis=1) - 1.0) <= 1e-12) and lp[2].tolist() == [0.0] + [-np.inf] * K
    # the mean of the distribution is expected_runs where the tail slot is empty
    mean = (np.exp(crf.run_count_log_probability(X, inside, 32)) * np.arange(33)).sum(axis=1)
    short = np.diff(cptr) < 63
    assert np.allclose(mean[short], crf.expected_runs(X, [inside])[short, 0], rtol=0, atol=1e-9)
    out = crf.predict_run_counts(X, inside, K)
    assert len(out) == len(X) and all(sorted(o) == ["log_probabilities", "paths", "scores"] for o in out)
    assert out[2]["paths"] == [[]] + [None] * K and out[2]["scores"].tolist() == [0.0] + [-np.inf] * K
    best = crf.predict(X)
    for s, (o, T) in enumerate(zip(out, np.diff(cptr).tolist())):
        if T == 0:
            continue
        assert np.array_equal(o["scores"], sc[s]) and np.array_equal(o["log_probabilities"], sc[s] - lz[s])
        for k, path in enumerate(o["paths"]):
            if path is None:
                assert sc[s, k] == -np.inf and k > 0
                continue
            assert path == [classes[c] for c in y[k, cptr[s]:cptr[s + 1]].tolist()]
            runs = cn.n_runs([classes.index(name) for name in path], (1 << L) - 2)
            assert runs >= K if k == K else runs == k
            again = crf.log_likelihood([X[s]], [path])[0]
            assert abs(again - o["log_probabilities"][k]) <= 1e-12 * max(1.0, abs(o["scores"][k]))
        assert o["paths"][int(np.argmax(o["scores"]))] == best[s], "the best of the slots is predict's path"
    # with allowed sets every path stays inside them
    allowed = [[{classes[0], classes[-1]} if t % 2 else None for t in range(T)] for T in np.diff(cptr).tolist()]
    for o, sets in zip(crf.predict_run_counts(X, inside, 2, allowed=allowed), allowed):
        for path in o["paths"]:
            assert path is None or all(a is None or lab in a for lab, a in zip(path, sets))


# ---------------------------------------------------------------- 5. the typed front end
def test_typed_front_end_counts_clusters(nat, tmp_path):
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
    L, bg, K = len(crf.classes_), crf.classes_.index("0"), 5
    ordered = sorted(genes, key=operator.attrgetter("source.id", "start"))
    contigs = [list(g) for _, g in itertools.groupby(ordered, key=operator.attrgetter("source.id"))]
    batch = packing.pack_contigs(contigs, crf._attr_index, "protein")
    cptr, gptr, attr = batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id
    model = nat.Model.from_lcrf(crf._blob)
    S = ((1 << L) - 1) & ~(1 << bg)
    mass, sc, y, lz = model.run_counts(cptr, gptr, attr, S, K)
    rows = crf.predict_cluster_counts(genes, max_clusters=K)
    names = typed.count_columns(K)
    assert rows is crf.cluster_counts_ and tuple(rows) == names and names[2:-1] == ("p_0", "p_1", "p_2", "p_3", "p_4", "p_ge_5")
    assert rows["sequence_id"] == [c[0].source.id for c in contigs] and rows["genes"] == np.diff(cptr).tolist()
    p = np.array([rows[name] for name in names[2:-1]]).T
    assert close(p, np.exp(mass - np.array([lse(r) for r in mass])[:, None]))
    for ci, T in enumerate(np.diff(cptr).tolist()):
        # (K + 1 slots, each off by at most the bound relative to its value: the row sums to 1 within (K + 1) times the bound)
        assert abs(p[ci].sum() - 1.0) <= (K + 1) * cn.lognorm_bound(T, L, float(np.abs(mass[ci][np.isfinite(mass[ci])]).max()))
        assert rows["map_clusters"][ci] == int(np.argmax(p[ci])) and p[ci][rows["map_clusters"][ci]] == p[ci].max()
    # exactly one cluster per contig
    found = crf.predict_count_clusters(genes, n_clusters=1)
    _, sc2, y2, _ = model.run_counts(cptr, gptr, attr, S, 2, want_log_mass=False)
    assert crf.count_scores_ == sc2[:, 1].tolist() and len(found) == len(contigs)
    ids = [g.id for g in ordered]
    for ci, (contig, cluster) in enumerate(zip(contigs, found)):
        assert cluster.id == f"{contig[0].source.id}_cluster_1"
        first, last = ids.index(cluster.genes[0].id), ids.index(cluster.genes[-1].id) + 1
        plane = y2[1, cptr[ci]:cptr[ci + 1]]
        assert cn.n_runs(plane, S) == 1, "plane 1 holds exactly one run"
        assert np.all(y2[1, first:last] != bg) and np.count_nonzero(plane != bg) == last - first
        major = int(np.argmax(np.bincount(y2[1, first:last].astype(np.int64), minlength=L)))
        assert cluster.path_type == (";".join(crf.label_types_[major]) or "Unknown")
    assert crf.predict_count_clusters(genes, n_clusters=0) == [] and all(np.isfinite(crf.count_scores_))
    two = crf.predict_count_clusters(genes, n_clusters=2)
    assert len(two) == 2 * len(contigs) and [c.id for c in two[:2]] == [f"{contigs[0][0].source.id}_cluster_{k}" for k in (1, 2)]
    # the command line: both files with the flags, and the other tables byte for byte what they are without them
    crf.save(os.path.join(base, "model"))
    common = ["predict", "--model", os.path.join(base, "model"), "--genes", os.path.join(base, "fresh", "genes.tsv"), "--features",
              os.path.join(base, "fresh", "features.tsv")]
    assert typed.main(common + ["-o", os.path.join(base, "plain")]) == 0
    assert typed.main(common + ["--cluster-counts", str(K), "--exact-clusters", "1", "-o", os.path.join(base, "cli")]) == 0
    assert sorted(os.listdir(os.path.join(base, "cli"))) == sorted(os.listdir(os.path.join(base, "plain")) + ["cluster_counts.tsv", "count_clusters.tsv"])
    for name in os.listdir(os.path.join(base, "plain")):
        assert open(os.path.join(base, "plain", name), "rb").read() == open(os.path.join(base, "cli", name), "rb").read(), name
    with open(os.path.join(base, "cli", "cluster_counts.tsv")) as fh:
        lines = [line.rstrip("\n").split("\t") for line in fh]
    assert lines[0] == list(names) and [row[0] for row in lines[1:]] == rows["sequence_id"]
    assert [int(row[-1]) for row in lines[1:]] == rows["map_clusters"] and [float(row[3]) for row in lines[1:]] == rows["p_1"]
    with open(os.path.join(base, "cli", "count_clusters.tsv")) as fh:
        lines = [line.rstrip("\n").split("\t") for line in fh]
    assert lines[0] == ["sequence_id", "cluster_id", "start", "end", "genes", "type"]
    assert [row[1] for row in lines[1:]] == [c.id for c in found] and [int(row[4]) for row in lines[1:]] == [len(c.genes) for c in found]
