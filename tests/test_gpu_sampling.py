"""Label paths drawn from the posterior on the device: ``gecco_crf_sample_paths`` against the independent numpy yardstick
(tests/sampling_reference.py), through every whole-contig arrangement, and up through ``SequenceCRF`` and the typed front end.

The rule is checked exactly, draw by draw: the teacher-forced checker takes the device's label of the item behind, forms the
reference's running sums and requires the device's label, excusing a draw only when its u lies within 1e-9 of the boundary
between the two labels.  At most 4 draws of a case, and never more than 1e-6 of them, may be excused; the reference's own count
of draws that close to a boundary is held to the same cap, so a seed cannot hide a defect behind excuses.  (Checked on the CPU
with the reference alone: 6e6 draws per label count gave 0 to 1 draws inside the margin.)

The distribution is checked end to end at N = 4096: every frequency within ``6 sqrt(p (1 - p) / N) + 2 / N`` of the exact
probability (six standard deviations plus two counts); the reference sampler's worst deviation on the CPU was 4.7 sigma over
the five label counts.  Every test prints its worst ratio to the bound."""
import itertools
import operator
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import sampling_reference as sr
from tests import test_gpu_spans as gs
from tests import train_objective_partial as tp

pytestmark = pytest.mark.gpu

LABELS = [2, 3, 8, 17, 32]
A = gs.A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(False, False), (True, False), (False, True), (True, True)]  # (with values, with allowed masks)


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


def _kw(b, valued, masked):
    return dict(values=b["v"] if valued else None, allowed=b["allowed"] if masked else None)


def _exact(tag, y, b, score, seed):
    """The teacher-forced check of the paths `y` with its caps; returns the number of excused draws."""
    excused, near, draws = sr.check_teacher_forced(y, b["cptr"], score, b["trans"], seed)
    cap = min(4, int(1e-6 * draws))
    print(f"{tag}: {draws} draws, {excused} excused, {near} within 1e-9 of a boundary (cap {cap})")
    assert near <= cap, f"{tag}: choose another seed -- the reference itself has {near} draws inside the margin"
    assert excused <= cap, tag
    return excused


def _bound(p, N):
    return 6.0 * np.sqrt(p * (1.0 - p) / N) + 2.0 / N


# ---------------------------------------------------------------- 1. the rule, exactly
@pytest.mark.parametrize("valued,masked", KINDS)
@pytest.mark.parametrize("L", LABELS)
def test_the_rule_exactly(nat, L, valued, masked):
    b = gs._batch(L)
    n, N, seed = int(b["cptr"][-1]), 200, 1000 + 10 * L + 2 * valued + masked
    model = nat.Model.from_tables(b["w"], b["trans"])
    y, marg, logz = model.sample_paths(*b["csr"], N, seed=seed, want_marginals=True, **_kw(b, valued, masked))
    assert y.shape == (n, N) and y.dtype == np.int8
    _exact(f"L={L} values={valued} allowed={masked} N={N}", y, b, gs._score(b, valued, masked), seed)
    emarg, elogz = model.marginals_full(*b["csr"], **_kw(b, valued, masked))
    assert marg.tobytes() == emarg.tobytes() and logz.tobytes() == elogz.tobytes(), "want_marginals: marginals_full's bytes"
    if masked:
        assert np.all((b["allowed"][:, None] >> y.astype(np.uint32)) & 1), "a draw carries a disallowed label"


@pytest.mark.parametrize("N", [1, 64, 65])
def test_the_rule_at_the_edges_of_a_wave(nat, N):
    L, seed = 3, 2000 + N
    b = gs._batch(L)
    model = nat.Model.from_tables(b["w"], b["trans"])
    y = model.sample_paths(*b["csr"], N, seed=seed, **_kw(b, True, True))
    assert y.shape == (int(b["cptr"][-1]), N)
    _exact(f"L={L} N={N}", y, b, gs._score(b, True, True), seed)


# ---------------------------------------------------------------- 2. every whole-contig arrangement
@pytest.mark.parametrize("L,switch,mode", gs.ARRANGEMENTS)
def test_every_whole_contig_arrangement(nat, monkeypatch, L, switch, mode):
    lengths = gs._arrangement_lengths()
    assert {63, 64, 65, 66, 127, 128, 129, 300} <= set(lengths)
    b = gs._batch(L, lengths, 40)
    monkeypatch.setenv(switch, mode)
    model = nat.Model.from_tables(b["w"], b["trans"])
    for valued, masked in ((True, True), (False, False)):
        seed = 3000 + 10 * L + masked
        y, marg, logz = model.sample_paths(*b["csr"], 200, seed=seed, want_marginals=True, **_kw(b, valued, masked))
        _exact(f"L={L} {switch}={mode} values={valued} allowed={masked}", y, b, gs._score(b, valued, masked), seed)
        emarg, elogz = model.marginals_full(*b["csr"], **_kw(b, valued, masked))
        assert marg.tobytes() == emarg.tobytes() and logz.tobytes() == elogz.tobytes()


# ---------------------------------------------------------------- 3. exact properties
@pytest.mark.parametrize("L", [2, 8, 17])
def test_draws_are_a_function_of_the_seed_and_the_position(nat, L):
    b = gs._batch(L)
    model = nat.Model.from_tables(b["w"], b["trans"])
    seed = (0xDEADBEEF << 32) | 0x12345678  # (both key words in use)
    y = model.sample_paths(*b["csr"], 200, seed=seed)
    assert model.sample_paths(*b["csr"], 200, seed=seed).tobytes() == y.tobytes(), "the same seed gives the same bytes"
    for other in (seed + 1, seed ^ (1 << 40), 0):
        assert model.sample_paths(*b["csr"], 200, seed=other).tobytes() != y.tobytes(), "another seed gives other bytes"
    few = model.sample_paths(*b["csr"], 64, seed=seed)
    assert few.tobytes() == np.ascontiguousarray(y[:, :64]).tobytes(), "sample s does not depend on n_samples"
    _exact(f"L={L} a 64-bit seed", y, b, gs._score(b, False, False), seed)


@pytest.mark.parametrize("L", [3, 17])
def test_a_transition_of_minus_2000_never_occurs_and_a_lead_of_800_always_wins(nat, L):
    rng = np.random.default_rng(9700 + L)
    k, special, N = 1, A - 1, 256
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.0, size=(L, L))
    trans[0, 2] = -2000.0
    w[special] = 0.0
    w[special, k] = 800.0 + 2.0 * np.abs(w).sum(axis=0).max()  # (a lead of at least 800 whatever else the item carries)
    lengths = [12, 1, 40, 70, 5]
    leaders = [5, 0, 39, 0, 2]  # the item of every contig that carries the attribute
    cptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    deg = rng.integers(1, 4, size=int(cptr[-1]))
    rows = [list(rng.integers(0, A - 1, size=d)) for d in deg]
    for c, p in enumerate(leaders):
        rows[int(cptr[c]) + p].append(special)
    gptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    attr = np.array([a for r in rows for a in r], dtype=np.int32)
    y = nat.Model.from_tables(w, trans).sample_paths(cptr, gptr, attr, N, seed=5)
    inner = np.ones(len(y) - 1, dtype=bool)
    inner[cptr[1:-1] - 1] = False  # (pairs that straddle two contigs are no transitions)
    assert not np.any((y[:-1] == 0) & (y[1:] == 2) & inner[:, None]), "a transition of weight -2000 was drawn"
    assert np.any(y == 0) and np.any(y == 2)
    for c, p in enumerate(leaders):
        assert np.all(y[int(cptr[c]) + p] == k), "a label that leads by 800 was not drawn"
    score = cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L))
    _exact(f"L={L} extreme weights", y, dict(cptr=cptr, trans=trans), score, 5)


def test_one_item_empty_contigs_and_a_slice(nat):
    L, N = 5, 100
    rng = np.random.default_rng(9800)
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    model = nat.Model.from_tables(w, trans)
    # a sequence of one item: the draw is from its marginal's running sums
    cptr, gptr, attr = gs._csr(rng, [1])
    y, marg, _ = model.sample_paths(cptr, gptr, attr, 4096, seed=3, want_marginals=True)
    assert y.shape == (1, 4096)
    freq = np.bincount(y[0], minlength=L) / 4096
    assert np.all(np.abs(freq - marg[0]) <= _bound(marg[0], 4096))
    # empty contigs, at both ends too
    cptr, gptr, attr = gs._csr(rng, [0, 4, 0, 0, 9, 3, 0])
    score = cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L))
    y, marg, logz = model.sample_paths(cptr, gptr, attr, N, seed=4, want_marginals=True)
    emarg, elogz = model.marginals_full(cptr, gptr, attr)
    assert marg.tobytes() == emarg.tobytes() and logz.tobytes() == elogz.tobytes() and logz[0] == 0.0 and logz[-1] == 0.0
    _exact("empty contigs", y, dict(cptr=cptr, trans=trans), score, 4)
    # a batch without genes
    out = model.sample_paths(np.zeros(3, dtype=np.int32), gptr, attr, N, seed=4, want_marginals=True)
    assert out[0].shape == (0, N) and out[1].shape == (0, L) and np.all(out[2] == 0.0) and out[2].shape == (2,)
    # contig_ptr[0] > 0: the bytes of the rebased batch, whose contig indices (the Philox counter's) start at 0 as well
    cptr, gptr, attr = gs._csr(rng, [4, 9, 3, 30, 1, 70])
    v, allowed = gs._values(rng, len(attr)), gs._wide_masks(rng, int(cptr[-1]), L)
    g0 = int(cptr[2])
    a0 = int(gptr[g0])
    allowed[:g0] = 0  # (masks of genes outside the batch are not looked at)
    runs = ([0, 1, 3, 3], [2, 29, 0, 69], [3, 30, 1, 16])
    for kw_slice, kw_alone in ((dict(values=v, allowed=allowed), dict(values=v[a0:], allowed=allowed[g0:])), (dict(), dict())):
        got = model.sample_paths(cptr[2:], gptr, attr, N, seed=6, runs=runs, want_marginals=True, **kw_slice)
        alone = model.sample_paths(cptr[2:] - g0, gptr[g0:] - a0, attr[a0:], N, seed=6, runs=runs, want_marginals=True, **kw_alone)
        for x, z in zip(got, alone):
            assert x.size and x.tobytes() == z.tobytes()
        assert got[0].shape == (int(cptr[-1]) - g0, N)
    score = cr.masked_scores(gptr[g0:] - a0, attr[a0:], v[a0:], w, allowed[g0:])
    y = model.sample_paths(cptr[2:], gptr, attr, N, seed=6, values=v, allowed=allowed)
    _exact("a slice", y, dict(cptr=cptr[2:] - g0, trans=trans), score, 6)


def _anchor_mix(rng, cptr, L, count):
    """Run queries over the batch: anchors at a contig's first and last gene and inside, with random, singleton and full sets."""
    lens = np.diff(cptr)
    full = np.flatnonzero(lens > 0)
    out = []
    for q in range(count):
        c = int(np.argmax(lens)) if q < 3 else int(rng.choice(full))
        T = int(lens[c])
        anchor = (0, T - 1, int(rng.integers(0, T)))[q % 3]
        out.append((c, anchor, gs._set_mask(rng, L, ("random", "singleton", "full", "random", "bit31" if L == 32 else "random")[q % 5])))
    return out + out[:5]


@pytest.mark.parametrize("L", LABELS)
def test_runs_are_the_run_extents_of_the_returned_paths(nat, L):
    b = gs._batch(L)
    rng = np.random.default_rng(9900 + L)
    queries = _anchor_mix(rng, b["cptr"], L, 60)
    contig, anchor, mask = (np.array([q[k] for q in queries], dtype=np.int64) for k in range(3))
    model = nat.Model.from_tables(b["w"], b["trans"])
    for N in (1, 200):
        y, runs = model.sample_paths(*b["csr"], N, seed=11, runs=(contig, anchor, mask), **_kw(b, True, True))
        assert runs.shape == (len(queries), N, 2) and runs.dtype == np.int32
        want = sr.run_extents(y, b["cptr"], contig, anchor, mask)
        assert runs.tobytes() == want.tobytes()
        only = model.sample_paths(*b["csr"], N, seed=11, runs=(contig, anchor, mask), want_paths=False, **_kw(b, True, True))
        assert only.tobytes() == runs.tobytes(), "y = NULL gives the same runs"
        assert model.sample_paths(*b["csr"], N, seed=11, **_kw(b, True, True)).tobytes() == y.tobytes()
    assert np.any(runs[:, :, 0] == -1) or L == 2
    found = runs[runs[:, :, 0] >= 0]
    assert np.all(found[:, 0] < found[:, 1]) and found[:, 0].min() == 0
    lens = np.diff(b["cptr"])[contig]
    assert np.any(runs[:, :, 1] == lens[:, None]), "a run that reaches its contig's last gene"


def test_bad_runs_are_refused(nat):
    L = 5
    rng = np.random.default_rng(9300)
    model = nat.Model.from_tables(rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L)))
    cptr, gptr, attr = gs._csr(rng, [4, 0, 9, 0, 3])
    bad = {"contig": (5, 0, 1), "anchor": (2, 9, 1), "anchor below 0": (2, -1, 1), "a contig without genes": (1, 0, 1), "mask 0": (0, 0, 0),
           "a bit at L": (0, 0, 1 << L)}
    for what, query in bad.items():
        queries = [(0, 3, 3), (2, 8, 1), query]
        with pytest.raises(ValueError, match="run 2") as err:
            model.sample_paths(cptr, gptr, attr, 8, runs=tuple(np.array([q[k] for q in queries], dtype=np.int64) for k in range(3)))
        print(f"{what}: {err.value}")
    with pytest.raises(ValueError, match="n_samples = 0 is outside"):
        model.sample_paths(cptr, gptr, attr, 0)


# ---------------------------------------------------------------- 4. the distribution, end to end
@pytest.mark.parametrize("L", LABELS)
def test_the_distribution_end_to_end(nat, L):
    b = gs._batch(L)
    N = 4096
    model = nat.Model.from_tables(b["w"], b["trans"])
    worst = 0.0
    for valued, masked in ((False, False), (True, True)):
        kw = _kw(b, valued, masked)
        y, marg, _ = model.sample_paths(*b["csr"], N, seed=77 + L, want_marginals=True, **kw)
        freq = np.stack([(y == l).mean(axis=1) for l in range(L)], axis=1)
        ratio = np.abs(freq - marg) / _bound(marg, N)
        assert np.all(ratio <= 1.0), f"L={L}: a (gene, label) frequency outside the bound"
        assert np.all(freq[marg == 0.0] == 0.0)
        spans = list(b["spans"])[:40]
        p = np.exp(model.span_log_probabilities(*b["csr"], *gs._arrays(spans), **kw))
        share = np.zeros(len(spans))
        for q, (c, lo, hi, m) in enumerate(spans):
            g0 = int(b["cptr"][c])
            share[q] = np.all((m >> y[g0 + lo:g0 + hi].astype(np.int64)) & 1, axis=0).mean()
        sratio = np.abs(share - p) / _bound(p, N)
        assert np.all(sratio <= 1.0), f"L={L}: a span's share outside the bound"
        worst = max(worst, float(ratio.max()), float(sratio.max()))
        print(f"L={L} values={valued} allowed={masked}: worst |frequency - marginal| / bound = {ratio.max():.3g}, "
              f"worst |share - span probability| / bound = {sratio.max():.3g}")
    assert worst > 0.0


# ---------------------------------------------------------------- 5. SequenceCRF
def test_sequence_crf_samples(nat):
    L = 3
    b = gs._batch(L, (1, 6, 20, 33, 64, 3), 10)
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = gs._sequence_crf(w, b["trans"])
    X = gs._as_items(b, names)
    X.insert(2, [])
    rng = np.random.default_rng(9500)
    sets = [[None if rng.random() < 0.5 else {classes[int(rng.integers(0, L))], "l2"} for _ in xs] for xs in X]
    cptr, gptr, attr, _ = crf._pack(X)
    model = nat.Model.from_lcrf(crf.to_bytes())
    anchors = [(0, 0, "l0"), (1, 2, {"l1", "l2"}), (3, 19, ["l0", "l1"]), (4, 10, ("l2",)), (5, 0, frozenset(classes)), (6, 1, "l1")]
    masks = [sum(1 << classes.index(v) for v in ([labs] if isinstance(labs, str) else labs)) for *_, labs in anchors]
    native_runs = ([a[0] for a in anchors], [a[1] for a in anchors], masks)
    for allowed in (None, sets):
        amasks = None if allowed is None else crf._label_sets(allowed, cptr, "allowed")[0]
        want, want_runs = model.sample_paths(cptr, gptr, attr, 70, seed=21, allowed=amasks, runs=native_runs)
        got = crf.sample(X, 70, seed=21, allowed=allowed)
        assert len(got) == len(X) and [g.shape for g in got] == [(70, len(xs)) for xs in X] and all(g.dtype == np.int8 for g in got)
        assert got[2].shape == (70, 0)
        for k, g in enumerate(got):
            assert np.array_equal(g, want[cptr[k]:cptr[k + 1]].T) and g.min(initial=0) >= 0 and g.max(initial=0) < L
            assert g.base is not None, "a transposed view of the native block"
        runs = crf.sample_runs(X, anchors, 70, seed=21, allowed=allowed)
        assert runs.dtype == np.int32 and runs.tobytes() == want_runs.tobytes()
        assert np.all(runs[4] == [0, 64]), "the set of every label: the whole sequence"
        if allowed is not None:
            for k, g in enumerate(got):
                for t, entry in enumerate(sets[k]):
                    if entry is not None:
                        assert {classes[v] for v in set(g[:, t].tolist())} <= entry, "allowed= is honoured"
    assert crf.sample(X, 70, seed=22)[3].tobytes() != crf.sample(X, 70, seed=21)[3].tobytes()


# ---------------------------------------------------------------- 6. the typed front end
def test_typed_front_end_reports_boundary_intervals(nat, tmp_path):
    import math

    from gecco_amd import packing, tables, typed
    from gecco_amd.train_cli import join_clusters
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
    L, bg, N, seed = len(crf.classes_), crf.classes_.index("0"), 512, 9
    new = ["anchor_p", "exact_p", "start_lo", "start_hi", "end_lo", "end_hi"]
    # with 0: the columns and bytes of a call that omits the argument
    plain_genes, plain_clusters = crf.predict_genes_and_clusters(genes, region_posteriors=True)
    off_genes, off_clusters = crf.predict_genes_and_clusters(genes, region_posteriors=True, boundary_samples=0, seed=5)
    gs._dump(os.path.join(base, "plain"), crf, plain_genes, plain_clusters)
    gs._dump(os.path.join(base, "off"), crf, off_genes, off_clusters)
    gs._same_tables(os.path.join(base, "plain"), os.path.join(base, "off"))
    assert not any(col in typed.typed_cluster_table(off_clusters, crf.types_).columns for col in new)
    assert not any(hasattr(c, "anchor_probability") for c in off_clusters)
    # the batch as the front end packs it, for the native call
    ordered = sorted(genes, key=operator.attrgetter("source.id", "start"))
    ids = [g.id for g in ordered]
    contigs = [list(g) for _, g in itertools.groupby(ordered, key=operator.attrgetter("source.id"))]
    batch = packing.pack_contigs(contigs, crf._attr_index, "protein")
    cptr, gptr, attr = batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id
    model = nat.Model.from_lcrf(crf._blob)
    not_bg = ((1 << L) - 1) & ~(1 << bg)

    def check(annotated, found, known):
        assert found
        allowed = None if known is None else typed.known_masks(len(ordered), known, join_clusters(ordered, known, device=0),
                                                                crf.classes_, crf.background)
        p_any = np.array([g.average_probability for g in annotated])
        where = []
        for cl in found:
            first, last = ids.index(cl.genes[0].id), ids.index(cl.genes[-1].id) + 1
            c = int(np.searchsorted(cptr, first, side="right")) - 1
            where.append((c, first - int(cptr[c]), last - int(cptr[c]), first + int(np.argmax(p_any[first:last])) - int(cptr[c])))
        runs, marg, _ = model.sample_paths(cptr, gptr, attr, N, seed=seed, allowed=allowed, want_marginals=True, want_paths=False,
                                           runs=([w[0] for w in where], [w[3] for w in where], [not_bg] * len(where)))
        logp = model.span_log_probabilities(cptr, gptr, attr, [w[0] for w in where], [w[1] for w in where], [w[2] for w in where],
                                            [not_bg] * len(where), allowed=allowed)
        worst = 0.0
        for cl, (c, lo, hi, anchor), found_runs, region in zip(found, where, runs, np.exp(logp).tolist()):
            g0 = int(cptr[c])
            there = found_runs[found_runs[:, 0] >= 0]
            m = len(there)
            assert cl.anchor_probability == m / N
            assert cl.exact_probability == float(np.mean((found_runs[:, 0] == lo) & (found_runs[:, 1] == hi)))
            p_anchor = 1.0 - marg[g0 + anchor, bg]
            covering = float(np.mean((found_runs[:, 0] >= 0) & (found_runs[:, 0] <= lo) & (found_runs[:, 1] >= hi)))
            assert abs(cl.anchor_probability - p_anchor) <= _bound(p_anchor, N)
            assert abs(covering - region) <= _bound(region, N)
            if region_of.get(cl.id) is not None:
                assert region_of[cl.id] == region
            worst = max(worst, abs(cl.anchor_probability - p_anchor) / _bound(p_anchor, N), abs(covering - region) / _bound(region, N))
            assert cl.exact_probability <= covering <= cl.anchor_probability
            if m:
                starts = sorted(ordered[g0 + k].start for k in there[:, 0].tolist())
                ends = sorted(ordered[g0 + k - 1].end for k in there[:, 1].tolist())
                i_lo, i_hi = math.floor(0.05 * (m - 1)), math.ceil(0.95 * (m - 1))
                assert cl.start_interval == (starts[i_lo], starts[i_hi]) and cl.end_interval == (ends[i_lo], ends[i_hi])
            else:
                assert cl.start_interval == (cl.start, cl.start) and cl.end_interval == (cl.end, cl.end)
            assert cl.start_interval[0] <= cl.start_interval[1] and cl.end_interval[0] <= cl.end_interval[1]
            assert cl.start_interval[0] < cl.end_interval[1]
        print(f"known={'yes' if known is not None else 'no'}: {len(found)} clusters, worst ratio to the bound = {worst:.3g}, "
              f"intervals {[(c.start_interval, c.end_interval) for c in found[:3]]}")

    region_of = {}
    annotated, found = crf.predict_genes_and_clusters(genes, boundary_samples=N, seed=seed, region_posteriors=True)
    region_of = {c.id: c.region_probability for c in found}
    assert [c.id for c in found] == [c.id for c in plain_clusters]
    assert [g.average_probability for g in annotated] == [g.average_probability for g in plain_genes]
    assert [c.id for c in crf.predict_clusters(genes, boundary_samples=N, seed=seed)] == [c.id for c in found]
    check(annotated, found, None)
    again = crf.predict_clusters(genes, boundary_samples=N, seed=seed)
    assert [(c.anchor_probability, c.exact_probability, c.start_interval, c.end_interval) for c in again] == \
        [(c.anchor_probability, c.exact_probability, c.start_interval, c.end_interval) for c in found]
    # the columns are written and read back
    table = typed.typed_cluster_table(found, crf.types_)
    names = [n for n, _, _ in table.COLUMNS]
    assert names[names.index("proteins") - 6:names.index("proteins")] == new and names.index("region_p") < names.index("anchor_p")
    path = os.path.join(base, "clusters.tsv")
    table.dump(path)
    back = tables.ClusterTable.load(path)
    assert [float(v) for v in back.anchor_p] == [c.anchor_probability for c in found]
    assert [float(v) for v in back.exact_p] == [c.exact_probability for c in found]
    assert [(int(a), int(z)) for a, z in zip(back.start_lo, back.start_hi)] == [c.start_interval for c in found]
    assert [(int(a), int(z)) for a, z in zip(back.end_lo, back.end_hi)] == [c.end_interval for c in found]
    # a known region restricts the lattice the paths are drawn on
    region_of = {}
    known = tables.ClusterTable({"sequence_id": ["fresh00"], "cluster_id": ["k1"], "start": [plain_genes[60].start],
                                 "end": [plain_genes[69].end], "type": ["Beta"]})
    k_annotated, k_found = crf.predict_genes_and_clusters(genes, known=known, boundary_samples=N, seed=seed)
    check(k_annotated, k_found, known)
    inside = [c for c in k_found if c.source.id == "fresh00" and {g.id for g in c.genes} <= set(ids[60:70])]
    for cl in inside:  # (no path is background inside the known region: every run covers the call)
        assert cl.anchor_probability == 1.0 and cl.start_interval[1] <= cl.start and cl.end_interval[0] >= cl.end
    print(f"calls inside the known region: {len(inside)}")
    # the command line with --boundary-samples writes the method's table
    crf.save(os.path.join(base, "model"))
    known.dump(os.path.join(base, "known.tsv"))
    gs._dump(os.path.join(base, "method"), crf, k_annotated, k_found)
    done = subprocess.run([sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
                           os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv"),
                           "--known", os.path.join(base, "known.tsv"), "--boundary-samples", str(N), "--seed", str(seed), "-o",
                           os.path.join(base, "cli")], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    gs._same_tables(os.path.join(base, "method"), os.path.join(base, "cli"))
    with open(os.path.join(base, "cli", "clusters.tsv")) as fh:
        assert fh.readline().rstrip("\n").split("\t")[-8:-2] == new
