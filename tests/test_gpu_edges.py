"""Edge posteriors on the device: ``gecco_crf_edge_posteriors`` -- the pairwise marginals xi of the whole-contig lattice, the
probability that a run of labels of a set starts or ends at a gene, a contig's expected transition counts and its path entropy
-- against the independent numpy yardstick (tests/edges_reference.py), through every whole-contig arrangement, and up through
``SequenceCRF`` and the typed front end.

Tolerances, from the project's own (tests/test_gpu_constrained.py holds a whole-contig marginal to 1e-12): |xi - ref| <= 1e-12;
enter and leave, sums of up to L^2 entries of a normalised table, <= 1e-12 L; the transition counts and the entropy of a contig of
T items, sums of T per-edge terms, <= 1e-12 max(1, T).  Every test prints its worst difference and the worst difference over its
bound."""
import functools
import itertools
import operator
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import edges_reference as er
from tests import train_objective_partial as tp
from tests.test_gpu_spans import (A, ARRANGEMENTS, KINDS, LABELS, ROOT, _arrangement_lengths, _as_items, _csr, _dump, _load,
                                  _sequence_crf, _set_mask, _values, _wide_masks, _write_tables)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


# ---------------------------------------------------------------- batches and the yardstick
def _lengths(rng):
    """The batch shape of tests/test_gpu_spans.py -- contigs of 1, 2 and 3 items, 37 of 1 to 60, one of 300 -- and one of 0."""
    return [1, 2, 3, 0] + [int(x) for x in rng.integers(1, 61, size=37)] + [300]


def _sets(rng, L):
    """Random sets, a singleton, the full set, a duplicate of the first, and at 32 labels one with bit 31."""
    sets = [_set_mask(rng, L, "random"), _set_mask(rng, L, "singleton"), (1 << L) - 1, _set_mask(rng, L, "random")]
    sets.append(sets[0])
    if L == 32:
        sets.append((1 << 31) | int(rng.integers(0, 1 << 31)))
    return sets


@functools.lru_cache(maxsize=None)
def _batch(L, lengths=None):
    rng = np.random.default_rng(8700 + L)
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    cptr, gptr, attr = _csr(rng, _lengths(rng) if lengths is None else list(lengths))
    n = int(cptr[-1])
    return dict(L=L, w=w, trans=trans, cptr=cptr, gptr=gptr, attr=attr, csr=(cptr, gptr, attr), v=_values(rng, len(attr)),
                allowed=_wide_masks(rng, n, L), sets=tuple(_sets(rng, L)))


@functools.lru_cache(maxsize=None)
def _reference(L, lengths, valued, masked):
    """The yardstick of a batch, computed once and shared (read only)."""
    b = _batch(L, lengths)
    every = tp.full_masks(int(b["cptr"][-1]), L)
    score = cr.masked_scores(b["gptr"], b["attr"], b["v"] if valued else None, b["w"], b["allowed"] if masked else every)
    return er.edge_posteriors(b["cptr"], score, b["trans"], b["sets"])


def _check(tag, out, ref, cptr, L, sets):
    """The device outputs against the yardstick, and the identities that hold on the device outputs alone."""
    T = np.diff(cptr).astype(np.float64)
    per_contig = 1e-12 * np.maximum(1.0, T)
    figures = {}

    def worst(name, diff, bound):
        w, r = float(np.max(diff, initial=0.0)), float(np.max(diff / bound, initial=0.0))
        figures[name] = (w, r)
        return r

    for name, value in out.items():
        assert value.dtype == np.float64 and not np.any(np.isnan(value)), f"{tag}: NaN in {name}"
    ratios = []
    if "pair" in out:
        assert out["pair"].shape == ref["pair"].shape
        ratios.append(worst("xi", np.abs(out["pair"] - ref["pair"]), 1e-12))
        assert out["pair"].min() >= 0.0 and out["pair"].max() <= 1.0
        assert np.all(out["pair"][cptr[:-1][T > 0]] == 0.0), "zeros at a contig's first gene"
    for name in ("enter", "leave"):
        assert out[name].shape == ref[name].shape
        ratios.append(worst(name, np.abs(out[name] - ref[name]), 1e-12 * L))
        assert out[name].min() >= 0.0 and out[name].max() <= 1.0
    ratios.append(worst("transitions", np.abs(out["transitions"] - ref["transitions"]).max(axis=(1, 2)), per_contig))
    ratios.append(worst("entropy", np.abs(out["entropy"] - ref["entropy"]), per_contig))
    assert np.all(out["entropy"] >= 0.0)
    # identities on the device outputs alone
    marg = out["marginals"]
    inner = np.ones(len(marg), dtype=bool)
    inner[cptr[:-1][T > 0]] = False
    t = np.flatnonzero(inner)
    if "pair" in out:
        rows, cols = out["pair"][t].sum(axis=2), out["pair"][t].sum(axis=1)
        ratios.append(worst("row sums - marg[t-1]", np.abs(rows - marg[t - 1]), 2e-12))
        ratios.append(worst("column sums - marg[t]", np.abs(cols - marg[t]), 2e-12))
        by_contig = np.add.reduceat(out["pair"], cptr[:-1][T > 0], axis=0)
        assert np.abs(by_contig - out["transitions"][T > 0]).max(axis=(1, 2), initial=0.0).max(initial=0.0) <= 1e-12 * T.max()
    for c in range(len(T)):
        a, e = int(cptr[c]), int(cptr[c + 1])
        se, sl = out["enter"][a:e].sum(axis=0), out["leave"][a:e].sum(axis=0)
        assert np.all(np.abs(se - sl) <= 1e-12 * max(1.0, T[c])), f"{tag}: contig {c}: sum of enter != sum of leave"
        if e > a:
            for k, m in enumerate(sets):  # expected_runs' host formula = the sum of enter
                runs = er.expected_runs(marg[a], out["transitions"][c], m)
                assert abs(runs - se[k]) <= 1e-12 * max(1.0, T[c])
        else:
            assert out["entropy"][c] == 0.0 and not out["transitions"][c].any()
        if e - a == 1:  # one item: enter = leave = P(y in S), no transition, H = H(marg)
            p = np.array([marg[a][[bool((m >> y) & 1) for y in range(L)]].sum() for m in sets])
            assert np.all(np.abs(out["enter"][a] - p) <= 1e-15 * L) and np.array_equal(out["enter"][a], out["leave"][a])
            assert not out["transitions"][c].any()
            mm = marg[a][marg[a] > 0]
            assert abs(out["entropy"][c] + (mm * np.log(mm)).sum()) <= 1e-12
    full = [k for k, m in enumerate(sets) if m == (1 << L) - 1]
    for k in full:  # the full set: a run starts at a contig's first gene and nowhere else
        assert np.all(np.abs(out["enter"][~inner, k] - 1.0) <= 1e-12 * L) and np.all(out["enter"][inner, k] == 0.0)
    seen = {}
    for k, m in enumerate(sets):  # duplicate sets: equal bytes
        if m in seen:
            assert out["enter"][:, k].tobytes() == out["enter"][:, seen[m]].tobytes()
            assert out["leave"][:, k].tobytes() == out["leave"][:, seen[m]].tobytes()
        seen.setdefault(m, k)
    print(f"{tag}: " + ", ".join(f"{name}: worst {w:.3g} (x{r:.3g} of its bound)" for name, (w, r) in figures.items()))
    assert max(ratios) <= 1.0, f"{tag}: {figures}"
    return figures


def _call(model, b, valued, masked, **kw):
    kw.setdefault("sets", np.array(b["sets"], dtype=np.uint32))
    return model.edge_posteriors(*b["csr"], values=b["v"] if valued else None, allowed=b["allowed"] if masked else None,
                                 want_marginals=True, **kw)


def _same_bytes(x, y):
    assert x.keys() == y.keys()
    for name in x:
        assert x[name].tobytes() == y[name].tobytes(), name


# ---------------------------------------------------------------- 1. against the yardstick
@pytest.mark.parametrize("valued,masked", KINDS)
@pytest.mark.parametrize("L", LABELS)
def test_edges_against_the_yardstick(nat, L, valued, masked):
    b = _batch(L)
    assert {0, 1, 2, 3, 300} <= set(np.diff(b["cptr"]).tolist())
    if L == 32:
        assert any(m >> 31 for m in b["sets"])
    model = nat.Model.from_tables(b["w"], b["trans"])
    out = _call(model, b, valued, masked, want_pair=True)
    _check(f"L={L} values={valued} allowed={masked}", out, _reference(L, None, valued, masked), b["cptr"], L, b["sets"])
    # the same call gives the same bytes; without the pair table the other outputs keep theirs
    _same_bytes(out, _call(model, b, valued, masked, want_pair=True))
    lean = _call(model, b, valued, masked)
    assert "pair" not in lean
    _same_bytes({k: v for k, v in out.items() if k != "pair"}, lean)
    # marg / lognorm are the marginals entry's bytes
    emarg, elogz = model.marginals_full(*b["csr"], values=b["v"] if valued else None, allowed=b["allowed"] if masked else None)
    assert out["marginals"].tobytes() == emarg.tobytes() and out["lognorm"].tobytes() == elogz.tobytes()
    if masked:  # a disallowed (gene, label) pair: exact zeros in its column, and in the rows that leave it
        dead = ~tp.mask_matrix(b["allowed"], L)
        assert dead.any() and np.all(out["pair"].transpose(0, 2, 1)[dead] == 0.0)
        inner = np.ones(len(dead), dtype=bool)
        inner[b["cptr"][:-1][np.diff(b["cptr"]) > 0]] = False
        assert np.all(out["pair"][1:][(dead[:-1] & inner[1:, None])] == 0.0)


# ---------------------------------------------------------------- 2. every whole-contig arrangement
@pytest.mark.parametrize("L,switch,mode", ARRANGEMENTS)
def test_every_whole_contig_arrangement(nat, monkeypatch, L, switch, mode):
    lengths = _arrangement_lengths()
    b = _batch(L, lengths)
    monkeypatch.setenv(switch, mode)
    model = nat.Model.from_tables(b["w"], b["trans"])
    for valued, masked in ((True, True), (False, False)):
        out = _call(model, b, valued, masked, want_pair=True)
        _check(f"L={L} {switch}={mode} values={valued} allowed={masked}", out, _reference(L, lengths, valued, masked), b["cptr"], L,
               b["sets"])
        emarg, elogz = model.marginals_full(*b["csr"], values=b["v"] if valued else None, allowed=b["allowed"] if masked else None)
        assert out["marginals"].tobytes() == emarg.tobytes() and out["lognorm"].tobytes() == elogz.tobytes()


# ---------------------------------------------------------------- 3. a set does not depend on the other sets
@pytest.mark.parametrize("L", [3, 32])
def test_a_set_alone_and_among_31_others_in_another_order(nat, L):
    b = _batch(L)
    rng = np.random.default_rng(8800 + L)
    model = nat.Model.from_tables(b["w"], b["trans"])
    mine = b["sets"][0]
    alone = _call(model, b, True, True, sets=[mine])
    others = [_set_mask(rng, L, ("random", "singleton", "full")[k % 3]) for k in range(31)]
    for place in (0, 17, 31):
        sets = others[:place] + [mine] + others[place:]
        assert len(sets) == 32
        among = _call(model, b, True, True, sets=sets)
        assert among["enter"].shape[1] == 32
        assert among["enter"][:, place].tobytes() == alone["enter"][:, 0].tobytes()
        assert among["leave"][:, place].tobytes() == alone["leave"][:, 0].tobytes()
        for name in ("transitions", "entropy", "marginals", "lognorm"):
            assert among[name].tobytes() == alone[name].tobytes()


# ---------------------------------------------------------------- 4. the edges of the range
@pytest.mark.parametrize("L", [2, 17])
def test_every_item_restricted_to_one_label(nat, L):
    b = _batch(L)
    rng = np.random.default_rng(8900 + L)
    n = int(b["cptr"][-1])
    path = rng.integers(0, L, size=n)
    allowed = (np.uint32(1) << path.astype(np.uint32)).astype(np.uint32)
    model = nat.Model.from_tables(b["w"], b["trans"])
    out = model.edge_posteriors(*b["csr"], allowed=allowed, sets=[1], want_pair=True)
    T = np.diff(b["cptr"])
    print(f"L={L}: worst entropy / (1e-12 T) = {float((out['entropy'] / (1e-12 * np.maximum(T, 1))).max()):.3g}")
    assert np.all(out["entropy"] >= 0.0) and np.all(out["entropy"] <= 1e-12 * np.maximum(T, 1))
    inner = np.ones(n, dtype=bool)
    inner[b["cptr"][:-1][T > 0]] = False
    hot = np.zeros((n, L, L))
    t = np.flatnonzero(inner)
    hot[t, path[t - 1], path[t]] = 1.0
    assert np.array_equal(out["pair"] != 0.0, hot != 0.0) and np.abs(out["pair"] - hot).max() <= 1e-12
    counts = np.add.reduceat(hot, b["cptr"][:-1][T > 0], axis=0)
    assert np.abs(out["transitions"][T > 0] - counts).max() <= 1e-12 * T.max()


@pytest.mark.parametrize("L", [3, 17])
def test_one_label_leading_by_800_at_one_gene(nat, L):
    """As test_a_label_outside_the_set_that_leads_by_800 of tests/test_gpu_spans.py: one attribute gives label k a lead of 800
    over every other label on one item of each contig; the queried sets leave k out.  Every output is finite and within
    tolerance: the directions are divided by their own maxima before any product, and nothing is formed from exp(-800)."""
    rng = np.random.default_rng(8600 + L)
    k, T, special = 1, 12, A - 1
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    w[special] = 0.0
    w[special, k] = 800.0 + 2.0 * np.abs(w).sum(axis=0).max()
    leaders = [5, 2, T - 2, 0, T - 1]
    cptr = np.arange(0, (len(leaders) + 1) * T, T).astype(np.int32)
    deg = rng.integers(1, 4, size=int(cptr[-1]))
    rows = [list(rng.integers(0, A - 1, size=d)) for d in deg]
    for c, p in enumerate(leaders):
        rows[c * T + p].append(special)
    gptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    attr = np.array([a for r in rows for a in r], dtype=np.int32)
    score = cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L))
    for c, p in enumerate(leaders):
        assert score[c * T + p][k] - np.delete(score[c * T + p], k).max() >= 800.0
    sets = [((1 << L) - 1) & ~(1 << k), 1, 1 << k]
    model = nat.Model.from_tables(w, trans)
    out = model.edge_posteriors(cptr, gptr, attr, sets=sets, want_pair=True, want_marginals=True)
    assert all(np.all(np.isfinite(v)) for v in out.values())
    _check(f"L={L} leader by 800", out, er.edge_posteriors(cptr, score, trans, sets), cptr, L, sets)


# ---------------------------------------------------------------- 5. refusals, empty batches, slices
def test_refusals_and_batches_without_genes(nat):
    L = 5
    rng = np.random.default_rng(9300)
    model = nat.Model.from_tables(rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L)))
    cptr, gptr, attr = _csr(rng, [4, 0, 9, 0, 3])
    for what, sets, words in (("33 sets", [1] * 33, "n_sets = 33"), ("an empty mask", [3, 0], "set 1"), ("a bit at L", [3, 1, 1 << L], "set 2"),
                              ("bit 31", [(1 << 31) | 1], "set 0"), ("no set for enter and leave", [], "need a label set")):
        with pytest.raises(ValueError, match=words) as err:
            model.edge_posteriors(cptr, gptr, attr, sets=sets)
        print(f"{what}: {err.value}")
    # no set at all: the other outputs
    out = model.edge_posteriors(cptr, gptr, attr)
    assert sorted(out) == ["entropy", "transitions"] and out["transitions"].shape == (5, L, L) and out["entropy"][1] == 0.0
    assert model.edge_posteriors(cptr, gptr, attr, want_transitions=False, want_entropy=False) == {}
    # a batch without genes, and one without contigs
    none = model.edge_posteriors(np.zeros(4, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), sets=[1, 2],
                                 want_pair=True, want_marginals=True)
    assert none["pair"].shape == (0, L, L) and none["enter"].shape == (0, 2) and none["marginals"].shape == (0, L)
    assert not none["transitions"].any() and none["entropy"].tolist() == [0.0] * 3 and none["lognorm"].tolist() == [0.0] * 3
    nothing = model.edge_posteriors(np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), sets=[1])
    assert nothing["transitions"].shape == (0, L, L) and nothing["entropy"].shape == (0,)


@pytest.mark.parametrize("L", [2, 12])
def test_a_slice_gives_the_bytes_of_the_rebased_batch(nat, L):
    rng = np.random.default_rng(9400 + L)
    model = nat.Model.from_tables(rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L)))
    cptr, gptr, attr = _csr(rng, [4, 9, 3, 30, 1, 70])
    v = _values(rng, len(attr))
    allowed = _wide_masks(rng, int(cptr[-1]), L)
    g0 = int(cptr[2])
    a0 = int(gptr[g0])
    allowed[:g0] = 0  # (masks of genes outside the batch are not looked at)
    sets = [_set_mask(rng, L, "random"), (1 << L) - 1]
    for kw_slice, kw_alone in ((dict(values=v, allowed=allowed), dict(values=v[a0:], allowed=allowed[g0:])), (dict(), dict())):
        got = model.edge_posteriors(cptr[2:], gptr, attr, sets=sets, want_pair=True, want_marginals=True, **kw_slice)
        alone = model.edge_posteriors(cptr[2:] - g0, gptr[g0:] - a0, attr[a0:], sets=sets, want_pair=True, want_marginals=True, **kw_alone)
        _same_bytes(got, alone)
        assert got["pair"].shape == (int(cptr[-1]) - g0, L, L) and got["pair"].any()
    # a contig's outputs do not depend on what else the batch holds: the 70-item contig alone
    last = model.edge_posteriors(cptr[5:], gptr, attr, sets=sets, want_pair=True)
    whole = model.edge_posteriors(cptr, gptr, attr, sets=sets, want_pair=True)
    assert last["pair"].tobytes() == whole["pair"][cptr[5]:].tobytes() and last["entropy"].tobytes() == whole["entropy"][5:].tobytes()
    assert last["transitions"].tobytes() == whole["transitions"][5:].tobytes()


# ---------------------------------------------------------------- 6. SequenceCRF
def test_sequence_crf_against_the_native_call(nat):
    L = 5
    b = _batch(L, (1, 6, 20, 33, 64, 3))
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = _sequence_crf(w, b["trans"])
    X = _as_items(b, names)
    X.insert(2, [])
    rng = np.random.default_rng(9500)
    sets = ["l0", {"l1", "l4"}, ["l0", "l1", "l2", "l3"], ("l2",), frozenset(classes), {"l4", "l1"}]
    masks = [sum(1 << classes.index(y) for y in ([s] if isinstance(s, str) else s)) for s in sets]
    allowed_sets = [[None if rng.random() < 0.5 else {classes[int(rng.integers(0, L))], classes[int(rng.integers(0, L))], "l2"}
                     for _ in xs] for xs in X]
    cptr, gptr, attr, _ = crf._pack(X)
    model = nat.Model.from_lcrf(crf.to_bytes())
    for allowed in (None, allowed_sets):
        amasks = None if allowed is None else crf._label_sets(allowed, cptr, "allowed")[0]
        want = model.edge_posteriors(cptr, gptr, attr, sets=masks, want_pair=True, want_marginals=True, allowed=amasks)
        pairs = crf.predict_pair_marginals(X, allowed=allowed)
        assert [p.shape for p in pairs] == [(len(xs), L, L) for xs in X]
        assert np.concatenate(pairs).tobytes() == want["pair"].tobytes()
        bounds = crf.boundary_probability(X, sets, allowed=allowed)
        assert len(bounds) == len(X) and bounds[2][0].shape == (0, len(sets))
        assert np.concatenate([e for e, _ in bounds]).tobytes() == want["enter"].tobytes()
        assert np.concatenate([l for _, l in bounds]).tobytes() == want["leave"].tobytes()
        assert bounds[1][0][:, 1].tobytes() == bounds[1][0][:, 5].tobytes()
        assert crf.expected_transitions(X, allowed=allowed).tobytes() == want["transitions"].tobytes()
        assert crf.path_entropy(X, allowed=allowed).tobytes() == want["entropy"].tobytes()
        runs = crf.expected_runs(X, sets, allowed=allowed)
        assert runs.shape == (len(X), len(sets)) and not runs[2].any()
        for s, (e, _) in enumerate(bounds):
            assert np.all(np.abs(runs[s] - e.sum(axis=0)) <= 1e-12 * max(1, len(X[s])))
            if len(X[s]):
                for k, m in enumerate(masks):
                    assert runs[s, k] == pytest.approx(er.expected_runs(want["marginals"][cptr[s]], want["transitions"][s], m), abs=1e-12)
    # more than 32 sets: several native calls, the same columns
    many = [classes[k % L] for k in range(40)] + [{"l0", "l3"}]
    wide = crf.boundary_probability(X, many)
    head = crf.boundary_probability(X, many[:32])
    tail = crf.boundary_probability(X, many[32:])
    for s in range(len(X)):
        for side in (0, 1):
            assert wide[s][side].shape == (len(X[s]), 41)
            assert wide[s][side].tobytes() == np.concatenate([head[s][side], tail[s][side]], axis=1).tobytes()
    assert crf.expected_runs(X, many).shape == (len(X), 41)
    # items with values
    Xv = [[{a: 0.5 + 0.25 * k for k, a in enumerate(item)} for item in xs] for xs in X]
    cptr, gptr, attr, vals = crf._pack(Xv)
    want = model.edge_posteriors(cptr, gptr, attr, sets=masks[:2], values=vals)
    assert crf.path_entropy(Xv).tobytes() == want["entropy"].tobytes()
    assert np.concatenate([e for e, _ in crf.boundary_probability(Xv, sets[:2])]).tobytes() == want["enter"].tobytes()
    assert not np.array_equal(crf.path_entropy(Xv), crf.path_entropy(X))


# ---------------------------------------------------------------- 7. the typed front end
def test_typed_front_end_reports_boundary_posteriors(nat, tmp_path):
    from gecco_amd import packing, tables, typed
    from tests.typed_planted import C, W, planted_set

    train_genes, train_rows = planted_set(11, 12, "train", composite=True)
    fresh_genes, _ = planted_set(12, 2, "fresh", composite=False)
    base = str(tmp_path)
    _write_tables(os.path.join(base, "train"), train_genes, train_rows)
    _write_tables(os.path.join(base, "fresh"), fresh_genes)
    random.seed(42)
    np.random.seed(42)
    crf = typed.TypedClusterCRF(W, 1, c1=C, c2=C)
    crf.fit(_load(os.path.join(base, "train")), tables.ClusterTable.load(os.path.join(base, "train", "clusters.tsv")))
    genes = _load(os.path.join(base, "fresh"))
    L, bg = len(crf.classes_), crf.classes_.index("0")
    # without the flag: the columns and bytes of a call that omits it
    plain_genes, plain_clusters = crf.predict_genes_and_clusters(genes)
    off_genes, off_clusters = crf.predict_genes_and_clusters(genes, boundary_posteriors=False)
    _dump(os.path.join(base, "plain"), crf, plain_genes, plain_clusters)
    _dump(os.path.join(base, "off"), crf, off_genes, off_clusters)
    for name in ("genes.tsv", "features.tsv", "clusters.tsv"):
        with open(os.path.join(base, "plain", name), "rb") as fa, open(os.path.join(base, "off", name), "rb") as fb:
            assert fa.read() == fb.read(), name
    assert not hasattr(crf, "sequence_posteriors_") and not any(hasattr(c, "start_probability") for c in plain_clusters)
    assert "start_p" not in typed.typed_cluster_table(plain_clusters, crf.types_).columns
    # with it: the native call's values at the called boundaries
    annotated, found = crf.predict_genes_and_clusters(genes, boundary_posteriors=True)
    assert found and [c.id for c in found] == [c.id for c in plain_clusters]
    assert [g.average_probability for g in annotated] == [g.average_probability for g in plain_genes]
    ordered = sorted(genes, key=operator.attrgetter("source.id", "start"))
    ids = [g.id for g in ordered]
    contigs = [list(g) for _, g in itertools.groupby(ordered, key=operator.attrgetter("source.id"))]
    batch = packing.pack_contigs(contigs, crf._attr_index, "protein")
    cptr, gptr, attr = batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id
    not_bg = ((1 << L) - 1) & ~(1 << bg)
    model = nat.Model.from_lcrf(crf._blob)
    want = model.edge_posteriors(cptr, gptr, attr, sets=[not_bg], want_marginals=True)
    for cl in found:
        first, last = ids.index(cl.genes[0].id), ids.index(cl.genes[-1].id)
        assert cl.start_probability == want["enter"][first, 0] and cl.end_probability == want["leave"][last, 0]
        assert 0.0 <= cl.start_probability <= 1.0 and 0.0 <= cl.end_probability <= 1.0
    table = typed.typed_cluster_table(found, crf.types_)
    names = [n for n, _, _ in table.COLUMNS]
    assert table.columns["start_p"] == [c.start_probability for c in found] and table.columns["end_p"] == [c.end_probability for c in found]
    assert names.index("end_p") == names.index("start_p") + 1 and names.index("start_p") > names.index("type")
    seqs = crf.sequence_posteriors_
    assert tuple(seqs) == typed.TypedClusterCRF.SEQUENCE_COLUMNS
    assert seqs["sequence_id"] == [c[0].source.id for c in contigs] and seqs["genes"] == [len(c) for c in contigs]
    assert seqs["log_z"] == want["lognorm"].tolist() and seqs["entropy"] == want["entropy"].tolist()
    runs = [float(want["enter"][a:b, 0].sum()) for a, b in zip(cptr[:-1], cptr[1:])]
    assert seqs["expected_clusters"] == runs and all(h >= 0.0 for h in seqs["entropy"])
    print(f"{len(found)} clusters: start_p {[round(c.start_probability, 4) for c in found]}, end_p "
          f"{[round(c.end_probability, 4) for c in found]}; expected clusters per contig {[round(r, 4) for r in runs]}")
    # together with the other optional columns: behind them
    _, both = crf.predict_genes_and_clusters(genes, region_posteriors=True, boundary_samples=16, boundary_posteriors=True)
    names = [n for n, _, _ in typed.typed_cluster_table(both, crf.types_).COLUMNS]
    assert names.index("region_p") < names.index("end_hi") < names.index("start_p") < names.index("end_p") < names.index("proteins")
    assert [c.start_probability for c in both] == [c.start_probability for c in found]
    # the command line: with the flag the method's table and sequences.tsv, without it the files of a run that omits it
    crf.save(os.path.join(base, "model"))
    _dump(os.path.join(base, "method"), crf, annotated, found)
    common = [sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
              os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv")]
    for flags, out_dir in ((["--boundary-posteriors"], "cli"), ([], "cli_plain")):
        done = subprocess.run(common + flags + ["-o", os.path.join(base, out_dir)], cwd=ROOT, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
    for name in ("genes.tsv", "features.tsv", "clusters.tsv"):
        for a, b in (("method", "cli"), ("plain", "cli_plain")):
            with open(os.path.join(base, a, name), "rb") as fa, open(os.path.join(base, b, name), "rb") as fb:
                assert fa.read() == fb.read(), (a, b, name)
    assert sorted(os.listdir(os.path.join(base, "cli_plain"))) == ["clusters.tsv", "features.tsv", "genes.tsv"]
    with open(os.path.join(base, "cli", "clusters.tsv")) as fh:
        header = fh.readline().rstrip("\n").split("\t")
        assert "start_p" in header and "end_p" in header
    with open(os.path.join(base, "cli", "sequences.tsv")) as fh:
        lines = [line.rstrip("\n").split("\t") for line in fh]
    assert lines[0] == list(typed.TypedClusterCRF.SEQUENCE_COLUMNS) and len(lines) == 1 + len(contigs)
    assert [row[0] for row in lines[1:]] == seqs["sequence_id"] and [float(row[3]) for row in lines[1:]] == seqs["entropy"]
    assert [float(row[4]) for row in lines[1:]] == seqs["expected_clusters"] and [int(row[1]) for row in lines[1:]] == seqs["genes"]
