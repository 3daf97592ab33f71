"""Region posteriors on the device: ``gecco_crf_span_probabilities`` -- log P(every item of a span carries a label of a set | x)
on the whole-contig lattice -- against the independent numpy yardstick (tests/constrained_reference.py), through every
whole-contig arrangement, and up through ``SequenceCRF`` and the typed front end.

The yardstick of every result is ``ref = log Z_A' - log Z_A``: both from ``cr.marginals`` over ``cr.masked_scores``, A the
allowed masks of the call (every label without them) and A' = A and the span's set inside the span.  The tolerance is the one
tests/test_gpu_constrained.py holds ``log_likelihood`` with sets to: ``1e-10 (max(1, |log Z_A'|) + max(1, |log Z_A|))``.  Where
``ref`` is -inf the result has to be -inf.  Every test prints its worst |difference| and worst difference / bound."""
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
from tests import train_objective_partial as tp

pytestmark = pytest.mark.gpu

LABELS = [2, 3, 8, 17, 32]
A = 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(False, False), (True, False), (False, True), (True, True)]  # (with values, with allowed masks)


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


# ---------------------------------------------------------------- batches and the yardstick
def _csr(rng, lengths, max_attrs=4):
    cptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    deg = rng.integers(0, max_attrs + 1, size=int(cptr[-1]))
    gptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    attr = rng.integers(0, A, size=int(gptr[-1])).astype(np.int32)
    return cptr, gptr, attr


def _lengths(rng):
    """The batch shape of tests/test_gpu_constrained.py: about 40 contigs of 1 to 60 items, and one of 300."""
    return [1, 2, 3] + [int(x) for x in rng.integers(1, 61, size=37)] + [300]


def _values(rng, n):
    v = rng.normal(0.0, 1.0, size=n)
    kind = rng.integers(0, 6, size=n)
    v[kind == 3] = 0.0
    v[kind == 4] = 1.0
    v[kind == 5] = 2.0 ** rng.integers(-3, 4, size=int((kind == 5).sum()))
    return v


def _wide_masks(rng, n, L, p=0.8):
    """Allowed masks that leave most labels in (every label with probability p, never empty): most spans keep a path."""
    bits = rng.random((n, L)) < p
    for i in np.flatnonzero(~bits.any(axis=1)):
        bits[i, int(rng.integers(0, L))] = True
    return (bits.astype(np.uint64) << np.arange(L, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def _set_mask(rng, L, kind):
    full = (1 << L) - 1
    if kind == "full":
        return full
    if kind == "singleton":
        return 1 << int(rng.integers(0, L))
    if kind == "bit31":  # (L = 32 only: the top bit, alone or with company)
        return (1 << 31) | (int(rng.integers(0, 1 << 31)) if rng.random() < 0.5 else 0)
    m = 0
    for y in range(L):
        if rng.random() < 0.6:
            m |= 1 << y
    return m or 1 << int(rng.integers(0, L))


def _span_mix(rng, cptr, L, count):
    """`count` spans over the batch: lengths 1, whole contigs, spans from 0, spans to the end and interior ones, with
    random, singleton and full sets (and bit 31 at 32 labels), then the first ten again (duplicate queries)."""
    lens = np.diff(cptr)
    full_contigs = np.flatnonzero(lens > 0)
    long_ones = np.flatnonzero(lens >= 3)
    set_kinds = ["random", "singleton", "full", "random"] + (["bit31"] if L == 32 else [])
    spans = []
    for q in range(count):
        layout = ("one", "whole", "from0", "to_end", "interior")[q % 5]
        c = int(rng.choice(long_ones if layout == "interior" else full_contigs))
        if q == 1:
            c = int(np.argmax(lens))  # (the whole 300-item contig is among them)
        T = int(lens[c])
        if layout == "one":
            b = int(rng.integers(0, T))
            e = b + 1
        elif layout == "whole":
            b, e = 0, T
        elif layout == "from0":
            b, e = 0, int(rng.integers(1, T + 1))
        elif layout == "to_end":
            b, e = int(rng.integers(0, T)), T
        else:
            b = int(rng.integers(1, T - 1))
            e = int(rng.integers(b + 1, T))
        spans.append((c, b, e, _set_mask(rng, L, set_kinds[(q // 5) % len(set_kinds)])))
    return spans + spans[:10]


def _arrays(spans):
    sc, sb, se, sm = (np.array([s[k] for s in spans], dtype=np.int64) for k in range(4))
    return sc.astype(np.int32), sb.astype(np.int32), se.astype(np.int32), sm.astype(np.uint32)


def _yardstick(cptr, score, trans, spans):
    """(ref, bound) of every span on the lattice of the masked scores `score`."""
    L = score.shape[1]
    _, logz = cr.marginals(cptr, score, trans)
    ref, bound = np.zeros(len(spans)), np.zeros(len(spans))
    memo = {}
    for q, (c, b, e, m) in enumerate(spans):
        if (c, b, e, m) not in memo:
            g0, g1 = int(cptr[c]), int(cptr[c + 1])
            sc = score[g0:g1].copy()
            inside = tp.mask_matrix(np.array([m], dtype=np.uint32), L)[0]
            sc[b:e, ~inside] = -np.inf
            if np.any(np.all(np.isneginf(sc), axis=1)):
                inner = -np.inf  # (an item of the span allows no label of the set: no path, log Z_A' = -inf)
            else:
                inner = float(cr.marginals(np.array([0, g1 - g0]), sc, trans)[1][0])
            memo[(c, b, e, m)] = inner
        inner = memo[(c, b, e, m)]
        ref[q] = inner - logz[c]
        bound[q] = 1e-10 * ((max(1.0, abs(inner)) if np.isfinite(inner) else 1.0) + max(1.0, abs(logz[c])))
    return ref, bound


def _check(tag, got, ref, bound, spans=None, L=None):
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert not np.any(np.isnan(got)), f"{tag}: NaN"
    assert np.all(got <= 0.0), f"{tag}: a log-probability above 0"
    zero = np.isneginf(ref)
    fin = ~zero
    diff = np.abs(got[fin] - ref[fin])
    worst = float(diff.max()) if fin.any() else 0.0
    ratio = float((diff / bound[fin]).max()) if fin.any() else 0.0
    print(f"{tag}: {int(fin.sum())} finite / {int(zero.sum())} impossible spans, worst |logp - ref| = {worst:.3g}, "
          f"worst |logp - ref| / bound = {ratio:.3g}")
    assert np.array_equal(np.isneginf(got), zero), f"{tag}: -inf exactly where the yardstick has no path"
    assert np.all(diff <= bound[fin]), tag
    if spans is not None:
        full = np.array([s[3] == (1 << L) - 1 for s in spans])
        assert full.any() and np.all(got[full] == 0.0), f"{tag}: a full set is exactly 0.0"
        index = {}
        for q, s in enumerate(spans):
            if s in index:
                assert got[q].tobytes() == got[index[s]].tobytes(), f"{tag}: duplicate queries differ"
            index.setdefault(s, q)
    return worst, ratio


@functools.lru_cache(maxsize=None)
def _batch(L, lengths=None, n_spans=200):
    rng = np.random.default_rng(8100 + L)
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    cptr, gptr, attr = _csr(rng, _lengths(rng) if lengths is None else list(lengths))
    n = int(cptr[-1])
    return dict(L=L, w=w, trans=trans, cptr=cptr, gptr=gptr, attr=attr, csr=(cptr, gptr, attr), v=_values(rng, len(attr)),
                allowed=_wide_masks(rng, n, L), spans=tuple(_span_mix(rng, cptr, L, n_spans)))


def _score(b, valued, masked):
    every = tp.full_masks(int(b["cptr"][-1]), b["L"])
    return cr.masked_scores(b["gptr"], b["attr"], b["v"] if valued else None, b["w"], b["allowed"] if masked else every)


# ---------------------------------------------------------------- 1. against the yardstick
@pytest.mark.parametrize("valued,masked", KINDS)
@pytest.mark.parametrize("L", LABELS)
def test_spans_against_the_yardstick(nat, L, valued, masked):
    b = _batch(L)
    spans = list(b["spans"])
    if L == 32:
        assert any(s[3] >> 31 for s in spans)
    kw = dict(values=b["v"] if valued else None, allowed=b["allowed"] if masked else None)
    model = nat.Model.from_tables(b["w"], b["trans"])
    logp, marg, logz = model.span_log_probabilities(*b["csr"], *_arrays(spans), want_marginals=True, **kw)
    ref, bound = _yardstick(b["cptr"], _score(b, valued, masked), b["trans"], spans)
    assert np.isfinite(ref).sum() >= len(spans) // 3
    _check(f"L={L} values={valued} allowed={masked}", logp, ref, bound, spans, L)
    emarg, elogz = model.marginals_full(*b["csr"], **kw)
    assert marg.tobytes() == emarg.tobytes() and logz.tobytes() == elogz.tobytes(), "want_marginals: marginals_full's bytes"
    alone = model.span_log_probabilities(*b["csr"], *_arrays(spans), **kw)
    assert alone.tobytes() == logp.tobytes()


# ---------------------------------------------------------------- 2. every whole-contig arrangement
def _arrangement_lengths():
    rng = np.random.default_rng(77)
    return tuple([1, 2, 3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 300] + [int(x) for x in rng.integers(1, 90, size=20)])


def _boundary_spans(rng, cptr, L):
    """Spans that begin, end and cross at the chunk boundaries of the contigs of 63 items and more, each whole contig, and
    the 300-item contig under several sets."""
    spans = []
    lens = np.diff(cptr)
    for c in np.flatnonzero(lens >= 63):
        T = int(lens[c])
        marks = sorted({x for x in (0, 1, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, T - 1, T) if 0 <= x <= T})
        pairs = [(x, y) for x in marks for y in marks if x < y]
        for k in rng.choice(len(pairs), size=min(12, len(pairs)), replace=False):
            spans.append((int(c), pairs[k][0], pairs[k][1], _set_mask(rng, L, "random")))
        for x, y in ((31, 32), (32, 33), (31, 33), (32, 64), (33, 63), (0, 32), (0, T)):
            if y <= T:
                spans.append((int(c), x, y, _set_mask(rng, L, "random")))
    c300 = int(np.argmax(lens))
    spans += [(c300, 0, 300, (1 << L) - 1), (c300, 0, 300, 1), (c300, 64, 300, _set_mask(rng, L, "random"))]
    return spans


ARRANGEMENTS = [(L, "GECCO_CRF_GENERAL_CHUNKED", "0") for L in (3, 8)] + \
    [(L, "GECCO_CRF_GENERAL_MARGINALS", mode) for L in (9, 17, 32) for mode in ("wave", "chunked", "split")]


@pytest.mark.parametrize("L,switch,mode", ARRANGEMENTS)
def test_every_whole_contig_arrangement(nat, monkeypatch, L, switch, mode):
    lengths = _arrangement_lengths()
    assert {63, 64, 65, 66, 127, 128, 129, 300} <= set(lengths)
    b = _batch(L, lengths, 40)
    rng = np.random.default_rng(8300 + L)
    spans = _boundary_spans(rng, b["cptr"], L) + list(b["spans"])
    assert any(s[1:3] == (0, 300) for s in spans)
    monkeypatch.setenv(switch, mode)
    model = nat.Model.from_tables(b["w"], b["trans"])
    for valued, masked in ((True, True), (False, False)):
        kw = dict(values=b["v"] if valued else None, allowed=b["allowed"] if masked else None)
        logp, marg, logz = model.span_log_probabilities(*b["csr"], *_arrays(spans), want_marginals=True, **kw)
        ref, bound = _yardstick(b["cptr"], _score(b, valued, masked), b["trans"], spans)
        _check(f"L={L} {switch}={mode} values={valued} allowed={masked}", logp, ref, bound, spans, L)
        emarg, elogz = model.marginals_full(*b["csr"], **kw)
        assert marg.tobytes() == emarg.tobytes() and logz.tobytes() == elogz.tobytes()


# ---------------------------------------------------------------- 3. a leader outside the set
@pytest.mark.parametrize("L", [3, 17])
def test_a_label_outside_the_set_that_leads_by_800(nat, L):
    """One attribute gives label k a lead of 800 over every other label; it sits on one item of each contig, and k is outside
    every queried set.  With the masked recursion shifted by the maximum over all labels, the set's emissions at that item
    would all be exp(-800) = 0 and the result -inf or NaN; shifted by the maximum over the set it is finite and exact."""
    rng = np.random.default_rng(8600 + L)
    k, T, special = 1, 12, A - 1
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    w[special] = 0.0
    w[special, k] = 800.0 + 2.0 * np.abs(w).sum(axis=0).max()  # (a lead of at least 800 whatever else the item carries)
    leaders = [5, 2, T - 2, 0, T - 1]  # the item of every contig that carries the attribute
    cptr = np.arange(0, (len(leaders) + 1) * T, T).astype(np.int32)
    deg = rng.integers(1, 4, size=int(cptr[-1]))
    rows = [list(rng.integers(0, A - 1, size=d)) for d in deg]
    for c, p in enumerate(leaders):
        rows[c * T + p].append(special)
    gptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    attr = np.array([a for r in rows for a in r], dtype=np.int32)
    score = cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L))
    for c, p in enumerate(leaders):
        lead = score[c * T + p]
        assert lead[k] - np.delete(lead, k).max() >= 800.0
    others = ((1 << L) - 1) & ~(1 << k)
    layouts = [(0, 3, 8, "the leader in the middle of the span"), (0, 5, 6, "alone in a span of one item"),
               (1, 0, 5, "in a span that starts at the contig's start"), (2, T - 4, T, "in a span that ends at the contig's end"),
               (0, 6, 9, "on the item just before the span"), (0, 2, 5, "on the item just after the span"),
               (3, 0, 1, "alone on the contig's first item"), (3, 1, 4, "just before, on the contig's first item"),
               (4, T - 1, T, "alone on the contig's last item"), (4, T - 4, T - 1, "just after, on the contig's last item"),
               (0, 0, T, "inside a whole-contig span")]
    spans = [(c, b, e, others) for c, b, e, _ in layouts] + [(c, b, e, 1 << (0 if L == 3 else 7)) for c, b, e, _ in layouts]
    model = nat.Model.from_tables(w, trans)
    logp = model.span_log_probabilities(cptr, gptr, attr, *_arrays(spans))
    ref, bound = _yardstick(cptr, score, trans, spans)
    for (c, b, e, what), got, exp in zip(layouts, logp, ref):
        print(f"L={L} {what}: logp = {got!r}, ref = {exp!r}")
    assert np.all(np.isfinite(logp)) and np.all(np.isfinite(ref))
    assert ref[[0, 1, 2, 3, 6, 8, 10]].max() < -700.0  # (the spans that hold the leader cost its lead)
    _check(f"L={L} leader by 800", logp, ref, bound)


# ---------------------------------------------------------------- 4. consistency on the device
@pytest.mark.parametrize("L", [2, 5, 17])
def test_a_span_of_one_item_is_the_sum_of_its_marginals(nat, L):
    b = _batch(L) if L in LABELS else _batch(L, (1, 2, 7, 33, 64, 70))
    rng = np.random.default_rng(8900 + L)
    lens = np.diff(b["cptr"])
    spans = []
    for c in np.flatnonzero(lens > 0)[:12]:
        for t in range(int(lens[c])):
            spans.append((int(c), t, t + 1, _set_mask(rng, L, ("random", "singleton", "random")[t % 3])))
    for valued, masked in ((False, False), (True, True)):
        kw = dict(values=b["v"] if valued else None, allowed=b["allowed"] if masked else None)
        model = nat.Model.from_tables(b["w"], b["trans"])
        logp = model.span_log_probabilities(*b["csr"], *_arrays(spans), **kw)
        marg, _ = model.marginals_full(*b["csr"], **kw)
        worst = 0.0
        for (c, t, _, m), lp in zip(spans, logp):
            inside = tp.mask_matrix(np.array([m], dtype=np.uint32), L)[0]
            want = marg[int(b["cptr"][c]) + t][inside].sum()
            worst = max(worst, abs(np.exp(lp) - want) / (int(inside.sum()) * 1e-12))
            assert abs(np.exp(lp) - want) <= int(inside.sum()) * 1e-12, (c, t, m)
        print(f"L={L} values={valued} allowed={masked}: worst |exp(logp) - sum of marginals| / (k 1e-12) = {worst:.3g}")


def _sequence_crf(w, trans):
    from gecco_amd.crfsuite_model import model_bytes
    from gecco_amd.sequence import SequenceCRF

    An, L = w.shape
    names, classes = [f"a{k}" for k in range(An)], [f"l{k}" for k in range(L)]
    blob = model_bytes(classes, names, np.repeat(np.arange(An), L), np.tile(np.arange(L), An), np.repeat(np.arange(L), L),
                       np.tile(np.arange(L), L), np.concatenate([w.ravel(), trans.ravel()]))
    crf = SequenceCRF.from_bytes(blob, window_size=None)
    assert crf.classes_ == classes and crf.attributes_ == names
    return crf, names, classes


def _as_items(b, names):
    cptr, gptr, attr = b["csr"]
    return [[[names[a] for a in dict.fromkeys(attr[gptr[i]:gptr[i + 1]].tolist())] for i in range(cptr[s], cptr[s + 1])]
            for s in range(len(cptr) - 1)]


@pytest.mark.parametrize("L", [3, 17])
def test_a_whole_contig_span_is_log_likelihood_with_sets(nat, L):
    b = _batch(L, (1, 2, 9, 31, 32, 33, 64, 65, 100), 10)
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = _sequence_crf(w, b["trans"])
    X = _as_items(b, names)
    rng = np.random.default_rng(9000 + L)
    lens = np.diff(b["cptr"])
    spans, ysets = [], []
    for s, T in enumerate(lens.tolist()):
        m = _set_mask(rng, L, "random")
        members = [classes[y] for y in range(L) if (m >> y) & 1]
        spans.append((s, 0, T, members))
        ysets.append([set(members)] * T)
    got = crf.span_log_probability(X, spans)
    ll = crf.log_likelihood(X, ysets)
    cptr, gptr, attr = crf._pack(X)[:3]
    score = cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L))
    masks = [sum(1 << classes.index(y) for y in members) for _, _, _, members in spans]
    ref, bound = _yardstick(cptr, score, b["trans"], [(s, 0, int(T), m) for (s, T), m in zip(enumerate(lens.tolist()), masks)])
    print(f"L={L}: worst |span - log_likelihood| / bound = {(np.abs(got - ll) / bound).max():.3g}")
    _check(f"L={L} whole-contig spans", got, ref, bound)
    assert np.all(np.abs(got - ll) <= bound)


# ---------------------------------------------------------------- 5. path enumeration
def test_path_enumeration_of_every_span_and_set(nat):
    L = 3
    rng = np.random.default_rng(9100)
    w, trans = rng.normal(0.0, 1.5, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    cptr, gptr, attr = _csr(rng, [1, 2, 3, 4, 5, 6])
    n = int(cptr[-1])
    spans = [(c, b, e, m) for c in range(6) for b in range(c + 1) for e in range(b + 1, c + 2) for m in range(1, 8)]
    model = nat.Model.from_tables(w, trans)
    for masked in (False, True):
        allowed = _wide_masks(rng, n, L, 0.7) if masked else tp.full_masks(n, L)
        score = cr.masked_scores(gptr, attr, None, w, allowed)
        logz = [cr.enumerate_paths(score[cptr[c]:cptr[c + 1]], trans)[0] for c in range(6)]
        ref, bound = np.zeros(len(spans)), np.zeros(len(spans))
        for q, (c, b, e, m) in enumerate(spans):
            sc = score[cptr[c]:cptr[c + 1]].copy()
            sc[b:e, ~tp.mask_matrix(np.array([m], dtype=np.uint32), L)[0]] = -np.inf
            with np.errstate(invalid="ignore", divide="ignore"):
                dead = bool(np.any(np.all(np.isneginf(sc), axis=1)))
                inner = -np.inf if dead else cr.enumerate_paths(sc, trans)[0]
            ref[q] = inner - logz[c]
            bound[q] = 1e-10 * ((max(1.0, abs(inner)) if np.isfinite(inner) else 1.0) + max(1.0, abs(logz[c])))
        logp = model.span_log_probabilities(cptr, gptr, attr, *_arrays(spans), allowed=allowed if masked else None)
        _check(f"enumeration allowed={masked}", logp, ref, bound, spans, L)


# ---------------------------------------------------------------- 6. probability zero
@pytest.mark.parametrize("L", [3, 9])
def test_a_set_disjoint_from_the_allowed_labels_is_impossible(nat, L):
    rng = np.random.default_rng(9200 + L)
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    cptr, gptr, attr = _csr(rng, [10, 1, 40, 70])
    n = int(cptr[-1])
    allowed = tp.full_masks(n, L)
    pinned = [int(cptr[0]) + 4, int(cptr[1]), int(cptr[2]), int(cptr[3]) + 69]  # middle, a contig of one item, first and last items
    allowed[pinned] = 1
    away = ((1 << L) - 1) & ~1
    spans = [(0, 2, 7, away), (0, 4, 5, away), (0, 4, 10, away), (0, 0, 5, away), (1, 0, 1, away), (2, 0, 3, 2), (3, 60, 70, away),
             (3, 69, 70, 4), (0, 0, 4, away), (0, 5, 10, away), (0, 2, 7, 1 | 4), (3, 0, 70, (1 << L) - 1)]
    model = nat.Model.from_tables(w, trans)
    logp, marg, logz = model.span_log_probabilities(cptr, gptr, attr, *_arrays(spans), allowed=allowed, want_marginals=True)
    assert np.all(np.isneginf(logp[:8])) and np.all(np.isfinite(logp[8:])) and logp[-1] == 0.0
    assert not np.any(np.isnan(logp)) and not np.any(np.isnan(marg)) and not np.any(np.isnan(logz))
    ref, bound = _yardstick(cptr, cr.masked_scores(gptr, attr, None, w, allowed), trans, spans)
    _check(f"L={L} impossible spans", logp, ref, bound)


# ---------------------------------------------------------------- 7. refusals, empty calls, empty contigs, slices
def test_refusals_name_the_span(nat):
    L = 5
    rng = np.random.default_rng(9300)
    model = nat.Model.from_tables(rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L)))
    cptr, gptr, attr = _csr(rng, [4, 0, 9, 0, 3])
    good = [(0, 0, 4, 3), (2, 1, 5, 1)]
    bad = {"contig": (5, 0, 1, 1), "contig below 0": (-1, 0, 1, 1), "begin < 0": (0, -1, 2, 1), "begin >= end": (2, 3, 3, 1),
           "begin > end": (2, 5, 3, 1), "end beyond the contig": (2, 0, 10, 1), "a contig without genes": (1, 0, 1, 1),
           "mask 0": (0, 0, 2, 0), "a bit at L": (0, 0, 2, 1 << L), "bit 31": (0, 0, 2, (1 << 31) | 1)}
    for what, span in bad.items():
        with pytest.raises(ValueError, match="span 2") as err:
            model.span_log_probabilities(cptr, gptr, attr, *_arrays(good + [span]))
        print(f"{what}: {err.value}")
    # no spans: a successful call that still fills marg and lognorm
    logp, marg, logz = model.span_log_probabilities(cptr, gptr, attr, [], [], [], [], want_marginals=True)
    emarg, elogz = model.marginals_full(cptr, gptr, attr)
    assert logp.shape == (0,) and marg.tobytes() == emarg.tobytes() and logz.tobytes() == elogz.tobytes()
    assert model.span_log_probabilities(cptr, gptr, attr, [], [], [], []).shape == (0,)
    # a batch with empty contigs
    logp, marg, logz = model.span_log_probabilities(cptr, gptr, attr, *_arrays(good), want_marginals=True)
    score = cr.masked_scores(gptr, attr, None, model.state_weights()[0], tp.full_masks(int(cptr[-1]), L))
    ref, bound = _yardstick(cptr, score, model.trans_weights()[0], good)
    _check("empty contigs in the batch", logp, ref, bound)
    assert marg.tobytes() == emarg.tobytes() and logz.tobytes() == elogz.tobytes() and logz[1] == 0.0 and logz[3] == 0.0


@pytest.mark.parametrize("L", [2, 5, 12])
def test_a_slice_gives_the_bytes_of_the_rebased_batch(nat, L):
    """contig_ptr[0] > 0: span offsets are relative to their contig, the masks are indexed like gene_ptr's rows."""
    rng = np.random.default_rng(9400 + L)
    model = nat.Model.from_tables(rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L)))
    cptr, gptr, attr = _csr(rng, [4, 9, 3, 30, 1, 70])
    v = _values(rng, len(attr))
    allowed = _wide_masks(rng, int(cptr[-1]), L)
    g0 = int(cptr[2])
    a0 = int(gptr[g0])
    assert g0 > 0 and a0 > 0
    allowed[:g0] = 0  # (masks of genes outside the batch are not looked at)
    spans = [(0, 0, 3, _set_mask(rng, L, "random")), (1, 5, 30, _set_mask(rng, L, "random")), (2, 0, 1, (1 << L) - 1),
             (3, 64, 70, _set_mask(rng, L, "random")), (3, 0, 70, _set_mask(rng, L, "random")), (1, 0, 7, 1)]
    for kw_slice, kw_alone in ((dict(values=v, allowed=allowed), dict(values=v[a0:], allowed=allowed[g0:])),
                               (dict(), dict())):
        got = model.span_log_probabilities(cptr[2:], gptr, attr, *_arrays(spans), want_marginals=True, **kw_slice)
        alone = model.span_log_probabilities(cptr[2:] - g0, gptr[g0:] - a0, attr[a0:], *_arrays(spans), want_marginals=True, **kw_alone)
        for x, y in zip(got, alone):
            assert x.size and x.tobytes() == y.tobytes()
        assert np.any(np.isfinite(got[0]))
    score = cr.masked_scores(gptr[g0:] - a0, attr[a0:], v[a0:], model.state_weights()[0], allowed[g0:])
    got = model.span_log_probabilities(cptr[2:], gptr, attr, *_arrays(spans), values=v, allowed=allowed)
    ref, bound = _yardstick(cptr[2:] - g0, score, model.trans_weights()[0], spans)
    _check(f"L={L} slice", got, ref, bound)


# ---------------------------------------------------------------- 8. SequenceCRF
def test_sequence_crf_gives_the_native_calls_bytes(nat):
    L = 5
    b = _batch(L, (1, 6, 20, 33, 64, 3), 10)
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = _sequence_crf(w, b["trans"])
    X = _as_items(b, names)
    X.insert(2, [])
    rng = np.random.default_rng(9500)
    spans = [(0, 0, 1, "l0"), (1, 2, 5, {"l1", "l4"}), (3, 0, 20, ["l0", "l1", "l2", "l3"]), (4, 10, 33, ("l2",)),
             (5, 0, 64, frozenset(classes)), (6, 1, 2, "l3"), (1, 2, 5, {"l4", "l1"})]
    sets = [[None if rng.random() < 0.5 else {classes[int(rng.integers(0, L))], classes[int(rng.integers(0, L))], "l2"}
             for _ in xs] for xs in X]
    cptr, gptr, attr, _ = crf._pack(X)
    model = nat.Model.from_lcrf(crf.to_bytes())
    masks = [sum(1 << classes.index(y) for y in ([labs] if isinstance(labs, str) else labs)) for *_, labs in spans]
    arrays = _arrays([(s, a, e, m) for (s, a, e, _), m in zip(spans, masks)])
    for allowed in (None, sets):
        amasks = None if allowed is None else crf._label_sets(allowed, cptr, "allowed")[0]
        want = model.span_log_probabilities(cptr, gptr, attr, *arrays, allowed=amasks)
        got = crf.span_log_probability(X, spans, allowed=allowed)
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
        assert got[4] == 0.0 and got[1].tobytes() == got[6].tobytes() and np.any(got < -1e-3)
        assert crf.span_probability(X, spans, allowed=allowed).tobytes() == np.exp(want).tobytes()
    assert crf.span_log_probability(X, []).shape == (0,)
    with pytest.raises(ValueError, match="span 0"):
        crf.span_log_probability(X, [(2, 0, 1, "l0")])  # (the sequence without items holds no span)


# ---------------------------------------------------------------- 9. the typed front end
def _write_tables(directory, genes, rows=None):
    from gecco_amd import tables
    from tests.typed_planted import cluster_table

    os.makedirs(directory, exist_ok=True)
    tables.GeneTable.from_genes(genes).dump(os.path.join(directory, "genes.tsv"))
    tables.FeatureTable.from_genes(genes).dump(os.path.join(directory, "features.tsv"))
    if rows is not None:
        cluster_table(rows).dump(os.path.join(directory, "clusters.tsv"))


def _load(directory):
    from gecco_amd.train_cli import load_training_genes

    return load_training_genes(os.path.join(directory, "genes.tsv"), [os.path.join(directory, "features.tsv")], None, 1e-9)


def _dump(directory, crf, annotated, found):
    from gecco_amd import tables, typed

    os.makedirs(directory, exist_ok=True)
    tables.GeneTable.from_genes(annotated).dump(os.path.join(directory, "genes.tsv"))
    tables.FeatureTable.from_genes(annotated).dump(os.path.join(directory, "features.tsv"))
    typed.typed_cluster_table(found, crf.types_).dump(os.path.join(directory, "clusters.tsv"))


def _same_tables(a, b):
    for name in ("genes.tsv", "features.tsv", "clusters.tsv"):
        with open(os.path.join(a, name), "rb") as fa, open(os.path.join(b, name), "rb") as fb:
            assert fa.read() == fb.read(), name


def test_typed_front_end_reports_region_posteriors(nat, tmp_path):
    from gecco_amd import packing, tables, typed
    from gecco_amd.train_cli import join_clusters
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
    off_genes, off_clusters = crf.predict_genes_and_clusters(genes, region_posteriors=False)
    _dump(os.path.join(base, "plain"), crf, plain_genes, plain_clusters)
    _dump(os.path.join(base, "off"), crf, off_genes, off_clusters)
    _same_tables(os.path.join(base, "plain"), os.path.join(base, "off"))
    assert not any("region_p" in col for col in typed.typed_cluster_table(plain_clusters, crf.types_).columns)
    assert not any(hasattr(c, "region_probability") for c in plain_clusters)
    # the batch as the front end packs it, for the native call
    ordered = sorted(genes, key=operator.attrgetter("source.id", "start"))
    ids = [g.id for g in ordered]
    assert ids == [g.id for g in plain_genes]
    contigs = [list(g) for _, g in itertools.groupby(ordered, key=operator.attrgetter("source.id"))]
    batch = packing.pack_contigs(contigs, crf._attr_index, "protein")
    cptr, gptr, attr = batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id
    model = nat.Model.from_lcrf(crf._blob)
    not_bg = ((1 << L) - 1) & ~(1 << bg)
    type_masks = [sum(1 << l for l, names in enumerate(crf.label_types_) if t in names) for t in crf.types_]
    assert all(type_masks) and len(crf.types_) >= 2

    def check(found, known):
        """Every cluster's posteriors against the native call on its span and against the whole-contig marginals."""
        assert found and [c.id for c in found] == [c.id for c in crf.predict_clusters(genes, known=known, region_posteriors=True)]
        allowed = None if known is None else typed.known_masks(len(ordered), known, join_clusters(ordered, known, device=0),
                                                                crf.classes_, crf.background)
        where = []
        for cl in found:
            first, last = ids.index(cl.genes[0].id), ids.index(cl.genes[-1].id) + 1
            c = int(np.searchsorted(cptr, first, side="right")) - 1
            assert last <= cptr[c + 1] and last - first == len(cl.genes)
            where.append((c, first - int(cptr[c]), last - int(cptr[c])))
        queries = [(c, b, e, m) for c, b, e in where for m in [not_bg] + type_masks]
        logp, marg, logz = model.span_log_probabilities(cptr, gptr, attr, *_arrays(queries), allowed=allowed, want_marginals=True)
        prob = np.exp(logp).reshape(len(found), 1 + len(type_masks))
        logp = logp.reshape(len(found), 1 + len(type_masks))
        worst = -np.inf
        for cl, (c, b, e), row, prow in zip(found, where, logp, prob.tolist()):
            bound = 1e-10 * (max(1.0, abs(logz[c] + row[0])) + max(1.0, abs(logz[c])))
            assert cl.region_probability == prow[0], "region_p is the native call's value on the cluster's span"
            g0 = int(cptr[c])
            with np.errstate(divide="ignore"):
                floor = float(np.log(marg[g0 + b:g0 + e].sum(axis=1) - marg[g0 + b:g0 + e, bg]).min())
            assert row[0] <= floor + bound  # log region_p <= min over its genes of log P_whole(gene not background)
            assert set(cl.region_type_probabilities) == set(crf.types_)
            for t, lt, pt in zip(crf.types_, row[1:], prow[1:]):
                assert cl.region_type_probabilities[t] == pt
                assert lt <= row[0] + bound
                worst = max(worst, lt - row[0])
            worst = max(worst, row[0] - floor)
        print(f"known={'yes' if known is not None else 'no'}: {len(found)} clusters, largest excess over an upper bound = {worst:.3g}")
        return allowed

    annotated, found = crf.predict_genes_and_clusters(genes, region_posteriors=True)
    assert [c.id for c in found] == [c.id for c in plain_clusters]
    assert [g.average_probability for g in annotated] == [g.average_probability for g in plain_genes]
    check(found, None)
    table = typed.typed_cluster_table(found, crf.types_)
    assert "region_p" in table.columns and all(f"{t.lower()}_region_p" in table.columns for t in crf.types_)
    assert table.columns["region_p"] == [c.region_probability for c in found]
    # a known region of a type with its own label: that type's posterior over exactly that region is 1
    assert "Beta" in crf.classes_
    known = tables.ClusterTable({"sequence_id": ["fresh00"], "cluster_id": ["k1"], "start": [plain_genes[60].start],
                                 "end": [plain_genes[69].end], "type": ["Beta"]})
    k_annotated, k_found = crf.predict_genes_and_clusters(genes, known=known, region_posteriors=True)
    allowed = check(k_found, known)
    assert ids[60].startswith("fresh00") and cptr[0] == 0 and cptr[1] >= 70
    exact = model.span_log_probabilities(cptr, gptr, attr, [0], [60], [70], [type_masks[crf.types_.index("Beta")]], allowed=allowed)
    assert np.exp(exact[0]) >= 1.0 - 1e-12
    inside = [c for c in k_found if c.source.id == "fresh00" and {g.id for g in c.genes} <= set(ids[60:70])]
    for cl in inside:  # (a call that lies inside the known region is such a region too)
        assert cl.region_type_probabilities["Beta"] >= 1.0 - 1e-12 and cl.region_probability >= 1.0 - 1e-12
    print(f"calls inside the known region: {len(inside)}")
    # the command line with --region-posteriors writes the method's table
    crf.save(os.path.join(base, "model"))
    known.dump(os.path.join(base, "known.tsv"))
    _dump(os.path.join(base, "method"), crf, k_annotated, k_found)
    done = subprocess.run([sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
                           os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv"),
                           "--known", os.path.join(base, "known.tsv"), "--region-posteriors", "-o", os.path.join(base, "cli")],
                          cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    _same_tables(os.path.join(base, "method"), os.path.join(base, "cli"))
    with open(os.path.join(base, "cli", "clusters.tsv")) as fh:
        assert "region_p" in fh.readline().split("\t")
