"""Max-marginals on the device: ``gecco_crf_max_marginals`` against the independent yardstick (tests/maxmarg_reference.py:
path enumeration and a max-plus forward/backward whose restricted walks are plain Viterbi on masked tables), up through
``SequenceCRF.predict_max_marginals`` / ``span_best_scores`` and the typed front end's ``margins``.

The rule under rounding.  Every finite device value lies within B = 4 T eps (sum_t max_l |terms of s_t(l)| + (T - 1) max|A|) of
the yardstick's (maxmarg_reference.bound derives the 4 from the additions on a path through the forward and the backward
vector), every -inf sits exactly where the yardstick has one, and nothing is NaN.  Where every sum is exact (integer weights)
nothing is excused: every output is bit-equal to the yardstick's and the identities of the exact max-marginals hold with ==.

The batches are those of tests/test_gpu_kbest.py: labels 2, 4, 8, 9, 16, 17, 32; the enumeration lengths 1, 2, 3, 6 with an empty
sequence in the middle; the seam lengths 1 .. 300 mixed so that a wave's groups end at different steps; each plain, valued,
masked, and valued plus masked."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import kbest_reference as kr
from tests import maxmarg_reference as mr
from tests.test_gpu_kbest import (ROOT, SEAM_LABELS, SEAM_LENGTHS, enumeration_batch, kw, make_batch, seam_batch, sequence_crf,
                                  tables)

pytestmark = pytest.mark.gpu

KINDS = ((False, False), (True, False), (False, True), (True, True))  # (valued, masked)


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


# ---------------------------------------------------------------- queries and the yardstick
def label_sets(L, n_sets, seed=0):
    """``n_sets`` masks: the full set first, then random proper non-empty subsets."""
    rng = np.random.default_rng(9300 + 37 * L + seed)
    full = (1 << L) - 1
    out = [full]
    while len(out) < n_sets:
        m = int(rng.integers(1, full)) if full > 1 else 1
        out.append(m)
    return np.array(out[:n_sets], dtype=np.uint32)


def span_queries(b, seed=0, per_sequence=3):
    """(contig, begin, end, mask) arrays.  Per sequence with items: the whole sequence, its first item, its last item, and
    ``per_sequence`` random ranges (so every sequence carries several queries); masks are random non-empty sets, every fifth the
    full set; the order is shuffled."""
    rng = np.random.default_rng(9400 + 41 * b["L"] + seed)
    L, full = b["L"], (1 << b["L"]) - 1
    rows = []
    for c, T in enumerate(np.diff(b["cptr"]).tolist()):
        if T == 0:
            continue
        ranges = [(0, T), (0, 1), (T - 1, T)]
        for _ in range(per_sequence):
            lo = int(rng.integers(0, T))
            ranges.append((lo, int(rng.integers(lo + 1, T + 1))))
        for lo, hi in ranges:
            mask = full if len(rows) % 5 == 4 else int(rng.integers(1, full + 1))
            rows.append((c, lo, hi, mask))
    order = rng.permutation(len(rows))
    rows = [rows[k] for k in order]
    return (np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.int32),
            np.array([r[2] for r in rows], dtype=np.int32), np.array([r[3] for r in rows], dtype=np.uint32))


def reference(b, valued, masked, sets, spans, tag):
    """Per sequence the yardstick's dict (None for an empty sequence) and the bound, computed once per (batch, kind, tag), shared
    and left unchanged.  Enumeration where the lattice is small, else the max-plus forward/backward."""
    key = ("maxmarg", valued, masked, tag)
    if key not in b:
        score, absolute = tables(b, valued, masked)
        absT = np.abs(b["trans"])
        sc, sb, se, sm = spans
        out = []
        for c in range(len(b["cptr"]) - 1):
            g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
            if g1 == g0:
                out.append(None)
                continue
            mine = np.flatnonzero(sc == c)
            sp = [(int(sb[q]), int(se[q]), int(sm[q])) for q in mine]
            small = b["L"] ** (g1 - g0) <= 4096
            ref = (mr.enumerate_all if small else mr.all_quantities)(score[g0:g1], b["trans"], [int(m) for m in sets], sp)
            ref["queries"] = mine
            ref["bound"] = mr.bound(absolute[g0:g1], absT)
            out.append(ref)
        b[key] = out
    return b[key]


def close(tag, got, want, B, exact):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{tag}: shape {got.shape}, expected {want.shape}"
    assert not np.isnan(got).any(), f"{tag}: NaN"
    if exact:
        assert got.tobytes() == want.tobytes(), f"{tag}: not bit-equal to the yardstick"
        return 0.0
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), f"{tag}: -inf is not where the yardstick has it"
    assert not np.isposinf(got).any()
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    assert err <= B, f"{tag}: off by {err:.3g}, B = {B:.3g}"
    return err / B if B > 0 else 0.0


def accept(tag, b, ref, got, spans, exact=False):
    cptr = b["cptr"]
    worst = 0.0
    for c, r in enumerate(ref):
        g0, g1 = int(cptr[c]), int(cptr[c + 1])
        if r is None:
            assert got["best"][c] == 0.0, f"{tag}: an empty sequence has score 0"
            continue
        B = r["bound"]
        worst = max(worst, close(f"{tag} sequence {c} best", got["best"][c], r["best"], B, exact))
        for name in ("through", "inside", "outside"):
            if name in got:
                worst = max(worst, close(f"{tag} sequence {c} {name}", got[name][g0:g1], r[name], B, exact))
        for name in ("span_best", "span_broken"):
            if name in got:
                worst = max(worst, close(f"{tag} sequence {c} {name}", got[name][r["queries"]], r[name], B, exact))
    print(f"{tag}: worst |error| / B = {worst:.3g}")


def run_kinds(nat, b, tag, n_sets=3, exact=False, kinds=KINDS):
    model = nat.Model.from_tables(b["w"], b["trans"])
    sets, spans = label_sets(b["L"], n_sets), span_queries(b)
    for valued, masked in kinds:
        got = model.max_marginals(*b["csr"], sets=sets, spans=spans, **kw(b, valued, masked))
        ref = reference(b, valued, masked, sets, spans, tag)
        accept(f"{tag} L={b['L']} values={valued} allowed={masked}", b, ref, got, spans, exact=exact)
        _, score0, _, _ = model.viterbi_kbest(*b["csr"], 1, **kw(b, valued, masked))
        has = np.diff(b["cptr"]) > 0
        assert got["best"][has].tobytes() == np.ascontiguousarray(score0[has, 0]).tobytes(), "best has not the bits of the K-best rank 0"
    return model, sets, spans


# ---------------------------------------------------------------- 1. rounding: the enumeration batches and the seams
@pytest.mark.parametrize("L", SEAM_LABELS)
def test_enumeration_batches(nat, L):
    b = enumeration_batch(L)
    assert {1, 2, 3, 6} <= set(np.diff(b["cptr"]).tolist()) and np.diff(b["cptr"])[20] == 0
    run_kinds(nat, b, "enumeration")


@pytest.mark.parametrize("L", SEAM_LABELS)
def test_walks_at_the_seams(nat, L):
    b = seam_batch(L)
    assert set(SEAM_LENGTHS) <= set(np.diff(b["cptr"]).tolist())
    run_kinds(nat, b, "seams")


@pytest.mark.parametrize("L", [2, 5, 12])
def test_a_slice_gives_the_bytes_of_the_rebased_batch(nat, L):
    """``contig_ptr[0] > 0``."""
    b = make_batch(9500 + L, L, [4, 9, 3, 30, 1, 0, 70])
    model = nat.Model.from_tables(b["w"], b["trans"])
    cptr, gptr, attr = b["csr"]
    g0, a0 = int(cptr[2]), int(gptr[int(cptr[2])])
    assert g0 > 0 and a0 > 0
    allowed = b["allowed"].copy()
    allowed[:g0] = 0  # (masks of genes outside the batch are not looked at)
    sets = label_sets(L, 3)
    spans = (np.array([0, 1, 4, 1], dtype=np.int32), np.array([0, 2, 0, 29], dtype=np.int32), np.array([3, 30, 70, 30], dtype=np.int32),
             np.array([1, (1 << L) - 1, 2, 1], dtype=np.uint32))
    for kw_slice, kw_alone in ((dict(values=b["v"], allowed=allowed), dict(values=b["v"][a0:], allowed=allowed[g0:])), (dict(), dict())):
        got = model.max_marginals(cptr[2:], gptr, attr, sets=sets, spans=spans, want_lognorm=True, **kw_slice)
        alone = model.max_marginals(cptr[2:] - g0, gptr[g0:] - a0, attr[a0:], sets=sets, spans=spans, want_lognorm=True, **kw_alone)
        assert sorted(got) == sorted(alone) == ["best", "inside", "lognorm", "outside", "span_best", "span_broken", "through"]
        for name in got:
            assert got[name].size and got[name].tobytes() == alone[name].tobytes(), name
        assert got["through"].shape == (int(cptr[-1]) - g0, L) and got["best"][3] == 0.0


# ---------------------------------------------------------------- 2. integer weights: nothing is excused
@pytest.mark.parametrize("L", [2, 3, 5, 8, 17, 32])
def test_integer_weights_are_exact(nat, L):
    lengths = [1, 2, 3, 4, 5, 6, 0, 20, 40, 3, 2, 1, 33, 9] if L > 5 else [1, 2, 3, 4, 5, 6, 0, 3, 2, 1, 6, 5, 4]
    b = make_batch(9600 + L, L, lengths, integer=True)
    model, sets, spans = run_kinds(nat, b, "integer weights", exact=True, kinds=((False, False), (False, True)))
    sc, sb, se, sm = spans
    cptr = b["cptr"]
    for masked in (False, True):
        got = model.max_marginals(*b["csr"], sets=sets, spans=spans, **kw(b, False, masked))
        y, _ = model.viterbi(*b["csr"], **kw(b, False, masked))
        best_of_gene = np.repeat(got["best"], np.diff(cptr))
        assert np.all(got["through"].max(axis=1) == best_of_gene), "max_l through_t(l) == best at every item"
        assert np.all(got["through"][np.arange(len(y)), y] == best_of_gene), "through_t(y*_t) == best"
        assert np.all(got["inside"][:, 0] == best_of_gene) and np.all(np.isneginf(got["outside"][:, 0])), "the full set"
        assert np.all(np.maximum(got["inside"], got["outside"]) == best_of_gene[:, None])
        best_of_span = got["best"][sc]
        assert np.all(np.maximum(got["span_best"], got["span_broken"]) == best_of_span), "max(span_best, span_broken) == best"
        full = sm == (1 << L) - 1
        assert full.any() and np.all(got["span_best"][full] == best_of_span[full]) and np.all(np.isneginf(got["span_broken"][full]))
        stays = np.array([all((int(m) >> int(lab)) & 1 for lab in y[cptr[c] + lo:cptr[c] + hi]) for c, lo, hi, m in zip(sc, sb, se, sm)])
        assert stays.any() and not stays.all()
        assert np.all((best_of_span[stays] - got["span_best"][stays]) == 0.0), "the Viterbi path lies in the set: margin 0"
        # (the path leaves the set on the span: the best path inside is another one, at most as good; ties may make it as good)
        assert np.all(got["span_best"][~stays] <= best_of_span[~stays]) and np.all(got["span_broken"][~stays] == best_of_span[~stays])


# ---------------------------------------------------------------- 3. sets
@pytest.mark.parametrize("L", [2, 9, 32])
def test_sets(nat, L):
    b = seam_batch(L)
    model = nat.Model.from_tables(b["w"], b["trans"])
    spans = span_queries(b)
    every = label_sets(L, 32, seed=1)
    for valued, masked in ((True, False), (True, True)):
        many = model.max_marginals(*b["csr"], sets=every, **kw(b, valued, masked))
        assert many["inside"].shape == (int(b["cptr"][-1]), 32) and np.all(np.isneginf(many["outside"][:, 0])), "the full set has no outside"
        assert np.array_equal(many["inside"][:, 0], many["through"].max(axis=1))
        accept(f"32 sets L={L} values={valued} allowed={masked}", b, reference(b, valued, masked, every, spans, "sets32"), many, spans)
        for pick in ([5], [0], [31, 2, 17]):
            few = model.max_marginals(*b["csr"], sets=every[pick], **kw(b, valued, masked))
            assert few["inside"].shape[1] == len(pick)
            for col, s in enumerate(pick):
                for name in ("inside", "outside"):
                    assert np.ascontiguousarray(few[name][:, col]).tobytes() == np.ascontiguousarray(many[name][:, s]).tobytes(), \
                        f"set {s} alone and among 32: {name} differs"
            assert few["through"].tobytes() == many["through"].tobytes() and few["best"].tobytes() == many["best"].tobytes()


# ---------------------------------------------------------------- 4. spans
@pytest.mark.parametrize("L", [2, 8, 17])
def test_spans(nat, L):
    b = make_batch(9700 + L, L, [1, 12, 0, 40, 7, 1, 65])
    model = nat.Model.from_tables(b["w"], b["trans"])
    cptr = b["cptr"]
    full = (1 << L) - 1
    # a mask that leaves item 5 of sequence 3 only label 0, and a set without label 0: no path stays inside over that item
    allowed = np.full(int(cptr[-1]), full, dtype=np.uint32)
    allowed[int(cptr[3]) + 5] = 1
    rows = [(0, 0, 1, 1), (0, 0, 1, full), (5, 0, 1, full & ~1), (1, 0, 12, 2), (1, 0, 1, 1), (1, 11, 12, 1), (1, 3, 9, full), (3, 0, 40, 3),
            (3, 2, 9, full & ~1), (3, 5, 6, full & ~1), (3, 6, 40, full & ~1), (3, 2, 9, 1), (6, 0, 65, full), (6, 64, 65, 2), (6, 10, 30, 1)]
    spans = tuple(np.array([r[k] for r in rows], dtype=np.uint32 if k == 3 else np.int32) for k in range(4))
    got = model.max_marginals(*b["csr"], spans=spans, values=b["v"], allowed=allowed, want_through=True)
    score = tables(dict(b, allowed=allowed), True, True)[0]
    _, absolute = tables(b, True, False)
    for q, (c, lo, hi, m) in enumerate(rows):
        g0, g1 = int(cptr[c]), int(cptr[c + 1])
        B = mr.bound(absolute[g0:g1], np.abs(b["trans"]))
        close(f"span {q} best", got["span_best"][q], mr.span_best(score[g0:g1], b["trans"], lo, hi, m), B, False)
        close(f"span {q} broken", got["span_broken"][q], mr.span_broken_by_items(score[g0:g1], b["trans"], lo, hi, m), B, False)
        if m == full:
            assert got["span_best"][q] == got["best"][c] or abs(got["span_best"][q] - got["best"][c]) <= B
            assert np.isneginf(got["span_broken"][q]), "a full mask: nothing breaks it"
    assert np.isneginf(got["span_best"][8]) and np.isfinite(got["span_broken"][8]), "item 5 allows no label of the set"
    assert np.isneginf(got["span_best"][9]) and np.isfinite(got["span_broken"][9])
    assert np.isfinite(got["span_best"][10]) and np.isfinite(got["span_best"][11])
    # queries are independent: alone, in pairs on one sequence, and in another order -- byte for byte
    order = np.random.default_rng(L).permutation(len(rows))
    shuffled = model.max_marginals(*b["csr"], spans=tuple(a[order] for a in spans), values=b["v"], allowed=allowed, want_through=False)
    for name in ("span_best", "span_broken"):
        assert shuffled[name].tobytes() == got[name][order].tobytes(), f"{name} depends on the order of the queries"
    for pick in ([7], [8, 11], [3, 4], [14]):
        few = model.max_marginals(*b["csr"], spans=tuple(a[pick] for a in spans), values=b["v"], allowed=allowed, want_through=False)
        for name in ("span_best", "span_broken"):
            assert few[name].tobytes() == got[name][pick].tobytes(), f"{name} depends on the other queries"


# ---------------------------------------------------------------- 5. optional outputs, equal calls, log Z
@pytest.mark.parametrize("L", [2, 4, 17])
def test_optional_outputs_keep_the_others_bytes(nat, L):
    b = seam_batch(L)
    model = nat.Model.from_tables(b["w"], b["trans"])
    sets, spans = label_sets(L, 3), span_queries(b)
    for valued, masked in ((False, False), (True, True)):
        args = dict(sets=sets, spans=spans, want_lognorm=True, **kw(b, valued, masked))
        everything = model.max_marginals(*b["csr"], **args)
        again = model.max_marginals(*b["csr"], **args)
        assert sorted(everything) == ["best", "inside", "lognorm", "outside", "span_best", "span_broken", "through"]
        for name in everything:
            assert everything[name].tobytes() == again[name].tobytes(), f"two equal calls differ in {name}"
        _, elogz = model.marginals_full(*b["csr"], **kw(b, valued, masked))
        assert everything["lognorm"].tobytes() == elogz.tobytes(), "lognorm is not the marginals entry's"
        assert np.all(everything["best"] <= everything["lognorm"] + 1e-9)
        for drop in ("through", "inside", "outside", "span_best", "span_broken", "lognorm"):
            less = model.max_marginals(*b["csr"], **dict(args, **{"want_" + drop: False}))
            assert sorted(less) == sorted(set(everything) - {drop})
            for name in less:
                assert less[name].tobytes() == everything[name].tobytes(), f"without {drop}: {name} changes"
        bare = model.max_marginals(*b["csr"], want_through=False, **kw(b, valued, masked))
        assert list(bare) == ["best"] and bare["best"].tobytes() == everything["best"].tobytes()


def test_without_lognorm_no_transition_range_applies(nat):
    """The max walks read no exp(trans): a model the sum-product pass refuses is decoded, and refused only with lognorm."""
    b = make_batch(9800, 3, [5, 1, 9])
    trans = b["trans"] + 900.0
    model = nat.Model.from_tables(b["w"], trans)
    got = model.max_marginals(*b["csr"])
    score, _ = tables(b, False, False)
    for c in range(3):
        g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
        want = mr.through(score[g0:g1], trans)
        assert np.all(np.abs(got["through"][g0:g1] - want) <= 1e-9 * np.abs(want))
    with pytest.raises(Exception, match="outside \\[-700, 700\\]"):
        model.max_marginals(*b["csr"], want_lognorm=True)


# ---------------------------------------------------------------- 6. the sequence front end
@pytest.mark.parametrize("L", [2, 5, 17])
def test_sequence_front_end(nat, L):
    b = make_batch(9900 + L, L, [1, 2, 0, 9, 31, 64, 65, 3])
    w = b["w"].copy()
    w[w == 0] = 0.5
    b = dict(b, w=w)
    crf, names, classes = sequence_crf(w, b["trans"])
    cptr, gptr, attr = b["csr"]
    X = [[[names[a] for a in dict.fromkeys(attr[gptr[i]:gptr[i + 1]].tolist())] for i in range(cptr[s], cptr[s + 1])]
         for s in range(len(cptr) - 1)]
    # the yardstick on the items as the front end packs them (an attribute named twice counts once)
    packed = crf._pack(X)
    score, absolute = tables(dict(b, gptr=packed[1], attr=packed[2]), False, False)
    absT = np.abs(b["trans"])
    sets = [classes[0], {classes[0], classes[-1]}, list(classes)]
    bits = [1, 1 | (1 << (L - 1)), (1 << L) - 1]
    out = crf.predict_max_marginals(X, sets=sets)
    assert len(out) == len(X) and sorted(out[3]) == ["best", "inside", "margins", "outside", "through"]
    assert out[2]["through"].shape == (0, L) and out[2]["best"] == 0.0 and out[2]["inside"].shape == (0, 3)
    paths = crf.predict(X)
    for s, o in enumerate(out):
        g0, g1 = int(cptr[s]), int(cptr[s + 1])
        if g1 == g0:
            continue
        B = mr.bound(absolute[g0:g1], absT)
        th = mr.through(score[g0:g1], b["trans"])
        close(f"sequence {s} through", o["through"], th, B, False)
        close(f"sequence {s} best", o["best"], mr.viterbi_score(score[g0:g1], b["trans"]), B, False)
        ins, outs = mr.split_by_sets(th, bits)
        close(f"sequence {s} inside", o["inside"], ins, B, False)
        close(f"sequence {s} outside", o["outside"], outs, B, False)
        assert np.array_equal(o["margins"], o["through"] - o["best"]) and np.all(o["margins"] <= 2 * B)
        on_path = o["margins"][np.arange(g1 - g0), [classes.index(lab) for lab in paths[s]]]
        assert np.all(np.abs(on_path) <= 2 * B), "the margin of the Viterbi path's own label is 0 up to rounding"
    assert "inside" not in crf.predict_max_marginals(X)[3]
    # spans: against the yardstick, and against predict(X, allowed=...) on one copy of the sequence per span
    spans = [(3, 0, 9, classes[0]), (3, 2, 5, {classes[0], classes[-1]}), (4, 30, 31, classes[-1]), (5, 0, 64, list(classes)),
             (6, 10, 40, classes[0]), (0, 0, 1, classes[-1]), (7, 1, 3, {classes[-1]})]
    got = crf.span_best_scores(X, spans)
    assert sorted(got) == ["best", "broken", "inside"] and all(v.shape == (len(spans),) for v in got.values())
    copies = [X[k] for k, _, _, _ in spans]
    allowed = [[labels if lo <= t < hi else None for t in range(len(X[k]))] for k, lo, hi, labels in spans]
    pinned = crf.predict(copies, allowed=allowed)
    state, trans = crf._model.state_weights()[0], crf._model.trans_weights()[0]
    for q, (k, lo, hi, labels) in enumerate(spans):
        g0, g1 = int(cptr[k]), int(cptr[k + 1])
        B = mr.bound(absolute[g0:g1], absT)
        m = crf._label_bits("span", labels)
        close(f"span {q} inside", got["inside"][q], mr.span_best(score[g0:g1], b["trans"], lo, hi, m), B, False)
        close(f"span {q} broken", got["broken"][q], mr.span_broken_by_items(score[g0:g1], b["trans"], lo, hi, m), B, False)
        close(f"span {q} best", got["best"][q], mr.viterbi_score(score[g0:g1], b["trans"]), B, False)
        route = kr.path_score(score[g0:g1], trans, [classes.index(lab) for lab in pinned[q]])
        assert abs(got["inside"][q] - route) <= B, f"span {q}: {got['inside'][q]} against the copy-per-span route's {route}"
    assert state.shape == w.shape
    # the same score from the device's own constrained Viterbi on the copies
    copy_ptr = np.concatenate([[0], np.cumsum([cptr[k + 1] - cptr[k] for k, _, _, _ in spans])]).astype(np.int32)
    rows = np.concatenate([np.arange(cptr[k], cptr[k + 1]) for k, _, _, _ in spans])
    deg = np.diff(packed[1])[rows]
    copy_gptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    copy_attr = np.concatenate([packed[2][packed[1][g]:packed[1][g + 1]] for g in rows]).astype(np.int32)
    masks = crf._allowed(allowed, copy_ptr)
    _, vscore = crf._model.viterbi(copy_ptr, copy_gptr, copy_attr, allowed=masks)
    for q, (k, _, _, _) in enumerate(spans):
        B = mr.bound(absolute[int(cptr[k]):int(cptr[k + 1])], absT)
        assert abs(got["inside"][q] - vscore[q]) <= B, f"span {q}: {got['inside'][q]} against gecco_crf_viterbi_constrained's {vscore[q]}"
    assert all(v.size == 0 for v in crf.span_best_scores(X, []).values())


# ---------------------------------------------------------------- 7. refusals
def test_refusals_reach_the_caller(nat):
    b = make_batch(10000, 3, [3, 2])
    model = nat.Model.from_tables(b["w"], b["trans"])
    csr = b["csr"]
    one = lambda *r: tuple(np.array([x], dtype=np.uint32 if k == 3 else np.int32) for k, x in enumerate(r))  # noqa: E731
    cases = [
        (dict(sets=np.arange(1, 34, dtype=np.uint32) % 7 + 1), r"max_marginals: n_sets = 33 is outside 0 \.\. 32"),
        (dict(sets=[3, 0]), r"max_marginals: set 1: the label set is empty"),
        (dict(sets=[8]), r"max_marginals: set 0: the set holds a label at or above num_labels = 3"),
        (dict(sets=[]), r"max_marginals: inside or outside given without a label set"),
        (dict(spans=tuple(np.zeros(0, dtype=np.int32) for _ in range(4))), r"max_marginals: span_best or span_broken given without spans"),
        (dict(spans=one(2, 0, 1, 1)), r"max_marginals: span 0: contig 2 out of range"),
        (dict(spans=one(1, 0, 3, 1)), r"max_marginals: span 0: \[0, 3\) is not a non-empty range inside contig 1 of 2 genes"),
        (dict(spans=one(0, 2, 2, 1)), r"max_marginals: span 0: \[2, 2\) is not a non-empty range"),
        (dict(spans=one(0, -1, 2, 1)), r"max_marginals: span 0: \[-1, 2\) is not a non-empty range"),
        (dict(spans=one(0, 0, 1, 0)), r"max_marginals: span 0: the label set is empty"),
        (dict(spans=one(0, 0, 1, 8)), r"max_marginals: span 0: the set holds a label at or above num_labels = 3"),
        (dict(allowed=np.array([7, 7, 0, 7, 7], dtype=np.uint32)), r"constrained: gene 2 allows no label"),
        (dict(allowed=np.array([7, 7, 8, 7, 7], dtype=np.uint32)), r"constrained: gene 2 allows a label at or above num_labels"),
        (dict(values=np.array([np.nan] + [1.0] * (len(b["attr"]) - 1))), r"attribute value 0 is not finite"),
    ]
    for kwargs, text in cases:  # (GECCO_CRF_EINVAL is what _native raises as ValueError; any other status is a NativeError)
        with pytest.raises(ValueError, match=text):
            model.max_marginals(*csr, **kwargs)
    # the status itself, from the C entry
    lib = nat.load_library()
    head, _, _, _, _, _ = model._csr_head(*csr, None, None, 0)
    best = np.zeros(2)
    rc = lib.gecco_crf_max_marginals(*head, None, None, None, 33, None, None, None, None, 0, None, None, None, None, None,
                                     nat._ptr(best, nat._c_f64p), None)
    assert rc == nat.EINVAL == -1


# ---------------------------------------------------------------- 8. the typed front end
def test_typed_front_end_gives_margins(nat, tmp_path):
    import itertools
    import operator
    import random

    from gecco_amd import packing, tables as gtables, typed
    from tests import constrained_reference as cr
    from tests import test_gpu_spans as gs
    from tests import train_objective_partial as tp
    from tests.typed_planted import C, W, planted_set

    train_genes, train_rows = planted_set(11, 12, "train", composite=True)
    fresh_genes, _ = planted_set(12, 2, "fresh", composite=False)
    base = str(tmp_path)
    gs._write_tables(os.path.join(base, "train"), train_genes, train_rows)
    gs._write_tables(os.path.join(base, "fresh"), fresh_genes)
    random.seed(42)
    np.random.seed(42)
    crf = typed.TypedClusterCRF(W, 1, c1=C, c2=C)
    crf.fit(gs._load(os.path.join(base, "train")), gtables.ClusterTable.load(os.path.join(base, "train", "clusters.tsv")))
    genes = gs._load(os.path.join(base, "fresh"))
    # without the option: the tables of a call that omits the argument, byte for byte, and no attribute
    plain_genes, plain_clusters = crf.predict_genes_and_clusters(genes)
    off_genes, off_clusters = crf.predict_genes_and_clusters(genes, margins=False)
    gs._dump(os.path.join(base, "plain"), crf, plain_genes, plain_clusters)
    gs._dump(os.path.join(base, "off"), crf, off_genes, off_clusters)
    gs._same_tables(os.path.join(base, "plain"), os.path.join(base, "off"))
    assert not any(hasattr(c, "margin_present") for c in off_clusters)
    found = crf.predict_clusters(genes, margins=True)
    assert found and [c.id for c in found] == [c.id for c in plain_clusters]
    # the batch as the front end packs it, and the yardstick's tables
    ordered = sorted(genes, key=operator.attrgetter("source.id", "start"))
    ids = [g.id for g in ordered]
    contigs = [list(g) for _, g in itertools.groupby(ordered, key=operator.attrgetter("source.id"))]
    batch = packing.pack_contigs(contigs, crf._attr_index, "protein")
    cptr, gptr, attr = batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id
    model = nat.Model.from_lcrf(crf._blob)
    L, bg = len(crf.classes_), crf.classes_.index("0")
    weights, trans = model.state_weights()[0], model.trans_weights()[0]
    every = tp.full_masks(int(cptr[-1]), L)
    score = cr.masked_scores(gptr, attr, None, weights, every)
    absolute = cr.masked_scores(gptr, attr, None, np.abs(weights), every)
    assert int(np.diff(gptr).max()) <= 3, "the bound's constant is derived for items of at most 3 attributes"
    best = model.viterbi(cptr, gptr, attr)[0]
    not_bg = ((1 << L) - 1) & ~(1 << bg)
    contained = 0
    for cl in found:
        first, last = ids.index(cl.genes[0].id), ids.index(cl.genes[-1].id) + 1
        c = int(np.searchsorted(cptr, first, side="right")) - 1
        c0, c1 = int(cptr[c]), int(cptr[c + 1])
        B = mr.bound(absolute[c0:c1], np.abs(trans))
        lo, hi = first - c0, last - c0
        top = mr.viterbi_score(score[c0:c1], trans)
        assert abs(cl.margin_present - (top - mr.span_best(score[c0:c1], trans, lo, hi, not_bg))) <= 2 * B
        assert abs(cl.margin_absent - (top - mr.span_best(score[c0:c1], trans, lo, hi, 1 << bg))) <= 2 * B
        assert abs(cl.margin_broken - (top - mr.span_broken_by_items(score[c0:c1], trans, lo, hi, not_bg))) <= 2 * B
        assert sorted(cl.type_margins) == sorted(crf.types_)
        for t, value in cl.type_margins.items():
            mask = sum(1 << l for l, names in enumerate(crf.label_types_) if t in names)
            assert abs(value - (top - mr.span_best(score[c0:c1], trans, lo, hi, mask))) <= 2 * B
        for value in (cl.margin_present, cl.margin_absent, cl.margin_broken, *cl.type_margins.values()):
            assert value >= -B and not np.isnan(value)
        if np.all(best[first:last] != bg):
            contained += 1
            assert cl.margin_present == 0.0, "the Viterbi path keeps the whole call inside a cluster"
            assert cl.margin_absent >= -B and cl.margin_broken >= -B
    print(f"{len(found)} clusters, {contained} contained in the Viterbi path")
    assert contained
    # the command line writes the three columns
    crf.save(os.path.join(base, "model"))
    done = subprocess.run([sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
                           os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv"),
                           "--margins", "-o", os.path.join(base, "cli")], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    with open(os.path.join(base, "cli", "clusters.tsv")) as fh:
        lines = [line.rstrip("\n").split("\t") for line in fh]
    with open(os.path.join(base, "plain", "clusters.tsv")) as fh:
        plain = [line.rstrip("\n").split("\t") for line in fh]
    added = [k for k, name in enumerate(lines[0]) if name not in plain[0]]
    assert [lines[0][k] for k in added] == ["margin_present", "margin_absent", "margin_broken"]
    assert [[x for k, x in enumerate(row) if k not in added] for row in lines] == plain, "the other columns are unchanged"
    for row, cl in zip(lines[1:], found):
        assert [float(row[k]) for k in added] == [cl.margin_present, cl.margin_absent, cl.margin_broken]
