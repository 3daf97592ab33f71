"""Run posteriors on the device: ``gecco_crf_run_posteriors`` -- the exact start and end distributions of the run through an
anchor, and the probability that a run is exactly a range -- against the independent numpy yardstick (tests/runs_reference.py),
and up through ``SequenceCRF`` and the typed front end.

The yardstick of every entry is ``ref = log Z_A' - log Z_A`` (tests/runs_reference.py): whole distributions from its direct
recursion (b), a seeded sample of entries of every family from its definition (a) as well.  The tolerance per entry is the
project's own for log-ratios, ``1e-10 (max(1, |log Z_A'|) + max(1, |log Z_A|))``.  Where the yardstick is -inf the result has to
be -inf, and the other way round.  Every test prints its worst |difference| / bound and its counts of finite entries."""
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
from tests import runs_reference as rr
from tests import test_gpu_spans as sp
from tests import train_objective_partial as tp

pytestmark = pytest.mark.gpu

LABELS = [2, 3, 8, 17, 32]
KINDS = sp.KINDS  # (with values, with allowed masks)
REACHES = [0, 1, 7, 64, 400]  # (400 exceeds the longest sequence)
KEYS = ("log_anchor", "log_start", "log_start_beyond", "log_end", "log_end_beyond")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


# ---------------------------------------------------------------- batches, queries and the yardstick
def _proper_mask(rng, L, kind):
    """`kind` of tests/test_gpu_spans.py, with "random" a PROPER subset (at least one label outside)."""
    full = (1 << L) - 1
    m = sp._set_mask(rng, L, kind)
    if kind in ("random", "bit31") and m == full:
        m &= ~(1 << int(rng.integers(0, min(L, 31))))
    return m


def _anchor_mix(rng, cptr, L, count=100):
    """About `count` anchors over the batch: item 0, the last item, sequences of one item, interior items, with random proper,
    singleton and full sets (and bit 31 at 32 labels), then the first eight again (duplicate queries)."""
    lens = np.diff(cptr)
    full_contigs, ones = np.flatnonzero(lens > 0), np.flatnonzero(lens == 1)
    set_kinds = ["random", "singleton", "random", "full"] + (["bit31"] if L == 32 else [])
    anchors = []
    for q in range(count - 8):
        layout = ("first", "last", "interior", "interior", "one")[q % 5]
        c = int(rng.choice(ones if layout == "one" else full_contigs))
        if q in (2, 3, 7, 8, 12):
            c = int(np.argmax(lens))  # (the 300-item sequence: offsets beyond 64)
        T = int(lens[c])
        a = 0 if layout == "first" else T - 1 if layout == "last" else int(rng.integers(0, T))
        anchors.append((c, a, _proper_mask(rng, L, set_kinds[(q // 5) % len(set_kinds)])))
    return anchors + anchors[:8]


def _anchor_arrays(anchors):
    c, a, m = (np.array([s[k] for s in anchors], dtype=np.int64) for k in range(3))
    return c.astype(np.int32), a.astype(np.int32), m.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _family(L, valued, masked):
    """One (label count, kind) family on the batch of tests/test_gpu_spans.py: the batch, the masks (denser at 2 and 3 labels: at
    p = 0.8 only 22 % and 39 % of the entries there keep a path), the masked scores, the anchors and the closed runs."""
    b = sp._batch(L)
    n = int(b["cptr"][-1])
    rng = np.random.default_rng(9700 + 10 * L + 2 * valued + masked)
    allowed = None
    if masked:
        allowed = sp._wide_masks(np.random.default_rng(9600 + L), n, L, 0.9) if L <= 3 else b["allowed"]
    score = cr.masked_scores(b["gptr"], b["attr"], b["v"] if valued else None, b["w"], allowed if masked else tp.full_masks(n, L))
    return dict(b=b, L=L, allowed=allowed, values=b["v"] if valued else None, score=score, trans=b["trans"], cptr=b["cptr"],
                anchors=tuple(_anchor_mix(rng, b["cptr"], L)), runs=tuple(sp._span_mix(rng, b["cptr"], L, 120)), fb={})


def _fb(f, c):
    if c not in f["fb"]:
        g0, g1 = int(f["cptr"][c]), int(f["cptr"][c + 1])
        f["fb"][c] = rr.forward_backward(f["score"][g0:g1], f["trans"])
    return f["fb"][c]


def _seq(f, c):
    return f["score"][int(f["cptr"][c]):int(f["cptr"][c + 1])]


@functools.lru_cache(maxsize=None)
def _anchor_reference(L, valued, masked, reach):
    """(values, log Z_A', bounds) of the family's anchors at `reach` by the direct recursion, stacked under the product's keys."""
    f = _family(L, valued, masked)
    val, inn, bnd = ({k: [] for k in KEYS} for _ in range(3))
    memo = {}
    for c, a, m in f["anchors"]:
        if (c, a, m) not in memo:
            memo[(c, a, m)] = rr.anchor_direct(_seq(f, c), f["trans"], a, m, reach, _fb(f, c))
        v, tot, logz = memo[(c, a, m)]
        for k in KEYS:
            val[k].append(v[k])
            inn[k].append(tot[k])
            bnd[k].append(rr.bound(tot[k], logz))
    return tuple({k: np.array(x[k], dtype=np.float64) for k in KEYS} for x in (val, inn, bnd))


def _compare(tag, got, ref, bound):
    """Worst |difference| / bound over the finite entries; -inf exactly where the yardstick has no path; never NaN, never > 0."""
    got, ref, bound = (np.asarray(x, dtype=np.float64) for x in (got, ref, bound))
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert not np.any(np.isnan(got)), f"{tag}: NaN"
    assert np.all(got <= 0.0), f"{tag}: a log-probability above 0"
    fin = np.isfinite(ref)
    assert np.array_equal(np.isneginf(got), ~fin), f"{tag}: -inf exactly where the yardstick has no path"
    ratio = float((np.abs(got[fin] - ref[fin]) / bound[fin]).max()) if fin.any() else 0.0
    assert ratio <= 1.0, f"{tag}: worst |difference| / bound = {ratio}"
    return ratio, int(fin.sum())


def _run(nat, f, anchors=None, reach=64, runs=None, **kw):
    model = nat.Model.from_tables(f["b"]["w"], f["trans"])
    return model.run_posteriors(*f["b"]["csr"], anchors=None if anchors is None else _anchor_arrays(anchors), reach=reach,
                                runs=None if runs is None else sp._arrays(runs), values=f["values"], allowed=f["allowed"], **kw)


# ---------------------------------------------------------------- 0. the conditions on the yardstick alone
@pytest.mark.parametrize("valued,masked", KINDS)
@pytest.mark.parametrize("L", LABELS)
def test_the_families_hold_what_the_checks_need(L, valued, masked):
    """Conditions, not measurements: without masks a proper subset is finite at every offset inside the sequence; with masks
    every family holds at least 100 finite yardstick entries at offsets >= 8."""
    f = _family(L, valued, masked)
    val, _, _ = _anchor_reference(L, valued, masked, 400)
    lens = np.diff(f["cptr"])
    far = 0
    for q, (c, a, m) in enumerate(f["anchors"]):
        T = int(lens[c])
        far += int(np.isfinite(val["log_start"][q][8:]).sum() + np.isfinite(val["log_end"][q][8:]).sum())
        if not masked and m != (1 << L) - 1:
            assert np.all(np.isfinite(val["log_start"][q][:a + 1])) and np.all(np.isneginf(val["log_start"][q][a + 1:]))
            assert np.all(np.isfinite(val["log_end"][q][:T - a])) and np.all(np.isneginf(val["log_end"][q][T - a:]))
            assert np.isfinite(val["log_anchor"][q])
    print(f"L={L} values={valued} allowed={masked}: {far} finite yardstick entries at offsets >= 8")
    assert far >= 100
    if L == 32:
        assert any(m >> 31 for _, _, m in f["anchors"])
    assert any(m == (1 << L) - 1 for _, _, m in f["anchors"]) and any(lens[c] == 1 for c, _, _ in f["anchors"])


# ---------------------------------------------------------------- 1. anchors against the yardstick, at every reach
@pytest.mark.parametrize("valued,masked", KINDS)
@pytest.mark.parametrize("L", LABELS)
def test_anchors_against_the_yardstick(nat, L, valued, masked):
    f = _family(L, valued, masked)
    anchors = list(f["anchors"])
    out = {reach: _run(nat, f, anchors, reach, want_marginals=(reach == 64)) for reach in REACHES}
    worst, finite = 0.0, 0
    for reach in REACHES:
        val, _, bnd = _anchor_reference(L, valued, masked, reach)
        for k in KEYS:
            assert out[reach][k].dtype == np.float64
            ratio, n = _compare(f"L={L} values={valued} allowed={masked} reach={reach} {k}", out[reach][k], val[k], bnd[k])
            worst, finite = max(worst, ratio), finite + n
    print(f"L={L} values={valued} allowed={masked}: {finite} finite entries over the reaches {REACHES}, worst |difference| / bound = {worst:.3g}")
    # a seeded sample of entries against the definition (a)
    rng = np.random.default_rng(9800 + L)
    got, worst_a, finite_a = out[64], 0.0, 0
    for q in rng.choice(len(anchors), size=12, replace=False).tolist():
        c, a, m = anchors[q]
        for what, key, r in (("anchor", "log_anchor", 0), ("start", "log_start", int(rng.integers(0, 65))), ("end", "log_end", int(rng.integers(0, 65))),
                             ("start", "log_start", min(a, 64)), ("start_beyond", "log_start_beyond", 0), ("end_beyond", "log_end_beyond", 0)):
            ref, inner, logz = rr.anchor_entry_by_definition(_seq(f, c), f["trans"], a, m, what, r=r, reach=64)
            value = got[key][q][r] if got[key].ndim == 2 else got[key][q]
            ratio, n = _compare(f"(a) {key}[{q}][{r}]", [value], [ref], [rr.bound(inner, logz)])
            worst_a, finite_a = max(worst_a, ratio), finite_a + n
    print(f"  against the definition: {finite_a} finite entries, worst |difference| / bound = {worst_a:.3g}")
    # a full set: log_anchor exactly 0.0 without masks, every start but item 0 and every end but the last item -inf
    for q, (c, a, m) in enumerate(anchors):
        if m == (1 << L) - 1:
            assert got["log_anchor"][q] == 0.0
            assert np.all(np.isneginf(np.delete(got["log_start"][q], a))) if a <= 64 else np.all(np.isneginf(got["log_start"][q]))
    # the identity: the starts (+) the mass beyond = the anchor, and the same for the ends
    for reach in (7, 64):
        o = out[reach]
        _, inn, bnd = _anchor_reference(L, valued, masked, reach)
        for side in ("start", "end"):
            rows = np.concatenate([o[f"log_{side}"], o[f"log_{side}_beyond"][:, None]], axis=1)
            for q in range(len(anchors)):
                total = rr._lse(rows[q])
                if np.isneginf(o["log_anchor"][q]):
                    assert np.isneginf(total)
                else:  # (every term within its bound: the sum within the largest of them, and the anchor within its own)
                    tol = max(bnd[f"log_{side}"][q].max(), bnd[f"log_{side}_beyond"][q]) + bnd["log_anchor"][q]
                    assert abs(total - o["log_anchor"][q]) <= tol, (side, q, total, o["log_anchor"][q])
    # entry r is the same bits at every reach >= r
    for lo, hi in ((0, 1), (1, 7), (7, 64), (64, 400)):
        for k in ("log_start", "log_end"):
            assert out[lo][k].tobytes() == np.ascontiguousarray(out[hi][k][:, :lo + 1]).tobytes(), f"{k}: reach {lo} against {hi}"
        assert out[lo]["log_anchor"].tobytes() == out[hi]["log_anchor"].tobytes()
    # marg and lognorm are marginals_full's bytes
    model = nat.Model.from_tables(f["b"]["w"], f["trans"])
    emarg, elogz = model.marginals_full(*f["b"]["csr"], values=f["values"], allowed=f["allowed"])
    assert out[64]["marginals"].tobytes() == emarg.tobytes() and out[64]["lognorm"].tobytes() == elogz.tobytes()


# ---------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("L", [3, 32])
def test_equal_queries_give_equal_bytes_in_any_order(nat, L):
    f = _family(L, True, True)
    anchors, runs = list(f["anchors"]), list(f["runs"])
    one = _run(nat, f, anchors, 64, runs)
    two = _run(nat, f, anchors, 64, runs)
    for k in KEYS + ("log_run",):
        assert one[k].tobytes() == two[k].tobytes(), f"{k}: a repeated call"
    for name, queries, keys in (("anchor", anchors, KEYS), ("run", runs, ("log_run",))):
        first = {}
        for q, s in enumerate(queries):
            if s in first:
                for k in keys:
                    assert one[k][q].tobytes() == one[k][first[s]].tobytes(), f"{k}: duplicate {name} queries differ"
            first.setdefault(s, q)
        assert len(first) < len(queries)
    rng = np.random.default_rng(9900 + L)
    pa, pr = rng.permutation(len(anchors)), rng.permutation(len(runs))
    shuffled = _run(nat, f, [anchors[i] for i in pa], 64, [runs[i] for i in pr])
    for k in KEYS:
        assert shuffled[k].tobytes() == np.ascontiguousarray(one[k][pa]).tobytes(), f"{k}: the order of the queries"
    assert shuffled["log_run"].tobytes() == np.ascontiguousarray(one["log_run"][pr]).tobytes()
    # either list alone gives the same bits as both together
    alone_a, alone_r = _run(nat, f, anchors, 64), _run(nat, f, None, 64, runs)
    assert all(alone_a[k].tobytes() == one[k].tobytes() for k in KEYS) and alone_r["log_run"].tobytes() == one["log_run"].tobytes()
    assert "log_run" not in alone_a and "log_anchor" not in alone_r


# ---------------------------------------------------------------- 3. a leader outside the set
@pytest.mark.parametrize("L", [3, 17])
def test_a_label_outside_the_set_that_leads_inside_the_walk(nat, L):
    """At a few items inside the walks a label outside S leads every label of S by 300 .. 700; at others a label of S leads.
    Shifted by the maximum over all labels the set's emissions would be flushed and the results -inf; shifted by the maximum
    over S they are finite and exact."""
    A = sp.A
    rng = np.random.default_rng(9950 + L)
    k, inside_leader, T = 1, 0, 24
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    leads = {A - 1: 320.0, A - 2: 480.0, A - 3: 640.0}  # attribute -> the lead it gives label k (outside S)
    for att, lead in leads.items():
        w[att] = 0.0
        w[att, k] = lead
    w[A - 4] = 0.0
    w[A - 4, inside_leader] = 40.0  # a label of S that leads
    places = {3: A - 1, 9: A - 2, 10: A - 4, 15: A - 3, 20: A - 4, 0: A - 4}  # item of every sequence -> its special attribute
    n_seq = 3
    cptr = np.arange(0, (n_seq + 1) * T, T).astype(np.int32)
    rows = [list(rng.integers(0, A - 4, size=int(d))) for d in rng.integers(1, 3, size=int(cptr[-1]))]
    for c in range(n_seq):
        for item, att in places.items():
            rows[c * T + item].append(att)
    gptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    attr = np.array([x for r in rows for x in r], dtype=np.int32)
    score = cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L))
    others = ((1 << L) - 1) & ~(1 << k)
    for item, att in places.items():
        lead = score[item, k] - np.delete(score[item], k).max()
        assert (300.0 <= lead <= 700.0) if att in leads else (score[item, inside_leader] - score[item, k] >= 20.0), (item, lead)
    sets = [others, 1 << inside_leader, (1 << inside_leader) | (1 << 2)]
    anchors = [(c, a, m) for c, a in ((0, 12), (1, 6), (2, 22), (0, 10), (1, 0), (2, T - 1), (0, 3)) for m in sets]
    runs = [(c, b, e, m) for c, b, e in ((0, 5, 18), (1, 0, T), (2, 9, 11), (0, 3, 4), (1, 2, 16), (2, 4, 9)) for m in sets]
    model = nat.Model.from_tables(w, trans)
    got = model.run_posteriors(cptr, gptr, attr, anchors=_anchor_arrays(anchors), reach=T, runs=sp._arrays(runs))
    worst, finite = 0.0, 0
    for q, (c, a, m) in enumerate(anchors):
        X = score[c * T:(c + 1) * T]
        val, tot, logz = rr.anchor_direct(X, trans, a, m, T)
        assert np.all(np.isfinite(val["log_start"][:a + 1])) and np.all(np.isfinite(val["log_end"][:T - a]))
        for key in KEYS:
            ratio, n = _compare(f"L={L} leader outside, anchor {q} {key}", got[key][q], val[key], rr.bound(tot[key], logz))
            worst, finite = max(worst, ratio), finite + n
        assert np.all(np.isfinite(got["log_start"][q][:a + 1])) and np.all(np.isfinite(got["log_end"][q][:T - a]))
    low = 0
    for q, (c, b, e, m) in enumerate(runs):
        ref, inner, logz = rr.run_by_definition(score[c * T:(c + 1) * T], trans, b, e, m)
        assert np.isfinite(ref)
        low += ref < -300.0
        ratio, n = _compare(f"L={L} leader outside, run {q}", [got["log_run"][q]], [ref], [rr.bound(inner, logz)])
        worst, finite = max(worst, ratio), finite + n
    assert low >= 6  # (the runs that hold a leader cost its lead)
    print(f"L={L} leader outside: {finite} finite entries, worst |difference| / bound = {worst:.3g}")


# ---------------------------------------------------------------- 4. a long reach
def test_a_start_1500_items_away_keeps_its_relative_accuracy(nat):
    """One sequence of 2000 items under a strongly sticky model: a run of the one label of S that reaches 1500 items back from
    the anchor has a probability around e^-600.  It is finite and within the tolerance of its log."""
    L, T, A = 4, 2000, sp.A
    rng = np.random.default_rng(9960)
    w = rng.normal(0.0, 0.3, size=(A, L))
    trans = rng.normal(0.0, 0.1, size=(L, L)) + 2.0 * np.eye(L)
    cptr, gptr, attr = sp._csr(rng, [T, 7], max_attrs=2)
    score = cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L))
    anchors = [(0, 1990, 2), (0, 1000, 2), (0, 5, 2), (0, 1990, 2 | 4), (1, 3, 2)]
    model = nat.Model.from_tables(w, trans)
    got = model.run_posteriors(cptr, gptr, attr, anchors=_anchor_arrays(anchors), reach=T)
    fb = rr.forward_backward(score[:T], trans)
    worst, finite = 0.0, 0
    for q, (c, a, m) in enumerate(anchors):
        X = score[int(cptr[c]):int(cptr[c + 1])]
        val, tot, logz = rr.anchor_direct(X, trans, a, m, T, fb if c == 0 else None)
        for key in KEYS:
            ratio, n = _compare(f"long reach, anchor {q} {key}", got[key][q], val[key], rr.bound(tot[key], logz))
            worst, finite = max(worst, ratio), finite + n
        if q == 0:
            far = val["log_start"][1500:1991]
            print(f"  starts 1500 .. 1990 items away: log p from {far.max():.1f} down to {far.min():.1f}")
            assert np.all(np.isfinite(far)) and far.max() < -450.0 and far.min() < -600.0
            assert np.all(np.isfinite(got["log_start"][q][1500:1991]))
    print(f"long reach: {finite} finite entries, worst |difference| / bound = {worst:.3g}")


# ---------------------------------------------------------------- 5. closed runs
@pytest.mark.parametrize("valued,masked", KINDS)
@pytest.mark.parametrize("L", LABELS)
def test_closed_runs_against_the_yardstick(nat, L, valued, masked):
    f = _family(L, valued, masked)
    runs = list(f["runs"])
    lens = np.diff(f["cptr"])
    assert any(b == 0 and e == lens[c] for c, b, e, _ in runs) and any(e - b == 1 for _, b, e, _ in runs)
    got = _run(nat, f, None, 64, runs)["log_run"]
    rows, ref, bnd = {}, np.zeros(len(runs)), np.zeros(len(runs))
    for q, (c, b, e, m) in enumerate(runs):
        if (c, b, m) not in rows:
            rows[(c, b, m)] = rr.joint_row_direct(_seq(f, c), f["trans"], b, m, _fb(f, c))
        val, tot, logz = rows[(c, b, m)]
        ref[q], bnd[q] = val[e - 1 - b], rr.bound(tot[e - 1 - b], logz)
    ratio, n = _compare(f"L={L} values={valued} allowed={masked} closed runs", got, ref, bnd)
    print(f"L={L} values={valued} allowed={masked}: {n} finite / {len(runs) - n} impossible closed runs, worst |difference| / bound = {ratio:.3g}")
    assert n >= len(runs) // 6
    rng = np.random.default_rng(9850 + L)
    worst = 0.0
    for q in rng.choice(len(runs), size=15, replace=False).tolist():
        c, b, e, m = runs[q]
        r, inner, logz = rr.run_by_definition(_seq(f, c), f["trans"], b, e, m)
        worst = max(worst, _compare(f"(a) run {q}", [got[q]], [r], [rr.bound(inner, logz)])[0])
    print(f"  against the definition: worst |difference| / bound = {worst:.3g}")
    # a whole sequence under the full set is certain
    whole = [q for q, (c, b, e, m) in enumerate(runs) if b == 0 and e == lens[c] and m == (1 << L) - 1]
    assert all(got[q] == 0.0 for q in whole)


@pytest.mark.parametrize("L", [3, 8])
def test_the_joint_sums_to_the_marginal_of_the_start(nat, L):
    """sum over e of P(the run is [s, e)) = P(the run through a starts at s): closed runs against ``log_start``, both from the
    device.  Every term is within its bound, so their sum is within the largest of them; the start is within its own."""
    f = _family(L, False, True)
    lens = np.diff(f["cptr"])
    c = int(np.flatnonzero((lens >= 25) & (lens <= 60))[0])
    T = int(lens[c])
    rng = np.random.default_rng(9870 + L)
    worst, checked = 0.0, 0
    for a in (0, T // 3, T // 2, T - 1):
        m = _proper_mask(rng, L, "random")
        out = _run(nat, f, [(c, a, m)], T)
        val, tot, logz = rr.anchor_direct(_seq(f, c), f["trans"], a, m, T, _fb(f, c))
        runs = [(c, a - r, e, m) for r in range(a + 1) for e in range(a + 1, T + 1)]
        joint = _run(nat, f, None, 0, runs)["log_run"].reshape(a + 1, T - a)
        for r in range(a + 1):
            row, jtot, _ = rr.joint_row_direct(_seq(f, c), f["trans"], a - r, m, _fb(f, c))
            total, start = rr._lse(joint[r]), out["log_start"][0][r]
            assert np.isneginf(total) == np.isneginf(start)
            if np.isfinite(start):
                tol = float(rr.bound(jtot[r:], logz).max()) + float(rr.bound(tot["log_start"][r], logz))
                worst, checked = max(worst, abs(total - start) / tol), checked + 1
                assert abs(total - start) <= tol, (a, r, total, start)
    print(f"L={L}: {checked} starts, worst |sum of the joint - log_start| / bound = {worst:.3g}")
    assert checked >= 20


# ---------------------------------------------------------------- 6. against the sampler
def test_the_sampler_agrees_within_six_sigma(nat):
    """One batch, seed fixed, N = 20 000 paths: the share of paths whose label at the anchor lies in the set, and the share whose
    run is exactly a given range, lie within 6 sigma of the exact values, sigma^2 = p (1 - p) / N from the exact p with a floor
    of 1 / N, for every query.  The ranges are the runs of ONE path drawn under another seed (where that path has no run: the
    anchor alone)."""
    L, N = 3, 20000
    b = sp._batch(L, (1, 2, 5, 20, 40, 60), 10)
    rng = np.random.default_rng(9980)
    lens = np.diff(b["cptr"])
    anchors = []
    for q in range(50):
        c = int(rng.integers(0, len(lens)))
        anchors.append((c, int(rng.integers(0, lens[c])), _proper_mask(rng, L, ("random", "singleton")[q % 2])))
    model = nat.Model.from_tables(b["w"], b["trans"])
    arrays = _anchor_arrays(anchors)
    drawn = model.sample_paths(*b["csr"], N, seed=77, runs=arrays, want_paths=False)
    pick = model.sample_paths(*b["csr"], 1, seed=78, runs=arrays, want_paths=False)
    ranges = [(c, int(p[0, 0]), int(p[0, 1]), m) if p[0, 0] >= 0 else (c, a, a + 1, m) for (c, a, m), p in zip(anchors, pick)]
    out = model.run_posteriors(*b["csr"], anchors=arrays, reach=64, runs=sp._arrays(ranges))
    worst = 0.0
    for q, (c, first, last, m) in enumerate(ranges):
        there = drawn[q][:, 0] >= 0
        for what, exact, share in (("anchor", np.exp(out["log_anchor"][q]), there.mean()),
                                   ("exact range", np.exp(out["log_run"][q]), ((drawn[q][:, 0] == first) & (drawn[q][:, 1] == last)).mean())):
            sigma = np.sqrt(max(exact * (1.0 - exact) / N, 1.0 / N))
            worst = max(worst, abs(share - exact) / sigma)
            assert abs(share - exact) <= 6.0 * sigma, (q, what, share, exact, sigma)
    print(f"{len(ranges)} queries, N = {N}: worst |share - exact| / sigma = {worst:.3g}")


# ---------------------------------------------------------------- 7. SequenceCRF
def test_sequence_crf_reports_the_native_values(nat):
    L = 8
    b = sp._batch(L, (1, 2, 9, 31, 64, 100), 10)
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = sp._sequence_crf(w, b["trans"])
    X = sp._as_items(b, names)
    rng = np.random.default_rng(9990)
    lens = np.diff(b["cptr"])
    anchors, runs = [], []
    for s, T in enumerate(lens.tolist()):
        m = _proper_mask(rng, L, "random")
        members = [classes[y] for y in range(L) if (m >> y) & 1]
        a = int(rng.integers(0, T))
        anchors.append((s, a, members, m))
        runs.append((s, max(a - 1, 0), min(a + 2, T), set(members), m))
    got = crf.run_posteriors(X, [q[:3] for q in anchors], reach=16)
    logp = crf.run_log_probability(X, [q[:4] for q in runs])
    cptr, gptr, attr = crf._pack(X)[:3]
    score = cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L))
    assert len(got) == len(anchors) and logp.shape == (len(runs),) and np.array_equal(np.exp(logp), crf.run_probability(X, [q[:4] for q in runs]))
    worst = 0.0
    for (s, a, _, m), (_, rb, re_, _, _), res, lp in zip(anchors, runs, got, logp):
        Xs = score[int(cptr[s]):int(cptr[s + 1])]
        val, tot, logz = rr.anchor_direct(Xs, b["trans"], a, m, 16)
        assert set(res) == set(KEYS) and res["log_start"].shape == (17,) and isinstance(res["log_anchor"], float)
        for key in KEYS:
            worst = max(worst, _compare(f"SequenceCRF {key}", res[key], val[key], rr.bound(tot[key], logz))[0])
        ref, inner, _ = rr.run_by_definition(Xs, b["trans"], rb, re_, m)
        worst = max(worst, _compare("SequenceCRF run", [lp], [ref], [rr.bound(inner, logz)])[0])
    print(f"SequenceCRF: worst |difference| / bound = {worst:.3g}")
    masked = crf.run_posteriors(X, [q[:3] for q in anchors[:2]], reach=3, allowed=[[set(anchors[s][2]) if t == anchors[s][1] else None
                                                                                     for t in range(int(lens[s]))] for s in range(len(lens))])
    assert all(r["log_anchor"] == 0.0 for r in masked)  # (the anchor's item allows the labels of the set only)


# ---------------------------------------------------------------- 8. the typed front end
def _interval(p, beyond, side):
    """The interval rule, written out: positions in ascending coordinate order, the first with cumulative mass >= 0.05 and >=
    0.95, as offsets from the anchor; inside the mass beyond the reach: the reach."""
    reach = len(p) - 1
    order = [("beyond", reach)] + [(r, r) for r in range(reach, -1, -1)] if side == "start" else \
        [(r, r) for r in range(reach + 1)] + [("beyond", reach)]
    bounds, cum = [], 0.0
    levels = [0.05, 0.95]
    for which, offset in order:
        cum += beyond if which == "beyond" else p[which]
        while levels and cum >= levels[0]:
            bounds.append(offset)
            levels.pop(0)
    return tuple(bounds)


def test_typed_front_end_reports_run_posteriors(nat, tmp_path):
    from gecco_amd import packing, tables, typed
    from gecco_amd.train_cli import join_clusters
    from tests.typed_planted import C, W, planted_set

    train_genes, train_rows = planted_set(11, 12, "train", composite=True)
    fresh_genes, _ = planted_set(12, 2, "fresh", composite=False)
    base = str(tmp_path)
    sp._write_tables(os.path.join(base, "train"), train_genes, train_rows)
    sp._write_tables(os.path.join(base, "fresh"), fresh_genes)
    random.seed(42)
    np.random.seed(42)
    crf = typed.TypedClusterCRF(W, 1, c1=C, c2=C)
    crf.fit(sp._load(os.path.join(base, "train")), tables.ClusterTable.load(os.path.join(base, "train", "clusters.tsv")))
    genes = sp._load(os.path.join(base, "fresh"))
    L, bg = len(crf.classes_), crf.classes_.index("0")
    not_bg = ((1 << L) - 1) & ~(1 << bg)
    # without the flag: the columns and bytes of a call that omits it
    plain_genes, plain_clusters = crf.predict_genes_and_clusters(genes)
    off_genes, off_clusters = crf.predict_genes_and_clusters(genes, run_posteriors=False, run_reach=5)
    sp._dump(os.path.join(base, "plain"), crf, plain_genes, plain_clusters)
    sp._dump(os.path.join(base, "off"), crf, off_genes, off_clusters)
    sp._same_tables(os.path.join(base, "plain"), os.path.join(base, "off"))
    assert not any(col.startswith("run_") for col in typed.typed_cluster_table(plain_clusters, crf.types_).columns)
    assert not any(hasattr(c, "run_probability") for c in plain_clusters)
    # the lattice as the front end packs it, for the yardstick
    ordered = sorted(genes, key=operator.attrgetter("source.id", "start"))
    ids = [g.id for g in ordered]
    contigs = [list(g) for _, g in itertools.groupby(ordered, key=operator.attrgetter("source.id"))]
    batch = packing.pack_contigs(contigs, crf._attr_index, "protein")
    cptr, gptr, attr = batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id
    model = nat.Model.from_lcrf(crf._blob)
    w, trans = model.state_weights()[0], model.trans_weights()[0]

    def check(found, annotated, known, reach):
        allowed = tp.full_masks(len(ordered), L) if known is None else \
            typed.known_masks(len(ordered), known, join_clusters(ordered, known, device=0), crf.classes_, crf.background)
        score = cr.masked_scores(gptr, attr, None, w, allowed)
        worst, clamped = 0.0, 0
        for cl in found:
            first, last = ids.index(cl.genes[0].id), ids.index(cl.genes[-1].id) + 1
            c = int(np.searchsorted(cptr, first, side="right")) - 1
            g0 = int(cptr[c])
            p_any = [g.average_probability for g in cl.genes]
            a = first + int(np.argmax(p_any))  # (the greatest any-cluster probability, the first on ties)
            X = score[g0:int(cptr[c + 1])]
            val, tot, logz = rr.anchor_direct(X, trans, a - g0, not_bg, reach)
            rel = lambda got, ref: abs(got - ref) / max(abs(ref), 1e-300)
            assert rel(cl.run_anchor_probability, np.exp(val["log_anchor"])) <= 1e-9
            ref_run = rr.run_by_definition(X, trans, first - g0, last - g0, not_bg)[0]
            assert rel(cl.run_probability, np.exp(ref_run)) <= 1e-9 and cl.run_probability <= cl.run_anchor_probability * (1 + 1e-12)
            for side, step, coordinate in (("start", -1, "start"), ("end", 1, "end")):
                p = np.exp(val[f"log_{side}"] - val["log_anchor"])
                beyond = float(np.exp(val[f"log_{side}_beyond"] - val["log_anchor"]))
                assert abs(getattr(cl, f"run_{side}_beyond_probability") - beyond) <= 1e-9
                mine = {r: q for s, g, pos, q in cl.run_boundaries if s == side for r in [abs(ids.index(g.id) - a)]}
                assert all(abs(mine.get(r, 0.0) - p[r]) <= 1e-9 for r in range(reach + 1))
                worst = max(worst, max(abs(mine.get(r, 0.0) - p[r]) for r in range(reach + 1)))
                # the rule on the reported distribution (a cumulative mass within 1e-9 of a level could fall either way)
                got_p = np.array([mine.get(r, 0.0) for r in range(reach + 1)])
                cum = np.cumsum(np.concatenate([[beyond], got_p[::-1]]) if side == "start" else np.concatenate([got_p, [beyond]]))
                if np.min(np.abs(cum[:, None] - np.array([0.05, 0.95])[None, :])) > 1e-8:
                    lo, hi = _interval(got_p, getattr(cl, f"run_{side}_beyond_probability"), side)
                    want = (getattr(ordered[a + step * lo], coordinate), getattr(ordered[a + step * hi], coordinate))
                    assert getattr(cl, f"run_{side}_interval") == want, (cl.id, side, getattr(cl, f"run_{side}_interval"), want)
                    clamped += int(beyond >= 0.05)
        print(f"known={'yes' if known is not None else 'no'} reach={reach}: {len(found)} clusters, worst |p - yardstick| = {worst:.3g}, "
              f"{clamped} clamped bounds")
        return clamped

    annotated, found = crf.predict_genes_and_clusters(genes, run_posteriors=True)
    assert found and [c.id for c in found] == [c.id for c in plain_clusters]
    assert [g.average_probability for g in annotated] == [g.average_probability for g in plain_genes]
    check(found, annotated, None, 256)
    assert all(c.run_start_interval[0] <= c.run_start_interval[1] and c.run_end_interval[0] <= c.run_end_interval[1] for c in found)
    table = typed.typed_cluster_table(found, crf.types_)
    names = ["run_anchor_p", "run_p", "run_start_lo", "run_start_hi", "run_end_lo", "run_end_hi", "run_start_beyond_p", "run_end_beyond_p"]
    assert [n for n, _, _ in table.COLUMNS if n.startswith("run_")] == names
    assert table.columns["run_p"] == [c.run_probability for c in found]
    assert table.columns["run_start_lo"] == [c.run_start_interval[0] for c in found]
    # with the run_ columns taken out, the table is the one without the flag
    sp._dump(os.path.join(base, "on"), crf, annotated, found)
    with open(os.path.join(base, "on", "clusters.tsv")) as fh:
        lines = [line.rstrip("\n").split("\t") for line in fh]
    keep = [i for i, name in enumerate(lines[0]) if not name.startswith("run_")]
    stripped = "".join("\t".join(row[i] for i in keep) + "\n" for row in lines)
    with open(os.path.join(base, "plain", "clusters.tsv")) as fh:
        assert fh.read() == stripped
    # a tiny reach: the bounds that fall beyond it are clamped to the gene at the reach
    _, tiny = crf.predict_genes_and_clusters(genes, run_posteriors=True, run_reach=1)
    assert check(tiny, annotated, None, 1) >= 1
    assert any(c.run_start_beyond_probability > 0.05 or c.run_end_beyond_probability > 0.05 for c in tiny)
    for a, b2 in zip(found, tiny):
        assert a.run_anchor_probability == b2.run_anchor_probability and a.run_probability == b2.run_probability
    # known=: the lattice is the restricted one; a gene of a known region cannot be background
    known = tables.ClusterTable({"sequence_id": ["fresh00"], "cluster_id": ["k1"], "start": [plain_genes[60].start],
                                 "end": [plain_genes[69].end], "type": ["Beta"]})
    k_annotated, k_found = crf.predict_genes_and_clusters(genes, known=known, run_posteriors=True, run_reach=40)
    check(k_found, k_annotated, known, 40)
    inside = [c for c in k_found if c.source.id == "fresh00" and {g.id for g in c.genes} <= set(ids[60:70])]
    assert inside and all(c.run_anchor_probability >= 1.0 - 1e-12 for c in inside)
    # the command line writes the method's table, and boundaries.tsv
    crf.save(os.path.join(base, "model"))
    known.dump(os.path.join(base, "known.tsv"))
    sp._dump(os.path.join(base, "method"), crf, k_annotated, k_found)
    typed.write_boundaries(os.path.join(base, "method", "boundaries.tsv"), k_found)
    done = subprocess.run([sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
                           os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv"),
                           "--known", os.path.join(base, "known.tsv"), "--run-posteriors", "--run-reach", "40", "-o",
                           os.path.join(base, "cli")], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    sp._same_tables(os.path.join(base, "method"), os.path.join(base, "cli"))
    with open(os.path.join(base, "cli", "boundaries.tsv")) as fh, open(os.path.join(base, "method", "boundaries.tsv")) as fm:
        text = fh.read()
        assert text == fm.read()
    rows = [line.split("\t") for line in text.splitlines()]
    assert rows[0] == ["cluster_id", "side", "protein_id", "position", "p"] and len(rows) > 2 * len(k_found)
    assert {r[0] for r in rows[1:]} == {c.id for c in k_found} and {r[1] for r in rows[1:]} == {"start", "end"}
    assert all(float(r[4]) >= 1e-6 for r in rows[1:])
    # without the flag the command line writes no boundaries.tsv and the plain table
    done = subprocess.run([sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
                           os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv"),
                           "-o", os.path.join(base, "cli_plain")], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    sp._same_tables(os.path.join(base, "plain"), os.path.join(base, "cli_plain"))
    assert not os.path.exists(os.path.join(base, "cli_plain", "boundaries.tsv"))
