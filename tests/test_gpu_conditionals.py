"""Marginals given a region and knock-out attributions on the device: ``gecco_crf_span_conditionals`` against the independent
numpy yardstick (tests/conditionals_reference.py), through every whole-contig arrangement, and up through ``SequenceCRF`` and
the typed front end.  The batches, spans and label sets are those of tests/test_gpu_spans.py.

``cond`` is held to the yardstick's conditional marginals within 1e-12 absolute, the project's tolerance for marginals.  A
contribution is held to the yardstick's -- the region's log-probability before the change minus the one after it, the changed
input scored again -- within b1 + b2, the two log-probabilities' own bounds, each the span tests'
``1e-10 (max(1, |log Z_E|) + max(1, |log Z|))``.  Every test prints its worst differences."""
import functools
import itertools
import math
import operator
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import conditionals_reference as cd
from tests import constrained_reference as cr
from tests import test_gpu_spans as sp
from tests import train_objective_partial as tp

pytestmark = pytest.mark.gpu

A = sp.A
ROOT = sp.ROOT
REACHES = [0, 1, 5, 64, 1000]


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


# ---------------------------------------------------------------- the yardstick, computed once per (batch, kind)
class Yardstick:
    """The regions of one lattice (the masked scores of a batch), memoised: ``region(c, b, e, m)`` = (cond [T, L], log Z_E,
    log Z) of tests.conditionals_reference."""

    def __init__(self, cptr, gptr, attr, values, w, trans, allowed):
        self.cptr, self.gptr, self.attr, self.values, self.w, self.trans = cptr, gptr, attr, values, w, trans
        self.score = cr.masked_scores(gptr, attr, values, w, allowed)
        self.memo = {}

    def contig(self, c):
        return self.score[int(self.cptr[c]):int(self.cptr[c + 1])]

    def region(self, c, b, e, m):
        key = (c, b, e, m)
        if key not in self.memo:
            self.memo[key] = cd.region(self.contig(c), self.trans, b, e, m)
        return self.memo[key]

    def knock_out(self, c, b, e, m, t, k=None):
        """(contribution, bound) of item t of contig c (k None) or of its attribute occurrence k (an index of attr)."""
        _, logze, logz = self.region(c, b, e, m)
        delta = None if k is None else -(1.0 if self.values is None else self.values[k]) * self.w[self.attr[k]]
        return cd.contribution(self.contig(c), self.trans, b, e, m, t, delta, base=(logze, logz))


def _yard(b, valued, masked):
    key = ("yard", valued, masked)
    if key not in b:
        every = tp.full_masks(int(b["cptr"][-1]), b["L"])
        b[key] = Yardstick(b["cptr"], b["gptr"], b["attr"], b["v"] if valued else None, b["w"], b["trans"],
                           b["allowed"] if masked else every)
    return b[key]


@functools.lru_cache(maxsize=None)
def _batch(L, lengths=None, n_spans=200):
    return dict(sp._batch(L, lengths, n_spans))  # (a copy: the yardsticks are kept in it)


def _rows(out, q):
    return int(out["row_ptr"][q]), int(out["row_ptr"][q + 1])


def _check_cond(tag, yard, spans, out, reach):
    """Check 1: every row against the yardstick, the row sums, the exact zeros; -inf and all zeros where the region is impossible."""
    worst, worst_sum, possible = 0.0, 0.0, 0
    assert out["cond"].dtype == np.float64 and not np.any(np.isnan(out["cond"])) and not np.any(np.isnan(out["logp"]))
    for q, (c, b, e, m) in enumerate(spans):
        want, logze, logz = yard.region(c, b, e, m)
        T = len(want)
        lo, hi = max(b - reach, 0), min(e + reach, T)
        r0, r1 = _rows(out, q)
        assert int(out["first"][q]) == lo and r1 - r0 == hi - lo, f"{tag}: the rows of span {q}"
        got = out["cond"][r0:r1]
        if not np.isfinite(logze):
            assert np.isneginf(out["logp"][q]) and not got.any(), f"{tag}: an impossible span has -inf and rows of 0.0"
            continue
        possible += 1
        assert np.isfinite(out["logp"][q])
        worst = max(worst, float(np.abs(got - want[lo:hi]).max()))
        worst_sum = max(worst_sum, float(np.abs(got.sum(axis=1) - 1.0).max()))
        dead = np.isneginf(cd.restricted(yard.contig(c), b, e, m)[lo:hi])
        assert np.all(got[dead] == 0.0), f"{tag}: exact zeros where the yardstick's scores are -inf (span {q})"
    print(f"{tag}: {possible} possible / {len(spans) - possible} impossible spans, worst |cond - yardstick| = {worst:.3g}, "
          f"worst |row sum - 1| = {worst_sum:.3g}")
    assert worst <= 1e-12 and worst_sum <= 1e-12, tag
    return possible


def _check_contributions(tag, yard, spans, out, reach, rng, per_span=2, limit=40):
    """Check 2: the gene's and every occurrence's contribution of a few rows of up to `limit` spans, scored again."""
    worst, cases = 0.0, 0
    order = rng.permutation(len(spans))[:limit].tolist()
    for q in order:
        c, b, e, m = spans[q]
        _, logze, _ = yard.region(c, b, e, m)
        r0, r1 = _rows(out, q)
        lo = int(out["first"][q])
        if not np.isfinite(logze):
            assert not out["item"][r0:r1].any() and not out["attr"][out["occ_ptr"][r0]:out["occ_ptr"][r1]].any(), \
                f"{tag}: an impossible span has contributions of 0.0"
            continue
        picks = sorted({int(rng.integers(b, e)), int(rng.integers(lo, lo + r1 - r0))})[:per_span]  # (one inside the span, one anywhere)
        for t in picks:
            r = r0 + t - lo
            g = int(yard.cptr[c]) + t
            k0, k1 = int(yard.gptr[g]), int(yard.gptr[g + 1])
            assert int(out["occ_ptr"][r + 1] - out["occ_ptr"][r]) == k1 - k0
            for k, got in [(None, out["item"][r])] + [(k, out["attr"][int(out["occ_ptr"][r]) + k - k0]) for k in range(k0, k1)]:
                want, bound = yard.knock_out(c, b, e, m, t, k)
                worst = max(worst, abs(got - want) / bound)
                cases += 1
                assert np.isfinite(got) and abs(got - want) <= bound, f"{tag}: span {q} item {t} occurrence {k}: {got!r} vs {want!r}"
    print(f"{tag}: {cases} knock-outs, worst |contribution - scoring again| / bound = {worst:.3g}")
    assert cases > 0
    return worst


# ---------------------------------------------------------------- 1, 2. against the yardstick
@pytest.mark.parametrize("valued,masked", sp.KINDS)
@pytest.mark.parametrize("L", sp.LABELS)
def test_conditionals_and_contributions_against_the_yardstick(nat, L, valued, masked):
    b = _batch(L)
    spans = list(b["spans"])
    if L == 32:
        assert any(s[3] >> 31 for s in spans)
    kw = dict(values=b["v"] if valued else None, allowed=b["allowed"] if masked else None)
    model = nat.Model.from_tables(b["w"], b["trans"])
    yard = _yard(b, valued, masked)
    rng = np.random.default_rng(6100 + L)
    reach = REACHES[(sp.LABELS.index(L) + 2 * valued + masked) % len(REACHES)]
    tag = f"L={L} values={valued} allowed={masked} reach={reach}"
    out = model.span_conditionals(*b["csr"], *sp._arrays(spans), reach=reach, want_marginals=True, **kw)
    possible = _check_cond(tag, yard, spans, out, reach)
    assert possible >= len(spans) // 3, "at least a third of the queries are possible spans"
    _check_contributions(tag, yard, spans, out, reach, rng)
    # check 4, first half: the bytes of the entries this one contains
    logp = model.span_log_probabilities(*b["csr"], *sp._arrays(spans), **kw)
    emarg, elogz = model.marginals_full(*b["csr"], **kw)
    assert out["logp"].tobytes() == logp.tobytes(), "logp: span_log_probabilities' bytes"
    assert out["marginals"].tobytes() == emarg.tobytes() and out["lognorm"].tobytes() == elogz.tobytes()
    # duplicate queries (the first ten come again at the end)
    n = len(spans) - 10
    for q in range(10):
        assert spans[q] == spans[n + q]
        (a0, a1), (b0, b1) = _rows(out, q), _rows(out, n + q)
        assert out["cond"][a0:a1].tobytes() == out["cond"][b0:b1].tobytes() and out["item"][a0:a1].tobytes() == out["item"][b0:b1].tobytes()
        assert out["attr"][out["occ_ptr"][a0]:out["occ_ptr"][a1]].tobytes() == out["attr"][out["occ_ptr"][b0]:out["occ_ptr"][b1]].tobytes()


@pytest.mark.parametrize("L,switch,mode", sp.ARRANGEMENTS)
def test_every_whole_contig_arrangement(nat, monkeypatch, L, switch, mode):
    lengths = sp._arrangement_lengths()
    assert {63, 64, 65, 66, 127, 128, 129, 300} <= set(lengths)
    b = _batch(L, lengths, 40)
    rng = np.random.default_rng(8300 + L)
    spans = sp._boundary_spans(rng, b["cptr"], L) + list(b["spans"])
    assert any(s[1:3] == (0, 300) for s in spans) and any(s[1:3] == (31, 33) for s in spans) and any(s[1:3] == (32, 64) for s in spans)
    monkeypatch.setenv(switch, mode)
    model = nat.Model.from_tables(b["w"], b["trans"])
    for valued, masked in ((True, True), (False, False)):
        kw = dict(values=b["v"] if valued else None, allowed=b["allowed"] if masked else None)
        yard = _yard(b, valued, masked)
        tag = f"L={L} {switch}={mode} values={valued} allowed={masked}"
        out = model.span_conditionals(*b["csr"], *sp._arrays(spans), reach=64, want_marginals=True, **kw)
        _check_cond(tag, yard, spans, out, 64)
        _check_contributions(tag, yard, spans, out, 64, rng, limit=25)
        emarg, elogz = model.marginals_full(*b["csr"], **kw)
        assert out["marginals"].tobytes() == emarg.tobytes() and out["lognorm"].tobytes() == elogz.tobytes()
        assert out["logp"].tobytes() == model.span_log_probabilities(*b["csr"], *sp._arrays(spans), **kw).tobytes()


# ---------------------------------------------------------------- 3. device against device
@pytest.mark.parametrize("L", [3, 17])
def test_an_occurrence_removed_from_the_csr_gives_the_contribution(nat, L):
    b = _batch(L)
    cptr, gptr, attr = b["csr"]
    spans = [s for s in b["spans"] if cptr[s[0] + 1] - cptr[s[0]] <= 60][:60]
    model = nat.Model.from_tables(b["w"], b["trans"])
    rng = np.random.default_rng(6300 + L)
    out = model.span_conditionals(cptr, gptr, attr, *sp._arrays(spans), reach=5, values=b["v"], want_marginals=True)
    logz = out["lognorm"]
    done, worst = 0, 0.0
    for q in rng.permutation(len(spans)).tolist():
        if done == 12:
            break
        c = spans[q][0]
        r0, r1 = _rows(out, q)
        rows = [r for r in range(r0, r1) if out["occ_ptr"][r + 1] > out["occ_ptr"][r]]
        if not np.isfinite(out["logp"][q]) or not rows:
            continue
        r = int(rng.choice(rows))
        i = int(rng.integers(0, out["occ_ptr"][r + 1] - out["occ_ptr"][r]))
        g = int(cptr[c]) + int(out["first"][q]) + r - r0
        k = int(gptr[g]) + i
        gptr2 = gptr.copy()
        gptr2[g + 1:] -= 1
        after = model.span_log_probabilities(cptr, gptr2, np.delete(attr, k), *sp._arrays([spans[q]]), values=np.delete(b["v"], k),
                                             want_marginals=True)
        lp0, lp1, z1 = float(out["logp"][q]), float(after[0][0]), float(after[2][c])
        bound = 1e-10 * (max(1.0, abs(logz[c] + lp0)) + max(1.0, abs(logz[c]))) + 1e-10 * (max(1.0, abs(z1 + lp1)) + max(1.0, abs(z1)))
        got = float(out["attr"][int(out["occ_ptr"][r]) + i])
        worst = max(worst, abs(got - (lp0 - lp1)) / bound)
        assert abs(got - (lp0 - lp1)) <= bound, (q, g, k)
        done += 1
    assert done == 12
    print(f"L={L}: 12 occurrences removed on the device, worst |contribution - (logp - logp without)| / bound = {worst:.3g}")


# ---------------------------------------------------------------- 4. bytes
def _row_bytes(out, q, t0, t1):
    """The bytes of the rows of the genes [t0, t1) of span q's contig: cond, item, attr."""
    r0 = int(out["row_ptr"][q]) + t0 - int(out["first"][q])
    r1 = r0 + t1 - t0
    assert int(out["row_ptr"][q]) <= r0 and r1 <= int(out["row_ptr"][q + 1])
    return (out["cond"][r0:r1].tobytes(), out["item"][r0:r1].tobytes(), out["attr"][out["occ_ptr"][r0]:out["occ_ptr"][r1]].tobytes())


@pytest.mark.parametrize("L", [2, 8, 32])
def test_a_rows_bytes_depend_on_neither_reach_nor_order(nat, L):
    b = _batch(L, sp._arrangement_lengths(), 40)
    rng = np.random.default_rng(6400 + L)
    spans = list(b["spans"]) + sp._boundary_spans(rng, b["cptr"], L)[:30]
    kw = dict(values=b["v"], allowed=b["allowed"])
    model = nat.Model.from_tables(b["w"], b["trans"])
    outs = {reach: model.span_conditionals(*b["csr"], *sp._arrays(spans), reach=reach, **kw) for reach in REACHES}
    wide = outs[1000]
    assert np.isfinite(wide["logp"]).sum() >= len(spans) // 3 and wide["cond"].any()
    lens = np.diff(b["cptr"])
    for reach in REACHES[:-1]:
        assert outs[reach]["logp"].tobytes() == wide["logp"].tobytes()
        for q, (c, s, e, _) in enumerate(spans):
            lo, hi = max(s - reach, 0), min(e + reach, int(lens[c]))
            assert _row_bytes(outs[reach], q, lo, hi) == _row_bytes(wide, q, lo, hi), f"reach {reach} against 1000, span {q}"
    back = model.span_conditionals(*b["csr"], *sp._arrays(spans[::-1]), reach=5, **kw)
    n = len(spans)
    for q, (c, s, e, _) in enumerate(spans):
        lo, hi = max(s - 5, 0), min(e + 5, int(lens[c]))
        assert _row_bytes(back, n - 1 - q, lo, hi) == _row_bytes(outs[5], q, lo, hi), f"reversed queries, span {q}"
        assert back["logp"][n - 1 - q].tobytes() == outs[5]["logp"][q].tobytes()


@pytest.mark.parametrize("L", [2, 5, 12])
def test_a_slice_gives_the_bytes_of_the_rebased_batch(nat, L):
    rng = np.random.default_rng(9400 + L)
    model = nat.Model.from_tables(rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L)))
    cptr, gptr, attr = sp._csr(rng, [4, 9, 3, 30, 1, 70])
    v = sp._values(rng, len(attr))
    allowed = sp._wide_masks(rng, int(cptr[-1]), L)
    g0 = int(cptr[2])
    a0 = int(gptr[g0])
    assert g0 > 0 and a0 > 0
    allowed[:g0] = 0
    spans = [(0, 0, 3, sp._set_mask(rng, L, "random")), (1, 5, 30, sp._set_mask(rng, L, "random")), (2, 0, 1, (1 << L) - 1),
             (3, 64, 70, sp._set_mask(rng, L, "random")), (3, 0, 70, sp._set_mask(rng, L, "random")), (1, 0, 7, 1)]
    for kw_slice, kw_alone in ((dict(values=v, allowed=allowed), dict(values=v[a0:], allowed=allowed[g0:])), (dict(), dict())):
        got = model.span_conditionals(cptr[2:], gptr, attr, *sp._arrays(spans), reach=5, want_marginals=True, **kw_slice)
        alone = model.span_conditionals(cptr[2:] - g0, gptr[g0:] - a0, attr[a0:], *sp._arrays(spans), reach=5, want_marginals=True, **kw_alone)
        assert set(got) == set(alone)
        for key in got:
            assert got[key].size and got[key].tobytes() == alone[key].tobytes(), key
        assert np.any(np.isfinite(got["logp"])) and got["cond"].any() and got["attr"].any()
    yard = Yardstick(cptr[2:] - g0, gptr[g0:] - a0, attr[a0:], v[a0:], model.state_weights()[0], model.trans_weights()[0], allowed[g0:])
    got = model.span_conditionals(cptr[2:], gptr, attr, *sp._arrays(spans), reach=5, values=v, allowed=allowed)
    _check_cond(f"L={L} slice", yard, spans, got, 5)
    _check_contributions(f"L={L} slice", yard, spans, got, 5, rng, per_span=3)


# ---------------------------------------------------------------- 5. range
@pytest.mark.parametrize("L", [3, 17])
def test_a_label_outside_the_set_that_leads_by_800(nat, L):
    """The layouts of tests/test_gpu_spans.py: one attribute gives label k a lead of 800; it sits on one item of each contig, and k
    is outside every queried set.  Where that item lies inside the span the region costs the lead and taking the attribute out
    gives it back: a contribution near -800.  Where it lies beside or away from the span, the item keeps label k under both
    distributions whatever the region does, and both sums of the identity are led by the same term: near 0 next to 800 (the
    rest is what the neighbours' transitions make of the freed item, a few units of the transition weights)."""
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
    others = ((1 << L) - 1) & ~(1 << k)
    layouts = [(0, 3, 8, True), (0, 5, 6, True), (1, 0, 5, True), (2, T - 4, T, True), (0, 6, 9, False), (0, 2, 5, False),
               (3, 0, 1, True), (3, 1, 4, False), (4, T - 1, T, True), (4, T - 4, T - 1, False), (0, 0, T, True),
               (0, 9, 11, False), (2, 0, 3, False), (1, 8, T, False)]  # (the last three: the leader away from the span)
    spans = [(c, b, e, others) for c, b, e, _ in layouts] + [(c, b, e, 1 << (0 if L == 3 else 7)) for c, b, e, _ in layouts]
    model = nat.Model.from_tables(w, trans)
    yard = Yardstick(cptr, gptr, attr, None, w, trans, tp.full_masks(int(cptr[-1]), L))
    out = model.span_conditionals(cptr, gptr, attr, *sp._arrays(spans), reach=T)
    assert np.all(np.isfinite(out["logp"])) and np.all(np.isfinite(out["cond"])) and np.all(np.isfinite(out["attr"]))
    _check_cond(f"L={L} leader by 800", yard, spans, out, T)
    worst = 0.0
    for q, ((c, b, e, m), (_, _, _, inside)) in enumerate(zip(spans, layouts + layouts)):
        t = leaders[c]
        assert (b <= t < e) == inside
        r = int(out["row_ptr"][q]) + t - int(out["first"][q])
        g = c * T + t
        kk = int(gptr[g + 1]) - 1  # (the leading attribute is the item's last occurrence)
        assert attr[kk] == special
        got = float(out["attr"][int(out["occ_ptr"][r + 1]) - 1])
        want, bound = yard.knock_out(c, b, e, m, t, kk)
        worst = max(worst, abs(got - want) / bound)
        print(f"L={L} span {(c, b, e)} set {m:#x}, leader {'inside' if inside else 'outside'}: contribution = {got!r}, scored again = {want!r}")
        assert abs(got - want) <= bound
        assert (got < -700.0) if inside else (abs(got) < 100.0)
        _, bound_item = yard.knock_out(c, b, e, m, t, None)
        assert abs(float(out["item"][r]) - yard.knock_out(c, b, e, m, t, None)[0]) <= bound_item
    print(f"L={L}: worst |contribution of the leading attribute - scoring again| / bound = {worst:.3g}")


@pytest.mark.parametrize("L", [3, 17])
def test_a_transition_of_minus_1e300_gives_no_nan(nat, L):
    b = _batch(L, (1, 2, 7, 33, 64, 70), 40)
    trans = b["trans"].copy()
    trans[1, 0] = -1e300
    model = nat.Model.from_tables(b["w"], trans)
    spans = list(b["spans"])
    out = model.span_conditionals(*b["csr"], *sp._arrays(spans), reach=5, values=b["v"], allowed=b["allowed"], want_marginals=True)
    for key, value in out.items():
        assert not np.any(np.isnan(value)), key
    assert np.isfinite(out["logp"]).any()
    yard = Yardstick(b["cptr"], b["gptr"], b["attr"], b["v"], b["w"], trans, b["allowed"])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        possible = [q for q, s in enumerate(spans) if np.isfinite(yard.region(*s)[1])]
    for q in possible:
        r0, r1 = _rows(out, q)
        assert np.all(np.abs(out["cond"][r0:r1].sum(axis=1) - 1.0) <= 1e-12)


# ---------------------------------------------------------------- 6. a full set
@pytest.mark.parametrize("L", [2, 8, 32])
def test_a_full_set_conditions_on_nothing(nat, L):
    b = _batch(L)
    full = (1 << L) - 1
    spans = [(c, s, e, full) for c, s, e, _ in b["spans"][:60]]
    model = nat.Model.from_tables(b["w"], b["trans"])
    yard = _yard(b, True, True)
    out = model.span_conditionals(*b["csr"], *sp._arrays(spans), reach=5, values=b["v"], allowed=b["allowed"], want_marginals=True)
    assert np.all(out["logp"] == 0.0)
    worst_c = worst = 0.0
    for q, (c, s, e, m) in enumerate(spans):
        r0, r1 = _rows(out, q)
        g = int(b["cptr"][c]) + int(out["first"][q])
        worst_c = max(worst_c, float(np.abs(out["cond"][r0:r1] - out["marginals"][g:g + r1 - r0]).max()))
        _, logze, logz = yard.region(c, s, e, m)
        bound = cd.bound_of(logze, logz) + 2e-10  # (b1, and what b2 is at the least: 1e-10 (1 + 1))
        for values in (out["item"][r0:r1], out["attr"][out["occ_ptr"][r0]:out["occ_ptr"][r1]]):
            if values.size:
                worst = max(worst, float(np.abs(values).max()) / bound)
    print(f"L={L}: worst |cond - marg| = {worst_c:.3g}, worst |contribution| / bound = {worst:.3g}")
    assert worst_c <= 1e-12 and worst <= 1.0


# ---------------------------------------------------------------- 7. impossible spans
@pytest.mark.parametrize("L", [3, 9])
def test_a_set_disjoint_from_the_allowed_labels_is_impossible(nat, L):
    rng = np.random.default_rng(9200 + L)
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    cptr, gptr, attr = sp._csr(rng, [10, 1, 40, 70])
    n = int(cptr[-1])
    allowed = tp.full_masks(n, L)
    pinned = [int(cptr[0]) + 4, int(cptr[1]), int(cptr[2]), int(cptr[3]) + 69]
    allowed[pinned] = 1
    away = ((1 << L) - 1) & ~1
    dead = [(0, 2, 7, away), (0, 4, 5, away), (0, 4, 10, away), (0, 0, 5, away), (1, 0, 1, away), (2, 0, 3, 2), (3, 60, 70, away),
            (3, 69, 70, 4)]
    alive = [(0, 0, 4, away), (0, 5, 10, away), (0, 2, 7, 1 | 4), (3, 0, 70, (1 << L) - 1)]
    spans = [x for pair in itertools.zip_longest(dead, alive) for x in pair if x is not None]
    model = nat.Model.from_tables(w, trans)
    out = model.span_conditionals(cptr, gptr, attr, *sp._arrays(spans), reach=64, allowed=allowed, want_marginals=True)
    for key, value in out.items():
        assert not np.any(np.isnan(value)), key
    alone = model.span_conditionals(cptr, gptr, attr, *sp._arrays(alive), reach=64, allowed=allowed)
    for q, s in enumerate(spans):
        r0, r1 = _rows(out, q)
        if s in dead:
            assert np.isneginf(out["logp"][q]) and r1 > r0
            assert not out["cond"][r0:r1].any() and not out["item"][r0:r1].any()
            assert not out["attr"][out["occ_ptr"][r0]:out["occ_ptr"][r1]].any()
        else:
            k = alive.index(s)
            a0, a1 = _rows(alone, k)
            assert np.isfinite(out["logp"][q]) and out["logp"][q].tobytes() == alone["logp"][k].tobytes()
            assert out["cond"][r0:r1].tobytes() == alone["cond"][a0:a1].tobytes() and out["cond"][r0:r1].any()
            assert out["item"][r0:r1].tobytes() == alone["item"][a0:a1].tobytes()
            assert out["attr"][out["occ_ptr"][r0]:out["occ_ptr"][r1]].tobytes() == \
                alone["attr"][alone["occ_ptr"][a0]:alone["occ_ptr"][a1]].tobytes()
    yard = Yardstick(cptr, gptr, attr, None, w, trans, allowed)
    _check_cond(f"L={L} impossible spans", yard, spans, out, 64)
    # no spans: a successful call that still fills marg and lognorm
    none = model.span_conditionals(cptr, gptr, attr, [], [], [], [], reach=3, allowed=allowed, want_marginals=True)
    emarg, elogz = model.marginals_full(cptr, gptr, attr, allowed=allowed)
    assert none["logp"].shape == (0,) and none["cond"].shape == (0, L) and none["item"].shape == (0,)
    assert none["marginals"].tobytes() == emarg.tobytes() and none["lognorm"].tobytes() == elogz.tobytes()


# ---------------------------------------------------------------- 8. SequenceCRF
@pytest.mark.parametrize("valued", [False, True])
def test_sequence_crf_gives_the_native_calls_bytes(nat, valued):
    L = 5
    b = _batch(L, (1, 6, 20, 33, 64, 3), 10)
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = sp._sequence_crf(w, b["trans"])
    X = sp._as_items(b, names)
    rng = np.random.default_rng(9500)
    if valued:  # (dict items: real-valued attributes)
        X = [[{name: float(rng.normal()) for name in item} for item in xs] for xs in X]
    X.insert(2, [])
    spans = [(0, 0, 1, "l0"), (1, 2, 5, {"l1", "l4"}), (3, 0, 20, ["l0", "l1", "l2", "l3"]), (4, 10, 33, ("l2",)),
             (5, 0, 64, frozenset(classes)), (6, 1, 2, "l3"), (1, 2, 5, {"l4", "l1"})]
    sets = [[None if rng.random() < 0.5 else {classes[int(rng.integers(0, L))], classes[int(rng.integers(0, L))], "l2"}
             for _ in xs] for xs in X]
    cptr, gptr, attr, values = crf._pack(X)
    assert (values is not None) == valued
    model = nat.Model.from_lcrf(crf.to_bytes())
    masks = [sum(1 << classes.index(y) for y in ([labs] if isinstance(labs, str) else labs)) for *_, labs in spans]
    arrays = sp._arrays([(s, a, e, m) for (s, a, e, _), m in zip(spans, masks)])
    for allowed in (None, sets):
        amasks = None if allowed is None else crf._label_sets(allowed, cptr, "allowed")[0]
        want = model.span_conditionals(cptr, gptr, attr, *arrays, reach=4, values=values, allowed=amasks)
        given = crf.predict_marginals_given_span(X, spans, reach=4, allowed=allowed)
        found = crf.span_attributions(X, spans, reach=4, allowed=allowed)
        assert len(given) == len(found) == len(spans) and want["cond"].any() and want["attr"].any()
        for q, (g, f) in enumerate(zip(given, found)):
            r0, r1 = _rows(want, q)
            assert g["first"] == f["first"] == int(want["first"][q]) == max(spans[q][1] - 4, 0)
            assert np.float64(g["log_probability"]).tobytes() == want["logp"][q].tobytes() == np.float64(f["log_probability"]).tobytes()
            assert g["marginals"].shape == (r1 - r0, L) and g["marginals"].tobytes() == want["cond"][r0:r1].tobytes()
            assert f["items"].tobytes() == want["item"][r0:r1].tobytes() and len(f["attributes"]) == r1 - r0
            for r, entries in zip(range(r0, r1), f["attributes"]):
                item = int(cptr[spans[q][0]]) + f["first"] + r - r0
                k0, k1 = int(gptr[item]), int(gptr[item + 1])
                assert [e[0] for e in entries] == [names[a] for a in attr[k0:k1]]
                assert [e[1] for e in entries] == ([1.0] * (k1 - k0) if values is None else values[k0:k1].tolist())
                assert np.array([e[2] for e in entries]).tobytes() == want["attr"][want["occ_ptr"][r]:want["occ_ptr"][r + 1]].tobytes()
        assert given[4]["log_probability"] == 0.0 and given[1]["marginals"].tobytes() == given[6]["marginals"].tobytes()
    assert crf.predict_marginals_given_span(X, []) == [] and crf.span_attributions(X, []) == []
    with pytest.raises(ValueError, match="span 0"):
        crf.span_attributions(X, [(2, 0, 1, "l0")])


# ---------------------------------------------------------------- 9. the typed front end
def test_typed_front_end_reports_attributions(nat, tmp_path):
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
    # without the flag: the columns and bytes of a call that omits it
    plain_genes, plain_clusters = crf.predict_genes_and_clusters(genes)
    off_genes, off_clusters = crf.predict_genes_and_clusters(genes, attributions=False)
    sp._dump(os.path.join(base, "plain"), crf, plain_genes, plain_clusters)
    sp._dump(os.path.join(base, "off"), crf, off_genes, off_clusters)
    sp._same_tables(os.path.join(base, "plain"), os.path.join(base, "off"))
    assert not any(hasattr(c, "attributions") for c in plain_clusters)
    # the batch as the front end packs it, for the native call
    ordered = sorted(genes, key=operator.attrgetter("source.id", "start"))
    ids = [g.id for g in ordered]
    contigs = [list(g) for _, g in itertools.groupby(ordered, key=operator.attrgetter("source.id"))]
    batch = packing.pack_contigs(contigs, crf._attr_index, "protein")
    cptr, gptr, attr = batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id
    model = nat.Model.from_lcrf(crf._blob)
    names = model.attrs()
    not_bg = ((1 << L) - 1) & ~(1 << bg)
    known = tables.ClusterTable({"sequence_id": ["fresh00"], "cluster_id": ["k1"], "start": [plain_genes[60].start],
                                 "end": [plain_genes[69].end], "type": ["Beta"]})
    for kn, reach in ((None, 10), (known, 3)):
        annotated, found = crf.predict_genes_and_clusters(genes, known=kn, attributions=True, attribution_reach=reach)
        assert found and [c.id for c in found] == [c.id for c in crf.predict_clusters(genes, known=kn)]
        if kn is None:
            sp._dump(os.path.join(base, "on"), crf, annotated, found)
            sp._same_tables(os.path.join(base, "plain"), os.path.join(base, "on"))
        allowed = None if kn is None else typed.known_masks(len(ordered), kn, join_clusters(ordered, kn, device=0), crf.classes_,
                                                            crf.background)
        where = []
        for cl in found:
            first, last = ids.index(cl.genes[0].id), ids.index(cl.genes[-1].id) + 1
            c = int(np.searchsorted(cptr, first, side="right")) - 1
            where.append((c, first - int(cptr[c]), last - int(cptr[c]), not_bg))
        want = model.span_conditionals(cptr, gptr, attr, *sp._arrays(where), reach=reach, allowed=allowed)
        assert want["item"].any() and want["attr"].any()
        for q, (cl, (c, s, e, _)) in enumerate(zip(found, where)):
            r0, r1 = _rows(want, q)
            assert cl.attribution_log_probability == float(want["logp"][q]) and len(cl.attributions) == r1 - r0
            for r, row in zip(range(r0, r1), cl.attributions):
                g = int(cptr[c]) + int(want["first"][q]) + r - r0
                assert row["protein_id"] == ordered[g].protein.id and row["offset"] == g - int(cptr[c]) - s
                assert row["contribution"] == float(want["item"][r])
                assert [d[0] for d in row["domains"]] == [names[a] for a in attr[gptr[g]:gptr[g + 1]]]
                assert [d[1] for d in row["domains"]] == want["attr"][want["occ_ptr"][r]:want["occ_ptr"][r + 1]].tolist()
            assert cl.attributions[0]["offset"] == -min(reach, s) and any(row["offset"] == 0 for row in cl.attributions)
    # the command line with --attributions writes the method's table
    crf.save(os.path.join(base, "model"))
    known.dump(os.path.join(base, "known.tsv"))
    sp._dump(os.path.join(base, "method"), crf, annotated, found)
    typed.write_attributions(os.path.join(base, "method", "attributions.tsv"), found)
    done = subprocess.run([sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
                           os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv"),
                           "--known", os.path.join(base, "known.tsv"), "--attributions", "--attribution-reach", "3", "-o",
                           os.path.join(base, "cli")], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    sp._same_tables(os.path.join(base, "method"), os.path.join(base, "cli"))
    with open(os.path.join(base, "method", "attributions.tsv"), "rb") as fa, open(os.path.join(base, "cli", "attributions.tsv"), "rb") as fb:
        text = fa.read()
        assert text == fb.read()
    lines = text.decode().splitlines()
    assert lines[0].split("\t") == ["cluster_id", "sequence_id", "protein_id", "offset", "domain", "contribution", "p_without"]
    assert len(lines) == 1 + sum(1 + len(row["domains"]) for cl in found for row in cl.attributions)
    fields = lines[1].split("\t")
    assert fields[4] == "" and float(fields[6]) == math.exp(found[0].attribution_log_probability - float(fields[5]))
