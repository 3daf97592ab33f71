"""Run-length potentials on the device: ``gecco_crf_viterbi_run_length`` and ``gecco_crf_marginals_run_length`` against the
independent yardstick (tests/runlength_reference.py: the recursion over the explicit expanded state list in ``numpy.longdouble``,
the max semiring in the product's operation order and tie rule, path enumeration), their reductions to the entries the model
contains (the plain lattice, the minimum run length, a maximum run length), their invariances, the fit of the length scores, and
the typed front end.

The sum-semiring tolerance is derived, not measured.  A log-quantity of the device -- a forward value, a backward value, log Z_g --
is within ``rl.log_bound(T, L, M, mag)`` = (T + 1)(2 L + 8 + M + 2) eps max(1, mag) of its exact value: per item at most 2 L
exponentials and positive additions, one logarithm and three additions (the bound of tests/test_gpu_minrun_marginals.py), and the
exit aggregate's M + 2 operations more (backward: the exit and stay continuations and their combination, no more than that), all
at magnitude <= mag, the yardstick's largest finite |alpha, beta or alpha + end score| on the sequence.  A marginal is a sum over
the run counter of exp(alpha + beta - log Z_g): three log-quantities and (M + 4) eps for the slot sum, so where the yardstick's
value is >= 1e-280 the relative error is at most ``rl.marginal_bound`` = expm1(3 log_bound + (M + 4) eps), and the device's value
is <= 1e-279 where the yardstick's is smaller.  A count is a sum of at most T L terms exp((alpha + g) + continuation - log Z_g),
three log-quantities each, added in fp64: ``rl.count_bound`` = expm1(3 log_bound + (T L + L + 4) eps), relative, with the same
rule below 1e-280.  Every entry is compared; no case is skipped for ties or range.  A wrong source set, a dropped slot or a
misplaced length score misses these bounds by many orders of magnitude.

The max semiring is compared exactly: with integer weights and scores ``y`` and ``score`` equal the yardstick's bit for bit;
with random weights ``score`` equals the yardstick's, which is evaluated in the stated operation order, and ``y`` is compared
where the yardstick met no tied maximum.

A yardstick is computed once per (batch, set, model) and shared."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import runlength_reference as rl
from tests import test_gpu_kbest as gk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf
EPS = rl.EPS
# every LP (2, 4, 8, 16, 32) with lanes without a label at 3, 5, 9 and 17; the table lengths 1, 2, 3 and 32.  The yardstick's
# dense table has (labels in the set) * M + (labels outside) states: the cases keep it under about 160.
CASES = [(L, M) for L in (2, 3, 5, 9, 17, 32) for M in (1, 2, 3, 32)]
WORST = {"ratio": 0.0}


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


# ---------------------------------------------------------------- batches, models, the yardstick
def seam_lengths(M):
    """1, M - 1, M, M + 1, an empty contig in the middle, 7 / 8 / 9 / 17 around the eight-item prefetch, 40: eleven contigs,
    no multiple of any 64 / LP."""
    return [1, M - 1, M, 0, M + 1, 7, 8, 9, 17, 40, 2]


def direct_batch(seed, L, lengths, integer=False):
    """A batch whose state scores are a table of its own: every gene has one private attribute, so the model's weights are the
    scores.  (score [n, L], trans [L, L], the CSR arrays)."""
    rng = np.random.default_rng(seed)
    cptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(cptr[-1])
    if integer:
        score, trans = rng.integers(-3, 4, size=(n, L)).astype(np.float64), rng.integers(-2, 3, size=(L, L)).astype(np.float64)
    else:
        score, trans = rng.normal(0.0, 1.0, size=(n, L)), rng.normal(0.0, 1.5, size=(L, L))
    return dict(L=L, score=score, trans=trans, cptr=cptr, csr=(cptr, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)))


@functools.lru_cache(maxsize=None)
def seam_batch(L, M, integer):
    return direct_batch(12000 + 40 * L + M + (7000 if integer else 0), L, seam_lengths(M), integer)


def label_sets(L, M):
    """One label; several labels; every label -- the last two while the yardstick's state list stays short."""
    one, every = 1 << (L - 1), (1 << L) - 1
    several = every & ~1 if L <= 5 else ((1 << (L // 2 + 1)) - 1) & ~1  # (every label but 0; the labels 1 .. L / 2)
    sets = [one]
    for mask in (several, every):
        inside = bin(mask).count("1")
        if mask not in sets and inside * M + (L - inside) <= 130:
            sets.append(mask)
    return sets


def soft_model(seed, M, integer=False):
    """A table with a -inf entry (where it has more than two) and a finite tail."""
    rng = np.random.default_rng(seed)
    if integer:
        g, tau = rng.integers(-3, 4, size=M).astype(np.float64), float(rng.integers(-2, 2))
    else:
        g, tau = rng.normal(0.0, 1.5, size=M), float(rng.normal(0.0, 0.7))
    if M > 2:
        g[int(rng.integers(0, M - 1))] = NINF
    return g, tau


def min_run_table(m):
    return np.array([NINF] * (m - 1) + [0.0])


def contigs(b):
    return [(c, int(b["cptr"][c]), int(b["cptr"][c + 1])) for c in range(len(b["cptr"]) - 1)]


def yardstick(b, score, mask, g, tau, kind):
    """Per contig the yardstick's answer (None for a contig without genes); kept on the batch and left unchanged."""
    key = (kind, mask, tuple(np.asarray(g).tolist()), float(tau), id(score))
    if key not in b:
        fn = rl.forward_backward if kind == "sum" else rl.max_recursion
        b[key] = [fn(score[g0:g1], b["trans"], mask, g, tau) if g1 > g0 else None for _, g0, g1 in contigs(b)]
    return b[key]


def judge_sum(tag, b, score, mask, g, tau, got):
    """One marginals call against the yardstick, contig by contig, every entry; returns the worst error / bound."""
    marg, inside, counts, lzg, lz = got
    L, M = b["L"], len(g)
    n, nc = int(b["cptr"][-1]), len(b["cptr"]) - 1
    assert marg.shape == (n, L) and inside.shape == (n,) and counts.shape == (nc, M + 1) and lzg.shape == lz.shape == (nc,)
    for a in (marg, inside, counts, lzg, lz):
        assert a.dtype == np.float64 and not np.isnan(a).any(), f"{tag}: a NaN"
    assert np.all(marg[score == NINF] == 0.0), f"{tag}: a disallowed pair is not exactly 0.0"
    cols = [j for j in range(L) if (mask >> j) & 1]
    worst = 0.0
    for (c, g0, g1), ref in zip(contigs(b), yardstick(b, score, mask, g, tau, "sum")):
        T = g1 - g0
        where = f"{tag} contig {c} (T={T})"
        if ref is None:
            assert lzg[c] == 0.0 and lz[c] == 0.0 and not counts[c].any(), f"{where}: a contig without genes has zeros"
            continue
        mine = marg[g0:g1]
        if ref["logz"] == NINF:
            assert lzg[c] == NINF and not mine.any() and not inside[g0:g1].any() and not counts[c].any(), f"{where}: no feasible path"
            continue
        mag = ref["largest"]
        zb = rl.log_bound(T, L, M, mag)
        err = abs(float(np.longdouble(lzg[c]) - ref["logz"]))
        print(f"{where}: log Z_g error {err:.3g}, bound {zb:.3g}")
        assert np.isfinite(lzg[c]) and err <= zb, f"{where}: log Z_g off by {err:.3g}, bound {zb:.3g}"
        for name, have, want, B in (("marginals", mine, ref["marg"], rl.marginal_bound(T, L, M, mag)),
                                    ("counts", counts[c], ref["counts"], rl.count_bound(T, L, M, mag))):
            big = want >= 1e-280
            rel = np.abs((have.astype(np.longdouble)[big] - want[big]) / want[big]).astype(np.float64)
            ratio = float(rel.max()) / B if rel.size else 0.0
            worst = max(worst, ratio)
            print(f"{where}: {name} relative error {float(rel.max()) if rel.size else 0.0:.3g}, bound {B:.3g}")
            assert ratio <= 1.0, f"{where}: {name} relative error {float(rel.max()):.3g}, bound {B:.3g} (L={L}, M={M}, mag={mag:.3g})"
            assert np.all(have[~big] <= 1e-279), f"{where}: {name} has mass where the yardstick has none"
        total = np.abs(mine.sum(axis=1) - 1.0).max()
        assert total <= rl.marginal_bound(T, L, M, mag) + L * EPS, f"{where}: |sum of a gene's marginals - 1| = {total:.3g}"
        assert np.abs(inside[g0:g1] - mine[:, cols].sum(axis=1)).max() <= L * EPS, f"{where}: inside is not the sum of the set's columns"
    WORST["ratio"] = max(WORST["ratio"], worst)
    return worst


def judge_max(tag, b, score, mask, g, tau, got, exact, absolute=None):
    """One decoding call against the yardstick.  ``absolute`` (the sums of the absolute values of the terms of every item score)
    is given when the device sums an item's score from several attribute terms, in its own order: the table the yardstick reads
    is then the device's up to rounding, not bit for bit, and the score is compared under B = 8 (T + 1) eps S, S = sum_t max_l
    absolute[t][l] + T (max|trans| + max|finite g| + |finite tau|): a path's score is a sum of at most 6 T terms, first-order
    error 3 T eps S on either side, and a maximum over paths moves by no more than its paths do."""
    y, sc = got[0], got[1]
    assert y.dtype == np.int8 and y.shape == (int(b["cptr"][-1]),) and sc.shape == (len(b["cptr"]) - 1,) and not np.isnan(sc).any()
    compared = 0
    for (c, g0, g1), ref in zip(contigs(b), yardstick(b, score, mask, g, tau, "max")):
        where = f"{tag} contig {c} (T={g1 - g0})"
        if ref is None:
            assert sc[c] == 0.0, where
            continue
        path, best, tie_free = ref
        if absolute is not None:
            T = g1 - g0
            fin = np.concatenate([np.asarray(g, dtype=np.float64), [tau]])
            fin = np.abs(fin[np.isfinite(fin)])
            S = float(absolute[g0:g1].max(axis=1).sum()) + T * (float(np.abs(b["trans"]).max()) + (float(fin.max()) if fin.size else 0.0))
            B = 8 * (T + 1) * EPS * S
            if path is None:
                assert sc[c] == NINF and np.all(y[g0:g1] == -1), f"{where}: no feasible path is -inf and -1"
                continue
            mine = rl.path_score_g(score[g0:g1], b["trans"], y[g0:g1].tolist(), mask, g, tau)
            print(f"{where}: |score - yardstick| = {abs(sc[c] - best):.3g}, bound {B:.3g}")
            assert abs(sc[c] - best) <= B and abs(mine - sc[c]) <= B, f"{where}: score {sc[c]!r}, the yardstick's {best!r}, y scores {mine!r}"
            compared += 1
            continue
        assert sc[c] == best, f"{where}: score {sc[c]!r}, the yardstick's {best!r}"
        if path is None:
            assert np.all(y[g0:g1] == -1), f"{where}: no feasible path is -1 at every gene"
        elif exact or tie_free:
            assert y[g0:g1].tolist() == path.tolist(), f"{where}: another path"
            compared += 1
        if path is not None:
            assert rl.path_score_g(score[g0:g1], b["trans"], y[g0:g1].tolist(), mask, g, tau) == sc[c], f"{where}: y does not score `score`"
    return compared


def same_bytes(a, b):
    return all((x is None and z is None) or (x is not None and z is not None and x.tobytes() == z.tobytes()) for x, z in zip(a, b))


def alone(b, c):
    """Contig c of a direct batch as a batch of its own."""
    g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
    T = g1 - g0
    return (np.array([0, T], dtype=np.int32), np.arange(T + 1, dtype=np.int32), np.arange(g0, g1, dtype=np.int32)), g0, g1


# ---------------------------------------------------------------- 1. the seams: both semirings against the yardstick
@pytest.mark.parametrize("L,M", CASES)
def test_seams(nat, L, M):
    turn = CASES.index((L, M))
    assert all(len(seam_lengths(M)) % k for k in (2, 4, 8, 16, 32))
    b, bi = seam_batch(L, M, False), seam_batch(L, M, True)
    model, model_i = nat.Model.from_tables(b["score"], b["trans"]), nat.Model.from_tables(bi["score"], bi["trans"])
    for s, mask in enumerate(label_sets(L, M)):
        g, tau = soft_model(100 * turn + s, M)
        gi, taui = soft_model(100 * turn + s + 50, M, integer=True)
        tag = f"L={L} M={M} set={mask:#x}"
        # the max semiring: integer weights bit for bit, random weights in the stated operation order
        got_i = model_i.viterbi_run_length(*bi["csr"], mask, gi, taui)
        judge_max(tag + " integer", bi, bi["score"], mask, gi, taui, got_i, exact=True)
        got = model.viterbi_run_length(*b["csr"], mask, g, tau)
        assert judge_max(tag, b, b["score"], mask, g, tau, got, exact=False) >= 1
        # the sum semiring
        full = model.marginals_run_length(*b["csr"], mask, g, tau)
        worst = judge_sum(tag, b, b["score"], mask, g, tau, full)
        print(f"{tag}: worst error / bound = {worst:.3g}")
        # log Z_g has the decoder's bits, log Z the marginals entry's
        assert full[3].tobytes() == got[2].tobytes(), f"{tag}: lognorm_run_length is not viterbi_run_length's"
        assert full[4].tobytes() == got[3].tobytes() == model.marginals_full(*b["csr"])[1].tobytes(), f"{tag}: lognorm"
        # equal calls, equal bytes; an output keeps its bytes whatever else is asked for
        assert same_bytes(model.marginals_run_length(*b["csr"], mask, g, tau), full), f"{tag}: equal calls, other bytes"
        assert same_bytes(model.viterbi_run_length(*b["csr"], mask, g, tau), got), f"{tag}: equal calls, other bytes"
        bare = model.viterbi_run_length(*b["csr"], mask, g, tau, want_lognorm=False)
        assert bare[2] is None and bare[3] is None and same_bytes(bare[:2], got[:2]), f"{tag}: y or score changes without log Z_g"
        for drop in ("want_marginals", "want_inside", "want_counts"):
            part = model.marginals_run_length(*b["csr"], mask, g, tau, **{drop: False})
            keep = [k for k, name in enumerate(("want_marginals", "want_inside", "want_counts")) if name != drop]
            assert part[3].tobytes() == full[3].tobytes() and all(part[k].tobytes() == full[k].tobytes() for k in keep), f"{tag}: {drop}"
        only = model.marginals_run_length(*b["csr"], mask, g, tau, want_marginals=False, want_inside=False)
        assert only[0] is None and only[1] is None and only[2].tobytes() == full[2].tobytes(), f"{tag}: counts alone"
        if s == turn % len(label_sets(L, M)):  # every contig alone has the bytes it has inside the batch
            for c, g0, g1 in contigs(b):
                if g1 == g0:
                    continue
                csr = alone(b, c)[0]
                am, ai, ac, alzg, _ = model.marginals_run_length(*csr, mask, g, tau)
                assert am.tobytes() == full[0][g0:g1].tobytes() and ai.tobytes() == full[1][g0:g1].tobytes(), f"{tag} contig {c}: alone"
                assert ac[0].tobytes() == full[2][c].tobytes() and alzg.tobytes() == full[3][c:c + 1].tobytes(), f"{tag} contig {c}: alone"
                ay, asc, _, _ = model.viterbi_run_length(*csr, mask, g, tau)
                assert ay.tobytes() == got[0][g0:g1].tobytes() and asc.tobytes() == got[1][c:c + 1].tobytes(), f"{tag} contig {c}: alone"
    print(f"largest error / bound so far: {WORST['ratio']:.3g}")


def test_a_batch_that_does_not_start_at_gene_zero(nat):
    """contig_ptr[0] > 0: the genes before it are not part of the batch."""
    b = direct_batch(12900, 5, [4, 9, 0, 3, 17])
    model = nat.Model.from_tables(b["score"], b["trans"])
    g, tau = soft_model(5, 3)
    cptr, gptr, attr = b["csr"]
    full_v, full_m = model.viterbi_run_length(cptr, gptr, attr, 0b10110, g, tau), model.marginals_run_length(cptr, gptr, attr, 0b10110, g, tau)
    tail_v, tail_m = model.viterbi_run_length(cptr[1:], gptr, attr, 0b10110, g, tau), model.marginals_run_length(cptr[1:], gptr, attr, 0b10110, g, tau)
    assert tail_v[0].tobytes() == full_v[0][4:].tobytes() and all(tail_v[k].tobytes() == full_v[k][1:].tobytes() for k in (1, 2, 3))
    assert tail_m[0].tobytes() == full_m[0][4:].tobytes() and tail_m[1].tobytes() == full_m[1][4:].tobytes()
    assert all(tail_m[k].tobytes() == full_m[k][1:].tobytes() for k in (2, 3, 4))


# ---------------------------------------------------------------- 2. enumeration on small shapes
@pytest.mark.parametrize("L,longest", [(2, 7), (3, 5)])
def test_enumeration(nat, L, longest):
    lengths = list(range(1, longest + 1)) + [0]
    b, bi = direct_batch(12100 + L, L, lengths), direct_batch(12150 + L, L, lengths, integer=True)
    model, model_i = nat.Model.from_tables(b["score"], b["trans"]), nat.Model.from_tables(bi["score"], bi["trans"])
    for M in (1, 2, 3, 4):
        for mask in range(1, 1 << L):
            for k, (g, tau) in enumerate(((np.zeros(M), 0.0), soft_model(M + mask, M), (soft_model(M + mask + 9, M)[0], NINF))):
                gi = np.where(np.isfinite(g), np.round(2 * g), g)
                taui = tau if tau == NINF else float(round(2 * tau))
                y, sc, _, _ = model_i.viterbi_run_length(*bi["csr"], mask, gi, taui)
                marg, _, counts, lzg, _ = model.marginals_run_length(*b["csr"], mask, g, tau)
                for c, g0, g1 in contigs(b):
                    if g1 == g0:
                        continue
                    where = f"L={L} M={M} set={mask:#x} model {k} contig {c}"
                    want = rl.enumerate_all(bi["score"][g0:g1], bi["trans"], mask, gi, taui)
                    assert sc[c] == want["best"], where
                    assert (tuple(y[g0:g1].tolist()) in [tuple(p) for p in want["paths"]]) if want["paths"] else np.all(y[g0:g1] == -1), where
                    want = rl.enumerate_all(b["score"][g0:g1], b["trans"], mask, g, tau)
                    if want["logz"] == NINF:
                        assert lzg[c] == NINF and not marg[g0:g1].any() and not counts[c].any(), where
                        continue
                    T = g1 - g0
                    mag = rl.forward_backward(b["score"][g0:g1], b["trans"], mask, g, tau)["largest"]
                    assert abs(float(np.longdouble(lzg[c]) - want["logz"])) <= rl.log_bound(T, L, M, mag), where
                    for have, ref, B in ((marg[g0:g1], want["marg"], rl.marginal_bound(T, L, M, mag)),
                                         (counts[c], want["counts"], rl.count_bound(T, L, M, mag))):
                        big = ref >= 1e-280
                        rel = np.abs((have.astype(np.longdouble)[big] - ref[big]) / ref[big]).astype(np.float64)
                        assert (rel.size == 0 or rel.max() <= B) and np.all(have[~big] <= 1e-279), f"{where}: {rel.max():.3g}, bound {B:.3g}"


# ---------------------------------------------------------------- 3. the reductions
@pytest.mark.parametrize("L", [2, 5, 17])
def test_zeros_are_the_plain_lattice(nat, L):
    b = gk.make_batch(12200 + L, L, [1, 2, 0, 9, 31, 40, 3])
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = gk.sequence_crf(w, b["trans"])
    cptr, gptr, attr = b["csr"]
    X = [[[names[a] for a in dict.fromkeys(attr[gptr[i]:gptr[i + 1]].tolist())] for i in range(cptr[s], cptr[s + 1])]
         for s in range(len(cptr) - 1)]
    seq_ptr, item_ptr, ids, values = crf._pack(X)
    score = gk.cr.masked_scores(item_ptr, ids, values, crf._model.state_weights()[0], gk.tp.full_masks(int(seq_ptr[-1]), L))
    bb = dict(L=L, trans=crf._model.trans_weights()[0], cptr=seq_ptr)
    inside_names = classes[1:] if L > 2 else classes[1]
    mask = (1 << L) - 2
    free = crf.predict_marginals(X)
    plain = crf.predict(X)
    runs = crf.expected_runs(X, [inside_names])
    kbest = crf._model.viterbi_kbest(seq_ptr, item_ptr, ids, 1, values=values)
    for M in (1, 3, 32):
        zeros = np.zeros(M)
        out = crf.predict_run_length(X, inside_names, zeros)
        assert [o["labels"] for o in out] == [list(p) for p in plain], f"M={M}: zeros do not decode predict's path"
        assert [o["score"] for o in out] == [float(v) if T else 0.0 for v, T in zip(kbest[1][:, 0], np.diff(seq_ptr))], f"M={M}: rank 0"
        ms = crf.predict_marginals_run_length(X, inside_names, zeros)
        counts = crf.run_length_counts(X, inside_names, zeros)
        ref = yardstick(bb, score, mask, zeros, 0.0, "sum")
        for s, (o, r) in enumerate(zip(ms, ref)):
            T = int(seq_ptr[s + 1] - seq_ptr[s])
            assert counts[s].tobytes() == o["counts"].tobytes()
            if r is None:
                assert not counts[s].any() and o["log_mass_ratio"] == 0.0
                continue
            mag = max(r["largest"], 1.0)
            Bm, Bc = rl.marginal_bound(T, L, M, mag), rl.count_bound(T, L, M, mag)
            # (the other entries' own numbers are accepted at 1e-12 by their tests: the sum of both sides' allowances)
            assert abs(o["log_mass_ratio"]) <= 2 * rl.log_bound(T, L, M, mag) + 1e-12, f"M={M} sequence {s}: log Z_g is not log Z"
            assert np.abs(o["marginals"] - free[s]).max() <= Bm + 1e-12, f"M={M} sequence {s}: not predict_marginals"
            total = counts[s][:M].sum()
            assert abs(total - runs[s, 0]) <= Bc * total + 1e-12 * max(1.0, total), f"M={M} sequence {s}: runs {total!r}, expected_runs {runs[s, 0]!r}"
            items = float((np.arange(1, M + 1) * counts[s][:M]).sum() + counts[s][M])
            assert abs(items - o["inside"].sum()) <= (Bc + Bm) * max(1.0, items) + T * EPS * max(1.0, items), f"M={M} sequence {s}: items"


@pytest.mark.parametrize("L", [3, 9, 32])
def test_the_min_run_table_is_the_min_run_entries(nat, L):
    b, bi = direct_batch(12300 + L, L, [1, 2, 3, 0, 4, 7, 8, 9, 17, 40]), direct_batch(12350 + L, L, [1, 2, 3, 0, 4, 7, 8, 9, 17, 40], True)
    model, model_i = nat.Model.from_tables(b["score"], b["trans"]), nat.Model.from_tables(bi["score"], bi["trans"])
    for mask in (1 << (L - 1), ((1 << L) - 1) & ~1, (1 << L) - 1):
        for m in (1, 2, 3):
            g = min_run_table(m)
            for mdl, bb in ((model, b), (model_i, bi)):
                y, sc, lzg, lz = mdl.viterbi_run_length(*bb["csr"], mask, g, 0.0)
                wy, wsc, wlzc, wlz = mdl.viterbi_min_run(*bb["csr"], mask, m)
                tag = f"L={L} set={mask:#x} m={m}"
                assert sc.tobytes() == wsc.tobytes(), f"{tag}: score is not viterbi_min_run's"
                if bb is b:  # (random weights: no ties, one best path)
                    assert y.tobytes() == wy.tobytes(), f"{tag}: labels are not viterbi_min_run's"
                assert lz.tobytes() == wlz.tobytes()
            marg, inside, counts, lzg, _ = model.marginals_run_length(*b["csr"], mask, g, 0.0)
            wm, wi, wlzc, _ = model.marginals_min_run(*b["csr"], mask, m)
            for (c, g0, g1), ref in zip(contigs(b), yardstick(b, b["score"], mask, g, 0.0, "sum")):
                if ref is None:
                    continue
                T = g1 - g0
                if ref["logz"] == NINF:
                    assert lzg[c] == NINF and wlzc[c] == NINF and not marg[g0:g1].any() and np.all(y[g0:g1] == -1)
                    continue
                mag = ref["largest"]
                assert abs(lzg[c] - wlzc[c]) <= 2 * rl.log_bound(T, L, m, mag), f"{tag} contig {c}: log Z_g is not log Z_C"
                B = 2 * rl.marginal_bound(T, L, m, mag)
                want = ref["marg"].astype(np.float64)
                big = ref["marg"] >= 1e-280
                assert np.all(np.abs(marg[g0:g1][big] - wm[g0:g1][big]) <= B * want[big]), f"{tag} contig {c}: not marginals_min_run"
                assert np.all(marg[g0:g1][~big] <= 1e-279) and np.all(counts[c][:m - 1] == 0.0) and counts[c][m] <= T


@pytest.mark.parametrize("L,M", [(2, 1), (3, 2), (5, 3), (9, 32)])
def test_a_tail_of_minus_infinity_is_a_maximum_run_length(nat, L, M):
    lengths = [1, M, M + 1, 0, 2 * M + 3, 40, 9]
    base = direct_batch(12400 + L, L, lengths)
    for mask in (1 << (L - 1), ((1 << L) - 1) & ~1, (1 << L) - 1):
        ins = rl.inside_labels(mask, L)
        b = dict(base, score=base["score"].copy(), trans=base["trans"].copy())
        b["score"][:, ins] += 3.0  # (the labels of the set are favoured, and staying among them: the free path has long runs)
        b["trans"][np.ix_(ins, ins)] += 3.0
        model = nat.Model.from_tables(b["score"], b["trans"])
        g = np.zeros(M)
        y, sc, lzg, lz = model.viterbi_run_length(*b["csr"], mask, g, NINF)
        marg, inside, counts, lzg2, _ = model.marginals_run_length(*b["csr"], mask, g, NINF)
        assert np.all(counts[:, M] == 0.0), "tau = -inf: a tail step has mass"
        assert not np.isnan(sc).any() and not np.isnan(marg).any() and not np.isnan(counts).any() and lzg.tobytes() == lzg2.tobytes()
        free_y = model.viterbi(*b["csr"])[0]
        longer = 0
        for c, g0, g1 in contigs(b):
            if g1 == g0:
                continue
            if mask == (1 << L) - 1 and g1 - g0 > M:  # every label in the set: the contig is one run, which is too long
                assert sc[c] == NINF and lzg[c] == NINF and np.all(y[g0:g1] == -1) and not marg[g0:g1].any() and not counts[c].any()
                continue
            assert np.isfinite(sc[c]) and max(rl.runs_of(y[g0:g1].tolist(), mask), default=0) <= M, f"contig {c}: a run longer than {M}"
            assert rl.path_score_g(b["score"][g0:g1], b["trans"], y[g0:g1].tolist(), mask, g, NINF) == sc[c]
            longer += max(rl.runs_of(free_y[g0:g1].tolist(), mask), default=0) > M
        if mask != (1 << L) - 1:
            assert longer >= 1, "the premise: the free path has a longer run somewhere"


def test_infeasible_contigs_and_masks(nat):
    """g[1] = g[2] = -inf with every label in the set: contigs of one or two genes have no path; `allowed` and values."""
    L, M, mask = 5, 3, 0b11100
    b = gk.make_batch(12500, L, [0, 1, 2, 3, 4, 7, 9, 17, 40, 3])
    model = nat.Model.from_tables(b["w"], b["trans"])
    g, tau = np.array([NINF, NINF, 0.25]), -0.5
    for valued, masked in ((False, False), (True, False), (False, True), (True, True)):
        score, absolute = gk.tables(b, valued, masked)
        bb = dict(L=L, trans=b["trans"], cptr=b["cptr"])
        kw = gk.kw(b, valued, masked)
        for set_mask in (mask, (1 << L) - 1):
            tag = f"values={valued} allowed={masked} set={set_mask:#x}"
            got = model.marginals_run_length(*b["csr"], set_mask, g, tau, **kw)
            judge_sum(tag, bb, score, set_mask, g, tau, got)
            dec = model.viterbi_run_length(*b["csr"], set_mask, g, tau, **kw)
            judge_max(tag, bb, score, set_mask, g, tau, dec, exact=False, absolute=absolute)
            assert got[4].tobytes() == model.marginals_full(*b["csr"], **kw)[1].tobytes()
            if set_mask == (1 << L) - 1:
                short = np.diff(b["cptr"])
                assert np.all(dec[1][(short > 0) & (short < 3)] == NINF) and np.all(got[3][(short > 0) & (short < 3)] == NINF)
            if masked:
                assert (score == NINF).any() and np.all(got[0][score == NINF] == 0.0)


def test_refusals_reach_the_caller(nat):
    b = direct_batch(12600, 3, [3, 2])
    model = nat.Model.from_tables(b["score"], b["trans"])
    for fn, name in ((model.viterbi_run_length, "viterbi_run_length"), (model.marginals_run_length, "marginals_run_length")):
        with pytest.raises(Exception, match=rf"{name}: max_length = 33 is outside 1 \.\. 32"):
            fn(*b["csr"], 6, np.zeros(33))
        with pytest.raises(Exception, match=rf"{name}: length_score\[1\] is NaN"):
            fn(*b["csr"], 6, [0.0, np.nan])
        with pytest.raises(Exception, match=f"{name}: tail is NaN"):
            fn(*b["csr"], 6, [0.0], tail=np.inf)
        for bad in (0, 8):
            with pytest.raises(Exception, match=f"{name}: set_mask"):
                fn(*b["csr"], bad, [0.0, 0.0])


# ---------------------------------------------------------------- 4. the fit
FIT_SEED, FIT_M, FIT_C2 = 4, 8, 1.0


def planted_fit_set(seed=FIT_SEED, n_seqs=40, T=30):
    """40 sequences of 30 items at three labels: gold runs of labels 1 and 2 of 3 to 6 items only, between stretches of label 0
    of at least two items; an item shows the attribute of its label three times out of four and another one otherwise, so that
    the plain decoder calls lone items.  (weights [attributes, L], trans, X as attribute names, y as label indices)"""
    rng = np.random.default_rng(seed)
    L = 3
    w = np.array([[1.1, 0.0, 0.0], [0.0, 1.1, 0.0], [0.0, 0.0, 1.1], [0.2, 0.1, 0.1]])
    trans = np.array([[0.2, -0.1, -0.1], [-0.1, 0.3, 0.0], [-0.1, 0.0, 0.3]])
    ys, xs = [], []
    for _ in range(n_seqs):
        y = []
        while len(y) < T:
            y.extend([0] * int(rng.integers(2, 6)))
            run = int(rng.integers(3, 7))
            lab = int(rng.integers(1, L))
            y.extend([lab if rng.random() < 0.8 else 3 - lab for _ in range(run)])
        y = y[:T]
        # (cutting at T may shorten the last run: put label 0 there instead)
        k = T
        while k > 0 and y[k - 1] != 0:
            k -= 1
        if T - k < 3:
            y[k:] = [0] * (T - k)
        x = [int(lab) if rng.random() < 0.75 else int(rng.integers(0, 4)) for lab in y]
        ys.append(y)
        xs.append(x)
    return w, trans, xs, ys


def test_the_fit(nat):
    from scipy import optimize

    w, trans, xs, ys = planted_fit_set()
    L, M, c2, mask = 3, FIT_M, FIT_C2, 0b110
    crf, names, classes = gk.sequence_crf(w, trans)
    X = [[[names[a]] for a in x] for x in xs]
    Y = [[classes[k] for k in y] for y in ys]
    lengths = [n for y in ys for n in rl.runs_of(y, mask)]
    assert lengths and min(lengths) >= 3 and max(lengths) <= 6, "the planted runs have 3 to 6 items"
    g, tau = crf.fit_run_length_scores(X, Y, classes[1:], M, c2=c2, epsilon=1e-9, delta=0.0)
    result = crf.fit_run_length_result_
    print(f"fit: {result!r}, g = {g.tolist()}, tau = {tau}")
    theta_dev = np.concatenate([g, [tau]])
    observed = sum(rl.observed_counts(y, mask, M) for y in ys)
    scores = [w[np.array(x)] for x in xs]

    def F(theta, dtype=np.float64):
        f, grad = 0.5 * c2 * float(theta @ theta) - float(observed @ theta), c2 * theta - observed
        for s in scores:
            r = rl.forward_backward(s, trans, mask, theta[:M], theta[M], dtype)
            f, grad = f + float(r["logz"]), grad + r["counts"].astype(np.float64)
        return f, grad

    ref = optimize.minimize(F, theta_dev, jac=True, method="BFGS", options=dict(gtol=1e-9))
    theta_ref = ref.x
    grad_dev, grad_ref = F(theta_dev, np.longdouble)[1], F(theta_ref, np.longdouble)[1]
    gap, allow = float(np.linalg.norm(theta_dev - theta_ref)), float(np.linalg.norm(grad_dev) + np.linalg.norm(grad_ref)) / c2
    print(f"|theta_device - theta_ref| = {gap:.3g}, (|grad F(device)| + |grad F(ref)|) / c2 = {allow:.3g}, scipy: {ref.nit} iterations")
    # F is strongly convex with modulus c2: |theta - theta*| <= |grad F(theta)| / c2 for either point
    assert gap <= allow
    assert g[2:6].min() > max(g[0], g[1]), f"the planted lengths 3 .. 6 do not rank above 1 and 2: {g.tolist()}"
    lone = lambda paths: sum(n == 1 for p in paths for n in rl.runs_of([classes.index(lab) for lab in p], mask))  # noqa: E731
    plain = lone(crf.predict(X))
    assert plain >= 1, "the premise: the plain decoder calls a run of one item somewhere"
    fitted = crf.predict_run_length(X, classes[1:], g, tau)
    assert all(o["labels"] is not None for o in fitted) and lone([o["labels"] for o in fitted]) == 0
    print(f"runs of one item: plain {plain}, with the fitted length model 0")
    # the objective the fit reports is the yardstick's, up to the constant part of F
    gold = -float(crf.log_likelihood(X, Y).sum())
    lz = crf._model.marginals_full(*crf._pack(X)[:3])[1]
    assert abs((result.f - gold + float(lz.sum())) - F(theta_dev)[0]) <= 1e-8 * max(1.0, abs(result.f))


# ---------------------------------------------------------------- 6. the typed front end
def test_typed_front_end_length_model(nat, tmp_path):
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
    clusters = tables.ClusterTable.load(os.path.join(base, "train", "clusters.tsv"))
    crf.fit(gs._load(os.path.join(base, "train")), clusters)
    genes = gs._load(os.path.join(base, "fresh"))
    with pytest.raises(ValueError, match="has no length model"):
        crf.predict_path_clusters(genes, length_model=True)
    crf.save(os.path.join(base, "old"))
    assert typed.LENGTH_FILE not in os.listdir(os.path.join(base, "old"))
    assert typed.TypedClusterCRF.trained(os.path.join(base, "old")).length_scores_ is None  # (a directory without a length model)
    M = 6
    assert crf.fit_length_model(gs._load(os.path.join(base, "train")), clusters, max_length=M, c2=0.5) is crf
    g, tau = crf.length_scores_, crf.length_tail_
    assert g.shape == (M,) and g.dtype == np.float64 and np.all(np.isfinite(g)) and np.isfinite(tau) and np.abs(g).max() > 0.0
    print(f"typed length model: g = {g.tolist()}, tau = {tau}, {crf.length_fit_result_!r}")
    # the direct calls
    L, bg = len(crf.classes_), crf.classes_.index("0")
    ordered = sorted(genes, key=operator.attrgetter("source.id", "start"))
    contigs_ = [list(x) for _, x in itertools.groupby(ordered, key=operator.attrgetter("source.id"))]
    batch = packing.pack_contigs(contigs_, crf._attr_index, "protein")
    cptr, gptr, attr = batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id
    model = nat.Model.from_lcrf(crf._blob)
    mask = ((1 << L) - 1) & ~(1 << bg)
    y, score, lzg, lz = model.viterbi_run_length(cptr, gptr, attr, mask, g, tau)
    inside = model.marginals_run_length(cptr, gptr, attr, mask, g, tau)[1]
    with pytest.raises(ValueError, match="give one"):
        crf.predict_path_clusters(genes, min_run=3, length_model=True)
    found = crf.predict_path_clusters(genes, length_model=True, marginals=True)
    assert crf.path_gene_probabilities_.tobytes() == inside.tobytes()
    assert crf.path_genes_["path_label"] == [crf.classes_[k] for k in y.tolist()]
    assert crf.path_posteriors_["score"] == score.tolist() and crf.path_posteriors_["constraint_log_p"] == (lzg - lz).tolist()
    runs = [(c, a, b) for c in range(len(cptr) - 1) for a, b in _runs(y[cptr[c]:cptr[c + 1]] != bg)]
    assert found and [len(c.genes) for c in found] == [b - a for _, a, b in runs]
    ids = [x.id for x in ordered]
    for cl, (c, a, b) in zip(found, runs):
        assert ids.index(cl.genes[0].id) == int(cptr[c]) + a
        ps = inside[int(cptr[c]) + a:int(cptr[c]) + b]
        assert (cl.average_p, cl.max_p, cl.min_p) == (float(np.mean(ps)), float(ps.max()), float(ps.min()))
    # save, load: the same bits, the same clusters
    crf.save(os.path.join(base, "model"))
    again = typed.TypedClusterCRF.trained(os.path.join(base, "model"))
    assert again.length_scores_.tobytes() == g.tobytes() and again.length_tail_ == tau
    assert [c.id for c in again.predict_path_clusters(genes, length_model=True)] == [c.id for c in found]
    # the command line
    common = [sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
              os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv")]
    done = subprocess.run(common + ["--path-clusters", "--length-model", "-o", os.path.join(base, "cli")], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    rows = [line.rstrip("\n").split("\t") for line in open(os.path.join(base, "cli", "path_clusters.tsv"))]
    assert [r[1] for r in rows[1:]] == [c.id for c in found]
    for flags, text in ((["--path-clusters", "3", "--length-model"], "give one"), (["--length-model"], "--length-model needs --path-clusters"),
                        (["--path-clusters"], "--path-clusters needs M")):
        done = subprocess.run(common + flags + ["-o", os.path.join(base, "bad")], cwd=ROOT, capture_output=True, text=True)
        assert done.returncode != 0 and text in done.stderr, flags


def _runs(inside):
    edges = np.flatnonzero(np.diff(np.concatenate([[False], np.asarray(inside, dtype=bool), [False]]).astype(np.int8)))
    return list(zip(edges[::2].tolist(), edges[1::2].tolist()))


# ---------------------------------------------------------------- 5. SequenceCRF
def test_predict_run_length(nat):
    L = 5
    b = gk.make_batch(12700, L, [1, 2, 0, 9, 31, 40, 3])
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = gk.sequence_crf(w, b["trans"])
    cptr, gptr, attr = b["csr"]
    X = [[[names[a] for a in dict.fromkeys(attr[gptr[i]:gptr[i + 1]].tolist())] for i in range(cptr[s], cptr[s + 1])]
         for s in range(len(cptr) - 1)]
    seq_ptr, item_ptr, ids, values = crf._pack(X)
    g, tau = np.array([NINF, -1.0, 0.5, 0.25]), -0.125
    mask = (1 << L) - 2
    y, sc, lzg, lz = crf._model.viterbi_run_length(seq_ptr, item_ptr, ids, mask, g, tau, values=values)
    marg, ins, counts, lzg2, _ = crf._model.marginals_run_length(seq_ptr, item_ptr, ids, mask, g, tau, values=values)
    out = crf.predict_run_length(X, classes[1:], g, tau)
    more = crf.predict_marginals_run_length(X, classes[1:], g.tolist(), tail=tau)
    assert all(sorted(o) == ["labels", "log_mass_ratio", "log_probability_given_model", "score"] for o in out)
    assert all(sorted(o) == ["counts", "inside", "log_mass_ratio", "marginals"] for o in more)
    assert crf.run_length_counts(X, classes[1:], g, tau).tobytes() == counts.tobytes()
    for s, (o, m) in enumerate(zip(out, more)):
        g0, g1 = int(seq_ptr[s]), int(seq_ptr[s + 1])
        if g1 == g0:
            assert o == {"labels": [], "score": 0.0, "log_probability_given_model": 0.0, "log_mass_ratio": 0.0}
            assert m["marginals"].shape == (0, L) and not m["counts"].any()
            continue
        assert o["labels"] == [classes[k] for k in y[g0:g1].tolist()] and o["score"] == float(sc[s])
        assert o["log_probability_given_model"] == float(sc[s] - lzg[s]) <= 1e-12 and o["log_mass_ratio"] == float(lzg[s] - lz[s]) == m["log_mass_ratio"]
        assert m["marginals"].tobytes() == marg[g0:g1].tobytes() and m["inside"].tobytes() == ins[g0:g1].tobytes()
        assert m["counts"].tobytes() == counts[s].tobytes() and 1 not in rl.runs_of(y[g0:g1].tolist(), mask)
    # every label in the set and a forbidden short run: the short sequences have no path
    short = crf.predict_run_length(X, classes, [NINF, NINF, 0.0])
    assert short[0]["labels"] is None and short[0]["score"] == NINF and short[0]["log_probability_given_model"] == NINF
    assert short[1]["labels"] is None and short[2]["labels"] == [] and short[3]["labels"] is not None
    none = crf.predict_marginals_run_length(X, classes, [NINF, NINF, 0.0])
    assert none[0]["marginals"] is None and none[0]["inside"] is None and none[0]["log_mass_ratio"] == NINF and not none[0]["counts"].any()
    # with allowed sets the path and the mass stay inside them
    allowed = [[{classes[0], classes[-1]} if t % 2 else None for t in range(T)] for T in np.diff(cptr).tolist()]
    for o, m, sets in zip(crf.predict_run_length(X, classes[1:], g, tau, allowed=allowed),
                          crf.predict_marginals_run_length(X, classes[1:], g, tau, allowed=allowed), allowed):
        for t, a in enumerate(sets):
            if a is not None and o["labels"] is not None:
                assert o["labels"][t] in a and all(m["marginals"][t, k] == 0.0 for k, name in enumerate(classes) if name not in a)
