"""Inference under allowed-label sets on the device: ``gecco_crf_viterbi_constrained``, ``gecco_crf_marginals_full_constrained``,
``gecco_crf_windowed_marginals_constrained`` and ``gecco_crf_windowed_marginals_all_constrained`` against the independent
numpy yardstick (tests/constrained_reference.py), through every whole-contig arrangement and every window tier, and up
through ``SequenceCRF`` and the typed front end.  Shapes and tolerances are tests/test_gpu_sequence_valued.py's: whole-sequence
marginals 1e-12, log Z 1e-10 max(1, |ref|), Viterbi score 1e-9 max(1, |ref|), windowed outputs 2e-12."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import train_objective_partial as tp
from tests import train_objective_valued as tv

pytestmark = pytest.mark.gpu

LABELS = [2, 3, 8, 17, 32]
A = 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [("random", True), ("random", False), ("hide", True), ("hide", False)]  # (masks, with values)


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


def _csr(rng, lengths, max_attrs=4):
    cptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    deg = rng.integers(0, max_attrs + 1, size=int(cptr[-1]))
    gptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    attr = rng.integers(0, A, size=int(gptr[-1])).astype(np.int32)
    return cptr, gptr, attr


def _lengths(rng):
    """About 40 contigs of 1 to 60 items, and one of 300 (several chunks of the whole-contig kernels)."""
    return [1, 2, 3] + [int(x) for x in rng.integers(1, 61, size=37)] + [300]


def _values(rng, n):
    v = rng.normal(0.0, 1.0, size=n)
    kind = rng.integers(0, 6, size=n)
    v[kind == 3] = 0.0
    v[kind == 4] = 1.0
    v[kind == 5] = 2.0 ** rng.integers(-3, 4, size=int((kind == 5).sum()))
    return v


@functools.lru_cache(maxsize=None)
def _batch(L, lengths=None):
    """The model tables, the batch, its values and both kinds of masks for L labels (computed once, never changed)."""
    rng = np.random.default_rng(5200 + L)
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    cptr, gptr, attr = _csr(rng, _lengths(rng) if lengths is None else list(lengths))
    n = int(cptr[-1])
    masks = {"random": tp.random_masks(rng, n, L), "hide": tp.hide_labels(rng, rng.integers(0, L, size=n), L)[0]}
    return dict(L=L, w=w, trans=trans, cptr=cptr, gptr=gptr, attr=attr, csr=(cptr, gptr, attr), v=_values(rng, len(attr)), masks=masks)


@functools.lru_cache(maxsize=None)
def _ref(L, kind, valued, lengths=None):
    """The yardstick's whole-sequence results for one batch, masks and values: computed once."""
    b = _batch(L, lengths)
    score = cr.masked_scores(b["gptr"], b["attr"], b["v"] if valued else None, b["w"], b["masks"][kind])
    marg, logz = cr.marginals(b["cptr"], score, b["trans"])
    y, vscore = cr.viterbi(b["cptr"], score, b["trans"])
    return dict(score=score, marg=marg, logz=logz, y=y, vscore=vscore)


def _model(nat, b):
    return nat.Model.from_tables(b["w"], b["trans"])


def _check_whole(b, r, allowed, marg, logz, y, score, tag):
    ok = tp.mask_matrix(allowed, b["L"])
    print(f"{tag}: max |marg - ref| = {np.abs(marg - r['marg']).max():.3g}, max |ln Z_A - ref| / max(1, |ref|) = "
          f"{(np.abs(logz - r['logz']) / np.maximum(1, np.abs(r['logz']))).max():.3g}, max |score - ref| / max(1, |ref|) = "
          f"{(np.abs(score - r['vscore']) / np.maximum(1, np.abs(r['vscore']))).max():.3g}")
    assert np.all(np.isfinite(marg)) and np.all(np.isfinite(logz)) and np.all(np.isfinite(score))
    assert np.all(marg[~ok] == 0.0), "a disallowed marginal is exactly 0.0"
    assert np.abs(marg - r["marg"]).max() <= 1e-12
    assert np.all(np.abs(logz - r["logz"]) <= 1e-10 * np.maximum(1.0, np.abs(r["logz"])))
    assert np.all(ok[np.arange(len(y)), y.astype(int)]), "every returned label is allowed"
    assert np.all(np.abs(score - r["vscore"]) <= 1e-9 * np.maximum(1.0, np.abs(r["vscore"])))
    for c in range(len(b["cptr"]) - 1):
        g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
        if g1 > g0:
            mine = tv.path_score(r["score"][g0:g1], b["trans"], y[g0:g1].astype(int))
            assert abs(mine - r["vscore"][c]) <= 1e-9 * max(1.0, abs(r["vscore"][c])), c


# ---------------------------------------------------------------- 1. against the yardstick
@pytest.mark.parametrize("kind,valued", KINDS)
@pytest.mark.parametrize("L", LABELS)
def test_whole_contig_entries_against_the_yardstick(nat, L, kind, valued):
    b, r = _batch(L), _ref(L, kind, valued)
    allowed, v = b["masks"][kind], (b["v"] if valued else None)
    model = _model(nat, b)
    marg, logz = model.marginals_full(*b["csr"], values=v, allowed=allowed)
    y, score = model.viterbi(*b["csr"], values=v, allowed=allowed)
    _check_whole(b, r, allowed, marg, logz, y, score, f"L={L} {kind} values={valued}")
    y2, none = model.viterbi(*b["csr"], values=v, allowed=allowed, want_score=False)
    assert none is None and np.array_equal(y, y2)


def _check_windowed(model, b, score, allowed, v, W, step, pad, tag):
    L = b["L"]
    bg = L - 1
    ok = tp.mask_matrix(allowed, L)
    exp_all, exp_any = cr.windowed(b["cptr"], score, b["trans"], W, step, background=bg, pad=pad)
    p_all, p_any = model.windowed_marginals_all(*b["csr"], W, step, background=bg, pad=pad, values=v, allowed=allowed)
    assert np.array_equal(np.isnan(p_all), np.isnan(exp_all)) and np.array_equal(np.isnan(p_any), np.isnan(exp_any))
    fin = ~np.isnan(exp_any)
    assert fin.any()
    assert np.all(p_all[fin][~ok[fin]] == 0.0), "a disallowed entry of p_all is exactly 0.0"
    assert np.array_equal(p_all == 0.0, exp_all == 0.0)
    print(f"{tag} W={W} step={step} pad={pad}: max |p_all - ref| = {np.abs(p_all[fin] - exp_all[fin]).max():.3g}, "
          f"max |p_any - ref| = {np.abs(p_any[fin] - exp_any[fin]).max():.3g}")
    assert np.abs(p_all[fin] - exp_all[fin]).max() <= 2e-12 and np.abs(p_any[fin] - exp_any[fin]).max() <= 2e-12
    for label in (0, L - 1):
        p = model.windowed_marginals(*b["csr"], W, step, label=label, pad=pad, values=v, allowed=allowed)
        assert np.array_equal(np.isnan(p), np.isnan(exp_all[:, label]))
        assert np.all(p[fin][~ok[fin, label]] == 0.0)
        assert np.abs(p[fin] - exp_all[fin, label]).max() <= 2e-12


WINDOWS = [(L, 5, 1, True) for L in LABELS] + [(L, 20, 3, True) for L in LABELS] + [(L, 20, 1, False) for L in LABELS] + \
    [(3, 40, 1, True)]  # (the last: beyond the lane-per-window tier's 32 genes, the lane-group tier)


@pytest.mark.parametrize("L,W,step,pad", WINDOWS)
def test_windowed_entries_against_the_yardstick(nat, L, W, step, pad):
    b = _batch(L)
    model = _model(nat, b)
    for kind, valued in KINDS:
        _check_windowed(model, b, _ref(L, kind, valued)["score"], b["masks"][kind], b["v"] if valued else None, W, step, pad,
                        f"L={L} {kind} values={valued}")


# ---------------------------------------------------------------- 2. every whole-contig arrangement
def _arrangement_lengths():
    rng = np.random.default_rng(77)
    return tuple([1, 2, 3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 300] + [int(x) for x in rng.integers(1, 90, size=20)])


ARRANGEMENTS = [(L, "GECCO_CRF_GENERAL_CHUNKED", "0") for L in (3, 8)] + \
    [(L, "both", mode) for L in (9, 17, 32) for mode in ("wave", "chunked", "split")]


@pytest.mark.parametrize("L,switch,mode", ARRANGEMENTS)
def test_every_whole_contig_arrangement(nat, monkeypatch, L, switch, mode):
    lengths = _arrangement_lengths()
    b, r = _batch(L, lengths), _ref(L, "random", True, lengths)
    for name in (("GECCO_CRF_GENERAL_VITERBI", "GECCO_CRF_GENERAL_MARGINALS") if switch == "both" else (switch,)):
        monkeypatch.setenv(name, mode)
    allowed = b["masks"]["random"]
    model = _model(nat, b)
    marg, logz = model.marginals_full(*b["csr"], values=b["v"], allowed=allowed)
    y, score = model.viterbi(*b["csr"], values=b["v"], allowed=allowed)
    _check_whole(b, r, allowed, marg, logz, y, score, f"L={L} {switch}={mode}")


# ---------------------------------------------------------------- 3. exact ties
@pytest.mark.parametrize("mode", [None, "wave"])
@pytest.mark.parametrize("L", [3, 17])
def test_exact_ties_take_crfsuites_path(nat, monkeypatch, L, mode):
    """Integer weights: every sum is exact on both sides, so every tie is a true tie, and the device has to break it the way
    the sequential recursion does on the masked table."""
    if mode:
        monkeypatch.setenv("GECCO_CRF_GENERAL_VITERBI", mode)
    rng = np.random.default_rng(6100 + L)
    w = rng.integers(-2, 3, size=(A, L)).astype(float)
    trans = rng.integers(-1, 2, size=(L, L)).astype(float)
    cptr, gptr, attr = _csr(rng, _lengths(rng))
    allowed = tp.random_masks(rng, int(cptr[-1]), L)
    score = cr.masked_scores(gptr, attr, None, w, allowed)
    ey, escore = cr.viterbi(cptr, score, trans)
    y, got = nat.Model.from_tables(w, trans).viterbi(cptr, gptr, attr, allowed=allowed)
    assert np.array_equal(y.astype(np.int64), ey)
    assert got.tobytes() == escore.tobytes()


# ---------------------------------------------------------------- 4. the maximum is over the allowed labels
@pytest.mark.parametrize("L", [3, 17])
def test_a_forbidden_label_that_leads_by_800(nat, L):
    """Label k leads every other label by 800 on every attribute and is forbidden everywhere.  With the state scores' maximum
    taken over all labels every allowed emission of a gene with an attribute is exp(-800 or less) = 0, and this fails."""
    rng = np.random.default_rng(6400 + L)
    k = 1
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    w[:, k] = np.delete(w, k, axis=1).max(axis=1) + 800.0
    cptr, gptr, attr = _csr(rng, _lengths(rng))
    n = int(cptr[-1])
    allowed = np.full(n, ((1 << L) - 1) & ~(1 << k), dtype=np.uint32)
    b = dict(L=L, w=w, trans=trans, cptr=cptr, gptr=gptr, attr=attr, csr=(cptr, gptr, attr))
    score = cr.masked_scores(gptr, attr, None, w, allowed)
    marg_ref, logz_ref = cr.marginals(cptr, score, trans)
    y_ref, vscore_ref = cr.viterbi(cptr, score, trans)
    model = nat.Model.from_tables(w, trans)
    marg, logz = model.marginals_full(cptr, gptr, attr, allowed=allowed)
    y, vscore = model.viterbi(cptr, gptr, attr, allowed=allowed)
    _check_whole(b, dict(score=score, marg=marg_ref, logz=logz_ref, y=y_ref, vscore=vscore_ref), allowed, marg, logz, y, vscore,
                 f"L={L} forbidden leader")
    assert not np.any(y == k)
    for W, step in ((5, 1), (20, 3)):
        _check_windowed(model, b, score, allowed, None, W, step, True, f"L={L} forbidden leader")


# ---------------------------------------------------------------- 5. a forbidden label is a smaller model
@pytest.mark.parametrize("L", [17, 9])
def test_a_label_forbidden_everywhere_is_the_smaller_model(nat, L):
    """17 -> 16 and 9 -> 8 labels: the two sides take different kernels (lane groups of 32 / 16 and 16 / 8 lanes)."""
    rng = np.random.default_rng(6700 + L)
    k = 5
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    cptr, gptr, attr = _csr(rng, _lengths(rng))
    n = int(cptr[-1])
    allowed = np.full(n, ((1 << L) - 1) & ~(1 << k), dtype=np.uint32)
    big = nat.Model.from_tables(w, trans)
    small = nat.Model.from_tables(np.delete(w, k, axis=1), np.delete(np.delete(trans, k, axis=0), k, axis=1))
    marg, _ = big.marginals_full(cptr, gptr, attr, allowed=allowed)
    smarg, _ = small.marginals_full(cptr, gptr, attr)
    assert np.all(marg[:, k] == 0.0) and np.abs(np.delete(marg, k, axis=1) - smarg).max() <= 1e-12
    y, score = big.viterbi(cptr, gptr, attr, allowed=allowed)
    sy, sscore = small.viterbi(cptr, gptr, attr)
    assert np.all(np.abs(score - sscore) <= 1e-9 * np.maximum(1.0, np.abs(sscore)))
    assert not np.any(y == k)
    assert np.array_equal(np.where(y > k, y - 1, y), sy)


# ---------------------------------------------------------------- 6. bits
def _four(model, csr, **kw):
    L = model.num_labels
    return (model.marginals_full(*csr, **kw) + model.viterbi(*csr, **kw) + model.windowed_marginals_all(*csr, 5, 1, background=0, **kw)
            + (model.windowed_marginals(*csr, 20, 3, label=L - 1, pad=False, **kw),))


@pytest.mark.parametrize("L", LABELS)
def test_full_masks_and_no_masks_give_the_same_bytes(nat, L):
    b = _batch(L)
    model = _model(nat, b)
    every = tp.full_masks(int(b["cptr"][-1]), L)
    if L == 32:
        assert every[0] == 0xFFFFFFFF
    ones = np.ones(len(b["attr"]))
    for got, exp in zip(_four(model, b["csr"], values=b["v"], allowed=every), _four(model, b["csr"], values=b["v"])):
        assert got.tobytes() == exp.tobytes()
    for got, exp in zip(_four(model, b["csr"], allowed=every), _four(model, b["csr"], values=ones)):
        assert got.tobytes() == exp.tobytes()
    for got, exp in zip(_four(model, b["csr"], allowed=None), _four(model, b["csr"])):
        assert got.tobytes() == exp.tobytes()
    for got, exp in zip(_four(model, b["csr"], values=b["v"], allowed=None), _four(model, b["csr"], values=b["v"])):
        assert got.tobytes() == exp.tobytes()


def test_bit_31_is_a_label(nat):
    b = _batch(32)
    model = _model(nat, b)
    n = int(b["cptr"][-1])
    only = np.full(n, 1 << 31, dtype=np.uint32)
    y, _ = model.viterbi(*b["csr"], allowed=only)
    marg, _ = model.marginals_full(*b["csr"], allowed=only)
    assert np.all(y == 31) and np.all(marg[:, :31] == 0.0) and np.abs(marg[:, 31] - 1.0).max() <= 1e-12
    assert np.any(b["masks"]["random"] >> 31)  # (and the yardstick tests above use it among others)


# ---------------------------------------------------------------- 7. singletons
@pytest.mark.parametrize("L", LABELS)
def test_singleton_masks_pin_the_path(nat, L):
    b = _batch(L)
    rng = np.random.default_rng(7000 + L)
    n = int(b["cptr"][-1])
    path = rng.integers(0, L, size=n)
    allowed = tp.singleton_masks(path)
    model = _model(nat, b)
    y, score = model.viterbi(*b["csr"], values=b["v"], allowed=allowed)
    marg, logz = model.marginals_full(*b["csr"], values=b["v"], allowed=allowed)
    assert np.array_equal(y.astype(np.int64), path)
    st = tv.item_scores(b["gptr"], b["attr"], b["v"], b["w"])
    for c in range(len(b["cptr"]) - 1):
        g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
        ref = tv.path_score(st[g0:g1], b["trans"], path[g0:g1])
        assert abs(score[c] - ref) <= 1e-9 * max(1.0, abs(ref)) and abs(logz[c] - ref) <= 1e-10 * max(1.0, abs(ref)), c
    on = tp.mask_matrix(allowed, L)
    assert np.all(marg[~on] == 0.0) and np.abs(marg[on] - 1.0).max() <= 1e-12


# ---------------------------------------------------------------- 8. slices
RAW = {  # entry -> (symbol, windowed, outputs as (dtype, "gene" | "gene_label" | "contig"))
    "viterbi": ("gecco_crf_viterbi_constrained", False, ((np.int8, "gene"), (np.float64, "contig"))),
    "full": ("gecco_crf_marginals_full_constrained", False, ((np.float64, "gene_label"), (np.float64, "contig"))),
    "windowed": ("gecco_crf_windowed_marginals_constrained", True, ((np.float64, "gene"),)),
    "all": ("gecco_crf_windowed_marginals_all_constrained", True, ((np.float64, "gene_label"), (np.float64, "gene"))),
}
FILL = -7.0


def _raw(nat, model, entry, cptr, gptr, attr, v, allowed):
    symbol, windowed, outputs = RAW[entry]
    cptr, gptr, attr, v, allowed = (np.ascontiguousarray(x) for x in (cptr, gptr, attr, v, allowed))
    nc, n, L = len(cptr) - 1, int(cptr[-1] - cptr[0]), model.num_labels
    size = {"gene": n, "gene_label": n * L, "contig": nc}
    bufs = [np.full(max(size[kind], 1), FILL).astype(dtype) for dtype, kind in outputs]
    fn = getattr(nat.load_library(), symbol)
    args = [cptr, nc, gptr, attr, v, allowed] + ([5, 2, 1 if entry == "windowed" else 0, 1] if windowed else []) + bufs
    c_args = [x.ctypes.data_as(t) if isinstance(x, np.ndarray) else x for x, t in zip(args, fn.argtypes[2:])]
    rc = fn(model._h, 0, *c_args)
    assert rc == nat.OK, nat.load_library().gecco_crf_last_error().decode()
    return [buf[:size[kind]] for buf, (_, kind) in zip(bufs, outputs)]


@pytest.mark.parametrize("entry", list(RAW))
@pytest.mark.parametrize("L", [2, 5, 12])
def test_a_slice_gives_the_bytes_of_the_rebased_batch(nat, L, entry):
    """contig_ptr[0] > 0: one set of arrays, the contigs behind the first two.  The masks are indexed like gene_ptr's rows."""
    rng = np.random.default_rng(7300 + L)
    model = nat.Model.from_tables(rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L)))
    cptr, gptr, attr = _csr(rng, [4, 9, 3, 30, 1, 70])
    gptr = (gptr + 0).astype(np.int32)
    v = _values(rng, len(attr))
    allowed = tp.random_masks(rng, int(cptr[-1]), L)
    g0 = int(cptr[2])
    a0 = int(gptr[g0])
    assert g0 > 0 and a0 > 0
    allowed[:g0] = 0  # (masks of genes outside the batch are not looked at)
    got = _raw(nat, model, entry, cptr[2:], gptr, attr, v, allowed)
    alone = _raw(nat, model, entry, cptr[2:] - g0, gptr[g0:] - a0, attr[a0:], v[a0:], allowed[g0:])
    for x, y in zip(got, alone):
        assert x.size and not np.any(x == np.asarray(FILL).astype(x.dtype)), "not written"
        assert x.tobytes() == y.tobytes()
    if entry == "full":  # ... and they are the yardstick's
        score = cr.masked_scores(gptr[g0:] - a0, attr[a0:], v[a0:], model.state_weights()[0], allowed[g0:])
        marg, _ = cr.marginals(cptr[2:] - g0, score, model.trans_weights()[0])
        assert np.abs(got[0].reshape(-1, L) - marg).max() <= 1e-12


# ---------------------------------------------------------------- 9. SequenceCRF end to end
def _names_data(rng, n_seqs, lo=6, hi=20):
    X, y = [], []
    for _ in range(n_seqs):
        n = int(rng.integers(lo, hi + 1))
        labs = [str(rng.choice(["a", "b", "c"])) for _ in range(n)]
        X.append([["bias", "kind:" + ("c" if lab == "c" else "ab")] + (["tag:" + lab] if rng.random() < 0.4 else []) for lab in labs])
        y.append(labs)
    return X, y


def _sets_for(rng, yseq):
    """fit's grammar: the label, a set holding it, a tuple, or None."""
    out = []
    for lab in yseq:
        kind = int(rng.integers(0, 4))
        other = str(rng.choice(["a", "b", "c"]))
        out.append(lab if kind == 0 else {lab, other} if kind == 1 else (other, lab) if kind == 2 else None)
    return out


@pytest.fixture(scope="module")
def fitted(nat):
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(31)
    X, y = _names_data(rng, 25)
    return SequenceCRF(window_size=None, c1=0.05, c2=0.1, max_iterations=30).fit(X, y)


def _pack_names(crf, X):
    index = {a: i for i, a in enumerate(crf.attributes_)}
    cptr, gptr, attr = [0], [0], []
    for xs in X:
        for item in xs:
            attr.extend(index[nm] for nm in dict.fromkeys(item) if nm in index)
            gptr.append(len(attr))
        cptr.append(len(gptr) - 1)
    return tuple(np.array(a, dtype=np.int32) for a in (cptr, gptr, attr))


def test_sequence_crf_end_to_end(nat, fitted):
    crf = fitted
    assert sorted(crf.classes_) == ["a", "b", "c"]
    rng = np.random.default_rng(32)
    X, y = _names_data(rng, 8, lo=1)
    X.insert(2, [])
    y.insert(2, [])
    sets = [_sets_for(rng, ys) for ys in y]
    cptr, gptr, attr = _pack_names(crf, X)
    masks, single = crf._label_sets(sets, cptr, "allowed")
    assert not single
    model = nat.Model.from_lcrf(crf.to_bytes())
    ey, _ = model.viterbi(cptr, gptr, attr, allowed=masks)
    emarg, elogz = model.marginals_full(cptr, gptr, attr, allowed=masks)
    got = crf.predict(X, allowed=sets)
    assert [len(ys) for ys in got] == [len(xs) for xs in X]
    assert [lab for ys in got for lab in ys] == [crf.classes_[k] for k in ey.tolist()]
    assert np.concatenate(crf.predict_marginals(X, allowed=sets)).tobytes() == emarg.tobytes()
    assert crf.predict(X, allowed=None) == crf.predict(X)
    # log_likelihood with sets: log Z_A - log Z, against the yardstick within the sum of the two log Z bounds
    w, trans = model.state_weights()[0], model.trans_weights()[0]
    every = tp.full_masks(len(masks), 3)
    _, ref_a = cr.marginals(cptr, cr.masked_scores(gptr, attr, None, w, masks), trans)
    _, ref_z = cr.marginals(cptr, cr.masked_scores(gptr, attr, None, w, every), trans)
    ll = crf.log_likelihood(X, sets)
    bound = 1e-10 * (np.maximum(1.0, np.abs(ref_a)) + np.maximum(1.0, np.abs(ref_z)))
    print(f"log_likelihood with sets: max |ll - ref| = {np.abs(ll - (ref_a - ref_z)).max():.3g}, max ll = {ll.max():.3g}")
    assert np.all(np.abs(ll - (ref_a - ref_z)) <= bound)
    assert np.all(ll <= bound) and ll[2] == 0.0 and np.any(ll < -1e-3)
    nothing = crf.log_likelihood(X, [[None] * len(xs) for xs in X])
    assert nothing.tobytes() == np.zeros(len(X)).tobytes()
    # entries that each name one label, however written: the gold-path code and its bits
    assert crf.log_likelihood(X, [[{lab} if t % 2 else (lab,) for t, lab in enumerate(ys)] for ys in y]).tobytes() == \
        crf.log_likelihood(X, y).tobytes()
    # ... which the restricted lattice of singletons agrees with (one path: log Z_A is its score)
    pinned = crf._log_probability_inside(cptr, gptr, attr, None, crf._label_sets(y, cptr, "y")[0])
    assert np.allclose(pinned, crf.log_likelihood(X, y), rtol=0, atol=float(bound.max()))


def test_windowed_sequence_crf_takes_allowed(nat, fitted):
    from gecco_amd.sequence import SequenceCRF

    crf = SequenceCRF.from_bytes(fitted.to_bytes(), window_size=5)
    rng = np.random.default_rng(33)
    X, y = _names_data(rng, 6, lo=2)
    sets = [_sets_for(rng, ys) for ys in y]
    cptr, gptr, attr = _pack_names(crf, X)
    masks = crf._label_sets(sets, cptr, "allowed")[0]
    model = nat.Model.from_lcrf(crf.to_bytes())
    bg = crf.classes_.index("c")
    eall, eany = model.windowed_marginals_all(cptr, gptr, attr, 5, 1, background=bg, allowed=masks)
    ep = model.windowed_marginals(cptr, gptr, attr, 5, 1, label=crf.classes_.index("b"), allowed=masks)
    p_all, p_any = crf.predict_windowed_all(X, background="c", allowed=sets)
    assert np.concatenate(p_all).tobytes() == eall.tobytes() and np.concatenate(p_any).tobytes() == eany.tobytes()
    assert np.concatenate(crf.predict_windowed(X, "b", allowed=sets)).tobytes() == ep.tobytes()
    assert np.all(eall[~tp.mask_matrix(masks, 3)] == 0.0)


def test_log_likelihood_is_the_partial_trainers_objective(nat):
    """One whole-sequence problem with masks: the trainer's f = sum over sequences of (log Z - log Z_A) is minus the sum of
    log_likelihood under the model of the same weights."""
    from gecco_amd import _native
    from gecco_amd.crfsuite_model import model_bytes
    from gecco_amd.sequence import SequenceCRF
    from tests.train_objective_labels import labelled_sequences

    rng = np.random.default_rng(41)
    L, An = 3, 12
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, [1, 2, 7, 30, 64, 65, 9], An, L, stay=0.8)
    sfid = np.arange(An * L, dtype=np.int32)
    tfid = An * L + np.arange(L * L, dtype=np.int32)
    K = An * L + L * L
    masks, _ = tp.hide_labels(rng, labels, L)
    w = rng.normal(0.0, 1.0, size=K)
    w[w == 0] = 0.5
    tr = _native.TrainerSequences([(seq_ptr, item_ptr, attr_id, None, An, sfid, tfid, K)], allowed=[masks])
    f, _ = tr.eval([w])
    _, _, _, groups = tp.objective_partial(seq_ptr, item_ptr, attr_id, masks, An, L, None, None, sfid, tfid, w, details=True)
    tol_f, _ = tp.partial_tolerances(L, groups)
    names, classes = [f"a{k}" for k in range(An)], [f"l{k}" for k in range(L)]
    blob = model_bytes(classes, names, np.repeat(np.arange(An), L), np.tile(np.arange(L), An), np.repeat(np.arange(L), L),
                       np.tile(np.arange(L), L), w)
    crf = SequenceCRF.from_bytes(blob, window_size=None)
    assert crf.classes_ == classes and crf.attributes_ == names
    X = [[[names[a] for a in attr_id[item_ptr[i]:item_ptr[i + 1]]] for i in range(seq_ptr[s], seq_ptr[s + 1])]
         for s in range(len(seq_ptr) - 1)]
    ysets = [[{classes[l] for l in range(L) if (int(masks[i]) >> l) & 1} for i in range(seq_ptr[s], seq_ptr[s + 1])]
             for s in range(len(seq_ptr) - 1)]
    ll = crf.log_likelihood(X, ysets)
    S, T = w[:An * L].reshape(An, L), w[An * L:].reshape(L, L)
    _, ref_a = cr.marginals(seq_ptr, cr.masked_scores(item_ptr, attr_id, None, S, masks), T)
    _, ref_z = cr.marginals(seq_ptr, cr.masked_scores(item_ptr, attr_id, None, S, tp.full_masks(len(masks), L)), T)
    ll_bound = float(np.sum(1e-10 * (np.maximum(1.0, np.abs(ref_a)) + np.maximum(1.0, np.abs(ref_z)))))
    print(f"trainer f = {f[0]!r}, -sum log_likelihood = {-ll.sum()!r}, tol_f = {tol_f:.3g}, log-likelihood bound = {ll_bound:.3g}")
    assert abs(f[0] + ll.sum()) <= tol_f + ll_bound


# ---------------------------------------------------------------- 10. the typed front end
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


def test_typed_front_end_with_known_regions(nat, tmp_path):
    from gecco_amd import tables, typed
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
    plain_genes, plain_clusters = crf.predict_genes_and_clusters(genes)
    # background genes 60 .. 69 of the first contig: below the threshold without knowledge, outside every called cluster
    region = list(range(60, 70))
    ids = [g.id for g in plain_genes]
    assert ids[60].startswith("fresh00")
    assert max(plain_genes[i].average_probability for i in region) < 0.8
    assert sum(1 for i in region if plain_genes[i].protein.domains) >= 3
    inside = lambda c: c.source.id == "fresh00" and c.start <= plain_genes[69].end and plain_genes[60].start <= c.end
    assert not any(inside(c) for c in plain_clusters)
    bg = crf.classes_.index("0")
    for kind, mask in (("Beta", 1 << crf.classes_.index("Beta")), ("Unknown", ((1 << len(crf.classes_)) - 1) & ~(1 << bg))):
        known = tables.ClusterTable({"sequence_id": ["fresh00"], "cluster_id": ["k1"], "start": [plain_genes[60].start],
                                     "end": [plain_genes[69].end], "type": [kind]})
        annotated, found = crf.predict_genes_and_clusters(genes, known=known)
        p_all = crf.predict_label_probabilities(genes, known=known)
        p_any = np.array([g.average_probability for g in annotated])
        assert [g.id for g in annotated] == ids
        assert np.all(p_any[region] >= 1.0 - 1e-12) and np.all(p_all[region, bg] == 0.0)
        off = ~tp.mask_matrix(np.full(len(region), mask, dtype=np.uint32), len(crf.classes_))
        assert np.all(p_all[region][off] == 0.0)
        assert [g.average_probability for g in crf.predict_probabilities(genes, known=known)] == p_any.tolist()
        called = [c for c in found if inside(c)]
        assert len(called) == 1 and {g.id for g in called[0].genes} >= {ids[i] for i in region if plain_genes[i].protein.domains}
        assert [c.id for c in crf.predict_clusters(genes, known=known)] == [c.id for c in found]
        if kind == "Beta":
            assert str(called[0].type) == "Beta"
            beta_known, beta_found, beta_annotated = known, found, annotated
    # known=None: today's tables, byte for byte
    again_genes, again_clusters = crf.predict_genes_and_clusters(genes, known=None)
    _dump(os.path.join(base, "plain"), crf, plain_genes, plain_clusters)
    _dump(os.path.join(base, "again"), crf, again_genes, again_clusters)
    _same_tables(os.path.join(base, "plain"), os.path.join(base, "again"))
    # the command line with --known writes the method's tables
    crf.save(os.path.join(base, "model"))
    beta_known.dump(os.path.join(base, "known.tsv"))
    _dump(os.path.join(base, "method"), crf, beta_annotated, beta_found)
    done = subprocess.run([sys.executable, "-m", "gecco_amd.typed", "predict", "--model", os.path.join(base, "model"), "--genes",
                           os.path.join(base, "fresh", "genes.tsv"), "--features", os.path.join(base, "fresh", "features.tsv"),
                           "--known", os.path.join(base, "known.tsv"), "-o", os.path.join(base, "cli")],
                          cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    _same_tables(os.path.join(base, "method"), os.path.join(base, "cli"))
