"""``gecco_crf_ring`` on the device against tests/ring_reference.py (pinned on path enumeration by tests/test_ring_host.py): every
contig is a ring whose last item has a transition into its first.  The batches are those of tests/test_gpu_kbest.py; every kind of
call -- plain, valued, masked, valued and masked -- runs everywhere.  Tolerances: log Z of the ring within
``ring_reference.lognorm_bound``, marginals within 1e-12 (the project's tolerance for a whole-contig marginal,
tests/test_gpu_constrained.py), scores within ``ring_reference.bound``; with integer weights scores and labels are exact."""
import functools
import os

import numpy as np
import pytest

from tests import minrun_reference as mr
from tests import ring_reference as rr
from tests.test_gpu_kbest import enumeration_lengths, kw, make_batch, nat, seam_lengths, sequence_crf, tables  # noqa: F401

pytestmark = pytest.mark.gpu

NINF = -np.inf
KINDS = [(False, False), (True, False), (False, True), (True, True)]
ENUMERATE_UP_TO = 1100  # paths: 2**6, 3**6, 8**3, 9**3, 32**2


# ---------------------------------------------------------------- batches and the yardstick
def assemble(b, rings, masks=None):
    """A batch over the items of ``b``: ``rings`` holds per ring the indices of its items in ``b`` (-1: an item without
    attributes), ``masks`` (optional) their masks in place of ``b``'s."""
    gptr, attr, v = b["gptr"], b["attr"], b["v"]
    new_attr, new_v, new_gptr, new_allowed = [], [], [0], []
    every = np.uint32((1 << b["L"]) - 1)
    for k, items in enumerate(rings):
        for t, i in enumerate(items):
            if i >= 0:
                new_attr.append(attr[gptr[i]:gptr[i + 1]])
                new_v.append(v[gptr[i]:gptr[i + 1]])
            new_gptr.append(new_gptr[-1] + (int(gptr[i + 1] - gptr[i]) if i >= 0 else 0))
            new_allowed.append(masks[k][t] if masks is not None else (b["allowed"][i] if i >= 0 else every))
    cptr = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    out = dict(L=b["L"], w=b["w"], trans=b["trans"], cptr=cptr, gptr=np.array(new_gptr, dtype=np.int32),
               attr=np.concatenate(new_attr + [np.zeros(0, dtype=np.int32)]).astype(np.int32),
               v=np.concatenate(new_v + [np.zeros(0)]), allowed=np.array(new_allowed, dtype=np.uint32))
    out["csr"] = (out["cptr"], out["gptr"], out["attr"])
    return out


def items_of(b, c):
    return list(range(int(b["cptr"][c]), int(b["cptr"][c + 1])))


def reference(b, valued, masked):
    """Per ring None (no items) or a dict: ``lognorm``, ``marginals``, ``score``, ``path`` (by enumeration where the ring has at
    most ENUMERATE_UP_TO paths, else by the yardstick's walks), ``largest`` and the bounds.  Computed once per batch and kind."""
    key = ("ring", valued, masked)
    if key not in b:
        score, absolute = tables(b, valued, masked)
        out = []
        for c in range(len(b["cptr"]) - 1):
            g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
            if g1 == g0:
                out.append(None)
                continue
            T = g1 - g0
            lognorm, marg, largest = rr.sum_walks(score[g0:g1], b["trans"])
            path, best = rr.best_path(score[g0:g1], b["trans"])
            if b["L"] ** T <= ENUMERATE_UP_TO:
                e = rr.enumerate_ring(score[g0:g1], b["trans"])
                lognorm, marg, best = e["lognorm"], e["marginals"], e["score"]
            out.append(dict(lognorm=float(lognorm), marginals=marg, score=best, path=path, largest=largest, table=score[g0:g1],
                            lognorm_bound=rr.lognorm_bound(T, b["L"], largest), B=rr.bound(absolute[g0:g1], np.abs(b["trans"]))))
        b[key] = out
    return b[key]


def accept(tag, b, ref, out, exact=False):
    """The acceptance of a whole call: shapes, no NaN, -inf exactly where the yardstick has it, log Z within its bound, marginals
    and their row sums within 1e-12, the score and the returned path's own score within B (exact: bits and labels)."""
    cptr = b["cptr"]
    n, nc, L = int(cptr[-1]), len(cptr) - 1, b["L"]
    y, score, marg, lognorm = out["labels"], out["score"], out["marginals"], out["lognorm"]
    assert y.shape == (n,) and y.dtype == np.int8 and score.shape == (nc,) and marg.shape == (n, L) and lognorm.shape == (nc,)
    assert not np.isnan(score).any() and not np.isnan(marg).any() and not np.isnan(lognorm).any(), f"{tag}: NaN"
    assert not np.isposinf(score).any() and not np.isposinf(lognorm).any() and marg.min() >= 0.0 and marg.max() <= 1.0, tag
    worst = [0.0, 0.0, 0.0]
    for c, r in enumerate(ref):
        g0, g1 = int(cptr[c]), int(cptr[c + 1])
        if r is None:
            assert lognorm[c] == 0.0 and score[c] == 0.0, f"{tag} ring {c}: a ring without items has log Z 0 and score 0"
            continue
        where = f"{tag} ring {c} of {g1 - g0} items"
        if r["lognorm"] == NINF:
            assert lognorm[c] == NINF and score[c] == NINF and not marg[g0:g1].any() and np.all(y[g0:g1] == -1), where
            continue
        err = abs(lognorm[c] - r["lognorm"])
        worst[0] = max(worst[0], err / r["lognorm_bound"])
        assert err <= r["lognorm_bound"], f"{where}: log Z off by {err:.3g}, bound {r['lognorm_bound']:.3g}"
        err = np.abs(marg[g0:g1] - r["marginals"]).max()
        worst[1] = max(worst[1], err)
        assert err <= 1e-12, f"{where}: a marginal is off by {err:.3g}"
        assert np.abs(marg[g0:g1].sum(axis=1) - 1.0).max() <= 1e-12, f"{where}: a row of marginals does not sum to 1"
        assert np.all(marg[g0:g1][r["table"] == NINF] == 0.0), f"{where}: a disallowed pair is exactly 0.0"
        assert np.all((y[g0:g1] >= 0) & (y[g0:g1] < L)), where
        own = rr.ring_score(r["table"], b["trans"], y[g0:g1].astype(np.int64))
        if exact:
            assert score[c] == r["score"], f"{where}: score {score[c]!r}, expected {r['score']!r}"
            assert y[g0:g1].tolist() == r["path"].tolist(), f"{where}: another path"
            assert own == score[c], where
        else:
            err = abs(score[c] - r["score"])
            worst[2] = max(worst[2], err / r["B"] if r["B"] > 0 else (0.0 if err == 0 else np.inf))
            assert err <= r["B"], f"{where}: score off by {err:.3g}, B = {r['B']:.3g}"
            assert abs(own - score[c]) <= r["B"], f"{where}: the returned path scores {own!r}, the call says {score[c]!r}"
    print(f"{tag}: worst |log Z error| / bound = {worst[0]:.3g}, worst marginal error = {worst[1]:.3g}, worst |score error| / B = {worst[2]:.3g}")


def run(nat, b, valued, masked, **more):
    model = nat.Model.from_tables(b["w"], b["trans"])
    return model.ring(*b["csr"], **kw(b, valued, masked), **more)


@functools.lru_cache(maxsize=None)
def enumeration_batch(L):
    return make_batch(9500 + L, L, enumeration_lengths())


# ---------------------------------------------------------------- 1. enumeration
@pytest.mark.parametrize("L", [2, 3, 8, 9, 32])
def test_enumeration(nat, L):
    b = enumeration_batch(L)
    assert 0 in np.diff(b["cptr"]).tolist()[1:-1], "an empty ring in the middle of the batch"
    for valued, masked in KINDS:
        accept(f"L={L} valued={valued} masked={masked}", b, reference(b, valued, masked), run(nat, b, valued, masked))


# ---------------------------------------------------------------- 2. exact arithmetic
@pytest.mark.parametrize("L", [2, 3, 8, 9, 17, 32])
def test_exact_arithmetic_and_planted_ties(nat, L):
    b = make_batch(9600 + L, L, [1, 2, 3, 6, 0, 9, 17, 33, 5, 64], integer=True)
    b["v"] = np.round(b["v"])  # (integer values keep the valued kinds exact)
    for valued, masked in KINDS:
        accept(f"integer L={L} valued={valued} masked={masked}", b, reference(b, valued, masked), run(nat, b, valued, masked), exact=True)
    # every path ties: the smallest start label, then the earlier source at every step
    plain = {k: x for k, x in b.items() if isinstance(k, str)}  # (without the cached references)
    z = dict(plain, w=np.zeros_like(b["w"]), trans=np.zeros_like(b["trans"]))
    out = run(nat, z, False, False)
    assert not out["labels"].any() and not out["score"].any()
    # two start labels with equal closed[a], and equal sources inside the conditioned walk: labels 0 and 1 are twins
    t = dict(plain, w=b["w"].copy(), trans=b["trans"].copy())
    t["w"][:, 1] = t["w"][:, 0]
    t["trans"][1, :] = t["trans"][0, :]
    t["trans"][:, 1] = t["trans"][:, 0]
    for valued, masked in ((False, False), (True, False)):
        out = run(nat, t, valued, masked)
        accept(f"twins L={L} valued={valued}", t, reference(t, valued, masked), out, exact=True)
        assert not (out["labels"] == 1).any(), "the smaller of two tied labels wins everywhere"


# ---------------------------------------------------------------- 3. seams
@pytest.mark.parametrize("L", [2, 9, 17, 32])
def test_walks_at_the_seams(nat, L):
    lengths = seam_lengths(L)
    assert min(lengths) == 1 and max(lengths) == 300
    b = make_batch(9700 + L, L, lengths)
    for valued, masked in KINDS:
        accept(f"seams L={L} valued={valued} masked={masked}", b, reference(b, valued, masked), run(nat, b, valued, masked))


# ---------------------------------------------------------------- 4. device against device
@pytest.mark.parametrize("L", [2, 8, 32])
def test_the_ring_is_the_mix_of_its_pinned_chain_copies(nat, L):
    """The route the entry replaces: one (n + 1)-item chain per start label a, item 0 pinned to a and an appended item without
    attributes pinned to a as well, so that the chain's last transition is the closing edge; log Z_ring is the log-sum-exp of
    the copies' log Z and a ring marginal the mix of the copies' marginals under those weights.  The copies go through the
    constrained whole-contig marginals the project already trusts.  (On the parent commit the ring entry does not exist.)"""
    lengths = list(range(1, 41))
    b = make_batch(9800 + L, L, lengths)
    model = nat.Model.from_tables(b["w"], b["trans"])
    every = (1 << L) - 1
    for valued, masked in KINDS:
        ring = run(nat, b, valued, masked, want_path=False)
        ref = reference(b, valued, masked)
        rings, masks, owner = [], [], []
        for c, T in enumerate(lengths):
            items = items_of(b, c)
            base = [int(b["allowed"][i]) if masked else every for i in items]
            for a in range(L):
                if not (base[0] >> a) & 1:
                    continue  # (no path starts at a: the copy has no mass)
                rings.append(items + [-1])
                masks.append([1 << a] + base[1:] + [1 << a])
                owner.append((c, a))
        copies = assemble(b, rings, masks)
        marg, lognorm = model.marginals_full(*copies["csr"], values=copies["v"] if valued else None, allowed=copies["allowed"])
        worst = 0.0
        for c, T in enumerate(lengths):
            mine = [k for k, (cc, _) in enumerate(owner) if cc == c]
            ln = lognorm[mine]
            total = ln.max() + np.log(np.exp(ln - ln.max()).sum())
            bound = ref[c]["lognorm_bound"] + mr.lognorm_bound(T + 1, L, ref[c]["largest"])
            assert abs(ring["lognorm"][c] - total) <= bound, (L, valued, masked, c, ring["lognorm"][c], total, bound)
            mix = sum(np.exp(lognorm[k] - total) * marg[copies["cptr"][k]:copies["cptr"][k] + T] for k in mine)
            err = np.abs(ring["marginals"][b["cptr"][c]:b["cptr"][c + 1]] - mix).max()
            worst = max(worst, err)
            assert err <= 1e-12, (L, valued, masked, c, err)
        print(f"copies L={L} valued={valued} masked={masked}: worst marginal difference {worst:.3g}")


# ---------------------------------------------------------------- 5. rotation
@pytest.mark.parametrize("L", [2, 5, 32])
def test_rotating_a_ring_rotates_its_answers(nat, L):
    """Every rotation of rings of 7 and 64 items: log Z of the ring within the bound of the yardstick's value for the ring as
    given, the marginals rotated within 1e-12, the score within B; with integer weights and a unique best path the path rotates
    label for label.  The same sequences through the chain entries (``viterbi``, ``marginals_full``) fail this property: a
    chain has two free ends, and where they lie changes log Z, the marginals near them and the path."""
    b = make_batch(9900 + L, L, [7, 64])
    rings = [np.roll(items_of(b, c), -r).tolist() for c in (0, 1) for r in range(len(items_of(b, c)))]
    rot = assemble(b, rings)
    first = {0: 0, 1: 7}
    for valued, masked in KINDS:
        out = run(nat, rot, valued, masked)
        ref = reference(b, valued, masked)
        for c in (0, 1):
            T = 7 if c == 0 else 64
            r0 = ref[c]
            for r in range(T):
                k = first[c] + r
                g0 = int(rot["cptr"][k])
                assert abs(out["lognorm"][k] - r0["lognorm"]) <= r0["lognorm_bound"], (L, valued, masked, c, r)
                assert np.abs(out["marginals"][g0:g0 + T] - np.roll(r0["marginals"], -r, axis=0)).max() <= 1e-12, (L, valued, masked, c, r)
                assert abs(out["score"][k] - r0["score"]) <= r0["B"], (L, valued, masked, c, r)
    # integer weights, and one label of every item lifted so that the best path is unique
    rng = np.random.default_rng(L)
    bi = make_batch(9950 + L, L, [7, 64], integer=True)
    n = int(bi["cptr"][-1])
    lift = rng.integers(0, L, size=n)
    bi["w"][bi["attr"][bi["gptr"][:-1]], lift] += 50.0  # (an item's first attribute is its own)
    bi["allowed"] |= (np.uint32(1) << lift.astype(np.uint32))
    rot = assemble(bi, rings)
    for masked in (False, True):
        base = run(nat, bi, False, masked, want_marginals=False)
        out = run(nat, rot, False, masked, want_marginals=False)
        for c in (0, 1):
            T = 7 if c == 0 else 64
            path = base["labels"][bi["cptr"][c]:bi["cptr"][c + 1]]
            assert path.tolist() == lift[bi["cptr"][c]:bi["cptr"][c + 1]].tolist(), "the lifted labels are the best path"
            for r in range(T):
                k = first[c] + r
                g0 = int(rot["cptr"][k])
                assert out["score"][k] == base["score"][c] and out["labels"][g0:g0 + T].tolist() == np.roll(path, -r).tolist()


# ---------------------------------------------------------------- 6. extreme weights
@pytest.mark.parametrize("L", [2, 9, 32])
def test_extreme_weights(nat, L):
    """Weights of +-700 and, in the valued kinds, values of +-1 and +-2: state scores of magnitude 700 to 4200 with mixed signs.
    The values are integers because the tolerance of a marginal is absolute: at this magnitude one ulp of a state score is
    4.5e-13, the device forms a valued score with fused multiply-adds and numpy with a product and a sum, and a ring of 33
    items with real values starts from tables that differ by more than 1e-12 in a path's score before any walk has run.  With
    integer values the tables are equal and exact, and every difference the test sees is the walks'."""
    b = make_batch(10000 + L, L, [1, 2, 3, 9, 33, 0, 100])
    rng = np.random.default_rng(L)
    b["w"] = 700.0 * rng.choice([-1.0, 1.0], size=b["w"].shape)
    b["trans"] = 700.0 * rng.choice([-1.0, 1.0], size=b["trans"].shape)
    b["v"] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=b["v"].shape)
    # real weights of the same magnitude, without values: the device and numpy add an item's weights in the same order, so the
    # tables are the same bits and rounding at this magnitude is the walks' own
    r = make_batch(10050 + L, L, [1, 2, 3, 9, 33, 0, 100])
    r["w"] = rng.uniform(500.0, 700.0, size=r["w"].shape) * rng.choice([-1.0, 1.0], size=r["w"].shape)
    r["trans"] = rng.uniform(500.0, 700.0, size=r["trans"].shape) * rng.choice([-1.0, 1.0], size=r["trans"].shape)
    for masked in (False, True):
        accept(f"extreme real L={L} masked={masked}", r, reference(r, False, masked), run(nat, r, False, masked))
    for valued, masked in KINDS:
        accept(f"extreme L={L} valued={valued} masked={masked}", b, reference(b, valued, masked), run(nat, b, valued, masked))


# ---------------------------------------------------------------- 7. infeasible and degenerate rings
@pytest.mark.parametrize("L", [2, 9, 32])
def test_infeasible_and_pinned_rings(nat, L):
    b = make_batch(10100 + L, L, [4, 1, 6, 3, 1, 12])
    allowed = b["allowed"].copy()
    allowed[int(b["cptr"][2]) + 3] = 0  # ring 2: one item allows no label
    allowed[int(b["cptr"][4])] = 0      # ring 4, of one item: likewise
    model = nat.Model.from_tables(b["w"], b["trans"])
    out = model.ring(*b["csr"], allowed=allowed)
    for c in range(6):
        g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
        if c in (2, 4):
            assert out["lognorm"][c] == NINF and out["score"][c] == NINF and np.all(out["labels"][g0:g1] == -1)
            assert not out["marginals"][g0:g1].any()
        else:
            assert np.isfinite(out["lognorm"][c]) and np.isfinite(out["score"][c]) and np.all(out["labels"][g0:g1] >= 0)
    assert not np.isnan(out["marginals"]).any() and not np.isnan(out["lognorm"]).any() and not np.isnan(out["score"]).any()
    alone = model.ring(*b["csr"], allowed=b["allowed"])  # the other rings do not notice
    for c in (0, 1, 3, 5):
        g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
        assert out["lognorm"][c] == alone["lognorm"][c] and out["labels"][g0:g1].tobytes() == alone["labels"][g0:g1].tobytes()
    # every item pinned: one path, log-probability 0, one-hot marginals -- exactly so with integer weights
    rng = np.random.default_rng(L)
    for integer in (False, True):
        p = make_batch(10150 + L, L, [4, 1, 6, 3, 2, 40], integer=integer)
        n = int(p["cptr"][-1])
        pins = rng.integers(0, L, size=n)
        out = nat.Model.from_tables(p["w"], p["trans"]).ring(*p["csr"], allowed=(np.uint32(1) << pins.astype(np.uint32)))
        assert out["labels"].tolist() == pins.tolist()
        assert np.all(np.abs(out["score"] - out["lognorm"]) <= 1e-12), "the one path has log-probability 0"
        hot = np.eye(L)[pins]
        assert np.all(out["marginals"][hot == 0] == 0.0) and np.abs(out["marginals"] - hot).max() <= 1e-12
        if integer:
            assert np.array_equal(out["marginals"], hot) and np.array_equal(out["score"], out["lognorm"])


# ---------------------------------------------------------------- 8. independence and determinism
@pytest.mark.parametrize("L", [2, 9, 17, 32])
def test_a_rings_bytes_are_its_own(nat, L):
    b = make_batch(10200 + L, L, seam_lengths(L)[:24] + [0, 5])
    nc = len(b["cptr"]) - 1
    for valued, masked in KINDS:
        whole = run(nat, b, valued, masked)
        again = run(nat, b, valued, masked)
        for name in whole:
            assert whole[name].tobytes() == again[name].tobytes(), f"{name}: two equal calls give equal bytes"
        order = np.random.default_rng(L).permutation(nc)
        shuffled = assemble(b, [items_of(b, c) for c in order])
        out = run(nat, shuffled, valued, masked)
        for k, c in enumerate(order.tolist()):
            for name in ("lognorm", "score"):
                assert out[name][k:k + 1].tobytes() == whole[name][c:c + 1].tobytes(), (name, c)
            s0, s1, g0, g1 = int(shuffled["cptr"][k]), int(shuffled["cptr"][k + 1]), int(b["cptr"][c]), int(b["cptr"][c + 1])
            for name in ("labels", "marginals"):
                assert out[name][s0:s1].tobytes() == whole[name][g0:g1].tobytes(), (name, c)
        for c in (0, nc // 2, nc - 1):  # the same ring alone
            alone = run(nat, assemble(b, [items_of(b, c)]), valued, masked)
            g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
            assert alone["lognorm"].tobytes() == whole["lognorm"][c:c + 1].tobytes() and alone["score"].tobytes() == whole["score"][c:c + 1].tobytes()
            assert alone["labels"].tobytes() == whole["labels"][g0:g1].tobytes() and alone["marginals"].tobytes() == whole["marginals"][g0:g1].tobytes()
        # what is asked for changes no byte of the rest
        paths = run(nat, b, valued, masked, want_marginals=False)
        margs = run(nat, b, valued, masked, want_path=False)
        only = run(nat, b, valued, masked, want_path=False, want_marginals=False)
        assert sorted(paths) == ["labels", "lognorm", "score"] and sorted(margs) == ["lognorm", "marginals"] and sorted(only) == ["lognorm"]
        for got in (paths, margs, only):
            for name in got:
                assert got[name].tobytes() == whole[name].tobytes(), name


# ---------------------------------------------------------------- 9. refusals
def test_refusals_reach_the_caller(nat):
    b = make_batch(10300, 3, [3, 2])
    model = nat.Model.from_tables(b["w"], b["trans"])
    lib = nat.load_library()
    cptr, gptr, attr = b["csr"]
    head = [model._h, 0, nat._ptr(cptr, nat._c_i32p), 2, nat._ptr(gptr, nat._c_i32p), nat._ptr(attr, nat._c_i32p), None, None]
    y, score, lz = np.zeros(5, dtype=np.int8), np.zeros(2), np.zeros(2)
    py, ps, pl = nat._ptr(y, nat._c_i8p), nat._ptr(score, nat._c_f64p), nat._ptr(lz, nat._c_f64p)
    for tail, text in (((py, ps, None, None), "ring: lognorm_ring is NULL"), ((py, None, None, pl), "ring: y given without score"),
                       ((None, ps, None, pl), "ring: score given without y")):
        with pytest.raises(ValueError, match=text):
            nat._check(lib.gecco_crf_ring(*head, *tail))
    wide = nat.Model.from_tables(np.random.default_rng(0).normal(size=(40, 33)), np.random.default_rng(1).normal(size=(33, 33)))
    with pytest.raises(ValueError, match="ring: num_labels = 33 is above 32"):
        wide.ring(*b["csr"])
    with pytest.raises(ValueError, match="ring: num_labels = 33 is above 32"):
        nat._check(lib.gecco_crf_ring(wide._h, *head[1:], py, ps, None, pl))
    with pytest.raises(ValueError, match="allows a label at or above num_labels"):
        model.ring(*b["csr"], allowed=np.full(5, 8, dtype=np.uint32))
    with pytest.raises(ValueError, match="allowed holds 2 masks for 5 genes"):
        model.ring(*b["csr"], allowed=[1, 1])


# ---------------------------------------------------------------- 10. SequenceCRF
@pytest.mark.parametrize("L", [2, 5, 17])
def test_sequence_crf_front_ends(nat, L):
    b = make_batch(10400 + L, L, [1, 2, 0, 9, 31, 64, 65, 3])
    w = b["w"].copy()
    w[w == 0] = 0.5
    crf, names, classes = sequence_crf(w, b["trans"])
    cptr, gptr, attr = b["csr"]
    X = [[[names[a] for a in dict.fromkeys(attr[gptr[i]:gptr[i + 1]].tolist())] for i in range(cptr[s], cptr[s + 1])]
         for s in range(len(cptr) - 1)]
    flags = [True, False, True, True, False, True, False, False]
    lin, cir = [s for s, f in enumerate(flags) if not f], [s for s, f in enumerate(flags) if f]
    some = {classes[0]} if L == 2 else {classes[0], classes[-1]}
    allowed = [[some if t % 2 else None for t in range(T)] for T in np.diff(cptr).tolist()]
    for sets in (None, allowed):
        pick = lambda idx: None if sets is None else [sets[s] for s in idx]
        mixed, mixed_marg = crf.predict(X, allowed=sets, circular=flags), crf.predict_marginals(X, allowed=sets, circular=flags)
        chain, chain_marg = crf.predict([X[s] for s in lin], allowed=pick(lin)), crf.predict_marginals([X[s] for s in lin], allowed=pick(lin))
        ring = crf.predict_ring([X[s] for s in cir], allowed=pick(cir))
        for k, s in enumerate(lin):
            assert mixed[s] == chain[k] and mixed_marg[s].tobytes() == chain_marg[k].tobytes()
        for k, s in enumerate(cir):
            assert mixed[s] == ring[k]["labels"] and mixed_marg[s].tobytes() == ring[k]["marginals"].tobytes()
        assert crf.predict(X, allowed=sets, circular=True) == [o["labels"] for o in crf.predict_ring(X, allowed=sets)]
        if sets is not None:
            assert all(a is None or lab in a for o, ss in zip(ring, pick(cir)) for lab, a in zip(o["labels"], ss))
    out = crf.predict_ring(X)
    assert (out[2]["labels"], out[2]["score"], out[2]["log_probability"], out[2]["lognorm"]) == ([], 0.0, 0.0, 0.0)
    assert out[2]["marginals"].shape == (0, L)
    ll = crf.log_likelihood(X, [o["labels"] for o in out], circular=True)
    for s, o in enumerate(out):
        assert abs(o["log_probability"] - ll[s]) <= 1e-12 * max(1.0, abs(o["score"])), (s, o["log_probability"], ll[s])
        assert o["log_probability"] <= 1e-12
    # a mixed call: the chain's number for the linear sequences, the ring's for the others; sets give log Z_A,ring - log Z_ring
    paths = crf.predict(X, circular=flags)
    both = crf.log_likelihood(X, paths, circular=flags)
    chain_ll = crf.log_likelihood([X[s] for s in lin], [paths[s] for s in lin])
    assert both[lin].tobytes() == chain_ll.tobytes() and np.all(np.abs(both[cir] - ll[cir]) <= 1e-12 * np.maximum(1.0, np.abs(ll[cir])))
    free = crf.log_likelihood(X, [[None] * len(x) for x in X], circular=True)
    assert not free.any()
    inside = crf.log_likelihood(X, allowed, circular=True)
    assert np.all(inside <= 1e-12) and inside[3] < 0.0


# ---------------------------------------------------------------- 11. the typed front end
def _rotated(genes, r, name):
    """The contig cut r genes further on: new genes with the proteins' domains, in ring order from the new cut."""
    from gecco_amd import model

    src = model.Source(name)
    out = []
    for i, g in enumerate(genes[r:] + genes[:r]):
        protein = model.Protein(g.protein.id, None, [model.Domain(d.name, d.start, d.end, "Pfam", 1e-20, 1e-12) for d in g.protein.domains])
        out.append(model.Gene(src, 1000 * i + 1, 1000 * i + 900, model.Strand.Coding, protein))
    return out


def test_typed_front_end_joins_a_cluster_across_the_cut(nat, tmp_path):
    import random

    from gecco_amd import tables, typed
    from tests import test_gpu_spans as gs
    from tests.typed_planted import C, SPOTS, W, contig, planted_set

    train_genes, train_rows = planted_set(21, 12, "train", composite=False)
    base = str(tmp_path)
    gs._write_tables(os.path.join(base, "train"), train_genes, train_rows)
    random.seed(42)
    np.random.seed(42)
    crf = typed.TypedClusterCRF(W, 1, c1=C, c2=C)
    crf.fit(gs._load(os.path.join(base, "train")), tables.ClusterTable.load(os.path.join(base, "train", "clusters.tsv")))
    fresh, _ = contig(np.random.default_rng(5), "ring", [("Alpha",), ("Beta",)])
    planted = {g.protein.id for g in fresh[SPOTS[0]:SPOTS[0] + 12]}
    cut = _rotated(fresh, SPOTS[0] + 5, "ring")  # the cut lies inside the first planted cluster
    found = crf.predict_path_clusters(cut, min_run=1, circular=True)
    across = [c for c in found if c.wraps_origin]
    assert len(across) == 1 and len({g.protein.id for g in across[0].genes} & planted) >= 10
    ids = [g.protein.id for g in across[0].genes]
    order = [g.protein.id for g in cut]
    assert ids == [p for p in order[order.index(ids[0]):] + order[:order.index(ids[0])]][:len(ids)], "contig[a:] + contig[:b]"
    assert across[0] is found[-1] and across[0].id == f"ring_cluster_{len(found)}", "numbered by where it starts"
    chain = crf.predict_path_clusters(cut, min_run=1)
    assert not any(hasattr(c, "wraps_origin") for c in chain)
    ends = [c for c in chain if c.genes[0] is cut[0] or c.genes[-1] is cut[-1]]
    assert len(ends) in (0, 2), "a chain sees the cluster across the cut as two fragments, or not at all"
    # every rotation of the contig returns the same gene sets
    rotations = sorted(set(range(0, 150, 7)) | {SPOTS[0], SPOTS[0] + 11, SPOTS[1] + 3})
    genes = [g for r in rotations for g in _rotated(fresh, r, f"rot{r:03d}")]
    found_all = crf.predict_path_clusters(genes, min_run=1, circular=True, marginals=True)
    want = sorted(sorted(g.protein.id for g in c.genes) for c in found)
    for r in rotations:
        mine = [c for c in found_all if c.genes[0].source.id == f"rot{r:03d}"]
        assert sorted(sorted(g.protein.id for g in c.genes) for c in mine) == want, r
        assert all(0.0 <= c.min_p <= c.average_p <= c.max_p <= 1.0 for c in mine)
    assert all(v == 0.0 for v in crf.path_posteriors_["constraint_log_p"])
    log_z = crf.path_posteriors_["log_z"]
    assert max(log_z) - min(log_z) <= 1e-9, "log Z of the ring does not depend on the cut"
    # the command line: --circular all writes the column, and without the flag the table is the one of a call without it
    model_dir, data = os.path.join(base, "model"), os.path.join(base, "data")
    crf.save(model_dir)
    gs._write_tables(data, cut)
    args = ["predict", "--model", model_dir, "-g", os.path.join(data, "genes.tsv"), "-f", os.path.join(data, "features.tsv"),
            "--path-clusters", "1"]
    assert typed.main(args + ["-o", os.path.join(base, "out_ring"), "--circular", "all"]) == 0
    assert typed.main(args + ["-o", os.path.join(base, "out_chain")]) == 0
    rows = [line.rstrip("\n").split("\t") for line in open(os.path.join(base, "out_ring", "path_clusters.tsv"))]
    assert rows[0] == ["sequence_id", "cluster_id", "start", "end", "genes", "type", "wraps"]
    assert [r[-1] for r in rows[1:]] == ["0"] * (len(rows) - 2) + ["1"] and int(rows[-1][2]) > int(rows[-1][3])
    typed.write_path_clusters(os.path.join(base, "chain.tsv"), crf.predict_path_clusters(gs._load(data), min_run=1))
    with open(os.path.join(base, "out_chain", "path_clusters.tsv"), "rb") as fa, open(os.path.join(base, "chain.tsv"), "rb") as fb:
        got = fa.read()
        assert got == fb.read() and got.split(b"\n")[0] == b"sequence_id\tcluster_id\tstart\tend\tgenes\ttype"
