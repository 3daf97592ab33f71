"""GPU: the W = 20 window kernels build a slot's constant r = mu01 * prod exp(delta_a) from the per-attribute factor table and
hand the Viterbi decoder d = sum delta_a.  Marginals of the plain window launch, of the two-launch decode
and of the pipelined launch against the oracle at 1e-12, labels against the oracle's exactly: at tile and phase boundaries
inside contigs, on both sides of the attribute count where a slot goes back to the exponential of its sum, with attribute ids
outside the dictionary, at extreme weights, and on planted Viterbi ties."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W = 20
LENGTHS = [20, 21, 237, 238, 474, 475, 600]  # 237 output slots per phase, 474 per tile: boundaries fall inside contigs
TOL = 1e-12


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    assert _native.device_count() >= 1
    return _native


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]


def _csr(counts, draw):
    gptr = np.zeros(len(counts) + 1, dtype=np.int32)
    np.cumsum(counts, out=gptr[1:])
    attr = np.concatenate([draw(int(k)) for k in counts] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return gptr, attr


def _without_foreign_ids(gptr, attr, A):
    """The same batch as the oracle takes it: ids outside the dictionary carry no weight."""
    keep = (attr >= 0) & (attr < A)
    kept = np.concatenate([[0], np.cumsum(keep)]).astype(np.int32)
    return kept[gptr], attr[keep]


def _contig_ptr(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def _run_all(nat, model, batches, label):
    """[(p_windowed, p_decode, y_decode, p_pipelined, y_pipelined)] per batch; the pipelined calls are chained over the batches
    and flushed."""
    devs = [_dev(g, a) for _, g, a in batches]
    ns = [int(c[-1]) for c, _, _ in batches]
    out = []
    for (cptr, _, _), (d_gp, d_at), n in zip(batches, devs, ns):
        plan = nat.Plan(model, cptr, W, 1, True, device=0)
        pw, pd = (torch.full((n,), 7.0, dtype=torch.float64, device="cuda:0") for _ in range(2))
        yd = torch.full((n,), 5, dtype=torch.int8, device="cuda:0")
        plan.run_windowed(d_gp.data_ptr(), d_at.data_ptr(), pw.data_ptr(), label)
        plan.run_decode(d_gp.data_ptr(), d_at.data_ptr(), pd.data_ptr(), yd.data_ptr(), label)
        torch.cuda.synchronize()
        out.append([pw.cpu().numpy(), pd.cpu().numpy(), yd.cpu().numpy().astype(np.int32)])
    plans = [nat.Plan(model, c, W, 1, True, device=0) for c, _, _ in batches]
    pp = [torch.full((n,), 7.0, dtype=torch.float64, device="cuda:0") for n in ns]
    yp = [torch.full((n,), 5, dtype=torch.int8, device="cuda:0") for n in ns]
    for k, (d_gp, d_at) in enumerate(devs):
        plans[k].run_decode_pipelined(d_gp.data_ptr(), d_at.data_ptr(), pp[k].data_ptr(), plans[k - 1] if k else None,
                                      yp[k - 1].data_ptr() if k else 0, label)
    plans[-1].flush_decode_pipelined(yp[-1].data_ptr())
    torch.cuda.synchronize()
    for k in range(len(batches)):
        out[k] += [pp[k].cpu().numpy(), yp[k].cpu().numpy().astype(np.int32)]
    return out


def _check(nat, w, trans, batches, label, what):
    from oracle import crf_oracle as orc

    A = w.shape[0]
    model = nat.Model.from_tables(w, trans)
    got = _run_all(nat, model, batches, label)
    for k, ((cptr, gptr, attr), (pw, pd, yd, pp, yp)) in enumerate(zip(batches, got)):
        og, oa = _without_foreign_ids(gptr, attr, A)
        exp = orc.windowed_marginals(w, trans, cptr, og, oa, W, 1, label, True)
        ey, _ = orc.viterbi(w, trans, cptr, og, oa)
        assert not np.isnan(exp).any()
        for name, p in (("windowed", pw), ("decode", pd), ("pipelined", pp)):
            assert not np.isnan(p).any(), (what, k, name)
            assert p.min() >= 0.0 and p.max() <= 1.0, (what, k, name)
            err = float(np.abs(p - exp).max())
            print(f"{what} batch {k} label {label} {name}: max |dp| = {err:.3e}")
            assert err <= TOL, (what, k, name, err)
        assert np.array_equal(yd, ey), (what, k, "decode labels")
        assert np.array_equal(yp, ey), (what, k, "pipelined labels")


# ---- attribute counts on both sides of the product's limit, tile and phase boundaries, foreign ids ------------------------
TRANS = {"mild": np.array([[0.6, -0.9], [-1.1, 0.8]]), "sticky": np.array([[2.67, -2.6], [-2.6, 2.57]])}


def _moderate_model(trans_kind):
    rng = np.random.default_rng(11)
    A = 200
    w = rng.normal(0.0, 1.2, size=(A, 2))
    w[0] = (0.5, 24.5)  # delta = 24 exactly, far above every other |delta|: dmax = 24, 29 attributes at most in a product
    return w, TRANS[trans_kind]


def _product_limit(trans, label, dmax, pmc):
    """The attribute count up to which a slot's constant is the running product: the table's prod_max_cnt, lowered where
    |ln mu01| -- the product's first factor -- takes its share of the e^700 the partial products may span."""
    o = 1 - label
    lmu = trans[o, label] + trans[label, o] - 2.0 * trans[o, o]
    return min(pmc, int(math.floor((700.0 - abs(lmu)) / dmax)))


def _moderate_batch(seed, A, limit, lengths=LENGTHS):
    rng = np.random.default_rng(seed)
    lengths = list(lengths)
    rng.shuffle(lengths)
    n = int(sum(lengths))
    kinds = np.array([0, 1, 8, 9, limit, limit + 1, limit + 40])
    counts = kinds[rng.integers(0, len(kinds), size=n)]
    counts[:7] = kinds  # every count at least once
    foreign = np.array([A, A + 7, 2 ** 31 - 1, -1, -5], dtype=np.int64)

    def draw(k):
        ids = rng.integers(0, A, size=k).astype(np.int64)
        bad = rng.random(k) < 0.05
        ids[bad] = foreign[rng.integers(0, len(foreign), size=int(bad.sum()))]
        return ids

    gptr, attr = _csr(counts, draw)
    return _contig_ptr(lengths), gptr, attr


@pytest.mark.parametrize("label", [1, 0])
@pytest.mark.parametrize("trans_kind", ["mild", "sticky"])
def test_counts_around_the_product_limit(nat, trans_kind, label):
    w, trans = _moderate_model(trans_kind)
    A = w.shape[0]
    _, dmax, pmc = nat.Model.from_tables(w, trans).slot_table(label)
    assert dmax == 24.0 and pmc == 29
    limit = _product_limit(trans, label, dmax, pmc)
    assert limit == (29 if trans_kind == "mild" else 28)  # (sticky transitions: ln mu01 = -10.5, as the benchmark's model)
    batches = [_moderate_batch(100, A, limit), _moderate_batch(101, A, limit)]
    assert any((a >= A).any() and (a < 0).any() for _, _, a in batches)
    _check(nat, w, trans, batches, label, f"counts/{trans_kind}")


def test_padded_contigs_take_the_same_constants(nat):
    """Contigs shorter than the window are padded: their tiles look every slot up and gather per slot.  Same counts on both
    sides of the limit, same tolerance; and a gene's probability does not depend on which kind of tile held it: the long
    contigs of the batch alone give the same bits."""
    w, trans = _moderate_model("sticky")
    A = w.shape[0]
    limit = _product_limit(trans, 1, 24.0, 29)
    lengths = [5, 19, 238, 20, 3, 237, 1, 475]
    batch = _moderate_batch(102, A, limit, lengths)
    _check(nat, w, trans, [batch, _moderate_batch(103, A, limit, lengths)], 1, "padded")
    # the 475-gene contig on its own (a regular batch) against the same genes inside the padded batch
    cptr, gptr, attr = batch
    g0, g1 = int(cptr[-2]), int(cptr[-1])
    lone = (np.array([0, g1 - g0], dtype=np.int32), (gptr[g0:g1 + 1] - gptr[g0]).astype(np.int32), attr[gptr[g0]:gptr[g1]])
    model = nat.Model.from_tables(w, trans)
    both = []
    for c, g, a in (batch, lone):
        d_gp, d_at = _dev(g, a)
        p = torch.zeros(int(c[-1]), dtype=torch.float64, device="cuda:0")
        nat.Plan(model, c, W, 1, True, device=0).run_windowed(d_gp.data_ptr(), d_at.data_ptr(), p.data_ptr(), 1)
        torch.cuda.synchronize()
        both.append(p.cpu().numpy())
    assert np.array_equal(both[0][g0:g1], both[1])


# ---- extreme weights --------------------------------------------------------------------------------------------------
def _planted_batch(seed, A_small, planted):
    """Contigs of 237, 238 and 475 genes with 0 to 2 ordinary attributes (ids 4 .. A - 1) per gene and the planted attribute
    lists every 13 genes."""
    rng = np.random.default_rng(seed)
    lengths = [237, 238, 475]
    n = sum(lengths)
    lists = [list(rng.integers(4, A_small, size=int(rng.integers(0, 3)))) for _ in range(n)]
    for i, g in enumerate(range(5, n, 13)):
        lists[g] = list(planted[i % len(planted)])
    counts = np.array([len(x) for x in lists])
    it = iter(lists)
    gptr, attr = _csr(counts, lambda k: np.array(next(it), dtype=np.int64))
    return _contig_ptr(lengths), gptr, attr


@pytest.mark.parametrize("label", [1, 0])
def test_fallback_and_cancelling_sums(nat, label):
    """|delta| up to 300: two attributes is the most a product may take (floor(700 / 300)); genes with two and three attributes
    of +-300 sit on both sides of that, and +300 next to -300 must cancel in the product as it does in the sum."""
    rng = np.random.default_rng(5)
    A = 16
    w = rng.normal(0.0, 1.0, size=(A, 2))
    # delta = +300, -300, +150, -150 (label 1), split over the two labels so that every state score stays where the oracle is finite
    w[0], w[1], w[2], w[3] = (-150.0, 150.0), (150.0, -150.0), (-75.0, 75.0), (100.0, -50.0)
    trans = np.array([[0.4, -0.7], [-0.5, 0.9]])
    _, dmax, pmc = nat.Model.from_tables(w, trans).slot_table(label)
    assert dmax == 300.0 and pmc == 2
    planted = [[0, 0], [0, 0, 0], [1, 1], [1, 1, 1], [0, 1], [1, 0], [0, 1, 5], [1, 6, 0], [2, 2, 2, 2], [3, 3, 0], [0], [1],
               [2, 3], [0, 0, 1, 1]]
    batches = [_planted_batch(31, A, planted), _planted_batch(32, A, planted[::-1])]
    _check(nat, w, trans, batches, label, "fallback")


@pytest.mark.parametrize("label", [1, 0])
def test_zero_threshold(nat, label):
    """dmax >= 700: no attribute may enter a product, every slot with an attribute takes the exponential of its sum."""
    rng = np.random.default_rng(6)
    A = 16
    w = rng.normal(0.0, 1.0, size=(A, 2))
    w[0], w[1] = (-355.0, 355.0), (355.0, -355.0)  # delta = +710, -710 (label 1); split likewise
    trans = np.array([[0.4, -0.7], [-0.5, 0.9]])
    _, dmax, pmc = nat.Model.from_tables(w, trans).slot_table(label)
    assert dmax == 710.0 and pmc == 0
    planted = [[0], [1], [0, 1], [1, 0], [0, 5], [1, 6, 7], [0, 1, 0], [5, 1, 0, 1]]
    batches = [_planted_batch(41, A, planted), _planted_batch(42, A, planted[::-1])]
    _check(nat, w, trans, batches, label, "zero threshold")


# ---- Viterbi ties under the widened margin ---------------------------------------------------------------------------------
def _labels_and_stats(nat, w, trans, cptr, gptr, attr):
    model = nat.Model.from_tables(w, trans)
    n = int(cptr[-1])
    d_gp, d_at = _dev(gptr, attr)
    plan = nat.Plan(model, cptr, W, 1, True, device=0)
    p = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    y = torch.full((n,), 5, dtype=torch.int8, device="cuda:0")
    plan.viterbi_stats(reset=True)
    plan.run_decode(d_gp.data_ptr(), d_at.data_ptr(), p.data_ptr(), y.data_ptr())
    stats = plan.viterbi_stats(reset=True)
    # the pipelined launch: the plan follows itself, the second call decodes what the first scored
    y2 = torch.full((n,), 5, dtype=torch.int8, device="cuda:0")
    plan.run_decode_pipelined(d_gp.data_ptr(), d_at.data_ptr(), p.data_ptr(), None, 0)
    plan.run_decode_pipelined(d_gp.data_ptr(), d_at.data_ptr(), p.data_ptr(), plan, y2.data_ptr())
    plan.flush_decode_pipelined(y.data_ptr())
    torch.cuda.synchronize()
    stats2 = plan.viterbi_stats(reset=True)
    assert torch.equal(y, y2)
    return y2.cpu().numpy().astype(np.int32), stats, stats2


def _has_exact_tie(state, trans):
    """CRFsuite's recursion on one contig's state scores: does some decision compare two equal candidates?"""
    d = state[0].copy()
    for t in range(1, len(state)):
        c = d[:, None] + trans
        if c[0, 0] == c[1, 0] or c[0, 1] == c[1, 1]:
            return True
        d = c.max(axis=0) + state[t]
    return bool(d[0] == d[1])


def test_integer_weight_ties(nat):
    from oracle import crf_oracle as orc

    rng = np.random.default_rng(99)
    A = 30
    w = rng.integers(-2, 3, size=(A, 2)).astype(np.float64)
    trans = np.array([[1.0, -1.0], [-1.0, 1.0]])
    cptr = _contig_ptr([200])
    counts = rng.integers(0, 4, size=200)
    gptr, attr = _csr(counts, lambda k: rng.integers(0, A, size=k))
    state = np.array([w[attr[gptr[g]:gptr[g + 1]]].sum(axis=0) for g in range(200)])
    assert _has_exact_tie(state, trans)
    y, stats, stats2 = _labels_and_stats(nat, w, trans, cptr, gptr, attr)
    ey, _ = orc.viterbi(w, trans, cptr, gptr, attr)
    assert np.array_equal(y, ey)
    print("integer ties:", stats, stats2)
    assert stats["contigs_redecoded"] == 1 and stats2["contigs_redecoded"] >= 1


def _plant_weights(rng, target):
    """Three weight pairs whose two CSR-order sums give fl(s1 - s0) == target while the sum of the three rounded differences
    gives another number."""
    for _ in range(20000):
        v = rng.normal(0.0, 1.5, size=(3, 2))
        s0 = (v[0, 0] + v[1, 0]) + v[2, 0]
        base = v[0, 1] + v[1, 1]
        x = (target + s0) - base
        for _ in range(8):
            s1 = base + x
            if s1 - s0 == target:
                break
            x = np.nextafter(x, math.inf if s1 - s0 < target else -math.inf)
        else:
            continue
        v[2, 1] = x
        d = ((v[0, 1] - v[0, 0]) + (v[1, 1] - v[1, 0])) + (v[2, 1] - v[2, 0])
        if d != target:
            return v, d
    raise AssertionError("no planted triple found")


def test_planted_decision_one_ulp_from_its_threshold(nat):
    """The first gene of six 200-gene contigs carries three attributes of its own whose score difference, as CRFsuite sums it,
    lies on a threshold of the second gene's decision or one ulp to either side, while the sum of the rounded differences --
    what the window tiles hand over -- is another number (checked here first).  The margin must catch all six."""
    from oracle import crf_oracle as orc

    rng = np.random.default_rng(2718)
    A = 60
    w = rng.normal(0.0, 1.5, size=(A, 2))
    trans = np.array([[0.731, -0.412], [-0.958, 0.377]])
    hi, lo = trans[0, 0] - trans[1, 0], trans[0, 1] - trans[1, 1]  # thresholds of the decisions for label 0 / label 1
    targets = [np.nextafter(hi, -math.inf), hi, np.nextafter(hi, math.inf), np.nextafter(lo, -math.inf), lo, np.nextafter(lo, math.inf)]
    lists = []
    for c, target in enumerate(targets):
        v, d = _plant_weights(rng, target)
        ids = [3 * c, 3 * c + 1, 3 * c + 2]
        w[ids] = v
        s = np.zeros(2)
        for a in ids:  # CSR order, as CRFsuite and the tiles add
            s = s + w[a]
        assert s[1] - s[0] == target and d != target, c
        lists += [ids] + [list(rng.integers(18, A, size=int(rng.integers(0, 3)))) for _ in range(199)]
    cptr = _contig_ptr([200] * 6)
    it = iter(lists)
    gptr, attr = _csr(np.array([len(x) for x in lists]), lambda k: np.array(next(it), dtype=np.int64))
    y, stats, stats2 = _labels_and_stats(nat, w, trans, cptr, gptr, attr)
    ey, _ = orc.viterbi(w, trans, cptr, gptr, attr)
    assert np.array_equal(y, ey)
    print("planted decisions:", stats, stats2)
    assert stats["contigs_redecoded"] >= 6 and stats2["contigs_redecoded"] >= 6
