"""Inference with real-valued attributes on the device: ``gecco_crf_viterbi_valued``, ``gecco_crf_marginals_full_valued``,
``gecco_crf_windowed_marginals_valued`` and ``gecco_crf_windowed_marginals_all_valued`` against the independent numpy
yardstick (tests/train_objective_valued.py): exact sets on which every tie is a true tie, near-ties planted inside the
Viterbi margin of the *valued* bound, the all-ones identity with the unvalued entries, batch independence, unknown ids,
padding, refusals, and ``SequenceCRF`` on dict items end to end."""
import ctypes

import numpy as np
import pytest

from tests import train_objective_valued as tv
from tests.helpers import _delta_step, _solve_sum

pytestmark = pytest.mark.gpu

LABELS = [2, 3, 8, 17, 32]
A = 30


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


def _csr(rng, lengths, max_attrs=4, n_attrs=A):
    cptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    deg = rng.integers(0, max_attrs + 1, size=int(cptr[-1]))
    gptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    attr = rng.integers(0, n_attrs, size=int(gptr[-1])).astype(np.int32)
    return cptr, gptr, attr


def _lengths(rng):
    """About 40 contigs of 1 to 60 items, and one of 300 (several chunks of the whole-contig kernels)."""
    return [1, 2, 3] + [int(x) for x in rng.integers(1, 61, size=37)] + [300]


def _moderate_values(rng, n):
    """N(0, 1), exact 0, exact 1 and powers of two in 2^-3 .. 2^3: state scores stay of the order the unvalued entries'
    bounds were set for (values of 2^10 are the exact sets' and the margin set's)."""
    v = rng.normal(0.0, 1.0, size=n)
    kind = rng.integers(0, 6, size=n)
    v[kind == 3] = 0.0
    v[kind == 4] = 1.0
    v[kind == 5] = 2.0 ** rng.integers(-3, 4, size=int((kind == 5).sum()))
    return v


@pytest.fixture(scope="module")
def batches():
    """Per label count: the model tables, the batch, its values, and the yardstick's results, computed once."""
    out = {}
    for L in LABELS:
        rng = np.random.default_rng(1200 + L)
        w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
        cptr, gptr, attr = _csr(rng, _lengths(rng))
        v = _moderate_values(rng, len(attr))
        marg, logz = tv.marginals_sequences(cptr, gptr, attr, v, w, trans)
        y, score = tv.viterbi(cptr, gptr, attr, v, w, trans)
        out[L] = dict(w=w, trans=trans, cptr=cptr, gptr=gptr, attr=attr, v=v, marg=marg, logz=logz, y=y, score=score)
    return out


# ---------------------------------------------------------------- against the yardstick
@pytest.mark.parametrize("L", LABELS)
def test_whole_contig_entries_against_the_yardstick(nat, batches, L):
    b = batches[L]
    model = nat.Model.from_tables(b["w"], b["trans"])
    marg, logz = model.marginals_full(b["cptr"], b["gptr"], b["attr"], values=b["v"])
    print(f"L={L}: max |marg - ref| = {np.abs(marg - b['marg']).max():.3g}, "
          f"max |ln Z - ref| / max(1, |ref|) = {(np.abs(logz - b['logz']) / np.maximum(1, np.abs(b['logz']))).max():.3g}")
    assert np.abs(marg - b["marg"]).max() <= 1e-12
    assert np.all(np.abs(logz - b["logz"]) <= 1e-10 * np.maximum(1.0, np.abs(b["logz"])))
    y, score = model.viterbi(b["cptr"], b["gptr"], b["attr"], values=b["v"])
    assert np.all(np.abs(score - b["score"]) <= 1e-9 * np.maximum(1.0, np.abs(b["score"])))
    st = tv.item_scores(b["gptr"], b["attr"], b["v"], b["w"])
    for c in range(len(b["cptr"]) - 1):
        g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
        mine = tv.path_score(st[g0:g1], b["trans"], y[g0:g1].astype(int))
        assert abs(mine - b["score"][c]) <= 1e-9 * max(1.0, abs(b["score"][c])), c
    y2, none = model.viterbi(b["cptr"], b["gptr"], b["attr"], values=b["v"], want_score=False)
    assert none is None and np.array_equal(y, y2)


@pytest.mark.parametrize("W,step,pad", [(5, 1, True), (20, 3, True), (20, 1, False)])
@pytest.mark.parametrize("L", LABELS)
def test_windowed_entries_against_the_yardstick(nat, batches, L, W, step, pad):
    """Columns, p_any and the single-label entry; short contigs padded (pad) or NaN in every column (not pad); at step 3 the
    genes no window covers hold 0.0."""
    b = batches[L]
    model = nat.Model.from_tables(b["w"], b["trans"])
    bg = L - 1
    exp_all, exp_any = tv.windowed(b["cptr"], b["gptr"], b["attr"], b["v"], b["w"], b["trans"], W, step, background=bg, pad=pad)
    p_all, p_any = model.windowed_marginals_all(b["cptr"], b["gptr"], b["attr"], W, step, background=bg, pad=pad, values=b["v"])
    short = np.repeat(np.diff(b["cptr"]) < W, np.diff(b["cptr"]))
    assert short.any() and not short.all()
    if pad:
        assert np.all(np.isfinite(p_all)) and np.all(np.isfinite(exp_all))
    else:
        assert np.all(np.isnan(p_all[short])) and np.all(np.isnan(p_any[short])) and np.all(np.isfinite(p_all[~short]))
    if step == 3:
        assert np.any(exp_all.sum(axis=1) == 0.0)
    same_nan = np.array_equal(np.isnan(p_all), np.isnan(exp_all)) and np.array_equal(np.isnan(p_any), np.isnan(exp_any))
    assert same_nan and np.array_equal(p_all == 0.0, exp_all == 0.0)
    ok = ~np.isnan(exp_any)
    print(f"L={L} W={W}: max |p_all - ref| = {np.abs(p_all[ok] - exp_all[ok]).max():.3g}, "
          f"max |p_any - ref| = {np.abs(p_any[ok] - exp_any[ok]).max():.3g}")
    assert np.abs(p_all[ok] - exp_all[ok]).max() <= 2e-12 and np.abs(p_any[ok] - exp_any[ok]).max() <= 2e-12
    for label in (0, L - 1):
        p = model.windowed_marginals(b["cptr"], b["gptr"], b["attr"], W, step, label=label, pad=pad, values=b["v"])
        assert np.array_equal(np.isnan(p), np.isnan(exp_all[:, label]))
        assert np.abs(p[ok] - exp_all[ok, label]).max() <= 2e-12


# ---------------------------------------------------------------- exact sets: every tie is a true tie
@pytest.mark.parametrize("L", LABELS)
def test_exact_sets_give_the_first_arg_max_path(nat, L):
    """Values 2^-3 .. 2^10, weights and transitions multiples of 1/8 up to 4: every product and sum is exact, so the
    device, whatever its multiply-add form and order, sees the yardstick's numbers, ties included."""
    rng = np.random.default_rng(3300 + L)
    w = rng.integers(-32, 33, size=(A, L)) / 8.0
    trans = rng.integers(-32, 33, size=(L, L)) / 8.0
    w[:, 1] = w[:, 0]  # labels 0 and 1 tie wherever the transitions let them
    trans[:, 1], trans[1, :] = trans[:, 0], trans[0, :]
    trans[1, 1] = trans[0, 0]
    cptr, gptr, attr = _csr(rng, _lengths(rng))
    v = 2.0 ** rng.integers(-3, 11, size=len(attr))
    ey, escore = tv.viterbi(cptr, gptr, attr, v, w, trans)
    assert not np.any(ey == 1)  # (the first arg max never picks the twin)
    model = nat.Model.from_tables(w, trans)
    y, score = model.viterbi(cptr, gptr, attr, values=v)
    assert np.array_equal(y.astype(np.int64), ey)
    assert np.array_equal(score, escore)


# ---------------------------------------------------------------- near-ties inside the margin of the valued bound
GAPS = (1, -2, 4, -8, 16, -32, 64, -1, 2, -4, 8, -16, 32, -64)


def _margin_batch(rng, L, lengths, trans):
    """Contigs whose gene g carries attribute g alone with a value v_g that is a power of two and the weight row
    u_g = s_g / v_g (exact), so that the state score v_g u_g is s_g whatever the multiply-add form.  Near-ties of
    CRFsuite's recursion are planted as tests/helpers.py plants them (a candidate pair for label j solved to a gap, the
    next gene deciding for j), but with gaps of k ulp(M), k in +-1 .. +-64, where M = nnz max|v| max|u| + (n + 2) max|trans|
    is the bound the chunked Viterbi's margin uses with values.  Most genes carry 2^10, so the scores the recursion sums
    are near that bound, and max|u| stays small: a margin built from max|u| alone is a thousand times too narrow.
    Decisions sit at the first genes of the 32-gene chunks and at the contig's end."""
    n = sum(lengths)
    cptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    v = np.full(n, 1024.0)
    small = rng.random(n) < 0.15
    v[small] = 2.0 ** rng.integers(-3, 10, size=int(small.sum()))
    big = 12.0
    # (a first pass fixes max|u|: every row is drawn within +-big, so max|u| <= big and M can be stated before planting)
    pairs = [(0, 1)] if L == 2 else [(0, 1), (0, L - 1), (L // 2 - 1, L // 2), (1, L - 1)]
    s = np.zeros((n, L))
    planted = []
    cnt = 0
    tmax = float(np.abs(trans).max())
    for c, T in enumerate(lengths):
        start = int(cptr[c])
        M = T * 1024.0 * big + (T + 2) * tmax
        ulpM = float(np.spacing(M))
        plan = {t - 1: None for t in range(32, T - 2, 32)}
        d = np.zeros(L)
        for t in range(T):
            g = start + t
            m = _delta_step(d, trans)[0] if t else np.zeros(L)
            if t in plan or t == T - 1:
                v[g] = 1024.0
                i1, i2 = pairs[cnt % len(pairs)]
                j = -1 if t == T - 1 else (i1, i2, L - 1)[cnt % 3]
                k = GAPS[cnt % len(GAPS)]
                cnt += 1
                b1, b2 = (0.0, 0.0) if j < 0 else (trans[i1, j], trans[i2, j])
                for attempt in range(400):
                    row = 1024.0 * rng.normal(0.0, 1.0, size=L)
                    row[[x for x in range(L) if x not in (i1, i2)]] = -1024.0 * big
                    d1 = (m[i1] + row[i1]) if t else row[i1]
                    target = (d1 + b1) + k * ulpM
                    s2 = _solve_sum(m[i2] if t else 0.0, b2, target)
                    if s2 is None or abs(s2) >= 1024.0 * big:
                        continue
                    row[i2] = s2
                    dd = (m + row) if t else row.copy()
                    cand = dd + (0.0 if j < 0 else trans[:, j])
                    if cand[i2] - cand[i1] == k * ulpM:
                        break
                else:
                    raise AssertionError("could not plant a near-tie")
                s[g] = row
                plan[t] = j
                planted.append((c, t, k))
            elif t - 1 in plan and plan[t - 1] is not None and plan[t - 1] >= 0:  # the decision gene: label j by a wide margin
                v[g] = 1024.0
                s[g] = -1024.0 * big
                s[g, plan[t - 1]] = 1024.0 * big
            else:
                s[g] = v[g] * rng.normal(0.0, 1.0, size=L)
            d = (m + s[g]) if t else s[g].copy()
    u = s / v[:, None]
    assert np.array_equal(u * v[:, None], s) and np.abs(u).max() <= big
    return u, cptr, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), v, planted


@pytest.mark.parametrize("L", LABELS)
def test_planted_near_ties_inside_the_valued_margin(nat, L):
    rng = np.random.default_rng(4400 + L)
    trans = rng.normal(0.0, 1.5, size=(L, L)) / 64.0  # (small beside the state scores: the state term is the bound)
    lengths = [65, 66, 97, 128, 129, 200, 257, 300]
    u, cptr, gptr, attr, v, planted = _margin_batch(rng, L, lengths, trans)
    assert len(planted) >= 30 and {abs(k) for _, _, k in planted} == {1, 2, 4, 8, 16, 32, 64}
    ey, escore = tv.viterbi(cptr, gptr, attr, v, u, trans)
    model = nat.Model.from_tables(u, trans)
    y, score = model.viterbi(cptr, gptr, attr, values=v)
    wrong = np.flatnonzero(y.astype(np.int64) != ey)
    print(f"L={L}: {len(planted)} planted near-ties, {len(wrong)} labels differ from the sequential recursion")
    assert len(wrong) == 0, wrong[:10]
    assert np.all(np.abs(score - escore) <= 1e-9 * np.maximum(1.0, np.abs(escore)))


# ---------------------------------------------------------------- all values 1.0
@pytest.mark.parametrize("L", LABELS)
def test_all_ones_are_the_unvalued_entries(nat, batches, L):
    """At three or more labels the valued call runs the kernels the unvalued one runs: the same bytes.  At two labels the
    unvalued entries have kernels of their own: agreement to the entries' bounds."""
    b = batches[L]
    model = nat.Model.from_tables(b["w"], b["trans"])
    ones = np.ones(len(b["attr"]))
    csr = (b["cptr"], b["gptr"], b["attr"])
    pairs = [
        (model.marginals_full(*csr), model.marginals_full(*csr, values=ones), (1e-12, 1e-10)),
        (model.viterbi(*csr), model.viterbi(*csr, values=ones), (0, 1e-9)),
        (model.windowed_marginals_all(*csr, 5, 1, background=0), model.windowed_marginals_all(*csr, 5, 1, background=0, values=ones),
         (2e-12, 2e-12)),
        ((model.windowed_marginals(*csr, 20, 3, label=L - 1, pad=False),),
         (model.windowed_marginals(*csr, 20, 3, label=L - 1, pad=False, values=ones),), (2e-12,)),
    ]
    for plain, valued, tols in pairs:
        for p, q, tol in zip(plain, valued, tols):
            if L >= 3:
                assert p.tobytes() == q.tobytes()
            else:
                assert np.array_equal(np.isnan(p), np.isnan(q))
                ok = ~np.isnan(np.asarray(p, dtype=np.float64))
                scale = np.maximum(1.0, np.abs(p[ok])) if tol in (1e-10, 1e-9) else 1.0
                assert np.all(np.abs(p[ok].astype(np.float64) - q[ok]) <= tol * scale)


# ---------------------------------------------------------------- other inference checks
@pytest.mark.parametrize("L", [2, 8, 32])
def test_a_contig_alone_gives_the_batch_bytes(nat, batches, L):
    b = batches[L]
    model = nat.Model.from_tables(b["w"], b["trans"])
    csr = (b["cptr"], b["gptr"], b["attr"])
    marg, logz = model.marginals_full(*csr, values=b["v"])
    y, score = model.viterbi(*csr, values=b["v"])
    p_all, p_any = model.windowed_marginals_all(*csr, 5, 1, background=0, values=b["v"])
    p = model.windowed_marginals(*csr, 5, 1, label=1, values=b["v"])
    n_contigs = len(b["cptr"]) - 1
    for c in (0, 7, n_contigs - 1):  # (the last one is the 300-item contig)
        g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
        a0, a1 = int(b["gptr"][g0]), int(b["gptr"][g1])
        one = (np.array([0, g1 - g0], dtype=np.int32), (b["gptr"][g0:g1 + 1] - a0).astype(np.int32), b["attr"][a0:a1])
        vals = b["v"][a0:a1]
        m1, z1 = model.marginals_full(*one, values=vals)
        y1, s1 = model.viterbi(*one, values=vals)
        pa1, pn1 = model.windowed_marginals_all(*one, 5, 1, background=0, values=vals)
        p1 = model.windowed_marginals(*one, 5, 1, label=1, values=vals)
        assert m1.tobytes() == marg[g0:g1].tobytes() and z1.tobytes() == logz[c:c + 1].tobytes()
        assert y1.tobytes() == y[g0:g1].tobytes() and s1.tobytes() == score[c:c + 1].tobytes()
        assert pa1.tobytes() == p_all[g0:g1].tobytes() and pn1.tobytes() == p_any[g0:g1].tobytes()
        assert p1.tobytes() == p[g0:g1].tobytes()


@pytest.mark.parametrize("L", [2, 5])
def test_unknown_attribute_ids_carry_no_weight(nat, L):
    rng = np.random.default_rng(90 + L)
    w, trans = rng.normal(size=(A, L)), rng.normal(size=(L, L))
    cptr, gptr, attr = _csr(rng, [4, 30, 1, 12])
    v = _moderate_values(rng, len(attr))
    # the same items with an unknown id in front of, inside and behind every item's list, each with a large value
    attr2, v2, gptr2 = [], [], [0]
    for g in range(len(gptr) - 1):
        ids, vals = attr[gptr[g]:gptr[g + 1]].tolist(), v[gptr[g]:gptr[g + 1]].tolist()
        attr2 += [-1] + ids[:1] + [A] + ids[1:] + [A + 1000]
        v2 += [1e300] + vals[:1] + [-7.5] + vals[1:] + [2.0 ** 10]
        gptr2.append(len(attr2))
    model = nat.Model.from_tables(w, trans)
    base, more = (cptr, gptr, attr), (cptr, np.array(gptr2, dtype=np.int32), np.array(attr2, dtype=np.int32))
    v2 = np.array(v2)
    for a, b in zip(model.marginals_full(*base, values=v) + model.viterbi(*base, values=v)
                    + model.windowed_marginals_all(*base, 5, 2, background=1, values=v),
                    model.marginals_full(*more, values=v2) + model.viterbi(*more, values=v2)
                    + model.windowed_marginals_all(*more, 5, 2, background=1, values=v2)):
        assert a.tobytes() == b.tobytes()


def test_refusals(nat):
    rng = np.random.default_rng(8)
    L = 2
    model = nat.Model.from_tables(rng.normal(size=(A, L)), rng.normal(size=(L, L)))
    cptr, gptr, attr = _csr(rng, [60, 5])
    v = np.ones(len(attr))
    lib = nat.load_library()
    for bad in (float("nan"), float("inf")):
        vb = v.copy()
        vb[3] = bad
        for call in (lambda: model.viterbi(cptr, gptr, attr, values=vb), lambda: model.marginals_full(cptr, gptr, attr, values=vb),
                     lambda: model.windowed_marginals(cptr, gptr, attr, 5, values=vb),
                     lambda: model.windowed_marginals_all(cptr, gptr, attr, 5, values=vb)):
            with pytest.raises(ValueError, match="attribute value 3 is not finite"):
                call()
            assert lib.gecco_crf_last_error().decode() == "attribute value 3 is not finite (NaN or infinite)"
    # NULL values with attribute entries, past the Python layer
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    y = np.zeros(int(cptr[-1]), dtype=np.int8)
    rc = lib.gecco_crf_viterbi_valued(model._h, 0, cptr.ctypes.data_as(i32p), 2, gptr.ctypes.data_as(i32p), attr.ctypes.data_as(i32p),
                                      None, y.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), None)
    assert rc == nat.EINVAL and "null attr_value" in lib.gecco_crf_last_error().decode()
    p = np.zeros(int(cptr[-1]))
    rc = lib.gecco_crf_windowed_marginals_valued(model._h, 0, cptr.ctypes.data_as(i32p), 2, gptr.ctypes.data_as(i32p),
                                                 attr.ctypes.data_as(i32p), None, 5, 1, 1, 1, p.ctypes.data_as(f64p))
    assert rc == nat.EINVAL and "null attr_value" in lib.gecco_crf_last_error().decode()
    with pytest.raises(ValueError, match="values holds"):
        model.viterbi(cptr, gptr, attr, values=v[:-1])
    # two labels: the valued single-label entry has the any-L kernel's window limit, the unvalued one its own kernels
    assert np.all(np.isfinite(model.windowed_marginals(cptr, gptr, attr, 48, values=v)))
    assert np.all(np.isfinite(model.windowed_marginals(cptr, gptr, attr, 49)))
    with pytest.raises(nat.NativeError, match="window too long") as e:
        model.windowed_marginals(cptr, gptr, attr, 49, values=v)
    assert e.value.code == nat.EUNSUPPORTED


# ---------------------------------------------------------------- the estimator end to end
def _dict_data(rng, n_seqs, lo=6, hi=20):
    X, y = [], []
    for _ in range(n_seqs):
        n = int(rng.integers(lo, hi + 1))
        labs = [str(rng.choice(["a", "b", "c"])) for _ in range(n)]
        X.append([{"bias": 1.0, "kind": "c" if lab == "c" else "ab", "tags": ["x", lab] if rng.random() < 0.3 else ["x"],
                   "score": {"a": 1.0, "b": -1.0, "c": 0.0}[lab] + float(rng.normal(0, 0.4))} for lab in labs])
        y.append(labs)
    return X, y


def test_sequence_crf_on_dict_items_end_to_end(nat):
    from gecco_amd import train
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(21)
    X, y = _dict_data(rng, 25)
    crf = SequenceCRF(window_size=5, c1=0.05, c2=0.1, max_iterations=30).fit(X, y)
    assert crf.training_result_.n_iter > 0 and "score" in crf.attributes_ and "tags:x" in crf.attributes_
    Xt, _ = _dict_data(np.random.default_rng(22), 8, lo=1)
    Xt[0][0] = dict(Xt[0][0], unseen=3.5, other="never")  # names the model does not know are dropped with their values
    Xt.insert(2, [])
    index = {a: i for i, a in enumerate(crf.attributes_)}
    cptr, gptr, attr, vals = [0], [0], [], []
    for xs in Xt:
        for item in xs:
            for name, value in zip(*train.item_attributes(item)):
                if name in index:
                    attr.append(index[name])
                    vals.append(value)
            gptr.append(len(attr))
        cptr.append(len(gptr) - 1)
    cptr, gptr, attr = (np.array(a, dtype=np.int32) for a in (cptr, gptr, attr))
    vals = np.array(vals)
    assert len(attr) < sum(len(train.item_attributes(it)[0]) for xs in Xt for it in xs)
    model = nat.Model.from_lcrf(crf.to_bytes())
    ey, _ = model.viterbi(cptr, gptr, attr, values=vals)
    emarg, _ = model.marginals_full(cptr, gptr, attr, values=vals)
    ep = model.windowed_marginals(cptr, gptr, attr, 5, 1, label=crf.classes_.index("b"), values=vals)
    eall, eany = model.windowed_marginals_all(cptr, gptr, attr, 5, 1, background=crf.classes_.index("c"), values=vals)
    assert [lab for ys in crf.predict(Xt) for lab in ys] == [crf.classes_[k] for k in ey.tolist()]
    assert [len(ys) for ys in crf.predict(Xt)] == [len(xs) for xs in Xt]
    assert np.concatenate(crf.predict_marginals(Xt)).tobytes() == emarg.tobytes()
    assert np.concatenate(crf.predict_windowed(Xt, "b")).tobytes() == ep.tobytes()
    p_all, p_any = crf.predict_windowed_all(Xt, background="c")
    assert np.concatenate(p_all).tobytes() == eall.tobytes() and np.concatenate(p_any).tobytes() == eany.tobytes()
    # a model fitted on plain names gives, on plain names, what the unvalued entries give
    names = lambda data: [[["bias", "kind:" + it["kind"]] + ["tags:" + t for t in it["tags"]] for it in xs] for xs in data]
    plain = SequenceCRF(window_size=5, c1=0.05, c2=0.1, max_iterations=30).fit(names(X), y)
    Xn = names([xs for xs in Xt if xs])
    idx = {a: i for i, a in enumerate(plain.attributes_)}
    cptr, gptr, attr = [0], [0], []
    for xs in Xn:
        for item in xs:
            attr.extend(idx[nm] for nm in dict.fromkeys(item) if nm in idx)
            gptr.append(len(attr))
        cptr.append(len(gptr) - 1)
    cptr, gptr, attr = (np.array(a, dtype=np.int32) for a in (cptr, gptr, attr))
    pm = nat.Model.from_lcrf(plain.to_bytes())
    assert [lab for ys in plain.predict(Xn) for lab in ys] == [plain.classes_[k] for k in pm.viterbi(cptr, gptr, attr)[0].tolist()]
    assert np.concatenate(plain.predict_marginals(Xn)).tobytes() == pm.marginals_full(cptr, gptr, attr)[0].tobytes()
    assert np.concatenate(plain.predict_windowed(Xn, "a")).tobytes() == \
        pm.windowed_marginals(cptr, gptr, attr, 5, 1, label=plain.classes_.index("a")).tobytes()
