"""Every lattice query across the transition range the guard accepts: the entries behind ``run_lattice`` on the
planted families of tests/lattice_range_families.py -- the six uniform shifts of family a, the guard's own figures of family g
(max trans at exactly +700 and -700), family b's far entry at 74.9, 151 and 2000, the forbidden row, column and diagonal of
family c, the alternating 800-leaders on the base and the +-600 transitions (d') and one mid leader of 150 on seven transition
matrices (m) -- through every whole-contig arrangement, which store alpha at different scales.

The yardsticks, the query lists and the floor rule are tests/query_range_reference.py's; tests/test_query_range_host.py pins
the yardsticks on path enumeration on these very models and asserts the conditions the floor rule needs.  Every check function
and every bound is the query's own, imported unchanged: ``_check`` of tests/test_gpu_spans.py and tests/test_gpu_edges.py,
``_compare`` of tests/test_gpu_runs.py, ``_check_cond`` / ``_check_contributions`` of tests/test_gpu_conditionals.py, ``_exact``
of tests/test_gpu_sampling.py.  A case of the five linear-space queries is (query, arrangement, family); the models of a family
are looped inside and every one is run and printed before the case fails.  A case of the four log-space walks is one model.  Every case prints its worst error / bound, and for the log-valued queries how many
deep entries (yardstick < -790) came back finite and how many -inf.  ``run_posteriors`` has a narrower range of its own, max|trans|
<= 150: ``test_runs`` holds it to the yardstick inside it and to its refusal beyond."""
import numpy as np
import pytest

from tests import lattice_range_families as fam
from tests import minrun_reference as mr
from tests import query_range_reference as qr
from tests import runs_reference as rr
from tests import test_gpu_conditionals as gc
from tests import test_gpu_counts as gcn
from tests import test_gpu_edges as ge
from tests import test_gpu_kbest as gk
from tests import test_gpu_lattice_range as glr
from tests import test_gpu_minrun as gmr
from tests import test_gpu_minrun_marginals as gmm
from tests import test_gpu_runs as gr
from tests import test_gpu_sampling as gsm
from tests import test_gpu_spans as gs

pytestmark = pytest.mark.gpu

# the general kernels at 2 labels (a query's plan is laid out for them), and the arrangements of the lattice-range test
ARRANGEMENTS = [("L2-general", 2, ())] + glr.QUERY_ARRANGEMENTS
ARR_IDS = [a[0] for a in ARRANGEMENTS]
FAMILIES = sorted(fam.QUERY_FAMILIES)
N_SAMPLES = 200


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


def _models(nat, name, L, family):
    """Every model of a family: (tag, key, the distribution's key, model, csr, raw transitions, marginals_full's outputs).  The
    pass itself is held to its yardstick on the way (the tolerances of tests/test_gpu_lattice_range.py)."""
    for key in fam.QUERY_FAMILIES[family]:
        w, trans, leaders = fam.query_model(L, family, key)
        fig = fam.figures(trans)
        assert fig["in_range"]
        csr = fam.query_batch(L, leaders)
        model = nat.Model.from_tables(w, trans)
        emarg, elogz = model.marginals_full(*csr)
        yield f"{name} family {family} {key} (max trans {fig['tmax']:.6g})", key, qr.canon(family, key), model, csr, trans, (emarg, elogz)


def _run_family(nat, monkeypatch, name, L, switches, family, body):
    glr._switch(monkeypatch, switches)
    failed = []
    for tag, key, dist, model, csr, trans, full in _models(nat, name, L, family):
        try:  # (every model of the family is run and printed before the case fails)
            ref_marg, ref_logz = qr.marginal_reference(L, *dist)
            steps = np.maximum(np.diff(csr[0]).astype(np.float64) - 1.0, 0.0)
            glr._judge(f"{tag} pass", full[0], full[1], ref_marg, ref_logz + steps * fam.query_shift(L, family, key))
            body(tag, key, dist, model, csr, trans, full)
        except AssertionError as miss:
            failed.append(f"{tag}: {str(miss).splitlines()[0] if str(miss) else 'assertion'}")
    assert not failed, "\n".join(failed)


def _same_pass(tag, marg, logz, full):
    assert marg.tobytes() == full[0].tobytes() and logz.tobytes() == full[1].tobytes(), f"{tag}: want_marginals is not marginals_full's bytes"


def _deep_counts(tag, got, ref):
    _, deep = qr.classes(ref)
    g = np.asarray(got)[deep]
    print(f"{tag}: {int(deep.sum())} deep entries, {int(np.isfinite(g).sum())} came back finite, {int(np.isneginf(g).sum())} -inf")


# ---------------------------------------------------------------- spans
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,L,switches", ARRANGEMENTS, ids=ARR_IDS)
def test_spans(nat, monkeypatch, name, L, switches, family):
    spans = list(qr.spans(L))

    def body(tag, key, dist, model, csr, trans, full):
        ref, bound = qr.span_reference(L, *dist)
        logp, marg, logz = model.span_log_probabilities(*csr, *gs._arrays(spans), want_marginals=True)
        _deep_counts(f"{tag} spans", logp, ref)
        gs._check(f"{tag} spans", logp, ref, bound, spans, L)  # (strict at every depth: the masked pass reads raw scores)
        _same_pass(tag, marg, logz, full)

    _run_family(nat, monkeypatch, name, L, switches, family, body)


# ---------------------------------------------------------------- edges
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,L,switches", ARRANGEMENTS, ids=ARR_IDS)
def test_edges(nat, monkeypatch, name, L, switches, family):
    sets = qr.edge_sets(L)

    def body(tag, key, dist, model, csr, trans, full):
        out = model.edge_posteriors(*csr, sets=np.array(sets, dtype=np.uint32), want_pair=True, want_marginals=True)
        ge._check(f"{tag} edges", out, qr.edge_reference(L, *dist), csr[0], L, sets)
        _same_pass(tag, out["marginals"], out["lognorm"], full)
        dead = np.isneginf(fam.exp_zero(trans))
        assert not out["pair"][:, dead].any(), f"{tag}: mass on a transition whose exp is 0"

    _run_family(nat, monkeypatch, name, L, switches, family, body)


# ---------------------------------------------------------------- runs, under the floor rule
def _ordinary_rows(val):
    """The anchors every entry of whose rows is ordinary, per side."""
    rows = {}
    for side in ("start", "end"):
        stack = np.concatenate([val[f"log_{side}"], val[f"log_{side}_beyond"][:, None], val["log_anchor"][:, None]], axis=1)
        rows[side] = np.all((stack >= qr.ORDINARY) | np.isneginf(stack), axis=1)
    return rows


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,L,switches", ARRANGEMENTS, ids=ARR_IDS)
def test_runs(nat, monkeypatch, name, L, switches, family):
    """run_posteriors takes max|trans| <= 150 among the transitions whose exp is not 0 (plan_run_run_posteriors): the models on
    that side -- family a at 150 on both signs, b, c, d' and m on the base transitions, m at +-150 -- are held to the
    yardstick; the models beyond it (shifts of +-600 and +-700) are refused.  Before the refusal, under family m at those
    shifts 30 to 50 of about 3 400 ordinary entries a model came back -inf (yardstick -164 to -487, profiles/query_range.txt):
    the pass had flushed the label 150 nats behind at the leader's gene out of the stored alpha that the walks read."""
    anchors, runs = list(qr.anchors(L)), list(qr.closed_runs(L))

    def body(tag, key, dist, model, csr, trans, full):
        if not fam.runs_in_range(trans):  # the entry's own, narrower range: refused, with a message that names the weights and 150
            with pytest.raises(ValueError) as refusal:
                model.run_posteriors(*csr, anchors=gr._anchor_arrays(anchors), reach=qr.REACH, runs=gs._arrays(runs))
            assert glr.REFUSAL in str(refusal.value) and "150" in str(refusal.value), f"{tag}: {refusal.value}"
            print(f"{tag} runs: refused -- {refusal.value}")
            return
        (val, bnd), (rval, rbnd) = qr.runs_reference(L, *dist)
        out = model.run_posteriors(*csr, anchors=gr._anchor_arrays(anchors), reach=qr.REACH, runs=gs._arrays(runs), want_marginals=True)
        near = model.run_posteriors(*csr, anchors=gr._anchor_arrays(anchors), reach=7)
        worst, n_ord, kept, lost, failed = 0.0, 0, 0, 0, []
        for k, ref, b in [(k, val[k], bnd[k]) for k in qr.KEYS] + [("log_run", rval, rbnd)]:
            gone = np.isneginf(out[k]) & np.isfinite(ref) & (ref >= qr.ORDINARY)
            if gone.any():
                print(f"{tag} {k}: {int(gone.sum())} ordinary entries came back -inf, yardstick {ref[gone].min():.6g} .. {ref[gone].max():.6g}")
            try:
                ratio, n, fin, gone = qr.floor_compare(f"{tag} {k}", out[k], ref, b, gr._compare)
                worst, n_ord, kept, lost = max(worst, ratio), n_ord + n, kept + fin, lost + gone
            except AssertionError as miss:
                failed.append(str(miss).splitlines()[0])
        print(f"{tag} runs: {n_ord} ordinary finite entries, worst |difference| / bound = {worst:.3g}; deep entries: {kept} came back "
              f"finite, {lost} -inf")
        assert not failed, "; ".join(failed)
        # the identities of test_anchors_against_the_yardstick, on the ordinary rows
        rows = _ordinary_rows(val)
        checked = 0
        for side in ("start", "end"):
            stack = np.concatenate([out[f"log_{side}"], out[f"log_{side}_beyond"][:, None]], axis=1)
            for q in np.flatnonzero(rows[side]):
                total = rr._lse(stack[q])
                if np.isneginf(out["log_anchor"][q]):
                    assert np.isneginf(total), f"{tag}: anchor {q} is impossible and its {side}s are not"
                else:  # (every term within its bound: the sum within the largest of them, and the anchor within its own)
                    tol = max(bnd[f"log_{side}"][q].max(), bnd[f"log_{side}_beyond"][q]) + bnd["log_anchor"][q]
                    assert abs(total - out["log_anchor"][q]) <= tol, f"{tag}: the {side}s of anchor {q} add up to {total!r}, not {out['log_anchor'][q]!r}"
                checked += 1
            both = rows[side]
            assert near[f"log_{side}"][both].tobytes() == np.ascontiguousarray(out[f"log_{side}"][both][:, :8]).tobytes(), \
                f"{tag}: log_{side}: reach 7 against {qr.REACH}"
        assert near["log_anchor"].tobytes() == out["log_anchor"].tobytes(), f"{tag}: log_anchor depends on the reach"
        assert checked > 0
        _same_pass(tag, out["marginals"], out["lognorm"], full)

    _run_family(nat, monkeypatch, name, L, switches, family, body)


# ---------------------------------------------------------------- conditionals
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,L,switches", ARRANGEMENTS, ids=ARR_IDS)
def test_conditionals(nat, monkeypatch, name, L, switches, family):
    spans = list(qr.spans(L))

    def body(tag, key, dist, model, csr, trans, full):
        yard = qr.regions(L, *dist)
        ref, bound = qr.span_reference(L, *dist)
        for reach in (0, 8):
            out = model.span_conditionals(*csr, *gs._arrays(spans), reach=reach, want_marginals=True)
            _deep_counts(f"{tag} reach {reach} logp", out["logp"], ref)
            gs._check(f"{tag} reach {reach} logp", out["logp"], ref, bound, spans, L)
            gc._check_cond(f"{tag} reach {reach}", yard, spans, out, reach)
            _same_pass(tag, out["marginals"], out["lognorm"], full)
        gc._check_contributions(f"{tag} reach 8", yard, spans, out, 8, np.random.default_rng(7700 + L), limit=40)

    _run_family(nat, monkeypatch, name, L, switches, family, body)


# ---------------------------------------------------------------- sampling
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,L,switches", ARRANGEMENTS, ids=ARR_IDS)
def test_sampling(nat, monkeypatch, name, L, switches, family):
    def body(tag, key, dist, model, csr, trans, full):
        seed = 7800 + L
        _, _, leaders = fam.query_model(L, family, key)
        y, marg, logz = model.sample_paths(*csr, N_SAMPLES, seed=seed, want_marginals=True)
        assert y.shape == (int(csr[0][-1]), N_SAMPLES) and y.dtype == np.int8
        gsm._exact(f"{tag} N={N_SAMPLES}", y, dict(cptr=csr[0], trans=trans), qr.scores(L, leaders), seed)
        _same_pass(tag, marg, logz, full)
        inner = np.ones(len(y) - 1, dtype=bool)
        inner[csr[0][1:-1][(csr[0][1:-1] > 0) & (csr[0][1:-1] < len(y))] - 1] = False  # (pairs that straddle two contigs are no transitions)
        for i, j in zip(*np.nonzero(np.isneginf(fam.exp_zero(trans)))):
            assert not np.any((y[:-1] == i) & (y[1:] == j) & inner[:, None]), f"{tag}: a transition ({i}, {j}) whose exp is 0 was drawn"
        if leaders == "d":
            lead = fam.leader_of(csr)
            assert (lead >= 0).sum() > 100 and np.all(y[lead >= 0] == lead[lead >= 0][:, None]), f"{tag}: a label that leads by 800 was not drawn"

    _run_family(nat, monkeypatch, name, L, switches, family, body)


# ---------------------------------------------------------------- the four log-space walks, on the raw transitions
# K-best, min-run decoding, min-run marginals and run counts read the raw state scores and transition weights (an entry of -2000
# is a finite weight to them) and only share the pass's log Z, so they run through the default arrangement of every label count;
# every arrangement's log Z is held to the yardstick by the five queries above.  Each file's own `judge` and bounds, imported.
WALK_LABELS = (2, 3, 8, 17, 32)
_WALK_BATCHES = {}


def _walk_batch(L, family, key, distinct=False):
    """A planted model as the batch dict of tests/test_gpu_kbest.py (its judges keep their yardsticks on it).  `distinct`: every
    item carries an attribute of its own as well (fam.distinct_items), for the test that compares ranked paths."""
    if (L, family, key, distinct) not in _WALK_BATCHES:
        w, trans, leaders = fam.query_model(L, family, key)
        cptr, gptr, attr = csr = fam.query_batch(L, leaders)
        score = qr.scores(L, leaders)
        if distinct:
            csr, w = fam.distinct_items(L, csr, w)
            cptr, gptr, attr = csr
            score = gk.tables(dict(L=L, w=w, cptr=cptr, gptr=gptr, attr=attr), False, False)[0]
        _WALK_BATCHES[(L, family, key, distinct)] = dict(L=L, w=w, trans=trans, cptr=cptr, gptr=gptr, attr=attr, csr=csr,
                                                         v=np.ones(len(attr)), allowed=None, score=score)
    return _WALK_BATCHES[(L, family, key, distinct)]


def _walk_sets(sets, L, turn):
    """Every set up to 8 labels; beyond, one per call in rotation (a yardstick of 257 items at 32 labels takes a third of a second)."""
    return list(sets) if L <= 8 else [sets[turn % len(sets)]]


WALK_MODELS = [(f, k) for f in FAMILIES for k in fam.QUERY_FAMILIES[f]]
WALK_IDS = [f"{f}-{k}" for f, k in WALK_MODELS]


def _run_walk(nat, monkeypatch, L, family, key, body, distinct=False):
    """One model a case: a walk's yardstick of 257 items takes up to a second at 32 labels, and a family has up to seven models."""
    glr._switch(monkeypatch, ())
    turn = fam.QUERY_FAMILIES[family].index(key)
    b = _walk_batch(L, family, key, distinct)
    fig = fam.figures(b["trans"])
    assert fig["in_range"]
    model = nat.Model.from_tables(b["w"], b["trans"])
    body(f"L={L} family {family} {key} (max trans {fig['tmax']:.6g})", key, turn, b, model, model.marginals_full(*b["csr"])[1])


def _lz_bound(lz):
    return 1e-10 * np.maximum(1.0, np.abs(lz))


@pytest.mark.parametrize("family,key", WALK_MODELS, ids=WALK_IDS)
@pytest.mark.parametrize("L", WALK_LABELS)
def test_kbest(nat, monkeypatch, L, family, key):
    def body(tag, key, turn, b, model, elogz):
        ref = gk.reference(b, False, False)
        worst = -np.inf
        for K in (1, 5, 32):
            got = model.viterbi_kbest(*b["csr"], K)
            gk.accept(f"{tag} k={K}", b, ref, K, got)
            y, sc, npaths, lz = got
            assert lz.tobytes() == elogz.tobytes(), f"{tag}: lognorm is not marginals_full's bytes"
            for c, r in enumerate(ref):  # every path's probability is at most 1: the score and log Z each within its own bound
                for k in range(int(npaths[c])):
                    over = (sc[c, k] - lz[c]) - (r[2][k] + _lz_bound(lz[c]))
                    worst = max(worst, float(over))
                    assert over <= 0.0, f"{tag} k={K} contig {c} rank {k}: score {sc[c, k]!r} above log Z {lz[c]!r}"
        print(f"{tag}: largest (score - log Z) - bound = {worst:.3g}")

    _run_walk(nat, monkeypatch, L, family, key, body, distinct=True)


@pytest.mark.parametrize("family,key", WALK_MODELS, ids=WALK_IDS)
@pytest.mark.parametrize("L", WALK_LABELS)
def test_min_run_decoding(nat, monkeypatch, L, family, key):
    def body(tag, key, turn, b, model, elogz):
        worst = 0.0
        for i, m in enumerate((1, 2, 3, 32)):
            for mask in _walk_sets(gmr.label_sets(L), L, turn + i):
                got = model.viterbi_min_run(*b["csr"], mask, m)
                assert got[3].tobytes() == elogz.tobytes(), f"{tag}: lognorm is not marginals_full's bytes"
                # (judge holds log Z_C <= log Z, and = at m = 1, within the bound of the two)
                worst = max(worst, gmr.judge(f"{tag} set {mask:#x} m={m}", b, mask, m, False, False, got, False, base=0)[1])
        print(f"{tag}: worst |log Z_C - reference| / bound = {worst:.3g}")

    _run_walk(nat, monkeypatch, L, family, key, body)


@pytest.mark.parametrize("family,key", WALK_MODELS, ids=WALK_IDS)
@pytest.mark.parametrize("L", WALK_LABELS)
def test_min_run_marginals(nat, monkeypatch, L, family, key):
    def body(tag, key, turn, b, model, elogz):
        worst = 0.0
        sets = gmm.label_sets(L)
        for i, m in enumerate((1, 2, 3, 32)):
            for mask in _walk_sets(sets, L, turn + i) + ([1 << (L - 1)] if key == "diagonal" and L > 8 and m >= 2 else []):
                got = model.marginals_min_run(*b["csr"], mask, m)
                marg, inside, lzc, lz = got
                assert lz.tobytes() == elogz.tobytes(), f"{tag}: lognorm is not marginals_full's bytes"
                worst = max(worst, gmm.judge(f"{tag} set {mask:#x} m={m}", b, b["score"], mask, m, got))
                for c, ref in enumerate(gmm.yardstick(b, b["score"], mask, m)):  # log Z_C <= log Z, each within its own bound
                    if ref is not None and ref[1] > -np.inf:
                        T = int(b["cptr"][c + 1] - b["cptr"][c])
                        assert lzc[c] - lz[c] <= mr.lognorm_bound(T, L, ref[2]) + _lz_bound(lz[c]), f"{tag} set {mask:#x} m={m} contig {c}: log Z_C above log Z"
                # a run of two needs the forbidden self-transition (at 2 labels so does every other path: nothing to compare with)
                if key == "diagonal" and L > 2 and m >= 2 and bin(mask).count("1") == 1:
                    col = mask.bit_length() - 1
                    assert not np.isnan(marg).any() and np.all(marg[:, col] < 1e-279), f"{tag} set {mask:#x} m={m}: mass on a run the diagonal forbids"
        print(f"{tag}: worst error / bound = {worst:.3g}")

    _run_walk(nat, monkeypatch, L, family, key, body)


@pytest.mark.parametrize("family,key", WALK_MODELS, ids=WALK_IDS)
@pytest.mark.parametrize("L", WALK_LABELS)
def test_run_counts(nat, monkeypatch, L, family, key):
    def body(tag, key, turn, b, model, elogz):
        worst = 0.0
        for i, K in enumerate((1, 3, 32)):
            for mask in _walk_sets(gcn.label_sets(L), L, turn + i):
                got = model.run_counts(*b["csr"], mask, K)
                assert got[3].tobytes() == elogz.tobytes(), f"{tag}: lognorm is not marginals_full's bytes"
                # (judge holds the log-sum-exp of the count masses to log Z within the bound of the two)
                worst = max(worst, gcn.judge(f"{tag} set {mask:#x} K={K}", b, mask, K, False, False, got, False, base=0)[1])
        print(f"{tag}: worst |log Z_k - reference| / bound = {worst:.3g}")

    _run_walk(nat, monkeypatch, L, family, key, body)


# ---------------------------------------------------------------- the refusal outside [-700, 700]
def _entries(model, csr, L, empty):
    """The nine entries as thunks: with good arguments, or (`empty`) with an empty query list where the entry takes a list."""
    T = fam.QUERY_LENGTHS
    c = T.index(9)
    spans = [] if empty else [(c, 2, 6, 1), (c, 0, 9, 2)]
    anchors = [] if empty else [(c, 4, 1), (c, 0, 2)]
    empty3 = tuple(np.zeros(0, dtype=x) for x in (np.int32, np.int32, np.uint32))
    entries = {
        "span_log_probabilities": lambda: model.span_log_probabilities(*csr, *gs._arrays(spans), want_marginals=True),
        "edge_posteriors": lambda: model.edge_posteriors(*csr, sets=None if empty else np.array([1], dtype=np.uint32), want_marginals=True),
        "run_posteriors": lambda: model.run_posteriors(*csr, anchors=empty3 if empty else gr._anchor_arrays(anchors), reach=4, want_marginals=True),
        "span_conditionals": lambda: model.span_conditionals(*csr, *gs._arrays(spans), reach=1, want_marginals=True),
    }
    if not empty:
        entries.update({
            "sample_paths": lambda: model.sample_paths(*csr, 3, seed=1),
            "viterbi_kbest": lambda: model.viterbi_kbest(*csr, 2),
            "viterbi_min_run": lambda: model.viterbi_min_run(*csr, 1, 2),
            "marginals_min_run": lambda: model.marginals_min_run(*csr, 1, 2),
            "run_counts": lambda: model.run_counts(*csr, 1, 2),
        })
    return entries


@pytest.mark.parametrize("L", [2, 3, 17])
def test_every_query_refuses_outside_the_range_and_none_at_its_edge(nat, monkeypatch, L):
    """One grid step beyond +-700 and at +-800 each of the nine entries raises the binding's ValueError, whose message names the
    transition weights and 700, for good arguments and for an empty query list alike (at 2 labels an entry without queries is
    marginals_full's 2-label scan, which answers); at exactly +-700 none refuses but run_posteriors, whose own range ends at 150."""
    glr._switch(monkeypatch, ())
    w = fam.base(L)[0]
    csr = fam.query_batch(L, None)
    outside = [(k, fam.shift_any(L, k)[0]) for k in fam.BEYOND_G] + [(f"{c:+g}", fam.shifted(L, c)[0]) for c in fam.SHIFTS_E]
    for key, trans in outside:
        assert not fam.figures(trans)["in_range"] and np.all(np.isfinite(trans))
        model = nat.Model.from_tables(w, trans)
        answered = []
        for empty in (False, True):
            scan = L == 2 and empty  # (edge_posteriors without sets still returns transition counts and the entropy: a query)
            for name, call in _entries(model, csr, L, empty).items():
                try:
                    got = call()
                except ValueError as refusal:
                    assert glr.REFUSAL in str(refusal) and "700" in str(refusal), f"{name} at {key}: {refusal}"
                    assert not (scan and name != "edge_posteriors"), f"{name} at {key}: refused what the 2-label scan runs"
                    continue
                if scan and name != "edge_posteriors":  # without queries the entry is marginals_full, whose 2-label scan forms ratios of transitions
                    marg, logz = got[-2:] if isinstance(got, tuple) else (got["marginals"], got["lognorm"])
                    assert np.all(np.isfinite(marg)) and np.all(np.isfinite(logz)) and np.all(np.abs(marg.sum(axis=1) - 1.0) <= 1e-13)
                else:
                    answered.append(f"{name}{' (no queries)' if empty else ''}")
        assert not answered, f"at {key} these entries answered instead of refusing: {answered}"
        y, sc = model.viterbi(*csr)  # (Viterbi reads the raw weights and answers)
        assert y.shape == (int(csr[0][-1]),) and np.all(np.isfinite(sc))
    for key in fam.GUARD_G:
        trans = fam.shift_any(L, key)[0]
        assert abs(float(trans.max())) == 700.0 and fam.figures(trans)["in_range"]
        model = nat.Model.from_tables(w, trans)
        for empty in (False, True):
            for name, call in _entries(model, csr, L, empty).items():
                if name == "run_posteriors" and not empty:  # (its own range ends at 150: test_runs)
                    with pytest.raises(ValueError, match="150"):
                        call()
                else:
                    call()
    print(f"L={L}: nine entries refuse at {[k for k, _ in outside]} and answer at {list(fam.GUARD_G)}")
