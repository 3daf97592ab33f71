"""Every Viterbi path returns CRFsuite's labels ([EXT] crf1dc_viterbi: strict '<', first arg max) on planted near-ties.

The batches come from tests/helpers.py (plant_viterbi_ties): real-valued weights, and at the genes right after the boundaries
the kernels compose across (8-gene lanes, 64-gene chunks, 2048-gene scan blocks, a block boundary more than 64 blocks into a
300 000-gene contig) two candidates of CRFsuite's own delta recursion lie 0, +-1 or +-2 ulps apart -- at a contig's end
(the final scores) and inside it (a back-pointer).  A kernel that regroups the recursion (composed max-plus products, the
difference form) sees another rounding of the same two sums and, without a margin test and a second pass, decides some of
them the other way.  Labels must equal oracle.viterbi exactly; path scores lie within a per-contig bound of the oracle's and
of the exact sum of the returned path (helpers.check_viterbi_scores)."""
import functools

import numpy as np
import pytest

from tests.helpers import check_viterbi_scores, plant_viterbi_ties, synth_contigs, synth_model

pytestmark = pytest.mark.gpu

TRANS2 = np.array([[2.669891070463728, -2.599571900486168], [-2.6019205422130995, 2.5683226020688488]])
ANTI2 = np.array([[-1.3, 2.1], [1.7, -0.9]])  # t01 - t11 > t00 - t10: no difference form
SHAPES = {
    "short": [9, 0, 200, 1, 2048, 3, 17] + [200] * 24,  # every contig <= 2048 genes: whole contigs per workgroup
    "long": [9, 0, 200, 1, 2049, 3, 50000, 0, 300000, 7],
    "any": [9, 0, 200, 1, 2049, 3, 50000, 7, 66],
}


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    assert _native.device_count() >= 1
    return _native


@functools.lru_cache(maxsize=None)
def _batch(L, shape, anti=False):
    from oracle import crf_oracle as orc

    rng = np.random.default_rng(1000 * L + len(shape) + (7 if anti else 0))
    trans = (ANTI2 if anti else TRANS2) if L == 2 else rng.normal(0.0, 1.5, size=(L, L))
    w, cptr, gptr, attr, cases = plant_viterbi_ties(rng, SHAPES[shape], L, trans)
    ey, esc = orc.viterbi(w, trans, cptr, gptr, attr)
    for c in cases:  # (the planter's own test pins this; a cheap restatement against the batch at hand)
        assert ey[c["gene"]] == c["winner"]
    return dict(w=w, trans=trans, cptr=cptr, gptr=gptr, attr=attr, cases=cases, ey=ey, esc=esc, n=int(cptr[-1]))


def _labels(b, y, what):
    y = np.asarray(y).astype(np.int32)
    bad = np.nonzero(y != b["ey"])[0]
    missed = [c for c in b["cases"] if y[c["gene"]] != c["winner"]]
    assert bad.size == 0, f"{what}: {bad.size} labels differ from the oracle's (first at gene {bad[:5]}); planted decisions missed: {missed[:3]}"


def _scores(b, sc, y, what):
    check_viterbi_scores(sc, b["esc"], b["w"], b["trans"], b["cptr"], b["gptr"], b["attr"], y, what)


def _dev(b):
    import torch

    return torch.from_numpy(b["gptr"]).cuda(), torch.from_numpy(b["attr"]).cuda()


def _run_plan_viterbi(nat, model, b, score):
    import torch

    d_gp, d_at = _dev(b)
    n, nc = b["n"], len(b["cptr"]) - 1
    plan = nat.Plan(model, b["cptr"], 20, 1, True, device=0)
    d_y = torch.full((n,), 7, dtype=torch.int8, device="cuda:0")
    d_sc = torch.zeros(nc, dtype=torch.float64, device="cuda:0") if score else None
    plan.viterbi_stats(reset=True)
    plan.run_viterbi(d_gp.data_ptr(), d_at.data_ptr(), d_y.data_ptr(), d_sc.data_ptr() if score else 0)
    st = plan.viterbi_stats()
    return d_y.cpu().numpy(), (d_sc.cpu().numpy() if score else None), st


def _run_plan_decode(nat, model, b):
    import torch

    d_gp, d_at = _dev(b)
    n, nc = b["n"], len(b["cptr"]) - 1
    plan = nat.Plan(model, b["cptr"], 20, 1, True, device=0)
    d_p = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    d_y = torch.full((n,), 7, dtype=torch.int8, device="cuda:0")
    d_sc = torch.zeros(nc, dtype=torch.float64, device="cuda:0")
    plan.run_decode(d_gp.data_ptr(), d_at.data_ptr(), d_p.data_ptr(), d_y.data_ptr(), 1, d_sc.data_ptr())
    return d_y.cpu().numpy(), d_sc.cpu().numpy()


# ---- two labels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["short", "long"])
def test_difference_form_on_planted_ties(nat, shape):
    """Labels without a score, sticky transitions: the difference form (vd_short; vd_fold -> vd_replay -> v_labels_refine ->
    vd_exact_fix) with its margin test -- end ties and, new here, interior ties at lane and block boundaries."""
    import torch

    b = _batch(2, shape)
    model = nat.Model.from_tables(b["w"], b["trans"])
    y, _ = model.viterbi(b["cptr"], b["gptr"], b["attr"], want_score=False)
    _labels(b, y, "Model.viterbi(want_score=False)")
    y, _, st = _run_plan_viterbi(nat, model, b, score=False)
    _labels(b, y, "Plan.run_viterbi")
    assert st["contigs_redecoded"] >= len({c["contig"] for c in b["cases"]}), st
    _, y = nat.Session(model, [0]).decode(b["cptr"], b["gptr"], b["attr"], 20)
    _labels(b, y, "Session.decode")
    # the throughput form: labels of a batch leave with the next call's launch (or the flush)
    d_gp, d_at = _dev(b)
    n = b["n"]
    plans = [nat.Plan(model, b["cptr"], 20, 1, True, device=0) for _ in range(2)]
    p = [torch.zeros(n, dtype=torch.float64, device="cuda:0") for _ in range(2)]
    yy = [torch.full((n,), 7, dtype=torch.int8, device="cuda:0") for _ in range(2)]
    plans[0].run_decode_pipelined(d_gp.data_ptr(), d_at.data_ptr(), p[0].data_ptr())
    plans[1].run_decode_pipelined(d_gp.data_ptr(), d_at.data_ptr(), p[1].data_ptr(), plans[0], yy[0].data_ptr())
    plans[1].flush_decode_pipelined(yy[1].data_ptr())
    torch.cuda.synchronize()
    for k in range(2):
        _labels(b, yy[k].cpu().numpy(), f"Plan.run_decode_pipelined[{k}]")


@pytest.mark.parametrize("shape", ["short", "long"])
def test_score_requested_on_planted_ties(nat, shape):
    """A path score requested (Model.viterbi's default, Plan.run_viterbi / run_decode with d_score): CRFsuite's labels, and
    per contig a score within its bound of the oracle's and of the exact sum of the returned path."""
    b = _batch(2, shape)
    model = nat.Model.from_tables(b["w"], b["trans"])
    y, sc = model.viterbi(b["cptr"], b["gptr"], b["attr"])
    _labels(b, y, "Model.viterbi()")
    _scores(b, sc, y, "Model.viterbi()")
    y, sc, _ = _run_plan_viterbi(nat, model, b, score=True)
    _labels(b, y, "Plan.run_viterbi(d_score)")
    _scores(b, sc, y, "Plan.run_viterbi(d_score)")
    y, sc = _run_plan_decode(nat, model, b)
    _labels(b, y, "Plan.run_decode(d_score)")
    _scores(b, sc, y, "Plan.run_decode(d_score)")


@pytest.mark.parametrize("shape", ["short", "long"])
@pytest.mark.parametrize("variant", ["anti-sticky", "GECCO_CRF_VITERBI=matrix"])
def test_matrix_form_without_score_on_planted_ties(nat, shape, variant, monkeypatch):
    """Labels without a score from the matrix form: transitions with t01 - t11 > t00 - t10 (no difference form), or the
    matrix form forced on sticky ones."""
    anti = variant == "anti-sticky"
    if not anti:
        monkeypatch.setenv("GECCO_CRF_VITERBI", "matrix")
    b = _batch(2, shape, anti)
    model = nat.Model.from_tables(b["w"], b["trans"])
    y, _ = model.viterbi(b["cptr"], b["gptr"], b["attr"], want_score=False)
    _labels(b, y, f"{variant}: Model.viterbi(want_score=False)")
    y, sc = model.viterbi(b["cptr"], b["gptr"], b["attr"])
    _labels(b, y, f"{variant}: Model.viterbi()")
    _scores(b, sc, y, f"{variant}: Model.viterbi()")
    y, _, st = _run_plan_viterbi(nat, model, b, score=False)
    _labels(b, y, f"{variant}: Plan.run_viterbi")
    # every planted decision lies inside the margin: every contig with one went through CRFsuite's recursion
    assert st["contigs_redecoded"] >= len({c["contig"] for c in b["cases"]}), st
    y, sc = _run_plan_decode(nat, model, b)
    _labels(b, y, f"{variant}: Plan.run_decode(d_score)")
    _scores(b, sc, y, f"{variant}: Plan.run_decode(d_score)")


@pytest.mark.parametrize("chunked", [None, "0", "1"])
def test_general_kernels_on_two_labels_on_planted_ties(nat, chunked, monkeypatch):
    """GECCO_CRF_FORCE_GENERAL=1: a 2-label model through the any-L kernels (contig-sequential and chunked)."""
    monkeypatch.setenv("GECCO_CRF_FORCE_GENERAL", "1")
    if chunked is not None:
        monkeypatch.setenv("GECCO_CRF_GENERAL_CHUNKED", chunked)
    b = _batch(2, "long")
    model = nat.Model.from_tables(b["w"], b["trans"])
    y, sc = model.viterbi(b["cptr"], b["gptr"], b["attr"])
    _labels(b, y, f"general, chunked={chunked}")
    _scores(b, sc, y, f"general, chunked={chunked}")


# ---- any label count ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 5, 8])
@pytest.mark.parametrize("chunked", [None, "0", "1"])
def test_small_label_counts_on_planted_ties(nat, L, chunked, monkeypatch):
    if chunked is not None:
        monkeypatch.setenv("GECCO_CRF_GENERAL_CHUNKED", chunked)
    b = _batch(L, "any")
    model = nat.Model.from_tables(b["w"], b["trans"])
    y, sc = model.viterbi(b["cptr"], b["gptr"], b["attr"])
    _labels(b, y, f"L={L}, chunked={chunked}")
    _scores(b, sc, y, f"L={L}, chunked={chunked}")
    if chunked != "0":  # (the default takes the chunked kernels too: a contig is longer than 2048 genes)
        y, _, st = _run_plan_viterbi(nat, model, b, score=False)
        _labels(b, y, f"L={L}, chunked={chunked}: Plan.run_viterbi")
        # every planted decision lies inside gl_chunk_vit's margin: each contig with one went through gl_viterbi_seq
        assert st["contigs_redecoded"] >= len({c["contig"] for c in b["cases"]}), st


@pytest.mark.parametrize("L", [9, 13, 16, 17, 32])
@pytest.mark.parametrize("mode", ["wave", "chunked", "split"])
def test_large_label_counts_on_planted_ties(nat, L, mode, monkeypatch):
    monkeypatch.setenv("GECCO_CRF_GENERAL_VITERBI", mode)
    b = _batch(L, "any")
    y, sc = nat.Model.from_tables(b["w"], b["trans"]).viterbi(b["cptr"], b["gptr"], b["attr"])
    _labels(b, y, f"L={L}, {mode}")
    _scores(b, sc, y, f"L={L}, {mode}")


def test_predict_single_on_planted_ties(nat):
    """The drop-in class: ClusterCRF.model.predict_single (Model.viterbi with its default score) on planted contigs."""
    from gecco_amd.crf import _CRFSuiteModelView

    b = _batch(2, "long")
    view = _CRFSuiteModelView(nat.Model.from_tables(b["w"], b["trans"]))
    for c in (2, 4, 6):  # 200, 2049 and 50 000 genes
        g0, g1 = int(b["cptr"][c]), int(b["cptr"][c + 1])
        xseq = [{view.attributes_[g]: True} for g in range(g0, g1)]
        want = [view.classes_[v] for v in b["ey"][g0:g1].tolist()]
        assert view.predict_single(xseq) == want, c


@pytest.mark.parametrize("variant", ["anti-sticky", "GECCO_CRF_VITERBI=matrix"])
def test_matrix_margin_is_rigorous_and_rarely_met(nat, variant, monkeypatch):
    """The matrix form's margin, (4 t + 4) ulp(M) at the t-th gene of a contig (crf_sequence.hip, v_margin), is practically
    never met on real-valued models: no contig of a C2-shaped batch, nor of five 30 000-gene contigs, is decoded again, and
    the labels are the oracle's.  (Anti-sticky transitions make alternating paths the best ones, and over genes with equal
    state scores -- genes without domains -- their permutations tie in real arithmetic: there CRFsuite's own rounding
    decides, and the second pass rightly runs.  So the anti-sticky model here gives every gene N(0, 1) scores of its own.)"""
    from oracle import crf_oracle as orc

    anti = variant == "anti-sticky"
    if not anti:
        monkeypatch.setenv("GECCO_CRF_VITERBI", "matrix")
    rng = np.random.default_rng(4343)
    A = 3000
    w, trans = synth_model(A, rng)
    if anti:
        trans = ANTI2
    for lengths in (list(np.clip(np.round(rng.lognormal(np.log(200), 0.5, size=400)), 5, 2000).astype(int)), [30000] * 5):
        cptr, gptr, attr = synth_contigs(rng, lengths, A)
        if anti:
            n = int(cptr[-1])
            w, gptr, attr = rng.normal(0.0, 1.0, size=(n, 2)), np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
        ey, _ = orc.viterbi(w, trans, cptr, gptr, attr)
        b = dict(cptr=cptr, gptr=gptr, attr=attr, n=int(cptr[-1]), ey=ey, cases=[])
        y, _, st = _run_plan_viterbi(nat, nat.Model.from_tables(w, trans), b, score=False)
        _labels(b, y, variant)
        assert st["contigs_redecoded"] == 0 and st["inside_margin"] == 0, st


@pytest.mark.parametrize("L", [2, 3, 8, 17])
def test_chunked_margin_is_rigorous_and_rarely_met(nat, L, monkeypatch):
    """gl_chunk_vit's margin, (4 t + 8) ulp(M) between the best and the second-best candidate of a decision at the t-th gene of
    a contig (crf_general.hip), is practically never met on real-valued models: with the chunked kernels forced, no contig of
    a C2-shaped batch is decoded again, and the labels are the oracle's.  (The bound is linear in the gene's position: on five
    30 000-gene contigs it is met, rarely at 8 labels and in every contig at 17, which then take gl_viterbi_seq.  On the synthetic
    model of SURVEY.md 8d a third of the genes have no domains, and along a run of them the best paths circle the heaviest
    transition cycle: paths entering it at different labels sum the same transitions in another order, an exact tie in real
    arithmetic that only CRFsuite's rounding decides -- at 17 labels in most contigs of the C2 batch.  There the second pass
    rightly runs and the labels are still the oracle's; the zero count is asserted on every gene scoring N(0, 1) of its own.)"""
    from oracle import crf_oracle as orc

    monkeypatch.setenv("GECCO_CRF_GENERAL_CHUNKED", "1")
    monkeypatch.setenv("GECCO_CRF_GENERAL_VITERBI", "chunked")
    if L == 2:
        monkeypatch.setenv("GECCO_CRF_FORCE_GENERAL", "1")
    rng = np.random.default_rng(4444 + L)
    A = 3000
    w, trans = synth_model(A, rng, L=L)
    for lengths in (list(np.clip(np.round(rng.lognormal(np.log(200), 0.5, size=400)), 5, 2000).astype(int)), [30000] * 5):
        cptr, gptr, attr = synth_contigs(rng, lengths, A)
        ey, _ = orc.viterbi(w, trans, cptr, gptr, attr)
        b = dict(cptr=cptr, gptr=gptr, attr=attr, n=int(cptr[-1]), ey=ey, cases=[])
        y, _, _ = _run_plan_viterbi(nat, nat.Model.from_tables(w, trans), b, score=False)
        _labels(b, y, f"L={L}, chunked, synthetic model")
        n = int(cptr[-1])
        wn, gn, an = rng.normal(0.0, 1.0, size=(n, L)), np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
        en, _ = orc.viterbi(wn, trans, cptr, gn, an)
        b = dict(cptr=cptr, gptr=gn, attr=an, n=n, ey=en, cases=[])
        y, _, st = _run_plan_viterbi(nat, nat.Model.from_tables(wn, trans), b, score=False)
        _labels(b, y, f"L={L}, chunked, N(0, 1) scores")
        if len(lengths) > 5:
            assert st["contigs_redecoded"] == 0 and st["inside_margin"] == 0, st
        else:  # (30 000 genes: the margin grows with t -- (4 t + 8) ulp(M) is ~1e-5 at the end -- and at 17 labels every
            # such contig holds a decision inside it; the labels are CRFsuite's either way)
            assert st["contigs_redecoded"] <= len(lengths), st
