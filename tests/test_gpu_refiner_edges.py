"""GPU: row R (csrc/crf_segment.hip) at every refiner boundary, through every entry point of the kernel, against the
numpy-mean reference of tests/helpers.py (RefinerReference: a literal statement of gecco/refine.py:51-64, 118-200).

The planted batches (plant_refiner_boundaries) put each decision on its boundary or one or two ulps from it: the grouper's
strict `>`, NaN inheritance, the "gecco" counts against n_cds and edge_distance, the "antismash" mean (numpy.mean's order:
8192-element chunks of pairwise sums), marker and gene counts, runs on lane and workgroup boundaries, batches of exactly
2048 genes (`seg_small`) and of 2049 (four launches).  A scale batch gives validate and compact several tiles per workgroup.

Out of scope, stated here: a gene without probability (NaN) inside an antismash run.  The reference raises TypeError out of
numpy.mean there; the device rejects the run (its mean is NaN)."""
import numpy as np
import pytest

# PyTorch ships its own copy of the HIP runtime: it has to be the one this process loads first
import torch

from tests.helpers import (GOLDEN, ULP_STEPS, RefinerReference, _markers_for, _ulp_step, plant_antismash_params, plant_refiner_boundaries,
                           refiner_params, synth_contigs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU suite must run on an MI355X"
    return _native


@pytest.fixture(scope="module")
def batches():
    return {b["name"]: b for b in plant_refiner_boundaries()}


@pytest.fixture(scope="module")
def real_model(nat):
    import os

    from oracle import lcrf

    st = lcrf.load_pickle(os.path.join(GOLDEN, "model.pkl"))
    return nat.Model.from_lcrf(st["blob"])


def _ref(b):
    return RefinerReference(b["p"], b["ann"], b["cptr"], b["mptr"], b["mid"])


def _native_segment(nat, b, kw):
    return nat.segment(b["p"], b["ann"], b["cptr"], kw["threshold"], kw["n_cds"], kw["edge_distance"], kw["trim"],
                       carry_state=kw["carry_state"], criterion=kw["criterion"], n_biopfams=kw.get("n_biopfams", 5),
                       average_threshold=kw.get("average_threshold", 0.6), marker_ptr=b["mptr"], marker_id=b["mid"])


@pytest.mark.parametrize("name", ["grouper", "gecco", "antismash", "geometry2048", "geometry2049", "geometry6150"])
def test_segment_planted(nat, batches, name):
    """`_native.segment` (gecco_crf_segment_ex): every planted parameter set decided as the reference decides it."""
    b = batches[name]
    ref = _ref(b)
    kept = dropped = 0
    for prm in b["params"]:
        kw = refiner_params(prm)
        exp = ref(**kw)
        got = _native_segment(nat, b, kw)
        assert got.tolist() == exp, (name, prm)
        if "plant" in prm and prm["plant"][1] == "mean":
            row = ref.stats(kw["threshold"], kw["carry_state"], kw["trim"])[prm["plant"][0]]["row"]
            kept += row in exp
            dropped += row not in exp
    if b["params"][-1]["criterion"] == "antismash":
        assert kept and dropped


@pytest.mark.parametrize("name", ["antismash", "geometry2048", "geometry2049", "geometry6150"])
def test_plan_run_segment_planted(nat, real_model, batches, name):
    """`Plan.run_segment` on device arrays: the rows, the total, and with max_seg below the total only the first max_seg rows
    written (the rows behind them untouched)."""
    b = batches[name]
    ref = _ref(b)
    dev = torch.device("cuda", 0)
    n = len(b["p"])
    plan = nat.Plan(real_model, b["cptr"], 20, 1, True, device=0)
    d_p, d_ann, d_mptr, d_mid = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (b["p"], b["ann"], b["mptr"],
                                                                                          b["mid"] if len(b["mid"]) else np.zeros(1, np.int32)))
    d_seg = torch.empty((n, 4), dtype=torch.int32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cut = 0
    for prm in b["params"]:
        kw = refiner_params(prm)
        exp = ref(**kw)
        for max_seg in (n, len(exp) - 1, len(exp) // 2):
            if max_seg < 0:
                continue
            d_seg.fill_(-7)
            plan.run_segment(d_p.data_ptr(), d_ann.data_ptr(), d_seg.data_ptr(), max_seg, d_n.data_ptr(), kw["threshold"],
                             kw["n_cds"], kw["edge_distance"], kw["trim"], kw["carry_state"], stream, criterion=kw["criterion"],
                             n_biopfams=kw.get("n_biopfams", 5), average_threshold=kw.get("average_threshold", 0.6),
                             d_marker_ptr=d_mptr.data_ptr(), d_marker_id=d_mid.data_ptr())
            torch.cuda.synchronize(dev)
            seg = d_seg.cpu().numpy()
            assert int(d_n.item()) == len(exp), (name, prm, max_seg)
            w = min(max_seg, len(exp))
            assert seg[:w].tolist() == exp[:w], (name, prm, max_seg)
            assert (seg[w:] == -7).all(), (name, prm, max_seg)
            cut += max_seg < len(exp)
    assert cut > 10


def _session_batch(rng, oracle_model):
    lengths = [1, 7, 8, 9, 2049, 3000, 40, 0, 300] + [int(x) for x in rng.integers(1, 400, size=40)]
    cptr, gptr, attr = synth_contigs(rng, lengths, oracle_model["state"].shape[0])
    ann = (np.diff(gptr) > 0).astype(np.uint8)
    mptr, mid = _markers_for(rng, ann, np.arange(12), rate=0.5)
    return cptr, gptr, attr, ann, np.asarray(mptr, dtype=np.int32), np.asarray(mid, dtype=np.int32)


@pytest.mark.parametrize("chunk", [None, 1024])
def test_session_clusters_planted(nat, real_model, oracle_model, monkeypatch, chunk):
    """`Session.clusters` (direct path; GECCO_CRF_CHUNK_GENES=1024: many chunks), both criteria, thresholds planted on the
    session's own probabilities: the grouper threshold at a gene's p and one ulp either side, the antismash threshold at the
    mean of a run and 1, 2 ulps either side.  `seg_p[seg_off[i]:seg_off[i+1]]` is p of row i's genes, bit for bit."""
    if chunk:
        monkeypatch.setenv("GECCO_CRF_CHUNK_GENES", str(chunk))
    rng = np.random.default_rng(31)
    cptr, gptr, attr, ann, mptr, mid = _session_batch(rng, oracle_model)
    ses = nat.Session(real_model, [0])
    _, _, _, p = ses.clusters(cptr, gptr, attr, ann, 20, threshold=0.5, want_p=True)
    p = np.array(p)
    ref = RefinerReference(p, ann, cptr, mptr, mid)
    v = np.sort(p)
    params = []
    for q in (0.3, 0.5, 0.7):
        x = float(v[int(q * len(v))])
        for k in (-1, 0, 1):
            for n_cds in (1, 3):
                params.append(dict(threshold=_ulp_step(x, k), criterion="gecco", n_cds=n_cds, edge_distance=2, trim=True, carry_state=False))
    thr = float(v[len(v) // 2])
    runs = ref.stats(thr, False, True)
    longest = sorted(range(len(runs)), key=lambda i: runs[i]["row"][3] - runs[i]["row"][2])[-4:]
    params += [prm for prm in plant_antismash_params(ref, thr, trims=(True,), runs=set(longest) | {0, 1, 2})]
    for prm in params:
        kw = refiner_params(prm)
        exp = ref(**kw)
        seg, seg_p, seg_off, _ = ses.clusters(cptr, gptr, attr, ann, 20, threshold=kw["threshold"], n_cds=kw["n_cds"],
                                              edge_distance=kw["edge_distance"], trim=kw["trim"], criterion=kw["criterion"],
                                              n_biopfams=kw.get("n_biopfams", 5), average_threshold=kw.get("average_threshold", 0.6),
                                              marker_ptr=mptr, marker_id=mid)
        assert seg.tolist() == exp, prm
        lens = [b - a for _, _, a, b in exp]
        assert seg_off.tolist() == np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).tolist()
        want = np.concatenate([p[a:b] for _, _, a, b in exp] + [np.zeros(0)])
        assert seg_p.tobytes() == want.tobytes()


def test_predict_tables_antismash_planted(oracle_model):
    """`predict.predict_tables(criterion="antismash")` (packer -> device probabilities -> device refiner -> cluster table)
    against `refine.ClusterRefiner` on the same probabilities, average_threshold planted at a cluster's numpy.mean and 1, 2
    ulps either side: the cluster is kept exactly when the threshold does not exceed its mean."""
    import itertools
    import warnings

    from gecco_amd import predict, refine, tables
    from gecco_amd.crf import ClusterCRF
    from tests.test_gpu_dropin import _random_tables

    rng = np.random.default_rng(37)
    bio = sorted(refine.BIO_PFAMS)
    names = list(oracle_model["attrs"][:60]) + bio[:40] + ["PF99999"]
    genes_t, feats_t = _random_tables(rng, 40, names, True)
    crf = ClusterCRF.trained(GOLDEN)
    by_pid = {g.protein.id: g for g in genes_t.to_genes()}
    for g in feats_t.to_genes():
        by_pid[g.protein.id].protein.domains.extend(g.protein.domains)
    annotated = crf.predict_probabilities(list(by_pid.values()))

    def objects(**kw):
        refiner = refine.ClusterRefiner(criterion="antismash", **kw)
        out = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _, group in itertools.groupby(annotated, key=lambda g: g.source.id):
                out.extend(refiner.iter_clusters(list(group)))
        return out

    base = dict(threshold=0.3, n_cds=2, n_biopfams=1)
    candidates = objects(average_threshold=0.0, **base)
    assert len(candidates) >= 3
    planted = 0
    for cl in candidates[:3]:
        mean = float(np.mean([g.average_probability for g in cl.genes]))
        for k in ULP_STEPS:
            kw = dict(base, average_threshold=_ulp_step(mean, k))
            exp = objects(**kw)
            assert (k <= 0) == any(c.id == cl.id for c in exp)
            exp_t = tables.ClusterTable.from_clusters(exp)
            _, _, c_out = predict.predict_tables(genes_t, feats_t, crf, criterion="antismash", **kw)
            for name in ("sequence_id", "cluster_id", "start", "end", "average_p", "max_p", "proteins", "domains"):
                assert list(c_out.columns[name]) == list(exp_t.columns[name]), (name, k)
            planted += 1
    assert planted == 15


def test_segment_scale_several_tiles_per_workgroup(nat):
    """1.2 M genes alternating in and out (600 000 one-gene runs: more than 2048 x 256, so every validate / compact workgroup
    takes several tiles and compact carries the tiles before), then one 300 000-gene contig that is a single run whose
    antismash mean spans 37 numpy buffer chunks.  Rows, offsets and gathered probabilities through `Session.clusters` on a
    model whose marginals are each gene's own (zero transitions), rows through `_native.segment`; all exact."""
    from oracle import crf_oracle as orc

    rng = np.random.default_rng(41)
    n_alt, n_big, per = 1_200_000, 300_000, 20_000
    # zero transitions: the marginal of a gene is the logistic of its own score difference, whatever the window
    A = 102
    state = np.zeros((A, 2))
    state[0, 1], state[1, 0] = 4.0, 4.0
    state[2:, 1] = rng.uniform(0.5, 4.0, size=A - 2)
    model = nat.Model.from_tables(state, np.zeros((2, 2)))
    attr = np.concatenate([np.arange(n_alt) % 2, rng.integers(2, A, size=n_big)]).astype(np.int32)
    n = n_alt + n_big
    gptr = np.arange(n + 1, dtype=np.int32)
    cptr = np.array(list(range(0, n_alt + 1, per)) + [n], dtype=np.int32)
    ann = (rng.random(n) < 0.7).astype(np.uint8)
    ann[n_alt] = ann[n - 1] = 0  # the big run trims at both ends
    ses = nat.Session(model, [0])
    _, _, _, p = ses.clusters(cptr, gptr, attr, ann, 20, threshold=0.5, want_p=True)
    p = np.array(p)
    assert (p[:n_alt:2] > 0.5).all() and (p[1:n_alt:2] < 0.5).all() and (p[n_alt:] > 0.5).all()
    # expected by construction: one run per even gene of the alternating contigs, numbered per contig; then the big run
    g = np.arange(0, n_alt, 2)
    keep = ann[g] == 1
    rows = np.stack([g // per, (g % per) // 2 + 1, g, g + 1], axis=1)[keep]
    big_ann = np.flatnonzero(ann[n_alt:]) + n_alt
    big = [len(cptr) - 2, 1, int(big_ann[0]), int(big_ann[-1]) + 1]
    exp = np.concatenate([rows, [big]]).tolist()
    assert orc.segment(p, ann, cptr, 0.5, 1, 0, True).tolist() == exp
    got = nat.segment(p, ann, cptr, 0.5, 1, 0, True)
    assert got.tolist() == exp
    seg, seg_p, seg_off, _ = ses.clusters(cptr, gptr, attr, ann, 20, threshold=0.5, n_cds=1)
    assert seg.tolist() == exp
    lens = np.array([b - a for _, _, a, b in exp], dtype=np.int64)
    assert seg_off.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert seg_p.tobytes() == np.concatenate([p[a:b] for _, _, a, b in exp]).tobytes()
    # antismash: the big run's mean planted (no markers asked for); every one-gene run is far above it
    mptr = np.zeros(n + 1, dtype=np.int32)
    a, b = big[2], big[3]
    assert b - a > 36 * 8192
    mean = float(np.mean([float(x) for x in p[a:b]]))
    assert p[:n_alt:2].min() > mean + 0.01
    for k in ULP_STEPS:
        avg = _ulp_step(mean, k)
        exp_k = rows.tolist() + ([big] if k <= 0 else [])
        got = nat.segment(p, ann, cptr, 0.5, 1, 0, True, criterion="antismash", n_biopfams=0, average_threshold=avg,
                          marker_ptr=mptr, marker_id=np.zeros(1, np.int32))
        assert got.tolist() == exp_k, k
        seg, seg_p, seg_off, _ = ses.clusters(cptr, gptr, attr, ann, 20, threshold=0.5, n_cds=1, criterion="antismash", n_biopfams=0,
                                              average_threshold=avg, marker_ptr=mptr, marker_id=np.zeros(1, np.int32))
        assert seg.tolist() == exp_k, k
        assert int(seg_off[-1]) == sum(r[3] - r[2] for r in exp_k)
