"""The refiner boundary planter of tests/helpers.py (plant_refiner_boundaries) and its reference (RefinerReference, a literal
statement of gecco/refine.py:51-64, 118-200 with numpy.mean), checked on the CPU before any device sees the batches: the
planted antismash thresholds lie 0, +-1 and +-2 ulps from numpy.mean of their run, and the oracle (the checker of
csrc/crf_segment.hip) and the object-level `gecco_amd.refine.ClusterRefiner` decide every planted parameter set as the
reference does."""
import warnings

import numpy as np
import pytest

from tests.helpers import (RefinerReference, _ulp_step, genes_from_planted, plant_refiner_boundaries, refiner_params,
                           rows_from_clusters)


@pytest.fixture(scope="module")
def batches():
    return plant_refiner_boundaries()


def _ref(b):
    return RefinerReference(b["p"], b["ann"], b["cptr"], b["mptr"], b["mid"])


def _placed(rows):
    """rows with an empty (trimmed to nothing) cluster carrying no position"""
    return [[c, k, None, None] if a == b else [c, k, a, b] for c, k, a, b in rows]


def test_planted_means_sit_on_the_boundary(batches):
    """numpy.mean of every planted run equals numpy's order restated scalar by scalar (oracle/composition.py), the planted
    threshold is k ulps from it, and the run is kept exactly when k <= 0.  The left-to-right sum misses numpy's mean on
    runs of 8 genes and more often enough for the planted decisions to tell the two orders apart."""
    from oracle.composition import pairwise_sum

    seen, ltr_off = set(), 0
    for b in batches:
        ref = _ref(b)
        for prm in b["params"]:
            if prm.get("plant", (0, ""))[1] != "mean":
                continue
            i, _, k = prm["plant"]
            st = ref.stats(prm["threshold"], prm["carry_state"], prm["trim"])[i]
            c, num, a, e = st["row"]
            run = [float(x) for x in b["p"][a:e]]
            assert float(np.mean(run)) == st["mean"] == pairwise_sum(run) / len(run)
            assert prm["average_threshold"] == _ulp_step(st["mean"], k)
            assert (k <= 0) == ([c, num, a, e] in ref(**refiner_params(prm)))
            seen.add((b["name"], e - a))
            if k == 0:
                ltr = 0.0
                for x in run:
                    ltr += x
                ltr_off += ltr / len(run) != st["mean"]
    lengths = {n for name, n in seen if name == "antismash"}
    assert {1, 7, 8, 9, 16, 127, 128, 129, 136, 1000, 8191, 8192, 8193, 20000} <= lengths
    assert ltr_off >= 5


def test_planter_covers_the_boundaries(batches):
    by = {b["name"]: b for b in batches}
    g = by["grouper"]
    p = g["p"]
    thr = {prm["threshold"] for prm in g["params"]}
    assert 0.0 in thr and 1.0 in thr and sum(1 for t in thr if t in set(p[~np.isnan(p)].tolist())) >= 5
    assert np.any(np.signbit(p) & (p == 0.0)) and 5e-324 in p.tolist() and 1.0 in p.tolist()
    cptr = g["cptr"]
    assert np.any(np.diff(cptr) == 0)
    assert any(np.isnan(p[cptr[c]]) for c in range(len(cptr) - 1) if cptr[c + 1] > cptr[c])
    gec = by["gecco"]
    assert {prm["edge_distance"] for prm in gec["params"]} >= {0, 1, 10 ** 6} and any(prm["n_cds"] == 0 for prm in gec["params"])
    for name in ("geometry2048", "geometry2049", "geometry6150"):
        assert len(by[name]["p"]) == int(name[8:])
    assert 2048 in by["geometry6150"]["cptr"].tolist()
    kinds = {(prm["plant"][1], prm["plant"][2]) for prm in by["antismash"]["params"]}
    assert {("empty", 0), ("markers", 0), ("markers", 1), ("genes", 0), ("genes", 1)} <= kinds


def test_oracle_equals_the_reference(batches):
    from oracle import crf_oracle as orc

    for b in batches:
        ref = _ref(b)
        for prm in b["params"]:
            kw = refiner_params(prm)
            exp = ref(**kw)
            if kw["criterion"] == "gecco":
                got = orc.segment(b["p"], b["ann"], b["cptr"], kw["threshold"], kw["n_cds"], kw["edge_distance"], kw["trim"],
                                  carry_state=kw["carry_state"])
            else:
                got = orc.segment_antismash(b["p"], b["ann"], b["cptr"], b["mptr"], b["mid"], kw["threshold"], kw["n_cds"],
                                            kw["n_biopfams"], kw["average_threshold"], kw["trim"], carry_state=kw["carry_state"])
            assert got.tolist() == exp, (b["name"], prm)


def test_object_refiner_equals_the_reference(batches):
    """`gecco_amd.refine.ClusterRefiner.iter_clusters` on gene objects: one call per contig, or one over all contigs when
    the grouper state is carried.  A planted antismash parameter set is checked on the contig of its run."""
    from gecco_amd.model import Cluster
    from gecco_amd.refine import ClusterRefiner

    for b in batches:
        ref = _ref(b)
        contigs = genes_from_planted(b)
        for prm in b["params"]:
            kw = refiner_params(prm)
            exp = _placed(ref(**kw))
            refiner = ClusterRefiner(cluster_type=Cluster, **{k: v for k, v in kw.items() if k != "carry_state"})
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                if kw["carry_state"]:
                    got = rows_from_clusters(refiner.iter_clusters([g for c in sorted(contigs) for g in contigs[c]]))
                elif "plant" in prm:
                    c = ref.stats(kw["threshold"], False, kw["trim"])[prm["plant"][0]]["row"][0]
                    got = rows_from_clusters(refiner.iter_clusters(contigs[c]))
                    exp = [r for r in exp if r[0] == c]
                else:
                    got = [r for c in sorted(contigs) for r in rows_from_clusters(refiner.iter_clusters(contigs[c]))]
            assert got == exp, (b["name"], prm)
