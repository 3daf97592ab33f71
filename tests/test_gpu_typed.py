"""The typed cluster CRF end to end on a planted set: three cluster types with vocabularies of their own, one cluster of
two types (a composite label), 12 training contigs of 150 genes with two 12-gene clusters each.  The fitted model's calls
on fresh contigs against the numpy yardstick + the host refiner, against the planted truth, through the model directory
and through the command line; and the 2-label degenerate case against ``ClusterCRF``."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import typed_yardstick as ty
from tests.typed_planted import C, TYPES, W, cluster_table as _cluster_table, planted_set as _set

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_tables(directory, genes, rows=None):
    from gecco_amd import tables

    os.makedirs(directory, exist_ok=True)
    tables.GeneTable.from_genes(genes).dump(os.path.join(directory, "genes.tsv"))
    tables.FeatureTable.from_genes(genes).dump(os.path.join(directory, "features.tsv"))
    if rows is not None:
        _cluster_table(rows).dump(os.path.join(directory, "clusters.tsv"))


def _load(directory):
    from gecco_amd.train_cli import load_training_genes

    return load_training_genes(os.path.join(directory, "genes.tsv"), [os.path.join(directory, "features.tsv")], None, 1e-9)


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """The tables of the training and of the fresh set, the model fitted on the former (seeded as the command line seeds
    it) and its calls on the latter."""
    from gecco_amd import tables, typed

    base = tmp_path_factory.mktemp("typed")
    train_genes, train_rows = _set(11, 12, "train", composite=True)
    fresh_genes, fresh_rows = _set(12, 4, "fresh", composite=False)
    _write_tables(str(base / "train"), train_genes, train_rows)
    _write_tables(str(base / "fresh"), fresh_genes)
    random.seed(42)
    np.random.seed(42)
    crf = typed.TypedClusterCRF(W, 1, c1=C, c2=C)
    crf.fit(_load(str(base / "train")), tables.ClusterTable.load(str(base / "train" / "clusters.tsv")))
    genes = _load(str(base / "fresh"))
    annotated, clusters = crf.predict_genes_and_clusters(genes)
    return {"base": base, "crf": crf, "fresh_rows": fresh_rows, "annotated": annotated, "clusters": clusters}


def _rows(clusters):
    return [(c.id, [g.id for g in c.genes], str(c.type)) for c in clusters]


def test_labels_of_the_planted_set(planted):
    crf = planted["crf"]
    assert crf.classes_[0] == "0" and sorted(crf.classes_) == sorted(["0", "Alpha", "Beta", "Gamma", "Alpha;Beta"])
    assert crf.types_ == TYPES
    assert crf.label_types_[crf.classes_.index("Alpha;Beta")] == ("Alpha", "Beta")


def test_calls_equal_yardstick_and_host_refiner(planted):
    import itertools

    from gecco_amd import packing
    from gecco_amd.refine import ClusterRefiner

    crf = planted["crf"]
    genes = _load(str(planted["base"] / "fresh"))
    contigs = [list(g) for _, g in itertools.groupby(genes, key=lambda g: g.source.id)]
    batch = packing.pack_contigs(contigs, crf._attr_index, "protein")
    w, trans = crf._model.state_weights()[0], crf._model.trans_weights()[0]
    bg = crf.classes_.index("0")
    e_all, e_any = ty.windowed_all(w, trans, batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id,
                                   W, 1, bg, True)
    p_all = crf.predict_label_probabilities(genes)
    assert p_all.shape == e_all.shape and np.abs(p_all - e_all).max() <= 1e-12
    got_any = np.array([g.average_probability for g in planted["annotated"]])
    assert np.abs(got_any - e_any).max() <= 1e-12
    index = {g.id: k for k, g in enumerate(genes)}
    scored = [g.with_probability(float(p)) for g, p in zip(genes, e_any)]
    refiner = ClusterRefiner(threshold=0.8, criterion="gecco", n_cds=3, edge_distance=0, trim=True)
    expected = []
    for _, group in itertools.groupby(scored, key=lambda g: g.source.id):
        expected.extend(refiner.iter_clusters(list(group)))
    clusters = planted["clusters"]
    assert [(c.id, [g.id for g in c.genes]) for c in clusters] == [(c.id, [g.id for g in c.genes]) for c in expected]
    assert len(clusters) >= 8
    for got, exp in zip(clusters, expected):
        rows = [index[g.id] for g in exp.genes]
        proba = ty.type_probabilities(e_all[rows], crf.label_types_, crf.types_)
        assert sorted(got.type_probabilities) == TYPES
        for t in TYPES:
            assert abs(got.type_probabilities[t] - proba[t]) <= 1e-12, (got.id, t)
        assert got.type.names == frozenset(t for t in TYPES if proba[t] > 0.5)


def test_every_planted_cluster_is_called_once_with_its_type(planted):
    clusters = planted["clusters"]
    for cid, seq, start, end, type_, _ in planted["fresh_rows"]:
        over = [c for c in clusters if c.source.id == seq and c.start <= end and start <= c.end]
        assert len(over) == 1, (cid, [c.id for c in over])
        assert str(over[0].type) == type_, (cid, str(over[0].type), over[0].type_probabilities)


def test_model_directory_gives_the_same_bits(planted, tmp_path):
    from gecco_amd import typed

    crf = planted["crf"]
    crf.save(tmp_path)
    back = typed.TypedClusterCRF.trained(tmp_path)
    genes = _load(str(planted["base"] / "fresh"))
    assert np.array_equal(back.predict_label_probabilities(genes), crf.predict_label_probabilities(genes))
    annotated, clusters = back.predict_genes_and_clusters(genes)
    assert [g.average_probability for g in annotated] == [g.average_probability for g in planted["annotated"]]
    assert _rows(clusters) == _rows(planted["clusters"])
    assert [c.type_probabilities for c in clusters] == [c.type_probabilities for c in planted["clusters"]]


def test_command_line_train_then_predict(planted, tmp_path):
    from gecco_amd import tables

    base = planted["base"]
    model_dir, out_dir = str(tmp_path / "model"), str(tmp_path / "out")
    run = [sys.executable, "-m", "gecco_amd.typed"]
    done = subprocess.run(run + ["train", "--genes", str(base / "train" / "genes.tsv"), "--features",
                                 str(base / "train" / "features.tsv"), "--clusters", str(base / "train" / "clusters.tsv"),
                                 "-W", str(W), "--c1", str(C), "--c2", str(C), "-o", model_dir], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert open(os.path.join(model_dir, "typed_model.crfsuite"), "rb").read() == planted["crf"]._blob
    done = subprocess.run(run + ["predict", "--model", model_dir, "--genes", str(base / "fresh" / "genes.tsv"), "--features",
                                 str(base / "fresh" / "features.tsv"), "-o", out_dir], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    for name in ("genes.tsv", "features.tsv", "clusters.tsv"):
        assert os.path.exists(os.path.join(out_dir, name))
    table = tables.ClusterTable.load(os.path.join(out_dir, "clusters.tsv"))
    clusters = planted["clusters"]
    assert [str(v) for v in table.cluster_id] == [c.id for c in clusters]
    assert [str(v) for v in table.type] == [str(c.type) for c in clusters]
    with open(os.path.join(out_dir, "clusters.tsv")) as fh:
        header = fh.readline().rstrip("\n").split("\t")
        cells = [line.rstrip("\n").split("\t") for line in fh]
    for t in TYPES:
        col = f"{t.lower()}_probability"
        assert col in table.columns and col in header
        assert [row[header.index(col)] for row in cells] == [tables._fmt(c.type_probabilities[t]) for c in clusters]
    genes = tables.GeneTable.load(os.path.join(out_dir, "genes.tsv"))
    assert [tables._fmt(float(v)) for v in genes.average_p] == [tables._fmt(g.average_probability) for g in planted["annotated"]]


def test_two_label_case_against_cluster_crf(monkeypatch):
    """All clusters ``Unknown``: the labels are ``0`` and ``Unknown``, and the fit is ``ClusterCRF``'s native fit on the same
    genes and labels (the same shuffle: ``random`` seeded alike).  The probabilities agree to 1e-12: the weights come from
    the same 2-label trainer, the probabilities from `gl_all_small` here and from the 2-label window kernel there
    (measured: max |dp| = 5.6e-16, so not bit for bit)."""
    from gecco_amd import typed
    from gecco_amd.crf import ClusterCRF

    monkeypatch.setenv("GECCO_AMD_FIT", "native")
    train_genes, rows = _set(21, 6, "two", composite=False)
    fresh, _ = _set(22, 2, "new", composite=False)
    table = _cluster_table(rows, ["Unknown"] * len(rows))
    random.seed(7)
    crf = typed.TypedClusterCRF(W, 1, c1=C, c2=C).fit(train_genes, table)
    assert crf.classes_ == ["0", "Unknown"] and crf.types_ == []
    inside = set()
    for _, seq, start, end, _, _ in rows:
        inside.update(g.id for g in train_genes if g.source.id == seq and g.start <= end and start <= g.end)
    labelled = [g.with_probability(1.0 if g.id in inside else 0.0) for g in train_genes]
    random.seed(7)
    ref = ClusterCRF("protein", "lbfgs", W, 1, c1=C, c2=C)
    ref.reference_bits = False
    ref.fit(labelled)
    got = np.array([g.average_probability for g in crf.predict_probabilities(fresh)])
    exp = np.array([g.average_probability for g in ref.predict_probabilities(fresh)])
    assert np.abs(got - exp).max() <= 1e-12
    clusters = crf.predict_clusters(fresh)
    assert clusters and all(str(c.type) == "Unknown" and c.type_probabilities == {} for c in clusters)


def test_fit_with_fisher_selection(monkeypatch):
    """``fit(select=...)`` is ``ClusterCRF.fit(select=...)`` on the in-cluster / background labels: the same significance,
    the same selected domains, and a model that knows no other domain."""
    from gecco_amd import typed
    from gecco_amd.crf import ClusterCRF

    monkeypatch.setenv("GECCO_AMD_FIT", "native")
    train_genes, rows = _set(31, 6, "sel", composite=False)
    random.seed(9)
    crf = typed.TypedClusterCRF(W, 1, c1=C, c2=C).fit(train_genes, _cluster_table(rows), select=0.5)
    inside = set()
    for _, seq, start, end, _, _ in rows:
        inside.update(g.id for g in train_genes if g.source.id == seq and g.start <= end and start <= g.end)
    random.seed(9)
    ref = ClusterCRF("protein", "lbfgs", W, 1, c1=C, c2=C)
    ref.fit([g.with_probability(1.0 if g.id in inside else 0.0) for g in train_genes], select=0.5)
    assert crf.significance == ref.significance and crf.significant_features == ref.significant_features
    assert 0 < len(crf.significant_features) < 54 and set(crf._attr_index) <= set(crf.significant_features)
    assert sorted(crf.classes_) == sorted(["0"] + TYPES)
    assert crf.predict_clusters(_set(32, 1, "new", composite=False)[0])
