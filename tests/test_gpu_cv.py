"""Cross-validation on the device (gecco_amd/cv.py): every fold of ``cross_validate`` is bit for bit the reference's order
of operations replayed by hand with ``ClusterCRF.fit`` / ``predict_probabilities``, and ``python -m gecco_amd.cv`` writes
what the API computes."""
import os
import random
import subprocess
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ["NRP", "Polyketide", "RiPP", "NRP;Polyketide", "Unknown", "Terpene"]


def _dataset(seed=29, n_seqs=30, vocab_size=40):
    """Labelled genes of ``n_seqs`` sequences (one positive run on most of them) and the clusters table of the runs."""
    from gecco_amd import tables
    from gecco_amd.model import Domain, Gene, Protein, Source, Strand

    rng = np.random.default_rng(seed)
    vocab = [f"PF{k:05d}" for k in range(vocab_size)]
    half = vocab_size // 2
    genes, clusters = [], {"sequence_id": [], "cluster_id": [], "start": [], "end": [], "type": []}
    for c in range(n_seqs):
        src = Source(f"seq{c:02d}")
        n = int(rng.integers(20, 45))
        lab = np.zeros(n, dtype=int)
        if c % 5 != 4:
            a = int(rng.integers(0, n - 8))
            lab[a:a + int(rng.integers(4, 9))] = 1
        for i in range(n):
            k = int(rng.integers(0, 4))
            pool = vocab[half - 4:] if lab[i] else vocab[:half + 4]
            doms = [Domain(str(nm), 10 * j, 10 * j + 9, "Pfam", 1e-5, 1e-6, probability=float(lab[i]))
                    for j, nm in enumerate(rng.choice(pool, size=k))]
            genes.append(Gene(src, 1000 * i + 1, 1000 * i + 900, Strand.Coding if i % 3 else Strand.Reverse,
                              Protein(f"seq{c:02d}_g{i}", None, doms), _probability=float(lab[i])))
        if lab.any():
            idx = np.flatnonzero(lab)
            clusters["sequence_id"].append(src.id)
            clusters["cluster_id"].append(f"{src.id}_cluster_1")
            clusters["start"].append(1000 * int(idx[0]) + 1)
            clusters["end"].append(1000 * int(idx[-1]) + 900)
            clusters["type"].append(TYPES[c % len(TYPES)])
    return genes, tables.ClusterTable(clusters)


def _template():
    from gecco_amd.crf import ClusterCRF

    return ClusterCRF("protein", window_size=5, window_step=1, c1=0.15, c2=0.15)


def _splitter(loto, clusters, k=5):
    from gecco_amd import cv

    if loto:
        return lambda seqs: list(cv.LeaveOneGroupOut().split(seqs, groups=cv.loto_groups(seqs, clusters)))
    return lambda seqs: cv.kfold_splits(len(seqs), k)


def _replay(genes, splitter, shuffle, select, seed):
    """The reference's cv loop, by hand: group and shuffle, then per fold fit and predict."""
    from gecco_amd import cv

    random.seed(seed)
    seqs = cv.group_genes(genes, shuffle=shuffle)
    out = []
    for train_idx, test_idx in splitter(seqs):
        crf = _template()
        crf.fit([g for i in train_idx for g in seqs[i]], shuffle=shuffle, select=select)
        out.append((crf, crf.predict_probabilities([cv._test_copy(g) for i in test_idx for g in seqs[i]])))
    return out


def _model_bytes(crf, path):
    crf.save(path)
    with open(os.path.join(path, "model.pkl"), "rb") as f:
        return f.read()


@pytest.mark.parametrize("loto,shuffle,select", [(False, True, None), (False, False, None), (True, True, None),
                                                 (True, False, None), (False, True, 0.5), (True, True, 0.5)])
def test_cross_validate_replays_the_reference_order(tmp_path, monkeypatch, loto, shuffle, select):
    from gecco_amd import cv

    monkeypatch.setenv("GECCO_AMD_FIT", "native")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        genes, clusters = _dataset()
        expected = _replay(genes, _splitter(loto, clusters), shuffle, select, seed=5)
        genes, clusters = _dataset()
        random.seed(5)
        result = cv.cross_validate(_template(), genes, _splitter(loto, clusters), shuffle=shuffle, select=select)
    assert len(result.folds) == len(expected) >= 3
    for fold, (crf, predicted) in zip(result.folds, expected):
        a, b = fold.crf.training_result_, crf.training_result_
        assert (a.n_iter, a.n_eval, a.status) == (b.n_iter, b.n_eval, b.status) and a.n_iter > 0
        assert np.float64(a.f).tobytes() == np.float64(b.f).tobytes() and a.x.tobytes() == b.x.tobytes()
        assert fold.crf.significant_features == crf.significant_features
        assert fold.crf.significance == crf.significance
        assert (_model_bytes(fold.crf, str(tmp_path / f"a{fold.index}"))
                == _model_bytes(crf, str(tmp_path / f"b{fold.index}")))
        assert [cv._gene_key(g) for g in fold.predicted] == [cv._gene_key(g) for g in predicted]
        pa = np.array([g.average_probability for g in fold.predicted])
        pb = np.array([g.average_probability for g in predicted])
        assert pa.tobytes() == pb.tobytes()
        # the truth is the label of the same gene
        labels = {cv._gene_key(g): g.average_probability > 0.5 for g in genes}
        assert fold.truth == [labels[cv._gene_key(g)] for g in fold.predicted]
    if loto:
        assert len(result.folds) == 4  # NRP, Polyketide, RiPP, Terpene (Unknown and unlabelled sequences: no group)
        assert [len(f.test) for f in result.folds] == [4, 4, 4, 4]
    # the whole-run metrics are over the joined pairs
    labels = [t for f in result.folds for t in f.truth]
    probas = [g.average_probability for f in result.folds for g in f.predicted]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert result.auroc == cv.roc_auc(labels, probas) and result.aupr == cv.average_precision(labels, probas)
    assert 0.5 < result.auroc <= 1.0


@pytest.mark.parametrize("loto", [False, True])
def test_front_end_writes_what_the_api_computes(tmp_path, loto):
    from gecco_amd import cv, tables

    genes, clusters = _dataset(seed=31)
    gpath, fpath, cpath = tmp_path / "g.tsv", tmp_path / "f.tsv", tmp_path / "c.tsv"
    tables.GeneTable.from_genes(genes).dump(str(gpath))
    tables.FeatureTable.from_genes(genes).dump(str(fpath))
    clusters.dump(str(cpath))
    out = tmp_path / "cv.tsv"
    cmd = [sys.executable, "-m", "gecco_amd.cv", "--genes", str(gpath), "--features", str(fpath), "--clusters",
           str(cpath), "--splits", "4", "--seed", "7", "-o", str(out)] + (["--loto"] if loto else [])
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600,
                          env={**os.environ, "GECCO_AMD_FIT": "native"})
    assert proc.returncode == 0, proc.stderr
    assert "cross-validation: AUROC=" in proc.stderr and "fold 1: AUROC=" in proc.stderr

    random.seed(7)
    np.random.seed(7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded = cv.label_genes(cv.annotate_genes(tables.GeneTable.load(str(gpath)).to_genes(),
                                                  tables.FeatureTable.load(str(fpath))), tables.ClusterTable.load(str(cpath)))
        crf = _template()
        res = cv.cross_validate(crf, loaded, _splitter(loto, tables.ClusterTable.load(str(cpath)), k=4))
    text = out.read_bytes()
    assert text == res.table()
    lines = text.decode().splitlines()
    assert lines[0].endswith("\tfold\tis_cluster")
    assert {ln.rsplit("\t", 1)[1] for ln in lines[1:]} == {"true", "false"}
    assert len(lines) - 1 == sum(len(f.predicted) for f in res.folds)


def test_loto_groups_split_types_and_refuse_several_clusters():
    from gecco_amd import cv, tables
    from gecco_amd.model import Gene, Protein, Source, Strand

    def seq(name):
        return [Gene(Source(name), 1, 100, Strand.Coding, Protein(f"{name}_1", None))]

    t = tables.ClusterTable({"sequence_id": ["a", "b", "c"], "cluster_id": ["a1", "b1", "c1"], "start": [1, 1, 1],
                             "end": [9, 9, 9], "type": ["NRP;Polyketide", "Unknown", "RiPP"]})
    assert cv.loto_groups([seq("a"), seq("b"), seq("c"), seq("d")], t) == [["NRP", "Polyketide"], [], ["RiPP"], []]
    t2 = tables.ClusterTable({"sequence_id": ["a", "a"], "cluster_id": ["a1", "a2"], "start": [1, 20], "end": [9, 30],
                              "type": ["NRP", "RiPP"]})
    with pytest.raises(ValueError, match="several clusters per sequence"):
        cv.loto_groups([seq("a")], t2)
