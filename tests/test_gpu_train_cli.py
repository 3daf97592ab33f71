"""``python -m gecco_amd.train`` on the device: the overlap join (gecco_crf_cluster_overlaps) against the pure-Python
restatement of the reference in tests/test_train_cli_host.py, the member-list compositions against
``composition.cluster_compositions``, and the whole front end against ``ClusterCRF.fit`` on genes built by cv's loaders."""
import os
import random
import subprocess
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_train_cli_host import planted, restate_assign, restate_labels, restate_members

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _check_join(genes, clusters):
    from gecco_amd import train_cli

    join = train_cli.join_clusters(genes, clusters)
    assert join.labels.dtype == np.uint8 and join.labels.tolist() == restate_labels(genes, clusters)
    members = restate_members(genes, clusters)
    for i in range(len(clusters)):
        assert join.members(i).tolist() == members[i], i
    assert int(join.member_ptr[-1]) == len(join.member_gene) == sum(len(v) for v in members.values())
    return join


def test_join_on_planted_boundaries():
    genes, clusters, labels, members = planted()
    join = _check_join(genes, clusters)
    assert join.labels.tolist() == labels


def _synthetic_coordinates(rng, n_genes, n_contigs, clusters_per_contig=4):
    """Genes of ``gecco_amd.synth`` contigs placed on coordinates (gaps and lengths drawn per gene, a few genes 20 times
    longer, equal starts now and then), sorted by (sequence, start, end); several clusters per contig, overlapping and
    nested, some contigs without any, and clusters on sequences no gene is on."""
    from gecco_amd import synth, tables

    lengths = synth.contig_lengths(rng, n_contigs, total_genes=n_genes)
    genes = []
    cl = {"sequence_id": [], "cluster_id": [], "start": [], "end": [], "type": []}
    for c, n in enumerate(lengths.tolist()):
        sid = f"contig{c:05d}"
        gap = rng.integers(-200, 400, size=n)
        length = rng.integers(100, 3000, size=n) * np.where(rng.random(n) < 0.01, 20, 1)
        start = 1 + np.cumsum(np.maximum(gap, 0) + np.where(rng.random(n) < 0.05, 0, 1))
        end = start + length
        order = np.lexsort((end, start))
        genes.extend(SimpleNamespace(source=SimpleNamespace(id=sid), start=int(start[i]), end=int(end[i])) for i in order)
        if c % 7 == 3 or n == 0:
            continue
        span = int(end.max())
        for k in range(int(rng.integers(1, clusters_per_contig + 1))):
            a = int(rng.integers(0, span))
            b = a + int(rng.integers(0, 60000))
            cl["sequence_id"].append(sid)
            cl["cluster_id"].append(f"{sid}_cluster_{k}")
            cl["start"].append(a)
            cl["end"].append(b)
            cl["type"].append("Polyketide")
    for k in range(3):
        cl["sequence_id"].append(f"absent{k}")
        cl["cluster_id"].append(f"absent{k}_cluster_1")
        cl["start"].append(1)
        cl["end"].append(10 ** 6)
        cl["type"].append("")
    genes.sort(key=lambda g: (g.source.id, g.start, g.end))
    return genes, tables.ClusterTable(cl)


def test_join_on_synthetic_tables():
    rng = np.random.default_rng(11)
    genes, clusters = _synthetic_coordinates(rng, 100_000, 400)
    assert 90_000 < len(genes) < 110_000
    join = _check_join(genes, clusters)
    assert 0 < int(join.labels.sum()) < len(genes)
    assert len(join.member_gene) > int(join.labels.sum())  # genes in several clusters are listed in each


def test_join_without_clusters_or_genes():
    from gecco_amd import tables

    rng = np.random.default_rng(12)
    genes, clusters = _synthetic_coordinates(rng, 5000, 20)
    empty = tables.ClusterTable()
    join = _check_join(genes, empty)
    assert not join.labels.any() and join.member_ptr.tolist() == [0]
    join = _check_join([], clusters)
    assert len(join.labels) == 0 and not join.member_ptr.any() and len(join.member_ptr) == len(clusters) + 1
    join = _check_join([], empty)
    assert len(join.labels) == 0 and join.member_ptr.tolist() == [0]


def test_join_refuses_unsorted_genes():
    from gecco_amd import _native

    with pytest.raises(ValueError, match="sorted by start"):
        _native.cluster_overlaps([0, 0, 0], [5, 1, 9], [6, 2, 10], [0, 1], [1], [3])
    with pytest.raises(ValueError, match="not sorted by start"):
        _native.cluster_overlaps([0], [1], [2], [0, 2], [5, 1], [6, 3])


def test_member_compositions_match_the_contiguous_kernel():
    """Random member lists (repeats, empty clusters, genes without domains) against ``composition.cluster_compositions``
    on clusters that list the same genes."""
    from gecco_amd import _native, composition, train_cli
    from gecco_amd.model import Cluster, Domain, Gene, Protein, Source, Strand

    rng = np.random.default_rng(13)
    names = [f"PF{k:05d}" for k in range(30)]
    genes = []
    for g in range(400):
        doms = [Domain(str(rng.choice(names + ["PFxxxxx"])), j, j + 5, "Pfam", 1e-5, float(rng.random() * 1e-3))
                for j in range(int(rng.integers(0, 5)))]
        genes.append(Gene(Source("s"), g, g + 1, Strand.Coding, Protein(f"p{g}", None, doms)))
    lists = [sorted(rng.choice(400, size=int(rng.integers(0, 40)), replace=False).tolist()) for _ in range(60)]
    lists[5] = []
    lists[7] = lists[7] + lists[7][:3]
    all_possible = sorted(rng.choice(names, size=20, replace=False).tolist())

    dom_ptr, dom_col, dom_w = train_cli.domain_rows(genes, all_possible)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    got = _native.domain_composition_members(ptr, [g for x in lists for g in x], dom_ptr, dom_col, dom_w, len(all_possible))
    exp = composition.cluster_compositions([Cluster(f"c{k}", [genes[g] for g in x]) for k, x in enumerate(lists)],
                                           all_possible)
    assert got.shape == exp.shape and got.tobytes() == exp.tobytes()


# ---------------------------------------------------------------------------------------------- the front end
def _golden_inputs(tmp_path):
    """The golden genes and features tables, with a clusters table over genes 6 to 15 of the 23 (the golden cluster
    covers them all, which leaves a single label) and a second, nested one."""
    from gecco_amd import tables

    g = tables.GeneTable.load(os.path.join(GOLDEN, "BGC0001866.genes.tsv"))
    starts, ends = np.asarray(g.start), np.asarray(g.end)
    order = np.argsort(starts, kind="stable")
    cl = tables.ClusterTable({"sequence_id": ["BGC0001866.1", "BGC0001866.1"],
                              "cluster_id": ["BGC0001866.1_cluster_1", "BGC0001866.1_cluster_0"],
                              "start": [int(starts[order[5]]), int(starts[order[8]])],
                              "end": [int(ends[order[14]]), int(ends[order[10]])],
                              "type": ["Polyketide", "NRP;Polyketide"]})
    cpath = str(tmp_path / "clusters.tsv")
    cl.dump(cpath)
    return os.path.join(GOLDEN, "BGC0001866.genes.tsv"), [os.path.join(GOLDEN, "BGC0001866.features.tsv")], cpath


def _synthetic_inputs(tmp_path, seed=23, n_seqs=24):
    """Multi-contig tables: a positive run on most contigs, clusters over the runs (a nested second one on some)."""
    from gecco_amd import tables
    from gecco_amd.model import Domain, Gene, Protein, Source, Strand

    rng = np.random.default_rng(seed)
    vocab = [f"PF{k:05d}" for k in range(40)]
    genes, cl = [], {"sequence_id": [], "cluster_id": [], "start": [], "end": [], "type": []}
    for c in range(n_seqs):
        src = Source(f"seq{c:02d}")
        n = int(rng.integers(20, 45))
        lab = np.zeros(n, dtype=int)
        runs = [] if c % 6 == 5 else [(a := int(rng.integers(0, n - 9)), a + int(rng.integers(4, 9)))]
        if c % 6 == 2:
            runs.append((a + 1, a + 3))  # nested in the first: its genes are in both
        for a, b in runs:
            lab[a:b] = 1
        for i in range(n):
            pool = vocab[16:] if lab[i] else vocab[:24]
            doms = [Domain(str(nm), 10 * j, 10 * j + 9, "Pfam", float(10.0 ** -rng.integers(3, 20)),
                           float(10.0 ** -rng.integers(5, 25))) for j, nm in enumerate(rng.choice(pool, size=int(rng.integers(1, 5))))]
            genes.append(Gene(src, 1000 * i + 1, 1000 * i + 900, Strand.Coding if i % 3 else Strand.Reverse,
                              Protein(f"{src.id}_g{i}", None, doms)))
        for k, (a, b) in enumerate(runs):
            cl["sequence_id"].append(src.id)
            cl["cluster_id"].append(f"{src.id}_cluster_{k + 1}")
            cl["start"].append(1000 * a + 1)
            cl["end"].append(1000 * (b - 1) + 900)
            cl["type"].append(["NRP", "Polyketide", "RiPP;NRP", "Unknown"][c % 4])
    gpath, fpath, cpath = str(tmp_path / "g.tsv"), str(tmp_path / "f.tsv"), str(tmp_path / "c.tsv")
    rng.shuffle(genes)  # (the front end sorts)
    tables.GeneTable.from_genes(genes).dump(gpath)
    tables.FeatureTable.from_genes(genes).dump(fpath)
    tables.ClusterTable(cl).dump(cpath)
    return gpath, [fpath], cpath


def _replay(gpath, fpaths, cpath, feature_type, select, shuffle, seed, p_filter=1e-9):
    """The reference's ``train`` by hand on Gene objects from cv's loaders: seed, annotate, sort, filter, label with
    ``cv.label_genes``, fit."""
    from gecco_amd import cv, tables
    from gecco_amd.crf import ClusterCRF

    random.seed(seed)
    np.random.seed(seed)
    genes = tables.GeneTable.load(gpath).to_genes()
    for f in fpaths:
        genes = cv.annotate_genes(genes, tables.FeatureTable.load(f))
    genes.sort(key=lambda g: (g.source.id, g.start, g.end))
    for g in genes:
        g.protein.domains.sort(key=lambda d: (d.start, d.end))
    genes = [g.with_protein(g.protein.with_domains([d for d in g.protein.domains if d.pvalue < p_filter])) for g in genes]
    clusters = tables.ClusterTable.load(cpath)
    genes = cv.label_genes(genes, clusters)
    crf = ClusterCRF(feature_type, "lbfgs", 5, 1, c1=0.15, c2=0.15)
    crf.fit(genes, select=select, shuffle=shuffle)
    return crf, genes, clusters


def _blob(state):
    """The CRFsuite model file inside a ``ClusterCRF`` record."""
    return state["model"].state["modelfile"].state["__FILE_RESOURCE_DATA__"]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("inputs", ["golden", "synthetic"])
@pytest.mark.parametrize("feature_type,select,shuffle", [("protein", None, True), ("protein", 0.5, False),
                                                         ("domain", None, False), ("domain", 0.5, True)])
def test_front_end_writes_the_model_fit_computes(tmp_path, monkeypatch, inputs, feature_type, select, shuffle):
    from gecco_amd import composition, pickle_model, predict, tables
    from gecco_amd.crf import ClusterCRF
    from gecco_amd.model import Cluster

    monkeypatch.setenv("GECCO_AMD_FIT", "native")
    gpath, fpaths, cpath = (_golden_inputs if inputs == "golden" else _synthetic_inputs)(tmp_path)
    out = tmp_path / "model"
    cmd = [sys.executable, "-m", "gecco_amd.train", "--genes", gpath, "--features", *fpaths, "--clusters", cpath,
           "--feature-type", feature_type, "--seed", "7", "-o", str(out)]
    cmd += (["--select", str(select)] if select is not None else []) + ([] if shuffle else ["--no-shuffle"])
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr
    assert "train:" in proc.stderr

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        crf, genes, clusters = _replay(gpath, fpaths, cpath, feature_type, select, shuffle, seed=7)
    ref = tmp_path / "ref"
    crf.save(str(ref))
    # the CRFsuite model inside the pickle is the same bytes (the pickles themselves may differ where they hold a
    # frozenset of names: its order follows the string hashes of the process)
    got_st = pickle_model.load_model_dir(str(out)).state  # (md5-checked)
    ref_st = pickle_model.load_model_dir(str(ref)).state
    assert _blob(got_st) == _blob(ref_st)
    assert got_st["significance"] == ref_st["significance"]
    assert got_st["significant_features"] == ref_st["significant_features"]
    assert (select is None) == (got_st["significant_features"] is None)
    if select is None:
        assert _read(out / "model.pkl") == _read(ref / "model.pkl")

    # type classifier files: the restatement's clusters, composed by the contiguous kernel
    assigned = restate_assign(genes, clusters)
    assert len(assigned) >= 1
    assert _read(out / "types.tsv") == "".join(f"{cid}\t{';'.join(names)}\r\n" for cid, _, names in assigned).encode()
    if select is not None:
        domains = sorted(crf.significant_features)
    else:
        domains = sorted({d.name for g in genes for d in g.protein.domains})
    assert _read(out / "domains.tsv") == "".join(f"{d}\n" for d in domains).encode()
    exp = composition.cluster_compositions([Cluster(cid, [genes[i] for i in idx]) for cid, idx, _ in assigned], domains)
    with np.load(out / "compositions.npz") as z:
        assert z["format"].item() == b"coo" and tuple(z["shape"]) == exp.shape
        got = np.zeros(exp.shape)
        got[z["row"], z["col"]] = z["data"]
    assert got.tobytes() == exp.tobytes()
    trans = _read(out / "model.trans.tsv").decode().split("\r\n")
    assert trans[0] == "from\tto\tweight" and len(trans) == len(crf.model.transition_features_) + 2

    # the directory loads, and the columnar predict front end reproduces the in-memory model
    loaded = ClusterCRF.trained(str(out))
    assert loaded.feature_type == feature_type and loaded.significant_features == crf.significant_features
    if feature_type == "protein":
        pred = tmp_path / "pred"
        proc = subprocess.run([sys.executable, "-m", "gecco_amd.predict", "--genes", gpath, "--features", fpaths[0],
                               "--model", str(out), "-o", str(pred)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert proc.returncode == 0, proc.stderr
        base = os.path.splitext(os.path.basename(gpath))[0]
        base = base[:-len(".genes")] if base.endswith(".genes") else base
        written = tables.GeneTable.load(str(pred / f"{base}.genes.tsv"))
        feats = predict.filter_features(tables.FeatureTable.load(fpaths[0]), None, 1e-9)
        mem, _, _ = predict.predict_tables(tables.GeneTable.load(gpath), feats, crf)
        assert list(written.protein_id) == list(mem.protein_id)
        assert np.asarray(written.average_p).tobytes() == np.asarray(mem.average_p, dtype=np.float64).tobytes()
