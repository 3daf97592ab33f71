"""The training front end without a device (gecco_amd/train_cli.py): GECCO's argument defaults, the byte formats of the
model directory's text files, the COO layout of compositions.npz, and a pure-Python restatement of the reference's
overlap join (``_common.label_genes``, ``train._assign_clusters``) on planted boundary cases.  The restatement is what
tests/test_gpu_train_cli.py holds the device join to."""
import collections
import itertools
import operator
from types import SimpleNamespace

import numpy as np
import pytest


# ---------------------------------------------------------------------------------------------- the restatement
def restate_labels(genes, clusters):
    """``_common.label_genes``: 1 for a gene overlapping any cluster of its sequence (bounds inclusive), else 0."""
    by_seq = collections.defaultdict(list)
    for i in range(len(clusters)):
        by_seq[str(clusters.sequence_id[i])].append((int(clusters.start[i]), int(clusters.end[i])))
    out = []
    for seq_id, seq_genes in itertools.groupby(genes, key=operator.attrgetter("source.id")):
        for gene in seq_genes:
            out.append(1 if any(cs <= gene.end and gene.start <= ce for cs, ce in by_seq[seq_id]) else 0)
    return out


def restate_members(genes, clusters):
    """``train._assign_clusters`` up to the Cluster objects: per clusters-table row, the indices of its genes in gene
    order."""
    by_seq = collections.defaultdict(list)
    for i in range(len(clusters)):
        by_seq[str(clusters.sequence_id[i])].append((int(clusters.start[i]), int(clusters.end[i]), i))
    members = {i: [] for i in range(len(clusters))}
    for g, gene in enumerate(genes):
        for cs, ce, i in by_seq[gene.source.id]:
            if cs <= gene.end and gene.start <= ce:
                members[i].append(g)
    return members


def restate_assign(genes, clusters):
    """``(cluster_id, member indices, type names)`` of every cluster with genes, in sorted id order."""
    members = restate_members(genes, clusters)
    row = {str(cid): i for i, cid in enumerate(clusters.cluster_id)}
    out = []
    for cid in sorted(filter(None, (str(c) for c in clusters.cluster_id))):
        i = row[cid]
        if members[i]:
            t = clusters.type[i]
            names = () if t in (None, "", "Unknown") else tuple(sorted(frozenset(str(t).split(";"))))
            out.append((cid, members[i], names))
    return out


def _gene(sid, start, end):
    return SimpleNamespace(source=SimpleNamespace(id=sid), start=start, end=end)


def planted():
    """Three sequences with genes and a fourth with a cluster only.  seqA: nested and overlapping clusters (A2 inside A1,
    A3 across A1's end), a gene ending on A1's start, one starting on A1's end, one a base before A1, one a base after A3,
    one spanning everything, and one inside A1 behind the end of A2 (found only through the running maximum of the
    cluster ends).  seqB: genes, no clusters.  seqC: a cluster no gene reaches.  seqD: a cluster, no genes."""
    from gecco_amd import tables

    genes = [
        _gene("seqA", 1, 100),      # 0: before everything
        _gene("seqA", 50, 2000),    # 1: spans A1, A2, A3
        _gene("seqA", 150, 300),    # 2: ends on A1's start
        _gene("seqA", 200, 299),    # 3: one base before A1
        _gene("seqA", 400, 500),    # 4: A1 and A2 (nested)
        _gene("seqA", 460, 470),    # 5: A1 only, past A2's end
        _gene("seqA", 600, 620),    # 6: starts on A1's end; A3 too
        _gene("seqA", 901, 1000),   # 7: one base after A3 -- but the spanning gene is no cluster: none
        _gene("seqB", 1, 100),
        _gene("seqB", 200, 300),
        _gene("seqC", 1, 100),
        _gene("seqC", 7000, 8000),
    ]
    clusters = tables.ClusterTable({
        "sequence_id": ["seqA", "seqD", "seqA", "seqC", "seqA"],
        "cluster_id": ["seqA_c3", "seqD_c1", "seqA_c1", "seqC_c1", "seqA_c2"],
        "start": [580, 1, 300, 5000, 400],
        "end": [900, 100, 600, 6000, 450],
        "type": ["", "Terpene", "Polyketide;NRP", "RiPP", "Unknown"],
    })
    labels = [0, 1, 1, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    members = {0: [1, 6], 1: [], 2: [1, 2, 4, 5, 6], 3: [], 4: [1, 4]}
    return genes, clusters, labels, members


def test_restatement_on_planted_boundaries():
    genes, clusters, labels, members = planted()
    assert restate_labels(genes, clusters) == labels
    assert restate_members(genes, clusters) == members
    assert restate_assign(genes, clusters) == [("seqA_c1", [1, 2, 4, 5, 6], ("NRP", "Polyketide")),
                                               ("seqA_c2", [1, 4], ()), ("seqA_c3", [1, 6], ())]


def test_restatement_matches_the_cv_labeller():
    from gecco_amd import cv
    from gecco_amd.model import Gene, Protein, Source, Strand

    genes, clusters, labels, _ = planted()
    objs = [Gene(Source(g.source.id), g.start, g.end, Strand.Coding, Protein(f"p{i}", None)) for i, g in enumerate(genes)]
    assert [g.average_probability for g in cv.label_genes(objs, clusters)] == labels


def _join_from_restatement(genes, clusters):
    from gecco_amd import train_cli

    members = restate_members(genes, clusters)
    ptr = np.zeros(len(clusters) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(members[i]) for i in range(len(clusters))])
    flat = np.array([g for i in range(len(clusters)) for g in members[i]], dtype=np.int32)
    return train_cli.ClusterJoin(np.array(restate_labels(genes, clusters), dtype=np.uint8), np.arange(len(clusters)),
                                 ptr, flat)


def test_assigned_clusters_follow_the_reference():
    from gecco_amd import tables, train_cli

    genes, clusters, _, _ = planted()
    join = _join_from_restatement(genes, clusters)
    got = [(cid, join.members(i).tolist(), names) for cid, i, names in train_cli.assigned_clusters(clusters, join)]
    assert got == restate_assign(genes, clusters)
    dup = tables.ClusterTable({"sequence_id": ["seqA", "seqA"], "cluster_id": ["x", "x"], "start": [1, 5], "end": [2, 9],
                               "type": ["", ""]})
    with pytest.raises(ValueError, match="duplicate cluster id"):
        train_cli.assigned_clusters(dup, _join_from_restatement(genes, dup))


def test_type_names():
    from gecco_amd.train_cli import type_names

    assert type_names("Unknown") == () and type_names("") == () and type_names(None) == ()
    assert type_names("Polyketide;NRP;Polyketide") == ("NRP", "Polyketide")


# ---------------------------------------------------------------------------------------------- arguments
def test_argument_defaults_are_gecco_s():
    from gecco_amd.train_cli import build_parser

    args = build_parser().parse_args(["-g", "G.tsv", "-f", "F.tsv", "-c", "C.tsv"])
    assert vars(args) == {
        "genes": "G.tsv", "features": ["F.tsv"], "clusters": "C.tsv", "output_dir": ".", "e_filter": None,
        "p_filter": 1e-9, "feature_type": "protein", "window_size": 5, "window_step": 1, "c1": 0.15, "c2": 0.15,
        "select": None, "correction": None, "shuffle": True, "seed": 42, "jobs": 0,
    }
    args = build_parser().parse_args(["--genes", "G", "--features", "F1", "F2", "-f", "F3", "--clusters", "C", "-o", "D",
                                      "-e", "1e-5", "-p", "1e-3", "--feature-type", "domain", "-W", "7", "--window-step",
                                      "2", "--c1", "0", "--c2", "1", "--select", "0.25", "--correction", "fdr_bh",
                                      "--no-shuffle", "--seed", "3", "-j", "4"])
    assert args.features == ["F1", "F2", "F3"] and args.output_dir == "D" and args.e_filter == 1e-5
    assert (args.p_filter, args.feature_type, args.window_size, args.window_step) == (1e-3, "domain", 7, 2)
    assert (args.c1, args.c2, args.select, args.correction, args.shuffle, args.seed, args.jobs) == (0.0, 1.0, 0.25, "fdr_bh",
                                                                                                     False, 3, 4)


def test_train_module_is_the_front_end():
    from gecco_amd import train, train_cli

    with pytest.raises(SystemExit) as err:
        train.main(["--help"])
    assert err.value.code == 0
    assert train_cli.main.__doc__ and "type" in train_cli.main.__doc__


# ---------------------------------------------------------------------------------------------- file formats
class _FakeCRF:
    def __init__(self, trans, state, significant=None):
        self.model = SimpleNamespace(transition_features_=trans, state_features_=state)
        self.significant_features = significant


def test_text_files_are_byte_exact(tmp_path):
    from gecco_amd import train_cli

    crf = _FakeCRF({("0", "0"): 2.5, ("0", "1"): -1.25, ("1", "0"): -0.1, ("1", "1"): 3.0},
                   {("PF00001", "0"): 0.75, ("PF00001", "1"): -0.75, ("PF00002", "1"): 1e-07})
    train_cli.write_weight_tables(str(tmp_path), crf)
    genes, clusters, _, _ = planted()
    join = _join_from_restatement(genes, clusters)
    train_cli.write_type_labels(str(tmp_path), ["PF00001", "PF00002", "PF00003"],
                                train_cli.assigned_clusters(clusters, join))
    expected = {
        "model.trans.tsv": b"from\tto\tweight\r\n0\t0\t2.5\r\n0\t1\t-1.25\r\n1\t0\t-0.1\r\n1\t1\t3.0\r\n",
        "model.state.tsv": b"attr\tlabel\tweight\r\nPF00001\t0\t0.75\r\nPF00001\t1\t-0.75\r\nPF00002\t1\t1e-07\r\n",
        "domains.tsv": b"PF00001\nPF00002\nPF00003\n",
        "types.tsv": b"seqA_c1\tNRP;Polyketide\r\nseqA_c2\t\r\nseqA_c3\t\r\n",
    }
    for name, data in expected.items():
        with open(tmp_path / name, "rb") as f:
            assert f.read() == data, name


def test_composition_domains():
    from gecco_amd.train_cli import composition_domains

    genes = [SimpleNamespace(protein=SimpleNamespace(domains=[SimpleNamespace(name=n) for n in names]))
             for names in (["PF3", "PF1"], [], ["PF1", "PF2"])]
    assert composition_domains(_FakeCRF({}, {}), genes) == ["PF1", "PF2", "PF3"]
    assert composition_domains(_FakeCRF({}, {}, frozenset({"PF9", "PF2"})), genes) == ["PF2", "PF9"]


@pytest.mark.parametrize("shape", [(3, 4), (0, 4), (2, 0), (1, 1)])
def test_compositions_npz_is_scipy_s_coo_layout(tmp_path, shape):
    from gecco_amd.train_cli import save_npz_coo

    rng = np.random.default_rng(sum(shape))
    dense = rng.random(shape) * (rng.random(shape) < 0.5)
    path = str(tmp_path / "compositions.npz")
    save_npz_coo(path, dense)
    with np.load(path) as z:
        assert sorted(z.files) == ["col", "data", "format", "row", "shape"]
        assert z["format"].item() == b"coo" and tuple(z["shape"]) == shape
        back = np.zeros(shape)
        back[z["row"], z["col"]] = z["data"]
    assert back.tobytes() == dense.tobytes()
    sparse = pytest.importorskip("scipy.sparse")
    assert sparse.load_npz(path).toarray().tobytes() == dense.tobytes()
    ref = str(tmp_path / "ref.npz")
    sparse.save_npz(ref, sparse.coo_matrix(dense))
    with np.load(path) as a, np.load(ref) as b:
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
