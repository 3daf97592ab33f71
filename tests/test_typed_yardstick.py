"""The yardstick of the all-label windowed marginals (tests/typed_yardstick.py) pinned against the CPU oracle and
brute-force path enumeration, and the host rules of the typed cluster CRF (gecco_amd/typed.py): labels from a clusters
table, the fold to "Mixed", the type-probability rule and the model directory.  No GPU."""
import hashlib
import json
import os
import warnings

import numpy as np
import pytest

from tests import typed_yardstick as ty
from tests.helpers import synth_contigs


def _join(members, n_genes):
    """A ``train_cli.ClusterJoin`` made by hand: ``members[i]`` = the genes of clusters-table row i."""
    from gecco_amd.train_cli import ClusterJoin

    ptr = np.zeros(len(members) + 1, dtype=np.int64)
    np.cumsum([len(m) for m in members], out=ptr[1:])
    gene = np.array([g for m in members for g in m], dtype=np.int64)
    labels = np.zeros(n_genes, dtype=np.int32)
    labels[gene] = 1
    return ClusterJoin(labels, np.arange(len(members)), ptr, gene)


def _table(ids, types):
    from gecco_amd import tables

    n = len(ids)
    return tables.ClusterTable({"sequence_id": ["s"] * n, "cluster_id": list(ids), "start": [1] * n, "end": [2] * n,
                                "type": list(types)})


# ---- the yardstick itself
def test_yardstick_columns_are_the_oracle_and_p_any_is_brute_force():
    from oracle import crf_oracle as orc

    rng = np.random.default_rng(5)
    A, L, W = 12, 3, 4
    w = rng.normal(0, 1.5, size=(A, L))
    trans = rng.normal(0, 1.0, size=(L, L))
    cptr, gptr, attr = synth_contigs(rng, [7], A)
    for background in (0, 2):
        p_all, p_any = ty.windowed_all(w, trans, cptr, gptr, attr, W, 1, background, True)
        for l in range(L):
            exp = orc.windowed_marginals(w, trans, cptr, gptr, attr, W, 1, l, True)
            assert np.abs(p_all[:, l] - exp).max() <= 1e-15
        state = orc.state_scores(w, gptr, attr)
        brute = np.zeros(7)
        for s in range(7 - W + 1):
            marg, _ = orc.brute_marginals(state[s:s + W], trans)
            keep = [l for l in range(L) if l != background]
            brute[s:s + W] = np.maximum(brute[s:s + W], marg[:, keep].sum(axis=1))
        assert np.abs(p_any - brute).max() <= 1e-13
    assert ty.windowed_all(w, trans, cptr, gptr, attr, W, 1, None, True)[1] is None


def test_yardstick_padding_skipping_and_steps():
    from oracle import crf_oracle as orc

    rng = np.random.default_rng(6)
    A, L, W = 20, 4, 5
    w = rng.normal(0, 1.5, size=(A, L))
    trans = rng.normal(0, 1.0, size=(L, L))
    cptr, gptr, attr = synth_contigs(rng, [0, 2, 5, 11, 0, 3], A)
    for step, pad in ((1, True), (2, True), (5, False), (3, False)):
        p_all, p_any = ty.windowed_all(w, trans, cptr, gptr, attr, W, step, 0, pad)
        for l in range(L):
            exp = orc.windowed_marginals(w, trans, cptr, gptr, attr, W, step, l, pad)
            assert np.array_equal(np.isnan(exp), np.isnan(p_all[:, l]))
            ok = ~np.isnan(exp)
            assert np.abs(p_all[ok, l] - exp[ok]).max() <= 1e-15
        assert np.array_equal(np.isnan(p_any), np.isnan(p_all[:, 0]))


def test_entry_refuses_a_bad_background_before_it_needs_a_device():
    from gecco_amd import _native

    model = _native.Model.from_tables(np.zeros((3, 2)), np.zeros((2, 2)))
    with pytest.raises(ValueError, match="background label out of range"):
        model.windowed_marginals_all([0, 2], [0, 1, 2], [0, 1], 2, 1, background=2)
    lib = _native.load_library()
    cptr, gptr, attr = (np.array(v, dtype=np.int32) for v in ([0, 2], [0, 1, 2], [0, 1]))
    p_all, p_any = np.zeros((2, 2)), np.zeros(2)
    args = (model._h, 0, _native._ptr(cptr, _native._c_i32p), 1, _native._ptr(gptr, _native._c_i32p),
            _native._ptr(attr, _native._c_i32p), 2, 1)
    rc = lib.gecco_crf_windowed_marginals_all(*args, -1, 1, _native._ptr(p_all, _native._c_f64p), _native._ptr(p_any, _native._c_f64p))
    assert rc == -1 and b"background" in lib.gecco_crf_last_error()  # GECCO_CRF_EINVAL: a buffer without a background label
    rc = lib.gecco_crf_windowed_marginals_all(*args, 0, 1, _native._ptr(p_all, _native._c_f64p), None)
    assert rc == -1 and b"p_any" in lib.gecco_crf_last_error()
    assert lib.gecco_crf_version() >= 310


# ---- labels
def test_labels_from_a_clusters_table():
    from gecco_amd import typed

    table = _table(["c3", "c1", "c2", "c4"], ["Polyketide", "Unknown", "NRP;Polyketide", "Terpene"])
    join = _join([[0, 1, 2], [5, 6], [8, 9], []], 12)
    labels = typed.gene_labels(12, table, join)
    assert labels == ["Polyketide"] * 3 + ["0", "0"] + ["Unknown"] * 2 + ["0"] + ["NRP;Polyketide"] * 2 + ["0", "0"]
    assert typed.label_type_names("NRP;Polyketide") == ("NRP", "Polyketide")
    assert typed.label_type_names("Unknown") == typed.label_type_names("0") == typed.label_type_names("Mixed") == ()
    # a gene in two clusters: the first in cluster-id order labels it
    join = _join([[0, 1, 2], [2, 3], [], []], 12)
    assert typed.gene_labels(12, table, join)[:4] == ["Polyketide", "Polyketide", "Unknown", "Unknown"]
    # train_cli.assigned_clusters' rules: a row without an id labels no gene, a repeated id is an error
    table = _table(["c1", "", None, "c2"], ["A", "B", "B", "C"])
    assert typed.gene_labels(6, table, _join([[0], [1, 2], [3], [4]], 6)) == ["A", "0", "0", "0", "C", "0"]
    with pytest.raises(ValueError, match="duplicate cluster id"):
        typed.gene_labels(6, _table(["c1", "c1"], ["A", "B"]), _join([[0], [1]], 6))
    # a type cell in any order is one label
    assert typed.cluster_labels(_table(["a", "b", "c"], ["Polyketide;NRP", "", "NRP;Polyketide"])) == ["NRP;Polyketide", "Unknown",
                                                                                                     "NRP;Polyketide"]


def test_fold_to_mixed_fewest_first_ties_by_name():
    from gecco_amd import typed

    counts = {f"T{k:02d}": 5 for k in range(29)}  # 29 plain labels
    counts.update({"A;B": 3, "A;C": 1, "B;C": 1, "C;D": 2})  # 33 in all
    with pytest.warns(UserWarning, match="A;C, B;C, C;D") as rec:
        folded = typed.fold_labels(counts)
    assert len(rec) == 1
    # 33 -> fold A;C (1, first by name): 32 + Mixed = 33 -> B;C: 32 -> C;D: 31
    assert {k for k, v in folded.items() if v == "Mixed"} == {"A;C", "B;C", "C;D"}
    assert folded["A;B"] == "A;B" and len(set(folded.values())) == 31
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert typed.fold_labels({f"T{k}": 1 for k in range(31)}) == {f"T{k}": f"T{k}" for k in range(31)}
    with pytest.raises(ValueError, match="32 cluster labels"):
        typed.fold_labels({f"T{k}": 1 for k in range(32)})
    with pytest.raises(ValueError, match="33 cluster labels"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        typed.fold_labels({**{f"T{k}": 1 for k in range(32)}, "A;B": 1, "A;C": 1})
    # through gene_labels: the folded clusters' genes are "Mixed"
    table = _table([f"c{k:02d}" for k in range(35)], [f"T{k:02d}" for k in range(29)] + ["A;B", "A;C", "A;C", "A;D", "A;D", "A;D"])
    join = _join([[k] for k in range(35)], 40)
    with pytest.warns(UserWarning, match="'Mixed': A;B, A;C$"):
        labels = typed.gene_labels(40, table, join)
    assert labels[29:35] == ["Mixed"] * 3 + ["A;D"] * 3 and labels[35] == "0" and len(set(labels)) == 32


# ---- types of a call
def test_type_probability_rule():
    from gecco_amd import typed

    classes = ["0", "A", "A;B", "B", "Unknown", "Mixed"]
    label_types = [typed.label_type_names(c) for c in classes]
    assert label_types == [(), ("A",), ("A", "B"), ("B",), (), ()]
    types = ["A", "B"]
    p_all = np.array([[0.1, 0.7, 0.6, 0.0, 0.9, 0.9],    # A: 1.3, B: 0.6
                      [0.2, 0.5, 0.5, 0.0, 0.9, 0.9],    # A: 1.0, B: 0.5
                      [0.3, 0.9, 0.0, 0.4, 0.9, 0.9]])   # A: 0.9, B: 0.4
    got = typed.type_probabilities(p_all, label_types, types)
    assert got == {"A": 1.0, "B": 0.5}  # the clip at 1 (mean 3.2 / 3), and exactly 0.5 (mean 1.5 / 3)
    assert typed.type_of(got) == frozenset({"A"})  # 0.5 is not a type
    assert typed.type_of({"A": 0.5, "B": 0.5}) == frozenset()
    assert typed.type_of({"A": 0.5000000000000001, "B": 0.2}) == frozenset({"A"})
    rng = np.random.default_rng(3)
    p = rng.random((17, 6)) * 0.3
    assert typed.type_probabilities(p, label_types, types) == ty.type_probabilities(p, label_types, types)
    from gecco_amd.types import ClusterType

    assert str(ClusterType(*typed.type_of({"A": 0.1}))) == "Unknown"


def test_typed_cluster_table_columns(tmp_path):
    from gecco_amd import model, tables, typed
    from gecco_amd.types import ClusterType

    genes = [model.Gene(model.Source("s"), 10 * k, 10 * k + 5, model.Strand.Coding, model.Protein(f"p{k}", None),
                        _probability=0.9) for k in range(3)]
    cluster = model.Cluster("s_cluster_1", genes, ClusterType("B"), {"B": 0.75, "a": 0.125})
    table = typed.typed_cluster_table([cluster], ["B", "a"])
    path = str(tmp_path / "clusters.tsv")
    table.dump(path)
    header = open(path).readline().rstrip("\n").split("\t")
    assert header[header.index("type"):header.index("proteins")] == ["type", "a_probability", "b_probability"]
    back = tables.ClusterTable.load(path)
    assert list(back.type) == ["B"] and float(back.a_probability[0]) == 0.125 and float(back.b_probability[0]) == 0.75


# ---- the model directory
def _tiny_blob():
    from gecco_amd import train

    feats = [[["x"], ["y"], ["x", "z"], ["y"], ["z"], ["x"]]]
    labels = [["0", "A", "A;B", "0", "Unknown", "0"]]
    ts = train.build_training_set(feats, labels, 3, 1, max_labels=train.MAX_LABELS)
    w = np.linspace(-1.0, 1.0, ts.num_features)
    return train.model_blob(ts, w)


def test_model_directory_round_trip_and_md5(tmp_path):
    from gecco_amd import typed

    crf = typed.TypedClusterCRF(3, 1)
    crf._set_blob(_tiny_blob())
    assert crf.classes_ == ["0", "A", "A;B", "Unknown"]
    assert crf.label_types_ == [(), ("A",), ("A", "B"), ()] and crf.types_ == ["A", "B"]
    crf.save(tmp_path)
    meta = json.load(open(tmp_path / "typed_model.json"))
    blob = open(tmp_path / "typed_model.crfsuite", "rb").read()
    assert blob == crf._blob and meta["md5"] == hashlib.md5(blob).hexdigest()
    assert (meta["window_size"], meta["window_step"], meta["feature_type"], meta["background"]) == (3, 1, "protein", "0")
    assert meta["labels"] == [{"name": "0", "types": []}, {"name": "A", "types": ["A"]}, {"name": "A;B", "types": ["A", "B"]},
                              {"name": "Unknown", "types": []}]
    back = typed.TypedClusterCRF.trained(tmp_path)
    assert (back.window_size, back.window_step, back.classes_, back.label_types_, back.types_, back._blob) == (
        3, 1, crf.classes_, crf.label_types_, crf.types_, crf._blob)
    with open(tmp_path / "typed_model.crfsuite", "ab") as fh:
        fh.write(b"\0")
    with pytest.raises(ValueError, match="MD5 hash of model data does not match signature"):
        typed.TypedClusterCRF.trained(tmp_path)


def test_domain_features_are_refused():
    from gecco_amd import typed

    with pytest.raises(ValueError, match="typed models use protein features"):
        typed.TypedClusterCRF(5, 1, feature_type="domain")
    with pytest.raises(ValueError, match="typed models use protein features"):
        typed.main(["train", "--genes", os.devnull, "--features", os.devnull, "--clusters", os.devnull, "--feature-type", "domain"])
