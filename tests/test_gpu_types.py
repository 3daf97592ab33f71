"""The cluster type classifier on the device (gecco_crf_forest_*, gecco_amd.types): every tree of the forest against the
hashes sklearn 1.7 recorded (tests/golden/types/ref_forest.json.gz <- tools/gen_type_fixtures.py), the predicted
probabilities bit for bit, and `predict --classify` against the reference's clusters.tsv.  Fixtures only: no sklearn, no
reference tree needed."""
import gzip
import hashlib
import json
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before libgecco_crf.so: the wheel's own HIP runtime has to be the first one loaded)

from gecco_amd import _native, types  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TYPES = os.path.join(GOLDEN, "types")


@pytest.fixture(scope="module")
def ref():
    with gzip.open(os.path.join(TYPES, "ref_forest.json.gz")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def embedded():
    return types.TypeClassifier.trained(TYPES)


def _bits(values) -> np.ndarray:
    return np.asarray(values, dtype=np.uint64).view(np.float64)


def _tree_mismatches(model, expected, arrays):
    bad = []
    fr = model.forest
    for t, rec in enumerate(expected):
        if int(fr.node_count[t]) != rec["node_count"] or int(fr.max_depth[t]) != rec["max_depth"]:
            bad.append((t, "node_count/max_depth", int(fr.node_count[t]), rec["node_count"], int(fr.max_depth[t]), rec["max_depth"]))
            continue
        ex = model.export(t)
        for name in arrays:
            got = hashlib.sha256(np.ascontiguousarray(ex[name]).tobytes()).hexdigest()
            if got != rec[name]:
                bad.append((t, name))
    return bad


def test_embedded_forest_matches_sklearn_tree_for_tree(ref, embedded):
    e = ref["embedded"]
    assert embedded.classes_ == e["classes"]
    assert embedded.model.seeds.tolist() == e["seeds"]
    bad = _tree_mismatches(embedded.model, e["trees"], ref["tree_arrays"])
    assert not bad, f"{len(bad)} mismatches, first: {bad[:5]}"
    assert int(embedded.model.forest.node_count.sum()) == 118958


def test_fit_is_deterministic(ref, embedded):
    again = types.TypeClassifier.trained(TYPES)
    for t in (0, 37, 99):
        a, b = embedded.model.export(t), again.model.export(t)
        for name in ref["tree_arrays"]:
            assert a[name].tobytes() == b[name].tobytes()


def test_embedded_posit_bitwise(ref, embedded):
    e = ref["embedded"]
    comp = types.load_npz(os.path.join(TYPES, "compositions.npz"))
    got = embedded.predict_probabilities(comp)
    exp = _bits(e["train_posit"])
    assert got.shape == exp.shape
    assert got.tobytes() == exp.tobytes(), f"{int((got != exp).sum())} training posit cells differ"
    pr = e["planted_rows"]
    planted = np.zeros(pr["shape"])
    planted[pr["rows"], pr["cols"]] = _bits(pr["bits"])
    got = embedded.predict_probabilities(planted)
    exp = _bits(e["planted_posit"])
    assert got.tobytes() == exp.tobytes(), f"{int((got != exp).sum())} planted posit cells differ"
    _, names = embedded.predict_type_names(planted)
    assert [types.type_string(n) for n in names] == [types.type_string(
        c for c, p in zip(embedded.classes_, row) if p > 0.5) for row in exp]


@pytest.mark.parametrize("name", ["two_classes", "type_in_every_cluster", "three_features", "duplicated_rows",
                                  "random_state_7", "single_class"])
def test_synthetic_sets(ref, name):
    rec = next(s for s in ref["synthetic"] if s["name"] == name)
    X = (tuple(rec["shape"]), np.array(rec["rows"]), np.array(rec["cols"]), np.array(rec["values"]))
    clf = types.TypeClassifier(classes=rec["classes"], random_state=rec["random_state"])
    if rec["trees"] is None:  # one class: the reference fits nothing and `gecco predict` classifies nothing
        assert len(clf.classes_) == 1 and clf.model.forest is None
        with pytest.raises(RuntimeError):
            clf.predict_probabilities(np.zeros((1, rec["shape"][1])))
        return
    clf.fit(X, rec["types"])
    bad = _tree_mismatches(clf.model, rec["trees"], ref["tree_arrays"])
    assert not bad, f"{len(bad)} mismatches, first: {bad[:5]}"
    rows = _bits(rec["test_rows"])
    got = clf.predict_probabilities(rows)
    exp = _bits(rec["test_posit"])
    assert got.tobytes() == exp.tobytes()


def test_zero_rows_and_bad_shapes(embedded):
    out = embedded.predict_probabilities(np.zeros((0, 2766)))
    assert out.shape == (0, 6)
    with pytest.raises(ValueError):
        embedded.predict_probabilities(np.zeros((2, 5)))
    assert embedded.predict_types([]) == []


def test_fit_refuses_out_of_range_sizes():
    ok = dict(col_ptr=np.array([0, 1]), row_idx=np.array([0]), values=np.array([1.0], np.float32), n_samples=2,
              y=np.array([[0], [1]]), n_classes=np.array([2]), sample_counts=np.array([[1, 1]]), rand_state=np.array([5]),
              max_features=1)
    _native.Forest(**ok)  # in range: fits
    cases = [
        dict(n_samples=5000, y=np.zeros((5000, 1)), sample_counts=np.ones((1, 5000))),  # too many samples
        dict(col_ptr=np.zeros(8194, np.int32)),                                      # too many features
        dict(y=np.zeros((2, 65)), n_classes=np.full(65, 2)),                           # too many outputs
        dict(row_idx=np.array([7])),                                                  # row index outside the matrix
        dict(values=np.array([np.inf], np.float32)),                                  # non-finite value
        dict(y=np.array([[0], [3]])),                                                 # class index out of range
        dict(sample_counts=np.array([[0, 0]])),                                       # a tree without samples
        dict(max_features=2),                                                         # more features than exist
    ]
    for change in cases:
        args = dict(ok, **change)
        with pytest.raises(ValueError):
            _native.Forest(**args)


def test_training_output_roundtrip(tmp_path, ref):
    """`gecco_amd.train`'s classifier files (save_npz_coo, domains.tsv, types.tsv) -> trained() -> the same forest as
    fitting the matrix directly; and, where sklearn is installed, sklearn's forest on the same directory."""
    from gecco_amd import train_cli

    rec = next(s for s in ref["synthetic"] if s["name"] == "random_state_7")
    dense = np.zeros(rec["shape"])
    dense[rec["rows"], rec["cols"]] = rec["values"]
    train_cli.save_npz_coo(str(tmp_path / "compositions.npz"), dense)
    (tmp_path / "domains.tsv").write_text("".join(f"PF{i:05d}\n" for i in range(dense.shape[1])))
    (tmp_path / "types.tsv").write_text("".join(f"c{i}\t{t}\r\n" for i, t in enumerate(rec["types"])))
    clf = types.TypeClassifier.trained(tmp_path)
    assert clf.model.attributes_[:2] == ["PF00000", "PF00001"]
    direct = types.TypeClassifier(classes=clf.classes_, random_state=0).fit(dense, rec["types"])
    rows = dense[:30]
    assert clf.predict_probabilities(rows).tobytes() == direct.predict_probabilities(rows).tobytes()
    try:
        import scipy.sparse
        import sklearn.ensemble
    except ImportError:
        return
    rf = sklearn.ensemble.RandomForestClassifier(random_state=0)
    rf.fit(scipy.sparse.load_npz(str(tmp_path / "compositions.npz")), clf.binarizer.transform(rec["types"]))
    exp = np.stack([1 - p[:, 0] for p in rf.predict_proba(rows)], axis=1)
    assert clf.predict_probabilities(rows).tobytes() == exp.tobytes()


def test_predict_types_on_objects_matches_columns(embedded):
    from gecco_amd import composition
    from gecco_amd.model import Cluster, Domain, Gene, Protein, Source, Strand

    rng = np.random.default_rng(3)
    names = embedded.model.attributes_
    clusters = []
    for k in range(12):
        genes = []
        for g in range(int(rng.integers(1, 6))):
            doms = [Domain(str(names[int(rng.integers(len(names)))]), 1, 10, "Pfam", 1e-9, float(rng.uniform(0, 1e-3)))
                    for _ in range(int(rng.integers(0, 4)))]
            genes.append(Gene(Source(f"s{k}"), 100 * g + 1, 100 * g + 90, Strand.Coding, Protein(f"p{k}_{g}", None, doms)))
        clusters.append(Cluster(f"c{k}", genes))
    comps = composition.cluster_compositions(clusters, names)
    posit, labels = embedded.predict_type_names(comps)
    embedded.predict_types(clusters)
    for c, p, names_k in zip(clusters, posit, labels):
        assert str(c.type) == types.type_string(names_k)
        assert list(c.type_probabilities) == embedded.classes_
        assert np.array(list(c.type_probabilities.values())).tobytes() == p.tobytes()


def test_predict_classify_reproduces_reference_clusters(tmp_path):
    from gecco_amd import predict

    model = tmp_path / "model"
    model.mkdir()
    for name in ("model.pkl", "model.pkl.md5"):
        shutil.copy(os.path.join(GOLDEN, name), model / name)
    for name in ("domains.tsv", "types.tsv", "compositions.npz"):
        shutil.copy(os.path.join(TYPES, name), model / name)
    out = tmp_path / "out"
    rc = predict.main(["--genes", os.path.join(GOLDEN, "BGC0001866.genes.tsv"), "--features",
                       os.path.join(GOLDEN, "BGC0001866.features.tsv"), "--model", str(model), "-o", str(out), "--classify"])
    assert rc == 0
    got = (out / "BGC0001866.clusters.tsv").read_text().splitlines()
    exp = open(os.path.join(GOLDEN, "BGC0001866.clusters.tsv")).read().splitlines()
    assert got[0] == exp[0]
    assert len(got) == len(exp)
    header = exp[0].split("\t")
    for g, e in zip(got[1:], exp[1:]):
        gf, ef = g.split("\t"), e.split("\t")
        for col, a, b in zip(header, gf, ef):
            if col in ("average_p", "max_p"):  # the CRF floats: the bound of the existing identity tests
                assert abs(float(a) - float(b)) <= 1e-14, (col, a, b)
            elif col in ("proteins", "domains"):
                # the fixture (an older GECCO's writer) lists proteins in gene order and each domain once; the table
                # writer, unchanged here, sorts and repeats them: the same names
                assert sorted(set(a.split(";"))) == sorted(set(b.split(";"))), (col, a, b)
            else:
                assert a == b, (col, a, b)
