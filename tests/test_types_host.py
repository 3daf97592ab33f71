"""Host side of the type classifier (gecco_amd.types), no device needed: sklearn's random streams, the numpy-only npz
reader and sklearn's CSC float32 layout, binariser / type strings / probability columns, the clusters.tsv writer, and the
fixture generator.  sklearn, scipy and the reference are optional: what needs them is skipped without them."""
import gzip
import hashlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gecco_amd import tables, types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TYPES = os.path.join(GOLDEN, "types")


def test_tree_seeds_match_the_fixture():
    with gzip.open(os.path.join(TYPES, "ref_forest.json.gz")) as fh:
        seeds = json.load(fh)["embedded"]["seeds"]
    assert types.tree_seeds(0, 100).tolist() == seeds


def test_random_streams_equal_sklearn():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.ensemble._forest import _generate_sample_indices

    rng = np.random.default_rng(1)
    X, y = rng.random((60, 5)), rng.integers(0, 2, (60, 2))
    for rs in (0, 7, 123):
        rf = RandomForestClassifier(n_estimators=12, random_state=rs).fit(X, y)
        seeds = types.tree_seeds(rs, 12)
        assert seeds.tolist() == [e.random_state for e in rf.estimators_]
        for s in seeds:
            exp = np.bincount(_generate_sample_indices(int(s), 60, 60), minlength=60)
            assert np.array_equal(types.bootstrap_counts(int(s), 60), exp)


def _check_npz(path):
    sp = pytest.importorskip("scipy.sparse")
    shape, r, c, d = types.load_npz(path)
    ref = sp.load_npz(path).tocoo()
    assert shape == ref.shape
    assert np.array_equal(r, ref.row) and np.array_equal(c, ref.col) and d.tobytes() == ref.data.tobytes()
    from sklearn.utils import check_array

    X = check_array(sp.load_npz(path), accept_sparse="csc", dtype=np.float32)
    X.sort_indices()
    indptr, indices, data = types.csc_float32(shape, r, c, d)
    assert np.array_equal(indptr, X.indptr) and np.array_equal(indices, X.indices) and data.tobytes() == X.data.tobytes()


def test_npz_reader_on_the_embedded_file():
    pytest.importorskip("sklearn")
    _check_npz(os.path.join(TYPES, "compositions.npz"))


def test_npz_reader_on_a_training_output(tmp_path):
    pytest.importorskip("sklearn")
    from gecco_amd import train_cli

    rng = np.random.default_rng(4)
    dense = np.round(rng.random((50, 30)) * (rng.random((50, 30)) < 0.2), 4)
    path = str(tmp_path / "compositions.npz")
    train_cli.save_npz_coo(path, dense)
    _check_npz(path)
    sp = pytest.importorskip("scipy.sparse")
    for fmt in ("csr", "csc"):  # the other layouts save_npz writes are read too
        p = str(tmp_path / f"{fmt}.npz")
        sp.save_npz(p, sp.coo_matrix(dense).asformat(fmt))
        shape, r, c, d = types.load_npz(p)
        out = np.zeros(shape)
        out[r, c] = d
        assert np.array_equal(out, dense)


def test_npz_reader_refuses_other_formats(tmp_path):
    p = str(tmp_path / "x.npz")
    np.savez(p, format=b"dia", shape=np.array([2, 2]), data=np.zeros(1))
    with pytest.raises(ValueError):
        types.load_npz(p)


def test_duplicates_are_summed_before_the_cast():
    shape = (3, 2)
    r, c = np.array([2, 0, 2, 1]), np.array([1, 0, 1, 1])
    d = np.array([0.1, 0.0, 0.2, 5.0])
    indptr, indices, data = types.csc_float32(shape, r, c, d)
    assert indptr.tolist() == [0, 1, 3] and indices.tolist() == [0, 1, 2]
    assert data.tolist() == [0.0, 5.0, float(np.float32(0.1 + 0.2))]  # the stored zero stays


def test_binariser_and_type_strings():
    b = types.TypeBinarizer(["Alkaloid", "NRP", "Polyketide"])
    y = b.transform(["NRP;Polyketide", "", "Alkaloid", types.ClusterType("NRP")])
    assert y.tolist() == [[0, 1, 1], [0, 0, 0], [1, 0, 0], [0, 1, 0]]
    assert [types.type_string(n) for n in b.inverse_transform(y > 0.5)] == ["NRP;Polyketide", "Unknown", "Alkaloid", "NRP"]
    assert str(types.ClusterType("Polyketide", "NRP")) == "NRP;Polyketide" and str(types.ClusterType()) == "Unknown"
    assert types.probability_columns(["RiPP", "alpha", "NRP"]) == ["alpha_probability", "nrp_probability", "ripp_probability"]


class _Stub:
    def __init__(self, classes, posit):
        self.classes_, self._posit = classes, posit

    def predict_type_names(self, comps):
        return self._posit, [frozenset(c for c, p in zip(self.classes_, row) if p > 0.5) for row in self._posit]


def test_cluster_table_rewrites_the_golden_row_byte_for_byte():
    path = os.path.join(GOLDEN, "BGC0001866.clusters.tsv")
    raw = open(path, "rb").read()
    header, row = raw.decode().splitlines()[:2]
    cells = dict(zip(header.split("\t"), row.split("\t")))
    classes = ["Alkaloid", "NRP", "Polyketide", "RiPP", "Saccharide", "Terpene"]
    posit = np.array([[float(cells[f"{c.lower()}_probability"]) for c in classes]])
    base = {name: [cells[name]] for name, _, _ in tables.ClusterTable.COLUMNS}
    for name in ("start", "end"):
        base[name] = [int(cells[name])]
    for name in ("average_p", "max_p"):
        base[name] = [float(cells[name])]
    base["type"] = ["Unknown"]
    out = types.classified_cluster_table(tables.ClusterTable(base), _Stub(classes, posit), None)
    buf = io.StringIO()
    out.dump(buf)
    # every cell byte for byte (the reference writes \r\n line ends, this project's tables \n)
    assert buf.getvalue().splitlines() == raw.decode().splitlines()


def test_generator_reproduces_the_fixture(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_type_fixtures as gen
    finally:
        sys.path.pop(0)
    pytest.importorskip("sklearn")
    pytest.importorskip("scipy")
    if not os.path.isdir(os.path.join(gen.REFERENCE, "gecco")):
        pytest.skip("the reference is not on this machine")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_type_fixtures.py"), "--out", str(tmp_path)],
                          stdout=subprocess.DEVNULL)
    for name in ("ref_forest.json.gz", "domains.tsv", "types.tsv", "compositions.npz"):
        new = (tmp_path / name).read_bytes()
        old = open(os.path.join(TYPES, name), "rb").read()
        assert hashlib.sha256(new).hexdigest() == hashlib.sha256(old).hexdigest(), name
