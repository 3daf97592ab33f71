"""Host side of the type classifier's cross-validation (gecco_amd.types.cross_validate, gecco_amd.types_cv), no device
needed: the folds against sklearn's recorded indices, the metrics on hand-made matrices with every NaN case, the table's
columns, the command line's refusal of fewer than two classes, the argument checks of gecco_crf_forest_fit_batch /
_predict_batch, and the synthetic cases of tests/types_cv_sets.py against the digests and properties the fixture was
recorded with."""
import ctypes
import gzip
import hashlib
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from gecco_amd import _native, types, types_cv
from tests import types_cv_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = os.path.join(ROOT, "tests", "golden", "types")
FIXTURE = os.path.join(TYPES, "forest_cv.json.gz")


@pytest.fixture(scope="module")
def ref():
    with gzip.open(FIXTURE) as fh:
        doc = json.load(fh)
    doc["by_name"] = {r["name"]: r for r in doc["cases"]}
    return doc


# ---------------------------------------------------------------------------------------------- folds
def test_folds_equal_sklearns_recorded_indices(ref):
    assert [r["name"] for r in ref["cases"]] == ["embedded"] + sets.NAMES
    for rec in ref["cases"]:
        n = sum(len(f["test"]) for f in rec["folds"])
        got = types.type_folds(n, rec["splits"], True, rec["seed"])
        assert len(got) == len(rec["folds"]) == rec["splits"]
        for (train, test), f in zip(got, rec["folds"]):
            assert train.tolist() == f["train"] and test.tolist() == f["test"], rec["name"]
    assert sum(len(f["test"]) for f in ref["by_name"]["embedded"]["folds"]) == 1870


def test_folds_without_shuffle_are_consecutive_blocks():
    got = types.type_folds(7, 3, shuffle=False)
    assert [t.tolist() for _, t in got] == [[0, 1, 2], [3, 4], [5, 6]]
    assert got[1][0].tolist() == [0, 1, 2, 5, 6]
    for n, k in ((5, 1), (3, 4)):
        with pytest.raises(ValueError):
            types.type_folds(n, k)


def test_folds_equal_live_sklearn():
    ms = pytest.importorskip("sklearn.model_selection")
    for n, k, seed in ((23, 5, 42), (10, 10, 0), (61, 3, 7), (1870, 10, 42)):
        exp = list(ms.KFold(k, shuffle=True, random_state=seed).split(np.arange(n)))
        for (a, b), (c, d) in zip(types.type_folds(n, k, True, seed), exp):
            assert np.array_equal(a, c) and np.array_equal(b, d)


def test_synthetic_cases_are_the_recorded_ones_and_keep_their_property(ref):
    for name in sets.NAMES:
        case = sets.build(name)
        assert sets.digest(case) == ref["by_name"][name]["input_sha256"], name
        assert case["classes"] == ref["by_name"][name]["classes"]
        fl = types.type_folds(len(case["labels"]), case["splits"], True, case["seed"])
        for (a, b), (c, d) in zip(fl, sets.folds(len(case["labels"]), case["splits"], case["seed"])):
            assert np.array_equal(a, c) and np.array_equal(b, d)
        sets.PROPERTIES[name](case, fl)
        assert types.TypeBinarizer(case["classes"]).transform(case["labels"]).tolist() == case["y"].tolist()


def test_fixture_is_well_under_the_forest_fixture():
    assert os.path.getsize(FIXTURE) < os.path.getsize(os.path.join(TYPES, "ref_forest.json.gz")) // 2


def test_generator_reproduces_the_fixture(tmp_path, ref):
    sklearn = pytest.importorskip("sklearn")
    pytest.importorskip("scipy")
    if sklearn.__version__ != ref["sklearn"]:
        pytest.skip(f"the installed sklearn is {sklearn.__version__}, the fixture records {ref['sklearn']}")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_type_cv_fixtures.py"), "--out", str(tmp_path)],
                          stdout=subprocess.DEVNULL)
    new = (tmp_path / "forest_cv.json.gz").read_bytes()
    assert hashlib.sha256(new).hexdigest() == hashlib.sha256(open(FIXTURE, "rb").read()).hexdigest()


# ---------------------------------------------------------------------------------------------- metrics
def test_metrics_on_a_hand_made_matrix():
    truth = np.array([[1, 0], [1, 1], [0, 0], [0, 1]])
    posit = np.array([[0.9, 0.2], [0.4, 0.8], [0.6, 0.1], [0.3, 0.7]])
    m = types.type_metrics(truth, posit)
    # class 0: predicted {0, 2}, true {0, 1}: tp 1, fp 1, fn 1; ranking 0.9(+) 0.6(-) 0.4(+) 0.3(-)
    assert m["precision"][0] == 0.5 and m["recall"][0] == 0.5 and m["f1"][0] == 0.5
    assert m["auroc"][0] == 0.75 and m["aupr"][0] == pytest.approx(0.5 * 1.0 + 0.5 * (2 / 3), abs=1e-15)
    # class 1: predicted {1, 3} = truth
    assert [m[k][1] for k in ("precision", "recall", "f1", "auroc", "aupr")] == [1.0] * 5
    assert m["subset_accuracy"] == 0.5 and m["n"] == 4  # the first and the last row's sets are exact
    from gecco_amd import cv

    assert m["micro_aupr"] == cv.average_precision(truth.ravel(), posit.ravel())
    assert m["auroc"][0] == cv.roc_auc(truth[:, 0], posit[:, 0])


def test_undefined_metrics_are_nan_never_an_exception():
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # and nothing warns either: the undefined cases never reach the rank metrics
        # class 0: truth all absent, something predicted; class 1: truth all present, nothing predicted; class 2: neither
        truth = np.array([[0, 1, 0], [0, 1, 0]])
        posit = np.array([[0.9, 0.1, 0.0], [0.2, 0.3, 0.4]])
        m = types.type_metrics(truth, posit)
    assert all(math.isnan(v) for k in ("auroc", "aupr") for v in m[k])
    assert m["precision"][0] == 0.0 and math.isnan(m["recall"][0]) and math.isnan(m["f1"][0])
    assert math.isnan(m["precision"][1]) and m["recall"][1] == 0.0 and math.isnan(m["f1"][1])
    assert all(math.isnan(m[k][2]) for k in ("precision", "recall", "f1"))
    assert m["subset_accuracy"] == 0.0 and not math.isnan(m["micro_aupr"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = types.type_metrics(np.zeros((3, 2)), np.full((3, 2), 0.25))
    assert math.isnan(m["micro_aupr"]) and m["subset_accuracy"] == 1.0
    m = types.type_metrics(np.zeros((0, 2)), np.zeros((0, 2)))  # no rows at all
    assert math.isnan(m["subset_accuracy"]) and math.isnan(m["micro_aupr"]) and m["n"] == 0
    with pytest.raises(ValueError):
        types.type_metrics(np.zeros((2, 2)), np.zeros((2, 3)))


def _result(classes, truth, posit, fold):
    folds = [(np.flatnonzero(fold != i), np.flatnonzero(fold == i)) for i in range(int(fold.max()) + 1)]
    return types.TypeCrossValidation(list(classes), np.asarray(truth, dtype=np.float64), np.asarray(posit), fold, folds, [])


def test_result_and_table_columns_and_order():
    classes = ["RiPP", "alpha", "NRP"]  # the table orders the columns casefolded, as clusters.tsv does
    posit = np.array([[0.75, 0.1, 0.2], [0.3, 0.1 + 0.2, 0.9], [0.0, 0.0, 1 / 3]])
    truth = [[1, 0, 0], [0, 0, 1], [0, 0, 0]]
    res = _result(classes, truth, posit, np.array([1, 0, 1]))
    assert res.predicted == [frozenset({"RiPP"}), frozenset({"NRP"}), frozenset()]
    assert len(res.fold_metrics) == 2 and res.fold_metrics[0]["n"] == 1 and res.pooled["n"] == 3
    assert res.pooled["subset_accuracy"] == 1.0
    table = types_cv.cv_table(["c0", "c1", "c2"], res)
    buf = io.StringIO()
    table.dump(buf)
    lines = buf.getvalue().splitlines()
    assert lines[0].split("\t") == ["cluster_id", "fold", "type", "predicted_type", "alpha_probability", "nrp_probability",
                                    "ripp_probability"]
    assert lines[1].split("\t") == ["c0", "1", "RiPP", "RiPP", "0.1", "0.2", "0.75"]
    assert lines[3].split("\t")[:4] == ["c2", "1", "Unknown", "Unknown"]
    back = np.array([[float(c) for c in line.split("\t")[4:]] for line in lines[1:]])
    assert back.tobytes() == posit[:, [1, 2, 0]].tobytes()  # repr digits: the bits survive the round trip
    text = res.summary()
    assert text.count("fold ") == 2 and "pooled: n=3" in text and "  alpha: auroc=nan" in text


def test_command_line_refuses_fewer_than_two_classes(tmp_path, capsys, monkeypatch):
    (tmp_path / "domains.tsv").write_text("PF00001\nPF00002\n")
    (tmp_path / "types.tsv").write_text("c0\tTerpene\nc1\tTerpene\nc2\t\n")
    from gecco_amd import train_cli

    train_cli.save_npz_coo(str(tmp_path / "compositions.npz"), np.array([[0.5, 0.0], [0.0, 1.0], [0.25, 0.25]]))

    def no_fit(*a, **k):
        raise AssertionError("nothing is to be fitted")

    monkeypatch.setattr(types, "cross_validate", no_fit)
    out = tmp_path / "cv.tsv"
    assert types_cv.main(["--model", str(tmp_path), "-o", str(out)]) != 0
    err = capsys.readouterr().err
    assert "at least two" in err and "1 type" in err and not out.exists()


# ---------------------------------------------------------------------------------------------- native argument checks
def _problem(**change):
    ok = dict(col_ptr=np.array([0, 1]), row_idx=np.array([0]), values=np.array([1.0], np.float32), n_samples=2,
              y=np.array([[0], [1]]), n_classes=np.array([2]), sample_counts=np.array([[1, 1]]), rand_state=np.array([5]))
    return dict(ok, **change)


def test_fit_batch_checks_its_arguments_before_any_device_work():
    lib = _native.load_library()
    assert lib.gecco_crf_version() >= 290
    with pytest.raises(ValueError, match=r"forest_fit_batch: n_problems must be in \[1, 1024\]"):
        _native.fit_forests([_problem()] * 1025, 1)
    big = _problem(n_samples=4097, y=np.zeros((4097, 1)), sample_counts=np.ones((1, 4097)))
    with pytest.raises(ValueError, match=r"forest_fit_batch: problem 2: n_samples must be in \[1, 4096\]"):
        _native.fit_forests([_problem(), _problem(), big], 1)
    cases = [(dict(row_idx=np.array([7])), "problem 1: row index out of range"),
             (dict(values=np.array([np.inf], np.float32)), "problem 1: values must be finite"),
             (dict(y=np.array([[0], [3]])), "problem 1: class index out of range"),
             (dict(n_classes=np.array([3])), "problem 1: every output must have 1 or 2 classes"),
             (dict(sample_counts=np.array([[0, 0]])), "problem 1: a tree without samples")]
    for change, message in cases:
        with pytest.raises(ValueError, match="forest_fit_batch: " + message):
            _native.fit_forests([_problem(), _problem(**change)], 1)
    with pytest.raises(ValueError, match="forest_fit_batch: max_features must be in"):
        _native.fit_forests([_problem(), _problem()], 2)
    with pytest.raises(ValueError, match="share n_features"):
        _native.fit_forests([_problem(), _problem(col_ptr=np.array([0, 1, 1]))], 1)
    with pytest.raises(ValueError, match="forest_fit: n_samples must be in"):  # the lone fit keeps its own prefix
        _native.Forest(max_features=1, **big)
    assert _native.fit_forests([], 1) == []
    # the C entry point itself: null pointers, and out[] cleared on failure
    out = (ctypes.c_void_p * 2)(1, 1)
    n = np.array([2, 2], dtype=np.int32)
    null = (ctypes.c_void_p * 2)()
    args = [0, 2, 1, 1, 1, 1, n.ctypes.data] + [null] * 7
    assert lib.gecco_crf_forest_fit_batch(*args, out) == _native.EINVAL
    assert lib.gecco_crf_last_error() == b"forest_fit_batch: problem 0: null buffer" and list(out) == [None, None]
    assert lib.gecco_crf_forest_fit_batch(*args[:6], None, *args[7:], out) == _native.EINVAL
    assert lib.gecco_crf_last_error() == b"gecco_crf_forest_fit_batch: null buffer"
    assert lib.gecco_crf_forest_fit_batch(*args, None) == _native.EINVAL
    args[1] = 0
    assert lib.gecco_crf_forest_fit_batch(*args, out) == _native.EINVAL
    assert b"n_problems must be in" in lib.gecco_crf_last_error()


def test_predict_batch_checks_its_arguments_before_any_device_work():
    lib = _native.load_library()
    null = (ctypes.c_void_p * 2)()
    rows = np.array([1, 1], dtype=np.int32)
    call = lib.gecco_crf_forest_predict_batch
    for n_problems in (0, -1, 1025):
        assert call(null, n_problems, rows.ctypes.data, null, null) == _native.EINVAL
        assert b"forest_predict_batch: n_problems must be in [1, 1024]" == lib.gecco_crf_last_error()
    for args in ((None, 2, rows.ctypes.data, null, null), (null, 2, None, null, null), (null, 2, rows.ctypes.data, None, null),
                 (null, 2, rows.ctypes.data, null, None)):
        assert call(*args) == _native.EINVAL and lib.gecco_crf_last_error() == b"forest_predict_batch: null buffer"
    bad = np.array([1, -1], dtype=np.int32)
    assert call(null, 2, bad.ctypes.data, null, null) == _native.EINVAL
    assert lib.gecco_crf_last_error() == b"forest_predict_batch: problem 1: n_rows must be >= 0"
    assert call(null, 2, rows.ctypes.data, null, null) == _native.EINVAL
    assert lib.gecco_crf_last_error() == b"forest_predict_batch: problem 0: null forest"
    with pytest.raises(ValueError, match="0 forests but 1 blocks"):  # one block of rows per forest
        _native.predict_forests([], [np.zeros((1, 2))])
    assert _native.predict_forests([], []) == []
