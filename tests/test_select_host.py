"""Host side of the Fisher feature selection (gecco_amd/select.py), without a GPU: the contingency counting followed by
scipy reproduces the reference's uncorrected p-values bit for bit, the corrections reproduce statsmodels' bit for bit, and
the selection rule gives the shipped model's own selection back."""
import gzip
import hashlib
import os
import subprocess
import sys
import warnings

import pytest

from tests.select_fixtures import ALIASES, GOLDEN, load, proteins_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scipy_significance(proteins):
    from scipy.stats import fisher_exact

    from gecco_amd.select import contingency_tables

    names, tables = contingency_tables(proteins)
    return {name: fisher_exact(t, alternative="two-sided").pvalue for name, t in zip(names, tables)}


def test_fixture_shape():
    doc = load()
    assert len(doc["tables"]) == len(doc["pvalue"]) > 20000
    kinds = [c["kind"] for c in doc["cases"]]
    assert len(kinds) >= 55 and kinds.count("none_prob") == 1
    assert {"plain", "mixed", "shared", "repeat", "half", "all_neg", "all_pos", "no_domains"} <= set(kinds)
    assert max(len(c["proteins"]) for c in doc["cases"]) == 20000
    assert sum(1 for p in doc["pvalue"] if p == 0.0) > 0 and sum(1 for p in doc["pvalue"] if 0 < p < 1e-300) > 0


def test_counting_then_scipy_is_the_reference_bit_for_bit():
    n = 0
    for case in load()["cases"]:
        if "error" in case:
            continue
        got = _scipy_significance(proteins_of(case))
        exp = case["expect"]["none"]
        assert sorted(got) == sorted(exp), case["kind"]
        for name, p in exp.items():
            assert float(got[name]) == p, (case["kind"], name, float(got[name]), p)
        n += len(exp)
    assert n > 4000


def test_missing_probability_raises_the_reference_error():
    from gecco_amd.select import contingency_tables, fisher_significance

    case = next(c for c in load()["cases"] if "error" in c)
    with pytest.raises(ValueError) as err:
        contingency_tables(proteins_of(case))
    assert str(err.value) == case["error"] == "Domain is missing a gene cluster probability"
    with pytest.raises(ValueError, match="missing a gene cluster probability"):
        fisher_significance(proteins_of(case), correction_method=None)


def test_counting_rules():
    """Sets keyed by protein id: repeated domains and shared ids count once, a protein of both classes counts in both
    rows, a probability of exactly 0.5 is not in a cluster, a protein without domains counts nowhere."""
    from gecco_amd.model import Domain, Protein
    from gecco_amd.select import contingency_tables

    def dom(name, p):
        return Domain(name, 0, 1, "Pfam", 1e-5, 1e-6, probability=p)

    proteins = [Protein("p1", None, [dom("A", 1.0), dom("A", 1.0), dom("B", 0.0)]),
                Protein("p1", None, [dom("A", 1.0)]),
                Protein("p2", None, [dom("A", 0.5)]),
                Protein("p3", None, []),
                Protein("p4", None, [dom("C", 0.75)])]
    names, tables = contingency_tables(proteins)
    assert names == ["A", "B", "C"]
    # in cluster: p1, p4 (2);  not: p1, p2 (2)
    assert tables.tolist() == [[[1, 1], [1, 1]], [[0, 2], [1, 1]], [[1, 1], [0, 2]]]


def test_corrections_are_statsmodels_bit_for_bit():
    from gecco_amd.select import significance_correction

    doc = load()
    n = 0
    for case in doc["cases"]:
        if "error" in case:
            continue
        raw = case["expect"]["none"]
        for method in doc["methods"]:
            exp = case["expect"][method]
            for name in [method] + ALIASES[method]:
                got = significance_correction(raw, name)
                assert got == exp, (case["kind"], name)
                assert all(type(v) is float for v in got.values())
                n += 1
    assert n >= 50 * 30


def test_unknown_correction_raises():
    from gecco_amd.select import significance_correction

    with pytest.raises(ValueError):
        significance_correction({"A": 0.5}, "fdr")
    with pytest.raises(ValueError):
        significance_correction({"A": 0.5}, "fdr_gbs")  # (statsmodels has it; the reference's ten methods do not)


def test_selection_of_the_shipped_model():
    from gecco_amd import pickle_model
    from gecco_amd.select import select_features

    st = pickle_model.load_model_dir(GOLDEN).state
    sig, exp = st["significance"], st["significant_features"]
    assert len(sig) == 11064 and len(exp) == 2766
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert select_features(sig, 0.25) == exp


def test_selection_edges():
    from gecco_amd.select import SELECT_WARNING, select_features

    sig = {"d": 0.5, "b": 0.1, "c": 0.1, "a": 0.1, "e": 1.0, "f": 1.0}
    assert select_features(sig, 0.5) == {"a", "b", "c"}
    assert select_features(sig, 0.34) == {"a", "b"}  # ties broken by name
    assert select_features(sig, 0.17) == {"a"}
    with pytest.warns(UserWarning) as rec:
        assert select_features(sig, 5 / 6) == {"a", "b", "c", "d", "e"}
    assert [str(w.message) for w in rec] == [SELECT_WARNING]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        select_features(sig, 4 / 6)
    for bad in (0, 1.5, -0.1):
        with pytest.raises(ValueError, match=f"invalid value for select: {bad}"):
            select_features(sig, bad)
    with pytest.raises(ValueError):
        select_features(sig, 0.1)  # int(0.6) == 0: nothing selected


def test_fit_select_validates_before_any_device_work(monkeypatch):
    from gecco_amd.crf import ClusterCRF
    from gecco_amd.model import Domain, Gene, Protein, Source, Strand

    monkeypatch.setenv("GECCO_AMD_FIT", "native")
    genes = [Gene(Source("c"), 10 * i, 10 * i + 5, Strand.Coding,
                  Protein(f"p{i}", None, [Domain("A", 0, 1, "Pfam", 1e-5, 1e-6, probability=float(i % 2))]))
             for i in range(10)]
    crf = ClusterCRF("protein", window_size=5)
    for bad in (0, 1.5):
        with pytest.raises(ValueError, match="invalid value for select"):
            crf.fit(genes, select=bad)
    assert crf.significance is None and crf.significant_features is None


def test_generator_reproduces_the_fixture(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_select_fixtures as gen
    finally:
        sys.path.pop(0)
    if not os.path.isdir(os.path.join(gen.REFERENCE, "gecco")) or gen.multitest_path() is None:
        pytest.skip("the reference or statsmodels' multitest.py is not on this machine")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_select_fixtures.py"), "--out", str(tmp_path)],
                          stdout=subprocess.DEVNULL)
    new = (tmp_path / "ref_select.json.gz").read_bytes()
    old = open(os.path.join(GOLDEN, "ref_select.json.gz"), "rb").read()
    assert hashlib.sha256(new).hexdigest() == hashlib.sha256(old).hexdigest()
    assert gzip.decompress(new) == gzip.decompress(old)


def test_selection_is_saved_with_the_model(tmp_path):
    """The record a native fit adopts carries `significance` and `significant_features`; save -> trained keeps them,
    and so does the allow-list unpickler (floats in a dict, a frozenset of str)."""
    from gecco_amd import pickle_model
    from gecco_amd.crf import ClusterCRF

    shipped = pickle_model.load_model_dir(GOLDEN).state
    crf = ClusterCRF("protein", window_size=20)
    crf.significance, crf.significant_features = dict(shipped["significance"]), frozenset(shipped["significant_features"])
    crf._adopt_model_blob(pickle_model.crfsuite_blob(pickle_model.load_model_dir(GOLDEN)))
    assert crf.significance == shipped["significance"] and crf.significant_features == shipped["significant_features"]
    crf.save(tmp_path)
    st = pickle_model.load_model_dir(tmp_path).state
    assert st["significance"] == shipped["significance"] and st["significant_features"] == shipped["significant_features"]
    loaded = ClusterCRF.trained(tmp_path)
    assert isinstance(loaded.significant_features, frozenset) and loaded.significance == shipped["significance"]
