"""Fisher feature selection on the device: gecco_crf_fisher_exact against scipy (fixture tables and fresh seeded ones),
fisher_significance against the reference's own outputs, and ClusterCRF.fit(select=...) on the native training path."""
import os
import random
import warnings

import numpy as np
import pytest

from tests.select_fixtures import check_pvalues, exact_pvalue, fixture_tables, load, proteins_of

pytestmark = pytest.mark.gpu


def _scipy_p(tables):
    from scipy.stats import fisher_exact

    return np.array([fisher_exact([[a, b], [c, d]], alternative="two-sided").pvalue for a, b, c, d in tables])


def test_fixture_tables_meet_the_accuracy_target():
    from gecco_amd.select import fisher_exact_pvalues

    tables, exp = fixture_tables()
    got = fisher_exact_pvalues(tables)
    check_pvalues(got, exp, "fixture tables", tables)
    assert (tables.sum(axis=1) > 2_000_000).any()
    # bits depend on the table alone: a second call, a permutation, a slice
    again = fisher_exact_pvalues(tables)
    assert got.tobytes() == again.tobytes()
    perm = np.random.default_rng(3).permutation(len(tables))
    assert fisher_exact_pvalues(tables[perm]).tobytes() == got[perm].tobytes()
    assert fisher_exact_pvalues(tables[7:1000:3]).tobytes() == got[7:1000:3].tobytes()


def test_planted_ties_are_included():
    """Symmetric tables (K = N/2 or n = N/2): pmf(k) = pmf(mirror of k) exactly, so the observed value and its mirror
    give the same p-value, which includes the mirror term (without it, p would be about half of scipy's)."""
    from gecco_amd.select import fisher_exact_pvalues

    rng = np.random.default_rng(11)
    tabs = []
    for _ in range(400):
        h = int(np.exp(rng.uniform(np.log(2), np.log(3e5))))
        k, j = (int(x) for x in rng.integers(0, h + 1, size=2))
        tabs += [[k, h - k, h - k, k], [h - k, k, k, h - k], [k, j, h - k, h - j], [j, k, h - j, h - k]]
    tabs = np.asarray(tabs, dtype=np.int64)
    got = fisher_exact_pvalues(tabs).reshape(-1, 2)
    np.testing.assert_allclose(got[:, 0], got[:, 1], rtol=1e-13, atol=0)
    check_pvalues(got.ravel(), _scipy_p(tabs), "planted ties", tabs)


def test_fresh_seeded_tables_against_scipy():
    from gecco_amd.select import fisher_exact_pvalues

    rng = np.random.default_rng(20261016)
    n = 10_000
    tabs = np.exp(rng.uniform(0, np.log(1e6), size=(n, 4))).astype(np.int64)
    small = rng.random(n) < 0.4
    tabs[small] = rng.integers(0, 40, size=(int(small.sum()), 4))
    tabs[0] = [1_200_000, 1_100_000, 1_050_000, 1_300_000]  # support >= 1e6
    exp = _scipy_p(tabs)
    got = fisher_exact_pvalues(tabs)
    check_pvalues(got, exp, "fresh tables", tabs)
    assert (exp == 1.0).any() and (got == 1.0).sum() == (exp == 1.0).sum()


def test_errors():
    from gecco_amd.select import fisher_exact_pvalues

    with pytest.raises(ValueError, match="negative"):
        fisher_exact_pvalues([[1, 2, -1, 4]])
    with pytest.raises(ValueError, match="exceeds"):
        fisher_exact_pvalues([[2**30, 2**30, 1, 0]])
    with pytest.raises(ValueError, match="exceeds"):
        fisher_exact_pvalues([[2**62, 2**62, 0, 0]])
    assert fisher_exact_pvalues(np.zeros((0, 4), dtype=np.int64)).shape == (0,)
    # the largest total accepted (scipy is 3e-9 off here: checked against the exact value)
    top = fisher_exact_pvalues([[2**31 - 4, 1, 1, 1], [2**31 - 1, 0, 0, 0]])
    assert abs(top[0] - exact_pvalue([2**31 - 4, 1, 1, 1])) <= 1e-12 * top[0] and top[1] == 1.0


def test_protein_sets_match_the_reference():
    from gecco_amd.select import fisher_significance

    doc = load()
    n = 0
    for case in doc["cases"]:
        proteins = proteins_of(case)
        if "error" in case:
            with pytest.raises(ValueError, match=case["error"]):
                fisher_significance(proteins, correction_method=None)
            continue
        for method, exp in case["expect"].items():
            got = fisher_significance(proteins, correction_method=None if method == "none" else method)
            assert sorted(got) == sorted(exp), (case["kind"], method)
            assert all(type(v) is float for v in got.values())
            e = np.array([exp[k] for k in sorted(exp)])
            g = np.array([got[k] for k in sorted(exp)])
            assert np.array_equal(g == 1.0, e == 1.0), (case["kind"], method)
            assert np.all(np.abs(g - e) <= 1e-9 * e), (case["kind"], method, np.max(np.abs(g - e) / np.maximum(e, 1e-300)))
            n += 1
    assert n >= 50 * 11


# ---------------------------------------------------------------- fit(select=...) on the native path
def _genes(rng, n_contigs=12, vocab_size=30):
    """tests/test_gpu_train.py's synthetic training genes, with a larger vocabulary split between the two classes."""
    from gecco_amd.model import Domain, Gene, Protein, Source, Strand

    genes = []
    vocab = [f"PF{k:05d}" for k in range(vocab_size)]
    half = vocab_size // 2
    for c in range(n_contigs):
        src = Source(f"contig{c}")
        n = int(rng.integers(25, 60))
        lab = np.cumsum(rng.random(n) < 0.08) & 1
        for i in range(n):
            k = int(rng.integers(0, 4))
            pool = vocab[half - 3:] if lab[i] else vocab[:half + 3]
            names = rng.choice(pool, size=k)
            doms = [Domain(str(nm), 10 * j, 10 * j + 9, "Pfam", 1e-5, 1e-6, probability=float(lab[i]))
                    for j, nm in enumerate(names)]
            genes.append(Gene(src, 1000 * i, 1000 * i + 900, Strand.Coding,
                              Protein(f"contig{c}_{i}", None, doms), _probability=float(lab[i])))
    return genes


def _fit(crf, genes, seed, **kw):
    random.seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        crf.fit(genes, **kw)


@pytest.mark.parametrize("feature_type", ["protein", "domain"])
def test_fit_select_native(tmp_path, monkeypatch, feature_type):
    from gecco_amd.crf import ClusterCRF
    from gecco_amd.select import contingency_tables

    monkeypatch.setenv("GECCO_AMD_FIT", "native")
    rng = np.random.default_rng(17)
    genes = _genes(rng, vocab_size=40)
    crf = ClusterCRF(feature_type, window_size=5, window_step=1, c1=0.1, c2=0.05)
    _fit(crf, genes, 3, select=0.4)
    sig, keep = crf.significance, crf.significant_features
    assert isinstance(keep, frozenset) and len(keep) == int(0.4 * len(sig)) > 0
    assert all(type(v) is float for v in sig.values())
    # the selection is valid at the cut under scipy's values of the same tables
    names, tables = contingency_tables(g.protein for g in genes)
    ref = dict(zip(names, _scipy_p(tables.reshape(-1, 4)).tolist()))
    assert set(ref) == set(sig)
    assert all(sig[k] == 1.0 if ref[k] == 1.0 else abs(sig[k] - ref[k]) <= 1e-10 * ref[k] for k in ref)
    assert max(ref[k] for k in keep) <= min(ref[k] for k in set(ref) - keep)
    # the model knows the surviving names only
    assert set(crf.model.attributes_) <= keep
    # the same weights as a fit on genes pre-filtered to the same names, with the same random seed
    filtered = [g.with_protein(g.protein.with_domains([d for d in g.protein.domains if d.name in keep])) for g in genes]
    plain = ClusterCRF(feature_type, window_size=5, window_step=1, c1=0.1, c2=0.05)
    _fit(plain, filtered, 3)
    assert plain.significance is None and plain.significant_features is None
    w1, p1 = crf.model.native.state_weights()
    w2, p2 = plain.model.native.state_weights()
    assert crf.model.attributes_ == plain.model.attributes_
    assert w1.tobytes() == w2.tobytes() and np.array_equal(p1, p2)
    assert crf.model.native.trans_weights()[0].tobytes() == plain.model.native.trans_weights()[0].tobytes()
    # significance and the selection survive save -> trained
    crf.save(tmp_path)
    loaded = ClusterCRF.trained(tmp_path)
    assert loaded.significance == sig and loaded.significant_features == keep
    assert isinstance(loaded.significant_features, frozenset)


def test_fit_select_corrected_and_rejected(monkeypatch):
    from gecco_amd.crf import ClusterCRF
    from gecco_amd.select import fisher_significance

    monkeypatch.setenv("GECCO_AMD_FIT", "native")
    genes = _genes(np.random.default_rng(23), vocab_size=36)
    crf = ClusterCRF("protein", window_size=5, window_step=1, c1=0.1, c2=0.05)
    _fit(crf, genes, 4, select=0.25, correction_method="fdr_bh")
    assert crf.significance == fisher_significance([g.protein for g in genes], "fdr_bh")
    for bad in (0, 1.5, 0.001):
        with pytest.raises(ValueError):
            crf.fit(genes, select=bad)
    with pytest.raises(ValueError):
        crf.fit(genes, select=0.5, correction_method="nope")
