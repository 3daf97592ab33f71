"""Shared readers of tests/golden/ref_select.json.gz (tools/gen_select_fixtures.py): the reference's Fisher feature
selection on seeded protein sets, and scipy's two-sided Fisher exact p-values of a set of 2x2 tables."""
import functools
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALIASES = {
    "bonferroni": ["b", "bonf", "BONFERRONI"], "sidak": ["s", "Sidak"], "holm-sidak": ["hs"], "holm": ["h", "Holm"],
    "simes-hochberg": ["sh"], "hommel": ["ho"], "fdr_bh": ["fdr_i", "fdr_p", "fdri", "fdrp"],
    "fdr_by": ["fdr_n", "fdr_c", "fdrn", "fdrcorr"], "fdr_tsbh": ["fdr_2sbh"], "fdr_tsbky": ["fdr_2sbky", "fdr_twostage"],
}


@functools.lru_cache(maxsize=1)
def load():
    with gzip.open(os.path.join(GOLDEN, "ref_select.json.gz"), "rt") as fh:
        return json.load(fh)


def fixture_tables():
    doc = load()
    return np.asarray(doc["tables"], dtype=np.int64), np.asarray(doc["pvalue"], dtype=np.float64)


def proteins_of(case):
    """`gecco_amd.model.Protein` objects of a protein-set case, in the order the reference was given them."""
    from gecco_amd.model import Domain, Protein

    names = case["names"]
    return [Protein(pid, None, [Domain(names[j], 10 * k, 10 * k + 9, "Pfam", 1e-5, 1e-6, probability=p)
                                for k, (j, p) in enumerate(doms)])
            for pid, doms in case["proteins"]]


def exact_pvalue(table, digits=50):
    """The two-sided p-value of scipy's rule, in `digits`-digit arithmetic: hypergeometric terms as exact step ratios
    from the mode outward, each side until its terms fall below 1e-40 of the total and of pmf(a)."""
    import mpmath

    a, b, c, d = (int(x) for x in table)
    K, n2, n = a + b, c + d, a + c
    N = K + n2
    lo, hi = max(0, n - n2), min(n, K)
    m = min(max(int((n + 1) * (K + 1) / (N + 2)), lo), hi)
    dirs = (1, -1) if a > m else (-1, 1)  # a's side first
    with mpmath.workdps(digits):
        r = {m: mpmath.mpf(1)}
        for step in dirs:
            k, v = m, mpmath.mpf(1)
            while lo <= k + step <= hi:
                if step > 0:
                    v = v * (K - k) * (n - k) / ((k + 1) * (N - K - n + k + 1))
                else:
                    v = v * k * (N - K - n + k) / ((K - k + 1) * (n - k + 1))
                k += step
                r[k] = v
                if a in r and (k - a) * step > 0 and v < 1e-40 * min(r[a], 1):
                    break
        total = mpmath.fsum(r.values())
        ra = r[a]
        side = [v for k, v in r.items() if (k <= a if a < m else k >= a)]
        other = [v for k, v in r.items() if (k > m if a < m else k < m) and v <= ra * (1 + mpmath.mpf(1e-14))]
        return float(min((mpmath.fsum(side) + mpmath.fsum(other)) / total, 1))


def check_pvalues(got, exp, what="", tables=None):
    """The accuracy target against scipy: relative 1e-10 where scipy's p >= 1e-280, both < 1e-250 below, 1.0 exactly.
    Where scipy itself is off by more than 1e-10 (it sums hypergeometric terms it evaluates to ~1e-9 at N ~ 10^7), the
    value is checked against the exact p-value instead, and scipy's own error must then exceed the tolerance."""
    got, exp = np.asarray(got), np.asarray(exp)
    one = exp == 1.0
    bad = np.flatnonzero(one & (got != 1.0))
    assert bad.size == 0, f"{what}: scipy gives exactly 1.0 at {bad[:10]}, got {got[bad[:10]]}"
    big = ~one & (exp >= 1e-280)
    rel = np.abs(got[big] - exp[big]) / exp[big]
    off = np.flatnonzero(big)[rel > 1e-10]
    for i in off:
        assert tables is not None, f"{what}: relative error {rel.max()} at {off[:10]}"
        ex = exact_pvalue(tables[i])
        assert abs(got[i] - ex) <= 1e-12 * ex, (what, tables[i].tolist(), got[i], ex, exp[i])
        assert abs(exp[i] - ex) > 1e-10 * ex, (what, tables[i].tolist(), got[i], ex, exp[i])
    small = ~one & ~big
    assert (got[small] < 1e-250).all(), f"{what}: scipy < 1e-280 but got {got[small].max()}"
