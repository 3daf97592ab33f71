#!/usr/bin/env python3
"""BUILD CONTAINER ONLY: generate reference-produced golden vectors for the Fisher feature selection
(gecco_amd/select.py, csrc/crf_fisher.hip) -> tests/golden/ref_select.json.gz.

Runs the REFERENCE'S OWN `gecco.crf.select.fisher_significance` (gecco/crf/select.py) on seeded protein sets, for no correction
and for each of the ten correction methods the reference accepts, and `scipy.stats.fisher_exact(..., "two-sided")` on a set of
2x2 tables.  Only data is written: the inputs and the outputs.

What is supplied in memory, never shipped: the placeholders of tools/gen_reference_fixtures.py for what `gecco.model` imports,
and statsmodels' `multitest` module, which the default interpreter of the build container cannot import.  Its pure-Python
source file (statsmodels 0.12, under the conda site-packages) is loaded on its own, after stub `statsmodels`,
`statsmodels.stats` and `statsmodels.stats._knockoff` (`RegressionFDR = None`, used by nothing here) modules are registered.

usage:  python tools/gen_select_fixtures.py [--out tests/golden]
"""
import argparse
import glob
import gzip
import importlib.util
import itertools
import json
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_reference_fixtures import REFERENCE, _install_placeholders  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 0xF15E
METHODS = ["bonferroni", "sidak", "holm-sidak", "holm", "simes-hochberg", "hommel", "fdr_bh", "fdr_by", "fdr_tsbh", "fdr_tsbky"]
MULTITEST_GLOB = "/opt/conda/lib/python3*/site-packages/statsmodels/stats/multitest.py"


def multitest_path():
    found = sorted(glob.glob(MULTITEST_GLOB))
    return found[-1] if found else None


def load_multitest():
    path = multitest_path()
    if path is None:
        raise SystemExit("statsmodels/stats/multitest.py not found: this generator runs in the build container only")
    if "statsmodels.stats.multitest" not in sys.modules:
        sm, sms, knock = (types.ModuleType(n) for n in ("statsmodels", "statsmodels.stats", "statsmodels.stats._knockoff"))
        sm.__path__, sms.__path__ = [], []
        knock.RegressionFDR = None
        sm.stats, sms._knockoff = sms, knock
        sys.modules.update({"statsmodels": sm, "statsmodels.stats": sms, "statsmodels.stats._knockoff": knock})
        spec = importlib.util.spec_from_file_location("statsmodels.stats.multitest", path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["statsmodels.stats.multitest"] = mod
        spec.loader.exec_module(mod)
        sms.multitest = mod
    return sys.modules["statsmodels.stats.multitest"]


def import_reference():
    if not os.path.isdir(os.path.join(REFERENCE, "gecco")):
        raise SystemExit(f"{REFERENCE}/gecco not found: this generator runs in the build container only")
    _install_placeholders()
    load_multitest()
    sys.path.insert(0, REFERENCE)
    import gecco.crf.select
    import gecco.model

    assert os.path.abspath(gecco.crf.select.__file__).startswith(REFERENCE)
    return gecco


# ---- tables ------------------------------------------------------------------------------------------------------------------
def make_tables(rng):
    tables = [list(t) for t in itertools.product(range(25), repeat=4) if sum(t) <= 24]  # every table with total <= 24
    for _ in range(3000):  # margins log-uniform up to 1e7
        tables.append([int(x) for x in np.exp(rng.uniform(0, np.log(1e7), 4)).astype(np.int64)])
    for _ in range(150):  # planted symmetric tables and their mirrors (K = N / 2: k <-> n - k; n = N / 2: k <-> K - k)
        h = int(np.exp(rng.uniform(np.log(2), np.log(2e5))))
        k = int(rng.integers(0, h + 1))
        j = int(rng.integers(0, h + 1))
        tables += [[k, h - k, h - k, k], [h - k, k, k, h - k], [k, h - k, k, h - k], [h - k, k, h - k, k],
                   [k, j, h - k, h - j], [j, k, h - j, h - k]]
    for _ in range(100):  # observed at the mode, and one off it
        K, n2, n = (int(x) for x in np.exp(rng.uniform(0, np.log(1e6), 3)))
        n = min(n, K + n2)
        N = K + n2
        m = int((n + 1) * (K + 1) / (N + 2))
        m = min(max(m, max(0, n - n2)), min(n, K))
        for a in (m, m + 1, m - 1):
            if max(0, n - n2) <= a <= min(n, K):
                tables.append([a, K - a, n - a, n2 - n + a])
    for x in (0, 1, 7, 1000, 123456):  # zero rows and zero columns
        tables += [[0, 0, x, 3], [x, 3, 0, 0], [0, x, 0, 5], [x, 0, 4, 0], [0, 0, 0, 0]]
    for k in (300, 400, 480, 500, 520, 550, 600, 1000, 5000):  # p below 1e-300, and p that underflows to 0
        tables += [[k, 0, 0, k], [k, 1, 2, k], [0, k, k + 3, 0]]
    tables.append([1_000_000, 1_000_000, 1_000_000, 1_000_010])  # support >= 1e6
    tables.append([600_000, 1_400_000, 1_401_000, 599_000])
    return tables


# ---- protein sets ------------------------------------------------------------------------------------------------------------
def make_case(rng, gecco, n_prot, n_names, kind):
    model = gecco.model
    names = [f"PF{k:05d}" for k in rng.choice(20000, size=n_names, replace=False)]
    hot = set(rng.choice(n_names, size=max(1, n_names // 5), replace=False).tolist())
    desc, proteins = [], []
    for i in range(n_prot):
        pid = f"prot{i:05d}"
        if kind == "shared" and i > 0 and rng.random() < 0.2:
            pid = f"prot{int(rng.integers(0, i)):05d}"  # a protein id another gene already has
        label = rng.random() < 0.3
        if kind == "all_neg":
            label = False
        elif kind == "all_pos":
            label = True
        n_dom = int(rng.integers(0, 5)) if kind != "no_domains" or rng.random() < 0.5 else 0
        doms = []
        for _ in range(n_dom):
            j = int(rng.integers(0, n_names))
            if label and rng.random() < 0.5:
                j = int(rng.choice(sorted(hot)))
            p = 1.0 if label else 0.0
            r = rng.random()
            if kind == "mixed" and r < 0.3:
                p = 1.0 - p  # a protein whose domains have both classes
            elif kind == "half" and r < 0.3:
                p = [0.5, 0.25, 0.75, 0.5000000000000001][int(rng.integers(0, 4))]
            doms.append([j, p])
            if kind == "repeat" and rng.random() < 0.4:
                doms.append([j, p])  # the same domain twice
        desc.append([pid, doms])
    if kind == "none_prob":
        desc[len(desc) // 2][1].append([0, None])
    for pid, doms in desc:
        proteins.append(model.Protein(pid, None, [model.Domain(names[j], 10 * k, 10 * k + 9, "Pfam", 1e-5, 1e-6, probability=p)
                                                  for k, (j, p) in enumerate(doms)]))
    return {"kind": kind, "names": names, "proteins": desc}, proteins


def run_case(gecco, case, proteins):
    select = gecco.crf.select
    if case["kind"] == "none_prob":
        try:
            select.fisher_significance(proteins, correction_method=None)
        except ValueError as err:
            case["error"] = str(err)
            return case
        raise AssertionError("the reference accepted a domain without probability")
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for method in [None] + METHODS:
            sig = select.fisher_significance(proteins, correction_method=method)
            out["none" if method is None else method] = {k: float(v) for k, v in sorted(sig.items())}
    case["expect"] = out
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    gecco = import_reference()
    from scipy.stats import fisher_exact

    rng = np.random.default_rng(SEED)
    tables = make_tables(rng)
    pvalues = [float(fisher_exact([[a, b], [c, d]], alternative="two-sided").pvalue) for a, b, c, d in tables]
    kinds = ["plain"] * 20 + ["mixed"] * 8 + ["shared"] * 8 + ["repeat"] * 8 + ["half"] * 8 + ["all_neg", "all_pos"] * 2 \
        + ["no_domains"] * 3 + ["none_prob"]
    cases = []
    for idx, kind in enumerate(kinds):
        if idx < 3:
            n_prot = [20000, 8000, 3000][idx]
        else:
            n_prot = int(np.exp(rng.uniform(np.log(10), np.log(1500))))
        n_names = int(np.exp(rng.uniform(np.log(5), np.log(800))))
        case, proteins = make_case(rng, gecco, n_prot, n_names, kind)
        cases.append(run_case(gecco, case, proteins))
    doc = {"tables": tables, "pvalue": pvalues, "methods": METHODS, "cases": cases}
    path = os.path.join(args.out, "ref_select.json.gz")
    text = json.dumps(doc, separators=(",", ":"), allow_nan=False)
    with open(path, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as fh:
        fh.write(text.encode())
    print(f"{path}: {len(tables)} tables, {len(cases)} protein sets, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
