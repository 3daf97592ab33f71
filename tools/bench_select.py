#!/usr/bin/env python3
"""Time the Fisher p-values of feature selection: `gecco_amd.select.fisher_exact_pvalues` (one device call) against a
Python loop over `scipy.stats.fisher_exact` on the same tables -- what `gecco.crf.select.fisher_significance` does.

The tables are those of a synthetic training set shaped like GECCO's: ~11 000 domain names (Zipf-distributed use),
`--proteins` proteins of which ~25 % lie in clusters, where a fifth of the names are enriched.

usage:  python tools/bench_select.py [--proteins 200000] [--names 11064] [--repeat 5] [--device 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_tables(rng, n_prot, n_names):
    from gecco_amd.model import Domain, Protein
    from gecco_amd.select import contingency_tables

    names = [f"PF{k:05d}" for k in range(n_names)]
    weight = 1.0 / np.arange(1, n_names + 1) ** 1.1
    weight /= weight.sum()
    enriched = rng.random(n_names) < 0.2
    proteins = []
    for i in range(n_prot):
        label = rng.random() < 0.25
        k = int(rng.integers(1, 4))
        idx = rng.choice(n_names, size=k, p=weight)
        if label:
            idx = np.where(enriched[idx] | (rng.random(k) < 0.5), idx, rng.choice(np.flatnonzero(enriched), size=k))
        proteins.append(Protein(f"p{i}", None, [Domain(names[j], 0, 1, "Pfam", 1e-5, 1e-6, probability=float(label))
                                                for j in idx]))
    return contingency_tables(proteins)[1].reshape(-1, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=200_000)
    ap.add_argument("--names", type=int, default=11064)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from scipy.stats import fisher_exact

    from gecco_amd.select import fisher_exact_pvalues

    tables = synthetic_tables(np.random.default_rng(1), args.proteins, args.names)
    fisher_exact_pvalues(tables[:8], device=args.device)  # (warm-up: context, code object)
    dev = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        got = fisher_exact_pvalues(tables, device=args.device)
        dev.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    exp = np.array([fisher_exact([[a, b], [c, d]], alternative="two-sided").pvalue for a, b, c, d in tables])
    cpu = time.perf_counter() - t0
    big = exp >= 1e-280
    rel = float(np.max(np.abs(got[big] - exp[big]) / exp[big])) if big.any() else 0.0
    print(json.dumps({"tables": int(len(tables)), "proteins": args.proteins, "device_s_median": float(np.median(dev)),
                      "device_s_min": float(np.min(dev)), "scipy_loop_s": cpu, "speedup": cpu / float(np.median(dev)),
                      "max_rel_err": rel}))


if __name__ == "__main__":
    main()
