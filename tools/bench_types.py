#!/usr/bin/env python3
"""Time the type classifier: the device forest fit (gecco_crf_forest_fit, 100 trees on the embedded 1870 x 2766
compositions) and predict, against sklearn's RandomForestClassifier fit / predict_proba on this machine's CPU when sklearn
is installed.  Wall times of synchronous calls (the fit call includes its uploads and the download of the node counts),
the median of --repeat runs after one warm-up.  Prints one JSON line; --out also writes it to a file.

usage:  python tools/bench_types.py [--repeat 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (before libgecco_crf.so: the wheel's own HIP runtime has to be the first one loaded)

from gecco_amd import types  # noqa: E402

TYPES = os.path.join(ROOT, "tests", "golden", "types")


def timed(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    clf = types.TypeClassifier.trained(TYPES)
    comp = types.load_npz(os.path.join(TYPES, "compositions.npz"))
    dense = types._dense(comp)
    labels = clf.binarizer.transform([frozenset(filter(None, ln.split("\t")[1].strip().split(";")))
                                      for ln in open(os.path.join(TYPES, "types.tsv"))])
    res = {"n_samples": int(dense.shape[0]), "n_features": int(dense.shape[1]), "n_trees": clf.model.n_estimators,
           "nodes": int(clf.model.forest.node_count.sum()), "max_depth": int(clf.model.forest.max_depth.max())}
    res["device_fit_s"], res["device_fit_min_s"] = timed(lambda: clf.model.fit(comp, labels), args.repeat)
    res["device_predict_1870_s"], _ = timed(lambda: clf.predict_probabilities(dense), args.repeat)
    res["device_predict_1_s"], _ = timed(lambda: clf.predict_probabilities(dense[:1]), args.repeat)
    try:
        import scipy.sparse
        import sklearn
        from sklearn.ensemble import RandomForestClassifier
    except ImportError:
        res["sklearn"] = None
    else:
        X = scipy.sparse.load_npz(os.path.join(TYPES, "compositions.npz"))
        rf = RandomForestClassifier(random_state=0)
        res["sklearn"] = sklearn.__version__
        res["cpu_threads"] = len(os.sched_getaffinity(0))
        res["sklearn_fit_s"], res["sklearn_fit_min_s"] = timed(lambda: rf.fit(X, labels), args.repeat)
        res["sklearn_predict_1870_s"], _ = timed(lambda: rf.predict_proba(dense), args.repeat)
        res["sklearn_predict_1_s"], _ = timed(lambda: rf.predict_proba(dense[:1]), args.repeat)
        res["fit_speedup"] = res["sklearn_fit_s"] / res["device_fit_s"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
