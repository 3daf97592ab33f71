#!/usr/bin/env python3
"""Time the type classifier's cross-validation on the embedded data (1870 x 2766 compositions, 10 folds of 100 trees):
`types.cross_validate`, which fits every fold's forest in one launch and scores every test block in another, against the
same folds through the lone `DeviceForest.fit` and `predict_posit` in turn.  Both sides do the same host work per fold
(slicing, sklearn's CSC layout, drawing the random streams); `native_*` times the native calls alone on prepared
arguments.  Wall times of synchronous calls in one process, the median (and min, max) of --repeat runs after one warm-up
each.  The two sides' out-of-fold probabilities are compared bit for bit before anything is timed.  sklearn's time for
the same folds on this machine's CPU, once, when sklearn is installed (--no-sklearn leaves it out).  Prints one JSON line;
--out also writes it to a file.

usage:  python tools/bench_types_cv.py [--repeat 5] [--splits 10] [--no-sklearn] [--out FILE]
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

from gecco_amd import _native, types  # noqa: E402

TYPES = os.path.join(ROOT, "tests", "golden", "types")


def timed(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--splits", type=int, default=10)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    comp, _, _, labels = types.read_training_data(TYPES)
    dense = types._dense(comp)
    classes = sorted(set().union(*labels))
    truth = types.TypeBinarizer(classes).transform(labels)
    folds = types.type_folds(len(labels), args.splits)

    def batched():
        return types.cross_validate(dense, labels, classes=classes, splits=args.splits).posit

    def sequential():
        posit = np.zeros(truth.shape)
        for train, test in folds:
            model = types.DeviceForest(random_state=0).fit(dense[train], truth[train])
            posit[test] = model.predict_posit(dense[test])
        return posit

    assert batched().tobytes() == sequential().tobytes(), "the batched and the sequential folds differ"
    res = {"n_samples": int(dense.shape[0]), "n_features": int(dense.shape[1]), "splits": args.splits, "n_trees": 100,
           "repeat": args.repeat, "device": torch.cuda.get_device_name(0)}
    res["batched"] = timed(batched, args.repeat)
    res["sequential"] = timed(sequential, args.repeat)
    res["sequential_over_batched"] = res["sequential"]["median_s"] / res["batched"]["median_s"]
    # the native calls alone, on arguments prepared once
    prepared = [types.DeviceForest(random_state=0)._problem(dense[train], truth[train]) for train, _ in folds]
    problems, max_features = [p for p, _ in prepared], prepared[0][1]
    tests = [np.ascontiguousarray(dense[test]) for _, test in folds]

    def native_batched():
        _native.predict_forests(_native.fit_forests(problems, max_features), tests)

    def native_sequential():
        for p, x in zip(problems, tests):
            _native.Forest(**p, max_features=max_features).predict(x)

    res["native_batched"] = timed(native_batched, args.repeat)
    res["native_sequential"] = timed(native_sequential, args.repeat)
    res["native_fit_batched"] = timed(lambda: _native.fit_forests(problems, max_features), args.repeat)
    res["native_fit_sequential"] = timed(lambda: [_native.Forest(**p, max_features=max_features) for p in problems], args.repeat)
    res["sklearn"] = None
    if not args.no_sklearn:
        try:
            import scipy.sparse
            import sklearn
            from sklearn.ensemble import RandomForestClassifier
        except ImportError:
            pass
        else:
            X = scipy.sparse.load_npz(os.path.join(TYPES, "compositions.npz")).tocsr()
            t0 = time.perf_counter()
            for train, test in folds:
                RandomForestClassifier(random_state=0).fit(X[train], truth[train]).predict_proba(X[test])
            res["sklearn_s"] = time.perf_counter() - t0
            res["sklearn"] = sklearn.__version__
            res["cpu_threads"] = len(os.sched_getaffinity(0))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
