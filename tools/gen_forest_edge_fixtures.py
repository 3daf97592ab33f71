#!/usr/bin/env python3
"""Record what the installed sklearn fits on the edge sets of tests/forest_edge_sets.py.

Every set is fitted the way the device forest is entered (DecisionTreeClassifier per seed with sample weights, or
RandomForestClassifier), and tests/golden/types/forest_edges.json.gz receives: sklearn's version; per set the SHA-256 of
the built arrays, per tree `node_count`, `max_depth` and the SHA-256 of each of the eight node arrays (the dtypes of
tools/gen_type_fixtures.py), and the `posit` bits of the set's planted predict rows with the SHA-256 of those rows.
Inputs are not stored: the tests rebuild them and check the digests first.  sklearn and scipy only.

usage:  python tools/gen_forest_edge_fixtures.py [--out tests/golden/types]
"""
import argparse
import gzip
import hashlib
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import forest_edge_sets as sets  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "types")
NAME = "forest_edges.json.gz"
# the node arrays of sklearn's Tree, with the dtype each is hashed in (as tools/gen_type_fixtures.py)
TREE_ARRAYS = (("children_left", np.int64), ("children_right", np.int64), ("feature", np.int64), ("threshold", np.float64),
               ("impurity", np.float64), ("n_node_samples", np.int64), ("weighted_n_node_samples", np.float64),
               ("value", np.float64))


def fit_sklearn(s):
    """The fitted sklearn trees of a set, in the device forest's tree order."""
    import scipy.sparse
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.tree import DecisionTreeClassifier

    X = scipy.sparse.csc_matrix((s["data"], s["indices"], s["indptr"]), shape=(s["n"], s["F"]))
    y = s["y"].astype(np.int64)
    y = y[:, 0] if y.shape[1] == 1 else y
    if s["mode"] == "tree":
        w = s["counts"].astype(np.float64)
        return [DecisionTreeClassifier(max_features=s["max_features"], random_state=seed).fit(X, y, sample_weight=w)
                for seed in s["seeds"]]
    rf = RandomForestClassifier(n_estimators=s["n_estimators"], random_state=s["random_state"], max_features=s["max_features"])
    return list(rf.fit(X, y).estimators_)


def tree_arrays(est) -> dict:
    return {name: np.ascontiguousarray(getattr(est.tree_, name), dtype=dt) for name, dt in TREE_ARRAYS}


def tree_record(est) -> dict:
    rec = {"node_count": int(est.tree_.node_count), "max_depth": int(est.tree_.max_depth)}
    for name, a in tree_arrays(est).items():
        rec[name] = hashlib.sha256(a.tobytes()).hexdigest()
    return rec


def posit(trees, rows, n_outputs) -> np.ndarray:
    """`1 - predict_proba[k][:, 0]` of the forest made of `trees`: the per-tree probabilities summed in tree order and
    divided by the number of trees, as RandomForestClassifier.predict_proba does."""
    acc = np.zeros((len(rows), n_outputs))
    for t in trees:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            p = t.predict_proba(rows)
        p = [p] if n_outputs == 1 else p
        for k in range(n_outputs):
            acc[:, k] += p[k][:, 0]
    acc /= len(trees)
    return 1 - acc


def set_record(s) -> dict:
    trees = fit_sklearn(s)
    rows = sets.planted_rows(s, sets.split_nodes([tree_arrays(t) for t in trees]))
    out = posit(trees, rows, s["y"].shape[1])
    return {"name": s["name"], "path": sets.PATHS[s["name"]], "input_sha256": sets.digest(s), "trees": [tree_record(t) for t in trees],
            "rows_sha256": hashlib.sha256(rows.tobytes()).hexdigest(), "rows_shape": list(rows.shape),
            "posit": np.ascontiguousarray(out, dtype=np.float64).view(np.uint64).ravel().tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import sklearn

    os.makedirs(args.out, exist_ok=True)
    recs = [set_record(sets.build(name)) for name in sets.NAMES]
    doc = {"sklearn": sklearn.__version__, "tree_arrays": [n for n, _ in TREE_ARRAYS], "sets": recs}
    path = os.path.join(args.out, NAME)
    text = json.dumps(doc, separators=(",", ":"), allow_nan=False)
    with open(path, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as fh:
        fh.write(text.encode())
    print(f"{path}: {len(recs)} sets, {sum(len(r['trees']) for r in recs)} trees, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
