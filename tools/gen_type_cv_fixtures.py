#!/usr/bin/env python3
"""Record what the installed sklearn gives for the type classifier's cross-validation cases.

For the embedded training data of tests/golden/types (3 folds, seed 42) and for every synthetic case of
tests/types_cv_sets.py, and for every fold of ``KFold(splits, shuffle=True, random_state=seed)``: a
``RandomForestClassifier(n_estimators, random_state=random_state)`` is fitted on ``X[train]`` and
tests/golden/types/forest_cv.json.gz receives the train and test indices, per tree ``node_count``, ``max_depth`` and one
SHA-256 over the eight node arrays (order and dtypes of tools/gen_type_fixtures.py's TREE_ARRAYS), and the ``posit`` bits of
the test rows, formed output by output as ``1 - proba_k[:, 0]``.  Inputs are not stored: the synthetic ones are rebuilt by
the tests, which check their digest first.  Every synthetic case is asserted to have the property it was planted for under
sklearn's own folds.  sklearn, scipy and numpy only.

usage:  python tools/gen_type_cv_fixtures.py [--out tests/golden/types]
"""
import argparse
import gzip
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import types_cv_sets as sets  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "types")
NAME = "forest_cv.json.gz"
# the node arrays of sklearn's Tree, with the dtype each is hashed in (as tools/gen_type_fixtures.py)
TREE_ARRAYS = (("children_left", np.int64), ("children_right", np.int64), ("feature", np.int64), ("threshold", np.float64),
               ("impurity", np.float64), ("n_node_samples", np.int64), ("weighted_n_node_samples", np.float64),
               ("value", np.float64))
EMBEDDED = dict(splits=3, seed=42, random_state=0, n_estimators=100)


def tree_record(est) -> list:
    """[node_count, max_depth, SHA-256 over the eight arrays end to end]."""
    h = hashlib.sha256()
    for name, dt in TREE_ARRAYS:
        h.update(np.ascontiguousarray(getattr(est.tree_, name), dtype=dt).tobytes())
    return [int(est.tree_.node_count), int(est.tree_.max_depth), h.hexdigest()]


def embedded_case() -> dict:
    """The embedded data, read as ``gecco.types.TypeClassifier.trained`` reads it."""
    import scipy.sparse

    X = scipy.sparse.load_npz(os.path.join(OUT, "compositions.npz")).tocsr()
    labels = [line.split("\t")[1].strip() for line in open(os.path.join(OUT, "types.tsv"))]
    classes = sorted({n for t in labels for n in t.split(";") if n})
    y = np.array([[c in t.split(";") for c in classes] for t in labels], dtype=np.float64)
    return dict(EMBEDDED, name="embedded", X=X, y=y, classes=classes)


def case_record(case) -> dict:
    import scipy.sparse
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import KFold

    X = scipy.sparse.csr_matrix(case["X"])  # sparse input, as GECCO trains: sklearn's sparse splitter
    n = X.shape[0]
    fold_list = list(KFold(case["splits"], shuffle=True, random_state=case["seed"]).split(np.arange(n)))
    if case["name"] in sets.PROPERTIES:
        sets.PROPERTIES[case["name"]](case, fold_list)
    rec = {"name": case["name"], "classes": case["classes"], "folds": [],
           **{k: case[k] for k in ("splits", "seed", "random_state", "n_estimators")}}
    if case["name"] in sets.PROPERTIES:
        rec["input_sha256"] = sets.digest(case)
    for train, test in fold_list:
        rf = RandomForestClassifier(n_estimators=case["n_estimators"], random_state=case["random_state"])
        rf.fit(X[train], case["y"][train])
        posit = np.stack([1 - p[:, 0] for p in rf.predict_proba(X[test])], axis=1)
        rec["folds"].append({"train": train.tolist(), "test": test.tolist(), "trees": [tree_record(e) for e in rf.estimators_],
                             "posit": np.ascontiguousarray(posit, dtype=np.float64).view(np.uint64).ravel().tolist()})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import sklearn

    os.makedirs(args.out, exist_ok=True)
    recs = [case_record(embedded_case())] + [case_record(sets.build(name)) for name in sets.NAMES]
    doc = {"sklearn": sklearn.__version__, "tree_arrays": [n for n, _ in TREE_ARRAYS], "cases": recs}
    path = os.path.join(args.out, NAME)
    text = json.dumps(doc, separators=(",", ":"), allow_nan=False)
    with open(path, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as fh:
        fh.write(text.encode())
    print(f"{path}: {len(recs)} cases, {sum(len(f['trees']) for r in recs for f in r['folds'])} trees, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
