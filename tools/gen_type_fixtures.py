#!/usr/bin/env python3
"""BUILD CONTAINER ONLY: generate reference-produced golden vectors for the cluster type classifier.

Runs the REFERENCE'S OWN `gecco.types.TypeClassifier` (gecco/types/__init__.py: `trained()` fits a
`sklearn.ensemble.RandomForestClassifier(random_state=0)` on the embedded compositions; `predict_types` turns
`predict_proba` into `posit = 1 - proba[:, k, 0]`) and records, for the embedded training data and for a few small
synthetic training sets, every fitted tree (node count, depth, SHA-256 of each node array) and the `posit` bits of the
training rows and of planted composition rows.  Writes tests/golden/types/: copies of the embedded data files and
ref_forest.json.gz.  The placeholders of tools/gen_reference_fixtures.py stand in for what `gecco.model` imports and the
image lacks; nothing of the reference is written out but its data files and recorded results.

usage:  python tools/gen_type_fixtures.py [--out tests/golden/types]
"""
import argparse
import gzip
import hashlib
import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_reference_fixtures import REFERENCE, _install_placeholders  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "types")
SEED = 0x7E9E5
DATA_FILES = ("domains.tsv", "types.tsv", "compositions.npz")
# the node arrays of sklearn's Tree, with the dtype each is hashed in
TREE_ARRAYS = (("children_left", np.int64), ("children_right", np.int64), ("feature", np.int64), ("threshold", np.float64),
               ("impurity", np.float64), ("n_node_samples", np.int64), ("weighted_n_node_samples", np.float64),
               ("value", np.float64))


def import_reference():
    if not os.path.isdir(os.path.join(REFERENCE, "gecco")):
        raise SystemExit(f"{REFERENCE}/gecco not found: this generator runs in the build container only")
    _install_placeholders()
    sys.path.insert(0, REFERENCE)
    import gecco.types

    assert os.path.abspath(gecco.types.__file__).startswith(REFERENCE)
    return gecco


def tree_record(est) -> dict:
    t = est.tree_
    rec = {"node_count": int(t.node_count), "max_depth": int(t.max_depth)}
    for name, dt in TREE_ARRAYS:
        rec[name] = hashlib.sha256(np.ascontiguousarray(getattr(t, name), dtype=dt).tobytes()).hexdigest()
    return rec


def posit_bits(clf, X) -> list:
    """`TypeClassifier.predict_types`' positive probabilities of the rows of X, as float64 bit patterns (output by output:
    with a one-class output the per-output arrays differ in width, which only the reference's one-row path copes with)."""
    probas = clf.model.predict_proba(X)
    posit = np.stack([1 - p[:, 0] for p in probas], axis=1)
    return np.ascontiguousarray(posit, dtype=np.float64).view(np.uint64).tolist()


def planted_rows(rng, forest, n_features: int, train: np.ndarray) -> np.ndarray:
    """Composition rows at the forest's decision boundaries: all-zero rows, single-domain rows, a feature set to a node's
    threshold exactly, to its float32 rounding and to the float64 neighbours of both, and perturbed training rows."""
    rows = [np.zeros(n_features), np.zeros(n_features)]
    for f in rng.choice(n_features, 20, replace=False):
        r = np.zeros(n_features)
        r[f] = 1.0
        rows.append(r)
    nodes = [(t.tree_.feature[i], t.tree_.threshold[i]) for t in forest.estimators_[:10]
             for i in range(t.tree_.node_count) if t.tree_.children_left[i] >= 0]
    pick = rng.choice(len(nodes), 40, replace=False)
    for k in pick:
        f, th = nodes[k]
        f32 = float(np.float32(th))
        for v in (th, f32, np.nextafter(th, np.inf), np.nextafter(th, -np.inf), np.nextafter(f32, np.inf),
                  np.nextafter(f32, -np.inf)):
            r = train[rng.integers(len(train))].copy() if rng.random() < 0.5 else np.zeros(n_features)
            r[f] = v
            rows.append(r)
    for i in rng.choice(len(train), 40, replace=False):
        r = train[i] * rng.uniform(0.9, 1.1, n_features)
        rows.append(r)
    return np.array(rows)


def synthetic_sets(rng):
    """Small training sets: (name, rows, cols, values (COO), type strings, random_state, n_features)."""
    sets = []

    def coo(dense):
        r, c = np.nonzero(dense)
        return r.tolist(), c.tolist(), dense[r, c].tolist()

    def sparse(n, f, density, neg=False):
        d = rng.random((n, f)) * (rng.random((n, f)) < density)
        if neg:
            d[rng.random((n, f)) < 0.1] *= -1
        return np.round(d, 3)

    names = ["Alkaloid", "NRP", "Polyketide", "RiPP", "Saccharide", "Terpene"]
    # two classes, with negative values (the splitter's negative / zero / positive layout)
    d = sparse(120, 40, 0.2, neg=True)
    y = ["NRP" if rng.random() < 0.4 else "Polyketide" for _ in range(120)]
    sets.append(("two_classes", d, y, 0))
    # one type in every cluster: a one-class output next to ordinary ones
    d = sparse(150, 60, 0.15)
    y = [";".join(sorted({"RiPP"} | set(rng.choice(names[:3], rng.integers(0, 3), replace=False)))) for _ in range(150)]
    sets.append(("type_in_every_cluster", d, y, 0))
    # three features: max_features = 1
    d = sparse(80, 3, 0.6)
    y = [names[int(rng.integers(0, 4))] for _ in range(80)]
    sets.append(("three_features", d, y, 0))
    # duplicated rows with different labels: impure leaves
    base = sparse(30, 20, 0.3)
    d = np.concatenate([base, base, base])
    y = [names[int(rng.integers(0, 3))] for _ in range(90)]
    sets.append(("duplicated_rows", d, y, 0))
    # another random_state, more classes, a wider matrix
    d = sparse(200, 300, 0.05)
    y = [";".join(sorted(set(rng.choice(names, rng.integers(1, 3), replace=False)))) for _ in range(200)]
    sets.append(("random_state_7", d, y, 7))
    # a single class: the reference does not fit
    d = sparse(40, 10, 0.3)
    sets.append(("single_class", d, ["Terpene"] * 40, 0))
    return [(name, coo(dense), dense.shape, y, rs) for name, dense, y, rs in sets]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    gecco = import_reference()
    import scipy.sparse
    import sklearn

    from gecco.model import ClusterType
    from gecco.types import TypeClassifier

    os.makedirs(args.out, exist_ok=True)
    src = os.path.join(REFERENCE, "gecco", "types")
    for name in DATA_FILES:
        shutil.copyfile(os.path.join(src, name), os.path.join(args.out, name))
    rng = np.random.default_rng(SEED)

    clf = TypeClassifier.trained(None)
    comp = scipy.sparse.load_npz(os.path.join(src, "compositions.npz"))
    train = comp.toarray()
    planted = planted_rows(rng, clf.model, train.shape[1], train)
    embedded = {
        "classes": list(clf.classes_), "n_features": int(train.shape[1]),
        "trees": [tree_record(e) for e in clf.model.estimators_],
        "seeds": [int(e.random_state) for e in clf.model.estimators_],
        "train_posit": posit_bits(clf, comp),
        "planted_rows": {"shape": list(planted.shape), "rows": np.nonzero(planted)[0].tolist(),
                         "cols": np.nonzero(planted)[1].tolist(),
                         "bits": planted[np.nonzero(planted)].view(np.uint64).tolist()},
        "planted_posit": posit_bits(clf, planted),
    }
    synth = []
    for name, (r, c, v), shape, ytext, rs in synthetic_sets(rng):
        X = scipy.sparse.coo_matrix((v, (r, c)), shape=shape)
        types = [ClusterType(*filter(None, t.split(";"))) for t in ytext]
        classes = sorted({n for t in types for n in t.names})
        model = TypeClassifier(classes=classes, random_state=rs)
        rec = {"name": name, "shape": list(shape), "rows": r, "cols": c, "values": v, "types": ytext, "classes": classes,
               "random_state": rs}
        if len(classes) > 1:
            model.model.fit(X, y=model.binarizer.transform(types))
            rec["trees"] = [tree_record(e) for e in model.model.estimators_]
            test = X.toarray()[rng.choice(shape[0], min(shape[0], 40), replace=False)]
            test = np.concatenate([test, np.zeros((2, shape[1])), test[:10] * rng.uniform(0.5, 1.5, (10, shape[1]))])
            rec["test_rows"] = test.view(np.uint64).tolist()
            rec["test_posit"] = posit_bits(model, test)
        else:
            rec["trees"] = None
        synth.append(rec)
    doc = {"sklearn": sklearn.__version__, "tree_arrays": [n for n, _ in TREE_ARRAYS], "embedded": embedded, "synthetic": synth}
    path = os.path.join(args.out, "ref_forest.json.gz")
    text = json.dumps(doc, separators=(",", ":"), allow_nan=False)
    with open(path, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as fh:
        fh.write(text.encode())
    print(f"{path}: {len(embedded['trees'])} embedded trees, {len(synth)} synthetic sets, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
