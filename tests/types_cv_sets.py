"""Synthetic training sets for the type classifier's cross-validation and the batched forest fit (numpy only, seeded):
tests/test_types_cv_host.py, tests/test_gpu_types_cv.py and tools/gen_type_cv_fixtures.py build them from here, so the
fixture records inputs nobody has to store.

A cross-validation case is ``dict(name, X (dense float64), labels (type strings), splits, seed, random_state,
n_estimators)``; every case is planted for one way a batch of folds can differ from its folds fitted alone, and
``PROPERTIES[name](case, folds)`` asserts that the folds it is given -- sklearn's in the generator -- have that property.
"""
import hashlib

import numpy as np

NAMES = ["unequal_61", "rare_type_one_fold", "type_in_every_training_cluster", "column_empty_in_one_fold", "smallest_n"]
SEED = 0x7C5


def folds(n, splits, seed):
    """KFold(splits, shuffle=True, random_state=seed) written out: blocks of a seeded permutation, the first n % splits one
    longer, train and test each ascending.  (The planting needs the folds; the tests compare them with sklearn's record.)"""
    order = np.random.RandomState(seed).permutation(n)
    sizes = np.full(splits, n // splits)
    sizes[:n % splits] += 1
    out, at = [], 0
    for size in sizes.tolist():
        test = np.sort(order[at:at + size])
        out.append((np.setdiff1d(np.arange(n), test), test))
        at += size
    return out


def _sparse(rng, n, f, density, neg=False):
    d = rng.random((n, f)) * (rng.random((n, f)) < density)
    if neg:
        d[rng.random((n, f)) < 0.1] *= -1
    return np.round(d, 3)


def _labels(y, classes):
    return [";".join(c for c, on in zip(classes, row) if on) for row in y]


def _case(name, X, y, classes, splits, seed, n_estimators, random_state=0):
    return dict(name=name, X=X, labels=_labels(y, classes), classes=list(classes), y=np.asarray(y, dtype=np.float64), splits=splits,
                seed=seed, random_state=random_state, n_estimators=n_estimators)


def build(name):
    rng = np.random.default_rng([SEED, NAMES.index(name)])
    if name == "unequal_61":
        # 61 clusters in 3 folds: training sets of 40 / 41 / 41, so node capacity, stack capacity and the stride of the
        # bootstrap counts differ between the problems of one launch; 3 x 100 trees are more workgroups than the card has CUs
        X = _sparse(rng, 61, 40, 0.2, neg=True)
        y = (X[:, :3] != 0) ^ (rng.random((61, 3)) < 0.25)
        return _case(name, X, y, ["NRP", "Polyketide", "RiPP"], 3, 42, 100)
    if name == "rare_type_one_fold":
        # the only two clusters of type "Rare" sit in the test block of fold 1: that fold trains a one-class output (all
        # absent) beside two-class ones, the other folds train two classes there
        n, k, seed = 30, 3, 5
        X = _sparse(rng, n, 12, 0.3)
        y = np.zeros((n, 3), dtype=bool)
        y[:, :2] = (X[:, :2] > 0.3) ^ (rng.random((n, 2)) < 0.2)
        y[folds(n, k, seed)[1][1][:2], 2] = True
        return _case(name, X, y, ["NRP", "Polyketide", "Rare"], k, seed, 25)
    if name == "type_in_every_training_cluster":
        # every cluster is of type "Every" but three of fold 2's test block: that fold trains a one-class output (all present)
        n, k, seed = 33, 3, 9
        X = _sparse(rng, n, 10, 0.35)
        y = np.ones((n, 3), dtype=bool)
        y[:, 1:] = (X[:, :2] > 0.25) ^ (rng.random((n, 2)) < 0.2)
        y[folds(n, k, seed)[2][1][:3], 0] = False
        return _case(name, X, y, ["Every", "NRP", "Polyketide"], k, seed, 25)
    if name == "column_empty_in_one_fold":
        # column 0 is nonzero only in fold 0's test block, columns 8 .. 15 only in fold 2's: fold 0 trains with an empty
        # column, fold 2 with half of its columns empty, fold 1 with none
        n, k, seed = 36, 3, 3
        X = _sparse(rng, n, 16, 0.45)
        f = folds(n, k, seed)
        keep0 = np.zeros(n, dtype=bool)
        keep0[f[0][1]] = True
        keep2 = np.zeros(n, dtype=bool)
        keep2[f[2][1]] = True
        X[~keep0, 0] = 0.0
        X[~keep2, 8:] = 0.0
        X[f[0][1][0], 0] = 0.5
        X[f[2][1][0], 8:] = 0.25
        y = (X[:, 1:3] > 0.3) ^ (rng.random((n, 2)) < 0.2)
        return _case(name, X, y, ["NRP", "Terpene"], k, seed, 25)
    if name == "smallest_n":
        # two clusters, two folds: every fold trains on one sample, the smallest set the fit accepts -- a root that is a leaf
        X = np.array([[0.5, 0.0, 0.25], [0.0, 0.75, 0.25]])
        y = np.array([[True, False], [False, True]])
        return _case(name, X, y, ["NRP", "Terpene"], 2, 0, 25)
    raise KeyError(name)


def _train_y(case, fold_list):
    return [case["y"][train] for train, _ in fold_list]


def _unequal(case, fl):
    assert sorted(len(train) for train, _ in fl) == [40, 41, 41]
    assert all(len(np.unique(y[:, k])) == 2 for y in _train_y(case, fl) for k in range(3))
    assert len(fl) * case["n_estimators"] > 256


def _rare(case, fl):
    k = case["classes"].index("Rare")
    assert int(case["y"][:, k].sum()) == 2
    assert [len(np.unique(y[:, k])) for y in _train_y(case, fl)] == [2, 1, 2]
    assert not _train_y(case, fl)[1][:, k].any()
    assert all(len(np.unique(y[:, j])) == 2 for y in _train_y(case, fl) for j in range(2))


def _every(case, fl):
    assert [len(np.unique(y[:, 0])) for y in _train_y(case, fl)] == [2, 2, 1]
    assert _train_y(case, fl)[2][:, 0].all()


def _empty(case, fl):
    X = case["X"]
    empty = [np.flatnonzero(~(X[train] != 0).any(axis=0)).tolist() for train, _ in fl]
    assert empty == [[0], [], list(range(8, 16))], empty
    assert (X[fl[0][1], 0] != 0).any() and (X[fl[2][1], 8:] != 0).any(axis=0).all()


def _smallest(case, fl):
    assert [len(train) for train, _ in fl] == [1, 1]


PROPERTIES = {"unequal_61": _unequal, "rare_type_one_fold": _rare, "type_in_every_training_cluster": _every,
              "column_empty_in_one_fold": _empty, "smallest_n": _smallest}


def digest(case) -> str:
    """SHA-256 over a case's inputs: what the fixture stores instead of them."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(case["X"], dtype=np.float64).tobytes())
    h.update("\n".join(case["labels"]).encode())
    h.update(repr((case["splits"], case["seed"], case["random_state"], case["n_estimators"])).encode())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------- plain training sets
def training_set(name):
    """``(X, y)`` for the batched fit's own shapes: "small_12" (12 x 5, 2 outputs) and "limit_4096" (the largest sample
    count the kernel takes, 4096 x 24, 2 outputs)."""
    n, f = {"small_12": (12, 5), "limit_4096": (4096, 24)}[name]
    rng = np.random.default_rng([SEED, 100 + n])
    X = _sparse(rng, n, f, 0.4, neg=True)
    y = ((X[:, :2] > 0.2) ^ (rng.random((n, 2)) < 0.2)).astype(np.float64)
    return X, y


def threshold_rows(rng, trees, n_features, n_rows):
    """`n_rows` rows on the decision boundaries of exported `trees` (the idea of tools/gen_type_fixtures.py's planted rows):
    a node's feature set to its threshold, to the threshold's float32 rounding, and to the float64 neighbours of both."""
    nodes = [(int(t["feature"][i]), float(t["threshold"][i])) for t in trees for i in range(len(t["feature"]))
             if t["children_left"][i] >= 0]
    rows = np.zeros((n_rows, n_features))
    if not nodes:
        return rows
    for r in range(n_rows):
        f, th = nodes[int(rng.integers(len(nodes)))]
        f32 = float(np.float32(th))
        variants = (th, f32, np.nextafter(th, np.inf), np.nextafter(th, -np.inf), np.nextafter(f32, np.inf), np.nextafter(f32, -np.inf))
        if rng.random() < 0.5:
            rows[r] = np.round(rng.random(n_features) * (rng.random(n_features) < 0.3), 3)
        rows[r, f] = variants[r % 6]
    return rows
