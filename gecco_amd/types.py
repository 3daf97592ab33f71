"""Cluster type classifier with a random forest fitted and evaluated on the device.

Mirrors ``gecco.types.TypeClassifier`` (gecco/types/__init__.py): ``trained()`` reads ``domains.tsv``, ``types.tsv``
and ``compositions.npz`` from a model directory and fits ``RandomForestClassifier(random_state=0)`` on them;
``predict_types`` annotates clusters with ``type`` and ``type_probabilities``.  The forest is sklearn 1.7's, tree for tree
and bit for bit (``gecco_crf_forest_fit``; at near-equal feature values it is the 1.7.2 build's behaviour
that is followed, which splits any two distinct float32 values), without sklearn or scipy: the host only reads the files, draws
sklearn's random streams with numpy's ``RandomState`` and lays the matrix out as sklearn does (CSC, float32, sorted
indices).

    clf = TypeClassifier.trained(model_dir)      # or None: GECCO's embedded data / $GECCO_AMD_MODEL_DIR
    posit = clf.predict_probabilities(compositions)   # (n_clusters, n_classes), 1 - P(class absent)

``cross_validate`` gives the held-out predictions of that classifier: k folds, every fold's forest fitted in one launch
(``gecco_crf_forest_fit_batch``) and each bit for bit the forest its training rows give alone;
``python -m gecco_amd.types_cv`` is its command line.
"""
import os
import pathlib
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _native, cv

__all__ = ["TypeClassifier", "TypeBinarizer", "ClusterType", "type_string", "probability_columns", "classified_cluster_table",
           "load_npz", "csc_float32", "tree_seeds", "bootstrap_counts", "splitter_state", "cross_validate", "TypeCrossValidation",
           "type_folds", "type_metrics", "read_training_data"]

MAX_INT = int(np.iinfo(np.int32).max)  # sklearn.ensemble._forest.MAX_INT
RAND_R_MAX = 2147483647                # sklearn.utils._random.RAND_R_MAX


# ---------------------------------------------------------------------------------------------- type names
def type_string(names: Iterable[str]) -> str:
    """``str(ClusterType(*names))``: the sorted names joined with ";", or "Unknown" when there are none."""
    names = set(names)
    return ";".join(sorted(names)) if names else "Unknown"


def _names(label: Any) -> frozenset:
    if label is None:
        return frozenset()
    if isinstance(label, str):
        return frozenset(n for n in label.split(";") if n and n != "Unknown")
    names = getattr(label, "names", None)
    return frozenset(names if names is not None else label)


class TypeBinarizer:
    """``gecco.types.binarizer.TypeBinarizer`` without sklearn: type labels <-> a 0/1 matrix over ``classes_``."""

    def __init__(self, classes: Sequence[str]):
        self.classes_ = list(classes)

    def transform(self, labels: Sequence[Any]) -> np.ndarray:
        out = np.zeros((len(labels), len(self.classes_)))
        for i, label in enumerate(labels):
            names = _names(label)
            for j, cls in enumerate(self.classes_):
                out[i, j] = cls in names
        return out

    def inverse_transform(self, yt) -> List[frozenset]:
        return [frozenset(cls for i, cls in enumerate(self.classes_) if row[i]) for row in yt]


def probability_columns(classes: Sequence[str]) -> List[str]:
    """The ``*_probability`` columns of clusters.tsv in ``ClusterTable.from_clusters`` order (gecco/model.py:731-760):
    casefold-sorted class names, lower-cased."""
    return [f"{name.lower()}_probability" for name in sorted(classes, key=str.casefold)]


# ---------------------------------------------------------------------------------------------- input files
def load_npz(path) -> Tuple[Tuple[int, int], np.ndarray, np.ndarray, np.ndarray]:
    """A ``scipy.sparse.save_npz`` file read with numpy alone, as COO triplets ``(shape, row, col, data)`` (COO, CSR and
    CSC layouts; stored entries are kept as they are)."""
    with np.load(path, allow_pickle=False) as z:
        fmt = z["format"].item()
        fmt = fmt.decode() if isinstance(fmt, bytes) else str(fmt)
        shape = tuple(int(v) for v in z["shape"])
        data = np.asarray(z["data"])
        if fmt == "coo":
            row, col = (np.asarray(z["row"]), np.asarray(z["col"])) if "row" in z.files else (z["coords"][0], z["coords"][1])
        elif fmt in ("csr", "csc"):
            indptr, indices = np.asarray(z["indptr"]), np.asarray(z["indices"])
            major = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
            row, col = (major, indices) if fmt == "csr" else (indices, major)
        else:
            raise ValueError(f"{path}: unsupported sparse format {fmt!r} (expected coo, csr or csc)")
    if len(shape) != 2:
        raise ValueError(f"{path}: expected a 2-D matrix, got shape {shape}")
    return shape, np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(data)


def csc_float32(shape, row, col, data):
    """sklearn's training input: ``check_array(X, accept_sparse="csc", dtype=np.float32)`` + ``sort_indices()`` of a COO
    matrix -- duplicates summed in the input dtype (scipy's COO -> CSC), then cast to float32; stored zeros stay.
    Returns ``(indptr int32, indices int32, data float32)``."""
    n_rows, n_cols = int(shape[0]), int(shape[1])
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    data = np.asarray(data)
    if len(row) and (row.min() < 0 or row.max() >= n_rows or col.min() < 0 or col.max() >= n_cols):
        raise ValueError("sparse matrix entry outside its shape")
    order = np.lexsort((row, col))
    r, c, d = row[order], col[order], data[order]
    if len(r):
        first = np.ones(len(r), dtype=bool)
        first[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
        if not first.all():
            start = np.flatnonzero(first)
            d = np.add.reduceat(d, start)
            r, c = r[start], c[start]
    indptr = np.zeros(n_cols + 1, dtype=np.int32)
    np.cumsum(np.bincount(c, minlength=n_cols), out=indptr[1:])
    return indptr, r.astype(np.int32), d.astype(np.float32)


def _as_coo(X):
    """(shape, row, col, data) of a dense array, a scipy sparse matrix or a `load_npz` tuple."""
    if isinstance(X, tuple) and len(X) == 4:
        return X
    if hasattr(X, "tocoo"):
        m = X.tocoo()
        return m.shape, np.asarray(m.row), np.asarray(m.col), np.asarray(m.data)
    a = np.asarray(X, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"expected a 2-D matrix, got shape {a.shape}")
    r, c = np.nonzero(a)
    return a.shape, r, c, a[r, c]


def _dense(X) -> np.ndarray:
    if isinstance(X, tuple) and len(X) == 4:
        shape, r, c, d = X
        out = np.zeros(shape, dtype=np.float64)
        np.add.at(out, (r, c), d)
        return out
    if hasattr(X, "toarray"):
        return np.asarray(X.toarray(), dtype=np.float64)
    return np.asarray(X, dtype=np.float64)


# ---------------------------------------------------------------------------------------------- random streams
def _random_state(random_state):
    if random_state is None:
        return np.random.mtrand._rand  # check_random_state(None): numpy's global RandomState
    if isinstance(random_state, np.random.RandomState):
        return random_state
    return np.random.RandomState(random_state)


def tree_seeds(random_state, n_estimators: int) -> np.ndarray:
    """The per-tree ``random_state`` sklearn gives each estimator (``_set_random_states`` via ``_make_estimator``)."""
    rs = _random_state(random_state)
    return np.array([rs.randint(MAX_INT) for _ in range(n_estimators)], dtype=np.int64)


def bootstrap_counts(seed: int, n_samples: int) -> np.ndarray:
    """``bincount(_generate_sample_indices(seed, n, n), minlength=n)``: each sample's weight in the tree."""
    idx = np.random.RandomState(seed).randint(0, n_samples, n_samples, dtype=np.int32)
    return np.bincount(idx, minlength=n_samples).astype(np.int32)


def splitter_state(seed: int) -> int:
    """The splitter's initial ``rand_r_state``: ``RandomState(seed).randint(0, RAND_R_MAX)`` (``Splitter.init``)."""
    return int(np.random.RandomState(seed).randint(0, RAND_R_MAX))


# ---------------------------------------------------------------------------------------------- the forest
class DeviceForest:
    """The classifier's ``model``: what GECCO reads of a fitted ``RandomForestClassifier`` (``attributes_``) and the forest."""

    def __init__(self, n_estimators: int = 100, random_state=None, max_features="sqrt", device: int = 0):
        self.n_estimators = int(n_estimators)
        self.random_state = random_state
        self.max_features = max_features
        self.device = device
        self.forest: Optional[_native.Forest] = None
        self.seeds: Optional[np.ndarray] = None
        self.attributes_: List[str] = []

    def _max_features(self, n_features: int) -> int:
        mf = self.max_features
        if mf == "sqrt":
            return max(1, int(np.sqrt(n_features)))
        if mf == "log2":
            return max(1, int(np.log2(n_features)))
        if mf is None:
            return n_features
        if isinstance(mf, float):
            return max(1, int(mf * n_features))
        return int(mf)

    def _problem(self, X, y) -> Tuple[Dict[str, Any], int]:
        """The native fit's arguments for training set (X, y), with this forest's random streams drawn, and max_features."""
        shape, row, col, data = _as_coo(X)
        y = np.asarray(y)
        if y.ndim != 2 or y.shape[0] != shape[0]:
            raise ValueError(f"y must have one row per sample: X is {shape}, y is {y.shape}")
        codes = np.zeros(y.shape, dtype=np.uint8)
        n_classes = np.zeros(y.shape[1], dtype=np.uint8)
        for k in range(y.shape[1]):  # np.unique per output, like the forest's _validate_y_class_weight
            cls, inv = np.unique(y[:, k], return_inverse=True)
            if len(cls) > 2:
                raise ValueError("every output must be binary")
            codes[:, k], n_classes[k] = inv, len(cls)
        indptr, indices, values = csc_float32(shape, row, col, data)
        n = int(shape[0])
        self.seeds = tree_seeds(self.random_state, self.n_estimators)
        counts = np.stack([bootstrap_counts(int(s), n) for s in self.seeds]) if n else np.zeros((self.n_estimators, 0), np.int32)
        states = np.array([splitter_state(int(s)) for s in self.seeds], dtype=np.uint32)
        problem = dict(col_ptr=indptr, row_idx=indices, values=values, n_samples=n, y=codes, n_classes=n_classes,
                       sample_counts=counts, rand_state=states)
        return problem, self._max_features(int(shape[1]))

    def fit(self, X, y) -> "DeviceForest":
        problem, max_features = self._problem(X, y)
        self.forest = _native.Forest(**problem, max_features=max_features, device=self.device)
        return self

    @classmethod
    def fit_many(cls, Xs: Sequence[Any], ys: Sequence[Any], *, n_estimators: int = 100, random_state=None, max_features="sqrt",
                 device: int = 0) -> List["DeviceForest"]:
        """One forest per training set ``(Xs[k], ys[k])``, all fitted by one launch (``_native.fit_forests``).  Forest k is
        what ``DeviceForest(n_estimators, random_state, max_features).fit(Xs[k], ys[k])`` gives: it draws its random streams
        (``tree_seeds``, ``bootstrap_counts``, ``splitter_state``) for its own number of samples, in the order of `Xs`.  The
        sets share the number of features and of outputs."""
        if len(Xs) != len(ys):
            raise ValueError(f"{len(Xs)} matrices but {len(ys)} label matrices")
        models = [cls(n_estimators=n_estimators, random_state=random_state, max_features=max_features, device=device) for _ in Xs]
        prepared = [m._problem(X, y) for m, X, y in zip(models, Xs, ys)]
        if not prepared:
            return []
        forests = _native.fit_forests([p for p, _ in prepared], prepared[0][1], device=device)
        for m, f in zip(models, forests):
            m.forest = f
        return models

    def predict_posit(self, X) -> np.ndarray:
        if self.forest is None:
            raise RuntimeError("the forest is not fitted")
        return self.forest.predict(_dense(X))

    def export(self, tree: int) -> Dict[str, np.ndarray]:
        return self.forest.export(tree)


class TypeClassifier:
    """Drop-in for ``gecco.types.TypeClassifier`` (``classifier_type=`` of ``gecco.cli.main``)."""

    def __init__(self, classes: Iterable[str] = (), random_state=None, n_estimators: int = 100, max_features="sqrt",
                 device: int = 0, **kwargs: object):
        unknown = set(kwargs) - {"n_jobs", "verbose"}
        if unknown:
            raise TypeError(f"unsupported RandomForestClassifier arguments: {sorted(unknown)}")
        self.model = DeviceForest(n_estimators=n_estimators, random_state=random_state, max_features=max_features,
                                  device=device)
        self.binarizer = TypeBinarizer(list(classes))

    @property
    def classes_(self) -> List[str]:
        return self.binarizer.classes_

    @staticmethod
    def _embedded_dir():
        env = os.environ.get("GECCO_AMD_MODEL_DIR")
        if env:
            return pathlib.Path(env)
        import importlib.util

        spec = importlib.util.find_spec("gecco")
        if spec is not None and spec.submodule_search_locations:
            for loc in spec.submodule_search_locations:
                cand = pathlib.Path(loc) / "types"
                if (cand / "compositions.npz").exists():
                    return cand
        raise FileNotFoundError("no embedded type classifier data: GECCO is not installed; pass a model directory "
                                "or set GECCO_AMD_MODEL_DIR")

    @classmethod
    def trained(cls, model_path=None, device: int = 0) -> "TypeClassifier":
        """Fit on ``domains.tsv`` / ``types.tsv`` / ``compositions.npz`` of `model_path` (GECCO's embedded data if None),
        with ``random_state=0``; with fewer than two classes nothing is fitted, like the reference."""
        comp, domains, _, types = read_training_data(cls._embedded_dir() if model_path is None else model_path)
        clf = cls(classes=sorted(set().union(*types)), random_state=0, device=device)
        if len(clf.classes_) > 1:
            clf.model.fit(comp, clf.binarizer.transform(types))
        clf.model.attributes_ = domains
        return clf

    def fit(self, X, labels) -> "TypeClassifier":
        """Fit on compositions `X` and type labels (strings, name sets or ClusterType objects)."""
        self.model.fit(X, self.binarizer.transform(list(labels)))
        return self

    def predict_probabilities(self, compositions) -> np.ndarray:
        """``posit``: (n_clusters, n_classes) probabilities that each class is present (``1 - proba[:, k, 0]``)."""
        return self.model.predict_posit(compositions)

    def predict_type_names(self, compositions) -> Tuple[np.ndarray, List[frozenset]]:
        posit = self.predict_probabilities(compositions)
        return posit, self.binarizer.inverse_transform(posit > 0.5)

    def predict_types(self, clusters):
        """Set ``type`` and ``type_probabilities`` on every cluster (gecco/types/__init__.py:114-138)."""
        from .composition import cluster_compositions

        clusters_l = list(clusters)
        if not clusters_l:
            return clusters
        comps = cluster_compositions(clusters_l, self.model.attributes_, device=self.model.device)
        posit, names = self.predict_type_names(comps)
        make = _cluster_type_factory(clusters_l[0])
        for cluster, proba, ty in zip(clusters_l, posit, names):
            cluster.type = make(ty)
            cluster.type_probabilities = dict(zip(self.binarizer.classes_, proba))
        return clusters


def read_training_data(path) -> Tuple[tuple, List[str], List[str], List[frozenset]]:
    """The classifier's training files of a model directory, as ``gecco.types.TypeClassifier.trained`` reads them:
    ``(compositions (a `load_npz` tuple), domains, cluster ids, type name sets)``."""
    path = pathlib.Path(path)
    comp = load_npz(path / "compositions.npz")
    with open(path / "domains.tsv") as fh:
        domains = [line.strip() for line in fh]
    ids, types = [], []
    with open(path / "types.tsv") as fh:
        for line in fh:
            cells = line.split("\t")
            ids.append(cells[0])
            types.append(frozenset(filter(None, cells[1].strip().split(";"))))
    return comp, domains, ids, types


# ---------------------------------------------------------------------------------------------- cross-validation
def type_folds(n: int, splits: int = 10, shuffle: bool = True, seed: int = 42) -> List[Tuple[np.ndarray, np.ndarray]]:
    """``sklearn.model_selection.KFold(splits, shuffle=shuffle, random_state=seed).split(range(n))``: the blocks of
    ``cv.kfold_splits`` taken from ``RandomState(seed).permutation(n)`` (from ``arange(n)`` without shuffle), the train and
    the test indices of a fold each sorted ascending."""
    order = np.random.RandomState(seed).permutation(n) if shuffle else np.arange(n)
    return [(np.sort(order[train]), np.sort(order[test])) for train, test in cv.kfold_splits(n, splits)]


def _or_nan(num: float, den: float) -> float:
    return float(num) / float(den) if den else float("nan")


def type_metrics(truth, posit) -> Dict[str, Any]:
    """Metrics of probabilities `posit` (rows x classes) against the 0/1 matrix `truth`.  Per class (arrays): ``auroc`` and
    ``aupr`` (``cv.roc_auc`` / ``cv.average_precision``), ``precision``, ``recall`` and ``f1`` of ``posit > 0.5``.  Over
    all classes: ``micro_aupr`` (the average precision of the flattened matrices) and ``subset_accuracy`` (the share of rows
    whose predicted set is the true set).  What is undefined is NaN: AUROC and AUPR of a truth that is all one value,
    precision when nothing is predicted positive, recall when nothing is truly positive, F1 (``2 tp / (2 tp + fp + fn)``)
    when either of the two is."""
    truth = np.asarray(truth) > 0.5
    posit = np.asarray(posit, dtype=np.float64)
    if truth.shape != posit.shape or truth.ndim != 2:
        raise ValueError(f"truth {truth.shape} and posit {posit.shape} must be one rows x classes shape")
    pred = posit > 0.5
    nan = float("nan")

    def ranked(t, p):
        if t.size == 0 or t.all() or not t.any():
            return nan, nan
        return cv.roc_auc(t, p), cv.average_precision(t, p)

    per = {name: np.full(truth.shape[1], nan) for name in ("auroc", "aupr", "precision", "recall", "f1")}
    for k in range(truth.shape[1]):
        t, p = truth[:, k], pred[:, k]
        per["auroc"][k], per["aupr"][k] = ranked(t, posit[:, k])
        tp, fp, fn = int((t & p).sum()), int((~t & p).sum()), int((t & ~p).sum())
        per["precision"][k] = _or_nan(tp, tp + fp)
        per["recall"][k] = _or_nan(tp, tp + fn)
        if tp + fp and tp + fn:
            per["f1"][k] = 2 * tp / (2 * tp + fp + fn)
    out: Dict[str, Any] = dict(per)
    out["n"] = int(truth.shape[0])
    out["micro_aupr"] = ranked(truth.ravel(), posit.ravel())[1]
    out["subset_accuracy"] = _or_nan(int((pred == truth).all(axis=1).sum()), truth.shape[0])
    return out


class TypeCrossValidation:
    """Held-out type predictions.  ``classes``; ``truth`` (n x classes, 0/1); ``posit`` (n x classes: every row scored by
    the forest of the fold that held it out); ``fold`` (per row); ``folds`` (``(train, test)`` indices); ``predicted``
    (name sets, ``posit > 0.5``); ``fold_metrics`` (one `type_metrics` dict per fold, on its test rows) and ``pooled`` (on
    all rows); ``models``: the folds' fitted `DeviceForest` s (they hold device memory while the result lives)."""

    def __init__(self, classes: List[str], truth: np.ndarray, posit: np.ndarray, fold: np.ndarray,
                 folds: List[Tuple[np.ndarray, np.ndarray]], models: List[DeviceForest]):
        self.classes, self.truth, self.posit, self.fold, self.folds, self.models = classes, truth, posit, fold, folds, models
        self.predicted = TypeBinarizer(classes).inverse_transform(posit > 0.5)
        self.fold_metrics = [type_metrics(truth[test], posit[test]) for _, test in folds]
        self.pooled = type_metrics(truth, posit)

    def summary(self) -> str:
        """The per-fold and pooled metrics as text, one block per fold and one line per class."""
        def fmt(x: float) -> str:
            return "nan" if np.isnan(x) else f"{x:.4f}"

        lines = []
        for name, m in [(f"fold {i}", m) for i, m in enumerate(self.fold_metrics)] + [("pooled", self.pooled)]:
            lines.append(f"{name}: n={m['n']} subset_accuracy={fmt(m['subset_accuracy'])} micro_aupr={fmt(m['micro_aupr'])}")
            for k, cls in enumerate(self.classes):
                lines.append(f"  {cls}: " + " ".join(f"{key}={fmt(m[key][k])}" for key in ("auroc", "aupr", "precision", "recall", "f1")))
        return "\n".join(lines) + "\n"


def cross_validate(X, labels, *, classes: Optional[Sequence[str]] = None, splits: int = 10, shuffle: bool = True, seed: int = 42,
                   random_state=0, n_estimators: int = 100, max_features="sqrt", device: int = 0) -> TypeCrossValidation:
    """k-fold cross-validation of the type classifier on compositions `X` and type `labels` (strings, name sets or
    ClusterType objects; a cluster without a type stays in).  The folds are `type_folds`; every fold fits
    ``RandomForestClassifier(n_estimators, random_state=random_state, max_features=max_features)`` on its training rows,
    all folds in one launch, and one more launch scores every fold's test rows."""
    labels = list(labels)
    dense = _dense(X)
    if dense.ndim != 2 or dense.shape[0] != len(labels):
        raise ValueError(f"one label per row of X: X is {dense.shape}, {len(labels)} labels")
    classes = sorted(set().union(*map(_names, labels))) if classes is None else list(classes)
    truth = TypeBinarizer(classes).transform(labels)
    folds = type_folds(len(labels), splits, shuffle, seed)
    models = DeviceForest.fit_many([dense[train] for train, _ in folds], [truth[train] for train, _ in folds],
                                   n_estimators=n_estimators, random_state=random_state, max_features=max_features, device=device)
    blocks = _native.predict_forests([m.forest for m in models], [dense[test] for _, test in folds])
    posit = np.zeros(truth.shape, dtype=np.float64)
    fold = np.zeros(len(labels), dtype=np.int64)
    for i, ((_, test), block) in enumerate(zip(folds, blocks)):
        posit[test], fold[test] = block, i
    return TypeCrossValidation(classes, truth, posit, fold, folds, models)


def classified_cluster_table(table, classifier: "TypeClassifier", compositions):
    """`table` (a ``tables.ClusterTable``, one row per row of `compositions`) with ``type`` predicted and one
    ``{name.lower()}_probability`` column per class between ``type`` and ``proteins``, as ``ClusterTable.from_clusters``
    writes them (gecco/model.py:731-760)."""
    from .tables import ClusterTable

    posit, names = classifier.predict_type_names(compositions)
    cols = dict(table.columns)
    cols["type"] = np.array([type_string(n) for n in names], dtype=object)
    extra = []
    for name in sorted(classifier.classes_, key=str.casefold):
        col = f"{name.lower()}_probability"
        cols[col] = posit[:, classifier.classes_.index(name)] if len(posit) else np.zeros(0)
        extra.append((col, float, None))
    out = ClusterTable(cols)
    at = [n for n, _, _ in ClusterTable.COLUMNS].index("type") + 1
    out.COLUMNS = ClusterTable.COLUMNS[:at] + extra + ClusterTable.COLUMNS[at:]
    return out


class ClusterType:
    """``gecco.model.ClusterType``'s value semantics for the native object model: a set of names, printed sorted."""

    def __init__(self, *names: str):
        self.names = frozenset(names)

    def __str__(self) -> str:
        return type_string(self.names)

    def __eq__(self, other) -> bool:
        return isinstance(other, ClusterType) and self.names == other.names

    def __hash__(self) -> int:
        return hash(self.names)

    def __repr__(self) -> str:
        return f"ClusterType({', '.join(map(repr, sorted(self.names)))})"


def _cluster_type_factory(cluster):
    """GECCO's ``ClusterType`` for GECCO's clusters, this module's otherwise."""
    if type(cluster).__module__.startswith("gecco."):
        try:
            from gecco.model import ClusterType as GeccoClusterType

            return lambda names: GeccoClusterType(*names)
        except ImportError:
            pass
    return lambda names: ClusterType(*names)
