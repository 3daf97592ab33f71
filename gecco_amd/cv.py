"""Cross-validation of ``ClusterCRF`` (``gecco cv``): every fold trained in one batch on the device.

What the reference runs (``gecco/cli/commands/cv.py``, ``gecco/crf/cv.py`` at v0.11), restated without sklearn or
polars: genes are grouped by sequence and the groups shuffled with the global ``random``; each fold fits a CRF to its
training sequences (Fisher selection first with ``select``) and predicts its test sequences with their domain
probabilities cleared.  Two things differ on purpose:

* all folds are optimised together (``train.fit_training_sets``: one batched objective per round for every unfinished
  fold) instead of one after another.  Each fold's model is bit for bit what ``ClusterCRF.fit`` gives on its own: the
  random-number stream is consumed in the reference's order (one shuffle of the groups, then one per fold);
* the truth is joined to the predictions by gene (sequence id, protein id, start, end).  The reference pairs them by
  position, between lists in different orders (fold order and prediction order), which misassigns ``is_cluster``,
  AUROC and AUPR whenever the two differ (whenever ``shuffle`` is on).

    python -m gecco_amd.cv --genes G.tsv --features F.tsv --clusters C.tsv [--loto] [-o cv.tsv]
"""
import argparse
import itertools
import math
import operator
import random
import statistics
import sys
import warnings
from typing import Any, Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Set, Tuple, Union

import numpy as np

from . import tables

__all__ = ["LeaveOneGroupOut", "kfold_splits", "roc_auc", "average_precision", "group_genes", "cross_validate",
           "CrossValidation", "Fold", "cv_table", "grid_points", "rank_points", "grid_search", "GridSearch", "GridFold"]


# ---------------------------------------------------------------------------------------------- splitters
class LeaveOneGroupOut:
    """A leave-one-group-out splitter supporting multiple labels (``gecco.crf.cv.LeaveOneGroupOut``).

    If a sample has multiple class labels, it will be excluded from both training and testing data when one of its
    labels corresponds to the fold::

        >>> loto = LeaveOneGroupOut()
        >>> groups = [["a"], ["b"], ["c"], ["a", "b"]]
        >>> for i, (trn, tst) in enumerate(loto.split(range(4), groups=groups)):
        ...     print("-"*20)
        ...     print(" FOLD", i+1)
        ...     print("TRAIN", f"{str(trn):<7}", [groups[i] for i in trn])
        ...     print(" TEST", f"{str(tst):<7}", [groups[i] for i in tst])
        ...
        --------------------
         FOLD 1
        TRAIN [1 2]   [['b'], ['c']]
         TEST [0]     [['a']]
        --------------------
         FOLD 2
        TRAIN [0 2]   [['a'], ['c']]
         TEST [1]     [['b']]
        --------------------
         FOLD 3
        TRAIN [0 1 3] [['a'], ['b'], ['a', 'b']]
         TEST [2]     [['c']]

    """

    def get_n_splits(self, X: object = None, y: object = None, groups: Optional[Iterable[Iterable[str]]] = None) -> int:
        """The number of distinct labels over ``groups``; ``ValueError`` when ``groups`` is None."""
        if groups is None:
            raise ValueError("The 'groups' parameter should not be None")
        return len({label for labels in groups for label in labels})

    def split(self, X: Any, y: Any = None, groups: Any = None) -> Iterator[Tuple[np.ndarray, np.ndarray]]:
        """One fold per label, in sorted order: test = the samples whose labels are exactly that one, train = the samples
        without it."""
        if groups is None:
            raise ValueError("The 'groups' parameter should not be None")
        group_sets: List[Set[object]] = list(map(set, groups))
        unique_groups = {label for labels in group_sets for label in labels}
        indices = np.arange(len(X))
        for ty in sorted(unique_groups):  # type: ignore
            test_mask = np.array([list(group) == [ty] for group in groups], dtype=bool)
            train_mask = np.array([ty not in group for group in groups], dtype=bool)
            yield indices[train_mask], indices[test_mask]


def kfold_splits(n: int, k: int) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The folds of ``sklearn.model_selection.KFold(k).split(range(n))`` (no shuffle): consecutive test blocks, the
    first ``n % k`` of them one longer; the same ``ValueError`` when ``k < 2`` or ``k > n``."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"The number of folds must be of Integral type. {k!r} of type {type(k)} was passed.")
    k = int(k)
    if k <= 1:
        raise ValueError("k-fold cross-validation requires at least one train/test split by setting n_splits=2 or more, "
                         f"got n_splits={k}.")
    if k > n:
        raise ValueError(f"Cannot have number of splits n_splits={k} greater than the number of samples: n_samples={n}.")
    sizes = np.full(k, n // k, dtype=np.int64)
    sizes[:n % k] += 1
    indices = np.arange(n)
    out = []
    current = 0
    for size in sizes.tolist():
        test = indices[current:current + size]
        train = np.concatenate([indices[:current], indices[current + size:]])
        out.append((train, test))
        current += size
    return out


# ---------------------------------------------------------------------------------------------- metrics
def _binary_inputs(y_true: Any, y_score: Any) -> Tuple[np.ndarray, np.ndarray]:
    y_true = np.asarray(y_true).ravel()
    y_score = np.asarray(y_score, dtype=np.float64).ravel()
    if len(y_true) != len(y_score):
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{len(y_true)}, {len(y_score)}]")
    if len(y_true) == 0:
        raise ValueError("Found array with 0 sample(s) (shape=(0,)) while a minimum of 1 is required.")
    if not np.all(np.isfinite(y_score)):
        raise ValueError("Input y_score contains NaN or infinity.")
    if y_true.dtype == bool:
        return y_true, y_score
    values = set(np.unique(y_true).tolist())
    if not values <= {0, 1}:
        raise ValueError(f"y_true takes values in {sorted(values)}: only binary 0/1 labels are supported")
    return y_true == 1, y_score


def _binary_clf_curve(y_true: np.ndarray, y_score: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """False and true positives at every distinct threshold, high to low (sklearn's ``_binary_clf_curve``)."""
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score = y_score[order]
    y_true = y_true[order]
    distinct = np.where(np.diff(y_score))[0]
    threshold_idxs = np.r_[distinct, y_true.size - 1]
    tps = np.cumsum(y_true * 1.0, dtype=np.float64)[threshold_idxs]
    fps = 1 + threshold_idxs - tps
    return fps, tps


def roc_auc(y_true: Any, y_score: Any) -> float:
    """Area under the ROC curve of binary labels, as sklearn 1.7's ``roc_auc_score``: the trapezoids of the ROC curve
    over the distinct scores (ties count half).  With only one class present, warns and returns NaN as sklearn does."""
    y_true, y_score = _binary_inputs(y_true, y_score)
    if len(np.unique(y_true)) != 2:
        warnings.warn("Only one class is present in y_true. ROC AUC score is not defined in that case.", UserWarning)
        return math.nan
    fps, tps = _binary_clf_curve(y_true, y_score)
    if len(fps) > 2:  # (roc_curve's drop_intermediate: collinear points do not change the area's terms)
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps = fps[keep], tps[keep]
    fpr = np.r_[0, fps] / fps[-1]
    tpr = np.r_[0, tps] / tps[-1]
    return float(np.add.reduce(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))


def average_precision(y_true: Any, y_score: Any) -> float:
    """Average precision of binary labels, as sklearn 1.7's ``average_precision_score``: the step integral of the
    precision-recall curve.  Without positives, warns and returns 0.0 as sklearn does."""
    y_true, y_score = _binary_inputs(y_true, y_score)
    fps, tps = _binary_clf_curve(y_true, y_score)
    ps = tps + fps
    precision = np.zeros_like(tps)
    np.divide(tps, ps, out=precision, where=(ps != 0))
    if tps[-1] == 0:
        warnings.warn("No positive class found in y_true, recall is set to one for all thresholds.", UserWarning)
        recall = np.ones_like(tps)
    else:
        recall = tps / tps[-1]
    precision = np.hstack((precision[::-1], 1))
    recall = np.hstack((recall[::-1], 0))
    return float(max(0.0, -np.sum(np.diff(recall) * precision[:-1])))


def _metrics(labels: Sequence[bool], probas: Sequence[float]) -> Tuple[float, float]:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return roc_auc(labels, probas), average_precision(labels, probas)


# ---------------------------------------------------------------------------------------------- cross-validation
def group_genes(genes: Iterable[Any], *, shuffle: bool = True) -> List[List[Any]]:
    """``_group_genes`` of the reference's cv: consecutive genes of one sequence form a group (no sorting first), each
    sorted by start; the groups are shuffled with the global ``random`` when ``shuffle`` is set."""
    groups = itertools.groupby(genes, key=operator.attrgetter("source.id"))
    seqs = [sorted(group, key=operator.attrgetter("start")) for _, group in groups]
    if shuffle:
        random.shuffle(seqs)
    return seqs


def _gene_key(gene: Any) -> Tuple[str, str, int, int]:
    return (gene.source.id, gene.protein.id, gene.start, gene.end)


def _test_copy(gene: Any) -> Any:
    """The reference's ``_get_test_data``: the gene with the probabilities of its domains cleared."""
    return gene.with_protein(gene.protein.with_domains(d.with_probability(None) for d in gene.protein.domains))


class Fold:
    """One fold: its 1-based ``index``, the sequence indices it trained and tested on, the fitted ``crf``
    (``training_result_``, ``significance``, ``significant_features``), the ``predicted`` genes in prediction order,
    ``truth`` (``is_cluster`` of every predicted gene, joined by gene), ``auroc`` and ``aupr`` (NaN where a fold's test
    genes hold a single class)."""

    def __init__(self, **kw: Any) -> None:
        self.__dict__.update(kw)

    def __repr__(self) -> str:
        return f"Fold({self.index}, n_test={len(self.predicted)}, auroc={self.auroc:.3f}, aupr={self.aupr:.3f})"


class CrossValidation:
    """The result of ``cross_validate``: ``folds`` in order, and ``auroc`` / ``aupr`` over the predictions of all."""

    def __init__(self, folds: List[Fold]) -> None:
        self.folds = folds
        labels = [t for f in folds for t in f.truth]
        probas = [g.average_probability for f in folds for g in f.predicted]
        self.auroc, self.aupr = _metrics(labels, probas) if labels else (math.nan, math.nan)

    def table(self) -> bytes:
        return cv_table(self.folds)

    def write(self, path: str) -> None:
        with open(path, "wb") as out:
            out.write(self.table())


def cv_table(folds: Sequence[Fold]) -> bytes:
    """``cv.tsv``: the reference's ``GeneTable`` columns of every fold's predicted genes, then ``fold`` (1-based) and
    ``is_cluster`` (``true`` / ``false``, as polars writes booleans); fold by fold, in prediction order, one header."""
    import io

    names = [name for name, _, _ in tables.GeneTable.COLUMNS]
    out = io.StringIO()
    out.write("\t".join(names + ["fold", "is_cluster"]) + "\n")
    for f in folds:
        t = tables.GeneTable.from_genes(f.predicted)
        for i in range(len(t)):
            cells = [tables._fmt(t.columns[n][i]) for n in names]
            out.write("\t".join(cells + [str(f.index), "true" if f.truth[i] else "false"]) + "\n")
    return out.getvalue().encode("utf-8")


SplitSpec = Union[int, Sequence[Tuple[Sequence[int], Sequence[int]]], Callable[[List[List[Any]]], Sequence[Tuple[Any, Any]]]]


def _fold_indices(seqs: List[List[Any]], splits: SplitSpec) -> List[Tuple[Any, Any]]:
    if isinstance(splits, (int, np.integer)) and not isinstance(splits, bool):
        return kfold_splits(len(seqs), int(splits))
    if callable(splits):
        return list(splits(seqs))
    return list(splits)


def _clone(crf: Any, window_size: int, options: Dict[str, Any]) -> Any:
    """An unfitted model like the template ``crf`` with the given window size and trainer options."""
    model = type(crf)(crf.feature_type, crf.algorithm, window_size, crf.window_step, **options)
    model.devices, model.reference_bits = list(crf.devices), crf.reference_bits
    return model


def _fold_selection(model: Any, seqs: List[List[Any]], train_idx: Any, select: Optional[float],
                    correction_method: Optional[str]) -> Tuple[List[Any], Any, Any]:
    """A fold's training genes after ``fit``'s Fisher selection, with the significance table and the kept features
    (both None without ``select``)."""
    train_genes: List[Any] = [gene for i in train_idx for gene in seqs[i]]
    if select is None:
        return train_genes, None, None
    return model._select_features(train_genes, select, correction_method)


def _fold_truth(seqs: List[List[Any]], test_idx: Any) -> Tuple[List[Any], Dict[Tuple[str, str, int, int], bool]]:
    """A fold's test genes and their labels by gene key."""
    truth_genes = [gene for i in test_idx for gene in seqs[i]]
    truth: Dict[Tuple[str, str, int, int], bool] = {}
    for gene in truth_genes:
        key, label = _gene_key(gene), gene.average_probability > 0.5
        if truth.setdefault(key, label) != label:
            raise ValueError(f"two genes {key!r} with different labels")
    return truth_genes, truth


def cost_options(miss_cost: float, false_cost: float) -> Dict[str, Any]:
    """The ``label_costs`` option of the binary models from the command lines' ``--miss-cost`` (gold '1', predicted '0') and
    ``--false-cost`` (the reverse): no option at all when both are 0."""
    costs = {pair: float(c) for pair, c in ((("1", "0"), miss_cost), (("0", "1"), false_cost)) if c}
    return {"label_costs": costs} if costs else {}


def cross_validate(crf: Any, genes: Iterable[Any], splits: SplitSpec, *, shuffle: bool = True,
                   select: Optional[float] = None, correction_method: Optional[str] = None) -> CrossValidation:
    """Cross-validate the unfitted ``ClusterCRF`` template ``crf`` (its feature type, window, trainer options, ``devices``
    and ``reference_bits`` apply to every fold) on labelled ``genes``.

    ``splits`` selects the folds over the sequence groups (``group_genes``, in their shuffled order): an int k for
    ``kfold_splits(n_groups, k)``, a callable taking the groups and returning ``(train, test)`` index pairs (what
    leave-one-type-out needs, since its groups follow the shuffled order), or the pairs themselves.  Every fold's
    training data goes through ``fit``'s preparation in fold order (Fisher selection with ``select``, then the
    instances with their own shuffle); all folds are then optimised in one batch (``train.fit_training_sets``), and
    each predicts its test genes with their domain probabilities cleared."""
    from . import train

    seqs = group_genes(genes, shuffle=shuffle)
    folds_idx = _fold_indices(seqs, splits)
    template_options = {k: v for k, v in crf._options.items() if k != "algorithm"}
    models, sets, params = [], [], None
    for train_idx, _ in folds_idx:
        model = _clone(crf, crf.window_size, template_options)
        train_genes, model.significance, model.significant_features = _fold_selection(model, seqs, train_idx, select,
                                                                                      correction_method)
        ts, params = model._training_set(train_genes, shuffle=shuffle)
        models.append(model)
        sets.append(ts)
    devices = crf.devices or [0]
    results = train.fit_training_sets(sets, params, device=int(devices[0])) if sets else []
    folds = []
    for k, ((train_idx, test_idx), model, ts, result) in enumerate(zip(folds_idx, models, sets, results)):
        model._adopt_fit(ts, result)
        truth_genes, truth = _fold_truth(seqs, test_idx)
        predicted = model.predict_probabilities([_test_copy(gene) for gene in truth_genes])
        is_cluster = [truth[_gene_key(gene)] for gene in predicted]
        auroc, aupr = _metrics(is_cluster, [g.average_probability for g in predicted]) if predicted else (math.nan, math.nan)
        folds.append(Fold(index=k + 1, train=np.asarray(train_idx), test=np.asarray(test_idx), crf=model,
                          predicted=predicted, truth=is_cluster, auroc=auroc, aupr=aupr))
    return CrossValidation(folds)


# ---------------------------------------------------------------------------------------------- hyperparameter search
GRID_KEYS = ("c1", "c2", "window_size")
#: an axis a grid may have: the cost of a missed cluster gene, ``label_costs[('1', '0')]`` of the point's fits
COST_KEY = "miss_cost"
METRICS = ("aupr", "auroc")


def grid_points(grid: Dict[str, Sequence[Any]], crf: Any = None) -> List[Dict[str, Any]]:
    """The points of a ``{"c1": [...], "c2": [...], "window_size": [...]}`` grid, in grid order: c1 outermost, then c2,
    then the window size.  A key left out takes the template ``crf``'s value.  ``ValueError`` for an unknown key, an
    empty list, a regularisation strength that is negative or not finite, or a window size outside 1 .. 32.

    A grid may also have a ``"miss_cost"`` axis, in the form of the ``c1`` / ``c2`` axes: the points then carry the key
    (innermost), and a point's fits take ``label_costs[('1', '0')]`` from it (0: no cost).  Without it the points are
    what they always were."""
    unknown = sorted(set(grid) - set(GRID_KEYS) - {COST_KEY})
    if unknown:
        raise ValueError(f"grid: unknown parameter(s) {', '.join(map(repr, unknown))} (expected {', '.join(GRID_KEYS)})")
    values: Dict[str, List[Any]] = {}
    for key in GRID_KEYS:
        if key in grid:
            vals = list(grid[key])
        elif crf is None:
            raise ValueError(f"grid: no values for {key!r}")
        else:
            vals = [crf.window_size if key == "window_size" else crf._options.get(key, 0.0 if key == "c1" else 1.0)]
        if not vals:
            raise ValueError(f"grid: empty list of values for {key!r}")
        out = []
        for v in vals:
            if key == "window_size":
                if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= 32:
                    raise ValueError(f"grid: window_size {v!r} is not an integer in 1 .. 32 (the trainable windows)")
                out.append(int(v))
            else:  # (kept as given: the value is stored with the model's options)
                x = float(v)
                if isinstance(v, bool) or not math.isfinite(x) or x < 0:
                    raise ValueError(f"grid: {key} {v!r} is not a finite value >= 0")
                out.append(v)
        values[key] = out
    points = [{"c1": c1, "c2": c2, "window_size": w}
              for c1, c2, w in itertools.product(values["c1"], values["c2"], values["window_size"])]
    if COST_KEY not in grid:
        return points
    costs = list(grid[COST_KEY])
    if not costs:
        raise ValueError(f"grid: empty list of values for {COST_KEY!r}")
    for v in costs:
        if isinstance(v, bool) or not math.isfinite(float(v)) or float(v) < 0:
            raise ValueError(f"grid: {COST_KEY} {v!r} is not a finite value >= 0")
    return [{**pt, COST_KEY: v} for pt in points for v in costs]


def rank_points(auroc: Sequence[float], aupr: Sequence[float], metric: str = "aupr") -> List[int]:
    """Point indices best first: by ``metric`` (higher is better, NaN last), then by the other metric, then grid order."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {', '.join(METRICS)}, not {metric!r}")
    first, second = (aupr, auroc) if metric == "aupr" else (auroc, aupr)

    def key(i: int) -> Tuple[float, float, int]:
        a, b = float(first[i]), float(second[i])
        return (-a if not math.isnan(a) else math.inf, -b if not math.isnan(b) else math.inf, i)

    return sorted(range(len(first)), key=key)


def _nanmean(values: Sequence[float]) -> float:
    vals = [v for v in values if not math.isnan(v)]
    return float(np.mean(vals)) if vals else math.nan


def _fmt_float(x: float) -> str:
    return "nan" if math.isnan(x) else repr(float(x))


class GridFold:
    """One fold of one grid point: its 1-based ``index``, the sequence indices it trained and tested on, the fitted
    ``crf`` (``training_result_``), ``keys`` (sequence id, protein id, start, end) of the test genes in prediction
    order, their ``probabilities`` (float64, what ``average_probability`` of ``predict_probabilities``' genes gives),
    ``truth`` (``is_cluster`` joined by gene), ``auroc`` and ``aupr``."""

    def __init__(self, **kw: Any) -> None:
        self.__dict__.update(kw)

    def __repr__(self) -> str:
        return f"GridFold({self.index}, n_test={len(self.keys)}, auroc={self.auroc:.3f}, aupr={self.aupr:.3f})"


class GridSearch:
    """The result of ``grid_search``: ``points`` in grid order, ``folds[p]`` the folds of point p, per point the
    ``mean_auroc`` / ``mean_aupr`` over its folds (NaN folds left out) and the pooled ``auroc`` / ``aupr`` over the
    predictions of all its folds (what ``CrossValidation`` reports), ``ranking`` (best first, by ``metric``'s mean) and
    ``best`` (the first of the ranking)."""

    def __init__(self, points: List[Dict[str, Any]], folds: List[List[GridFold]], metric: str = "aupr") -> None:
        self.points, self.folds, self.metric = points, folds, metric
        self.mean_auroc = [_nanmean([f.auroc for f in fs]) for fs in folds]
        self.mean_aupr = [_nanmean([f.aupr for f in fs]) for fs in folds]
        self.auroc, self.aupr = [], []
        for fs in folds:
            labels = [t for f in fs for t in f.truth]
            probas = [p for f in fs for p in np.asarray(f.probabilities).tolist()]
            a, b = _metrics(labels, probas) if labels else (math.nan, math.nan)
            self.auroc.append(a)
            self.aupr.append(b)
        self.ranking = rank_points(self.mean_auroc, self.mean_aupr, metric)
        self.best = self.ranking[0]

    @property
    def best_point(self) -> Dict[str, Any]:
        return self.points[self.best]

    def table(self) -> bytes:
        """One row per (point, fold), points in grid order: ``point`` (1-based), ``c1``, ``c2``, ``window_size``,
        ``fold``, ``n_train`` / ``n_test`` (sequences), ``auroc``, ``aupr``."""
        cost = any(COST_KEY in pt for pt in self.points)  # (a grid with the axis: one more column, after window_size)
        rows = ["point\tc1\tc2\twindow_size\t" + (COST_KEY + "\t" if cost else "") + "fold\tn_train\tn_test\tauroc\taupr"]
        for p, (pt, fs) in enumerate(zip(self.points, self.folds)):
            for f in fs:
                rows.append("\t".join([str(p + 1), _fmt_float(pt["c1"]), _fmt_float(pt["c2"]), str(pt["window_size"]),
                                       *([_fmt_float(pt[COST_KEY])] if cost else []), str(f.index), str(len(f.train)), str(len(f.test)), _fmt_float(f.auroc),
                                       _fmt_float(f.aupr)]))
        return ("\n".join(rows) + "\n").encode("utf-8")

    def summary(self) -> bytes:
        """One row per point, in grid order: ``point``, ``c1``, ``c2``, ``window_size``, ``mean_auroc``, ``mean_aupr``,
        the pooled ``auroc`` / ``aupr``, and ``rank`` (1 = best)."""
        rank = {p: r + 1 for r, p in enumerate(self.ranking)}
        cost = any(COST_KEY in pt for pt in self.points)
        rows = ["point\tc1\tc2\twindow_size\t" + (COST_KEY + "\t" if cost else "") + "mean_auroc\tmean_aupr\tauroc\taupr\trank"]
        for p, pt in enumerate(self.points):
            rows.append("\t".join([str(p + 1), _fmt_float(pt["c1"]), _fmt_float(pt["c2"]), str(pt["window_size"]),
                                   *([_fmt_float(pt[COST_KEY])] if cost else []),
                                   _fmt_float(self.mean_auroc[p]), _fmt_float(self.mean_aupr[p]),
                                   _fmt_float(self.auroc[p]), _fmt_float(self.aupr[p]), str(rank[p])]))
        return ("\n".join(rows) + "\n").encode("utf-8")


def _encode_test_genes(genes: List[Any], feature_type: str):
    """The test genes as ``predict_probabilities`` orders and packs them, once per fold: sorted by (sequence, start), their
    domains by start, grouped by sequence; items CSR over a vocabulary of the fold's domain names (ids in order of first
    appearance).  Returns the sorted genes, contig_ptr, item_ptr, vocabulary ids and the vocabulary."""
    genes = sorted(genes, key=operator.attrgetter("source.id", "start"))
    for gene in genes:
        gene.protein.domains.sort(key=operator.attrgetter("start"))
    vocab: Dict[str, int] = {}
    contig_ptr, item_ptr, attr = [0], [0], []
    for _, group in itertools.groupby(genes, key=operator.attrgetter("source.id")):
        n_items = 0
        for gene in group:
            doms = gene.protein.domains
            if feature_type == "protein":
                for name in dict.fromkeys(d.name for d in doms):  # (a repeated domain is one feature)
                    attr.append(vocab.setdefault(name, len(vocab)))
                item_ptr.append(len(attr))
                n_items += 1
            elif doms:
                for d in doms:
                    attr.append(vocab.setdefault(d.name, len(vocab)))
                    item_ptr.append(len(attr))
                    n_items += 1
            else:
                item_ptr.append(len(attr))
                n_items += 1
        contig_ptr.append(contig_ptr[-1] + n_items)
    return (genes, np.asarray(contig_ptr, dtype=np.int32), np.asarray(item_ptr, dtype=np.int64),
            np.asarray(attr, dtype=np.int32), list(vocab))


def _score_test_genes(model: Any, encoded) -> np.ndarray:
    """``average_probability`` of every gene ``model.predict_probabilities`` would return for the encoded genes, scored
    through ``predict_probabilities_csr``: the fold's vocabulary is mapped to the model's attribute ids and the names the
    model does not know are dropped, as the object path drops them."""
    genes, contig_ptr, item_ptr, attr, vocab = encoded
    index = model.model._attr_index
    to_model = np.asarray([index.get(name, -1) for name in vocab] or [-1], dtype=np.int32)
    mapped = to_model[attr] if attr.size else attr
    known = mapped >= 0
    kept = np.concatenate([[0], np.cumsum(known, dtype=np.int64)])
    gene_ptr = kept[item_ptr].astype(np.int32)
    p_items = model.predict_probabilities_csr(contig_ptr, gene_ptr, mapped[known], pad=True)
    if model.feature_type == "protein":
        return np.ascontiguousarray(p_items, dtype=np.float64)
    out = np.empty(len(genes), dtype=np.float64)
    k = 0
    for i, gene in enumerate(genes):
        n = len(gene.protein.domains)
        if n:
            # (_annotate keeps the gene's own probability and sets the domains'; the average is the gene's if it has one)
            own = getattr(gene, "_probability", None)
            out[i] = own if own is not None else statistics.mean(float(x) for x in p_items[k:k + n])
            k += n
        else:
            out[i] = float(p_items[k])
            k += 1
    return out


def grid_search(crf: Any, genes: Iterable[Any], splits: SplitSpec, grid: Dict[str, Sequence[Any]], *,
                shuffle: bool = True, select: Optional[float] = None, correction_method: Optional[str] = None,
                metric: str = "aupr") -> GridSearch:
    """Cross-validate every point of ``grid`` (``grid_points``: ``c1``, ``c2``, ``window_size``) on labelled ``genes``, with
    the unfitted ``ClusterCRF`` template ``crf`` giving every other option.

    The point's ``cross_validate`` (a template with the point's values, the same ``splits``, ``shuffle``, ``select`` and
    random state) gives each (point, fold) the same model and test probabilities, bit for bit.  The work shared between
    points is done once: the groups are shuffled once, Fisher selection runs once per fold, the training set is built
    once per (fold, window size) from the same random state, all (point, fold) problems are fitted in one
    ``train.fit_grid``, and each fold's test genes are sorted and encoded once; every model then scores them through
    ``predict_probabilities_csr``.  The global ``random`` is left as ``cross_validate`` leaves it."""
    from . import train

    if metric not in METRICS:
        raise ValueError(f"metric must be one of {', '.join(METRICS)}, not {metric!r}")
    points = grid_points(grid, crf)
    seqs = group_genes(genes, shuffle=shuffle)
    folds_idx = _fold_indices(seqs, splits)
    template_options = {k: v for k, v in crf._options.items() if k != "algorithm"}

    def model_of(pt: Dict[str, Any]) -> Any:
        # (the template's options with the point's values, as the point's own template would hold them)
        options = dict(template_options)
        options.update({k: pt[k] for k in ("c1", "c2") if k in grid or k in options})
        if COST_KEY in pt:  # (the template's costs with the point's cost of a miss; a point without one keeps TrainerGrid)
            options["label_costs"] = {**(options.get("label_costs") or {}), ("1", "0"): pt[COST_KEY]}
        return _clone(crf, pt["window_size"], options)

    windows = list(dict.fromkeys(pt["window_size"] for pt in points))
    sets: List[Any] = []
    set_of: Dict[Tuple[int, int], int] = {}
    selection = []
    for f, (train_idx, _) in enumerate(folds_idx):
        train_genes, sig, keep = _fold_selection(model_of(points[0]), seqs, train_idx, select, correction_method)
        selection.append((sig, keep))
        state = random.getstate()
        for w in windows:  # (every window size draws the same shuffle: the state before it is restored)
            random.setstate(state)
            ts, _ = model_of({**points[0], "window_size": w})._training_set(train_genes, shuffle=shuffle)
            set_of[(f, w)] = len(sets)
            sets.append(ts)
    problems = [(set_of[(f, pt["window_size"])], train.trainer_params(model_of(pt)._options))
                for pt in points for f in range(len(folds_idx))]
    devices = crf.devices or [0]
    results = train.fit_grid(sets, problems, device=int(devices[0]))

    tests = []
    for train_idx, test_idx in folds_idx:
        truth_genes, truth = _fold_truth(seqs, test_idx)
        encoded = _encode_test_genes([_test_copy(gene) for gene in truth_genes], crf.feature_type)
        keys = [_gene_key(gene) for gene in encoded[0]]
        tests.append((encoded, keys, [truth[k] for k in keys]))

    folds: List[List[GridFold]] = []
    for p, pt in enumerate(points):
        row = []
        for f, (train_idx, test_idx) in enumerate(folds_idx):
            k = p * len(folds_idx) + f
            model = model_of(pt)
            model.significance, model.significant_features = selection[f]
            model._adopt_fit(sets[problems[k][0]], results[k])
            encoded, keys, is_cluster = tests[f]
            probas = _score_test_genes(model, encoded) if keys else np.zeros(0)
            auroc, aupr = _metrics(is_cluster, probas) if keys else (math.nan, math.nan)
            row.append(GridFold(index=f + 1, train=np.asarray(train_idx), test=np.asarray(test_idx), crf=model, keys=keys,
                                probabilities=probas, truth=is_cluster, auroc=auroc, aupr=aupr))
        folds.append(row)
    return GridSearch(points, folds, metric)


# ---------------------------------------------------------------------------------------------- front end
def label_genes(genes: List[Any], clusters: tables.ClusterTable) -> List[Any]:
    """``_common.label_genes``: probability 1 for a gene overlapping any cluster of its sequence, 0 otherwise."""
    by_seq: Dict[str, List[Tuple[int, int]]] = {}
    for i in range(len(clusters)):
        by_seq.setdefault(str(clusters.sequence_id[i]), []).append((int(clusters.start[i]), int(clusters.end[i])))
    out = []
    for gene in genes:
        spans = by_seq.get(gene.source.id, [])
        hit = any(s <= gene.end and gene.start <= e for s, e in spans)
        out.append(gene.with_probability(1 if hit else 0))
    return out


def annotate_genes(genes: List[Any], features: tables.FeatureTable) -> List[Any]:
    """``_common.annotate_genes``: the domains of the features table added to the genes of the genes table."""
    from .model import Domain

    index = {gene.protein.id: gene for gene in genes}
    if len(index) < len(genes):
        raise ValueError("Duplicate gene names in input genes")
    for i in range(len(features)):
        pid = str(features.protein_id[i])
        gene = index[pid]
        if gene.source.id != features.sequence_id[i]:
            raise ValueError(f"Mismatched source sequence for {pid!r}: {gene.source.id!r} != {features.sequence_id[i]!r}")
        if gene.start != features.start[i] or gene.end != features.end[i] or gene.strand.sign != features.strand[i]:
            raise ValueError(f"Mismatched gene coordinates for {pid!r}")
        p = features.cluster_probability[i]
        gene.protein.domains.append(Domain(str(features.domain[i]), int(features.domain_start[i]),
                                           int(features.domain_end[i]), str(features.hmm[i]), float(features.i_evalue[i]),
                                           float(features.pvalue[i]), None if math.isnan(p) else float(p)))
    return list(index.values())


def loto_groups(seqs: List[List[Any]], clusters: tables.ClusterTable) -> List[List[str]]:
    """The leave-one-type-out groups of the sequences: the ``type`` of the cluster on each sequence split on ``;``;
    ``Unknown``, empty or no cluster give no group (the sequence is always trained on, never tested).  Several clusters
    on one sequence are the reference's ``ValueError``."""
    index = {str(sid): str(ty) for sid, ty in zip(clusters.sequence_id, clusters.type)}
    if len(index) != len(clusters):
        raise ValueError("Training data contains several clusters per sequence")
    groups = []
    for seq in seqs:
        ty = next((index[g.source.id] for g in seq if g.source.id in index), None)
        if ty is None:
            print(f"warning: failed to find type of cluster in {seq[0].source.id!r}", file=sys.stderr)
            ty = ""
        groups.append([] if ty in ("", "Unknown") else ty.split(";"))
    return groups


def main(argv: Optional[List[str]] = None) -> int:
    from .crf import ClusterCRF

    ap = argparse.ArgumentParser(prog="python -m gecco_amd.cv", description=(
        "Cross-validate a CRF on labelled tables (gecco cv), with every fold trained in one batch on the device."))
    ap.add_argument("--genes", required=True, help="genes table (TSV)")
    ap.add_argument("--features", required=True, nargs="+", help="features table(s) (TSV)")
    ap.add_argument("--clusters", required=True, help="clusters table (TSV): the genes overlapping a cluster are positive")
    ap.add_argument("--e-filter", type=float, default=None,
                    help="accepted as gecco cv accepts it, and ignored as gecco cv ignores it")
    ap.add_argument("--p-filter", type=float, default=1e-9,
                    help="accepted as gecco cv accepts it, and ignored as gecco cv ignores it")
    ap.add_argument("--no-shuffle", dest="shuffle", action="store_false", help="do not shuffle the sequences")
    ap.add_argument("--seed", type=int, default=42, help="seed of random and numpy.random")
    ap.add_argument("--feature-type", choices=("protein", "domain"), default="protein")
    ap.add_argument("--window-size", type=int, default=5)
    ap.add_argument("--window-step", type=int, default=1)
    ap.add_argument("--c1", type=float, default=0.15)
    ap.add_argument("--c2", type=float, default=0.15)
    ap.add_argument("--miss-cost", type=float, default=0.0, help="training cost of a missed cluster gene (every fold)")
    ap.add_argument("--false-cost", type=float, default=0.0, help="training cost of a false cluster gene (every fold)")
    ap.add_argument("--select", type=float, default=None, help="fraction of domains kept by Fisher selection")
    ap.add_argument("--correction", default=None, help="multiple-testing correction of the selection p-values")
    ap.add_argument("--loto", action="store_true", help="leave-one-type-out instead of K-fold cross-validation")
    ap.add_argument("--splits", type=int, default=10, help="number of folds (K-fold)")
    ap.add_argument("-o", "--output", default="cv.tsv")
    args = ap.parse_args(argv)

    random.seed(args.seed)
    np.random.seed(args.seed)
    genes = tables.GeneTable.load(args.genes).to_genes()
    for path in args.features:
        genes = annotate_genes(genes, tables.FeatureTable.load(path))
    clusters = tables.ClusterTable.load(args.clusters)
    genes = label_genes(genes, clusters)

    crf = ClusterCRF(args.feature_type, algorithm="lbfgs", window_size=args.window_size, window_step=args.window_step,
                     c1=args.c1, c2=args.c2, **cost_options(args.miss_cost, args.false_cost))
    if args.loto:
        def splits(seqs):
            return list(LeaveOneGroupOut().split(seqs, groups=loto_groups(seqs, clusters)))
    else:
        splits = args.splits
    result = cross_validate(crf, genes, splits, shuffle=args.shuffle, select=args.select,
                            correction_method=args.correction)
    for f in result.folds:
        print(f"fold {f.index}: AUROC={f.auroc:.3f} AUPR={f.aupr:.3f}", file=sys.stderr)
    print(f"cross-validation: AUROC={result.auroc:.3f} AUPR={result.aupr:.3f}", file=sys.stderr)
    result.write(args.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
