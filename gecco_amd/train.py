"""Host side of CRF training (``ClusterCRF.fit``): the training set, CRFsuite's feature generation, and the L-BFGS /
OWL-QN optimiser.  The objective and its gradient are evaluated on the device (``_native.Trainer``,
``csrc/crf_train.hip``; sets of 3 to 32 labels: ``_native.TrainerGeneral``, ``csrc/crf_train_general.hip``; sets whose
instances are the whole sequences, ``window=None``: ``_native.TrainerSequences``, same file); everything here is cheap
bookkeeping around that.

What is reproduced ([EXT] CRFsuite 0.12 ``crf1d`` + ``train_lbfgs`` with libLBFGS, as sklearn-crfsuite drives it):

* instances are the sliding windows of every sequence (``gecco/crf/__init__.py:364-367``), or with ``window=None`` the
  sequences themselves, as CRFsuite is driven outside GECCO; labels and attributes get ids
  in order of first appearance over the instances, attribute names before the label of every item;
* a state feature exists for every observed (attribute, label) pair and a transition feature for every observed label
  bigram inside an instance; ``all_possible_states`` / ``all_possible_transitions`` add the unobserved ones and
  ``min_freq`` drops features seen fewer times; feature ids follow (type, source, destination) order;
* ``f(w) = sum of -log p(y | x) over the instances + c2 * |w|^2 + c1 * |w|_1``: OWL-QN when ``c1 > 0``;
* libLBFGS's defaults as CRFsuite sets them: 6 memories, epsilon 1e-5 (stop when |g| < epsilon * max(1, |w|)), a
  delta test over a period of 10 iterations (1e-5), no iteration limit, 20 line-search trials.  The line search is
  backtracking: with the sufficient-decrease test on the orthant-projected step when ``c1 > 0`` (what CRFsuite uses
  there), and with the Wolfe conditions when ``c1 = 0`` (CRFsuite's default there is More-Thuente; the optimum is
  the same, the iterates are not).

``python -m gecco_amd.train`` is ``gecco train``: labelled tables in, a model directory out (``train_cli``).
"""
import math
import sys
from collections.abc import Mapping
from typing import Callable, Dict, Generator, List, Optional, Sequence, Tuple

import numpy as np

__all__ = ["TRAINER_DEFAULTS", "MAX_LABELS", "trainer_params", "minimize", "minimize_steps", "OptimizeResult", "TrainingSet",
           "item_attributes", "build_training_set", "fit_training_set", "fit_training_sets", "fit_grid", "model_blob"]

#: the most labels a training set may have (``_native.TrainerGeneral`` / ``TrainerSequences``; the inference kernels' limit)
MAX_LABELS = 32
#: libLBFGS parameters as CRFsuite's ``train_lbfgs`` sets them (``max_iterations`` None = unbounded)
TRAINER_DEFAULTS = {"num_memories": 6, "epsilon": 1e-5, "period": 10, "delta": 1e-5, "max_iterations": None}
#: options of ``sklearn_crfsuite.CRF`` accepted without effect on the fit
_SILENT_OPTIONS = ("verbose",)


def trainer_params(options: Dict[str, object]) -> Dict[str, object]:
    """Check ``sklearn_crfsuite.CRF``-style options (what ``ClusterCRF(**kwargs)`` stores) and return the complete set:
    ``c1``, ``c2``, the feature-generation options and the five libLBFGS parameters, defaults filled in.

    ``label_costs`` (not a CRFsuite option): a mapping ``{(gold, predicted): cost}`` of label names, the softmax-margin
    cost matrix of the training objective (``fit_training_set``); missing pairs cost 0.  A cost that is negative, NaN or
    infinite, or a non-zero cost on the diagonal, is a ``ValueError`` here; a label the training set does not have is one
    at fit time.  Returned as a dict of the non-zero entries, or None (the default, and what an empty mapping gives)."""
    out: Dict[str, object] = {"c1": 0.0, "c2": 1.0, "min_freq": 0.0, "all_possible_states": False,
                              "all_possible_transitions": False, "label_costs": None, **TRAINER_DEFAULTS}
    for key, value in options.items():
        if key == "algorithm":
            if value != "lbfgs":
                raise ValueError(f"unsupported training algorithm {value!r} (only 'lbfgs' is implemented)")
            continue
        if value is None or key in _SILENT_OPTIONS:
            continue
        if key in ("c1", "c2", "epsilon", "delta", "min_freq"):
            value = float(value)
            if value < 0 or not math.isfinite(value):
                raise ValueError(f"invalid value for {key}: {value}")
        elif key in ("num_memories", "period", "max_iterations"):
            value = int(value)
            if value < (1 if key != "period" else 0):
                raise ValueError(f"invalid value for {key}: {value}")
        elif key in ("all_possible_states", "all_possible_transitions"):
            value = bool(value)
        elif key == "label_costs":
            value = _checked_label_costs(value)
        else:
            raise ValueError(f"unsupported trainer option {key!r}")
        out[key] = value
    return out


def _checked_label_costs(costs) -> Optional[Dict[Tuple[object, object], float]]:
    """``label_costs`` as ``trainer_params`` keeps it: the non-zero entries, or None when there is none."""
    if not isinstance(costs, Mapping):
        raise ValueError(f"label_costs is a mapping {{(gold, predicted): cost}}, got {type(costs).__name__}")
    out = {}
    for pair, cost in costs.items():
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError(f"label_costs: a key is a (gold, predicted) pair of labels, got {pair!r}")
        gold, predicted = pair
        cost = float(cost)
        if cost < 0 or not math.isfinite(cost):
            raise ValueError(f"label_costs: the cost of {(gold, predicted)!r} is {cost}: costs are finite and not negative")
        if gold == predicted and cost != 0:
            raise ValueError(f"label_costs: the cost of {(gold, predicted)!r} is {cost}: predicting the gold label costs 0")
        if cost != 0:
            out[(gold, predicted)] = cost
    return out or None


# ---------------------------------------------------------------------------------------------- optimiser
class OptimizeResult:
    def __init__(self, x: np.ndarray, f: float, n_iter: int, n_eval: int, status: str):
        self.x, self.f, self.n_iter, self.n_eval, self.status = x, f, n_iter, n_eval, status

    def __repr__(self) -> str:
        return f"OptimizeResult(f={self.f!r}, n_iter={self.n_iter}, n_eval={self.n_eval}, status={self.status!r})"


def _pseudo_gradient(x: np.ndarray, g: np.ndarray, c1: float) -> np.ndarray:
    """OWL-QN's pseudo-gradient of f + c1 |x|_1: the one-sided derivative of steepest descent."""
    pg = np.where(x < 0, g - c1, np.where(x > 0, g + c1, 0.0))
    zero = x == 0
    pg = np.where(zero & (g + c1 < 0), g + c1, pg)
    pg = np.where(zero & (g - c1 > 0), g - c1, pg)
    return pg


def minimize(fg: Callable[[np.ndarray], Tuple[float, np.ndarray]], x0: np.ndarray, c1: float = 0.0,
             num_memories: int = 6, epsilon: float = 1e-5, period: int = 10, delta: float = 1e-5,
             max_iterations: Optional[int] = None, max_linesearch: int = 20,
             callback: Optional[Callable[[int, float, np.ndarray], None]] = None,
             skip_nonpositive_curvature: bool = False) -> OptimizeResult:
    """Minimise ``fg(x)[0] + c1 * |x|_1`` with L-BFGS (``c1 = 0``) or OWL-QN (``c1 > 0``), libLBFGS's algorithm.
    ``fg`` returns the smooth part of the objective and its gradient.  Stops on the gradient test, the delta test, the
    iteration limit, or a failed line search (status "line search failed": the point before that search is returned, as
    libLBFGS does; near the optimum this is where the objective's rounding hides any further decrease).  A trial point
    whose f or g is not finite fails the sufficient-decrease test, so the step is halved: it is never accepted.  A start
    ``x0`` whose f or g is not finite raises ``ValueError``.  This drives ``minimize_steps`` with ``fg``.

    ``skip_nonpositive_curvature`` (for objectives that are not convex; off by default, and then every iterate is what it
    always was): a correction pair with y.s <= 0 is not stored, the usual safeguard.  The Wolfe search of ``c1 = 0`` forces
    y.s > 0 on every accepted step, but OWL-QN's search only backtracks, so on a non-convex objective it can accept a step
    with y.s <= 0, and the two-loop recursion then divides by it.  The direction after a skipped pair comes from the pairs
    already stored (steepest descent, with libLBFGS's first step 1 / |d|, when there is none)."""
    steps = minimize_steps(x0, c1=c1, num_memories=num_memories, epsilon=epsilon, period=period, delta=delta,
                           max_iterations=max_iterations, max_linesearch=max_linesearch, callback=callback,
                           skip_nonpositive_curvature=skip_nonpositive_curvature)
    try:
        x = next(steps)
        while True:
            x = steps.send(fg(x))
    except StopIteration as stop:
        return stop.value


def minimize_steps(x0: np.ndarray, c1: float = 0.0, num_memories: int = 6, epsilon: float = 1e-5, period: int = 10,
                   delta: float = 1e-5, max_iterations: Optional[int] = None, max_linesearch: int = 20,
                   callback: Optional[Callable[[int, float, np.ndarray], None]] = None,
                   skip_nonpositive_curvature: bool = False
                   ) -> Generator[np.ndarray, Tuple[float, np.ndarray], OptimizeResult]:
    """``minimize`` in stepping form, for driving several optimisations in lock-step: a generator that yields every
    point to evaluate, takes ``(f, g)`` of the smooth part there back through ``send``, and returns the
    ``OptimizeResult`` (``StopIteration.value``).  The same iterates, statuses and evaluation counts as ``minimize``."""
    ftol, wolfe, min_step, max_step = 1e-4, 0.9, 1e-20, 1e20
    x = np.array(x0, dtype=np.float64)
    n_eval = 0

    def evaluate(xv):
        nonlocal n_eval
        n_eval += 1
        f, g = yield xv
        g = np.asarray(g, dtype=np.float64)
        if c1 > 0:
            f = f + c1 * float(np.abs(xv).sum())
        return float(f), g

    def finite(fv, gv):
        return math.isfinite(fv) and bool(np.all(np.isfinite(gv)))

    fx, g = yield from evaluate(x)
    if not finite(fx, g):
        raise ValueError(f"minimize: the objective is not finite at the start point (f = {fx}, "
                         f"{int(np.count_nonzero(~np.isfinite(g)))} non-finite gradient entries)")
    pg = _pseudo_gradient(x, g, c1) if c1 > 0 else g
    history = [fx] * max(period, 1)
    d = -pg
    xnorm, gnorm = max(float(np.linalg.norm(x)), 1.0), float(np.linalg.norm(pg))
    if gnorm / xnorm <= epsilon:
        return OptimizeResult(x, fx, 0, n_eval, "converged")
    step = 1.0 / float(np.linalg.norm(d))
    mem_s: List[np.ndarray] = []
    mem_y: List[np.ndarray] = []
    mem_ys: List[float] = []
    k = 1
    while True:
        xp, gp, pgp, fp = x, g, pg, fx
        # ---- line search
        count = 0
        ok = False
        if c1 > 0:
            orthant = np.where(xp == 0, -pgp, xp)
            while True:
                x = xp + step * d
                x = np.where(x * orthant <= 0, 0.0, x)
                fx, g = yield from evaluate(x)
                count += 1
                if finite(fx, g) and fx <= fp + ftol * float(np.dot(x - xp, pgp)):
                    ok = True
                    break
                if step < min_step or step > max_step or count >= max_linesearch:
                    break
                step *= 0.5
        else:
            dginit = float(np.dot(gp, d))
            if dginit > 0:
                x, fx, g = xp, fp, gp
                return OptimizeResult(x, fx, k - 1, n_eval, "search direction is not a descent direction")
            while True:
                x = xp + step * d
                fx, g = yield from evaluate(x)
                count += 1
                if not finite(fx, g) or fx > fp + step * ftol * dginit:
                    width = 0.5
                elif float(np.dot(g, d)) < wolfe * dginit:
                    width = 2.1
                else:
                    ok = True
                    break
                if step < min_step or step > max_step or count >= max_linesearch:
                    break
                step *= width
        if not ok:
            # libLBFGS returns the point before the failed search
            return OptimizeResult(xp, fp, k - 1, n_eval, "line search failed")
        pg = _pseudo_gradient(x, g, c1) if c1 > 0 else g
        if callback is not None:
            callback(k, fx, x)
        # ---- stopping tests
        xnorm, gnorm = max(float(np.linalg.norm(x)), 1.0), float(np.linalg.norm(pg))
        if gnorm / xnorm <= epsilon:
            return OptimizeResult(x, fx, k, n_eval, "converged")
        if period > 0:
            if k >= period:
                rate = (history[k % period] - fx) / fx if fx != 0 else 0.0
                if rate < delta:
                    return OptimizeResult(x, fx, k, n_eval, "delta test")
            history[k % period] = fx
        if max_iterations is not None and k >= max_iterations:
            return OptimizeResult(x, fx, k, n_eval, "maximum number of iterations")
        # ---- L-BFGS direction (two-loop recursion on the smooth gradient's differences)
        s, y = x - xp, g - gp
        ys, yy = float(np.dot(y, s)), float(np.dot(y, y))
        if not (skip_nonpositive_curvature and not ys > 0):  # (a pair without positive curvature: not stored, on request)
            mem_s.append(s)
            mem_y.append(y)
            mem_ys.append(ys)
            scale = ys / yy
            if len(mem_s) > num_memories:
                mem_s.pop(0)
                mem_y.pop(0)
                mem_ys.pop(0)
        d = -pg
        if not mem_s:  # (only after a skipped first pair: steepest descent again, with the first iteration's step)
            if c1 > 0:
                d = np.where(d * pg >= 0, 0.0, d)
            dnorm = float(np.linalg.norm(d))
            step = 1.0 / dnorm if dnorm > 0 else 1.0
            k += 1
            continue
        alphas = []
        for si, yi, ysi in zip(reversed(mem_s), reversed(mem_y), reversed(mem_ys)):
            a = float(np.dot(si, d)) / ysi
            alphas.append(a)
            d = d - a * yi
        d = d * scale
        for si, yi, ysi, a in zip(mem_s, mem_y, mem_ys, reversed(alphas)):
            b = float(np.dot(yi, d)) / ysi
            d = d + (a - b) * si
        if c1 > 0:
            d = np.where(d * pg >= 0, 0.0, d)
        step = 1.0
        k += 1


# ---------------------------------------------------------------------------------------------- training set
class TrainingSet:
    """Encoded training data and the generated features.

    ``seq_ptr`` / ``item_ptr`` / ``attr_id`` / ``labels``: the sequences as CSR over items and attribute ids (ids in order
    of first appearance over the instances); ``labels_`` / ``attrs_``: the id -> name tables; ``state_attr``,
    ``state_label``, ``trans_src``, ``trans_dst``: the generated features (state features first, feature id = position);
    ``state_fid`` [A, L] / ``trans_fid`` [L, L]: feature id of every pair, -1 where there is none.  ``attr_value``: the value
    of every attribute entry (float64, parallel to ``attr_id``), or None when every item was plain names (each entry then
    weighs 1, and the set trains on the unvalued kernels).  ``allowed``: one uint32 mask per item, bit y set when label y is
    allowed on it, or None when every item has exactly one label (a labelled set, which trains on the labelled kernels); a set
    with ``allowed`` is partially labelled, trains by marginal likelihood, and its ``labels`` hold every item's lowest allowed
    id, which nothing reads.  ``seq_weight``: one float64 weight >= 0 per sequence, which every instance cut from it carries
    in the objective, or None (every sequence weighs 1, and the set trains on the kernels it always did)."""

    attr_value = None  # (a set built without the field has no values)
    allowed = None     # (and is labelled)
    seq_weight = None  # (and every sequence weighs 1)

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def num_features(self) -> int:
        return len(self.state_attr) + len(self.trans_src)

    @property
    def num_labels(self) -> int:
        return len(self.labels_)

    def native_args(self) -> tuple:
        """The set as ``_native.TrainerGrid`` takes it (``TrainerBatch``: without the last two, window and step); a set of
        whole sequences (``window is None``) as ``_native.TrainerSequences`` takes it, which is without those two."""
        args = (self.seq_ptr, self.item_ptr, self.attr_id, self.labels, len(self.attrs_), self.state_fid, self.trans_fid,
                self.num_features)
        return args if self.window is None else args + (self.window, self.step)


def _coverage(n: int, window: int, step: int) -> np.ndarray:
    """Number of windows (gecco/_meta.py:124-132 ``sliding_window``) covering every position of a sequence of n items."""
    cov = np.zeros(n + 1, dtype=np.int64)
    starts = np.arange(0, n + 1 - window, step)
    np.add.at(cov, starts, 1)
    np.add.at(cov, starts + window, -1)
    return np.cumsum(cov)[:n]


def _pair_coverage(n: int, window: int, step: int) -> np.ndarray:
    """Number of windows holding both positions p - 1 and p, for p = 1 .. n - 1."""
    if n < 2 or window < 2:
        return np.zeros(max(n - 1, 0), dtype=np.int64)
    nw = (n - window) // step + 1
    p = np.arange(1, n)
    lo = np.maximum(0, -((window - 1 - p) // step))  # ceil((p - W + 1) / step)
    hi = np.minimum(nw - 1, (p - 1) // step)
    return np.maximum(hi - lo + 1, 0)


def _mapping_pairs(item: Mapping, prefix: str, out: List[Tuple[str, float]]) -> None:
    for key, value in item.items():
        key = prefix + str(key)
        if isinstance(value, Mapping):
            _mapping_pairs(value, key + ":", out)
        elif isinstance(value, (bool, np.bool_)):
            out.append((key, 1.0 if value else 0.0))
        elif isinstance(value, (int, float, np.integer, np.floating)):
            out.append((key, float(value)))
        elif isinstance(value, (str, bytes)):
            out.append((f"{key}:{value.decode() if isinstance(value, bytes) else value}", 1.0))
        elif isinstance(value, (list, tuple, set, frozenset)):
            out.extend((f"{key}:{s}", 1.0) for s in value)
        else:
            raise ValueError(f"attribute {key!r}: a value is a number, a bool, a string, a list or set of strings, or a dict; "
                             f"got {type(value).__name__}")


def item_attributes(item) -> Tuple[List[str], Optional[List[float]]]:
    """One item as ``(names, values)``; ``values`` is None for an item of plain names (every attribute weighs 1).

    * an iterable of names: the names, duplicates kept as they are given (``values`` None);
    * an iterable of ``(name, value)`` pairs (a bare name among them weighs 1);
    * a mapping, by python-crfsuite's ``ItemSequence`` conversion: ``{k: number}`` -> (k, value); ``{k: bool}`` -> (k, 1.0 /
      0.0); ``{k: str}`` -> ("k:str", 1.0); ``{k: [s1, s2]}`` or a set -> ("k:s1", 1.0), ...; ``{k: {...}}`` -> the inner
      mapping's attributes with the prefix "k:".

    A value that is NaN or infinite raises ``ValueError``; so does an item that is a string."""
    if isinstance(item, (str, bytes)):
        raise ValueError("an item is an iterable of attribute names, of (name, value) pairs, or a mapping, not a string")
    if isinstance(item, Mapping):
        pairs: List[Tuple[str, float]] = []
        _mapping_pairs(item, "", pairs)
    else:
        entries = list(item)
        if all(isinstance(e, str) for e in entries):
            return entries, None
        pairs = []
        for e in entries:
            if isinstance(e, str):
                pairs.append((e, 1.0))
                continue
            try:
                name, value = e
            except (TypeError, ValueError):
                raise ValueError(f"an attribute is a name or a (name, value) pair, got {e!r}") from None
            pairs.append((str(name), float(value)))
    for name, value in pairs:
        if not math.isfinite(value):
            raise ValueError(f"attribute {name!r} has the value {value}: values must be finite")
    return [name for name, _ in pairs], [value for _, value in pairs]


def _label_entry(entry):
    """One entry of ``sequence_labels`` as a tuple of label names, in the order their ids are assigned, or None for "every
    label": a plain label is itself, a set / frozenset / list / tuple of labels is its names sorted (duplicates once)."""
    if entry is None:
        return None
    if isinstance(entry, (set, frozenset, list, tuple)):
        if len(entry) == 0:
            raise ValueError("an item's set of allowed labels is empty: every item needs at least one label")
        return tuple(sorted(set(entry)))
    return (entry,)


def build_training_set(sequences: Sequence[Sequence[Sequence[str]]], sequence_labels: Sequence[Sequence[str]],
                       window: Optional[int] = None, step: Optional[int] = None, min_freq: float = 0.0,
                       all_possible_states: bool = False, all_possible_transitions: bool = False,
                       max_labels: int = 2, sample_weight=None) -> TrainingSet:
    """Encode sequences (per item the attribute names, per item a label) and generate CRFsuite's features over the
    sliding-window instances.  An item may also be a list of ``(name, value)`` pairs or a mapping (``item_attributes``):
    the set then has ``attr_value``, a state feature (a, y) exists if the pair is observed on a covered item whatever the
    value (0 included), and its frequency, which ``min_freq`` compares, is the sum of value x coverage.  A NaN or infinite
    value raises ``ValueError``.  A set of plain names is what it always was, with ``attr_value`` None.  Every sequence must hold at least `window` items.  Raises ``ValueError`` unless exactly
    two labels occur, or, with ``max_labels`` = m in 2..32, unless 2 to m labels occur.

    ``window=None``: the instances are the whole sequences, of any length from one item up (``step`` is not read, and the
    set's ``window`` and ``step`` are None): a state feature's frequency is its plain count, a transition's its count over
    adjacent pairs.  An empty sequence raises ``ValueError``.

    Partial labels: an entry of ``sequence_labels`` may also be a ``set`` / ``frozenset`` / ``list`` / ``tuple`` of labels,
    the labels allowed on that item, or None, every label of the set.  Label ids follow first appearance as ever, the names
    inside a set scanned in sorted order (None names no label).  A feature is generated when some allowed path of some
    instance fires it: state (a, y) when a sits on a covered item whose set holds y, transition (i, j) when two adjacent items
    inside an instance hold i and j; its frequency is the sum over those occurrences of value x coverage (pair coverage
    for a transition).  The set then has ``allowed`` and trains by marginal likelihood (``fit_training_set``).  A set whose
    entries all name one label, however written, is the labelled set it always was, without ``allowed``.  An empty set is a
    ``ValueError``, and so is a None where fewer than 2 labels occur overall.

    ``sample_weight``: None, or one finite number >= 0 per sequence (anything else is a ``ValueError``), kept as the set's
    ``seq_weight``.  Feature generation, the frequencies ``min_freq`` compares and the windows do not depend on it."""
    if not 2 <= int(max_labels) <= MAX_LABELS:
        raise ValueError(f"max_labels must lie in 2..{MAX_LABELS}, got {max_labels}")
    seq_weight = None
    if sample_weight is not None:
        seq_weight = np.array(sample_weight, dtype=np.float64)
        if seq_weight.shape != (len(sequences),):
            raise ValueError(f"sample_weight holds one weight per sequence: expected {len(sequences)}, got shape {seq_weight.shape}")
        bad = np.flatnonzero(~(np.isfinite(seq_weight) & (seq_weight >= 0)))
        if bad.size:
            raise ValueError(f"sample_weight[{int(bad[0])}] is {seq_weight[bad[0]]}: weights are finite and not negative")
    whole = window is None
    if whole:
        step = None
        for k, items in enumerate(sequences):
            if len(items) == 0:
                raise ValueError(f"sequence {k} has no items: a whole-sequence instance holds at least one")
    converted = [[item_attributes(item) for item in items] for items in sequences]
    valued = any(vals is not None for items in converted for _, vals in items)
    sequences = [[names for names, _ in items] for items in converted]
    entries = [[_label_entry(lab) for lab in labs] for labs in sequence_labels]
    partial = any(e is None or len(e) != 1 for labs in entries for e in labs)
    if not partial:  # (every item names one label: the labels as they are given, or the one member of a set)
        sequence_labels = [[e[0] for e in labs] for labs in entries]
    label_index: Dict[str, int] = {}
    attr_index: Dict[str, int] = {}
    covs = []
    # ids in order of first appearance over the instances: an item no window covers is never seen by CRFsuite
    for items, labs in zip(sequences, sequence_labels):
        cov = np.ones(len(items), dtype=np.int64) if whole else _coverage(len(items), window, step)
        covs.append(cov)
        for names, lab, c in zip(items, labs, cov.tolist()):
            if c == 0:
                continue
            for name in names:
                if name not in attr_index:
                    attr_index[name] = len(attr_index)
            if not partial:
                if lab not in label_index:
                    label_index[lab] = len(label_index)
        if partial:  # (the same scan, over the names of every covered item's set)
            for e, c in zip(entries[len(covs) - 1], cov.tolist()):
                for lab in (e or ()) if c else ():
                    if lab not in label_index:
                        label_index[lab] = len(label_index)
    if max_labels == 2 and len(label_index) != 2:
        raise ValueError(f"training needs exactly 2 labels, found {len(label_index)} ({sorted(label_index)}): "
                         "GECCO's protein and domain modes are binary")
    if not 2 <= len(label_index) <= max_labels:
        raise ValueError(f"training needs 2 to {max_labels} labels, found {len(label_index)} ({sorted(label_index)})")
    L, A = len(label_index), len(attr_index)
    seq_ptr = [0]
    item_ptr = [0]
    attr_id: List[int] = []
    labels: List[int] = []
    attr_value: List[float] = []
    masks: List[int] = []
    for items, labs, conv, ents in zip(sequences, sequence_labels, converted, entries):
        for names, lab, (_, vals), e in zip(items, labs, conv, ents):
            # (names outside the dictionary can only sit on items no window covers: they carry no weight)
            attr_id.extend(attr_index[nm] for nm in names if nm in attr_index)
            if valued:  # (an item of plain names inside a valued set: every value is 1)
                vals = vals if vals is not None else [1.0] * len(names)
                attr_value.extend(v for nm, v in zip(names, vals) if nm in attr_index)
            item_ptr.append(len(attr_id))
            if partial:  # (names outside the dictionary sit on items no window covers, whose mask nothing trains on)
                mask = (1 << L) - 1 if e is None else sum(1 << label_index[nm] for nm in e if nm in label_index)
                masks.append(mask or 1)
                labels.append((masks[-1] & -masks[-1]).bit_length() - 1)
            else:
                labels.append(label_index.get(lab, 0))
        seq_ptr.append(len(labels))
    seq_ptr_a = np.array(seq_ptr, dtype=np.int32)
    item_ptr_a = np.array(item_ptr, dtype=np.int64)
    attr_a = np.array(attr_id, dtype=np.int64)
    lab_a = np.array(labels, dtype=np.int64)
    cov_a = np.concatenate(covs) if covs else np.zeros(0, dtype=np.int64)

    # observed frequencies: state (a, y) once per window holding the item, transitions once per window holding the pair
    deg = np.diff(item_ptr_a)
    occ_item = np.repeat(np.arange(len(lab_a)), deg)
    state_freq = np.zeros(A * L, dtype=np.float64)
    val_a = np.array(attr_value, dtype=np.float64) if valued else None
    occ_freq = cov_a[occ_item].astype(np.float64)
    if valued:  # frequency = value x coverage (a pair seen with value 0 alone is still seen, below)
        occ_freq = val_a * occ_freq
    np.add.at(state_freq, attr_a * L + lab_a[occ_item], occ_freq)
    state_seen = np.zeros(A * L, dtype=bool)
    state_seen[(attr_a * L + lab_a[occ_item])[cov_a[occ_item] > 0]] = True
    trans_freq = np.zeros(L * L, dtype=np.float64)
    trans_seen = np.zeros(L * L, dtype=bool)
    for s in range(len(seq_ptr) - 1):
        b, e = seq_ptr[s], seq_ptr[s + 1]
        pc = np.ones(e - b - 1, dtype=np.int64) if whole else _pair_coverage(e - b, window, step)
        pair = lab_a[b:e - 1] * L + lab_a[b + 1:e]
        np.add.at(trans_freq, pair, pc.astype(np.float64))
        trans_seen[pair[pc > 0]] = True
    if partial:  # one rule for both kinds of feature: some allowed path of some instance fires it (in place of the above)
        ok = ((np.array(masks, dtype=np.uint64)[:, None] >> np.arange(L, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
        state_freq = np.zeros((A, L), dtype=np.float64)
        np.add.at(state_freq, attr_a, occ_freq[:, None] * ok[occ_item])
        state_freq = state_freq.ravel()
        state_seen = np.zeros((A, L), dtype=bool)
        covered = cov_a[occ_item] > 0
        np.logical_or.at(state_seen, attr_a[covered], ok[occ_item[covered]])
        state_seen = state_seen.ravel()
        trans_freq = np.zeros((L, L), dtype=np.float64)
        trans_seen = np.zeros((L, L), dtype=bool)
        for s in range(len(seq_ptr) - 1):
            b, e = seq_ptr[s], seq_ptr[s + 1]
            pc = np.ones(e - b - 1, dtype=np.int64) if whole else _pair_coverage(e - b, window, step)
            pairs = ok[b:e - 1, :, None] & ok[b + 1:e, None, :]  # [positions, L, L]
            trans_freq += (pairs * pc[:, None, None].astype(np.float64)).sum(axis=0)
            trans_seen |= pairs[pc > 0].any(axis=0)
        trans_freq, trans_seen = trans_freq.ravel(), trans_seen.ravel()
    if all_possible_states:
        state_seen[:] = True
    if all_possible_transitions:
        trans_seen[:] = True
    state_keep = state_seen & (state_freq >= min_freq)
    trans_keep = trans_seen & (trans_freq >= min_freq)
    s_idx = np.flatnonzero(state_keep)  # (attribute, label) order
    t_idx = np.flatnonzero(trans_keep)  # (source, destination) order
    state_fid = np.full(A * L, -1, dtype=np.int32)
    state_fid[s_idx] = np.arange(len(s_idx), dtype=np.int32)
    trans_fid = np.full(L * L, -1, dtype=np.int32)
    trans_fid[t_idx] = len(s_idx) + np.arange(len(t_idx), dtype=np.int32)
    return TrainingSet(
        seq_ptr=seq_ptr_a, item_ptr=item_ptr_a.astype(np.int32), attr_id=attr_a.astype(np.int32),
        labels=lab_a.astype(np.int32), labels_=list(label_index), attrs_=list(attr_index),
        state_attr=s_idx // L, state_label=s_idx % L, trans_src=t_idx // L, trans_dst=t_idx % L,
        state_fid=state_fid.reshape(A, L), trans_fid=trans_fid.reshape(L, L), window=window, step=step,
        attr_value=val_a, allowed=np.array(masks, dtype=np.uint32) if partial else None, seq_weight=seq_weight,
    )


def _cost_matrix(ts: TrainingSet, params: Optional[Dict[str, object]]) -> Optional[np.ndarray]:
    """``params['label_costs']`` as the matrix [L, L] (row = gold) over the label ids of ``ts``, or None without costs.  A
    label the set does not have, and costs on a partially labelled set, raise ``ValueError``."""
    costs = (params or {}).get("label_costs")
    if not costs:
        return None
    if ts.allowed is not None:
        raise ValueError("label_costs need a gold label on every item: the training set is partially labelled")
    index = {name: k for k, name in enumerate(ts.labels_)}
    C = np.zeros((len(index), len(index)), dtype=np.float64)
    for (gold, predicted), cost in costs.items():
        for name in (gold, predicted):
            if name not in index:
                raise ValueError(f"label_costs names the label {name!r}, which the training set does not have "
                                 f"(its labels: {list(ts.labels_)})")
        C[index[gold], index[predicted]] = cost
    return C


def _weighting(sets: Sequence[TrainingSet], params: Sequence[Optional[Dict[str, object]]]) -> Dict[str, list]:
    """The ``weights=`` / ``costs=`` keywords of a ``_native`` trainer of these problems: none at all when no problem has
    sequence weights or label costs (the call it always was), else both lists, None for a problem without."""
    weights = [ts.seq_weight for ts in sets]
    costs = [_cost_matrix(ts, p) for ts, p in zip(sets, params)]
    if all(w is None for w in weights) and all(c is None for c in costs):
        return {}
    return {"weights": weights, "costs": costs}


def fit_training_set(ts: TrainingSet, params: Dict[str, object], device: int = 0,
                     callback: Optional[Callable[[int, float, np.ndarray], None]] = None) -> OptimizeResult:
    """Optimise the weights of the generated features on the device: L-BFGS / OWL-QN from w = 0.  A set of whole
    sequences (``window is None``) takes ``_native.TrainerSequences`` at any label count; of the windowed sets, one of two
    labels takes the 2-label trainer, one of more labels ``_native.TrainerGeneral``.  A set with values (``attr_value``)
    takes ``TrainerGeneral`` at any label count, 2 included, or ``TrainerSequences``, with its values.

    A partially labelled set (``allowed``) goes the same two ways with its masks and minimises the marginal likelihood
    log Z - log Z_A, which is not convex: the optimiser then skips correction pairs without positive curvature
    (``minimize``'s ``skip_nonpositive_curvature``; labelled fits keep their iterates bit for bit).  It starts at w = 0 like
    every fit.  There every label scores alike, so an item's restricted marginal is uniform over its set: a set in which no
    item names a single label has a zero gradient at 0 and the fit returns "converged" at w = 0.

    Cost-sensitive fits: a set with sequence weights (``seq_weight``) or ``params`` with ``label_costs`` minimises
    ``sum over instances of seq_weight * (log sum_y' exp(score(y') + sum_t C[y_t][y'_t]) - score(y))`` and takes
    ``TrainerGeneral`` (windowed, 2 labels included) or ``TrainerSequences``.  With every weight 1 and no non-zero cost
    such a 2-label windowed fit agrees with the 2-label trainer's to rounding; it is not bit-equal to it (the kernels
    differ).  Costs exist in training only: the model and every prediction are what they always were."""
    from . import _native

    args = ts.native_args()
    # (a set with values: the general kernels at any label count; one without: the calls they always were)
    valued = {} if ts.attr_value is None else {"values": [ts.attr_value]}
    if ts.allowed is not None:
        valued["allowed"] = [ts.allowed]
    valued.update(_weighting([ts], [params]))
    if ts.window is None:
        trainer = _native.TrainerSequences([args], device=device, **valued)
    elif ts.num_labels == 2 and not valued:
        trainer = _native.Trainer(*args[:5], *args[8:], *args[5:8], device=device)  # (window and step in the middle)
    else:
        trainer = _native.TrainerGeneral([args], device=device, **valued)
    return _fit_lockstep(trainer, [ts], [params], callback)[0]


def _valued_entries(ts: TrainingSet) -> int:
    """What a set with values adds to its scratch, in doubles: the values in attribute -> items order, one per entry."""
    return 0 if ts.attr_value is None else int(len(ts.attr_value))


def _weighted_entries(ts: TrainingSet, params: Optional[Dict[str, object]], instances: int) -> int:
    """What sequence weights or label costs add to a problem's scratch, in doubles: exactly what is uploaded for them, one
    weight per instance and, with costs, the matrix [L, L]."""
    costs = bool((params or {}).get("label_costs"))
    if ts.seq_weight is None and not costs:
        return 0
    return instances + (ts.num_labels ** 2 if costs else 0)


def _general_trainer(ts: TrainingSet, params: Optional[Dict[str, object]] = None) -> bool:
    """A windowed set that takes ``_native.TrainerGeneral`` at any label count: one with values, with allowed-label masks or
    with sequence weights, or any set when the fit's ``params`` carry label costs."""
    return (ts.attr_value is not None or ts.allowed is not None or ts.seq_weight is not None
            or bool((params or {}).get("label_costs")))


def _general_scratch_bytes(ts: TrainingSet, params: Optional[Dict[str, object]] = None) -> int:
    """The scratch ``_native.TrainerGeneral`` allocates for ``ts`` (``scratch_bytes(k)``; the formula of DESIGN.md §4.9b:
    item scores and marginals, node marginals, and one (f, xi) block per 128 windows plus 32 slabs), fitted with ``params``
    (whose label costs, like the set's sequence weights, add what ``_weighted_entries`` says)."""
    L, W = ts.num_labels, ts.window
    n = np.diff(np.asarray(ts.seq_ptr, dtype=np.int64))
    windows = int(np.sum((n[n >= W] - W) // ts.step + 1))
    second_pass = windows * W * L if ts.allowed is not None else 0  # (a partial set: the restricted pass's log alpha, §4.9e)
    return 8 * (2 * int(ts.seq_ptr[-1]) * L + windows * W * L + (-(-windows // 128) + 32) * (1 + L * L) + second_pass
                + _valued_entries(ts) + _weighted_entries(ts, params, windows))


def _sequences_scratch_bytes(ts: TrainingSet, params: Optional[Dict[str, object]] = None) -> int:
    """The scratch ``_native.TrainerSequences`` allocates for ``ts`` (``scratch_bytes(k)``; the formula of DESIGN.md
    §4.9c: item scores and marginals, and one (f, xi) block per 256 / G sequences, G the power of two at or above L,
    plus 32 slabs), fitted with ``params`` (as above)."""
    L = ts.num_labels
    per_block = 256 // max(2, 1 << (L - 1).bit_length())
    second_pass = int(ts.seq_ptr[-1]) * L if ts.allowed is not None else 0  # (a partial set: as above, §4.9e)
    return 8 * (2 * int(ts.seq_ptr[-1]) * L + (-(-(len(ts.seq_ptr) - 1) // per_block) + 32) * (1 + L * L) + second_pass
                + _valued_entries(ts) + _weighted_entries(ts, params, len(ts.seq_ptr) - 1))


def _by_label_count(sets: Sequence[TrainingSet], fit_two: Callable[[List[int]], List[OptimizeResult]],
                    params: Callable[[int], Dict[str, object]], device: int,
                    scratch_budget_bytes: Optional[int] = None) -> List[OptimizeResult]:
    """Results of fits whose sets may mix label counts: ``fit_two(indices)`` fits the windowed sets of two labels as
    before, the other windowed sets run in ``_native.TrainerGeneral`` and the sets of whole sequences (``window is
    None``, any label count) in ``_native.TrainerSequences``; fit k trains ``sets[k]`` with ``params(k)``.  Without a
    budget the fits of such a family share one trainer; with one they run, in their order, in groups whose scratch fits the
    budget (a group holds at least one fit), one trainer after another, so that only one group is resident at a time.  A
    fit's result does not depend on its group: problem k of a trainer has the bits of a lone trainer of it.  A windowed
    2-label fit with sequence weights or label costs goes with the sets of more labels (``_general_trainer``)."""
    from . import _native

    results: List[Optional[OptimizeResult]] = [None] * len(sets)
    # (a windowed set with values or with masks goes with the sets of more labels, at any label count)
    two = [k for k, ts in enumerate(sets) if ts.window is not None and ts.num_labels == 2 and not _general_trainer(ts, params(k))]
    more = [k for k, ts in enumerate(sets) if ts.window is not None and (ts.num_labels != 2 or _general_trainer(ts, params(k)))]
    whole = [k for k, ts in enumerate(sets) if ts.window is None]
    if two:
        for k, r in zip(two, fit_two(two)):
            results[k] = r
    budget = scratch_budget_bytes if scratch_budget_bytes and scratch_budget_bytes > 0 else None  # as TrainerGrid: 0 = none
    for members, scratch, family in ((more, _general_scratch_bytes, "TrainerGeneral"),
                                     (whole, _sequences_scratch_bytes, "TrainerSequences")):
        groups: List[List[int]] = []
        used = 0
        for k in members:
            need = scratch(sets[k], params(k)) if budget is not None else 0
            if not groups or (budget is not None and used + need > budget):
                groups.append([])
                used = 0
            groups[-1].append(k)
            used += need
        for group in groups:
            values = [sets[k].attr_value for k in group]
            valued = {} if all(v is None for v in values) else {"values": values}  # (no values: the call it always was)
            if any(sets[k].allowed is not None for k in group):  # (partial sets beside labelled ones: None for the latter)
                valued["allowed"] = [sets[k].allowed for k in group]
            valued.update(_weighting([sets[k] for k in group], [params(k) for k in group]))  # (none: no keyword)
            trainer = getattr(_native, family)([sets[k].native_args() for k in group], device=device, **valued)
            for k, r in zip(group, _fit_lockstep(trainer, [sets[k] for k in group], [params(k) for k in group])):
                results[k] = r
            del trainer  # frees the group's device memory before the next group is created
    return results


def fit_training_sets(sets: Sequence[TrainingSet], params: Dict[str, object], device: int = 0) -> List[OptimizeResult]:
    """``fit_training_set`` of every set at once: all sets are resident on the device together (``_native.TrainerBatch``)
    and one optimiser per set runs in lock-step, each round evaluating the pending points of the unfinished sets in one
    batched pass.  Sets drop out as they stop.  Result k is exactly ``fit_training_set(sets[k], params, device)``:
    the batched objective gives every set the bits a lone trainer gives it, and the optimiser loop is the same one.
    The sets must share ``window`` and ``step`` (sets of whole sequences, ``window is None``, share them).  Sets of more
    than two labels run in a ``_native.TrainerGeneral`` of their own, beside the batch of the 2-label sets; sets of whole
    sequences in a ``_native.TrainerSequences``."""
    from . import _native

    if not sets:
        return []
    window, step = sets[0].window, sets[0].step
    if any(ts.window != window or ts.step != step for ts in sets):
        raise ValueError("fit_training_sets: every training set must have the same window and step")

    def fit_two(idx):
        batch = _native.TrainerBatch([sets[k].native_args()[:-2] for k in idx], window, step, device=device)
        return _fit_lockstep(batch, [sets[k] for k in idx], [params] * len(idx))

    return _by_label_count(sets, fit_two, lambda k: params, device)


#: default cap of ``fit_grid``'s work space: the scratch of one group of problems evaluated together
GRID_SCRATCH_BUDGET = 8 << 30


def fit_grid(sets: Sequence[TrainingSet], problems: Sequence[Tuple[int, Dict[str, object]]], device: int = 0,
             scratch_budget_bytes: int = GRID_SCRATCH_BUDGET) -> List[OptimizeResult]:
    """A grid of fits over shared training sets: problem k is ``(set index, params)``.  Every set is resident on the device
    once, with its own window and step (``_native.TrainerGrid``); one optimiser per problem, with that problem's
    ``c1`` / ``c2`` and libLBFGS parameters, runs in lock-step, each round evaluating the pending points of the unfinished
    problems in one batched pass (in groups whose scratch fits ``scratch_budget_bytes``).  Result k is exactly
    ``fit_training_set(sets[set_k], params_k, device)``.  Problems on sets of more than two labels run in
    ``_native.TrainerGeneral`` (one copy of the set per problem), also in groups whose scratch fits the budget, one
    group resident at a time; so do problems on sets of whole sequences, in ``_native.TrainerSequences``.  ``label_costs``
    are a trainer parameter like ``c1`` / ``c2`` and may differ from problem to problem: a problem with costs, or on a set
    with sequence weights, runs in ``TrainerGeneral`` at 2 labels too, the others keep ``TrainerGrid`` and their bits."""
    from . import _native

    if not problems:
        return []
    for k, (s, _) in enumerate(problems):
        if not 0 <= int(s) < len(sets):
            raise ValueError(f"fit_grid: problem {k} names set {s}, but there are {len(sets)} sets")

    def fit_two(idx):
        used = [s for s, ts in enumerate(sets) if ts.window is not None and ts.num_labels == 2 and not _general_trainer(ts)]
        grid = _native.TrainerGrid([sets[s].native_args() for s in used], [used.index(int(problems[k][0])) for k in idx],
                                   scratch_budget_bytes, device=device)
        return _fit_lockstep(grid, [sets[int(problems[k][0])] for k in idx], [problems[k][1] for k in idx])

    return _by_label_count([sets[int(s)] for s, _ in problems], fit_two, lambda k: problems[k][1], device,
                           scratch_budget_bytes)


def _fit_lockstep(trainer, sets: Sequence[TrainingSet], params: Sequence[Dict[str, object]],
                  callback: Optional[Callable[[int, float, np.ndarray], None]] = None) -> List[OptimizeResult]:
    """The optimiser loop of every fit: one ``minimize_steps`` per problem of ``trainer`` (a ``_native`` trainer of any
    family; problem k trains ``sets[k]`` with ``params[k]``) in lock-step, each round evaluating the pending points of the
    unfinished problems in one pass; problems drop out as they stop.  The host adds each problem's L2 term.  ``callback``
    goes to every problem's optimiser (``fit_training_set`` has one problem)."""
    n = len(sets)
    steppers = [minimize_steps(np.zeros(ts.num_features), c1=float(p["c1"]), num_memories=int(p["num_memories"]),
                               epsilon=float(p["epsilon"]), period=int(p["period"]), delta=float(p["delta"]),
                               max_iterations=p["max_iterations"], callback=callback,
                               skip_nonpositive_curvature=ts.allowed is not None)  # (a partial set is not convex)
                for ts, p in zip(sets, params)]
    c2 = [float(p["c2"]) for p in params]
    pending: List[Optional[np.ndarray]] = [next(st) for st in steppers]
    results: List[Optional[OptimizeResult]] = [None] * n
    f = np.zeros(n)
    g = [np.empty(ts.num_features) for ts in sets]
    while any(x is not None for x in pending):
        trainer._eval_problems(pending, [x is not None for x in pending], f, g)
        for k, w in enumerate(pending):
            if w is None:
                continue
            fk, gk = float(f[k]), g[k]
            if c2[k] > 0:
                fk += c2[k] * float(np.dot(w, w))
                gk = gk + (2.0 * c2[k]) * w
            else:
                gk = gk.copy()  # (the stepper keeps it, and g[k] is written again next round)
            try:
                pending[k] = steppers[k].send((fk, gk))
            except StopIteration as stop:
                pending[k] = None
                results[k] = stop.value
    return results


def model_blob(ts: TrainingSet, w: np.ndarray) -> bytes:
    """The CRFsuite model file of trained weights (zero weights and unused attributes dropped, as CRFsuite saves)."""
    from .crfsuite_model import model_bytes

    return model_bytes(ts.labels_, ts.attrs_, ts.state_attr, ts.state_label, ts.trans_src, ts.trans_dst, w)


def main(argv: Optional[List[str]] = None) -> int:
    """``gecco train`` (``train_cli.main``)."""
    from . import train_cli

    return train_cli.main(argv)


if __name__ == "__main__":
    sys.exit(main())
