"""A linear-chain CRF over sequences of items with string attributes, plain or with a real value each (CRFsuite's
name:value items, given as dicts as ``sklearn_crfsuite`` takes them), and 2 to 32 string labels, trained and applied on
the device: the shape of ``sklearn_crfsuite.CRF`` over this package's training stack (``train``) and inference entry
points (``_native.Model``).  Training instances are the sliding windows of every sequence, as everywhere in GECCO, or
with ``window_size=None`` the whole sequences, as CRFsuite trains outside GECCO: the objective ``predict`` and
``predict_marginals`` decode with.
"""
import operator
from collections.abc import Mapping
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import train

__all__ = ["SequenceCRF"]


def _items(xseq) -> Tuple[List[List[str]], Optional[List[List[float]]]]:
    """The attributes of every item of a sequence as ``(names, values)``: ``values`` is None when every item is a plain
    iterable of names, whose duplicates are collapsed (the first occurrence is kept) -- the unvalued path.  An item that is
    a dict (python-crfsuite's conversion, ``train.item_attributes``) or a list of ``(name, value)`` pairs gives every item
    of the sequence values, 1.0 for the attributes of its plain items."""
    names, values = [], []
    for item in xseq:
        if isinstance(item, str):
            raise ValueError("an item is an iterable of attribute names, not a string")
        if not isinstance(item, Mapping):
            item = list(item)
            if not any(isinstance(e, tuple) for e in item):
                item = list(dict.fromkeys(str(name) for name in item))  # (plain names, as ever)
        nm, vals = train.item_attributes(item)
        names.append(nm)
        values.append(vals)
    if all(v is None for v in values):
        return names, None
    return names, [[1.0] * len(nm) if v is None else v for nm, v in zip(names, values)]


class SequenceCRF:
    """``SequenceCRF(window_size=5, window_step=1, device=0, **options)``: ``options`` are the trainer's
    (``train.trainer_params``: ``c1``, ``c2``, ``min_freq``, ``all_possible_states``, ``all_possible_transitions`` and the
    libLBFGS parameters, and ``label_costs``, a mapping ``{(gold, predicted): cost}`` that makes the fit cost-sensitive;
    costs exist in training only).  ``window_size=None``: the training instances are the whole sequences, of any length from one
    item up; ``window_step`` is then ignored and stored as 1, and the model has no windowed predictions.

    After ``fit(X, y)``: ``classes_`` (labels in order of first appearance), ``attributes_`` (the attributes the model
    keeps), ``state_features_`` ``{(attribute, label): weight}``, ``transition_features_`` ``{(from, to): weight}`` (the
    non-zero weights, unrounded) and ``training_result_`` (``train.OptimizeResult``)."""

    def __init__(self, window_size: Optional[int] = 5, window_step: int = 1, device: int = 0, **options):
        if window_size is None:
            window_step = 1
        else:
            window_size, window_step = int(window_size), int(window_step)
            if not 1 <= window_size <= 32:
                raise ValueError(f"window_size must lie in 1..32, got {window_size}")
            if not 1 <= window_step <= window_size:
                raise ValueError("Window step must be strictly positive and under `window_size`")
        self.window_size, self.window_step, self.device = window_size, window_step, int(device)
        self.params = train.trainer_params(options)
        self.training_result_: Optional[train.OptimizeResult] = None
        self._blob: Optional[bytes] = None
        self._model = None

    # ---- training
    def fit(self, X: Sequence[Iterable[Iterable[str]]], y: Sequence[Sequence[str]], sample_weight=None) -> "SequenceCRF":
        """``X``: sequences of items; an item is an iterable of attribute names, or a dict / a list of ``(name, value)``
        pairs (``train.item_attributes``), as in every prediction method.  An entry of ``y`` is a label, a ``set`` /
        ``frozenset`` / ``list`` / ``tuple`` of labels (the labels allowed on that item) or None (every label): with any
        entry that is not one label the fit maximises the marginal likelihood of the allowed paths
        (``train.build_training_set``), and ``label_costs`` are then a ``ValueError``.  ``sample_weight``: None, or one finite
        weight >= 0 per sequence, which every training instance cut from that sequence carries in the objective."""
        seqs = []
        for xseq in X:  # (a sequence with values goes to the training set as (name, value) pairs, one without as names)
            names, values = _items(xseq)
            seqs.append(names if values is None else [list(zip(nm, v)) for nm, v in zip(names, values)])
        labs = [[None if lab is None else frozenset(str(m) for m in lab) if isinstance(lab, (set, frozenset, list, tuple))
                 else str(lab) for lab in yseq] for yseq in y]
        if len(seqs) != len(labs):
            raise ValueError(f"X holds {len(seqs)} sequences and y {len(labs)}")
        for k, (items, ls) in enumerate(zip(seqs, labs)):
            if len(items) != len(ls):
                raise ValueError(f"sequence {k}: {len(items)} items but {len(ls)} labels")
            if self.window_size is not None and len(items) < self.window_size:
                raise ValueError(f"sequence {k} has {len(items)} items, fewer than the window of {self.window_size}")
        p = self.params
        step = None if self.window_size is None else self.window_step
        ts = train.build_training_set(seqs, labs, self.window_size, step, min_freq=p["min_freq"],
                                      all_possible_states=p["all_possible_states"],
                                      all_possible_transitions=p["all_possible_transitions"], max_labels=train.MAX_LABELS,
                                      sample_weight=sample_weight)
        self.training_result_ = train.fit_training_set(ts, p, device=self.device)
        self._set_blob(train.model_blob(ts, self.training_result_.x))
        return self

    # ---- the model file
    def _set_blob(self, blob: bytes) -> None:
        from . import _native

        self._blob = bytes(blob)
        self._model = m = _native.Model.from_lcrf(self._blob)
        self.classes_: List[str] = m.labels()
        self.attributes_: List[str] = m.attrs()
        self._attr_index = {a: i for i, a in enumerate(self.attributes_)}
        sw, sp = m.state_weights()
        tw, tp = m.trans_weights()
        self.state_features_: Dict[Tuple[str, str], float] = {
            (self.attributes_[a], self.classes_[l]): float(sw[a, l]) for a, l in zip(*(i.tolist() for i in np.nonzero(sp)))}
        self.transition_features_: Dict[Tuple[str, str], float] = {
            (self.classes_[i], self.classes_[j]): float(tw[i, j]) for i, j in zip(*(i.tolist() for i in np.nonzero(tp)))}

    def _fitted(self):
        if self._model is None:
            raise ValueError("this SequenceCRF is not fitted: call fit, from_bytes or load first")
        return self._model

    def to_bytes(self) -> bytes:
        """The CRFsuite model file."""
        self._fitted()
        return self._blob

    def save(self, path) -> None:
        with open(path, "wb") as fh:
            fh.write(self.to_bytes())

    @classmethod
    def from_bytes(cls, blob: bytes, window_size: Optional[int] = 5, window_step: int = 1, device: int = 0, **options) -> "SequenceCRF":
        crf = cls(window_size, window_step, device, **options)
        crf._set_blob(blob)
        return crf

    @classmethod
    def load(cls, path, window_size: Optional[int] = 5, window_step: int = 1, device: int = 0, **options) -> "SequenceCRF":
        with open(path, "rb") as fh:
            return cls.from_bytes(fh.read(), window_size, window_step, device, **options)

    # ---- prediction
    def _pack(self, X) -> Tuple[np.ndarray, np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """X as CSR over the model's attribute ids, and the value of every entry or None when every item of X is plain
        names (the unvalued entries are then called); names the model does not know are dropped, with their values."""
        self._fitted()
        seq_ptr, item_ptr, attr, vals = [0], [0], [], []
        packed = [_items(xseq) for xseq in X]
        valued = any(values is not None for _, values in packed)
        for names_seq, values_seq in packed:
            for k, names in enumerate(names_seq):
                known = [j for j, nm in enumerate(names) if nm in self._attr_index]
                attr.extend(self._attr_index[names[j]] for j in known)
                if valued:
                    vals.extend(1.0 if values_seq is None else values_seq[k][j] for j in known)
                item_ptr.append(len(attr))
            seq_ptr.append(len(item_ptr) - 1)
        return (np.array(seq_ptr, dtype=np.int32), np.array(item_ptr, dtype=np.int32), np.array(attr, dtype=np.int32),
                np.array(vals, dtype=np.float64) if valued else None)

    @staticmethod
    def _split(values: np.ndarray, seq_ptr: np.ndarray) -> list:
        return [values[a:b] for a, b in zip(seq_ptr[:-1].tolist(), seq_ptr[1:].tolist())]

    # ``allowed=`` of the prediction methods, and ``y`` of ``log_likelihood``: per sequence a list as long as the sequence whose
    # entries follow ``fit``'s grammar for ``y`` -- a label, a ``set`` / ``frozenset`` / ``list`` / ``tuple`` of labels, or None
    # for every label of the model.  The prediction is then made on the lattice without the other (item, label) pairs: the
    # best path inside the sets, the marginals given that the path lies inside them (exactly 0.0 outside).
    def _label_sets(self, sets, seq_ptr: np.ndarray, what: str) -> Tuple[np.ndarray, bool]:
        """One uint32 mask per item (bit k: ``classes_[k]`` is allowed), and whether every entry names exactly one label."""
        index = {c: k for k, c in enumerate(self.classes_)}
        every = (1 << len(self.classes_)) - 1
        n_seqs = len(seq_ptr) - 1
        sets = list(sets)
        if len(sets) != n_seqs:
            raise ValueError(f"X holds {n_seqs} sequences and {what} {len(sets)}")
        masks, single = [], True
        for k, entries in enumerate(sets):
            entries = list(entries)
            if len(entries) != seq_ptr[k + 1] - seq_ptr[k]:
                raise ValueError(f"sequence {k}: {seq_ptr[k + 1] - seq_ptr[k]} items but {len(entries)} labels")
            for t, entry in enumerate(entries):
                if entry is None:
                    masks.append(every)
                    single = False
                    continue
                names = [str(m) for m in entry] if isinstance(entry, (set, frozenset, list, tuple)) else [str(entry)]
                if not names:
                    raise ValueError(f"sequence {k}, item {t}: an empty set allows no label")
                bits = 0
                for name in names:
                    if name not in index:
                        raise ValueError(f"unknown label {name!r} (classes_: {self.classes_})")
                    bits |= 1 << index[name]
                masks.append(bits)
                single = single and bits & (bits - 1) == 0
        return np.array(masks, dtype=np.uint32), single

    def _allowed(self, allowed, seq_ptr: np.ndarray) -> Optional[np.ndarray]:
        return None if allowed is None else self._label_sets(allowed, seq_ptr, "allowed")[0]

    # ``circular=`` of ``predict``, ``predict_marginals`` and ``log_likelihood``: None (every sequence is a chain with two free
    # ends: the calls and the bytes there have always been), True (every sequence is a RING, whose last item has a transition
    # into its first: a complete chromosome or plasmid) or one boolean per sequence.  The circular sequences go to the ring entry
    # in one call, the others to the chain entry in one call, and the results come back in the caller's order.
    @staticmethod
    def _ring_flags(circular, n_seqs: int) -> np.ndarray:
        if isinstance(circular, (bool, np.bool_)):
            return np.full(n_seqs, bool(circular))
        flags = [bool(c) for c in circular]
        if len(flags) != n_seqs:
            raise ValueError(f"X holds {n_seqs} sequences and circular {len(flags)} flags")
        return np.array(flags, dtype=bool)

    def _by_topology(self, X, circular, per_sequence, chain, ring) -> list:
        """``chain(X', extras')`` of the linear sequences and ``ring(X', extras')`` of the circular ones, each a list with one
        result per sequence, merged in the caller's order; ``per_sequence`` holds the arguments that go sequence by sequence
        (``allowed``, ``y``; None stays None)."""
        X = list(X)
        flags = self._ring_flags(circular, len(X))
        per_sequence = [None if arg is None else list(arg) for arg in per_sequence]
        for arg, what in zip(per_sequence, ("allowed", "y")):
            if arg is not None and len(arg) != len(X):
                raise ValueError(f"X holds {len(X)} sequences and {what} {len(arg)}")
        out: list = [None] * len(X)
        for keep, call in ((np.flatnonzero(~flags), chain), (np.flatnonzero(flags), ring)):
            if len(keep):
                part = call([X[k] for k in keep], *[None if arg is None else [arg[k] for k in keep] for arg in per_sequence])
                for k, result in zip(keep.tolist(), part):
                    out[k] = result
        return out

    def _ring(self, X, allowed, want_path: bool, want_marginals: bool):
        """The ring entry's outputs for X, every sequence a ring, and the packed batch: ``(out, seq_ptr, item_ptr, attr, values)``.
        A batch without items never reaches the device."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        n_seqs, L = len(seq_ptr) - 1, len(self.classes_)
        if seq_ptr[-1] == 0:
            out = {"lognorm": np.zeros(n_seqs)}
            if want_path:
                out.update(labels=np.zeros(0, dtype=np.int8), score=np.zeros(n_seqs))
            if want_marginals:
                out["marginals"] = np.zeros((0, L))
        else:
            out = self._model.ring(seq_ptr, item_ptr, attr, device=self.device, values=values, allowed=masks, want_path=want_path,
                                   want_marginals=want_marginals)
        return out, seq_ptr, item_ptr, attr, values

    def _ring_labels(self, X, allowed) -> List[List[str]]:
        out, seq_ptr = self._ring(X, allowed, True, False)[:2]
        return [[self.classes_[k] for k in ys.tolist()] for ys in self._split(out["labels"], seq_ptr)]

    def _ring_marginals(self, X, allowed) -> List[np.ndarray]:
        out, seq_ptr = self._ring(X, allowed, False, True)[:2]
        return self._split(out["marginals"], seq_ptr)

    def predict(self, X, allowed=None, circular=None) -> List[List[str]]:
        """Viterbi labels of every sequence; with ``allowed``, the best path inside the allowed sets.  ``circular``: the
        sequences that are rings get the ring's best path, closing edge included (ties: the smaller first label, then the
        chain's rule)."""
        if circular is not None:
            return self._by_topology(X, circular, [allowed], self.predict, self._ring_labels)
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        if seq_ptr[-1] == 0:
            return [[] for _ in X]
        y, _ = self._model.viterbi(seq_ptr, item_ptr, attr, device=self.device, values=values, allowed=masks)
        return [[self.classes_[k] for k in ys.tolist()] for ys in self._split(y, seq_ptr)]

    def predict_marginals(self, X, allowed=None, circular=None) -> List[np.ndarray]:
        """Whole-sequence marginals: one ``[n_items, L]`` array per sequence, columns in ``classes_`` order; with
        ``allowed``, given that the path lies inside the allowed sets (exactly 0.0 outside them).  ``circular``: the
        sequences that are rings get the ring's marginals, which do not depend on where the ring was cut."""
        if circular is not None:
            return self._by_topology(X, circular, [allowed], self.predict_marginals, self._ring_marginals)
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        if seq_ptr[-1] == 0:
            return [np.zeros((0, len(self.classes_))) for _ in X]
        marg, _ = self._model.marginals_full(seq_ptr, item_ptr, attr, device=self.device, values=values, allowed=masks)
        return self._split(marg, seq_ptr)

    def predict_ring(self, X, allowed=None) -> List[Dict[str, object]]:
        """Every sequence as a ring, in one device call: per sequence ``labels`` (the ring's best path), ``score`` (its score:
        the state scores, the transitions and the closing edge from the last item into the first), ``log_probability`` (=
        ``score - lognorm``), ``lognorm`` (log Z of the ring) and ``marginals`` ``[n_items, L]``.  Rotating a ring rotates
        ``labels`` and ``marginals`` and keeps the rest.  A sequence without items has no labels, score 0 and log Z 0."""
        out, seq_ptr = self._ring(X, allowed, True, True)[:2]
        labels, marginals = self._split(out["labels"], seq_ptr), self._split(out["marginals"], seq_ptr)
        return [{"labels": [self.classes_[k] for k in labels[s].tolist()], "score": float(out["score"][s]),
                 "log_probability": float(out["score"][s] - out["lognorm"][s]), "lognorm": float(out["lognorm"][s]),
                 "marginals": marginals[s]} for s in range(len(seq_ptr) - 1)]

    def _ring_log_likelihood(self, X, y) -> List[float]:
        """``log_likelihood`` of rings: the path's ring score minus log Z of the ring, or with sets log Z_A,ring - log Z_ring."""
        y = [list(yseq) for yseq in y]
        out, seq_ptr, item_ptr, attr, values = self._ring(X, None, False, False)
        masks, single = self._label_sets(y, seq_ptr, "y")
        if len(masks) == 0:
            return [0.0] * (len(seq_ptr) - 1)
        if not single:
            inside = self._model.ring(seq_ptr, item_ptr, attr, device=self.device, values=values, allowed=masks, want_path=False,
                                      want_marginals=False)["lognorm"]
            return (inside - out["lognorm"]).tolist()
        yy = np.log2(masks.astype(np.float64)).astype(np.int64)  # (one bit per mask)
        state, _ = self._model.state_weights()
        trans, _ = self._model.trans_weights()
        owner = np.repeat(np.arange(len(yy)), np.diff(item_ptr))
        score = np.zeros(len(yy))  # per item: its state score under its label, and the transition into it -- the closing edge at the first
        np.add.at(score, owner, state[attr, yy[owner]] if values is None else values * state[attr, yy[owner]])
        lengths = np.diff(seq_ptr)
        full = np.flatnonzero(lengths > 0)
        first = np.repeat(seq_ptr[:-1][full], lengths[full])
        before = first + (np.arange(len(yy)) - first - 1) % np.repeat(lengths[full], lengths[full])
        score += trans[yy[before], yy]
        result = np.zeros(len(seq_ptr) - 1)
        result[full] = np.add.reduceat(score, seq_ptr[:-1][full]) - out["lognorm"][full]
        return result.tolist()

    def log_likelihood(self, X, y: Sequence[Sequence[str]], circular=None) -> np.ndarray:
        """``log p(y | x)`` of every sequence under the model (CRFsuite's ``Tagger.probability`` in logs): the gold path's
        score, gathered on the host from the weight tables (value x weight for items with values), minus the log partition function of the whole-sequence
        marginals.  An unknown label raises ``ValueError``; an empty sequence gives 0.0.

        An entry of ``y`` may also be a set of labels or None, as in ``fit``: the result is then ``log Z_A - log Z``, the
        log-probability that the path lies inside the sets -- the negative of the sequence's term in the partial trainer's
        objective -- from two whole-sequence forward-backward passes, one on the restricted lattice and one on the full one.
        (Both take the masked state-score kernel, the second with every label allowed, which has the unmasked kernels' bits:
        with every entry None the result is exactly 0.0 at every label count.)

        ``circular``: for the sequences that are rings the path's score has the closing edge from the last item into the first
        (added on the host) and the partition function is the ring's; with sets the result is ``log Z_A,ring - log Z_ring``."""
        if circular is not None:
            return np.array(self._by_topology(X, circular, [None, y], lambda Xs, _, ys: self.log_likelihood(Xs, ys).tolist(),
                                              lambda Xs, _, ys: self._ring_log_likelihood(Xs, ys)), dtype=np.float64)
        seq_ptr, item_ptr, attr, values = self._pack(X)
        y = [list(yseq) for yseq in y]
        if any(lab is None or isinstance(lab, (set, frozenset, list, tuple)) for yseq in y for lab in yseq):
            masks, single = self._label_sets(y, seq_ptr, "y")
            if not single:
                return self._log_probability_inside(seq_ptr, item_ptr, attr, values, masks)
            y = [[next(iter(lab)) if isinstance(lab, (set, frozenset, list, tuple)) else lab for lab in yseq] for yseq in y]
        index = {c: k for k, c in enumerate(self.classes_)}
        labs = [[str(lab) for lab in yseq] for yseq in y]
        n_seqs = len(seq_ptr) - 1
        if len(labs) != n_seqs:
            raise ValueError(f"X holds {n_seqs} sequences and y {len(labs)}")
        for k, ls in enumerate(labs):
            if len(ls) != seq_ptr[k + 1] - seq_ptr[k]:
                raise ValueError(f"sequence {k}: {seq_ptr[k + 1] - seq_ptr[k]} items but {len(ls)} labels")
            for lab in ls:
                if lab not in index:
                    raise ValueError(f"unknown label {lab!r} (classes_: {self.classes_})")
        out = np.zeros(n_seqs)
        if seq_ptr[-1] == 0:
            return out
        lengths = np.diff(seq_ptr)
        full = np.flatnonzero(lengths > 0)  # (an empty sequence stays at 0.0 and never reaches the device)
        ptr = np.concatenate([[0], np.cumsum(lengths[full])]).astype(np.int32)
        _, lognorm = self._model.marginals_full(ptr, item_ptr, attr, device=self.device, values=values)
        state, _ = self._model.state_weights()
        trans, _ = self._model.trans_weights()
        yy = np.array([index[lab] for ls in labs for lab in ls], dtype=np.int64)
        owner = np.repeat(np.arange(len(yy)), np.diff(item_ptr))
        score = np.zeros(len(yy))  # per item: its state score under its label, and the transition into it
        np.add.at(score, owner, state[attr, yy[owner]] if values is None else values * state[attr, yy[owner]])
        inner = np.ones(len(yy), dtype=bool)
        inner[ptr[:-1]] = False  # (the first item of a sequence has no predecessor)
        score[inner] += trans[yy[np.flatnonzero(inner) - 1], yy[inner]]
        out[full] = np.add.reduceat(score, ptr[:-1]) - lognorm
        return out

    def _log_probability_inside(self, seq_ptr, item_ptr, attr, values, masks: np.ndarray) -> np.ndarray:
        out = np.zeros(len(seq_ptr) - 1)
        if seq_ptr[-1] == 0:
            return out
        lengths = np.diff(seq_ptr)
        full = np.flatnonzero(lengths > 0)  # (an empty sequence stays at 0.0 and never reaches the device)
        ptr = np.concatenate([[0], np.cumsum(lengths[full])]).astype(np.int32)
        every = np.full(len(masks), (1 << len(self.classes_)) - 1, dtype=np.uint32)
        _, inside = self._model.marginals_full(ptr, item_ptr, attr, device=self.device, values=values, allowed=masks)
        _, free = self._model.marginals_full(ptr, item_ptr, attr, device=self.device, values=values, allowed=every)
        out[full] = inside - free
        return out

    @staticmethod
    def _sequence_length(who: str, k: int, seq_ptr: np.ndarray) -> int:
        """The number of items of sequence ``k``, the sequence of the query ``who`` ("span 3"), once ``k`` is one of ``X``'s."""
        n_seqs = len(seq_ptr) - 1
        if not 0 <= k < n_seqs:
            raise ValueError(f"{who}: sequence index {k} out of range (X holds {n_seqs} sequences)")
        return int(seq_ptr[k + 1] - seq_ptr[k])

    def _label_bits(self, who: str, labels) -> int:
        """The mask of a query's label set: a label, or a ``set`` / ``frozenset`` / ``list`` / ``tuple`` of labels."""
        names = [str(m) for m in labels] if isinstance(labels, (set, frozenset, list, tuple)) else [str(labels)]
        if not names:
            raise ValueError(f"{who}: an empty set holds no label")
        bits = 0
        for name in names:
            if name not in self.classes_:
                raise ValueError(f"{who}: unknown label {name!r} (classes_: {self.classes_})")
            bits |= 1 << self.classes_.index(name)
        return bits

    def _span_queries(self, spans, seq_ptr: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """``spans`` as the native call's four arrays; every refusal is raised here, before any device call."""
        contig, begin, end, mask = [], [], [], []
        for q, span in enumerate(spans):
            try:
                k, start, stop, labels = span
                k, start, stop = operator.index(k), operator.index(start), operator.index(stop)
            except (TypeError, ValueError):
                raise ValueError(f"span {q}: expected (sequence_index, start, stop, labels), got {span!r}") from None
            length = self._sequence_length(f"span {q}", k, seq_ptr)
            if start < 0 or start >= stop:
                raise ValueError(f"span {q}: [{start}, {stop}) is not a non-empty range of items (start >= stop, or start < 0)")
            if stop > length:
                raise ValueError(f"span {q}: stop {stop} lies beyond sequence {k} of {length} items")
            contig.append(k)
            begin.append(start)
            end.append(stop)
            mask.append(self._label_bits(f"span {q}", labels))
        return (np.array(contig, dtype=np.int32), np.array(begin, dtype=np.int32), np.array(end, dtype=np.int32),
                np.array(mask, dtype=np.uint32))

    def span_log_probability(self, X, spans, allowed=None) -> np.ndarray:
        """Region posteriors: for every ``(sequence_index, start, stop, labels)`` of ``spans`` the log-probability, given the
        whole sequence, that EVERY item of ``X[sequence_index][start:stop]`` carries a label of ``labels`` -- a label, or a
        ``set`` / ``frozenset`` / ``list`` / ``tuple`` of labels.  One float64 per span, ``<= 0``; ``-inf`` where the
        probability is zero.  This is a property of the path distribution on the whole-sequence lattice (that of ``predict``
        and ``predict_marginals``, not a windowed one), not a function of the per-item marginals; with ``allowed`` (as in
        ``predict_marginals``) the lattice is the restricted one.  All spans take one forward-backward pass over ``X`` and one
        native call.  Raises ``ValueError`` before any device call for an unknown label, an empty set, a sequence index out
        of range, ``start >= stop`` or ``start < 0``, and ``stop`` beyond the sequence."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        contig, begin, end, mask = self._span_queries(spans, seq_ptr)
        if len(contig) == 0:
            return np.zeros(0)
        return self._model.span_log_probabilities(seq_ptr, item_ptr, attr, contig, begin, end, mask, device=self.device,
                                                  values=values, allowed=masks)

    def _span_conditionals(self, X, spans, reach, allowed, want_contributions: bool):
        """The native call behind ``predict_marginals_given_span`` and ``span_attributions``: ``(result or None, attr, values)``."""
        try:
            reach = operator.index(reach)
        except TypeError:
            raise ValueError(f"reach = {reach!r} is not an integer") from None
        if reach < 0:
            raise ValueError(f"reach = {reach} is negative")
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        contig, begin, end, mask = self._span_queries(spans, seq_ptr)
        if len(contig) == 0:
            return None, attr, values
        res = self._model.span_conditionals(seq_ptr, item_ptr, attr, contig, begin, end, mask, reach=reach, device=self.device,
                                            values=values, allowed=masks, want_contributions=want_contributions)
        # (the attribute occurrences of row r, as the packer kept them: item_ptr of the row's item)
        res["item_index"] = np.repeat(seq_ptr[contig].astype(np.int64) + res["first"] - res["row_ptr"][:-1],
                                      np.diff(res["row_ptr"])) + np.arange(int(res["row_ptr"][-1]))
        res["item_ptr"] = item_ptr
        return res, attr, values

    def predict_marginals_given_span(self, X, spans, reach=0, allowed=None) -> List[dict]:
        """Marginals given a region: for every ``(sequence_index, start, stop, labels)`` of ``spans`` (as in
        ``span_log_probability``) a dict with ``first`` (the index of the first row's item in its sequence: ``max(start - reach,
        0)``), ``log_probability`` (``span_log_probability``'s value) and ``marginals [rows, L]``: P(item t has label l | every
        item of the span carries a label of ``labels``, the whole sequence), for the items ``first .. min(stop + reach, T) - 1``,
        columns in ``classes_`` order.  Inside the span a label outside the set has exactly 0.0; a row sums to 1; where the span
        is impossible (``-inf``) the rows are 0.0.  One forward-backward pass over ``X`` and one native call for all spans.
        Raises ``ValueError`` before any device call for what ``span_log_probability`` refuses, and for a negative ``reach``."""
        res, _, _ = self._span_conditionals(X, spans, reach, allowed, False)
        if res is None:
            return []
        rows = res["row_ptr"]
        return [dict(first=int(res["first"][q]), log_probability=float(res["logp"][q]), marginals=res["cond"][rows[q]:rows[q + 1]])
                for q in range(len(res["logp"]))]

    def span_attributions(self, X, spans, reach=0, allowed=None) -> List[dict]:
        """Exact knock-out attributions of a region: for every span (as in ``predict_marginals_given_span``, whose rows these
        are) a dict with ``first``, ``log_probability``, ``items [rows]`` and ``attributes``.  ``items[r]`` is log P(region | x)
        minus log P(region | x with everything row r's item carries removed); ``attributes[r]`` lists, for every attribute
        occurrence the packer kept of that item and in its order, ``(name, value, contribution)``: the same difference with that
        one occurrence removed (value 1.0 for an attribute without one).  Positive where the region's probability leans on
        it.  Exact: the values ``span_log_probability`` would give on the changed input, from one pass and one native call.
        Where the span is impossible everything is 0.0.  Refusals as in ``predict_marginals_given_span``."""
        res, attr, values = self._span_conditionals(X, spans, reach, allowed, True)
        if res is None:
            return []
        rows, occ, item_ptr = res["row_ptr"], res["occ_ptr"], res["item_ptr"]
        contribution = res["attr"].tolist()
        out = []
        for q in range(len(res["logp"])):
            attributes = []
            for r in range(int(rows[q]), int(rows[q + 1])):
                k0 = int(item_ptr[res["item_index"][r]])
                attributes.append([(self.attributes_[int(attr[k0 + i])], 1.0 if values is None else float(values[k0 + i]),
                                    contribution[int(occ[r]) + i]) for i in range(int(occ[r + 1] - occ[r]))])
            out.append(dict(first=int(res["first"][q]), log_probability=float(res["logp"][q]), items=res["item"][rows[q]:rows[q + 1]],
                            attributes=attributes))
        return out

    def span_probability(self, X, spans, allowed=None) -> np.ndarray:
        """``exp`` of ``span_log_probability``."""
        return np.exp(self.span_log_probability(X, spans, allowed=allowed))

    def _anchor_queries(self, anchors, seq_ptr: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``anchors`` as the native call's three arrays; every refusal is raised here, before any device call."""
        contig, anchor, mask = [], [], []
        for q, entry in enumerate(anchors):
            try:
                k, item, labels = entry
                k, item = operator.index(k), operator.index(item)
            except (TypeError, ValueError):
                raise ValueError(f"anchor {q}: expected (sequence_index, item, labels), got {entry!r}") from None
            length = self._sequence_length(f"anchor {q}", k, seq_ptr)
            if not 0 <= item < length:
                raise ValueError(f"anchor {q}: item {item} lies outside sequence {k} of {length} items")
            contig.append(k)
            anchor.append(item)
            mask.append(self._label_bits(f"anchor {q}", labels))
        return np.array(contig, dtype=np.int32), np.array(anchor, dtype=np.int32), np.array(mask, dtype=np.uint32)

    @staticmethod
    def _sample_count(n_samples, seed) -> Tuple[int, int]:
        try:
            n_samples, seed = operator.index(n_samples), operator.index(seed)
        except TypeError:
            raise ValueError(f"n_samples and seed are integers, got {n_samples!r} and {seed!r}") from None
        if not 1 <= n_samples <= 1 << 20:
            raise ValueError(f"n_samples = {n_samples} is outside 1 .. 1048576")
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed {seed} is outside 0 .. 2**64 - 1")
        return n_samples, seed

    def sample(self, X, n_samples, seed=0, allowed=None) -> List[np.ndarray]:
        """Label paths drawn from the posterior ``p(y | x)`` on the whole-sequence lattice (that of ``predict`` and
        ``predict_marginals``, not a windowed one): per sequence one int8 ``[n_samples, n_items]`` array of indices into
        ``classes_``, row s the s-th path (a transposed view of the native call's item-major block; ``[n_samples, 0]`` for a
        sequence without items).  All samples take one forward-backward pass over ``X`` and one native call.  The draws are a
        function of ``seed`` and the position alone (Philox counters: item, sample, sequence): the same call gives the same
        paths, and path s does not depend on ``n_samples``.  With ``allowed`` (as in ``predict_marginals``) the paths are drawn
        on the restricted lattice and never leave the sets."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        n_samples, seed = self._sample_count(n_samples, seed)
        if seq_ptr[-1] == 0:
            return [np.zeros((n_samples, 0), dtype=np.int8) for _ in range(len(seq_ptr) - 1)]
        y = self._model.sample_paths(seq_ptr, item_ptr, attr, n_samples, seed=seed, device=self.device, values=values,
                                     allowed=masks)
        return [rows.T for rows in self._split(y, seq_ptr)]

    def sample_runs(self, X, anchors, n_samples, seed=0, allowed=None) -> np.ndarray:
        """For every ``(sequence_index, item, labels)`` of ``anchors`` and every one of the ``n_samples`` paths ``sample`` draws
        with the same ``seed`` and ``allowed``: the maximal run of items around ``X[sequence_index][item]`` whose labels all lie
        in ``labels`` (a label, or a ``set`` / ``frozenset`` / ``list`` / ``tuple`` of labels), as ``(first, last + 1)`` item
        indices inside the sequence, or ``(-1, -1)`` where the path's label at the anchor is outside ``labels``.  int32
        ``[n_anchors, n_samples, 2]``; the paths stay on the device.  Raises ``ValueError`` before any device call for an
        unknown label, an empty set, a sequence index out of range and an item outside its sequence."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        n_samples, seed = self._sample_count(n_samples, seed)
        contig, anchor, mask = self._anchor_queries(anchors, seq_ptr)
        if len(contig) == 0:
            return np.zeros((0, n_samples, 2), dtype=np.int32)
        return self._model.sample_paths(seq_ptr, item_ptr, attr, n_samples, seed=seed, device=self.device, values=values,
                                        allowed=masks, runs=(contig, anchor, mask), want_paths=False)

    @staticmethod
    def _reach(reach) -> int:
        try:
            reach = operator.index(reach)
        except TypeError:
            raise ValueError(f"reach is an integer, got {reach!r}") from None
        if not 0 <= reach <= 65536:
            raise ValueError(f"reach = {reach} is outside 0 .. 65536")
        return reach

    def run_posteriors(self, X, anchors, reach=64, allowed=None) -> List[Dict[str, object]]:
        """Exact start and end distributions of runs.  For every ``(sequence_index, item, labels)`` of ``anchors`` (what
        ``sample_runs`` takes), "the run through the anchor" is the maximal stretch of items around ``X[sequence_index][item]``
        whose labels all lie in ``labels``.  Per anchor one dict of natural logs (``<= 0``, ``-inf`` for probability zero):
        ``log_anchor``, log P(the anchor's label is in the set); ``log_start``, float64 ``[reach + 1]``, entry r the
        log-probability that the run starts at ``item - r`` (``-inf`` for ``r > item``); ``log_start_beyond``, that it starts
        before ``item - reach``; ``log_end`` (entry r: the run's last item is ``item + r``) and ``log_end_beyond`` likewise.
        The starts and the beyond-mass sum to the anchor's probability, as do the ends.  These are the exact values of what
        ``sample_runs`` estimates by counting; they are not ``boundary_probability``, which counts the start of ANY run at an
        item.  The start and the end are not independent: the joint is ``run_log_probability``.  Whole-sequence lattice (that
        of ``predict`` and ``predict_marginals``); with ``allowed`` the restricted one.  One forward-backward pass and one
        native call.  Raises ``ValueError`` before any device call for what ``sample_runs`` refuses, for ``reach`` outside
        0 .. 65536 and for ``n_anchors * (reach + 1) >= 2**31``."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        reach = self._reach(reach)
        contig, anchor, mask = self._anchor_queries(anchors, seq_ptr)
        if len(contig) * (reach + 1) >= 1 << 31:
            raise ValueError(f"{len(contig)} anchors at reach {reach}: n_anchors * (reach + 1) does not stay below 2**31")
        if len(contig) == 0:
            return []
        out = self._model.run_posteriors(seq_ptr, item_ptr, attr, anchors=(contig, anchor, mask), reach=reach, device=self.device,
                                         values=values, allowed=masks)
        keys = ("log_anchor", "log_start", "log_start_beyond", "log_end", "log_end_beyond")
        return [{k: (out[k][q] if out[k].ndim == 2 else float(out[k][q])) for k in keys} for q in range(len(contig))]

    def run_log_probability(self, X, runs, allowed=None) -> np.ndarray:
        """For every ``(sequence_index, start, stop, labels)`` of ``runs`` (as in ``span_log_probability``) the log-probability
        that a run is EXACTLY ``X[sequence_index][start:stop]``: every item of the range carries a label of ``labels``, the item
        before it (if any) does not, and the item after it (if any) does not.  It is one entry of the joint distribution of a
        run's start and end, which is not the product of ``run_posteriors``' two marginals.  One float64 per run, ``<= 0``,
        ``-inf`` where the probability is zero.  Raises ``ValueError`` before any device call for what ``span_log_probability``
        refuses."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        contig, begin, end, mask = self._span_queries(runs, seq_ptr)
        if len(contig) == 0:
            return np.zeros(0)
        return self._model.run_posteriors(seq_ptr, item_ptr, attr, runs=(contig, begin, end, mask), device=self.device,
                                          values=values, allowed=masks)["log_run"]

    def run_probability(self, X, runs, allowed=None) -> np.ndarray:
        """``exp`` of ``run_log_probability``."""
        return np.exp(self.run_log_probability(X, runs, allowed=allowed))

    @staticmethod
    def _kbest_count(k) -> int:
        try:
            k = operator.index(k)
        except TypeError:
            raise ValueError(f"k is an integer, got {k!r}") from None
        if not 1 <= k <= 32:
            raise ValueError(f"k = {k} is outside 1 .. 32")
        return k

    def predict_kbest(self, X, k, allowed=None) -> List[Dict[str, object]]:
        """The ``k`` best label paths of every sequence with their exact probabilities, on the whole-sequence lattice (that of
        ``predict`` and ``predict_marginals``, not a windowed one).  Per sequence a dict with ``paths``: a list of label lists,
        best first, holding only the paths that exist (at most ``k``, and at most the number of label paths of the sequence:
        ``L ** n_items`` without ``allowed``); ``scores``: their scores, float64, non-increasing; ``log_probabilities``:
        ``score - log Z``, the exact ``log p(y | x)`` of each path -- not a share of draws, so an alternative of probability 1e-3
        is reported as such.  ``paths[0]`` is ``predict``'s path.  Among paths of equal score the order is that of the reversed
        path (last item's label first) in ``classes_`` order, and the first ``k'`` entries of a call with ``k`` are the call
        with ``k'``.  One forward-backward pass (for ``log Z``) and one list-Viterbi walk over ``X``, one native call.  With
        ``allowed`` (as in ``predict``) the paths are the best inside the sets and the probabilities are given that the path
        lies inside them.  A sequence without items has no path: three empty entries.  Raises ``ValueError`` before any device
        call for a ``k`` that is not an integer or lies outside 1 .. 32."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        k = self._kbest_count(k)
        n_seqs = len(seq_ptr) - 1
        if seq_ptr[-1] == 0:
            return [{"paths": [], "scores": np.zeros(0), "log_probabilities": np.zeros(0)} for _ in range(n_seqs)]
        y, score, n_paths, lognorm = self._model.viterbi_kbest(seq_ptr, item_ptr, attr, k, device=self.device, values=values,
                                                               allowed=masks)
        out = []
        for s, ys in enumerate(self._split(y, seq_ptr)):
            m = int(n_paths[s])
            out.append({"paths": [[self.classes_[c] for c in ys[:, r].tolist()] for r in range(m)],
                        "scores": score[s, :m].copy(), "log_probabilities": score[s, :m] - lognorm[s]})
        return out

    # ---- max-marginals: scores of best paths under a restriction (``_native.Model.max_marginals``).  Every number is a path score
    # or a difference of two: the log of the ratio of the probabilities of two single paths, NOT a posterior (a margin of 3 says the
    # best competing reading is e^3 times less probable than the best one, not that the call holds with probability 0.95), on the
    # whole-sequence lattice of ``predict``, not a windowed one.
    def predict_max_marginals(self, X, sets=None, allowed=None) -> List[Dict[str, object]]:
        """Max-marginals: per sequence a dict with ``through``, float64 ``[n_items, L]``, ``through[t, l]`` the score of the best
        whole-sequence label path that gives item t the label ``classes_[l]`` (``-inf`` where ``allowed`` leaves no such path);
        ``best``, the score of ``predict``'s path; ``margins`` = ``through - best``, ``<= 0`` up to a few ulps: how much worse the
        best reading becomes when the item is labelled that way; and, with ``sets`` (a list of label sets, each a label or a
        ``set`` / ``frozenset`` / ``list`` / ``tuple`` of labels), ``inside`` and ``outside``, ``[n_items, n_sets]``: the best
        score with the item's label in / not in the set (``-inf`` for a side that is empty or wholly disallowed).

        These are score differences -- the log of the ratio of the probabilities of two single paths --, not posteriors:
        ``predict_marginals`` sums over all paths, this takes the best one.  They live on the whole-sequence lattice (that of
        ``predict``), not a windowed one.  One max-plus forward and one backward walk over ``X``, one native call per 32 sets;
        no forward-backward pass runs.  A sequence without items gets empty arrays and ``best`` 0.0.  Raises ``ValueError``
        before any device call for an unknown label or an empty set."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        bits = None
        if sets is not None:
            try:
                sets = list(sets)
            except TypeError:
                raise ValueError(f"sets is a list of label sets, got {sets!r}") from None
            bits = np.array([self._label_bits(f"set {q}", labels) for q, labels in enumerate(sets)], dtype=np.uint32)
        n_seqs, L = len(seq_ptr) - 1, len(self.classes_)
        n_sets = 0 if bits is None else len(bits)
        if seq_ptr[-1] == 0:
            out = [{"through": np.zeros((0, L)), "margins": np.zeros((0, L)), "best": 0.0} for _ in range(n_seqs)]
            if bits is not None:
                for o in out:
                    o["inside"], o["outside"] = np.zeros((0, n_sets)), np.zeros((0, n_sets))
            return out
        first = self._model.max_marginals(seq_ptr, item_ptr, attr, sets=bits[:32] if n_sets else None, device=self.device,
                                          values=values, allowed=masks)
        inside, outside = [first.get("inside")], [first.get("outside")]
        for k in range(32, n_sets, 32):
            part = self._model.max_marginals(seq_ptr, item_ptr, attr, sets=bits[k:k + 32], device=self.device, values=values,
                                             allowed=masks, want_through=False)
            inside.append(part["inside"])
            outside.append(part["outside"])
        out = []
        for s, th in enumerate(self._split(first["through"], seq_ptr)):
            best = float(first["best"][s])
            out.append({"through": th, "margins": th - best if len(th) else th.copy(), "best": best})
        if bits is not None:
            rows = int(seq_ptr[-1])
            ins = np.concatenate(inside, axis=1) if n_sets else np.zeros((rows, 0))
            outs = np.concatenate(outside, axis=1) if n_sets else np.zeros((rows, 0))
            for o, a, b in zip(out, self._split(ins, seq_ptr), self._split(outs, seq_ptr)):
                o["inside"], o["outside"] = a, b
        return out

    def span_best_scores(self, X, spans, allowed=None) -> Dict[str, np.ndarray]:
        """For every ``(sequence_index, start, stop, labels)`` of ``spans`` (written as ``span_log_probability`` takes them) the
        scores of three best whole-sequence paths, each float64 ``[n_spans]``: ``best``, the sequence's best path (``predict``'s);
        ``inside``, the best path that gives EVERY item of ``X[sequence_index][start:stop]`` a label of ``labels`` -- the score
        ``predict(X, allowed=...)`` reaches with the span pinned to the set --; ``broken``, the best path that gives at least
        one item of the span a label outside ``labels``.  ``-inf`` where no such path exists (``broken`` when ``labels`` holds
        every label).  ``max(inside, broken) = best`` up to rounding.

        ``best - inside`` and ``best - broken`` are score differences -- the log of the ratio of the probabilities of two single
        paths --, not posteriors (``span_log_probability`` gives those).  They live on the whole-sequence lattice, not a windowed
        one; with ``allowed`` (as in ``predict``) on the restricted one.  All spans take two walks over ``X`` and a walk over
        each span, in one native call.  Raises ``ValueError`` before any device call for an unknown label, an empty set, a
        sequence index out of range, ``start >= stop`` or ``start < 0``, and ``stop`` beyond the sequence."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        contig, begin, end, mask = self._span_queries(spans, seq_ptr)
        if len(contig) == 0:
            return {"best": np.zeros(0), "inside": np.zeros(0), "broken": np.zeros(0)}
        got = self._model.max_marginals(seq_ptr, item_ptr, attr, spans=(contig, begin, end, mask), device=self.device, values=values,
                                        allowed=masks, want_through=False)
        return {"best": got["best"][contig], "inside": got["span_best"], "broken": got["span_broken"]}

    @staticmethod
    def _min_run(min_run) -> int:
        try:
            min_run = operator.index(min_run)
        except TypeError:
            raise ValueError(f"min_run is an integer, got {min_run!r}") from None
        if not 1 <= min_run <= 32:
            raise ValueError(f"min_run = {min_run} is outside 1 .. 32")
        return min_run

    def predict_min_run(self, X, labels, min_run, allowed=None) -> List[Dict[str, object]]:
        """The best label path of every sequence AMONG THOSE in which every maximal run of consecutive items carrying a label of
        ``labels`` (a label, or a ``set`` / ``frozenset`` / ``list`` / ``tuple`` of labels; the labels inside a run may differ)
        has at least ``min_run`` items, runs at either end of the sequence included -- on the whole-sequence lattice, that of
        ``predict`` and ``predict_marginals``.  This is not ``predict``'s path with its short runs deleted: the model may prefer
        to stretch a run or to merge two.  Per sequence a dict with ``labels``: the path as a list of label names, or None when
        no path satisfies the constraint (every label in the set and fewer than ``min_run`` items, or ``allowed`` forbids it);
        ``score``: its score (``-inf`` without a path); ``log_probability``: ``score - log Z``, the exact ``log p(y | x)`` of
        the path; ``constraint_log_probability``: ``log Z_C - log Z``, the log of the probability that a path drawn from the
        model satisfies the constraint -- ``<= 0`` up to rounding, reported as computed -- so that ``log_probability -
        constraint_log_probability`` is the path's log-probability given the constraint.  With ``min_run = 1`` the path is
        ``predict``'s.  Ties go by the kernel's scan order over run-counter states (include/gecco_crf.h).  One forward-backward
        pass and two walks over ``X``, one native call.  With ``allowed`` (as in ``predict``) everything is on the restricted
        lattice.  A sequence without items has the empty path: ``labels`` ``[]`` and zeros.  Raises ``ValueError`` before any
        device call for an unknown label, an empty set, and a ``min_run`` that is not an integer or lies outside 1 .. 32."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        bits = self._label_bits("predict_min_run", labels)
        min_run = self._min_run(min_run)
        n_seqs = len(seq_ptr) - 1
        if seq_ptr[-1] == 0:
            return [{"labels": [], "score": 0.0, "log_probability": 0.0, "constraint_log_probability": 0.0} for _ in range(n_seqs)]
        y, score, lognorm_c, lognorm = self._model.viterbi_min_run(seq_ptr, item_ptr, attr, bits, min_run, device=self.device,
                                                                   values=values, allowed=masks)
        out = []
        for s, ys in enumerate(self._split(y, seq_ptr)):
            found = score[s] > -np.inf
            out.append({"labels": [self.classes_[c] for c in ys.tolist()] if found else None, "score": float(score[s]),
                        "log_probability": float(score[s] - lognorm[s]),
                        "constraint_log_probability": float(lognorm_c[s] - lognorm[s])})
        return out

    def predict_marginals_min_run(self, X, labels, min_run, allowed=None) -> List[Dict[str, object]]:
        """How sure the model is of every item AMONG THE PATHS ``predict_min_run`` decodes over: those in which every maximal
        run of consecutive items carrying a label of ``labels`` has at least ``min_run`` items (``labels``, ``min_run`` and
        ``allowed`` as there).  These are not ``predict_marginals``' numbers, which give mass to paths with short runs: a lone
        high-scoring item can have a free marginal of 0.9 and a constrained one near 0.  Per sequence a dict with
        ``marginals``: ``[n_items, L]``, P(item has label | x, the constraint), columns in ``predict_marginals``' order
        (``classes_``); ``inside``: ``[n_items]``, the probability that the item carries a label of ``labels``, the sum of those
        columns; ``constraint_log_probability``: ``log Z_C - log Z`` as ``predict_min_run`` reports it.  ``marginals`` and
        ``inside`` are None when no path satisfies the constraint (``constraint_log_probability`` is then ``-inf``).  One
        forward-backward pass and two walks over ``X``, one native call.  A sequence without items has empty arrays and 0.0.
        Raises the ``ValueError`` s of ``predict_min_run``, before any device call."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        bits = self._label_bits("predict_marginals_min_run", labels)
        min_run = self._min_run(min_run)
        n_seqs = len(seq_ptr) - 1
        L = len(self.classes_)
        if seq_ptr[-1] == 0:
            return [{"marginals": np.zeros((0, L)), "inside": np.zeros(0), "constraint_log_probability": 0.0} for _ in range(n_seqs)]
        marg, inside, lognorm_c, lognorm = self._model.marginals_min_run(seq_ptr, item_ptr, attr, bits, min_run, device=self.device,
                                                                         values=values, allowed=masks)
        out = []
        for s, (ms, ins) in enumerate(zip(self._split(marg, seq_ptr), self._split(inside, seq_ptr))):
            found = lognorm_c[s] > -np.inf
            out.append({"marginals": ms if found else None, "inside": ins if found else None,
                        "constraint_log_probability": float(lognorm_c[s] - lognorm[s])})
        return out

    # ---- run-length potentials: a score on the length of a run (``_native.Model.viterbi_run_length`` / ``marginals_run_length``)
    @staticmethod
    def _length_model(length_scores, tail) -> Tuple[np.ndarray, float]:
        """The table and the tail of a length model, checked before any device call: 1 .. 32 entries, each finite or ``-inf``."""
        try:
            g = np.array(length_scores, dtype=np.float64)
            tail = float(tail)
        except (TypeError, ValueError):
            raise ValueError(f"length_scores is a list of numbers and tail a number, got {length_scores!r} and {tail!r}") from None
        if g.ndim != 1 or not 1 <= g.size <= 32:
            raise ValueError(f"length_scores holds 1 .. 32 scores, got shape {g.shape}")
        if np.isnan(g).any() or (g == np.inf).any():
            raise ValueError("length_scores: a score is finite or -inf, not NaN or +inf")
        if np.isnan(tail) or tail == np.inf:
            raise ValueError(f"tail = {tail} is not finite or -inf")
        return g, tail

    def predict_run_length(self, X, labels, length_scores, tail=0.0, allowed=None) -> List[Dict[str, object]]:
        """The best label path of every sequence under a score on the LENGTH of its runs.  A run is ``predict_min_run``'s: a
        maximal stretch of consecutive items carrying a label of ``labels`` (the labels inside it may differ; runs at either
        end of the sequence count).  With M = ``len(length_scores)`` (1 .. 32), a run of n items adds ``length_scores[min(n, M)
        - 1] + tail * max(n - M, 0)`` to the path's score; every entry is finite or ``-inf``, and ``-inf`` forbids what it
        scores.  Zeros are ``predict``; ``[-inf] * (m - 1) + [0]`` is ``predict_min_run(m)``; ``tail=-inf`` is a maximum run
        length M; anything else is a soft duration model (``fit_run_length_scores`` learns one).  Per sequence a dict with
        ``labels``: the path, or None when no path is feasible; ``score``: its score with the length terms (``-inf`` without a
        path); ``log_probability_given_model``: ``score - log Z_g``, the path's log-probability under the extended model;
        ``log_mass_ratio``: ``log Z_g - log Z``, the log of the expected ``exp`` of the length terms under the plain model.
        On the whole-sequence lattice, not a windowed one; with ``allowed`` (as in ``predict``) on the restricted one.  One
        forward-backward pass and two walks over ``X``, one native call.  A sequence without items has the empty path and zeros.
        Raises ``ValueError`` before any device call for an unknown label, an empty set, a table that does not hold 1 .. 32
        scores, and a NaN or ``+inf`` among the scores."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        bits = self._label_bits("predict_run_length", labels)
        g, tail = self._length_model(length_scores, tail)
        n_seqs = len(seq_ptr) - 1
        if seq_ptr[-1] == 0:
            return [{"labels": [], "score": 0.0, "log_probability_given_model": 0.0, "log_mass_ratio": 0.0} for _ in range(n_seqs)]
        y, score, lognorm_g, lognorm = self._model.viterbi_run_length(seq_ptr, item_ptr, attr, bits, g, tail, device=self.device,
                                                                      values=values, allowed=masks)
        out = []
        for s, ys in enumerate(self._split(y, seq_ptr)):
            found = score[s] > -np.inf
            out.append({"labels": [self.classes_[c] for c in ys.tolist()] if found else None, "score": float(score[s]),
                        "log_probability_given_model": float(score[s] - lognorm_g[s]) if found else -np.inf,
                        "log_mass_ratio": float(lognorm_g[s] - lognorm[s])})
        return out

    def predict_marginals_run_length(self, X, labels, length_scores, tail=0.0, allowed=None) -> List[Dict[str, object]]:
        """How sure the model is of every item under the length model of ``predict_run_length`` (the same arguments).  Per
        sequence a dict with ``marginals``: ``[n_items, L]``, columns in ``predict_marginals``' order; ``inside``: ``[n_items]``,
        the probability that the item carries a label of ``labels``; ``counts``: ``[M + 1]``, entry d - 1 the expected number of
        runs with min(length, M) = d and the last entry the expected number of items beyond the M-th of their runs;
        ``log_mass_ratio``: ``log Z_g - log Z``.  ``marginals`` and ``inside`` are None when no path is feasible
        (``log_mass_ratio`` is then ``-inf`` and ``counts`` zeros).  One forward-backward pass and two walks over ``X``, one
        native call.  A sequence without items has empty arrays, zero counts and 0.0.  Raises the ``ValueError`` s of
        ``predict_run_length``, before any device call."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        bits = self._label_bits("predict_marginals_run_length", labels)
        g, tail = self._length_model(length_scores, tail)
        n_seqs, L = len(seq_ptr) - 1, len(self.classes_)
        if seq_ptr[-1] == 0:
            return [{"marginals": np.zeros((0, L)), "inside": np.zeros(0), "counts": np.zeros(g.size + 1), "log_mass_ratio": 0.0}
                    for _ in range(n_seqs)]
        marg, inside, counts, lognorm_g, lognorm = self._model.marginals_run_length(seq_ptr, item_ptr, attr, bits, g, tail,
                                                                                    device=self.device, values=values, allowed=masks)
        out = []
        for s, (ms, ins) in enumerate(zip(self._split(marg, seq_ptr), self._split(inside, seq_ptr))):
            found = lognorm_g[s] > -np.inf
            out.append({"marginals": ms if found else None, "inside": ins if found else None, "counts": counts[s].copy(),
                        "log_mass_ratio": float(lognorm_g[s] - lognorm[s])})
        return out

    def run_length_counts(self, X, labels, length_scores, tail=0.0) -> np.ndarray:
        """The expected run-length counts of every sequence under the length model of ``predict_run_length``: float64 ``[n_seqs,
        M + 1]``, column d - 1 the expected number of runs with min(length, M) = d, the last column the expected number of
        items beyond the M-th of their runs.  With zeros for the scores these are the plain model's expectations (their first M
        columns sum to ``expected_runs``).  One native call; a sequence without items, or without a feasible path, has zeros."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        bits = self._label_bits("run_length_counts", labels)
        g, tail = self._length_model(length_scores, tail)
        if seq_ptr[-1] == 0:
            return np.zeros((len(seq_ptr) - 1, g.size + 1))
        return self._model.marginals_run_length(seq_ptr, item_ptr, attr, bits, g, tail, device=self.device, values=values,
                                                want_marginals=False, want_inside=False)[2]

    @staticmethod
    def observed_run_lengths(paths, inside, max_length: int) -> np.ndarray:
        """The run-length counts of label paths: ``[len(paths), max_length + 1]`` in ``run_length_counts``' columns; ``inside``
        says of a label whether it belongs to the set."""
        out = np.zeros((len(paths), max_length + 1))
        for q, path in enumerate(paths):
            run = 0
            for lab in list(path) + [None]:
                if lab is not None and inside(lab):
                    run += 1
                    continue
                if run:
                    out[q, min(run, max_length) - 1] += 1.0
                    out[q, max_length] += max(run - max_length, 0)
                run = 0
        return out

    def fit_run_length_scores(self, X, y, labels, max_length, c2=1.0, **lbfgs) -> Tuple[np.ndarray, float]:
        """Learn the length model of ``predict_run_length`` from labelled sequences, the CRF's own weights held fixed:
        ``(length_scores [max_length], tail)`` that minimise

            F(g, tau) = sum over the sequences of (log Z_g(x) - score_g(y)) + c2 / 2 * (|g|^2 + tau^2),

        the penalised negative log-likelihood of ``y`` under the extended model.  The length scores are log-linear features
        ("the number of runs of length d"), so F is convex -- strongly, with modulus ``c2`` -- and its gradient is the expected
        minus the observed run-length counts plus ``c2`` times the parameters.  L-BFGS (``train.minimize`` with ``c1 = 0``) from
        zeros; one evaluation is one ``marginals_run_length`` call over all of ``X`` (``lbfgs`` passes ``epsilon``, ``delta``,
        ``max_iterations`` ... on).  The observed counts are taken from ``y`` on the host.  ``fit_run_length_result_`` keeps the
        optimiser's result (its ``n_eval`` counts the native calls).  Raises ``ValueError`` before any device call for an
        unknown label, an empty set, ``max_length`` outside 1 .. 32, ``c2 <= 0``, a ``y`` that does not match ``X``, and an entry
        of ``y`` that is a set of labels or None (partial labels carry no run lengths)."""
        from . import train

        seq_ptr, item_ptr, attr, values = self._pack(X)
        bits = self._label_bits("fit_run_length_scores", labels)
        try:
            M = operator.index(max_length)
        except TypeError:
            raise ValueError(f"max_length is an integer, got {max_length!r}") from None
        if not 1 <= M <= 32:
            raise ValueError(f"max_length = {M} is outside 1 .. 32")
        c2 = float(c2)
        if not c2 > 0.0 or not np.isfinite(c2):
            raise ValueError(f"c2 = {c2} is not a positive number (it is what makes the fit strongly convex)")
        y = [list(yseq) for yseq in y]
        n_seqs = len(seq_ptr) - 1
        if len(y) != n_seqs:
            raise ValueError(f"X holds {n_seqs} sequences and y {len(y)}")
        index = {c: k for k, c in enumerate(self.classes_)}
        for k, ls in enumerate(y):
            if len(ls) != seq_ptr[k + 1] - seq_ptr[k]:
                raise ValueError(f"sequence {k}: {seq_ptr[k + 1] - seq_ptr[k]} items but {len(ls)} labels")
            for lab in ls:
                if lab is None or isinstance(lab, (set, frozenset, list, tuple)):
                    raise ValueError(f"sequence {k}: fit_run_length_scores takes one label per item, got {lab!r} (a partially labelled "
                                     f"sequence has no run lengths to count)")
                if str(lab) not in index:
                    raise ValueError(f"unknown label {str(lab)!r} (classes_: {self.classes_})")
        observed = self.observed_run_lengths([[index[str(lab)] for lab in ls] for ls in y], lambda k: (bits >> k) & 1, M).sum(axis=0)
        if seq_ptr[-1] == 0:
            self.fit_run_length_result_ = None
            return np.zeros(M), 0.0
        gold = -float(self.log_likelihood(X, y).sum())  # sum of log Z - score(y): the part of F that the length model does not move

        def fg(theta):
            _, _, counts, lognorm_g, lognorm = self._model.marginals_run_length(
                seq_ptr, item_ptr, attr, bits, theta[:M], theta[M], device=self.device, values=values, want_marginals=False,
                want_inside=False)
            f = gold + float((lognorm_g - lognorm).sum()) - float(observed @ theta) + 0.5 * c2 * float(theta @ theta)
            return f, counts.sum(axis=0) - observed + c2 * theta

        result = train.minimize(fg, np.zeros(M + 1), c1=0.0, **lbfgs)
        self.fit_run_length_result_ = result
        theta = np.asarray(result.x, dtype=np.float64)
        return theta[:M].copy(), float(theta[M])

    # ---- run counts: how many runs a sequence holds, and the best path of every count (``_native.Model.run_counts``)
    @staticmethod
    def _max_runs(max_runs) -> int:
        try:
            max_runs = operator.index(max_runs)
        except TypeError:
            raise ValueError(f"max_runs is an integer, got {max_runs!r}") from None
        if not 1 <= max_runs <= 32:
            raise ValueError(f"max_runs = {max_runs} is outside 1 .. 32")
        return max_runs

    def run_count_log_probability(self, X, labels, max_runs, allowed=None) -> np.ndarray:
        """The distribution of the NUMBER of runs: float64 ``[n_seqs, max_runs + 1]``, column k the log-probability that the
        sequence holds exactly k maximal runs of consecutive items carrying a label of ``labels`` (a label, or a ``set`` /
        ``frozenset`` / ``list`` / ``tuple`` of labels; the labels inside a run may differ; runs at either end of the sequence
        count), and the last column log P(at least ``max_runs`` runs).  ``expected_runs`` is the mean of this distribution and
        says nothing else of it: a mean of 1.0 can be "certainly one" or a coin flip between none and two.  Column 0 is the
        probability that the sequence holds no such item at all.  Exact, on the whole-sequence lattice (that of ``predict`` and
        ``predict_marginals``): one forward-backward pass and one walk over ``X`` on the lattice expanded by a run counter,
        one native call.  A row is normalised by the walk's own total, so its exponentials sum to 1 to rounding; a count that
        no path has is ``-inf``.  With ``allowed`` (as in ``predict``) everything is on the restricted lattice.  A sequence
        without items has no run: 0 in column 0.  Raises ``ValueError`` before any device call for an unknown label, an empty
        set, and a ``max_runs`` that is not an integer or lies outside 1 .. 32."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        bits = self._label_bits("run_count_log_probability", labels)
        max_runs = self._max_runs(max_runs)
        n_seqs = len(seq_ptr) - 1
        if seq_ptr[-1] == 0:
            out = np.full((n_seqs, max_runs + 1), -np.inf)
            out[:, 0] = 0.0
            return out
        mass, _, _, _ = self._model.run_counts(seq_ptr, item_ptr, attr, bits, max_runs, device=self.device, values=values,
                                               allowed=masks, want_paths=False, want_lognorm=False)
        top = mass.max(axis=1, keepdims=True)  # (finite: every sequence has a path)
        return mass - (top + np.log(np.exp(mass - top).sum(axis=1, keepdims=True)))

    def run_count_probability(self, X, labels, max_runs, allowed=None) -> np.ndarray:
        """``exp`` of ``run_count_log_probability``: column k is P(exactly k runs), the last column P(at least ``max_runs``)."""
        return np.exp(self.run_count_log_probability(X, labels, max_runs, allowed=allowed))

    def predict_run_counts(self, X, labels, max_runs, allowed=None) -> List[Dict[str, object]]:
        """The best label path of every sequence for every number of runs: among the paths with exactly k maximal runs of items
        carrying a label of ``labels``, k = 0 .. ``max_runs`` - 1, and among those with at least ``max_runs`` (``labels``,
        ``max_runs`` and ``allowed`` as in ``run_count_log_probability``).  The best path with exactly one run is not
        ``predict``'s path with its surplus runs deleted or merged by hand.  Per sequence a dict with ``paths``: ``max_runs +
        1`` entries, each a list of label names, or None where no path has that count (more runs than ``ceil(n_items / 2)``,
        none when every label is in the set, or ``allowed`` forbids it); ``scores``: float64 ``[max_runs + 1]``, ``-inf`` without
        a path; ``log_probabilities``: ``score - log Z``, the exact ``log p(y | x)`` of each path.  The best of the ``max_runs +
        1`` scores is ``predict``'s path's.  Ties go by the kernel's scan order over run-counter states (include/gecco_crf.h).
        One forward-backward pass and one walk over ``X``, one native call.  A sequence without items has the empty path in
        entry 0.  Raises the ``ValueError`` s of ``run_count_log_probability``, before any device call."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        bits = self._label_bits("predict_run_counts", labels)
        max_runs = self._max_runs(max_runs)
        n_seqs = len(seq_ptr) - 1
        if seq_ptr[-1] == 0:
            first = np.full(max_runs + 1, -np.inf)
            first[0] = 0.0
            return [{"paths": [[]] + [None] * max_runs, "scores": first.copy(), "log_probabilities": first.copy()} for _ in range(n_seqs)]
        _, score, y, lognorm = self._model.run_counts(seq_ptr, item_ptr, attr, bits, max_runs, device=self.device, values=values,
                                                      allowed=masks, want_log_mass=False)
        out = []
        for s in range(n_seqs):
            b, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
            paths = [[self.classes_[c] for c in y[k, b:e].tolist()] if score[s, k] > -np.inf else None for k in range(max_runs + 1)]
            out.append({"paths": paths, "scores": score[s].copy(), "log_probabilities": score[s] - lognorm[s]})
        return out

    # ---- edge posteriors: the pairwise marginals of the whole-sequence lattice and their sums (``_native.Model.edge_posteriors``)
    def _edges(self, X, allowed, sets=None, **want):
        """One pass over ``X`` for the edge outputs ``want`` names: ``(seq_ptr, masks of sets, the native call's dict)``, the dict
        None when ``X`` holds no item (the device is not reached).  Every refusal is raised here, before any device call.  More
        than 32 sets are served by several native calls: the outputs that do not depend on the sets come from the first."""
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        bits = None
        if sets is not None:
            try:
                sets = list(sets)
            except TypeError:
                raise ValueError(f"sets is a list of label sets, got {sets!r}") from None
            bits = np.array([self._label_bits(f"set {q}", labels) for q, labels in enumerate(sets)], dtype=np.uint32)
        if seq_ptr[-1] == 0:
            return seq_ptr, bits, None
        if bits is None or len(bits) == 0:
            return seq_ptr, bits, self._model.edge_posteriors(seq_ptr, item_ptr, attr, device=self.device, values=values,
                                                              allowed=masks, **want)
        out = None
        for k in range(0, len(bits), 32):
            part = self._model.edge_posteriors(seq_ptr, item_ptr, attr, sets=bits[k:k + 32], device=self.device, values=values,
                                               allowed=masks, **(want if out is None else self._NO_EDGE_EXTRAS))
            if out is None:
                out = part
            else:
                out["enter"] = np.concatenate([out["enter"], part["enter"]], axis=1)
                out["leave"] = np.concatenate([out["leave"], part["leave"]], axis=1)
        return seq_ptr, bits, out

    _NO_EDGE_EXTRAS = dict(want_pair=False, want_transitions=False, want_entropy=False, want_marginals=False)

    def predict_pair_marginals(self, X, allowed=None) -> List[np.ndarray]:
        """Pairwise (edge) marginals on the whole-sequence lattice (that of ``predict`` and ``predict_marginals``): per sequence
        one float64 ``[n_items, L, L]`` array, ``out[t, i, j] = P(y_{t-1} = classes_[i], y_t = classes_[j] | x)``; row 0, which
        no edge enters, is zeros.  Memory: 8 L^2 bytes per item on the device and on the host -- 8 KB per item at 32 labels, 1.6 GB
        for 200 000 items; ``boundary_probability``, ``expected_transitions`` and ``path_entropy`` form their sums on the
        device without this table.  With ``allowed`` (as in ``predict_marginals``) the lattice is the restricted one and a
        disallowed (item, label) pair is exactly 0.0."""
        seq_ptr, _, out = self._edges(X, allowed, want_pair=True, want_transitions=False, want_entropy=False)
        L = len(self.classes_)
        if out is None:
            return [np.zeros((0, L, L)) for _ in range(len(seq_ptr) - 1)]
        return self._split(out["pair"], seq_ptr)

    def boundary_probability(self, X, sets, allowed=None) -> List[Tuple[np.ndarray, np.ndarray]]:
        """Where runs of labels start and end, exactly: per sequence ``(enter, leave)``, each float64 ``[n_items, n_sets]``.  For
        the label set S = ``sets[s]`` (a label, or a ``set`` / ``frozenset`` / ``list`` / ``tuple`` of labels, as in
        ``span_log_probability``) ``enter[t, s]`` is the probability, given the whole sequence, that item t carries a label of S
        and item t - 1 does not (or t is the first item): a run of S starts at t.  ``leave[t, s]`` likewise for a run that ends
        at t.  Sums of entries of the pairwise marginals, formed on the device; an alternative of probability 1e-6 is reported
        as such.  One forward-backward pass and one native call per 32 sets.  Raises ``ValueError`` before any device call for
        an unknown label or an empty set."""
        seq_ptr, bits, out = self._edges(X, allowed, sets=() if sets is None else sets, want_transitions=False, want_entropy=False)
        if out is None or len(bits) == 0:
            return [(np.zeros((int(n), len(bits))), np.zeros((int(n), len(bits)))) for n in np.diff(seq_ptr)]
        return list(zip(self._split(out["enter"], seq_ptr), self._split(out["leave"], seq_ptr)))

    def expected_transitions(self, X, allowed=None) -> np.ndarray:
        """Expected transition counts: float64 ``[n_seqs, L, L]``, ``out[s, i, j]`` = the expected number of items of sequence s
        that carry ``classes_[j]`` right after an item that carries ``classes_[i]``, under the path distribution p(y | x): the
        sum of the pairwise marginals over the sequence's edges (zeros for a sequence of 0 or 1 items)."""
        seq_ptr, _, out = self._edges(X, allowed, want_entropy=False)
        L = len(self.classes_)
        return np.zeros((len(seq_ptr) - 1, L, L)) if out is None else out["transitions"]

    def expected_runs(self, X, sets, allowed=None) -> np.ndarray:
        """The expected number of maximal runs of items whose labels lie in a set: float64 ``[n_seqs, n_sets]``, for
        ``sets[s]`` = S the value P(y_0 in S) + the sum over i outside S and j inside S of ``expected_transitions[i, j]``, added
        on the host (with S every label but the background: the expected number of clusters of a contig).  Equal to the sum
        over the sequence of ``boundary_probability``'s ``enter``."""
        seq_ptr, bits, out = self._edges(X, allowed, sets=() if sets is None else sets, want_entropy=False, want_marginals=True)
        n_seqs, L = len(seq_ptr) - 1, len(self.classes_)
        runs = np.zeros((n_seqs, len(bits)))
        if out is None:
            return runs
        full = np.flatnonzero(np.diff(seq_ptr) > 0)  # (a sequence without items has no run)
        first = out["marginals"][seq_ptr[:-1][full]]
        for s, m in enumerate(bits.tolist()):
            inside = np.array([(m >> y) & 1 for y in range(L)], dtype=bool)
            runs[:, s] = out["transitions"][:, ~inside][:, :, inside].sum(axis=(1, 2))
            runs[full, s] += first[:, inside].sum(axis=1)
        return runs

    def path_entropy(self, X, allowed=None) -> np.ndarray:
        """The entropy H(Y | x) of every sequence's path distribution in nats, float64 ``[n_seqs]``: 0 when one path has all
        the mass, at most ``n_items * log(L)``.  By the chain rule over the sequence's edges, a sum of non-negative terms:
        never negative, and small on a confident sequence without cancellation.  0.0 for a sequence without items."""
        seq_ptr, _, out = self._edges(X, allowed, want_transitions=False)
        return np.zeros(len(seq_ptr) - 1) if out is None else out["entropy"]

    def _windowed(self) -> None:
        self._fitted()
        if self.window_size is None:
            raise ValueError("this SequenceCRF has no window (window_size=None): it has no windowed predictions")

    def predict_windowed(self, X, label: str, pad: bool = True, allowed=None) -> List[np.ndarray]:
        """GECCO's windowed probability of ``label``: per item the maximum, over the windows covering it, of the
        label's marginal inside the window (``pad``: a sequence shorter than the window is one window).  With ``allowed``
        every window runs on the lattice restricted to the allowed sets (padding items allow every label)."""
        self._windowed()
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        if str(label) not in self.classes_:
            raise ValueError(f"unknown label {label!r} (classes_: {self.classes_})")
        if seq_ptr[-1] == 0:
            return [np.zeros(0) for _ in X]
        p = self._model.windowed_marginals(seq_ptr, item_ptr, attr, self.window_size, self.window_step,
                                           label=self.classes_.index(str(label)), pad=pad, device=self.device,
                                           values=values, allowed=masks)
        return self._split(p, seq_ptr)

    def predict_windowed_all(self, X, background: Optional[str] = None, pad: bool = True, allowed=None):
        """GECCO's windowed probability of every label in one device pass: one ``[n_items, L]`` array per sequence, columns
        in ``classes_`` order (per item and label the maximum, over the windows covering the item, of the label's marginal
        inside the window).  With ``background`` also, second, one ``[n_items]`` array per sequence: the maximum over the
        same windows of the probability of any label but ``background``.  ``allowed``: as in ``predict_windowed``."""
        self._windowed()
        seq_ptr, item_ptr, attr, values = self._pack(X)
        masks = self._allowed(allowed, seq_ptr)
        L = len(self.classes_)
        if background is not None and str(background) not in self.classes_:
            raise ValueError(f"unknown label {background!r} (classes_: {self.classes_})")
        if seq_ptr[-1] == 0:
            empty = [np.zeros((0, L)) for _ in X]
            return empty if background is None else (empty, [np.zeros(0) for _ in X])
        bg = None if background is None else self.classes_.index(str(background))
        p_all, p_any = self._model.windowed_marginals_all(seq_ptr, item_ptr, attr, self.window_size, self.window_step,
                                                          background=bg, pad=pad, device=self.device,
                                                          values=values, allowed=masks)
        if background is None:
            return self._split(p_all, seq_ptr)
        return self._split(p_all, seq_ptr), self._split(p_any, seq_ptr)
