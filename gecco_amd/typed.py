"""A type-aware cluster CRF: a gene is labelled ``0`` or with the type of the cluster it lies in.

``TypedClusterCRF`` trains a many-label CRF on GECCO's tables (``train.build_training_set`` with up to 32 labels,
``train.fit_training_set``), scores genes with ONE device pass that gives every label's windowed probability and the
probability of lying in any cluster (``_native.Model.windowed_marginals_all``, ``csrc/crf_general_windowed.hip``), calls
clusters on the latter with the segment kernel, and gives every call a type and per-type probabilities from the former:
the ``type`` and ``*_probability`` columns of ``clusters.tsv``, which the random forest fills otherwise.

Labels.  A gene outside every cluster is ``"0"`` (the background).  A gene inside a cluster carries the ``";"``-joined
sorted type names of that cluster, ``"Unknown"`` when it has none.  A gene overlaps a cluster as ``train_cli`` decides it
for the 2-label model (``join_clusters``: same sequence, bounds inclusive; ``assigned_clusters``: rows without a
cluster id are skipped, a repeated id is an error); of several clusters the first in ``cluster_id`` order gives the label.  More than 31 cluster labels do not fit the trainer's 32: the
composite labels (those with a ``";"``) with the fewest clusters are folded into one label ``"Mixed"``, fewest first,
ties by name, until 31 remain.

``unknown="any"`` (``--unknown any``): a cluster without a type says that its genes lie in a cluster of *some* type, which is
a set of allowed labels, not a label.  Its genes then carry the set of every cluster label of the training set (everything but
the background), ``"Unknown"`` is no label of the model, and the fit maximises the marginal likelihood of the allowed paths
(``train.build_training_set``'s partial labels).  The set needs at least one cluster with a type.  The default,
``unknown="label"``, is the labelling above.

Type of a call.  For a type t and a gene g, v[g] = the sum over the labels whose names contain t, in label order, of the
label's windowed probability; the cluster's probability of t is ``min(1, exact mean of v over its genes)``; its type is
the set of t with a probability above 0.5 (the rule of ``TypeClassifier.predict_types``), ``Unknown`` when empty.
``"Mixed"`` and ``"Unknown"`` contain no type.

Region posteriors (opt-in: ``region_posteriors=True``, ``predict --region-posteriors``).  The numbers above are per-gene
numbers.  With the flag every called cluster also carries ``region_probability``, the posterior probability that EVERY gene
of the called region carries a cluster label (anything but the background), and ``region_type_probabilities[t]``, the
posterior probability that every gene's label contains type t -- probabilities of the whole region under the model, which
are not functions of the per-gene numbers.  They are WHOLE-CONTIG posteriors, on the lattice of ``SequenceCRF.predict`` and
``predict_marginals`` (``_native.Model.span_log_probabilities``: one forward-backward pass per batch, all regions in one
native call), not windowed ones: the model's parameters are those fitted on windows, the conditioning is on the whole
contig.  ``known=`` restricts that lattice as it restricts the windows.  ``clusters.tsv`` then has the columns ``region_p``
and ``{type}_region_p``; without the flag the tables are unchanged.

Attributions (opt-in: ``attributions=True``, ``predict --attributions [--attribution-reach R]``).  "Which genes and domains
does this call rest on": with E the event that every gene of the called region carries a cluster label, every gene in the
region and R genes on either side gets ``contribution`` = log P(E | x) - log P(E | x without anything the gene carries), and
every domain of such a gene the same with that one domain taken out -- exact, the values a second run on the edited input
would give, from the marginals conditioned on E (``_native.Model.span_conditionals``: one forward-backward pass per batch,
every cluster in one native call).  Positive where the call leans on the gene or domain, negative where it speaks against
it.  WHOLE-CONTIG posteriors like the region posteriors, and ``known=`` restricts the lattice in the same way.  The command
line writes ``attributions.tsv``; without the flag the tables and every launch are unchanged.

Boundary intervals (opt-in: ``boundary_samples=N > 0``, ``predict --boundary-samples N [--seed S]``).  "How sure are you about
where it starts and ends": N label paths per contig are drawn from the path distribution p(y | x)
(``_native.Model.sample_paths``: forward filtering, backward sampling, one forward-backward pass and one native call per
batch; the draws are a function of ``seed`` alone).  Every called cluster gets one run query: its anchor is the cluster's gene
with the greatest any-cluster probability (the first on ties), and in every path whose label at the anchor is not the
background, the run is the maximal stretch of genes around the anchor without a background label.  With m the number of such
paths: ``anchor_probability = m / N``; ``exact_probability`` = the share of the N paths whose run is exactly the called gene
range; ``start_interval`` and ``end_interval`` = (lower, upper), the 5 % and 95 % order statistics over the m runs of the first
gene's ``start`` and of the last gene's ``end`` -- the sorted values at indices floor(0.05 (m - 1)) and ceil(0.95 (m - 1)); with
m = 0 the called cluster's own start and end.  Like the region posteriors these are WHOLE-CONTIG posteriors, not windowed
ones, and ``known=`` restricts the lattice in the same way.  ``clusters.tsv`` then has the columns ``anchor_p``, ``exact_p``,
``start_lo``, ``start_hi``, ``end_lo`` and ``end_hi`` behind the region columns; with N = 0 the tables and every launch are
unchanged.

Boundary posteriors (opt-in: ``boundary_posteriors=True``, ``predict --boundary-posteriors``).  The exact counterpart of the
sampled intervals: with S the set of every label but the background, every called cluster carries ``start_probability``, the
whole-contig posterior probability that a run of cluster labels STARTS at its first gene (that gene is in S and the gene
before it, if any, is not), and ``end_probability``, that one ENDS at its last gene -- sums of entries of the pairwise
marginals of the edge entering the first gene, and of the edge leaving the last (``_native.Model.edge_posteriors``: one forward-backward pass and one native call per
batch, every gene of the batch at once).  ``sequence_posteriors_`` then holds, per contig, ``sequence_id``, ``genes``,
``log_z``, ``entropy`` (of the contig's path distribution, in nats) and ``expected_clusters`` (the expected number of runs of
S: the sum over the contig of the start probabilities).  Whole-contig posteriors like the region posteriors, and ``known=``
restricts the lattice in the same way.  ``clusters.tsv`` then has the columns ``start_p`` and ``end_p`` behind the other
optional columns, and the command line writes ``sequences.tsv``; without the flag the tables and every launch are unchanged.

Run posteriors (opt-in: ``run_posteriors=True``, ``predict --run-posteriors [--run-reach R]``, R = 256 by default).  The three
boundary features answer three different questions.  The SAMPLED intervals above estimate the distribution of the run through a
cluster's anchor by counting N drawn paths: an alternative of probability 1e-4 is seen rarely or never, and the numbers move with
the seed.  The per-gene EDGE posteriors above are exact, but ``start_p`` is the probability that SOME run starts at a gene, a
neighbouring run's start included.  The per-run posteriors here are the exact distribution of where THE RUN THROUGH THE ANCHOR
starts and ends (``_native.Model.run_posteriors``: one forward-backward pass and one native call per batch, per cluster a masked
walk of at most R + 2 genes to either side of the anchor).  With S every label but the background and the anchor of the boundary
intervals (the gene with the greatest any-cluster probability, the first on ties), every called cluster carries
``run_anchor_probability`` = P(the anchor's label is in S); ``run_probability`` = P(a run of S is EXACTLY the called gene range:
every gene inside, the neighbours outside) -- one entry of the joint distribution of start and end, which is NOT the product of
the two marginal distributions; ``run_start_interval`` and ``run_end_interval`` = (lower, upper) from the distribution GIVEN that
the anchor is in S: positions in ascending coordinate order, the mass beyond the reach placed outside the farthest gene the walk
reaches, lower = the first position whose cumulative mass is >= 0.05 and upper = the first with >= 0.95, reported as the gene's
``start`` (starts) or ``end`` (ends) like the sampled columns, a bound that falls into the mass beyond the reach clamped to the
gene at the reach, and the cluster's own start and end where the anchor's probability is 0; ``run_start_beyond_probability`` and
``run_end_beyond_probability``, the conditional mass beyond the reach (0 says the interval was not clamped); and
``run_boundaries``, the conditional distributions themselves as ``(side, gene, position, p)``.  Whole-contig posteriors like the
others, and ``known=`` restricts the lattice in the same way.  ``clusters.tsv`` then has the columns ``run_anchor_p``, ``run_p``,
``run_start_lo``, ``run_start_hi``, ``run_end_lo``, ``run_end_hi``, ``run_start_beyond_p`` and ``run_end_beyond_p`` behind every
other optional column, and the command line writes ``boundaries.tsv`` (columns ``cluster_id, side, protein_id, position, p``: the
entries with p >= 1e-6); without the flag the tables and every launch are unchanged.

Alternatives (opt-in: ``alternatives=K``, 1 <= K <= 32, ``predict --alternatives K [--alternatives-margin M]``, M = 10 by default).
"What are the next-best readings of this region, and how much probability does each carry": for every called cluster the K best
label paths of its neighbourhood, exactly (``_native.Model.viterbi_kbest``: list Viterbi on the device, one native call for all
clusters), not a share of draws.  The neighbourhood is the contig's genes [first - M - 1, last + M + 1), clipped to the contig,
as a short sequence of its own; a copied end gene that is not a contig end is pinned, by a singleton mask, to the label the
contig's Viterbi path gives it, and ``known=`` masks carry over.  Conditioning a chain on both border labels separates the
inside from the rest of the contig: the K paths are exactly the K best WHOLE-CONTIG paths among those that agree with the
Viterbi path outside the neighbourhood, and exp(score - log Z) of the short, masked sequence is each path's probability GIVEN
that agreement (not its unconditional probability).  Every cluster gets ``alternatives``, a list of dicts, best first:
``rank``; ``window`` = (first, last + 1), the neighbourhood as gene offsets inside the contig, and ``labels``, the path's label
names over it; ``run`` = (first, last + 1), contig offsets of the maximal stretch of genes without a background label around
the cluster's anchor (the anchor of the boundary intervals) on the path spliced into the contig's Viterbi path, or None where
the anchor's label is the background; ``start`` and ``end``, the run's coordinates (None without a run); ``type``, the
``";"``-joined types of the run's most frequent label (the smaller label id on ties; ``"Unknown"`` for a label without types,
None without a run); ``log_p``.  Rank 0 is the Viterbi path's reading.  The command line writes ``alternatives.tsv`` (columns
``cluster_id, rank, start, end, type, log_p, p``; start, end and type empty without a run); ``clusters.tsv`` is unchanged, and
without the option the tables and every launch are unchanged.

Margins (opt-in: ``margins=True``, ``predict --margins``).  "How much worse is the best reading without this cluster, or one that
breaks it somewhere": differences of best-path scores from the max-marginals of the whole-contig lattice
(``_native.Model.max_marginals``: one max-plus forward and one backward walk of the batch and a short walk per call, one native
call for all clusters, no forward-backward pass).  Every cluster gets ``margin_present``, ``margin_absent``, ``margin_broken`` and
``type_margins`` (``TypedClusterCRF._margins`` defines them).  They are score differences -- the log of the ratio of the
probabilities of two single label paths -- and not posteriors; they live on the whole-contig lattice (that of the path clusters),
not the windowed one the calls come from.  ``clusters.tsv`` then has the columns ``margin_present``, ``margin_absent`` and
``margin_broken`` behind every other optional column; without the flag the tables and every launch are unchanged.

Path clusters (``predict_path_clusters(genes, min_run=M)``, ``predict --path-clusters M``, 1 <= M <= 32).  The refiner drops a
cluster of fewer than ``n_cds`` annotated genes after the fact; a decoded path with its short runs deleted is not the best path
among those without short runs -- the model may prefer to stretch a run of two genes to three, or to merge two runs across a gap
of one.  One whole-contig call (``_native.Model.viterbi_min_run``: a Viterbi recursion on the lattice expanded by a run counter)
gives every contig its best label path among those in which every run of genes with a label other than the background has at
least M GENES (genes, not annotated genes: ``n_cds`` counts annotated ones), and the clusters are that path's runs: ids
``{sequence}_cluster_{number}``, ``type`` from the run's most frequent label as the alternatives derive it.
``path_posteriors_`` then holds one row per contig: ``sequence_id``, ``genes``, ``log_z``, ``score`` and ``log_p`` (the path's
score and exact log-probability; ``-inf`` where no path satisfies the constraint, a contig shorter than M whose every label is
a cluster label under ``known=``), ``constraint_log_p`` = log P(no run shorter than M | x), and ``clusters``.  The command line
writes ``path_clusters.tsv`` (columns ``sequence_id, cluster_id, start, end, genes, type``) and ``paths.tsv`` next to the other
tables, which stay byte for byte what they are without the flag.

Path marginals (``predict_path_clusters(..., marginals=True)``, ``predict --path-clusters M --path-marginals``).  The free
marginals are the wrong numbers to attach to a path cluster: they give mass to paths with runs shorter than M, which the
constrained decoder rules out.  One more whole-contig call after the decode (``_native.Model.marginals_min_run`` with the same
set and the same ``known`` masks, 8 bytes per gene back) gives every gene ``inside`` = P(the gene lies in a region | x, no region
is shorter than M); every path cluster gains ``average_p``, ``max_p`` and ``min_p`` of it over its genes (the mean is
``numpy.mean``, as the refiner takes a cluster's mean), and ``path_gene_probabilities_`` holds it per gene.  The command line
appends the three columns to ``path_clusters.tsv`` and writes ``path_genes.tsv`` (columns ``sequence_id, protein_id, path_label,
p``).  Without the flag every table and every launch is what it is today.

A length model (``fit_length_model(genes, clusters, max_length=M)``, ``train --length-model M``; ``predict_path_clusters(...,
length_model=True)``, ``predict --path-clusters --length-model``).  A minimum of M genes is one hand-picked point of what a
region's length can say: real regions have almost none under three genes and most between ten and forty.  The length model is a
table of M scores (entry d - 1: a region of min(genes, M) = d genes) and a tail score per gene beyond the M-th, learnt from the
training tables with the CRF's weights held fixed (``SequenceCRF.fit_run_length_scores``: convex, one whole-contig call per
evaluation), saved as ``typed_length_model.tsv`` next to the model and loaded with it; a directory without the table has no
length model.  With ``length_model=True`` the path clusters are the runs of the best whole-contig path under those scores
(``_native.Model.viterbi_run_length``), ``marginals=True`` takes its probabilities under them
(``_native.Model.marginals_run_length``), and ``min_run`` is not used: giving both is an error.

Cluster counts (``predict_cluster_counts(genes, max_clusters=K)``, ``predict --cluster-counts K``, 1 <= K <= 32).  How many
clusters does a contig hold, and how sure is the model of that number?  ``expected_clusters`` of ``sequences.tsv`` is the mean of
the distribution and nothing else: 1.0 can be "certainly one" or a coin flip between none and two.  One whole-contig call
(``_native.Model.run_counts``: a sum-product recursion on the lattice expanded by a saturating run counter, with the set of
every label but the background) gives ``cluster_counts_``, one row per contig: ``sequence_id``, ``genes``, ``p_0 .. p_{K-1}``
= P(exactly k clusters | x), ``p_ge_K`` = P(at least K), and ``map_clusters``, the arg max over 0 .. K (the smaller on a tie; K
stands for "K or more").  ``p_0`` is the exact P(no cluster).  ``predict_count_clusters(genes, n_clusters=N)``
(``predict --exact-clusters N``, 0 <= N <= 31) is the decoding counterpart, for a user who knows how many clusters a record
holds (a MIBiG-style record holds one): the runs of the best whole-contig label path AMONG THOSE with exactly N runs of cluster
labels, which is not the free path with surplus runs deleted or merged by hand.  The command line writes ``cluster_counts.tsv``
and ``count_clusters.tsv`` (``path_clusters.tsv``'s columns); without the flags every table and every launch is what it is today.

Run as ``python -m gecco_amd.typed train --genes G.tsv --features F.tsv --clusters C.tsv -o DIR`` and
``python -m gecco_amd.typed predict --model DIR --genes G.tsv --features F.tsv -o OUT``.
"""
import argparse
import gc
import hashlib
import itertools
import json
import math
import operator
import os
import random
import sys
import warnings
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import tables

__all__ = ["BACKGROUND", "MIXED", "UNKNOWN", "MAX_CLUSTER_LABELS", "TypedClusterCRF", "cluster_labels", "fold_labels",
           "gene_labels", "label_type_names", "type_probabilities", "type_of", "typed_cluster_table", "write_alternatives",
           "write_sequences", "write_path_clusters", "write_path_genes", "write_paths", "count_columns", "write_cluster_counts",
           "build_parser", "main"]

BACKGROUND = "0"
MIXED = "Mixed"
UNKNOWN = "Unknown"
MAX_CLUSTER_LABELS = 31  # the trainer's 32 labels less the background

MODEL_FILE = "typed_model.crfsuite"
META_FILE = "typed_model.json"
LENGTH_FILE = "typed_length_model.tsv"  # the length model, if the classifier has one: a settings table, "length<TAB>score"


class _DefaultMinRun(int):
    """The default ``min_run`` of ``predict_path_clusters``: 3, and told apart from a 3 the caller wrote."""


_DEFAULT_MIN_RUN = _DefaultMinRun(3)


# ---------------------------------------------------------------------------------------------- labels
def cluster_labels(clusters: tables.ClusterTable) -> List[str]:
    """The label of every clusters-table row: its sorted type names joined with ``";"``, ``"Unknown"`` without any."""
    from .train_cli import type_names

    return [";".join(type_names(cell)) or UNKNOWN for cell in clusters.type]


def fold_labels(counts: Dict[str, int], limit: int = MAX_CLUSTER_LABELS) -> Dict[str, str]:
    """``counts``: clusters per cluster label.  Returns label -> label after folding: while more than ``limit`` labels
    remain, the composite label with the fewest clusters (ties by name) becomes ``"Mixed"``.  Warns with what was folded;
    a set that still does not fit raises ``ValueError``."""
    names = set(counts)
    folded: List[str] = []

    def remaining() -> int:
        return len(names) - len(folded) + (1 if folded and MIXED not in names else 0)

    for label in sorted((lab for lab in names if ";" in lab), key=lambda lab: (counts[lab], lab)):
        if remaining() <= limit:
            break
        folded.append(label)
    if remaining() > limit:
        raise ValueError(f"{remaining()} cluster labels do not fit the trainer's {limit} (after folding {len(folded)} "
                         f"composite labels into {MIXED!r})")
    if folded:
        warnings.warn(f"more than {limit} cluster labels: folded into {MIXED!r}: " + ", ".join(folded), UserWarning)
    gone = set(folded)
    return {label: (MIXED if label in gone else label) for label in names}


def gene_labels(n_genes: int, clusters: tables.ClusterTable, join: Any, limit: int = MAX_CLUSTER_LABELS,
                unknown: str = "label") -> List[Any]:
    """The label of every gene from the overlap join (``train_cli.ClusterJoin``) of the genes with ``clusters``.  The
    clusters are ``train_cli.assigned_clusters``': those with at least one gene, in sorted ``cluster_id`` order; a row with
    an empty id labels no gene, and a repeated id is a ``ValueError``.  ``unknown="any"``: the genes of a cluster without a
    type carry the frozenset of every cluster label (after folding, which then counts the clusters with a type only) instead
    of ``"Unknown"``; a table without any cluster with a type is a ``ValueError``."""
    from .train_cli import assigned_clusters

    if unknown not in ("label", "any"):
        raise ValueError(f"unknown must be 'label' or 'any', got {unknown!r}")
    row_label = cluster_labels(clusters)
    rows = [i for _, i, _ in assigned_clusters(clusters, join)]
    counts: Dict[str, int] = {}
    for i in rows:
        if unknown == "any" and row_label[i] == UNKNOWN:
            continue
        counts[row_label[i]] = counts.get(row_label[i], 0) + 1
    folded: Dict[str, Any] = fold_labels(counts, limit)
    if unknown == "any":
        if not counts:
            raise ValueError("unknown='any' needs at least one cluster with a type: an untyped cluster's genes take the set "
                             "of the typed clusters' labels")
        folded[UNKNOWN] = frozenset(folded.values())
    labels: List[Any] = [BACKGROUND] * n_genes
    for i in rows:
        label = folded[row_label[i]]
        for g in np.asarray(join.members(i)).tolist():
            if labels[g] == BACKGROUND:
                labels[g] = label
    return labels


def balanced_class_weight(counts: Dict[str, int]) -> Dict[str, float]:
    """sklearn's ``class_weight="balanced"`` over clusters: label l weighs n / (k * count_l), n the number of clusters, k
    the number of labels present and count_l the clusters of label l."""
    n, k = sum(counts.values()), len(counts)
    return {label: n / (k * c) for label, c in counts.items()}


def sequence_weights(genes: Sequence[Any], clusters: tables.ClusterTable, join: Any, labels: Sequence[Any],
                     class_weight: Any) -> Tuple[Dict[str, float], Dict[str, float]]:
    """``(class_weight_, weight of every sequence that holds a cluster)`` for ``TypedClusterCRF(class_weight=...)``.  The
    clusters are ``gene_labels``' (``train_cli.assigned_clusters``), a cluster's label is the one ``labels`` (that
    function's result) gives its first gene; a cluster whose genes carry a set of labels (``unknown="any"``) has no label
    and weighs 1.  ``class_weight``: ``"balanced"`` (``balanced_class_weight`` over the clusters with a label) or a mapping
    ``{label: weight}`` of finite weights >= 0 (a label it does not name weighs 1).  A sequence's weight is the mean of the
    weights of the clusters on it, keyed by its source id; a sequence without a cluster is not listed and weighs 1."""
    from .train_cli import assigned_clusters

    on_sequence: Dict[str, List[Any]] = {}
    counts: Dict[str, int] = {}
    for _, i, _ in assigned_clusters(clusters, join):
        members = np.asarray(join.members(i)).tolist()
        label = labels[members[0]]
        on_sequence.setdefault(genes[members[0]].source.id, []).append(label)
        if isinstance(label, str) and label != BACKGROUND:
            counts[label] = counts.get(label, 0) + 1
    if class_weight == "balanced":
        weights = balanced_class_weight(counts)
    elif isinstance(class_weight, dict):
        weights = {label: float(class_weight.get(label, 1.0)) for label in counts}
        for label, w in class_weight.items():
            if not (float(w) >= 0 and np.isfinite(float(w))):
                raise ValueError(f"class_weight[{label!r}] is {w}: weights are finite and not negative")
    else:
        raise ValueError(f"class_weight is None, 'balanced' or a mapping {{label: weight}}, got {class_weight!r}")
    return weights, {sid: float(np.mean([weights.get(lab, 1.0) if isinstance(lab, str) else 1.0 for lab in labs]))
                     for sid, labs in on_sequence.items()}


def known_masks(n_genes: int, known: tables.ClusterTable, join: Any, classes: Sequence[str],
                background: str = BACKGROUND) -> np.ndarray:
    """The allowed-label mask of every gene (one uint32, bit k: ``classes[k]``) from what is known about some regions: the
    overlap join (``train_cli.ClusterJoin``) of the sorted genes with the ``known`` table, as ``gene_labels`` reads it.  A gene
    that overlaps a row may not take the background label: where the row's label (``cluster_labels``) is one of ``classes``
    that label alone is allowed, otherwise every label but the background.  A gene under several rows takes the first in
    ``train_cli.assigned_clusters`` order.  Every other gene allows every label."""
    from .train_cli import assigned_clusters

    classes = list(classes)
    if background not in classes:
        raise ValueError(f"the model has no background label {background!r} (labels: {classes})")
    every = (1 << len(classes)) - 1
    no_background = every & ~(1 << classes.index(background))
    if no_background == 0:
        raise ValueError("the model has no label but the background: nothing is left for a known region")
    row_label = cluster_labels(known)
    masks = [every] * n_genes
    taken = [False] * n_genes
    for _, i, _ in assigned_clusters(known, join):
        label = row_label[i]
        mask = 1 << classes.index(label) if label in classes and label != background else no_background
        for g in np.asarray(join.members(i)).tolist():
            if not taken[g]:
                taken[g] = True
                masks[g] = mask
    return np.array(masks, dtype=np.uint32)


def label_type_names(label: str) -> Tuple[str, ...]:
    """The type names a label contains: none for the background, ``"Mixed"`` and ``"Unknown"``."""
    if label in (BACKGROUND, MIXED, UNKNOWN):
        return ()
    return tuple(label.split(";"))


# ---------------------------------------------------------------------------------------------- types of a call
def type_probabilities(p_all: np.ndarray, label_types: Sequence[Sequence[str]], types: Sequence[str]) -> Dict[str, float]:
    """``p_all`` [genes of one cluster, L] -> the cluster's probability of every type (module docstring)."""
    from . import _native

    p_all = np.asarray(p_all, dtype=np.float64)
    out: Dict[str, float] = {}
    for t in types:
        v = np.zeros(p_all.shape[0], dtype=np.float64)
        for l, names in enumerate(label_types):
            if t in names:
                v = v + p_all[:, l]
        out[t] = min(1.0, _native.exact_mean(v))
    return out


def type_of(probabilities: Dict[str, float]) -> frozenset:
    """The types with a probability above 0.5."""
    return frozenset(t for t, p in probabilities.items() if p > 0.5)


def typed_cluster_table(clusters: Sequence[Any], types: Sequence[str]) -> tables.ClusterTable:
    """``ClusterTable.from_clusters`` with one ``{type.lower()}_probability`` column per type between ``type`` and
    ``proteins``, in ``types.probability_columns`` order; behind them ``region_p`` and one ``{type.lower()}_region_p`` per type
    when clusters carry region posteriors (NaN for a cluster of the list that does not); behind those ``anchor_p``, ``exact_p``,
    ``start_lo``, ``start_hi``, ``end_lo`` and ``end_hi`` when clusters carry boundary intervals (``boundary_samples > 0``; a
    cluster of the list that does not: NaN, and its own start and end); last ``start_p`` and ``end_p`` when clusters carry
    boundary posteriors (``boundary_posteriors=True``), then ``run_anchor_p``, ``run_p``, ``run_start_lo``, ``run_start_hi``,
    ``run_end_lo``, ``run_end_hi``, ``run_start_beyond_p`` and ``run_end_beyond_p`` when clusters carry run posteriors
    (``run_posteriors=True``), then ``margin_present``, ``margin_absent`` and ``margin_broken`` when clusters carry margins
    (``margins=True``)."""
    table = tables.ClusterTable.from_clusters(clusters)
    extra = []
    for name in sorted(types, key=str.casefold):
        col = f"{name.lower()}_probability"
        table.columns[col] = [float(c.type_probabilities.get(name, float("nan"))) for c in clusters]
        extra.append((col, float, None))
    # region posteriors, behind the per-gene type columns: only when clusters carry them (``region_posteriors=True``)
    if any(hasattr(c, "region_probability") for c in clusters):
        nan = float("nan")
        table.columns["region_p"] = [float(getattr(c, "region_probability", nan)) for c in clusters]
        extra.append(("region_p", float, None))
        for name in sorted(types, key=str.casefold):
            col = f"{name.lower()}_region_p"
            table.columns[col] = [float(getattr(c, "region_type_probabilities", {}).get(name, nan)) for c in clusters]
            extra.append((col, float, None))
    # boundary intervals from sampled paths, behind the region columns: only when clusters carry them (``boundary_samples > 0``)
    if any(hasattr(c, "anchor_probability") for c in clusters):
        nan = float("nan")
        table.columns["anchor_p"] = [float(getattr(c, "anchor_probability", nan)) for c in clusters]
        table.columns["exact_p"] = [float(getattr(c, "exact_probability", nan)) for c in clusters]
        extra += [("anchor_p", float, None), ("exact_p", float, None)]
        for col, attribute, k, own in (("start_lo", "start_interval", 0, "start"), ("start_hi", "start_interval", 1, "start"),
                                       ("end_lo", "end_interval", 0, "end"), ("end_hi", "end_interval", 1, "end")):
            table.columns[col] = [int(getattr(c, attribute)[k]) if hasattr(c, attribute) else int(getattr(c, own)) for c in clusters]
            extra.append((col, int, None))
    # boundary posteriors, behind every other optional column: only when clusters carry them (``boundary_posteriors=True``)
    if any(hasattr(c, "start_probability") for c in clusters):
        nan = float("nan")
        table.columns["start_p"] = [float(getattr(c, "start_probability", nan)) for c in clusters]
        table.columns["end_p"] = [float(getattr(c, "end_probability", nan)) for c in clusters]
        extra += [("start_p", float, None), ("end_p", float, None)]
    # run posteriors, behind every other optional column: only when clusters carry them (``run_posteriors=True``)
    if any(hasattr(c, "run_anchor_probability") for c in clusters):
        nan = float("nan")
        table.columns["run_anchor_p"] = [float(getattr(c, "run_anchor_probability", nan)) for c in clusters]
        table.columns["run_p"] = [float(getattr(c, "run_probability", nan)) for c in clusters]
        extra += [("run_anchor_p", float, None), ("run_p", float, None)]
        for col, attribute, k, own in (("run_start_lo", "run_start_interval", 0, "start"), ("run_start_hi", "run_start_interval", 1, "start"),
                                       ("run_end_lo", "run_end_interval", 0, "end"), ("run_end_hi", "run_end_interval", 1, "end")):
            table.columns[col] = [int(getattr(c, attribute)[k]) if hasattr(c, attribute) else int(getattr(c, own)) for c in clusters]
            extra.append((col, int, None))
        table.columns["run_start_beyond_p"] = [float(getattr(c, "run_start_beyond_probability", nan)) for c in clusters]
        table.columns["run_end_beyond_p"] = [float(getattr(c, "run_end_beyond_probability", nan)) for c in clusters]
        extra += [("run_start_beyond_p", float, None), ("run_end_beyond_p", float, None)]
    # best-path score margins, behind every other optional column: only when clusters carry them (``margins=True``)
    if any(hasattr(c, "margin_present") for c in clusters):
        nan = float("nan")
        for col in ("margin_present", "margin_absent", "margin_broken"):
            table.columns[col] = [float(getattr(c, col, nan)) for c in clusters]
            extra.append((col, float, None))
    at = [n for n, _, _ in tables.ClusterTable.COLUMNS].index("type") + 1
    table.COLUMNS = tables.ClusterTable.COLUMNS[:at] + extra + tables.ClusterTable.COLUMNS[at:]
    return table


def run_interval_offsets(p: np.ndarray, beyond: float, side: str) -> Tuple[int, int]:
    """The interval rule of the run posteriors (module docstring) on one conditional distribution: ``p[r]`` the probability
    that the run starts ``r`` genes before the anchor (``side="start"``) or ends ``r`` genes after it (``"end"``), ``beyond`` the
    mass beyond the reach ``len(p) - 1``.  Positions are taken in ascending coordinate order -- for starts the mass beyond the
    reach first, then r = reach .. 0; for ends r = 0 .. reach, then the mass beyond -- and the bounds are the first positions
    whose cumulative mass is >= 0.05 and >= 0.95, as offsets r; a bound inside the mass beyond the reach is the reach.  (Should
    rounding keep the total below 0.95, the upper bound is the last position with mass.)"""
    reach = len(p) - 1
    if side == "start":
        mass = np.concatenate([[beyond], p[::-1]])
        offset = [reach] + list(range(reach, -1, -1))
    else:
        mass = np.concatenate([p, [beyond]])
        offset = list(range(reach + 1)) + [reach]
    cum = np.cumsum(mass)
    with_mass = np.flatnonzero(mass > 0.0)
    last = int(with_mass[-1]) if len(with_mass) else 0
    pick = lambda level: offset[int(np.argmax(cum >= level))] if cum[-1] >= level else offset[last]
    return pick(0.05), pick(0.95)


# ---------------------------------------------------------------------------------------------- the model
class TypedClusterCRF:
    """``TypedClusterCRF(window_size=5, window_step=1, device=0, unknown="label", **options)``; ``options`` are the
    trainer's (``train.trainer_params``: ``c1``, ``c2``, ``label_costs``, ...); ``class_weight``: None, ``"balanced"`` or
    ``{label: weight}``: every training sequence then weighs the mean of the label weights of the clusters on it
    (``sequence_weights``; the weights used are kept as ``class_weight_``); ``miss_cost`` / ``false_cost``: the training cost
    of predicting the background on a gene of any cluster label / a cluster label on a background gene, added to the options'
    ``label_costs`` for the pairs they do not name; ``unknown``: how ``fit`` labels the genes of a cluster without
    a type, ``"label"`` (the label ``"Unknown"``) or ``"any"`` (the set of every cluster label: module docstring).  After ``fit`` or ``trained``: ``classes_`` (labels in id order),
    ``label_types_`` (per label its type names), ``types_`` (the sorted distinct type names), ``background`` (``"0"``)."""

    feature_type = "protein"

    def __init__(self, window_size: int = 5, window_step: int = 1, device: int = 0, unknown: str = "label",
                 class_weight: Any = None, miss_cost: float = 0.0, false_cost: float = 0.0, **options: Any) -> None:
        if options.pop("feature_type", "protein") != "protein":
            raise ValueError("typed models use protein features")
        if unknown not in ("label", "any"):
            raise ValueError(f"unknown must be 'label' or 'any', got {unknown!r}")
        self.unknown = unknown
        if not (class_weight is None or class_weight == "balanced" or isinstance(class_weight, dict)):
            raise ValueError(f"class_weight is None, 'balanced' or a mapping {{label: weight}}, got {class_weight!r}")
        self.class_weight = class_weight
        for name, cost in (("miss_cost", miss_cost), ("false_cost", false_cost)):
            if not (float(cost) >= 0 and math.isfinite(float(cost))):
                raise ValueError(f"{name} is {cost}: costs are finite and not negative")
        self.miss_cost, self.false_cost = float(miss_cost), float(false_cost)
        self.class_weight_: Optional[Dict[str, float]] = None
        if window_size <= 0:
            raise ValueError("Window size must be strictly positive")
        if window_step <= 0 or window_step > window_size:
            raise ValueError("Window step must be strictly positive and under `window_size`")
        self.window_size, self.window_step, self.device = int(window_size), int(window_step), int(device)
        self._options = dict(options)
        self.background = BACKGROUND
        self.significance: Optional[Dict[str, float]] = None
        self.significant_features = None
        self.training_result_ = None
        self.length_scores_: Optional[np.ndarray] = None  # (fit_length_model, or the model directory)
        self.length_tail_: Optional[float] = None
        self._blob: Optional[bytes] = None
        self._model = None

    # ---- training
    def fit(self, genes: Iterable[Any], clusters: tables.ClusterTable, *, shuffle: bool = True, select: Optional[float] = None,
            correction_method: Optional[str] = None) -> "TypedClusterCRF":
        """Label ``genes`` from the ``clusters`` table and fit.  Gene ordering, feature extraction, the warnings and the
        errors are ``ClusterCRF``'s (``training_instances``), and so is the Fisher selection with ``select``, which sees a
        gene inside any cluster as positive."""
        from . import train
        from .crf import ClusterCRF
        from .train_cli import join_clusters

        genes = sorted(genes, key=operator.attrgetter("source.id", "start"))
        join = join_clusters(genes, clusters, device=self.device)
        labels = gene_labels(len(genes), clusters, join, unknown=self.unknown)
        if BACKGROUND not in labels:
            raise ValueError("no gene outside every cluster: the background label '0' must be present")
        helper = ClusterCRF("protein", "lbfgs", self.window_size, self.window_step, **self._options)
        helper.devices = [self.device]
        binary = [gene.with_probability(0.0 if label == BACKGROUND else 1.0) for gene, label in zip(genes, labels)]
        self.significance = self.significant_features = None
        if select is not None:
            binary, self.significance, self.significant_features = helper._select_features(binary, select, correction_method)
        # the instances are the helper's, in its order of sequences; features and labels are then shuffled together, by the
        # one ``random.shuffle`` over the sequences that ``training_instances`` itself would make
        feats, binary_labels = helper.training_instances(binary, shuffle=False)
        order = [[i for i, _ in group] for _, group in
                 itertools.groupby(enumerate(binary), key=lambda ig: ig[1].source.id)]
        typed = [[labels[i] for i in seq] for seq in order]
        seq_weight = None
        if self.class_weight is not None:  # (a sequence weighs the mean of its clusters' label weights, 1 without a cluster)
            self.class_weight_, by_source = sequence_weights(genes, clusters, join, labels, self.class_weight)
            seq_weight = [by_source.get(binary[seq[0]].source.id, 1.0) for seq in order]
        if [[lab != BACKGROUND for lab in seq] for seq in typed] != [[lab == "1" for lab in seq] for seq in binary_labels]:
            raise ValueError("different features and labels found, something is wrong")
        if shuffle:
            pairs = list(zip(feats, typed, seq_weight or [1.0] * len(feats)))
            random.shuffle(pairs)
            feats, typed = [f for f, _, _ in pairs], [t for _, t, _ in pairs]
            seq_weight = [w for _, _, w in pairs] if seq_weight is not None else None
        options = dict(self._options)
        if self.miss_cost or self.false_cost:  # (on top of the options' label_costs: every cluster label against the background)
            costs = dict(options.get("label_costs") or {})
            for label in dict.fromkeys(lab for seq in typed for lab in seq if isinstance(lab, str) and lab != BACKGROUND):
                costs.setdefault((label, BACKGROUND), self.miss_cost)
                costs.setdefault((BACKGROUND, label), self.false_cost)
            options["label_costs"] = costs
        params = train.trainer_params(options)
        ts = train.build_training_set(feats, typed, self.window_size, self.window_step, min_freq=float(params["min_freq"]),
                                      all_possible_states=bool(params["all_possible_states"]),
                                      all_possible_transitions=bool(params["all_possible_transitions"]),
                                      max_labels=train.MAX_LABELS, sample_weight=seq_weight)
        self.training_result_ = train.fit_training_set(ts, params, device=self.device)
        self._set_blob(train.model_blob(ts, self.training_result_.x))
        return self

    def _set_blob(self, blob: bytes, types_by_label: Optional[Dict[str, Sequence[str]]] = None) -> None:
        from . import _native

        self._blob = bytes(blob)
        self._model = m = _native.Model.from_lcrf(self._blob)
        self.classes_: List[str] = m.labels()
        if self.background not in self.classes_:
            raise ValueError(f"the model has no background label {self.background!r} (labels: {self.classes_})")
        if types_by_label is not None and set(types_by_label) != set(self.classes_):
            raise ValueError("the labels of typed_model.json are not the model's")
        self.label_types_: List[Tuple[str, ...]] = [
            tuple(types_by_label[label]) if types_by_label is not None else label_type_names(label) for label in self.classes_]
        self.types_: List[str] = sorted({t for names in self.label_types_ for t in names})
        self._attr_index = {a: i for i, a in enumerate(m.attrs())}

    def _fitted(self):
        if self._model is None:
            raise ValueError("this TypedClusterCRF is not fitted: call fit or trained first")
        return self._model

    # ---- the model directory
    def save(self, model_dir) -> None:
        """``typed_model.crfsuite`` (the CRFsuite model file) and ``typed_model.json`` (window, step, feature type,
        background label, every label's type names, the md5 of the model file)."""
        self._fitted()
        os.makedirs(model_dir, exist_ok=True)
        with open(os.path.join(model_dir, MODEL_FILE), "wb") as fh:
            fh.write(self._blob)
        meta = {"window_size": self.window_size, "window_step": self.window_step, "feature_type": self.feature_type,
                "background": self.background,
                "labels": [{"name": label, "types": list(names)} for label, names in zip(self.classes_, self.label_types_)],
                "md5": hashlib.md5(self._blob).hexdigest()}
        with open(os.path.join(model_dir, META_FILE), "w") as fh:
            json.dump(meta, fh, indent=1)
            fh.write("\n")
        length_file = os.path.join(model_dir, LENGTH_FILE)
        if self.length_scores_ is None:
            if os.path.exists(length_file):  # (a directory written before by a classifier that had one)
                os.remove(length_file)
            return
        with open(length_file, "w") as fh:  # floats with repr: they load as the same bits
            fh.write("length\tscore\n")
            for d, value in enumerate(np.asarray(self.length_scores_, dtype=np.float64).tolist(), 1):
                fh.write(f"{d}\t{value!r}\n")
            fh.write(f"tail\t{float(self.length_tail_)!r}\n")

    @classmethod
    def trained(cls, model_dir, device: int = 0) -> "TypedClusterCRF":
        """Load a directory written by ``save``; a model file whose md5 is not the recorded one is a ``ValueError``."""
        with open(os.path.join(model_dir, META_FILE)) as fh:
            meta = json.load(fh)
        with open(os.path.join(model_dir, MODEL_FILE), "rb") as fh:
            blob = fh.read()
        if hashlib.md5(blob).hexdigest() != meta["md5"]:
            raise ValueError("MD5 hash of model data does not match signature")
        if meta.get("feature_type", "protein") != "protein":
            raise ValueError("typed models use protein features")
        self = cls(int(meta["window_size"]), int(meta["window_step"]), device)
        self.background = str(meta["background"])
        self._set_blob(blob, {entry["name"]: tuple(entry["types"]) for entry in meta["labels"]})
        length_file = os.path.join(model_dir, LENGTH_FILE)
        if os.path.exists(length_file):  # (a directory without the table has no length model)
            with open(length_file) as fh:
                rows = [line.rstrip("\n").split("\t") for line in fh if line.strip()]
            if rows[:1] != [["length", "score"]] or len(rows) < 3 or rows[-1][0] != "tail" or \
                    [r[0] for r in rows[1:-1]] != [str(d) for d in range(1, len(rows) - 1)]:
                raise ValueError(f"{LENGTH_FILE}: expected the columns length, score, the rows 1 .. M and a row 'tail'")
            self.length_scores_ = np.array([float(r[1]) for r in rows[1:-1]], dtype=np.float64)
            self.length_tail_ = float(rows[-1][1])
        return self

    # ---- prediction
    def _score(self, genes: Iterable[Any], pad: bool, known: Optional[tables.ClusterTable] = None):
        """Genes sorted as ``ClusterCRF.predict_probabilities`` sorts them, their contigs, which contigs are scored, and
        the device pass: ``p_all`` [n, L] and ``p_any`` [n] (NaN on unscored contigs), and last the allowed-label masks made
        from ``known`` (None without).  ``known``: a clusters table of
        regions known beforehand (``known_masks``): every window then runs on the lattice in which a gene of a known region
        cannot be background, and can only take the region's label where the model has it."""
        from . import packing

        model = self._fitted()
        genes = sorted(genes, key=operator.attrgetter("source.id", "start"))
        for gene in genes:
            gene.protein.domains.sort(key=operator.attrgetter("start"))
        contigs = [list(g) for _, g in itertools.groupby(genes, key=operator.attrgetter("source.id"))]
        batch = packing.pack_contigs(contigs, self._attr_index, "protein")
        W = self.window_size
        scored = np.ones(len(contigs), dtype=bool)
        for ci in np.flatnonzero(np.diff(batch.item_ptr) < W).tolist():
            contig = contigs[ci]
            if pad:
                unit = "protein" if W - len(contig) == 1 else "proteins"
                warnings.warn(f"Contig {contig[0].source.id!r} does not contain enough proteins ({len(contig)}) for sliding "
                              f"window of size {W}, padding with {W - len(contig)} {unit}")
            else:
                warnings.warn(f"Contig {contig[0].source.id!r} does not contain enough proteins ({len(contig)}) for sliding "
                              f"window of size {W}")
                scored[ci] = False
        L = len(self.classes_)
        if not genes:
            return genes, contigs, scored, batch, np.zeros((0, L)), np.zeros(0), None
        allowed = None
        if known is not None:
            from .train_cli import join_clusters

            allowed = known_masks(len(genes), known, join_clusters(genes, known, device=self.device), self.classes_, self.background)
        p_all, p_any = model.windowed_marginals_all(batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32),
                                                    batch.attr_id, W, self.window_step,
                                                    background=self.classes_.index(self.background), pad=pad, device=self.device,
                                                    allowed=allowed)
        return genes, contigs, scored, batch, p_all, p_any, allowed

    def _annotated(self, contigs, scored, batch, p_any) -> List[Any]:
        """New genes carrying ``p_any``, through ``ClusterCRF``'s annotate path (no label ``'1'``: no cluster weights);
        the genes of unscored contigs keep their probabilities."""
        from .crf import _annotate, _annotate_all

        out: List[Any] = []
        gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            for ci, contig in enumerate(contigs):
                if not scored[ci]:
                    out.extend(_annotate(gene, None, None, {}) for gene in contig)
                    continue
                i0 = int(batch.item_ptr[ci])
                probs = p_any[i0:i0 + len(contig)].tolist()
                fast = _annotate_all(contig, probs, {})
                out.extend(fast if fast is not None else [_annotate(gene, p, None, {}) for gene, p in zip(contig, probs)])
        finally:
            if gc_was_enabled:
                gc.enable()
        return out

    def predict_probabilities(self, genes: Iterable[Any], *, pad: bool = True,
                              known: Optional[tables.ClusterTable] = None) -> List[Any]:
        """New genes, sorted by (sequence, start), carrying as their probability the windowed probability of lying in any
        cluster: ``ClusterRefiner`` and the table writers work on them unchanged.  ``known`` (here and in the other
        prediction methods): a clusters table of regions known beforehand, whose genes cannot be background (``_score``)."""
        _, contigs, scored, batch, _, p_any, _ = self._score(genes, pad, known)
        return self._annotated(contigs, scored, batch, p_any)

    def predict_label_probabilities(self, genes: Iterable[Any], *, pad: bool = True,
                                    known: Optional[tables.ClusterTable] = None) -> np.ndarray:
        """Every label's windowed probability, ``[n, L]`` in the gene order ``predict_probabilities`` returns, columns in
        ``classes_`` order."""
        return self._score(genes, pad, known)[4]

    def predict_clusters(self, genes: Iterable[Any], *, threshold: float = 0.8, n_cds: int = 3, edge_distance: int = 0,
                         trim: bool = True, pad: bool = True, known: Optional[tables.ClusterTable] = None,
                         region_posteriors: bool = False, boundary_samples: int = 0, seed: int = 0, alternatives: int = 0,
                         alternatives_margin: int = 10, boundary_posteriors: bool = False, run_posteriors: bool = False,
                         run_reach: int = 256, attributions: bool = False, attribution_reach: int = 10,
                         margins: bool = False) -> List[Any]:
        """Clusters by the refiner's ``gecco`` criterion on the any-cluster probability (the segment kernel, one grouper
        per contig as the CLI runs it), each with ``type`` and ``type_probabilities`` from the labels' probabilities, with
        ``region_posteriors`` each with ``region_probability`` and ``region_type_probabilities``, and with
        ``boundary_samples > 0`` each with ``anchor_probability``, ``exact_probability``, ``start_interval`` and
        ``end_interval``, and with ``alternatives = K > 0`` each with ``alternatives``, the K best readings of its
        neighbourhood with their exact conditional probabilities, and with ``boundary_posteriors`` each with
        ``start_probability`` and ``end_probability``, and with ``run_posteriors`` each with ``run_anchor_probability``,
        ``run_probability``, ``run_start_interval``, ``run_end_interval``, ``run_start_beyond_probability``,
        ``run_end_beyond_probability`` and ``run_boundaries``, exact over ``run_reach`` genes to either side of the anchor
        (module docstring), and with ``attributions`` each with ``attributions``: for every gene of the call and of
        ``attribution_reach`` genes on either side a dict with its ``protein_id``, its ``offset`` (0 = the cluster's first gene,
        negative before it), its ``contribution`` -- log P(every gene of the call lies in a cluster | x) minus the same without
        anything the gene carries, exact, positive where the call leans on the gene -- and ``domains``, the ``(name,
        contribution)`` of each of its domains the model knows; the cluster's ``attribution_log_probability`` is the
        log-probability they are differences of, and with ``margins`` each with ``margin_present``, ``margin_absent``,
        ``margin_broken`` and ``type_margins`` (``_margins``): differences of best-path scores on the whole-contig lattice, not
        posteriors."""
        return self.predict_genes_and_clusters(genes, threshold=threshold, n_cds=n_cds, edge_distance=edge_distance, trim=trim,
                                               pad=pad, known=known, region_posteriors=region_posteriors,
                                               boundary_samples=boundary_samples, seed=seed, alternatives=alternatives,
                                               alternatives_margin=alternatives_margin,
                                               boundary_posteriors=boundary_posteriors, run_posteriors=run_posteriors,
                                               run_reach=run_reach, attributions=attributions,
                                               attribution_reach=attribution_reach, margins=margins)[1]

    def _margins(self, batch, allowed, rows: np.ndarray, item_ptr: np.ndarray, not_background: int, clusters: List[Any]) -> None:
        """The margins of every called cluster (``rows``: the segment kernel's (contig, number, first gene, last gene + 1)),
        from ONE native call over the batch (``_native.Model.max_marginals``): per cluster one span with the set of every label
        but the background, one with the background alone, and one per type with the labels whose names contain it.  With
        ``best`` the score of the contig's Viterbi path (read off the max-marginals at the call's last gene: the same number up
        to a few ulps, in the summation order a span's score ends in, so that an exact 0.0 is an exact 0.0):
        ``margin_present`` = best - (the best path that gives every gene of the call a cluster label): 0.0 when the Viterbi path
        keeps the whole call inside a cluster;
        ``margin_absent`` = best - (the best path that gives every gene of the call the background): the score the best reading
        loses when the call is removed altogether;
        ``margin_broken`` = best - (the best path that gives at least one gene of the call the background);
        ``type_margins`` = {type: best - (the best path that gives every gene of the call a label of that type)}.
        Each is a difference of two path scores, that is, the log of the ratio of the probabilities of two single label paths
        (``inf`` where no path qualifies) -- not a posterior: ``region_posteriors`` sums over all paths, a margin compares the
        two best.  The paths are those of the whole-contig lattice (``predict_path_clusters``'s), not of the windowed one the
        calls themselves come from, so a call the windowed marginals make may have a positive ``margin_present``."""
        type_masks = [sum(1 << l for l, names in enumerate(self.label_types_) if t in names) for t in self.types_]
        full = (1 << len(self.classes_)) - 1
        sets = [not_background, full & ~not_background] + type_masks
        contig = np.repeat(rows[:, 0], len(sets)).astype(np.int32)
        begin = np.repeat(rows[:, 2] - item_ptr[rows[:, 0]], len(sets)).astype(np.int32)
        end = np.repeat(rows[:, 3] - item_ptr[rows[:, 0]], len(sets)).astype(np.int32)
        mask = np.tile(np.array(sets, dtype=np.uint32), len(rows))
        got = self._fitted().max_marginals(item_ptr, batch.attr_ptr.astype(np.int32), batch.attr_id, spans=(contig, begin, end, mask),
                                           device=self.device, allowed=allowed)
        # ``best`` as the forward and backward vectors give it at the call's last gene: the contig's best score up to a few ulps
        # (a max-marginal is a sum in another order than the Viterbi score), and the very sum a span's score ends in -- so a call
        # the Viterbi path contains gets exactly 0.0, not a rounding residue of either sign
        best = np.repeat(got["through"][rows[:, 3] - 1].max(axis=1), len(sets)).reshape(len(rows), len(sets))
        inside = best - got["span_best"].reshape(len(rows), len(sets))
        broken = best - got["span_broken"].reshape(len(rows), len(sets))
        for cluster, row, brk in zip(clusters, inside.tolist(), broken[:, 0].tolist()):
            cluster.margin_present, cluster.margin_absent, cluster.margin_broken = row[0], row[1], brk
            cluster.type_margins = dict(zip(self.types_, row[2:]))

    def _region_posteriors(self, batch, allowed, rows: np.ndarray, item_ptr: np.ndarray, not_background: int,
                           clusters: List[Any]) -> None:
        """``region_probability`` and ``region_type_probabilities`` of every called cluster (``rows``: the segment kernel's
        (contig, number, first gene, last gene + 1)), from ONE native call over the batch: per cluster one span with the set of
        every label but the background, and one per type with the labels whose names contain it."""
        type_masks = [sum(1 << l for l, names in enumerate(self.label_types_) if t in names) for t in self.types_]
        sets = [not_background] + type_masks
        contig = np.repeat(rows[:, 0], len(sets)).astype(np.int32)
        begin = np.repeat(rows[:, 2] - item_ptr[rows[:, 0]], len(sets)).astype(np.int32)
        end = np.repeat(rows[:, 3] - item_ptr[rows[:, 0]], len(sets)).astype(np.int32)
        mask = np.tile(np.array(sets, dtype=np.uint32), len(rows))
        logp = self._fitted().span_log_probabilities(item_ptr, batch.attr_ptr.astype(np.int32), batch.attr_id, contig, begin, end,
                                                     mask, device=self.device, allowed=allowed)
        p = np.exp(logp).reshape(len(rows), len(sets))
        for cluster, row in zip(clusters, p.tolist()):
            cluster.region_probability = row[0]
            cluster.region_type_probabilities = dict(zip(self.types_, row[1:]))

    def _attributions(self, batch, allowed, rows: np.ndarray, item_ptr: np.ndarray, not_background: int, clusters: List[Any],
                      annotated: List[Any], reach: int) -> None:
        """``attributions`` and ``attribution_log_probability`` of every called cluster (``rows``: the segment kernel's (contig,
        number, first gene, last gene + 1)), from ONE native call over the batch: per cluster one query with the set of every
        label but the background; the call's rows are the cluster's genes and ``reach`` genes on either side."""
        base = item_ptr[rows[:, 0]].astype(np.int64)
        attr_ptr = batch.attr_ptr.astype(np.int32)
        out = self._fitted().span_conditionals(item_ptr, attr_ptr, batch.attr_id, rows[:, 0].astype(np.int32),
                                               (rows[:, 2] - base).astype(np.int32), (rows[:, 3] - base).astype(np.int32),
                                               np.full(len(rows), not_background, dtype=np.uint32), reach=reach, device=self.device,
                                               allowed=allowed)
        names = self._fitted().attrs()
        row_ptr, occ_ptr, item, attr = out["row_ptr"].tolist(), out["occ_ptr"].tolist(), out["item"].tolist(), out["attr"].tolist()
        for q, (cluster, (_, _, first, _), g0) in enumerate(zip(clusters, rows.tolist(), base.tolist())):
            cluster.attribution_log_probability = float(out["logp"][q])
            cluster.attributions = []
            gene0 = g0 + int(out["first"][q])  # (the gene of the query's first row)
            for r in range(row_ptr[q], row_ptr[q + 1]):
                g = gene0 + r - row_ptr[q]
                k0 = int(attr_ptr[g])
                cluster.attributions.append({
                    "protein_id": annotated[g].protein.id, "offset": g - first, "contribution": item[r],
                    "domains": [(names[int(batch.attr_id[k0 + i])], attr[occ_ptr[r] + i]) for i in range(occ_ptr[r + 1] - occ_ptr[r])]})

    def _boundary_intervals(self, batch, allowed, rows: np.ndarray, item_ptr: np.ndarray, not_background: int, clusters: List[Any],
                            annotated: List[Any], p_any: np.ndarray, n_samples: int, seed: int) -> None:
        """``anchor_probability``, ``exact_probability``, ``start_interval`` and ``end_interval`` of every called cluster
        (``rows``: the segment kernel's (contig, number, first gene, last gene + 1)), from ONE native call over the batch:
        ``n_samples`` label paths per contig drawn from the whole-contig posterior, and per cluster one run query -- the run of
        genes outside the background around the cluster's gene with the greatest ``p_any`` (the first on ties)."""
        base = item_ptr[rows[:, 0]].astype(np.int64)
        anchor = np.array([first + int(np.argmax(p_any[first:last])) for first, last in rows[:, 2:4].tolist()], dtype=np.int64)
        runs = self._fitted().sample_paths(item_ptr, batch.attr_ptr.astype(np.int32), batch.attr_id, n_samples, seed=seed,
                                           device=self.device, allowed=allowed,
                                           runs=(rows[:, 0].astype(np.int32), (anchor - base).astype(np.int32),
                                                 np.full(len(rows), not_background, dtype=np.uint32)), want_paths=False)
        for cluster, (_, _, first, last), g0, found in zip(clusters, rows.tolist(), base.tolist(), runs):
            there = found[found[:, 0] >= 0]
            m = len(there)
            cluster.anchor_probability = m / n_samples
            cluster.exact_probability = int(np.count_nonzero((there[:, 0] == first - g0) & (there[:, 1] == last - g0))) / n_samples
            if m == 0:
                cluster.start_interval = (int(cluster.start), int(cluster.start))
                cluster.end_interval = (int(cluster.end), int(cluster.end))
                continue
            starts = sorted(annotated[g0 + k].start for k in there[:, 0].tolist())
            ends = sorted(annotated[g0 + k - 1].end for k in there[:, 1].tolist())
            lo, hi = int(math.floor(0.05 * (m - 1))), int(math.ceil(0.95 * (m - 1)))
            cluster.start_interval = (int(starts[lo]), int(starts[hi]))
            cluster.end_interval = (int(ends[lo]), int(ends[hi]))

    SEQUENCE_COLUMNS = ("sequence_id", "genes", "log_z", "entropy", "expected_clusters")

    def _boundary_posteriors(self, batch, allowed, rows: np.ndarray, item_ptr: np.ndarray, not_background: int, clusters: List[Any],
                             annotated: List[Any]) -> None:
        """``start_probability`` and ``end_probability`` of every called cluster (``rows``: the segment kernel's (contig,
        number, first gene, last gene + 1)) and ``sequence_posteriors_``, from ONE native call over the batch: the probability
        that a run of labels outside the background starts / ends at every gene, every contig's log Z and path entropy."""
        out = self._fitted().edge_posteriors(item_ptr, batch.attr_ptr.astype(np.int32), batch.attr_id,
                                             sets=np.array([not_background], dtype=np.uint32), want_transitions=False,
                                             want_entropy=True, want_marginals=True, device=self.device, allowed=allowed)
        enter, leave = out["enter"][:, 0], out["leave"][:, 0]
        for cluster, (_, _, first, last) in zip(clusters, rows.tolist()):
            cluster.start_probability = float(enter[first])
            cluster.end_probability = float(leave[last - 1])
        starts = item_ptr[:-1].astype(np.int64)
        self.sequence_posteriors_ = {
            "sequence_id": [annotated[g].source.id for g in starts.tolist()],
            "genes": np.diff(item_ptr).astype(np.int64).tolist(),
            "log_z": out["lognorm"].tolist(),
            "entropy": out["entropy"].tolist(),
            "expected_clusters": [float(enter[a:b].sum()) for a, b in zip(item_ptr[:-1].tolist(), item_ptr[1:].tolist())]}

    def _run_posteriors(self, batch, allowed, rows: np.ndarray, item_ptr: np.ndarray, not_background: int, clusters: List[Any],
                        annotated: List[Any], p_any: np.ndarray, reach: int) -> None:
        """``run_anchor_probability``, ``run_probability``, ``run_start_interval``, ``run_end_interval``, the two beyond-masses
        and ``run_boundaries`` of every called cluster (``rows``: the segment kernel's (contig, number, first gene, last gene +
        1)), from ONE native call over the batch: per cluster one anchor query -- the run of genes outside the background
        through the cluster's gene with the greatest ``p_any`` (the first on ties) -- and one closed-run query over the called
        range."""
        base = item_ptr[rows[:, 0]].astype(np.int64)
        anchor = np.array([first + int(np.argmax(p_any[first:last])) for first, last in rows[:, 2:4].tolist()], dtype=np.int64)
        contig, sets = rows[:, 0].astype(np.int32), np.full(len(rows), not_background, dtype=np.uint32)
        out = self._fitted().run_posteriors(item_ptr, batch.attr_ptr.astype(np.int32), batch.attr_id,
                                            anchors=(contig, (anchor - base).astype(np.int32), sets), reach=reach,
                                            runs=(contig, (rows[:, 2] - base).astype(np.int32), (rows[:, 3] - base).astype(np.int32), sets),
                                            device=self.device, allowed=allowed)
        for q, (cluster, a) in enumerate(zip(clusters, anchor.tolist())):
            log_anchor = float(out["log_anchor"][q])
            cluster.run_anchor_probability = math.exp(log_anchor)
            cluster.run_probability = math.exp(float(out["log_run"][q]))
            cluster.run_boundaries = []
            if log_anchor == -math.inf:
                cluster.run_start_interval = (int(cluster.start), int(cluster.start))
                cluster.run_end_interval = (int(cluster.end), int(cluster.end))
                cluster.run_start_beyond_probability = cluster.run_end_beyond_probability = 0.0
                continue
            for side, step, coordinate in (("start", -1, "start"), ("end", 1, "end")):
                p = np.exp(out[f"log_{side}"][q] - log_anchor)
                beyond = math.exp(float(out[f"log_{side}_beyond"][q]) - log_anchor)
                lo, hi = run_interval_offsets(p, beyond, side)
                setattr(cluster, f"run_{side}_interval", (int(getattr(annotated[a + step * lo], coordinate)),
                                                          int(getattr(annotated[a + step * hi], coordinate))))
                setattr(cluster, f"run_{side}_beyond_probability", beyond)
                cluster.run_boundaries += [(side, annotated[a + step * r], int(getattr(annotated[a + step * r], coordinate)), float(p[r]))
                                           for r in np.flatnonzero(p > 0.0).tolist()]

    def _alternatives(self, batch, allowed, rows: np.ndarray, item_ptr: np.ndarray, clusters: List[Any], annotated: List[Any],
                      p_any: np.ndarray, k: int, margin: int) -> None:
        """``alternatives`` of every called cluster (``rows``: the segment kernel's (contig, number, first gene, last gene +
        1)): the contig's Viterbi path from one native call, then ONE ``viterbi_kbest`` call over all clusters' neighbourhoods,
        each a short sequence whose copied end genes are pinned to the Viterbi path's labels unless they are contig ends.  The
        k paths of a neighbourhood are exactly the k best whole-contig paths that agree with the Viterbi path outside it, and
        ``log_p`` is each path's log-probability given that agreement (module docstring)."""
        model = self._fitted()
        L = len(self.classes_)
        bg = self.classes_.index(self.background)
        attr_ptr = batch.attr_ptr.astype(np.int64)
        best, _ = model.viterbi(item_ptr, attr_ptr.astype(np.int32), batch.attr_id, device=self.device,
                                want_score=False, allowed=allowed)
        best = np.asarray(best, dtype=np.int64)
        every = np.uint32((1 << L) - 1)
        windows, seq_ptr, rows_ptr, ids, masks = [], [0], [0], [], []
        for contig, _, first, last in rows.tolist():
            c0, c1 = int(item_ptr[contig]), int(item_ptr[contig + 1])
            lo, hi = max(c0, first - margin - 1), min(c1, last + margin + 1)
            windows.append((c0, c1, lo, hi))
            seq_ptr.append(seq_ptr[-1] + hi - lo)
            a0, a1 = int(attr_ptr[lo]), int(attr_ptr[hi])
            ids.append(batch.attr_id[a0:a1])
            rows_ptr.extend((attr_ptr[lo + 1:hi + 1] - a0 + rows_ptr[-1]).tolist())
            m = np.full(hi - lo, every, dtype=np.uint32) if allowed is None else np.array(allowed[lo:hi], dtype=np.uint32)
            if lo > c0:
                m[0] = np.uint32(1) << np.uint32(best[lo])
            if hi < c1:
                m[-1] = np.uint32(1) << np.uint32(best[hi - 1])
            masks.append(m)
        y, score, n_paths, lognorm = model.viterbi_kbest(np.array(seq_ptr, dtype=np.int32), np.array(rows_ptr, dtype=np.int32),
                                                         np.concatenate(ids).astype(np.int32), k, device=self.device,
                                                         allowed=np.concatenate(masks))
        for q, (cluster, (_, _, first, last), (c0, c1, lo, hi)) in enumerate(zip(clusters, rows.tolist(), windows)):
            anchor = first + int(np.argmax(p_any[first:last]))
            found = []
            for r in range(int(n_paths[q])):
                path = y[seq_ptr[q]:seq_ptr[q + 1], r].astype(np.int64)
                whole = best[c0:c1].copy()
                whole[lo - c0:hi - c0] = path
                entry = {"rank": r, "window": (lo - c0, hi - c0), "labels": [self.classes_[l] for l in path.tolist()],
                         "run": None, "start": None, "end": None, "type": None, "log_p": float(score[q, r] - lognorm[q])}
                if whole[anchor - c0] != bg:
                    a = b = anchor - c0
                    while a > 0 and whole[a - 1] != bg:
                        a -= 1
                    while b + 1 < c1 - c0 and whole[b + 1] != bg:
                        b += 1
                    counts = np.bincount(whole[a:b + 1], minlength=L)
                    entry["run"] = (a, b + 1)
                    entry["start"], entry["end"] = int(annotated[c0 + a].start), int(annotated[c0 + b].end)
                    entry["type"] = ";".join(self.label_types_[int(np.argmax(counts))]) or UNKNOWN
                found.append(entry)
            cluster.alternatives = found

    PATH_COLUMNS = ("sequence_id", "genes", "log_z", "score", "log_p", "constraint_log_p", "clusters")

    PATH_GENE_COLUMNS = ("sequence_id", "protein_id", "path_label", "p")

    def fit_length_model(self, genes: Iterable[Any], clusters: tables.ClusterTable, max_length: int = 32,
                         c2: float = 1.0) -> "TypedClusterCRF":
        """Learn a score on the LENGTH of a region from labelled contigs, the CRF's weights held fixed, and keep it as
        ``length_scores_`` (``[max_length]``; entry d - 1 scores a region of min(genes, max_length) = d genes) and
        ``length_tail_`` (the score of every gene beyond the ``max_length``-th).  A region is a maximal run of genes with a
        label other than the background, as ``predict_path_clusters`` calls them; the genes are labelled from ``clusters`` as
        ``fit`` labels them.  The fit is ``SequenceCRF.fit_run_length_scores`` over the whole contigs: convex, L-BFGS from
        zeros, one whole-contig native call per evaluation, ``c2`` its L2 penalty.  ``predict_path_clusters(...,
        length_model=True)`` decodes with the result, and ``save`` writes it next to the model."""
        from .sequence import SequenceCRF
        from .train_cli import join_clusters

        model = self._fitted()
        genes = sorted(genes, key=operator.attrgetter("source.id", "start"))
        labels = gene_labels(len(genes), clusters, join_clusters(genes, clusters, device=self.device), unknown=self.unknown)
        contigs, csr, _ = self._whole_contigs(genes, None)
        if csr is None:
            raise ValueError("fit_length_model: no genes")
        item_ptr, attr_ptr, attr_id = csr
        names = model.attrs()
        X = [[[names[a] for a in attr_id[attr_ptr[i]:attr_ptr[i + 1]].tolist()] for i in range(int(item_ptr[c]), int(item_ptr[c + 1]))]
             for c in range(len(contigs))]
        y = [labels[int(item_ptr[c]):int(item_ptr[c + 1])] for c in range(len(contigs))]
        seq = SequenceCRF.from_bytes(self._blob, window_size=None, device=self.device)
        g, tau = seq.fit_run_length_scores(X, y, [c for c in self.classes_ if c != self.background], max_length, c2=c2)
        self.length_scores_, self.length_tail_ = g, tau
        self.length_fit_result_ = seq.fit_run_length_result_
        return self

    def predict_path_clusters(self, genes: Iterable[Any], *, min_run: int = _DEFAULT_MIN_RUN,
                              known: Optional[tables.ClusterTable] = None, marginals: bool = False,
                              length_model: bool = False, circular=None) -> List[Any]:
        """Clusters as the runs of the best whole-contig label path AMONG THOSE in which every maximal run of genes with a label
        other than the background has at least ``min_run`` genes (module docstring): one ``viterbi_min_run`` call over all
        contigs with the set of every label but the background.  ``min_run`` counts genes, not annotated genes (the refiner's
        ``n_cds`` counts annotated ones), 1 <= ``min_run`` <= 32.  Every cluster has the id ``{sequence}_cluster_{number}``
        (numbered from 1 along its contig), its genes (the caller's, sorted by (sequence, start); no probability is computed
        unless ``marginals`` is set),
        ``type`` from the run's most frequent label (the smaller label id on ties) and ``path_type``, its ``";"``-joined names
        (``"Unknown"`` for a label without types).  Fills ``path_posteriors_``, the
        per-contig columns ``PATH_COLUMNS``.  ``known`` restricts the lattice as in the other prediction methods.
        With ``marginals=True`` one ``marginals_min_run`` call follows the decode (the same set, the same masks, no marginals
        table: 8 bytes per gene come back): every cluster gains ``average_p`` (``numpy.mean``), ``max_p`` and ``min_p`` of
        ``inside`` = P(gene in a region | x, the constraint) over its genes, ``path_gene_probabilities_`` holds ``inside`` per
        gene in (sequence, start) order and ``path_genes_`` the columns ``PATH_GENE_COLUMNS`` (``path_label``: the gene's label
        on the path, empty where a contig has no path).  Without it neither attribute is set and no further launch runs.
        ``ValueError`` before any device call for a ``min_run`` that is not an integer or lies outside its range.
        With ``length_model=True`` the path is the best one under the length scores of ``fit_length_model`` (or of the model
        directory) instead: one ``viterbi_run_length`` call, and with ``marginals`` one ``marginals_run_length`` call, in place
        of the min-run ones; ``constraint_log_p`` is then ``log Z_g - log Z``.  ``min_run`` is ignored then, and giving both
        explicitly is a ``ValueError``, as is asking for a length model the classifier does not have.
        ``circular`` names the contigs that are RINGS -- a collection of sequence ids (a single string is one id), or True for every contig; None or an
        empty collection: every contig is a chain, and the call is the one it has always been.  On a circular contig the path
        is the ring's best path (one ``ring`` call over all of them; the last gene has a transition into the first), and a run
        that crosses the cut is ONE cluster: its genes are ``contig[a:] + contig[:b]``, ``wraps_origin`` is True and it is
        numbered by where it starts.  A ring labelled non-background throughout is one cluster of all genes in contig order
        with ``wraps_origin`` False.  Every cluster of such a call has ``wraps_origin``.  With ``marginals`` the per-gene
        ``inside`` of a ring comes from the ring's marginals; ``path_posteriors_`` gets its columns from the ring's quantities,
        and ``constraint_log_p`` is 0 there.  On a circular contig only ``min_run=1`` is defined: ``min_run`` > 1 (the default
        included) or ``length_model=True`` together with a non-empty ``circular`` is a ``ValueError`` before any device call.
        The linear contigs of the same call behave as ever."""
        rings_all = circular is True
        if isinstance(circular, (str, bytes)):  # (one sequence id, not its characters)
            circular = [circular.decode() if isinstance(circular, bytes) else circular]
        ring_ids = frozenset() if circular is None or isinstance(circular, (bool, np.bool_)) else frozenset(str(c) for c in circular)
        with_rings = rings_all or bool(ring_ids)
        if with_rings and (length_model or min_run is _DEFAULT_MIN_RUN or min_run != 1):
            raise ValueError("predict_path_clusters: on a circular contig only min_run=1 is defined: a minimum run length across the "
                             "cut needs the head run's length as a second counter (L * m**2 slots) and is left out, so min_run > 1 "
                             "(the default included) or length_model=True cannot go with a non-empty circular")
        if length_model:
            if min_run is not _DEFAULT_MIN_RUN:
                raise ValueError("predict_path_clusters: min_run and length_model=True are two ways to say how long a region is: give one")
            if getattr(self, "length_scores_", None) is None:
                raise ValueError("predict_path_clusters: this classifier has no length model: call fit_length_model first")
        try:
            min_run = operator.index(min_run)
        except TypeError:
            raise ValueError(f"min_run is an integer, got {min_run!r}") from None
        if not 1 <= min_run <= 32:
            raise ValueError(f"min_run = {min_run} is outside 1 .. 32")
        from . import packing
        from .refine import _cluster_class
        from .types import _cluster_type_factory

        model = self._fitted()
        genes = sorted(genes, key=operator.attrgetter("source.id", "start"))
        for gene in genes:
            gene.protein.domains.sort(key=operator.attrgetter("start"))
        contigs = [list(g) for _, g in itertools.groupby(genes, key=operator.attrgetter("source.id"))]
        self.path_posteriors_ = {name: [] for name in self.PATH_COLUMNS}
        if marginals:
            self.path_gene_probabilities_ = np.zeros(0)
            self.path_genes_ = {name: [] for name in self.PATH_GENE_COLUMNS}
        if not genes:
            return []
        batch = packing.pack_contigs(contigs, self._attr_index, "protein")
        allowed = None
        if known is not None:
            from .train_cli import join_clusters

            allowed = known_masks(len(genes), known, join_clusters(genes, known, device=self.device), self.classes_, self.background)
        L = len(self.classes_)
        bg = self.classes_.index(self.background)
        item_ptr = batch.item_ptr.astype(np.int32)
        inside_p = None
        is_ring = [with_rings and (rings_all or str(contig[0].source.id) in ring_ids) for contig in contigs]
        if any(is_ring):
            y, score, lognorm_c, lognorm, inside_p = self._paths_with_rings(model, contigs, is_ring, item_ptr, allowed, marginals)
        elif length_model:
            head = (item_ptr, batch.attr_ptr.astype(np.int32), batch.attr_id, ((1 << L) - 1) & ~(1 << bg), self.length_scores_,
                    self.length_tail_)
            y, score, lognorm_c, lognorm = model.viterbi_run_length(*head, device=self.device, allowed=allowed)
            if marginals:
                inside_p = model.marginals_run_length(*head, device=self.device, allowed=allowed, want_marginals=False,
                                                      want_counts=False)[1]
        else:
            y, score, lognorm_c, lognorm = model.viterbi_min_run(item_ptr, batch.attr_ptr.astype(np.int32), batch.attr_id,
                                                                 ((1 << L) - 1) & ~(1 << bg), min_run, device=self.device,
                                                                 allowed=allowed)
            if marginals:
                _, inside_p, _, _ = model.marginals_min_run(item_ptr, batch.attr_ptr.astype(np.int32), batch.attr_id,
                                                            ((1 << L) - 1) & ~(1 << bg), min_run, device=self.device, allowed=allowed,
                                                            want_marginals=False)
        if marginals:
            self.path_gene_probabilities_ = inside_p
        Cluster = _cluster_class()
        clusters: List[Any] = []
        for ci, contig in enumerate(contigs):
            c0, c1 = int(item_ptr[ci]), int(item_ptr[ci + 1])
            path = y[c0:c1].astype(np.int64)
            found = 0
            if score[ci] > -np.inf:
                inside = np.concatenate([[False], path != bg, [False]])
                edges = np.flatnonzero(inside[1:] != inside[:-1])
                runs = [np.arange(a, b) for a, b in zip(edges[::2].tolist(), edges[1::2].tolist())]
                wraps = is_ring[ci] and len(runs) >= 2 and runs[0][0] == 0 and runs[-1][-1] == c1 - c0 - 1
                if wraps:  # the run across the cut is one cluster, numbered by where it starts: after the others
                    runs = runs[1:-1] + [np.concatenate([runs[-1], runs[0]])]
                for k, members in enumerate(runs):
                    found += 1
                    cluster = Cluster(f"{contig[0].source.id}_cluster_{found}", [contig[t] for t in members.tolist()])
                    major = int(np.argmax(np.bincount(path[members], minlength=L)))
                    cluster.type = _cluster_type_factory(cluster)(self.label_types_[major])
                    cluster.path_type = ";".join(self.label_types_[major]) or UNKNOWN  # (as the alternatives name a run's type)
                    if with_rings:
                        cluster.wraps_origin = bool(wraps and k == len(runs) - 1)
                    if inside_p is not None:
                        ps = inside_p[c0 + members]
                        cluster.average_p, cluster.max_p, cluster.min_p = float(np.mean(ps)), float(ps.max()), float(ps.min())
                    clusters.append(cluster)
            if inside_p is not None:
                rows = self.path_genes_
                rows["sequence_id"].extend(g.source.id for g in contig)
                rows["protein_id"].extend(g.protein.id for g in contig)
                rows["path_label"].extend(self.classes_[k] if k >= 0 else "" for k in path.tolist())
                rows["p"].extend(inside_p[c0:c1].tolist())
            for name, value in zip(self.PATH_COLUMNS, (contig[0].source.id, c1 - c0, float(lognorm[ci]), float(score[ci]),
                                                       float(score[ci] - lognorm[ci]), float(lognorm_c[ci] - lognorm[ci]), found)):
                self.path_posteriors_[name].append(value)
        return clusters

    def _paths_with_rings(self, model, contigs, is_ring, item_ptr: np.ndarray, allowed, marginals: bool):
        """``predict_path_clusters``'s ``(y, score, lognorm_c, lognorm, inside_p)`` at ``min_run = 1`` for a batch with circular
        contigs: the linear contigs through the calls they always take, in one batch of their own, the circular ones through
        one ``ring`` call -- there log Z of the ring stands for both ``lognorm`` columns, and ``inside_p`` is the sum of the
        ring's marginals over the cluster labels.  The results are in the caller's contig order."""
        from . import packing

        n, nc = int(item_ptr[-1]), len(contigs)
        bg = self.classes_.index(self.background)
        y, score, lognorm_c, lognorm = np.zeros(n, dtype=np.int8), np.zeros(nc), np.zeros(nc), np.zeros(nc)
        inside_p = np.zeros(n) if marginals else None
        for ring in (False, True):
            keep = [ci for ci in range(nc) if bool(is_ring[ci]) == ring]
            if not keep:
                continue
            at = np.concatenate([np.arange(item_ptr[ci], item_ptr[ci + 1]) for ci in keep])
            sub = packing.pack_contigs([contigs[ci] for ci in keep], self._attr_index, "protein")
            csr = (sub.item_ptr.astype(np.int32), sub.attr_ptr.astype(np.int32), sub.attr_id)
            masks = None if allowed is None else np.ascontiguousarray(np.asarray(allowed)[at])
            if ring:
                out = model.ring(*csr, device=self.device, allowed=masks, want_path=True, want_marginals=marginals)
                y[at], score[keep], lognorm_c[keep], lognorm[keep] = out["labels"], out["score"], out["lognorm"], out["lognorm"]
                if marginals:
                    inside_p[at] = np.delete(out["marginals"], bg, axis=1).sum(axis=1)
            else:
                y[at], score[keep], lognorm_c[keep], lognorm[keep] = model.viterbi_min_run(*csr, self._cluster_set(), 1,
                                                                                            device=self.device, allowed=masks)
                if marginals:
                    inside_p[at] = model.marginals_min_run(*csr, self._cluster_set(), 1, device=self.device, allowed=masks,
                                                           want_marginals=False)[1]
        return y, score, lognorm_c, lognorm, inside_p

    def _whole_contigs(self, genes: Iterable[Any], known: Optional[tables.ClusterTable]):
        """``(contigs, CSR arrays, known masks or None)`` of the caller's genes sorted by (sequence, start), for a whole-contig
        call; ``(contigs, None, None)`` without genes."""
        from . import packing

        genes = sorted(genes, key=operator.attrgetter("source.id", "start"))
        for gene in genes:
            gene.protein.domains.sort(key=operator.attrgetter("start"))
        contigs = [list(g) for _, g in itertools.groupby(genes, key=operator.attrgetter("source.id"))]
        if not genes:
            return contigs, None, None
        batch = packing.pack_contigs(contigs, self._attr_index, "protein")
        allowed = None
        if known is not None:
            from .train_cli import join_clusters

            allowed = known_masks(len(genes), known, join_clusters(genes, known, device=self.device), self.classes_, self.background)
        return contigs, (batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32), batch.attr_id), allowed

    def _cluster_set(self) -> int:
        """The mask of every label but the background."""
        return ((1 << len(self.classes_)) - 1) & ~(1 << self.classes_.index(self.background))

    def predict_cluster_counts(self, genes: Iterable[Any], max_clusters: int = 8,
                               known: Optional[tables.ClusterTable] = None) -> Dict[str, List[Any]]:
        """How many clusters every contig holds, as a distribution (module docstring): one ``run_counts`` call over all contigs
        with the set of every label but the background, sum semiring only.  Fills and returns ``cluster_counts_``, the
        per-contig columns ``count_columns(max_clusters)``: ``sequence_id``, ``genes``, ``p_0 .. p_{K-1}`` = P(exactly k maximal
        runs of genes with a cluster label | x), ``p_ge_K`` = P(at least K), K = ``max_clusters``, and ``map_clusters``, the arg
        max over 0 .. K, the smaller winning a tie.  A row is normalised by the recursion's own total: it sums to 1 to
        rounding.  A run counts genes of any length, annotated or not; no threshold and no refiner is applied.  ``known``
        restricts the lattice as in the other prediction methods.  ``ValueError`` before any device call for a
        ``max_clusters`` that is not an integer or lies outside 1 .. 32."""
        try:
            max_clusters = operator.index(max_clusters)
        except TypeError:
            raise ValueError(f"max_clusters is an integer, got {max_clusters!r}") from None
        if not 1 <= max_clusters <= 32:
            raise ValueError(f"max_clusters = {max_clusters} is outside 1 .. 32")
        model = self._fitted()
        names = count_columns(max_clusters)
        self.cluster_counts_ = {name: [] for name in names}
        contigs, csr, allowed = self._whole_contigs(genes, known)
        if csr is None:
            return self.cluster_counts_
        mass, _, _, _ = model.run_counts(*csr, self._cluster_set(), max_clusters, device=self.device, allowed=allowed,
                                         want_paths=False, want_lognorm=False)
        top = mass.max(axis=1, keepdims=True)
        p = np.exp(mass - (top + np.log(np.exp(mass - top).sum(axis=1, keepdims=True))))
        for ci, contig in enumerate(contigs):
            row = (contig[0].source.id, int(csr[0][ci + 1] - csr[0][ci]), *p[ci].tolist(), int(np.argmax(p[ci])))
            for name, value in zip(names, row):
                self.cluster_counts_[name].append(value)
        return self.cluster_counts_

    def predict_count_clusters(self, genes: Iterable[Any], n_clusters: int = 1,
                               known: Optional[tables.ClusterTable] = None) -> List[Any]:
        """Clusters as the runs of the best whole-contig label path AMONG THOSE with exactly ``n_clusters`` maximal runs of genes
        with a label other than the background (module docstring): plane ``n_clusters`` of one ``run_counts`` call with K =
        ``n_clusters + 1``, max semiring only.  The clusters are what ``predict_path_clusters`` returns for its path: ids
        ``{sequence}_cluster_{number}``, the caller's genes, ``type`` from the run's most frequent label (the smaller label id
        on ties) and ``path_type``.  A contig on which no path has that many runs (fewer than ``2 n_clusters - 1`` genes, or
        ``known`` forbids it) gives no cluster.  ``count_scores_`` holds per contig the path's score (``-inf`` without a path).
        ``ValueError`` before any device call for an ``n_clusters`` that is not an integer or lies outside 0 .. 31."""
        try:
            n_clusters = operator.index(n_clusters)
        except TypeError:
            raise ValueError(f"n_clusters is an integer, got {n_clusters!r}") from None
        if not 0 <= n_clusters <= 31:
            raise ValueError(f"n_clusters = {n_clusters} is outside 0 .. 31")
        from .refine import _cluster_class
        from .types import _cluster_type_factory

        model = self._fitted()
        self.count_scores_ = []
        contigs, csr, allowed = self._whole_contigs(genes, known)
        if csr is None:
            return []
        _, score, y, _ = model.run_counts(*csr, self._cluster_set(), n_clusters + 1, device=self.device, allowed=allowed,
                                          want_log_mass=False, want_lognorm=False)
        L = len(self.classes_)
        bg = self.classes_.index(self.background)
        Cluster = _cluster_class()
        clusters: List[Any] = []
        for ci, contig in enumerate(contigs):
            c0, c1 = int(csr[0][ci]), int(csr[0][ci + 1])
            self.count_scores_.append(float(score[ci, n_clusters]))
            if not score[ci, n_clusters] > -np.inf:
                continue
            path = y[n_clusters, c0:c1].astype(np.int64)
            inside = np.concatenate([[False], path != bg, [False]])
            edges = np.flatnonzero(inside[1:] != inside[:-1])
            for found, (a, b) in enumerate(zip(edges[::2].tolist(), edges[1::2].tolist()), 1):
                cluster = Cluster(f"{contig[0].source.id}_cluster_{found}", list(contig[a:b]))
                major = int(np.argmax(np.bincount(path[a:b], minlength=L)))
                cluster.type = _cluster_type_factory(cluster)(self.label_types_[major])
                cluster.path_type = ";".join(self.label_types_[major]) or UNKNOWN
                clusters.append(cluster)
        return clusters

    def predict_genes_and_clusters(self, genes: Iterable[Any], *, threshold: float = 0.8, n_cds: int = 3, edge_distance: int = 0,
                                   trim: bool = True, pad: bool = True, known: Optional[tables.ClusterTable] = None,
                                   region_posteriors: bool = False, boundary_samples: int = 0,
                                   seed: int = 0, alternatives: int = 0,
                                   alternatives_margin: int = 10,
                                   boundary_posteriors: bool = False, run_posteriors: bool = False,
                                   run_reach: int = 256, attributions: bool = False,
                                   attribution_reach: int = 10, margins: bool = False) -> Tuple[List[Any], List[Any]]:
        """``(predict_probabilities(genes), predict_clusters(genes))`` from one device pass; with ``region_posteriors`` a
        second, whole-contig pass gives every cluster its region posteriors, and with ``boundary_samples = N > 0`` one more
        draws N label paths per contig under ``seed`` and gives every cluster its boundary intervals; with ``alternatives = K >
        0`` (at most 32) a Viterbi pass and one list-Viterbi call give every cluster the K best readings of its neighbourhood of
        ``alternatives_margin`` genes on either side; with ``boundary_posteriors`` one more whole-contig pass gives every
        cluster ``start_probability`` and ``end_probability`` and the model ``sequence_posteriors_``, the per-contig columns
        ``SEQUENCE_COLUMNS``; with ``run_posteriors`` one more whole-contig pass and one native call give every cluster
        the exact start and end distributions of the run through its anchor, over ``run_reach`` (0 .. 65536) genes to either
        side (module docstring); with ``attributions`` one more whole-contig pass and one native call give every cluster the
        exact knock-out contribution of every gene and domain in it and ``attribution_reach`` genes around it
        (``predict_clusters``); with ``margins`` one native call (two max-plus walks of the contigs, no forward-backward pass)
        gives every cluster its best-path score margins (``_margins``).  ``ValueError`` before any device call for an option
        that is not an integer or lies outside its range."""
        from . import _native

        try:
            alternatives, alternatives_margin = operator.index(alternatives), operator.index(alternatives_margin)
        except TypeError:
            raise ValueError(f"alternatives and alternatives_margin are integers, got {alternatives!r} and "
                             f"{alternatives_margin!r}") from None
        if not 0 <= alternatives <= 32:
            raise ValueError(f"alternatives = {alternatives} is outside 0 .. 32")
        if alternatives_margin < 0:
            raise ValueError(f"alternatives_margin = {alternatives_margin} is negative")

        try:
            boundary_samples, seed = operator.index(boundary_samples), operator.index(seed)
        except TypeError:
            raise ValueError(f"boundary_samples and seed are integers, got {boundary_samples!r} and {seed!r}") from None
        if not 0 <= boundary_samples <= 1 << 20:
            raise ValueError(f"boundary_samples = {boundary_samples} is outside 0 .. 1048576")
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed {seed} is outside 0 .. 2**64 - 1")
        try:
            run_reach = operator.index(run_reach)
        except TypeError:
            raise ValueError(f"run_reach is an integer, got {run_reach!r}") from None
        if not 0 <= run_reach <= 65536:
            raise ValueError(f"run_reach = {run_reach} is outside 0 .. 65536")
        try:
            attribution_reach = operator.index(attribution_reach)
        except TypeError:
            raise ValueError(f"attribution_reach is an integer, got {attribution_reach!r}") from None
        if attribution_reach < 0:
            raise ValueError(f"attribution_reach = {attribution_reach} is negative")
        from .refine import _cluster_class
        from .types import _cluster_type_factory

        _, contigs, scored, batch, p_all, p_any, allowed = self._score(genes, pad, known)
        annotated = self._annotated(contigs, scored, batch, p_any)
        if boundary_posteriors:
            self.sequence_posteriors_ = {name: [] for name in self.SEQUENCE_COLUMNS}
        if not annotated:
            return annotated, []
        has_domains = np.fromiter((1 if g.protein.domains else 0 for g in annotated), dtype=np.uint8, count=len(annotated))
        item_ptr = batch.item_ptr.astype(np.int32)
        rows = _native.segment(p_any, has_domains, item_ptr, threshold=threshold, n_cds=n_cds, edge_distance=edge_distance,
                               trim=trim, device=self.device, carry_state=False)
        Cluster = _cluster_class()
        clusters: List[Any] = []
        for contig, number, first, last in rows.tolist():
            members = annotated[first:last]
            cluster = Cluster(f"{members[0].source.id}_cluster_{number}", list(members))
            proba = type_probabilities(p_all[first:last], self.label_types_, self.types_)
            cluster.type_probabilities = proba
            cluster.type = _cluster_type_factory(cluster)(type_of(proba))
            clusters.append(cluster)
        # what the whole-contig passes below share: the segment kernel's rows and the set of every label but the background
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
        not_background = ((1 << len(self.classes_)) - 1) & ~(1 << self.classes_.index(self.background))
        if region_posteriors and clusters:
            self._region_posteriors(batch, allowed, rows, item_ptr, not_background, clusters)
        if boundary_samples > 0 and clusters:
            self._boundary_intervals(batch, allowed, rows, item_ptr, not_background, clusters, annotated, p_any, boundary_samples, seed)
        if boundary_posteriors:  # (the per-contig table does not need a called cluster)
            self._boundary_posteriors(batch, allowed, rows, item_ptr, not_background, clusters, annotated)
        if alternatives > 0 and clusters:
            self._alternatives(batch, allowed, rows, item_ptr, clusters, annotated, p_any, alternatives, alternatives_margin)
        if run_posteriors and clusters:
            self._run_posteriors(batch, allowed, rows, item_ptr, not_background, clusters, annotated, p_any, run_reach)
        if attributions and clusters:
            self._attributions(batch, allowed, rows, item_ptr, not_background, clusters, annotated, attribution_reach)
        if margins and clusters:
            self._margins(batch, allowed, rows, item_ptr, not_background, clusters)
        return annotated, clusters


def write_attributions(path, clusters: Sequence[Any]) -> None:
    """``attributions.tsv``: what every called cluster rests on, one row per gene of the call and its neighbourhood (``domain``
    empty) and per domain of such a gene, columns ``cluster_id, sequence_id, protein_id, offset, domain, contribution,
    p_without``: ``contribution`` = log P(region | x) - log P(region | x without it), positive when the call leans on it, and
    ``p_without`` = exp(log P(region | x) - contribution), the region's probability without it; floats with ``repr``."""
    with open(path, "w") as out:
        out.write("\t".join(("cluster_id", "sequence_id", "protein_id", "offset", "domain", "contribution", "p_without")) + "\n")
        for cluster in clusters:
            logp = getattr(cluster, "attribution_log_probability", -math.inf)
            for row in getattr(cluster, "attributions", ()):
                for domain, contribution in [("", row["contribution"])] + list(row["domains"]):
                    without = math.exp(logp - contribution) if logp > -math.inf else 0.0
                    out.write("\t".join((str(cluster.id), str(cluster.source.id), str(row["protein_id"]), str(row["offset"]), domain,
                                         repr(contribution), repr(without))) + "\n")


def write_alternatives(path, clusters: Sequence[Any]) -> None:
    """``alternatives.tsv``: one row per called cluster and rank, columns ``cluster_id, rank, start, end, type, log_p, p``
    (start, end and type empty where the path has no run around the cluster's anchor); floats with ``repr``."""
    with open(path, "w") as out:
        out.write("\t".join(("cluster_id", "rank", "start", "end", "type", "log_p", "p")) + "\n")
        for cluster in clusters:
            for alt in getattr(cluster, "alternatives", ()):
                run = alt["run"] is not None
                where = (str(alt["start"]), str(alt["end"]), alt["type"]) if run else ("", "", "")
                out.write("\t".join((str(cluster.id), str(alt["rank"]), *where, repr(alt["log_p"]), repr(math.exp(alt["log_p"])))) + "\n")


def write_boundaries(path, clusters: Sequence[Any], floor: float = 1e-6) -> None:
    """``boundaries.tsv``: the exact start and end distributions of the run through every called cluster's anchor, given that the
    anchor lies in a cluster: one row per cluster, side (``start`` / ``end``) and gene with conditional probability >= ``floor``,
    columns ``cluster_id, side, protein_id, position, p`` (position: the gene's start for a start, its end for an end); floats
    with ``repr``."""
    with open(path, "w") as out:
        out.write("\t".join(("cluster_id", "side", "protein_id", "position", "p")) + "\n")
        for cluster in clusters:
            for side, gene, position, p in getattr(cluster, "run_boundaries", ()):
                if p >= floor:
                    out.write("\t".join((str(cluster.id), side, str(gene.protein.id), str(position), repr(p))) + "\n")


def write_path_clusters(path, clusters: Sequence[Any], marginals: bool = False, wraps: bool = False) -> None:
    """``path_clusters.tsv``: one row per cluster of ``predict_path_clusters``, columns ``sequence_id, cluster_id, start, end,
    genes, type`` (type: the ``";"``-joined names, ``"Unknown"`` for a label without types); with ``marginals`` (clusters of
    ``predict_path_clusters(..., marginals=True)``) ``average_p, max_p, min_p`` behind them, floats with ``repr``; with ``wraps``
    (clusters of ``predict_path_clusters(..., circular=...)``) a last column ``wraps``, 1 for a cluster that crosses the cut of
    its circular contig and 0 otherwise.  Such a cluster's row has ``start`` > ``end``: it runs from the start of its first
    gene, near the contig's end, across the origin to the end of its last gene."""
    more = ("average_p", "max_p", "min_p") if marginals else ()
    with open(path, "w") as out:
        out.write("\t".join(("sequence_id", "cluster_id", "start", "end", "genes", "type") + more + (("wraps",) if wraps else ())) + "\n")
        for cluster in clusters:
            members = cluster.genes
            names = getattr(cluster, "path_type", None) or ";".join(sorted(getattr(cluster.type, "names", ()))) or UNKNOWN
            across = bool(getattr(cluster, "wraps_origin", False))
            start, end = (members[0].start, members[-1].end) if across else (min(g.start for g in members), max(g.end for g in members))
            out.write("\t".join((str(members[0].source.id), str(cluster.id), str(start), str(end), str(len(members)), names,
                                 *(repr(float(getattr(cluster, name))) for name in more),
                                 *((str(int(across)),) if wraps else ()))) + "\n")


def write_path_genes(path, columns) -> None:
    """``path_genes.tsv``: one row per gene, columns ``TypedClusterCRF.PATH_GENE_COLUMNS`` (``path_genes_``); ``p`` with
    ``repr``."""
    names = TypedClusterCRF.PATH_GENE_COLUMNS
    with open(path, "w") as out:
        out.write("\t".join(names) + "\n")
        for row in zip(*(columns[name] for name in names)):
            out.write("\t".join(repr(v) if isinstance(v, float) else str(v) for v in row) + "\n")


def write_paths(path, columns) -> None:
    """``paths.tsv``: one row per contig, columns ``TypedClusterCRF.PATH_COLUMNS`` (``path_posteriors_``, or a list of row
    dicts); floats with ``repr``."""
    names = TypedClusterCRF.PATH_COLUMNS
    rows = zip(*(columns[name] for name in names)) if isinstance(columns, dict) else ([row[name] for name in names] for row in columns)
    with open(path, "w") as out:
        out.write("\t".join(names) + "\n")
        for row in rows:
            out.write("\t".join(repr(v) if isinstance(v, float) else str(v) for v in row) + "\n")


def count_columns(max_clusters: int) -> Tuple[str, ...]:
    """The columns of ``cluster_counts_`` / ``cluster_counts.tsv`` at K = ``max_clusters``: ``sequence_id, genes, p_0 .. p_{K-1},
    p_ge_K, map_clusters``."""
    return ("sequence_id", "genes", *(f"p_{k}" for k in range(max_clusters)), f"p_ge_{max_clusters}", "map_clusters")


def write_cluster_counts(path, columns: Dict[str, Sequence[Any]]) -> None:
    """``cluster_counts.tsv``: one row per contig, the columns of ``cluster_counts_`` in their order; floats with ``repr``."""
    names = list(columns)
    with open(path, "w") as out:
        out.write("\t".join(names) + "\n")
        for row in zip(*(columns[name] for name in names)):
            out.write("\t".join(repr(v) if isinstance(v, float) else str(v) for v in row) + "\n")


def write_sequences(path, columns: Dict[str, Sequence[Any]]) -> None:
    """``sequences.tsv``: one row per contig, columns ``TypedClusterCRF.SEQUENCE_COLUMNS`` (``sequence_posteriors_``); floats
    with ``repr``."""
    names = TypedClusterCRF.SEQUENCE_COLUMNS
    with open(path, "w") as out:
        out.write("\t".join(names) + "\n")
        for row in zip(*(columns[name] for name in names)):
            out.write("\t".join(repr(v) if isinstance(v, float) else str(v) for v in row) + "\n")


# ---------------------------------------------------------------------------------------------- command line
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m gecco_amd.typed", description=(
        "Train a type-aware cluster CRF on labelled tables, or call typed clusters with one."))
    sub = ap.add_subparsers(dest="command", required=True)
    tr = sub.add_parser("train", help="tables in, a typed model directory out")
    tr.add_argument("-f", "--features", required=True, nargs="+", action="extend", help="domain annotation table(s) (TSV)")
    tr.add_argument("-g", "--genes", required=True, help="gene table (TSV)")
    tr.add_argument("-c", "--clusters", required=True, help="cluster table (TSV): a gene overlapping a cluster takes its type")
    tr.add_argument("-e", "--e-filter", type=float, default=None, help="e-value cutoff for protein domains to be included")
    tr.add_argument("-p", "--p-filter", type=float, default=1e-9, help="p-value cutoff for protein domains to be included")
    tr.add_argument("--no-shuffle", dest="shuffle", action="store_false", help="do not shuffle the data before fitting")
    tr.add_argument("--seed", type=int, default=42, help="seed of random and numpy.random")
    tr.add_argument("-W", "--window-size", type=int, default=5)
    tr.add_argument("--window-step", type=int, default=1)
    tr.add_argument("--c1", type=float, default=0.15, help="strength of the L1 regularisation")
    tr.add_argument("--c2", type=float, default=0.15, help="strength of the L2 regularisation")
    tr.add_argument("--class-weight", choices=("balanced",), default=None,
                    help="weigh every training sequence by its clusters' types: 'balanced' is n / (k * count) per type")
    tr.add_argument("--miss-cost", type=float, default=0.0, help="training cost of calling a cluster gene background")
    tr.add_argument("--false-cost", type=float, default=0.0, help="training cost of calling a background gene a cluster gene")
    tr.add_argument("--feature-type", choices=("protein", "domain"), default="protein")
    tr.add_argument("--select", type=float, default=None, help="fraction of domains kept by Fisher selection")
    tr.add_argument("--correction", type=str, default=None, help="multiple-testing correction of the selection p-values")
    tr.add_argument("--unknown", choices=("label", "any"), default="label",
                    help="genes of a cluster without a type: the label 'Unknown', or the set of every cluster label")
    tr.add_argument("--length-model", type=int, default=None, metavar="M",
                    help="after the fit, learn a score on the length of a region from the same tables (a table of M scores, at "
                    "most 32, and a tail score) and write it next to the model: predict --path-clusters --length-model decodes "
                    "with it")
    tr.add_argument("--length-c2", type=float, default=1.0, metavar="C", help="the L2 penalty of the length model's fit")
    tr.add_argument("--device", type=int, default=0)
    tr.add_argument("-o", "--output-dir", default=".", help="the model directory")
    pr = sub.add_parser("predict", help="tables in; genes.tsv, features.tsv and clusters.tsv out")
    pr.add_argument("--model", required=True, help="a directory written by train")
    pr.add_argument("-f", "--features", required=True, nargs="+", action="extend", help="domain annotation table(s) (TSV)")
    pr.add_argument("-g", "--genes", required=True, help="gene table (TSV)")
    pr.add_argument("-e", "--e-filter", type=float, default=None, help="e-value cutoff for protein domains to be included")
    pr.add_argument("-p", "--p-filter", type=float, default=1e-9, help="p-value cutoff for protein domains to be included")
    pr.add_argument("-m", "--threshold", type=float, default=0.8, help="probability above which a gene is in a cluster")
    pr.add_argument("-c", "--cds", type=int, default=3, help="minimum number of annotated genes of a cluster")
    pr.add_argument("-E", "--edge-distance", type=int, default=0, help="annotated genes separating a cluster from the edge")
    pr.add_argument("--no-trim", dest="trim", action="store_false", help="keep genes without domains on cluster edges")
    pr.add_argument("--no-pad", dest="pad", action="store_false", help="skip sequences shorter than the window")
    pr.add_argument("--known", default=None, help="cluster table (TSV) of regions known beforehand: their genes cannot be "
                    "background, and take the region's type where the model has a label for it")
    pr.add_argument("--region-posteriors", action="store_true",
                    help="add region_p and {type}_region_p to clusters.tsv: the whole-contig posterior probability that every gene of "
                    "a called region lies in a cluster, and in one of the type")
    pr.add_argument("--boundary-samples", type=int, default=0, metavar="N",
                    help="add anchor_p, exact_p, start_lo, start_hi, end_lo and end_hi to clusters.tsv: 90 %% intervals of every "
                    "called region's start and end from N label paths drawn from the whole-contig posterior")
    pr.add_argument("--seed", type=int, default=0, help="seed of the drawn paths (with --boundary-samples)")
    pr.add_argument("--alternatives", type=int, default=0, metavar="K",
                    help="write alternatives.tsv: for every called region the K (at most 32) best label paths of its neighbourhood, "
                    "each with its exact probability given that the rest of the contig follows the Viterbi path")
    pr.add_argument("--alternatives-margin", type=int, default=10, metavar="M",
                    help="genes on either side of a called region in its neighbourhood (with --alternatives)")
    pr.add_argument("--boundary-posteriors", action="store_true",
                    help="add start_p and end_p to clusters.tsv: the whole-contig posterior probability that a run of cluster labels "
                    "starts at a called region's first gene, and ends at its last; write sequences.tsv: per contig its log Z, "
                    "path entropy and expected number of clusters")
    pr.add_argument("--run-posteriors", action="store_true",
                    help="add run_anchor_p, run_p, run_start_lo, run_start_hi, run_end_lo, run_end_hi, run_start_beyond_p and "
                    "run_end_beyond_p to clusters.tsv: the exact whole-contig distribution of where the run of cluster labels through "
                    "every called region starts and ends; write boundaries.tsv, the distributions themselves")
    pr.add_argument("--run-reach", type=int, default=256, metavar="R",
                    help="genes on either side of a called region's anchor that the exact distributions cover (with --run-posteriors)")
    pr.add_argument("--attributions", action="store_true",
                    help="write attributions.tsv: for every called region the exact change of its whole-contig log-probability when "
                    "one gene, or one domain of a gene, is taken out of the input, for the genes in and around it")
    pr.add_argument("--attribution-reach", type=int, default=10, metavar="R",
                    help="genes on either side of a called region that attributions.tsv covers (with --attributions)")
    pr.add_argument("--margins", action="store_true",
                    help="add margin_present, margin_absent and margin_broken to clusters.tsv: how much the score of the best "
                    "whole-contig label path drops when every gene of a called region must lie in a cluster, must not, or when one "
                    "must not (log-ratios of two paths' probabilities, not posteriors)")
    pr.add_argument("--path-clusters", type=int, default=None, nargs="?", const=0, metavar="M",
                    help="write path_clusters.tsv and paths.tsv: the regions of the best whole-contig label path among those in "
                    "which every region has at least M (at most 32) genes, and per contig that path's probability and the "
                    "probability that no region is shorter; without M and with --length-model: the best path under the "
                    "model directory's length scores")
    pr.add_argument("--length-model", action="store_true",
                    help="with --path-clusters (and no M): decode under the length scores that train --length-model wrote, in "
                    "place of a minimum length")
    pr.add_argument("--path-marginals", action="store_true",
                    help="with --path-clusters M: add average_p, max_p and min_p to path_clusters.tsv, of the probability that a "
                    "gene lies in a region given that no region has fewer than M genes; write path_genes.tsv, that probability "
                    "per gene")
    pr.add_argument("--circular", default=None, metavar="FILE|all",
                    help="with --path-clusters 1: the contigs that are rings (complete chromosomes, plasmids) -- a file with one "
                    "sequence id per line, or `all`; a region across the cut of such a contig is one cluster, and "
                    "path_clusters.tsv gains the column wraps")
    pr.add_argument("--cluster-counts", type=int, default=None, metavar="K",
                    help="write cluster_counts.tsv: per contig the exact whole-contig probability that it holds 0, 1, ... K - 1 "
                    "clusters and at least K (at most 32), and the most probable number")
    pr.add_argument("--exact-clusters", type=int, default=None, metavar="N",
                    help="write count_clusters.tsv: the regions of the best whole-contig label path among those with exactly N (at "
                    "most 31) regions")
    pr.add_argument("--device", type=int, default=0)
    pr.add_argument("-o", "--output-dir", default=".", help="directory of the output tables")
    return ap


def main(argv: Optional[List[str]] = None) -> int:
    from .train_cli import load_training_genes

    args = build_parser().parse_args(argv)
    if args.command == "train":
        if args.feature_type != "protein":
            raise ValueError("typed models use protein features")
        random.seed(args.seed)
        np.random.seed(args.seed)
        genes = load_training_genes(args.genes, args.features, args.e_filter, args.p_filter)
        clusters = tables.ClusterTable.load(args.clusters)
        crf = TypedClusterCRF(args.window_size, args.window_step, args.device, unknown=args.unknown, c1=args.c1, c2=args.c2,
                              class_weight=args.class_weight, miss_cost=args.miss_cost, false_cost=args.false_cost)
        if args.length_model is not None and not 1 <= args.length_model <= 32:
            raise ValueError(f"--length-model {args.length_model} is outside 1 .. 32")
        crf.fit(genes, clusters, shuffle=args.shuffle, select=args.select, correction_method=args.correction)
        if args.length_model is not None:
            crf.fit_length_model(genes, clusters, max_length=args.length_model, c2=args.length_c2)
        crf.save(args.output_dir)
        print(f"train: {len(genes)} genes, {len(clusters)} clusters, labels {crf.classes_} -> {args.output_dir}", file=sys.stderr)
        return 0
    if args.length_model:
        if args.path_clusters is None:
            raise ValueError("--length-model needs --path-clusters")
        if args.path_clusters != 0:
            raise ValueError("--path-clusters M and --length-model are two ways to say how long a region is: give one")
    elif args.path_clusters == 0:
        raise ValueError("--path-clusters needs M, or --length-model")
    if args.path_clusters is not None and not args.length_model and not 1 <= args.path_clusters <= 32:
        raise ValueError(f"--path-clusters {args.path_clusters} is outside 1 .. 32")
    if args.path_marginals and args.path_clusters is None:
        raise ValueError("--path-marginals needs --path-clusters M")
    circular = None
    if args.circular is not None:
        if args.path_clusters is None:
            raise ValueError("--circular needs --path-clusters 1")
        if args.circular == "all":
            circular = True
        else:
            with open(args.circular) as fh:
                circular = [line.strip() for line in fh if line.strip()]
    if args.cluster_counts is not None and not 1 <= args.cluster_counts <= 32:
        raise ValueError(f"--cluster-counts {args.cluster_counts} is outside 1 .. 32")
    if args.exact_clusters is not None and not 0 <= args.exact_clusters <= 31:
        raise ValueError(f"--exact-clusters {args.exact_clusters} is outside 0 .. 31")
    crf = TypedClusterCRF.trained(args.model, device=args.device)
    genes = load_training_genes(args.genes, args.features, args.e_filter, args.p_filter)
    annotated, found = crf.predict_genes_and_clusters(genes, threshold=args.threshold, n_cds=args.cds,
                                                      edge_distance=args.edge_distance, trim=args.trim, pad=args.pad,
                                                      known=None if args.known is None else tables.ClusterTable.load(args.known),
                                                      region_posteriors=args.region_posteriors,
                                                      boundary_samples=args.boundary_samples, seed=args.seed,
                                                      alternatives=args.alternatives,
                                                      alternatives_margin=args.alternatives_margin,
                                                      boundary_posteriors=args.boundary_posteriors,
                                                      run_posteriors=args.run_posteriors, run_reach=args.run_reach,
                                                      attributions=args.attributions, attribution_reach=args.attribution_reach,
                                                      margins=args.margins)
    os.makedirs(args.output_dir, exist_ok=True)
    tables.GeneTable.from_genes(annotated).dump(os.path.join(args.output_dir, "genes.tsv"))
    tables.FeatureTable.from_genes(annotated).dump(os.path.join(args.output_dir, "features.tsv"))
    typed_cluster_table(found, crf.types_).dump(os.path.join(args.output_dir, "clusters.tsv"))
    if args.alternatives > 0:
        write_alternatives(os.path.join(args.output_dir, "alternatives.tsv"), found)
    if args.boundary_posteriors:
        write_sequences(os.path.join(args.output_dir, "sequences.tsv"), crf.sequence_posteriors_)
    if args.run_posteriors:
        write_boundaries(os.path.join(args.output_dir, "boundaries.tsv"), found)
    if args.attributions:
        write_attributions(os.path.join(args.output_dir, "attributions.tsv"), found)
    if args.path_clusters is not None:
        known = None if args.known is None else tables.ClusterTable.load(args.known)
        write_path_clusters(os.path.join(args.output_dir, "path_clusters.tsv"),
                            crf.predict_path_clusters(genes, known=known, marginals=args.path_marginals,
                                                      **({"length_model": True} if args.length_model else {"min_run": args.path_clusters}),
                                                      **({} if args.circular is None else {"circular": circular})),
                            marginals=args.path_marginals, **({} if args.circular is None else {"wraps": True}))
        if args.path_marginals:
            write_path_genes(os.path.join(args.output_dir, "path_genes.tsv"), crf.path_genes_)
        write_paths(os.path.join(args.output_dir, "paths.tsv"), crf.path_posteriors_)
    if args.cluster_counts is not None or args.exact_clusters is not None:
        known = None if args.known is None else tables.ClusterTable.load(args.known)
        if args.cluster_counts is not None:
            write_cluster_counts(os.path.join(args.output_dir, "cluster_counts.tsv"),
                                 crf.predict_cluster_counts(genes, max_clusters=args.cluster_counts, known=known))
        if args.exact_clusters is not None:
            write_path_clusters(os.path.join(args.output_dir, "count_clusters.tsv"),
                                crf.predict_count_clusters(genes, n_clusters=args.exact_clusters, known=known))
    print(f"predict: {len(annotated)} genes, {len(found)} clusters -> {args.output_dir}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
