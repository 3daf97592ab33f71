"""Training front end (``gecco train``): labelled tables in, a complete GECCO model directory out.

What the reference runs (``gecco/cli/commands/train.py``, ``_common.py``), restated without polars, Biopython or scipy:
the genes table is annotated with the features tables (``cv.annotate_genes``, with its checks), genes are sorted by
(sequence, start, end) and domains by (start, end), domains are filtered by e-value and p-value, genes overlapping a
cluster are labelled positive, and ``ClusterCRF.fit`` trains the model.  The overlap join of genes and clusters runs on the
device (``_native.cluster_overlaps``, ``csrc/crf_overlap.hip``): one pass gives both the labels and the genes of every
cluster, which feed the type classifier's training files.

The directory written::

    model.pkl, model.pkl.md5   the fitted ClusterCRF (``ClusterCRF.save``)
    model.trans.tsv            transition weights: from, to, weight
    model.state.tsv            state weights: attr, label, weight
    domains.tsv                the composition's columns: the selected domains with --select, else every domain left
    types.tsv                  cluster id and its ";"-joined sorted type names, for every cluster with genes
    compositions.npz           the clusters' weighted domain compositions, in scipy.sparse.save_npz's COO layout

Run as ``python -m gecco_amd.train --genes G.tsv --features F.tsv --clusters C.tsv -o DIR``.
"""
import argparse
import csv
import math
import operator
import os
import random
import sys
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native, tables

__all__ = ["ClusterJoin", "join_clusters", "assigned_clusters", "type_names", "save_npz_coo", "domain_rows",
           "cluster_compositions", "write_weight_tables", "write_type_labels", "composition_domains", "write_model_dir",
           "load_training_genes", "build_parser", "main"]


# ---------------------------------------------------------------------------------------------- overlap join
class ClusterJoin:
    """The overlap join of sorted genes with a clusters table.

    ``labels[g]``: 1 where gene g overlaps any cluster of its sequence (bounds inclusive), else 0.  ``row_of[i]``: the
    position of clusters-table row i in the member CSR; ``member_ptr`` / ``member_gene``: the genes of every cluster, in
    gene order."""

    def __init__(self, labels: np.ndarray, row_of: np.ndarray, member_ptr: np.ndarray, member_gene: np.ndarray) -> None:
        self.labels, self.row_of, self.member_ptr, self.member_gene = labels, row_of, member_ptr, member_gene

    def members(self, i: int) -> np.ndarray:
        """The genes of clusters-table row i."""
        r = int(self.row_of[i])
        return self.member_gene[self.member_ptr[r]:self.member_ptr[r + 1]]


def join_clusters(genes: Sequence[Any], clusters: tables.ClusterTable, device: int = 0) -> ClusterJoin:
    """Join ``genes`` (sorted by sequence id, then start) with the clusters of their sequences on the device.  A cluster on
    a sequence without genes has no members; a gene on a sequence without clusters is labelled 0."""
    gene_sid = [g.source.id for g in genes]
    cluster_sid = [str(s) for s in clusters.sequence_id]
    names = sorted(set(gene_sid).union(cluster_sid))
    code_of = {name: i for i, name in enumerate(names)}
    n, m = len(gene_sid), len(cluster_sid)
    g_seq = np.fromiter((code_of[s] for s in gene_sid), dtype=np.int32, count=n)
    g_start = np.fromiter((g.start for g in genes), dtype=np.int64, count=n)
    g_end = np.fromiter((g.end for g in genes), dtype=np.int64, count=n)
    c_seq = np.fromiter((code_of[s] for s in cluster_sid), dtype=np.int32, count=m)
    c_start = np.asarray(clusters.start, dtype=np.int64).reshape(m)
    c_end = np.asarray(clusters.end, dtype=np.int64).reshape(m)
    order = np.lexsort((c_start, c_seq))  # the kernel's layout: by sequence, then start
    c_ptr = np.searchsorted(c_seq[order], np.arange(len(names) + 1), side="left").astype(np.int32)
    labels, member_ptr, member_gene = _native.cluster_overlaps(g_seq, g_start, g_end, c_ptr, c_start[order], c_end[order],
                                                               device=device)
    row_of = np.empty(m, dtype=np.int64)
    row_of[order] = np.arange(m)
    return ClusterJoin(labels, row_of, member_ptr, member_gene)


def type_names(value: Any) -> Tuple[str, ...]:
    """The sorted type names of a clusters-table ``type`` cell: ``Unknown``, an empty cell or a missing value give none."""
    if value is None or (isinstance(value, float) and math.isnan(value)):
        return ()
    value = str(value)
    if value in ("", "Unknown"):
        return ()
    return tuple(sorted(set(value.split(";"))))


def assigned_clusters(clusters: tables.ClusterTable, join: ClusterJoin) -> List[Tuple[str, int, Tuple[str, ...]]]:
    """``_assign_clusters`` of the reference: ``(cluster_id, table row, type names)`` of every cluster with at least one
    gene, in sorted ``cluster_id`` order; rows with an empty id are skipped.  A repeated cluster id is a ``ValueError``
    (the reference would merge the genes of both rows and list the id twice)."""
    row_of_id: Dict[str, int] = {}
    for i, cid in enumerate(clusters.cluster_id):
        if cid is None or cid == "":
            continue
        cid = str(cid)
        if cid in row_of_id:
            raise ValueError(f"duplicate cluster id in the clusters table: {cid!r}")
        row_of_id[cid] = i
    out = []
    for cid in sorted(row_of_id):
        i = row_of_id[cid]
        if len(join.members(i)):
            out.append((cid, i, type_names(clusters.type[i])))
    return out


# ---------------------------------------------------------------------------------------------- outputs
def save_npz_coo(path: str, dense: np.ndarray) -> None:
    """``scipy.sparse.save_npz(path, scipy.sparse.coo_matrix(dense))`` with numpy alone: the nonzero entries in row-major
    order, int32 coordinates, compressed."""
    dense = np.asarray(dense, dtype=np.float64)
    row, col = np.nonzero(dense)
    np.savez_compressed(path, row=row.astype(np.int32), col=col.astype(np.int32), format=b"coo",
                        shape=np.array(dense.shape, dtype=np.int64), data=dense[row, col])


def _write_rows(path: str, header: List[str], rows) -> None:
    with open(path, "w") as f:  # (the reference's writer: csv's excel-tab dialect, so lines end with \r\n)
        writer = csv.writer(f, dialect="excel-tab")
        writer.writerow(header)
        for row in rows:
            writer.writerow(row)


def domain_rows(genes: Sequence[Any], all_possible: Sequence[str]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The composition kernel's domain rows of every gene: ``dom_ptr``, the column of each domain in ``all_possible``
    (-1 when absent) and its weight ``1 - pvalue`` (``Cluster.domain_composition``'s defaults)."""
    col_of = {name: i for i, name in enumerate(all_possible)}
    counts = np.fromiter((len(g.protein.domains) for g in genes), dtype=np.int64, count=len(genes))
    dom_ptr = np.zeros(len(genes) + 1, dtype=np.int64)
    np.cumsum(counts, out=dom_ptr[1:])
    nnz = int(dom_ptr[-1])
    dom_col = np.fromiter((col_of.get(d.name, -1) for g in genes for d in g.protein.domains), dtype=np.int32, count=nnz)
    dom_w = np.fromiter((1 - d.pvalue for g in genes for d in g.protein.domains), dtype=np.float64, count=nnz)
    return dom_ptr, dom_col, dom_w


def cluster_compositions(genes: Sequence[Any], join: ClusterJoin, assigned: Sequence[Tuple[str, int, Any]],
                         all_possible: Sequence[str], device: int = 0) -> np.ndarray:
    """The (clusters, domains) composition matrix of the ``assigned`` clusters over ``all_possible``, on the device from the
    member lists (``_native.domain_composition_members``)."""
    rows = np.array([join.row_of[i] for _, i, _ in assigned], dtype=np.int64)
    first = join.member_ptr[rows].astype(np.int64) if len(rows) else np.zeros(0, dtype=np.int64)
    counts = join.member_ptr[rows + 1].astype(np.int64) - first if len(rows) else np.zeros(0, dtype=np.int64)
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    take = np.repeat(first - ptr[:-1], counts) + np.arange(int(ptr[-1]), dtype=np.int64)
    dom_ptr, dom_col, dom_w = domain_rows(genes, all_possible)
    return _native.domain_composition_members(ptr, join.member_gene[take], dom_ptr, dom_col, dom_w, len(all_possible),
                                              normalize=True, device=device)


def write_weight_tables(output_dir: str, crf: Any) -> None:
    """``model.trans.tsv`` and ``model.state.tsv``: the fitted weights in ``transition_features_`` /
    ``state_features_`` order."""
    _write_rows(os.path.join(output_dir, "model.trans.tsv"), ["from", "to", "weight"],
                ([*labels, weight] for labels, weight in crf.model.transition_features_.items()))
    _write_rows(os.path.join(output_dir, "model.state.tsv"), ["attr", "label", "weight"],
                ([*attrs, weight] for attrs, weight in crf.model.state_features_.items()))


def write_type_labels(output_dir: str, all_possible: Sequence[str], assigned: Sequence[Tuple[str, int, Sequence[str]]]) -> None:
    """``domains.tsv`` (one domain per line) and ``types.tsv`` (cluster id, ";"-joined type names)."""
    with open(os.path.join(output_dir, "domains.tsv"), "w") as out:
        out.writelines(f"{domain}\n" for domain in all_possible)
    with open(os.path.join(output_dir, "types.tsv"), "w") as out:
        writer = csv.writer(out, dialect="excel-tab")
        for cid, _, names in assigned:
            writer.writerow([cid, ";".join(names)])


def composition_domains(crf: Any, genes: Sequence[Any]) -> List[str]:
    """The columns of the composition matrix: the selected domains after ``fit(select=...)``, else every domain name of
    the genes; sorted."""
    if crf.significant_features is not None:
        return sorted(crf.significant_features)
    return sorted({d.name for g in genes for d in g.protein.domains})


def write_model_dir(output_dir: str, crf: Any, genes: Sequence[Any], clusters: tables.ClusterTable, join: ClusterJoin,
                    device: int = 0) -> None:
    """Every file of the model directory (``train.py:190-215`` of the reference)."""
    os.makedirs(output_dir, exist_ok=True)
    crf.save(output_dir)
    write_weight_tables(output_dir, crf)
    all_possible = composition_domains(crf, genes)
    assigned = assigned_clusters(clusters, join)
    write_type_labels(output_dir, all_possible, assigned)
    comp = cluster_compositions(genes, join, assigned, all_possible, device=device)
    save_npz_coo(os.path.join(output_dir, "compositions.npz"), comp)


# ---------------------------------------------------------------------------------------------- front end
def load_training_genes(genes_path: str, features_paths: Sequence[str], e_filter: Optional[float] = None,
                        p_filter: Optional[float] = None) -> List[Any]:
    """Steps 2-4 of the reference's ``run``: genes annotated with every features table (``cv.annotate_genes``), sorted
    by (sequence, start, end) with domains sorted by (start, end), then the domains with ``i_evalue >= e_filter`` or
    ``pvalue >= p_filter`` removed."""
    from . import cv

    genes = tables.GeneTable.load(genes_path).to_genes()
    for path in features_paths:
        genes = cv.annotate_genes(genes, tables.FeatureTable.load(path))
    genes.sort(key=operator.attrgetter("source.id", "start", "end"))
    for gene in genes:
        gene.protein.domains.sort(key=operator.attrgetter("start", "end"))
        if e_filter is not None or p_filter is not None:
            gene.protein.domains[:] = [d for d in gene.protein.domains
                                       if (e_filter is None or d.i_evalue < e_filter) and (p_filter is None or d.pvalue < p_filter)]
    return genes


def build_parser() -> argparse.ArgumentParser:
    """The arguments of ``gecco train`` (``gecco/cli/commands/_parser.py``), with its defaults."""
    ap = argparse.ArgumentParser(prog="python -m gecco_amd.train", description=(
        "Train a CRF on labelled tables (gecco train) and write the model directory and the type classifier's training "
        "files."))
    ap.add_argument("-j", "--jobs", type=int, default=0, help="accepted as gecco train accepts it, and ignored")
    group = ap.add_argument_group("Input Tables")
    group.add_argument("-f", "--features", required=True, nargs="+", action="extend",
                       help="domain annotation table(s) (TSV), used to train the CRF")
    group.add_argument("-g", "--genes", required=True, help="gene table (TSV) with the coordinates of the training genes")
    group.add_argument("-c", "--clusters", required=True, help="cluster table (TSV): the genes overlapping a cluster are "
                                                               "positive; the clusters' types go to types.tsv")
    group = ap.add_argument_group("Domain Annotation")
    group.add_argument("-e", "--e-filter", type=float, default=None, help="e-value cutoff for protein domains to be included")
    group.add_argument("-p", "--p-filter", type=float, default=1e-9, help="p-value cutoff for protein domains to be included")
    group = ap.add_argument_group("Training Data")
    group.add_argument("--no-shuffle", dest="shuffle", action="store_false", help="do not shuffle the data before fitting")
    group.add_argument("--seed", type=int, default=42, help="seed of random and numpy.random")
    group = ap.add_argument_group("Training Parameters")
    group.add_argument("-W", "--window-size", type=int, default=5)
    group.add_argument("--window-step", type=int, default=1)
    group.add_argument("--c1", type=float, default=0.15, help="strength of the L1 regularisation")
    group.add_argument("--c2", type=float, default=0.15, help="strength of the L2 regularisation")
    # (not gecco train's: the options exist on the parsed arguments only when they are given)
    group.add_argument("--miss-cost", type=float, default=argparse.SUPPRESS,
                       help="training cost of a missed cluster gene (label_costs[('1', '0')]; default: none)")
    group.add_argument("--false-cost", type=float, default=argparse.SUPPRESS,
                       help="training cost of a false cluster gene (label_costs[('0', '1')]; default: none)")
    group.add_argument("--feature-type", choices=("protein", "domain"), default="protein")
    group.add_argument("--select", type=float, default=None, help="fraction of domains kept by Fisher selection")
    group.add_argument("--correction", type=str, default=None,
                       help="multiple-testing correction of the selection p-values")
    group = ap.add_argument_group("Output")
    group.add_argument("-o", "--output-dir", default=".", help="directory of the output files")
    return ap


def main(argv: Optional[List[str]] = None) -> int:
    """``gecco train``.  A clusters table without a ``type`` column reads as ``Unknown`` for every cluster (the table's
    default), so ``types.tsv`` then lists every cluster with no type names; GECCO itself fails on such a table."""
    from .crf import ClusterCRF

    args = build_parser().parse_args(argv)
    times: Dict[str, float] = {}
    t0 = time.perf_counter()
    random.seed(args.seed)
    np.random.seed(args.seed)
    genes = load_training_genes(args.genes, args.features, args.e_filter, args.p_filter)
    clusters = tables.ClusterTable.load(args.clusters)
    t1 = time.perf_counter()
    times["load"] = t1 - t0
    from .cv import cost_options

    crf = ClusterCRF(args.feature_type, "lbfgs", args.window_size, args.window_step, c1=args.c1, c2=args.c2,
                     **cost_options(getattr(args, "miss_cost", 0.0), getattr(args, "false_cost", 0.0)))
    device = int((crf.devices or [0])[0])
    join = join_clusters(genes, clusters, device=device)
    t2 = time.perf_counter()
    times["join"] = t2 - t1
    genes = [gene.with_probability(int(label)) for gene, label in zip(genes, join.labels.tolist())]
    t3 = time.perf_counter()
    times["label"] = t3 - t2
    crf.fit(genes, select=args.select, shuffle=args.shuffle, correction_method=args.correction, cpus=args.jobs)
    t4 = time.perf_counter()
    times["fit"] = t4 - t3
    write_model_dir(args.output_dir, crf, genes, clusters, join, device=device)
    times["write"] = time.perf_counter() - t4
    total = sum(times.values())
    print(f"train: {len(genes)} genes, {len(clusters)} clusters -> {args.output_dir} in {total:.3f} s ("
          + ", ".join(f"{k} {v:.3f} s" for k, v in times.items()) + ")", file=sys.stderr)
    return 0
