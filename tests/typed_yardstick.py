"""Yardstick of the all-label windowed marginals and of the typed cluster CRF's host rules: plain numpy over the CPU
oracle (``oracle.crf_oracle``), written for reading, not for speed.

Per window, ``oracle.marginals_seq`` runs on the window's state rows (``oracle.state_scores``; padding rows are zeros,
``delta // 2`` of them in front, as the reference centres a short contig); per gene the maximum over the windows covering
it is taken of every label's marginal and of the sum of the non-background marginals (label-index order).  Genes of
unpadded contigs shorter than the window hold NaN, genes no window covers 0.0, as in ``oracle.windowed_marginals``."""
import statistics

import numpy as np

from oracle import crf_oracle as orc


def windows_of(n, W, step, pad):
    """(rows in front, window starts in the padded frame) of a contig of n genes, or None when it is skipped."""
    if n < W:
        if not pad:
            return None
        front = (W - n) // 2
        return front, [0]
    return 0, list(range(0, n - W + 1, step))


def windowed_all(w, trans, contig_ptr, gene_ptr, attr_id, W, step=1, background=None, pad=True):
    """``(p_all [n, L], p_any [n] or None)``."""
    w = np.asarray(w, dtype=np.float64)
    L = w.shape[1]
    n = int(contig_ptr[-1])
    state = orc.state_scores(w, np.asarray(gene_ptr)[:n + 1], attr_id)
    p_all = np.zeros((n, L))
    p_any = np.zeros(n)
    for c in range(len(contig_ptr) - 1):
        g0, g1 = int(contig_ptr[c]), int(contig_ptr[c + 1])
        m = g1 - g0
        if m == 0:
            continue
        plan = windows_of(m, W, step, pad)
        if plan is None:
            p_all[g0:g1] = np.nan
            p_any[g0:g1] = np.nan
            continue
        front, starts = plan
        rows = np.zeros((max(m, W), L))
        rows[front:front + m] = state[g0:g1]
        for s in starts:
            marg, _ = orc.marginals_seq(rows[s:s + W], trans)
            lo, hi = max(s, front), min(s + W, front + m)  # the window's positions that are genes
            sl = slice(g0 + lo - front, g0 + hi - front)
            p_all[sl] = np.maximum(p_all[sl], marg[lo - s:hi - s])
            if background is not None:
                any_ = np.zeros(hi - lo)
                for l in range(L):
                    if l != background:
                        any_ = any_ + marg[lo - s:hi - s, l]
                p_any[sl] = np.maximum(p_any[sl], any_)
    return p_all, (p_any if background is not None else None)


def type_probabilities(p_all, label_types, types):
    """The cluster's probability of every type: min(1, statistics.mean over its genes of the sum, in label order, of the
    columns whose label contains the type)."""
    out = {}
    for t in types:
        v = [0.0] * len(p_all)
        for l, names in enumerate(label_types):
            if t in names:
                v = [a + float(b) for a, b in zip(v, p_all[:, l])]
        out[t] = min(1.0, statistics.mean(v))
    return out
