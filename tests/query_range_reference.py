"""The lattice queries on the planted transition families (tests/lattice_range_families.py): the query lists, the yardsticks and
the floor rule shared by tests/test_query_range_host.py (which pins every yardstick on path enumeration on these very models)
and tests/test_gpu_query_range.py (which holds the device to them).  It shares no code with the product.

The device uploads exp(trans); an entry of -2000 (families b and c) arrives as an exact 0.0, i.e. as a transition that does not
exist.  The five queries that read the stored linear-space vectors (spans, edges, runs, conditionals, sampling) are therefore
judged on ``fam.exp_zero(trans)``, the matrix with -inf in those places.

* The log-valued yardsticks (spans, runs, the conditionals' logp and knock-outs) are formed here on ``exp_zero(trans)`` with the
  log-sum-exps of tests/runs_reference.py, which take rows that are -inf throughout; the yardsticks of tests/test_gpu_spans.py
  and tests/conditionals_reference.py form -inf - -inf there.  The bounds are theirs, to the letter.
* The probability-valued yardsticks (``edges_reference``, ``sampling_reference``, the conditional marginals where the region
  has a path) take the RAW matrix: a term of relative weight e^-2000 is an exact 0.0 in a double sum, so both matrices give the
  same numbers; tests/test_query_range_host.py holds them to enumeration on ``exp_zero(trans)``.

Under a uniform shift of the transitions (families a, g, and the shifted models of d' and m) the distribution is the unshifted
model's EXACTLY (the families' grid), so ONE yardstick per (label count, distribution) judges all of them, as in
tests/test_gpu_lattice_range.py; the host test computes the shifted models' own yardsticks and holds the two together.

The floor rule.  Entries of a log-valued query with yardstick >= -700 or = -inf are ORDINARY and judged by the
query's own check function, unchanged.  Entries below -790 are DEEP: crf_runs.hip reads the complement's stored linear alpha,
which cannot hold e^-800 next to 1, so for runs a deep entry may come back -inf, or finite within its bound -- never NaN, above
0, or finite outside the bound.  Spans and the conditionals' logp stay strict.  [-790, -700) is empty in every yardstick."""
import functools

import numpy as np

from tests import constrained_reference as cr
from tests import lattice_range_families as fam
from tests import runs_reference as rr
from tests import train_objective_partial as tp

NINF = -np.inf
ORDINARY, DEEP = -700.0, -790.0
KEYS = ("log_anchor", "log_start", "log_start_beyond", "log_end", "log_end_beyond")
REACH = 64


# ---------------------------------------------------------------- the distributions
def canon(family, key):
    """The model whose distribution a query model has: a uniform shift changes nothing (module docstring)."""
    if family in ("a", "g"):
        return ("a", "base")
    if family in ("d'", "m"):
        return (family, "base")
    return (family, key)


def model(L, family, key):
    """fam.query_model, with ("a", "base") the unshifted base model."""
    return fam.query_model(L, family, key)


@functools.lru_cache(maxsize=None)
def scores(L, leaders, lengths=fam.QUERY_LENGTHS):
    cptr, gptr, attr = fam.query_batch(L, leaders, lengths)
    w = fam.leader_weights(L) if leaders == "d" else fam.mid_weights(L) if leaders == "m" else fam.base(L)[0]
    score = cr.masked_scores(gptr, attr, None, w, tp.full_masks(int(cptr[-1]), L))
    score.setflags(write=False)
    return score


def contig(score, cptr, c):
    return score[int(cptr[c]):int(cptr[c + 1])]


# ---------------------------------------------------------------- the query lists
def label_sets(L):
    """{0}, {1}, {0, 1}, {L - 1}, {0, 2}, all but {0, 1}: the proper, non-empty ones, without repeats."""
    full = (1 << L) - 1
    out = []
    for m in (1, 2, 3, 1 << (L - 1), 5 & full, full & ~3):
        if 0 < m < full and m not in out:
            out.append(m)
    return out


def _rand_set(rng, L):
    m = 0
    for y in range(L):
        if rng.random() < 0.6:
            m |= 1 << y
    return m or 1 << int(rng.integers(0, L))


def special_stretches(T):
    """The item ranges [b, e) of a T-item contig that a leader family marks: d's runs, and m's one item."""
    out = [r for r in fam.leader_runs(T) if r[1] > r[0]]
    if fam.mid_item(T) >= 0:
        out.append((fam.mid_item(T), fam.mid_item(T) + 1))
    return out


@functools.lru_cache(maxsize=None)
def spans(L):
    """Spans over fam.QUERY_LENGTHS: sixteen whose first and last item take every phase mod 4 on each of the contigs of 9, 33,
    65 and 129 items (the `_phase_spans` of tests/test_gpu_lattice_range.py), random sets; every short contig whole; spans
    that cover a leader stretch and spans that straddle its two ends, under the sets of label_sets; the 129-item contig under
    the full set (exactly 0.0); the first six again (duplicate queries)."""
    rng = np.random.default_rng(7600 + L)
    full = (1 << L) - 1
    out = []
    for T in (9, 33, 65, 129):
        c = fam.QUERY_LENGTHS.index(T)
        for rb in range(4):
            for re in range(4):
                b = rb + (4 * ((rb + re) % 2) if T > 9 else 0)
                lasts = [x for x in range(b, T) if x % 4 == re]
                last = lasts[-1] if (rb + re) % 2 else lasts[len(lasts) // 2]
                out.append((c, b, last + 1, _rand_set(rng, L)))
    sets = label_sets(L)
    k = 0
    for c, T in enumerate(fam.QUERY_LENGTHS):
        if T == 0:
            continue
        out.append((c, 0, T, sets[k % len(sets)]))
        out.append((c, 0, T, full))
        k += 1
        for b, e in special_stretches(T):
            for lo, hi in ((b, e), (max(b - 2, 0), min(b + 2, T)), (max(e - 2, 0), min(e + 2, T)), (max(b - 1, 0), min(e + 1, T))):
                if lo < hi:
                    out.append((c, lo, hi, sets[k % len(sets)]))
                    k += 1
    # a seeded mix, half of it short spans: under d' a short span inside a plain stretch, or inside a leader run under a set
    # that holds both leaders, is ordinary, and most others are deep
    long_ones = [c for c, T in enumerate(fam.QUERY_LENGTHS) if T >= 7]
    for i in range(200):
        c = long_ones[i % len(long_ones)]
        T = fam.QUERY_LENGTHS[c]
        b = int(rng.integers(0, T))
        e = min(T, b + 1 + int(rng.integers(0, 4 if i % 2 else T)))
        out.append((c, b, e, sets[(i // 2) % len(sets)] if i % 4 else _rand_set(rng, L)))
    out = [s for i, s in enumerate(out) if s not in out[:i]]
    return tuple(out + out[:6])


@functools.lru_cache(maxsize=None)
def anchors(L):
    """Anchors at both ends, the middle, item 10 and T - 5 of every contig, each under three of the sets of label_sets in
    rotation (every set meets every kind of place); the first four again."""
    sets = label_sets(L)
    out, k = [], 0
    for c, T in enumerate(fam.QUERY_LENGTHS):
        for a in sorted({x for x in (0, T - 1, T // 2, 10, T - 5) if 0 <= x < T}):
            for j in range(min(3, len(sets))):
                out.append((c, a, sets[(k + j) % len(sets)]))
            k += 1
    return tuple(out + out[:4])


@functools.lru_cache(maxsize=None)
def closed_runs(L):
    """Closed runs: the spans of `spans` whose set is proper, and every stretch of special_stretches under every set."""
    full = (1 << L) - 1
    out = [s for s in spans(L) if s[3] != full]
    for c, T in enumerate(fam.QUERY_LENGTHS):
        for b, e in special_stretches(T):
            out += [(c, b, e, m) for m in label_sets(L)]
    return tuple(s for i, s in enumerate(out) if s not in out[:i])


def edge_sets(L):
    """The two sets of tests/test_gpu_lattice_range.py: the even labels, and the last label alone."""
    return (sum(1 << y for y in range(0, L, 2)), 1 << (L - 1))


# ---------------------------------------------------------------- log Z that takes -inf transitions
def log_z(X, trans):
    """log Z of one sequence of masked scores in unscaled log space; -inf where no path exists, whether an item is left
    without a label or the transitions that would connect the labels do not exist."""
    la = X[0]
    for t in range(1, len(X)):
        la = rr._lse_rows((la[:, None] + trans).T) + X[t]
    return rr._lse(la)


def restricted(X, b, e, mask):
    Y = np.array(X, dtype=np.float64, copy=True)
    Y[b:e, ~rr.inside_of(mask, X.shape[1])] = NINF
    return Y


def log_bound(inner, logz):
    """The span tests' bound of log Z_A' - log Z_A (tests/test_gpu_spans.py::_yardstick)."""
    return 1e-10 * ((max(1.0, abs(inner)) if np.isfinite(inner) else 1.0) + max(1.0, abs(logz)))


def span_yardstick(cptr, score, trans, span_list):
    """(ref, bound) of every span: ``_yardstick`` of tests/test_gpu_spans.py with `log_z` for its two log Z."""
    ref, bound = np.zeros(len(span_list)), np.zeros(len(span_list))
    memo, whole = {}, {}
    for q, (c, b, e, m) in enumerate(span_list):
        X = contig(score, cptr, c)
        if c not in whole:
            whole[c] = log_z(X, trans)
        if (c, b, e, m) not in memo:
            memo[(c, b, e, m)] = log_z(restricted(X, b, e, m), trans)
        inner = memo[(c, b, e, m)]
        ref[q], bound[q] = inner - whole[c], log_bound(inner, whole[c])
    return ref, bound


class Regions:
    """The regions of one lattice for ``_check_cond`` / ``_check_contributions`` of tests/test_gpu_conditionals.py: the
    interface of that file's ``Yardstick`` on a transition matrix that may hold -inf."""

    def __init__(self, csr, w, score, trans, raw):
        self.cptr, self.gptr, self.attr = csr
        self.values, self.w, self.trans, self.raw, self.score = None, w, trans, raw, score
        self.memo, self.knocked = {}, {}

    def contig(self, c):
        return contig(self.score, self.cptr, c)

    def _region(self, X, b, e, m):
        """(cond, log Z_E, log Z) of conditionals_reference.region.  Where the region has a path, cond is cr.marginals' (every
        vector shifted by its own log-sum-exp: 1e-12 absolute needs that at scores of 800 per item) on the RAW matrix, which
        differs from the exp_zero one by terms of relative weight e^-2000, exact zeros in a double sum."""
        logz = log_z(X, self.trans)
        Y = restricted(X, b, e, m)
        logze = log_z(Y, self.trans)
        if not np.isfinite(logze):
            return np.zeros_like(X), NINF, logz
        return cr.marginals(np.array([0, len(Y)]), Y, self.raw)[0], logze, logz

    def region(self, c, b, e, m):
        if (c, b, e, m) not in self.memo:
            self.memo[(c, b, e, m)] = self._region(self.contig(c), b, e, m)
        return self.memo[(c, b, e, m)]

    def knock_out(self, c, b, e, m, t, k=None):
        """(contribution, bound) of conditionals_reference.contribution: the changed input scored again."""
        if (c, b, e, m, t, k) not in self.knocked:
            _, logze, logz = self.region(c, b, e, m)
            changed = np.array(self.contig(c), dtype=np.float64, copy=True)
            finite = np.isfinite(changed[t])
            changed[t, finite] = 0.0 if k is None else changed[t, finite] - self.w[self.attr[k]][finite]
            logz2 = log_z(changed, self.trans)
            logze2 = log_z(restricted(changed, b, e, m), self.trans)
            bound = log_bound(logze, logz) + log_bound(logze2, logz2)
            self.knocked[(c, b, e, m, t, k)] = (0.0 if not np.isfinite(logze) else (logze - logz) - (logze2 - logz2), bound)
        return self.knocked[(c, b, e, m, t, k)]


def anchor_yardstick(cptr, score, trans, anchor_list, reach=REACH):
    """(values, bounds) of the anchors by ``runs_reference.anchor_direct``, stacked under the product's keys."""
    val, bnd = ({k: [] for k in KEYS} for _ in range(2))
    memo, fb = {}, {}
    for c, a, m in anchor_list:
        if c not in fb:
            fb[c] = rr.forward_backward(contig(score, cptr, c), trans)
        if (c, a, m) not in memo:
            memo[(c, a, m)] = rr.anchor_direct(contig(score, cptr, c), trans, a, m, reach, fb[c])
        v, tot, logz = memo[(c, a, m)]
        for k in KEYS:
            val[k].append(v[k])
            bnd[k].append(rr.bound(tot[k], logz))
    return tuple({k: np.array(x[k], dtype=np.float64) for k in KEYS} for x in (val, bnd))


def run_yardstick(cptr, score, trans, run_list):
    """(ref, bound) of the closed runs by ``runs_reference.joint_row_direct``."""
    rows, fb = {}, {}
    ref, bnd = np.zeros(len(run_list)), np.zeros(len(run_list))
    for q, (c, b, e, m) in enumerate(run_list):
        if c not in fb:
            fb[c] = rr.forward_backward(contig(score, cptr, c), trans)
        if (c, b, m) not in rows:
            rows[(c, b, m)] = rr.joint_row_direct(contig(score, cptr, c), trans, b, m, fb[c])
        val, tot, logz = rows[(c, b, m)]
        ref[q], bnd[q] = val[e - 1 - b], rr.bound(tot[e - 1 - b], logz)
    return ref, bnd


# ---------------------------------------------------------------- one yardstick per (label count, distribution)
def _frozen(x):
    for v in (x.values() if isinstance(x, dict) else x if isinstance(x, tuple) else (x,)):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, (dict, tuple)):
            _frozen(v)
    return x


def lattice(L, family, key):
    """(cptr, masked scores, exp_zero(trans), raw trans) of a query model."""
    w, trans, leaders = model(L, family, key)
    return fam.query_batch(L, leaders)[0], scores(L, leaders), fam.exp_zero(trans), trans


@functools.lru_cache(maxsize=None)
def span_reference(L, family, key):
    cptr, score, tz, _ = lattice(L, family, key)
    return _frozen(span_yardstick(cptr, score, tz, list(spans(L))))


@functools.lru_cache(maxsize=None)
def runs_reference(L, family, key):
    """((anchor values, anchor bounds), (run values, run bounds))."""
    cptr, score, tz, _ = lattice(L, family, key)
    return _frozen((anchor_yardstick(cptr, score, tz, list(anchors(L))), run_yardstick(cptr, score, tz, list(closed_runs(L)))))


@functools.lru_cache(maxsize=None)
def regions(L, family, key):
    w, trans, leaders = model(L, family, key)
    return Regions(fam.query_batch(L, leaders), w, scores(L, leaders), fam.exp_zero(trans), trans)


@functools.lru_cache(maxsize=None)
def edge_reference(L, family, key):
    from tests import edges_reference as er

    cptr, score, _, raw = lattice(L, family, key)
    return _frozen(er.edge_posteriors(cptr, score, raw, edge_sets(L)))


@functools.lru_cache(maxsize=None)
def marginal_reference(L, family, key):
    cptr, score, _, raw = lattice(L, family, key)
    return _frozen(cr.marginals(cptr, score, raw))


# ---------------------------------------------------------------- the floor rule
def classes(ref):
    """(ordinary, deep) boolean arrays of a log-valued yardstick; nothing may lie in the gap between them."""
    ref = np.asarray(ref, dtype=np.float64)
    ordinary = (ref >= ORDINARY) | np.isneginf(ref)
    deep = (ref < DEEP) & np.isfinite(ref)
    assert not np.isnan(ref).any(), "NaN in a yardstick"
    assert np.all(ordinary | deep), f"{int((~(ordinary | deep)).sum())} yardstick entries in [{DEEP}, {ORDINARY})"
    return ordinary, deep


def floor_compare(tag, got, ref, bound, compare):
    """The floor rule for runs: the ordinary entries under `compare` (tests/test_gpu_runs.py::_compare, unchanged); a deep
    entry is -inf, or finite and within its bound.  Returns (worst ratio, ordinary finite, deep finite, deep -inf)."""
    got, ref, bound = (np.asarray(x, dtype=np.float64) for x in (got, ref, bound))
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    ordinary, deep = classes(ref)
    assert not np.any(np.isnan(got)), f"{tag}: NaN"
    assert np.all(got <= 0.0), f"{tag}: a log-probability above 0"
    ratio, n = compare(tag, got[ordinary], ref[ordinary], bound[ordinary])
    g, r, b = got[deep], ref[deep], bound[deep]
    kept = np.isfinite(g)
    assert np.all(kept | np.isneginf(g)), f"{tag}: a deep entry that is neither finite nor -inf"
    off = float((np.abs(g[kept] - r[kept]) / b[kept]).max(initial=0.0))
    assert off <= 1.0, f"{tag}: a deep entry came back finite and {off:.3g} of its bound away from the yardstick"
    return max(ratio, off), n, int(kept.sum()), int((~kept).sum())
