"""Marginals given a region and knock-out contributions in numpy, log space: the independent yardstick of
``gecco_crf_span_conditionals`` (tests/test_gpu_conditionals.py), pinned on path enumeration by tests/test_conditionals_host.py.

Everything is ``tests.constrained_reference.marginals`` on a table of item scores of ONE sequence (``-inf`` at disallowed
pairs): the conditional marginals are its marginals on the scores with ``-inf`` outside the set inside the span, and a
contribution is the difference of two log-probabilities of the region, log Z_E - log Z before the change and after it, every
log Z from that function -- the input is changed and scored again, the identity the product uses is not.  It shares no code
with the product."""
import numpy as np

from tests import constrained_reference as cr
from tests.train_objective_partial import mask_matrix


def restricted(score, b, e, mask):
    """The scores of one sequence with ``-inf`` outside the set ``mask`` at the items [b, e)."""
    out = np.array(score, dtype=np.float64, copy=True)
    inside = mask_matrix(np.array([mask], dtype=np.uint32), out.shape[1])[0]
    out[b:e, ~inside] = -np.inf
    return out


def _logz(score, trans):
    """(marginals, log Z) of one sequence; (None, -inf) when an item allows no label (no path)."""
    if np.any(np.all(np.isneginf(score), axis=1)):
        return None, -np.inf
    marg, logz = cr.marginals(np.array([0, len(score)]), score, trans)
    return marg, float(logz[0])


def region(score, trans, b, e, mask):
    """(cond [T, L], log Z_E, log Z): the marginals given that every item of [b, e) carries a label of the set, zeros where the
    region is impossible (log Z_E = -inf)."""
    _, logz = _logz(score, trans)
    cond, logze = _logz(restricted(score, b, e, mask), trans)
    return (np.zeros_like(score) if cond is None else cond), logze, logz


def bound_of(logze, logz):
    """The span tests' bound of one region log-probability log Z_E - log Z."""
    return 1e-10 * ((max(1.0, abs(logze)) if np.isfinite(logze) else 1.0) + max(1.0, abs(logz)))


def contribution(score, trans, b, e, mask, t, delta, base=None):
    """(log P(E | x) - log P(E | x with ``delta`` [L] added to the scores of item t), its bound): both log-probabilities from
    scoring again, the bound the sum of the two log-probabilities' own.  ``delta = None``: the item's scores are removed (0
    under every allowed label).  (0.0, bound) where the region is impossible.  ``base``: ``region``'s (log Z_E, log Z) of the
    unchanged scores, when the caller has them."""
    logze, logz = region(score, trans, b, e, mask)[1:] if base is None else base
    changed = np.array(score, dtype=np.float64, copy=True)
    finite = np.isfinite(changed[t])
    changed[t, finite] = 0.0 if delta is None else changed[t, finite] + np.asarray(delta, dtype=np.float64)[finite]
    _, logze2, logz2 = region(changed, trans, b, e, mask)
    bound = bound_of(logze, logz) + bound_of(logze2, logz2)
    if not np.isfinite(logze):
        return 0.0, bound
    return (logze - logz) - (logze2 - logz2), bound


def identity(marg_t, cond_t, delta):
    """log sum_l marg_t(l) e^{delta_l} - log sum_l cond_t(l) e^{delta_l}, each over the labels with mass, shifted by its largest
    delta: what the product computes from its two rows (here for the test of the identity against scoring again)."""
    delta = np.asarray(delta, dtype=np.float64)

    def side(p):
        keep = p > 0.0
        top = delta[keep].max()
        return top + np.log(np.sum(p[keep] * np.exp(delta[keep] - top)))

    return side(np.asarray(marg_t)) - side(np.asarray(cond_t))


def enumerate_region(score, trans, b, e, mask):
    """(cond [T, L], log P(E | x)) of one short sequence from every path."""
    logz, _, _, _ = cr.enumerate_paths(score, trans)
    sc = restricted(score, b, e, mask)
    if np.any(np.all(np.isneginf(sc), axis=1)):
        return np.zeros_like(score), -np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        logze, cond, _, _ = cr.enumerate_paths(sc, trans)
    if not np.isfinite(logze):
        return np.zeros_like(score), -np.inf
    return cond, logze - logz
