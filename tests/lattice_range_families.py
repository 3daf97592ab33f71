"""Planted transition families for the whole-contig sum-product pass at its transition-range guards: the models and batches of
tests/test_lattice_range_host.py (which shows that the log-space yardstick is right on them) and tests/test_gpu_lattice_range.py
(which holds every whole-contig arrangement to that yardstick on them).  Builders only: no reference arithmetic lives here.

The guards (crf_plan.cpp) read the transition weights alone:

* ``rows_rescale_period = 4 max|trans| < 600 ? 4 : 1`` -- four un-normalised steps of gl_marginals_wave / gl_chunk_rows_mfma;
* ``raw_fold = 8 (max trans - min trans) < 600`` -- eight un-renormalised 2 x 2 factors per lane of the 2-label scan;
* ``exp(trans)`` uploaded raw for the any-L kernels, accepted while -700 <= max trans <= 700.

One base model per label count: state weights N(0, 1) and a transition matrix N(0, 1) rounded to multiples of 2^-20.  On that
grid ``trans + c`` is exact for every shift c used here (c itself is on the grid and |trans + c| < 2^11, 31 significant bits),
so a shifted model is the base model's distribution EXACTLY, not up to the rounding of 30 000 sums, and max|trans + c| is the
planted figure to the bit.

The second half of the file plants the window kernels' guard (``gen_small_ok``: spread (W - 1) < 600) for
tests/test_window_range_host.py and tests/test_gpu_window_range.py: the spread of the base matrix set to the last grid value
inside the guard or the first beyond it, in four shapes, and batches of contigs around a window of W items.

The third part plants the models of the lattice queries (tests/test_query_range_host.py, tests/test_gpu_query_range.py): family g,
the guard's own figures (max trans at exactly +700 and -700, and one grid step beyond either); family m, one mid leader of 150;
family d', the alternating 800-leaders on the base and the +-600 transitions; and ``exp_zero``, the matrix the device uploads."""
import functools

import numpy as np

A = 12                       # attributes; the last two are family d's leaders
LEAD0, LEAD1 = A - 2, A - 1  # the attribute that makes label 0 / label 1 lead by 800
GRID = 2.0 ** -20
LABELS = (2, 3, 8, 9, 17, 32)
LENGTHS = (0, 1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129, 300)
LONG_LENGTHS = (2049, 65, 0, 1)  # one contig past kGenLongContig = 2048: chunks of 64 genes

SHIFTS_A = ("under+", "at+", "under-", "at-", "+600", "-600")
FAR_B = (74.9, 75.1, 149.0, 151.0, 600.0, 2000.0)
FORBID_C = ("row", "column", "diagonal", "row-150")
LEADERS_D = (74.9, 75.1)
SHIFTS_E = (800.0, -800.0)
FORBIDDEN = -2000.0


@functools.lru_cache(maxsize=None)
def base(L):
    """(state weights [A, L], transitions [L, L]) of the base model; the two leader attributes weigh nothing here."""
    rng = np.random.default_rng(7300 + L)
    w = rng.normal(0.0, 1.0, size=(A, L))
    w[LEAD0:] = 0.0
    trans = np.round(rng.normal(0.0, 1.0, size=(L, L)) / GRID) * GRID
    w.setflags(write=False)
    trans.setflags(write=False)
    return w, trans


def shift_of(L, which):
    """Family a / e: the uniform shift c.  "under+" / "at+": max|trans + c| = 150 - 2^-20 / = 150 with c > 0 (the largest
    entry lands there); "under-" / "at-" with c < 0 (the smallest entry); "+600" / "-600" / a number: that shift."""
    _, trans = base(L)
    if which in ("under+", "at+"):
        return 150.0 - float(trans.max()) - (GRID if which == "under+" else 0.0)
    if which in ("under-", "at-"):
        return -150.0 - float(trans.min()) + (GRID if which == "under-" else 0.0)
    return float(which)


def shifted(L, which):
    """Family a / e: (trans + c, c); the sum is exact (module docstring)."""
    c = shift_of(L, which)
    out = base(L)[1] + c
    assert np.array_equal(out - c, base(L)[1]), "the shift is exact on the grid"
    return out, c


def far_cell(L):
    """The off-diagonal entry family b moves: (0, 1), or (1, 0) where (0, 1) holds the base matrix's maximum."""
    _, trans = base(L)
    return (1, 0) if np.unravel_index(int(np.argmax(trans)), trans.shape) == (0, 1) else (0, 1)


def far_entry(L, s):
    """Family b: one off-diagonal entry at max - s."""
    out = base(L)[1].copy()
    out[far_cell(L)] = out.max() - s
    return out


def forbidden(L, what):
    """Family c: (trans, dead) with -2000 in a whole row (label L - 1 is followed by nothing: legal at a contig's last item
    only), a whole column (label 0 follows nothing: legal at the first item only) or the whole diagonal (no self-transition).
    ``dead(T)`` is the boolean [T, L] table of the (item, label) pairs that no path of a T-item contig goes through.
    "row-150": the row in the matrix shifted to max|trans| just under 150 on the negative side -- the other rows of a chunk's
    transfer matrix then carry exponents near -7000 next to the zero row's."""
    out = (shifted(L, "under-")[0] if what.endswith("-150") else base(L)[1]).copy()
    what = what.split("-")[0]
    if what == "row":
        out[L - 1, :] = FORBIDDEN

        def dead(T):
            d = np.zeros((T, L), dtype=bool)
            d[:max(T - 1, 0), L - 1] = True
            return d
    elif what == "column":
        out[:, 0] = FORBIDDEN

        def dead(T):
            d = np.zeros((T, L), dtype=bool)
            d[1:, 0] = True
            return d
    else:
        out[np.arange(L), np.arange(L)] = FORBIDDEN

        def dead(T):
            return np.zeros((T, L), dtype=bool)
    return out, dead


def leader_weights(L):
    """Family d: the base state weights with the two leader attributes switched on: LEAD0 gives label 0, LEAD1 label 1 a lead of
    at least 800 over every other label whatever else an item carries (the `special` attribute of
    tests/test_gpu_spans.py::test_a_label_outside_the_set_that_leads_by_800)."""
    w = base(L)[0].copy()
    lead = 800.0 + 2.0 * 4 * np.abs(w).max()  # (an item carries at most 4 other attributes)
    w[LEAD0, 0] = lead
    w[LEAD1, 1] = lead
    return w


def leader_runs(T):
    """Family d: the item ranges [b, e) of a T-item contig whose items carry alternately LEAD0 and LEAD1: the whole contig up
    to 33 items; beyond, 24 items from item 5 (across the 8-item lane folds at 8, 16 and 24) and the last 16 items."""
    if T <= 33:
        return [(0, T)]
    return [(5, 29), (T - 16, T)]


@functools.lru_cache(maxsize=None)
def batch(L, lengths=LENGTHS, leaders=False, whole=False):
    """(contig_ptr, gene_ptr, attr_id) over `lengths`: 0 to 4 of the ten plain attributes per item, and with `leaders` family
    d's alternating leader attribute on the items of leader_runs (`whole`: on every item of every contig)."""
    rng = np.random.default_rng(7400 + L)
    cptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    rows = [list(rng.integers(0, LEAD0, size=int(d))) for d in rng.integers(0, 5, size=int(cptr[-1]))]
    if leaders:
        for g0, T in zip(cptr[:-1].tolist(), lengths):
            for b, e in ([(0, T)] if whole else leader_runs(T)):
                for t in range(b, e):
                    rows[g0 + t].append(LEAD0 if (t - b) % 2 == 0 else LEAD1)
    gptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    attr = np.array([a for r in rows for a in r], dtype=np.int32)
    for x in (cptr, gptr, attr):
        x.setflags(write=False)
    return cptr, gptr, attr


def model_of(L, family, key):
    """(state weights, transitions, leaders) of a planted model: family "base", "a" (key in SHIFTS_A), "b" (s in FAR_B), "c"
    (key in FORBID_C), "d" (s in LEADERS_D: the leaders and family b's entry at max - s) or "e" (a shift in SHIFTS_E)."""
    w, trans = base(L)
    if family == "base":
        return w, trans, False
    if family in ("a", "e"):
        return w, shifted(L, key)[0], False
    if family == "b":
        return w, far_entry(L, key), False
    if family == "c":
        return w, forbidden(L, key)[0], False
    assert family == "d"
    return leader_weights(L), far_entry(L, key), True


def figures(trans):
    """What the guards read: (max|trans|, max trans - min trans, max trans), and the sides they land on."""
    amax, spread, tmax = float(np.abs(trans).max()), float(trans.max() - trans.min()), float(trans.max())
    return dict(amax=amax, spread=spread, tmax=tmax, period=4 if 4.0 * amax < 600.0 else 1, raw_fold=1 if spread * 8.0 < 600.0 else 0,
                in_range=-700.0 <= tmax <= 700.0)


# ---------------------------------------------------------------- the window kernels' guard (tests/test_gpu_window_range.py)
# gen_small_ok (crf_general_windowed.hip): the un-normalised window tiers run W - 1 steps on exp(trans - max trans) while
# ``(max trans - min trans) * (W - 1) < 600``; everything else takes the scaled lane-group tier.
WINDOWS = (2, 5, 20, 32)
SPREAD_SHAPES = ("one", "sticky", "restless", "column")


def guard_spread(W):
    """The largest grid value s with ``s * (W - 1) < 600.0`` in double arithmetic; s + 2^-20 is the first grid value on the
    other side."""
    s = np.floor(600.0 / (W - 1) / GRID) * GRID
    while not s * float(W - 1) < 600.0:
        s -= GRID
    while (s + GRID) * float(W - 1) < 600.0:
        s += GRID
    assert s * float(W - 1) < 600.0 and not (s + GRID) * float(W - 1) < 600.0
    return float(s)


def spread_model(L, shape, s):
    """The base matrix clipped from below at max - s, with max - min at exactly s in one of four shapes: "one", one
    off-diagonal entry at max - s (family b's cell); "sticky", the diagonal at max and every other entry at max - s (every
    change of label costs s); "restless", the diagonal at max - s; "column", every transition into label 0 at max - s.  The
    maximum is planted again at (0, 1) where the shape removed it."""
    trans = base(L)[1]
    hi = float(trans.max())
    out = np.maximum(trans, hi - s)
    diag = np.arange(L)
    if shape == "one":
        out[far_cell(L)] = hi - s
    elif shape == "sticky":
        out[:] = hi - s
        out[diag, diag] = hi
    elif shape == "restless":
        out[diag, diag] = hi - s
    else:
        assert shape == "column"
        out[:, 0] = hi - s
    if out.max() != hi:
        out[0, 1] = hi
    assert out.max() == hi and out.min() == hi - s and float(out.max() - out.min()) == s, "the spread is s to the bit"
    return out


def window_lengths(W):
    """Contigs around a window of W items: padded (or, without padding, skipped) ones, one across a wave's 64 lanes, one
    across a tile of 256 window starts, empty ones at both ends."""
    return (0, 1, W - 1, W, W + 1, 2 * W + 3, 65, 300, 0)


def window_batch(L, W, leaders=False):
    """(contig_ptr, gene_ptr, attr_id) over window_lengths(W); `leaders`: family d's alternating leader attribute on every item."""
    return batch(L, window_lengths(W), leaders, whole=leaders)


def leader_of(csr):
    """Per item the label that a leader attribute makes lead (0 or 1), or -1."""
    cptr, gptr, attr = csr
    out = np.full(int(cptr[-1]), -1, dtype=np.int64)
    for g in range(len(out)):
        mine = attr[gptr[g]:gptr[g + 1]]
        if (mine == LEAD0).any():
            out[g] = 0
        elif (mine == LEAD1).any():
            out[g] = 1
    return out


def forbid_the_leader(L, csr):
    """uint32 masks that allow every label but the one that leads on the item."""
    lead = leader_of(csr)
    full = np.full(len(lead), (1 << L) - 1, dtype=np.uint64)
    full[lead >= 0] &= ~(np.uint64(1) << lead[lead >= 0].astype(np.uint64))
    return full.astype(np.uint32)


def small_tier_ok(L, W, trans, all_labels=False):
    """What the plan's guard computes: the un-normalised tier takes this (label count, window, matrix)."""
    wmax = 32 if (L <= 4 or (L > 8 and not all_labels)) else 20
    if all_labels and L > 8:
        return False
    return bool(2 <= L <= 32 and 1 <= W <= wmax and float(trans.max() - trans.min()) * float(W - 1) < 600.0)


def window_model(L, key):
    """(state weights, transitions, leaders) of a model of the window tests: ("edge", shape, W, side, leaders) is the spread
    shape at guard_spread(W) (side 0) or one grid step beyond (side 1), with or without the leaders; (family, key) with a
    family of model_of is that model."""
    if key[0] == "edge":
        _, shape, W, side, leaders = key
        return (leader_weights(L) if leaders else base(L)[0]), spread_model(L, shape, guard_spread(W) + side * GRID), leaders
    return model_of(L, key[0], key[1])


# ---------------------------------------------------------------- the lattice queries (tests/test_gpu_query_range.py)
# The nine entries behind run_lattice (crf_plan.cpp) are held to every family the pass accepts.  QUERY_LENGTHS: an empty contig,
# contigs shorter than any run, both sides of the 8-item lane fold and of a 64-lane wave, one contig across two waves.
QUERY_LENGTHS = (0, 1, 2, 3, 7, 8, 9, 33, 65, 129)
QUERY_LABELS = (2, 3, 8, 9, 17, 32)
GUARD_G = ("at+700", "at-700")           # accepted: check_exp_trans_range takes -700 <= max trans <= 700
BEYOND_G = ("beyond+700", "beyond-700")  # refused: one grid step further out
FAR_QUERY_B = (74.9, 151.0, 2000.0)
LEADERS_DP = ("base", "+600", "-600")
MID_M = ("base", "+600", "-600", "at+700", "at-700", "at+", "at-")  # (the last two: max|trans| = 150, the side run_posteriors takes)
QUERY_FAMILIES = {"a": SHIFTS_A, "g": GUARD_G, "b": FAR_QUERY_B, "c": FORBID_C, "d'": LEADERS_DP, "m": MID_M}
MID_LEAD = 150.0


def guard_shift(L, which):
    """Family g: the uniform shift that puts max trans at exactly +700 / -700 ("at+700" / "at-700"), or one grid step beyond."""
    tmax = float(base(L)[1].max())
    side = 1.0 if "+" in which else -1.0
    return side * 700.0 - tmax + (side * GRID if which.startswith("beyond") else 0.0)


def shift_any(L, which):
    """(trans + c, c) for a key of family a, of family g or "base" (c = 0); the sum is exact on the grid."""
    c = 0.0 if which == "base" else guard_shift(L, which) if which in GUARD_G + BEYOND_G else shift_of(L, which)
    out = base(L)[1] + c
    assert np.array_equal(out - c, base(L)[1]), "the shift is exact on the grid"
    return out, c


def mid_weights(L):
    """Family m: the base state weights with LEAD0 giving label 0 a lead of at least 150 over every other label whatever else
    the item carries (leader_weights' construction: the lead plus 8 max|w|)."""
    w = base(L)[0].copy()
    w[LEAD0, 0] = MID_LEAD + 2.0 * 4 * np.abs(w).max()
    return w


def mid_item(T):
    """Family m: the one interior item of a contig of 7 or more items that carries the leader, or -1."""
    return T // 2 if T >= 7 else -1


@functools.lru_cache(maxsize=None)
def mid_batch(L, lengths=QUERY_LENGTHS):
    """batch(L, lengths) with LEAD0 appended to mid_item(T) of every contig, and to no other item."""
    cptr, gptr, attr = batch(L, lengths)
    rows = [list(attr[gptr[g]:gptr[g + 1]]) for g in range(int(cptr[-1]))]
    for g0, T in zip(cptr[:-1].tolist(), lengths):
        if mid_item(T) >= 0:
            rows[g0 + mid_item(T)].append(LEAD0)
    gptr2 = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    attr2 = np.array([a for r in rows for a in r], dtype=np.int32)
    for x in (gptr2, attr2):
        x.setflags(write=False)
    return cptr, gptr2, attr2


def query_model(L, family, key):
    """(state weights, transitions, leaders) of a model of the query tests; leaders is None, "d" (the alternating 800-leaders
    of leader_runs) or "m" (the mid leader).  Families a, b, c as model_of; g, d' and m move the base transitions by a uniform
    shift.  d' is never combined with family b's far entry."""
    if family in ("a", "g"):
        return base(L)[0], shift_any(L, key)[0], None
    if family in ("b", "c"):
        return model_of(L, family, key)[:2] + (None,)
    if family == "d'":
        return leader_weights(L), shift_any(L, key)[0], "d"
    assert family == "m"
    return mid_weights(L), shift_any(L, key)[0], "m"


def query_batch(L, leaders, lengths=QUERY_LENGTHS):
    """The CSR batch of a query model over `lengths`."""
    if leaders == "m":
        return mid_batch(L, lengths)
    return batch(L, lengths, leaders == "d")


def distinct_items(L, csr, w):
    """(csr, state weights) with one more attribute per item that no other item carries, first in its row, weights N(0, 1):
    items without attributes, or with equal ones, have equal score rows, and whole families of paths then tie exactly -- which a
    test that compares ranked paths (tests/test_gpu_kbest.py::accept) cannot take."""
    cptr, gptr, attr = csr
    n = int(cptr[-1])
    rows = [[A + g] + list(attr[gptr[g]:gptr[g + 1]]) for g in range(n)]
    gptr2 = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    attr2 = np.array([a for r in rows for a in r], dtype=np.int32)
    w2 = np.concatenate([w, np.random.default_rng(7900 + L).normal(0.0, 1.0, size=(n, L))], axis=0)
    return (cptr, gptr2, attr2), w2


def query_shift(L, family, key):
    """The uniform shift c by which a query model's transitions differ from its family's unshifted model (0 for b and c)."""
    return shift_any(L, key)[1] if family in ("a", "g", "d'", "m") else 0.0


RUNS_MAX_TRANS = 150.0


def runs_in_range(trans):
    """What plan_run_run_posteriors reads: the largest |transition weight| among those whose exp is not 0 is at most 150."""
    with np.errstate(under="ignore"):
        live = np.exp(trans) != 0.0
    return bool(np.abs(trans[live]).max(initial=0.0) <= RUNS_MAX_TRANS)


def exp_zero(trans):
    """The matrix with -inf wherever numpy.exp(trans) == 0.0: what the device uploads as exp(trans), back in log space."""
    with np.errstate(under="ignore"):
        dead = np.exp(trans) == 0.0
    return np.where(dead, -np.inf, trans)
