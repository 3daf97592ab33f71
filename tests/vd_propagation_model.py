"""Host model of the Viterbi workgroups' entering values (gecco_amd/csrc/crf_vd_short.hpp: vd_short_block) and planted
batches for it; shared by tests/test_vd_propagation_host.py and tests/test_gpu_vd_propagation.py.

The model restates, operation by operation, what a workgroup does up to the value that enters every lane: whole contigs
packed greedily into workgroups of at most 2048 genes (plan_ensure_seq), a lane's eight genes folded into one clamp map
(a, L, H), and then value propagation: a lane whose map is constant (L == H) knows the value that leaves it, any other
lane applies its map to its left neighbour's value, one lane of a run per step and at most RUN steps in front of the
barrier and behind it; a workgroup in which that does not reach every lane takes the scan of whole maps instead (the
"fallback").  The reference is the strictly sequential difference recursion (oracle_viterbi_delta's), gene by gene.

Batches here give gene g the attribute g alone with weights (0, d_g), so a gene's score difference is d_g itself."""
import numpy as np

from tests.helpers import _delta_step, _solve_sum, _ulp_step

TRANS2 = np.array([[2.669891070463728, -2.599571900486168], [-2.6019205422130995, 2.5683226020688488]])
LANES, GPL, RUN = 256, 8, 6  # kT, kGPL, kVdRun
BLOCK = LANES * GPL
PAD = 1e30  # kVdPad


def constants(trans):
    t00, t01, t10, t11 = (float(x) for x in np.asarray(trans, dtype=np.float64).ravel())
    return t01 - t11, t00 - t10, t11 - t00  # lo, hi, k


def pack_blocks(cptr):
    """first gene of every workgroup (+ the total): a contig that no longer fits closes the workgroup before it"""
    cptr = [int(x) for x in cptr]
    cblk, start = [0], 0
    for c in range(len(cptr) - 1):
        if cptr[c + 1] - start > BLOCK:
            start = cptr[c]
            cblk.append(start)
    cblk.append(cptr[-1])
    return cblk


def sequential_delta(d, cptr, trans):
    """Delta of every gene by the sequential recursion: clamp(Delta, lo, hi) + (k + d), a contig's first gene: d itself"""
    lo, hi, k = constants(trans)
    out = np.zeros(len(d))
    for c in range(len(cptr) - 1):
        D = 0.0
        for g in range(int(cptr[c]), int(cptr[c + 1])):
            D = float(d[g]) if g == cptr[c] else min(max(D, lo), hi) + (k + float(d[g]))
            out[g] = D
    return out


def labels_from_delta(delta, cptr, trans):
    """the labels these values decide (oracle_viterbi_delta's back-pointers and end label)"""
    lo, hi, _ = constants(trans)
    y = np.zeros(len(delta), dtype=np.int32)
    for c in range(len(cptr) - 1):
        g0, g1 = int(cptr[c]), int(cptr[c + 1])
        if g1 == g0:
            continue
        lab = 1 if delta[g1 - 1] > 0.0 else 0
        y[g1 - 1] = lab
        for g in range(g1 - 1, g0, -1):
            D = delta[g - 1]
            lab = (((1 if D > hi else 0) | (2 if D > lo else 0)) >> lab) & 1
            y[g - 1] = lab
    return y


def fold_block(d, first, trans):
    """the 256 lane maps of one workgroup: d, first = its 2048 positions (padding: PAD, first set)"""
    lo, hi, k = constants(trans)
    x = np.asarray(d, dtype=np.float64).reshape(LANES, GPL)
    f = np.asarray(first, dtype=bool).reshape(LANES, GPL)
    a = np.zeros(LANES)
    L = np.full(LANES, -np.inf)
    H = np.full(LANES, np.inf)
    for j in range(GPL):
        c = k + x[:, j]
        l2 = np.minimum(np.maximum(L, lo), hi) + c
        h2 = np.minimum(np.maximum(H, lo), hi) + c
        a = a + c
        L = np.where(f[:, j], x[:, j], l2)
        H = np.where(f[:, j], x[:, j], h2)
    return a, L, H


def _steps(a, L, H, v, known, lanes):
    """vd_propagate on one wave (`lanes`: its 64 lane indices): at most RUN steps"""
    for _ in range(RUN):
        todo = [i for i in lanes[1:] if not known[i] and known[i - 1]]
        if not todo:
            break
        new = {i: min(max(v[i - 1] + a[i], L[i]), H[i]) for i in todo}
        for i, val in new.items():
            v[i], known[i] = val, True


def propagate_block(a, L, H):
    """(entering value of every lane, fallback needed) as the workgroup computes them; the values are None when the
    workgroup takes the fallback"""
    known = list(L == H)
    v = [float(x) for x in L]
    bad = False
    for w in range(LANES // 64):
        lanes = list(range(64 * w, 64 * w + 64))
        _steps(a, L, H, v, known, lanes)
        kn = [known[i] for i in lanes]
        lead = kn.index(True) if True in kn else 64
        bad = bad or lead > (RUN if w else 0) or not all(kn[lead:])
    if bad:
        return None, True
    for w in range(1, LANES // 64):
        lanes = list(range(64 * w, 64 * w + 64))
        if not known[lanes[0]]:
            i = lanes[0]
            v[i], known[i] = min(max(v[i - 1] + a[i], L[i]), H[i]), True
            _steps(a, L, H, v, known, lanes)
    assert all(known)
    return np.array([0.0] + v[:-1]), False


def run_model(d, cptr, trans):
    """per workgroup: dict(g0, n, a, L, H, constant, din, fallback, seq_in, first) -- seq_in[i]: the sequential recursion's
    value entering lane i (nan where nothing enters: the lane's first position starts a contig or is padding)"""
    d = np.asarray(d, dtype=np.float64)
    n_all = int(cptr[-1])
    is_first = np.zeros(n_all + 1, dtype=bool)
    for c in range(len(cptr) - 1):
        if cptr[c + 1] > cptr[c]:
            is_first[int(cptr[c])] = True
    delta = sequential_delta(d, cptr, trans)
    cblk = pack_blocks(cptr)
    out = []
    for b in range(len(cblk) - 1):
        g0, n = cblk[b], cblk[b + 1] - cblk[b]
        x = np.full(BLOCK, PAD)
        f = np.ones(BLOCK, dtype=bool)
        x[:n] = d[g0:g0 + n]
        f[:n] = is_first[g0:g0 + n]
        a, L, H = fold_block(x, f, trans)
        din, fallback = propagate_block(a, L, H)
        seq_in = np.full(LANES, np.nan)
        for i in range(1, LANES):
            if GPL * i < n and not f[GPL * i]:
                seq_in[i] = delta[g0 + GPL * i - 1]
        out.append(dict(g0=g0, n=n, a=a, L=L, H=H, constant=(L == H), din=din, fallback=fallback, seq_in=seq_in,
                        first=f.reshape(LANES, GPL)))
    return out


def coarse_margin(n, wmax, tmax):
    """(4 n + 4) ulp(M) of a workgroup of n genes with one attribute each (vd_bound, vd_margin)"""
    M = n * 2.0 * wmax + (n + 2.0) * tmax
    return (4.0 * n + 4.0) * M * 2.0 ** -52


# ---- planted batches ---------------------------------------------------------------------------------------------------
def batch_from_d(d, lengths):
    """(w, cptr, gptr, attr): gene g carries attribute g alone, weights (0, d_g)"""
    d = np.asarray(d, dtype=np.float64)
    n = len(d)
    assert sum(lengths) == n
    w = np.zeros((n, 2))
    w[:, 1] = d
    cptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return w, cptr, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)


def lane_background(rng, n, trans=TRANS2):
    """Score differences that make EVERY 8-gene lane's map constant: the lane's first gene lies 20 beyond the recursion's
    interval on a random side (both tracks of the fold leave [lo, hi] together and are clamped to the same bound at the
    next gene), the other seven are N(0, 2)."""
    _, _, k = constants(trans)
    d = rng.normal(0.0, 2.0, size=n)
    d[::GPL] = rng.choice([-20.0, 20.0], size=len(d[::GPL])) - k
    return d


def quiet(rng, m, trans=TRANS2):
    """m score differences that keep Delta strictly inside (lo, hi) whatever enters: c = k + d is a wobble of at most 0.02
    a gene, so a lane of them has a map that is NOT constant (the fold's two tracks stay hi - lo apart, or both clamped
    to different bounds)"""
    _, _, k = constants(trans)
    return -k + rng.uniform(-0.02, 0.02, size=m)


def plant_runs(rng, runs, lengths, trans=TRANS2):
    """a batch of ONE workgroup (sum(lengths) <= 2048) on the constant background with runs of non-constant lanes:
    runs = [(first lane, number of lanes)]"""
    n = sum(lengths)
    assert n <= BLOCK
    d = lane_background(rng, n, trans)
    for lane, m in runs:
        lo_g, hi_g = GPL * lane, min(GPL * (lane + m), n)
        d[lo_g:hi_g] = quiet(rng, hi_g - lo_g, trans)
    return d


def needs_fallback(runs):
    """what the planted runs ask for, from their geometry alone: the fallback, iff the part of some run inside one wave is
    longer than RUN lanes (lane 0 of the workgroup is never part of a run)"""
    for lane, m in runs:
        for w in range(LANES // 64):
            if min(lane + m, 64 * (w + 1)) - max(lane, 64 * w) > RUN:
                return True
    return False


def plant_tie(d, cptr, trans, g, ulps, j, big=20.0):
    """Rewrite d[g] so that CRFsuite's two candidates for label j at gene g + 1 (delta_g[0] + t0j and delta_g[1] + t1j,
    from ITS recursion over the contig up to g) lie `ulps` units in the last place apart, and d[g + 1] so that gene g + 1
    takes label j by `big`: the planted back-pointer decides gene g's label.  Returns (w row of g, w row of g + 1, winner)
    -- the rows replace (0, d) for the two genes (a tie needs both of gene g's weights)."""
    trans = np.asarray(trans, dtype=np.float64)
    c = int(np.searchsorted(cptr, g, side="right") - 1)
    g0 = int(cptr[c])
    assert g0 < g and g + 1 < int(cptr[c + 1]) - 1
    delta = np.array([0.0, float(d[g0])])
    for t in range(g0 + 1, g):
        m, _ = _delta_step(delta, trans)
        delta = m + np.array([0.0, float(d[t])])
    m, _ = _delta_step(delta, trans)
    for attempt in range(400):
        s0 = float(np.random.default_rng(1000 * g + attempt).normal(0.0, 0.5))
        target = _ulp_step((m[0] + s0) + trans[0, j], ulps)
        s1 = _solve_sum(m[1], trans[1, j], target)
        if s1 is not None and abs(s1) < big:
            assert (m[1] + s1) + trans[1, j] == target
            row1 = np.full(2, -big)
            row1[j] = big
            return np.array([s0, s1]), row1, (1 if ulps > 0 else 0)
    raise AssertionError("could not plant a tie")
