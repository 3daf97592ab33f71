"""Backward sampling of label paths in numpy, log space: the independent yardstick of ``gecco_crf_sample_paths``
(tests/test_gpu_sampling.py), pinned on known answers and on path enumeration by tests/test_sampling_host.py.  It shares no
code with the product.

The rule.  ``la[t]`` is the log forward vector of item t, shifted by its own log-sum-exp (any shift cancels).  Given the label j
of item t + 1, the weights are ``w_i = exp(la[t][i] + T[i][j])`` (``exp(la[t][i])`` at a sequence's last item), the running
sums ``c_i = w_0 + ... + w_i`` in label order, and the label is the smallest i with ``c_i > u c_{L-1}``; a label of weight
exactly 0 is never drawn, and if rounding leaves no such i the label is the last i with ``w_i > 0``.  u is Philox4x32-10 with
key ``(seed & 0xffffffff, seed >> 32)`` and counter ``(item offset inside the sequence, sample, sequence index, 0)``:
``u = ((x0 << 21) ^ (x1 >> 11)) 2^-53`` from the first two output words."""
import numpy as np

from tests.train_objective_valued import lse

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
MARGIN = 1e-9  # a draw whose u lies this close to a boundary of the running sums may fall on either side of it


def philox4x32_10(counter, key):
    """``counter`` [..., 4] and ``key`` [..., 2] (uint32 words, broadcast against each other) -> output [..., 4] uint32."""
    counter, key = np.asarray(counter, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(counter[..., k], shape).copy() for k in range(4)]
    k0, k1 = np.broadcast_to(key[..., 0], shape).copy(), np.broadcast_to(key[..., 1], shape).copy()
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]  # (32 x 32 -> 64 bits: no overflow in uint64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _LOW, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _LOW]
        k0, k1 = (k0 + np.uint64(_W0)) & _LOW, (k1 + np.uint64(_W1)) & _LOW
    return np.stack(c, axis=-1).astype(np.uint32)


def uniforms(seed, t, s, c):
    """u in [0, 1) of (item offset t, sample s, sequence c), arrays broadcast against each other."""
    seed = int(seed)
    t, s, c = np.broadcast_arrays(np.asarray(t, dtype=np.uint64), np.asarray(s, dtype=np.uint64), np.asarray(c, dtype=np.uint64))
    counter = np.stack([t, s, c, np.zeros_like(t)], axis=-1)
    x = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).astype(np.uint64)
    return ((x[..., 0] << np.uint64(21)) ^ (x[..., 1] >> np.uint64(11))).astype(np.float64) * 2.0 ** -53


def log_forward(seq_ptr, score, T):
    """[n, L] log forward vectors over the masked item scores `score` (``-inf`` where disallowed), every one shifted by its own
    log-sum-exp as in ``tests.constrained_reference.marginals``."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    la = np.zeros_like(score)
    for k in range(len(seq_ptr) - 1):
        b, e = int(seq_ptr[k]), int(seq_ptr[k + 1])
        for t in range(b, e):
            v = score[t] if t == b else lse(la[t - 1][:, None] + T, axis=0) + score[t]
            la[t] = v - lse(v, 0)
    return la


def _positions(seq_ptr):
    """Per item: its sequence, its offset inside it, and whether it is its sequence's last."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    lens = np.diff(seq_ptr)
    owner = np.repeat(np.arange(len(lens)), lens)
    offset = np.arange(int(lens.sum())) - (seq_ptr[:-1] - seq_ptr[0])[owner]
    last = np.zeros(len(owner), dtype=bool)
    last[(seq_ptr[1:] - seq_ptr[0] - 1)[lens > 0]] = True
    return owner, offset, last


def _weights(la_rows, T, nxt, last):
    """[m, N, L] weights of m items given the labels `nxt` [m, N] of the items behind them (`last` [m]: no item behind)."""
    with np.errstate(invalid="ignore"):
        logw = la_rows[:, None, :] + np.where(last[:, None, None], 0.0, T.T[nxt])  # T.T[j] = T[:, j]
        logw = np.where(np.isnan(logw), -np.inf, logw)  # (-inf + inf cannot arise from finite weights; kept out all the same)
    top = logw.max(axis=2, keepdims=True)
    return np.exp(logw - top)


def _draw(w, u):
    """The rule on weights [..., L] and uniforms [...]: (labels, normalised running sums [..., L])."""
    c = np.cumsum(w, axis=-1)
    total = c[..., -1]
    over = c > (u * total)[..., None]
    lab = np.where(over.any(axis=-1), over.argmax(axis=-1), 0)
    L = w.shape[-1]
    last_positive = L - 1 - (w[..., ::-1] > 0).argmax(axis=-1)
    lab = np.where(over.any(axis=-1), lab, last_positive)
    return lab, c / total[..., None]


def sample(seq_ptr, score, T, n_samples, seed):
    """int8 [n, n_samples]: the reference's own paths."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    la = log_forward(seq_ptr, score, T)
    y = np.zeros((len(score), n_samples), dtype=np.int8)
    s = np.arange(n_samples)
    for k in range(len(seq_ptr) - 1):
        b, e = int(seq_ptr[k]), int(seq_ptr[k + 1])
        for t in range(e - 1, b - 1, -1):
            is_last = np.array([t == e - 1])
            nxt = np.zeros((1, n_samples), dtype=np.int64) if t == e - 1 else y[t + 1][None, :].astype(np.int64)
            w = _weights(la[t][None, :], T, nxt, is_last)[0]
            y[t] = _draw(w, uniforms(seed, t - b, s, k))[0]
    return y


def check_teacher_forced(y, seq_ptr, score, T, seed, block=128):
    """Every (sample, item) of the paths `y` [n, N] on its own: given y's label of the item behind, the reference's label has to
    be y's.  A draw is excused only when every boundary of the normalised running sums between the two labels lies within
    MARGIN of u (u then sits on the edge between them).  Returns (excused, near, draws): the excused draws, the draws whose u
    lies within MARGIN of any inner boundary (the reference's own count of draws that could go either way), and all draws.
    Raises AssertionError on a draw that is neither the reference's nor excused."""
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    y = np.asarray(y)
    n, N = y.shape
    L = score.shape[1]
    assert n == len(score) and y.dtype == np.int8
    assert y.min(initial=0) >= 0 and y.max(initial=0) < L, "a label outside 0 .. L - 1"
    la = log_forward(seq_ptr, score, T)
    owner, offset, last = _positions(seq_ptr)
    excused = near = 0
    s = np.arange(N)
    for g0 in range(0, n, block):
        g1 = min(n, g0 + block)
        behind = np.minimum(np.arange(g0, g1) + 1, n - 1)
        nxt = y[behind].astype(np.int64)
        w = _weights(la[g0:g1], T, nxt, last[g0:g1])
        u = uniforms(seed, offset[g0:g1, None], s[None, :], owner[g0:g1, None])
        ref, C = _draw(w, u)
        close = np.abs(u[..., None] - C[..., :L - 1]) <= MARGIN
        near += int(close.any(axis=-1).sum())
        got = y[g0:g1].astype(np.int64)
        for i, k in zip(*np.nonzero(got != ref)):
            a, b = sorted((int(got[i, k]), int(ref[i, k])))
            assert close[i, k, a:b].all(), (
                f"item {g0 + i} sample {k}: label {got[i, k]}, the reference draws {ref[i, k]} (u = {u[i, k]!r}, "
                f"running sums {C[i, k].tolist()})")
            excused += 1
    return excused, near, n * N


def run_extents(y, seq_ptr, contig, anchor, mask):
    """int32 [q, N, 2]: per query and sample the maximal run ``(first, last + 1)`` of items around the anchor whose labels all lie
    in the mask, offsets inside the sequence; ``(-1, -1)`` where the anchor's label does not."""
    y = np.asarray(y)
    seq_ptr = np.asarray(seq_ptr, dtype=np.int64)
    out = np.full((len(contig), y.shape[1], 2), -1, dtype=np.int32)
    for q, (c, a, m) in enumerate(zip(contig, anchor, mask)):
        b, e = int(seq_ptr[c]) - int(seq_ptr[0]), int(seq_ptr[c + 1]) - int(seq_ptr[0])
        inside = ((int(m) >> y[b:e].astype(np.int64)) & 1).astype(bool)
        left = np.logical_and.accumulate(inside[a::-1], axis=0).sum(axis=0)
        right = np.logical_and.accumulate(inside[a:], axis=0).sum(axis=0)
        hit = inside[a]
        out[q, hit, 0] = (a - left + 1)[hit]
        out[q, hit, 1] = (a + right)[hit]
    return out
