"""Training sets aimed at the edges of the device forest (gecco_amd/csrc/crf_forest.hip): sklearn's split rules at
near-equal feature values, the negative / zero / positive layout of a sparse column, ties in the argmax and between
features, and the kernel's size limits.  Every set is built from fixed seeds with numpy alone (legacy `RandomState`
streams, which numpy keeps frozen), by `build(name)`; `NAMES` lists them and `PATHS[name]` says which kernel path a set is
for.  Imported by tools/gen_forest_edge_fixtures.py (sklearn's side, recorded in tests/golden/types/forest_edges.json.gz)
and by tests/test_gpu_forest_edges.py / tests/test_forest_edges_host.py.

A set is a dict:
    n, F            samples, features
    indptr, indices, data      the CSC triplet sklearn trains on (int32, int32, float32; stored zeros are kept)
    y               (n, n_outputs) uint8 class indices; an output whose column is all 0 has one class
    mode "tree":    `seeds` (one DecisionTreeClassifier(max_features=max_features, random_state=seed) each) and `counts`
                    (n,) int32 sample weights -> _native.Forest with rand_state = types.splitter_state(seed)
    mode "forest":  `n_estimators`, `random_state`, `max_features` -> RandomForestClassifier / types.DeviceForest
"""
import hashlib
from fractions import Fraction

import numpy as np

F32 = np.float32
DENORM = float(np.float32(1.4e-45))  # the smallest positive float32
THREADS = 256                        # crf_forest.hip kThreads: block_argmax's layout, for the mirrored sets
MAX_SAMPLES, MAX_FEATURES, MAX_OUTPUTS = 4096, 8192, 64

_BUILDERS = {}
PATHS = {}


def _register(name, path, fn, *args):
    assert name not in _BUILDERS, name
    _BUILDERS[name] = (fn, args)
    PATHS[name] = path


def ulps(a, k: int) -> np.float32:
    """The float32 `k` steps above `a` (towards +inf)."""
    v = np.float32(a)
    for _ in range(k):
        v = np.nextafter(v, np.float32(np.inf))
    return v


def _from_dense(dense, stored=None):
    """CSC of a dense float32 matrix: the entries that are nonzero or marked in `stored` (explicit zeros)."""
    dense = np.asarray(dense, dtype=F32)
    keep = dense != 0
    if stored is not None:
        keep |= stored
    indptr = np.zeros(dense.shape[1] + 1, dtype=np.int32)
    indices, data = [], []
    for f in range(dense.shape[1]):
        r = np.flatnonzero(keep[:, f])
        indices.append(r)
        data.append(dense[r, f])
        indptr[f + 1] = indptr[f] + len(r)
    return (indptr, np.concatenate(indices).astype(np.int32) if indices else np.zeros(0, np.int32),
            np.concatenate(data).astype(F32) if data else np.zeros(0, F32))


def _tree(dense, y, seeds, max_features, counts=None, stored=None, csc=None):
    n, F = (dense.shape if csc is None else csc[0])
    indptr, indices, data = _from_dense(dense, stored) if csc is None else csc[1:]
    y = np.asarray(y, dtype=np.uint8).reshape(n, -1)
    counts = np.ones(n, np.int32) if counts is None else np.asarray(counts, dtype=np.int32)
    return dict(n=int(n), F=int(F), indptr=indptr, indices=indices, data=data, y=y, mode="tree", seeds=[int(s) for s in seeds],
                max_features=int(max_features), counts=counts)


def _forest(dense, y, n_estimators, random_state, max_features="sqrt", stored=None, csc=None):
    n, F = (dense.shape if csc is None else csc[0])
    indptr, indices, data = _from_dense(dense, stored) if csc is None else csc[1:]
    y = np.asarray(y, dtype=np.uint8).reshape(n, -1)
    return dict(n=int(n), F=int(F), indptr=indptr, indices=indices, data=data, y=y, mode="forest",
                n_estimators=int(n_estimators), random_state=int(random_state), max_features=max_features)


def _sparse(rs, n, f, density, neg=False):
    d = rs.random_sample((n, f)) * (rs.random_sample((n, f)) < density)
    if neg:
        d = d * np.where(rs.random_sample((n, f)) < 0.3, -1.0, 1.0)
    return np.round(d, 3).astype(F32)


def _flip(rs, y, p):
    """`y` with each label flipped with probability p (noise: deeper trees)."""
    return np.where(rs.random_sample(y.shape) < p, 1 - y, y)


def digest(s) -> str:
    """SHA-256 of a set's built arrays and fit arguments."""
    h = hashlib.sha256()
    h.update(np.array([s["n"], s["F"]], dtype=np.int64).tobytes())
    for key, dt in (("indptr", np.int32), ("indices", np.int32), ("data", np.float32), ("y", np.uint8)):
        h.update(np.ascontiguousarray(s[key], dtype=dt).tobytes())
    if s["mode"] == "tree":
        h.update(np.asarray(s["counts"], dtype=np.int32).tobytes())
        h.update(np.asarray(s["seeds"] + [s["max_features"]], dtype=np.int64).tobytes())
    else:
        h.update(repr((s["n_estimators"], s["random_state"], s["max_features"])).encode())
    return h.hexdigest()


def coo(s):
    """The set as the `(shape, row, col, data)` tuple `types.DeviceForest.fit` accepts."""
    col = np.repeat(np.arange(s["F"]), np.diff(s["indptr"]))
    return (s["n"], s["F"]), s["indices"].astype(np.int64), col.astype(np.int64), s["data"]


def dense_rows(s, rows) -> np.ndarray:
    """Training rows `rows` as dense float64."""
    out = np.zeros((len(rows), s["F"]))
    col = np.repeat(np.arange(s["F"]), np.diff(s["indptr"]))
    for k, i in enumerate(rows):
        sel = s["indices"] == i
        out[k, col[sel]] = s["data"][sel]
    return out


# ------------------------------------------------------------------------------------------ near-equal values
def ulp_pair(base, k, seed):
    """Two values k ulps apart: a dense column, the same pair behind a zero block, an ordinary column."""
    rs = np.random.RandomState(seed)
    n = 36
    a, b = np.float32(base), ulps(base, k)
    hi = rs.permutation(n) < n // 2
    c0 = np.where(hi, b, a)
    third = rs.permutation(n) % 3
    c1 = np.where(third == 0, F32(0), np.where(third == 1, a, b))
    dense = np.stack([c0, c1, _sparse(rs, n, 1, 0.5)[:, 0]], axis=1)
    y = np.stack([hi.astype(int), _flip(rs, (third == 2).astype(int), 0.1)], axis=1)
    return _tree(dense, y, seeds=(11, 12, 13, 14), max_features=2)


for _base, _k in ((0.2, 1), (0.75, 1), (1.0, 1), (3.0, 1), (1e-8, 1), (0.2, 6), (0.2, 7), (-0.2, 6), (-0.2, 7), (0.75, 2)):
    _register(f"ulp{_k}_at_{_base:g}", f"valid-position and constant tests: two values {_k} ulp apart at {_base:g} (double + 1e-7, "
              "float + 1e-7f and a plain > disagree)", ulp_pair, _base, _k, 100 + len(_BUILDERS))


def zero_block(v, far, seed):
    """The implicit zero block against the tiny value v, alone or with ordinary nonzeros beyond both."""
    rs = np.random.RandomState(seed)
    n = 40
    kind = rs.permutation(n) % 4  # 0, 1: zero; 2: v; 3: v or a far value
    c0 = np.where(kind >= 2, F32(v), F32(0))
    if far:
        sel = np.flatnonzero(kind == 3)
        c0[sel[::2]] = F32(-0.5 if v > 0 else 0.7)   # beyond the zero block
        c0[sel[1::2]] = F32(0.7 if v > 0 else -0.5)  # beyond v
    side = (c0 >= F32(v)) if v > 0 else (c0 <= F32(v))
    dense = np.stack([c0, _sparse(rs, n, 1, 0.4, neg=True)[:, 0]], axis=1)
    y = np.stack([side.astype(int), _flip(rs, side.astype(int), 0.15)], axis=1)
    return _tree(dense, y, seeds=(21, 22, 23), max_features=2)


for _v in (DENORM, -DENORM, 1e-8, -1e-8, 9e-8, -9e-8):
    for _far in (False, True):
        _register(f"zero_vs_{_v:g}" + ("_far" if _far else ""), f"the zero block next to {_v:g}" +
                  (" with nonzeros on the far side" if _far else "") + ": zpos neighbours in the valid-position test, threshold "
                  "between 0 and a tiny value", zero_block, _v, _far, 200 + len(_BUILDERS))


def _const_column(off_by_one, seed):
    rs = np.random.RandomState(seed)
    n = 48
    c0 = np.full(n, F32(0.37))
    if off_by_one:
        c0[17] = ulps(0.37, 1)
    rest = _sparse(rs, n, 3, 0.4)
    y0 = (rest[:, 0] > 0.3).astype(int)
    if off_by_one:
        y0[17] = 1 - y0[17]
    y = np.stack([_flip(rs, y0, 0.1), (np.arange(n) == 17).astype(int) if off_by_one else (rest[:, 1] > 0).astype(int)], axis=1)
    return _tree(np.concatenate([c0[:, None], rest], axis=1), y, seeds=(31, 32, 33, 34), max_features=2)


_register("const_equal_nonzeros", "a column of equal nonzeros covering the node: constant through evaluate_feature (m == n_node), "
          "not through the nonzero pre-pass", _const_column, False, 301)
_register("const_one_ulp_off", "the same column with one sample 1 ulp off: not constant, one valid position", _const_column, True, 302)


def chain(base, zero_block, seed):
    """a, a + 1 ulp, a + 2 ulp, ... over 300 samples: every position valid under >, none under + 1e-7."""
    rs = np.random.RandomState(seed)
    n = 300
    step = np.arange(n) if not zero_block else np.maximum(np.arange(n) - 40, 0)
    vals = np.array([ulps(base, int(k)) for k in range(int(step.max()) + 1)], dtype=F32)[step] if base else \
        (step.astype(np.int32)).view(F32)  # 0, then the denormals 1, 2, 3 ... ulps above it
    if zero_block and base:
        vals = np.where(np.arange(n) < 40, F32(0), vals)
    perm = rs.permutation(n)
    c0 = vals[perm]
    y0 = ((step[perm] // 7) % 2).astype(int)
    dense = np.stack([c0, _sparse(rs, n, 1, 0.2)[:, 0]], axis=1)
    return _tree(dense, np.stack([y0, _flip(rs, y0, 0.2)], axis=1), seeds=(41, 42), max_features=2)


_register("chain_300_at_0.2", "a chain of 300 values 1 ulp apart at 0.2 (dense column): every neighbour pair within 1e-7", chain, 0.2, False, 311)
_register("chain_300_at_1e-8", "the same chain at 1e-8 behind a zero block of 40", chain, 1e-8, True, 312)
_register("chain_300_denormals", "a zero block, then the denormals 1, 2, 3 ... ulps above zero", chain, 0.0, True, 313)


def _mixed(seed, neg):
    """Near-equal columns among ordinary sparse ones: whether a drawn feature counts as constant several levels down feeds
    the draw loop's n_known / n_found / n_drawn bookkeeping of every node below."""
    rs = np.random.RandomState(seed)
    n, F = 300, 60
    d = _sparse(rs, n, F, 0.12, neg=neg)
    bases = (0.2, 0.75, 1e-8, 3.0, 0.0, -0.2)
    for j, f in enumerate(rs.permutation(F)[:24]):
        base = bases[j % len(bases)]
        nz = d[:, f] != 0
        k = rs.randint(0, 4, n)
        if base == 0.0:
            near = k.astype(np.int32).view(F32)  # zeros and denormals
        else:
            near = np.array([ulps(base, int(i)) for i in range(4)], dtype=F32)[k]
        d[:, f] = np.where(nz if j % 2 else np.ones(n, bool), near, F32(0))
    score = (d[:, :8] != 0).sum(axis=1)
    y = np.stack([score >= 2, d[:, 9] > d[:, 10], rs.random_sample(n) < 0.3], axis=1).astype(int)
    y[:, 0] = _flip(rs, y[:, 0], 0.1)
    return _forest(d, y, n_estimators=8, random_state=seed, max_features="sqrt")


_register("mixed_near_equal", "near-equal columns among ordinary sparse ones (bootstrap weights): the constants bookkeeping of the "
          "draw loop depends on them levels down", _mixed, 321, False)
_register("mixed_near_equal_neg", "the same with negative values", _mixed, 322, True)


# ------------------------------------------------------------------------------------------ negative / zero / positive
def _layout(kind, seed):
    rs = np.random.RandomState(seed)
    n = 64
    u = np.round(rs.random_sample(n) * 0.9 + 0.05, 3).astype(F32)
    stored = np.zeros((n, 4), dtype=bool)
    part = rs.permutation(n) % 4
    if kind == "all_negative":
        c0 = -u
    elif kind == "negatives_and_zeros":
        c0 = np.where(part < 2, -u, F32(0))
    elif kind == "dense_mixed_signs":
        c0 = np.where(part < 2, -u, u)
    elif kind == "symmetric_pm_a":          # -a | +a: the midpoint is +0.0 exactly
        c0 = np.where(part < 2, F32(-0.625), F32(0.625))
    elif kind == "threshold_below_zero":    # negatives | zero block | positives, classes split between negatives and zeros
        c0 = np.where(part == 0, F32(-1e-30), np.where(part == 1, F32(0), u))
    elif kind == "denormal_below_zero":
        c0 = np.where(part == 0, F32(-DENORM), np.where(part == 1, F32(0), u))
    elif kind == "stored_zeros":            # explicit +0.0 / -0.0 entries in the CSC data belong to the zero block
        c0 = np.where(part == 0, -u, np.where(part == 3, u, F32(0)))
        c0[(part == 1) & (np.arange(n) % 2 == 0)] = F32(-0.0)
        stored[:, 0] = part == 1
    else:
        raise KeyError(kind)
    if kind in ("threshold_below_zero", "denormal_below_zero"):
        y0 = (part == 0).astype(int)
    elif kind == "symmetric_pm_a":
        y0 = (c0 > 0).astype(int)
    else:
        y0 = (c0 > np.median(c0)).astype(int)
    rest = _sparse(rs, n, 3, 0.3, neg=True)
    y = np.stack([y0, _flip(rs, y0, 0.2)], axis=1)
    return _tree(np.concatenate([c0[:, None], rest], axis=1), y, seeds=(51, 52, 53), max_features=4, stored=stored)


for _kind, _path in (("all_negative", "an all-negative dense column: nneg == m, no zero block"),
                     ("negatives_and_zeros", "negatives and zeros only: the zero block is the last entry"),
                     ("dense_mixed_signs", "a dense column, m == n_node: no zero block between negatives and positives"),
                     ("symmetric_pm_a", "-a and +a without zeros: the threshold is +0.0 (zero_left with nothing in the block)"),
                     ("threshold_below_zero", "a threshold a hair below zero (-5e-31): the zero block goes right"),
                     ("denormal_below_zero", "-1.4e-45 against the zero block: threshold -7e-46, zeros go right"),
                     ("stored_zeros", "explicit +0.0 and -0.0 entries in the CSC data count as the zero block")):
    _register(_kind, _path, _layout, _kind, 400 + len(_BUILDERS))


# ------------------------------------------------------------------------------------------ ties
# name: (N, where block_argmax meets the tied pair, first index of the class-1 band in the lower half, label seed)
MIRRORED = {"mirrored_300": (300, "two_lanes", 138, 2), "mirrored_1025": (1025, "one_chunk", 511, 1),
            "mirrored_4096": (4096, "two_waves", 700, 1)}


def mirrored_labels(N, centre, seed):
    """Labels with y[i] == y[N-1-i]: class 1 in the band [centre, N - centre) around the middle, class 0 outside, each
    label of the lower half flipped with probability 0.04 where the band is wide enough to stay the best split (a band of
    three, which puts both tied positions into one thread's chunk, is left clean)."""
    rs = np.random.RandomState(seed)
    half = (N + 1) // 2
    h = (np.arange(half) >= centre).astype(np.uint8)
    if N - 2 * centre > 8:
        h = _flip(rs, h, 0.04).astype(np.uint8)
    y = np.zeros(N, np.uint8)
    y[:half] = h
    y[N - half:] = h[::-1]
    return y


def mirrored_proxies(y):
    """Exact proxy improvement (-w_r gini_r - w_l gini_l, one output, unit weights) of every position 1..N-1, as Fractions."""
    N = len(y)
    ones = np.concatenate([[0], np.cumsum(y.astype(np.int64))])
    tot = int(ones[-1])
    out = [None]
    for j in range(1, N):
        l1, r1 = int(ones[j]), tot - int(ones[j])
        l0, r0 = j - l1, (N - j) - r1
        gl = 1 - Fraction(l0 * l0 + l1 * l1, j * j)
        gr = 1 - Fraction(r0 * r0 + r1 * r1, (N - j) * (N - j))
        out.append(-(N - j) * gr - j * gl)
    return out


def tied_best(y):
    """(j, N - j) when exactly the positions j < N - j hold the maximum of the exact proxies; else None."""
    px = mirrored_proxies(y)
    N = len(y)
    best = max(px[1:])
    at = [j for j in range(1, N) if px[j] == best]
    return tuple(at) if len(at) == 2 and at[0] + at[1] == N else None


def landing(N, pair):
    """Where block_argmax meets the pair: thread t owns entries [t C, (t + 1) C), C = ceil(N / 256); waves of 64 threads."""
    C = -(-N // THREADS)
    ta, tb = pair[0] // C, pair[1] // C
    if ta == tb:
        return "one_chunk"
    return "two_lanes" if ta // 64 == tb // 64 else "two_waves"


def _mirrored(name):
    N, _, centre, seed = MIRRORED[name]
    y = mirrored_labels(N, centre, seed)
    c0 = np.arange(1, N + 1, dtype=F32)
    return _tree(c0[:, None], y, seeds=(61,), max_features=1)


for _name, (_N, _want, _, _) in MIRRORED.items():
    _register(_name, f"feature 1..{_N}, mirrored labels: proxy(j) == proxy(N - j) bit for bit, the tied best pair in "
              f"{_want.replace('_', ' ')} of block_argmax; the first position wins", _mirrored, _name)


def _duplicated_columns(seed):
    rs = np.random.RandomState(seed)
    n = 120
    base = _sparse(rs, n, 4, 0.5, neg=True)
    dense = np.concatenate([base, base[:, [2, 0, 3, 1]], base[:, :2]], axis=1)  # every column two or three times
    y = np.stack([_flip(rs, (base[:, 0] > 0.2).astype(int), 0.1), (base[:, 1] + base[:, 2] > 0.3).astype(int)], axis=1)
    return _tree(dense, y, seeds=(71, 72, 73, 74, 75, 76), max_features=10)


_register("duplicated_columns", "identical columns: equal best proxies between features, the first drawn wins (strict >)",
          _duplicated_columns, 501)


# ------------------------------------------------------------------------------------------ size limits
def _node_cap():
    n = MAX_SAMPLES
    bits = (np.arange(n)[:, None] >> np.arange(12)) & 1
    return _tree(bits.astype(F32), bits, seeds=(81,), max_features=12)


_register("node_cap_4096", "4096 distinct rows, 12 outputs holding the row number's bits: 8191 nodes, cap = 2n - 1 exactly", _node_cap)


def _stack_cap():
    n = MAX_SAMPLES
    return _tree(np.arange(1, n + 1, dtype=F32)[:, None], np.arange(n) % 2, seeds=(82,), max_features=1)


_register("stack_cap_4096", "feature 1..4096, y = i % 2: 8191 nodes at depth 4095, stack_cap = n + 1 records, a full 4096-entry "
          "column gathered and sorted (P == m)", _stack_cap)


def _bitonic(m, seed):
    """A root with exactly m nonzeros in its column (distinct values, both signs) and a zero block."""
    rs = np.random.RandomState(seed)
    n = m + 37
    vals = (rs.permutation(4 * m)[:m].astype(np.float64) - 2 * m + 0.5) / 64.0
    rows = rs.permutation(n)[:m]
    c0 = np.zeros(n, F32)
    c0[rows] = vals.astype(F32)
    y0 = ((np.argsort(np.argsort(c0)) // 9) % 2).astype(int)
    dense = np.stack([c0, _sparse(rs, n, 1, 0.1)[:, 0]], axis=1)
    return _tree(dense, np.stack([y0, _flip(rs, y0, 0.3)], axis=1), seeds=(91, 92), max_features=2)


for _m in (255, 256, 257, 1023, 1025):
    _register(f"bitonic_{_m}", f"{_m} nonzeros in the root's column: the bitonic sort's padding to a power of two", _bitonic, _m, 600 + _m)


def _wide():
    """4096 x 8192 at density 0.004 with 64 outputs, one-class outputs at 0 and 63."""
    rs = np.random.RandomState(701)
    n, F, K = MAX_SAMPLES, MAX_FEATURES, MAX_OUTPUTS
    flat = np.unique(rs.randint(0, n * F, int(0.004 * n * F)))
    col, row = flat // n, flat % n  # column-major: CSC order
    data = np.round(rs.random_sample(len(flat)) + 0.001, 3).astype(F32)
    indptr = np.zeros(F + 1, np.int32)
    np.cumsum(np.bincount(col, minlength=F), out=indptr[1:])
    load = np.zeros((n, K))
    for k in range(K):  # output k follows the presence of a few columns
        sel = np.isin(col, rs.randint(0, F, 40))
        load[row[sel], k] += 1
    y = (load > 0).astype(np.uint8)
    y = _flip(rs, y, 0.05).astype(np.uint8)
    y[:, 0] = 0  # one class each
    y[:, K - 1] = 0
    return _forest(None, y, n_estimators=3, random_state=7, csc=((n, F), indptr, row.astype(np.int32), data))


_register("wide_4096x8192_64out", "the largest accepted matrix, 64 outputs with one-class outputs first and last", _wide)


def _outputs_64(seed):
    rs = np.random.RandomState(seed)
    n, F, K = 200, 50, MAX_OUTPUTS
    d = _sparse(rs, n, F, 0.15)
    y = (rs.random_sample((n, K)) < 0.3).astype(int)
    y[:, K - 1] = _flip(rs, (d[:, 3] > 0).astype(int), 0.1)
    return _forest(d, y, n_estimators=4, random_state=seed)


_register("outputs_64_two_class", "64 two-class outputs: bit 63 of ybits and of two_class", _outputs_64, 702)


def _small(kind):
    rs = np.random.RandomState(800)
    if kind == "one_feature":
        c = _sparse(rs, 50, 1, 0.7, neg=True)
        return _tree(c, _flip(rs, (c[:, 0] > 0.2).astype(int), 0.1), seeds=(1, 2), max_features=1)
    if kind == "one_sample":
        return _tree(np.array([[0.5, 0.0]], F32), [[1, 0]], seeds=(1,), max_features=1)
    if kind == "two_samples":
        return _tree(np.array([[0.5, 0.0], [0.25, 0.0]], F32), [[1, 0], [0, 0]], seeds=(1, 2), max_features=2)
    if kind == "constant_root":  # every feature constant at the root (equal nonzeros, zeros, an empty column): an impure leaf
        d = np.zeros((30, 4), F32)
        d[:, 0] = 1.5
        d[:, 2] = -2.0
        return _tree(d, rs.randint(0, 2, (30, 2)), seeds=(1, 2), max_features=2)
    if kind == "empty_column":
        d = _sparse(rs, 60, 5, 0.4)
        d[:, [1, 4]] = 0
        return _tree(d, np.stack([d[:, 0] > 0.3, d[:, 2] > d[:, 3]], axis=1).astype(int), seeds=(1, 2, 3), max_features=3)
    raise KeyError(kind)


for _kind, _path in (("one_feature", "n_features == 1"), ("one_sample", "n_samples == 1: the root is a leaf"),
                     ("two_samples", "n_samples == 2"), ("constant_root", "a root whose features are all constant: an impure leaf"),
                     ("empty_column", "columns without entries among ordinary ones")):
    _register(_kind, _path, _small, _kind)


def _skewed(kind):
    rs = np.random.RandomState(900)
    if kind == "one_heavy_sample":
        n = 64
        d = _sparse(rs, n, 5, 0.4, neg=True)
        counts = rs.randint(0, 2, n)
        counts[9] = n
        y = np.stack([d[:, 0] > 0.1, d[:, 1] > d[:, 2]], axis=1).astype(int)
        return _tree(d, _flip(rs, y, 0.15), seeds=(1, 2, 3), max_features=2, counts=counts)
    n = MAX_SAMPLES  # every count 4096 but one at 4095: a total of 2^24 - 1, the largest accepted
    d = _sparse(rs, n, 6, 0.3, neg=True)
    counts = np.full(n, n)
    counts[1234] = n - 1
    y = np.stack([d[:, 0] > 0.4, d[:, 1] + d[:, 2] > 0.5], axis=1).astype(int)
    return _tree(d, _flip(rs, y, 0.02), seeds=(1,), max_features=3, counts=counts)


_register("one_heavy_sample", "one sample with count n among counts of 0 and 1", _skewed, "one_heavy_sample")
_register("total_weight_2p24_minus_1", "4096 samples, counts 4096 but one 4095: total weight 2^24 - 1, the largest accepted",
          _skewed, "largest_total")

NAMES = list(_BUILDERS)
NEAR_EQUAL = [n for n in NAMES if n.startswith(("ulp", "zero_vs_", "const_", "chain_", "mixed_"))]


def build(name):
    fn, args = _BUILDERS[name]
    s = fn(*args)
    s["name"] = name
    return s


# ------------------------------------------------------------------------------------------ predict rows
def split_nodes(exports):
    """(feature, threshold) of the split nodes of the exported trees, in tree and node order."""
    return [(int(ex["feature"][i]), float(ex["threshold"][i])) for ex in exports for i in range(len(ex["feature"]))
            if ex["children_left"][i] >= 0]


def planted_rows(s, nodes) -> np.ndarray:
    """Predict rows at the decision boundaries of a fitted set: zero rows and training rows; for up to twelve split nodes
    (evenly spaced among `nodes`), a row with the node's feature at its threshold, at the threshold's float32 rounding and
    at the float64 neighbours of both; for the first and last picked node's feature, -0.0, +0.0, +-1.4e-45, doubles just
    below and just above half of it (the float64 -> float32 cast of a denormal) and negative values."""
    rs = np.random.RandomState(s["n"] * 7 + s["F"])
    F = s["F"]
    train = dense_rows(s, [int(i) for i in rs.permutation(s["n"])[:6]])
    rows = [np.zeros(F), *train]
    pick = [nodes[i] for i in sorted(set(np.linspace(0, len(nodes) - 1, 12).astype(int)))] if nodes else []
    for j, (f, th) in enumerate(pick):
        f32 = float(np.float32(th))
        for v in (th, f32, np.nextafter(th, np.inf), np.nextafter(th, -np.inf), np.nextafter(f32, np.inf), np.nextafter(f32, -np.inf)):
            r = train[j % len(train)].copy() if j % 2 else np.zeros(F)
            r[f] = v
            rows.append(r)
    for f, th in (pick[:1] + pick[-1:]):
        for v in (-0.0, 0.0, DENORM, -DENORM, 7.0e-46, -7.0e-46, 7.1e-46, -7.1e-46, DENORM / 2, -1.0, -abs(th), -2.5e-8):
            r = np.zeros(F)
            r[f] = v
            rows.append(r)
    return np.array(rows)
