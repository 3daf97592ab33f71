"""Partially labelled training sets, the host side: the numpy yardstick (tests/train_objective_partial.py) against path
enumeration, ``train.build_training_set``'s three kinds of label entries and its feature rule, the optimiser's curvature
safeguard, the refusals of the ``*_create_partial`` entries (found before the device is looked at), the typed front end's
``unknown="any"`` labels, and the ABI.  No GPU."""
import itertools

import numpy as np
import pytest

from tests import train_objective_partial as tp
from tests.train_objective_labels import labelled_sequences


# ---------------------------------------------------------------- the yardstick against path enumeration
def _enumerate(seq_ptr, item_ptr, attr_id, allowed, A, L, W, step, state_fid, trans_fid, w):
    """f and g by enumerating all L^n label paths of every instance: Z and Z_A as plain sums of exp(score - best score), each over its own paths."""
    sfid, tfid = np.asarray(state_fid).reshape(A, L), np.asarray(trans_fid).reshape(L, L)
    S = np.where(sfid >= 0, w[np.maximum(sfid, 0)], 0.0)
    T = np.where(tfid >= 0, w[np.maximum(tfid, 0)], 0.0)
    ok = tp.mask_matrix(allowed, L)
    f, g = 0.0, np.zeros(len(w))
    for n, starts in tp.instance_groups(seq_ptr, W, step):
        paths = np.array(list(itertools.product(range(L), repeat=n)))  # [L^n, n]
        for i0 in starts.tolist():
            items = range(i0, i0 + n)
            attrs = [attr_id[item_ptr[i]:item_ptr[i + 1]] for i in items]
            score = np.array([[sum(S[a, y] for a in attrs[t]) for y in range(L)] for t in range(n)])
            total = score[np.arange(n)[None, :], paths].sum(axis=1) + T[paths[:, :-1], paths[:, 1:]].sum(axis=1)
            inside = ok[i0 + np.arange(n)[None, :], paths].all(axis=1)
            best, best_a = total.max(), total[inside].max()  # (each sum relative to its own best path)
            e, ea = np.exp(total - best), np.where(inside, np.exp(np.where(inside, total, best_a) - best_a), 0.0)
            f += (best + np.log(e.sum())) - (best_a + np.log(ea.sum()))
            weight = e / e.sum() - ea / ea.sum()  # p(path) - p_A(path)
            for t in range(n):
                for y in range(L):
                    m = weight[paths[:, t] == y].sum()
                    for a in attrs[t]:
                        if sfid[a, y] >= 0:
                            g[sfid[a, y]] += m
            for t in range(1, n):
                for i, j in itertools.product(range(L), repeat=2):
                    if tfid[i, j] >= 0:
                        g[tfid[i, j]] += weight[(paths[:, t - 1] == i) & (paths[:, t] == j)].sum()
    return f, g


def _tiny(rng, L, lengths, A=5):
    seq_ptr, item_ptr, attr_id, _ = labelled_sequences(rng, lengths, A, L)
    fid = np.arange(A * L + L * L, dtype=np.int32)
    fid[[1, A * L + 1]] = -1  # (one pair of each kind without a feature)
    keep = fid >= 0
    fid[keep] = np.arange(int(keep.sum()))
    return seq_ptr, item_ptr, attr_id, A, fid[:A * L], fid[A * L:], int(keep.sum())


@pytest.mark.parametrize("scale", [1.0, 300.0])
@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("L", [2, 3, 5])
def test_yardstick_against_path_enumeration(L, whole, scale):
    rng = np.random.default_rng(100 * L + int(whole))
    lengths = [1, 2, 6, 4] if whole else [3, 5, 6]
    W, step = (None, None) if whole else (3, 2)
    seq_ptr, item_ptr, attr_id, A, sfid, tfid, K = _tiny(rng, L, lengths)
    allowed = tp.random_masks(rng, int(seq_ptr[-1]), L)
    assert (allowed != 0).all()
    w = scale * rng.normal(size=K)
    with np.errstate(invalid="raise", divide="raise"):  # (the masked recursion forms nothing invalid)
        f, g, count, groups = tp.objective_partial(seq_ptr, item_ptr, attr_id, allowed, A, L, W, step, sfid, tfid, w,
                                                   details=True)
    ef, eg = _enumerate(seq_ptr, item_ptr, attr_id, allowed, A, L, W, step, sfid, tfid, w)
    tol_f, tol_g = tp.partial_tolerances(L, groups)
    assert count == (len(lengths) if whole else sum((n - W) // step + 1 for n in lengths))
    assert np.isfinite(f) and np.isfinite(g).all()
    assert abs(f - ef) <= tol_f, (f, ef, tol_f)
    assert (np.abs(g - eg) <= tol_g).all(), float(np.max(np.abs(g - eg) - tol_g))
    assert f >= -tol_f  # (Z_A <= Z)


@pytest.mark.parametrize("whole", [False, True])
def test_yardstick_singletons_and_full_sets(whole):
    """With singletons the objective is the labelled one; with full sets f = 0 and g = 0, exactly (the two passes are the
    same operations)."""
    from tests.train_objective_labels import objective
    from tests.train_objective_sequences import objective_sequences

    rng = np.random.default_rng(3)
    L, lengths = 4, [5, 5, 9, 6]
    W, step = (None, None) if whole else (5, 1)
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, lengths, 6, L)
    A, sfid, tfid = 6, np.arange(6 * L, dtype=np.int32), 6 * L + np.arange(L * L, dtype=np.int32)
    w = rng.normal(size=6 * L + L * L)
    f, g, _, groups = tp.objective_partial(seq_ptr, item_ptr, attr_id, tp.singleton_masks(labels), A, L, W, step, sfid, tfid, w,
                                           details=True)
    if whole:
        lf, lg, _ = objective_sequences(seq_ptr, item_ptr, attr_id, labels, A, L, sfid, tfid, w)
    else:
        lf, lg, _ = objective(seq_ptr, item_ptr, attr_id, labels, A, L, W, step, sfid, tfid, w)
    tol_f, tol_g = tp.partial_tolerances(L, groups)
    assert abs(f - lf) <= tol_f and (np.abs(g - lg) <= tol_g).all()
    f, g, _ = tp.objective_partial(seq_ptr, item_ptr, attr_id, tp.full_masks(int(seq_ptr[-1]), L), A, L, W, step, sfid, tfid, w)
    assert f == 0.0 and not g.any()


def test_yardstick_masks_are_unsigned_and_never_empty():
    assert tp.mask_matrix(np.array([1 << 31], dtype=np.uint32), 32)[0].tolist() == [False] * 31 + [True]
    with pytest.raises(ValueError, match="at least one allowed label"):
        tp.objective_partial([0, 1], [0, 1], np.array([0]), np.array([0], dtype=np.uint32), 1, 2, None, None, [0, 1], [-1] * 4, np.zeros(2))


# ---------------------------------------------------------------- build_training_set
SEQS = [[["a"], ["a", "b"], ["b"]], [["b"], ["c"]], [["a"], ["c"], ["c"]]]


def test_build_training_set_three_kinds_of_entries_and_the_feature_rule():
    from gecco_amd import train

    # ids: x (first), then the set {z, y} scanned sorted: y = 1, z = 2; None names no label
    labels = [["x", {"z", "y"}, "y"], [None, "z"], ["x", ("x", "z"), ["z"]]]
    ts = train.build_training_set(SEQS, labels, None, max_labels=32)
    assert ts.labels_ == ["x", "y", "z"] and ts.attrs_ == ["a", "b", "c"]
    assert ts.allowed.dtype == np.uint32
    assert ts.allowed.tolist() == [0b001, 0b110, 0b010, 0b111, 0b100, 0b001, 0b101, 0b100]
    # state (attribute, label): an attribute on an item whose set holds the label, frequency = the occurrences
    state = {(ts.attrs_[a], ts.labels_[y]) for a, y in zip(ts.state_attr, ts.state_label)}
    assert state == {("a", "x"), ("a", "y"), ("a", "z"), ("b", "y"), ("b", "z"), ("b", "x"), ("c", "z"), ("c", "x")}
    # transitions: adjacent items holding i and j
    trans = {(ts.labels_[i], ts.labels_[j]) for i, j in zip(ts.trans_src, ts.trans_dst)}
    assert trans == {("x", "y"), ("x", "z"), ("y", "y"), ("z", "y"), ("y", "z"), ("z", "z"), ("x", "x")}
    # min_freq compares the summed occurrences: (a, x) on items 0 and 5, (b, y) on items 1, 2 and 3, (b, z) on items 1 and 3,
    # (c, z) on items 4, 6 and 7; every other state feature once.  (x, z): pairs 0-1, 3-4, 5-6 and 6-7; (z, z): 3-4 and 6-7
    ts2 = train.build_training_set(SEQS, labels, None, min_freq=2, max_labels=32)
    state2 = {(ts2.attrs_[a], ts2.labels_[y]) for a, y in zip(ts2.state_attr, ts2.state_label)}
    assert state2 == {("a", "x"), ("b", "y"), ("b", "z"), ("c", "z")}
    trans2 = {(ts2.labels_[i], ts2.labels_[j]) for i, j in zip(ts2.trans_src, ts2.trans_dst)}
    assert trans2 == {("x", "z"), ("z", "z")}
    # all_possible_* keep their meaning
    ts3 = train.build_training_set(SEQS, labels, None, all_possible_states=True, all_possible_transitions=True, max_labels=32)
    assert len(ts3.state_attr) == 9 and len(ts3.trans_src) == 9
    # feature ids follow (type, source, destination) order
    assert ts.state_fid[ts.state_attr, ts.state_label].tolist() == list(range(len(ts.state_attr)))


def test_build_training_set_windows_weigh_by_coverage():
    from gecco_amd import train

    seqs = [[["a"], ["b"], ["a"], ["b"]]]
    labels = [["x", {"x", "y"}, "y", "y"]]
    ts = train.build_training_set(seqs, labels, 2, 1, max_labels=32)  # windows 0-1, 1-2, 2-3: coverage 1, 2, 2, 1
    assert ts.allowed.tolist() == [1, 3, 2, 2]
    freq2 = train.build_training_set(seqs, labels, 2, 1, min_freq=2, max_labels=32)
    state = {(freq2.attrs_[a], freq2.labels_[y]) for a, y in zip(freq2.state_attr, freq2.state_label)}
    # (a, x): item 0, coverage 1; (a, y): item 2, coverage 2; (b, x): item 1, coverage 2; (b, y): items 1 and 3, 2 + 1
    assert state == {("a", "y"), ("b", "x"), ("b", "y")}
    trans = {(freq2.labels_[i], freq2.labels_[j]) for i, j in zip(freq2.trans_src, freq2.trans_dst)}
    # pairs 0-1: (x, x), (x, y); 1-2: (x, y), (y, y); 2-3: (y, y), each pair in one window
    assert trans == {("x", "y"), ("y", "y")}
    # an item no window covers names no label and generates nothing
    ts = train.build_training_set([[["a"], ["b"], ["q"]]] * 2, [["x", {"x", "y"}, {"never"}]] * 2, 2, 2, max_labels=32)
    assert ts.labels_ == ["x", "y"] and ts.attrs_ == ["a", "b"] and ts.allowed.tolist() == [1, 3, 1] * 2


@pytest.mark.parametrize("window, step", [(None, None), (2, 1)])
def test_singletons_however_written_are_the_labelled_set(window, step):
    from gecco_amd import train

    plain = [["x", "y", "y"], ["z", "x"], ["y", "x", "x"]]
    written = [[{"x"}, ["y"], ("y",)], [frozenset({"z"}), "x"], ["y", {"x"}, "x"]]
    a = train.build_training_set(SEQS, plain, window, step, max_labels=32)
    b = train.build_training_set(SEQS, written, window, step, max_labels=32)
    assert a.allowed is None and b.allowed is None
    assert set(a.__dict__) == set(b.__dict__)
    for name, va in a.__dict__.items():
        vb = b.__dict__[name]
        if isinstance(va, np.ndarray):
            assert va.dtype == vb.dtype and va.shape == vb.shape and va.tobytes() == vb.tobytes(), name
        else:
            assert va == vb, name


def test_empty_sets_and_none_handling():
    from gecco_amd import train

    with pytest.raises(ValueError, match="empty"):
        train.build_training_set(SEQS, [["x", set(), "y"], ["x", "y"], ["x", "y", "y"]], None, max_labels=32)
    with pytest.raises(ValueError, match="empty"):
        train.build_training_set(SEQS, [["x", [], "y"], ["x", "y"], ["x", "y", "y"]], None, max_labels=32)
    # None where fewer than 2 labels occur overall
    with pytest.raises(ValueError, match="labels"):
        train.build_training_set(SEQS, [["x", None, "x"], [None, "x"], ["x", "x", None]], None, max_labels=32)
    # None is every label of the set, whatever comes after it
    ts = train.build_training_set(SEQS, [[None, "x", "x"], ["y", "x"], ["x", "x", "z"]], None, max_labels=32)
    assert ts.labels_ == ["x", "y", "z"] and ts.allowed[0] == 0b111
    # two labels: a partial set is allowed where exactly two labels are asked for
    ts = train.build_training_set(SEQS, [[None, "x", "x"], ["y", "x"], ["x", "x", {"x", "y"}]], None, max_labels=2)
    assert ts.allowed.tolist() == [3, 1, 1, 2, 1, 1, 1, 3]
    # at 32 labels bit 31 is a label like any other
    names = [f"l{k:02d}" for k in range(32)]
    ts = train.build_training_set([[["a"]] * 33], [names + [None]], None, max_labels=32)
    assert ts.allowed[31] == 1 << 31 and ts.allowed[32] == 0xFFFFFFFF and ts.allowed.dtype == np.uint32


def test_scratch_restatements_grow_by_the_second_log_alpha():
    from gecco_amd import train

    plain = [["x", "y", "y"], ["z", "x"], ["y", "x", "x"]]
    partial = [["x", {"y", "z"}, "y"], ["z", "x"], ["y", "x", "x"]]
    for window, step, mirror in ((None, None, train._sequences_scratch_bytes), (2, 1, train._general_scratch_bytes)):
        a = train.build_training_set(SEQS, plain, window, step, max_labels=32)
        b = train.build_training_set(SEQS, partial, window, step, max_labels=32)
        instances_items = 8 if window is None else (2 + 1 + 2) * 2
        assert mirror(b) - mirror(a) == 8 * instances_items * 3


# ---------------------------------------------------------------- the optimiser's safeguard
def _double_well(x):
    """sum of x^4 / 4 - x^2 / 2: concave inside |x| < 1 / sqrt(3), minima at +-1."""
    return float(np.sum(x ** 4 / 4 - x ** 2 / 2)), x ** 3 - x


def test_minimize_skips_pairs_without_positive_curvature():
    from gecco_amd import train

    x0, c1 = np.array([0.1, 0.1]), 0.01
    # the first accepted step stays inside the concave region: that pair has y.s <= 0
    accepted = [x0]
    res = train.minimize(_double_well, x0, c1=c1, skip_nonpositive_curvature=True,
                         callback=lambda k, f, x: accepted.append(x.copy()))
    pairs = [(b - a, _double_well(b)[1] - _double_well(a)[1]) for a, b in zip(accepted, accepted[1:])]
    assert any(float(np.dot(y, s)) <= 0 for s, y in pairs)
    start = _double_well(x0)[0] + c1 * float(np.abs(x0).sum())
    assert np.isfinite(res.f) and np.isfinite(res.x).all() and res.f < start
    assert res.status in ("converged", "delta test", "line search failed")
    # it reaches the minimum of x^4 / 4 - x^2 / 2 + c1 |x| on the positive side, x^3 - x + c1 = 0
    root = max(np.roots([1.0, 0.0, -1.0, c1]).real)
    assert np.abs(res.x - root).max() <= 1e-3


def test_minimize_keyword_leaves_convex_fits_alone():
    from gecco_amd import train

    rng = np.random.default_rng(1)
    Q = rng.normal(size=(6, 6))
    Q = Q @ Q.T + np.eye(6)
    b = rng.normal(size=6)

    def fg(x):
        return float(0.5 * x @ Q @ x - b @ x), Q @ x - b

    for c1 in (0.0, 0.05):
        runs = []
        for kw in ({}, {"skip_nonpositive_curvature": False}, {"skip_nonpositive_curvature": True}):
            its = []
            res = train.minimize(fg, np.zeros(6), c1=c1, callback=lambda k, f, x: its.append((k, f, x.tobytes())), **kw)
            runs.append((its, res.x.tobytes(), res.f, res.n_iter, res.n_eval, res.status))
        assert runs[0] == runs[1] == runs[2]  # (a convex objective has y.s > 0 on every pair: nothing is ever skipped)
        assert runs[0][5] in ("converged", "delta test", "line search failed")


# ---------------------------------------------------------------- the refusals of the partial creates
def _problem(L=3, window=None):
    rng = np.random.default_rng(9)
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, [4, 3], 5, L)
    sfid, tfid = np.arange(5 * L, dtype=np.int32), 5 * L + np.arange(L * L, dtype=np.int32)
    args = (seq_ptr, item_ptr, attr_id, None, 5, sfid, tfid, 5 * L + L * L)  # (the labels of a problem with masks are not read)
    return (args if window is None else args + (window, 1)), tp.singleton_masks(labels)


@pytest.mark.parametrize("device", [0, 99])
@pytest.mark.parametrize("whole", [False, True])
def test_create_partial_refuses_bad_masks_before_the_device(whole, device):
    from gecco_amd import _native as nat

    family, name = (nat.TrainerSequences, "trainer sequences") if whole else (nat.TrainerGeneral, "trainer general")
    problem, masks = _problem(3, None if whole else 2)
    good, _ = _problem(3, None if whole else 2)
    zero = masks.copy()
    zero[5] = 0
    with pytest.raises(ValueError, match=rf"^{name}: problem 1: item 5 allows no label"):
        family([good, problem], device=device, allowed=[masks, zero])
    high = masks.copy()
    high[2] |= 1 << 3
    with pytest.raises(ValueError, match=rf"^{name}: problem 0: item 2 allows a label at or above num_labels = 3"):
        family([problem, good], device=device, allowed=[high, masks])
    top = masks.copy()
    top[6] = 1 << 31
    with pytest.raises(ValueError, match=rf"^{name}: problem 0: item 6 allows a label at or above"):
        family([problem], device=device, allowed=[top])
    # the wrapper's own checks
    with pytest.raises(ValueError, match="2 entries for 1 problems"):
        family([problem], device=device, allowed=[masks, masks])
    with pytest.raises(ValueError, match="hold 3 entries, the problem 7 items"):
        family([problem], device=device, allowed=[masks[:3]])
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        family([problem], device=device, allowed=[masks.astype(np.int64) - 5])


def test_bit_31_is_a_legal_label_at_32_labels():
    """At L = 32 a mask of bit 31 alone passes the host checks: what is refused afterwards, on a box without a device, is the
    device."""
    from gecco_amd import _native as nat

    L = 32
    seq_ptr, item_ptr, attr_id, _ = labelled_sequences(np.random.default_rng(2), [3], 4, L)
    sfid, tfid = np.arange(4 * L, dtype=np.int32), 4 * L + np.arange(L * L, dtype=np.int32)
    problem = (seq_ptr, item_ptr, attr_id, None, 4, sfid, tfid, 4 * L + L * L)
    masks = np.array([1 << 31, 0xFFFFFFFF, 1 << 31], dtype=np.uint32)
    try:
        nat.TrainerSequences([problem], device=99, allowed=[masks])
    except nat.NativeError as err:  # (ENODEV: the masks were accepted)
        assert "device" in str(err)
    else:
        pytest.fail("device 99 was accepted")


def test_abi_2_14_exports_the_partial_creates():
    from gecco_amd import _native as nat

    lib = nat.load_library()
    assert lib.gecco_crf_version() == 340
    for symbol in ("gecco_crf_trainer_general_create_partial", "gecco_crf_trainer_sequences_create_partial"):
        assert getattr(lib, symbol) is not None


# ---------------------------------------------------------------- the typed front end's labels
def test_typed_labels_with_unknown_any():
    from gecco_amd import typed
    from tests.test_typed_yardstick import _join, _table

    table = _table(["c3", "c1", "c2", "c4"], ["Polyketide", "Unknown", "NRP;Polyketide", ""])
    join = _join([[0, 1, 2], [5, 6], [8, 9], [10]], 12)
    every = frozenset({"Polyketide", "NRP;Polyketide"})
    assert typed.gene_labels(12, table, join, unknown="any") == (
        ["Polyketide"] * 3 + ["0", "0"] + [every] * 2 + ["0"] + ["NRP;Polyketide"] * 2 + [every, "0"])
    assert typed.gene_labels(12, table, join) == typed.gene_labels(12, table, join, unknown="label")
    assert "Unknown" in typed.gene_labels(12, table, join)
    # no cluster with a type: nothing an untyped cluster's genes could be
    with pytest.raises(ValueError, match="at least one cluster with a type"):
        typed.gene_labels(6, _table(["c1", "c2"], ["", "Unknown"]), _join([[0], [3]], 6), unknown="any")
    with pytest.raises(ValueError, match="'label' or 'any'"):
        typed.gene_labels(6, table, join, unknown="some")
    with pytest.raises(ValueError, match="'label' or 'any'"):
        typed.TypedClusterCRF(unknown="some")
    # fold_labels counts only real labels: 31 typed labels and an untyped cluster fit with "any", not with "label"
    ids = [f"c{k:02d}" for k in range(32)]
    table = _table(ids, [f"T{k:02d}" for k in range(31)] + [""])
    join = _join([[k] for k in range(32)], 33)
    labels = typed.gene_labels(33, table, join, unknown="any")
    assert labels[31] == frozenset(f"T{k:02d}" for k in range(31)) and labels[32] == "0"
    with pytest.raises(ValueError, match="32 cluster labels"):
        typed.gene_labels(33, table, join)
    assert typed.build_parser().parse_args(["train", "-f", "f", "-g", "g", "-c", "c", "--unknown", "any"]).unknown == "any"
    assert typed.build_parser().parse_args(["train", "-f", "f", "-g", "g", "-c", "c"]).unknown == "label"
