"""Partially labelled training on the device: the ``*_create_partial`` trainers against the independent numpy yardstick
(tests/train_objective_partial.py) at every lane-group size and the first label count past it, on whole sequences and on
windows, with masks and weights at their edges; the bit contracts; singleton and full masks against what they must equal;
values, scratch, and the fits through ``SequenceCRF`` and ``TypedClusterCRF(unknown="any")``."""
import hashlib
import random

import numpy as np
import pytest

from tests import train_objective_partial as tp
from tests.train_objective_labels import labelled_sequences, objective, objective_tolerances, same_bits
from tests.train_objective_sequences import objective_sequences, objective_sequences_tolerances

pytestmark = pytest.mark.gpu

LABEL_COUNTS = [2, 3, 4, 5, 8, 9, 16, 17, 32]  # each lane-group size G and the first L past it
SEQUENCE_LENGTHS = [1, 2, 3, 7, 64, 65, 200]
THREADS = 256


def _group(L):
    G = 2
    while G < L:
        G *= 2
    return G


def _family(whole):
    from gecco_amd import _native

    return _native.TrainerSequences if whole else _native.TrainerGeneral


def _features(rng, A, L, drop=0.1):
    fid = np.arange(A * L + L * L, dtype=np.int32)
    fid[rng.random(len(fid)) < drop] = -1
    fid[[int(rng.integers(0, A * L)), A * L + int(rng.integers(0, L * L))]] = -1
    keep = fid >= 0
    fid[keep] = np.arange(int(keep.sum()))
    return fid[:A * L], fid[A * L:], int(keep.sum())


def _problem(rng, L, lengths, W=None, step=None, A=12):
    """(problem as the trainer takes it, its true labels); the labels entry of the problem is None: nothing reads it."""
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, lengths, A, L, stay=0.8)
    sfid, tfid, K = _features(rng, A, L)
    p = (seq_ptr, item_ptr, attr_id, None, A, sfid, tfid, K)
    return (p if W is None else p + (W, step)), labels


def _neighbour(rng, whole):
    """A small labelled problem of another label count, to sit beside the one under test."""
    seq_ptr, item_ptr, attr_id, labels = labelled_sequences(rng, [6, 9, 7], 5, 3)
    p = (seq_ptr, item_ptr, attr_id, labels, 5, np.arange(15, dtype=np.int32), 15 + np.arange(9, dtype=np.int32), 24)
    return p if whole else p + (3, 1)


def _reference(p, masks, w):
    L = np.asarray(p[5]).size // p[4]
    W, step = (p[8], p[9]) if len(p) == 10 else (None, None)
    f, g, count, groups = tp.objective_partial(p[0], p[1], p[2], masks, p[4], L, W, step, p[5], p[6], w, details=True)
    return f, g, count, tp.partial_tolerances(L, groups)


def check(p, masks, weights, rng):
    """Problem `p` with `masks` at every w of `weights`: f and g finite and within the derived bounds of the yardstick, the
    same bytes from a second evaluation, and the same bytes beside a labelled problem in one trainer.  Returns the last (f,
    g, tol_f, tol_g)."""
    whole = len(p) == 8
    L = np.asarray(p[5]).size // p[4]
    other = _neighbour(rng, whole)
    tr = _family(whole)([p], allowed=[masks])
    pair = _family(whole)([other, p], allowed=[None, masks])
    for name, w in weights:
        f, g = tr.eval([w])
        ef, eg, count, (tol_f, tol_g) = _reference(p, masks, w)
        assert tr.num_windows(0) == count
        assert np.isfinite(ef) and np.isfinite(eg).all()
        assert np.isfinite(f[0]) and np.isfinite(g[0]).all(), (name, f[0], int(np.count_nonzero(~np.isfinite(g[0]))))
        err = np.abs(g[0] - eg)
        print(f"L={L} {'sequences' if whole else f'W={p[8]} step={p[9]}'} {name}: |f - ref| = {abs(f[0] - ef):.3g} (bound "
              f"{tol_f:.3g}), max |g - ref| / bound = {(err / np.maximum(tol_g, 1e-300)).max() if len(err) else 0.0:.3g}")
        assert abs(f[0] - ef) <= tol_f, (name, f[0], ef, tol_f)
        assert np.all(err <= tol_g), (name, int(np.argmax(err / np.maximum(tol_g, 1e-300))), float(err.max()))
        f2, g2 = tr.eval([w])
        assert same_bits(f[0], g[0], f2[0], g2[0]), name
        fb, gb = pair.eval([rng.normal(size=other[7]), w])
        assert same_bits(f[0], g[0], fb[1], gb[1]), name
    return f[0], g[0], tol_f, tol_g


def _weights(rng, K):
    return [("zero", np.zeros(K)), ("normal", rng.normal(0, 1, size=K))]


def _dominant_excluded(rng, p, L):
    """(masks, w): every state weight of label d is +700 and every other -700, and every item's mask is everything but d, so
    the excluded label carries essentially all of the free mass."""
    d = int(rng.integers(0, L))
    n = int(p[0][-1])
    masks = np.full(n, ((1 << L) - 1) & ~(1 << d), dtype=np.uint32)
    w = rng.normal(0, 1, size=p[7])
    sfid = np.asarray(p[5]).reshape(p[4], L)
    for y in range(L):
        ids = sfid[:, y][sfid[:, y] >= 0]
        w[ids] = 700.0 if y == d else -700.0
    return masks, w


def _special(rng, L, n_items, instance, lone):
    """Random masks with, planted in them: an instance (`instance`: its items) that is full everywhere but at its middle
    item, which names one label; the item `lone` (a length-1 instance where there is one) with a two-label set; and at 32
    labels two items with bit 31 alone."""
    masks = tp.random_masks(rng, n_items, L)
    masks[instance] = (1 << L) - 1
    masks[instance[len(instance) // 2]] = 1 << int(rng.integers(0, L))
    if lone is not None:
        masks[lone] = 0b11
    if L == 32:
        free = [i for i in range(n_items) if i != lone and i not in set(instance.tolist())][:2]
        masks[free] = np.uint32(1 << 31)
        assert len(free) == 2
    return masks


# ---------------------------------------------------------------- whole sequences
@pytest.mark.parametrize("L", LABEL_COUNTS)
def test_sequences_against_the_yardstick(L):
    """256 / G + 1 sequences of the lengths 1, 2, 3, 7, 64, 65, 200 mixed: a second workgroup with one occupied slot."""
    rng = np.random.default_rng(9100 + L)
    count = THREADS // _group(L) + 1
    lengths = [SEQUENCE_LENGTHS[k % len(SEQUENCE_LENGTHS)] for k in range(count)]
    rng.shuffle(lengths)
    p, labels = _problem(rng, L, lengths)
    n = int(p[0][-1])
    assert _family(True)([p], allowed=[tp.singleton_masks(labels)]).num_sequences(0) == count
    longest = int(np.argmax(lengths))
    instance = np.arange(p[0][longest], p[0][longest + 1])
    lone = int(p[0][lengths.index(1)])
    for masks in (tp.random_masks(rng, n, L), _special(rng, L, n, instance, lone)):
        check(p, masks, _weights(rng, p[7]), rng)
    masks, w = _dominant_excluded(rng, p, L)
    f, _, _, _ = check(p, masks, [("+-700, dominant label excluded", w)], rng)
    assert f > 700.0  # (the free mass sits on the excluded label: log Z - log Z_A is large, and finite)


@pytest.mark.parametrize("L", LABEL_COUNTS)
def test_sequences_singleton_and_full_masks(L):
    """Singletons through the partial entry agree with the labelled trainer within the sum of both sides' bounds; all-full
    masks give |f| and |g| within the bounds of 0."""
    rng = np.random.default_rng(9200 + L)
    count = THREADS // _group(L) + 1
    lengths = [SEQUENCE_LENGTHS[k % len(SEQUENCE_LENGTHS)] for k in range(count)]
    p, labels = _problem(rng, L, lengths)
    labelled = p[:3] + (labels,) + p[4:]
    weights = _weights(rng, p[7])
    f, g, tol_f, tol_g = check(p, tp.singleton_masks(labels), weights, rng)
    w = weights[-1][1]
    lf, lg = _family(True)([labelled]).eval([w])
    ltol_f, ltol_g = objective_sequences_tolerances(*labelled[:5], L, p[5], p[6], w)
    ef, eg, _ = objective_sequences(*labelled[:5], L, p[5], p[6], w)
    assert abs(lf[0] - ef) <= ltol_f and np.all(np.abs(lg[0] - eg) <= ltol_g)
    assert abs(f - lf[0]) <= tol_f + ltol_f and np.all(np.abs(g - lg[0]) <= tol_g + ltol_g)
    f, g, tol_f, tol_g = check(p, tp.full_masks(int(p[0][-1]), L), weights, rng)
    assert abs(f) <= tol_f and np.all(np.abs(g) <= tol_g)


# ---------------------------------------------------------------- windows
def _window_lengths(W, step, windows=129):
    """Three sequences with `windows` windows in all (one past a workgroup's 128), the last with items no window covers
    where the step allows."""
    counts = [1, 40, windows - 41]
    return [W + (c - 1) * step + (step - 1 if k == 2 else 0) for k, c in enumerate(counts)]


@pytest.mark.parametrize("W", [1, 2, 5, 20, 32])
@pytest.mark.parametrize("L", LABEL_COUNTS)
def test_windows_against_the_yardstick(L, W):
    rng = np.random.default_rng(9300 + 40 * L + W)
    for step in sorted({1, W}):
        p, labels = _problem(rng, L, _window_lengths(W, step), W, step)
        n = int(p[0][-1])
        start = int(p[0][1]) + 3 * step  # (a window of the second sequence)
        instance = np.arange(start, start + W)
        lone = 0 if W == 1 else None  # (W = 1: every instance has one item)
        if W == 1:
            instance = np.arange(5, 6)
        masks = _special(rng, L, n, instance, lone)
        f, g, tol_f, tol_g = check(p, masks, _weights(rng, p[7]), rng)
        masks, w = _dominant_excluded(rng, p, L)
        check(p, masks, [("+-700, dominant label excluded", w)], rng)
        # singletons against the labelled trainer, and all-full masks against 0
        w = rng.normal(0, 1, size=p[7])
        f, g, tol_f, tol_g = check(p, tp.singleton_masks(labels), [("singletons", w)], rng)
        labelled = p[:3] + (labels,) + p[4:]
        lf, lg = _family(False)([labelled]).eval([w])
        ef, eg, _, details = objective(*labelled[:5], L, W, step, p[5], p[6], w, details=True)
        ltol_f, ltol_g = objective_tolerances(p[0], p[1], p[2], L, W, step, p[5], p[6], w, details)
        assert abs(lf[0] - ef) <= ltol_f and np.all(np.abs(lg[0] - eg) <= ltol_g)
        assert abs(f - lf[0]) <= tol_f + ltol_f and np.all(np.abs(g - lg[0]) <= tol_g + ltol_g)
        f, g, tol_f, tol_g = check(p, tp.full_masks(n, L), [("full", w)], rng)
        assert abs(f) <= tol_f and np.all(np.abs(g) <= tol_g)


# ---------------------------------------------------------------- values, mixing, scratch
@pytest.mark.parametrize("whole", [False, True])
def test_values_of_one_have_the_unvalued_bits(whole):
    rng = np.random.default_rng(17 + whole)
    L = 5
    p, labels = _problem(rng, L, [9, 30, 12, 7, 20], *(() if whole else (5, 2)))
    masks, _ = tp.hide_labels(rng, labels, L)
    w = rng.normal(0, 1, size=p[7])
    f, g = _family(whole)([p], allowed=[masks]).eval([w])
    ones = np.ones(len(p[2]))
    fv, gv = _family(whole)([p], allowed=[masks], values=[ones]).eval([w])
    assert same_bits(f[0], g[0], fv[0], gv[0])
    # values that are not 1 move the state gradient, and the objective still reproduces
    half = _family(whole)([p], allowed=[masks], values=[0.5 * ones])
    fh, gh = half.eval([w])
    fh2, gh2 = half.eval([w])
    assert same_bits(fh[0], gh[0], fh2[0], gh2[0]) and not same_bits(f[0], g[0], fh[0], gh[0])
    assert np.isfinite(fh[0]) and np.isfinite(gh[0]).all()


@pytest.mark.parametrize("whole", [False, True])
def test_labelled_problems_keep_their_bits_beside_partial_ones(whole):
    """A problem without masks in a trainer made by the partial create has the bits of the labelled create."""
    rng = np.random.default_rng(23 + whole)
    other = _neighbour(rng, whole)
    p, labels = _problem(rng, 4, [9, 30, 12], *(() if whole else (5, 1)))
    w = rng.normal(size=other[7])
    f, g = _family(whole)([other]).eval([w])
    fb, gb = _family(whole)([p, other], allowed=[tp.hide_labels(rng, labels, 4)[0], None]).eval([np.zeros(p[7]), w])
    assert same_bits(f[0], g[0], fb[1], gb[1])


NAMES = [[["a"], ["a", "b"], ["b"], ["c"], ["a"], ["c"]], [["b"], ["c"], ["b"], ["a"], ["c"]], [["a"], ["c"], ["c"], ["b"], ["b"]]]
SETS = [["x", {"y", "z"}, "y", "z", None, "x"], ["z", "x", "x", {"x", "y"}, "y"], ["y", "x", "x", "z", "z"]]


@pytest.mark.parametrize("window, step", [(None, None), (3, 1), (5, 5)])
def test_scratch_bytes_is_the_mirror(window, step):
    from gecco_amd import train

    ts = train.build_training_set(NAMES, SETS, window, step, max_labels=32)
    assert ts.allowed is not None
    whole = window is None
    tr = _family(whole)([ts.native_args()], allowed=[ts.allowed])
    mirror = train._sequences_scratch_bytes if whole else train._general_scratch_bytes
    assert tr.scratch_bytes(0) == tr.scratch_bytes(-1) == mirror(ts)
    valued = train.build_training_set([[[(nm, 1.5) for nm in item] for item in seq] for seq in NAMES], SETS, window, step,
                                      max_labels=32)
    tr = _family(whole)([valued.native_args()], allowed=[valued.allowed], values=[valued.attr_value])
    assert tr.scratch_bytes(0) == mirror(valued) == mirror(ts) + 8 * len(valued.attr_value)


# ---------------------------------------------------------------- fits through SequenceCRF
LABELS = ["A", "B", "C", "D"]
PLANTED_SEED, PLANTED_C2 = 5, 0.05


def planted(seed=PLANTED_SEED, n_seqs=12, n=14, share=0.5):
    """A planted 4-label problem: every label owns an attribute that always fires on its items, beside up to two noise
    attributes; a seeded half of the labels is hidden as {truth, one other label}.  Returns (X, y with the hidden sets, the
    true labels, hidden [per sequence, per item])."""
    rng = np.random.default_rng(seed)
    X, y, truth, hidden = [], [], [], []
    for _ in range(n_seqs):
        lab = int(rng.integers(0, 4))
        xs, ys, ts, hs = [], [], [], []
        for _ in range(n):
            if rng.random() >= 0.7:
                lab = int(rng.integers(0, 4))
            noise = [f"noise_{int(k)}" for k in rng.choice(6, size=int(rng.integers(0, 3)), replace=False)]
            hide = bool(rng.random() < share)
            other = LABELS[(lab + int(rng.integers(1, 4))) % 4]
            xs.append([f"own_{LABELS[lab]}"] + noise)
            ts.append(LABELS[lab])
            ys.append({LABELS[lab], other} if hide else LABELS[lab])
            hs.append(hide)
        X.append(xs), y.append(ys), truth.append(ts), hidden.append(hs)
    return X, y, truth, hidden


def _planted_set(window=None):
    from gecco_amd import train

    X, y, _, _ = planted()
    return train.build_training_set(X, y, window, None if window is None else 1, max_labels=32)


@pytest.fixture(scope="module")
def planted_fit():
    from gecco_amd.sequence import SequenceCRF

    X, y, truth, hidden = planted()
    crf = SequenceCRF(window_size=None, c2=PLANTED_C2).fit(X, y)
    return crf, X, y, truth, hidden


def test_planted_fit_recovers_the_hidden_labels(planted_fit):
    """The device fit labels every hidden item with its truth.  That the objective's optimum does so was established on the
    CPU first: scipy's L-BFGS-B on tests/train_objective_partial.py's objective + c2 |w|^2 of this set (seed 5, c2 = 0.05)
    converged, and the Viterbi labels of its weights equal the truth on every one of the hidden items (and on every
    other item), which is why this seed and this c2 are the ones used."""
    crf, X, y, truth, hidden = planted_fit
    assert sum(h for hs in hidden for h in hs) > 60 and any(not h for hs in hidden for h in hs)
    assert sorted(crf.classes_) == LABELS
    assert crf.predict(X) == truth
    res = crf.training_result_
    assert res.status in ("converged", "delta test", "line search failed", "maximum number of iterations")


def test_planted_fit_objective_reproduces_under_the_yardstick(planted_fit):
    from gecco_amd import _native

    crf = planted_fit[0]
    res = crf.training_result_
    ts = _planted_set()
    L = ts.num_labels
    tr = _native.TrainerSequences([ts.native_args()], allowed=[ts.allowed])
    f0, _ = tr.eval([np.zeros(ts.num_features)])
    f, g = tr.eval([res.x])
    ef, eg, _, groups = tp.objective_partial(ts.seq_ptr, ts.item_ptr, ts.attr_id, ts.allowed, len(ts.attrs_), L, None, None,
                                             ts.state_fid, ts.trans_fid, res.x, details=True)
    tol_f, tol_g = tp.partial_tolerances(L, groups)
    assert abs(f[0] - ef) <= tol_f and np.all(np.abs(g[0] - eg) <= tol_g)
    total = float(f[0]) + PLANTED_C2 * float(np.dot(res.x, res.x))
    assert np.isfinite(res.f) and res.f == total and res.f < float(f0[0])
    assert f0[0] > 0.0


def test_planted_fit_is_reproducible(planted_fit):
    from gecco_amd.sequence import SequenceCRF

    crf, X, y, _, _ = planted_fit
    assert SequenceCRF(window_size=None, c2=PLANTED_C2).fit(X, y).to_bytes() == crf.to_bytes()


@pytest.mark.parametrize("window", [None, 5])
def test_planted_fit_with_l1_ends_with_finite_weights(window):
    from gecco_amd.sequence import SequenceCRF

    X, y, truth, _ = planted()
    crf = SequenceCRF(window_size=window, c1=0.1, c2=PLANTED_C2).fit(X, y)
    res = crf.training_result_
    assert np.isfinite(res.x).all() and np.isfinite(res.f)
    assert res.status in ("converged", "delta test", "line search failed", "maximum number of iterations")
    ts = _planted_set(window)
    from gecco_amd import _native

    family = _native.TrainerSequences if window is None else _native.TrainerGeneral
    f0, _ = family([ts.native_args()], allowed=[ts.allowed]).eval([np.zeros(ts.num_features)])
    assert res.f < float(f0[0])


@pytest.mark.parametrize("window", [None, 5])
def test_singletons_as_sets_give_the_plain_fit(window):
    from gecco_amd.sequence import SequenceCRF

    X, _, truth, _ = planted(n_seqs=6)
    plain = SequenceCRF(window_size=window, c2=PLANTED_C2, max_iterations=30).fit(X, truth)
    written = [[{lab} if k % 2 else [lab] for k, lab in enumerate(seq)] for seq in truth]
    assert SequenceCRF(window_size=window, c2=PLANTED_C2, max_iterations=30).fit(X, written).to_bytes() == plain.to_bytes()


def test_lockstep_and_grid_mix_partial_and_labelled_sets():
    """``fit_training_sets`` and ``fit_grid`` over a partial and a labelled set give the lone fits."""
    from gecco_amd import train

    X, y, truth, _ = planted(n_seqs=6)
    params = train.trainer_params({"c2": PLANTED_C2, "max_iterations": 15})
    for window, step in ((None, None), (5, 1)):
        sets = [train.build_training_set(X, labs, window, step, max_labels=32) for labs in (y, truth)]
        assert sets[0].allowed is not None and sets[1].allowed is None
        lone = [train.fit_training_set(ts, params) for ts in sets]
        for got in (train.fit_training_sets(sets, params), train.fit_grid(sets, [(0, params), (1, params)]),
                    train.fit_grid(sets, [(0, params), (1, params)], scratch_budget_bytes=1)):
            for a, b in zip(got, lone):
                assert a.x.tobytes() == b.x.tobytes() and a.f == b.f and a.status == b.status and a.n_eval == b.n_eval


# ---------------------------------------------------------------- the typed front end
def _typed_tables():
    from tests.typed_planted import cluster_table, planted_set

    train_genes, rows = planted_set(11, 12, "train", composite=False)
    fresh_genes, fresh_rows = planted_set(12, 4, "fresh", composite=False)
    # the second cluster of every fourth contig (one of each type) loses its type; every type keeps clusters that have it
    blanked = ["" if (k % 2 == 1 and (k // 2) % 4 == 0) else r[4] for k, r in enumerate(rows)]
    return train_genes, cluster_table(rows, blanked), cluster_table(rows), fresh_genes, fresh_rows


def test_typed_unknown_any(tmp_path):
    from gecco_amd import typed
    from tests.typed_planted import C, TYPES, W

    train_genes, blanked, _, fresh_genes, fresh_rows = _typed_tables()
    assert "" in list(blanked.type)
    random.seed(42)
    np.random.seed(42)
    crf = typed.TypedClusterCRF(W, 1, unknown="any", c1=C, c2=C).fit(train_genes, blanked)
    assert "Unknown" not in crf.classes_ and sorted(crf.classes_) == sorted(["0"] + TYPES)
    assert np.isfinite(crf.training_result_.x).all()
    crf.save(tmp_path)
    back = typed.TypedClusterCRF.trained(tmp_path)
    assert back.classes_ == crf.classes_
    assert np.array_equal(back.predict_label_probabilities(fresh_genes), crf.predict_label_probabilities(fresh_genes))
    clusters = crf.predict_clusters(fresh_genes)
    for cid, seq, start, end, type_, _ in fresh_rows:
        over = [c for c in clusters if c.source.id == seq and c.start <= end and start <= c.end]
        assert len(over) == 1, (cid, [c.id for c in over])
        assert str(over[0].type) == type_, (cid, str(over[0].type), over[0].type_probabilities)


# the model file of TypedClusterCRF(W, 1, c1=C, c2=C) fitted on the blanked table below under the seeds 42, as the commit
# before ``unknown=`` existed wrote it (its md5, recorded from that commit's build on an MI355X)
PARENT_TYPED_MD5 = "510e9b509f296fb3432877badb2a3069"


def test_typed_unknown_label_is_what_it_was():
    from gecco_amd import typed
    from tests.typed_planted import C, W

    train_genes, blanked, _, _, _ = _typed_tables()
    blobs = []
    for kw in ({}, {"unknown": "label"}):
        random.seed(42)
        np.random.seed(42)
        crf = typed.TypedClusterCRF(W, 1, c1=C, c2=C, **kw).fit(train_genes, blanked)
        assert "Unknown" in crf.classes_
        blobs.append(crf._blob)
    assert blobs[0] == blobs[1]
    print("typed model md5:", hashlib.md5(blobs[0]).hexdigest())
    assert hashlib.md5(blobs[0]).hexdigest() == PARENT_TYPED_MD5
