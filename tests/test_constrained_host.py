"""Inference under allowed-label sets, the parts that need no device: the numpy yardstick (tests/constrained_reference.py)
against path enumeration, the set grammar of ``SequenceCRF`` (``allowed=`` and ``log_likelihood``'s ``y``), the four
``*_constrained`` symbols with their host refusals, and the masks the typed front end builds from a ``known`` table."""
import numpy as np
import pytest

from gecco_amd import _native as nat
from tests import constrained_reference as cr
from tests import train_objective_partial as tp
from tests import train_objective_valued as tv

SYMBOLS = ("gecco_crf_viterbi_constrained", "gecco_crf_marginals_full_constrained", "gecco_crf_windowed_marginals_constrained",
           "gecco_crf_windowed_marginals_all_constrained")


# ---------------------------------------------------------------- the yardstick against enumeration
@pytest.mark.parametrize("L", [2, 3])
def test_the_yardstick_against_path_enumeration(L):
    rng = np.random.default_rng(70 + L)
    A = 6
    for trial in range(12):
        T_len = int(rng.integers(1, 7))
        S, T = rng.normal(size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
        deg = rng.integers(0, 4, size=T_len)
        gptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
        attr = rng.integers(0, A, size=int(gptr[-1])).astype(np.int32)
        values = None if trial % 2 else rng.normal(size=len(attr))
        allowed = tp.random_masks(rng, T_len, L)
        score = cr.masked_scores(gptr, attr, values, S, allowed)
        assert np.array_equal(np.isinf(score), ~tp.mask_matrix(allowed, L))
        cptr = np.array([0, T_len])
        marg, logz = cr.marginals(cptr, score, T)
        y, best = cr.viterbi(cptr, score, T)
        e_logz, e_marg, e_best, e_paths = cr.enumerate_paths(score, T)
        assert abs(logz[0] - e_logz) <= 1e-12 * max(1.0, abs(e_logz))
        assert np.abs(marg - e_marg).max() <= 1e-12 and np.all(marg[np.isinf(score)] == 0.0)
        assert tuple(y.tolist()) in e_paths and abs(best - e_best) <= 1e-12 * max(1.0, abs(e_best))
        assert np.all(np.isfinite(score[np.arange(T_len), y]))
        # the vectorised recursion is CRFsuite's loop
        ly, lbest = tv.viterbi_scores(score, T)
        assert np.array_equal(ly, y) and lbest == best
        # one window over the whole sequence is the whole-sequence marginal; the non-background sum likewise
        p_all, p_any = cr.windowed(cptr, score, T, T_len, 1, background=0)
        assert np.abs(p_all - e_marg).max() <= 1e-12 and np.abs(p_any - e_marg[:, 1:].sum(axis=1)).max() <= 1e-12


def test_the_yardstick_on_exact_ties_takes_the_first_arg_max():
    rng = np.random.default_rng(5)
    L, n = 3, 6
    for _ in range(20):
        score = rng.integers(-2, 3, size=(n, L)).astype(float)
        T = rng.integers(-1, 2, size=(L, L)).astype(float)
        score[~tp.mask_matrix(tp.random_masks(rng, n, L), L)] = -np.inf
        y, best = cr.viterbi_one(score, T)
        ly, lbest = tv.viterbi_scores(score, T)
        assert np.array_equal(y, ly) and best == lbest
        assert best == cr.enumerate_paths(score, T)[2]


def test_padding_items_allow_every_label():
    """A sequence shorter than the window: the padded window is the enumeration over W items whose padding rows are 0."""
    rng = np.random.default_rng(9)
    L, W = 3, 5
    T = rng.normal(size=(L, L))
    score = rng.normal(size=(2, L))
    score[0, 1] = score[1, 0] = -np.inf
    p_all, _ = cr.windowed(np.array([0, 2]), score, T, W, 1, background=0)
    X = np.zeros((W, L))
    X[1:3] = score  # ((5 - 2) // 2 = 1 empty item in front)
    e_marg = cr.enumerate_paths(X, T)[1]
    assert np.abs(p_all - e_marg[1:3]).max() <= 1e-12 and p_all[0, 1] == 0.0 and p_all[1, 0] == 0.0


# ---------------------------------------------------------------- SequenceCRF's grammar
@pytest.fixture(scope="module")
def crf():
    from gecco_amd.crfsuite_model import model_bytes
    from gecco_amd.sequence import SequenceCRF

    labels, attrs = ["a", "b", "c"], ["x", "y"]
    sa, sl = np.repeat(np.arange(2), 3), np.tile(np.arange(3), 2)
    ts, td = np.repeat(np.arange(3), 3), np.tile(np.arange(3), 3)
    w = np.random.default_rng(1).normal(size=len(sa) + len(ts))
    return SequenceCRF.from_bytes(model_bytes(labels, attrs, sa, sl, ts, td, w), window_size=None, device=99)


def test_the_set_grammar(crf):
    assert crf.classes_ == ["a", "b", "c"]
    seq_ptr = np.array([0, 4, 4, 6])
    masks, single = crf._label_sets([["a", {"a", "c"}, None, ("b",)], [], [frozenset({"b", "c"}), ["c", "a", "c"]]], seq_ptr, "allowed")
    assert masks.dtype == np.uint32 and masks.tolist() == [1, 5, 7, 2, 6, 5] and not single
    masks, single = crf._label_sets([["a", {"c"}, ("b",), "b"], [], [["a"], "c"]], seq_ptr, "y")
    assert masks.tolist() == [1, 4, 2, 2, 1, 4] and single


@pytest.mark.parametrize("method", ["predict", "predict_marginals", "log_likelihood"])
def test_the_grammar_errors_come_before_the_device(crf, method):
    """(device 99 does not exist: a call that reached the device would raise something else)"""
    X = [[["x"], ["y"], ["x", "y"]], [["x"]]]
    call = (lambda sets: crf.log_likelihood(X, sets)) if method == "log_likelihood" else \
        (lambda sets: getattr(crf, method)(X, allowed=sets))
    with pytest.raises(ValueError, match="unknown label 'z'"):
        call([["a", {"a", "z"}, None], ["b"]])
    with pytest.raises(ValueError, match="an empty set allows no label"):
        call([["a", set(), None], ["b"]])
    with pytest.raises(ValueError, match="sequence 0: 3 items but 2 labels"):
        call([["a", None], ["b"]])
    with pytest.raises(ValueError, match="X holds 2 sequences"):
        call([["a", None, None]])


def test_windowed_methods_take_allowed(crf):
    from gecco_amd.sequence import SequenceCRF

    windowed = SequenceCRF.from_bytes(crf.to_bytes(), window_size=2, device=99)
    X = [[["x"], ["y"]]]
    for call in (lambda s: windowed.predict_windowed(X, "a", allowed=s), lambda s: windowed.predict_windowed_all(X, allowed=s)):
        with pytest.raises(ValueError, match="unknown label 'z'"):
            call([["a", {"z"}]])
    # nothing to decode: no device needed, the sets are still checked
    assert crf.predict([[]], allowed=[[]]) == [[]] and crf.log_likelihood([[]], [[]]).tolist() == [0.0]
    assert crf.log_likelihood([], []).tolist() == []
    with pytest.raises(ValueError, match="0 items but 1 labels"):
        crf.predict([[]], allowed=[[None]])


def test_native_allowed_size_mismatch():
    m = nat.Model.from_tables(np.zeros((2, 3)), np.zeros((3, 3)))
    cptr, gptr, attr = np.array([0, 2], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    for call in (lambda a: m.viterbi(cptr, gptr, attr, device=99, allowed=a), lambda a: m.marginals_full(cptr, gptr, attr, device=99, allowed=a),
                 lambda a: m.windowed_marginals(cptr, gptr, attr, 2, device=99, allowed=a),
                 lambda a: m.windowed_marginals_all(cptr, gptr, attr, 2, device=99, allowed=a)):
        with pytest.raises(ValueError, match="allowed holds 3 masks for 2 genes"):
            call(np.array([1, 1, 1], dtype=np.uint32))
        with pytest.raises(ValueError, match="allows no label"):  # (EINVAL from the host checks of the entry)
            call(np.array([1, 0], dtype=np.uint32))


# ---------------------------------------------------------------- the C entries
def test_the_symbols_exist_and_the_version_stays():
    lib = nat.load_library()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.gecco_crf_version() == 340


L3 = 3
ENTRIES = {
    "viterbi": ("gecco_crf_viterbi_constrained", ("y_out", "score")),
    "full": ("gecco_crf_marginals_full_constrained", ("marg", "lognorm")),
    "windowed": ("gecco_crf_windowed_marginals_constrained", ("window", "step", "label", "pad", "p_out")),
    "all": ("gecco_crf_windowed_marginals_all_constrained", ("window", "step", "background", "pad", "p_all", "p_any")),
}


def _call(model, entry, **change):
    """A valid batch of two contigs (2 and 3 genes) on a device that does not exist, with `change` applied."""
    symbol, tail = ENTRIES[entry]
    a = {"contig_ptr": np.array([0, 2, 5], dtype=np.int32), "n_contigs": 2, "gene_ptr": np.arange(0, 12, 2, dtype=np.int32),
         "attr_id": (np.arange(10, dtype=np.int32) * 3) % 7, "attr_value": None,
         "allowed": np.array([7, 1, 6, 4, 3], dtype=np.uint32),
         "window": 5, "step": 2, "label": 1, "background": 0, "pad": 1,
         "p_out": np.zeros(5), "p_all": np.zeros(5 * L3), "p_any": np.zeros(5), "marg": np.zeros(5 * L3), "lognorm": np.zeros(2),
         "y_out": np.zeros(5, dtype=np.int8), "score": np.zeros(2)}
    a.update(change)
    fn = getattr(nat.load_library(), symbol)
    names = ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed") + tail
    args = [a[n] if a[n] is None or not isinstance(a[n], np.ndarray) else a[n].ctypes.data_as(t) for n, t in zip(names, fn.argtypes[2:])]
    rc = fn(model._h, 99, *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


@pytest.fixture(scope="module")
def model3():
    rng = np.random.default_rng(5)
    return nat.Model.from_tables(rng.normal(size=(7, L3)), rng.normal(size=(L3, L3)))


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_host_refusals_come_before_the_device(model3, entry):
    assert _call(model3, entry, allowed=np.array([7, 1, 0, 4, 3], dtype=np.uint32)) == \
        (nat.EINVAL, "constrained: gene 2 allows no label (a mask of 0)")
    rc, msg = _call(model3, entry, allowed=np.array([7, 1, 6, 4, 8 | 1], dtype=np.uint32))
    assert rc == nat.EINVAL and msg == "constrained: gene 4 allows a label at or above num_labels = 3 (mask 9)"
    rc, msg = _call(model3, entry, allowed=np.array([7, 1, 6, 4, 1 << 31], dtype=np.uint32))
    assert rc == nat.EINVAL and "at or above num_labels = 3" in msg
    rc, msg = _call(model3, entry, allowed=None)
    assert rc == nat.EINVAL and msg.startswith("null allowed with genes")
    # a valid batch gets past the host checks: what stops it is the device that does not exist
    assert _call(model3, entry)[0] not in (nat.OK, nat.EINVAL)
    # values, when given, are checked as the valued entries check them
    v = np.ones(10)
    v[3] = np.nan
    assert _call(model3, entry, attr_value=v) == (nat.EINVAL, "attribute value 3 is not finite (NaN or infinite)")


def test_masks_are_indexed_by_the_callers_gene(model3):
    """contig_ptr[0] = 2: genes 0 and 1 are not part of the batch, and their masks are not looked at."""
    sliced = {"contig_ptr": np.array([2, 5], dtype=np.int32), "n_contigs": 1}
    assert _call(model3, "viterbi", allowed=np.array([0, 99, 6, 4, 3], dtype=np.uint32), **sliced)[0] not in (nat.OK, nat.EINVAL)
    assert _call(model3, "viterbi", allowed=np.array([7, 7, 6, 0, 3], dtype=np.uint32), **sliced) == \
        (nat.EINVAL, "constrained: gene 3 allows no label (a mask of 0)")


def test_a_batch_without_genes_needs_no_masks(model3):
    empty = {"contig_ptr": np.zeros(4, dtype=np.int32), "n_contigs": 3, "allowed": None}
    assert _call(model3, "viterbi", y_out=None, **empty)[0] == nat.OK
    assert _call(model3, "full", marg=None, lognorm=None, **empty)[0] == nat.OK
    # (with outputs asked for, the host checks pass and the call goes on to the device)
    for entry in ENTRIES:
        rc, msg = _call(model3, entry, **empty)
        assert rc != nat.EINVAL, msg


def test_the_two_label_window_limit_is_a_plan_matter():
    """The masked plan takes the any-L kernels at two labels too: the window checks in front of the device are the shared
    ones."""
    m = nat.Model.from_tables(np.zeros((7, 2)), np.zeros((2, 2)))
    rc, msg = _call(m, "windowed", window=0, allowed=np.array([3, 1, 2, 3, 3], dtype=np.uint32))
    assert (rc, msg) == (nat.EINVAL, "Window size must be strictly positive")


# ---------------------------------------------------------------- the typed front end's masks
class _Join:
    """A hand-made overlap join: the genes of every clusters-table row."""

    def __init__(self, members):
        self._members = [np.array(m, dtype=np.int64) for m in members]

    def members(self, i):
        return self._members[i]


def test_typed_masks_from_a_known_table():
    from gecco_amd import tables, typed

    classes = ["0", "Alpha", "Beta", "Alpha;Beta"]
    known = tables.ClusterTable({"sequence_id": ["s"] * 5, "cluster_id": ["c2", "c1", "c3", "c4", "c0"],
                                 "start": [1] * 5, "end": [2] * 5,
                                 "type": ["Beta", "Alpha", "Gamma", "Beta;Alpha", "Unknown"]})
    # rows in table order: c2 (Beta) genes 2-4; c1 (Alpha) genes 4-5; c3 (Gamma: no such label) gene 7; c4 (Alpha;Beta,
    # sorted) genes 8-9; c0 (no type) genes 9-10
    join = _Join([[2, 3, 4], [4, 5], [7], [8, 9], [9, 10]])
    masks = typed.known_masks(12, known, join, classes)
    every, cluster = 0b1111, 0b1110
    assert masks.dtype == np.uint32
    assert masks.tolist() == [every, every, 0b0100, 0b0100, 0b0010,  # gene 4 is under c1 and c2: c1 comes first by id
                              0b0010, every, cluster, 0b1000, cluster,  # gene 9: c0 (untyped) sorts before c4
                              cluster, every]
    # no known row with a gene: every label everywhere
    assert typed.known_masks(3, known, _Join([[], [], [], [], []]), classes).tolist() == [every] * 3
    # the background as a known type does not pin the gene to the background
    bg = tables.ClusterTable({"sequence_id": ["s"], "cluster_id": ["c"], "start": [1], "end": [2], "type": ["0"]})
    assert typed.known_masks(2, bg, _Join([[1]]), classes).tolist() == [every, cluster]
    with pytest.raises(ValueError, match="no background label"):
        typed.known_masks(2, bg, _Join([[1]]), ["Alpha", "Beta"])


def test_the_command_line_takes_known():
    from gecco_amd import typed

    args = typed.build_parser().parse_args(["predict", "--model", "m", "-f", "f.tsv", "-g", "g.tsv", "--known", "K.tsv"])
    assert args.known == "K.tsv"
    assert typed.build_parser().parse_args(["predict", "--model", "m", "-f", "f.tsv", "-g", "g.tsv"]).known is None
