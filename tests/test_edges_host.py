"""Edge posteriors, host side (no device): the numpy yardstick (tests/edges_reference.py) against path enumeration, the host
formula of ``SequenceCRF.expected_runs`` on the yardstick, the refusals of the new ``SequenceCRF`` methods before any device
call, and the header's declaration of ``gecco_crf_edge_posteriors``."""
import os
import re

import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import edges_reference as er
from tests import train_objective_partial as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 6


def _case(rng, L, n, sigma, masked):
    w, trans = rng.normal(0.0, sigma, size=(A, L)), rng.normal(0.0, sigma, size=(L, L))
    deg = rng.integers(0, 4, size=n)
    gptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    attr = rng.integers(0, A, size=int(gptr[-1])).astype(np.int32)
    allowed = tp.full_masks(n, L)
    if masked:
        t = int(rng.integers(0, n))
        allowed[t] &= ~np.uint32(1 << int(rng.integers(0, L)))  # (one disallowed pair; L >= 2 leaves a label)
    return cr.masked_scores(gptr, attr, None, w, allowed), trans


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("L", [2, 3])
def test_the_reference_against_path_enumeration(L, masked):
    rng = np.random.default_rng(4100 + L + 10 * masked)
    sets = list(range(1, 1 << L))
    worst_xi = worst_h = worst_runs = 0.0
    for n in range(1, 8):
        for sigma in (1.0, 4.0, 12.0):
            score, trans = _case(rng, L, n, sigma, masked)
            ref = er.edge_posteriors(np.array([0, n]), score, trans, sets)
            with np.errstate(invalid="ignore", divide="ignore"):
                xi, H, runs = er.enumerate_edges(score, trans, sets)
            logz, marg = cr.enumerate_paths(score, trans)[:2]
            worst_xi = max(worst_xi, float(np.abs(ref["pair"] - xi).max()))
            worst_h = max(worst_h, abs(ref["entropy"][0] - H) / n)
            assert np.abs(ref["pair"] - xi).max() <= 1e-13 and np.abs(ref["marg"] - marg).max() <= 1e-13
            assert abs(ref["entropy"][0] - H) <= 1e-13 * n and ref["entropy"][0] >= 0.0
            assert np.all(ref["pair"][0] == 0.0)
            assert np.abs(ref["transitions"][0] - xi.sum(axis=0)).max() <= 1e-13 * n
            # enter / leave: the expected number of runs, either way, and the host formula of expected_runs
            for k, m in enumerate(sets):
                formula = er.expected_runs(ref["marg"][0], ref["transitions"][0], m)
                worst_runs = max(worst_runs, abs(formula - runs[k]))
                assert abs(formula - runs[k]) <= 1e-13 * n
                assert abs(ref["enter"][:, k].sum() - runs[k]) <= 1e-13 * n and abs(ref["leave"][:, k].sum() - runs[k]) <= 1e-13 * n
            full = sets.index((1 << L) - 1)
            assert abs(ref["enter"][0, full] - 1.0) <= 1e-14 and np.all(ref["enter"][1:, full] == 0.0)
            if masked:
                dead = np.isneginf(score)
                assert dead.any() and np.all(ref["pair"].transpose(0, 2, 1)[dead] == 0.0)
    print(f"L={L} masked={masked}: worst |xi - enumeration| = {worst_xi:.3g}, worst |H - enumeration| / T = {worst_h:.3g}, "
          f"worst |expected_runs formula - enumeration| = {worst_runs:.3g}")


def test_the_reference_on_a_batch_with_empty_and_single_item_sequences():
    rng = np.random.default_rng(4200)
    L = 3
    score, trans = _case(rng, L, 6, 1.0, False)
    ref = er.edge_posteriors(np.array([0, 0, 1, 6, 6]), score, trans, [1, 6])
    assert ref["entropy"][0] == 0.0 and ref["entropy"][3] == 0.0 and np.all(ref["transitions"][[0, 1, 3]] == 0.0)
    m = ref["marg"][0]
    assert np.allclose(ref["enter"][0], [m[0], m[1] + m[2]], atol=1e-15) and np.array_equal(ref["enter"][0], ref["leave"][0])
    assert abs(ref["entropy"][1] + (m * np.log(m)).sum()) <= 1e-15
    assert abs(ref["transitions"][2].sum() - 4.0) <= 1e-13


# ---------------------------------------------------------------- SequenceCRF: refusals before any device call
@pytest.fixture()
def crf(monkeypatch):
    from gecco_amd import _native
    from gecco_amd.crfsuite_model import model_bytes
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(5)
    An, L = 4, 3
    names, classes = [f"a{k}" for k in range(An)], ["x", "y", "z"]
    w = rng.normal(0.0, 1.0, size=An * L + L * L)
    blob = model_bytes(classes, names, np.repeat(np.arange(An), L), np.tile(np.arange(L), An), np.repeat(np.arange(L), L),
                       np.tile(np.arange(L), L), w)
    crf = SequenceCRF.from_bytes(blob, window_size=None)

    def no_device(*args, **kwargs):
        raise AssertionError("the native call was reached")

    # (every compute entry of the model: a refusal has to come before any of them)
    for name in ("edge_posteriors", "span_log_probabilities", "marginals_full", "viterbi", "windowed_marginals",
                 "windowed_marginals_all"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [], [["a0", "a3"]]]


@pytest.mark.parametrize("method", ["boundary_probability", "expected_runs"])
@pytest.mark.parametrize("bad,words", [
    ("w", "unknown label 'w'"),
    ({"x", "nope"}, "unknown label 'nope'"),
    (set(), "empty set"),
    ([], "empty set"),
])
def test_bad_sets_are_refused_before_any_device_call(crf, method, bad, words):
    with pytest.raises(ValueError) as err:
        getattr(crf, method)(X, [{"x", "y"}, bad])
    assert "set 1" in str(err.value) and words in str(err.value), str(err.value)


@pytest.mark.parametrize("method,args", [("predict_pair_marginals", ()), ("boundary_probability", (["x"],)),
                                         ("expected_transitions", ()), ("expected_runs", (["x"],)), ("path_entropy", ())])
def test_bad_allowed_sets_are_refused_before_any_device_call(crf, method, args):
    with pytest.raises(ValueError, match="unknown label"):
        getattr(crf, method)(X, *args, allowed=[["x", "q", None], [], [None]])
    with pytest.raises(ValueError, match="items but"):
        getattr(crf, method)(X, *args, allowed=[["x", None], [], [None]])
    with pytest.raises(ValueError, match="sequences and allowed"):
        getattr(crf, method)(X, *args, allowed=[[None, None, None]])


def test_sets_that_are_no_list_are_refused(crf):
    with pytest.raises(ValueError, match="list of label sets"):
        crf.boundary_probability(X, 5)


def test_sequences_without_items_never_reach_the_device(crf):
    empty = [[], []]
    assert [p.shape for p in crf.predict_pair_marginals(empty)] == [(0, 3, 3), (0, 3, 3)]
    pairs = crf.boundary_probability(empty, ["x", {"y", "z"}])
    assert [(e.shape, l.shape) for e, l in pairs] == [((0, 2), (0, 2))] * 2
    assert crf.expected_transitions(empty).shape == (2, 3, 3) and not crf.expected_transitions(empty).any()
    assert crf.expected_runs(empty, ["x", "y"]).tolist() == [[0.0, 0.0], [0.0, 0.0]]
    assert crf.path_entropy(empty).tolist() == [0.0, 0.0]
    assert crf.path_entropy([]).shape == (0,) and crf.predict_pair_marginals([]) == []


def test_an_unfitted_model_is_refused():
    from gecco_amd.sequence import SequenceCRF

    for method, args in (("predict_pair_marginals", ()), ("boundary_probability", (["x"],)), ("expected_transitions", ()),
                         ("expected_runs", (["x"],)), ("path_entropy", ())):
        with pytest.raises(ValueError, match="not fitted"):
            getattr(SequenceCRF(window_size=None), method)(X, *args)


def test_the_header_declares_the_entry_and_the_library_exports_it():
    from gecco_amd import _native as nat
    from gecco_amd import build

    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    assert "ABI 2.19.0" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+gecco_crf_edge_posteriors\s*\(([^;]*)\)\s*;", code)
    assert m, "gecco_crf_edge_posteriors is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "m", "device", "contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "set_mask", "n_sets", "pair",
        "enter", "leave", "transitions", "entropy", "marg", "lognorm"]
    lib = nat.load_library()
    assert hasattr(lib, "gecco_crf_edge_posteriors")
    assert len(nat.SIGNATURES["gecco_crf_edge_posteriors"][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    assert callable(nat.Model.edge_posteriors)
    assert "crf_edges.hip" in build.SOURCES and "crf_edges.hip" not in build.EXTRA_FLAGS  # (contraction stays on: DESIGN.md §4.9j)


def test_the_typed_front_end_takes_the_flag():
    import inspect

    from gecco_amd import typed

    for name in ("predict_clusters", "predict_genes_and_clusters"):
        assert inspect.signature(getattr(typed.TypedClusterCRF, name)).parameters["boundary_posteriors"].default is False
    args = typed.build_parser().parse_args(["predict", "--model", "m", "-f", "f", "-g", "g"])
    assert args.boundary_posteriors is False
    assert typed.build_parser().parse_args(["predict", "--model", "m", "-f", "f", "-g", "g", "--boundary-posteriors"]).boundary_posteriors


def test_the_cluster_table_gets_the_columns_only_when_clusters_carry_them():
    from gecco_amd import typed

    assert typed.TypedClusterCRF.SEQUENCE_COLUMNS == ("sequence_id", "genes", "log_z", "entropy", "expected_clusters")
    assert "start_p" not in typed.typed_cluster_table([], ["A"]).columns
