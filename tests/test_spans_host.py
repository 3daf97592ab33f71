"""Region posteriors, host side (no device): ``SequenceCRF.span_log_probability`` refuses bad spans before any device call,
and the header declares ``gecco_crf_span_probabilities`` and the library exports it."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    for name in ("span_log_probabilities", "marginals_full", "viterbi", "windowed_marginals", "windowed_marginals_all"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [], [["a0", "a3"]]]


@pytest.mark.parametrize("span,words", [
    ((0, 0, 2, "w"), "unknown label 'w'"),
    ((0, 0, 2, {"x", "nope"}), "unknown label 'nope'"),
    ((0, 0, 2, set()), "empty set"),
    ((0, 0, 2, []), "empty set"),
    ((3, 0, 1, "x"), "sequence index 3 out of range"),
    ((-1, 0, 1, "x"), "sequence index -1 out of range"),
    ((0, 2, 2, "x"), "start >= stop"),
    ((0, 2, 1, "x"), "start >= stop"),
    ((0, -1, 2, "x"), "start < 0"),
    ((0, 0, 4, "x"), "stop 4 lies beyond sequence 0 of 3 items"),
    ((1, 0, 1, "x"), "stop 1 lies beyond sequence 1 of 0 items"),
    ((0, 0.5, 2, "x"), "expected (sequence_index, start, stop, labels)"),
    ((0, 0, 2), "expected (sequence_index, start, stop, labels)"),
])
def test_bad_spans_are_refused_before_any_device_call(crf, span, words):
    good = (0, 0, 3, {"x", "y"})
    for method in (crf.span_log_probability, crf.span_probability):
        with pytest.raises(ValueError) as err:
            method(X, [good, span])
        assert "span 1" in str(err.value) and words in str(err.value), str(err.value)


def test_bad_allowed_sets_are_refused_before_any_device_call(crf):
    with pytest.raises(ValueError, match="unknown label"):
        crf.span_log_probability(X, [(0, 0, 1, "x")], allowed=[["x", "q", None], [], [None]])
    with pytest.raises(ValueError, match="items but"):
        crf.span_log_probability(X, [(0, 0, 1, "x")], allowed=[["x", None], [], [None]])


def test_no_spans_need_no_device(crf):
    out = crf.span_log_probability(X, [])
    assert out.shape == (0,) and out.dtype == np.float64
    assert crf.span_probability(X, iter(())).shape == (0,)


def test_an_unfitted_model_is_refused():
    from gecco_amd.sequence import SequenceCRF

    with pytest.raises(ValueError, match="not fitted"):
        SequenceCRF(window_size=None).span_log_probability(X, [(0, 0, 1, "x")])


def test_the_header_declares_the_entry_and_the_library_exports_it():
    from gecco_amd import _native as nat

    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    assert "ABI 2.16.0" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+gecco_crf_span_probabilities\s*\(([^;]*)\)\s*;", code)
    assert m, "gecco_crf_span_probabilities is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "m", "device", "contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "span_contig", "span_begin",
        "span_end", "span_mask", "n_spans", "logp", "marg", "lognorm"]
    lib = nat.load_library()
    assert hasattr(lib, "gecco_crf_span_probabilities")
    assert len(nat.SIGNATURES["gecco_crf_span_probabilities"][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    assert callable(nat.Model.span_log_probabilities)


def test_the_typed_front_end_takes_the_flag():
    import inspect

    from gecco_amd import typed

    for name in ("predict_clusters", "predict_genes_and_clusters"):
        assert inspect.signature(getattr(typed.TypedClusterCRF, name)).parameters["region_posteriors"].default is False
    args = typed.build_parser().parse_args(["predict", "--model", "m", "-f", "f", "-g", "g"])
    assert args.region_posteriors is False
    assert typed.build_parser().parse_args(["predict", "--model", "m", "-f", "f", "-g", "g", "--region-posteriors"]).region_posteriors
