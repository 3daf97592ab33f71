"""The host checks that the three lattice queries -- ``gecco_crf_span_probabilities``, ``gecco_crf_sample_paths`` and
``gecco_crf_viterbi_kbest`` -- share (no device): the batch's own refusals read the same from all three, and a span query and
a run query with a bad label set are told so in the same words behind their ``span q:`` / ``run q:``."""
import numpy as np
import pytest

L3 = 3
I32, U32 = np.int32, np.uint32

# per entry: the arguments behind (model, device), and those of a valid call that differ from the shared batch below
ENTRIES = {
    "gecco_crf_span_probabilities": (
        ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "span_contig", "span_begin", "span_end",
         "span_mask", "n_spans", "logp", "marg", "lognorm"),
        {"span_contig": np.array([0, 1], dtype=I32), "span_begin": np.array([0, 1], dtype=I32), "span_end": np.array([2, 3], dtype=I32),
         "span_mask": np.array([5, 2], dtype=U32), "n_spans": 2, "logp": np.zeros(2)}),
    "gecco_crf_sample_paths": (
        ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "n_samples", "seed", "run_contig", "run_anchor",
         "run_mask", "n_runs", "y", "runs", "marg", "lognorm"),
        {"n_samples": 3, "seed": 11, "run_contig": np.array([0, 1], dtype=I32), "run_anchor": np.array([1, 2], dtype=I32),
         "run_mask": np.array([5, 2], dtype=U32), "n_runs": 2, "y": np.zeros(5 * 3, dtype=np.int8), "runs": np.zeros(2 * 3 * 2, dtype=I32)}),
    "gecco_crf_viterbi_kbest": (
        ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "k", "y", "score", "n_paths", "lognorm"),
        {"k": 4, "y": np.zeros(5 * 4, dtype=np.int8), "score": np.zeros(2 * 4), "n_paths": np.zeros(2, dtype=I32)}),
}


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    return _native


@pytest.fixture(scope="module")
def model3(nat):
    rng = np.random.default_rng(5)
    return nat.Model.from_tables(rng.normal(size=(7, L3)), rng.normal(size=(L3, L3)))


def _call(nat, model, entry, **change):
    """A valid call of `entry` on two contigs (2 and 3 genes), on a device that does not exist, with `change` applied."""
    names, own = ENTRIES[entry]
    a = {"contig_ptr": np.array([0, 2, 5], dtype=I32), "n_contigs": 2, "gene_ptr": np.arange(0, 12, 2, dtype=I32),
         "attr_id": (np.arange(10, dtype=I32) * 3) % 7, "attr_value": None, "allowed": None, "marg": np.zeros(5 * L3),
         "lognorm": np.zeros(2)}
    a.update(own)
    a.update(change)
    fn = getattr(nat.load_library(), entry)
    args = [a[n].ctypes.data_as(t) if isinstance(a[n], np.ndarray) else a[n] for n, t in zip(names, fn.argtypes[2:])]
    rc = fn(model._h, 99, *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_batch_is_refused_in_the_same_words_by_every_entry(nat, model3, entry):
    call = lambda **kw: _call(nat, model3, entry, **kw)
    # a valid call gets past the host checks: what stops it is the device that does not exist
    assert call()[0] not in (nat.OK, nat.EINVAL)
    assert call(contig_ptr=None) == (nat.EINVAL, "bad contig_ptr")
    assert call(attr_value=np.ones(10), allowed=np.array([7, 1, 6, 4, 9], dtype=U32)) == \
        (nat.EINVAL, "constrained: gene 4 allows a label at or above num_labels = 3 (mask 9)")


@pytest.mark.parametrize("mask,words", [
    (0, "the label set is empty (a mask of 0)"),
    (1 << L3, "the set holds a label at or above num_labels = 3 (mask 8)"),
    (9, "the set holds a label at or above num_labels = 3 (mask 9)"),
])
def test_a_span_and_a_run_with_a_bad_label_set_differ_in_their_prefix_only(nat, model3, mask, words):
    masks = np.array([5, mask], dtype=U32)
    assert _call(nat, model3, "gecco_crf_span_probabilities", span_mask=masks) == (nat.EINVAL, "span 1: " + words)
    assert _call(nat, model3, "gecco_crf_sample_paths", run_mask=masks) == (nat.EINVAL, "run 1: " + words)


def test_a_query_on_a_contig_out_of_range_differs_in_its_prefix_only(nat, model3):
    contigs = np.array([2, 0], dtype=I32)
    words = "contig 2 out of range (the batch has 2)"
    assert _call(nat, model3, "gecco_crf_span_probabilities", span_contig=contigs) == (nat.EINVAL, "span 0: " + words)
    assert _call(nat, model3, "gecco_crf_sample_paths", run_contig=contigs) == (nat.EINVAL, "run 0: " + words)
