"""Every family of entry that takes a `device`, on a box without one: valid arguments are refused with ENODEV and the one
text of `check_device` (crf_hip_own.hpp), and an argument error still surfaces as itself, since every entry checks its
arguments first.  Three entries check the device before the rest of their arguments (`gecco_crf_plan_create`,
`gecco_crf_segment_ex` past its null checks, `gecco_crf_domain_composition`): their order is pinned as it is."""
import numpy as np
import pytest

from gecco_amd import _native as nat

pytestmark = pytest.mark.skipif(nat.device_count() > 0, reason="only meaningful on a box without a GPU")

NO_DEVICE = "no HIP device available (this library has no CPU fallback)"

# one contig of two genes, one attribute each; a 2-label model over the two attributes
C, G, A = [0, 2], [0, 1, 2], [0, 1]
# one training sequence of `window` = 2 items: (seq_ptr, item_ptr, attr_id, labels, num_attrs, state_fid, trans_fid, num_features)
T8 = ([0, 2], [0, 1, 2], [0, 1], [0, 1], 2, [0, 1, 2, 3], [4, 5, 6, 7], 8)
NO_ITEMS = ([0, 0], [0], [], [], 2, [0, 1, 2, 3], [4, 5, 6, 7], 8)
FOREST = dict(col_ptr=np.array([0, 1]), row_idx=np.array([0]), values=np.array([1.0], np.float32), n_samples=2,
              y=np.array([[0], [1]]), n_classes=np.array([2]), sample_counts=np.array([[1, 1]]), rand_state=np.array([5]))
BAD_ROW = dict(FOREST, row_idx=np.array([7]))


@pytest.fixture(scope="module")
def m():
    return nat.Model.from_tables(np.array([[0.5, -0.5], [-0.25, 0.25]]), np.array([[0.1, -0.1], [-0.2, 0.2]]))


# name -> (the call with valid arguments, the same call with a bad argument, the bad argument's own message)
CASES = {
    "windowed_marginals": (lambda m: m.windowed_marginals(C, G, A, 2), lambda m: m.windowed_marginals(C, G, A, 0),
                           "Window size must be strictly positive"),
    "windowed_marginals_all": (lambda m: m.windowed_marginals_all(C, G, A, 2), lambda m: m.windowed_marginals_all(C, G, A, 2, step=3),
                               "Window step must be strictly positive"),
    "marginals_full_valued": (lambda m: m.marginals_full(C, G, A, values=[1.0, 2.0]),
                              lambda m: m.marginals_full(C, G, A, values=[1.0, np.inf]), "attribute value 1 is not finite"),
    "viterbi_constrained": (lambda m: m.viterbi(C, G, A, allowed=[1, 3]), lambda m: m.viterbi(C, G, A, allowed=[0, 3]),
                            "gene 0 allows no label"),
    "span_log_probabilities": (lambda m: m.span_log_probabilities(C, G, A, [0], [0], [2], [1]),
                               lambda m: m.span_log_probabilities(C, G, A, [0], [0], [2], [0]), "span 0: the label set is empty"),
    "sample_paths": (lambda m: m.sample_paths(C, G, A, 2), lambda m: m.sample_paths(C, G, A, 0), "n_samples = 0 is outside"),
    "viterbi_kbest": (lambda m: m.viterbi_kbest(C, G, A, 2), lambda m: m.viterbi_kbest(C, G, A, 0), "k = 0 is outside"),
    "Session": (lambda m: nat.Session(m, [0]), lambda m: nat.Session(m, []), "session: no devices given"),
    "Trainer": (lambda m: nat.Trainer(*T8[:5], 2, 1, *T8[5:]), lambda m: nat.Trainer(*T8[:5], 2, 3, *T8[5:]),
                "Window step must be strictly positive"),
    "TrainerBatch": (lambda m: nat.TrainerBatch([T8], 2, 1), lambda m: nat.TrainerBatch([T8], 2, 3),
                     "trainer batch: problem 0: Window step"),
    "TrainerGrid": (lambda m: nat.TrainerGrid([T8 + (2, 1)], [0]), lambda m: nat.TrainerGrid([T8 + (2, 1)], [1]),
                    "trainer grid: problem 0: set 1 out of range"),
    "TrainerGeneral": (lambda m: nat.TrainerGeneral([T8 + (2, 1)]), lambda m: nat.TrainerGeneral([T8 + (2, 3)]),
                       "trainer general: problem 0: Window step"),
    "TrainerGeneral_partial": (lambda m: nat.TrainerGeneral([T8 + (2, 1)], allowed=[[1, 3]]),
                               lambda m: nat.TrainerGeneral([T8 + (2, 1)], allowed=[[0, 3]]), "item 0 allows no label"),
    "TrainerSequences": (lambda m: nat.TrainerSequences([T8]), lambda m: nat.TrainerSequences([NO_ITEMS]),
                         "trainer sequences: problem 0: trainer: sequence 0 has no items"),
    "fisher_exact": (lambda m: nat.fisher_exact([[1, 2], [3, 4]]), lambda m: nat.fisher_exact([[1, -2], [3, 4]]),
                     "table 0 has a negative cell"),
    "cluster_overlaps": (lambda m: nat.cluster_overlaps([0], [1], [5], [0, 1], [2], [4]),
                         lambda m: nat.cluster_overlaps([0], [1], [5], [0, 2], [5, 2], [6, 4]), "not sorted by start"),
    "domain_composition_members": (lambda m: nat.domain_composition_members([0, 1], [0], [0, 1], [0], [0.5], 1),
                                   lambda m: nat.domain_composition_members([0, 1], [3], [0, 1], [0], [0.5], 1),
                                   "member 0 outside the gene range"),
    "Forest": (lambda m: nat.Forest(**FOREST, max_features=1), lambda m: nat.Forest(**BAD_ROW, max_features=1),
               "forest_fit: row index out of range"),
    "fit_forests": (lambda m: nat.fit_forests([FOREST], 1), lambda m: nat.fit_forests([BAD_ROW], 1),
                    "forest_fit_batch: problem 0: row index out of range"),
    # the device is checked before these entries' remaining arguments: the bad argument does not get its say
    "Plan": (lambda m: nat.Plan(m, C, 2, device=0), lambda m: nat.Plan(m, [1, 2], 2, device=0), None),
    "segment": (lambda m: nat.segment([0.9], [1], [0, 1]), lambda m: nat.segment([0.9], [1], [1, 1]), None),
    "domain_composition": (lambda m: nat.domain_composition([(0, 1, 0, 1)], [0, 1], [0], [0.5], 1),
                           lambda m: nat.domain_composition([(0, 1, 0, 1)], [0, 1], [3], [0.5], 1), None),
}


def refused_without_device(call, m):
    with pytest.raises(nat.NativeError) as ei:
        call(m)
    assert ei.value.code == nat.ENODEV
    assert str(ei.value).startswith(NO_DEVICE + " (gecco_crf status")


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_without_a_device(m, name):
    good, bad, message = CASES[name]
    refused_without_device(good, m)
    if message is None:
        refused_without_device(bad, m)
        return
    with pytest.raises(ValueError) as ei:
        bad(m)
    assert message in str(ei.value)
