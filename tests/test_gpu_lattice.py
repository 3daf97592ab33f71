"""What the three lattice queries share on the device, in one place: for a plain 2-label model -- no values, no masks -- the
marginals entry has kernels of its own, which the queries ask in a second pass over the rebased slice; marg and lognorm of
all three are that entry's bytes."""
import numpy as np
import pytest

from tests import test_gpu_kbest as gk

pytestmark = pytest.mark.gpu


def test_a_plain_two_label_slice_gives_the_marginals_entrys_bytes_from_every_entry():
    """Four contigs of 0, 1, 5 and 70 genes behind a leading one that the slice leaves out, so that rows and attribute entries
    are both rebased."""
    from gecco_amd import _native as nat

    if nat.device_count() < 1:
        pytest.skip("no HIP device")
    b = gk.make_batch(9200, 2, [6, 0, 1, 5, 70])
    model = nat.Model.from_tables(b["w"], b["trans"])
    cptr, gptr, attr = b["csr"]
    g0 = int(cptr[1])
    a0 = int(gptr[g0])
    assert g0 > 0 and a0 > 0
    marg, lognorm = model.marginals_full(cptr[1:] - g0, gptr[g0:] - a0, attr[a0:])
    assert marg.shape == (76, 2) and lognorm.shape == (4,) and lognorm[0] == 0.0 and np.all(lognorm[1:] != 0.0)

    spans = (np.array([3, 1], dtype=np.int32), np.array([3, 0], dtype=np.int32), np.array([40, 1], dtype=np.int32),
             np.array([1, 2], dtype=np.uint32))
    logp, m_spans, ln_spans = model.span_log_probabilities(cptr[1:], gptr, attr, *spans, want_marginals=True)
    y, m_paths, ln_paths = model.sample_paths(cptr[1:], gptr, attr, 4, seed=3, want_marginals=True)
    yk, score, n_paths, ln_kbest = model.viterbi_kbest(cptr[1:], gptr, attr, 3)
    assert logp.shape == (2,) and np.all(logp <= 0.0) and y.shape == (76, 4) and yk.shape == (76, 3) and n_paths.tolist() == [0, 2, 3, 3]
    for tag, got in (("span_probabilities", m_spans), ("sample_paths", m_paths)):
        assert got.shape == marg.shape and got.tobytes() == marg.tobytes(), tag
    for tag, got in (("span_probabilities", ln_spans), ("sample_paths", ln_paths), ("viterbi_kbest", ln_kbest)):
        assert got.shape == lognorm.shape and got.tobytes() == lognorm.tobytes(), tag
