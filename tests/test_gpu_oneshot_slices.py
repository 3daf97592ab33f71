"""A batch handed to the whole-batch one-shots as a slice of a larger CSR: ``contig_ptr[0] > 0``, the first gene's
``gene_ptr`` > 0, and ``attr_id`` / ``attr_value`` with a prefix that belongs to other contigs.  The unvalued
``gecco_crf_windowed_marginals_all`` and the four ``*_valued`` entries must return, byte for byte, what they return for the
same contigs rebased to start at zero: the entries rebase the row pointers on the host and upload the arrays from the
slice's first entry, and nothing else may depend on where the slice lies.

Both sides of every comparison are calls of the code under test (the numpy yardstick is tests/test_gpu_sequence_valued.py's
and tests/test_gpu_windowed_all.py's business).  The calls go through ``ctypes``: the Python wrappers size their outputs from
``contig_ptr[-1]`` and cannot express a slice.

Models of 2, 5 and 12 labels: the two-label model (forced onto the any-L kernels by values), the lane-per-window tier and
the matrix-core tier.  Contigs of 3, 30, 1 and 70 genes behind two others, W = 5, step = 2, so that without padding the
contigs of 3 and 1 genes are skipped, and 70 genes are several chunks of the whole-contig kernels."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = 30
LABELS = [2, 5, 12]
PREFIX, LENGTHS = [4, 9], [3, 30, 1, 70]
WINDOW, STEP, BACKGROUND, LABEL = 5, 2, 0, 1
FILL = -7.0  # what the output buffers hold before a call: no entry writes it

ENTRIES = {  # name -> (symbol, valued, windowed, outputs as (name, dtype, "gene" | "gene_label" | "contig"))
    "all": ("gecco_crf_windowed_marginals_all", False, True, (("p_all", np.float64, "gene_label"), ("p_any", np.float64, "gene"))),
    "windowed_valued": ("gecco_crf_windowed_marginals_valued", True, True, (("p", np.float64, "gene"),)),
    "all_valued": ("gecco_crf_windowed_marginals_all_valued", True, True,
                   (("p_all", np.float64, "gene_label"), ("p_any", np.float64, "gene"))),
    "full_valued": ("gecco_crf_marginals_full_valued", True, False, (("marg", np.float64, "gene_label"), ("lognorm", np.float64, "contig"))),
    "viterbi_valued": ("gecco_crf_viterbi_valued", True, False, (("y", np.int8, "gene"), ("score", np.float64, "contig"))),
}


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no HIP device")
    return _native


@pytest.fixture(scope="module")
def models(nat):
    out = {}
    for L in LABELS:
        rng = np.random.default_rng(3100 + L)
        out[L] = nat.Model.from_tables(rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L)))
    return out


def _whole_csr(seed, slice_has_attrs=True):
    """The larger CSR: PREFIX's contigs, then LENGTHS'.  Every gene of the prefix has attributes, so the slice's first row
    pointer is > 0 whatever its own genes hold."""
    rng = np.random.default_rng(seed)
    cptr = np.concatenate([[0], np.cumsum(PREFIX + LENGTHS)]).astype(np.int32)
    n0, n = int(cptr[len(PREFIX)]), int(cptr[-1])
    deg = np.concatenate([rng.integers(1, 5, size=n0), rng.integers(0, 5, size=n - n0) if slice_has_attrs else np.zeros(n - n0, int)])
    gptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    attr = rng.integers(0, A, size=int(gptr[-1])).astype(np.int32)
    v = rng.normal(0.0, 1.0, size=attr.size)
    v[rng.integers(0, 4, size=attr.size) == 0] = 1.0
    return cptr, gptr, attr, v


def _slice_and_rebased(cptr, gptr, attr, v, first=len(PREFIX)):
    """The same contigs twice: as they lie in the larger arrays, and as arrays of their own that start at zero."""
    g0 = int(cptr[first])
    a0 = int(gptr[g0])
    assert g0 > 0 and a0 > 0
    as_slice = (cptr[first:].copy(), gptr, attr, v)
    rebased = (cptr[first:] - g0, gptr[g0:] - a0, attr[a0:].copy(), v[a0:].copy())
    return as_slice, rebased


def _run(nat, model, entry, csr, pad=1):
    """One call of `entry` on the contigs of csr[0]; returns the status and the output buffers by name."""
    symbol, valued, windowed, outputs = ENTRIES[entry]
    cptr, gptr, attr, v = (np.ascontiguousarray(x) for x in csr)
    nc, n, L = len(cptr) - 1, int(cptr[-1] - cptr[0]), model.num_labels
    attr = attr if attr.size else np.zeros(1, dtype=np.int32)  # (a valid pointer for an array without entries)
    v = v if v.size else np.zeros(1)
    size = {"gene": n, "gene_label": n * L, "contig": nc}
    bufs = {name: np.full(max(size[kind], 1), FILL).astype(dtype) for name, dtype, kind in outputs}
    fn = getattr(nat.load_library(), symbol)
    args = [cptr, nc, gptr, attr] + ([v] if valued else [])
    if windowed:
        args += [WINDOW, STEP, LABEL if entry == "windowed_valued" else BACKGROUND, pad]
    args += [bufs[name] for name, _, _ in outputs]
    c_args = [x.ctypes.data_as(t) if isinstance(x, np.ndarray) else x for x, t in zip(args, fn.argtypes[2:])]
    rc = fn(model._h, 0, *c_args)
    return rc, {name: bufs[name][:size[kind]] for name, _, kind in outputs}


def _assert_same_bytes(nat, model, entry, as_slice, rebased, pad):
    rc_s, got_s = _run(nat, model, entry, as_slice, pad)
    rc_r, got_r = _run(nat, model, entry, rebased, pad)
    assert (rc_s, rc_r) == (nat.OK, nat.OK), nat.load_library().gecco_crf_last_error().decode()
    for name in got_s:
        assert got_s[name].size and not np.any(got_s[name] == np.asarray(FILL).astype(got_s[name].dtype)), f"{name}: not written"
        assert got_s[name].tobytes() == got_r[name].tobytes(), f"{entry}, pad={pad}: {name} depends on where the slice lies"
    return got_s


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("L", LABELS)
def test_a_slice_gives_the_bytes_of_the_rebased_batch(nat, models, L, entry):
    as_slice, rebased = _slice_and_rebased(*_whole_csr(41))
    for pad in (1, 0) if ENTRIES[entry][2] else (1,):
        got = _assert_same_bytes(nat, models[L], entry, as_slice, rebased, pad)
        if ENTRIES[entry][2]:
            # without padding the contigs shorter than the window (3 genes and 1 gene) have no prediction, all others one
            skipped = np.zeros(sum(LENGTHS), dtype=bool)
            if not pad:
                skipped[:3] = skipped[33:34] = True
            p = got["p_any" if "p_any" in got else "p"]
            assert np.array_equal(np.isnan(p), skipped)


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("L", LABELS)
def test_a_slice_whose_genes_have_no_attributes(nat, models, L, entry):
    cptr, gptr, attr, v = _whole_csr(43, slice_has_attrs=False)
    as_slice, rebased = _slice_and_rebased(cptr, gptr, attr, v)
    assert rebased[2].size == 0 and not rebased[1].any()  # nnz = 0 behind a prefix that has entries
    _assert_same_bytes(nat, models[L], entry, as_slice, rebased, 1)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_three_empty_contigs(nat, models, entry):
    cptr, gptr, attr, v = _whole_csr(41)
    empty = (np.full(4, cptr[len(PREFIX)], dtype=np.int32), gptr, attr, v)
    rc, got = _run(nat, models[5], entry, empty)
    assert rc == nat.OK
    for name in ("lognorm", "score"):
        if name in got:
            assert got[name].tolist() == [0.0, 0.0, 0.0]
