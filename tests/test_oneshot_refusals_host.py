"""The refusals of the five whole-batch one-shots, each on its own: (entry, bad argument) -> (status, gecco_crf_last_error()).

The entries are the unvalued ``gecco_crf_windowed_marginals_all`` and the four ``*_valued`` ones: each builds one plan over the
whole batch and keeps the batch on the device for the one call.  Every refusal here is an argument error, found before any
device work, so the table needs no GPU: the calls go through ``ctypes`` with a valid batch in which one argument is wrong.

Precedence (``test_argument_error_comes_before_a_bad_device``): an argument error together with ``device = 99`` reports the
argument error, "so that they surface even on a box without a GPU".  While the unvalued all-label entry had a path of its
own, it looked at the device and built its plan before it looked at ``contig_ptr``, the buffers and ``gene_ptr``: those rows
gave ENODEV for it (and so did, on a box without a GPU, its rows of the first table that are checked behind the device).
That order is the one thing that changed when the five entries were given one path; nothing else about which call is
refused, or with what status and message, did: on a box with a GPU every other row passed before it as well."""
import ctypes

import numpy as np
import pytest

from gecco_amd import _native as nat

L = 3
I32P, F64P, I8P = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_double, ctypes.c_int8))

ENTRIES = {  # name -> (symbol, valued, the arguments behind the CSR arrays)
    "all": ("gecco_crf_windowed_marginals_all", False, ("window", "step", "background", "pad", "p_all", "p_any")),
    "windowed_valued": ("gecco_crf_windowed_marginals_valued", True, ("window", "step", "label", "pad", "p_out")),
    "all_valued": ("gecco_crf_windowed_marginals_all_valued", True, ("window", "step", "background", "pad", "p_all", "p_any")),
    "full_valued": ("gecco_crf_marginals_full_valued", True, ("marg", "lognorm")),
    "viterbi_valued": ("gecco_crf_viterbi_valued", True, ("y_out", "score")),
}
VALUED = [e for e, (_, valued, _) in ENTRIES.items() if valued]
WINDOWED = ["all", "windowed_valued", "all_valued"]
EVERY = list(ENTRIES)

WINDOW = "Window size must be strictly positive"
STEP = "Window step must be strictly positive and under `window_size`"
NO_VALUES = "null attr_value with attribute entries (the unvalued entry takes attributes without values)"


@pytest.fixture(scope="module")
def model():
    rng = np.random.default_rng(5)
    return nat.Model.from_tables(rng.normal(size=(7, L)), rng.normal(size=(L, L)))


def good_batch():
    """Two contigs of 2 and 3 genes, two attributes per gene; gene_ptr starts at 2, so entry k of the batch is entry 2 + k of
    attr_id / attr_value."""
    a = {
        "device": 0,
        "contig_ptr": np.array([0, 2, 5], dtype=np.int32),
        "n_contigs": 2,
        "gene_ptr": np.arange(2, 14, 2, dtype=np.int32),
        "attr_id": (np.arange(12, dtype=np.int32) * 3) % 7,
        "attr_value": np.linspace(0.5, 1.5, 12),
        "window": 5, "step": 2, "label": 1, "background": 0, "pad": 1,
        "p_out": np.zeros(5), "p_all": np.zeros(5 * L), "p_any": np.zeros(5),
        "marg": np.zeros(5 * L), "lognorm": np.zeros(2), "y_out": np.zeros(5, dtype=np.int8), "score": np.zeros(2),
    }
    assert a["gene_ptr"][0] == 2
    return a


def call(model, entry, **bad):
    symbol, valued, tail = ENTRIES[entry]
    a = good_batch()
    a.update(bad)
    names = ("contig_ptr", "n_contigs", "gene_ptr", "attr_id") + (("attr_value",) if valued else ()) + tail
    fn = getattr(nat.load_library(), symbol)
    args = []
    for name, ctype in zip(names, fn.argtypes[2:]):
        v = a[name]
        args.append(v if v is None or not isinstance(v, np.ndarray) else v.ctypes.data_as(ctype))
    rc = fn(model._h, a["device"], *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


def nan_at_entry_3():
    v = good_batch()["attr_value"]
    v[3] = np.nan
    return v


# (entries, the bad arguments, the message) -- every refusal is GECCO_CRF_EINVAL
REFUSALS = [
    (WINDOWED, {"window": 0}, WINDOW),
    (WINDOWED, {"step": 0}, STEP),
    (WINDOWED, {"step": 6}, STEP),
    (["windowed_valued"], {"label": -1}, "label out of range"),
    (["windowed_valued"], {"label": L}, "label out of range"),
    (["all", "all_valued"], {"background": -2}, "background label out of range"),
    (["all", "all_valued"], {"background": L}, "background label out of range"),
    (["all", "all_valued"], {"background": -1}, "p_any needs a background label"),
    (["all", "all_valued"], {"p_any": None}, "null p_any buffer with a background label"),
    (["all", "all_valued"], {"p_all": None}, "null buffer"),
    (["windowed_valued"], {"p_out": None}, "null buffer"),
    (["viterbi_valued"], {"y_out": None}, "null buffer"),
    (EVERY, {"n_contigs": -1}, "bad contig_ptr"),
    (EVERY, {"contig_ptr": None}, "bad contig_ptr"),
    (EVERY, {"gene_ptr": None}, "null buffer"),
    (EVERY, {"gene_ptr": np.array([2, 4, 6, 8, 10, 1], dtype=np.int32)}, "bad gene_ptr"),
    (VALUED, {"attr_value": None}, NO_VALUES),
    # entry 3 of the arrays is entry 1 of the batch: the message names the caller's index
    (VALUED, {"attr_value": nan_at_entry_3()}, "attribute value 3 is not finite (NaN or infinite)"),
]
ROWS = [pytest.param(e, bad, msg, id=f"{e}-{'-'.join(bad)}-{k}") for k, (es, bad, msg) in enumerate(REFUSALS) for e in es]


@pytest.mark.parametrize("entry, bad, message", ROWS)
def test_each_refusal_on_its_own(model, entry, bad, message):
    assert call(model, entry, **bad) == (nat.EINVAL, message)


# the argument errors that the unvalued all-label entry used to find only behind the device and the plan
ARGUMENT_ERRORS = [r for r in REFUSALS if r[2] in ("bad contig_ptr", "null buffer", "bad gene_ptr", NO_VALUES) or "finite" in r[2]]
DEVICE_ROWS = [pytest.param(e, bad, msg, id=f"{e}-{'-'.join(bad)}-{k}") for k, (es, bad, msg) in enumerate(ARGUMENT_ERRORS)
               for e in es]


@pytest.mark.parametrize("entry, bad, message", DEVICE_ROWS)
def test_argument_error_comes_before_a_bad_device(model, entry, bad, message):
    assert call(model, entry, device=99, **bad) == (nat.EINVAL, message)


def test_calls_that_end_before_any_device_work(model):
    # nothing asked for
    assert call(model, "full_valued", marg=None, lognorm=None, device=99)[0] == nat.OK
    # no labels asked for, and no genes to label
    empty = {"contig_ptr": np.zeros(4, dtype=np.int32), "n_contigs": 3, "y_out": None, "device": 99}
    assert call(model, "viterbi_valued", **empty)[0] == nat.OK
    # ... but with genes a null y_out is refused, whatever the device
    assert call(model, "viterbi_valued", y_out=None, device=99) == (nat.EINVAL, "null buffer")
