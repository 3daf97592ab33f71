"""Run posteriors, host side (no device): the yardstick of tests/test_gpu_runs.py -- its definition (a) and its direct
recursion (b), tests/runs_reference.py -- against path enumeration; the identities of the distributions; the host refusals of
``gecco_crf_run_posteriors`` and of the Python front ends, which come before any device call; and the declarations."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import runs_reference as rr
from tests import train_objective_partial as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, U32 = np.int32, np.uint32
SHAPES = [(2, 10), (3, 7), (4, 5)]  # (labels, longest sequence)


def _lattice(rng, L, T, masked):
    A = 6
    w, trans = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    deg = rng.integers(0, 4, size=T)
    gptr = np.concatenate([[0], np.cumsum(deg)]).astype(I32)
    attr = rng.integers(0, A, size=int(gptr[-1])).astype(I32)
    allowed = tp.random_masks(rng, T, L) if masked else tp.full_masks(T, L)
    return cr.masked_scores(gptr, attr, None, w, allowed), trans


def _sets(rng, L):
    full = (1 << L) - 1
    return [full] + [1 << y for y in range(L)] + [int(m) for m in rng.integers(1, full, size=3)]


def _close(tag, got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), f"{tag}: the -inf patterns differ"
    fin = np.isfinite(ref)
    assert not np.any(np.isnan(got))
    worst = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    assert worst <= 1e-12, f"{tag}: {worst}"
    return worst


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("L,Tmax", SHAPES)
def test_definition_and_recursion_against_enumeration(L, Tmax, masked):
    rng = np.random.default_rng(100 * L + masked)
    worst, finite = 0.0, 0
    for T in sorted({1, 2, Tmax - 1, Tmax}):
        X, trans = _lattice(rng, L, T, masked)
        fb = rr.forward_backward(X, trans)
        for mask in _sets(rng, L):
            logz, anchor, start, end, joint = rr.enumerate_runs(X, trans, mask)
            assert abs(logz - fb[2]) <= 1e-12 * max(1.0, abs(logz))
            for a in range(T):
                reach = int(rng.integers(0, T + 2))
                vb, _, _ = rr.anchor_direct(X, trans, a, mask, reach, fb)
                va, _, _ = rr.anchor_by_definition(X, trans, a, mask, reach)
                want = {"log_anchor": anchor[a],
                        "log_start": np.array([start[a, a - r] if a - r >= 0 else -np.inf for r in range(reach + 1)]),
                        "log_end": np.array([end[a, a + r] if a + r < T else -np.inf for r in range(reach + 1)])}
                with np.errstate(divide="ignore"):
                    want["log_start_beyond"] = np.log(np.sum(np.exp(start[a, :max(a - reach, 0)])))
                    want["log_end_beyond"] = np.log(np.sum(np.exp(end[a, a + reach + 1:])))
                for key, ref in want.items():
                    worst = max(worst, _close(f"(a) {key} T={T} a={a} S={mask}", va[key], ref),
                                _close(f"(b) {key} T={T} a={a} S={mask}", vb[key], ref))
                    finite += int(np.isfinite(ref).sum())
                if mask == (1 << L) - 1:
                    assert np.all(np.isneginf(vb["log_start"][:min(a, reach + 1)])), "a full set starts at item 0 only"
            for b in range(T):
                row, _, _ = rr.joint_row_direct(X, trans, b, mask, fb)
                worst = max(worst, _close(f"joint row {b}", row, joint[b, b + 1:]))
                for e in range(b + 1, T + 1):
                    worst = max(worst, _close(f"run [{b}, {e})", rr.run_by_definition(X, trans, b, e, mask)[0], joint[b, e]))
    print(f"L={L} masked={masked}: {finite} finite entries, worst difference {worst:.3g}")
    assert finite > 100


@pytest.mark.parametrize("L,T", [(2, 30), (3, 25), (8, 40), (32, 20)])
def test_the_identities_of_the_distributions(L, T):
    """sum of the starts (+) the beyond-mass = the anchor's probability at every reach, the same for the ends, and the joint
    from closed runs sums to the marginal of the start."""
    rng = np.random.default_rng(7 + L)
    X, trans = _lattice(rng, L, T, masked=L != 3)
    fb = rr.forward_backward(X, trans)
    lse = lambda v: rr._lse(np.asarray(v).ravel())
    for a in (0, 1, T // 2, T - 1):
        mask = int(rng.integers(1, (1 << L) - 1)) if L < 32 else int(rng.integers(1, 1 << 31)) | (1 << 31)
        for reach in (0, 3, T + 5):
            v, _, _ = rr.anchor_direct(X, trans, a, mask, reach, fb)
            for side in ("start", "end"):
                total = lse(list(v[f"log_{side}"]) + [v[f"log_{side}_beyond"]])
                if np.isneginf(v["log_anchor"]):
                    assert np.isneginf(total)
                else:
                    assert abs(total - v["log_anchor"]) <= 1e-12
        v, _, _ = rr.anchor_direct(X, trans, a, mask, T, fb)
        # P(the run through a starts at s) = sum over e >= a of P(the run is [s, e + 1))
        for r in range(a + 1):
            row, _, _ = rr.joint_row_direct(X, trans, a - r, mask, fb)
            total = lse(row[r:])
            if np.isneginf(v["log_start"][r]):
                assert np.isneginf(total)
            else:
                assert abs(total - v["log_start"][r]) <= 1e-12 * max(1.0, abs(total))


# ---------------------------------------------------------------- the ABI's host refusals (a device that does not exist)
NAMES = ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "anchor_contig", "anchor_item", "anchor_mask",
         "n_anchors", "reach", "log_anchor", "log_start", "log_start_beyond", "log_end", "log_end_beyond", "run_contig", "run_begin",
         "run_end", "run_mask", "n_runs", "log_run", "marg", "lognorm")


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    return _native


@pytest.fixture(scope="module")
def model3(nat):
    rng = np.random.default_rng(5)
    return nat.Model.from_tables(rng.normal(size=(7, 3)), rng.normal(size=(3, 3)))


def _call(nat, model, **change):
    """A valid call on two contigs (2 and 3 genes), on a device that does not exist, with `change` applied."""
    a = {"contig_ptr": np.array([0, 2, 5], dtype=I32), "n_contigs": 2, "gene_ptr": np.arange(0, 12, 2, dtype=I32),
         "attr_id": (np.arange(10, dtype=I32) * 3) % 7, "attr_value": None, "allowed": None, "marg": np.zeros(15), "lognorm": np.zeros(2),
         "anchor_contig": np.array([0, 1], dtype=I32), "anchor_item": np.array([1, 2], dtype=I32), "anchor_mask": np.array([5, 2], dtype=U32),
         "n_anchors": 2, "reach": 4, "log_anchor": np.zeros(2), "log_start": np.zeros(10), "log_start_beyond": np.zeros(2),
         "log_end": np.zeros(10), "log_end_beyond": np.zeros(2), "run_contig": np.array([0, 1], dtype=I32),
         "run_begin": np.array([0, 1], dtype=I32), "run_end": np.array([2, 3], dtype=I32), "run_mask": np.array([7, 4], dtype=U32),
         "n_runs": 2, "log_run": np.zeros(2)}
    a.update(change)
    fn = nat.load_library().gecco_crf_run_posteriors
    args = [a[n].ctypes.data_as(t) if isinstance(a[n], np.ndarray) else a[n] for n, t in zip(NAMES, fn.argtypes[2:])]
    rc = fn(model._h, 99, *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


def test_the_entry_refuses_on_the_host(nat, model3):
    call = lambda **kw: _call(nat, model3, **kw)
    # a valid call gets past the host checks: what stops it is the device that does not exist
    assert call()[0] not in (nat.OK, nat.EINVAL)
    assert call(n_anchors=0)[0] not in (nat.OK, nat.EINVAL) and call(n_runs=0)[0] not in (nat.OK, nat.EINVAL)
    assert call(reach=0)[0] not in (nat.OK, nat.EINVAL) and call(reach=65536, n_anchors=0)[0] not in (nat.OK, nat.EINVAL)
    for kw in (dict(n_anchors=-1), dict(n_runs=-1)):
        assert call(**kw) == (nat.EINVAL, "run_posteriors: negative number of anchors or runs")
    for bad in (-1, 65537, 1 << 30):
        assert call(reach=bad) == (nat.EINVAL, f"run_posteriors: reach = {bad} is outside 0 .. 65536")
    rc, msg = call(n_anchors=32768, reach=65535)  # (refused by the count alone, before the arrays are looked at)
    assert rc == nat.EINVAL and "does not stay below 2^31" in msg and str(32768 * 65536) in msg
    for name in ("anchor_contig", "anchor_item", "anchor_mask", "log_anchor", "log_start", "log_start_beyond", "log_end",
                 "log_end_beyond", "run_contig", "run_begin", "run_end", "run_mask", "log_run"):
        assert call(**{name: None}) == (nat.EINVAL, "null buffer"), name
    assert call(run_contig=None, n_runs=0)[0] != nat.EINVAL and call(log_start=None, n_anchors=0)[0] != nat.EINVAL
    masks = lambda bad: np.array([5, bad], dtype=U32)
    for kind, arg in (("anchor", "anchor_mask"), ("run", "run_mask")):
        assert call(**{arg: masks(0)}) == (nat.EINVAL, f"{kind} 1: the label set is empty (a mask of 0)")
        assert call(**{arg: masks(8)}) == (nat.EINVAL, f"{kind} 1: the set holds a label at or above num_labels = 3 (mask 8)")
    two = lambda x, y: np.array([x, y], dtype=I32)
    assert call(anchor_contig=two(2, 0)) == (nat.EINVAL, "anchor 0: contig 2 out of range (the batch has 2)")
    assert call(run_contig=two(0, -1)) == (nat.EINVAL, "run 1: contig -1 out of range (the batch has 2)")
    assert call(anchor_item=two(2, 2)) == (nat.EINVAL, "anchor 0: item 2 lies outside contig 0 of 2 genes")
    assert call(anchor_item=two(1, -1)) == (nat.EINVAL, "anchor 1: item -1 lies outside contig 1 of 3 genes")
    for b, e in ((1, 1), (2, 1), (-1, 2), (0, 4)):
        rc, msg = call(run_begin=two(0, b), run_end=two(2, e))
        assert rc == nat.EINVAL and msg == f"run 1: [{b}, {e}) is not a non-empty range inside contig 1 of 3 genes"
    assert call(contig_ptr=None) == (nat.EINVAL, "bad contig_ptr")
    assert call(allowed=np.array([7, 1, 0, 4, 3], dtype=U32)) == (nat.EINVAL, "constrained: gene 2 allows no label (a mask of 0)")


def test_the_header_declares_the_entry_and_the_library_exports_it(nat):
    from gecco_amd import build

    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    assert "ABI 2.21.0" in header and "ABI 2.21.0 gecco_crf_run_posteriors" in re.sub(r"\s*\n \*\s*", " ", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+gecco_crf_run_posteriors\s*\(([^;]*)\)\s*;", code)
    assert m, "gecco_crf_run_posteriors is not declared"
    params = [re.sub(r"\s+", " ", p).strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["m", "device", *NAMES]
    lib = nat.load_library()
    assert hasattr(lib, "gecco_crf_run_posteriors")
    assert len(nat.SIGNATURES["gecco_crf_run_posteriors"][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    assert callable(nat.Model.run_posteriors)
    assert "crf_runs.hip" in build.SOURCES and build.EXTRA_FLAGS["crf_runs.hip"] == ["-ffp-contract=off"]
    assert os.path.exists(os.path.join(build.CSRC, "crf_runs.hip"))


# ---------------------------------------------------------------- the Python front ends
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

    for name in ("run_posteriors", "span_log_probabilities", "sample_paths", "marginals_full", "viterbi"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [], [["a0", "a3"]]]


@pytest.mark.parametrize("anchor,words", [
    ((0, 0, "w"), "unknown label 'w'"),
    ((0, 0, set()), "empty set"),
    ((3, 0, "x"), "sequence index 3 out of range"),
    ((0, 3, "x"), "item 3 lies outside sequence 0 of 3 items"),
    ((1, 0, "x"), "item 0 lies outside sequence 1 of 0 items"),
    ((0, -1, "x"), "item -1 lies outside"),
    ((0, 0.5, "x"), "expected (sequence_index, item, labels)"),
])
def test_bad_anchors_are_refused_before_any_device_call(crf, anchor, words):
    with pytest.raises(ValueError) as err:
        crf.run_posteriors(X, [(0, 1, {"x", "y"}), anchor])
    assert "anchor 1" in str(err.value) and words in str(err.value), str(err.value)


@pytest.mark.parametrize("reach", [-1, 65537, 1.5, None])
def test_a_bad_reach_is_refused_before_any_device_call(crf, reach):
    with pytest.raises(ValueError, match="reach"):
        crf.run_posteriors(X, [(0, 1, "x")], reach=reach)


def test_too_many_entries_are_refused_before_any_device_call(crf):
    with pytest.raises(ValueError, match=r"below 2\*\*31"):
        crf.run_posteriors(X, [(0, 1, "x")] * 32768, reach=65535)


@pytest.mark.parametrize("run,words", [
    ((0, 0, 2, "w"), "unknown label 'w'"),
    ((0, 0, 2, []), "empty set"),
    ((3, 0, 1, "x"), "sequence index 3 out of range"),
    ((0, 2, 2, "x"), "start >= stop"),
    ((0, -1, 2, "x"), "start < 0"),
    ((0, 0, 4, "x"), "stop 4 lies beyond sequence 0 of 3 items"),
    ((0, 0, 2), "expected (sequence_index, start, stop, labels)"),
])
def test_bad_runs_are_refused_before_any_device_call(crf, run, words):
    for method in (crf.run_log_probability, crf.run_probability):
        with pytest.raises(ValueError) as err:
            method(X, [(0, 0, 3, {"x", "y"}), run])
        assert "span 1" in str(err.value) and words in str(err.value), str(err.value)


def test_no_queries_need_no_device(crf):
    assert crf.run_posteriors(X, []) == []
    out = crf.run_log_probability(X, [])
    assert out.shape == (0,) and out.dtype == np.float64 and crf.run_probability(X, iter(())).shape == (0,)
    with pytest.raises(ValueError, match="unknown label"):
        crf.run_posteriors(X, [(0, 0, "x")], allowed=[["x", "q", None], [], [None]])


def test_the_native_wrapper_checks_its_arrays(nat, model3):
    csr = (np.array([0, 2, 5], dtype=I32), np.arange(0, 12, 2, dtype=I32), (np.arange(10, dtype=I32) * 3) % 7)
    with pytest.raises(ValueError, match="differ in length"):
        model3.run_posteriors(*csr, anchors=([0, 1], [1], [1, 1]), device=99)
    with pytest.raises(ValueError, match="differ in length"):
        model3.run_posteriors(*csr, runs=([0], [0], [1, 2], [1]), device=99)


def test_the_typed_front_end_takes_the_flag():
    from gecco_amd import typed

    for name in ("predict_clusters", "predict_genes_and_clusters"):
        params = inspect.signature(getattr(typed.TypedClusterCRF, name)).parameters
        assert params["run_posteriors"].default is False and params["run_reach"].default == 256
    base = ["predict", "--model", "m", "-f", "f", "-g", "g"]
    args = typed.build_parser().parse_args(base)
    assert args.run_posteriors is False and args.run_reach == 256
    args = typed.build_parser().parse_args(base + ["--run-posteriors", "--run-reach", "12"])
    assert args.run_posteriors is True and args.run_reach == 12
