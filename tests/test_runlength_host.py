"""Run-length potentials without a device: the yardstick (tests/runlength_reference.py) against path enumeration -- log Z_g, the
best path and its score (integer weights: exact), the marginals and the expected length counts --, the counts against central
differences of the enumerated log Z_g, the host refusals of ``gecco_crf_viterbi_run_length`` and
``gecco_crf_marginals_run_length``, the header and the signatures of ABI 2.27.0, the build entry of the kernel file, and the
argument checks of the front ends, which come before any device call."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import minrun_reference as mr
from tests import runlength_reference as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


def lattice(rng, L, T, integer, masked=False):
    if integer:
        score, trans = rng.integers(-4, 5, size=(T, L)).astype(np.float64), rng.integers(-3, 4, size=(L, L)).astype(np.float64)
    else:
        score, trans = rng.normal(0.0, 1.0, size=(T, L)), rng.normal(0.0, 1.5, size=(L, L))
    if masked:
        for t in range(T):
            if rng.random() < 0.3:
                score[t, int(rng.integers(0, L))] = NINF
    return score, trans


def length_models(rng, M, integer):
    """The special cases of the model and random tables with -inf entries among them."""
    draw = (lambda k: rng.integers(-3, 4, size=k).astype(np.float64)) if integer else (lambda k: rng.normal(0.0, 1.5, size=k))
    out = [(np.zeros(M), 0.0), (np.array([NINF] * (M - 1) + [0.0]), 0.0), (draw(M), float(draw(1)[0])), (draw(M), NINF)]
    g = draw(M)
    g[int(rng.integers(0, M))] = NINF
    out.append((g, float(draw(1)[0])))
    return out


CASES = [(L, T, M) for L in (2, 3) for T in range(1, 8) for M in (1, 2, 3, 4) if L ** T <= 2200]


# ---------------------------------------------------------------- the yardstick equals enumeration
@pytest.mark.parametrize("L,T,M", CASES)
def test_the_yardstick_equals_enumeration(L, T, M):
    rng = np.random.default_rng(1000 * L + 10 * T + M)
    for integer in (True, False):
        score, trans = lattice(rng, L, T, integer, masked=T % 3 == 0)
        for g, tau in length_models(rng, M, integer):
            for mask in range(1, 1 << L):
                want = rl.enumerate_all(score, trans, mask, g, tau)
                got = rl.forward_backward(score, trans, mask, g, tau)
                path, best, tie_free = rl.max_recursion(score, trans, mask, g, tau)
                where = f"L={L} T={T} M={M} set={mask:#x} g={g} tau={tau} integer={integer}"
                if want["logz"] == NINF:
                    assert got["logz"] == NINF and not got["marg"].any() and not got["counts"].any(), where
                    assert path is None and best == NINF, where
                    continue
                assert abs(float(got["logz"] - want["logz"])) <= 1e-15 * max(1.0, abs(float(want["logz"]))) * (T + 2), where
                assert np.abs(got["marg"] - want["marg"]).max() <= 1e-16 * 50 * T, where
                assert np.abs(got["counts"] - want["counts"]).max() <= 1e-16 * 50 * T * L, where
                assert tuple(path.tolist()) in [tuple(p) for p in want["paths"]] or not integer, where
                assert rl.path_score_g(score, trans, path, mask, g, tau) == best, where
                if integer:  # exact arithmetic: the score of enumeration, bit for bit
                    assert best == want["best"], where
                else:
                    assert abs(best - want["best"]) <= 4 * (T + 2) * rl.EPS * max(1.0, abs(want["best"])) * 4, where
                    if tie_free:
                        assert [tuple(path.tolist())] == [tuple(p) for p in want["paths"]], where


def test_the_special_cases_are_what_the_table_says():
    rng = np.random.default_rng(77)
    for L, T, mask, m in ((2, 6, 2, 3), (3, 5, 6, 2), (3, 6, 7, 3), (3, 4, 1, 1)):
        score, trans = lattice(rng, L, T, integer=True)
        # the min-run table is tests/minrun_reference.py's constraint: the same best score and log Z_C
        g = np.array([NINF] * (m - 1) + [0.0])
        best, paths, logz, _ = mr.enumerate_paths(score, trans, mask, m)
        path, mine, _ = rl.max_recursion(score, trans, mask, g, 0.0)
        assert mine == best and (path is None or tuple(path.tolist()) in paths)
        assert abs(float(rl.forward_backward(score, trans, mask, g, 0.0)["logz"] - logz)) <= 1e-15 * T
        # zeros are the plain lattice
        free = mr.enumerate_paths(score, trans, mask, 1)
        assert rl.max_recursion(score, trans, mask, np.zeros(m), 0.0)[1] == free[0]
        assert abs(float(rl.forward_backward(score, trans, mask, np.zeros(m), 0.0)["logz"] - free[2])) <= 1e-15 * T
        # tau = -inf is a maximum run length
        path, _, _ = rl.max_recursion(score, trans, mask, np.zeros(m), NINF)
        assert path is None or max(rl.runs_of(path, mask), default=0) <= m
        assert rl.forward_backward(score, trans, mask, np.zeros(m), NINF)["counts"][m] == 0.0


@pytest.mark.parametrize("L,T,M", [(2, 6, 1), (2, 7, 3), (3, 5, 2), (3, 6, 4)])
def test_the_counts_are_the_derivatives_of_log_z(L, T, M):
    rng = np.random.default_rng(31 * L + T + M)
    score, trans = lattice(rng, L, T, integer=False)
    g, tau = rng.normal(0.0, 1.0, size=M), float(rng.normal())
    h = 1e-5
    for mask in range(1, 1 << L):
        counts = rl.forward_backward(score, trans, mask, g, tau)["counts"]
        assert np.abs(counts - rl.enumerate_all(score, trans, mask, g, tau)["counts"]).max() <= 1e-15 * T * L
        for d in range(M + 1):
            lo, hi = [g.copy(), tau], [g.copy(), tau]
            if d < M:
                lo[0][d] -= h
                hi[0][d] += h
            else:
                lo[1] -= h
                hi[1] += h
            slope = (rl.enumerate_all(score, trans, mask, *hi)["logz"] - rl.enumerate_all(score, trans, mask, *lo)["logz"]) / (2 * h)
            assert abs(float(slope - counts[d])) <= 1e-8, f"L={L} T={T} M={M} set={mask:#x} d={d}"


def test_observed_counts_and_the_bounds():
    assert rl.observed_counts([1, 1, 0, 1, 1, 1, 1, 0, 1], 2, 3).tolist() == [1.0, 1.0, 1.0, 1.0]
    assert rl.observed_counts([1, 2, 2, 0], 6, 1).tolist() == [1.0, 2.0]
    assert rl.observed_counts([0, 0], 2, 2).tolist() == [0.0, 0.0, 0.0]
    assert rl.log_bound(9, 3, 4, 0.5) == 10 * (6 + 8 + 4 + 2) * rl.EPS
    assert rl.log_bound(9, 3, 4, 20.0) == 20.0 * rl.log_bound(9, 3, 4, 1.0)
    assert rl.marginal_bound(9, 3, 4, 1.0) == float(np.expm1(3 * rl.log_bound(9, 3, 4, 1.0) + 8 * rl.EPS))
    assert rl.count_bound(9, 3, 4, 1.0) == float(np.expm1(3 * rl.log_bound(9, 3, 4, 1.0) + (27 + 3 + 4) * rl.EPS))


# ---------------------------------------------------------------- the C entries: refusals before the device, header, signatures
L3 = 3


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    return _native


@pytest.fixture(scope="module")
def model3(nat):
    rng = np.random.default_rng(5)
    return nat.Model.from_tables(rng.normal(size=(7, L3)), rng.normal(size=(L3, L3)))


MODEL_NAMES = ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "set_mask", "max_length", "length_score", "tail")
NAMES = {"viterbi_run_length": MODEL_NAMES + ("y", "score", "lognorm_run_length", "lognorm"),
         "marginals_run_length": MODEL_NAMES + ("marg", "inside", "counts", "lognorm_run_length", "lognorm")}


def _call(nat, model, entry, **change):
    """A valid batch of two contigs (2 and 3 genes) and a table of three scores, on a device that does not exist, with `change`."""
    i32 = lambda *x: np.array(x, dtype=np.int32)  # noqa: E731
    a = {"contig_ptr": i32(0, 2, 5), "n_contigs": 2, "gene_ptr": np.arange(0, 12, 2, dtype=np.int32),
         "attr_id": (np.arange(10, dtype=np.int32) * 3) % 7, "attr_value": None, "allowed": None, "set_mask": 6, "max_length": 3,
         "length_score": np.array([NINF, -1.0, 0.5]), "tail": -0.25, "y": np.zeros(5, dtype=np.int8), "score": np.zeros(2),
         "lognorm_run_length": np.zeros(2), "lognorm": np.zeros(2), "marg": np.zeros(15), "inside": np.zeros(5), "counts": np.zeros(8)}
    a.update(change)
    fn = getattr(nat.load_library(), "gecco_crf_" + entry)
    args = [a[n].ctypes.data_as(t) if isinstance(a[n], np.ndarray) else a[n] for n, t in zip(NAMES[entry], fn.argtypes[2:])]
    rc = fn(model._h, 99, *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


@pytest.mark.parametrize("entry", ["viterbi_run_length", "marginals_run_length"])
def test_host_refusals_come_before_the_device(nat, model3, entry):
    call = lambda **kw: _call(nat, model3, entry, **kw)  # noqa: E731
    u32 = lambda *x: np.array(x, dtype=np.uint32)  # noqa: E731
    # a valid call gets past the host checks: what stops it is the device that does not exist
    assert call()[0] not in (nat.OK, nat.EINVAL)
    assert call(tail=NINF)[0] not in (nat.OK, nat.EINVAL) and call(lognorm=None)[0] not in (nat.OK, nat.EINVAL)
    assert call(max_length=32, length_score=np.zeros(32), counts=np.zeros(66))[0] not in (nat.OK, nat.EINVAL)
    assert call(max_length=1, length_score=np.array([NINF]))[0] not in (nat.OK, nat.EINVAL)
    for bad in (0, -1, 33, 1 << 20):
        assert call(max_length=bad) == (nat.EINVAL, f"{entry}: max_length = {bad} is outside 1 .. 32")
    assert call(length_score=np.array([0.0, np.nan, 0.0])) == (
        nat.EINVAL, f"{entry}: length_score[1] is NaN or +infinity (a score is finite or -infinity)")
    assert call(length_score=np.array([0.0, 0.0, np.inf]))[1].startswith(f"{entry}: length_score[2] is NaN or +infinity")
    for bad in (np.nan, np.inf):
        assert call(tail=bad) == (nat.EINVAL, f"{entry}: tail is NaN or +infinity (a score is finite or -infinity)")
    assert call(length_score=None) == (nat.EINVAL, f"{entry}: length_score is NULL")
    rc, msg = call(set_mask=0)
    assert rc == nat.EINVAL and msg.startswith(f"{entry}: set_mask") and "the label set is empty" in msg
    rc, msg = call(set_mask=9)
    assert rc == nat.EINVAL and msg.startswith(f"{entry}: set_mask") and "at or above num_labels = 3" in msg
    if entry == "viterbi_run_length":
        assert call(lognorm_run_length=None)[0] not in (nat.OK, nat.EINVAL)
        assert call(score=None) == (nat.EINVAL, "viterbi_run_length: score is NULL")
        assert call(y=None) == (nat.EINVAL, "viterbi_run_length: y is NULL")
    else:
        for keep in ("marg", "inside", "counts"):
            others = {n: None for n in ("marg", "inside", "counts") if n != keep}
            assert call(**others)[0] not in (nat.OK, nat.EINVAL), keep
        assert call(marg=None, inside=None, counts=None) == (nat.EINVAL, "marginals_run_length: marg, inside and counts are all NULL")
        assert call(lognorm_run_length=None) == (nat.EINVAL, "marginals_run_length: lognorm_run_length is NULL")
    # the checks of the _valued and _constrained entries
    v = np.ones(10)
    v[3] = np.inf
    assert call(attr_value=v) == (nat.EINVAL, "attribute value 3 is not finite (NaN or infinite)")
    assert call(allowed=u32(7, 1, 0, 4, 3)) == (nat.EINVAL, "constrained: gene 2 allows no label (a mask of 0)")
    assert call(contig_ptr=None)[0] == nat.EINVAL and call(n_contigs=-1)[0] == nat.EINVAL
    assert call(gene_ptr=None) == (nat.EINVAL, "null buffer")


def test_a_batch_without_genes_needs_no_device(nat, model3):
    lz, lzg, counts = np.full(3, 7.0), np.full(3, 9.0), np.full(12, 5.0)
    rc, msg = _call(nat, model3, "marginals_run_length", contig_ptr=np.zeros(4, dtype=np.int32), n_contigs=3, lognorm=lz,
                    lognorm_run_length=lzg, counts=counts)
    assert rc == nat.OK, msg
    assert np.all(lz == 0.0) and np.all(lzg == 0.0) and np.all(counts == 0.0)
    score = np.full(3, 9.0)
    rc, msg = _call(nat, model3, "viterbi_run_length", contig_ptr=np.zeros(4, dtype=np.int32), n_contigs=3, score=score)
    assert rc != nat.EINVAL, msg
    if rc == nat.OK:
        assert np.all(score == 0.0)


def test_the_header_declares_the_entries_and_the_library_exports_them(nat):
    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    assert "ABI 2.27.0 gecco_crf_viterbi_run_length and gecco_crf_marginals_run_length" in flat
    for words in ("g[min(n_r, M)] + tau * max(n_r - M, 0)", "the plain lattice", "gecco_crf_viterbi_min_run with min_run = m",
                  "a maximum run length M", "a soft duration model", "never NaN", "1 <= max_length <= 32",
                  "((delta + g or tau) + trans) + state", "the aggregate scans d ascending with a strict `>`",
                  "n_genes * L * (M + 1) bytes", "counts[c][M] is exactly 0.0", "no atomics"):
        assert words in flat, words
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = nat.load_library()
    for entry, names in NAMES.items():
        m = re.search(rf"\bint\s+gecco_crf_{entry}\s*\(([^;]*)\)\s*;", code)
        assert m, f"gecco_crf_{entry} is not declared"
        params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == ["m", "device", *names]
        assert hasattr(lib, "gecco_crf_" + entry)
        assert len(nat.SIGNATURES["gecco_crf_" + entry][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    for fn in (nat.Model.viterbi_run_length, nat.Model.marginals_run_length):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[:10] == ["self", "contig_ptr", "gene_ptr", "attr_id", "set_mask", "length_scores", "tail", "device",
                                             "values", "allowed"]
        assert sig.parameters["tail"].default == 0.0
    assert inspect.signature(nat.Model.marginals_run_length).parameters["want_counts"].default is True


def test_the_kernel_file_is_built_without_contraction():
    from gecco_amd import build

    at = build.SOURCES.index("crf_maxmarg.hip")
    assert build.SOURCES[at + 1] == "crf_runlength.hip" and build.EXTRA_FLAGS["crf_runlength.hip"] == ["-ffp-contract=off"]
    assert build.SOURCES[build.SOURCES.index("crf_minrun.hip") + 1] == "crf_counts.hip"
    text = open(os.path.join(ROOT, "gecco_amd", "csrc", "crf_runlength.hip")).read()
    assert '#include "crf_contig_walk.hpp"' in text and "load_trans<true>" in text and "dispatch_lp(" in text
    for kernel in ("gl_runlen_forward", "gl_runlen_backtrack", "gl_runlen_backward"):
        assert kernel in text
    assert "atomic" not in text.replace("No atomics", "") and "asm" not in text


def test_the_native_wrapper_checks_its_arrays(nat, model3):
    cptr, gptr, attr = np.array([0, 2, 5], dtype=np.int32), np.arange(0, 12, 2, dtype=np.int32), (np.arange(10, dtype=np.int32) * 3) % 7
    for fn, name in ((model3.viterbi_run_length, "viterbi_run_length"), (model3.marginals_run_length, "marginals_run_length")):
        with pytest.raises(ValueError, match="values holds 3 entries"):
            fn(cptr, gptr, attr, 6, [0.0, 0.0], values=np.ones(3))
        with pytest.raises(ValueError, match="allowed holds 2 masks for 5 genes"):
            fn(cptr, gptr, attr, 6, [0.0, 0.0], allowed=[1, 1])
        with pytest.raises(ValueError, match=f"{name}: set_mask -1 is outside"):
            fn(cptr, gptr, attr, -1, [0.0])
        with pytest.raises(ValueError, match=f"{name}: length_scores is a one-dimensional table"):
            fn(cptr, gptr, attr, 6, [[0.0]])
        with pytest.raises(ValueError, match=rf"{name}: max_length = 33 is outside 1 \.\. 32"):
            fn(cptr, gptr, attr, 6, np.zeros(33))
        with pytest.raises(ValueError, match=rf"{name}: max_length = 0 is outside 1 \.\. 32"):
            fn(cptr, gptr, attr, 6, [])
        with pytest.raises(ValueError, match=rf"{name}: length_score\[0\] is NaN or \+infinity"):
            fn(cptr, gptr, attr, 6, [np.nan])
        with pytest.raises(ValueError, match=f"{name}: set_mask"):
            fn(cptr, gptr, attr, 8, [0.0])


# ---------------------------------------------------------------- SequenceCRF
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

    for name in ("viterbi_run_length", "marginals_run_length", "marginals_full", "viterbi"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [], [["a0", "a3"]]]
Y = [["x", "y", "y"], [], ["z"]]


def test_the_front_end_refuses_before_any_device_call(crf):
    for fn in (crf.predict_run_length, crf.predict_marginals_run_length, crf.run_length_counts):
        with pytest.raises(ValueError, match="unknown label 'w'"):
            fn(X, ["y", "w"], [0.0])
        with pytest.raises(ValueError, match="an empty set holds no label"):
            fn(X, [], [0.0])
        with pytest.raises(ValueError, match=r"length_scores holds 1 \.\. 32 scores"):
            fn(X, "y", [])
        with pytest.raises(ValueError, match=r"length_scores holds 1 \.\. 32 scores"):
            fn(X, "y", np.zeros(33))
        with pytest.raises(ValueError, match="a score is finite or -inf"):
            fn(X, "y", [0.0, np.nan])
        with pytest.raises(ValueError, match="a score is finite or -inf"):
            fn(X, "y", [np.inf])
        with pytest.raises(ValueError, match="tail = nan is not finite or -inf"):
            fn(X, "y", [0.0], tail=np.nan)
        with pytest.raises(ValueError, match="length_scores is a list of numbers"):
            fn(X, "y", ["a"])
    with pytest.raises(ValueError, match="unknown label 'w'"):
        crf.predict_run_length(X, "y", [0.0], allowed=[["x", "w", None], [], [None]])
    # nothing to ask: no device either
    empty = crf.predict_run_length([[], []], "y", [0.0, NINF], tail=NINF)
    assert empty == [{"labels": [], "score": 0.0, "log_probability_given_model": 0.0, "log_mass_ratio": 0.0}] * 2
    empty = crf.predict_marginals_run_length([[]], "y", [0.0, 1.0])
    assert empty[0]["marginals"].shape == (0, 3) and empty[0]["counts"].tolist() == [0.0, 0.0, 0.0] and empty[0]["log_mass_ratio"] == 0.0
    assert crf.run_length_counts([[], []], ["y", "z"], np.zeros(4)).shape == (2, 5)


def test_the_fit_refuses_before_any_device_call(crf):
    fit = crf.fit_run_length_scores
    with pytest.raises(ValueError, match="unknown label 'w'"):
        fit(X, Y, "w", 4)
    for bad in (0, 33, -2):
        with pytest.raises(ValueError, match=rf"max_length = {bad} is outside 1 \.\. 32"):
            fit(X, Y, "y", bad)
    with pytest.raises(ValueError, match="max_length is an integer"):
        fit(X, Y, "y", 2.5)
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="is not a positive number"):
            fit(X, Y, "y", 4, c2=bad)
    with pytest.raises(ValueError, match="X holds 3 sequences and y 2"):
        fit(X, Y[:2], "y", 4)
    with pytest.raises(ValueError, match="sequence 0: 3 items but 2 labels"):
        fit(X, [["x", "y"], [], ["z"]], "y", 4)
    with pytest.raises(ValueError, match="takes one label per item"):
        fit(X, [["x", {"y", "z"}, "y"], [], ["z"]], "y", 4)
    with pytest.raises(ValueError, match="takes one label per item"):
        fit(X, [["x", None, "y"], [], ["z"]], "y", 4)
    with pytest.raises(ValueError, match="unknown label 'q'"):
        fit(X, [["x", "q", "y"], [], ["z"]], "y", 4)
    g, tau = fit([[], []], [[], []], "y", 5)
    assert g.tolist() == [0.0] * 5 and tau == 0.0


def test_observed_run_lengths_are_the_yardsticks():
    from gecco_amd.sequence import SequenceCRF

    rng = np.random.default_rng(3)
    paths = [rng.integers(0, 3, size=int(rng.integers(0, 25))).tolist() for _ in range(30)]
    for mask, M in ((2, 1), (6, 3), (7, 4), (1, 32)):
        got = SequenceCRF.observed_run_lengths(paths, lambda k: (mask >> k) & 1, M)
        want = np.array([rl.observed_counts(p, mask, M) for p in paths])
        assert got.shape == (30, M + 1) and np.array_equal(got, want)


# ---------------------------------------------------------------- the typed front end
def test_the_typed_front_end_takes_the_arguments():
    from gecco_amd import typed

    params = inspect.signature(typed.TypedClusterCRF.predict_path_clusters).parameters
    assert params["length_model"].default is False and params["length_model"].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["min_run"].default == 3 and params["marginals"].default is False
    fit = inspect.signature(typed.TypedClusterCRF.fit_length_model).parameters
    assert list(fit) == ["self", "genes", "clusters", "max_length", "c2"] and fit["max_length"].default == 32 and fit["c2"].default == 1.0
    base = ["predict", "--model", "m", "-f", "f", "-g", "g"]
    args = typed.build_parser().parse_args(base)
    assert args.path_clusters is None and args.length_model is False
    args = typed.build_parser().parse_args(base + ["--path-clusters", "--length-model", "--path-marginals"])
    assert args.path_clusters == 0 and args.length_model is True and args.path_marginals is True
    assert typed.build_parser().parse_args(base + ["--path-clusters", "4"]).path_clusters == 4
    train = ["train", "-f", "f", "-g", "g", "-c", "c"]
    args = typed.build_parser().parse_args(train)
    assert args.length_model is None and args.length_c2 == 1.0
    args = typed.build_parser().parse_args(train + ["--length-model", "12", "--length-c2", "0.25"])
    assert args.length_model == 12 and args.length_c2 == 0.25


def test_the_length_model_travels_with_the_model_directory(tmp_path):
    from gecco_amd import typed
    from gecco_amd.crfsuite_model import model_bytes

    rng = np.random.default_rng(9)
    An, L = 3, 2
    blob = model_bytes(["0", "Polyketide"], [f"a{k}" for k in range(An)], np.repeat(np.arange(An), L), np.tile(np.arange(L), An),
                       np.repeat(np.arange(L), L), np.tile(np.arange(L), L), rng.normal(size=An * L + L * L))
    crf = typed.TypedClusterCRF(5, 1)
    crf._set_blob(blob)
    assert crf.length_scores_ is None and crf.length_tail_ is None
    with pytest.raises(ValueError, match="has no length model"):
        crf.predict_path_clusters([], length_model=True)
    old = os.path.join(str(tmp_path), "old")
    crf.save(old)
    assert sorted(os.listdir(old)) == sorted([typed.MODEL_FILE, typed.META_FILE])
    assert typed.TypedClusterCRF.trained(old).length_scores_ is None  # (an older directory loads with no length model)
    crf.length_scores_, crf.length_tail_ = np.array([NINF, -1.0 / 3.0, 0.1, 2.5e-300]), -0.7
    with pytest.raises(ValueError, match="give one"):
        crf.predict_path_clusters([], min_run=3, length_model=True)
    assert crf.predict_path_clusters([], length_model=True) == []
    new = os.path.join(str(tmp_path), "new")
    crf.save(new)
    assert sorted(os.listdir(new)) == sorted([typed.MODEL_FILE, typed.META_FILE, typed.LENGTH_FILE])
    lines = open(os.path.join(new, typed.LENGTH_FILE)).read().splitlines()
    assert lines[0] == "length\tscore" and [ln.split("\t")[0] for ln in lines[1:]] == ["1", "2", "3", "4", "tail"] and lines[1] == "1\t-inf"
    again = typed.TypedClusterCRF.trained(new)
    assert again.length_scores_.tobytes() == crf.length_scores_.tobytes() and again.length_tail_ == -0.7
    open(os.path.join(new, typed.LENGTH_FILE), "w").write("length\tscore\n1\t0.0\n3\t0.0\ntail\t0.0\n")
    with pytest.raises(ValueError, match="expected the columns length, score"):
        typed.TypedClusterCRF.trained(new)
    crf.length_scores_ = crf.length_tail_ = None
    crf.save(new)
    assert typed.LENGTH_FILE not in os.listdir(new)
