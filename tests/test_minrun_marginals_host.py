"""Marginals under a minimum run length without a device: the yardstick's forward-backward over the expanded state list against
path enumeration (tests/minrun_marginals_reference.py), the header and the signatures of ABI 2.22.0, the host refusals of
``gecco_crf_marginals_min_run``, and the argument checks of ``SequenceCRF.predict_marginals_min_run``,
``TypedClusterCRF.predict_path_clusters(marginals=...)`` and the command line, which come before any device call."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import minrun_marginals_reference as mm
from tests import minrun_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("L,longest", [(2, 8), (3, 6)])
def test_the_recursion_equals_enumeration(L, longest):
    """1e-15 absolute in longdouble: every m of 1 .. 4, every non-empty mask, a third of the cases with a -inf entry."""
    rng = np.random.default_rng(2200 + L)
    cases = infeasible = masked = 0
    worst = worst_z = 0.0
    for T in range(1, longest + 1):
        for m in (1, 2, 3, 4):
            for mask in range(1, 1 << L):
                score, trans = rng.normal(0.0, 1.0, size=(T, L)), rng.normal(0.0, 1.5, size=(L, L))
                if cases % 3 == 0:
                    score[int(rng.integers(0, T)), int(rng.integers(0, L))] = -np.inf
                    masked += 1
                cases += 1
                want, logz = mm.enumerate_marginals(score, trans, mask, m)
                got, z, largest = mm.forward_backward(score, trans, mask, m, np.longdouble)
                assert got.dtype == np.longdouble and not np.isnan(got).any()
                if logz == -np.inf:
                    infeasible += 1
                    assert z == -np.inf and not got.any()
                    continue
                err = float(np.abs(got - want).max())
                worst, worst_z = max(worst, err), max(worst_z, abs(float(z - logz)))
                assert err <= 1e-15, (L, T, m, mask, err)
                assert abs(float(z - logz)) <= 1e-15 * max(1.0, largest), (L, T, m, mask)
                assert abs(float(got.sum(axis=1).max()) - 1.0) <= 1e-15 * L and np.all(got[score == -np.inf] == 0.0)
                # (the structured recursion of tests/minrun_reference.py sums the same paths)
                assert abs(float(z - mr.recursion(score, trans, mask, m, "sum")[0])) <= 1e-15 * max(1.0, largest)
    print(f"L={L}: {cases} cases, {masked} with a -inf entry, {infeasible} without a feasible path, worst |marginal - enumeration| "
          f"= {worst:.3g}, worst |log Z_C - enumeration| = {worst_z:.3g}")
    assert infeasible > 0 and masked * 3 >= cases


def test_the_expanded_table_is_the_run_counter_lattice():
    states, E, start, end = mm.expanded_table(np.zeros((3, 3)), 0b110, 3)
    assert states == [(0, 0), (1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3)]
    assert start.tolist() == [True, True, False, False, True, False, False]
    assert end.tolist() == [True, False, False, True, False, False, True]
    allowed = {(a, b) for a in range(7) for b in range(7) if E[a, b] == 0}
    want = set()
    for a, (i, ds) in enumerate(states):
        for b, (k, dd) in enumerate(states):
            ok = (ds == 0 and dd in (0, 1)) or (0 < ds < 3 and dd == ds + 1) or (ds == 3 and dd in (0, 3))
            if ok:
                want.add((a, b))
    assert allowed == want
    # a minimum of 1: the plain lattice
    _, E1, start1, end1 = mm.expanded_table(np.zeros((3, 3)), 0b101, 1)
    assert np.all(E1 == 0) and start1.all() and end1.all()


def test_a_planted_lone_gene_loses_its_mass():
    score = np.stack([np.zeros(9), np.full(9, -3.0)], axis=1)
    score[4, 1] = 30.0
    trans = np.zeros((2, 2))
    free, _, _ = mm.forward_backward(score, trans, 2, 1)
    held, _, _ = mm.forward_backward(score, trans, 2, 3)
    want, _ = mm.enumerate_marginals(score, trans, 2, 3)
    assert free[4, 1] > 0.9 and abs(float(held[4, 1] - want[4, 1])) <= 1e-15
    assert held[3, 1] > 10 * free[3, 1]  # (under the constraint the gene's neighbours come with it)


# ---------------------------------------------------------------- the entry: declaration, export, signature
@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    return _native


def test_the_header_declares_the_entry_and_the_library_exports_it(nat):
    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    assert "ABI 2.22.0" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+gecco_crf_marginals_min_run\s*\(([^;]*)\)\s*;", code)
    assert m, "gecco_crf_marginals_min_run is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "m", "device", "contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "set_mask", "min_run", "marg",
        "inside", "lognorm_min_run", "lognorm"]
    lib = nat.load_library()
    assert hasattr(lib, "gecco_crf_marginals_min_run")
    assert len(nat.SIGNATURES["gecco_crf_marginals_min_run"][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    sig = inspect.signature(nat.Model.marginals_min_run)
    assert list(sig.parameters) == ["self", "contig_ptr", "gene_ptr", "attr_id", "set_mask", "min_run", "device", "values", "allowed",
                                    "want_marginals", "want_inside"]
    assert sig.parameters["device"].default == 0
    assert sig.parameters["want_marginals"].default is True and sig.parameters["want_inside"].default is True


# ---------------------------------------------------------------- the entry's host refusals
L3 = 3


@pytest.fixture(scope="module")
def model3(nat):
    rng = np.random.default_rng(5)
    return nat.Model.from_tables(rng.normal(size=(7, L3)), rng.normal(size=(L3, L3)))


def _call(nat, model, device=99, **change):
    """A valid batch of two contigs (2 and 3 genes), the set {1, 2} and a minimum of 2, on a device that does not exist, with
    `change` applied."""
    a = {"contig_ptr": np.array([0, 2, 5], dtype=np.int32), "n_contigs": 2, "gene_ptr": np.arange(0, 12, 2, dtype=np.int32),
         "attr_id": (np.arange(10, dtype=np.int32) * 3) % 7, "attr_value": None, "allowed": None, "set_mask": 6, "min_run": 2,
         "marg": np.zeros((5, L3)), "inside": np.zeros(5), "lognorm_min_run": np.zeros(2), "lognorm": np.zeros(2)}
    a.update(change)
    fn = nat.load_library().gecco_crf_marginals_min_run
    names = ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "set_mask", "min_run", "marg", "inside",
             "lognorm_min_run", "lognorm")
    args = [a[n].ctypes.data_as(t) if isinstance(a[n], np.ndarray) else a[n] for n, t in zip(names, fn.argtypes[2:])]
    rc = fn(model._h, device, *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


def test_host_refusals_come_before_the_device(nat, model3):
    call = lambda **kw: _call(nat, model3, **kw)
    # a valid call gets past the host checks: what stops it is the device that does not exist
    assert call()[0] not in (nat.OK, nat.EINVAL)
    assert call(lognorm=None)[0] not in (nat.OK, nat.EINVAL)
    assert call(marg=None)[0] not in (nat.OK, nat.EINVAL) and call(inside=None)[0] not in (nat.OK, nat.EINVAL)
    assert call(min_run=1, set_mask=7)[0] not in (nat.OK, nat.EINVAL) and call(min_run=32, set_mask=1)[0] not in (nat.OK, nat.EINVAL)
    # an argument error together with a device that does not exist reports the argument
    for bad in (0, -1, 33, 1 << 20):
        assert call(min_run=bad) == (nat.EINVAL, f"marginals_min_run: min_run = {bad} is outside 1 .. 32")
    rc, msg = call(set_mask=0)
    assert rc == nat.EINVAL and msg.startswith("marginals_min_run: set_mask") and "empty" in msg
    for bad in (8, 9, 1 << 31):
        rc, msg = call(set_mask=bad)
        assert rc == nat.EINVAL and msg.startswith("marginals_min_run: set_mask")
        assert f"at or above num_labels = 3 (mask {bad})" in msg
    rc, msg = call(marg=None, inside=None)
    assert rc == nat.EINVAL and msg.startswith("marginals_min_run:") and "both NULL" in msg
    rc, msg = call(lognorm_min_run=None)
    assert rc == nat.EINVAL and msg.startswith("marginals_min_run:") and "lognorm_min_run" in msg
    # the checks of the _valued and _constrained entries
    v = np.ones(10)
    v[3] = np.inf
    assert call(attr_value=v) == (nat.EINVAL, "attribute value 3 is not finite (NaN or infinite)")
    assert call(allowed=np.array([7, 1, 0, 4, 3], dtype=np.uint32)) == (nat.EINVAL, "constrained: gene 2 allows no label (a mask of 0)")
    assert call(allowed=np.array([7, 1, 6, 4, 9], dtype=np.uint32)) == \
        (nat.EINVAL, "constrained: gene 4 allows a label at or above num_labels = 3 (mask 9)")
    assert call(contig_ptr=None)[0] == nat.EINVAL and call(n_contigs=-1)[0] == nat.EINVAL
    assert call(gene_ptr=None) == (nat.EINVAL, "null buffer")


def test_a_batch_without_genes_needs_no_device(nat, model3):
    marg, inside = np.full((1, L3), 7.0), np.full(1, 7.0)
    ln_c, ln = np.full(3, 7.0), np.full(3, 7.0)
    rc, msg = _call(nat, model3, contig_ptr=np.zeros(4, dtype=np.int32), n_contigs=3, marg=marg, inside=inside, lognorm_min_run=ln_c,
                    lognorm=ln)
    assert rc == nat.OK, msg
    assert np.all(ln_c == 0.0) and np.all(ln == 0.0) and np.all(marg == 7.0) and np.all(inside == 7.0)
    m, i, c, z = model3.marginals_min_run(np.zeros(4, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), 6, 2,
                                          device=99)
    assert m.shape == (0, L3) and i.shape == (0,) and c.tolist() == [0.0] * 3 and z.tolist() == [0.0] * 3


def test_the_native_wrapper_checks_its_arrays(nat, model3):
    cptr, gptr, attr = np.array([0, 2, 5], dtype=np.int32), np.arange(0, 12, 2, dtype=np.int32), (np.arange(10, dtype=np.int32) * 3) % 7
    with pytest.raises(ValueError, match="values holds 3 entries"):
        model3.marginals_min_run(cptr, gptr, attr, 6, 2, values=np.ones(3))
    with pytest.raises(ValueError, match="allowed holds 2 masks for 5 genes"):
        model3.marginals_min_run(cptr, gptr, attr, 6, 2, allowed=[1, 1])
    for bad in (0, 33):
        with pytest.raises(ValueError, match=rf"marginals_min_run: min_run = {bad} is outside 1 \.\. 32"):
            model3.marginals_min_run(cptr, gptr, attr, 6, bad, device=99)
    with pytest.raises(ValueError, match="set_mask"):
        model3.marginals_min_run(cptr, gptr, attr, 0, 2, device=99)
    with pytest.raises(ValueError, match="set_mask"):
        model3.marginals_min_run(cptr, gptr, attr, -1, 2)
    with pytest.raises(ValueError, match="both NULL"):
        model3.marginals_min_run(cptr, gptr, attr, 6, 2, device=99, want_marginals=False, want_inside=False)
    with pytest.raises(TypeError):
        model3.marginals_min_run(cptr, gptr, attr, 6, 2.5)


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

    for name in ("marginals_min_run", "viterbi_min_run", "marginals_full", "viterbi"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [], [["a0", "a3"]]]


def test_bad_sets_and_minima_are_refused_before_any_device_call(crf):
    for bad in (0, -3, 33):
        with pytest.raises(ValueError, match=rf"min_run = {bad} is outside 1 \.\. 32"):
            crf.predict_marginals_min_run(X, ["y"], bad)
    for bad in (2.5, "3", None):
        with pytest.raises(ValueError, match="min_run is an integer"):
            crf.predict_marginals_min_run(X, ["y"], bad)
    with pytest.raises(ValueError, match="unknown label"):
        crf.predict_marginals_min_run(X, ["y", "q"], 2)
    with pytest.raises(ValueError, match="empty"):
        crf.predict_marginals_min_run(X, [], 2)
    with pytest.raises(ValueError, match="unknown label"):
        crf.predict_marginals_min_run(X, ["y"], 2, allowed=[["x", "q", None], [], [None]])
    sig = inspect.signature(type(crf).predict_marginals_min_run)
    assert list(sig.parameters) == ["self", "X", "labels", "min_run", "allowed"] and sig.parameters["allowed"].default is None


def test_no_item_needs_no_device(crf):
    out = crf.predict_marginals_min_run([[], []], ["y", "z"], 3)
    assert len(out) == 2
    for o in out:
        assert sorted(o) == ["constraint_log_probability", "inside", "marginals"]
        assert o["marginals"].shape == (0, 3) and o["inside"].shape == (0,) and o["constraint_log_probability"] == 0.0
    assert crf.predict_marginals_min_run([], ["y"], 3) == []


def test_an_unfitted_model_is_refused():
    from gecco_amd.sequence import SequenceCRF

    with pytest.raises(ValueError, match="not fitted"):
        SequenceCRF(window_size=None).predict_marginals_min_run(X, ["y"], 2)


# ---------------------------------------------------------------- the typed front end and the command line
def test_the_typed_front_end_takes_the_arguments():
    from gecco_amd import typed

    params = inspect.signature(typed.TypedClusterCRF.predict_path_clusters).parameters
    assert params["marginals"].default is False and params["marginals"].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["min_run"].default == 3 and params["known"].default is None
    base = ["predict", "--model", "m", "-f", "f", "-g", "g"]
    assert typed.build_parser().parse_args(base).path_marginals is False
    assert typed.build_parser().parse_args(base + ["--path-clusters", "4", "--path-marginals"]).path_marginals is True


def test_the_typed_front_end_checks_the_arguments_first():
    from gecco_amd import typed

    crf = typed.TypedClusterCRF()
    for bad, words in ((0, "min_run = 0 is outside 1 .. 32"), (33, "min_run = 33 is outside"), (1.5, "min_run is an integer")):
        with pytest.raises(ValueError, match=words):
            crf.predict_path_clusters([], min_run=bad, marginals=True)
    with pytest.raises(ValueError, match="not fitted"):
        crf.predict_path_clusters([], min_run=3, marginals=True)


def test_path_marginals_without_path_clusters_is_an_error(tmp_path):
    """Before the model directory is looked at: the one given here does not exist."""
    from gecco_amd import typed

    with pytest.raises(ValueError, match="--path-marginals needs --path-clusters"):
        typed.main(["predict", "--model", os.path.join(str(tmp_path), "none"), "-f", "f", "-g", "g", "--path-marginals"])


class _Gene:
    def __init__(self, seq, start, end):
        self.source = type("S", (), {"id": seq})()
        self.start, self.end = start, end


class _Cluster:
    def __init__(self, cid, genes, **more):
        self.id, self.genes, self.path_type = cid, genes, "Alpha;Beta"
        self.__dict__.update(more)


def test_path_cluster_tables(tmp_path):
    from gecco_amd import typed

    genes = [_Gene("s1", 10, 40), _Gene("s1", 50, 90), _Gene("s1", 100, 130)]
    found = [_Cluster("s1_cluster_1", genes, average_p=0.75, max_p=1.0, min_p=0.5)]
    path = os.path.join(str(tmp_path), "path_clusters.tsv")
    today = [["sequence_id", "cluster_id", "start", "end", "genes", "type"], ["s1", "s1_cluster_1", "10", "130", "3", "Alpha;Beta"]]
    typed.write_path_clusters(path, found)
    assert [line.rstrip("\n").split("\t") for line in open(path)] == today
    typed.write_path_clusters(path, [_Cluster("s1_cluster_1", genes)])  # (clusters without the attributes: today's table)
    assert [line.rstrip("\n").split("\t") for line in open(path)] == today
    typed.write_path_clusters(path, found, marginals=True)
    assert [line.rstrip("\n").split("\t") for line in open(path)] == [today[0] + ["average_p", "max_p", "min_p"],
                                                                      today[1] + ["0.75", "1.0", "0.5"]]
    rows = {"sequence_id": ["s1", "s1"], "protein_id": ["p1", "p2"], "path_label": ["0", ""], "p": [0.125, 0.0]}
    path = os.path.join(str(tmp_path), "path_genes.tsv")
    typed.write_path_genes(path, rows)
    assert [line.rstrip("\n").split("\t") for line in open(path)] == [["sequence_id", "protein_id", "path_label", "p"],
                                                                      ["s1", "p1", "0", "0.125"], ["s1", "p2", "", "0.0"]]
