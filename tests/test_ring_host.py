"""Circular sequences without a device: the yardstick (tests/ring_reference.py) against path enumeration -- log Z of the ring, the
marginals, the best path and its score (integer weights: exact) --, the one-item self-edge and the two-item double edge, rotation
of a ring, the header and the signature of ABI 2.28.0, the build entry of the kernel file, and the front ends with a stubbed
native call: a mixed batch split and put back in order, a cluster across the cut, a ring that is one cluster, every refusal."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import ring_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


def lattice(rng, L, n, integer, masked=False):
    if integer:
        score, trans = rng.integers(-4, 5, size=(n, L)).astype(np.float64), rng.integers(-3, 4, size=(L, L)).astype(np.float64)
    else:
        score, trans = rng.normal(0.0, 1.0, size=(n, L)), rng.normal(0.0, 1.5, size=(L, L))
    if masked:
        for t in range(n):
            if rng.random() < 0.4:
                score[t, int(rng.integers(0, L))] = NINF
    return score, trans


def ring_score_exact(score, trans, path):
    n = len(path)
    return sum(score[t, path[t]] + trans[path[t], path[(t + 1) % n]] for t in range(n))


# ---------------------------------------------------------------- the yardstick equals enumeration
CASES = [(L, n) for L in (2, 3, 4) for n in (1, 2, 3, 6) if L ** n <= 4096]


@pytest.mark.parametrize("L,n", CASES)
def test_the_walks_equal_enumeration(L, n):
    rng = np.random.default_rng(100 * L + n)
    for integer in (True, False):
        for masked in (False, True):
            for _ in range(3):
                score, trans = lattice(rng, L, n, integer, masked)
                want = rr.enumerate_ring(score, trans)
                lognorm, marg, largest = rr.sum_walks(score, trans)
                path, best = rr.best_path(score, trans)
                where = f"L={L} n={n} integer={integer} masked={masked}"
                if want["path"] is None:
                    assert lognorm == NINF and not marg.any() and path is None and best == NINF, where
                    continue
                assert abs(float(lognorm - want["lognorm"])) <= rr.lognorm_bound(n, L, largest), where
                assert np.abs(marg - want["marginals"]).max() <= 1e-12, where
                assert np.abs(marg.sum(axis=1) - 1.0).max() <= 1e-12, where
                assert best == want["score"], f"{where}: the best score is the best enumerated path's, bit for bit"
                assert best == rr.ring_score(score, trans, path), where
                if integer:
                    assert tuple(path.tolist()) == want["path"], f"{where}: the tie rule"
                    assert best == ring_score_exact(score, trans, want["path"]), where


def test_a_ring_of_one_item_has_the_self_edge():
    rng = np.random.default_rng(1)
    for L in (2, 3, 5):
        score, trans = lattice(rng, L, 1, integer=False)
        closed = score[0] + np.diag(trans)
        lognorm, marg, _ = rr.sum_walks(score, trans)
        assert abs(float(lognorm) - np.log(np.exp(closed).sum())) <= 1e-13
        assert np.abs(marg[0] - np.exp(closed) / np.exp(closed).sum()).max() <= 1e-13
        path, best = rr.best_path(score, trans)
        assert path.tolist() == [int(closed.argmax())] and best == closed.max()
        assert rr.ring_score(score, trans, [2 % L]) == score[0, 2 % L] + trans[2 % L, 2 % L]
        want = rr.enumerate_ring(score, trans)
        assert want["path"] == (int(closed.argmax()),) and want["score"] == best
    # the self-edge decides: the state scores prefer label 0, the ring label 1
    score, trans = np.array([[1.0, 0.0]]), np.array([[-5.0, 9.0], [9.0, 0.0]])
    path, best = rr.best_path(score, trans)
    assert path.tolist() == [1] and best == 0.0


def test_a_ring_of_two_items_has_both_edges():
    rng = np.random.default_rng(2)
    for L in (2, 3, 4):
        score, trans = lattice(rng, L, 2, integer=False)
        table = score[0][:, None] + trans + score[1][None, :] + trans.T  # [y0, y1]: T[y0, y1] and T[y1, y0]
        lognorm, marg, _ = rr.sum_walks(score, trans)
        z = np.exp(table).sum()
        assert abs(float(lognorm) - np.log(z)) <= 1e-13
        assert np.abs(marg[0] - np.exp(table).sum(axis=1) / z).max() <= 1e-13
        assert np.abs(marg[1] - np.exp(table).sum(axis=0) / z).max() <= 1e-13
        path, best = rr.best_path(score, trans)
        assert abs(best - table.max()) <= 1e-14 and abs(table[path[0], path[1]] - table.max()) <= 1e-14
    # an antisymmetric transition table: a chain prefers 0 -> 1, on the ring the edge back costs as much
    score, trans = np.zeros((2, 2)), np.array([[0.0, 3.0], [-3.0, 0.0]])
    path, best = rr.best_path(score, trans)
    assert best == 0.0 and path.tolist() == [0, 0]


@pytest.mark.parametrize("L,n", [(2, 5), (3, 7), (5, 12)])
def test_rotating_a_ring_rotates_the_marginals_and_keeps_log_z(L, n):
    rng = np.random.default_rng(7 * L + n)
    score, trans = lattice(rng, L, n, integer=False, masked=True)
    lognorm, marg, largest = rr.sum_walks(score, trans)
    _, best = rr.best_path(score, trans)
    bound = rr.bound(np.where(np.isfinite(score), np.abs(score), 0.0), np.abs(trans))
    for r in range(1, n):
        ln_r, marg_r, big = rr.sum_walks(np.roll(score, -r, axis=0), trans)
        assert abs(float(ln_r - lognorm)) <= 2 * rr.lognorm_bound(n, L, max(largest, big))
        assert np.abs(marg_r - np.roll(marg, -r, axis=0)).max() <= 1e-12
        assert abs(rr.best_path(np.roll(score, -r, axis=0), trans)[1] - best) <= bound
    # integer weights and a unique best path: the path rotates with the ring
    score, trans = lattice(rng, L, n, integer=True)
    score[np.arange(n), rng.integers(0, L, size=n)] += 40.0
    path, best = rr.best_path(score, trans)
    for r in range(1, n):
        path_r, best_r = rr.best_path(np.roll(score, -r, axis=0), trans)
        assert best_r == best and path_r.tolist() == np.roll(path, -r).tolist()


# ---------------------------------------------------------------- the ABI
def test_the_header_declares_the_entry_and_the_library_exports_it():
    from gecco_amd import _native as nat

    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    assert "ABI 2.28.0 gecco_crf_ring" in flat
    for words in ("EVERY contig of the call is a RING", "trans[y_0][y_0]", "the smaller a", "8 * n_genes * L * L bytes",
                  "n_genes * L bytes", "no atomics", "never NaN", 'prefixed "ring:"', "num_labels <= 32"):
        assert words in flat, words
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+gecco_crf_ring\s*\(([^;]*)\)\s*;", code)
    assert m, "gecco_crf_ring is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["m", "device", "contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value",
                                                           "allowed", "y", "score", "marg", "lognorm_ring"]
    lib = nat.load_library()
    assert hasattr(lib, "gecco_crf_ring") and len(nat.SIGNATURES["gecco_crf_ring"][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    sig = inspect.signature(nat.Model.ring)
    assert list(sig.parameters) == ["self", "contig_ptr", "gene_ptr", "attr_id", "device", "values", "allowed", "want_path", "want_marginals"]


def test_the_kernel_file_is_built_without_contraction():
    from gecco_amd import build

    assert build.SOURCES[build.SOURCES.index("crf_runlength.hip") + 1] == "crf_ring.hip"
    assert build.EXTRA_FLAGS["crf_ring.hip"] == ["-ffp-contract=off"]
    text = open(os.path.join(ROOT, "gecco_amd", "csrc", "crf_ring.hip")).read()
    assert '#include "crf_contig_walk.hpp"' in text and "load_trans<true>" in text and "dispatch_lp(" in text
    for kernel in ("gl_ring_forward", "gl_ring_viterbi", "gl_ring_backtrack", "gl_ring_backward"):
        assert kernel in text
    assert "atomic" not in text.replace("No atomics", "") and "asm" not in text


def test_the_host_refusals_come_before_the_device():
    from gecco_amd import _native as nat

    model = nat.Model.from_tables(np.zeros((4, 3)), np.zeros((3, 3)))
    lib = nat.load_library()
    cptr, gptr, attr = np.array([0, 2], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    y, score, lz = np.zeros(2, dtype=np.int8), np.zeros(1), np.zeros(1)
    i32, f64, i8 = nat._c_i32p, nat._c_f64p, nat._c_i8p
    head = [model._h, 0, nat._ptr(cptr, i32), 1, nat._ptr(gptr, i32), nat._ptr(attr, i32), None, None]

    def call(*tail):
        rc = lib.gecco_crf_ring(*head, *tail)
        return rc, lib.gecco_crf_last_error().decode()

    assert call(nat._ptr(y, i8), nat._ptr(score, f64), None, None) == (nat.EINVAL, "ring: lognorm_ring is NULL")
    assert call(nat._ptr(y, i8), None, None, nat._ptr(lz, f64)) == (nat.EINVAL, "ring: y given without score")
    assert call(None, nat._ptr(score, f64), None, nat._ptr(lz, f64)) == (nat.EINVAL, "ring: score given without y")
    # more than 32 labels: refused before the device is looked at -- device 12345 does not exist, and the answer is not ENODEV
    rng = np.random.default_rng(0)
    wide = nat.Model.from_tables(rng.normal(size=(9, 33)), rng.normal(size=(33, 33)))
    for device in (0, 12345):
        rc = lib.gecco_crf_ring(wide._h, device, *head[2:], nat._ptr(y, i8), nat._ptr(score, f64), None, nat._ptr(lz, f64))
        assert (rc, lib.gecco_crf_last_error().decode()) == (nat.EINVAL, "ring: num_labels = 33 is above 32")
    with pytest.raises(ValueError, match="ring: num_labels = 33 is above 32"):
        wide.ring(cptr, gptr, attr, device=12345)
    head[1] = 12345  # the other refusals likewise
    assert call(nat._ptr(y, i8), None, None, nat._ptr(lz, f64)) == (nat.EINVAL, "ring: y given without score")
    assert call(nat._ptr(y, i8), nat._ptr(score, f64), None, None) == (nat.EINVAL, "ring: lognorm_ring is NULL")
    # a batch without genes needs no device
    lz2, sc2 = np.full(3, 7.0), np.full(3, 7.0)
    zero = np.zeros(4, dtype=np.int32)
    rc = lib.gecco_crf_ring(model._h, 0, nat._ptr(zero, i32), 3, nat._ptr(gptr, i32), nat._ptr(attr, i32), None, None, nat._ptr(y, i8),
                            nat._ptr(sc2, f64), None, nat._ptr(lz2, f64))
    assert rc != nat.EINVAL
    if rc == nat.OK:
        assert np.all(lz2 == 0.0) and np.all(sc2 == 0.0)


# ---------------------------------------------------------------- SequenceCRF with a stubbed native call
class _StubModel:
    """Answers with numbers that name the call and the sequence: chain calls label every item 0, ring calls label it 1."""

    def __init__(self, L, real):
        self.L, self.calls = L, []
        self.state_weights, self.trans_weights = real.state_weights, real.trans_weights

    def viterbi(self, seq_ptr, item_ptr, attr, device=0, values=None, allowed=None):
        self.calls.append(("viterbi", np.diff(seq_ptr).tolist(), None if allowed is None else allowed.tolist()))
        return np.zeros(int(seq_ptr[-1]), dtype=np.int8), np.zeros(len(seq_ptr) - 1)

    def marginals_full(self, seq_ptr, item_ptr, attr, device=0, values=None, allowed=None):
        self.calls.append(("marginals_full", np.diff(seq_ptr).tolist(), None if allowed is None else allowed.tolist()))
        return np.full((int(seq_ptr[-1]), self.L), 0.25), np.full(len(seq_ptr) - 1, 2.0)

    def ring(self, seq_ptr, item_ptr, attr, device=0, values=None, allowed=None, want_path=True, want_marginals=True):
        self.calls.append(("ring", np.diff(seq_ptr).tolist(), None if allowed is None else allowed.tolist(), want_path, want_marginals))
        n, nc = int(seq_ptr[-1]), len(seq_ptr) - 1
        out = {"lognorm": 10.0 + np.arange(nc)}
        if want_path:
            out.update(labels=np.ones(n, dtype=np.int8), score=3.0 + np.arange(nc))
        if want_marginals:
            out["marginals"] = np.full((n, self.L), 0.5)
        return out


@pytest.fixture()
def crf():
    from gecco_amd.crfsuite_model import model_bytes
    from gecco_amd.sequence import SequenceCRF

    An, L = 4, 3
    names, classes = [f"a{k}" for k in range(An)], ["x", "y", "z"]
    w = np.arange(An * L + L * L, dtype=np.float64)
    blob = model_bytes(classes, names, np.repeat(np.arange(An), L), np.tile(np.arange(L), An), np.repeat(np.arange(L), L),
                       np.tile(np.arange(L), L), w)
    crf = SequenceCRF.from_bytes(blob, window_size=None)
    crf._model = _StubModel(L, crf._model)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [["a1"]], [], [["a0", "a3"], ["a2"]], [["a2"]]]


def test_a_mixed_batch_is_split_and_put_back_in_order(crf):
    flags = [True, False, False, True, False]
    got = crf.predict(X, circular=flags)
    assert got == [["y"] * 3, ["x"], [], ["y"] * 2, ["x"]]
    assert crf._model.calls == [("viterbi", [1, 0, 1], None), ("ring", [3, 2], None, True, False)]
    crf._model.calls.clear()
    allowed = [[None, "x", {"y", "z"}], [None], [], ["z", None], ["x"]]
    marg = crf.predict_marginals(X, allowed=allowed, circular=flags)
    assert [m.shape for m in marg] == [(3, 3), (1, 3), (0, 3), (2, 3), (1, 3)]
    assert [float(m[0, 0]) if len(m) else None for m in marg] == [0.5, 0.25, None, 0.5, 0.25]
    assert crf._model.calls == [("marginals_full", [1, 0, 1], [7, 1]), ("ring", [3, 2], [7, 1, 6, 4, 7], False, True)]
    # None: today's call, the whole batch at once; True: every sequence to the ring entry
    crf._model.calls.clear()
    assert crf.predict(X) == [["x"] * 3, ["x"], [], ["x"] * 2, ["x"]]
    assert crf.predict(X, circular=True) == [["y"] * 3, ["y"], [], ["y"] * 2, ["y"]]
    assert crf.predict(X, circular=[False] * 5) == crf.predict(X)
    assert [c[:2] for c in crf._model.calls] == [("viterbi", [3, 1, 0, 2, 1]), ("ring", [3, 1, 0, 2, 1]), ("viterbi", [3, 1, 0, 2, 1]),
                                                  ("viterbi", [3, 1, 0, 2, 1])]
    with pytest.raises(ValueError, match="X holds 5 sequences and circular 2 flags"):
        crf.predict(X, circular=[True, False])
    with pytest.raises(ValueError, match="X holds 5 sequences and allowed 1"):
        crf.predict(X, allowed=[[None]], circular=flags)
    # a batch without items never reaches the device
    crf._model.calls.clear()
    assert crf.predict([[], []], circular=True) == [[], []] and crf.predict_ring([[]])[0]["labels"] == []
    assert crf._model.calls == []


def test_predict_ring_and_the_ring_log_likelihood(crf):
    out = crf.predict_ring(X)
    assert [sorted(o) for o in out] == [["labels", "log_probability", "lognorm", "marginals", "score"]] * 5
    assert [o["score"] for o in out] == [3.0, 4.0, 5.0, 6.0, 7.0] and [o["log_probability"] for o in out] == [-7.0] * 5
    assert out[3]["labels"] == ["y", "y"] and out[3]["marginals"].shape == (2, 3)
    # the host adds the closing edge: state weights w[a, l] = 3 a + l, transitions 12 + 3 i + j
    y = [["x", "z", "y"], ["y"], [], ["z", "z"], ["x"]]
    flags = [True, True, True, True, False]
    crf._model.calls.clear()
    ll = crf.log_likelihood(X, y, circular=flags)
    state = lambda a, l: 3.0 * a + l
    trans = lambda i, j: 12.0 + 3 * i + j
    ring0 = state(0, 0) + trans(0, 2) + state(1, 2) + state(2, 2) + trans(2, 1) + state(3, 1) + trans(1, 0)
    ring1 = state(1, 1) + trans(1, 1)
    ring3 = state(0, 2) + state(3, 2) + trans(2, 2) + state(2, 2) + trans(2, 2)
    chain4 = state(2, 0)
    assert ll.tolist() == [ring0 - 10.0, ring1 - 11.0, 0.0, ring3 - 13.0, chain4 - 2.0]
    assert [c[0] for c in crf._model.calls] == ["marginals_full", "ring"]
    # sets: log Z_A,ring - log Z_ring through the same entry with masks
    crf._model.calls.clear()
    ll = crf.log_likelihood(X[:2], [[None, {"x", "y"}, "z"], ["x"]], circular=True)
    assert ll.tolist() == [0.0, 0.0]
    assert crf._model.calls == [("ring", [3, 1], None, False, False), ("ring", [3, 1], [7, 3, 4, 1], False, False)]
    with pytest.raises(ValueError, match="unknown label 'w'"):
        crf.log_likelihood(X[:2], [["x", "w", "z"], ["x"]], circular=True)
    with pytest.raises(ValueError, match="sequence 0: 3 items but 2 labels"):
        crf.log_likelihood(X[:2], [["x", "z"], ["x"]], circular=True)


# ---------------------------------------------------------------- the typed front end with a stubbed native call
def _typed(monkeypatch, ring_paths, chain_paths=None):
    """A typed classifier over labels (0, Alpha, Beta) whose native calls answer with the given paths (by contig length)."""
    from gecco_amd import _native, typed
    from gecco_amd.crfsuite_model import model_bytes

    An, L = 3, 3
    blob = model_bytes(["0", "Alpha", "Beta"], [f"d{k}" for k in range(An)], np.repeat(np.arange(An), L), np.tile(np.arange(L), An),
                       np.repeat(np.arange(L), L), np.tile(np.arange(L), L), np.zeros(An * L + L * L))
    crf = typed.TypedClusterCRF(5, 1)
    crf._set_blob(blob)
    calls = []

    def ring(self, cptr, gptr, attr, device=0, values=None, allowed=None, want_path=True, want_marginals=True):
        calls.append(("ring", np.diff(cptr).tolist(), want_marginals))
        labels = np.concatenate([ring_paths[T] for T in np.diff(cptr).tolist()]).astype(np.int8)
        out = {"lognorm": np.full(len(cptr) - 1, 5.0), "labels": labels, "score": np.full(len(cptr) - 1, 4.0)}
        if want_marginals:
            out["marginals"] = np.eye(L)[labels] * 0.75 + 0.25 * np.eye(L)[0][None, :]
        return out

    def viterbi_min_run(self, cptr, gptr, attr, set_mask, min_run, device=0, values=None, allowed=None, want_lognorm=True):
        calls.append(("viterbi_min_run", np.diff(cptr).tolist(), set_mask, min_run))
        labels = np.concatenate([chain_paths[T] for T in np.diff(cptr).tolist()]).astype(np.int8)
        nc = len(cptr) - 1
        return labels, np.full(nc, 1.0), np.full(nc, 2.0), np.full(nc, 3.0)

    def no_device(*args, **kwargs):
        raise AssertionError("the native call was reached")

    monkeypatch.setattr(_native.Model, "ring", ring)
    monkeypatch.setattr(_native.Model, "viterbi_min_run", viterbi_min_run)
    for name in ("marginals_min_run", "viterbi_run_length", "marginals_run_length", "viterbi", "marginals_full"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf, calls


def _contig(name, n):
    from gecco_amd import model

    src = model.Source(name)
    return [model.Gene(src, 1000 * i + 1, 1000 * i + 900, model.Strand.Coding,
                       model.Protein(f"{name}_{i + 1}", None, [model.Domain(f"d{i % 3}", 10, 90, "Pfam", 1e-20, 1e-12)])) for i in range(n)]


def test_a_cluster_across_the_cut_is_one_cluster(monkeypatch, tmp_path):
    from gecco_amd import typed

    ring8 = np.array([1, 1, 0, 0, 2, 2, 0, 1])     # runs: [0, 2), [4, 6), [7, 8) -- the first and the last are one across the cut
    chain5 = np.array([1, 0, 0, 0, 2])             # a chain keeps its two ends apart
    crf, calls = _typed(monkeypatch, {8: ring8}, {5: chain5})
    genes = _contig("ringA", 8) + _contig("lineB", 5)
    found = crf.predict_path_clusters(genes, min_run=1, circular=["ringA"], marginals=False)
    assert calls == [("viterbi_min_run", [5], 6, 1), ("ring", [8], False)]
    assert [c.id for c in found] == ["lineB_cluster_1", "lineB_cluster_2", "ringA_cluster_1", "ringA_cluster_2"]
    assert [c.wraps_origin for c in found] == [False, False, False, True]
    assert [[g.protein.id for g in c.genes] for c in found[2:]] == [["ringA_5", "ringA_6"], ["ringA_8", "ringA_1", "ringA_2"]]
    assert found[2].path_type == "Beta" and found[3].path_type == "Alpha"
    post = crf.path_posteriors_
    assert post["sequence_id"] == ["lineB", "ringA"] and post["clusters"] == [2, 2]
    assert post["log_z"] == [3.0, 5.0] and post["score"] == [1.0, 4.0] and post["log_p"] == [-2.0, -1.0]
    assert post["constraint_log_p"] == [-1.0, 0.0]
    path = os.path.join(str(tmp_path), "path_clusters.tsv")
    typed.write_path_clusters(path, found, wraps=True)
    rows = [line.rstrip("\n").split("\t") for line in open(path)]
    assert rows[0] == ["sequence_id", "cluster_id", "start", "end", "genes", "type", "wraps"]
    assert rows[3] == ["ringA", "ringA_cluster_1", "4001", "5900", "2", "Beta", "0"]
    assert rows[4] == ["ringA", "ringA_cluster_2", "7001", "1900", "3", "Alpha", "1"] and int(rows[4][2]) > int(rows[4][3])
    # with marginals the ring's inside comes from the ring marginals: 1 - P(background)
    calls.clear()
    found = crf.predict_path_clusters(_contig("ringA", 8), min_run=1, circular=True, marginals=True)
    assert calls == [("ring", [8], True)]
    assert crf.path_gene_probabilities_.tolist() == [0.75, 0.75, 0.0, 0.0, 0.75, 0.75, 0.0, 0.75]
    assert (found[1].average_p, found[1].max_p, found[1].min_p) == (0.75, 0.75, 0.75) and found[1].wraps_origin
    assert crf.path_genes_["path_label"] == ["Alpha", "Alpha", "0", "0", "Beta", "Beta", "0", "Alpha"]
    # without circular: the call of today, and no attribute
    calls.clear()
    crf2, calls2 = _typed(monkeypatch, {}, {8: ring8})
    found = crf2.predict_path_clusters(_contig("ringA", 8), min_run=1)
    assert [c[0] for c in calls2] == ["viterbi_min_run"] and len(found) == 3 and not any(hasattr(c, "wraps_origin") for c in found)
    typed.write_path_clusters(path, found)  # the table of a call without the argument, as it has always been written
    assert [line.rstrip("\n").split("\t") for line in open(path)] == [
        ["sequence_id", "cluster_id", "start", "end", "genes", "type"], ["ringA", "ringA_cluster_1", "1", "1900", "2", "Alpha"],
        ["ringA", "ringA_cluster_2", "4001", "5900", "2", "Beta"], ["ringA", "ringA_cluster_3", "7001", "7900", "1", "Alpha"]]
    assert [[g.protein.id for g in c.genes] for c in found] == [["ringA_1", "ringA_2"], ["ringA_5", "ringA_6"], ["ringA_8"]]
    assert crf2.path_posteriors_ == {"sequence_id": ["ringA"], "genes": [8], "log_z": [3.0], "score": [1.0], "log_p": [-2.0],
                                     "constraint_log_p": [-1.0], "clusters": [3]}
    found = crf2.predict_path_clusters(_contig("ringA", 8), min_run=1, circular=[])
    assert len(found) == 3 and not any(hasattr(c, "wraps_origin") for c in found)
    found = crf2.predict_path_clusters(_contig("ringA", 8), min_run=1, circular=["another"])
    assert len(found) == 3 and [c.wraps_origin for c in found] == [False] * 3
    # a single string is one sequence id, not its characters
    crf3, calls3 = _typed(monkeypatch, {8: ring8}, {1: np.array([1])})
    found = crf3.predict_path_clusters(_contig("ringA", 8) + _contig("A", 1), min_run=1, circular="ringA")
    assert calls3 == [("viterbi_min_run", [1], 6, 1), ("ring", [8], False)] and [c.wraps_origin for c in found] == [False, False, True]


def test_a_ring_that_is_inside_throughout_is_one_cluster(monkeypatch):
    crf, _ = _typed(monkeypatch, {4: np.array([1, 2, 2, 1]), 3: np.array([0, 0, 0]), 2: np.array([0, 2])})
    found = crf.predict_path_clusters(_contig("r4", 4) + _contig("r3", 3) + _contig("r2", 2), min_run=1, circular=True)
    assert [c.id for c in found] == ["r2_cluster_1", "r4_cluster_1"]
    assert [[g.protein.id for g in c.genes] for c in found] == [["r2_2"], ["r4_1", "r4_2", "r4_3", "r4_4"]]
    assert [c.wraps_origin for c in found] == [False, False]
    assert crf.path_posteriors_["clusters"] == [1, 0, 1]


def test_every_refusal_comes_before_any_device_call(monkeypatch):
    from gecco_amd import _native, typed

    crf, calls = _typed(monkeypatch, {}, {})
    genes = _contig("r", 4)
    message = "on a circular contig only min_run=1 is defined"
    for kwargs in (dict(circular=True), dict(circular=["r"]), dict(circular=True, min_run=3), dict(circular=True, min_run=2),
                   dict(circular=["r"], length_model=True), dict(circular=True, min_run=1, length_model=True)):
        with pytest.raises(ValueError, match=message):
            crf.predict_path_clusters(genes, **kwargs)
    with pytest.raises(ValueError, match="min_run = 0 is outside"):
        crf.predict_path_clusters(genes, min_run=0, circular=[])
    assert calls == []
    params = inspect.signature(typed.TypedClusterCRF.predict_path_clusters).parameters
    assert params["circular"].default is None and params["circular"].kind is inspect.Parameter.KEYWORD_ONLY
    base = ["predict", "--model", "m", "-f", "f", "-g", "g"]
    assert typed.build_parser().parse_args(base).circular is None
    assert typed.build_parser().parse_args(base + ["--path-clusters", "1", "--circular", "all"]).circular == "all"
    with pytest.raises(ValueError, match="--circular needs --path-clusters"):
        typed.main(base + ["--circular", "all"])
