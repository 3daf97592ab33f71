"""Sampled label paths, the parts that need no device: the numpy yardstick (tests/sampling_reference.py) against the Philox
known answers, path enumeration and a plain loop; the host refusals of ``gecco_crf_sample_paths``; the argument checks of
``SequenceCRF.sample`` / ``sample_runs`` and of the typed front end; the table columns."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest

from tests import constrained_reference as cr
from tests import sampling_reference as sr
from tests import train_objective_partial as tp
from tests.train_objective_valued import lse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- Philox4x32-10
@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{int(v):08x}" for v in sr.philox4x32_10(counter, key)) == want


def test_uniforms_follow_the_counter_layout():
    u = sr.uniforms(0, 0, 0, 0)
    assert float(u) == ((0x6627E8D5 << 21) ^ (0xE169C58D >> 11)) * 2.0 ** -53
    seed = (0x299F31D0 << 32) | 0xA4093822
    x = sr.philox4x32_10([5, 7, 11, 0], [0xA4093822, 0x299F31D0])
    assert float(sr.uniforms(seed, 5, 7, 11)) == ((int(x[0]) << 21) ^ (int(x[1]) >> 11)) * 2.0 ** -53
    grid = sr.uniforms(seed, np.arange(4)[:, None], np.arange(3)[None, :], 2)
    assert grid.shape == (4, 3) and grid[2, 1] == float(sr.uniforms(seed, 2, 1, 2))
    many = sr.uniforms(9, np.arange(100000), 0, 0)
    assert many.min() >= 0.0 and many.max() < 1.0 and abs(many.mean() - 0.5) < 6.0 / np.sqrt(12 * 100000)


# ---------------------------------------------------------------- the sampler against path enumeration
def _path_probabilities(score, T):
    n, L = score.shape
    paths = list(itertools.product(range(L), repeat=n))
    with np.errstate(invalid="ignore"):
        s = np.array([score[0, p[0]] + sum(T[p[t - 1], p[t]] + score[t, p[t]] for t in range(1, n)) for p in paths])
    return paths, np.exp(s - lse(s, 0))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n,L", [(1, 2), (2, 3), (3, 2), (4, 3), (5, 3), (5, 2)])
def test_the_reference_sampler_draws_from_the_path_distribution(n, L, masked):
    rng = np.random.default_rng(100 * n + 10 * L + masked)
    A, N = 6, 4096
    S, T = rng.normal(0.0, 1.0, size=(A, L)), rng.normal(0.0, 1.5, size=(L, L))
    lengths = [n, 0, n]
    seq_ptr = np.concatenate([[0], np.cumsum(lengths)])
    deg = rng.integers(0, 4, size=2 * n)
    item_ptr = np.concatenate([[0], np.cumsum(deg)])
    attr = rng.integers(0, A, size=int(item_ptr[-1]))
    allowed = tp.full_masks(2 * n, L)
    if masked:
        allowed = rng.integers(1, 1 << L, size=2 * n).astype(np.uint32)
    score = cr.masked_scores(item_ptr, attr, None, S, allowed)
    y = sr.sample(seq_ptr, score, T, N, seed=77 + n)
    assert y.shape == (2 * n, N) and y.dtype == np.int8
    worst = 0.0
    for k in (0, 2):
        b, e = int(seq_ptr[k]), int(seq_ptr[k + 1])
        paths, prob = _path_probabilities(score[b:e], T)
        logz, marg, _, _ = cr.enumerate_paths(score[b:e], T)
        assert abs(prob.sum() - 1.0) < 1e-12
        index = {p: i for i, p in enumerate(paths)}
        counts = np.zeros(len(paths))
        for row in y[b:e].T.tolist():
            counts[index[tuple(row)]] += 1
        bound = 6.0 * np.sqrt(prob * (1.0 - prob) / N) + 2.0 / N
        assert np.all(np.abs(counts / N - prob) <= bound)
        assert np.all(counts[prob == 0.0] == 0), "a path through a disallowed pair was drawn"
        worst = max(worst, float((np.abs(counts / N - prob) / bound).max()))
        # the teacher-forced checker accepts the reference's own paths without an excuse
    excused, near, draws = sr.check_teacher_forced(y, seq_ptr, score, T, seed=77 + n)
    assert excused == 0 and draws == 2 * n * N and near <= 4
    print(f"n={n} L={L} masked={masked}: worst |frequency - p| / bound = {worst:.3g}")
    if n > 1 and not masked:  # another seed gives other paths, and the checker refuses them under this one (masks may leave one path)
        other = sr.sample(seq_ptr, score, T, N, seed=78 + n)
        assert other.tobytes() != y.tobytes()
        with pytest.raises(AssertionError, match="the reference draws"):
            sr.check_teacher_forced(other, seq_ptr, score, T, seed=77 + n)


def test_sample_s_does_not_depend_on_the_number_of_samples():
    rng = np.random.default_rng(4)
    S, T = rng.normal(size=(5, 3)), rng.normal(size=(3, 3))
    score = cr.masked_scores(np.arange(10), rng.integers(0, 5, size=9), None, S, tp.full_masks(9, 3))
    few, many = sr.sample([0, 4, 9], score, T, 7, 3), sr.sample([0, 4, 9], score, T, 50, 3)
    assert few.tobytes() == many[:, :7].tobytes()


def test_zero_weights_are_never_drawn():
    """A transition of weight -2000 has exp() = 0 against any other: the pair never occurs."""
    rng = np.random.default_rng(6)
    L = 3
    S, T = rng.normal(size=(4, L)), rng.normal(size=(L, L))
    T[1, 2] = -2000.0
    score = cr.masked_scores(np.arange(41), rng.integers(0, 4, size=40), None, S, tp.full_masks(40, L))
    y = sr.sample([0, 40], score, T, 512, 1)
    assert not np.any((y[:-1] == 1) & (y[1:] == 2)) and np.any(y == 1) and np.any(y == 2)


# ---------------------------------------------------------------- the run extents against a plain loop
def test_run_extents_against_a_plain_loop():
    rng = np.random.default_rng(8)
    L, N = 4, 37
    seq_ptr = np.array([3, 4, 4, 12, 30])  # (a base offset: y's rows start at the batch's first item)
    y = rng.integers(0, L, size=(27, N)).astype(np.int8)
    y[9:20, :5] = 1  # (long runs, up to a sequence's ends)
    y[1:9, 5] = 2
    queries = [(0, 0, 0b0010), (2, 0, 0b0110), (2, 7, 0b0100), (3, 0, 0b0010), (3, 17, 0b1111), (3, 9, 0b0011), (2, 3, 0b1000),
               (3, 5, 0b0010)]
    contig, anchor, mask = (np.array([q[k] for q in queries]) for k in range(3))
    got = sr.run_extents(y, seq_ptr, contig, anchor, mask)
    assert got.shape == (len(queries), N, 2) and got.dtype == np.int32
    for q, (c, a, m) in enumerate(queries):
        b, e = seq_ptr[c] - seq_ptr[0], seq_ptr[c + 1] - seq_ptr[0]
        for s in range(N):
            col = y[b:e, s]
            if not (m >> col[a]) & 1:
                want = (-1, -1)
            else:
                first = a
                while first > 0 and (m >> col[first - 1]) & 1:
                    first -= 1
                last = a
                while last + 1 < len(col) and (m >> col[last + 1]) & 1:
                    last += 1
                want = (first, last + 1)
            assert tuple(got[q, s]) == want, (q, s)
    assert np.all(got[4] == [0, 18]) and np.any(got[:, :, 0] == -1) and np.all(got[3, :5] == [0, 11])


# ---------------------------------------------------------------- the entry's host refusals
L3 = 3


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    return _native


@pytest.fixture(scope="module")
def model3(nat):
    rng = np.random.default_rng(5)
    return nat.Model.from_tables(rng.normal(size=(7, L3)), rng.normal(size=(L3, L3)))


def _call(nat, model, **change):
    """A valid batch of two contigs (2 and 3 genes) and two runs on a device that does not exist, with `change` applied."""
    a = {"contig_ptr": np.array([0, 2, 5], dtype=np.int32), "n_contigs": 2, "gene_ptr": np.arange(0, 12, 2, dtype=np.int32),
         "attr_id": (np.arange(10, dtype=np.int32) * 3) % 7, "attr_value": None, "allowed": None, "n_samples": 8, "seed": 1,
         "run_contig": np.array([0, 1], dtype=np.int32), "run_anchor": np.array([1, 2], dtype=np.int32),
         "run_mask": np.array([6, 1], dtype=np.uint32), "n_runs": 2, "y": np.zeros(5 * 8, dtype=np.int8),
         "runs": np.zeros(2 * 8 * 2, dtype=np.int32), "marg": np.zeros(5 * L3), "lognorm": np.zeros(2)}
    a.update(change)
    fn = nat.load_library().gecco_crf_sample_paths
    names = ("contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "n_samples", "seed", "run_contig", "run_anchor",
             "run_mask", "n_runs", "y", "runs", "marg", "lognorm")
    args = [a[n].ctypes.data_as(t) if isinstance(a[n], np.ndarray) else a[n] for n, t in zip(names, fn.argtypes[2:])]
    rc = fn(model._h, 99, *args)
    return rc, nat.load_library().gecco_crf_last_error().decode()


def _i32(*v):
    return np.array(v, dtype=np.int32)


def test_host_refusals_come_before_the_device(nat, model3):
    call = lambda **kw: _call(nat, model3, **kw)
    # a valid call gets past the host checks: what stops it is the device that does not exist
    assert call()[0] not in (nat.OK, nat.EINVAL)
    assert call(y=None)[0] not in (nat.OK, nat.EINVAL)
    assert call(n_runs=0, run_contig=None, run_anchor=None, run_mask=None, runs=None)[0] not in (nat.OK, nat.EINVAL)
    for bad in (0, -1, (1 << 20) + 1):
        assert call(n_samples=bad) == (nat.EINVAL, f"sample_paths: n_samples = {bad} is outside 1 .. 1048576")
    assert call(n_samples=1 << 20, y=None, runs=None, n_runs=0)[0] not in (nat.OK, nat.EINVAL)
    assert call(n_runs=-1) == (nat.EINVAL, "sample_paths: negative n_runs")
    assert call(runs=None) == (nat.EINVAL, "null buffer")
    assert call(run_contig=_i32(0, 2)) == (nat.EINVAL, "run 1: contig 2 out of range (the batch has 2)")
    assert call(run_contig=_i32(-1, 1)) == (nat.EINVAL, "run 0: contig -1 out of range (the batch has 2)")
    assert call(run_anchor=_i32(2, 2)) == (nat.EINVAL, "run 0: anchor 2 lies outside contig 0 of 2 genes")
    assert call(run_anchor=_i32(1, -1)) == (nat.EINVAL, "run 1: anchor -1 lies outside contig 1 of 3 genes")
    assert call(run_mask=np.array([6, 0], dtype=np.uint32)) == (nat.EINVAL, "run 1: the label set is empty (a mask of 0)")
    assert call(run_mask=np.array([9, 1], dtype=np.uint32)) == \
        (nat.EINVAL, "run 0: the set holds a label at or above num_labels = 3 (mask 9)")
    rc, msg = call(run_mask=np.array([6, 1 << 31], dtype=np.uint32))
    assert rc == nat.EINVAL and msg.startswith("run 1: the set holds a label at or above num_labels = 3")
    # a contig without genes holds no anchor
    rc, msg = call(contig_ptr=_i32(0, 5, 5), run_contig=_i32(0, 1), run_anchor=_i32(1, 0))
    assert (rc, msg) == (nat.EINVAL, "run 1: anchor 0 lies outside contig 1 of 0 genes")
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
    logz = np.full(3, 7.0)
    rc, msg = _call(nat, model3, contig_ptr=np.zeros(4, dtype=np.int32), n_contigs=3, n_runs=0, run_contig=None, run_anchor=None,
                    run_mask=None, runs=None, lognorm=logz)
    assert rc != nat.EINVAL, msg  # (ENODEV from the device that does not exist, or OK: never a complaint about an argument)


def test_the_native_wrapper_checks_its_arrays(nat, model3, monkeypatch):
    cptr, gptr, attr = _i32(0, 2, 5), np.arange(0, 12, 2, dtype=np.int32), (np.arange(10, dtype=np.int32) * 3) % 7
    with pytest.raises(ValueError, match="seed"):
        model3.sample_paths(cptr, gptr, attr, 4, seed=-1)
    with pytest.raises(ValueError, match="seed"):
        model3.sample_paths(cptr, gptr, attr, 4, seed=1 << 64)
    with pytest.raises(ValueError, match="values holds 3 entries"):
        model3.sample_paths(cptr, gptr, attr, 4, values=np.ones(3))
    with pytest.raises(ValueError, match="allowed holds 2 masks for 5 genes"):
        model3.sample_paths(cptr, gptr, attr, 4, allowed=[1, 1])
    with pytest.raises(ValueError, match="differ in length"):
        model3.sample_paths(cptr, gptr, attr, 4, runs=([0, 1], [0], [1, 1]))
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(ValueError, match=f"n_samples = {bad} is outside"):
            model3.sample_paths(cptr, gptr, attr, bad)
    with pytest.raises(ValueError, match="run 0: anchor 2 lies outside contig 0 of 2 genes"):
        model3.sample_paths(cptr, gptr, attr, 4, runs=([0], [2], [1]))


def test_the_header_declares_the_entry_and_the_library_exports_it(nat):
    header = open(os.path.join(ROOT, "include", "gecco_crf.h")).read()
    assert "ABI 2.17.0" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+gecco_crf_sample_paths\s*\(([^;]*)\)\s*;", code)
    assert m, "gecco_crf_sample_paths is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "m", "device", "contig_ptr", "n_contigs", "gene_ptr", "attr_id", "attr_value", "allowed", "n_samples", "seed", "run_contig",
        "run_anchor", "run_mask", "n_runs", "y", "runs", "marg", "lognorm"]
    lib = nat.load_library()
    assert hasattr(lib, "gecco_crf_sample_paths")
    assert len(nat.SIGNATURES["gecco_crf_sample_paths"][1]) == len(params)
    assert lib.gecco_crf_version() == 340
    sig = inspect.signature(nat.Model.sample_paths)
    assert list(sig.parameters)[:11] == ["self", "contig_ptr", "gene_ptr", "attr_id", "n_samples", "seed", "device", "values", "allowed",
                                         "runs", "want_marginals"]
    assert sig.parameters["seed"].default == 0 and sig.parameters["want_marginals"].default is False


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

    for name in ("sample_paths", "span_log_probabilities", "marginals_full", "viterbi", "windowed_marginals", "windowed_marginals_all"):
        monkeypatch.setattr(_native.Model, name, no_device)
    return crf


X = [[["a0"], ["a1", "a2"], ["a3"]], [], [["a0", "a3"]]]


@pytest.mark.parametrize("anchor,words", [
    ((0, 0, "w"), "unknown label 'w'"),
    ((0, 0, {"x", "nope"}), "unknown label 'nope'"),
    ((0, 0, set()), "empty set"),
    ((0, 0, []), "empty set"),
    ((3, 0, "x"), "sequence index 3 out of range"),
    ((-1, 0, "x"), "sequence index -1 out of range"),
    ((0, 3, "x"), "item 3 lies outside sequence 0 of 3 items"),
    ((0, -1, "x"), "item -1 lies outside sequence 0 of 3 items"),
    ((1, 0, "x"), "item 0 lies outside sequence 1 of 0 items"),
    ((0, 0.5, "x"), "expected (sequence_index, item, labels)"),
    ((0, 0), "expected (sequence_index, item, labels)"),
])
def test_bad_anchors_are_refused_before_any_device_call(crf, anchor, words):
    with pytest.raises(ValueError) as err:
        crf.sample_runs(X, [(0, 2, {"x", "y"}), anchor], 16)
    assert "anchor 1" in str(err.value) and words in str(err.value), str(err.value)


@pytest.mark.parametrize("method", ["sample", "sample_runs"])
def test_bad_counts_seeds_and_sets_are_refused_before_any_device_call(crf, method):
    call = (lambda *a, **kw: crf.sample(X, *a, **kw)) if method == "sample" else (lambda *a, **kw: crf.sample_runs(X, [(0, 0, "x")], *a, **kw))
    for bad in (0, -3, (1 << 20) + 1):
        with pytest.raises(ValueError, match=f"n_samples = {bad} is outside"):
            call(bad)
    with pytest.raises(ValueError, match="integers"):
        call(2.5)
    with pytest.raises(ValueError, match="seed -1 is outside"):
        call(4, seed=-1)
    with pytest.raises(ValueError, match="is outside 0 .. 2"):
        call(4, seed=1 << 64)
    with pytest.raises(ValueError, match="unknown label"):
        call(4, allowed=[["x", "q", None], [], [None]])
    with pytest.raises(ValueError, match="items but"):
        call(4, allowed=[["x", None], [], [None]])


def test_nothing_to_draw_needs_no_device(crf):
    out = crf.sample([[], []], 5)
    assert [o.shape for o in out] == [(5, 0), (5, 0)] and all(o.dtype == np.int8 for o in out)
    assert crf.sample([], 3) == []
    runs = crf.sample_runs(X, [], 9)
    assert runs.shape == (0, 9, 2) and runs.dtype == np.int32


def test_an_unfitted_model_is_refused():
    from gecco_amd.sequence import SequenceCRF

    with pytest.raises(ValueError, match="not fitted"):
        SequenceCRF(window_size=None).sample(X, 4)
    with pytest.raises(ValueError, match="not fitted"):
        SequenceCRF(window_size=None).sample_runs(X, [(0, 0, "x")], 4)


# ---------------------------------------------------------------- the typed front end
def test_the_typed_front_end_takes_the_arguments():
    from gecco_amd import typed

    for name in ("predict_clusters", "predict_genes_and_clusters"):
        params = inspect.signature(getattr(typed.TypedClusterCRF, name)).parameters
        assert params["boundary_samples"].default == 0 and params["seed"].default == 0
    base = ["predict", "--model", "m", "-f", "f", "-g", "g"]
    args = typed.build_parser().parse_args(base)
    assert args.boundary_samples == 0 and args.seed == 0
    args = typed.build_parser().parse_args(base + ["--boundary-samples", "512", "--seed", "9"])
    assert args.boundary_samples == 512 and args.seed == 9


def test_the_typed_front_end_checks_the_arguments_first():
    """Before the model is looked at: an unfitted one never gets to say so."""
    from gecco_amd import typed

    crf = typed.TypedClusterCRF()
    for kw, words in ((dict(boundary_samples=-1), "boundary_samples = -1 is outside"),
                      (dict(boundary_samples=(1 << 20) + 1), "is outside 0 .. 1048576"),
                      (dict(boundary_samples=1.5), "integers"), (dict(boundary_samples=4, seed=-2), "seed -2 is outside"),
                      (dict(boundary_samples=4, seed=1 << 64), "is outside 0 .. 2")):
        for method in (crf.predict_clusters, crf.predict_genes_and_clusters):
            with pytest.raises(ValueError, match=words):
                method([], **kw)
    with pytest.raises(ValueError, match="not fitted"):
        crf.predict_clusters([], boundary_samples=4)


def test_typed_cluster_table_with_and_without_the_columns(tmp_path):
    from gecco_amd import model, tables, typed
    from gecco_amd.types import ClusterType

    def cluster(name, first):
        genes = [model.Gene(model.Source("s"), first + 10 * k, first + 10 * k + 5, model.Strand.Coding, model.Protein(f"{name}{k}", None),
                            _probability=0.9) for k in range(3)]
        return model.Cluster(f"s_cluster_{name}", genes, ClusterType("B"), {"B": 0.75, "a": 0.125})

    one, two = cluster("1", 100), cluster("2", 500)
    new = ["anchor_p", "exact_p", "start_lo", "start_hi", "end_lo", "end_hi"]
    plain = typed.typed_cluster_table([one, two], ["B", "a"])
    assert not any(col in plain.columns for col in new)
    plain.dump(str(tmp_path / "plain.tsv"))
    before = open(str(tmp_path / "plain.tsv"), "rb").read()
    one.anchor_probability, one.exact_probability = 0.75, 0.5
    one.start_interval, one.end_interval = (90, 110), (125, 160)
    table = typed.typed_cluster_table([one, two], ["B", "a"])
    path = str(tmp_path / "clusters.tsv")
    table.dump(path)
    header = open(path).readline().rstrip("\n").split("\t")
    at = header.index("b_probability")
    assert header[at + 1:at + 7] == new and header[at + 7] == "proteins"
    back = tables.ClusterTable.load(path)
    assert [float(v) for v in back.anchor_p][0] == 0.75 and np.isnan(float(back.anchor_p[1]))
    assert float(back.exact_p[0]) == 0.5 and np.isnan(float(back.exact_p[1]))
    # (a cluster of the list without intervals: its own start and end)
    assert [[int(v) for v in getattr(back, col)] for col in new[2:]] == [[90, 500], [110, 500], [125, 525], [160, 525]]
    # behind the region columns when both are there
    one.region_probability, one.region_type_probabilities = 0.25, {"B": 0.2, "a": 0.1}
    header = typed.typed_cluster_table([one, two], ["B", "a"]).COLUMNS
    names = [n for n, _, _ in header]
    assert names[names.index("b_probability") + 1:names.index("proteins")] == ["region_p", "a_region_p", "b_region_p"] + new
    # clusters without the attributes: the table of before, byte for byte
    typed.typed_cluster_table([cluster("1", 100), cluster("2", 500)], ["B", "a"]).dump(str(tmp_path / "again.tsv"))
    assert open(str(tmp_path / "again.tsv"), "rb").read() == before
