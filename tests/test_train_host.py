"""Host side of training, no GPU needed: the CRFsuite model writer, feature generation and the reference's input
checks, the L-BFGS / OWL-QN optimiser, and pickling a fitted object as GECCO's own record."""
import io
import os
import pickle
import sys
import types
import warnings

import numpy as np
import pytest

from tests.helpers import GOLDEN


# ---------------------------------------------------------------- writer
def test_writer_reproduces_the_shipped_model_byte_for_byte():
    from oracle import lcrf
    from gecco_amd import crfsuite_model, pickle_model

    blob = pickle_model.crfsuite_blob(pickle_model.load_model_dir(GOLDEN))
    assert len(blob) == 222468
    m = lcrf.parse_lcrf(blob)
    f = m["feats"]
    assert crfsuite_model.lcrf_bytes(m["labels"], m["attrs"], f["type"], f["src"], f["dst"], f["w"]) == blob
    s = f["type"] == 0
    assert crfsuite_model.model_bytes(m["labels"], m["attrs"], f["src"][s], f["dst"][s], f["src"][~s], f["dst"][~s],
                                      f["w"]) == blob


def test_cqdb_hash_is_lookup3():
    from gecco_amd.crfsuite_model import hashlittle

    # lookup3.c's own driver values: hashlittle("", 0) and "Four score and seven years ago" with seeds 0 and 1
    assert hashlittle(b"", 0) == 0xDEADBEEF
    assert hashlittle(b"Four score and seven years ago", 0) == 0x17770551
    assert hashlittle(b"Four score and seven years ago", 1) == 0xCD628161


def test_new_weights_parse_back_through_both_readers():
    from oracle import lcrf
    from gecco_amd import _native, crfsuite_model

    rng = np.random.default_rng(2)
    attrs = [f"PF{k:05d}" for k in range(40)] + ["domé"]
    A = len(attrs)
    sa = np.repeat(np.arange(A), 2)
    sl = np.tile([0, 1], A)
    w = rng.normal(size=2 * A + 4)
    w[:2 * A][rng.random(2 * A) < 0.3] = 0.0  # pruned on save
    w[3] = w[4] = 0.0                 # attribute 1 and 2 partly pruned
    w[6] = w[7] = 0.0                 # attribute 3 loses every feature: dropped
    w[2 * A + 1] = 0.0                # one transition pruned
    blob = crfsuite_model.model_bytes(["0", "1"], attrs, sa, sl, [0, 0, 1, 1], [0, 1, 0, 1], w)
    m = lcrf.parse_lcrf(blob)
    ws = w[:2 * A].reshape(A, 2)
    kept = [a for a in range(A) if (ws[a] != 0).any()]
    assert m["attrs"] == [attrs[a] for a in kept] and m["labels"] == ["0", "1"]
    np.testing.assert_array_equal(m["state"], ws[kept])
    np.testing.assert_array_equal(m["state_mask"], ws[kept] != 0)
    np.testing.assert_array_equal(m["trans"], w[2 * A:].reshape(2, 2))
    np.testing.assert_array_equal(m["trans_mask"], w[2 * A:].reshape(2, 2) != 0)
    assert m["header"][4] == 0 and m["n_feat"] == int((w != 0).sum())
    nat = _native.Model.from_lcrf(blob)
    assert nat.attrs() == m["attrs"] and nat.labels() == m["labels"]
    sw, sp = nat.state_weights()
    np.testing.assert_array_equal(sw, m["state"])
    np.testing.assert_array_equal(sp, m["state_mask"])
    tw, tp = nat.trans_weights()
    np.testing.assert_array_equal(tw, m["trans"])
    assert nat.attr_id("domé") == len(kept) - 1


# ---------------------------------------------------------------- feature generation
def test_ids_in_first_appearance_order_and_observed_features_only():
    from gecco_amd.train import build_training_set

    seqs = [[["b", "a"], [], ["c"]], [["a"], ["d"], ["d", "b"]]]
    labs = [["1", "1", "0"], ["1", "0", "0"]]
    ts = build_training_set(seqs, labs, window=2, step=1)
    assert ts.attrs_ == ["b", "a", "c", "d"] and ts.labels_ == ["1", "0"]
    # observed (attr, label) pairs, sorted by (attr id, label id)
    assert list(zip(ts.state_attr.tolist(), ts.state_label.tolist())) == [(0, 0), (0, 1), (1, 0), (2, 1), (3, 1)]
    # bigrams inside windows: 1->1, 1->0, 0->0
    assert list(zip(ts.trans_src.tolist(), ts.trans_dst.tolist())) == [(0, 0), (0, 1), (1, 1)]
    assert ts.state_fid.tolist() == [[0, 1], [2, -1], [-1, 3], [-1, 4]]
    assert ts.trans_fid.tolist() == [[5, 6], [-1, 7]]
    assert ts.seq_ptr.tolist() == [0, 3, 6] and ts.labels.tolist() == [0, 0, 1, 0, 1, 1]


def test_uncovered_items_are_not_seen():
    from gecco_amd.train import build_training_set

    # window 2, step 2 over 3 items: the last item is in no window (gecco/_meta.py sliding_window)
    ts = build_training_set([[["a"], ["b"], ["z"]]], [["0", "1", "1"]], window=2, step=2)
    assert ts.attrs_ == ["a", "b"]
    assert ts.item_ptr.tolist() == [0, 1, 2, 2]


def test_all_possible_and_min_freq():
    from gecco_amd.train import build_training_set

    seqs = [[["a"], ["b"], ["a"], ["c"]]]
    labs = [["0", "0", "1", "1"]]
    full = build_training_set(seqs, labs, 4, 1, all_possible_states=True, all_possible_transitions=True)
    assert len(full.state_attr) == 6 and len(full.trans_src) == 4
    # frequencies with window 2 step 1: a/0 in 1 window, b/0 in 2, a/1 in 2, c/1 in 1; 0->0, 0->1, 1->1 once each
    ts = build_training_set(seqs, labs, 2, 1, min_freq=2)
    names = [(ts.attrs_[a], ts.labels_[y]) for a, y in zip(ts.state_attr, ts.state_label)]
    assert names == [("a", "1"), ("b", "0")] and len(ts.trans_src) == 0
    assert ts.state_fid[ts.attrs_.index("a")].tolist() == [-1, 0]


def test_exactly_two_labels_are_required():
    from gecco_amd.train import build_training_set

    with pytest.raises(ValueError, match="exactly 2 labels"):
        build_training_set([[["a"], ["b"]]], [["0", "0"]], 2, 1)


def test_trainer_options():
    from gecco_amd.train import trainer_params

    p = trainer_params({"algorithm": "lbfgs", "c1": 0.4, "c2": None, "num_memories": 3, "verbose": False})
    assert p["c1"] == 0.4 and p["c2"] == 1.0 and p["num_memories"] == 3 and p["epsilon"] == 1e-5 and p["period"] == 10
    with pytest.raises(ValueError, match="'l2sgd'"):
        trainer_params({"algorithm": "l2sgd"})
    with pytest.raises(ValueError, match="'linesearch'"):
        trainer_params({"linesearch": "StrongBacktracking"})


def _gene(seq, start, names, p):
    from gecco_amd.model import Domain, Gene, Protein, Source, Strand

    doms = [Domain(n, 10 * j, 10 * j + 5, "Pfam", 1e-5, 1e-6, probability=p) for j, n in enumerate(names)]
    return Gene(Source(seq), start, start + 100, Strand.Coding, Protein(f"{seq}_{start}", None, doms), _probability=p)


def test_training_instances_follow_the_reference():
    from gecco_amd.crf import ClusterCRF

    genes = [_gene("s2", 300, ["x"], 0.9), _gene("s1", 200, ["b", "a"], 0.2), _gene("s1", 100, ["a"], 0.7),
             _gene("s2", 100, [], 0.1), _gene("s1", 300, [], 0.6)]
    crf = ClusterCRF("protein", window_size=2)
    feats, labels = crf.training_instances(genes, shuffle=False)
    assert feats == [[["a"], ["b", "a"], []], [[], ["x"]]]  # genes by start, domains by start
    assert labels == [["1", "0", "1"], ["0", "1"]]
    with pytest.warns(UserWarning, match="only negative labels found in sequence 's3'"):
        crf.training_instances([_gene("s3", 1, ["a"], 0.1), _gene("s3", 2, ["a"], 0.2)], shuffle=False)
    with pytest.warns(UserWarning, match="only positive labels found in sequence 's3'"):
        crf.training_instances([_gene("s3", 1, ["a"], 0.6), _gene("s3", 2, ["a"], 0.7)], shuffle=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=r"^'s4' has not enough observations \(1\) for requested window size \(2\)$"):
            crf.training_instances([_gene("s4", 1, ["a"], 0.6)], shuffle=False)
    dom = ClusterCRF("domain", window_size=2)
    feats, labels = dom.training_instances([_gene("s1", 1, ["a", "b"], 0.9), _gene("s1", 2, [], 0.2)], shuffle=False)
    assert feats == [[["a"], ["b"], []]] and labels == [["1", "1", "0"]]


def test_fit_refuses_unknown_options_before_training(monkeypatch):
    from gecco_amd.crf import ClusterCRF

    monkeypatch.setenv("GECCO_AMD_FIT", "native")
    with pytest.raises(ValueError, match="'pa_type'"):
        ClusterCRF("protein", window_size=2, pa_type=1).fit([])


# ---------------------------------------------------------------- optimiser
def _logreg(seed=0, n=300, d=12):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    y = (X @ rng.normal(size=d) + rng.normal(size=n) > 0).astype(float)

    def fg(w, c2):
        z = X @ w
        f = float(np.sum(np.logaddexp(0, z) - y * z)) + c2 * float(w @ w)
        return f, X.T @ (1 / (1 + np.exp(-z)) - y) + 2 * c2 * w

    return fg, d


@pytest.mark.parametrize("c1,c2", [(0.0, 0.1), (15.0, 0.1), (40.0, 0.5)])
def test_lbfgs_owlqn_match_scipy(c1, c2):
    import scipy.optimize
    from gecco_amd.train import minimize

    fg, d = _logreg()
    res = minimize(lambda w: fg(w, c2), np.zeros(d), c1=c1, epsilon=1e-12, delta=0.0)

    def split(u):
        f, g = fg(u[:d] - u[d:], c2)
        return f + c1 * u.sum(), np.concatenate([g + c1, -g + c1])

    ref = scipy.optimize.minimize(split, np.zeros(2 * d), jac=True, method="L-BFGS-B", bounds=[(0, None)] * (2 * d),
                                  options={"ftol": 1e-16, "gtol": 1e-13, "maxiter": 20000})
    assert np.abs(res.x - (ref.x[:d] - ref.x[d:])).max() <= 1e-6
    if c1 > 0:
        assert (res.x == 0).any()


def test_owlqn_kkt_without_l2():
    from gecco_amd.train import minimize

    fg, d = _logreg(3)
    c1 = 3.0
    res = minimize(lambda w: fg(w, 0.0), np.zeros(d), c1=c1, epsilon=1e-12, delta=0.0)
    _, g = fg(res.x, 0.0)
    nz = res.x != 0
    assert nz.any() and (~nz).any()
    assert np.abs(g[nz] + c1 * np.sign(res.x[nz])).max() <= 1e-6
    assert np.abs(g[~nz]).max() <= c1 + 1e-9


def test_stopping_rules():
    from gecco_amd.train import minimize

    fg, d = _logreg(4)
    assert minimize(lambda w: fg(w, 0.1), np.zeros(d), max_iterations=3).n_iter == 3
    loose = minimize(lambda w: fg(w, 0.1), np.zeros(d))
    assert loose.status in ("converged", "delta test")
    _, g = fg(loose.x, 0.1)
    assert np.linalg.norm(g) <= 1e-5 * max(1.0, np.linalg.norm(loose.x)) or loose.status == "delta test"


# ---------------------------------------------------------------- pickling as GECCO's record
def _stub_modules(monkeypatch, pairs):
    """Importable stand-ins for the classes `pairs` = ((module, class name), ...) of GECCO's model pickle."""
    made = {}
    for mod, name in pairs:
        parts = mod.split(".")
        for i in range(1, len(parts) + 1):
            sub = ".".join(parts[:i])
            if sub not in made:
                made[sub] = types.ModuleType(sub)
                monkeypatch.setitem(sys.modules, sub, made[sub])
                if i > 1:
                    setattr(made[".".join(parts[:i - 1])], parts[i - 1], made[sub])
        cls = type(name, (), {"__module__": mod, "__qualname__": name})
        setattr(made[mod], name, cls)
    return made


@pytest.fixture
def stub_reference_classes(monkeypatch):
    """GECCO with sklearn-crfsuite, which GECCO depends on."""
    return _stub_modules(monkeypatch, (("gecco.crf", "ClusterCRF"), ("sklearn_crfsuite.estimator", "CRF"),
                                       ("sklearn_crfsuite._fileresource", "FileResource")))


@pytest.fixture
def stub_gecco_without_crfsuite(monkeypatch):
    """GECCO importable, sklearn-crfsuite not (a None entry in sys.modules makes an import fail)."""
    for mod in ("sklearn_crfsuite", "sklearn_crfsuite.estimator", "sklearn_crfsuite._fileresource"):
        monkeypatch.setitem(sys.modules, mod, None)
    return _stub_modules(monkeypatch, (("gecco.crf", "ClusterCRF"),))


def test_plain_pickle_of_a_fitted_object_is_what_save_writes(tmp_path, stub_reference_classes):
    from gecco_amd import pickle_model
    from gecco_amd.crf import ClusterCRF

    blob = pickle_model.crfsuite_blob(pickle_model.load_model_dir(GOLDEN))
    crf = ClusterCRF("protein", window_size=20, c1=0.4, c2=0.0)
    crf._adopt_model_blob(blob)
    crf.save(tmp_path)
    buf = io.BytesIO()
    pickle.dump(crf, buf, protocol=4)  # what `gecco train` does (gecco/cli/commands/train.py)
    assert buf.getvalue() == (tmp_path / "model.pkl").read_bytes()
    loaded = ClusterCRF.trained(tmp_path)
    assert loaded.window_size == 20 and loaded.model.classes_ == ["0", "1"]
    assert len(loaded.model.state_features_) == 4211
    st = pickle_model.load_model_dir(tmp_path).state
    assert list(st) == ["feature_type", "window_size", "window_step", "algorithm", "significance", "significant_features",
                        "model", "_options"]
    shipped = pickle_model.load_model_dir(GOLDEN).state["model"].state
    crf_state = st["model"].state
    assert list(crf_state) == list(shipped)
    assert crf_state["c1"] == 0.4 and crf_state["c2"] == 0.0 and crf_state["training_log_"] is None
    assert pickle_model.crfsuite_blob(pickle_model.load_model_dir(tmp_path)) == blob


def test_plain_pickle_with_gecco_but_without_crfsuite_is_refused(tmp_path, stub_gecco_without_crfsuite):
    from gecco_amd import pickle_model
    from gecco_amd.crf import ClusterCRF

    blob = pickle_model.crfsuite_blob(pickle_model.load_model_dir(GOLDEN))
    crf = ClusterCRF("protein", window_size=20, c1=0.4, c2=0.0)
    crf._adopt_model_blob(blob)
    with pytest.raises(pickle.PicklingError, match=r"sklearn_crfsuite\.estimator\.CRF.*save\(\)"):
        pickle.dumps(crf, protocol=4)
    # save() still writes the record under its original class paths, and trained() reads it back
    crf.save(tmp_path)
    data = (tmp_path / "model.pkl").read_bytes()
    assert b"sklearn_crfsuite.estimator" in data and b"_RecordFactory" not in data
    loaded = ClusterCRF.trained(tmp_path)
    assert pickle_model.crfsuite_blob(loaded._record) == blob
    # a bare record whose class is not importable is not written under a helper's name by a plain pickler either
    with pytest.raises(pickle.PicklingError, match="dump_model_dir"):
        pickle.dumps(crf._record.state["model"], protocol=4)


def test_pickling_without_the_reference_classes_is_refused_clearly():
    from gecco_amd import pickle_model
    from gecco_amd.crf import ClusterCRF

    if "gecco" in sys.modules or pickle_model._original_class("gecco.crf", "ClusterCRF") is not None:
        pytest.skip("GECCO is importable here")
    crf = ClusterCRF("protein", window_size=20)
    crf._adopt_model_blob(pickle_model.crfsuite_blob(pickle_model.load_model_dir(GOLDEN)))
    with pytest.raises(pickle.PicklingError, match="save"):
        pickle.dumps(crf, protocol=4)


# ---------------------------------------------------------------- the yardstick of the device objective
def _mp_objective(seq_ptr, item_ptr, attr_id, labels, W, step, sfid, tfid, w):
    """f, g [K], per-window log Z of the training objective by enumerating all 2^W label paths of every window in
    50-digit arithmetic: no recursion, no scaling, no log-sum-exp."""
    import itertools

    import mpmath

    with mpmath.workdps(50):
        return _mp_objective_at_precision(mpmath, seq_ptr, item_ptr, attr_id, labels, W, step, sfid, tfid, w)


def _mp_objective_at_precision(mpmath, seq_ptr, item_ptr, attr_id, labels, W, step, sfid, tfid, w):
    import itertools

    K = len(w)
    wm = [mpmath.mpf(float(x)) for x in w]
    sfid, tfid = np.asarray(sfid).reshape(-1, 2), np.asarray(tfid).reshape(2, 2)
    n = int(seq_ptr[-1])
    item_feats = [[[int(sfid[a, y]) for a in attr_id[item_ptr[i]:item_ptr[i + 1]] if sfid[a, y] >= 0] for y in (0, 1)]
                  for i in range(n)]
    score = [[mpmath.fsum(wm[k] for k in item_feats[i][y]) for y in (0, 1)] for i in range(n)]
    tw = [[wm[tfid[i, j]] if tfid[i, j] >= 0 else mpmath.mpf(0) for j in (0, 1)] for i in (0, 1)]
    f = mpmath.mpf(0)
    g = [mpmath.mpf(0)] * K
    logzs = []
    paths = list(itertools.product((0, 1), repeat=W))
    for s in range(len(seq_ptr) - 1):
        for i0 in range(int(seq_ptr[s]), int(seq_ptr[s + 1]) - W + 1, step):
            sc = [mpmath.fsum([score[i0 + t][y[t]] for t in range(W)] + [tw[y[t - 1]][y[t]] for t in range(1, W)])
                  for y in paths]
            top = max(sc)
            ex = [mpmath.exp(v - top) for v in sc]
            z = mpmath.fsum(ex)
            logz = top + mpmath.log(z)
            logzs.append(logz)
            gold = [int(v) for v in labels[i0:i0 + W]]
            f += logz - sc[paths.index(tuple(gold))]
            for y, e in zip(paths, ex):  # expected - empirical counts, feature by feature
                p = e / z - (1 if list(y) == gold else 0)
                for t in range(W):
                    for k in item_feats[i0 + t][y[t]]:
                        g[k] += p
                    if t > 0 and tfid[y[t - 1], y[t]] >= 0:
                        g[tfid[y[t - 1], y[t]]] += p
    return f, g, logzs


@pytest.mark.parametrize("W,step", [(1, 1), (3, 2), (6, 1), (10, 3)])
@pytest.mark.parametrize("scale", [1.0, 100.0, 1000.0])
def test_numpy_objective_matches_path_enumeration(W, step, scale):
    """benchkit.train_objective (log space, vectorised recursions) against the definition of the objective summed over
    every label path, in 50-digit arithmetic, up to weights far beyond where any fp64 exp would overflow."""
    from benchkit.train_objective import objective
    from gecco_amd import synth
    from tests.helpers import objective_tolerances

    rng = np.random.default_rng(W * 100 + step)
    A = 6
    lengths = [W, W + 2 * step] if W >= 6 else [W, W + 1, W + 4]
    seq_ptr, item_ptr, attr_id, labels = synth.synth_training_set(rng, lengths, A, stay=0.7)
    fid = np.arange(2 * A + 4, dtype=np.int32)
    fid[[3, 2 * A + 1]] = -1  # a state and a transition pair without a feature
    keep = fid >= 0
    fid[keep] = np.arange(int(keep.sum()))
    sfid, tfid = fid[:2 * A], fid[2 * A:]
    w = scale * rng.normal(0, 1.5, size=int(keep.sum()))
    f, g, nw, d = objective(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, w, details=True)
    mf, mg, mlogz = _mp_objective(seq_ptr, item_ptr, attr_id, labels, W, step, sfid, tfid, w)
    assert nw == len(mlogz) > 0
    tol_f, tol_g = objective_tolerances(seq_ptr, item_ptr, attr_id, W, step, sfid, tfid, w, d)
    assert np.all(np.abs(d["logz"] - np.array([float(v) for v in mlogz])) <= tol_f)
    assert abs(f - float(mf)) <= tol_f / 2, (f, float(mf), tol_f)
    err = np.abs(g - np.array([float(v) for v in mg]))
    assert np.all(err <= tol_g / 2), (err / np.maximum(tol_g, 1e-300)).max()
    if scale <= 1:
        assert abs(f - float(mf)) <= 1e-12 * abs(float(mf)) and np.all(err <= 1e-9 * (1 + np.abs(g)))


# ---------------------------------------------------------------- the optimiser at non-finite points
class _OutOfBudget(Exception):
    pass


def _nan_beyond(limit=3.0, target=10.0, budget=500):
    """f = |x - target|^2 where every |x_i| <= limit, NaN (f and g) elsewhere; raises after `budget` calls."""
    calls = [0]

    def fg(x):
        calls[0] += 1
        if calls[0] > budget:
            raise _OutOfBudget(calls[0])
        if np.any(np.abs(x) > limit):
            return float("nan"), np.full_like(x, np.nan)
        return float(np.sum((x - target) ** 2)), 2 * (x - target)

    return fg, calls


@pytest.mark.parametrize("c1", [0.0, 0.5])
def test_minimize_never_accepts_a_non_finite_point(c1):
    from gecco_amd.train import minimize

    fg, calls = _nan_beyond()
    seen = []
    res = minimize(fg, np.zeros(3), c1=c1, max_iterations=None, callback=lambda k, f, x: seen.append((f, x.copy())))
    assert calls[0] <= 500
    assert np.all(np.isfinite(res.x)) and np.isfinite(res.f), res
    assert np.all(np.abs(res.x) <= 3.0)
    assert res.status in ("line search failed", "converged", "delta test"), res
    # every accepted iterate is finite, inside the finite region, and f decreases along them
    fs = [f for f, _ in seen]
    assert all(np.isfinite(f) for f in fs) and all(np.all(np.abs(x) <= 3.0) for _, x in seen)
    assert all(b <= a for a, b in zip(fs, fs[1:]))
    assert res.f < 300.0  # better than f(0)


@pytest.mark.parametrize("c1", [0.0, 0.5])
@pytest.mark.parametrize("bad", ["nan", "inf", "grad"])
def test_minimize_refuses_a_non_finite_start(c1, bad):
    from gecco_amd.train import minimize

    def fg(x):
        if bad == "grad":
            return 1.0, np.array([0.0, np.nan])
        return float(bad), np.zeros_like(x)

    with pytest.raises(ValueError, match="not finite at the start point"):
        minimize(fg, np.zeros(2), c1=c1)
