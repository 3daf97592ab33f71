"""Training on the device: gecco_crf_trainer_eval against an independent numpy log-space forward-backward, the fit
against scipy's optimum of the same numpy objective, and fit -> save -> trained -> predict_probabilities end to end."""
import os
import random
import warnings

import numpy as np
import pytest

from benchkit.train_objective import objective
from tests.helpers import GOLDEN, golden_csr, random_problem, read_tsv

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- independent numpy objective (log space)
def np_objective(seq_ptr, item_ptr, attr_id, labels, A, W, step, state_fid, trans_fid, w):
    f, g, _ = objective(seq_ptr, item_ptr, attr_id, labels, A, W, step, state_fid, trans_fid, w)
    return f, g


def check_eval(trainer, args, w, W, step):
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K = args
    f, g = trainer.eval(w)
    ef, eg = np_objective(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, w)
    assert abs(f - ef) <= 1e-12 * abs(ef), (f, ef)
    assert np.all(np.abs(g - eg) <= 1e-9 * (1 + np.abs(eg))), np.abs(g - eg).max()
    f2, g2 = trainer.eval(w)
    assert np.float64(f).tobytes() == np.float64(f2).tobytes() and g.tobytes() == g2.tobytes()


@pytest.mark.parametrize("W,step", [(1, 1), (2, 1), (5, 1), (5, 3), (20, 1), (20, 3), (32, 1), (32, 3)])
def test_eval_matches_numpy_forward_backward(W, step):
    from gecco_amd import _native

    rng = np.random.default_rng(1000 + 37 * W + step)
    seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K, w = random_problem(rng, W, step)
    tr = _native.Trainer(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, K)
    n_win = sum((int(seq_ptr[s + 1] - seq_ptr[s]) - W) // step + 1 for s in range(len(seq_ptr) - 1))
    assert tr.num_windows == n_win
    check_eval(tr, (seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K), w, W, step)
    check_eval(tr, (seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K), np.zeros(K), W, step)


def test_eval_on_bgc0001866_with_the_shipped_weights(oracle_model):
    from gecco_amd import _native

    ids, cptr, gptr, attr, _, _ = golden_csr(oracle_model["attr_index"])
    members = set()
    for row in read_tsv(os.path.join(GOLDEN, "BGC0001866.clusters.tsv")):
        members.update(row["proteins"].split(";"))
    in_cluster = np.array([1 if i in members else 0 for i in ids], dtype=np.int32)  # (every gene of the fixture)
    assert in_cluster.sum() > 0
    A = len(oracle_model["attrs"])
    smask, tmask = oracle_model["state_mask"], oracle_model["trans_mask"]
    sfid = np.full(A * 2, -1, dtype=np.int32)
    sfid[smask.ravel()] = np.arange(int(smask.sum()))
    tfid = np.full(4, -1, dtype=np.int32)
    tfid[tmask.ravel()] = int(smask.sum()) + np.arange(int(tmask.sum()))
    K = int(smask.sum() + tmask.sum())
    w = np.concatenate([oracle_model["state"][smask], oracle_model["trans"][tmask]])
    # labelled from clusters.tsv, and with a label switch inside the windows
    mixed = in_cluster.copy()
    mixed[:7] = 0
    for labels in (in_cluster, mixed):
        tr = _native.Trainer(cptr, gptr, attr, labels, A, 20, 1, sfid, tfid, K)
        check_eval(tr, (cptr, gptr, attr, labels, A, sfid, tfid, K), w, 20, 1)


def test_longer_windows_are_refused():
    from gecco_amd import _native

    with pytest.raises(_native.NativeError, match="windows of 1 to 32"):
        _native.Trainer([0, 40], np.zeros(41, dtype=np.int32), [], np.zeros(40, dtype=np.int32), 1, 33, 1, [-1, -1],
                        [-1] * 4, 0)


# ---------------------------------------------------------------- fit against scipy
def _synthetic_training_set(seed, W, step=1, A=40, n_items=3000):
    from gecco_amd import synth, train

    rng = np.random.default_rng(seed)
    lengths = rng.integers(W + 5, 120, size=n_items // 60)
    seq_ptr, item_ptr, attr_id, labels = synth.synth_training_set(rng, lengths, A, stay=0.93)
    seqs, labs = [], []
    for s in range(len(seq_ptr) - 1):
        items = []
        for i in range(seq_ptr[s], seq_ptr[s + 1]):
            items.append(list(dict.fromkeys(f"a{a}" for a in attr_id[item_ptr[i]:item_ptr[i + 1]])))
        seqs.append(items)
        labs.append([str(x) for x in labels[seq_ptr[s]:seq_ptr[s + 1]]])
    return train.build_training_set(seqs, labs, W, step)


def _np_fg(ts, c2):
    A = len(ts.attrs_)

    def fg(w):
        f, g = np_objective(ts.seq_ptr, ts.item_ptr, ts.attr_id, ts.labels, A, ts.window, ts.step, ts.state_fid.ravel(),
                            ts.trans_fid.ravel(), w)
        return f + c2 * float(w @ w), g + 2 * c2 * w

    return fg


def test_fit_l2_reaches_the_scipy_optimum():
    import scipy.optimize
    from gecco_amd import train

    ts = _synthetic_training_set(11, W=5)
    params = train.trainer_params({"c1": 0.0, "c2": 0.15, "epsilon": 1e-10, "delta": 0.0})
    res = train.fit_training_set(ts, params)
    fg = _np_fg(ts, 0.15)
    ref = scipy.optimize.minimize(fg, np.zeros(ts.num_features), jac=True, method="L-BFGS-B",
                                  options={"ftol": 1e-15, "gtol": 1e-10, "maxiter": 10000})
    f_ours = fg(res.x)[0]
    assert abs(f_ours - ref.fun) <= 1e-8 * abs(ref.fun), (f_ours, ref.fun, res)
    assert np.abs(res.x - ref.x).max() <= 1e-4


def test_fit_l1_satisfies_kkt():
    from gecco_amd import train

    ts = _synthetic_training_set(12, W=5, A=60, n_items=1200)  # (small enough for f's rounding not to hide a 1e-5 gradient)
    c1 = 0.4
    params = train.trainer_params({"c1": c1, "c2": 0.0, "epsilon": 1e-10, "delta": 0.0})
    res = train.fit_training_set(ts, params)
    _, g = _np_fg(ts, 0.0)(res.x)
    w = res.x
    nz = w != 0
    assert nz.any() and (~nz).any()
    assert np.abs(g[nz] + c1 * np.sign(w[nz])).max() <= 1e-5
    assert np.abs(g[~nz]).max() <= c1 + 1e-5


# ---------------------------------------------------------------- fit -> save -> trained -> predict
def _genes(rng, n_contigs=12):
    from gecco_amd.model import Domain, Gene, Protein, Source, Strand

    genes = []
    vocab = [f"PF{k:05d}" for k in range(30)]
    for c in range(n_contigs):
        src = Source(f"contig{c}")
        n = int(rng.integers(25, 60))
        lab = np.cumsum(rng.random(n) < 0.08) & 1
        for i in range(n):
            k = int(rng.integers(0, 4))
            names = rng.choice(vocab[15:] if lab[i] else vocab[:15], size=k)
            doms = [Domain(str(nm), 10 * j, 10 * j + 9, "Pfam", 1e-5, 1e-6, probability=float(lab[i]))
                    for j, nm in enumerate(names)]
            genes.append(Gene(src, 1000 * i, 1000 * i + 900, Strand.Coding,
                              Protein(f"contig{c}_{i}", None, doms), _probability=float(lab[i])))
    return genes


def test_fit_save_trained_predict(tmp_path, monkeypatch):
    from oracle import crf_oracle as orc
    from oracle import lcrf
    from gecco_amd import packing, pickle_model
    from gecco_amd.crf import ClusterCRF

    monkeypatch.delenv("GECCO_AMD_FIT", raising=False)
    rng = np.random.default_rng(5)
    genes = _genes(rng)
    random.seed(3)
    crf = ClusterCRF("protein", window_size=5, window_step=1, c1=0.1, c2=0.05)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        crf.fit(genes)
    assert crf.training_result_.n_iter > 0
    crf.save(tmp_path)
    loaded = ClusterCRF.trained(tmp_path)
    blob = pickle_model.crfsuite_blob(pickle_model.load_model_dir(tmp_path))
    m = lcrf.parse_lcrf(blob)
    crf_state = pickle_model.load_model_dir(tmp_path).state["model"].state
    assert crf_state["c1"] == 0.1 and crf_state["c2"] == 0.05 and crf_state["algorithm"] == "lbfgs"
    # the views name exactly the optimiser's non-zero weights (rounded to 6 decimals as sklearn-crfsuite's are): the
    # features rebuilt from the same instances (same shuffle), mapped through their names
    from gecco_amd import train

    random.seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        feats, labels = crf.training_instances(genes)
    ts = train.build_training_set(feats, labels, 5, 1)
    w = crf.training_result_.x
    S = len(ts.state_attr)
    assert len(w) == ts.num_features
    exp_state = {(ts.attrs_[a], ts.labels_[y]): float("%f" % w[k])
                 for k, (a, y) in enumerate(zip(ts.state_attr, ts.state_label)) if w[k] != 0}
    exp_trans = {(ts.labels_[i], ts.labels_[j]): float("%f" % w[S + k])
                 for k, (i, j) in enumerate(zip(ts.trans_src, ts.trans_dst)) if w[S + k] != 0}
    assert len(exp_state) > 0
    for view in (crf.model, loaded.model):
        assert view.state_features_ == exp_state
        assert view.transition_features_ == exp_trans
    # and the same views as the model file parsed back
    sf = loaded.model.state_features_
    assert sf == lcrf.state_features_view(m) and len(sf) == int(m["state_mask"].sum())
    tf = loaded.model.transition_features_
    for i, a in enumerate(m["labels"]):
        for j, b in enumerate(m["labels"]):
            if m["trans_mask"][i, j]:
                assert tf[(a, b)] == float("%f" % m["trans"][i, j])
    # probabilities = the oracle's windowed marginals under the trained tables
    preds = loaded.predict_probabilities(_genes(np.random.default_rng(9), 4), pad=True)
    contigs = [[g for g in preds if g.source.id == c] for c in dict.fromkeys(g.source.id for g in preds)]
    batch = packing.pack_contigs(contigs, {a: i for i, a in enumerate(m["attrs"])}, "protein")
    exp = orc.windowed_marginals(m["state"], m["trans"], batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32),
                                 batch.attr_id, 5, 1, m["labels"].index("1"), True)
    got = np.array([g.average_probability for g in preds])
    assert np.abs(got - exp).max() <= 1e-12
