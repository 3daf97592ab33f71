"""Cross-validation on the host: the splitters, the metrics against sklearn, the lock-step optimiser against
``minimize`` alone, and the cv.tsv format (gecco_amd/cv.py, gecco_amd/train.py)."""
import doctest
import io
import warnings

import numpy as np
import pytest

from benchkit.train_objective import objective


def test_leave_one_group_out_reproduces_the_reference_docstring():
    from gecco_amd import cv

    res = doctest.DocTestRunner(verbose=False)
    for t in doctest.DocTestFinder().find(cv.LeaveOneGroupOut):
        res.run(t)
    assert res.failures == 0 and res.tries >= 3
    loto = cv.LeaveOneGroupOut()
    groups = [["a"], ["b"], ["c"], ["a", "b"]]
    folds = list(loto.split(range(4), groups=groups))
    assert [(a.tolist(), b.tolist()) for a, b in folds] == [([1, 2], [0]), ([0, 2], [1]), ([0, 1, 3], [2])]
    assert loto.get_n_splits(groups=[["Polyketide"], ["NRP"], ["RiPP"]]) == 3
    assert loto.get_n_splits(groups=[["Terpene"], ["NRP"], ["RiPP"], ["Terpene", "NRP"]]) == 3
    with pytest.raises(ValueError, match="should not be None"):
        loto.get_n_splits()
    with pytest.raises(ValueError, match="should not be None"):
        list(loto.split(range(3)))
    # a sample without a group is always trained on and never tested
    folds = list(loto.split(range(3), groups=[["a"], [], ["b"]]))
    assert [(a.tolist(), b.tolist()) for a, b in folds] == [([1, 2], [0]), ([0, 1], [2])]


def test_kfold_splits_match_sklearn():
    KFold = pytest.importorskip("sklearn.model_selection").KFold
    from gecco_amd.cv import kfold_splits

    for n in range(2, 41):
        for k in range(2, n + 1):
            ours = kfold_splits(n, k)
            ref = list(KFold(k).split(range(n)))
            assert len(ours) == len(ref)
            for (a, b), (c, d) in zip(ours, ref):
                assert a.tolist() == c.tolist() and b.tolist() == d.tolist()
        for k in (n + 1, n + 5):
            with pytest.raises(ValueError) as ours_err:
                kfold_splits(n, k)
            with pytest.raises(ValueError) as ref_err:
                list(KFold(k).split(range(n)))
            assert str(ours_err.value) == str(ref_err.value)
    for k in (0, 1):
        with pytest.raises(ValueError) as ours_err:
            kfold_splits(10, k)
        with pytest.raises(ValueError) as ref_err:
            KFold(k)
        assert str(ours_err.value) == str(ref_err.value)


def _metric_cases():
    rng = np.random.default_rng(3)
    cases = []
    for n in (2, 3, 7, 50, 400):
        for ties in (0, 2, 5, 1000):
            y = rng.random(n) < 0.4
            y[0], y[-1] = True, False
            s = rng.random(n)
            if ties:
                s = np.round(s * ties) / ties if ties < 1000 else s
            cases.append((y, s))
    cases.append((np.array([1, 0, 1, 0]), np.array([0.5, 0.5, 0.5, 0.5])))  # every score tied
    cases.append((np.array([0, 0, 1, 1, 1]), np.array([0.1, 0.9, 0.9, 0.9, 0.2])))
    return cases


def test_roc_auc_and_average_precision_match_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    from gecco_amd.cv import average_precision, roc_auc

    for y, s in _metric_cases():
        assert abs(roc_auc(y, s) - metrics.roc_auc_score(y, s)) <= 1e-12
        assert abs(average_precision(y, s) - metrics.average_precision_score(y, s)) <= 1e-12
        yl = [bool(v) for v in y]
        assert abs(roc_auc(yl, list(s)) - metrics.roc_auc_score(yl, list(s))) <= 1e-12


def test_one_class_behaves_as_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    from gecco_amd.cv import average_precision, roc_auc

    s = [0.1, 0.4, 0.3]
    for y in ([0, 0, 0], [1, 1, 1]):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref_auc = metrics.roc_auc_score(y, s)
            ref_ap = metrics.average_precision_score(y, s)
        with pytest.warns(UserWarning, match="Only one class"):
            ours = roc_auc(y, s)
        assert np.isnan(ours) and np.isnan(ref_auc)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert average_precision(y, s) == ref_ap
    with pytest.raises(ValueError):
        roc_auc([0, 1], [0.1, float("nan")])
    with pytest.raises(ValueError):
        average_precision([0, 1, 1], [0.1, 0.2])


def _np_problem(seed, W, step, A=12, n_seqs=6):
    from gecco_amd import synth

    rng = np.random.default_rng(seed)
    lengths = [W] + list(rng.integers(W, W + 25, size=n_seqs))
    seq_ptr, item_ptr, attr_id, labels = synth.synth_training_set(rng, lengths, A, stay=0.85)
    sfid = np.arange(2 * A, dtype=np.int32)
    tfid = 2 * A + np.arange(4, dtype=np.int32)
    K = 2 * A + 4

    def fg(w, c2):
        f, g, _ = objective(seq_ptr, item_ptr, attr_id, labels, A, W, step, sfid, tfid, w)
        return f + c2 * float(w @ w), g + 2 * c2 * w

    return K, fg


@pytest.mark.parametrize("c1", [0.0, 0.3])
def test_stepping_minimize_in_lock_step_equals_minimize(c1):
    from gecco_amd import train

    c2 = 0.1
    problems = [_np_problem(s, W, step) for s, (W, step) in enumerate([(3, 1), (5, 2), (4, 1), (2, 1)])]
    alone = [train.minimize(lambda w, fg=fg: fg(w, c2), np.zeros(K), c1=c1) for K, fg in problems]
    steppers = [train.minimize_steps(np.zeros(K), c1=c1) for K, _ in problems]
    pending = [next(st) for st in steppers]
    results = [None] * len(problems)
    while any(x is not None for x in pending):
        for k, x in enumerate(pending):  # one round: every unfinished problem takes one step
            if x is None:
                continue
            try:
                pending[k] = steppers[k].send(problems[k][1](x, c2))
            except StopIteration as stop:
                pending[k], results[k] = None, stop.value
    for a, b in zip(alone, results):
        assert a.x.tobytes() == b.x.tobytes()
        assert np.float64(a.f).tobytes() == np.float64(b.f).tobytes()
        assert (a.n_iter, a.n_eval, a.status) == (b.n_iter, b.n_eval, b.status)
        assert a.n_iter > 0


def test_stepping_minimize_rejects_a_non_finite_start():
    from gecco_amd import train

    steps = train.minimize_steps(np.zeros(3))
    next(steps)
    with pytest.raises(ValueError, match="not finite at the start"):
        steps.send((float("nan"), np.zeros(3)))


def test_cv_table_format():
    from gecco_amd.cv import Fold, cv_table
    from gecco_amd.model import Gene, Protein, Source, Strand

    def gene(seq, pid, start, p):
        return Gene(Source(seq), start, start + 99, Strand.Coding if start % 2 else Strand.Reverse,
                    Protein(pid, None), _probability=p)

    folds = [Fold(index=1, predicted=[gene("s1", "a", 1, 0.25), gene("s1", "b", 200, 0.9)], truth=[False, True]),
             Fold(index=2, predicted=[gene("s2", "c", 7, 1.0)], truth=[True])]
    text = cv_table(folds).decode()
    lines = text.splitlines()
    assert lines[0] == "sequence_id\tprotein_id\tstart\tend\tstrand\taverage_p\tmax_p\tfold\tis_cluster"
    assert lines[1] == "s1\ta\t1\t100\t+\t0.25\t0.25\t1\tfalse"
    assert lines[2] == "s1\tb\t200\t299\t-\t0.9\t0.9\t1\ttrue"
    assert lines[3] == "s2\tc\t7\t106\t+\t1.0\t1.0\t2\ttrue"
    assert len(lines) == 4 and text.endswith("\n")
