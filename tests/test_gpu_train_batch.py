"""The batched training objective (gecco_crf_trainer_batch_*): every problem's f and g are bitwise a lone trainer's,
whatever the other problems hold and whichever are active."""
import numpy as np
import pytest

from tests.helpers import lone_trainer, same_bits, training_set

pytestmark = pytest.mark.gpu


def _problems(seed, W, step, n=10):
    """Problem 0 has more than 256 x 256 windows, problem 1 fewer than 256; the rest differ in A, features, lengths."""
    rng = np.random.default_rng(seed)
    big_seqs = (256 * 256 * step) // 60 + 200
    probs = [training_set(rng, W, step, A=90, n_seqs=big_seqs, drop=0.05, max_extra=120),
             training_set(rng, W, step, A=7, n_seqs=1, drop=0.0, max_extra=3)]
    for k in range(2, n):
        probs.append(training_set(rng, W, step, A=int(rng.integers(1, 120)), n_seqs=int(rng.integers(1, 40)),
                              drop=float(rng.choice([0.0, 0.1, 0.5]))))
    return probs


def _batch(probs, W, step):
    from gecco_amd import _native

    return _native.TrainerBatch([p[:8] for p in probs], W, step)


def _weights(rng, probs):
    return [rng.normal(0, 1.5, size=p[7]) for p in probs]


@pytest.mark.parametrize("W,step", [(1, 1), (5, 1), (5, 3), (20, 1), (20, 3), (32, 1), (32, 3)])
def test_batch_is_bitwise_the_lone_trainers(W, step):
    from gecco_amd import _native

    probs = _problems(7000 + 31 * W + step, W, step)
    lone = [lone_trainer(p) for p in probs]
    assert lone[0].num_windows > 256 * 256 and lone[1].num_windows < 256
    rng = np.random.default_rng(W * 10 + step)
    for K in (1, 2, 5, 10):
        batch = _batch(probs[:K], W, step)
        assert len(batch) == K
        assert [batch.num_windows(k) for k in range(K)] == [t.num_windows for t in lone[:K]]
        masks = [np.ones(K, dtype=bool)] + [rng.random(K) < 0.5 for _ in range(3)]
        for mask in masks:
            ws = _weights(rng, probs[:K])
            f, g = batch.eval(ws, mask)
            for k in np.flatnonzero(mask):
                ef, eg = lone[k].eval(ws[k])
                assert same_bits(f[k], g[k], ef, eg), (K, k, f[k], ef)

        # one problem in log space (transitions 720 / -800 apart), one with non-finite weights: the others keep their bits
        ws = _weights(rng, probs[:K])
        hot = K - 1
        tfid = probs[hot][6]
        for j, v in zip(range(4), (720.0, -800.0, 0.0, 720.0)):
            if tfid[j] >= 0:
                ws[hot][tfid[j]] = v
        if K > 2:
            ws[1] = ws[1].copy()
            ws[1][:] = np.nan
        f, g = batch.eval(ws)
        for k in range(K):
            if K > 2 and k == 1:
                assert not np.isfinite(f[k])
                continue
            ef, eg = lone[k].eval(ws[k])
            assert same_bits(f[k], g[k], ef, eg), (K, k)


def test_inactive_outputs_are_untouched_and_bad_problems_are_named():
    from gecco_amd import _native

    W, step = 5, 1
    probs = _problems(91, W, step, n=5)
    batch = _batch(probs, W, step)
    rng = np.random.default_rng(2)
    ws = _weights(rng, probs)
    f = np.full(5, 12345.0)
    g = [np.full(p[7], -7.0) for p in probs]
    mask = np.array([0, 1, 0, 1, 0], dtype=bool)
    batch.eval([w if m else None for w, m in zip(ws, mask)], mask, f, g)
    for k in range(5):
        if mask[k]:
            ef, eg = lone_trainer(probs[k]).eval(ws[k])
            assert same_bits(f[k], g[k], ef, eg)
        else:
            assert f[k] == 12345.0 and np.all(g[k] == -7.0)

    bad = list(probs)
    seq_ptr, item_ptr, attr_id, labels, *rest = bad[3]
    labels = labels.copy()
    labels[0] = 2
    bad[3] = (seq_ptr, item_ptr, attr_id, labels, *rest)
    with pytest.raises(ValueError, match="problem 3: trainer: labels must be 0 or 1"):  # (GECCO_CRF_EINVAL)
        _batch(bad, W, step)
    bad = list(probs)
    A = probs[2][4]
    bad[2] = probs[2][:5] + (np.full(A * 3, -1, dtype=np.int32), np.full(9, -1, dtype=np.int32), probs[2][7])  # 3 labels
    with pytest.raises(_native.NativeError, match="problem 2: trainer: only 2-label") as err:
        _batch(bad, W, step)
    assert err.value.code == _native.EUNSUPPORTED
    with pytest.raises(_native.NativeError, match="problem 0: .*windows of 1 to 32") as err:
        _batch(probs, 33, 1)
    assert err.value.code == _native.EUNSUPPORTED
