"""The library leaves the caller's current device alone: with device 0 current, work on device 1 (create, evaluate and free
a trainer of either family, a Fisher test, a one-shot Viterbi) hands device 0 back after every step, and computes there, bit for
bit, what the same calls compute on device 0 (crf_hip_own.hpp: DeviceScope)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")  # (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

from gecco_amd import _native as nat  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    """The HIP runtime the library itself runs on: the one copy of libamdhip64 in this process."""
    if nat.device_count() < 2:
        pytest.skip("needs two visible devices")
    nat.load_library()
    paths = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths[0])


def current_device(hip) -> int:
    d = ctypes.c_int(-1)
    assert hip.hipGetDevice(ctypes.byref(d)) == 0
    return d.value


def general_trainer(device):  # one problem: one sequence of 4 items, 3 labels, window 2
    problem = ([0, 4], [0, 1, 2, 3, 4], [0, 1, 2, 0], [0, 1, 2, 1], 3, np.arange(9), 9 + np.arange(9), 18, 2, 1)
    tr = nat.TrainerGeneral([problem], device=device)
    f, g = tr.eval([np.linspace(-1.0, 1.0, 18)])
    del tr
    return f.tobytes() + g[0].tobytes()


def binary_trainer(device):  # 2 labels, window 2
    tr = nat.Trainer([0, 4], [0, 1, 2, 3, 4], [0, 1, 1, 0], [0, 1, 1, 0], 2, 2, 1, [0, 1, 2, 3], [4, 5, 6, 7], 8, device=device)
    f, g = tr.eval(np.linspace(-1.0, 1.0, 8))
    del tr
    return np.float64(f).tobytes() + g.tobytes()


def fisher(device):
    return nat.fisher_exact([[3, 1], [2, 7]], device=device).tobytes()


def viterbi(device):  # one contig of 3 genes
    m = nat.Model.from_tables(np.array([[0.5, -0.5], [-0.25, 0.25]]), np.array([[0.1, -0.1], [-0.2, 0.2]]))
    y, score = m.viterbi([0, 3], [0, 1, 2, 3], [0, 1, 1], device=device)
    del m
    return y.tobytes() + score.tobytes()


def test_work_on_another_device_leaves_the_current_one(hip):
    assert hip.hipSetDevice(0) == 0
    for step in (general_trainer, binary_trainer, fisher, viterbi):
        there = step(1)
        assert current_device(hip) == 0, step.__name__
        here = step(0)
        assert current_device(hip) == 0, step.__name__
        assert there == here, step.__name__
