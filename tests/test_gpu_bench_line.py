"""GPU: bench.py itself prints ONE strict-JSON line under 4 KB with the contract's keys, `roofline`, `cpu_baseline` and `parity`, and
writes the full record where the line says (round 5's 29 KB line could not be parsed by the driver: this runs the real script)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_short_line(tmp_path):
    detail = str(tmp_path / "detail.json")
    env = dict(os.environ, GECCO_BENCH_DETAIL=detail)
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--workload", "C2",
                         "--no-levels", "--no-latency", "--no-past-l3", "--kernel-iters", "20", "--min-region-ms", "5"],
                        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stderr[-3000:]
    lines = [ln for ln in cp.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:3]
    text = lines[0]
    assert len(text.encode()) < 4096
    d = json.loads(text, parse_constant=lambda c: pytest.fail(f"non-strict JSON constant {c}"))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline", "parity", "detail"):
        assert k in d, k
    assert d["steps"] == 5 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["dtype"] == "f64" and d["unit"] == "genes/s"
    assert d["config"]["workload"].startswith("C2") and d["value"] > 1e9
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["limiter"] == "fp64-valu" and 0 < r["frac"] < 1 and r["peak"] == 8000.0
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["kernel_us"] * 1e-6) / 1e9) <= 1e-3 * r["achieved"]
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline"]["value"] > 1e5
    assert d["parity"]["cluster_call_mismatches"] == 0 and d["parity"]["viterbi_label_mismatches"] == 0
    assert d["parity"]["max_abs_dp_vs_oracle"] <= 1e-12
    full = json.load(open(detail))
    assert full["roofline"]["kernel_us"] == pytest.approx(r["kernel_us"], rel=1e-3) and "viterbi_exactness" in full


def test_bench_dumps_what_the_timed_steps_computed(tmp_path):
    """--dump-outputs: the marginals and Viterbi labels of the last timed step, for every gene of the batch, equal the CPU
    oracle's on the same seeded workload (marginals within 1e-12, labels exactly); the line still counts exactly --steps."""
    import numpy as np

    from gecco_amd import synth
    from oracle import crf_oracle as orc

    out = tmp_path / "outputs"
    env = dict(os.environ, GECCO_BENCH_DETAIL=str(tmp_path / "detail.json"))
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--workload", "C2",
                         "--no-levels", "--no-latency", "--no-past-l3", "--no-cpu-baseline", "--kernel-iters", "20", "--dump-outputs", str(out)],
                        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stderr[-3000:]
    d = json.loads(cp.stdout.strip().splitlines()[-1])
    assert d["steps"] == 7 and d["ms_per_step"] > 0
    full = json.load(open(tmp_path / "detail.json"))
    assert full["timed_region"]["steps"] == 7
    assert full["timed_region"]["ms"] == pytest.approx(d["ms_per_step"] * 7, rel=1e-3)
    assert sorted(full["dumped_outputs"]) == ["labels.npy", "marginals.npy"]

    wl = synth.workload("C2", seed=synth.SEED)
    n = int(wl["contig_ptr"][-1])
    p, y = np.load(out / "marginals.npy"), np.load(out / "labels.npy")
    assert p.dtype == np.float64 and y.dtype == np.float32 and p.shape == (n,) and y.shape == (n,)
    args = (wl["w"], wl["trans"], wl["contig_ptr"], wl["gene_ptr"], wl["attr_id"])
    exp_p = orc.windowed_marginals_mt(*args, 20, 1, 1, True)
    exp_y, _ = orc.viterbi_mt(*args)
    assert float(np.abs(p - exp_p).max()) <= 1e-12
    assert np.array_equal(y, exp_y.astype(np.float32))
