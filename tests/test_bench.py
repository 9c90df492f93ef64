"""bench.py's command line: a plain run measures the headline alone and can
write what its last timed step returned; --full adds the other figures.

Runs the benchmark itself (that is the subject) on its own 1M-trial dataset
(about half a second per run) with a few steps, and with every --full leg that
needs a workload of its own switched off.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1"]
TRIALS = 1_000_000


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout  # one JSON result line
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b" / "nested")
    out = _bench("--dump-outputs", d1)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1
    assert out["unit"] == "trials/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["ms_per_step"] > 0
    # value and ms_per_step are the same measurement
    assert out["value"] == pytest.approx(TRIALS / (out["ms_per_step"] * 1e-3), rel=1e-9)
    # nothing but the headline in a plain run
    for k in ("roofline", "stress", "c2", "c5_n1", "c4", "cpu_baseline"):
        assert k not in out, k
    assert "pdf_sv_evals_per_trial" not in out["config"]
    assert os.listdir(d1) == ["logp.npy"]
    a = np.load(os.path.join(d1, "logp.npy"))
    assert a.dtype == np.float64 and a.shape == (1,)
    assert np.isfinite(a[0]) and a[0] == out["config"]["logp"]
    # the same arguments give the same inputs, hence the same output
    _bench("--dump-outputs", d2)
    assert np.array_equal(np.load(os.path.join(d2, "logp.npy")), a)


@pytest.mark.gpu
def test_full_run_adds_the_kernel_figures(tmp_path):
    d = str(tmp_path / "full")
    out = _bench("--full", "--no-stress", "--no-extra", "--no-c4", "--no-cpu-baseline",
                 "--dump-outputs", d)
    assert out["roofline"]["kernel_launches"] >= 3 and out["roofline"]["kernel_ms_avg"] > 0
    assert out["config"]["pdf_sv_evals_per_trial"] >= 1
    a = np.load(os.path.join(d, "logp.npy"))
    assert a[0] == out["config"]["logp"]


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr
