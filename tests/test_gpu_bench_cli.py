"""bench.py's command line on the GPU, at BASELINE config 2's shape (n=256, T=64,
r=8), a fresh process per run as a user starts it:

* a plain run times exactly --steps iterations, prints one JSON line with the
  headline fields and none of the measurements that take runs of their own, and
  --dump-outputs writes the timed fit()'s outputs as float arrays whose last
  ELBO / MSE are the line's `elbo_last` / `mse_last`;
* --full (here without the CPU baselines) adds `kernels` and `roofline`, and
  its timed fit() computes what the plain run's did (same seed, same inputs:
  ELBO and MSE bit for bit).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SHAPE = ["--n", "256", "--t-per-gpu", "64", "--latent-dim", "8"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("kernels", "roofline", "cpu_baseline", "secondary")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", *SHAPE, *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_dumps_and_full_run_agrees(gpu_device, tmp_path):
    out = _bench("--dump-outputs", str(tmp_path))
    for k in HEADLINE:
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["ms_per_step"] > 0
    units = 64 * 256 * 255 / 2.0
    assert out["value"] == pytest.approx(units / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert not any(k in out for k in FULL_ONLY)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"elbo", "reconstruction_error", "X_mean", "X_cov"} == set(out["outputs_dumped"])
    assert got["elbo"].shape == (3,) and got["reconstruction_error"].shape == (3,)
    assert got["X_mean"].shape == (256, 64, 18) and got["X_mean"].dtype == np.float32
    assert got["X_cov"].shape == (256, 64, 18, 18) and got["X_cov"].dtype == np.float32
    assert all(np.isfinite(a).all() for a in got.values())
    assert got["elbo"][-1] == out["elbo_last"] and got["reconstruction_error"][-1] == out["mse_last"]
    assert sum(a.nbytes for a in got.values()) <= 64e6

    full = _bench("--full", "--no-cpu-baseline")
    assert full["full"] is True and full["steps"] == 3
    assert set(full["kernels"]) == {"sweep", "cov", "elbo", "pairs"}
    assert all(full["kernels"][k]["ms"] > 0 for k in full["kernels"])
    assert full["roofline"]["kernel"] == "sweep" and 0 < full["roofline"]["frac"] < 1
    assert full["elbo_last"] == out["elbo_last"] and full["mse_last"] == out["mse_last"]
