"""CPU: bench.py's --dump-outputs writer on a stand-in engine: float arrays, the
timed steps' history only, a full array below the per-array budget and a fixed
seeded row sample above it, identical from call to call."""
import os

import numpy as np
import torch

import bench


class _Engine:
    def __init__(self, n, TL, d):
        g = torch.Generator().manual_seed(3)
        # device layout (T_local, n, d[, d]); the views are (n, T_local, ...)
        self.x = torch.randn(TL, n, d, generator=g)
        self.c = torch.randn(TL, n, d, d, generator=g)

    def means_local(self):
        return self.x.permute(1, 0, 2)

    def covs_local(self):
        return self.c.permute(1, 0, 2, 3)


class _VI:
    def __init__(self, eng):
        self.engine = eng


def test_dump_outputs_sample_and_history(tmp_path, monkeypatch):
    n, TL, d = 12, 7, 6
    eng = _Engine(n, TL, d)
    # budget: the means (84 rows x 24 B) fit, the covariances (84 x 144 B) do not
    monkeypatch.setattr(bench, "DUMP_ARRAY_BYTES", 30 * 4 * d * d)
    hist = {"elbo": [torch.tensor(float(i)) for i in range(9)],
            "reconstruction_error": [0.5 * i for i in range(9)]}
    shapes = bench.dump_outputs(str(tmp_path / "a"), _VI(eng), hist, steps=4)
    assert shapes == {"elbo": [4], "reconstruction_error": [4], "X_mean": [n, TL, d],
                      "X_cov": [30, d, d]}
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == set(shapes)
    assert got["elbo"].dtype == np.float64 and got["reconstruction_error"].dtype == np.float64
    assert got["X_mean"].dtype == np.float32 and got["X_cov"].dtype == np.float32
    assert got["elbo"].tolist() == [5.0, 6.0, 7.0, 8.0]          # the timed steps, not the warmup
    assert got["reconstruction_error"].tolist() == [2.5, 3.0, 3.5, 4.0]
    assert np.array_equal(got["X_mean"], eng.means_local().numpy())
    rows = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(n * TL, 30, replace=False))
    assert np.array_equal(got["X_cov"], eng.covs_local().reshape(n * TL, d, d).numpy()[rows])
    # the same call again writes the same bytes
    bench.dump_outputs(str(tmp_path / "b"), _VI(eng), hist, steps=4)
    for name, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy"))


def test_dump_budget_keeps_the_headline_shape_under_64_mb():
    n, TL, d = 1024, 128, 34
    total = 0
    for row in (4 * d, 4 * d * d):
        total += min(n * TL, bench.DUMP_ARRAY_BYTES // row) * row
    assert total <= 64e6
