"""Generate the gp_* golden fixtures: the reference run at model parameters
that have none of the constructor defaults' symmetries.

TEST INFRASTRUCTURE ONLY, in the style of make_golden.py: runs in the build
container, where the reference (Alfieriek/Python-Temporal-AME-SVI) is mounted
read-only at /root/reference, imports the reference's own classes and writes
plain-data ``.npz`` files next to this script.  No test reads this script.

Usage (from the repo root)::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_params.py

For each parameter set the reference model TemporalAMEModel(n, T, r, seed=42)
is built, its attributes R, R_inv (= torch.linalg.inv(R)), Sigma, Psi, Phi, Q
are overwritten with fp32 tensors (the reference reads them as plain
attributes: temporal_ame.py:172-216, structured_mf.py:124-326,
naive_mf.py:114-376), generate_data(return_latents=True) is called, and good /
bad / naive run for 2 iterations in fp32 and in make_golden.to_f64's fp64 mode.

Sets (recipes in tests/generic_params.py, rng seeds below):
  gen    all six generic at once
  phi    only Phi generic (separates Q^-1 Phi from Phi^T Q^-1)
  rinv   only R with unequal variances
  ctor1..3  constructor arguments only (generic_params.CTOR)

Files: gp_<set>_<method>[_f64].npz, each self-contained (parameters, Y, initial
state, trajectory).  The names do not match *_lr*.npz, which other tests glob.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as G  # noqa: E402  (puts the reference on sys.path)
import generic_params as GP  # noqa: E402
from src.models import TemporalAMEModel  # noqa: E402

ITERS = 2
# lr = 0.2: the reference's own fp32 run then stays within 2e-6 of its fp64 run
# on the means over both iterations (at lr = 0.5 .. 0.7 the `bad` runs of phi
# and ctor1 / ctor3 drift 1e-5 .. 4e-5 apart), so the fixtures are comparable
# at test_oracle_golden.py's fp32 bound and test_gpu_parity.py's device bounds.
# set -> (n, T, r, lr, rng seed of the recipe)
GENERIC = {"gen": (12, 4, 3, 0.2, 20261), "phi": (15, 4, 2, 0.2, 20262),
           "rinv": (13, 4, 3, 0.2, 20263)}
CTOR_SHAPES = {"ctor1": (12, 4, 2, 0.2), "ctor2": (10, 4, 3, 0.2), "ctor3": (14, 4, 2, 0.2)}


def build(pset):
    if pset in GENERIC:
        n, T, r, lr, seed = GENERIC[pset]
        m = TemporalAMEModel(n_nodes=n, n_time=T, latent_dim=r, seed=42)
        for k, v in GP.generic_params(r, seed, GP.SETS[pset]).items():
            setattr(m, k, torch.from_numpy(v.copy()))
        if "R" in GP.SETS[pset]:
            m.R_inv = torch.linalg.inv(m.R)
    else:
        n, T, r, lr = CTOR_SHAPES[pset]
        m = TemporalAMEModel(n_nodes=n, n_time=T, latent_dim=r, seed=42, **GP.CTOR[pset])
    m.generate_data(return_latents=True)
    return m, lr


if __name__ == "__main__":
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    for pset in list(GENERIC) + list(CTOR_SHAPES):
        for method in ("good", "bad", "naive"):
            for f64 in (False, True):
                m, lr = build(pset)      # fresh copy: to_f64 converts the model in place
                arrays = G.model_arrays(m)
                rec = G.run_trajectory(m, method, lr, ITERS, {1, 2}, {2}, f64=f64)
                rec.update(arrays)
                rec["lr"] = np.float64(lr)
                rec["iters"] = np.int64(ITERS)
                G.save(f"gp_{pset}_{method}{'_f64' if f64 else ''}.npz", rec)
