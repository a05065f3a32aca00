"""The end-to-end EM experiment shared by tests/test_mstep_ref.py (CPU) and
tests/test_gpu_mstep.py: n = 40, T = 16, r = 2, seed 3; data generated at
ar = 0.8; EM starts from the parameters of ar = 0.5 with 3 x the true R;
"good" factorisation, lr = 0.5, 6 rounds of 5 sweeps, update = (Phi, Q, R).
The CPU runs are computed once per process."""
import functools

import numpy as np

import mstep_ref as M


def make_model():
    """The model with its data generated at the true parameters and its
    attributes then set to the EM start (fp32, as a user would set them)."""
    import torch
    import ame_oracle as O
    from ame_amd import TemporalAMEModel
    n, T, r = M.EM_SHAPE
    m = TemporalAMEModel(n, T, r, ar_coefficient=M.TRUE_AR, seed=M.EM_SEED)
    m.generate_data()
    start = O.model_params(r, ar=M.START_AR)
    m.Phi = torch.from_numpy(start["Phi"].copy())
    m.Q = torch.from_numpy(start["Q"].copy())
    m.R = (M.START_R_SCALE * m.R).clone()
    m.R_inv = torch.linalg.inv(m.R)
    return m


def start_params(m):
    return {k: getattr(m, k).numpy().astype(np.float64) for k in M.PARAMS}


def relative_deviation(a, b):
    """max over Phi, Q, R of max|a - b| / max|a|: one scale-free number."""
    return max(float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max() / np.abs(np.asarray(a[k])).max())
               for k in ("Phi", "Q", "R"))


@functools.lru_cache(maxsize=None)
def cpu_runs():
    """fp64 oracle EM and the same EM on fp32 state arrays, from the initial
    state a VI instance of this model starts with."""
    from ame_amd import TemporalAMEStructuredMFVI
    m = make_model()
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=M.EM_LR)
    X0 = vi.X_mean.numpy().astype(np.float64)
    S0 = vi.X_cov.numpy().astype(np.float64)
    Y = m.Y.numpy().astype(np.float64)
    p = start_params(m)
    return dict(em64=M.oracle_em(Y, X0, S0, p), em32=M.oracle_em(Y, X0, S0, p, dtype=np.float32))
