"""fp64 numpy reference of the M-step of variational EM: the sufficient
statistics of q, the closed-form maximisers and the objective F (test-only;
imports nothing from ame_amd except in gpu_network, which generates the GPU
tests' network).  V0 and C01 come from predictive_ref.moments.

q(x_it) = N(m_it, S_it), independent across nodes and time; E_it = m_it m_it' + S_it.

    A0  = sum_i E_i0                 A11 = sum_i sum_{t>=1} E_it
    A00 = sum_i sum_{t>=1} E_i,t-1   A10 = sum_i sum_{t>=1} m_it m_i,t-1'
    Rss = sum_t sum_{i<j} ( e e' + [[V0(i,j), C01(i,j)], [C01(i,j), V0(j,i)]] )

    F = -1/2 [ Np log|R| + tr(R^-1 Rss) ] - 1/2 [ n log|S0| + tr(S0^-1 A0) ]
        -1/2 [ n (T-1) log|Q| + tr(Q^-1 (A11 - Phi A10' - A10 Phi' + Phi A00 Phi')) ]
"""
import numpy as np

import predictive_ref as PR

PARAMS = ("Phi", "Q", "R", "Sigma", "Psi")


def state_rows(X, S):
    """X (n, T, d), S (n, T, d, d) -> rows (T, 2, d, d): P_t = sum_i E_it and
    C_t = sum_i m_it m_i,t-1' (zero at t = 0), and the sums of |summand| of each
    entry (the scale of a re-association error)."""
    X = np.asarray(X, np.float64)
    S = np.asarray(S, np.float64)
    n, T, d = X.shape
    rows = np.zeros((T, 2, d, d))
    mag = np.zeros((T, 2, d, d))
    for t in range(T):
        mm = np.einsum("ia,ib->iab", X[:, t], X[:, t])
        rows[t, 0] = mm.sum(0) + S[:, t].sum(0)
        mag[t, 0] = np.abs(mm).sum(0) + np.abs(S[:, t]).sum(0)
        if t > 0:
            mp = np.einsum("ia,ib->iab", X[:, t], X[:, t - 1])
            rows[t, 1] = mp.sum(0)
            mag[t, 1] = np.abs(mp).sum(0)
    return rows, mag


def dyad_rows(X, S, r, Y):
    """Rows (T, 4): pairs, Rss00, Rss11, Rss01 over i < j with Y[i, j, t] as the
    observation, and the per-slice sums of |summand| of the last three."""
    X = np.asarray(X, np.float64)
    S = np.asarray(S, np.float64)
    Y = np.asarray(Y, np.float64)
    n, T, _ = X.shape
    iu = np.triu_indices(n, 1)
    rows = np.zeros((T, 4))
    mag = np.zeros((T, 4))
    for t in range(T):
        mean, V0, C01 = PR.moments(X[:, t], S[:, t], r)
        e = Y[iu[0], iu[1], t] - mean[iu[0], iu[1]]
        v00, v11, c = V0[iu[0], iu[1]], V0[iu[1], iu[0]], C01[iu[0], iu[1]]
        rows[t] = (len(iu[0]), (e[:, 0] ** 2 + v00).sum(), (e[:, 1] ** 2 + v11).sum(),
                   (e[:, 0] * e[:, 1] + c).sum())
        mag[t] = (len(iu[0]), (e[:, 0] ** 2 + np.abs(v00)).sum(), (e[:, 1] ** 2 + np.abs(v11)).sum(),
                  (np.abs(e[:, 0] * e[:, 1]) + np.abs(c)).sum())
    return rows, mag


def gpu_network(n, T, r):
    """The network (n, n, T, 2), fp32, of the direct kernel cases of
    tests/test_gpu_mstep.py and tests/test_gpu_covar.py: what their _Device
    packs, and what the CPU tests of the references' sensitivity read."""
    from ame_amd import TemporalAMEModel
    m = TemporalAMEModel(n, T, r, seed=5)
    m.generate_data_fast(seed=9)
    return np.ascontiguousarray(m.Y.numpy(), dtype=np.float32)


def combine(srows, drows):
    """Per-slice rows in time order -> the statistics."""
    T = srows.shape[0]
    d = srows.shape[2]
    z = np.zeros((d, d))
    s = drows.sum(0)
    return dict(A0=srows[0, 0].copy(), A11=srows[1:, 0].sum(0) if T > 1 else z.copy(),
                A00=srows[:-1, 0].sum(0) if T > 1 else z.copy(),
                A10=srows[1:, 1].sum(0) if T > 1 else z.copy(),
                Rss=np.array([[s[1], s[3]], [s[3], s[2]]]), pairs=float(s[0]))


def statistics(X, S, r, Y):
    return combine(state_rows(X, S)[0], dyad_rows(X, S, r, Y)[0])


def blockdiag(Sigma, Psi):
    d = 2 + Psi.shape[0]
    S0 = np.zeros((d, d))
    S0[:2, :2] = Sigma
    S0[2:, 2:] = Psi
    return S0


def scatter(st, Phi):
    return st["A11"] - Phi @ st["A10"].T - st["A10"] @ Phi.T + Phi @ st["A00"] @ Phi.T


def _ld(a):
    sign, ld = np.linalg.slogdet(a)
    return ld if sign > 0 else float("nan")


def objective(st, p, n, T):
    """F(theta) for p = dict(Phi, Q, R, Sigma, Psi)."""
    S0 = blockdiag(p["Sigma"], p["Psi"])
    f = -0.5 * (st["pairs"] * _ld(p["R"]) + np.trace(np.linalg.solve(p["R"], st["Rss"])))
    f += -0.5 * (n * _ld(S0) + np.trace(np.linalg.solve(S0, st["A0"])))
    if T > 1:
        f += -0.5 * (n * (T - 1) * _ld(p["Q"]) + np.trace(np.linalg.solve(p["Q"], scatter(st, p["Phi"]))))
    return float(f)


def objective_magnitude(st, p, n, T):
    """Sum of the |terms| of F: the scale of its evaluation error."""
    S0 = blockdiag(p["Sigma"], p["Psi"])
    m = abs(st["pairs"] * _ld(p["R"])) + np.abs(np.linalg.inv(p["R"]) * st["Rss"]).sum()
    m += abs(n * _ld(S0)) + np.abs(np.linalg.inv(S0) * st["A0"]).sum()
    if T > 1:
        Phi = p["Phi"]
        parts = (st["A11"], Phi @ st["A10"].T, st["A10"] @ Phi.T, Phi @ st["A00"] @ Phi.T)
        Qi = np.abs(np.linalg.inv(p["Q"]))
        m += abs(n * (T - 1) * _ld(p["Q"])) + sum((Qi * np.abs(x)).sum() for x in parts)
    return float(m)


def phi_full(st):
    return np.linalg.solve(st["A00"].T, st["A10"].T).T          # A10 A00^-1


def phi_scalar(st, Q_old):
    Qi = np.linalg.inv(Q_old)
    return np.trace(Qi @ st["A10"]) / np.trace(Qi @ st["A00"])


def q_given_phi(st, Phi, n, T):
    M = scatter(st, Phi)
    return 0.5 * (M + M.T) / (n * (T - 1))


def m_step(st, p, n, T, update=("Phi", "Q", "R", "Sigma0"), phi_structure="full"):
    new = {k: np.array(p[k], dtype=np.float64) for k in PARAMS}
    d = new["Phi"].shape[0]
    if "Phi" in update:
        new["Phi"] = phi_full(st) if phi_structure == "full" else phi_scalar(st, new["Q"]) * np.eye(d)
    if "Q" in update:
        new["Q"] = q_given_phi(st, new["Phi"], n, T)
    if "R" in update:
        new["R"] = st["Rss"] / st["pairs"]
    if "Sigma0" in update:
        new["Sigma"] = 0.5 * (st["A0"][:2, :2] + st["A0"][:2, :2].T) / n
        new["Psi"] = 0.5 * (st["A0"][2:, 2:] + st["A0"][2:, 2:].T) / n
    return new


# ---- the end-to-end experiment of the GPU test (tests/test_gpu_mstep.py) ----
EM_SHAPE = (40, 16, 2)      # n, T, r
EM_SEED = 3
EM_ROUNDS, EM_SWEEPS = 6, 5
EM_LR = 0.5
EM_UPDATE = ("Phi", "Q", "R")
TRUE_AR, START_AR, START_R_SCALE = 0.8, 0.5, 3.0
TRUE_R = (0.1, 0.05, 0.1)   # R00, R01, R11


def oracle_em(Y, X0, S0, params, dtype=np.float64, rounds=EM_ROUNDS, sweeps=EM_SWEEPS, lr=EM_LR,
              update=EM_UPDATE, variant="good"):
    """EM on the CPU: `sweeps` oracle sweeps (ame_oracle.sweep_stats, arithmetic
    in `dtype`) then the fp64 M-step on the resulting state, `rounds` times.
    Returns the per-round parameter dictionaries (fp64)."""
    import ame_oracle as O
    n, T, d = X0.shape
    r = (d - 2) // 2
    X = np.array(X0, dtype=dtype)
    S = np.array(S0, dtype=dtype)
    p = {k: np.array(params[k], dtype=np.float64) for k in PARAMS}
    out = []
    for _ in range(rounds):
        q = dict(p, R_inv=np.linalg.inv(p["R"]))
        for _ in range(sweeps):
            O.sweep_stats(np.asarray(Y, dtype), X, S, q, variant, lr)
        st = statistics(X, S, r, Y)
        new = m_step(st, p, n, T, update)
        out.append(dict(new, objective_before=objective(st, p, n, T),
                        objective_after=objective(st, new, n, T)))
        p = new
    return out


def param_deviation(a, b):
    """max |a - b| over Phi, Q and R of two parameter dictionaries."""
    return {k: float(np.abs(a[k] - b[k]).max()) for k in ("Phi", "Q", "R")}
