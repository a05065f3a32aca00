"""fp64 numpy reference of ame_smooth (include/ame_amd.h): each node's exact
Gaussian posterior across time given the other nodes' means (test-only).

For node i, with the blocks the sweep uses,

    D_t = P_obs(i,t) + [t = 0] S0inv + [t > 0] Qinv + [t < T-1] PtQiP
    O   = -QiPhi          block (t, t-1);  O' is block (t-1, t)
    h_t = h_obs(i,t)
    Lambda_i = blocktridiag(D, O),  mu_i = Lambda_i^-1 h,  S_i = Lambda_i^-1

P_obs comes from oracle.observation_terms with the symmetric part of R_inv,
h_obs from the same function with R_inv as given.  Two independent routes:
`dense` builds the (T d) x (T d) matrix and inverts it; `recursion` is the block
forward / backward recursion.  `MUTATIONS` are the mistakes a kernel could make;
tests/test_smooth_ref.py checks that every test input tells them apart.
"""
import functools

import numpy as np

import ame_oracle as O_

CONST_KEYS = ("S0inv", "Qinv", "PtQiP", "QiPhi")
MUTATIONS = ("drop_O", "no_exclusion_P", "no_exclusion_h", "Qinv_at_0", "PtQiP_at_end", "transpose_O",
             "transpose_cross")
# the GPU parity shapes (n, T, r)
SHAPES = ((2, 3, 1), (9, 1, 1), (12, 2, 2), (65, 4, 5), (33, 5, 16), (130, 3, 23), (7, 3, 32))
PSETS = ("default", "gen")
# one small case per latent dim (d is a runtime value in the kernels: tile counts
# and the Gram kernel's instance change with r), `gen` parameters only
EVERY_R_SHAPES = tuple((5, 3, r) for r in range(1, 33))


def _obs_all(Y, X, R_inv, i, t):
    """observation_terms without the j != i exclusion (mutation only)."""
    n, T, d = X.shape
    r = (d - 2) // 2
    U, V = X[:, t, 2:2 + r], X[:, t, 2 + r:]
    E0 = np.zeros((n, d))
    E1 = np.zeros((n, d))
    E0[:, 0] = 1
    E0[:, 2:2 + r] = V
    E1[:, 1] = 1
    E1[:, 2 + r:] = U
    p, q, q2, s = R_inv[0, 0], R_inv[0, 1], R_inv[1, 0], R_inv[1, 1]
    P = p * (E0.T @ E0) + q * (E0.T @ E1) + q2 * (E1.T @ E0) + s * (E1.T @ E1)
    z = Y[i, :, t, :] @ R_inv.T
    return P, E0.T @ z[:, 0] + E1.T @ z[:, 1]


def blocks(Y, X, R_inv, consts, i, mutation=None):
    """D (T, d, d), O (d, d), h (T, d) of node i in fp64."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    R_inv = np.asarray(R_inv, np.float64)
    Rs = 0.5 * (R_inv + R_inv.T)
    n, T, d = X.shape
    D = np.zeros((T, d, d))
    h = np.zeros((T, d))
    for t in range(T):
        P, _ = O_.observation_terms(Y, X, Rs, i, t)
        _, ht = O_.observation_terms(Y, X, R_inv, i, t)
        if mutation == "no_exclusion_P":
            P, _ = _obs_all(Y, X, Rs, i, t)
        if mutation == "no_exclusion_h":
            _, ht = _obs_all(Y, X, R_inv, i, t)
        first = consts["Qinv"] if mutation == "Qinv_at_0" else consts["S0inv"]
        D[t] = P + (first if t == 0 else consts["Qinv"])
        if t < T - 1 or mutation == "PtQiP_at_end":
            D[t] += consts["PtQiP"]
        h[t] = ht
    Ob = -np.asarray(consts["QiPhi"], np.float64)
    if mutation == "drop_O":
        Ob = np.zeros_like(Ob)
    if mutation == "transpose_O":
        Ob = Ob.T.copy()
    return D, Ob, h


def joint_precision(D, Ob):
    T, d, _ = D.shape
    L = np.zeros((T * d, T * d))
    for t in range(T):
        L[t * d:(t + 1) * d, t * d:(t + 1) * d] = D[t]
        if t > 0:
            L[t * d:(t + 1) * d, (t - 1) * d:t * d] = Ob
            L[(t - 1) * d:t * d, t * d:(t + 1) * d] = Ob.T
    return L


def dense(D, Ob, h):
    """mu (T, d), S_tt (T, d, d), S_{t,t-1} (T, d, d; zero at t = 0), cond_2(Lambda)."""
    T, d, _ = D.shape
    L = joint_precision(D, Ob)
    S = np.linalg.inv(L)
    mu = (S @ h.reshape(-1)).reshape(T, d)
    Stt = np.stack([S[t * d:(t + 1) * d, t * d:(t + 1) * d] for t in range(T)])
    X = np.zeros((T, d, d))
    for t in range(1, T):
        X[t] = S[t * d:(t + 1) * d, (t - 1) * d:t * d]
    return mu, Stt, X, float(np.linalg.cond(L))


def recursion(D, Ob, h):
    """The same three outputs by the block forward / backward recursion."""
    T, d, _ = D.shape
    Ji = np.zeros((T, d, d))
    g = np.zeros((T, d))
    for t in range(T):
        if t == 0:
            J, g[t] = D[0], h[0]
        else:
            K = Ob @ Ji[t - 1]
            J = D[t] - K @ Ob.T
            g[t] = h[t] - K @ g[t - 1]
        Ji[t] = np.linalg.inv(J)
    S = np.zeros((T, d, d))
    X = np.zeros((T, d, d))
    mu = np.zeros((T, d))
    S[T - 1] = Ji[T - 1]
    mu[T - 1] = Ji[T - 1] @ g[T - 1]
    for t in range(T - 2, -1, -1):
        B = Ji[t] @ Ob.T
        S[t] = Ji[t] + B @ S[t + 1] @ B.T
        X[t + 1] = -S[t + 1] @ B.T
        mu[t] = Ji[t] @ g[t] - B @ mu[t + 1]
    return mu, S, X


def smooth(Y, X, R_inv, consts, route="dense", mutation=None, nodes=None):
    """All nodes: dict(mean (n, T, d), cov (n, T, d, d), cross (n, T, d, d), lag_sum
    (T, d, d), lag_abs (T, d, d) = sum_i |X_it|, cond (n,)), fp64."""
    n, T, d = X.shape
    nodes = range(n) if nodes is None else nodes
    k = len(nodes)
    out = dict(mean=np.zeros((k, T, d)), cov=np.zeros((k, T, d, d)), cross=np.zeros((k, T, d, d)),
               cond=np.zeros(k))
    for a, i in enumerate(nodes):
        D, Ob, h = blocks(Y, X, R_inv, consts, i, None if mutation == "transpose_cross" else mutation)
        if route == "dense":
            mu, S, Xc, cond = dense(D, Ob, h)
        else:
            mu, S, Xc = recursion(D, Ob, h)
            cond = np.nan
        if mutation == "transpose_cross":
            Xc = np.swapaxes(Xc, 1, 2).copy()
        out["mean"][a], out["cov"][a], out["cross"][a], out["cond"][a] = mu, S, Xc, cond
    out["lag_sum"] = out["cross"].sum(0)
    out["lag_abs"] = np.abs(out["cross"]).sum(0)
    return out


def tolerance(ref, T, d):
    """The bound of the GPU parity test per output array (n, ...):
    2^-24 |ref| + 8 (T d) 2^-52 cond_2(Lambda_i) scale_i, scale_i the largest
    |entry| of node i's array.  Returns dict(mean, cov, cross, lag_sum)."""
    out = {}
    solve = {}
    for k in ("mean", "cov", "cross"):
        a = ref[k]
        n = a.shape[0]
        scale = np.abs(a.reshape(n, -1)).max(1)
        s = 8.0 * T * d * 2.0 ** -52 * ref["cond"] * scale
        solve[k] = s
        out[k] = 2.0 ** -24 * np.abs(a) + s.reshape((n,) + (1,) * (a.ndim - 1))
    n = ref["cross"].shape[0]
    out["lag_sum"] = n * 2.0 ** -52 * ref["lag_abs"] + solve["cross"].sum()
    return out


def consts_of(model):
    """The fp64 constants exactly as the engine hands them to the kernels."""
    from ame_amd.engine import Constants
    C = Constants(model)
    return {k: getattr(C, k).numpy().copy() for k in CONST_KEYS}, C


@functools.lru_cache(maxsize=None)
def make_case(shape, pset="default"):
    """Inputs of one GPU parity case: fp32 means near the generating latents, a
    generated network with a non-zero diagonal (so a missing j != i exclusion in
    h_obs shows), the model's parameters (default, or the asymmetric `gen` set of
    generic_params), and the fp64 reference by the dense route."""
    import torch
    import generic_params as GP
    from ame_amd import TemporalAMEModel
    n, T, r = shape
    m = TemporalAMEModel(n, T, r, seed=5)
    if pset != "default":
        GP.assign(m, GP.generic_params(r, 1000 * n + 10 * r + T, GP.SETS[pset]))
    m.generate_data_fast(seed=9)
    rng = np.random.default_rng(100 * n + r)
    X = (m.X.numpy().astype(np.float64) + 0.2 * rng.standard_normal((n, T, 2 + 2 * r))).astype(np.float32)
    Y = m.Y.numpy().copy()
    idx = np.arange(n)
    Y[idx, idx] = rng.standard_normal((n, T, 2)).astype(np.float32)
    m.Y = torch.from_numpy(Y)
    consts, C = consts_of(m)
    R_inv = C.R_inv.numpy().copy()
    ref = smooth(Y, X, R_inv, consts)
    return dict(shape=shape, model=m, X=X, Y=Y, R_inv=R_inv, consts=consts, C=C, ref=ref)


# ---- EM with smoothed statistics (the experiment of em_case) ----
def smoothed_statistics(Y, X, r, params):
    """The M-step statistics with the smoothed means, marginals and lag-one
    blocks in place of the fit's: A10 gains sum_t>=1 lag_sum[t]."""
    import mstep_ref as M
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    Qinv = np.linalg.inv(p["Q"])
    S0 = M.blockdiag(p["Sigma"], p["Psi"])
    consts = dict(S0inv=np.linalg.inv(S0), Qinv=Qinv, PtQiP=p["Phi"].T @ Qinv @ p["Phi"],
                  QiPhi=Qinv @ p["Phi"])
    sm = smooth(Y, X, np.linalg.inv(p["R"]), consts)
    srows, _ = M.state_rows(sm["mean"], sm["cov"])
    srows[1:, 1] += sm["lag_sum"][1:]
    drows, _ = M.dyad_rows(sm["mean"], sm["cov"], r, Y)
    return M.combine(srows, drows), sm


def oracle_em_smoothed(Y, X0, S0, params, dtype=np.float64):
    """mstep_ref.oracle_em with the statistics of every round taken from the
    smoothed posterior of the state the sweeps reached.  The smoother reads the
    means as fp32 values (what the device holds) when dtype is fp32."""
    import mstep_ref as M
    n, T, d = X0.shape
    r = (d - 2) // 2
    X = np.array(X0, dtype=dtype)
    S = np.array(S0, dtype=dtype)
    p = {k: np.array(params[k], dtype=np.float64) for k in M.PARAMS}
    out = []
    for _ in range(M.EM_ROUNDS):
        q = dict(p, R_inv=np.linalg.inv(p["R"]))
        for _ in range(M.EM_SWEEPS):
            O_.sweep_stats(np.asarray(Y, dtype), X, S, q, "good", M.EM_LR)
        st, _ = smoothed_statistics(Y, X.astype(np.float64), r, p)
        new = M.m_step(st, p, n, T, M.EM_UPDATE)
        out.append(dict(new, objective_before=M.objective(st, p, n, T),
                        objective_after=M.objective(st, new, n, T)))
        p = new
    return out
