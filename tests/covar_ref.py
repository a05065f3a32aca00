"""fp64 numpy reference of the dyadic-covariate regression term (test-only;
imports nothing from ame_amd except in make_model / cpu_runs, which build the
end-to-end case, and through gpu_inputs' network).

    y_ij,t = mu_ij,t + sum_k beta_k w_k,ij,t + eps,   eps ~ N(0, R)

W is (p, n, n, T, 2) in Y's layout per covariate.  With the residual
y~ = y - sum_k beta_k w_k and e = y~ - E_q[mu_ij], per slice over i < j with
Y[i, j, t] and W[k, i, j, t] as the observation 2-vectors:

    G_t[k][a][b]    = sum w_k[a] e[b]
    H_t[k][l][a][b] = sum w_k[a] w_l[b]
    (sum_ab Rinv[a][b] H[k][l][a][b]) delta = sum_ab Rinv[a][b] G[k][a][b]
    Rss(beta + delta) = Rss - sum_k delta_k (G_k + G_k') + sum_kl delta_k delta_l H[k][l]
"""
import functools

import numpy as np

import mstep_ref as M

EPS = 2.0 ** -52


def make_w(n, T, p, seed=0):
    """iid N(0, 1) per dyad i < j and component, swap-consistent (W[k, j, i] =
    swap(W[k, i, j])), zero diagonal, fp32, (p, n, n, T, 2)."""
    rng = np.random.default_rng(77 + 1000 * n + 10 * T + p + 7919 * seed)
    W = np.zeros((p, n, n, T, 2), dtype=np.float32)
    iu = np.triu_indices(n, 1)
    w = rng.standard_normal((p, len(iu[0]), T, 2)).astype(np.float32)
    W[:, iu[0], iu[1]] = w
    W[:, iu[1], iu[0]] = w[..., ::-1]
    return W


def gpu_inputs(case):
    """(X, Y, W, beta) of a direct kernel case (n, T, r, p) of
    tests/test_gpu_covar.py: make_state's means, mstep_ref.gpu_network's network,
    make_w's covariates and a beta of scale 0.5.  What its _Device uploads, and
    what tests/test_covar_ref.py measures the reference's sensitivity on."""
    import predictive_ref as PR
    n, T, r, p = case
    X, _ = PR.make_state(n, T, r)
    beta = np.random.default_rng(p + n).standard_normal(p) * 0.5
    return X, M.gpu_network(n, T, r), make_w(n, T, p), beta


def effect(W, beta):
    """sum_k beta_k W_k in fp64, k ascending from zero."""
    s = np.zeros(W.shape[1:], dtype=np.float64)
    for k in range(W.shape[0]):
        s += np.float64(beta[k]) * W[k].astype(np.float64)
    return s


def resid(Y, W, beta):
    """The residual network as the device forms it: fp64, rounded once to fp32."""
    return (np.asarray(Y, np.float32).astype(np.float64) - effect(np.asarray(W, np.float32), beta)).astype(np.float32)


def mean_mu(X_t, r):
    """E_q[mu_ij] of one slice from the means (n, d): (n, n, 2)."""
    X_t = np.asarray(X_t, np.float64)
    a, b, u, v = X_t[:, 0], X_t[:, 1], X_t[:, 2:2 + r], X_t[:, 2 + r:2 + 2 * r]
    m0 = a[:, None] + b[None, :] + np.einsum("ik,jk->ij", u, v)
    return np.stack([m0, m0.T], axis=-1)


def gh_rows(X, r, Yres, W):
    """X (n, T, d), Yres (n, n, T, 2), W (p, n, n, T, 2) -> G (T, p, 2, 2),
    H (T, p, p, 2, 2) and the sums of |summand| of every entry."""
    X = np.asarray(X, np.float64)
    Yres = np.asarray(Yres, np.float64)
    W = np.asarray(W, np.float64)
    p, n, _, T, _ = W.shape
    iu = np.triu_indices(n, 1)
    G, Gm = np.zeros((T, p, 2, 2)), np.zeros((T, p, 2, 2))
    H, Hm = np.zeros((T, p, p, 2, 2)), np.zeros((T, p, p, 2, 2))
    for t in range(T):
        e = Yres[iu[0], iu[1], t] - mean_mu(X[:, t], r)[iu[0], iu[1]]      # (N, 2)
        w = W[:, iu[0], iu[1], t]                                        # (p, N, 2)
        G[t] = np.einsum("kna,nb->kab", w, e)
        Gm[t] = np.einsum("kna,nb->kab", np.abs(w), np.abs(e))
        H[t] = np.einsum("kna,lnb->klab", w, w)
        Hm[t] = np.einsum("kna,lnb->klab", np.abs(w), np.abs(w))
    return G, Gm, H, Hm


def beta_delta(G, H, R):
    Ri = np.linalg.inv(R)
    Ri = 0.5 * (Ri + Ri.T)
    A = np.einsum("ab,klab->kl", Ri, H)
    b = np.einsum("ab,kab->k", Ri, G)
    return np.linalg.solve(0.5 * (A + A.T), b)


def rss_at(Rss, G, H, delta):
    return (Rss - np.einsum("k,kab->ab", delta, G + np.swapaxes(G, 1, 2))
            + np.einsum("k,l,klab->ab", delta, delta, H))


def statistics(X, S, r, Yres, W, beta):
    """The M-step statistics on the residual network Yres = Y - sum_k beta_k W_k
    (taken at `beta`), with G, H and that beta."""
    Yres = np.asarray(Yres, np.float64)
    st = M.statistics(X, S, r, Yres)
    G, _, H, _ = gh_rows(X, r, Yres, W)
    st.update(G=G.sum(0), H=H.sum(0), beta=np.array(beta, dtype=np.float64))
    return st


def objective(st, p, n, T):
    """F at p (with p["beta"]): Rss taken at that beta."""
    delta = np.asarray(p["beta"], np.float64) - st["beta"]
    return M.objective(dict(st, Rss=rss_at(st["Rss"], st["G"], st["H"], delta)), p, n, T)


def m_step(st, p, n, T, update=("beta", "R")):
    """beta first (at the old R), then the other updates with Rss at the new beta."""
    beta = np.array(p["beta"], dtype=np.float64)
    delta = beta - st["beta"]
    if "beta" in update:
        delta = beta_delta(st["G"], st["H"], np.asarray(p["R"], np.float64))
        beta = st["beta"] + delta
    st2 = dict(st, Rss=rss_at(st["Rss"], st["G"], st["H"], delta))
    new = M.m_step(st2, p, n, T, tuple(u for u in update if u != "beta"))
    new["beta"] = beta
    return new


# ---- the end-to-end experiment (tests/test_gpu_covar.py, tests/test_covar_ref.py) ----
EM_SHAPE = (48, 6, 2)        # n, T, r
EM_P = 2
EM_BETA = (0.7, -0.4)
EM_SEED = 4
EM_ROUNDS, EM_SWEEPS = 4, 5
EM_LR = 0.5
EM_UPDATE = ("beta", "R")


def make_model():
    """Data generated with the true beta; the model then starts EM from beta = 0."""
    import torch
    from ame_amd import TemporalAMEModel
    n, T, r = EM_SHAPE
    m = TemporalAMEModel(n, T, r, seed=EM_SEED)
    W = make_w(n, T, EM_P, seed=EM_SEED)
    m.set_covariates(torch.from_numpy(W), beta=EM_BETA)
    m.generate_data_fast(seed=EM_SEED + 1)
    m.set_covariates(torch.from_numpy(W))
    return m


def oracle_em(Y, W, X0, S0, params, beta0, dtype=np.float64, rounds=EM_ROUNDS, sweeps=EM_SWEEPS,
              lr=EM_LR, update=EM_UPDATE, variant="good"):
    """EM on the CPU as mstep_ref.oracle_em runs it, on the residual network:
    `sweeps` oracle sweeps in `dtype` on Y - sum_k beta_k W_k (held in `dtype`,
    as the device holds it in fp32), then the fp64 M-step."""
    import ame_oracle as O
    n, T, d = X0.shape
    r = (d - 2) // 2
    X = np.array(X0, dtype=dtype)
    S = np.array(S0, dtype=dtype)
    p = {k: np.array(params[k], dtype=np.float64) for k in M.PARAMS}
    p["beta"] = np.array(beta0, dtype=np.float64)
    out = []
    for _ in range(rounds):
        q = dict(p, R_inv=np.linalg.inv(p["R"]))
        Yres = (np.asarray(Y, np.float64) - effect(W, p["beta"])).astype(dtype)
        for _ in range(sweeps):
            O.sweep_stats(Yres, X, S, q, variant, lr)
        st = statistics(X, S, r, Yres, W, p["beta"])
        new = m_step(st, p, n, T, update)
        out.append(dict(new, objective_before=objective(st, p, n, T),
                        objective_after=objective(st, new, n, T)))
        p = new
    return out


def relative_deviation(a, b):
    """max over beta and R of max|a - b| / max|a|."""
    return max(float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max() / np.abs(np.asarray(a[k])).max())
               for k in ("beta", "R"))


@functools.lru_cache(maxsize=None)
def cpu_runs():
    """fp64 oracle EM and the same EM on fp32 arrays, from the initial state a
    VI instance of make_model() starts with."""
    from ame_amd import TemporalAMEStructuredMFVI
    m = make_model()
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=EM_LR)
    X0 = vi.X_mean.numpy().astype(np.float64)
    S0 = vi.X_cov.numpy().astype(np.float64)
    Y = m.Y.numpy().astype(np.float64)
    W = m.W.numpy()
    p = {k: getattr(m, k).numpy().astype(np.float64) for k in M.PARAMS}
    b0 = np.zeros(EM_P)
    return dict(em64=oracle_em(Y, W, X0, S0, p, b0), em32=oracle_em(Y, W, X0, S0, p, b0, dtype=np.float32))


def contraction_probe():
    """One element (p = 2, y = 0) on which a fused multiply-add and the
    separate multiply-then-add of y - sum_k beta_k w_k round to different fp32
    values.  u = 2^-52.  w = (-1, 3); beta_1 = m 2^-54 with m = 1 mod 4, so
    3 beta_1 = T + 3u/4 with T a multiple of u: rounded on its own the product
    becomes T + u.  beta_0 = -(Mid - 3u/8 - T) with Mid = 1.25 + 2^-24, the
    midpoint of two fp32 values.  Then s is Mid + 3u/8 exactly: fused it rounds to
    Mid, an fp32 tie that goes to the even 1.25; unfused it is fl(Mid + 5u/8) =
    Mid + u, which goes to 1.25 + 2^-23.  Returns (w, beta, unfused, fused) with
    the two results as np.float32, evaluated exactly with fractions."""
    from fractions import Fraction as F
    u = F(1, 2 ** 52)
    mid = F(5, 4) + F(1, 2 ** 24)
    m = (int(0.47 * 2 ** 54) // 4) * 4 + 1
    b1 = F(m, 2 ** 54)
    T = (3 * b1) // u * u
    assert 3 * b1 - T == 3 * u / 4
    s0 = mid - 3 * u / 8 - T
    beta = np.array([float(-s0), float(b1)])
    assert F(beta[0]) == -s0 and F(beta[1]) == b1            # both exactly representable
    w = np.array([-1.0, 3.0], dtype=np.float32)
    fl = lambda x: F(float(x))                               # round to nearest fp64
    exact = [F(float(b)) * F(float(x)) for b, x in zip(beta, w)]
    s_unfused = fl(fl(F(0) + fl(exact[0])) + fl(exact[1]))
    s_fused = fl(fl(F(0) + exact[0]) + exact[1])
    assert s_fused == mid and s_unfused == mid + u
    return w, beta, np.float32(float(-s_unfused)), np.float32(float(-s_fused))
