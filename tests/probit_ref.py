"""fp64 numpy / scipy reference of the probit fit and the Bernoulli scoring of
binary networks (test-only; imports nothing from ame_amd except through
missing_ref.make_case).  The sweep is ame_oracle's, run on a working network.

Model: z_pair = (z_ij, z_ji) ~ N(mu_pair, [[1, rho], [rho, 1]]), y = 1[z > 0],
s = 2 y - 1.  q(z_ij) q(z_ji) are truncated normals that depend on q(x) only
through m = E[mu_pair].  With sd = sqrt(1 - rho^2), kappa = phi / Phi:

    e = m + s kappa(s m); then K times
    eta0 = m0 + rho (e1 - m1);  e0 = eta0 + s0 sd kappa(s0 eta0 / sd)
    eta1 = m1 + rho (e0 - m0);  e1 = eta1 + s1 sd kappa(s1 eta1 / sd)

and with d = e - m, x_a = s_a eta_a / sd the pair's part of the bound is

    l = 1/2 log(1 - rho^2) - 1/2 d' R^-1 d + sum_a [log Phi(x_a) + 1/2 kappa(x_a)^2].

The working network holds each row's own-perspective mean (missing_ref.own_values)
plus d; a hidden pair gets d = 0 and is left out of every sum.  B is (n, n, T)
bool, B[i, j, t] = the tie i -> j; arrays of pair values are in Y's layout
(n, n, [T,] 2) = (value of ij, value of ji).
"""
import functools
import math

import numpy as np
from scipy.special import erfc, erfcx

import missing_ref as MR
import predictive_ref as PR

K_STEPS = 2                 # AME_PROBIT_STEPS
N_STATS, N_SUMS = 4, 6      # AME_PROBIT_STATS, AME_PROBIT_SUMS
SQRT_2_PI = math.sqrt(2.0 / math.pi)
OBSERVED, HIDDEN = MR.OBSERVED, MR.HIDDEN


# ---------------------------------------------------------------------------
# the normal-distribution functions, by the formulas of include/ame_amd.h
# ---------------------------------------------------------------------------
def kappa(x):
    """phi(x) / Phi(x) = sqrt(2 / pi) / erfcx(-x / sqrt 2); 0 where erfcx overflows."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return SQRT_2_PI / erfcx(-x * math.sqrt(0.5))


def log_phi(x):
    """log Phi(x): log(erfcx(-x / sqrt 2) / 2) - x^2 / 2 for x < 0, log1p(-erfc(x / sqrt 2) / 2) otherwise."""
    x = np.asarray(x, np.float64)
    t = x * math.sqrt(0.5)
    neg = x < 0
    tn = np.where(neg, t, 0.0)
    lo = np.log(0.5 * erfcx(-tn)) - tn * tn
    hi = np.log1p(-0.5 * erfc(np.where(neg, 0.0, t)))
    return np.where(neg, lo, hi)


def phi_cdf(x):
    return 0.5 * erfc(-np.asarray(x, np.float64) * math.sqrt(0.5))


# ---------------------------------------------------------------------------
# the recursion and the bound
# ---------------------------------------------------------------------------
def recursion(m, s, rho, K=K_STEPS):
    """m, s (..., 2) -> (e, x, kap): the means of the two truncated normals after K
    alternating steps, x_a = s_a eta_a / sd of the last steps and kappa(x_a)."""
    m = np.asarray(m, np.float64)
    s = np.asarray(s, np.float64)
    sd = math.sqrt((1.0 - rho) * (1.0 + rho))
    m0, m1, s0, s1 = m[..., 0], m[..., 1], s[..., 0], s[..., 1]
    e0, e1 = m0 + s0 * kappa(s0 * m0), m1 + s1 * kappa(s1 * m1)
    x0, x1 = s0 * m0, s1 * m1          # K = 0: q = TN(m, 1), only consistent at rho = 0
    k0, k1 = kappa(x0), kappa(x1)
    for _ in range(K):
        eta0 = m0 + rho * (e1 - m1)
        x0 = s0 * eta0 / sd
        k0 = kappa(x0)
        e0 = eta0 + s0 * sd * k0
        eta1 = m1 + rho * (e0 - m0)
        x1 = s1 * eta1 / sd
        k1 = kappa(x1)
        e1 = eta1 + s1 * sd * k1
    return np.stack([e0, e1], -1), np.stack([x0, x1], -1), np.stack([k0, k1], -1)


def bound(m, s, rho, K=K_STEPS):
    """l per pair (K >= 1): the mean-field bound on log P(orthant s) for the q the K steps produce."""
    m = np.asarray(m, np.float64)
    e, x, k = recursion(m, s, rho, K)
    d = e - m
    om = (1.0 - rho) * (1.0 + rho)
    quad = (d[..., 0] ** 2 - 2.0 * rho * d[..., 0] * d[..., 1] + d[..., 1] ** 2) / om
    return 0.5 * math.log(om) - 0.5 * quad + (log_phi(x) + 0.5 * k * k).sum(-1)


def signs(B_t):
    """(n, n) bool ties of one slice -> (n, n, 2) signs in Y's layout (s_ij, s_ji)."""
    B_t = np.asarray(B_t, bool)
    return np.where(np.stack([B_t, B_t.T], -1), 1.0, -1.0)


def y_of(B):
    """(n, n, T) ties -> the (n, n, T, 2) 0 / 1 network model.set_binary stores in Y."""
    B = np.asarray(B, bool)
    return np.stack([B, B.transpose(1, 0, 2)], -1).astype(np.float64)


# ---------------------------------------------------------------------------
# the working network and ame_probit_fill's statistics
# ---------------------------------------------------------------------------
def corrections(X_t, B_t, rho, r, K=K_STEPS, mean=None):
    """(m, d), each (n, n, 2), of one slice; `mean` replaces E[mu] of X_t.  The
    recursion runs on the pairs i < j (entry ij first); [j, i] holds [i, j] swapped."""
    m = MR.mean_mu(X_t, r) if mean is None else np.asarray(mean, np.float64)
    e, _, _ = recursion(m, signs(B_t), rho, K)
    d = e - m
    il = np.tril_indices(m.shape[0], -1)
    d[il[0], il[1]] = d[il[1], il[0]][:, ::-1]
    return m, d


def working_network(X, B, mask, rho, dtype=np.float64, scheme="own"):
    """(n, n, T, 2) in `dtype` from means X (n, T, d).  scheme "own": own-perspective
    mean (formed in `dtype`) + d (fp64), rounded once; "ez": E[z] in both rows (the
    textbook choice); "pm1": the +-1 coding.  Hidden pairs hold the own-perspective
    mean under every scheme."""
    X = np.asarray(X)
    n, T, d = X.shape
    r = (d - 2) // 2
    hid = MR.clean(mask) if mask is not None else np.zeros((n, n, T), bool)
    Yw = np.zeros((n, n, T, 2), dtype)
    Xd = X.astype(dtype)
    for t in range(T):
        own = MR.own_values(Xd[:, t], r)
        if scheme == "pm1":
            yw = signs(B[:, :, t])
        else:
            m, dd = corrections(Xd[:, t].astype(np.float64), B[:, :, t], rho, r)
            yw = own.astype(np.float64) + dd if scheme == "own" else m + dd
        yw = np.asarray(yw, np.float64)
        yw[hid[:, :, t]] = own[hid[:, :, t]]
        Yw[:, :, t] = yw.astype(dtype)
    return Yw


def stat_rows(X, B, mask, rho, means=None):
    """ame_probit_fill's per-slice rows (T, 4) over the observed pairs i < j and
    the sums of |summand| (T, 4): pairs, sum l, sum over both entries of
    (y - Phi(m))^2, sum over both entries of log Phi(s m).  `means` (T, n, n, 2)
    replaces E[mu] of X."""
    X = np.asarray(X, np.float64)
    n, T, d = X.shape
    r = (d - 2) // 2
    hid = MR.clean(mask) if mask is not None else np.zeros((n, n, T), bool)
    iu = np.triu_indices(n, 1)
    rows, mag = np.zeros((T, N_STATS)), np.zeros((T, N_STATS))
    for t in range(T):
        o = ~hid[iu[0], iu[1], t]
        i, j = iu[0][o], iu[1][o]
        m = (MR.mean_mu(X[:, t], r) if means is None else np.asarray(means[t], np.float64))[i, j]
        s = signs(B[:, :, t])[i, j]
        l = bound(m, s, rho)
        f = (s > 0) - phi_cdf(m)
        lp = log_phi(s * m)
        rows[t] = (len(i), l.sum(), (f * f).sum(), lp.sum())
        mag[t] = (len(i), np.abs(l).sum(), (f * f).sum(), np.abs(lp).sum())
    return rows, mag


# ---------------------------------------------------------------------------
# ame_probit_score's sums
# ---------------------------------------------------------------------------
def score_rows(X, S, r, B, mask=None, select=0):
    """Per-slice rows (T, 6) over the selected pairs i < j, both entries: pairs,
    sum log pi(y), sum (y - pi)^2, entries with (pi > 1/2) == y, ties, sum pi, with
    pi = Phi(E[mu] / sqrt(1 + V0)); the sums of |summand| (T, 6); and per slice
    the number of entries whose pi lies within 1e-6 of 1/2."""
    X = np.asarray(X, np.float64)
    n, T, _ = X.shape
    iu = np.triu_indices(n, 1)
    rows, mag, near = np.zeros((T, N_SUMS)), np.zeros((T, N_SUMS)), np.zeros(T, int)
    msk = np.zeros((n, n, T), bool) if mask is None else mask
    for t in range(T):
        sel = MR._subset(msk[:, :, t], select, iu)
        i, j = iu[0][sel], iu[1][sel]
        mean, V0, _ = PR.moments(X[:, t], np.asarray(S)[:, t], r)
        tt = np.stack([mean[i, j, 0] / np.sqrt(1.0 + V0[i, j]), mean[i, j, 1] / np.sqrt(1.0 + V0[j, i])], -1)
        y = np.stack([B[i, j, t], B[j, i, t]], -1).astype(bool)
        pi = phi_cdf(tt)
        lp = log_phi(np.where(y, tt, -tt))
        rows[t] = (len(i), lp.sum(), ((y - pi) ** 2).sum(), ((pi > 0.5) == y).sum(), y.sum(), pi.sum())
        mag[t] = (len(i), np.abs(lp).sum(), ((y - pi) ** 2).sum(), 2 * len(i), y.sum(), pi.sum())
        near[t] = int((np.abs(pi - 0.5) <= 1e-6).sum())
    return rows, mag, near


def check_dict(rows):
    """predictive_check's dictionary of a binary model from score_rows' rows."""
    ent = 2.0 * rows[:, 0]
    return dict(pairs=rows[:, 0], log_score=rows[:, 1], brier=rows[:, 2] / ent, accuracy=rows[:, 3] / ent,
                base_rate=rows[:, 4] / ent, mean_prob=rows[:, 5] / ent)


# ---------------------------------------------------------------------------
# the ELBO terms and the fit
# ---------------------------------------------------------------------------
def binary_terms(B, X_mean, X_cov, params, variant, mask, rho):
    """dict(loglik, prior0, trans, entropy, elbo, recon) of a binary model: loglik =
    sum l over the observed pairs minus half the reference's heuristic variance
    term in missing_ref.masked_terms' degree-weighted form; recon = the mean of
    (y - Phi(m))^2 over the observed entries; the other terms are the oracle's."""
    import ame_oracle as O
    Xm = np.asarray(X_mean, np.float64)
    Sc = np.asarray(X_cov, np.float64)
    n, T, d = Xm.shape
    hid = MR.clean(mask) if mask is not None else np.zeros((n, n, T), bool)
    rows, _ = stat_rows(Xm, B, hid, rho)
    Ri = np.asarray(params["R_inv"], np.float64)
    if variant == "naive":
        corr = 0.0
    else:
        tr = np.trace(Sc, axis1=2, axis2=3)
        deg = (n - 1) - hid.sum(1)
        corr = 0.1 * float(np.trace(Ri)) / d * float((deg * tr).sum())
    loglik = float(rows[:, 1].sum()) - 0.5 * corr
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    prior0 = O.log_prior_initial(Xm, Sc, p64)
    trans = O.log_prior_transitions(Xm, Sc, p64)
    ent = O.entropy(Sc)
    return dict(loglik=loglik, prior0=prior0, trans=trans, entropy=ent, elbo=loglik + prior0 + trans + ent,
                recon=float(rows[:, 2].sum()) / (2.0 * float(rows[:, 0].sum())))


def probit_params(params, rho):
    """`params` with R / R_inv replaced by the rho matrix (what model.set_binary sets)."""
    R = np.array([[1.0, rho], [rho, 1.0]])
    return dict(params, R=R, R_inv=np.linalg.inv(R))


def oracle_fit(B, X0, S0, params, mask, rho, variant="good", lr=0.5, sweeps=10, dtype=np.float64,
               history=False, scheme="own"):
    """`sweeps` iterations of (working_network from the current means, then
    ame_oracle.sweep_stats on it), state and working network held in `dtype`.
    `params` must carry the rho matrix (probit_params).  Returns dict(X, S[,
    terms: binary_terms after every sweep]); stops early with diverged=<sweep>
    once a mean is not finite or exceeds 1e6."""
    import ame_oracle as O
    X = np.array(X0, dtype=dtype)
    S = np.array(S0, dtype=dtype)
    q = {k: np.asarray(v, np.float64) for k, v in params.items()}
    terms, out = [], {}
    for it in range(sweeps):
        Yw = working_network(X, B, mask, rho, dtype, scheme)
        O.sweep_stats(Yw, X, S, q, variant, lr)
        if not np.isfinite(X).all() or np.abs(X).max() > 1e6:
            out["diverged"] = it
            break
        if history:
            terms.append(binary_terms(B, X, S, q, variant, mask, rho))
    out.update(X=X, S=S)
    if history:
        out["terms"] = terms
    return out


# ---------------------------------------------------------------------------
# shared inputs
# ---------------------------------------------------------------------------
def draw_ties(mu, rho, rng):
    """B (n, n, T) = 1[mu + eps > 0], eps ~ N(0, [[1, rho], [rho, 1]]) per pair i < j; mu (n, n, T, 2)."""
    n, _, T, _ = mu.shape
    L = np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]]))
    iu = np.triu_indices(n, 1)
    Z = np.zeros_like(mu)
    for t in range(T):
        z = mu[iu[0], iu[1], t] + rng.standard_normal((len(iu[0]), 2)) @ L.T
        Z[iu[0], iu[1], t] = z
        Z[iu[1], iu[0], t] = z[:, ::-1]
    return Z[..., 0] > 0


def make_binary_case(n, T, r, rho, seed, variant="good", lr=0.5, tie_seed=5):
    """missing_ref.make_case with ties drawn from the generated latent states:
    dict(model, B, mu_true, X0, S0, params (with the rho matrix))."""
    c = MR.make_case(n, T, r, seed=seed, variant=variant, lr=lr)
    Xt = c["model"].X.numpy().astype(np.float64)
    mu = np.stack([MR.mean_mu(Xt[:, t], r) for t in range(T)], 2)
    B = draw_ties(mu, rho, np.random.default_rng(tie_seed))
    return dict(model=c["model"], B=B, mu_true=mu, X0=c["X0"], S0=c["S0"], params=probit_params(c["params"], rho))


@functools.lru_cache(maxsize=None)
def quality_case(rho, scheme, sweeps=60, lr=0.5):
    """n = 40, T = 4, r = 2, "good", 20 % of the pairs held out, `sweeps` oracle
    sweeps in fp64 under `scheme`: dict(held_out: the mean over the held-out
    entries of log Phi(s E[mu]), corr: the correlation of E[mu] with the truth
    over the observed entries, abs_mu: their mean |E[mu]|, abs_true, diverged)."""
    n, T, r = 40, 4, 2
    c = make_binary_case(n, T, r, rho, seed=31, lr=lr)
    mask = MR.random_mask(n, T, 0.2, seed=2)
    fit = oracle_fit(c["B"], c["X0"], c["S0"], c["params"], mask, rho, "good", lr, sweeps, scheme=scheme)
    X = fit["X"]
    mu = np.stack([MR.mean_mu(X[:, t], r) for t in range(T)], 2)
    hid = np.broadcast_to(MR.clean(mask)[..., None], mu.shape)
    obs = np.broadcast_to((~np.eye(n, dtype=bool)[:, :, None] & ~MR.clean(mask))[..., None], mu.shape)
    s = np.where(y_of(c["B"]) > 0, 1.0, -1.0)
    with np.errstate(all="ignore"):
        ll = log_phi(s * mu)
        return dict(held_out=float(ll[hid].mean()), corr=float(np.corrcoef(mu[obs], c["mu_true"][obs])[0, 1]),
                    abs_mu=float(np.abs(mu[obs]).mean()), abs_true=float(np.abs(c["mu_true"][obs]).mean()),
                    diverged=fit.get("diverged"))
