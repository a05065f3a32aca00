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


def bound(m, s, rho, K=K_STEPS, elementary=False):
    """l per pair (K >= 1): the mean-field bound on log P(orthant s) for the q the K
    steps produce; with `elementary`, also the sum of the absolute values of its
    terms |log(1 - rho^2) / 2| + quad / 2 + sum_a [|log Phi(x_a)| + kappa(x_a)^2 / 2]."""
    m = np.asarray(m, np.float64)
    e, x, k = recursion(m, s, rho, K)
    d = e - m
    om = (1.0 - rho) * (1.0 + rho)
    quad = (d[..., 0] ** 2 - 2.0 * rho * d[..., 0] * d[..., 1] + d[..., 1] ** 2) / om
    lp = log_phi(x)
    l = 0.5 * math.log(om) - 0.5 * quad + (lp + 0.5 * k * k).sum(-1)
    if elementary:
        return l, abs(0.5 * math.log(om)) + 0.5 * quad + (np.abs(lp) + 0.5 * k * k).sum(-1)
    return l


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


def stat_rows(X, B, mask, rho, means=None, K=K_STEPS, elementary=False):
    """ame_probit_fill's per-slice rows (T, 4) over the observed pairs i < j and
    the sums of |summand| (T, 4): pairs, sum l, sum over both entries of
    (y - Phi(m))^2, sum over both entries of log Phi(s m).  `means` (T, n, n, 2)
    replaces E[mu] of X.  With `elementary` the second column of the magnitudes
    is the sum of |elementary term| of l (bound), which does not shrink where the
    terms of one pair cancel."""
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
        l, el = bound(m, s, rho, K, elementary=True)
        f = (s > 0) - phi_cdf(m)
        lp = log_phi(s * m)
        rows[t] = (len(i), l.sum(), (f * f).sum(), lp.sum())
        mag[t] = (len(i), (el if elementary else np.abs(l)).sum(), (f * f).sum(), np.abs(lp).sum())
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


def state_ties(X, case, ties="drawn"):
    """(n, n, T) ties for the means X (n, T, d) of predictive_ref.make_state(*case):
    "drawn" 1[mu + N(0, 1) > 0], each direction on its own (B is not symmetric), which
    almost always agrees with the mean; "against" the same draw with both ties of
    every third pair i < j (in row order) set against their means."""
    assert ties in ("drawn", "against")
    n, T, r = case
    X64 = X.astype(np.float64)
    rng = np.random.default_rng(100 + n + 7 * T + r)
    mu = np.stack([MR.mean_mu(X64[:, t], r)[:, :, 0] for t in range(T)], 2)
    B = (mu + rng.standard_normal(mu.shape)) > 0
    if ties == "against":
        iu = np.triu_indices(n, 1)
        i, j = iu[0][::3], iu[1][::3]
        B[i, j], B[j, i] = mu[i, j] <= 0, mu[j, i] <= 0
    B[np.arange(n), np.arange(n)] = False
    return B


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


# ---------------------------------------------------------------------------
# the tail grid: inputs whose pair means the kernels form exactly
# ---------------------------------------------------------------------------
# Expected values come from tests/golden/probit_tails.npz (mpmath, written by
# tests/golden/make_golden_probit_tails.py), not from the formulas above.
GRID_SEED = 20240
GRID_T = 6
GRID_SHAPES = (20, 65)
GRID_RHOS = (0.0, 0.5, -0.7, 0.95, -0.95)
GRID_MASKS = ("none", "random30")
GRID_COVS = ("unit", "scaled")          # t = m; t = m or m / 2 by the row node
GRID_SELECTS = (0, OBSERVED, HIDDEN)
GRID_STEP = 2.0 ** -10
# m of slice 5's pairs (i, j) with i = j mod 10, both entries: the smallest
# means; either side of x = 37.66 where erfcx(x / sqrt 2) overflows (the branch
# x >= 0: kappa = 0 from there on); the same below zero; the largest |m| the
# grid can hold (Phi(-38) = 3e-316 is subnormal, Phi(-38.5) = 0 is out of reach
# of |a|, |b| <= 19 as a mean, but the recursion's arguments pass it for every
# rho != 0); either side of x = 8.29 where Phi rounds to 1.  Odd multiples of 2^-10.
GRID_SPECIAL = (GRID_STEP, -GRID_STEP, 37.5 + GRID_STEP, 37.75 + GRID_STEP, -37.5 - GRID_STEP,
                -37.75 - GRID_STEP, 38.0 - GRID_STEP, -38.0 + GRID_STEP, 8.25 + GRID_STEP, 8.375 + GRID_STEP)
# The largest deviation of this module's scipy formulas from the fixture on the
# grid: |delta d| / (1 + |d|) per entry off the diagonal, |delta row| / sum |terms|
# per slice for stat[1..3] and the score sums [1], [2], [5].  Measured 3.550e-15
# (stat[2] of slice 3 at n = 20, every rho: Phi(-3.67) is already 13 times as
# sensitive to its argument as the argument is precise; d stays below 2.9e-15, l
# below 3e-16); test_probit_ref.py re-measures it and requires measured <=
# TAIL_TAU0 <= 1.5 measured.  The kernels' allowance is 4 x TAIL_TAU0.
TAIL_TAU0 = 3.6e-15


def _grid_values(rng, n, lo, hi, odd):
    """n multiples of 2^-10 in [lo, hi] with odd (a) or even (b) numerators: an
    odd plus an even numerator is never 0, so no mean is."""
    k = rng.integers(int(math.ceil(lo / GRID_STEP / 2)), int(math.floor(hi / GRID_STEP / 2)), n)
    return (2 * k + (1 if odd else 0)) * GRID_STEP


@functools.lru_cache(maxsize=None)
def _grid_inputs(n):
    rng = np.random.default_rng(GRID_SEED + n)
    T = GRID_T
    a, b = np.zeros((T, n)), np.zeros((T, n))
    sg = lambda: rng.choice([-1.0, 1.0], n)
    # 0: central, |m| <= 3
    a[0], b[0] = _grid_values(rng, n, -1.5, 1.5, True), _grid_values(rng, n, -1.5, 1.5, False)
    # 1: |m| in [3, 12], the sign of a mean is its row node's
    a[1], b[1] = sg() * _grid_values(rng, n, 5.5, 9.5, True), _grid_values(rng, n, -2.5, 2.5, False)
    # 2: m in [12, 38], every tie 0; 3: m in [-38, -3], every tie 0.  (With m < 0 in slice 2 every
    # Phi(m) of the slice would be below 1e-33, and fp64 cannot form such a value to better than
    # x^2 2^-53 of itself, the rounding of x / sqrt 2 alone: the slice's sum of pi would measure that.
    # With m > 0 in slice 3 its Brier sum would measure the cancellation in 1 - Phi(m) instead.)
    a[2], b[2] = _grid_values(rng, n, 6.0, 19.0, True), _grid_values(rng, n, 6.0, 19.0, False)
    a[3], b[3] = -_grid_values(rng, n, 1.5, 19.0, True), -_grid_values(rng, n, 1.5, 19.0, False)
    # 4: |m| in [3, 25], the sign of a mean is its row node's
    a[4], b[4] = sg() * _grid_values(rng, n, 9.0, 19.0, True), _grid_values(rng, n, -6.0, 6.0, False)
    # 5: a_k + b_k = GRID_SPECIAL[k], met by the pairs (i, j) with i = j = k mod 10
    sp = np.array(GRID_SPECIAL)
    half = np.round(sp / 2 / GRID_STEP / 2) * 2 * GRID_STEP            # even numerators
    k = np.arange(n) % len(sp)
    a[5], b[5] = (sp - half)[k], half[k]
    assert np.abs(a).max() <= 19.0 and np.abs(b).max() <= 19.0
    X = np.zeros((n, T, 4))
    X[:, :, 0], X[:, :, 1] = a.T, b.T
    means = np.stack([MR.mean_mu(X[:, t], 1) for t in range(T)])                 # (T, n, n, 2)
    off = ~np.eye(n, dtype=bool)
    assert (means[:, off] != 0).all() and np.array_equal(X, X.astype(np.float32))
    assert np.array_equal(means.astype(np.float32).astype(np.float64), means)     # exact in fp32 too
    pos = means[..., 0] > 0                                                       # (T, n, n): m_ij > 0
    B = np.zeros((n, n, T), bool)
    up = np.triu(np.ones((n, n), bool), 1)
    B[:, :, 0] = rng.random((n, n)) < 0.5
    for t in (1, 2):
        B[:, :, t] = ~pos[t]                      # every tie against its mean
    B[:, :, 3] = pos[3]                           # every tie with its mean
    B[:, :, 4] = np.where(up, ~pos[4], pos[4])    # ij (i < j) against, ji with
    B[:, :, 5] = rng.random((n, n)) < 0.5
    B[np.arange(n), np.arange(n)] = False
    sm = np.where(B.transpose(2, 0, 1), 1.0, -1.0) * means[..., 0]                # s m of every entry
    for t, (lo, hi) in enumerate(((-3, 3), (-12, -3), (-38, -12), (3, 38))):
        assert lo <= sm[t][off].min() and sm[t][off].max() <= hi, (t, sm[t][off].min(), sm[t][off].max())
    S = {"unit": np.zeros((n, T, 4, 4)), "scaled": np.zeros((n, T, 4, 4))}
    S["scaled"][:, :, 0, 0] = 3.0 * (rng.random((n, T)) < 0.5)
    mask = MR.random_mask(n, T, 0.3, seed=7)
    return dict(n=n, T=T, r=1, X=X.astype(np.float32), B=B, S={k: v.astype(np.float32) for k, v in S.items()},
                means=means, masks={"none": None, "random30": mask})


def grid_case(n, rho):
    """The tail grid at n nodes: r = 1, u = v = 0 and a, b multiples of 2^-10 with
    |a|, |b| <= 19, so every pair mean m0 = a_i + b_j, m1 = a_j + b_i is exact in
    fp32 (the score kernel's MFMA) and in fp64 (the fill kernel); no m is 0.  One
    slice per regime of s m: 0 central with random ties; 1 [-12, -3] and 2
    [-38, -12], every tie against its mean; 3 [3, 38], every tie with its mean; 4
    mixed, entry ij (i < j) against and entry ji with its mean; 5 GRID_SPECIAL
    with random ties.  The scoring covariances hold S_aa in {0, 3} and nothing
    else, so V0 = S_aa(row node) and t = m or m / 2 exactly.  dict(n, T, r, rho,
    X (n, T, 4) fp32, B (n, n, T), S {name: (n, T, 4, 4) fp32}, means (T, n, n, 2),
    masks {name: (n, n, T) or None}).  Shared by the recipe of the fixture and the tests."""
    return dict(_grid_inputs(n), rho=float(rho))


def grid_key(n, rho, what, *tags):
    """Name of an array of tests/golden/probit_tails.npz."""
    head = f"n{n}" if rho is None else f"n{n}_rho{GRID_RHOS.index(rho)}"
    return "_".join((head, what) + tuple(str(t) for t in tags))


def grid_reference(n, rho, K=K_STEPS):
    """What the fixture holds for (n, rho), by this module's scipy formulas: dict
    of grid_key -> array (the score sums do not depend on rho: they are under rho None)."""
    g = grid_case(n, rho)
    out = {}
    for name, mask in g["masks"].items():
        rows, mag = stat_rows(g["X"], g["B"], mask, rho, K=K, elementary=True)
        out[grid_key(n, rho, "stat", name)], out[grid_key(n, rho, "statmag", name)] = rows, mag
    if n == GRID_SHAPES[0]:
        X64 = g["X"].astype(np.float64)
        out[grid_key(n, rho, "d")] = np.stack([corrections(X64[:, t], g["B"][:, :, t], rho, 1, K)[1]
                                               for t in range(g["T"])], 2)
    for cov in GRID_COVS:
        for sel in GRID_SELECTS:
            rows, mag, _ = score_rows(g["X"], g["S"][cov], 1, g["B"], g["masks"]["random30"], sel)
            out[grid_key(n, None, "score", cov, sel)], out[grid_key(n, None, "scoremag", cov, sel)] = rows, mag
    return out


def grid_deviation(ref, fixture):
    """{grid_key: the deviation of `ref` from `fixture` as TAIL_TAU0 measures it}
    over the d, stat and score arrays of `ref`: per entry for d, per slice and
    column for the sums.  A value that is not finite deviates infinitely."""
    out = {}
    for k, v in ref.items():
        what = next(p for p in k.split("_") if p in ("d", "stat", "statmag", "score", "scoremag"))
        w = np.asarray(fixture[k], np.float64)
        with np.errstate(invalid="ignore"):
            if what == "d":     # the diagonal means nothing: the fixture holds 0 there
                dev = np.where(np.eye(w.shape[0], dtype=bool)[:, :, None, None], 0.0, np.abs(v - w) / (1.0 + np.abs(w)))
            elif what in ("stat", "score"):
                cols = [1, 2, 3] if what == "stat" else [1, 2, 5]
                mag = np.asarray(fixture[k.replace(what, what + "mag")], np.float64)[:, cols]
                dev = np.abs(v - w)[:, cols] / np.where(mag > 0, mag, 1.0)
            else:
                continue
        out[k] = np.where(np.isfinite(dev), dev, np.inf)
    return out
