"""fp64 numpy reference of fitting and scoring with hidden dyads (test-only;
imports nothing from ame_amd except in make_case, which builds the end-to-end
inputs).  The sweep is ame_oracle's, run on a working network.

The reference's node update (structured_mf.py:289-326; ame_oracle.observation_terms)
treats y_ij as J_j x_i + noise with J_j x_i = (a_i + u_i.v_j, b_i + v_i.u_j).  A
hidden pair {i, j} contributes nothing to node i's update exactly when row i of
the working network holds J_j m_i:

    Yw[i, j, t] = (a_i + u_i.v_j, b_i + v_i.u_j)     (own_fill)

so the two rows of a hidden pair hold different values.  `mask` is (n, n, T)
bool, symmetric, True = hidden; the diagonal is ignored.
"""
import functools
import math

import numpy as np

import mstep_ref as M
import predictive_ref as PR

LOG2PI = math.log(2.0 * math.pi)
JITTER = 1e-6          # structured_mf.py: C = sym(P^-1) + 1e-6 I
OBSERVED, HIDDEN = 1, 2   # AME_MASK_OBSERVED / AME_MASK_HIDDEN


# ---------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------
def sym_mask(n, T, pairs):
    """Mask with the listed (i, j, t) pairs hidden (both orientations)."""
    m = np.zeros((n, n, T), dtype=bool)
    for i, j, t in pairs:
        assert i != j
        m[i, j, t] = m[j, i, t] = True
    return m


def random_mask(n, T, frac, seed=0):
    """Each unordered pair of each slice hidden independently with probability frac."""
    rng = np.random.default_rng(4000 + 100 * n + 10 * T + seed)
    iu = np.triu_indices(n, 1)
    m = np.zeros((n, n, T), dtype=bool)
    h = rng.random((len(iu[0]), T)) < frac
    m[iu[0], iu[1]] = h
    m[iu[1], iu[0]] = h
    return m


def clean(mask):
    """bool copy with a False diagonal."""
    m = np.array(mask, dtype=bool)
    i = np.arange(m.shape[0])
    m[i, i] = False
    return m


def pack(mask):
    """(words [T][n][nw] uint64, pairs [T], deg [T][n]) as ame_pack_mask returns them."""
    m = clean(mask)
    n, _, T = m.shape
    nw = (n + 63) // 64
    bits = np.zeros((T, n, nw * 64), dtype=np.uint64)
    bits[:, :, :n] = m.transpose(2, 0, 1)
    w = np.zeros((T, n, nw), dtype=np.uint64)
    for b in range(64):
        w |= bits[:, :, b::64] << np.uint64(b)
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    pairs = (m & up[:, :, None]).sum((0, 1)).astype(np.uint64)
    deg = ((n - 1) - m.sum(1)).T.astype(np.uint32)       # (T, n)
    return w, pairs, deg


def asym_entries(mask):
    """Ordered entries i != j with mask[i, j] != mask[j, i] (two per disagreeing pair)."""
    m = clean(mask)
    return int((m != m.transpose(1, 0, 2)).sum())


# ---------------------------------------------------------------------------
# the working network and the correction sums
# ---------------------------------------------------------------------------
def own_values(X_t, r):
    """(n, n, 2): J_j m_i of one slice, [i, j] = (a_i + u_i.v_j, b_i + v_i.u_j)."""
    X_t = np.asarray(X_t)
    a, b, u, v = X_t[:, 0], X_t[:, 1], X_t[:, 2:2 + r], X_t[:, 2 + r:2 + 2 * r]
    P = u @ v.T                                            # P[i, j] = u_i.v_j
    return np.stack([a[:, None] + P, b[:, None] + P.T], axis=-1)


def own_fill(Y, X, mask, dtype=np.float64):
    """Copy of Y (n, n, T, 2) in `dtype` with the hidden entries replaced by each
    row's own-perspective mean, computed in `dtype` from X (n, T, d)."""
    m = clean(mask)
    X = np.asarray(X, dtype)
    n, T, d = X.shape
    r = (d - 2) // 2
    Yw = np.array(Y, dtype=dtype)
    for t in range(T):
        own = own_values(X[:, t], r)
        Yw[:, :, t][m[:, :, t]] = own[m[:, :, t]]
    return Yw


def mean_mu(X_t, r):
    """E[mu_ij] of one slice (n, n, 2) in fp64."""
    X_t = np.asarray(X_t, np.float64)
    a, b, u, v = X_t[:, 0], X_t[:, 1], X_t[:, 2:2 + r], X_t[:, 2 + r:2 + 2 * r]
    m0 = a[:, None] + b[None, :] + u @ v.T
    return np.stack([m0, m0.T], axis=-1)


def corr_rows(Yw, X, mask, R_inv):
    """Per slice, over hidden pairs i < j: [sum r_up' R_inv r_up, sum |r_up|^2 +
    |r_lo|^2] with r_up = Yw[i, j] - E[mu_ij], r_lo = Yw[j, i] - E[mu_ji]: what
    ame_elbo's out[0] / out[7] accumulate at the hidden entries of the working
    network Yw.  Returns (rows (T, 2), sums of |summand| (T, 2))."""
    m = clean(mask)
    X = np.asarray(X, np.float64)
    Yw = np.asarray(Yw, np.float64)
    Ri = np.asarray(R_inv, np.float64)
    n, T, d = X.shape
    r = (d - 2) // 2
    iu = np.triu_indices(n, 1)
    rows, mag = np.zeros((T, 2)), np.zeros((T, 2))
    for t in range(T):
        h = m[iu[0], iu[1], t]
        i, j = iu[0][h], iu[1][h]
        mu = mean_mu(X[:, t], r)
        up = Yw[i, j, t] - mu[i, j]
        lo = Yw[j, i, t] - mu[j, i]
        terms = np.einsum("pa,ab,pb->pab", up, Ri, up)
        rows[t, 0] = terms.sum()
        mag[t, 0] = np.abs(terms).sum()
        rows[t, 1] = mag[t, 1] = (up ** 2).sum() + (lo ** 2).sum()
    return rows, mag


# ---------------------------------------------------------------------------
# the reference's ELBO and MSE over observed pairs
# ---------------------------------------------------------------------------
def masked_terms(Y, X_mean, X_cov, params, variant, mask):
    """dict(loglik, prior0, trans, entropy, elbo, recon): structured_mf.py:124-209 /
    temporal_ame.py:255-291 with the pair sums over observed pairs only; the
    heuristic variance term counts tr(S_it) once per observed partner of i."""
    import ame_oracle as O
    m = clean(mask)
    Xm = np.asarray(X_mean, np.float64)
    Sc = np.asarray(X_cov, np.float64)
    Y = np.asarray(Y, np.float64)
    n, T, d = Xm.shape
    r = (d - 2) // 2
    Ri = np.asarray(params["R_inv"], np.float64)
    logdetR = O._logdet(np.asarray(params["R"], np.float64))
    iu = np.triu_indices(n, 1)
    quad = sq = 0.0
    pairs = 0
    for t in range(T):
        o = ~m[iu[0], iu[1], t]
        i, j = iu[0][o], iu[1][o]
        mu = mean_mu(Xm[:, t], r)
        up = Y[i, j, t] - mu[i, j]
        lo = Y[j, i, t] - mu[j, i]
        quad += float(np.einsum("pa,ab,pb->", up, Ri, up))
        sq += float((up ** 2).sum() + (lo ** 2).sum())
        pairs += len(i)
    if variant == "naive":
        corr = 0.0
    else:
        tr = np.trace(Sc, axis1=2, axis2=3)                 # (n, T)
        deg = (n - 1) - m.sum(1)                            # (n, T)
        corr = 0.1 * float(np.trace(Ri)) / d * float((deg * tr).sum())
    loglik = -0.5 * (pairs * (logdetR + 2 * LOG2PI) + quad + corr)
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    prior0 = O.log_prior_initial(Xm, Sc, p64)
    trans = O.log_prior_transitions(Xm, Sc, p64)
    ent = O.entropy(Sc)
    return dict(loglik=loglik, prior0=prior0, trans=trans, entropy=ent,
                elbo=loglik + prior0 + trans + ent, recon=sq / (2.0 * pairs))


def hidden_error(Y, X_mean, mask):
    """Mean squared error of E[mu] against Y over the hidden entries (both orientations)."""
    m = clean(mask)
    Xm = np.asarray(X_mean, np.float64)
    n, T, d = Xm.shape
    r = (d - 2) // 2
    tot, cnt = 0.0, 0
    for t in range(T):
        e = (np.asarray(Y[:, :, t], np.float64) - mean_mu(Xm[:, t], r)) ** 2
        tot += float(e[m[:, :, t]].sum())
        cnt += 2 * int(m[:, :, t].sum())
    return tot / cnt


# ---------------------------------------------------------------------------
# the masked node update (the reference's rule over observed partners)
# ---------------------------------------------------------------------------
def _obs_terms(Y, X_mean, R_inv, i, t, partners):
    """P_obs, h_obs of ame_oracle.observation_terms over the given partners of i."""
    n, T, d = X_mean.shape
    r = (d - 2) // 2
    Mj = X_mean[partners, t, 2:]
    U, V = Mj[:, :r], Mj[:, r:]
    k = Mj.shape[0]
    E0, E1 = np.zeros((k, d)), np.zeros((k, d))
    E0[:, 0] = 1
    E0[:, 2:2 + r] = V
    E1[:, 1] = 1
    E1[:, 2 + r:] = U
    P = (R_inv[0, 0] * (E0.T @ E0) + R_inv[0, 1] * (E0.T @ E1) + R_inv[1, 0] * (E1.T @ E0)
         + R_inv[1, 1] * (E1.T @ E1))
    z = Y[i, partners, t, :] @ R_inv.T
    return P, E0.T @ z[:, 0] + E1.T @ z[:, 1]


def node_system(Y, X_mean, params, mask, i, t, which="observed"):
    """(P, h) of node i at slice t in fp64: prior terms plus the observation terms
    over its observed partners ("observed"), hidden partners ("hidden", no prior
    terms) or all of them ("all")."""
    import ame_oracle as O
    m = clean(mask)
    X = np.asarray(X_mean, np.float64)
    n, T, d = X.shape
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    others = np.arange(n) != i
    sel = {"observed": others & ~m[i, :, t], "hidden": others & m[i, :, t], "all": others}[which]
    P, h = _obs_terms(np.asarray(Y, np.float64), X, p["R_inv"], i, t, np.nonzero(sel)[0])
    if which == "hidden":
        return P, h
    Q_inv, S0_inv, PtQiP = O.prior_terms(p, T, np.dtype(np.float64))
    Phi = p["Phi"]
    if t == 0:
        P = P + S0_inv
    if t > 0:
        P = P + Q_inv
        h = h + Q_inv @ (Phi @ X[i, t - 1])
    if t < T - 1:
        P = P + PtQiP
        h = h + Phi.T @ (Q_inv @ X[i, t + 1])
    return P, h


def jittered_solve(P, h):
    """mu = C h, C = sym(P^-1) + 1e-6 I (the "good" variant's step, lr = 1)."""
    C = np.linalg.inv(P)
    C = 0.5 * (C + C.T) + JITTER * np.eye(P.shape[0])
    return C @ h


def masked_update(Y, X_mean, params, mask, i, t):
    """New mean of node i at slice t by the reference's rule restricted to its
    observed partners (lr = 1, "good")."""
    return jittered_solve(*node_system(Y, X_mean, params, mask, i, t, "observed"))


# ---------------------------------------------------------------------------
# scoring sums and M-step statistics over a subset of the pairs
# ---------------------------------------------------------------------------
def _subset(mask_t, select, iu):
    h = clean(mask_t[:, :, None])[iu[0], iu[1], 0]
    return {0: np.ones_like(h), OBSERVED: ~h, HIDDEN: h}[select]


def score_rows(X, S, r, Y, noise, zsq, csq, mask, select):
    """predictive_ref's 21 per-slice sums over the selected pairs: rows (T, 21)
    and the per-pair scores of every slice (restricted)."""
    X = np.asarray(X, np.float64)
    n, T, _ = X.shape
    iu = np.triu_indices(n, 1)
    rows, per = np.zeros((T, PR.N_SUMS)), []
    for t in range(T):
        mean, V0, C01 = PR.moments(X[:, t], np.asarray(S)[:, t], r)
        d = PR.dyad_scores(mean, V0, C01, np.asarray(Y)[:, :, t], noise)
        s = _subset(mask[:, :, t], select, iu)
        d = {k: v[s] for k, v in d.items()}
        rows[t] = PR.sums_from_scores(d, zsq, csq)
        per.append(d)
    return rows, per


def dyad_rows(X, S, r, Y, mask, select):
    """mstep_ref.dyad_rows over the selected pairs: rows (T, 4) and sums of |summand|."""
    X = np.asarray(X, np.float64)
    S = np.asarray(S, np.float64)
    Y = np.asarray(Y, np.float64)
    n, T, _ = X.shape
    iu = np.triu_indices(n, 1)
    rows, mag = np.zeros((T, 4)), np.zeros((T, 4))
    for t in range(T):
        s = _subset(mask[:, :, t], select, iu)
        i, j = iu[0][s], iu[1][s]
        mean, V0, C01 = PR.moments(X[:, t], S[:, t], r)
        e = Y[i, j, t] - mean[i, j]
        v00, v11, c = V0[i, j], V0[j, i], C01[i, j]
        rows[t] = (len(i), (e[:, 0] ** 2 + v00).sum(), (e[:, 1] ** 2 + v11).sum(), (e[:, 0] * e[:, 1] + c).sum())
        mag[t] = (len(i), (e[:, 0] ** 2 + np.abs(v00)).sum(), (e[:, 1] ** 2 + np.abs(v11)).sum(),
                  (np.abs(e[:, 0] * e[:, 1]) + np.abs(c)).sum())
    return rows, mag


def statistics(X, S, r, Y, mask):
    """The M-step statistics with Rss and pairs over observed pairs only."""
    st = M.combine(M.state_rows(X, S)[0], dyad_rows(X, S, r, Y, mask, OBSERVED)[0])
    st["hidden_pairs"] = float(pack(mask)[1].sum())
    return st


# ---------------------------------------------------------------------------
# the fit: fill, then one oracle sweep, repeated
# ---------------------------------------------------------------------------
def oracle_fit(Y, X0, S0, params, mask, variant="good", lr=1.0, sweeps=10, dtype=np.float64,
               tol=None, history=False):
    """`sweeps` iterations of (own_fill from the current means, then
    ame_oracle.sweep_stats on that working network), arithmetic in `dtype`; the
    working network is held in `dtype` as the device holds it in fp32.  With
    `tol`, stops once the largest change of a mean over one iteration is below
    it.  Returns dict(X, S, sweeps, change[, terms: masked_terms after every
    sweep])."""
    import ame_oracle as O
    X = np.array(X0, dtype=dtype)
    S = np.array(S0, dtype=dtype)
    q = {k: np.asarray(v, np.float64) for k, v in params.items()}
    terms, change, done = [], np.inf, 0
    for it in range(sweeps):
        Yw = own_fill(Y, X, mask, dtype)
        before = X.copy()
        O.sweep_stats(Yw, X, S, q, variant, lr)
        change = float(np.abs(X - before).max())
        done = it + 1
        if history:
            terms.append(masked_terms(Y, X, S, q, variant, mask))
        if tol is not None and change < tol:
            break
    out = dict(X=X, S=S, sweeps=done, change=change)
    if history:
        out["terms"] = terms
    return out


def oracle_em(Y, X0, S0, params, mask, dtype=np.float64, rounds=1, sweeps=5, lr=0.5, update=("R",),
              variant="good"):
    """mstep_ref.oracle_em with hidden dyads: `sweeps` iterations of oracle_fit in
    `dtype`, then the fp64 M-step with Rss / pairs over observed pairs."""
    n, T, d = X0.shape
    r = (d - 2) // 2
    X, S = np.array(X0, dtype=dtype), np.array(S0, dtype=dtype)
    p = {k: np.array(params[k], dtype=np.float64) for k in M.PARAMS}
    out = []
    for _ in range(rounds):
        q = dict(p, R_inv=np.linalg.inv(p["R"]))
        fit = oracle_fit(Y, X, S, q, mask, variant, lr, sweeps, dtype)
        X, S = fit["X"], fit["S"]
        new = M.m_step(statistics(X, S, r, Y, mask), p, n, T, update)
        out.append(new)
        p = new
    return out


def relative_deviation(a, b, keys):
    """covar_ref.relative_deviation over `keys`: max of max|a - b| / max|a|."""
    return max(float(np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)).max()
                     / np.abs(np.asarray(a[k], np.float64)).max()) for k in keys)


# ---------------------------------------------------------------------------
# shared inputs
# ---------------------------------------------------------------------------
def make_case(n, T, r, seed, variant="good", lr=0.5):
    """A generated network with the initial state and parameters a VI instance
    starts from: dict(model, Y, X0, S0, params) (fp64 copies of the fp32 values)."""
    from ame_amd import (TemporalAMEModel, TemporalAMENaiveMFVI, TemporalAMEStructuredMFVI)
    m = TemporalAMEModel(n, T, r, seed=seed)
    m.generate_data_fast(seed=seed + 1)
    if variant == "naive":
        vi = TemporalAMENaiveMFVI(m, learning_rate=lr)
    else:
        vi = TemporalAMEStructuredMFVI(m, factorization=variant, learning_rate=lr)
    params = {k: getattr(m, k).numpy().astype(np.float64) for k in ("R", "R_inv", "Sigma", "Psi", "Phi", "Q")}
    return dict(model=m, Y=m.Y.numpy().astype(np.float64), X0=vi.X_mean.numpy().astype(np.float64),
                S0=vi.X_cov.numpy().astype(np.float64), params=params)


@functools.lru_cache(maxsize=None)
def fixed_point_case():
    """n = 12, T = 2, r = 1, 30 % hidden, lr = 1: the fill-then-sweep iteration
    run until the successive change of the means is below 1e-10."""
    c = make_case(12, 2, 1, seed=21, lr=1.0)
    mask = random_mask(12, 2, 0.3, seed=1)
    fit = oracle_fit(c["Y"], c["X0"], c["S0"], c["params"], mask, "good", 1.0, sweeps=20000, tol=1e-10)
    return dict(c, mask=mask, fit=fit)


@functools.lru_cache(maxsize=None)
def heldout_case(frac=0.2, sweeps=25, lr=0.5):
    """n = 24, T = 3, r = 2, "good": the scheme, the zero-filled network and the
    fully observed network, each fitted with `sweeps` oracle sweeps; the errors
    on the hidden dyads."""
    import ame_oracle as O
    c = make_case(24, 3, 2, seed=31, lr=lr)
    mask = random_mask(24, 3, frac, seed=2)
    Y, p = c["Y"], c["params"]
    ours = oracle_fit(Y, c["X0"], c["S0"], p, mask, "good", lr, sweeps)
    Yz = Y.copy()
    Yz[clean(mask)] = 0.0
    Xz, Sz = c["X0"].copy(), c["S0"].copy()
    Xf, Sf = c["X0"].copy(), c["S0"].copy()
    for _ in range(sweeps):
        O.sweep_stats(Yz, Xz, Sz, p, "good", lr)
        O.sweep_stats(Y, Xf, Sf, p, "good", lr)
    return dict(scheme=hidden_error(Y, ours["X"], mask), zero_fill=hidden_error(Y, Xz, mask),
                full=hidden_error(Y, Xf, mask))
