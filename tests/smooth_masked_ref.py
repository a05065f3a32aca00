"""fp64 numpy reference of ame_smooth over observed partners (include/ame_amd.h,
`Mt` set): each node's exact Gaussian posterior across time given the other
nodes' means and only the dyads it has observed (test-only).

For node i, with m the cleaned symmetric mask and obs(i,t) = {j != i : not m[i,j,t]}:

    D_t = P_obs^m(i,t) + [t = 0] S0inv + [t > 0] Qinv + [t < T-1] PtQiP
    P_obs^m(i,t) = sum_{j in obs(i,t)} J_j' sym(R_inv) J_j
    h_t = sum_{j in obs(i,t)} J_j' R_inv y_ij       (y: the raw observations)
    O, the recursion and the outputs: as smooth_ref

`blocks` builds P and h with missing_ref._obs_terms over the restricted partner
set; smooth_ref.dense / recursion do the rest.  `MUTATIONS` are the mistakes the
masked kernels could make.  Those that live in the hidden partners' Gram matrix
H (w = [1, U, V]; P = sym(R_inv) (.) ((G - w_i w_i') - H)) are built on
`gram_route`, which is also a second route to P.
"""
import functools

import numpy as np

import missing_ref as MR
import smooth_ref as SR

MUTATIONS = ("drop_mask_P", "drop_mask_h", "wrong_slice", "drop_count", "drop_colsum", "pad_reads_node")
H_MUTATIONS = ("drop_count", "drop_colsum", "pad_reads_node")
KEYS = ("mean", "cov", "cross", "lag_sum")

# the GPU parity shapes (n, T, r): the word boundary at 64, the tile boundaries at 2r = 16 / 32 / 48
SHAPES = ((5, 2, 1), (65, 3, 8), (66, 2, 9), (130, 2, 16), (70, 2, 17), (40, 2, 25), (34, 2, 32))
EVERY_R_SHAPES = tuple((9, 2, r) for r in range(1, 33))
MASKS = ("random30", "one_pair", "last_pair", "cols63_64", "counts1345", "all_of_one", "none")
EVERY_R_MASK = "random30"


# ---------------------------------------------------------------------------
# masks (n, n, T) bool, symmetric, different in every slice
# ---------------------------------------------------------------------------
def make_mask(name, n, T):
    if name == "random30":
        return MR.random_mask(n, T, 0.3)
    if name == "none":
        return np.zeros((n, n, T), dtype=bool)
    pairs = []
    for t in range(T):
        if name == "one_pair":
            pairs.append((t % n, (t + 2) % n if (t + 2) % n != t % n else (t + 1) % n, t))
        elif name == "last_pair":      # the last column of the last row; then the last column of row t - 1
            pairs.append((n - 2 if t == 0 else (t - 1) % (n - 1), n - 1, t))
        elif name == "cols63_64":      # both sides of the word boundary (the last two columns when n < 65)
            c0, c1 = (63, 64) if n >= 65 else (n - 2, n - 1)
            for i in (t, t + 1, c0 - 1 - t):
                pairs += [(i, c0, t), (i, c1, t)]
        elif name == "counts1345":     # nodes t .. t+3 with 1, 3, 4 and 5 hidden partners (at most n - 1)
            for k, cnt in enumerate((1, 3, 4, 5)):
                i = t + k
                js = [j for j in range(n - 1, -1, -1) if j not in range(t, t + 4)][:cnt]
                pairs += [(i, j, t) for j in js]
        elif name == "all_of_one":     # every partner of one node, in one slice only
            if t == min(1, T - 1):
                i = n // 2
                pairs += [(i, j, t) for j in range(n) if j != i]
            else:
                pairs.append((t, n - 1, t))
        else:
            raise KeyError(name)
    return MR.sym_mask(n, T, [p for p in pairs if p[0] != p[1]])


# ---------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------
def _wrows(X, t, r):
    """w_j = [1, U_j, V_j] of slice t, (n, 1 + 2r)."""
    n = X.shape[0]
    return np.concatenate([np.ones((n, 1)), X[:, t, 2:2 + 2 * r]], axis=1)


def _expand(Rs, Mw, r):
    """d x d block from the (1 + 2r)^2 matrix over w: entry (k, m) = Rs[sel_k, sel_m] Mw[wi_k, wi_m],
    state index k -> (row of J it belongs to, index into w): a -> (0, 1), b -> (1, 1),
    u_c -> (0, V_c), v_c -> (1, U_c)."""
    sel = np.array([0, 1] + [0] * r + [1] * r)
    wi = np.array([0, 0] + [1 + r + c for c in range(r)] + [1 + c for c in range(r)])
    return Rs[np.ix_(sel, sel)] * Mw[np.ix_(wi, wi)]


def gram_route(X, Rs, m, i, t, mutation=None):
    """P_obs^m(i,t) = sym(R_inv) (.) ((G - w_i w_i') - H), H over the hidden partners."""
    n, T, d = X.shape
    r = (d - 2) // 2
    w = _wrows(X, t, r)
    hid = np.nonzero(m[i, :, t])[0]
    H = w[hid].T @ w[hid]
    if mutation == "drop_count":
        H[0, 0] = 0.0
    if mutation == "drop_colsum":
        H[0, 1:] = 0.0
        H[1:, 0] = 0.0
    if mutation == "pad_reads_node" and len(hid) % 4:
        pad = 4 - len(hid) % 4
        w0 = w[0].copy()
        w0[0] = 0.0                       # the count is the popcount
        H += pad * np.outer(w0, w0)
        H[0, 1:] += pad * w[0, 1:]
        H[1:, 0] += pad * w[0, 1:]
    return _expand(Rs, (w.T @ w - np.outer(w[i], w[i])) - H, r)


def blocks(Y, X, R_inv, consts, mask, i, mutation=None):
    """D (T, d, d), O (d, d), h (T, d) of node i in fp64, sums over obs(i,t)."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    R_inv = np.asarray(R_inv, np.float64)
    Rs = 0.5 * (R_inv + R_inv.T)
    m = MR.clean(mask)
    n, T, d = X.shape
    others = np.arange(n) != i
    D = np.zeros((T, d, d))
    h = np.zeros((T, d))
    for t in range(T):
        obs = others & ~m[i, :, t]
        obs_P = obs_h = np.nonzero(obs)[0]
        if mutation == "drop_mask_P":
            obs_P = np.nonzero(others)[0]
        if mutation == "drop_mask_h":
            obs_h = np.nonzero(others)[0]
        if mutation == "wrong_slice":
            obs_P = np.nonzero(others & ~m[i, :, (t + 1) % T])[0]
        if mutation in H_MUTATIONS:
            P = gram_route(X, Rs, m, i, t, mutation)
        else:
            P, _ = MR._obs_terms(Y, X, Rs, i, t, obs_P)
        _, ht = MR._obs_terms(Y, X, R_inv, i, t, obs_h)
        D[t] = P + (consts["S0inv"] if t == 0 else consts["Qinv"])
        if t < T - 1:
            D[t] += consts["PtQiP"]
        h[t] = ht
    return D, -np.asarray(consts["QiPhi"], np.float64), h


def abs_precision_norm(X, R_inv, i):
    """a_i = max_t || sum_{j != i} |J_j|' |sym R_inv| |J_j| ||_2: the size of the terms of which
    (G - w_i w_i') - H is a three-way difference."""
    X = np.abs(np.asarray(X, np.float64))
    R_inv = np.asarray(R_inv, np.float64)
    Ra = np.abs(0.5 * (R_inv + R_inv.T))
    n, T, d = X.shape
    partners = np.nonzero(np.arange(n) != i)[0]
    dummy = np.zeros((n, n, T, 2))
    return max(float(np.linalg.norm(MR._obs_terms(dummy, X, Ra, i, t, partners)[0], 2)) for t in range(T))


def smooth(Y, X, R_inv, consts, mask, route="dense", mutation=None, nodes=None):
    """smooth_ref.smooth over observed partners; adds snorm (n,) = ||S_i||_2 of the joint
    covariance and a (n,) = abs_precision_norm (dense route)."""
    X = np.asarray(X, np.float64)
    n, T, d = X.shape
    nodes = range(n) if nodes is None else nodes
    k = len(nodes)
    out = dict(mean=np.zeros((k, T, d)), cov=np.zeros((k, T, d, d)), cross=np.zeros((k, T, d, d)),
               cond=np.full(k, np.nan), snorm=np.full(k, np.nan), a=np.full(k, np.nan))
    for q, i in enumerate(nodes):
        D, Ob, h = blocks(Y, X, R_inv, consts, mask, i, mutation)
        if route == "dense":
            mu, S, Xc, cond = SR.dense(D, Ob, h)
            ev = np.linalg.eigvalsh(SR.joint_precision(D, Ob))
            out["cond"][q] = cond
            out["snorm"][q] = 1.0 / np.abs(ev).min()
            out["a"][q] = abs_precision_norm(X, R_inv, i)
        else:
            mu, S, Xc = SR.recursion(D, Ob, h)
        out["mean"][q], out["cov"][q], out["cross"][q] = mu, S, Xc
    out["lag_sum"] = out["cross"].sum(0)
    out["lag_abs"] = np.abs(out["cross"]).sum(0)
    return out


def tolerance(ref, n, T, d):
    """smooth_ref.tolerance plus, per node, (n + 2) 2^-52 ||S_i||_2 a_i scale_i: the rounding of
    the three-way difference (G - w_i w_i') - H, each of whose terms is an n-term sum bounded by
    a_i, carried to the outputs by S_i."""
    tol = SR.tolerance(ref, T, d)
    extra_cross = 0.0
    for k in ("mean", "cov", "cross"):
        a = ref[k]
        k_n = a.shape[0]
        scale = np.abs(a.reshape(k_n, -1)).max(1)
        e = (n + 2) * 2.0 ** -52 * ref["snorm"] * ref["a"] * scale
        tol[k] = tol[k] + e.reshape((k_n,) + (1,) * (a.ndim - 1))
        if k == "cross":
            extra_cross = e.sum()
    tol["lag_sum"] = tol["lag_sum"] + extra_cross
    return tol


@functools.lru_cache(maxsize=None)
def make_case(shape, pset, mask_name):
    """smooth_ref.make_case's inputs with a mask and the masked fp64 reference (dense route)."""
    base = SR.make_case(shape, pset)
    n, T, r = shape
    mask = make_mask(mask_name, n, T)
    ref = smooth(base["Y"], base["X"], base["R_inv"], base["consts"], mask)
    return dict(base, mask=mask, mref=ref)


# ---------------------------------------------------------------------------
# the calls built on the masked smoother
# ---------------------------------------------------------------------------
def consts_from(params):
    """The four blocks from fp64 model parameters (as smooth_ref.smoothed_statistics builds them)."""
    import mstep_ref as M
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    Qinv = np.linalg.inv(p["Q"])
    S0 = M.blockdiag(p["Sigma"], p["Psi"])
    return dict(S0inv=np.linalg.inv(S0), Qinv=Qinv, PtQiP=p["Phi"].T @ Qinv @ p["Phi"], QiPhi=Qinv @ p["Phi"])


def smoothed_statistics(Y, X, r, params, mask):
    """missing_ref.statistics of the observed-partner smoothed posterior: its means and
    marginals, sum_t>=1 lag_sum[t] added into A10, Rss and pairs over observed pairs."""
    import mstep_ref as M
    sm = smooth(Y, X, np.linalg.inv(np.asarray(params["R"], np.float64)), consts_from(params), mask)
    srows, _ = M.state_rows(sm["mean"], sm["cov"])
    srows[1:, 1] += sm["lag_sum"][1:]
    drows, _ = MR.dyad_rows(sm["mean"], sm["cov"], r, Y, mask, MR.OBSERVED)
    st = M.combine(srows, drows)
    st["hidden_pairs"] = float(MR.pack(mask)[1].sum())
    return st, sm


def oracle_em_round(Y, X0, S0, params, mask, dtype=np.float64, sweeps=5, lr=0.5, update=("R",)):
    """One round of missing_ref.oracle_em whose M-step takes the statistics of the
    observed-partner smoothed posterior; the smoother reads the means the sweeps left
    (fp32 values when dtype is fp32, as the device holds them)."""
    import mstep_ref as M
    n, T, d = X0.shape
    r = (d - 2) // 2
    p = {k: np.array(params[k], dtype=np.float64) for k in M.PARAMS}
    q = dict(p, R_inv=np.linalg.inv(p["R"]))
    fit = MR.oracle_fit(Y, np.array(X0, dtype=dtype), np.array(S0, dtype=dtype), q, mask, "good", lr, sweeps, dtype)
    st, _ = smoothed_statistics(Y, fit["X"].astype(np.float64), r, p, mask)
    return M.m_step(st, p, n, T, update)
