"""fp64 numpy reference of the goodness-of-fit extension (ame_net_moments,
ame_net_triads, ame_simulate, ame_amd/gof.py): the five network statistics in
the obvious dense form and in the raw-sum form the kernels produce, a numpy
Philox4x32-10, and the simulated network evaluated in fp64 from the same
Philox integers.  Test-only."""
import numpy as np

NAMES = ("sd_rowmean", "sd_colmean", "dyad_dep", "cycle_dep", "trans_dep")
EPS32 = 2.0 ** -24
EPS64 = 2.0 ** -52

# ---------------------------------------------------------------------------
# Philox4x32-10
# ---------------------------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two ints -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _LO for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _LO, p1 >> np.uint64(32), p1 & _LO
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def uniform24(w):
    """(float(w >> 8) + 0.5f) * 2^-24, every step in fp32 as the kernel does."""
    k = (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(EPS32)


def pair_normals(n, t_global, seed, sample):
    """(z0, z1) of every pair (i, j) of global slice t_global, fp64 (n, n) arrays
    (only i < j is used): Box-Muller in fp64 from the kernel's fp32 uniforms."""
    i, j = np.meshgrid(np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32), indexing="ij")
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    w = philox4x32_10((i, j, np.uint32(t_global), np.uint32(int(sample) & 0xFFFFFFFF)), key)
    u1, u2 = uniform24(w[0]).astype(np.float64), uniform24(w[1]).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


# ---------------------------------------------------------------------------
# packed layout
# ---------------------------------------------------------------------------
def pack(Y):
    """Dense (T, n, n, 2) -> packed (T, n, ny, 2) fp32 (pad pair zero)."""
    T, n = Y.shape[0], Y.shape[1]
    ny = n + (n & 1)
    out = np.zeros((T, n, ny, 2), dtype=np.float32)
    out[:, :, :n] = Y
    return out


def dense_from_directed(y):
    """A directed network y (T, n, n) -> the swap-consistent (T, n, n, 2) array
    Y[t, i, j] = (y_ij, y_ji)."""
    return np.stack([y, np.swapaxes(y, 1, 2)], axis=-1)


def unpack(Yt, n):
    """Packed (T, n, ny, 2) -> dense (T, n, n, 2)."""
    return np.asarray(Yt)[:, :, :n]


def make_network(n, T, seed, kind="plain"):
    """A directed fp32 network (T, n, n) with sender / receiver effects,
    reciprocity and a rank-2 term; kind "offset" adds a common offset far above
    its spread (ybar >> s).  The diagonal holds values that must never be read."""
    rng = np.random.default_rng(seed)
    a, b = rng.normal(size=(T, n, 1)), rng.normal(size=(T, 1, n))
    U = rng.normal(size=(T, n, 2))
    e = rng.normal(size=(T, n, n))
    y = a + b + np.einsum("tik,tjk->tij", U, U + 0.3 * rng.normal(size=(T, n, 2))) + e + 0.5 * np.swapaxes(e, 1, 2)
    if kind == "offset":
        y = y + 1000.0
    return y.astype(np.float32)


def make_states(n, T, r, seed):
    """fp32 states (T, n, d), every block of x = [a, b, U, V] of order one."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(T, n, 2 + 2 * r)).astype(np.float32) * np.float32(0.7)


def gof_states(seed, n=48, T=3, r=2, n_sim=8):
    """States (n_sim, n, T, d) with a strong multiplicative term (V close to U),
    and the same states with U and V zeroed: what the end-to-end sensitivity
    case simulates from."""
    rng = np.random.default_rng(seed)
    S = np.zeros((n_sim, n, T, 2 + 2 * r), dtype=np.float32)
    S[..., :2] = 0.5 * rng.normal(size=(n_sim, n, T, 2))
    U = rng.normal(size=(n_sim, n, T, r))
    S[..., 2:2 + r] = U
    S[..., 2 + r:] = U + 0.2 * rng.normal(size=(n_sim, n, T, r))
    S0 = S.copy()
    S0[..., 2:] = 0.0
    return S, S0


GOF_SENSITIVITY_SEED = 11


# ---------------------------------------------------------------------------
# the simulated network in fp64
# ---------------------------------------------------------------------------
def simulate(x, chol, seed, sample, t_begin=0):
    """x (T, n, d) -> dict: Y (T, n, n, 2) fp64 with Y[t, i, j] = (mu_ij + e0,
    mu_ji + e1) for i < j, its swap at [t, j, i], zero diagonal; `mu_abs`
    (T, n, n) = |a_i| + |b_j| + sum_k |u_ik v_jk| and `z` (T, n, n, 2), the
    normals of the pair (upper triangle)."""
    x = np.asarray(x, dtype=np.float64)
    T, n, d = x.shape
    r = (d - 2) // 2
    a, b, U, V = x[:, :, 0], x[:, :, 1], x[:, :, 2:2 + r], x[:, :, 2 + r:]
    mu = a[:, :, None] + b[:, None, :] + np.einsum("tik,tjk->tij", U, V)          # mu_ij
    mu_abs = np.abs(a)[:, :, None] + np.abs(b)[:, None, :] + np.einsum("tik,tjk->tij", np.abs(U), np.abs(V))
    l00, l10, l11 = (float(v) for v in chol)
    Y = np.zeros((T, n, n, 2))
    Z = np.zeros((T, n, n, 2))
    iu = np.triu_indices(n, 1)
    for t in range(T):
        z0, z1 = pair_normals(n, t_begin + t, seed, sample)
        Z[t, :, :, 0], Z[t, :, :, 1] = z0, z1
        up0 = mu[t] + l00 * z0
        up1 = mu[t].T + (l10 * z0 + l11 * z1)
        Y[t][iu + (0,)] = up0[iu]
        Y[t][iu + (1,)] = up1[iu]
        Y[t][(iu[1], iu[0], 0)] = up1[iu]
        Y[t][(iu[1], iu[0], 1)] = up0[iu]
    return {"Y": Y, "mu_abs": mu_abs, "z": Z}


# ---------------------------------------------------------------------------
# the five statistics, obvious dense form (one slice)
# ---------------------------------------------------------------------------
def direct_statistics(y, center=None, zero_diagonal=True, swap_triads=False):
    """y: (n, n) directed network, diagonal ignored.  `center` replaces ybar in E
    of the triad statistics only (the kernels centre by an fp32 number).  The
    two switches exist for the sensitivity tests: they break the definition."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    off = ~np.eye(n, dtype=bool)
    vals = y[off]
    N = n * (n - 1)
    ybar = vals.sum() / N
    s = np.sqrt(((vals - ybar) ** 2).sum() / (N - 1))
    rowm = np.array([y[i, off[i]].sum() / (n - 1) for i in range(n)])
    colm = np.array([y[off[:, i], i].sum() / (n - 1) for i in range(n)])
    a, b = y[off], y.T[off]
    dyad = ((a - a.mean()) * (b - b.mean())).sum() / np.sqrt(((a - a.mean()) ** 2).sum() * ((b - b.mean()) ** 2).sum())
    E = y - (ybar if center is None else float(center))
    if zero_diagonal:
        E = np.where(off, E, 0.0)
    out = {"mean": ybar, "sd": s, "sd_rowmean": np.std(rowm, ddof=1), "sd_colmean": np.std(colm, ddof=1),
           "dyad_dep": dyad}
    if n >= 3:
        den = n * (n - 1) * (n - 2) * s ** 3
        cyc, tra = np.trace(E @ E @ E) / den, np.trace(E @ E.T @ E) / den
        out["cycle_dep"], out["trans_dep"] = (tra, cyc) if swap_triads else (cyc, tra)
    else:
        out["cycle_dep"] = out["trans_dep"] = np.nan
    return out


# ---------------------------------------------------------------------------
# raw sums (what the kernels return) and the statistics from them
# ---------------------------------------------------------------------------
def raw_sums(Yd, center):
    """Yd: dense swap-consistent (T, n, n, 2); center (T,) -> fp64 raw sums as the
    kernels define them, with the sums of absolute summands the bounds use."""
    Yd = np.asarray(Yd, dtype=np.float64)
    T, n = Yd.shape[:2]
    off = ~np.eye(n, dtype=bool)
    y = np.where(off[None], Yd[..., 0], 0.0)
    yt = np.where(off[None], Yd[..., 1], 0.0)      # y_ji read from row i
    node = np.stack([y.sum(axis=2), yt.sum(axis=2)], axis=-1)
    node_abs = np.stack([np.abs(y).sum(axis=2), np.abs(yt).sum(axis=2)], axis=-1)
    sl = np.stack([(y * y).sum(axis=(1, 2)), (y * yt).sum(axis=(1, 2))], axis=-1)
    sl_abs = np.stack([(y * y).sum(axis=(1, 2)), np.abs(y * yt).sum(axis=(1, 2))], axis=-1)
    c = np.asarray(center, dtype=np.float32)
    # e = y - center formed in fp32, as the kernel forms it
    E = np.where(off[None], (Yd[..., 0].astype(np.float32) - c[:, None, None]).astype(np.float64), 0.0)
    Et = np.where(off[None], (Yd[..., 1].astype(np.float32) - c[:, None, None]).astype(np.float64), 0.0)
    tri = np.zeros((T, 2))
    tri_abs = np.zeros((T, 2))
    for t in range(T):
        EE, EEt = E[t] @ E[t], E[t] @ E[t].T
        tri[t] = (EE * Et[t]).sum(), (EEt * Et[t]).sum()
        A = np.abs(E[t])
        tri_abs[t] = ((A @ A) * np.abs(Et[t])).sum(), ((A @ A.T) * np.abs(Et[t])).sum()
    return {"node": node, "slice": sl, "tri": tri, "node_abs": node_abs, "slice_abs": sl_abs,
            "tri_abs": tri_abs}


def statistics_from_raw(node, sl, tri, n):
    """The raw-sum form, restated independently of ame_amd/gof.py (one slice or a
    leading slice axis)."""
    node, sl, tri = (np.asarray(v, dtype=np.float64) for v in (node, sl, tri))
    N = n * (n - 1)
    total = node[..., 0].sum(axis=-1)
    ybar = total / N
    css = sl[..., 0] - N * ybar ** 2
    s = np.sqrt(css / (N - 1))
    out = {"mean": ybar, "sd": s,
           "sd_rowmean": np.std(node[..., 0] / (n - 1), axis=-1, ddof=1),
           "sd_colmean": np.std(node[..., 1] / (n - 1), axis=-1, ddof=1),
           "dyad_dep": (sl[..., 1] - N * ybar ** 2) / css}
    if n >= 3:
        den = n * (n - 1) * (n - 2) * s ** 3
        out["cycle_dep"], out["trans_dep"] = tri[..., 0] / den, tri[..., 1] / den
    else:
        out["cycle_dep"] = out["trans_dep"] = np.full(np.shape(ybar), np.nan)
    return out


# ---------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------
def moment_bounds(raw, n):
    """|got - want| <= N 2^-52 sum |summand| for every fp64 sum of exact summands."""
    N = n * (n - 1)
    return {"node": N * EPS64 * raw["node_abs"], "slice": N * EPS64 * raw["slice_abs"]}


def simulate_bounds(sim, r, chol, noise_rel):
    """Per-entry bound (T, n, n, 2) on a simulated network against `simulate`:
    the fill kernel's rule for the fp32 mean, 2 (r + 1) 2^-24 (|a| + |b| +
    sum_k |u_k v_k|), plus noise_rel |l| (1 + |z|) per noise term."""
    l00, l10, l11 = (abs(float(v)) for v in chol)
    z0, z1 = np.abs(sim["z"][..., 0]), np.abs(sim["z"][..., 1])
    n = z0.shape[1]
    up = np.triu(np.ones((n, n), dtype=bool), 1)[None]
    mu = 2 * (r + 1) * EPS32 * sim["mu_abs"]
    e0 = noise_rel * l00 * (1.0 + z0)
    e1 = noise_rel * (l10 * (1.0 + z0) + l11 * (1.0 + z1))
    b0 = np.where(up, mu + e0, 0.0)                       # entry [i][j][0], i < j
    b1 = np.where(up, np.swapaxes(mu, 1, 2) + e1, 0.0)    # entry [i][j][1]
    out = np.stack([b0, b1], axis=-1)
    return out + np.swapaxes(out, 1, 2)[..., ::-1]        # [j][i] holds the swap


def triad_bounds(raw, n):
    """(n + 3) 2^-24 sum_ijk |E_ik E_kj E_ji|: one fp32 rounding per e and a
    K = n term fp32 MFMA accumulation (K 2^-24 on sum |a_k b_k|)."""
    return (n + 3) * EPS32 * raw["tri_abs"]


def statistic_bounds(node, sl, tri, n, b_node, b_slice, b_tri):
    """First-order propagation of raw-sum bounds through the statistics of one
    slice: every raw scalar k is moved by its bound and the changes of each
    statistic are added, doubled for the second-order terms; plus the fp64
    evaluation itself, 32 roundings amplified by the cancellation kappa =
    sum y^2 / sum (y - ybar)^2 of the centred sums."""
    base = statistics_from_raw(node, sl, tri, n)
    tol = {k: 0.0 for k in NAMES}
    def bump(arr, idx, b):
        a2 = [np.array(node, dtype=np.float64), np.array(sl, dtype=np.float64), np.array(tri, dtype=np.float64)]
        a2[arr][idx] += b
        st = statistics_from_raw(a2[0], a2[1], a2[2], n)
        for k in NAMES:
            if np.isfinite(st[k]) and np.isfinite(base[k]):
                tol[k] += abs(st[k] - base[k])
    for i in range(n):
        for c in range(2):
            bump(0, (i, c), b_node[i, c])
    for c in range(2):
        bump(1, (c,), b_slice[c])
        bump(2, (c,), b_tri[c])
    N = n * (n - 1)
    kappa = sl[0] / max(sl[0] - N * base["mean"] ** 2, np.finfo(float).tiny)
    return {k: 2.0 * tol[k] + 32 * EPS64 * kappa * (1.0 + abs(base[k])) for k in NAMES}
