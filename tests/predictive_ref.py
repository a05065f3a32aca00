"""fp64 numpy reference of the posterior-predictive dyad moments, the scoring
sums and the forecast recursion (test-only; imports nothing from ame_amd).

State of node i at one time: x_i = [a_i, b_i, U_i(r), V_i(r)], q(x_i) = N(m_i, S_i),
independent across nodes; mu_ij = (a_i + b_j + U_i.V_j, a_j + b_i + U_j.V_i).
Every term below is its own einsum, written as the formula reads: nothing is
regrouped into per-node features (the kernel's algebra), so the two agree only
if that regrouping is right.
"""
import math

import numpy as np

LOG2PI = math.log(2.0 * math.pi)
N_SUMS = 21
MAX_LEVELS = 4

V0_TERMS = ("add_i", "add_j", "quad_i", "quad_j", "trace", "cross_i", "cross_j")
C01_TERMS = ("ab_i", "ab_j", "lin_uj_SiaV", "lin_SjbU_vi", "lin_SibU_vj", "lin_ui_SjaV",
             "trCC", "bil_i", "bil_j")
# the term groups of the issue (a dropped group must show), besides each single term
GROUPS = {"additive": ("add_i", "add_j"), "quadratic": ("quad_i", "quad_j"),
          "cross": ("cross_i", "cross_j"), "bilinear": ("bil_i", "bil_j")}


def blocks(m, S, r):
    U, V = slice(2, 2 + r), slice(2 + r, 2 + 2 * r)
    return dict(a=m[:, 0], b=m[:, 1], u=m[:, U], v=m[:, V],
                Saa=S[:, 0, 0], Sbb=S[:, 1, 1], Sab=S[:, 0, 1],
                SaU=S[:, 0, U], SaV=S[:, 0, V], SbU=S[:, 1, U], SbV=S[:, 1, V],
                SUU=S[:, U, U], SVV=S[:, V, V], C=S[:, U, V])


def v0_terms(B):
    """The terms of V0[i, j] = Var[mu_ij[0]], each (n, n)."""
    n = B["a"].shape[0]
    one = np.ones((n, n), dtype=B["a"].dtype)
    es = lambda *a: np.einsum(*a, optimize=True)
    return {
        "add_i": B["Saa"][:, None] * one,
        "add_j": B["Sbb"][None, :] * one,
        "quad_i": es("jk,ikl,jl->ij", B["v"], B["SUU"], B["v"]),      # v_j' S_i[UU] v_j
        "quad_j": es("ik,jkl,il->ij", B["u"], B["SVV"], B["u"]),      # u_i' S_j[VV] u_i
        "trace": es("ikl,jlk->ij", B["SUU"], B["SVV"]),               # tr(S_i[UU] S_j[VV])
        "cross_i": 2.0 * es("ik,jk->ij", B["SaU"], B["v"]),           # 2 S_i[aU].v_j
        "cross_j": 2.0 * es("ik,jk->ij", B["u"], B["SbV"]),           # 2 u_i.S_j[bV]
    }


def c01_terms(B):
    """The terms of C01[i, j] = Cov[mu_ij[0], mu_ij[1]], each (n, n)."""
    n = B["a"].shape[0]
    one = np.ones((n, n), dtype=B["a"].dtype)
    es = lambda *a: np.einsum(*a, optimize=True)
    return {
        "ab_i": B["Sab"][:, None] * one,
        "ab_j": B["Sab"][None, :] * one,
        "lin_uj_SiaV": es("jk,ik->ij", B["u"], B["SaV"]),             # u_j.S_i[aV]
        "lin_SjbU_vi": es("jk,ik->ij", B["SbU"], B["v"]),             # S_j[bU].v_i
        "lin_SibU_vj": es("ik,jk->ij", B["SbU"], B["v"]),             # S_i[bU].v_j
        "lin_ui_SjaV": es("ik,jk->ij", B["u"], B["SaV"]),             # u_i.S_j[aV]
        "trCC": es("ikl,jlk->ij", B["C"], B["C"]),                    # tr(C_i C_j)
        "bil_i": es("jk,ikl,jl->ij", B["v"], B["C"], B["u"]),         # v_j' C_i u_j
        "bil_j": es("ik,jkl,il->ij", B["v"], B["C"], B["u"]),         # v_i' C_j u_i
    }


def moments(m, S, r, drop=()):
    """One slice.  m (n, d), S (n, d, d) -> mean (n, n, 2), V0 (n, n), C01 (n, n) in fp64.
    Var[mu_ij[1]] = V0[j, i].  `drop`: term names left out (input-quality test).
    The diagonal holds the formulas' values, which mean nothing there (i = j)."""
    m = np.asarray(m, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    B = blocks(m, S, r)
    mean0 = B["a"][:, None] + B["b"][None, :] + np.einsum("ik,jk->ij", B["u"], B["v"])
    mean = np.stack([mean0, mean0.T], axis=-1)
    V0 = sum(t for k, t in v0_terms(B).items() if k not in drop)
    C01 = sum(t for k, t in c01_terms(B).items() if k not in drop)
    return mean, V0, C01


def _products(B):
    """Elementary products of every term, (n, n, K) per quantity, in the order
    the formulas list them: what a plain fp32 loop would sum."""
    u, v = B["u"], B["v"]
    n, r = u.shape
    bc = lambda x: np.broadcast_to(x, (n, n) + x.shape[2:]).reshape(n, n, -1)
    mean0 = [bc(B["a"][:, None, None]), bc(B["b"][None, :, None]), u[:, None, :] * v[None, :, :]]
    v0 = [bc(B["Saa"][:, None, None]), bc(B["Sbb"][None, :, None]),
          bc(B["SUU"][:, None] * v[None, :, :, None] * v[None, :, None, :]),
          bc(B["SVV"][None, :] * u[:, None, :, None] * u[:, None, None, :]),
          bc(B["SUU"][:, None] * np.swapaxes(B["SVV"], 1, 2)[None, :]),
          2 * B["SaU"][:, None, :] * v[None, :, :], 2 * u[:, None, :] * B["SbV"][None, :, :]]
    C = B["C"]
    c01 = [bc(B["Sab"][:, None, None]), bc(B["Sab"][None, :, None]),
           u[None, :, :] * B["SaV"][:, None, :], B["SbU"][None, :, :] * v[:, None, :],
           B["SbU"][:, None, :] * v[None, :, :], u[:, None, :] * B["SaV"][None, :, :],
           bc(C[:, None] * np.swapaxes(C, 1, 2)[None, :]),
           bc(C[:, None] * v[None, :, :, None] * u[None, :, None, :]),
           bc(C[None, :] * v[:, None, :, None] * u[:, None, None, :])]
    cat = lambda xs: np.concatenate([np.ascontiguousarray(x) for x in xs], axis=-1)
    return cat(mean0), cat(v0), cat(c01)


def abs_sums(m, S, r):
    """Sum of |elementary products| of mean0, V0, C01 per dyad: the scale an
    fp32 evaluation's rounding error is proportional to."""
    B = blocks(np.asarray(m, np.float64), np.asarray(S, np.float64), r)
    return tuple(np.abs(p).sum(-1) for p in _products(B))


def moments_f32(m, S, r):
    """The same formulas in np.float32: every product rounded to fp32 and the
    products summed one after another in fp32 (np.cumsum is sequential).  Used
    only to measure what fp32 arithmetic costs on given inputs."""
    B = blocks(np.asarray(m, np.float32), np.asarray(S, np.float32), r)
    out = []
    for p in _products(B):
        assert p.dtype == np.float32
        out.append(np.cumsum(p, axis=-1, dtype=np.float32)[..., -1])
    return tuple(out)


def f32_relative_error(m, S, r):
    """max over dyads i != j and over (mean0, V0, C01) of |fp32 - fp64| / sum|products|."""
    mean, V0, C01 = moments(m, S, r)
    f = moments_f32(m, S, r)
    sc = abs_sums(m, S, r)
    off = ~np.eye(V0.shape[0], dtype=bool)
    return max(float((np.abs(a.astype(np.float64) - b) / s)[off].max())
               for a, b, s in zip(f, (mean[..., 0], V0, C01), sc))


def thresholds(levels):
    """zsq = Phi^-1((1 + p) / 2)^2, csq = -2 ln(1 - p) (chi-square, 2 dof)."""
    from statistics import NormalDist
    z = [NormalDist().inv_cdf((1.0 + p) / 2.0) ** 2 for p in levels]
    c = [-2.0 * math.log1p(-p) for p in levels]
    return np.array(z), np.array(c)


def dyad_scores(mean, V0, C01, Y, noise):
    """Per unordered pair i < j (upper triangle of Y as the observation):
    e (P, 2), Sigma entries s00, s11, s01, det, z2 (P, 2), m2, log density."""
    n = V0.shape[0]
    iu = np.triu_indices(n, 1)
    N = np.asarray(noise, dtype=np.float64).reshape(2, 2)
    y = np.asarray(Y, dtype=np.float64)[iu[0], iu[1]]
    e = y - mean[iu[0], iu[1]]
    s00 = V0[iu[0], iu[1]] + N[0, 0]
    s11 = V0[iu[1], iu[0]] + N[1, 1]
    s01 = C01[iu[0], iu[1]] + 0.5 * (N[0, 1] + N[1, 0])
    det = s00 * s11 - s01 * s01
    m2 = (s11 * e[:, 0] ** 2 - 2.0 * s01 * e[:, 0] * e[:, 1] + s00 * e[:, 1] ** 2) / det
    z2 = np.stack([e[:, 0] ** 2 / s00, e[:, 1] ** 2 / s11], axis=1)
    logp = -0.5 * (np.log(det) + m2 + 2.0 * LOG2PI)
    return dict(e=e, s00=s00, s11=s11, s01=s01, det=det, m2=m2, z2=z2, logp=logp)


def sums_from_scores(d, zsq, csq):
    """The 21 per-slice sums of ame_predict from dyad_scores()."""
    out = np.zeros(N_SUMS)
    out[0] = d["m2"].shape[0]
    out[1] = d["logp"].sum()
    out[2] = d["m2"].sum()
    out[3], out[4] = d["z2"][:, 0].sum(), d["z2"][:, 1].sum()
    out[5], out[6] = d["s00"].sum(), d["s11"].sum()
    out[7], out[8] = (d["e"][:, 0] ** 2).sum(), (d["e"][:, 1] ** 2).sum()
    for l in range(len(zsq)):
        out[9 + 3 * l] = (d["z2"][:, 0] <= zsq[l]).sum()
        out[10 + 3 * l] = (d["z2"][:, 1] <= zsq[l]).sum()
        out[11 + 3 * l] = (d["m2"] <= csq[l]).sum()
    return out


def score_slice(m, S, r, Y, noise, zsq, csq):
    mean, V0, C01 = moments(m, S, r)
    d = dyad_scores(mean, V0, C01, Y, noise)
    return sums_from_scores(d, zsq, csq), d


def forecast(m, S, Phi, Q, h):
    """m (n, d), S (n, d, d) at the last fitted slice -> (n, h, d), (n, h, d, d):
    m_k = Phi m_{k-1}, S_k = Phi S_{k-1} Phi' + Q."""
    m = np.asarray(m, np.float64)
    S = np.asarray(S, np.float64)
    Phi, Q = np.asarray(Phi, np.float64), np.asarray(Q, np.float64)
    ms, Ss = [], []
    for _ in range(h):
        m = m @ Phi.T
        S = Phi @ S @ Phi.T + Q
        ms.append(m)
        Ss.append(S)
    return np.stack(ms, axis=1), np.stack(Ss, axis=1)


def forecast_direct(m, S, Phi, Q, k):
    """Step k >= 1 in closed form: Phi^k m, Phi^k S Phi^k' + sum_{q<k} Phi^q Q Phi^q'."""
    Phi, Q = np.asarray(Phi, np.float64), np.asarray(Q, np.float64)
    Pk = np.linalg.matrix_power(Phi, k)
    acc = np.zeros_like(Q)
    for q in range(k):
        Pq = np.linalg.matrix_power(Phi, q)
        acc = acc + Pq @ Q @ Pq.T
    return np.asarray(m, np.float64) @ Pk.T, Pk @ np.asarray(S, np.float64) @ Pk.T + acc


# ---- the inputs of the GPU tests (tests/test_gpu_predictive.py) ----
# Largest error of the np.float32 evaluation (moments_f32) against the fp64
# reference over these inputs, relative to a dyad's sum of |products|: measured
# 2.366e-6 (at (65, 2, 31)), rounded down; test_predictive_ref.py re-measures it
# and requires DELTA0 <= measured.  The kernel's elementwise bound is 4 x DELTA0.
DELTA0 = 2.3e-6
TOL = 4.0 * DELTA0
# (70, 8, 3): a slice count that is a multiple of 8 takes the pair kernel's
# other workgroup -> (slice, tile) mapping
GPU_SHAPES = ((2, 1, 1), (3, 2, 2), (63, 2, 5), (64, 2, 5), (65, 2, 5), (130, 3, 16), (97, 2, 32),
              (200, 3, 8), (70, 8, 3))
# every other compiled r, at the two-tile shape with a one-wide edge tile: used
# by the dense-moment and scoring-sum tests, and part of DELTA0's measurement
GPU_SHAPES_EVERY_R = tuple((65, 2, r) for r in range(1, 33)
                           if r not in {s[2] for s in GPU_SHAPES})


def make_state(n, T, r, seed=0):
    """Means of scale 1 and SPD covariances 0.3 A A' + 0.1 I + w w' with every
    cross block populated.  A has entries N(0, 1/d) (diagonal ~0.4, off-diagonal
    ~0.3 / sqrt(d)); w >= 0 (|N(0,1)| on a and b, 0.2 |N(0,1)| on U and V) gives
    S[ab] and the U-V block a common sign, without which S[ab] and tr(C_i C_j)
    would be below 1e-3 of a dyad's sum of |products| at r = 32 and a dropped
    term could hide in the tolerance (test_predictive_ref.py (b)).
    Returns fp32 arrays in the reference layout (n, T, d), (n, T, d, d)."""
    d = 2 + 2 * r
    rng = np.random.default_rng(1000 * n + 10 * T + r + 7919 * seed)
    m = rng.standard_normal((n, T, d))
    A = rng.standard_normal((n, T, d, d)) / math.sqrt(d)
    w = np.abs(rng.standard_normal((n, T, d))) * np.r_[1.0, 1.0, np.full(2 * r, 0.2)]
    S = 0.3 * A @ np.swapaxes(A, -1, -2) + 0.1 * np.eye(d) + w[..., :, None] * w[..., None, :]
    S = 0.5 * (S + np.swapaxes(S, -1, -2))
    return m.astype(np.float32), S.astype(np.float32)
