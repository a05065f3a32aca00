"""Closed-form M-step of variational EM from the sufficient statistics of q
(ame_mstep_stats, include/ame_amd.h).  Host side, fp64, CPU: the matrices are
d x d and 2 x 2; the expensive part, the statistics, is computed on the GPU.

With q mean-field across nodes and time, E_it = m_it m_it' + S_it and

    A0  = sum_i E_i0                 A11 = sum_i sum_{t>=1} E_it
    A00 = sum_i sum_{t>=1} E_i,t-1   A10 = sum_i sum_{t>=1} m_it m_i,t-1'
    Rss = sum_t sum_{i<j} E_q[(y_ij - mu_ij)(y_ij - mu_ij)']

the expected complete-data log-likelihood is, up to constants,

    F = -1/2 [ Np log|R| + tr(R^-1 Rss) ] - 1/2 [ n log|S0| + tr(S0^-1 A0) ]
        -1/2 [ n (T-1) log|Q| + tr(Q^-1 (A11 - Phi A10' - A10 Phi' + Phi A00 Phi')) ]

(Np = T n (n-1) / 2, S0 = blockdiag(Sigma, Psi)), maximised by

    Phi = A10 A00^-1                       or  phi = tr(Q^-1 A10) / tr(Q^-1 A00), Phi = phi I
    Q   = sym(A11 - Phi A10' - A10 Phi' + Phi A00 Phi') / (n (T-1))
    R   = Rss / Np,   Sigma = A0[:2,:2] / n,   Psi = A0[2:,2:] / n.

F is not the ELBO fit() reports: that one (the reference's, structured_mf.py:
141-148, 193) uses a heuristic variance correction and omits tr(Phi' Q^-1 Phi
S_{t-1}); the M-step climbs F.
"""
from __future__ import annotations

import torch

UPDATES = ("Phi", "Q", "R", "Sigma0", "beta")
DEFAULT_UPDATE = ("Phi", "Q", "R", "Sigma0")   # "beta" only on request: it needs covariates
PHI_STRUCTURES = ("full", "scalar")

# Dyadic covariates (ame_covar_stats): y_ij = mu_ij + sum_k beta_k w_k,ij + eps.
# The statistics are taken on the residual y~ = y - sum_k beta_k w_k at the
# beta stored with them (stats["beta"]), e = y~ - E[mu]:
#     G[k] = sum w_k e'   (p, 2, 2)        H[k][l] = sum w_k w_l'   (p, p, 2, 2)
# and Rss at beta + delta is Rss - sum_k delta_k (G_k + G_k') + sum_kl delta_k
# delta_l H[k][l], so the R-term of F is maximised over beta, at fixed R, by
#     (sum_ab Rinv[a][b] H[k][l][a][b]) delta = sum_ab Rinv[a][b] G[k][a][b].
# With "beta" and "R" both updated the step is beta first, then R = Rss(beta_new)
# / pairs: a conditional-maximisation step, each half cannot lower F.


def combine_covar(G: torch.Tensor, H: torch.Tensor, beta) -> dict:
    """Per-slice rows G (T, p, 2, 2) and H (T, p, p, 2, 2) -> their sums, slice
    by slice in time order as :func:`combine` adds its rows, with the beta the
    residual was taken at."""
    G = G.to("cpu", torch.float64)
    H = H.to("cpu", torch.float64)
    g = torch.zeros(G.shape[1:], dtype=torch.float64)
    h = torch.zeros(H.shape[1:], dtype=torch.float64)
    for t in range(int(G.shape[0])):
        g += G[t]
        h += H[t]
    return {"G": g, "H": h, "beta": torch.as_tensor(beta).detach().to("cpu", torch.float64).clone()}


def rss_at(stats: dict, delta: torch.Tensor) -> torch.Tensor:
    """Rss at stats["beta"] + delta."""
    G, H = stats["G"], stats["H"]
    Rss = stats["Rss"] - torch.einsum("k,kab->ab", delta, G + G.transpose(1, 2))
    return Rss + torch.einsum("k,l,klab->ab", delta, delta, H)


def _rss_for(stats: dict, params: dict) -> torch.Tensor:
    """Rss at params["beta"] (the statistics' own Rss without covariates)."""
    if "G" not in stats or "beta" not in params:
        return stats["Rss"]
    delta = params["beta"] - stats["beta"]
    if not bool(delta.any()):
        return stats["Rss"]
    return rss_at(stats, delta)


def beta_step(stats: dict, R: torch.Tensor) -> torch.Tensor:
    """delta maximising the R-term of F over beta at fixed R; a singular system
    (collinear covariates) raises ValueError."""
    if "G" not in stats or "H" not in stats:
        raise ValueError('"beta" needs the covariate statistics G and H: the model has no covariates')
    Ri = _sym(torch.linalg.inv(R))
    A = _sym(torch.einsum("ab,klab->kl", Ri, stats["H"]))
    b = torch.einsum("ab,kab->k", Ri, stats["G"])
    _, info = torch.linalg.cholesky_ex(A)
    scale = A.diagonal().abs().max()
    if int(info) != 0 or not bool(torch.isfinite(A).all()) \
            or float(torch.linalg.eigvalsh(A)[0]) <= 2.0 ** -40 * float(scale):
        raise ValueError("M-step: the system for beta is singular (collinear or zero covariates)")
    return torch.linalg.solve(A, b)


def combine(state: torch.Tensor, dyad: torch.Tensor, cross=None) -> dict:
    """Per-slice rows in global time order (state (T, 2, d, d), dyad (T, 4),
    fp64, CPU) -> the statistics.  Slices are added one by one in time order,
    so every caller that holds the same rows gets the same bits.  ``cross``
    (T, d, d), optional: per-slice sums of the lag-one cross-covariances
    Cov(x_t, x_t-1) of a q that is not factorised across time (ame_smooth's
    lag_sum); slices 1.. are added into A10 after the mean part, in time order."""
    state = state.to("cpu", torch.float64)
    dyad = dyad.to("cpu", torch.float64)
    T, d = int(state.shape[0]), int(state.shape[2])
    A11 = torch.zeros(d, d, dtype=torch.float64)
    A00 = torch.zeros(d, d, dtype=torch.float64)
    A10 = torch.zeros(d, d, dtype=torch.float64)
    for t in range(1, T):
        A11 += state[t, 0]
        A00 += state[t - 1, 0]
        A10 += state[t, 1]
    if cross is not None:
        cross = cross.to("cpu", torch.float64)
        for t in range(1, T):
            A10 += cross[t]
    s = torch.zeros(4, dtype=torch.float64)
    for t in range(T):
        s += dyad[t]
    Rss = torch.stack([torch.stack([s[1], s[3]]), torch.stack([s[3], s[2]])])
    return {"A0": state[0, 0].clone(), "A11": A11, "A00": A00, "A10": A10, "Rss": Rss,
            "pairs": float(s[0])}


def blockdiag(Sigma, Psi):
    d = 2 + Psi.shape[0]
    S = torch.zeros(d, d, dtype=torch.float64)
    S[:2, :2] = Sigma
    S[2:, 2:] = Psi
    return S


def transition_scatter(stats, Phi):
    A10, A00 = stats["A10"], stats["A00"]
    return stats["A11"] - Phi @ A10.T - A10 @ Phi.T + Phi @ A00 @ Phi.T


def objective(stats: dict, params: dict, n: int, T: int) -> float:
    """F(theta) above; params holds fp64 Phi, Q, R, Sigma, Psi and, with
    covariate statistics G, H in `stats`, optionally beta (Rss is then taken at
    that beta)."""
    R, Q = params["R"], params["Q"]
    S0 = blockdiag(params["Sigma"], params["Psi"])
    f = -0.5 * (stats["pairs"] * torch.logdet(R) + torch.trace(torch.linalg.solve(R, _rss_for(stats, params))))
    f = f - 0.5 * (n * torch.logdet(S0) + torch.trace(torch.linalg.solve(S0, stats["A0"])))
    if T > 1:
        M = transition_scatter(stats, params["Phi"])
        f = f - 0.5 * (n * (T - 1) * torch.logdet(Q) + torch.trace(torch.linalg.solve(Q, M)))
    return float(f)


def objective_scale(stats: dict, params: dict, n: int, T: int) -> float:
    """Sum of the |terms| F is made of: rounding in evaluating F is a small
    multiple of 2^-52 times this, so a change of F below that means nothing."""
    R, Q = params["R"], params["Q"]
    S0 = blockdiag(params["Sigma"], params["Psi"])
    m = abs(stats["pairs"] * torch.logdet(R)) + (torch.linalg.inv(R) * stats["Rss"]).abs().sum()
    if "G" in stats and "beta" in params:   # the terms Rss at params["beta"] is made of
        dl = (params["beta"] - stats["beta"]).abs()
        G, H = stats["G"].abs(), stats["H"].abs()
        extra = torch.einsum("k,kab->ab", dl, G + G.transpose(1, 2)) + torch.einsum("k,l,klab->ab", dl, dl, H)
        m = m + (torch.linalg.inv(R).abs() * extra).sum()
    m = m + abs(n * torch.logdet(S0)) + (torch.linalg.inv(S0) * stats["A0"]).abs().sum()
    if T > 1:
        Phi, A10, A00 = params["Phi"], stats["A10"], stats["A00"]
        Qi = torch.linalg.inv(Q).abs()
        m = m + abs(n * (T - 1) * torch.logdet(Q))
        for part in (stats["A11"], Phi @ A10.T, A10 @ Phi.T, Phi @ A00 @ Phi.T):
            m = m + (Qi * part.abs()).sum()
    return float(m)


def _sym(a):
    return 0.5 * (a + a.T)


def solve(stats: dict, params: dict, n: int, T: int, update=DEFAULT_UPDATE, phi_structure="full") -> dict:
    """New fp64 parameters: those named in `update` at their maximisers (Q with
    the Phi just chosen; R with the beta just chosen), the others as in
    `params`.  "beta" needs the covariate statistics (G, H, beta) in `stats`;
    the result then has a "beta" entry as well."""
    update = tuple(update)
    bad = set(update) - set(UPDATES)
    if bad:
        raise ValueError(f"unknown parameter(s) {sorted(bad)}; known: {UPDATES}")
    if phi_structure not in PHI_STRUCTURES:
        raise ValueError(f"phi_structure must be one of {PHI_STRUCTURES} (got {phi_structure!r})")
    if T < 2 and ("Phi" in update or "Q" in update):
        raise ValueError("Phi and Q need at least two time steps")
    new = {k: params[k].clone() for k in ("Phi", "Q", "R", "Sigma", "Psi")}
    d = new["Phi"].shape[0]
    if "Phi" in update:
        if phi_structure == "full":
            new["Phi"] = torch.linalg.solve(stats["A00"], stats["A10"].T).T
        else:
            Qi = torch.linalg.inv(params["Q"])
            phi = torch.trace(Qi @ stats["A10"]) / torch.trace(Qi @ stats["A00"])
            new["Phi"] = phi * torch.eye(d, dtype=torch.float64)
    if "Q" in update:
        new["Q"] = _sym(transition_scatter(stats, new["Phi"])) / (n * (T - 1))
    Rss = stats["Rss"]
    if "beta" in params:
        new["beta"] = params["beta"].clone()
        Rss = _rss_for(stats, params)
    if "beta" in update:
        delta = beta_step(stats, params["R"])
        new["beta"] = stats["beta"] + delta
        Rss = rss_at(stats, delta)
    if "R" in update:
        new["R"] = Rss / stats["pairs"]
    if "Sigma0" in update:
        new["Sigma"] = _sym(stats["A0"][:2, :2]) / n
        new["Psi"] = _sym(stats["A0"][2:, 2:]) / n
    return new


def validate(params: dict) -> None:
    """Raise ValueError unless every entry is finite and Q, R, Sigma, Psi are
    symmetric positive definite."""
    for k, v in params.items():
        if not bool(torch.isfinite(v).all()):
            raise ValueError(f"M-step: {k} is not finite")
    for k in ("Q", "R", "Sigma", "Psi"):
        v = params[k]
        _, info = torch.linalg.cholesky_ex(_sym(v))
        if int(info) != 0:
            raise ValueError(f"M-step: {k} is not positive definite")
