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

UPDATES = ("Phi", "Q", "R", "Sigma0")
PHI_STRUCTURES = ("full", "scalar")


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
    """F(theta) above; params holds fp64 Phi, Q, R, Sigma, Psi."""
    R, Q = params["R"], params["Q"]
    S0 = blockdiag(params["Sigma"], params["Psi"])
    f = -0.5 * (stats["pairs"] * torch.logdet(R) + torch.trace(torch.linalg.solve(R, stats["Rss"])))
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


def solve(stats: dict, params: dict, n: int, T: int, update=UPDATES, phi_structure="full") -> dict:
    """New fp64 parameters: those named in `update` at their maximisers (Q with
    the Phi just chosen), the others as in `params`."""
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
    if "R" in update:
        new["R"] = stats["Rss"] / stats["pairs"]
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
