"""fp64 numpy reference of the eight sufficient sums of ame_elbo
(include/ame_amd.h) and of ame_pack_y's mismatch count (test-only; imports
nothing from ame_amd).

    out[0] sum_{t, i<j} e' Rinv e          out[1] sum_{i,t} tr(S_it)
    out[2] sum_i mu_i0' S0inv mu_i0        out[3] sum_i tr(S0inv S_i0)
    out[4] sum_{i,t>=1} e' Qinv e          out[5] sum_{i,t>=1} tr(Qinv S_it)
    out[6] sum_{i,t} logdet S_it           out[7] sum_{t, i!=j} |Y_ij - m_ij|^2

Time is global: out[2], out[3] come from global slice 0 only; out[4], out[5]
from global slices >= 1, with e = mu_it - Phi mu_i,t-1 and the previous mean
taken from slice t - 1 of the full X.  out[0] reads the upper triangle Y[i, j],
i < j, out[7] both triangles (tests/elbo_check.py: pair_sums).

Every sum comes with `mag`, the sum of the absolute values of its summands,
the scale rounding errors are proportional to:
    out[0]            |r00| e0^2 + |r01 + r10| |e0 e1| + |r11| e1^2
    out[2], out[4]    |e|' |M| |e| + 2 (|mu| + |Phi| |mu_prev|)' |M| |e|
                      (the second term covers the rounding of e itself; at
                      slice 0, e = mu and mu_prev = 0)
    the others        sum |term|
The node terms are accumulated in numpy's long double (64-bit mantissa on
x86, so their own error is 2^-11 of an fp64 evaluation's; plain fp64 elsewhere)
and rounded to fp64 once; the pair terms in fp64.
"""
import numpy as np

LD = np.longdouble
NODE_SUMS = (1, 2, 3, 4, 5, 6)
PAIR_SUMS = (0, 7)


def pair_mean(x, r):
    """compute_mean (static_ame.py:189-238) of one slice, x (n, d) fp64."""
    a, b = x[:, 0], x[:, 1]
    U, V = x[:, 2:2 + r], x[:, 2 + r:]
    add = a[:, None] + b[None, :]
    mult = U @ V.T
    return np.stack([add + mult, add.T + mult.T], axis=-1)


def _form(e, M, lead):
    """sum_i e_i' M e_i and its magnitude, `lead` (n, d) = |mu| + |Phi||mu_prev|."""
    ae, aM = np.abs(e), np.abs(M)
    val = np.einsum("na,ab,nb->", e, M, e)
    mag = np.einsum("na,ab,nb->", ae, aM, ae) + 2 * np.einsum("na,ab,nb->", lead, aM, ae)
    return val, mag


def slice_rows(X, cov_terms, Y, S0inv, Qinv, Phi, rinv):
    """The eight sums of every global slice on its own.

    X (n, T, d) fp32 means, cov_terms (T, n, 4) fp64 (logdet, trace,
    tr(Qinv S), tr(S0inv S)), Y (n, n, T, 2) fp32, S0inv / Qinv / Phi (d, d)
    fp64, rinv the four entries of R_inv row-major.
    Returns rows (T, 8), mags (T, 8) fp64."""
    X = np.asarray(X)
    n, T, d = X.shape
    r = (d - 2) // 2
    ct = np.asarray(cov_terms, dtype=np.float64)
    assert ct.shape == (T, n, 4) and np.asarray(Y).shape == (n, n, T, 2)
    r00, r01, r10, r11 = (float(v) for v in rinv)
    S0l, Ql, Pl = (np.asarray(a, dtype=np.float64).astype(LD) for a in (S0inv, Qinv, Phi))
    Xl = X.astype(np.float64).astype(LD)
    iu, ju = np.triu_indices(n, 1)
    off = ~np.eye(n, dtype=bool)
    rows = np.zeros((T, 8), dtype=LD)
    mags = np.zeros((T, 8), dtype=LD)
    with np.errstate(invalid="ignore"):   # a -inf logdet gives |x| = inf, inf - inf nowhere
        for t in range(T):
            mu = pair_mean(X[:, t].astype(np.float64), r)
            e = np.asarray(Y)[:, :, t].astype(np.float64) - mu
            e0, e1 = e[iu, ju, 0], e[iu, ju, 1]
            rows[t, 0] = (r00 * e0 * e0 + (r01 + r10) * e0 * e1 + r11 * e1 * e1).sum()
            mags[t, 0] = (abs(r00) * e0 * e0 + abs(r01 + r10) * np.abs(e0 * e1) + abs(r11) * e1 * e1).sum()
            rows[t, 7] = mags[t, 7] = (e[..., 0] ** 2 + e[..., 1] ** 2)[off].sum()
            c = ct[t].astype(LD)
            for k, col in ((6, 0), (1, 1)):
                rows[t, k], mags[t, k] = c[:, col].sum(), np.abs(c[:, col]).sum()
            m = Xl[:, t]
            if t == 0:
                rows[t, 2], mags[t, 2] = _form(m, S0l, np.abs(m))
                rows[t, 3], mags[t, 3] = c[:, 3].sum(), np.abs(c[:, 3]).sum()
            else:
                pm = Xl[:, t - 1]
                rows[t, 4], mags[t, 4] = _form(m - pm @ Pl.T, Ql, np.abs(m) + np.abs(pm) @ np.abs(Pl).T)
                rows[t, 5], mags[t, 5] = c[:, 2].sum(), np.abs(c[:, 2]).sum()
    return rows.astype(np.float64), mags.astype(np.float64)


def range_sums(rows, mags, t0, t1):
    """out[8], mag[8] of the slice range [t0, t1) from slice_rows' result."""
    return rows[t0:t1].astype(LD).sum(0).astype(np.float64), mags[t0:t1].astype(LD).sum(0).astype(np.float64)


def elbo_sums(X, cov_terms, Y, S0inv, Qinv, Phi, rinv, t0, t1):
    """out[8], mag[8] over [t0, t1), and the per-slice rows / mags of that range."""
    rows, mags = slice_rows(X, cov_terms, Y, S0inv, Qinv, Phi, rinv)
    out, mag = range_sums(rows, mags, t0, t1)
    return out, mag, rows[t0:t1], mags[t0:t1]


# ----------------------------------------------------------------------------
# the constructed state of tests/test_gpu_elbo_sums.py (shared with the CPU
# checks, so the sensitivity figures quoted there are of the same inputs)
# ----------------------------------------------------------------------------
def synthetic_cov_terms(n, T, seed):
    """(T, n, 4) fp64 stand-in for ame_cov's output: mixed signs, magnitudes over
    five decades, an independent draw (and a different decade offset) in each
    column, so a swapped column or a term of the wrong slice moves a sum by far
    more than its bound."""
    rng = np.random.default_rng(77 + 1000 * n + T + 7919 * seed)
    sign = np.where(rng.random((T, n, 4)) < 0.5, -1.0, 1.0)
    return sign * 10.0 ** rng.uniform(-3.0, 2.0, (T, n, 4)) * np.array([1.0, 3.0, 0.3, 7.0])


def is_fp32(a):
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) == a


def make_params(r, seed=0):
    """An asymmetric fp64 draw: generic_params' Phi / Q / Sigma / Psi / R, then
    Phi moved off the fp32 grid, S0inv and Qinv inverted in fp64, and R_inv the
    fp64 inverse with unequal off-diagonal entries (the C ABI takes four values).
    No entry of Phi or R_inv is representable in fp32, so fp32 staging shows."""
    from generic_params import generic_params
    d = 2 + 2 * r
    g = {k: v.astype(np.float64) for k, v in generic_params(r, 4242 + 10 * r + seed).items()}
    rng = np.random.default_rng(99 + r + 7919 * seed)
    Phi = g["Phi"] + 1e-4 * rng.standard_normal((d, d))
    S0 = np.zeros((d, d))
    S0[:2, :2], S0[2:, 2:] = g["Sigma"], g["Psi"]
    S0inv, Qinv = np.linalg.inv(S0), np.linalg.inv(g["Q"])
    Rinv = np.linalg.inv(g["R"]) + np.array([[0.0, 0.37], [-0.21, 0.0]]) / 3.0
    assert not is_fp32(Phi).any() and not is_fp32(Rinv).any()
    consts = np.stack([S0inv, Qinv, Phi.T @ Qinv @ Phi, Qinv @ Phi, Phi.T @ Qinv])
    return dict(Phi=Phi, S0inv=S0inv, Qinv=Qinv, rinv=tuple(Rinv.flatten()), consts=consts)


# ----------------------------------------------------------------------------
# ame_pack_y
# ----------------------------------------------------------------------------
def pack_layout(Y, t0, t1):
    """Yt [t1 - t0][n][ny][2] of include/ame_amd.h as uint32 bit patterns:
    Yt[tl, i, j] = Y[i, j, t0 + tl] for j < n, the pad pair j = n (odd n) +0.0."""
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    n = Y.shape[0]
    ny = n + (n & 1)
    out = np.zeros((t1 - t0, n, ny, 2), dtype=np.uint32)
    out[:, :, :n] = Y.view(np.uint32)[:, :, t0:t1].transpose(2, 0, 1, 3)
    return out


def pack_mismatches(Y, t0, t1):
    """The rule of the header: pairs i < j and slices t in [t0, t1) with
    Y[j, i, t] != swap(Y[i, j, t]), compared as BIT PATTERNS, as the kernel
    does: (0.0, x) against (x, -0.0) is a mismatch, a NaN with the same bits on
    both sides is none, and the diagonal is never looked at."""
    B = np.ascontiguousarray(Y, dtype=np.float32).view(np.uint32)[:, :, t0:t1]
    n = B.shape[0]
    iu, ju = np.triu_indices(n, 1)
    up, lo = B[iu, ju], B[ju, iu]            # (pairs, t, 2)
    return int(((lo[..., 0] != up[..., 1]) | (lo[..., 1] != up[..., 0])).sum())
