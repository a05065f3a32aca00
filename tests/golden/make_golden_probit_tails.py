"""Golden fixture of the probit kernels' tails: tests/golden/probit_tails.npz.

TEST INFRASTRUCTURE ONLY.  Reads nothing but this repository: the inputs are
probit_ref.grid_case (pair means that are exact in fp32 and fp64), and every
expected value is evaluated here with mpmath at 80 digits from the definitions

    Phi(x) = erfc(-x / sqrt 2) / 2        kappa(x) = phi(x) / Phi(x)
    log Phi(x) = log(Phi(x)) for x <= 0,  log1p(-Phi(-x)) for x > 0

(log(ncdf(x)) loses every digit from x = 16 on), never from the erfcx formulas
of csrc/ame_probit.h and probit_ref.py.  rho, sqrt(1 - rho^2) and the means
enter as the exact values of their doubles; sums are exact until the final
rounding to fp64.

    python tests/golden/make_golden_probit_tails.py

Contents, with the names of probit_ref.grid_key:
  seed, rhos                      the inputs' seed and the correlations
  n{n}_rho{k}_stat_{mask}         ame_probit_fill's rows (T, 4)
  n{n}_rho{k}_statmag_{mask}      (T, 4): pairs, the sum of |elementary term| of l,
                                  the sums of |summand| of columns 2 and 3
  n20_rho{k}_d                    the corrections d (n, n, T, 2) in fp64
  n{n}_score_{cov}_{select}       ame_probit_score's rows (T, 6)
  n{n}_scoremag_{cov}_{select}    their sums of |summand| (T, 6)
"""
import os
import sys

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import missing_ref as MR  # noqa: E402
import probit_ref as BR  # noqa: E402

mp.dps = 80
SQRT2 = mp.sqrt(2)
K_STEPS = 2


def Phi(x):
    return mp.erfc(-x / SQRT2) / 2


def normal(x):
    """(kappa(x), log Phi(x), Phi(-x)) from one erfc, of the smaller tail: the
    other tail is its complement, which 80 digits hold without loss."""
    if x <= 0:
        p = Phi(x)
        return mp.npdf(x) / p, mp.log(p), 1 - p
    q = Phi(-x)
    return mp.npdf(x) / (1 - q), mp.log1p(-q), q


def pair(m0, m1, s0, s1, rho, K=K_STEPS):
    """One pair from its exact means and signs: (d0, d1, l, sum |elementary term|
    of l, sum_a (y_a - Phi(m_a))^2, sum_a log Phi(s_a m_a)), all mpf."""
    m0, m1, rho = mpf(m0), mpf(m1), mpf(rho)
    om = 1 - rho * rho
    sd = mp.sqrt(om)
    # y - Phi(m) = s Phi(-s m): no cancellation
    k0, lp0, f0 = normal(s0 * m0)
    k1, lp1, f1 = normal(s1 * m1)
    e0, e1 = m0 + s0 * k0, m1 + s1 * k1
    for _ in range(K):
        eta0 = m0 + rho * (e1 - m1)
        k0, l0, _ = normal(s0 * eta0 / sd)
        e0 = eta0 + s0 * sd * k0
        eta1 = m1 + rho * (e0 - m0)
        k1, l1, _ = normal(s1 * eta1 / sd)
        e1 = eta1 + s1 * sd * k1
    d0, d1 = e0 - m0, e1 - m1
    quad = (d0 * d0 - 2 * rho * d0 * d1 + d1 * d1) / om
    l = mp.log(om) / 2 - quad / 2 + l0 + k0 * k0 / 2 + l1 + k1 * k1 / 2
    el = abs(mp.log(om)) / 2 + quad / 2 + abs(l0) + k0 * k0 / 2 + abs(l1) + k1 * k1 / 2
    return d0, d1, l, el, f0 * f0 + f1 * f1, lp0 + lp1


def fill_arrays(n, rho, slices=None):
    """The stat / statmag / d arrays of (n, rho); rows of slices not in `slices` stay 0."""
    g = BR.grid_case(n, rho)
    T = g["T"]
    iu = np.triu_indices(n, 1)
    hid = {k: (MR.clean(m) if m is not None else np.zeros((n, n, T), bool)) for k, m in g["masks"].items()}
    out = {}
    for name in BR.GRID_MASKS:
        out[BR.grid_key(n, rho, "stat", name)] = np.zeros((T, 4))
        out[BR.grid_key(n, rho, "statmag", name)] = np.zeros((T, 4))
    keep_d = n == BR.GRID_SHAPES[0]
    d = np.zeros((n, n, T, 2))
    for t in (range(T) if slices is None else slices):
        sg = BR.signs(g["B"][:, :, t])
        per = []
        for i, j in zip(*iu):
            m0, m1 = g["means"][t, i, j]
            per.append(pair(m0, m1, int(sg[i, j, 0]), int(sg[i, j, 1]), rho))
            if keep_d:
                d[i, j, t] = d[j, i, t, ::-1] = float(per[-1][0]), float(per[-1][1])
        for name in BR.GRID_MASKS:
            obs = [p for p, i, j in zip(per, *iu) if not hid[name][i, j, t]]
            l, el, f2, lp = (mp.fsum(p[c] for p in obs) for c in (2, 3, 4, 5))
            out[BR.grid_key(n, rho, "stat", name)][t] = len(obs), float(l), float(f2), float(lp)
            out[BR.grid_key(n, rho, "statmag", name)][t] = len(obs), float(el), float(f2), float(-lp)
    if keep_d:
        out[BR.grid_key(n, rho, "d")] = d
    return out


def score_arrays(n, slices=None):
    """The score / scoremag arrays of n nodes (they do not depend on rho)."""
    g = BR.grid_case(n, 0.0)
    T = g["T"]
    iu = np.triu_indices(n, 1)
    mask = g["masks"]["random30"]
    out = {}
    for cov in BR.GRID_COVS:
        rows = {sel: np.zeros((T, 6)) for sel in BR.GRID_SELECTS}
        mags = {sel: np.zeros((T, 6)) for sel in BR.GRID_SELECTS}
        v0 = g["S"][cov][:, :, 0, 0].astype(np.float64)            # V0 of entry (i, j) = S_aa(i): (n, T)
        for t in (range(T) if slices is None else slices):
            per = []
            for i, j in zip(*iu):
                ent = []
                for row, col, c in ((i, j, 0), (j, i, 1)):
                    tt = mpf(g["means"][t, i, j, c]) / mp.sqrt(1 + mpf(v0[row, t]))
                    y = bool(g["B"][row, col, t])
                    _, lp, miss = normal(tt if y else -tt)         # miss = |y - pi|, without cancellation
                    ent.append((lp, miss * miss, int((tt > 0) == y), int(y), Phi(tt)))
                per.append(ent)
            for sel in BR.GRID_SELECTS:
                keep = MR._subset(mask[:, :, t], sel, iu)
                es = [e for p, k in zip(per, keep) if k for e in p]
                lp, br, hit, tie, pi = (mp.fsum(e[c] for e in es) for c in range(5))
                rows[sel][t] = len(es) // 2, float(lp), float(br), float(hit), float(tie), float(pi)
                mags[sel][t] = len(es) // 2, float(-lp), float(br), len(es), float(tie), float(pi)
        for sel in BR.GRID_SELECTS:
            out[BR.grid_key(n, None, "score", cov, sel)] = rows[sel]
            out[BR.grid_key(n, None, "scoremag", cov, sel)] = mags[sel]
    return out


def main():
    res = {"seed": np.int64(BR.GRID_SEED), "rhos": np.array(BR.GRID_RHOS)}
    for n in BR.GRID_SHAPES:
        res.update(score_arrays(n))
        for rho in BR.GRID_RHOS:
            res.update(fill_arrays(n, rho))
            print("done", n, rho, flush=True)
    path = os.path.join(HERE, "probit_tails.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes,", len(res), "arrays")


if __name__ == "__main__":
    main()
