"""fp64 numpy reference of the residual diagnostics of a Gaussian fit (test-only;
imports nothing from ame_amd), built on predictive_ref: the per-pair quantities,
the per-node sums, the histogram of m2 by the bin rule of include/ame_amd.h, a
brute-force top-k, and the elementwise bounds.

The bounds.  The device forms E[mu], V0 and C01 with fp32 MFMA products and
everything after them in fp64.  test_gpu_predictive.py holds those products to
predictive_ref.TOL x the entry's sum of |elementary products| (abs_sums): dm for
a mean, dv for a variance, dc for the covariance.  With e the residual, Sigma
the predictive covariance and g = Sigma^-1 e, to first order

    d(m2)   = 1.001 (2 (|g0| dm0 + |g1| dm1) + g0^2 dv0 + g1^2 dv1 + 2 |g0 g1| dc) + 2^-40 (1 + m2)
    d(z2_c) = 2 |e_c| dm_c / Sigma_cc + e_c^2 dv_c / Sigma_cc^2
    d(e_c)  = dm_c            d(e_c^2) = 2 |e_c| dm_c
    d(logN) = d(m2) / 2 + (s11 dv0 + s00 dv1 + 2 |s01| dc) / (2 det)

(m2 = e' Sigma^-1 e has gradient -2 g in the means and -g g' in Sigma; log det
has gradient Sigma^-1 in Sigma), each plus 2^-40 |term| for the fp64 arithmetic
after the products.  The signed z_c = e_c / sqrt(Sigma_cc) of a record is
bounded as links_ref bounds its score: with Sigma_lo = Sigma_cc - dv_c,
    d(z_c) = dm_c / sqrt(Sigma_lo) + (|e_c| + dm_c) dv_c / (2 Sigma_lo^(3/2)) + 2^-40 (1 + |z_c|).
A node's bound is the sum of its pairs' bounds.  Nothing here is measured on the
kernels.
"""
import numpy as np

import missing_ref as MR
import predictive_ref as PR

NOISE = np.array([[1.0, 0.5], [0.5, 1.0]])
PLANTED = (20.0, 26.0, 40.0, 90.0, 200.0)
CEILING = 16.0          # no pair that is not planted has m2 above this
BINS, M2_MAX = 256, 32.0
SHAPES = ((2, 1, 1), (3, 2, 2), (63, 2, 5), (64, 2, 5), (65, 2, 5), (130, 3, 16), (97, 2, 32), (70, 8, 3))
# the shapes the issue's CPU measurements were taken on
CPU_SHAPES = ((33, 2, 2), (65, 2, 5), (130, 3, 16), (97, 2, 32))
EPS = 2.0 ** -40
NODE_SUMS = 9


def _extend(d, i, j):
    """i, j, the signed z (P, 2) and g = Sigma^-1 e (P, 2) added to dyad scores."""
    e, s00, s11, s01, det = d["e"], d["s00"], d["s11"], d["s01"], d["det"]
    d.update(i=i, j=j, z=e / np.sqrt(np.stack([s00, s11], 1)),
             g=np.stack([(s11 * e[:, 0] - s01 * e[:, 1]) / det, (s00 * e[:, 1] - s01 * e[:, 0]) / det], 1))
    return d


def _bounds(d, dm, dv, dc):
    """The module docstring's bounds d_m2, d_logp (P,), d_z2, d_e, d_q, d_z (P, 2)
    from the bounds dm, dv (P, 2) and dc (P,) of the means, variances and covariance."""
    e, s00, s11, s01, det = d["e"], d["s00"], d["s11"], d["s01"], d["det"]
    sig = np.stack([s00, s11], 1)
    g, ae = np.abs(d["g"]), np.abs(e)
    d["d_m2"] = 1.001 * (2.0 * (g * dm).sum(1) + (g * g * dv).sum(1) + 2.0 * g[:, 0] * g[:, 1] * dc) \
        + EPS * (1.0 + d["m2"])
    d["d_z2"] = 2.0 * ae * dm / sig + e * e * dv / (sig * sig) + EPS * d["z2"]
    d["d_e"] = dm + EPS * ae
    d["d_q"] = 2.0 * ae * dm + EPS * e * e
    d["d_logp"] = 0.5 * d["d_m2"] + 0.5 * (s11 * dv[:, 0] + s00 * dv[:, 1] + 2.0 * np.abs(s01) * dc) / det \
        + EPS * np.abs(d["logp"])
    lo = sig - dv
    assert (lo > 0.0).all()
    d["d_z"] = dm / np.sqrt(lo) + (ae + dm) * dv / (2.0 * lo ** 1.5) + EPS * (1.0 + np.abs(d["z"]))
    return d


def pair_scores(mean, V0, C01, Y_t, noise, sm=None, sv=None, sc=None):
    """predictive_ref.dyad_scores of one slice plus i, j, z, g and, given the
    |product| sums, the bounds."""
    i, j = np.triu_indices(V0.shape[0], 1)
    d = _extend(PR.dyad_scores(mean, V0, C01, Y_t, noise), i, j)
    if sm is None:
        return d
    return _bounds(d, PR.TOL * np.stack([sm[i, j], sm[j, i]], 1), PR.TOL * np.stack([sv[i, j], sv[j, i]], 1),
                   PR.TOL * sc[i, j])


def host_scores(mean, second, Y_t, rel=2.0 ** -22, extra=None):
    """The scores of one slice from dense predictive moments as predict_dyads
    returns them, mean (n, n, 2) and second (n, n, 3) = (Var entry 0, Var entry 1,
    Cov) with the noise in: the same fp32 products the scoring kernels use, rounded
    to fp32 once more (the noise is added in fp32 there, and with covariates the
    mean and the residual network are each an fp32 sum).  The bounds allow `rel`
    of |y| + |mean| on a residual and of every second moment: four fp32 roundings;
    `extra` (n, n, 2) = sum_k |beta_k w_k| joins |y| + |mean| when covariates were
    taken off y and added to the mean one after another in fp32."""
    mean, second, Y_t = (np.asarray(a, np.float64) for a in (mean, second, Y_t))
    i, j = np.triu_indices(mean.shape[0], 1)
    e = Y_t[i, j] - mean[i, j]
    s00, s11, s01 = second[i, j, 0], second[i, j, 1], second[i, j, 2]
    det = s00 * s11 - s01 * s01
    m2 = (s11 * e[:, 0] ** 2 - 2.0 * s01 * e[:, 0] * e[:, 1] + s00 * e[:, 1] ** 2) / det
    d = dict(e=e, s00=s00, s11=s11, s01=s01, det=det, m2=m2,
             z2=np.stack([e[:, 0] ** 2 / s00, e[:, 1] ** 2 / s11], 1),
             logp=-0.5 * (np.log(det) + m2 + 2.0 * PR.LOG2PI))
    d = _extend(d, i, j)
    size = np.abs(Y_t[i, j]) + np.abs(mean[i, j]) + (0.0 if extra is None else np.asarray(extra, np.float64)[i, j])
    return _bounds(d, rel * size, rel * np.stack([s00, s11], 1), rel * np.abs(s01))


def slice_scores(X_t, S_t, r, Y_t, noise=NOISE, moments=None, drop_c01=False):
    """pair_scores of one slice from the state; `moments` (mean0, V0, C01) replaces
    the fp64 moments (an fp32 evaluation, a mutation), the bounds stay the
    reference's."""
    sm, sv, sc = PR.abs_sums(X_t, S_t, r)
    if moments is None:
        mean, V0, C01 = PR.moments(X_t, S_t, r)
    else:
        m0, V0, C01 = (np.asarray(a, np.float64) for a in moments)
        mean = np.stack([m0, m0.T], -1)
    if drop_c01:
        C01 = np.zeros_like(C01)
    return pair_scores(mean, V0, C01, Y_t, noise, sm, sv, sc)


def subset(d, mask_t, select):
    """One slice's scores restricted to the pairs `select` (0, missing_ref.OBSERVED,
    missing_ref.HIDDEN) picks under the (n, n) mask."""
    if not select:
        return d
    hid = MR.clean(mask_t[:, :, None])[d["i"], d["j"], 0]
    keep = hid if select == MR.HIDDEN else ~hid
    return {k: v[keep] for k, v in d.items()}


def _node_add(d, n, one, logp, m2, z2, e, q, exchange=False):
    """(n, 9) sums over both ends of each pair: entry 0 is sent by i and received
    by j, entry 1 the reverse (exchange: the mutation that swaps the two)."""
    out = np.zeros((n, NODE_SUMS))
    i, j = d["i"], d["j"]
    a, b = (1, 0) if exchange else (0, 1)
    for node, snd, rcv in ((i, a, b), (j, b, a)):
        np.add.at(out[:, 0], node, one)
        np.add.at(out[:, 1], node, logp)
        np.add.at(out[:, 2], node, m2)
        for base, v in ((3, z2), (5, e), (7, q)):
            np.add.at(out[:, base], node, v[:, snd])
            np.add.at(out[:, base + 1], node, v[:, rcv])
    return out


def node_sums(d, n, exchange=False):
    """The (n, AME_NODE_SUMS) sums of one slice."""
    return _node_add(d, n, np.ones(len(d["i"])), d["logp"], d["m2"], d["z2"], d["e"], d["e"] ** 2, exchange)


def node_bounds(d, n):
    """The (n, AME_NODE_SUMS) bounds of node_sums (slot 0 is exact: 0)."""
    return _node_add(d, n, np.zeros(len(d["i"])), d["d_logp"], d["d_m2"], d["d_z2"], d["d_e"], d["d_q"])


def node_abs(d, n):
    """Sum of |term| of every slot: the scale of an fp64 reordering."""
    return _node_add(d, n, np.ones(len(d["i"])), np.abs(d["logp"]), np.abs(d["m2"]), d["z2"], np.abs(d["e"]),
                     d["e"] ** 2)


def edges(bins=BINS, m2_max=M2_MAX):
    return np.array([b * (m2_max / bins) for b in range(bins + 1)])


def bin_of(m2, bins=BINS, m2_max=M2_MAX):
    """b = floor(m2 * scale) clamped to [0, bins - 1], scale = bins / m2_max in fp64;
    NaN -> bins - 1."""
    sc = np.float64(bins) / np.float64(m2_max)
    m2 = np.asarray(m2, np.float64)
    out = np.full(m2.shape, bins - 1, np.int64)
    ok = ~np.isnan(m2)
    out[ok] = np.clip(np.floor(m2[ok] * sc), 0, bins - 1).astype(np.int64)
    return out


def histogram(d, bins=BINS, m2_max=M2_MAX):
    h = np.zeros(bins, np.int64)
    np.add.at(h, bin_of(d["m2"], bins, m2_max), 1)
    return h


def sandwich(hist_t, d, bins=BINS, m2_max=M2_MAX):
    """Whether one slice's device histogram (bins,) is consistent with the
    reference m2 under d_m2: the total is exact and for every interior edge
    #{m2 + d < edge} <= cumulative device count <= #{m2 - d < edge}."""
    ed = edges(bins, m2_max)[1:-1]
    if int(hist_t.sum()) != len(d["m2"]):
        return False, ("total", int(hist_t.sum()), len(d["m2"]))
    lo, hi = np.sort(d["m2"] + d["d_m2"]), np.sort(d["m2"] - d["d_m2"])
    cum = np.cumsum(hist_t)[:-1]
    least, most = np.searchsorted(lo, ed, side="left"), np.searchsorted(hi, ed, side="left")
    bad = np.nonzero((cum < least) | (cum > most))[0]
    if len(bad):
        e = int(bad[0])
        return False, (e + 1, int(least[e]), int(cum[e]), int(most[e]))
    return True, None


def near_edge_share(d, bins=BINS, m2_max=M2_MAX):
    """Share of one slice's pairs whose reference m2 lies within d_m2 of an interior edge."""
    ed = edges(bins, m2_max)[1:-1]
    if not len(d["m2"]):
        return 0.0
    k = np.clip(np.searchsorted(ed, d["m2"]), 0, len(ed) - 1)
    dist = np.minimum(np.abs(d["m2"] - ed[k]), np.abs(d["m2"] - ed[np.maximum(k - 1, 0)]))
    return float((dist <= d["d_m2"]).mean())


def top_k(d, k):
    """Indices into d of its k most surprising pairs by (-m2, i, j)."""
    return np.lexsort((d["j"], d["i"], -d["m2"]))[:k]


def make_network(X, S, r, seed, noise=NOISE):
    """A calibrated network for the state (X, S): per pair y = E[mu] + chol(Sigma) xi
    rounded to fp32, Y[j, i] the swap of Y[i, j], a zero diagonal.  A pair whose m2
    comes out above CEILING has its residual shrunk to below it; then in every slice
    min(5, pairs) planted pairs have theirs rescaled to m2 = the last of PLANTED.
    Returns Y (n, n, T, 2) fp32 and planted[t] = [(i, j, target), ..] by rising target."""
    n, T, _ = X.shape
    rng = np.random.default_rng(77000 + 100 * n + 10 * T + r + seed)
    N = np.asarray(noise, np.float64)
    Y = np.zeros((n, n, T, 2), np.float32)
    iu = np.triu_indices(n, 1)
    P = len(iu[0])
    planted = []
    for t in range(T):
        mean, V0, C01 = PR.moments(X[:, t], S[:, t], r)
        mu = mean[iu[0], iu[1]]
        s00, s11 = V0[iu[0], iu[1]] + N[0, 0], V0[iu[1], iu[0]] + N[1, 1]
        s01 = C01[iu[0], iu[1]] + 0.5 * (N[0, 1] + N[1, 0])
        l00 = np.sqrt(s00)
        l10 = s01 / l00
        l11 = np.sqrt(s11 - l10 * l10)
        xi = rng.standard_normal((P, 2))
        e = np.stack([l00 * xi[:, 0], l10 * xi[:, 0] + l11 * xi[:, 1]], 1)
        m2 = (xi ** 2).sum(1)
        want = m2.copy()
        high = m2 > CEILING
        want[high] = CEILING - 4.0 * rng.random(int(high.sum())) - 1.0
        picks = rng.choice(P, size=min(5, P), replace=False)
        targets = PLANTED[len(PLANTED) - len(picks):]
        want[picks] = targets
        e = e * np.sqrt(want / m2)[:, None]
        y = (mu + e).astype(np.float32)
        Y[iu[0], iu[1], t] = y
        Y[iu[1], iu[0], t] = y[:, ::-1]
        planted.append([(int(iu[0][p]), int(iu[1][p]), float(v)) for p, v in zip(picks, targets)])
    return Y, planted


def make_case(shape, seed=0):
    """dict(X, S (predictive_ref.make_state), Y, planted, mask (30 % of the pairs
    hidden, for the tests that use one)) of a shape (n, T, r)."""
    n, T, r = shape
    X, S = PR.make_state(n, T, r, seed)
    Y, planted = make_network(X, S, r, seed)
    return dict(X=X, S=S, Y=Y, planted=planted, mask=MR.random_mask(n, T, 0.3, seed=11 + seed))


def case_scores(case, r, **kw):
    """slice_scores of every slice of a make_case dict."""
    X, S, Y = case["X"], case["S"], case["Y"]
    return [slice_scores(X[:, t], S[:, t], r, Y[:, :, t], **kw) for t in range(X.shape[1])]
