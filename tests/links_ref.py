"""fp64 numpy reference of the link ranking of binary networks (test-only;
imports nothing from ame_amd): the scores t = E[mu] / sqrt(1 + V0) by
probit_ref.score_rows' formulas, the bin rule of include/ame_amd.h, class
histograms, a brute-force Mann-Whitney AUC and a brute-force top-k.

The bound DELTA on |t_dev - t_ref| per entry.  The device forms E[mu] and V0
with fp32 MFMA products and everything after them in fp64.  The bounds
test_gpu_predictive.py holds those products to are predictive_ref.TOL x the
entry's sum of |elementary products| (abs_sums): dm for the mean, dv for V0.
With V_lo = V0 - dv > -1,

    |m' / sqrt(1 + V') - m / sqrt(1 + V)| <= dm / sqrt(1 + V_lo) + (|m| + dm) dv / (2 (1 + V_lo)^(3/2))

(the mean-value theorem in V, the derivative of (1 + V)^(-1/2) being largest at
V_lo), plus 2^-50 (1 + |t|) for the fp64 add, square root, division and the
rounding of the bin rule's add and multiply.  Nothing here is measured on the
kernels.
"""
import numpy as np

import missing_ref as MR
import predictive_ref as PR

T_MAX = 8.0


def scores(X, S, r, B, mask=None, select=0, with_delta=False):
    """Per slice dict(i, j (P,), t (P, 2) fp64, y (P, 2) bool[, delta (P, 2)]) over
    the selected pairs i < j; entry 0 is i -> j, entry 1 is j -> i."""
    X = np.asarray(X, np.float64)
    S = np.asarray(S, np.float64)
    n, T, _ = X.shape
    iu = np.triu_indices(n, 1)
    msk = np.zeros((n, n, T), bool) if mask is None else mask
    out = []
    for t in range(T):
        sel = MR._subset(msk[:, :, t], select, iu)
        i, j = iu[0][sel], iu[1][sel]
        mean, V0, _ = PR.moments(X[:, t], S[:, t], r)
        m = np.stack([mean[i, j, 0], mean[i, j, 1]], -1)
        v = np.stack([V0[i, j], V0[j, i]], -1)
        d = dict(i=i, j=j, t=m / np.sqrt(1.0 + v), y=np.stack([B[i, j, t], B[j, i, t]], -1).astype(bool))
        if with_delta:
            am, av, _ = PR.abs_sums(X[:, t], S[:, t], r)
            dm = PR.TOL * np.stack([am[i, j], am[j, i]], -1)
            dv = PR.TOL * np.stack([av[i, j], av[j, i]], -1)
            vlo = v - dv
            assert (vlo > -1.0).all()
            d["delta"] = dm / np.sqrt(1.0 + vlo) + (np.abs(m) + dm) * dv / (2.0 * (1.0 + vlo) ** 1.5) \
                + 2.0 ** -50 * (1.0 + np.abs(d["t"]))
        out.append(d)
    return out


def subset(d, mask_t, select):
    """One slice of scores() over every pair, restricted to the pairs `select`
    (0, missing_ref.OBSERVED, missing_ref.HIDDEN) picks under the (n, n) mask."""
    if not select:
        return d
    hid = MR.clean(mask_t[:, :, None])[d["i"], d["j"], 0]
    keep = hid if select == MR.HIDDEN else ~hid
    return {k: v[keep] for k, v in d.items()}


def edges(bins, t_max=T_MAX):
    return np.array([-t_max + b * (2.0 * t_max / bins) for b in range(bins + 1)])


def bin_of(t, bins, t_max=T_MAX):
    """b = floor((t + t_max) * scale) clamped to [0, bins - 1], scale = bins / (2 t_max) in fp64."""
    sc = np.float64(bins) / (np.float64(2.0) * np.float64(t_max))
    fb = np.floor((np.asarray(t, np.float64) + np.float64(t_max)) * sc)
    return np.clip(fb, 0, bins - 1).astype(np.int64)


def histograms(sc, bins, t_max=T_MAX):
    """(T, 2, bins) int64 from scores()' list: [t, c, b] entries of class c in bin b."""
    h = np.zeros((len(sc), 2, bins), np.int64)
    for t, d in enumerate(sc):
        b = bin_of(d["t"], bins, t_max)
        for c in (0, 1):
            np.add.at(h[t, c], b[d["y"] == bool(c)], 1)
    return h


def auc_exact(tp, tn):
    """Mann-Whitney AUC of positive scores tp against negative scores tn by
    brute force over every pair, ties one half; (wins, ties, pairs) as integers
    and the AUC (NaN without a pair)."""
    tp, tn = np.asarray(tp, np.float64).ravel(), np.asarray(tn, np.float64).ravel()
    wins = ties = 0
    for lo in range(0, len(tp), 512):
        blk = tp[lo:lo + 512, None]
        wins += int((blk > tn[None, :]).sum())
        ties += int((blk == tn[None, :]).sum())
    pairs = len(tp) * len(tn)
    return wins, ties, pairs, ((wins + 0.5 * ties) / pairs if pairs else float("nan"))


def curves_brute(h):
    """One (2, bins) histogram -> dict of integers by plain loops: tp[e], fp[e] at
    threshold "bin >= e" (e = 0 .. bins), P, N, num_lo, num_tie."""
    neg, pos = [int(v) for v in h[0]], [int(v) for v in h[1]]
    B = len(neg)
    tp = [sum(pos[e:]) for e in range(B + 1)]
    fp = [sum(neg[e:]) for e in range(B + 1)]
    num_lo = sum(pos[b] * sum(neg[:b]) for b in range(B))
    num_tie = sum(pos[b] * neg[b] for b in range(B))
    return dict(tp=tp, fp=fp, P=sum(pos), N=sum(neg), num_lo=num_lo, num_tie=num_tie)


def entries(d, ties=None):
    """Flat (score, sender, receiver, tie) arrays of one slice of scores(), of
    class `ties` only when it is 0 or 1."""
    t = np.concatenate([d["t"][:, 0], d["t"][:, 1]])
    snd = np.concatenate([d["i"], d["j"]])
    rcv = np.concatenate([d["j"], d["i"]])
    tie = np.concatenate([d["y"][:, 0], d["y"][:, 1]]).astype(np.int64)
    keep = np.ones(len(t), bool) if ties is None else tie == ties
    return t[keep], snd[keep], rcv[keep], tie[keep]


def top_k(d, k, ties=None):
    """The k best entries of one slice by (-score, sender, receiver), padded with
    -1 / NaN: dict(sender, receiver, tie (k,) int64, score (k,) fp64)."""
    t, snd, rcv, tie = entries(d, ties)
    order = sorted(range(len(t)), key=lambda e: (-t[e], snd[e], rcv[e]))[:k]
    out = dict(sender=np.full(k, -1, np.int64), receiver=np.full(k, -1, np.int64), tie=np.full(k, -1, np.int64),
               score=np.full(k, np.nan))
    m = len(order)
    out["sender"][:m], out["receiver"][:m], out["tie"][:m], out["score"][:m] = snd[order], rcv[order], tie[order], t[order]
    return out


def sandwich(hist_t, d, bins, t_max=T_MAX):
    """Whether one slice's device histogram (2, bins) is consistent with the
    reference scores under their per-entry bound: for every class and edge,
    #{t_ref + delta < edge} <= cumulative device count below the edge <=
    #{t_ref - delta < edge}.  Returns (ok, detail)."""
    ed = edges(bins, t_max)[1:-1]                       # interior edges: the end bins are clamped
    for c in (0, 1):
        m = d["y"] == bool(c)
        lo, hi = np.sort((d["t"] + d["delta"])[m]), np.sort((d["t"] - d["delta"])[m])
        cum = np.cumsum(hist_t[c])[:-1]
        least, most = np.searchsorted(lo, ed, side="left"), np.searchsorted(hi, ed, side="left")
        if int(hist_t[c].sum()) != int(m.sum()):
            return False, (c, "total", int(hist_t[c].sum()), int(m.sum()))
        bad = np.nonzero((cum < least) | (cum > most))[0]
        if len(bad):
            e = int(bad[0])
            return False, (c, e + 1, int(least[e]), int(cum[e]), int(most[e]))
    return True, None


def near_edge_share(d, bins, t_max=T_MAX):
    """Share of one slice's entries whose reference score lies within its delta of an interior edge."""
    ed = edges(bins, t_max)[1:-1]
    t, dl = d["t"].ravel(), d["delta"].ravel()
    if not len(t):
        return 0.0
    k = np.clip(np.searchsorted(ed, t), 0, len(ed) - 1)
    dist = np.minimum(np.abs(t - ed[k]), np.abs(t - ed[np.maximum(k - 1, 0)]))
    return float((dist <= dl).mean())
