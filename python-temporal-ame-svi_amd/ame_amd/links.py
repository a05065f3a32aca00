"""Link ranking of a binary network: host int64 / fp64 arithmetic on the class
histograms of ame_probit_rank and the records of ame_probit_select
(include/ame_amd.h), the counterpart of :mod:`ame_amd.gof`.

The score of a directed entry is t = E[mu] / sqrt(1 + V0); pi = Phi(t) is
monotone in it, so every ranking is done on t.  Class 1 is a tie.  The device
bins t by

    b = floor((t + t_max) * scale)  clamped to [0, bins - 1],   scale = bins / (2 t_max)

(:func:`scale`, :func:`bin_of`), so bin b covers [edges[b], edges[b + 1]) and the
two end bins also hold what lies beyond +- t_max.  ``hist`` is (T, 2, bins):
hist[t, c, b] entries of slice t and class c in bin b.

Why binning is acceptable.  The exact (Mann-Whitney) AUC of the scores, ties
counted one half, is (sum over positive-negative pairs of 1[t+ > t-] + 1/2
1[t+ = t-]) / (P N).  A pair whose two scores fall into different bins is
ordered by the bins exactly as by the scores; only a pair inside one bin is
undecided.  ``auc_lo`` counts every such pair as lost and ``auc_hi`` as won, so
the exact AUC of the device's scores always lies in [auc_lo, auc_hi], whatever
the bins are; ``auc`` is their mean (pairs inside a bin count one half) and
auc_hi - auc_lo is the price of the binning, known to the caller.
"""
from __future__ import annotations

import math

import numpy as np

MAX_BINS = 2048   # AME_RANK_MAX_BINS
# ame_link_record
RECORD = np.dtype([("t", "<f8"), ("slice", "<i4"), ("sender", "<i4"), ("receiver", "<i4"), ("tie", "<i4")])
CURVES = ("fpr", "tpr", "precision", "recall")
SCALARS = ("auc", "auc_lo", "auc_hi", "average_precision")


def check_bins(bins, t_max):
    """(bins, t_max) as int and float; ValueError outside 1 .. MAX_BINS / t_max <= 0."""
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= MAX_BINS:
        raise ValueError(f"bins must be an integer in 1 .. {MAX_BINS} (got {bins!r})")
    t_max = float(t_max)
    if not (t_max > 0.0 and math.isfinite(t_max)):
        raise ValueError(f"t_max must be positive and finite (got {t_max!r})")
    return int(bins), t_max


def scale(bins: int, t_max: float) -> float:
    """The fp64 factor of the bin rule, bins / (2 t_max): computed once, here, and
    passed to the device."""
    return float(np.float64(bins) / (np.float64(2.0) * np.float64(t_max)))


def edges(bins: int, t_max: float):
    """(bins + 1,) fp64 bin edges -t_max + b (2 t_max / bins)."""
    return -float(t_max) + np.arange(bins + 1, dtype=np.float64) * (2.0 * float(t_max) / bins)


def bin_of(t, bins: int, t_max: float):
    """The device's bin of scores t (fp64): an add, a multiply, floor, clamp; NaN -> 0."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        fb = np.floor((t + np.float64(t_max)) * np.float64(scale(bins, t_max)))
        fb = np.where(fb >= 0.0, np.minimum(fb, float(bins - 1)), 0.0)
    return fb.astype(np.int64)


def _curves_one(h):
    """One (2, bins) int64 histogram -> dict of the scalars and the curves."""
    neg, pos = h[0], h[1]
    B = neg.shape[0]
    P, N = int(pos.sum()), int(neg.sum())
    out = {"positives": P, "negatives": N}
    nan = float("nan")
    if P == 0 or N == 0:
        for k in SCALARS:
            out[k] = nan
        for k in CURVES:
            out[k] = np.full(B + 1, nan)
        return out
    # counts at or above edge e (threshold "bin >= e"), e = 0 .. B
    tp = np.concatenate([np.cumsum(pos[::-1])[::-1], [0]]).astype(np.int64)
    fp = np.concatenate([np.cumsum(neg[::-1])[::-1], [0]]).astype(np.int64)
    neg_below = np.concatenate([[0], np.cumsum(neg)[:-1]]).astype(np.int64)
    num_lo = int((pos * neg_below).sum())
    num_tie = int((pos * neg).sum())
    den = P * N
    out["auc_lo"] = num_lo / den
    out["auc_hi"] = (num_lo + num_tie) / den
    out["auc"] = 0.5 * (out["auc_lo"] + out["auc_hi"])
    tpr = tp / float(P)
    called = tp + fp
    precision = np.where(called > 0, tp / np.where(called > 0, called, 1).astype(np.float64), 1.0)
    out["tpr"], out["recall"], out["fpr"], out["precision"] = tpr, tpr.copy(), fp / float(N), precision
    # the step sum from the top: sum_e (recall[e] - recall[e + 1]) precision[e], added
    # one after another from e = bins - 1 down (cumsum is sequential)
    out["average_precision"] = float(np.cumsum(((tpr[:-1] - tpr[1:]) * precision[:-1])[::-1])[-1])
    return out


def curves(hist) -> dict:
    """(T, 2, bins) histograms -> per slice ``positives`` / ``negatives`` (T,)
    int64, ``auc``, ``auc_lo``, ``auc_hi``, ``average_precision`` (T,) fp64 and
    ``fpr``, ``tpr``, ``precision``, ``recall`` (T, bins + 1) fp64.

    Index e of a curve is the threshold "bin >= e" (score >= edges[e] away from
    the end bins): e = 0 calls every entry a tie (tpr = fpr = 1), e = bins none
    (tpr = fpr = 0, precision 1 by convention); read from e = bins downwards the
    threshold comes down from the top.  auc_lo = sum_b pos_b (negatives in bins
    below b) / (P N) counts a positive-negative pair inside one bin as lost,
    auc_hi = auc_lo + sum_b pos_b neg_b / (P N) as won, auc is their mean: the exact
    Mann-Whitney AUC of the binned scores lies in [auc_lo, auc_hi] (module
    docstring).  average_precision is the step sum over the binned thresholds.
    A slice with no positive or no negative entry gives NaN, not an error."""
    hist = np.asarray(hist)
    if hist.ndim != 3 or hist.shape[1] != 2:
        raise ValueError(f"hist has shape {hist.shape}, expected (T, 2, bins)")
    hist = hist.astype(np.int64)
    rows = [_curves_one(hist[t]) for t in range(hist.shape[0])]
    out = {k: np.array([r[k] for r in rows], dtype=np.int64) for k in ("positives", "negatives")}
    for k in SCALARS:
        out[k] = np.array([r[k] for r in rows], dtype=np.float64)
    for k in CURVES:
        out[k] = np.stack([r[k] for r in rows]).astype(np.float64) if rows else np.zeros((0, hist.shape[2] + 1))
    return out


def roc(hist, bins: int, t_max: float) -> dict:
    """The public dictionary of link_roc from the device's histograms: ``edges``,
    ``hist``, ``pairs`` (entries / 2), :func:`curves` per slice, and the same
    under ``pooled`` for the histogram summed over the slices."""
    hist = np.asarray(hist).astype(np.int64)
    out = {"edges": edges(bins, t_max), "hist": hist, "pairs": hist.sum((1, 2)) // 2}
    out.update(curves(hist))
    tot = hist.sum(0, keepdims=True)
    pooled = {k: v[0] for k, v in curves(tot).items()}
    pooled["hist"], pooled["pairs"] = tot[0], int(tot.sum()) // 2
    out["pooled"] = pooled
    return out


def threshold(hist, k: int, ties=None):
    """(bin_min (T,) int32, capacity (T,) int64) of a top-k selection: bin_min[t] is
    the largest b with sum_{b' >= b} h[t, b'] >= k, 0 if fewer than k exist, and
    capacity[t] that sum; h is the histogram of class ``ties`` (0 / 1), or of
    both classes (None)."""
    hist = np.asarray(hist).astype(np.int64)
    if ties not in (None, 0, 1):
        raise ValueError(f"ties must be None, 0 or 1 (got {ties!r})")
    if int(k) < 1:
        raise ValueError(f"k must be at least 1 (got {k!r})")
    h = hist.sum(1) if ties is None else hist[:, int(ties)]
    above = np.cumsum(h[:, ::-1], axis=1)[:, ::-1]            # entries in bins >= b
    bin_min = np.maximum((above >= int(k)).sum(1) - 1, 0)
    capacity = above[np.arange(h.shape[0]), bin_min]
    return bin_min.astype(np.int32), capacity.astype(np.int64)


def top_k(records, offset, k: int) -> dict:
    """The k best records of every slice, best first by (-score, sender,
    receiver): ``sender``, ``receiver``, ``tie`` (T, k) int64 padded with -1 and
    ``score`` (T, k) fp64 padded with NaN.  ``records`` is a RECORD array whose
    slice t occupies [offset[t], offset[t + 1]) in any order."""
    records = np.asarray(records)
    T, k = len(offset) - 1, int(k)
    out = {name: np.full((T, k), -1, dtype=np.int64) for name in ("sender", "receiver", "tie")}
    out["score"] = np.full((T, k), np.nan, dtype=np.float64)
    for t in range(T):
        r = records[int(offset[t]):int(offset[t + 1])]
        r = r[np.lexsort((r["receiver"], r["sender"], -r["t"]))][:k]
        m = len(r)
        out["sender"][t, :m], out["receiver"][t, :m], out["tie"][t, :m] = r["sender"], r["receiver"], r["tie"]
        out["score"][t, :m] = r["t"]
    return out


def phi(t):
    """Phi(t) = erfc(-t / sqrt 2) / 2 of an fp64 array (NaN stays NaN)."""
    t = np.asarray(t, dtype=np.float64)
    return 0.5 * np.vectorize(math.erfc, otypes=[np.float64])(-t * math.sqrt(0.5)) if t.size else t.copy()
