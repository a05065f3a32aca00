"""Residual diagnostics of a Gaussian fit: host int64 / fp64 arithmetic on the
per-node sums of ame_resid_nodes, the histograms of ame_resid_hist and the
records of ame_resid_select (include/ame_amd.h), the counterpart of
:mod:`ame_amd.links`.

The surprise of a pair is its Mahalanobis distance m2 = e' Sigma^-1 e under the
posterior-predictive N(E[mu], Sigma); under the model m2 is chi-square with two
degrees of freedom, so P(m2 > x) = exp(-x / 2) is the pair's p-value and a node's
mean m2 is 2.  The device bins m2 by

    b = floor(m2 * scale)  clamped to [0, bins - 1],   scale = bins / m2_max

(:func:`scale`, :func:`bin_of`): bin b covers [edges[b], edges[b + 1]) and the
last bin also holds what lies beyond m2_max and every NaN, so that a broken pair
ranks among the most surprising ones.
"""
from __future__ import annotations

import math

import numpy as np

MAX_BINS = 2048   # AME_RANK_MAX_BINS
NODE_SUMS = 9     # AME_NODE_SUMS
# ame_resid_record
RECORD = np.dtype([("m2", "<f8"), ("z0", "<f8"), ("z1", "<f8"), ("slice", "<i4"), ("i", "<i4"), ("j", "<i4"),
                   ("pad", "<i4")])


def check_bins(bins, m2_max):
    """(bins, m2_max) as int and float; ValueError outside 1 .. MAX_BINS / m2_max <= 0."""
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= MAX_BINS:
        raise ValueError(f"bins must be an integer in 1 .. {MAX_BINS} (got {bins!r})")
    m2_max = float(m2_max)
    if not (m2_max > 0.0 and math.isfinite(m2_max)):
        raise ValueError(f"m2_max must be positive and finite (got {m2_max!r})")
    return int(bins), m2_max


def scale(bins: int, m2_max: float) -> float:
    """The fp64 factor of the bin rule, bins / m2_max: computed once, here, and
    passed to the device."""
    return float(np.float64(bins) / np.float64(m2_max))


def edges(bins: int, m2_max: float):
    """(bins + 1,) fp64 bin edges b (m2_max / bins)."""
    return np.arange(bins + 1, dtype=np.float64) * (float(m2_max) / bins)


def bin_of(m2, bins: int, m2_max: float):
    """The device's bin of m2 (fp64): a multiply, floor, clamp; NaN -> bins - 1."""
    m2 = np.asarray(m2, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        fb = np.floor(m2 * np.float64(scale(bins, m2_max)))
        fb = np.where(fb <= float(bins - 1), np.maximum(fb, 0.0), float(bins - 1))
    return fb.astype(np.int64)


def node_dict(node) -> dict:
    """node_check's dictionary from the device's (T, n, NODE_SUMS) sums."""
    s = np.asarray(node, dtype=np.float64)
    if s.ndim != 3 or s.shape[2] != NODE_SUMS:
        raise ValueError(f"node sums have shape {s.shape}, expected (T, n, {NODE_SUMS})")
    pairs = s[:, :, 0].astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(pairs > 0, s[:, :, 2] / np.where(pairs > 0, pairs, 1), np.nan)
    return {"pairs": pairs, "log_score": s[:, :, 1].copy(), "mahalanobis": s[:, :, 2].copy(),
            "z2": s[:, :, 3:5].copy(), "resid": s[:, :, 5:7].copy(), "sq_err": s[:, :, 7:9].copy(),
            "mean_mahalanobis": mean}


def expected(pairs, bins: int, m2_max: float):
    """(T, bins) fp64: the counts the model expects, pairs (exp(-lo / 2) - exp(-hi / 2))
    per bin [lo, hi), the last bin open (hi = infinity)."""
    ed = edges(bins, m2_max)
    surv = np.exp(-0.5 * ed)
    surv[-1] = 0.0
    return np.asarray(pairs, dtype=np.float64)[:, None] * (surv[:-1] - surv[1:])[None, :]


def histogram(hist, bins: int, m2_max: float) -> dict:
    """residual_histogram's dictionary from the device's (T, bins) counts."""
    hist = np.asarray(hist).astype(np.int64)
    if hist.ndim != 2 or hist.shape[1] != bins:
        raise ValueError(f"hist has shape {hist.shape}, expected (T, {bins})")
    pairs = hist.sum(1)
    return {"edges": edges(bins, m2_max), "hist": hist, "expected": expected(pairs, bins, m2_max), "pairs": pairs}


def threshold(hist, k: int):
    """(bin_min (T,) int32, capacity (T,) int64) of a top-k selection: bin_min[t] is
    the largest b with sum_{b' >= b} hist[t, b'] >= k, 0 if fewer than k exist, and
    capacity[t] that sum."""
    hist = np.asarray(hist).astype(np.int64)
    if int(k) < 1:
        raise ValueError(f"k must be at least 1 (got {k!r})")
    above = np.cumsum(hist[:, ::-1], axis=1)[:, ::-1]            # pairs in bins >= b
    bin_min = np.maximum((above >= int(k)).sum(1) - 1, 0)
    capacity = above[np.arange(hist.shape[0]), bin_min]
    return bin_min.astype(np.int32), capacity.astype(np.int64)


def order(r):
    """Indices that sort records by (NaN first, -m2, i, j): a total order within a slice."""
    nan = np.isnan(r["m2"])
    key = np.where(nan, 0.0, -r["m2"])
    return np.lexsort((r["j"], r["i"], key, ~nan))


def top_k(records, offset, k: int) -> dict:
    """The k most surprising records of every slice: ``i``, ``j`` (T, k) int64
    padded with -1, ``m2``, ``p_value`` (T, k) and ``z`` (T, k, 2) fp64 padded
    with NaN.  ``records`` is a RECORD array whose slice t occupies
    [offset[t], offset[t + 1]) in any order."""
    records = np.asarray(records)
    T, k = len(offset) - 1, int(k)
    out = {name: np.full((T, k), -1, dtype=np.int64) for name in ("i", "j")}
    out["m2"] = np.full((T, k), np.nan, dtype=np.float64)
    out["z"] = np.full((T, k, 2), np.nan, dtype=np.float64)
    for t in range(T):
        r = records[int(offset[t]):int(offset[t + 1])]
        r = r[order(r)][:k]
        m = len(r)
        out["i"][t, :m], out["j"][t, :m], out["m2"][t, :m] = r["i"], r["j"], r["m2"]
        out["z"][t, :m, 0], out["z"][t, :m, 1] = r["z0"], r["z1"]
    out["p_value"] = np.exp(-0.5 * out["m2"])
    return out
