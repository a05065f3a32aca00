"""Goodness of fit by network statistics: host fp64 arithmetic on the raw sums
of ame_net_moments / ame_net_triads (include/ame_amd.h), the counterpart of
:func:`ame_amd.mstep.combine_covar`.

For one slice of a directed network y_ij (i != j), N = n (n - 1):

    mean        ybar = sum y / N
    sd          s = sqrt(sum (y - ybar)^2 / (N - 1))
    sd_rowmean  sample sd over i of row_i / (n - 1)
    sd_colmean  the same for col_i
    dyad_dep    correlation of (y_ij, y_ji) over ordered pairs
    cycle_dep   tr(E E E)  / (n (n - 1) (n - 2) s^3),   E = Y - centre off the diagonal
    trans_dep   tr(E E' E) / (n (n - 1) (n - 2) s^3)

(the five statistics of the GOF panel of Hoff's ``amen`` for a complete
network).  The triad sums arrive centred by the fp32 number the kernel was
given (:func:`center32`, ybar rounded to fp32): the two triad statistics are
those of that centre.
"""
from __future__ import annotations

import numpy as np

NAMES = ("sd_rowmean", "sd_colmean", "dyad_dep", "cycle_dep", "trans_dep")


def center32(node, n: int):
    """The centre the triad kernel is given: ybar = sum_i row_i / N in fp64
    (rows added in order), rounded to fp32.  ``node`` is (T, n, 2)."""
    node = np.asarray(node, dtype=np.float64)
    tot = np.zeros(node.shape[0], dtype=np.float64)
    for i in range(node.shape[1]):
        tot += node[:, i, 0]
    return (tot / float(n * (n - 1))).astype(np.float32)


def combine(node, slice_sums, tri, n: int, total=None) -> dict:
    """Per-slice raw sums -> the statistics, fp64 (T,) arrays by name.

    node        (T, n, 2)  row_i, col_i
    slice_sums  (T, 2)     sum y^2, sum y_ij y_ji over ordered pairs
    tri         (T, 2)     sum (E E)_ij E_ji, sum (E E')_ij E_ji
    total       (T,)       sum y, or None: the rows are added here in order
    For n < 3 the triad statistics are NaN.
    """
    node = np.asarray(node, dtype=np.float64)
    q = np.asarray(slice_sums, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.float64)
    T = node.shape[0]
    N = float(n * (n - 1))
    if total is None:
        total = np.zeros(T, dtype=np.float64)
        for i in range(n):
            total += node[:, i, 0]
    total = np.asarray(total, dtype=np.float64)
    mean = total / N
    css = q[:, 0] - total * mean            # sum (y - ybar)^2
    cpp = q[:, 1] - total * mean            # sum (y_ij - ybar) (y_ji - ybar)
    var = css / (N - 1.0)
    sd = np.sqrt(var)
    rm = node[:, :, 0] / (n - 1.0)
    cm = node[:, :, 1] / (n - 1.0)
    out = {"mean": mean, "sd": sd,
           "sd_rowmean": np.sqrt(((rm - rm.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (n - 1.0)),
           "sd_colmean": np.sqrt(((cm - cm.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (n - 1.0))}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["dyad_dep"] = cpp / css
        if n >= 3:
            den = N * (n - 2.0) * sd ** 3
            out["cycle_dep"] = tri[:, 0] / den
            out["trans_dep"] = tri[:, 1] / den
        else:
            out["cycle_dep"] = np.full(T, np.nan)
            out["trans_dep"] = np.full(T, np.nan)
    return out


def stack(stats: dict) -> np.ndarray:
    """The five statistics of :func:`combine` as one (..., 5) array in NAMES order."""
    return np.stack([stats[k] for k in NAMES], axis=-1)


def quantile(observed: np.ndarray, simulated: np.ndarray) -> np.ndarray:
    """Share of the simulations (axis 0) at or below the observed value."""
    return (simulated <= observed[None]).mean(axis=0)
