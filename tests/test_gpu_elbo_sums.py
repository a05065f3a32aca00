"""ame_elbo through the C ABI on a constructed state, every one of its eight
sums against the fp64 reference tests/elbo_sums_ref.py, per slice range.

State: predictive_ref.make_state's means, a generated network packed with
ame_pack_y, elbo_sums_ref.make_params' asymmetric fp64 draw (no entry of Phi or
R_inv on the fp32 grid) and synthetic fp64 cov_terms (ame_elbo only adds them
up; ame_cov has its own test), so a swapped column or a term of the wrong slice
shows.  A range [t0, t1) with t0 > 0 is one call with t_begin = t0,
T_total = T and prev_final = x[t0 - 1].

Bounds (EPS = 2^-52, mag = the reference's sum of |summands| of the entry).
  out[1], out[3], out[5], out[6]: fp64 sums of T_local n cov_terms entries in
    some order: |got - ref| <= N EPS mag, N = T_local n.
  out[2], out[4]: per node, on fp32 inputs widened exactly,
      e_k = mu_k - (a0 + a1), a0, a1 FMA chains of d/2 products of Phi and mu_prev:
            |de_k| <= (d/2 + 2) u (|mu| + |Phi||mu_prev|)_k,  u = 2^-53
      r_k = (M e)_k, two FMA chains of d/2 and one add; q = sum_k e_k r_k, an
      FMA chain of d:
            |dq| <= (3d/2 + 1) u |e|'|M||e| + 2 |de|'|M||e|
                 <= (3d/2 + 2) u (|e|'|M||e| + 2 (|mu| + |Phi||mu_prev|)'|M||e|)
    which is below 4d fp64 operations' worth of the node's mag; adding the
    T_local n node terms in any order costs at most T_local n u of their
    magnitudes more, and the reference (64-bit-mantissa accumulation, rounded
    once) u mag.  Hence |got - ref| <= N EPS mag, N = 4d + T_local n.
  out[0], out[7]: fp32 products, the project's 5e-6 (test_gpu_pairs.py), here
    x mag and per range.  Whole range against the sum of T single-slice calls:
    every workgroup does the same (slice, strip) work in both, so the
    per-workgroup partials have the same bits and only the order of the fp64
    adds differs: B EPS mag, B the pair workgroups of the whole call.

What the node bound is worth, measured on the CPU with the reference itself on
this file's inputs (the figure is |change of out[4]| / bound over [0, T)):
  Phi rounded to fp32 once, shape (37, 3, 2):            ratio 2.3e+04
  e rounded to fp32 once, shape (37, 3, 2):              ratio 4.6e+02
  one node's transition term dropped, shape (130, 3, 5): ratio 3.4e+09 to
    1.1e+10 (slice 1 of node 129, 0, 64)
(the roundings are 2^-24 relative per entry and average out over the 74 node
terms; a systematic fp32 error, such as one fp32 product per term, costs more.)
"""
import ctypes
import functools

import numpy as np
import pytest

import elbo_sums_ref as E
import predictive_ref as PR

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
V1, V2 = 1, 2                      # enum ame_pairs_kernel_code
BASE_SHAPES = ((2, 1, 1), (37, 3, 2), (130, 3, 5), (257, 2, 16), (130, 8, 3))
POISON_SHAPES = ((130, 3, 5), (257, 2, 16))
# (shape, Y swap-consistent): the non-consistent states have two entries of Y
# mutated as in test_gpu_pairs.py, so the pair kernels walk every tile
CASES = tuple((s, True) for s in BASE_SHAPES) + (((130, 8, 3), False),) + tuple((s, False) for s in POISON_SHAPES)
EVERY_R = tuple((9, 3, r) for r in range(1, 33))
CID = lambda c: "n%d_T%d_r%d" % c[0] + ("" if c[1] else "-nonswap")
KID = lambda k: "v%d" % k


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ranges(T):
    if T == 1:
        return ((0, 1),)
    return ((0, T), (0, 1), (1, T)) + (((1, 2),) if T >= 3 else ())


class _Device:
    """The constructed state on the device in the layouts of include/ame_amd.h,
    its fp64 reference rows, and raw ame_elbo calls over slice ranges."""

    def __init__(self, shape, consistent=True):
        import torch
        from ame_amd import TemporalAMEModel, _lib
        self.L, self.lib = _lib, _lib.lib()
        n, T, r = self.shape = shape
        self.dev = torch.device("cuda", 0)
        self.X, _ = PR.make_state(n, T, r)
        m = TemporalAMEModel(n, T, r, seed=5)
        m.generate_data_fast(seed=9)
        self.Y = m.Y.numpy().astype(np.float32).copy()
        if not consistent:
            self.Y[1, n - 1, 0, 0] += 0.75
            self.Y[n - 2, 0, T - 1, 1] -= 0.5
        self.p = p = E.make_params(r)
        self.ct = E.synthetic_cov_terms(n, T, 0)
        self.rows, self.mags = E.slice_rows(self.X, self.ct, self.Y, p["S0inv"], p["Qinv"], p["Phi"], p["rinv"])
        self.x = torch.from_numpy(self.X).permute(1, 0, 2).contiguous().to(self.dev)
        self.ctd = torch.from_numpy(self.ct).to(self.dev)
        self.consts = torch.from_numpy(p["consts"]).contiguous().to(self.dev)
        self.phi = torch.from_numpy(p["Phi"]).contiguous().to(self.dev)
        self._poisoned = None
        self.Yt, mism = self.pack(self.Y)
        assert (mism == 0) == consistent
        self.swap = 1 if mism == 0 else 0
        self.nws = ((n + 63) // 64 + 1) // 2 if self.swap else (n + 63) // 64   # pair workgroups per slice

    def dims(self, t0, t1):
        n, T, r = self.shape
        return self.L.ame_dims(n, r, t1 - t0, t0, T, self.L.AME_GOOD)

    def pack(self, Y):
        import torch
        n, T, r = self.shape
        dims = self.dims(0, T)
        ysz = int(self.lib.ame_pack_y_size(ctypes.byref(dims)))
        Yt = torch.full((T, n, ysz // (2 * T * n), 2), float("nan"), dtype=torch.float32, device=self.dev)
        mm = torch.zeros(1, dtype=torch.int64, device=self.dev)
        Yd = torch.from_numpy(np.ascontiguousarray(Y)).to(self.dev)
        self.L.check(self.lib.ame_pack_y(_ptr(Yd), _ptr(Yt), ctypes.byref(dims), _ptr(mm), None), "ame_pack_y")
        torch.cuda.synchronize()
        return Yt, int(mm.item())

    def poisoned(self):
        """Yt of the same network with every Y[i, i, t, :] = NaN (packed once)."""
        if self._poisoned is None:
            self._poisoned = self._pack_poisoned()
        return self._poisoned

    def _pack_poisoned(self):
        Y = self.Y.copy()
        i = np.arange(self.shape[0])
        Y[i, i] = np.nan
        Yt, mism = self.pack(Y)
        assert (mism == 0) == bool(self.swap)     # the diagonal is no pair
        assert bool(Yt.isnan().any())
        return Yt

    def elbo(self, t0, t1, kernel, Yt=None, ct=None):
        """out[8] of one ame_elbo call over [t0, t1); `work` and `out` start as NaN."""
        import torch
        Yt = self.Yt if Yt is None else Yt
        ct = self.ctd if ct is None else ct
        dims = self.dims(t0, t1)
        ws = int(self.lib.ame_elbo_work_size(ctypes.byref(dims)))
        assert ws > 0
        work = torch.full((ws,), float("nan"), dtype=torch.float64, device=self.dev)
        out = torch.full((8,), float("nan"), dtype=torch.float64, device=self.dev)
        a = self.L.ame_elbo_args(
            Yt=_ptr(Yt[t0:t1]), x=_ptr(self.x[t0:t1]), prev_final=_ptr(self.x[t0 - 1]) if t0 > 0 else None,
            cov_terms=_ptr(ct[t0:t1]), consts=_ptr(self.consts), phi=_ptr(self.phi),
            rinv=(ctypes.c_double * 4)(*self.p["rinv"]), swap_consistent=self.swap,
            work=_ptr(work), out=_ptr(out), pairs_kernel=kernel)
        torch.cuda.synchronize()
        self.L.check(self.lib.ame_elbo(ctypes.byref(dims), ctypes.byref(a), None), "ame_elbo")
        torch.cuda.synchronize()
        return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _device(shape, consistent=True):
    return _Device(shape, consistent)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_range(dv, t0, t1, kernel, tag):
    """One call against the reference: derived bounds, exact zeros by global
    time, and a second call with the same bits."""
    n, T, r = dv.shape
    d, TL = 2 + 2 * r, t1 - t0
    got = dv.elbo(t0, t1, kernel)
    ref, mag = E.range_sums(dv.rows, dv.mags, t0, t1)
    assert np.isfinite(got).all(), (tag, got)
    N = {k: TL * n for k in (1, 3, 5, 6)}
    N.update({k: 4 * d + TL * n for k in (2, 4)})
    bound = np.array([5e-6 * mag[0]] + [N[k] * EPS * mag[k] for k in range(1, 7)] + [5e-6 * mag[7]])
    err = np.abs(got - ref)
    ratio = err / np.where(bound > 0, bound, 1.0)
    print(f"{tag} [{t0},{t1}) v{kernel}: err / bound = " + " ".join(f"{x:.2e}" for x in ratio))
    assert (err <= bound).all(), (tag, t0, t1, kernel, ratio)
    if t0 > 0:
        assert got[2] == 0.0 and got[3] == 0.0, (tag, got)
    else:
        assert got[2] > 0.0 and got[3] != 0.0
    if (t0, t1) == (0, 1):
        assert got[4] == 0.0 and got[5] == 0.0, (tag, got)
    else:
        assert got[4] > 0.0 and got[5] != 0.0
    again = dv.elbo(t0, t1, kernel)
    assert np.array_equal(_bits(again), _bits(got)), (tag, t0, t1, kernel)
    return got


@pytest.mark.parametrize("kernel", (V1, V2), ids=KID)
@pytest.mark.parametrize("case", CASES, ids=CID)
def test_sums_match_fp64_reference(case, kernel, gpu_device):
    dv = _device(*case)
    for t0, t1 in ranges(case[0][1]):
        _check_range(dv, t0, t1, kernel, CID(case))


@pytest.mark.parametrize("shape", EVERY_R, ids=lambda s: "r%d" % s[2])
def test_sums_at_every_latent_dim(shape, gpu_device):
    """D is a template parameter of the node kernel: every r from 1 to 32, over
    [0, 3) and over [1, 3) with prev_final."""
    dv = _device(shape)
    for t0, t1 in ((0, 3), (1, 3)):
        _check_range(dv, t0, t1, V2, "n%d_T%d_r%d" % shape)


@pytest.mark.parametrize("kernel", (V1, V2), ids=KID)
@pytest.mark.parametrize("case", CASES, ids=CID)
def test_pair_sums_of_whole_range_equal_the_slices(case, kernel, gpu_device):
    """out[0], out[7] of one call over [0, T) against the sum of T calls with
    T_local = 1, t_begin = t: the same per-workgroup partials, another workgroup
    index and another order of fp64 adds, so B EPS mag (module docstring).  A
    slice visited twice in place of a similar one hides inside 5e-6, not here.
    The node sums of the single-slice calls add up likewise."""
    dv = _device(*case)
    n, T, r = dv.shape
    whole = dv.elbo(0, T, kernel)
    parts = np.stack([dv.elbo(t, t + 1, kernel) for t in range(T)])
    _, mag = E.range_sums(dv.rows, dv.mags, 0, T)
    B = T * dv.nws
    total = parts.sum(0)
    for k in (0, 7):
        err, bound = abs(whole[k] - total[k]), B * EPS * mag[k]
        print(f"{CID(case)} v{kernel} out[{k}]: whole vs slices err / bound = {err / bound:.2e} (B = {B})")
        assert err <= bound, (k, whole[k], total[k])
        # each slice's own sum against its own reference row
        for t in range(T):
            assert abs(parts[t, k] - dv.rows[t, k]) <= 5e-6 * dv.mags[t, k], (k, t)
    for k in range(1, 7):   # both sides within their own bound of the same reference
        N = (4 * (2 + 2 * r) if k in (2, 4) else 0) + T * n
        assert abs(whole[k] - total[k]) <= 2 * N * EPS * mag[k], (k, whole[k], total[k])


@pytest.mark.parametrize("kernel", (V1, V2), ids=KID)
@pytest.mark.parametrize("consistent", (True, False), ids=("swap", "nonswap"))
@pytest.mark.parametrize("shape", POISON_SHAPES, ids=lambda s: "n%d_T%d_r%d" % s)
def test_diagonal_of_y_is_never_read_into_a_sum(shape, consistent, kernel, gpu_device):
    """The model has no Y_ii.  With every Y[i, i, t, :] = NaN all eight sums keep
    their bits: a masked lane is skipped, not multiplied by zero (the v2 kernel
    also substitutes the slice's first bytes, Y[0, 0], for chunks no pair needs)."""
    dv = _device(shape, consistent)
    T = shape[1]
    for t0, t1 in ((0, T), (1, T)):
        clean = dv.elbo(t0, t1, kernel)
        got = dv.elbo(t0, t1, kernel, Yt=dv.poisoned())
        assert np.isfinite(got).all(), got
        assert np.array_equal(_bits(got), _bits(clean)), (t0, t1, got, clean)


@pytest.mark.parametrize("where", ((0, 0), (1, 36), (2, 17)), ids=lambda w: "t%d_i%d" % w)
def test_nonfinite_logdet_reaches_out6_only(where, gpu_device):
    """One cov_terms[t, i, 0] = NaN makes out[6] NaN, -inf makes it -inf; the
    other seven sums keep their bits."""
    dv = _device((37, 3, 2))
    clean = dv.elbo(0, 3, V2)
    for bad in (float("nan"), float("-inf")):
        ct = dv.ctd.clone()
        ct[where[0], where[1], 0] = bad
        got = dv.elbo(0, 3, V2, ct=ct)
        assert np.isnan(got[6]) if bad != bad else got[6] == -np.inf, (bad, got[6])
        keep = [k for k in range(8) if k != 6]
        assert np.array_equal(_bits(got[keep]), _bits(clean[keep])), (bad, got, clean)
    # the slice range that does not hold the entry is untouched
    t = where[0]
    if t > 0:
        ct = dv.ctd.clone()
        ct[t, where[1], 0] = float("nan")
        assert np.array_equal(_bits(dv.elbo(0, t, V2, ct=ct)), _bits(dv.elbo(0, t, V2)))
