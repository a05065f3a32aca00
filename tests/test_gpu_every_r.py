"""GPU parity of every sweep kernel at every latent dim it is compiled for,
through the C-ABI, against the fp64 oracle.

libame_amd.so holds one template instance per r = 1..32, per variant and per
sweep kind, and the instances differ in more than a loop bound:

* v2 (kinds 20-24, csrc/ame_sweep.hip): the lane mapping VEC = 4 / 2 / 1 (from
  r % 4, r % 2), CW = 2r / VEC, GW = 192 / CW (integer division: 13 at r = 14,
  5 at r = 17, 3 at r = 25) and the AR split 4 -> 2 parts between r = 23 and 24;
* v3 (kind 3, csrc/ame_sweep3.hip): NSREG = clamp(96 / 2r, 1, 16), NP, MC, MCP,
  the wave reduce-scatter over D = 2 + 2r values, and the LDS overflow node
  slots (slots s >= NSREG, nodes j >= 448 NSREG) that only r in {7..11, 13}
  can reach within the 160 KiB LDS.

The matrix below runs every (kind, r) cell; tests/test_every_r_guard.py (no
GPU) holds the parameter lists to "every r" so an edit cannot thin them.

Reference: structured_mf.py:211-326, naive_mf.py:207-282.  Tolerances are those
of tests/test_gpu_large.py (_check_vs_oracle, with the four ELBO terms), lr 0.5;
the fp32 allowance of that check is capped at FP32_CAP here, so the bound on the
kernel is max(5e-6 scale, 1.5 fp32_err) with fp32_err <= 1e-4 scale asserted
from the CPU oracle alone.

Measured on an MI355X when this file was written: 321 cases in 37 s (0.1 s
typical, the overflow shapes 1.6 - 4.3 s, most of it the CPU oracle); largest
err / fp32_err 1.21 (kind 20, r = 4, good); largest fp32_err 0.51 of the cap
((70, 3), r = 31, bad); every overflow shape accepted by v3 at the n listed.
"""
import ctypes

import pytest

from test_gpu_large import _check_vs_oracle

pytestmark = pytest.mark.gpu

VARIANTS = ("good", "bad", "naive")   # enum ame_variant order
ALL_R = tuple(range(1, 33))
V3_R = tuple(range(1, 24))            # what kind 3 accepts at V3_SHAPE (asserted below)
LR = 0.5
FP32_CAP = 1e-4

V3_SHAPE = (120, 3)       # two helper waves lit; still fits r = 23
V2_SHAPE = (70, 3)
# all seven helper waves and a partial second slot; r = 22 fits n <= 384 only
# (six helper waves), r = 23 is left to V3_SHAPE
V3_WAVES = tuple((380 if r == 22 else 460, 2, r, VARIANTS[r % 3]) for r in range(1, 23))
V3_MATRIX = tuple((r, v) for r in V3_R for v in VARIANTS)
WORKERS_MATRIX = tuple((r, v) for r in ALL_R for v in VARIANTS)
OTHER_V2_KINDS = (20, 21, 23, 24)
OTHER_V2 = tuple((k, r, VARIANTS[(r + k) % 3]) for k in OTHER_V2_KINDS for r in ALL_R)
# nodes past the register slots of the helper lanes: n > 448 * NSREG(r)
V3_OVERFLOW = ((1400, 2, 13, "good"), (1400, 2, 13, "bad"), (1400, 2, 13, "naive"),
               (2200, 2, 10, "bad"), (2900, 1, 8, "naive"))


def nsreg(r):
    """Cfg<R>::NSREG of csrc/ame_sweep3.hip (kMREG = 96 VGPRs for the slice):
    node slots a helper lane keeps in registers; further slots live in LDS."""
    return min(16, max(1, 96 // (2 * r)))


def _kind(n, T, r, request, method="good"):
    from ame_amd import _lib
    d = _lib.ame_dims(n, r, T, 0, T, VARIANTS.index(method))
    return int(_lib.lib().ame_sweep_kind(ctypes.byref(d), request))


def _run(n, T, r, method, kind, dev, iters, request=None):
    request = kind if request is None else request
    assert _kind(n, T, r, request, method) == kind, (n, T, r, method, request)
    vi = _check_vs_oracle(n, T, r, method, LR, dev, iters=iters, check_terms=True,
                          fp32_cap=FP32_CAP, sweep_kernel=request)
    assert vi.engine.sweep_kind == kind
    return vi


def test_v3_accepts_r_1_to_23(gpu_device):
    """The v3 fit bound at V3_SHAPE, from the library: one state row per solver
    lane would allow d <= 64 (r <= 31), the slice's LDS stops at r = 23."""
    n, T = V3_SHAPE
    for v in VARIANTS:
        got = tuple(r for r in ALL_R if _kind(n, T, r, 3, v) == 3)
        assert got == V3_R, (v, got)


@pytest.mark.parametrize("r,method", V3_MATRIX)
def test_v3_every_r_every_variant(r, method, gpu_device):
    n, T = V3_SHAPE
    _run(n, T, r, method, 3, gpu_device, 2)


@pytest.mark.parametrize("n,T,r,method", V3_WAVES)
def test_v3_all_helper_waves(n, T, r, method, gpu_device):
    _run(n, T, r, method, 3, gpu_device, 1)


@pytest.mark.parametrize("r,method", WORKERS_MATRIX)
def test_workers_every_r_every_variant(r, method, gpu_device):
    """Kind 22: what AME_SWEEP_AUTO picks past v3."""
    n, T = V2_SHAPE
    _run(n, T, r, method, 22, gpu_device, 2)


@pytest.mark.parametrize("kind,r,method", OTHER_V2)
def test_other_v2_kinds_every_r(kind, r, method, gpu_device):
    n, T = V2_SHAPE
    _run(n, T, r, method, kind, gpu_device, 2)


@pytest.mark.parametrize("n,T,r,method", V3_OVERFLOW)
def test_v3_lds_overflow_slots(n, T, r, method, gpu_device):
    """AME_SWEEP_AUTO at shapes whose last nodes sit in the LDS overflow slots
    (the s >= NSREG branches of the GEMV, its prologue fill and the per-step
    refresh of csrc/ame_sweep3.hip)."""
    assert n > 448 * nsreg(r)
    _run(n, T, r, method, 3, gpu_device, 1, request=0)
