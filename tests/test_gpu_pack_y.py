"""ame_pack_y through the C ABI: the packed layout and the mismatch counter,
bit for bit against tests/elbo_sums_ref.py (pack_layout, pack_mismatches).

Every comparison is on uint32 views, so NaN payloads and signed zeros count.
Yt starts as NaN: a word the kernel does not write shows.  The network is an
exactly swap-consistent one (generate_data_fast) with a known set of edits:
single components inside and outside the slice windows, both components of
one pair (one mismatch, not two), a pair (0.0, x) / (x, -0.0) that is equal as
floats and differs in bits, a pair carrying one NaN bit pattern on both sides
(no mismatch: the kernel compares bits), and the diagonal (no pair).
"""
import ctypes
import functools

import numpy as np
import pytest

import elbo_sums_ref as E

pytestmark = pytest.mark.gpu

T5 = 5
SMALL_N = (2, 3, 37, 64, 65)
WINDOWS = ((0, 5), (2, 4), (4, 5))
NAN_BITS = 0x7FC01234


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def edited_network(n, T):
    """(n, n, T, 2) fp32, swap-consistent apart from the edits of the module
    docstring; at n = 2 everything lands on the one pair (0, 1)."""
    from ame_amd import TemporalAMEModel
    m = TemporalAMEModel(n, T, 1, seed=5)
    m.generate_data_fast(seed=9)
    Y = m.Y.numpy().astype(np.float32).copy()
    assert E.pack_mismatches(Y, 0, T) == 0
    B = Y.view(np.uint32)                                 # NaNs are written as bit patterns
    last = n - 1
    Y[0, 1, 0, 0] += 0.5                                  # slice 0: one component, upper triangle
    x = Y[0, last, 1 % T, 1]
    Y[0, last, 1 % T], Y[last, 0, 1 % T] = (0.0, x), (x, -0.0)   # slice 1: equal floats, other bits
    if T > 2:
        Y[0, last, 2], Y[last, 0, 2] = (0.0, 2.5), (2.5, 0.0)     # slice 2: same NaN bits, no mismatch
        B[0, last, 2, 0] = B[last, 0, 2, 1] = NAN_BITS
        if n > 2:
            Y[last, 1, 2, 1] -= 0.25                              # ... and a lower-triangle edit
    if T > 3:
        Y[0, last, 3] += np.float32(1.0)                          # slice 3: both components, one pair
    if T > 4:
        Y[0, 0, 4, 0] = 7.0                                       # slice 4: the diagonal is no pair
        B[0, 0, 4, 1] = NAN_BITS
        Y[last, last, 4, 0] = -0.0
        if n > 2:
            Y[1, last, 4, 0] += 0.125
            B[1, 0, 4, 1] = NAN_BITS                              # NaN on one side only
    assert np.isnan(Y).sum() == (0 if T <= 2 else 2 if T <= 4 else 3 + (n > 2))
    return Y


class _Packer:
    def __init__(self, n, T):
        import torch
        from ame_amd import _lib
        self.L, self.lib = _lib, _lib.lib()
        self.n, self.T = n, T
        self.dev = torch.device("cuda", 0)
        self.Y = edited_network(n, T)
        self.Yd = torch.from_numpy(self.Y).to(self.dev)

    def dims(self, t0, t1):
        return self.L.ame_dims(self.n, 1, t1 - t0, t0, self.T, self.L.AME_GOOD)

    def pack(self, t0, t1, start=0, counter=True):
        """(Yt as uint32 [T_local][n][ny][2], final counter value or None)."""
        import torch
        n = self.n
        dims = self.dims(t0, t1)
        size = int(self.lib.ame_pack_y_size(ctypes.byref(dims)))
        ny = n + (n & 1)
        assert size == (t1 - t0) * n * ny * 2
        Yt = torch.full((size,), float("nan"), dtype=torch.float32, device=self.dev)
        mm = torch.full((1,), start, dtype=torch.int64, device=self.dev) if counter else None
        torch.cuda.synchronize()
        self.L.check(self.lib.ame_pack_y(_ptr(self.Yd), _ptr(Yt), ctypes.byref(dims), _ptr(mm), None),
                     "ame_pack_y")
        torch.cuda.synchronize()
        bits = Yt.cpu().numpy().view(np.uint32).reshape(t1 - t0, n, ny, 2)
        return bits, (int(mm.item()) if counter else None)


@functools.lru_cache(maxsize=None)
def _packer(n, T):
    return _Packer(n, T)


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "t%d_%d" % w)
@pytest.mark.parametrize("n", SMALL_N)
def test_layout_and_counter(n, window, gpu_device):
    pk = _packer(n, T5)
    t0, t1 = window
    want = E.pack_layout(pk.Y, t0, t1)
    count = E.pack_mismatches(pk.Y, t0, t1)
    bits, got = pk.pack(t0, t1)
    assert np.array_equal(bits, want)
    if n & 1:
        assert (bits[:, :, n] == 0).all()               # the pad pair is +0.0, not -0.0 or NaN
    assert got == count, (got, count)
    # the counter accumulates
    bits7, got7 = pk.pack(t0, t1, start=7)
    assert got7 == 7 + count and np.array_equal(bits7, want)
    # mismatch = NULL is accepted and changes no word of Yt
    bits0, none = pk.pack(t0, t1, counter=False)
    assert none is None and np.array_equal(bits0, want)


@pytest.mark.parametrize("n", SMALL_N)
def test_counts_add_over_windows(n, gpu_device):
    pk = _packer(n, T5)
    whole = pk.pack(0, 5)[1]
    a, b = pk.pack(0, 2)[1], pk.pack(2, 5)[1]
    assert a + b == whole == E.pack_mismatches(pk.Y, 0, 5)
    # the edits are where the docstring says: by slice, as numpy counts them
    per = [E.pack_mismatches(pk.Y, t, t + 1) for t in range(5)]
    assert per == ([1, 1, 0, 1, 0] if n == 2 else [1, 1, 1, 1, 2]), per
    assert [pk.pack(t, t + 1)[1] for t in range(5)] == per


def test_grid_stride_loop(gpu_device):
    """n = 1025, T = 3: 1025 x 1026 x 3 elements, more than 8192 x 256, so the
    capped grid walks the array more than once; odd n, so every row ends in a
    pad pair."""
    n, T = 1025, 3
    assert n * (n + 1) * T > 8192 * 256
    pk = _Packer(n, T)
    bits, got = pk.pack(0, T)
    assert np.array_equal(bits, E.pack_layout(pk.Y, 0, T))
    assert got == E.pack_mismatches(pk.Y, 0, T) == 3


def test_engine_sees_a_mismatch_in_one_slice(gpu_device):
    """One mismatching pair in one slice makes an unsharded engine drop the
    swap-consistent shortcut."""
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI
    for edit in (False, True):
        m = TemporalAMEModel(37, T5, 2, seed=5)
        m.generate_data_fast(seed=9)
        if edit:
            m.Y[30, 4, 3, 1] += 0.5
        vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.3, device=gpu_device)
        assert vi.engine.swap_consistent == (not edit)
