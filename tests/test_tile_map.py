"""csrc/ame_tile.h on the host: the dyad-tile enumeration and the workgroup ->
(slice, item) mapping that ame_predict, ame_mstep_stats, ame_covar_stats,
ame_fill_missing and ame_elbo share (no GPU: the hooks call the header's
__host__ __device__ functions on the host, no HIP call is made)."""
import ctypes
import os

import pytest

TILE = 64


def _lib():
    from ame_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from ame_amd.build import build
        build(verbose=False)
    lib = L.lib()
    pi = ctypes.POINTER(ctypes.c_int)
    lib.ame_debug_tri_tile.argtypes = [ctypes.c_int, ctypes.c_int, pi, pi]
    lib.ame_debug_tri_tile.restype = ctypes.c_longlong
    lib.ame_debug_slice_block.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, pi, pi]
    lib.ame_debug_slice_block.restype = None
    return lib


@pytest.mark.parametrize("n", [2, 63, 64, 65, 128, 129, 200, 4096])
def test_tri_tiles_are_the_upper_triangle_row_major(n):
    lib = _lib()
    nb = (n + TILE - 1) // TILE
    want = [(I * TILE, J * TILE) for I in range(nb) for J in range(I, nb)]
    assert len(want) == nb * (nb + 1) // 2
    I0, J0 = ctypes.c_int(-1), ctypes.c_int(-1)
    got = []
    for tile in range(len(want)):
        assert lib.ame_debug_tri_tile(tile, n, ctypes.byref(I0), ctypes.byref(J0)) == len(want)
        assert I0.value % TILE == 0 and J0.value % TILE == 0
        got.append((I0.value, J0.value))
    assert got == want


@pytest.mark.parametrize("per_slice", [1, 3, 10])
@pytest.mark.parametrize("S", [1, 3, 8, 16, 24])
def test_slice_block_is_a_bijection_with_slices_on_one_xcd(S, per_slice):
    lib = _lib()
    tl, item = ctypes.c_int(-1), ctypes.c_int(-1)
    seen = {}
    for b in range(S * per_slice):
        lib.ame_debug_slice_block(b, S, per_slice, ctypes.byref(tl), ctypes.byref(item))
        assert 0 <= tl.value < S and 0 <= item.value < per_slice
        seen.setdefault((tl.value, item.value), []).append(b)
        if S % 8:
            assert tl.value == b // per_slice and item.value == b % per_slice
        else:   # workgroup b runs on XCD b % 8
            assert b % 8 == tl.value // (S // 8)
    assert len(seen) == S * per_slice and all(len(v) == 1 for v in seen.values())
