"""ame_predict's argument checks and the host-side threshold rules (no GPU:
every misuse returns before any HIP call)."""
import ctypes
import os

import pytest


def _lib():
    from ame_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from ame_amd.build import build
        build(verbose=False)
    return L


def argument_error_cases(L):
    """(name, dims, args) of every listed misuse; the pointers are never dereferenced."""
    fake = ctypes.c_void_p(4096)
    good = dict(x=fake, cov=fake, work=fake)
    dims = L.ame_dims(16, 2, 3, 0, 3, L.AME_GOOD)
    mk = lambda **kw: L.ame_predict_args(**{**good, **kw})
    dense = dict(dense=fake, i0=0, i1=4, j0=0, j1=4)
    return [
        ("x NULL", dims, mk(x=None)),
        ("cov NULL", dims, mk(cov=None)),
        ("n_levels above the maximum", dims, mk(n_levels=L.AME_PREDICT_MAX_LEVELS + 1)),
        ("n_levels negative", dims, mk(n_levels=-1)),
        ("dense rows beyond n", dims, mk(**{**dense, "i1": 17})),
        ("dense columns negative", dims, mk(**{**dense, "j0": -1})),
        ("dense block empty", dims, mk(**{**dense, "i0": 4})),
        ("sums without Yt", dims, mk(sums=fake)),
        ("uncompiled r", L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD), mk()),
    ]


def check_argument_errors():
    L = _lib()
    lib = L.lib()
    for name, dims, args in argument_error_cases(L):
        rc = lib.ame_predict(ctypes.byref(dims), ctypes.byref(args), None)
        msg = lib.ame_last_error()
        assert rc < 0, name
        assert msg and len(msg) > 0, name
        assert b"ame" in msg, (name, msg)


def test_argument_errors_return_negative_with_message():
    check_argument_errors()


def test_exports_and_work_size():
    L = _lib()
    lib = L.lib()
    assert "ame_predict" in L.EXPORTS and "ame_predict_work_size" in L.EXPORTS
    assert L.AME_PREDICT_SUMS == 21
    # feature rows (floats) + 21 doubles per upper-triangle tile, per slice
    row = lambda r: 2 * ((r + 2 + 3) // 4 * 4) + 2 * ((2 + r * (r + 1) + 2 * r + 3) // 4 * 4) \
        + 2 * ((2 + 4 * r + 2 * r * r + 3) // 4 * 4)
    for n, T, r in ((2, 1, 1), (65, 3, 5), (1024, 128, 16), (97, 2, 32)):
        d = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
        nb = (n + 63) // 64
        want = (T * n * row(r) + 1) // 2 + T * (nb * (nb + 1) // 2) * 21
        assert lib.ame_predict_work_size(ctypes.byref(d)) == want
    bad = L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD)
    assert lib.ame_predict_work_size(ctypes.byref(bad)) == -1


def test_threshold_rules():
    from ame_amd.inference._device_vi import DeviceTemporalVI as D
    levels, zsq, csq = D._thresholds((0.5, 0.9, 0.95))
    assert levels == (0.5, 0.9, 0.95)
    assert abs(zsq[2] - 1.959963984540054 ** 2) < 1e-12
    assert abs(csq[1] - 4.605170185988092) < 1e-12
    with pytest.raises(ValueError):
        D._thresholds((0.1, 0.2, 0.3, 0.4, 0.5))
    for p in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            D._thresholds((p,))
