"""ame_mstep_stats' argument checks and scratch size (no GPU: every misuse
returns before any HIP call)."""
import ctypes
import os


def _lib():
    from ame_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from ame_amd.build import build
        build(verbose=False)
    return L


def argument_error_cases(L):
    """(name, dims, args) of every listed misuse; the pointers are never dereferenced."""
    fake = ctypes.c_void_p(4096)
    good = dict(x=fake, cov=fake, Yt=fake, state=fake, dyad=fake, work=fake)
    dims = L.ame_dims(16, 2, 3, 0, 3, L.AME_GOOD)
    later = L.ame_dims(16, 2, 2, 1, 3, L.AME_GOOD)
    mk = lambda **kw: L.ame_mstep_args(**{**good, **kw})
    return [
        ("x NULL", dims, mk(x=None)),
        ("cov NULL", dims, mk(cov=None)),
        ("work NULL", dims, mk(work=None)),
        ("state and dyad both NULL", dims, mk(state=None, dyad=None)),
        ("dyad without Yt", dims, mk(Yt=None)),
        ("t_begin > 0 without prev_final", later, mk()),
        ("uncompiled r", L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD), mk()),
        ("n < 2", L.ame_dims(1, 2, 3, 0, 3, L.AME_GOOD), mk()),
        ("slices beyond T_total", L.ame_dims(16, 2, 3, 1, 3, L.AME_GOOD), mk(prev_final=fake)),
        ("T_local < 1", L.ame_dims(16, 2, 0, 0, 3, L.AME_GOOD), mk()),
    ]


def check_argument_errors():
    L = _lib()
    lib = L.lib()
    for name, dims, args in argument_error_cases(L):
        rc = lib.ame_mstep_stats(ctypes.byref(dims), ctypes.byref(args), None)
        msg = lib.ame_last_error()
        assert rc < 0, name
        assert msg and b"ame" in msg, (name, msg)
    rc = lib.ame_mstep_stats(ctypes.byref(L.ame_dims(16, 2, 3, 0, 3, L.AME_GOOD)), None, None)
    assert rc < 0 and b"ame_mstep_stats" in lib.ame_last_error()


def test_argument_errors_return_negative_with_message():
    check_argument_errors()


def test_exports_and_work_size():
    L = _lib()
    lib = L.lib()
    assert "ame_mstep_stats" in L.EXPORTS and "ame_mstep_work_size" in L.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include",
                               "ame_amd.h")).read()
    assert "ame_mstep_stats(" in header and "ame_mstep_work_size(" in header
    # chunk partials [T][ceil(n / 32)][2][d][d] + feature rows (floats) + 4 doubles per
    # upper-triangle tile: the chunk count depends on n alone
    row = lambda r: 2 * ((r + 2 + 3) // 4 * 4) + 2 * ((2 + r * (r + 1) + 2 * r + 3) // 4 * 4) \
        + 2 * ((2 + 4 * r + 2 * r * r + 3) // 4 * 4)
    for n, T, r in ((2, 1, 1), (65, 3, 5), (1024, 128, 16), (97, 2, 32)):
        dm = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
        d = 2 + 2 * r
        nb = (n + 63) // 64
        want = T * ((n + 31) // 32) * 2 * d * d + (T * n * row(r) + 1) // 2 + T * (nb * (nb + 1) // 2) * 4
        assert lib.ame_mstep_work_size(ctypes.byref(dm)) == want
        # the same per slice wherever the slices sit in time
        one = L.ame_dims(n, r, 1, 0, T, L.AME_GOOD)
        mid = L.ame_dims(n, r, 1, T - 1, T, L.AME_GOOD)
        assert lib.ame_mstep_work_size(ctypes.byref(one)) == lib.ame_mstep_work_size(ctypes.byref(mid))
    bad = L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD)
    assert lib.ame_mstep_work_size(ctypes.byref(bad)) == -1
