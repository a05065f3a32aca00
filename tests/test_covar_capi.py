"""ame_covar_stats / ame_covar_resid: argument checks and scratch size (no GPU:
every misuse returns before any HIP call)."""
import ctypes
import os


def _lib():
    from ame_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from ame_amd.build import build
        build(verbose=False)
    return L


def stats_error_cases(L):
    """(name, dims, args) of every listed misuse; the pointers are never dereferenced."""
    fake = ctypes.c_void_p(4096)
    dims = L.ame_dims(16, 2, 3, 0, 3, L.AME_GOOD)
    need = 3 * 1 * (4 * 3 + 4 * 9)      # T_local x tiles x (4 p + 4 p^2) at p = 3
    good = dict(x=fake, Yt=fake, Wt=fake, p=3, G=fake, H=fake, work=fake, work_doubles=need)
    mk = lambda **kw: L.ame_covar_args(**{**good, **kw})
    return [
        ("p = 0", dims, mk(p=0)),
        ("p = 9", dims, mk(p=9)),
        ("Wt NULL", dims, mk(Wt=None)),
        ("x NULL", dims, mk(x=None)),
        ("Yt NULL", dims, mk(Yt=None)),
        ("work NULL", dims, mk(work=None)),
        ("G and H both NULL", dims, mk(G=None, H=None)),
        ("short work", dims, mk(work_doubles=need - 1)),
        ("uncompiled r", L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD), mk()),
        ("n < 2", L.ame_dims(1, 2, 3, 0, 3, L.AME_GOOD), mk()),
        ("slices beyond T_total", L.ame_dims(16, 2, 3, 1, 3, L.AME_GOOD), mk()),
    ]


def check_argument_errors():
    L = _lib()
    lib = L.lib()
    for name, dims, args in stats_error_cases(L):
        rc = lib.ame_covar_stats(ctypes.byref(dims), ctypes.byref(args), None)
        msg = lib.ame_last_error()
        assert rc != 0, name
        assert msg and b"ame" in msg, (name, msg)
    dims = L.ame_dims(16, 2, 3, 0, 3, L.AME_GOOD)
    assert lib.ame_covar_stats(ctypes.byref(dims), None, None) != 0
    assert b"ame_covar_stats" in lib.ame_last_error()
    fake = ctypes.c_void_p(4096)
    other = ctypes.c_void_p(1 << 20)
    plane = 3 * 16 * 16 * 2 * 4                                   # bytes of one packed plane of `dims`
    beta = (ctypes.c_double * 8)(*([0.5] * 8))
    for name, a in (("p = 0", (fake, fake, beta, 0, other)), ("p = 9", (fake, fake, beta, 9, other)),
                    ("Yt_raw NULL", (None, fake, beta, 2, other)), ("Wt NULL", (fake, None, beta, 2, other)),
                    ("beta NULL", (fake, fake, None, 2, other)), ("Yt_out NULL", (fake, fake, beta, 2, None)),
                    ("Yt_out aliases Yt_raw", (fake, other, beta, 2, fake)),
                    ("Yt_out overlaps Yt_raw", (fake, other, beta, 2, ctypes.c_void_p(4096 + plane - 16))),
                    ("Yt_out aliases Wt's second plane", (fake, other, beta, 2, ctypes.c_void_p((1 << 20) + plane))),
                    ("misaligned Yt_out", (fake, other, beta, 2, ctypes.c_void_p((1 << 22) + 8))),
                    ("misaligned Wt", (fake, ctypes.c_void_p((1 << 20) + 4), beta, 2, ctypes.c_void_p(1 << 22)))):
        rc = lib.ame_covar_resid(ctypes.byref(dims), *a, None)
        assert rc != 0 and b"ame_covar_resid" in lib.ame_last_error(), name


def test_argument_errors_return_nonzero_with_message():
    check_argument_errors()


def test_exports_and_work_size():
    L = _lib()
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include",
                               "ame_amd.h")).read()
    for name in ("ame_covar_stats", "ame_covar_work_size", "ame_covar_resid"):
        assert name in L.EXPORTS and name + "(" in header
    assert "#define AME_MAX_COVARIATES 8" in header and L.AME_MAX_COVARIATES == 8
    for n, T, r, p in ((2, 1, 1, 1), (65, 3, 5, 3), (1024, 128, 16, 4), (97, 2, 32, 8)):
        dm = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
        nb = (n + 63) // 64
        assert lib.ame_covar_work_size(ctypes.byref(dm), p) == T * (nb * (nb + 1) // 2) * (4 * p + 4 * p * p)
        one = L.ame_dims(n, r, 1, 0, T, L.AME_GOOD)
        mid = L.ame_dims(n, r, 1, T - 1, T, L.AME_GOOD)
        assert lib.ame_covar_work_size(ctypes.byref(one), p) == lib.ame_covar_work_size(ctypes.byref(mid), p)
    dm = L.ame_dims(16, 2, 3, 0, 3, L.AME_GOOD)
    assert lib.ame_covar_work_size(ctypes.byref(dm), 0) == -1
    assert lib.ame_covar_work_size(ctypes.byref(dm), 9) == -1
    assert lib.ame_covar_work_size(ctypes.byref(L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD)), 2) == -1
