"""ame_smooth's exports, scratch size, LDS size and argument checks (no GPU:
every misuse returns before any HIP call)."""
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
    good = dict(x=fake, Yt=fake, consts=fake, mean=fake, cov=fake, cross=fake, lag_sum=fake,
                fail=fake, work=fake, i0=0, i1=40, stages=0, work_doubles=1 << 40)
    dims = L.ame_dims(40, 2, 3, 0, 3, L.AME_GOOD)
    mk = lambda **kw: L.ame_smooth_args(**{**good, **kw})
    cases = [(f"{k} NULL", dims, mk(**{k: None}))
             for k in ("x", "Yt", "consts", "mean", "cov", "cross", "lag_sum", "fail", "work")]
    cases += [
        ("short work", dims, mk(work_doubles=10)),
        ("i0 not a multiple of 32", dims, mk(i0=8)),
        ("empty node range", dims, mk(i0=32, i1=32)),
        ("i1 > n", dims, mk(i1=41)),
        ("i0 < 0", dims, mk(i0=-32)),
        ("bad stages", dims, mk(stages=4)),
        ("time shard: t_begin > 0", L.ame_dims(40, 2, 2, 1, 3, L.AME_GOOD), mk()),
        ("time shard: T_local < T_total", L.ame_dims(40, 2, 2, 0, 3, L.AME_GOOD), mk()),
        ("uncompiled r", L.ame_dims(40, 999, 3, 0, 3, L.AME_GOOD), mk()),
        ("n < 2", L.ame_dims(1, 2, 3, 0, 3, L.AME_GOOD), mk(i1=1)),
        ("bad variant", L.ame_dims(40, 2, 3, 0, 3, 7), mk()),
        ("T_local < 1", L.ame_dims(40, 2, 0, 0, 3, L.AME_GOOD), mk()),
    ]
    return cases


def check_argument_errors():
    L = _lib()
    lib = L.lib()
    for name, dims, args in argument_error_cases(L):
        rc = lib.ame_smooth(ctypes.byref(dims), ctypes.byref(args), None)
        msg = lib.ame_last_error()
        assert rc < 0, name
        assert msg and b"ame" in msg, (name, msg)
    rc = lib.ame_smooth(ctypes.byref(L.ame_dims(40, 2, 3, 0, 3, L.AME_GOOD)), None, None)
    assert rc < 0 and b"ame_smooth" in lib.ame_last_error()


def test_argument_errors_return_negative_with_message():
    check_argument_errors()


def test_exports_sizes_and_lds():
    L = _lib()
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include",
                               "ame_amd.h")).read()
    for name in ("ame_smooth", "ame_smooth_work_size", "ame_smooth_lds_bytes"):
        assert name in L.EXPORTS and name + "(" in header
        assert hasattr(lib, name)
    assert "ame_smooth_args" in header
    # Gram statistics [T][1+2r][1+2r] + per node and slice h_obs, J^-1 g (d each) and J^-1 (d^2)
    for n, T, r in ((2, 1, 1), (65, 3, 5), (1024, 128, 16), (97, 2, 32)):
        dm = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
        d = 2 + 2 * r
        for nodes in (1, min(n, 32), n):
            want = T * (1 + 2 * r) ** 2 + nodes * T * (d * d + 2 * d)
            assert lib.ame_smooth_work_size(ctypes.byref(dm), nodes) == want
        assert lib.ame_smooth_work_size(ctypes.byref(dm), 0) == -1
        assert lib.ame_smooth_work_size(ctypes.byref(dm), n + 1) == -1
    bad = L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD)
    assert lib.ame_smooth_work_size(ctypes.byref(bad), 1) == -1
    # four d x (d+1) fp64 matrices and six d-vectors, within one CU's 160 KiB at every r
    for r in range(1, 33):
        d = 2 + 2 * r
        assert lib.ame_smooth_lds_bytes(r) == 8 * (4 * d * (d + 1) + 6 * d) <= 163840
    assert lib.ame_smooth_lds_bytes(16) == 39712 and lib.ame_smooth_lds_bytes(32) == 144672
    assert lib.ame_smooth_lds_bytes(0) == -1 and lib.ame_smooth_lds_bytes(33) == -1
