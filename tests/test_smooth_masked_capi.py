"""ame_smooth with `Mt` set: the new export, its scratch size and the argument
checks (no GPU: every misuse returns before any HIP call)."""
import ctypes
import os

from test_smooth_capi import _lib, argument_error_cases


def masked_error_cases(L):
    """(name, dims, args): the misuses that exist only with a mask; the pointers are never dereferenced."""
    fake = ctypes.c_void_p(4096)
    n, r, T = 40, 2, 3
    dims = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
    lib = L.lib()
    plain = int(lib.ame_smooth_work_size(ctypes.byref(dims), n))
    masked = int(lib.ame_smooth_masked_work_size(ctypes.byref(dims), n))
    good = dict(x=fake, Yt=fake, consts=fake, mean=fake, cov=fake, cross=fake, lag_sum=fake,
                fail=fake, work=fake, i0=0, i1=n, stages=0, work_doubles=masked, Mt=fake)
    mk = lambda **kw: L.ame_smooth_args(**{**good, **kw})
    return [("work of the unmasked size", dims, mk(work_doubles=plain)),
            ("work one double short", dims, mk(work_doubles=masked - 1)),
            ("short work", dims, mk(work_doubles=10)),
            ("Mt not 8-byte aligned", dims, mk(Mt=ctypes.c_void_p(4100)))]


def check_argument_errors():
    L = _lib()
    lib = L.lib()
    for name, dims, args in masked_error_cases(L):
        rc = lib.ame_smooth(ctypes.byref(dims), ctypes.byref(args), None)
        msg = lib.ame_last_error()
        assert rc < 0, name
        assert msg and b"ame_smooth" in msg, (name, msg)
    # every misuse of the unmasked call is still one with Mt set
    fake = ctypes.c_void_p(4096)
    for name, dims, args in argument_error_cases(L):
        args.Mt = fake
        rc = lib.ame_smooth(ctypes.byref(dims), ctypes.byref(args), None)
        assert rc < 0 and b"ame" in lib.ame_last_error(), name


def test_argument_errors_return_negative_with_message():
    check_argument_errors()


def test_short_work_message_names_the_masked_size():
    L = _lib()
    lib = L.lib()
    name, dims, args = masked_error_cases(L)[0]
    assert lib.ame_smooth(ctypes.byref(dims), ctypes.byref(args), None) < 0
    assert b"ame_smooth_masked_work_size" in lib.ame_last_error()


def test_export_and_masked_work_size():
    L = _lib()
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include",
                               "ame_amd.h")).read()
    assert "ame_smooth_masked_work_size" in L.EXPORTS and "ame_smooth_masked_work_size(" in header
    assert hasattr(lib, "ame_smooth_masked_work_size")
    assert "const uint64_t* Mt" in header[header.index("typedef struct ame_smooth_args"):
                                          header.index("} ame_smooth_args;")]
    # Mt is the last field: a caller that zero-initialises the structure passes NULL
    assert L.ame_smooth_args._fields_[-1][0] == "Mt"
    assert L.ame_smooth_args().Mt is None
    for n, T, r in ((2, 1, 1), (65, 3, 5), (1024, 128, 16), (97, 2, 32)):
        dm = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
        d, W = 2 + 2 * r, 1 + 2 * r
        for nodes in (1, min(n, 32), n):
            plain = T * W * W + nodes * T * (d * d + 2 * d)
            assert lib.ame_smooth_work_size(ctypes.byref(dm), nodes) == plain       # unchanged
            assert lib.ame_smooth_masked_work_size(ctypes.byref(dm), nodes) == plain + nodes * T * W * W
        assert lib.ame_smooth_masked_work_size(ctypes.byref(dm), 0) == -1
        assert lib.ame_smooth_masked_work_size(ctypes.byref(dm), n + 1) == -1
        assert b"ame_smooth_masked_work_size" in lib.ame_last_error()
    bad = L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD)
    assert lib.ame_smooth_masked_work_size(ctypes.byref(bad), 1) == -1
    assert lib.ame_smooth_masked_work_size(ctypes.byref(L.ame_dims(16, 2, 0, 0, 3, L.AME_GOOD)), 1) == -1
    assert lib.ame_smooth_lds_bytes(16) == 39712 and lib.ame_smooth_lds_bytes(32) == 144672


def test_null_mask_calls_are_unaffected():
    """Mt = NULL: the unmasked size is enough, and the checks of the unmasked call
    hold as before (a structure built without the new field)."""
    L = _lib()
    lib = L.lib()
    for name, dims, args in argument_error_cases(L):
        assert args.Mt is None
        assert lib.ame_smooth(ctypes.byref(dims), ctypes.byref(args), None) < 0, name
    # with exactly the unmasked size, no check that belongs to the mask fires: the
    # first complaint of a call whose only defect is the stage word is about the stages
    fake = ctypes.c_void_p(4096)
    dims = L.ame_dims(40, 2, 3, 0, 3, L.AME_GOOD)
    plain = int(lib.ame_smooth_work_size(ctypes.byref(dims), 40))
    a = L.ame_smooth_args(x=fake, Yt=fake, consts=fake, mean=fake, cov=fake, cross=fake, lag_sum=fake,
                          fail=fake, work=fake, i0=0, i1=40, stages=4, work_doubles=plain)
    assert lib.ame_smooth(ctypes.byref(dims), ctypes.byref(a), None) < 0
    assert b"stages" in lib.ame_last_error()
