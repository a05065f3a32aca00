"""ame_probit_fill / ame_probit_score: ctypes struct layouts, work sizes and
argument checks (no GPU: every misuse returns before any HIP call)."""
import ctypes
import os
import re


def _lib():
    from ame_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from ame_amd.build import build
        build(verbose=False)
    return L


def _header():
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ame_amd.h")).read()


def _header_fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)(?:\[\d+\])?\s*$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]


def check_argument_errors():
    L = _lib()
    lib = L.lib()
    fake = ctypes.c_void_p(4096)
    dims = L.ame_dims(16, 2, 3, 0, 3, L.AME_GOOD)
    bad_dims = (("uncompiled r", L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD)),
                ("n < 2", L.ame_dims(1, 2, 3, 0, 3, L.AME_GOOD)),
                ("slices beyond T_total", L.ame_dims(16, 2, 3, 1, 3, L.AME_GOOD)))
    for name, bd in bad_dims:
        assert lib.ame_probit_fill_work_size(ctypes.byref(bd)) == -1 and b"ame" in lib.ame_last_error(), name
        assert lib.ame_probit_score_work_size(ctypes.byref(bd)) == -1, name
    assert lib.ame_probit_fill_work_size(None) == -1 and lib.ame_probit_score_work_size(None) == -1

    # ame_probit_fill
    ws = lib.ame_probit_fill_work_size(ctypes.byref(dims))
    full = dict(x=fake, Bt=fake, Mt=fake, rho=0.5, Yt=fake, stat=fake, work=fake, work_doubles=ws)
    for k in ("x", "Bt", "Yt", "stat", "work"):
        a = L.ame_probit_fill_args(**{**full, k: None})
        assert lib.ame_probit_fill(ctypes.byref(dims), ctypes.byref(a), None) != 0, k
        assert b"ame_probit_fill" in lib.ame_last_error() and b"NULL" in lib.ame_last_error(), k
    for rho in (1.0, -1.0, 1.5, float("nan"), float("inf")):
        a = L.ame_probit_fill_args(**{**full, "rho": rho})
        assert lib.ame_probit_fill(ctypes.byref(dims), ctypes.byref(a), None) != 0, rho
        assert b"rho" in lib.ame_last_error(), rho
    for k in ("Bt", "Mt", "Yt", "stat", "work"):
        a = L.ame_probit_fill_args(**{**full, k: ctypes.c_void_p(4096 + 4)})
        assert lib.ame_probit_fill(ctypes.byref(dims), ctypes.byref(a), None) != 0, k
        assert b"aligned" in lib.ame_last_error(), k
    a = L.ame_probit_fill_args(**{**full, "work_doubles": ws - 1})
    assert lib.ame_probit_fill(ctypes.byref(dims), ctypes.byref(a), None) != 0
    assert b"work" in lib.ame_last_error()
    assert lib.ame_probit_fill(ctypes.byref(dims), None, None) != 0 and b"ame_probit_fill" in lib.ame_last_error()
    for name, bd in bad_dims:
        a = L.ame_probit_fill_args(**full)
        assert lib.ame_probit_fill(ctypes.byref(bd), ctypes.byref(a), None) != 0, name

    # ame_probit_score
    ws = lib.ame_probit_score_work_size(ctypes.byref(dims))
    full = dict(x=fake, cov=fake, Yt=fake, sums=fake, work=fake, work_doubles=ws)
    for k in ("x", "cov", "Yt", "sums", "work"):
        a = L.ame_probit_score_args(**{**full, k: None})
        assert lib.ame_probit_score(ctypes.byref(dims), ctypes.byref(a), None) != 0, k
        assert b"ame_probit_score" in lib.ame_last_error() and b"NULL" in lib.ame_last_error(), k
    for name, kw, word in (("selector without a mask", dict(mask_select=L.AME_MASK_OBSERVED), b"Mt"),
                           ("hidden without a mask", dict(mask_select=L.AME_MASK_HIDDEN), b"Mt"),
                           ("unknown selector", dict(Mt=fake, mask_select=3), b"unknown"),
                           ("short work", dict(work_doubles=ws - 1), b"work")):
        a = L.ame_probit_score_args(**{**full, **kw})
        assert lib.ame_probit_score(ctypes.byref(dims), ctypes.byref(a), None) != 0, name
        msg = lib.ame_last_error()
        assert b"ame_probit_score" in msg and word in msg, (name, msg)
    assert lib.ame_probit_score(ctypes.byref(dims), None, None) != 0
    for name, bd in bad_dims:
        a = L.ame_probit_score_args(**full)
        assert lib.ame_probit_score(ctypes.byref(bd), ctypes.byref(a), None) != 0, name


def test_argument_errors_return_nonzero_with_message():
    check_argument_errors()


def test_exports_sizes_and_struct_mirrors():
    L = _lib()
    lib = L.lib()
    header = _header()
    for name in ("ame_probit_fill", "ame_probit_score", "ame_probit_fill_work_size", "ame_probit_score_work_size"):
        assert name in L.EXPORTS and name + "(" in header
        getattr(lib, name)
    for name, val in (("AME_PROBIT_STEPS", 2), ("AME_PROBIT_STATS", 4), ("AME_PROBIT_SUMS", 6)):
        assert f"#define {name} {val}" in header and getattr(L, name) == val
    assert [f[0] for f in L.ame_probit_fill_args._fields_] == _header_fields("ame_probit_fill_args") == \
        ["x", "Bt", "Mt", "rho", "Yt", "stat", "work", "work_doubles"]
    assert [f[0] for f in L.ame_probit_score_args._fields_] == _header_fields("ame_probit_score_args") == \
        ["x", "cov", "Yt", "sums", "work", "work_doubles", "Mt", "mask_select"]
    # LP64 layouts: pointers and doubles at 8-byte offsets, the trailing int32 padded
    assert ctypes.sizeof(L.ame_probit_fill_args) == 64 and L.ame_probit_fill_args.rho.offset == 24
    assert ctypes.sizeof(L.ame_probit_score_args) == 64 and L.ame_probit_score_args.mask_select.offset == 56
    # ame_predict_args is untouched by the new entry point
    assert [f[0] for f in L.ame_predict_args._fields_[-2:]] == ["Mt", "mask_select"]
    for n, T, r in ((2, 1, 1), (64, 2, 3), (65, 3, 5), (1024, 128, 16), (130, 2, 32)):
        dm = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
        nb = (n + 63) // 64
        tiles = nb * (nb + 1) // 2
        assert lib.ame_probit_fill_work_size(ctypes.byref(dm)) == T * tiles * 4
        feat = lib.ame_predict_work_size(ctypes.byref(dm)) - T * tiles * L.AME_PREDICT_SUMS
        assert lib.ame_probit_score_work_size(ctypes.byref(dm)) == feat + T * tiles * 6
