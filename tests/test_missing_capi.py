"""ame_mask_words / ame_pack_mask / ame_fill_missing and the mask fields of
ame_predict_args / ame_mstep_args: argument checks and sizes (no GPU: every
misuse returns before any HIP call)."""
import ctypes
import os


def _lib():
    from ame_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from ame_amd.build import build
        build(verbose=False)
    return L


def check_argument_errors():
    L = _lib()
    lib = L.lib()
    fake = ctypes.c_void_p(4096)
    dims = L.ame_dims(16, 2, 3, 0, 3, L.AME_GOOD)
    bad_dims = (("uncompiled r", L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD)),
                ("n < 2", L.ame_dims(1, 2, 3, 0, 3, L.AME_GOOD)),
                ("slices beyond T_total", L.ame_dims(16, 2, 3, 1, 3, L.AME_GOOD)))

    # ame_mask_words / ame_fill_work_size
    assert lib.ame_mask_words(ctypes.byref(dims)) == 3 * 16 * 1
    assert lib.ame_fill_work_size(ctypes.byref(dims)) == 3 * 1 * 2
    for name, bd in bad_dims:
        assert lib.ame_mask_words(ctypes.byref(bd)) == -1 and b"ame" in lib.ame_last_error(), name
        assert lib.ame_fill_work_size(ctypes.byref(bd)) == -1, name
    assert lib.ame_mask_words(None) == -1

    # ame_pack_mask(M, Mt, dims, pairs, deg, asym, stream)
    good = [fake, fake, ctypes.byref(dims), fake, fake, fake, None]
    for k, name in ((0, "M"), (1, "Mt"), (3, "pairs"), (4, "deg"), (5, "asym")):
        a = list(good)
        a[k] = None
        assert lib.ame_pack_mask(*a) != 0 and b"ame_pack_mask" in lib.ame_last_error(), name
    for k, name in ((1, "Mt"), (3, "pairs"), (5, "asym")):
        a = list(good)
        a[k] = ctypes.c_void_p(4096 + 4)
        assert lib.ame_pack_mask(*a) != 0 and b"aligned" in lib.ame_last_error(), name
    a = list(good)
    a[4] = ctypes.c_void_p(4096 + 2)
    assert lib.ame_pack_mask(*a) != 0 and b"aligned" in lib.ame_last_error()
    for name, bd in bad_dims:
        a = list(good)
        a[2] = ctypes.byref(bd)
        assert lib.ame_pack_mask(*a) != 0 and b"ame" in lib.ame_last_error(), name

    # ame_fill_missing
    full = dict(x=fake, Mt=fake, Yt=fake, corr=fake, work=fake)
    for k in full:
        a = L.ame_fill_args(**{**full, k: None})
        assert lib.ame_fill_missing(ctypes.byref(dims), ctypes.byref(a), None) != 0, k
        assert b"ame_fill_missing" in lib.ame_last_error(), k
    a = L.ame_fill_args(**{**full, "Mt": ctypes.c_void_p(4096 + 4)})
    assert lib.ame_fill_missing(ctypes.byref(dims), ctypes.byref(a), None) != 0
    assert b"aligned" in lib.ame_last_error()
    assert lib.ame_fill_missing(ctypes.byref(dims), None, None) != 0
    assert b"ame_fill_missing" in lib.ame_last_error()
    for name, bd in bad_dims:
        a = L.ame_fill_args(**full)
        assert lib.ame_fill_missing(ctypes.byref(bd), ctypes.byref(a), None) != 0, name

    # mask_select / Mt of ame_predict_args
    pa = dict(x=fake, cov=fake, Yt=fake, sums=fake, work=fake)
    for name, kw, word in (("selector without a mask", dict(mask_select=L.AME_MASK_OBSERVED), b"Mt"),
                           ("hidden without a mask", dict(mask_select=L.AME_MASK_HIDDEN), b"Mt"),
                           ("unknown selector", dict(Mt=fake, mask_select=3), b"unknown"),
                           ("negative selector", dict(Mt=fake, mask_select=-1), b"unknown"),
                           ("selector without sums", dict(Mt=fake, mask_select=L.AME_MASK_HIDDEN, sums=None,
                                                          dense=fake, i1=4, j1=4), b"sums")):
        a = L.ame_predict_args(**{**pa, **kw})
        assert lib.ame_predict(ctypes.byref(dims), ctypes.byref(a), None) != 0, name
        msg = lib.ame_last_error()
        assert b"ame_predict" in msg and word in msg, (name, msg)

    # mask_select / Mt of ame_mstep_args
    ma = dict(x=fake, cov=fake, Yt=fake, state=fake, dyad=fake, work=fake)
    for name, kw, word in (("selector without a mask", dict(mask_select=L.AME_MASK_OBSERVED), b"Mt"),
                           ("unknown selector", dict(Mt=fake, mask_select=7), b"unknown"),
                           ("selector without dyad", dict(Mt=fake, mask_select=L.AME_MASK_OBSERVED, dyad=None),
                            b"dyad")):
        a = L.ame_mstep_args(**{**ma, **kw})
        assert lib.ame_mstep_stats(ctypes.byref(dims), ctypes.byref(a), None) != 0, name
        msg = lib.ame_last_error()
        assert b"ame_mstep_stats" in msg and word in msg, (name, msg)


def test_argument_errors_return_nonzero_with_message():
    check_argument_errors()


def test_exports_sizes_and_struct_mirrors():
    L = _lib()
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include",
                               "ame_amd.h")).read()
    for name in ("ame_mask_words", "ame_pack_mask", "ame_fill_missing", "ame_fill_work_size"):
        assert name in L.EXPORTS and name + "(" in header
    assert "#define AME_MASK_OBSERVED 1" in header and L.AME_MASK_OBSERVED == 1
    assert "#define AME_MASK_HIDDEN 2" in header and L.AME_MASK_HIDDEN == 2
    # the two trailing fields, in the header's order
    assert [f[0] for f in L.ame_predict_args._fields_[-2:]] == ["Mt", "mask_select"]
    assert [f[0] for f in L.ame_mstep_args._fields_[-2:]] == ["Mt", "mask_select"]
    assert [f[0] for f in L.ame_fill_args._fields_] == ["x", "Mt", "Yt", "rinv", "corr", "work"]
    for n, T, r in ((2, 1, 1), (64, 2, 3), (65, 3, 5), (1024, 128, 16), (130, 2, 32)):
        dm = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
        nb = (n + 63) // 64
        assert lib.ame_mask_words(ctypes.byref(dm)) == T * n * nb
        assert lib.ame_fill_work_size(ctypes.byref(dm)) == T * (nb * (nb + 1) // 2) * 2
        mid = L.ame_dims(n, r, 1, T - 1, T, L.AME_GOOD)
        assert lib.ame_mask_words(ctypes.byref(mid)) == n * nb
