"""ame_net_moments / ame_net_triads / ame_simulate: argument checks and scratch
sizes (no GPU: every misuse returns before any HIP call)."""
import ctypes
import os


def _lib():
    from ame_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from ame_amd.build import build
        build(verbose=False)
    return L


def _dims(L, n=16, r=2, S=3, t0=0, T=3):
    return L.ame_dims(n, r, S, t0, T, L.AME_GOOD)


BAD_DIMS = (("uncompiled r", dict(r=999)), ("n < 2", dict(n=1)), ("slices beyond T_total", dict(t0=1)),
            ("T_local = 0", dict(S=0)))


def test_moments_and_triads_argument_errors():
    L = _lib()
    lib = L.lib()
    fake = ctypes.c_void_p(4096)
    for fn, Args, outs, need in (
            ("ame_net_moments", L.ame_moments_args, dict(node=fake, slice=fake), 3 * 16 * 2),
            ("ame_net_triads", L.ame_triads_args, dict(center=fake, tri=fake), 3 * 1 * 2)):
        call = getattr(lib, fn)
        good = dict(Yt=fake, work=fake, work_doubles=need, **outs)
        cases = [(f"{k} NULL", _dims(L), Args(**{**good, k: None})) for k in ("Yt", "work", *outs)]
        cases.append(("short work", _dims(L), Args(**{**good, "work_doubles": need - 1})))
        cases.append(("misaligned Yt", _dims(L), Args(**{**good, "Yt": ctypes.c_void_p(4096 + 8)})))
        cases.append(("misaligned work", _dims(L), Args(**{**good, "work": ctypes.c_void_p(4096 + 4)})))
        cases += [(name, _dims(L, **kw), Args(**good)) for name, kw in BAD_DIMS]
        for name, dims, args in cases:
            rc = call(ctypes.byref(dims), ctypes.byref(args), None)
            msg = lib.ame_last_error()
            assert rc < 0, (fn, name)
            assert msg and b"ame" in msg, (fn, name, msg)
        assert call(ctypes.byref(_dims(L)), None, None) < 0
        assert fn.encode() in lib.ame_last_error()
        assert call(None, ctypes.byref(Args(**good)), None) < 0


def test_simulate_argument_errors():
    L = _lib()
    lib = L.lib()
    fake = ctypes.c_void_p(4096)
    lr = (ctypes.c_double * 3)(1.0, 0.2, 0.9)
    good = dict(x=fake, lr=lr, seed=7, sample=1, Yt_out=ctypes.c_void_p(1 << 20))
    mk = lambda **kw: L.ame_simulate_args(**{**good, **kw})
    cases = [("x NULL", _dims(L), mk(x=None)), ("Yt_out NULL", _dims(L), mk(Yt_out=None)),
             ("misaligned Yt_out", _dims(L), mk(Yt_out=ctypes.c_void_p((1 << 20) + 8))),
             ("misaligned x", _dims(L), mk(x=ctypes.c_void_p(4096 + 2))),
             ("NaN in lr", _dims(L), mk(lr=(ctypes.c_double * 3)(1.0, float("nan"), 1.0)))]
    cases += [(name, _dims(L, **kw), mk()) for name, kw in BAD_DIMS]
    for name, dims, args in cases:
        rc = lib.ame_simulate(ctypes.byref(dims), ctypes.byref(args), None)
        msg = lib.ame_last_error()
        assert rc < 0, name
        assert msg and b"ame" in msg, (name, msg)
    assert lib.ame_simulate(ctypes.byref(_dims(L)), None, None) < 0
    assert b"ame_simulate" in lib.ame_last_error()


def test_exports_and_work_sizes():
    L = _lib()
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include",
                               "ame_amd.h")).read()
    for name in ("ame_net_moments", "ame_net_triads", "ame_simulate", "ame_net_moments_work_size",
                 "ame_net_triads_work_size"):
        assert name in L.EXPORTS and name + "(" in header
    for n, T, r in ((2, 1, 1), (65, 3, 5), (128, 2, 2), (129, 2, 2), (1024, 128, 16), (97, 2, 32)):
        dm = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
        nb = (n + 127) // 128
        assert lib.ame_net_moments_work_size(ctypes.byref(dm)) == T * n * 2
        assert lib.ame_net_triads_work_size(ctypes.byref(dm)) == T * nb * nb * 2
        one = L.ame_dims(n, r, 1, T - 1, T, L.AME_GOOD)
        assert lib.ame_net_triads_work_size(ctypes.byref(one)) == nb * nb * 2
    bad = L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD)
    assert lib.ame_net_moments_work_size(ctypes.byref(bad)) == -1
    assert lib.ame_net_triads_work_size(ctypes.byref(bad)) == -1
    # the struct layouts the header declares
    assert ctypes.sizeof(L.ame_moments_args) == 40 and ctypes.sizeof(L.ame_triads_args) == 40
    assert ctypes.sizeof(L.ame_simulate_args) == 56 and L.ame_simulate_args.Yt_out.offset == 48
