"""The C ABI of the residual diagnostics without a GPU: the ctypes structures
against the header's fields, sizes and offsets, the work-size queries, and every
argument error, which returns before any HIP call with a message."""
import ctypes
import os
import re

import numpy as np

STRUCTS = ("ame_resid_nodes_args", "ame_resid_hist_args", "ame_resid_record", "ame_resid_select_args")
ENTRY = ("ame_resid_nodes", "ame_resid_hist", "ame_resid_select")
# LP64 size (= alignment) of the header's scalar types
SIZES = {"double": 8, "uint64_t": 8, "int64_t": 8, "int32_t": 4, "uint32_t": 4, "float": 4}


def _lib():
    from ame_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from ame_amd.build import build
        build(verbose=False)
    return L


def _header():
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ame_amd.h")).read()


def _header_layout(struct):
    """[(name, offset, size)] and the struct's size by the LP64 rules, from the header's text."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out, off, align = [], 0, 1
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)$", decl)
        assert m, decl
        for item in m.group(3).split(","):          # "z0, z1" declares two
            name, count = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item).groups()
            unit = 8 if m.group(2) else SIZES[m.group(1)]
            size = unit * int(count or 1)
            off = (off + unit - 1) // unit * unit
            out.append((name, off, size))
            off += size
            align = max(align, unit)
    return out, (off + align - 1) // align * align


def test_structures_mirror_the_header():
    L = _lib()
    header = _header()
    for s in STRUCTS:
        cls = getattr(L, s)
        layout, size = _header_layout(s)
        assert [f[0] for f in cls._fields_] == [f[0] for f in layout], s
        for name, off, sz in layout:
            fld = getattr(cls, name)
            assert (fld.offset, fld.size) == (off, sz), (s, name, fld.offset, fld.size, off, sz)
        assert ctypes.sizeof(cls) == size, (s, ctypes.sizeof(cls), size)
    assert ctypes.sizeof(L.ame_resid_record) == 40
    assert ctypes.sizeof(L.ame_resid_nodes_args) == 96 and ctypes.sizeof(L.ame_resid_hist_args) == 104
    assert ctypes.sizeof(L.ame_resid_select_args) == 136 and L.ame_resid_select_args.offset.offset == 112
    assert "#define AME_NODE_SUMS 9" in header and L.AME_NODE_SUMS == 9
    from ame_amd import residuals
    assert residuals.RECORD.itemsize == 40 and residuals.NODE_SUMS == 9
    assert [residuals.RECORD.fields[f[0]][1] for f in L.ame_resid_record._fields_] == \
        [getattr(L.ame_resid_record, f[0]).offset for f in L.ame_resid_record._fields_]
    assert residuals.MAX_BINS == L.AME_RANK_MAX_BINS
    # no existing struct changed
    assert ctypes.sizeof(L.ame_probit_rank_args) == 80 and ctypes.sizeof(L.ame_link_record) == 24


def test_exports_and_work_sizes():
    L = _lib()
    lib = L.lib()
    header = _header()
    for name in ENTRY:
        for nm in (name, name + "_work_size"):
            assert nm in L.EXPORTS and nm + "(" in header
            getattr(lib, nm)
    for n, T, r in ((2, 1, 1), (65, 3, 5), (1024, 128, 16), (97, 2, 32)):
        d = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
        feat = lib.ame_probit_rank_work_size(ctypes.byref(d))
        nb = (n + 63) // 64
        assert lib.ame_resid_hist_work_size(ctypes.byref(d)) == feat
        assert lib.ame_resid_select_work_size(ctypes.byref(d)) == feat
        assert lib.ame_resid_nodes_work_size(ctypes.byref(d)) == feat + T * (nb + 1) * n * 9
    bad = L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD)
    for name in ENTRY:
        assert getattr(lib, name + "_work_size")(ctypes.byref(bad)) == -1


def argument_error_cases(L):
    """(entry point, name, dims, args) of every listed misuse; the pointers are never dereferenced."""
    lib = L.lib()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    dims = L.ame_dims(16, 2, 3, 0, 3, L.AME_GOOD)
    big = 10 ** 9
    noise = (ctypes.c_double * 4)(1.0, 0.5, 0.5, 1.0)
    nan = (ctypes.c_double * 4)(1.0, float("nan"), 0.5, 1.0)
    base = dict(x=fake, cov=fake, Yt=fake, noise=noise, work=fake, work_doubles=big)
    good = {"ame_resid_nodes": dict(base, node=fake),
            "ame_resid_hist": dict(base, hist=fake, nbins=64, scale=2.0),
            "ame_resid_select": dict(base, nbins=64, scale=2.0, bin_min=fake, offset=fake, count=fake, records=fake)}
    cls = {k: getattr(L, k + "_args") for k in good}
    cases = []
    for ep, g in good.items():
        mk = lambda ep=ep, g=g, **kw: cls[ep](**{**g, **kw})
        small = int(getattr(lib, ep + "_work_size")(ctypes.byref(dims))) - 1
        cases += [(ep, "dims NULL", None, mk()), (ep, "args NULL", dims, None),
                  (ep, "uncompiled r", L.ame_dims(16, 999, 3, 0, 3, L.AME_GOOD), mk()),
                  (ep, "n below 2", L.ame_dims(1, 2, 3, 0, 3, L.AME_GOOD), mk()),
                  (ep, "x NULL", dims, mk(x=None)), (ep, "cov NULL", dims, mk(cov=None)),
                  (ep, "Yt NULL", dims, mk(Yt=None)), (ep, "work NULL", dims, mk(work=None)),
                  (ep, "work too small", dims, mk(work_doubles=small)),
                  (ep, "mask_select without Mt", dims, mk(mask_select=L.AME_MASK_HIDDEN)),
                  (ep, "unknown mask_select", dims, mk(Mt=fake, mask_select=3)),
                  (ep, "Yt misaligned", dims, mk(Yt=odd)), (ep, "noise NaN", dims, mk(noise=nan))]
        if ep != "ame_resid_nodes":
            cases += [(ep, "nbins 0", dims, mk(nbins=0)),
                      (ep, "nbins above the maximum", dims, mk(nbins=L.AME_RANK_MAX_BINS + 1)),
                      (ep, "scale 0", dims, mk(scale=0.0)), (ep, "scale negative", dims, mk(scale=-1.0)),
                      (ep, "scale NaN", dims, mk(scale=float("nan"))), (ep, "scale infinite", dims, mk(scale=float("inf")))]
    mk = lambda **kw: cls["ame_resid_nodes"](**{**good["ame_resid_nodes"], **kw})
    cases += [("ame_resid_nodes", "node NULL", dims, mk(node=None)), ("ame_resid_nodes", "node misaligned", dims, mk(node=odd))]
    mk = lambda **kw: cls["ame_resid_hist"](**{**good["ame_resid_hist"], **kw})
    cases += [("ame_resid_hist", "hist NULL", dims, mk(hist=None))]
    mk = lambda **kw: cls["ame_resid_select"](**{**good["ame_resid_select"], **kw})
    cases += [("ame_resid_select", f"{f} NULL", dims, mk(**{f: None})) for f in ("bin_min", "offset", "count", "records")]
    cases += [("ame_resid_select", "slice0 negative", dims, mk(slice0=-1)),
              ("ame_resid_select", "bin_min misaligned", dims, mk(bin_min=ctypes.c_void_p(4098)))]
    return cases


def test_argument_errors_return_nonzero_with_message():
    L = _lib()
    lib = L.lib()
    for ep, name, dims, args in argument_error_cases(L):
        rc = getattr(lib, ep)(ctypes.byref(dims) if dims is not None else None,
                              ctypes.byref(args) if args is not None else None, None)
        msg = lib.ame_last_error()
        assert rc != 0, (ep, name)
        assert msg and b"ame" in msg, (ep, name, msg)
        if "NULL" not in name and name not in ("uncompiled r", "n below 2", "mask_select without Mt",
                                                "unknown mask_select"):
            assert ep.encode() in msg, (ep, name, msg)


def test_host_finish():
    """residuals.py on hand-made inputs: the bin rule, the threshold bin, the
    record order, p-values and the expected counts."""
    from ame_amd import residuals as R
    import resid_ref as RR
    m2 = np.array([0.0, 0.124, 0.125, 31.99, 32.0, 1e9, -1.0, np.nan, np.inf])
    assert np.array_equal(R.bin_of(m2, 256, 32.0), RR.bin_of(m2, 256, 32.0))
    assert R.scale(256, 32.0) == 8.0 and np.array_equal(R.edges(256, 32.0), RR.edges(256, 32.0))
    hist = np.array([[5, 0, 3, 2], [1, 0, 0, 0], [0, 0, 0, 0]])
    for k, want_b, want_c in ((1, [3, 0, 0], [2, 1, 0]), (2, [3, 0, 0], [2, 1, 0]), (3, [2, 0, 0], [5, 1, 0]),
                              (6, [0, 0, 0], [10, 1, 0]), (50, [0, 0, 0], [10, 1, 0])):
        b, c = R.threshold(hist, k)
        assert b.tolist() == want_b and c.tolist() == want_c, k
    rec = np.zeros(5, R.RECORD)
    rec["m2"] = [3.0, np.nan, 7.0, 7.0, 1.0]
    rec["i"], rec["j"] = [0, 4, 2, 1, 0], [1, 5, 3, 9, 2]
    rec["z0"], rec["z1"] = np.arange(5.0), -np.arange(5.0)
    top = R.top_k(rec, [0, 5, 5], 4)
    assert top["i"].tolist() == [[4, 1, 2, 0], [-1] * 4] and top["j"][0].tolist() == [5, 9, 3, 1]
    assert np.isnan(top["m2"][0, 0]) and top["m2"][0, 1:].tolist() == [7.0, 7.0, 3.0]
    assert top["z"][0, :, 0].tolist() == [1.0, 3.0, 2.0, 0.0] and np.isnan(top["m2"][1]).all()
    assert np.allclose(top["p_value"][0, 1:], np.exp(-0.5 * np.array([7.0, 7.0, 3.0])), rtol=1e-15)
    ex = R.expected([100, 0], 4, 8.0)
    assert np.allclose(ex.sum(1), [100.0, 0.0]) and np.isclose(ex[0, -1], 100 * np.exp(-3.0))
    nd = R.node_dict(np.array([[[2, -3.0, 5.0, 1, 2, 3, 4, 5, 6], [0] * 9]], float))
    assert nd["pairs"].tolist() == [[2, 0]] and nd["mean_mahalanobis"][0, 0] == 2.5
    assert np.isnan(nd["mean_mahalanobis"][0, 1]) and nd["resid"][0, 0].tolist() == [3.0, 4.0]
    for bad in ((0, 8.0), (2049, 8.0), (2.5, 8.0), (True, 8.0), (8, 0.0), (8, float("inf"))):
        try:
            R.check_bins(*bad)
        except ValueError:
            continue
        raise AssertionError(bad)
