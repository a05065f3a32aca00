"""Hidden dyads on the GPU: ame_pack_mask, ame_fill_missing, the mask selector of
ame_predict / ame_mstep_stats through the C ABI, and fit / predictive_check /
fit_em on a partially observed network, against the fp64 reference
tests/missing_ref.py.

Bounds.
  ame_pack_mask: integers, exact.
  ame_fill_missing, writes: every element that is not hidden keeps its bits (the
  pad column too); a hidden element is an fp32 dot product of K = r terms plus
  one add, gamma_K doubled for the MFMA's unspecified internal order:
  2 (r + 1) 2^-24 (|a| + sum_k |u_k v_k|) from the fp64 value.
  ame_fill_missing, sums: test_gpu_elbo_sums.py's rule for out[0] / out[7], 5e-6 x
  the sum of |summand| over the hidden pairs, (a) against the fp64 evaluation
  on the working network the call just stored (corr is defined on those values)
  and (b) against the all-fp64 own-perspective fill.
  Selection: counts exact; the per-sum rules of test_gpu_predictive.py (slots 2-8
  5e-6 relative, the log score 5e-6 x sum|summand|, coverage counts inside the
  threshold band) and test_gpu_mstep.py (Rss00 / Rss11 5e-6 relative, Rss01 5e-6 x
  sum|summand|) against the reference over the selected pairs.
  End to end: within 4 x the oracle's own fp32-vs-fp64 deviation, measured in the
  test (covar_ref.relative_deviation's rule: max|a - b| / max|a| per quantity,
  the largest over the quantities compared).

Room under the bounds, measured on an MI355X over the cases added for every
compiled r (EVERY_R, on EVERY_R_MASKS); for information, no bound comes from
them.  Worst error / bound: hidden entries 0.23 (of 2 (r + 1) 2^-24 x scale);
corr against the stored working network 0.20, against the all-fp64 fill 0.063
(of 5e-6 sum|summand|).
"""
import ctypes
import functools

import numpy as np
import pytest

import missing_ref as MR
import predictive_ref as PR

pytestmark = pytest.mark.gpu

# (n, T, r): odd n with a pad column and a partial tile; exactly one tile and one
# word; a tile edge, a second word and a pad column; three tile rows with
# off-diagonal tiles; the widest r
CASES = ((5, 1, 1), (64, 2, 3), (65, 3, 2), (130, 2, 16), (70, 2, 32))
# every other compiled r: ame_fill_kernel pads K to pad4(r), so these run every
# MFMA step count 1..8 and every r mod 4 of zero padding after the first step;
# the mask selector of ame_predict<R, 0> / <R, 2> is one instance per r.  Two
# tile rows with a one-wide edge tile, a second mask word, a middle slice.
EVERY_R = tuple((65, 3, r) for r in range(1, 33) if r not in {c[2] for c in CASES})
# their masks (ame_pack_mask does not depend on r): the random 30 %; bits 63 / 0 of
# adjacent words with the diagonal tile's bit trimming; a whole off-diagonal tile
EVERY_R_MASKS = ("random30", "cols63_64", "tile")
IDS = lambda c: "n%d_T%d_r%d" % c


def fill_masks(case, masks):
    """The masks the fill tests run a case on: all of masks_for at CASES."""
    return EVERY_R_MASKS if case in EVERY_R else tuple(masks)


def select_masks(case):
    """The masks the selection test runs a case on (both selections each)."""
    if case in EVERY_R:
        return ("random30",)
    return ("none", "one", "last", "node", "random30") + (("tile", "cols63_64") if case[0] > 64 else ())
LEVELS = (0.5, 0.9, 0.95)
OBS, HID = MR.OBSERVED, MR.HIDDEN


def masks_for(n, T):
    """name -> (n, n, T) mask: none hidden; one pair; the last pair; pairs at the
    columns 63 / 64 (where n reaches them); every dyad of one node at one slice;
    one whole off-diagonal tile (the part of it inside the network); a random 30 %."""
    out = {"none": np.zeros((n, n, T), dtype=bool), "one": MR.sym_mask(n, T, [(1, 3, 0)]),
           "last": MR.sym_mask(n, T, [(n - 2, n - 1, T - 1)])}
    if n >= 64:
        edge = [(0, 63, 0), (62, 63, T - 1), (5, 62, 0)]
        if n > 64:
            edge += [(0, 64, 0), (63, 64, 0), (63, 64, T - 1), (1, n - 1, T - 1)]
        out["cols63_64"] = MR.sym_mask(n, T, edge)
    node = min(n - 1, 63)
    out["node"] = MR.sym_mask(n, T, [(node, j, T - 1) for j in range(n) if j != node])
    if n > 64:
        out["tile"] = MR.sym_mask(n, T, [(i, j, 0) for i in range(64) for j in range(64, min(n, 128))])
    out["random30"] = MR.random_mask(n, T, 0.3, seed=7)
    return out


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


class _Device:
    """make_state's means and covariances and a generated network on the device in
    the layouts of include/ame_amd.h, with raw C-ABI calls over slice ranges."""

    def __init__(self, case):
        import torch
        from ame_amd import TemporalAMEModel, _lib
        self.torch, self.L, self.lib = torch, _lib, _lib.lib()
        n, T, r = self.case = case
        self.dev = torch.device("cuda", 0)
        self.X, self.S = PR.make_state(n, T, r)
        m = TemporalAMEModel(n, T, r, seed=5)
        m.generate_data_fast(seed=9)
        self.Y = m.Y.numpy()
        self.R = m.R.numpy().astype(np.float64)
        self.rinv = np.linalg.inv(self.R) + np.array([[0.0, 0.3], [-0.2, 0.0]])   # asymmetric on purpose
        self.x = torch.from_numpy(self.X).permute(1, 0, 2).contiguous().to(self.dev)
        self.cov = torch.from_numpy(self.S).permute(1, 0, 2, 3).contiguous().to(self.dev)
        dims = self.dims(0, T)
        self.ny = int(self.lib.ame_pack_y_size(ctypes.byref(dims))) // (2 * T * n)
        self.nw = (n + 63) // 64
        src = torch.from_numpy(np.ascontiguousarray(self.Y, dtype=np.float32)).to(self.dev)
        self.Yraw = torch.zeros(T, n, self.ny, 2, dtype=torch.float32, device=self.dev)
        mm = torch.zeros(1, dtype=torch.int64, device=self.dev)
        _lib.check(self.lib.ame_pack_y(_ptr(src), _ptr(self.Yraw), ctypes.byref(dims), _ptr(mm), None), "ame_pack_y")
        torch.cuda.synchronize()
        self.masks = masks_for(n, T)
        self._packed = {}

    def dims(self, t0, t1):
        n, T, r = self.case
        return self.L.ame_dims(n, r, t1 - t0, t0, T, self.L.AME_GOOD)

    def pack_mask(self, mask, t0=0, t1=None):
        """(Mt, pairs, deg, asym) device tensors of slices [t0, t1); every output
        starts as garbage (-1)."""
        torch = self.torch
        n, T, r = self.case
        t1 = T if t1 is None else t1
        dims = self.dims(t0, t1)
        words = int(self.lib.ame_mask_words(ctypes.byref(dims)))
        assert words == (t1 - t0) * n * self.nw
        M = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(self.dev)
        Mt = torch.full((t1 - t0, n, self.nw), -1, dtype=torch.int64, device=self.dev)
        pairs = torch.full((t1 - t0,), -1, dtype=torch.int64, device=self.dev)
        deg = torch.full((t1 - t0, n), -1, dtype=torch.int32, device=self.dev)
        asym = torch.full((1,), -1, dtype=torch.int64, device=self.dev)
        self.L.check(self.lib.ame_pack_mask(_ptr(M), _ptr(Mt), ctypes.byref(dims), _ptr(pairs), _ptr(deg),
                                            _ptr(asym), None), "ame_pack_mask")
        torch.cuda.synchronize()
        return Mt, pairs, deg, asym

    def packed(self, name):
        if name not in self._packed:
            self._packed[name] = self.pack_mask(self.masks[name])[0]
        return self._packed[name]

    def fill(self, Mt, t0=0, t1=None, start=None):
        """One ame_fill_missing call over [t0, t1) on a copy of the packed
        observations (or of `start`); returns (Yt, corr) as numpy."""
        torch = self.torch
        n, T, r = self.case
        t1 = T if t1 is None else t1
        dims = self.dims(t0, t1)
        ws = int(self.lib.ame_fill_work_size(ctypes.byref(dims)))
        assert ws > 0
        buf = (self.Yraw if start is None else start)[t0:t1].clone()
        work = torch.full((ws,), float("nan"), dtype=torch.float64, device=self.dev)
        corr = torch.full((t1 - t0, 2), float("nan"), dtype=torch.float64, device=self.dev)
        a = self.L.ame_fill_args(x=_ptr(self.x[t0:t1]), Mt=_ptr(Mt[t0:t1]), Yt=_ptr(buf),
                                 rinv=(ctypes.c_double * 4)(*self.rinv.flatten().tolist()), corr=_ptr(corr),
                                 work=_ptr(work))
        self.L.check(self.lib.ame_fill_missing(ctypes.byref(dims), ctypes.byref(a), None), "ame_fill_missing")
        torch.cuda.synchronize()
        return buf.cpu().numpy(), corr.cpu().numpy()

    def predict(self, Mt=None, select=0, explicit=True):
        """sums [T][21] of one ame_predict call; explicit=False leaves the two new
        fields at their defaults."""
        torch = self.torch
        n, T, r = self.case
        dims = self.dims(0, T)
        ws = int(self.lib.ame_predict_work_size(ctypes.byref(dims)))
        work = torch.empty(ws, dtype=torch.float64, device=self.dev)
        sums = torch.full((T, self.L.AME_PREDICT_SUMS), float("nan"), dtype=torch.float64, device=self.dev)
        zsq, csq = PR.thresholds(LEVELS)
        kw = dict(x=_ptr(self.x), cov=_ptr(self.cov), Yt=_ptr(self.Yraw),
                  noise=(ctypes.c_double * 4)(*self.R.flatten().tolist()), n_levels=len(LEVELS),
                  zsq=(ctypes.c_double * 4)(*zsq, 0.0), csq=(ctypes.c_double * 4)(*csq, 0.0), sums=_ptr(sums),
                  work=_ptr(work))
        if explicit:
            kw.update(Mt=_ptr(Mt), mask_select=select)
        a = self.L.ame_predict_args(**kw)
        self.L.check(self.lib.ame_predict(ctypes.byref(dims), ctypes.byref(a), None), "ame_predict")
        torch.cuda.synchronize()
        return sums.cpu().numpy()

    def mstep(self, Mt=None, select=0, explicit=True):
        torch = self.torch
        n, T, r = self.case
        dims = self.dims(0, T)
        ws = int(self.lib.ame_mstep_work_size(ctypes.byref(dims)))
        work = torch.empty(ws, dtype=torch.float64, device=self.dev)
        dyad = torch.full((T, 4), float("nan"), dtype=torch.float64, device=self.dev)
        kw = dict(x=_ptr(self.x), cov=_ptr(self.cov), Yt=_ptr(self.Yraw), dyad=_ptr(dyad), work=_ptr(work))
        if explicit:
            kw.update(Mt=_ptr(Mt), mask_select=select)
        a = self.L.ame_mstep_args(**kw)
        self.L.check(self.lib.ame_mstep_stats(ctypes.byref(dims), ctypes.byref(a), None), "ame_mstep_stats")
        torch.cuda.synchronize()
        return dyad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _device(case):
    return _Device(case)


# ---------------------------------------------------------------------------
# 1. ame_pack_mask
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pack_mask_is_exact(case, gpu_device):
    dv = _device(case)
    n, T, r = case
    for name, mask in dv.masks.items():
        want_w, want_p, want_d = MR.pack(mask)
        Mt, pairs, deg, asym = dv.pack_mask(mask)
        assert np.array_equal(_u64(Mt), want_w), name
        assert np.array_equal(_u64(pairs), want_p), name
        assert np.array_equal(deg.cpu().numpy().view(np.uint32), want_d), name
        assert int(asym.item()) == 0, name
        # a diagonal entry is ignored, a planted asymmetry counted (both orientations)
        bad = mask.copy()
        bad[0, 0, 0] = True
        bad[0, n - 1, T - 1] = not bad[0, n - 1, T - 1]
        Mt2, _, _, asym2 = dv.pack_mask(bad)
        assert int(asym2.item()) == 2 == MR.asym_entries(bad), name
        assert int(_u64(Mt2)[0, 0, 0]) & 1 == 0
    # a slice range with t_begin > 0 packs those slices of M
    if T > 1:
        mask = dv.masks["random30"]
        want_w, want_p, want_d = MR.pack(mask)
        Mt, pairs, deg, _ = dv.pack_mask(mask, 1, T)
        assert np.array_equal(_u64(Mt), want_w[1:]) and np.array_equal(_u64(pairs), want_p[1:])
        assert np.array_equal(deg.cpu().numpy().view(np.uint32), want_d[1:])


# ---------------------------------------------------------------------------
# 2. / 3. ame_fill_missing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + EVERY_R, ids=IDS)
def test_fill_writes_hidden_entries_only(case, gpu_device):
    dv = _device(case)
    n, T, r = case
    raw = dv.Yraw.cpu().numpy()
    X64 = dv.X.astype(np.float64)
    U, V = np.abs(X64[:, :, 2:2 + r]), np.abs(X64[:, :, 2 + r:])
    for name in fill_masks(case, dv.masks):
        mask = dv.masks[name]
        m = MR.clean(mask).transpose(2, 0, 1)                      # (T, n, n)
        # a NaN in an element that is not hidden (a diagonal one, an off-diagonal
        # one of a tile with hidden pairs where there is one) must survive
        start = dv.Yraw.clone()
        start[0, 0, 0, :] = float("nan")
        free = np.argwhere(~m[T - 1] & ~np.eye(n, dtype=bool))
        fi, fj = (int(v) for v in free[len(free) // 2])
        start[T - 1, fi, fj, 1] = float("nan")
        want_keep = start.cpu().numpy()
        got, corr = dv.fill(dv.packed(name), start=start)
        hidden = np.zeros(got.shape[:3], dtype=bool)
        hidden[:, :, :n] = m
        assert np.array_equal(_i32(got)[~hidden], _i32(want_keep)[~hidden]), name
        assert np.isnan(got[0, 0, 0]).all() and np.isnan(got[T - 1, fi, fj, 1])
        assert np.isfinite(corr).all(), (name, corr)
        if not m.any():
            assert np.array_equal(_i32(got), _i32(want_keep)) and (corr == 0.0).all(), name
            continue
        worst = 0.0
        for t in range(T):
            if not m[t].any():
                continue
            own = MR.own_values(X64[:, t], r)                      # (n, n, 2) fp64
            dot = np.einsum("ik,jk->ij", U[:, t], V[:, t])        # sum_k |u_ik v_jk|
            scale = np.stack([np.abs(X64[:, t, 0])[:, None] + dot, np.abs(X64[:, t, 1])[:, None] + dot.T], axis=-1)
            bound = 2 * (r + 1) * 2.0 ** -24 * scale
            err = np.abs(got[t, :, :n].astype(np.float64) - own)
            assert (err[m[t]] <= bound[m[t]]).all(), (name, t, (err[m[t]] / bound[m[t]]).max())
            worst = max(worst, float((err[m[t]] / bound[m[t]]).max()))
        print(f"{IDS(case)} {name}: hidden entries, max err / bound = {worst:.3f}")
        assert np.array_equal(_i32(raw[:, :, n:]), _i32(got[:, :, n:]))       # the pad column


@pytest.mark.parametrize("case", CASES + EVERY_R, ids=IDS)
def test_fill_correction_sums(case, gpu_device):
    dv = _device(case)
    n, T, r = case
    for name in fill_masks(case, dv.masks):
        mask, Mt = dv.masks[name], dv.packed(name)
        got, corr = dv.fill(Mt)
        stored = got[:, :, :n].transpose(1, 2, 0, 3)               # (n, n, T, 2), what the call wrote
        for tag, Yw in (("stored", stored), ("fp64", MR.own_fill(dv.Y, dv.X.astype(np.float64), mask))):
            ref, mag = MR.corr_rows(Yw, dv.X, mask, dv.rinv)
            err, bound = np.abs(corr - ref), 5e-6 * mag
            ratio = (err / np.where(bound > 0, bound, 1.0)).max()
            print(f"{IDS(case)} {name} corr vs {tag}: max err / bound = {ratio:.3e}")
            assert (err <= bound).all(), (name, tag, corr, ref)
        hid = MR.pack(mask)[1]
        assert ((corr[:, 1] > 0) == (hid > 0)).all() and ((corr[:, 0] != 0) == (hid > 0)).all(), name
        # the same bits from a second call, and from a split of the slices over two calls
        got2, corr2 = dv.fill(Mt)
        assert np.array_equal(corr2.view(np.uint64), corr.view(np.uint64)), name
        assert np.array_equal(_i32(got2), _i32(got)), name
        for k in range(1, T):
            ga, ca = dv.fill(Mt, 0, k)
            gb, cb = dv.fill(Mt, k, T)
            assert np.array_equal(np.concatenate([ca, cb]).view(np.uint64), corr.view(np.uint64)), (name, k)
            assert np.array_equal(_i32(np.concatenate([ga, gb])), _i32(got)), (name, k)


def test_fill_takes_both_slice_mappings(gpu_device):
    """A slice count that is a multiple of 8 takes the other workgroup -> (slice,
    tile) mapping: each slice's row equals the row of a one-slice call."""
    dv = _Device((70, 8, 2))
    mask = dv.masks["random30"]
    Mt = dv.packed("random30")
    got, corr = dv.fill(Mt)
    ref, mag = MR.corr_rows(got[:, :, :70].transpose(1, 2, 0, 3), dv.X, mask, dv.rinv)
    assert (np.abs(corr - ref) <= 5e-6 * mag).all()
    for t in (0, 3, 7):
        g1, c1 = dv.fill(Mt, t, t + 1)
        assert np.array_equal(c1.view(np.uint64), corr[t:t + 1].view(np.uint64)), t
        assert np.array_equal(_i32(g1[0]), _i32(got[t])), t


# ---------------------------------------------------------------------------
# 4. selection in ame_predict and ame_mstep_stats
# ---------------------------------------------------------------------------
def _band(values, thr):
    lo = (values <= thr * (1.0 - 4.0 * PR.TOL)).sum()
    hi = (values <= thr * (1.0 + 4.0 * PR.TOL)).sum()
    return lo, hi


def _assert_predict_rows(got, want, per, tag):
    zsq, csq = PR.thresholds(LEVELS)
    for t in range(got.shape[0]):
        assert got[t, 0] == want[t, 0], (tag, t, got[t, 0], want[t, 0])
        if want[t, 0] == 0:
            assert (got[t] == 0.0).all(), (tag, t)
            continue
        for k in range(2, 9):
            assert abs(got[t, k] - want[t, k]) <= 5e-6 * abs(want[t, k]), (tag, t, k, got[t, k], want[t, k])
        assert abs(got[t, 1] - want[t, 1]) <= 5e-6 * np.abs(per[t]["logp"]).sum(), (tag, t)
        for l in range(len(LEVELS)):
            for slot, vals, thr in ((9 + 3 * l, per[t]["z2"][:, 0], zsq[l]), (10 + 3 * l, per[t]["z2"][:, 1], zsq[l]),
                                    (11 + 3 * l, per[t]["m2"], csq[l])):
                lo, hi = _band(vals, thr)
                assert lo <= got[t, slot] <= hi and got[t, slot] == round(got[t, slot]), (tag, t, slot)


@pytest.mark.parametrize("case", CASES + EVERY_R, ids=IDS)
def test_predict_and_mstep_select_pairs(case, gpu_device):
    dv = _device(case)
    n, T, r = case
    zsq, csq = PR.thresholds(LEVELS)
    plain = dv.predict(explicit=False)
    plain_d = dv.mstep(explicit=False)
    assert (plain[:, 0] == n * (n - 1) // 2).all() and (plain_d[:, 0] == n * (n - 1) // 2).all()
    # Mt == NULL, mask_select == 0: the bits of a call built without the new fields
    assert np.array_equal(dv.predict(None, 0).view(np.uint64), plain.view(np.uint64))
    assert np.array_equal(dv.mstep(None, 0).view(np.uint64), plain_d.view(np.uint64))
    # a mask that is passed but not selected on changes nothing either
    assert np.array_equal(dv.predict(dv.packed("random30"), 0).view(np.uint64), plain.view(np.uint64))
    for name in select_masks(case):
        mask, Mt = dv.masks[name], dv.packed(name)
        cnt, cnt_d = np.zeros(T), np.zeros(T)
        for sel in (OBS, HID):
            tag = f"{IDS(case)} {name} select {sel}"
            got = dv.predict(Mt, sel)
            want, per = MR.score_rows(dv.X, dv.S, r, dv.Y, dv.R, zsq, csq, mask, sel)
            _assert_predict_rows(got, want, per, tag)
            gd = dv.mstep(Mt, sel)
            wd, mag = MR.dyad_rows(dv.X, dv.S, r, dv.Y, mask, sel)
            for t in range(T):
                assert gd[t, 0] == wd[t, 0], (tag, t)
                if wd[t, 0] == 0:
                    assert (gd[t] == 0.0).all(), (tag, t)
                    continue
                for k in (1, 2):
                    assert abs(gd[t, k] - wd[t, k]) <= 5e-6 * abs(wd[t, k]), (tag, t, k)
                assert abs(gd[t, 3] - wd[t, 3]) <= 5e-6 * mag[t, 3], (tag, t)
            cnt += got[:, 0]
            cnt_d += gd[:, 0]
            if name == "none" and sel == OBS:      # every pair, in the same order: the same bits
                assert np.array_equal(got.view(np.uint64), plain.view(np.uint64))
                assert np.array_equal(gd.view(np.uint64), plain_d.view(np.uint64))
        assert np.array_equal(cnt, plain[:, 0]) and np.array_equal(cnt_d, plain_d[:, 0]), name
    assert np.array_equal(dv.predict(dv.packed("random30"), HID).view(np.uint64),
                          dv.predict(dv.packed("random30"), HID).view(np.uint64))


def test_capi_argument_errors(gpu_device):
    import torch
    from test_missing_capi import check_argument_errors
    check_argument_errors()
    torch.cuda.synchronize()   # nothing was queued that could fault


# ---------------------------------------------------------------------------
# 5. - 8. the VI layer
# ---------------------------------------------------------------------------
E2E = (33, 3, 2)
E2E_LR, E2E_ITERS = 0.5, 6
TERM_KEYS = ("loglik", "prior0", "trans", "entropy", "elbo", "recon")


def _vi(model, variant="good", lr=E2E_LR, **kw):
    import torch
    from ame_amd import TemporalAMENaiveMFVI, TemporalAMEStructuredMFVI
    if variant == "naive":
        return TemporalAMENaiveMFVI(model, learning_rate=lr, device=torch.device("cuda", 0), **kw)
    return TemporalAMEStructuredMFVI(model, factorization=variant, learning_rate=lr,
                                     device=torch.device("cuda", 0), **kw)


@functools.lru_cache(maxsize=None)
def _e2e(variant, frac=0.3):
    """The masked fit on the GPU and the fp64 / fp32 oracle fits from the same start."""
    import torch
    n, T, r = E2E
    c = MR.make_case(n, T, r, seed=41, variant=variant, lr=E2E_LR)
    mask = MR.random_mask(n, T, frac, seed=5)
    m = c["model"]
    m.set_missing(torch.from_numpy(mask))
    vi = _vi(m, variant)
    assert np.array_equal(vi.X_mean.numpy().astype(np.float64), c["X0"])
    vi.fit(max_iter=E2E_ITERS, tolerance=0.0, verbose=False)
    o64 = MR.oracle_fit(c["Y"], c["X0"], c["S0"], c["params"], mask, variant, E2E_LR, E2E_ITERS, history=True)
    o32 = MR.oracle_fit(c["Y"], c["X0"], c["S0"], c["params"], mask, variant, E2E_LR, E2E_ITERS,
                        dtype=np.float32, history=True)
    return dict(c, mask=mask, vi=vi, o64=o64, o32=o32)


def _flat(X, S, terms):
    return dict(X=np.asarray(X, np.float64), S=np.asarray(S, np.float64),
                **{k: np.array([terms[k]]) for k in TERM_KEYS})


@pytest.mark.parametrize("variant", ("good", "bad", "naive"))
def test_fit_matches_the_oracle(variant, gpu_device):
    c = _e2e(variant)
    vi, o64, o32 = c["vi"], c["o64"], c["o32"]
    terms = vi.elbo_terms()
    got = _flat(vi.X_mean.numpy(), vi.X_cov.numpy(), terms)
    a = _flat(o64["X"], o64["S"], o64["terms"][-1])
    b = _flat(o32["X"], o32["S"], o32["terms"][-1])
    keys = ("X", "S") + TERM_KEYS
    for k in keys:
        print(f"{variant} {k}: GPU vs fp64 oracle {MR.relative_deviation(a, got, (k,)):.3e}; "
              f"fp32 vs fp64 oracle {MR.relative_deviation(a, b, (k,)):.3e}")
    own, dev = MR.relative_deviation(a, b, keys), MR.relative_deviation(a, got, keys)
    print(f"{variant}: GPU vs fp64 oracle {dev:.3e}; oracle fp32 vs fp64 {own:.3e}; allowance {4 * own:.3e}")
    assert dev <= 4.0 * own, (dev, own)
    # the history holds the same quantities after every iteration
    h = vi.history
    assert len(h["elbo"]) == E2E_ITERS
    for it in range(E2E_ITERS):
        want = o64["terms"][it]
        assert abs(float(h["elbo"][it]) - want["elbo"]) <= 4.0 * own * abs(want["elbo"]) + 2.0 ** -23 * abs(want["elbo"])
        assert abs(h["reconstruction_error"][it] - want["recon"]) <= 4.0 * own * want["recon"]
    # the working network holds the own-perspective values of the final means
    eng = vi.engine
    assert eng.Yt.data_ptr() != eng.Yt_raw.data_ptr() and not eng.swap_consistent
    n = E2E[0]
    m = MR.clean(c["mask"]).transpose(2, 0, 1)
    Yw, Yr = eng.Yt.cpu().numpy()[:, :, :n], eng.Yt_raw.cpu().numpy()[:, :, :n]
    assert np.array_equal(_i32(Yw[~m]), _i32(Yr[~m]))
    own_v = np.stack([MR.own_values(vi.X_mean.numpy().astype(np.float64)[:, t], E2E[2]) for t in range(E2E[1])])
    assert np.abs(Yw[m] - own_v[m]).max() <= 1e-5


def test_all_false_mask_is_the_unmasked_fit(gpu_device):
    import torch
    n, T, r = E2E
    runs = {}
    for key in ("plain", "masked"):
        c = MR.make_case(n, T, r, seed=41, lr=E2E_LR)
        m = c["model"]
        if key == "masked":
            m.set_missing(torch.zeros(n, n, T, dtype=torch.bool))
        vi = _vi(m, engine_options=dict(pipeline=False, speculate=False))
        vi.fit(max_iter=4, tolerance=0.0, verbose=False)
        runs[key] = (vi, vi.X_mean.clone(), vi.X_cov.clone(), vi.elbo_terms())
    (va, xa, sa, ta), (vb, xb, sb, tb) = runs["plain"], runs["masked"]
    assert torch.equal(xa, xb) and torch.equal(sa, sb)
    for k in ta:
        assert abs(ta[k] - tb[k]) <= 1e-12 * abs(ta[k]), (k, ta[k], tb[k])
    assert vb.engine.swap_consistent == va.engine.swap_consistent
    assert not hasattr(va.engine, "Yt_raw") and not va.engine.masked and vb.engine.masked


def test_held_out_scores(gpu_device):
    import torch
    from ame_amd import TemporalAMEModel
    c = _e2e("good")
    vi, mask = c["vi"], c["mask"]
    hid = MR.pack(mask)[1].astype(np.float64)
    total = E2E[0] * (E2E[0] - 1) // 2
    held = vi.predictive_check(levels=LEVELS, subset="held_out")
    seen = vi.predictive_check(levels=LEVELS)
    assert np.array_equal(held["pairs"], hid) and np.array_equal(seen["pairs"], total - hid)
    assert np.array_equal(vi.predictive_check(levels=LEVELS, subset="observed")["sq_err"], seen["sq_err"])
    # against the fp64 reference over those pairs, on the downloaded state
    zsq, csq = PR.thresholds(LEVELS)
    X, S = vi.X_mean.numpy(), vi.X_cov.numpy()
    want, per = MR.score_rows(X, S, E2E[2], c["Y"], c["params"]["R"], zsq, csq, mask, HID)
    for t in range(E2E[1]):
        for ch in range(2):
            assert abs(held["sq_err"][t, ch] - want[t, 7 + ch]) <= 5e-6 * want[t, 7 + ch]
    # a no-mask fit on the zero-filled network, scored on the same pairs through predict
    m0 = TemporalAMEModel(*E2E, seed=41)
    m0.Y = c["model"].Y.clone()
    m0.Y[torch.from_numpy(MR.clean(mask))] = 0.0
    v0 = _vi(m0)
    assert torch.equal(v0.X_mean, torch.from_numpy(c["X0"]).float())
    v0.fit(max_iter=E2E_ITERS, tolerance=0.0, verbose=False)
    e0, eng = v0.engine, vi.engine
    e0.discard_speculation()
    sums, _ = eng.predict(e0.x_a, e0.cov, Yt=eng.Yt_raw, zsq=zsq.tolist(), csq=csq.tolist(), Mt=eng.Mt,
                          mask_select=HID)
    zero = sums.cpu().numpy()
    assert np.array_equal(zero[:, 0], hid)
    print(f"held-out sq_err: scheme {held['sq_err'].sum(0).tolist()} zero-fill {zero[:, 7:9].sum(0).tolist()}")
    assert (held["sq_err"].sum(0) < zero[:, 7:9].sum(0)).all()
    # a subset without a mask, an unknown subset
    with pytest.raises(ValueError):
        v0.predictive_check(subset="held_out")
    with pytest.raises(ValueError):
        v0.predictive_check(subset="observed")
    with pytest.raises(ValueError):
        vi.predictive_check(subset="everything")


def test_forecast_check_scores_observed_future_pairs(gpu_device):
    import torch
    c = _e2e("good")
    vi = c["vi"]
    n, h = E2E[0], 2
    Yf = torch.randn(n, n, h, 2, generator=torch.Generator().manual_seed(3))
    mf = MR.random_mask(n, h, 0.25, seed=11)
    full = vi.forecast_check(Yf, levels=LEVELS)
    part = vi.forecast_check(Yf, levels=LEVELS, missing_future=torch.from_numpy(mf))
    hid = MR.pack(mf)[1].astype(np.float64)
    assert np.array_equal(full["pairs"], np.full(h, n * (n - 1) // 2))
    assert np.array_equal(part["pairs"], n * (n - 1) // 2 - hid)
    Xp, Sp = vi.forecast(h)
    zsq, csq = PR.thresholds(LEVELS)
    want, _ = MR.score_rows(Xp.numpy(), Sp.numpy(), E2E[2], Yf.numpy(), c["params"]["R"], zsq, csq, mf, OBS)
    for t in range(h):
        for ch in range(2):
            assert abs(part["sq_err"][t, ch] - want[t, 7 + ch]) <= 5e-6 * want[t, 7 + ch]
    bad = mf.copy()
    bad[0, 1, 0] = not bad[0, 1, 0]
    with pytest.raises(ValueError):
        vi.forecast_check(Yf, missing_future=torch.from_numpy(bad))
    with pytest.raises(ValueError):
        vi.forecast_check(Yf, missing_future=torch.from_numpy(mf[:, :, :1]))


def test_fit_em_learns_R_over_observed_pairs(gpu_device):
    import torch
    n, T, r = E2E
    sweeps = 5
    c = MR.make_case(n, T, r, seed=43, lr=E2E_LR)
    mask = MR.random_mask(n, T, 0.2, seed=6)
    m = c["model"]
    m.set_missing(torch.from_numpy(mask))
    vi = _vi(m)
    h = vi.fit_em(1, sweeps, update=("R",), tolerance=0.0, verbose=False)
    got = {"R": h["em"][0]["R"].numpy()}
    e64 = MR.oracle_em(c["Y"], c["X0"], c["S0"], c["params"], mask, rounds=1, sweeps=sweeps, lr=E2E_LR)
    e32 = MR.oracle_em(c["Y"], c["X0"], c["S0"], c["params"], mask, dtype=np.float32, rounds=1, sweeps=sweeps,
                       lr=E2E_LR)
    own = MR.relative_deviation(e64[0], e32[0], ("R",))
    dev = MR.relative_deviation(e64[0], got, ("R",))
    print(f"R after round 1: GPU vs fp64 EM {dev:.3e}; fp32 vs fp64 EM {own:.3e}; allowance {4 * own:.3e}")
    assert dev <= 4.0 * own, (dev, own)
    assert torch.equal(m.R, h["em"][0]["R"].float())
    st = vi.m_step_statistics()
    hid = float(MR.pack(mask)[1].sum())
    assert st["hidden_pairs"] == hid and st["pairs"] == T * n * (n - 1) // 2 - hid
    # R over all pairs (the hidden truth included) is another matrix
    allp = MR.M.statistics(vi.X_mean.numpy(), vi.X_cov.numpy(), r, c["Y"])
    assert allp["pairs"] > st["pairs"]


def test_unsupported_combinations_say_which(gpu_device):
    import torch
    import covar_ref as CR
    from ame_amd import TemporalAMEModel
    from ame_amd.engine import DeviceEngine, Shard
    n, T, r = 12, 4, 2
    mask = torch.from_numpy(MR.random_mask(n, T, 0.3))

    def model(covariates=False):
        m = TemporalAMEModel(n, T, r, seed=3)
        if covariates:
            m.set_covariates(torch.from_numpy(CR.make_w(n, T, 2)), beta=(0.3, -0.2))
        m.generate_data_fast(seed=4)
        m.set_missing(mask)
        return m

    m = model()
    vi = _vi(m)
    with pytest.raises(NotImplementedError, match="time-sharded"):
        DeviceEngine(m, "good", 0.5, vi.X_mean, vi.X_cov, device=torch.device("cuda", 0), shard=Shard(0, 2, T))
    with pytest.raises(NotImplementedError, match="covariates"):
        _vi(model(covariates=True)).fit(max_iter=1, tolerance=0.0, verbose=False)
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    with pytest.raises(NotImplementedError, match="smooth"):
        vi.smooth()
    with pytest.raises(NotImplementedError, match="smooth"):
        vi.predictive_check(smoothed=True)
    with pytest.raises(NotImplementedError, match="smooth"):
        vi.m_step_statistics(smoothed=True)
    with pytest.raises(NotImplementedError, match="smooth"):
        vi.engine.smooth()
    # the fit itself is untouched by the refusals
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    assert np.isfinite(vi.elbo_terms()["elbo"])
