"""Binary networks on the GPU: ame_probit_fill and ame_probit_score through the C
ABI, and fit / predictive_check / predict_proba on a binary model, against the
fp64 reference tests/probit_ref.py.

Bounds.
  ame_probit_fill, writes.  A hidden entry has ame_fill_missing's bits; NaNs
  planted on the diagonal and in the pad column survive.  Every other entry:
  the device forms m = a_i + b_j + p in fp64 from the fp32 MFMA product p, whose
  error is at most delta = 2 (r + 2) 2^-24 (|a_i| + |b_j| + sum_k |u_ik v_jk|) (gamma_K
  doubled for the MFMA's unspecified order, as in test_gpu_missing.py).  Each
  conditional step e_a = eta_a + s sd kappa(s eta_a / sd) has slope in (0, 1) in
  eta_a, and eta_a moves by at most delta_a + |rho| |delta e_b|, so |delta e| <=
  delta (1 + |rho|) / (1 - |rho|) and |delta d| <= 2 delta_max / (1 - |rho|), delta_max the larger
  of the pair's two.  The stored entry adds the own-perspective product's error
  and one rounding:
      2 (r + 1) 2^-24 scale_own + 2 delta_max / (1 - |rho|) + 2^-23 |value|.
  ame_probit_fill, stat: [0] exact; [1..3] within 5e-6 x the sum of |summand|
  (the project's rule) of the fp64 reference, evaluated (a) at the means the
  stored own-perspective network implies (an all-hidden call stores a_i + p in
  fp32; m0 = that + b_j) and (b) in fp64 throughout.
  Reproducibility: the same bits from a second call, from every two-way split of
  the slices and under both slice mappings.
  ame_probit_score: pairs and ties exact; the hit count exact up to the entries
  whose pi lies within 1e-6 of 1/2 (at most 0.1 % of them, checked on the
  reference); the three sums within 5e-6 x the sum of |summand|.
  End to end: within 4 x the oracle's own fp32-vs-fp64 deviation (test_gpu_missing.py's rule).
  The tails (section 5): on probit_ref.grid_case the device forms every pair mean
  exactly, so both kernels are held to 4 x TAIL_TAU0 = 1.44e-14 x the sum of
  |terms| of an mpmath fixture, TAIL_TAU0 being the scipy reference's own
  deviation from it; the device measures at most 0.20 of that.  The random
  states run once more with every third pair's ties against their means.
"""
import ctypes
import functools

import numpy as np
import pytest

import missing_ref as MR
import predictive_ref as PR
import probit_ref as BR

pytestmark = pytest.mark.gpu

CASES = ((5, 1, 1), (64, 2, 3), (65, 3, 2), (130, 2, 16), (70, 2, 32))
EVERY_R = tuple((65, 3, r) for r in range(1, 33) if r not in {c[2] for c in CASES})
RHOS = (0.0, 0.5, -0.7)
IDS = lambda c: "n%d_T%d_r%d" % c
OBS, HID = MR.OBSERVED, MR.HIDDEN


def masks_for(n, T):
    """name -> (n, n, T) mask or None: no mask; a random 30 %; one whole
    off-diagonal tile (where the network has one)."""
    out = {"none": None, "random30": MR.random_mask(n, T, 0.3, seed=7)}
    if n > 64:
        out["tile"] = MR.sym_mask(n, T, [(i, j, 0) for i in range(64) for j in range(64, min(n, 128))])
    return out


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class _Device:
    """make_state's means and covariances and ties drawn from them, on the device
    in the layouts of include/ame_amd.h, with raw C-ABI calls over slice ranges.
    ties "drawn": 1[mu + N(0, 1) > 0], which almost always agrees with the mean;
    "against": the same draw with both ties of every third pair i < j (in row
    order) set against their means.  `state` = (X, S, B) replaces all three."""

    def __init__(self, case, ties="drawn", state=None):
        import torch
        from ame_amd import _lib
        self.torch, self.L, self.lib = torch, _lib, _lib.lib()
        n, T, r = self.case = case
        self.dev = torch.device("cuda", 0)
        if state is not None:
            self.X, self.S, self.B = state
        else:
            self.X, self.S = PR.make_state(n, T, r)
            self.B = BR.state_ties(self.X, case, ties)
        self.x = torch.from_numpy(self.X).permute(1, 0, 2).contiguous().to(self.dev)
        self.cov = torch.from_numpy(self.S).permute(1, 0, 2, 3).contiguous().to(self.dev)
        dims = self.dims(0, T)
        self.ny = int(self.lib.ame_pack_y_size(ctypes.byref(dims))) // (2 * T * n)
        self.nw = (n + 63) // 64
        src = torch.from_numpy(np.ascontiguousarray(BR.y_of(self.B), dtype=np.float32)).to(self.dev)
        self.Y01 = torch.zeros(T, n, self.ny, 2, dtype=torch.float32, device=self.dev)
        mm = torch.zeros(1, dtype=torch.int64, device=self.dev)
        _lib.check(self.lib.ame_pack_y(_ptr(src), _ptr(self.Y01), ctypes.byref(dims), _ptr(mm), None), "ame_pack_y")
        torch.cuda.synchronize()
        self.masks = masks_for(n, T)
        self.Bt = self.pack(self.B)
        self._packed = {"none": None}
        # NaN on the diagonal and in the pad column, zero elsewhere
        self.start = torch.zeros(T, n, self.ny, 2, dtype=torch.float32, device=self.dev)
        idx = torch.arange(n, device=self.dev)
        self.start[:, idx, idx, :] = float("nan")
        self.start[:, :, n:, :] = float("nan")

    def dims(self, t0, t1):
        n, T, r = self.case
        return self.L.ame_dims(n, r, t1 - t0, t0, T, self.L.AME_GOOD)

    def pack(self, bits):
        """ame_pack_mask's words [T][n][nw] of an (n, n, T) array (its counts are dropped)."""
        torch = self.torch
        n, T, r = self.case
        M = torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint8)).to(self.dev)
        Mt = torch.full((T, n, self.nw), -1, dtype=torch.int64, device=self.dev)
        pairs = torch.zeros(T, dtype=torch.int64, device=self.dev)
        deg = torch.zeros(T, n, dtype=torch.int32, device=self.dev)
        asym = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.L.check(self.lib.ame_pack_mask(_ptr(M), _ptr(Mt), ctypes.byref(self.dims(0, T)), _ptr(pairs), _ptr(deg),
                                            _ptr(asym), None), "ame_pack_mask")
        torch.cuda.synchronize()
        return Mt

    def packed(self, name):
        if name not in self._packed:
            self._packed[name] = self.pack(self.masks[name])
        return self._packed[name]

    def fill(self, rho, Mt=None, t0=0, t1=None):
        """One ame_probit_fill call over [t0, t1) on a copy of `start`; (Yt, stat) as numpy."""
        torch = self.torch
        n, T, r = self.case
        t1 = T if t1 is None else t1
        dims = self.dims(t0, t1)
        ws = int(self.lib.ame_probit_fill_work_size(ctypes.byref(dims)))
        assert ws > 0
        buf = self.start[t0:t1].clone()
        work = torch.full((ws,), float("nan"), dtype=torch.float64, device=self.dev)
        stat = torch.full((t1 - t0, 4), float("nan"), dtype=torch.float64, device=self.dev)
        a = self.L.ame_probit_fill_args(x=_ptr(self.x[t0:t1]), Bt=_ptr(self.Bt[t0:t1]),
                                        Mt=_ptr(Mt[t0:t1]) if Mt is not None else None, rho=rho, Yt=_ptr(buf),
                                        stat=_ptr(stat), work=_ptr(work), work_doubles=ws)
        self.L.check(self.lib.ame_probit_fill(ctypes.byref(dims), ctypes.byref(a), None), "ame_probit_fill")
        torch.cuda.synchronize()
        return buf.cpu().numpy(), stat.cpu().numpy()

    def fill_missing(self, Mt):
        """ame_fill_missing on a copy of `start`: the bits a hidden entry must have."""
        torch = self.torch
        n, T, r = self.case
        dims = self.dims(0, T)
        ws = int(self.lib.ame_fill_work_size(ctypes.byref(dims)))
        buf = self.start.clone()
        work = torch.empty(ws, dtype=torch.float64, device=self.dev)
        corr = torch.empty(T, 2, dtype=torch.float64, device=self.dev)
        a = self.L.ame_fill_args(x=_ptr(self.x), Mt=_ptr(Mt), Yt=_ptr(buf), rinv=(ctypes.c_double * 4)(1, 0, 0, 1),
                                 corr=_ptr(corr), work=_ptr(work))
        self.L.check(self.lib.ame_fill_missing(ctypes.byref(dims), ctypes.byref(a), None), "ame_fill_missing")
        torch.cuda.synchronize()
        return buf.cpu().numpy()

    @functools.lru_cache(maxsize=None)
    def own_network(self):
        """The own-perspective network of every pair as the device stores it (an all-hidden fill)."""
        n, T, r = self.case
        return self.fill_missing(self.pack(np.ones((n, n, T), bool)))[:, :, :n]

    def implied_means(self):
        """(T, n, n, 2) fp64: m0 = (a_i + p)_fp32 + b_j from the stored own-perspective network."""
        own = self.own_network().astype(np.float64)
        b = self.X.astype(np.float64)[:, :, 1].T                    # (T, n)
        m0 = own[..., 0] + b[:, None, :]
        return np.stack([m0, m0.transpose(0, 2, 1)], -1)

    def score(self, Mt=None, select=0, t0=0, t1=None):
        torch = self.torch
        n, T, r = self.case
        t1 = T if t1 is None else t1
        dims = self.dims(t0, t1)
        ws = int(self.lib.ame_probit_score_work_size(ctypes.byref(dims)))
        work = torch.empty(ws, dtype=torch.float64, device=self.dev)
        sums = torch.full((t1 - t0, 6), float("nan"), dtype=torch.float64, device=self.dev)
        a = self.L.ame_probit_score_args(x=_ptr(self.x[t0:t1]), cov=_ptr(self.cov[t0:t1]), Yt=_ptr(self.Y01[t0:t1]),
                                         sums=_ptr(sums), work=_ptr(work), work_doubles=ws,
                                         Mt=_ptr(Mt[t0:t1]) if Mt is not None else None, mask_select=select)
        self.L.check(self.lib.ame_probit_score(ctypes.byref(dims), ctypes.byref(a), None), "ame_probit_score")
        torch.cuda.synchronize()
        return sums.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _device(case, ties="drawn"):
    return _Device(case, ties)


# ---------------------------------------------------------------------------
# 1. ame_probit_fill: what is written
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + EVERY_R, ids=IDS)
def test_fill_writes_every_pair_within_the_bound(case, gpu_device):
    _check_fill_writes(_device(case))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fill_writes_every_pair_within_the_bound_with_ties_against_the_means(case, gpu_device):
    """s m reaches about -23 at r = 16, 32 with p != 0; the derived bound holds for any ties."""
    _check_fill_writes(_device(case, "against"))


def _check_fill_writes(dv):
    n, T, r = case = dv.case
    X64 = dv.X.astype(np.float64)
    U, V = np.abs(X64[:, :, 2:2 + r]), np.abs(X64[:, :, 2 + r:])
    eye = np.eye(n, dtype=bool)
    for name, mask in dv.masks.items():
        Mt = dv.packed(name)
        hid = np.zeros((T, n, n), bool) if mask is None else MR.clean(mask).transpose(2, 0, 1)
        want_hidden = dv.fill_missing(Mt) if mask is not None else None
        for rho in RHOS:
            got, stat = dv.fill(rho, Mt)
            tag = f"{IDS(case)} {name} rho={rho}"
            # the diagonal and the pad column keep their NaNs; nothing else does
            assert np.isnan(got[:, :, :n][:, eye]).all() and np.isnan(got[:, :, n:]).all(), tag
            assert np.isfinite(got[:, :, :n][:, ~eye]).all() and np.isfinite(stat).all(), tag
            if mask is not None:
                assert np.array_equal(_i32(got[:, :, :n][hid]), _i32(want_hidden[:, :, :n][hid])), tag
            ref = BR.working_network(X64, dv.B, mask, rho)                       # (n, n, T, 2) fp64
            worst = 0.0
            for t in range(T):
                dot = np.einsum("ik,jk->ij", U[:, t], V[:, t])                    # sum_k |u_ik v_jk|
                aa, bb = np.abs(X64[:, t, 0]), np.abs(X64[:, t, 1])
                scale_own = np.stack([aa[:, None] + dot, bb[:, None] + dot.T], -1)
                delta = 2 * (r + 2) * 2.0 ** -24 * (aa[:, None] + bb[None, :] + dot)
                dmax = np.maximum(delta, delta.T)[:, :, None]
                bound = 2 * (r + 1) * 2.0 ** -24 * scale_own + 2.0 * dmax / (1.0 - abs(rho)) \
                    + 2.0 ** -23 * np.abs(ref[:, :, t])
                err = np.abs(got[t, :, :n].astype(np.float64) - ref[:, :, t])
                sel = ~eye & ~hid[t]
                if sel.any():
                    ratio = float((err[sel] / bound[sel]).max())
                    assert ratio <= 1.0, (tag, t, ratio)
                    worst = max(worst, ratio)
            print(f"{tag}: observed entries, max err / bound = {worst:.3f}")


# ---------------------------------------------------------------------------
# 2. ame_probit_fill: the statistics
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + EVERY_R, ids=IDS)
def test_fill_statistics(case, gpu_device):
    dv = _device(case)
    n, T, r = case
    implied = dv.implied_means()
    for name, mask in dv.masks.items():
        Mt = dv.packed(name)
        for rho in RHOS:
            got, stat = dv.fill(rho, Mt)
            tag = f"{IDS(case)} {name} rho={rho}"
            for kind, means in (("implied", implied), ("fp64", None)):
                ref, mag = BR.stat_rows(dv.X, dv.B, mask, rho, means=means)
                assert np.array_equal(stat[:, 0], ref[:, 0]), (tag, kind)
                err, bound = np.abs(stat[:, 1:] - ref[:, 1:]), 5e-6 * mag[:, 1:]
                ratio = (err / np.where(bound > 0, bound, 1.0)).max()
                print(f"{tag} stat vs {kind}: max err / bound = {ratio:.3e}")
                assert (err <= bound).all(), (tag, kind, stat, ref)
            if rho == 0.0:   # the bound is the sum of log Phi(s m) there
                assert (np.abs(stat[:, 1] - stat[:, 3]) <= 1e-12 * np.abs(stat[:, 3])).all(), tag
            if case in EVERY_R and rho != RHOS[1]:
                continue
            # the same bits from a second call and from every two-way split of the slices
            got2, stat2 = dv.fill(rho, Mt)
            assert np.array_equal(stat2.view(np.uint64), stat.view(np.uint64)), tag
            assert np.array_equal(_i32(got2), _i32(got)), tag
            for k in range(1, T):
                ga, sa = dv.fill(rho, Mt, 0, k)
                gb, sb = dv.fill(rho, Mt, k, T)
                assert np.array_equal(np.concatenate([sa, sb]).view(np.uint64), stat.view(np.uint64)), (tag, k)
                assert np.array_equal(_i32(np.concatenate([ga, gb])), _i32(got)), (tag, k)


def test_fill_and_score_take_both_slice_mappings(gpu_device):
    """A slice count that is a multiple of 8 takes the other workgroup -> (slice,
    tile) mapping: each slice's row equals the row of a one-slice call."""
    dv = _Device((70, 8, 2))
    mask, Mt = dv.masks["random30"], dv.packed("random30")
    for rho in RHOS:
        got, stat = dv.fill(rho, Mt)
        ref, mag = BR.stat_rows(dv.X, dv.B, mask, rho)
        assert np.array_equal(stat[:, 0], ref[:, 0])
        assert (np.abs(stat[:, 1:] - ref[:, 1:]) <= 5e-6 * mag[:, 1:]).all(), rho
        for t in (0, 3, 7):
            g1, s1 = dv.fill(rho, Mt, t, t + 1)
            assert np.array_equal(s1.view(np.uint64), stat[t:t + 1].view(np.uint64)), (rho, t)
            assert np.array_equal(_i32(g1[0]), _i32(got[t])), (rho, t)
    sums = dv.score(Mt, HID)
    for t in (0, 4, 7):
        assert np.array_equal(dv.score(Mt, HID, t, t + 1).view(np.uint64), sums[t:t + 1].view(np.uint64)), t


# ---------------------------------------------------------------------------
# 3. ame_probit_score
# ---------------------------------------------------------------------------
def _assert_score_rows(got, want, mag, near, tag):
    for t in range(got.shape[0]):
        assert got[t, 0] == want[t, 0] and got[t, 4] == want[t, 4], (tag, t, got[t], want[t])
        if want[t, 0] == 0:
            assert (got[t] == 0.0).all(), (tag, t)
            continue
        assert near[t] <= 1e-3 * 2 * want[t, 0], (tag, t, near[t])
        assert abs(got[t, 3] - want[t, 3]) <= near[t] and got[t, 3] == round(got[t, 3]), (tag, t, got[t, 3], want[t, 3])
        for k in (1, 2, 5):
            assert abs(got[t, k] - want[t, k]) <= 5e-6 * mag[t, k], (tag, t, k, got[t, k], want[t, k], mag[t, k])


@pytest.mark.parametrize("case", CASES + EVERY_R, ids=IDS)
def test_score_sums(case, gpu_device):
    _check_score_sums(_device(case))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_score_sums_with_ties_against_the_means(case, gpu_device):
    _check_score_sums(_device(case, "against"))


def _check_score_sums(dv):
    n, T, r = case = dv.case
    plain = dv.score()
    want, mag, near = BR.score_rows(dv.X, dv.S, r, dv.B)
    assert (plain[:, 0] == n * (n - 1) // 2).all()
    _assert_score_rows(plain, want, mag, near, f"{IDS(case)} every pair")
    worst = (np.abs(plain - want)[:, [1, 2, 5]] / (5e-6 * mag[:, [1, 2, 5]])).max()
    print(f"{IDS(case)} score sums, max err / bound = {worst:.3e}")
    # a mask that is passed but not selected on changes nothing
    assert np.array_equal(dv.score(dv.packed("random30"), 0).view(np.uint64), plain.view(np.uint64))
    for name, mask in dv.masks.items():
        if mask is None:
            continue
        cnt = np.zeros(T)
        for sel in (OBS, HID):
            got = dv.score(dv.packed(name), sel)
            w, mg, nr = BR.score_rows(dv.X, dv.S, r, dv.B, mask, sel)
            _assert_score_rows(got, w, mg, nr, f"{IDS(case)} {name} select {sel}")
            cnt += got[:, 0]
        assert np.array_equal(cnt, plain[:, 0]), name
    # the same bits from a second call and from a split of the slices
    assert np.array_equal(dv.score().view(np.uint64), plain.view(np.uint64))
    for k in range(1, T):
        both = np.concatenate([dv.score(None, 0, 0, k), dv.score(None, 0, k, T)])
        assert np.array_equal(both.view(np.uint64), plain.view(np.uint64)), k


def test_capi_argument_errors(gpu_device):
    import torch
    from test_probit_capi import check_argument_errors
    check_argument_errors()
    torch.cuda.synchronize()   # nothing was queued that could fault


# ---------------------------------------------------------------------------
# 4. the VI layer
# ---------------------------------------------------------------------------
E2E = (33, 3, 2)
E2E_LR, E2E_ITERS, E2E_RHO = 0.5, 6, 0.5
TERM_KEYS = ("loglik", "prior0", "trans", "entropy", "elbo", "recon")


def _vi(model, variant="good", lr=E2E_LR, **kw):
    import torch
    from ame_amd import TemporalAMEStructuredMFVI
    return TemporalAMEStructuredMFVI(model, factorization=variant, learning_rate=lr,
                                     device=torch.device("cuda", 0), **kw)


@functools.lru_cache(maxsize=None)
def _e2e():
    """The binary fit with 30 % of the pairs held out on the GPU and the fp64 /
    fp32 oracle fits from the same start."""
    import torch
    n, T, r = E2E
    c = BR.make_binary_case(n, T, r, E2E_RHO, seed=41, lr=E2E_LR)
    mask = MR.random_mask(n, T, 0.3, seed=5)
    m = c["model"]
    m.set_binary(torch.from_numpy(c["B"]), rho=E2E_RHO)
    m.set_missing(torch.from_numpy(mask))
    vi = _vi(m)
    assert np.array_equal(vi.X_mean.numpy().astype(np.float64), c["X0"])
    vi.fit(max_iter=E2E_ITERS, tolerance=0.0, verbose=False)
    kw = dict(variant="good", lr=E2E_LR, sweeps=E2E_ITERS, history=True)
    o64 = BR.oracle_fit(c["B"], c["X0"], c["S0"], c["params"], mask, E2E_RHO, **kw)
    o32 = BR.oracle_fit(c["B"], c["X0"], c["S0"], c["params"], mask, E2E_RHO, dtype=np.float32, **kw)
    return dict(c, mask=mask, vi=vi, o64=o64, o32=o32)


def _flat(X, S, terms):
    return dict(X=np.asarray(X, np.float64), S=np.asarray(S, np.float64),
                **{k: np.array([terms[k]]) for k in TERM_KEYS})


def test_set_binary_sets_the_model(gpu_device):
    import torch
    c = _e2e()
    m = c["model"]
    assert torch.equal(m.binary, torch.from_numpy(c["B"])) and m.binary_rho == E2E_RHO
    assert torch.equal(m.R, torch.tensor([[1.0, 0.5], [0.5, 1.0]])) and torch.allclose(m.R_inv @ m.R, torch.eye(2))
    assert torch.equal(m.Y, torch.from_numpy(BR.y_of(c["B"])).float())
    from ame_amd import TemporalAMEModel
    q = TemporalAMEModel(6, 2, 1, seed=1)
    for bad, kw in ((torch.zeros(6, 6, 2), {}), (torch.zeros(6, 5, 2, dtype=torch.bool), {}),
                    (torch.zeros(6, 6, 2, dtype=torch.bool), dict(rho=1.0)),
                    (torch.zeros(6, 6, 2, dtype=torch.uint8), dict(rho=-1.5))):
        with pytest.raises(ValueError):
            q.set_binary(bad, **kw)
    q.set_binary(torch.ones(6, 6, 2, dtype=torch.uint8))
    assert not bool(q.binary[torch.arange(6), torch.arange(6)].any()) and q.binary_rho == 0.0
    q.set_binary(None)
    assert q.binary is None


def test_fit_matches_the_oracle(gpu_device):
    c = _e2e()
    vi, o64, o32 = c["vi"], c["o64"], c["o32"]
    got = _flat(vi.X_mean.numpy(), vi.X_cov.numpy(), vi.elbo_terms())
    a = _flat(o64["X"], o64["S"], o64["terms"][-1])
    b = _flat(o32["X"], o32["S"], o32["terms"][-1])
    keys = ("X", "S") + TERM_KEYS
    for k in keys:
        print(f"{k}: GPU vs fp64 oracle {MR.relative_deviation(a, got, (k,)):.3e}; "
              f"fp32 vs fp64 oracle {MR.relative_deviation(a, b, (k,)):.3e}")
    own, dev = MR.relative_deviation(a, b, keys), MR.relative_deviation(a, got, keys)
    print(f"GPU vs fp64 oracle {dev:.3e}; oracle fp32 vs fp64 {own:.3e}; allowance {4 * own:.3e}")
    assert dev <= 4.0 * own, (dev, own)
    h = vi.history
    assert len(h["elbo"]) == E2E_ITERS
    for it in range(E2E_ITERS):
        want = o64["terms"][it]
        assert abs(float(h["elbo"][it]) - want["elbo"]) <= 4.0 * own * abs(want["elbo"]) + 2.0 ** -23 * abs(want["elbo"])
        assert abs(h["reconstruction_error"][it] - want["recon"]) <= 4.0 * own * want["recon"]
    # the working network is a buffer of its own, rewritten from the final means
    eng = vi.engine
    assert eng.binary and eng.masked and eng.Yt.data_ptr() != eng.Yt_raw.data_ptr() and not eng.swap_consistent
    assert eng.options.pipeline is False and eng.options.speculate is False
    n, T, r = E2E
    Yw = eng.Yt.cpu().numpy()[:, :, :n].transpose(1, 2, 0, 3)
    ref = BR.working_network(vi.X_mean.numpy().astype(np.float64), c["B"], c["mask"], E2E_RHO)
    off = ~np.eye(n, dtype=bool)
    assert np.abs(Yw - ref)[off].max() <= 1e-5
    assert np.array_equal(eng.Yt_raw.cpu().numpy()[:, :, :n].transpose(1, 2, 0, 3), BR.y_of(c["B"]).astype(np.float32))


def test_held_out_scores_and_probabilities(gpu_device):
    c = _e2e()
    vi, mask, B = c["vi"], c["mask"], c["B"]
    n, T, r = E2E
    hid = MR.pack(mask)[1].astype(np.float64)
    total = n * (n - 1) // 2
    held = vi.predictive_check(subset="held_out")
    seen = vi.predictive_check()
    assert sorted(held) == ["accuracy", "base_rate", "brier", "log_score", "mean_prob", "pairs"]
    assert np.array_equal(held["pairs"], hid) and np.array_equal(seen["pairs"], total - hid)
    assert np.array_equal(vi.predictive_check(subset="observed")["brier"], seen["brier"])
    X, S = vi.X_mean.numpy(), vi.X_cov.numpy()
    for got, sel in ((held, HID), (seen, OBS)):
        rows, mag, near = BR.score_rows(X, S, r, B, mask, sel)
        want, ent = BR.check_dict(rows), 2.0 * rows[:, 0]
        assert np.array_equal(got["base_rate"], want["base_rate"])
        assert (np.abs(got["log_score"] - want["log_score"]) <= 5e-6 * mag[:, 1]).all()
        assert (np.abs(got["brier"] - want["brier"]) <= 5e-6 * mag[:, 2] / ent).all()
        assert (np.abs(got["mean_prob"] - want["mean_prob"]) <= 5e-6 * mag[:, 5] / ent).all()
        assert (np.abs(got["accuracy"] - want["accuracy"]) <= near / ent).all()
    print(f"held-out: log score per entry {(held['log_score'] / (2 * hid)).tolist()} accuracy "
          f"{held['accuracy'].tolist()} base rate {held['base_rate'].tolist()}")
    # predict_proba: the same probabilities, entry by entry
    p = vi.predict_proba(slice(0, T), rows=range(2, 20), cols=slice(1, 33)).numpy()
    assert p.shape == (18, 32, T, 2)
    for t in range(T):
        mean, V0, _ = PR.moments(X[:, t], S[:, t], r)
        want = np.stack([BR.phi_cdf(mean[..., 0] / np.sqrt(1 + V0)), BR.phi_cdf(mean[..., 1] / np.sqrt(1 + V0.T))], -1)
        blk = want[2:20, 1:33]
        od = ~np.eye(n, dtype=bool)[2:20, 1:33]
        assert np.abs(p[:, :, t][od] - blk[od]).max() <= 1e-5
        assert np.isnan(p[:, :, t][~od]).all()
    with pytest.raises(ValueError):
        vi.predictive_check(subset="everything")
    Xp, Sp = vi.forecast(2)
    assert tuple(Xp.shape) == (n, 2, 2 + 2 * r) and np.isfinite(Xp.numpy()).all()
    assert np.array_equal(vi.get_variational_means().numpy(), X)


def test_a_model_without_set_binary_is_untouched(gpu_device):
    import torch
    n, T, r = E2E
    runs = {}
    for key in ("plain", "cleared"):
        c = MR.make_case(n, T, r, seed=41, lr=E2E_LR)
        m = c["model"]
        if key == "cleared":   # set, then cleared and the Gaussian data put back
            Y, R, Ri = m.Y.clone(), m.R.clone(), m.R_inv.clone()
            m.set_binary(torch.zeros(n, n, T, dtype=torch.bool), rho=0.3)
            m.set_binary(None)
            m.Y, m.R, m.R_inv = Y, R, Ri
        vi = _vi(m)
        vi.fit(max_iter=3, tolerance=0.0, verbose=False)
        runs[key] = (vi, vi.X_mean.clone(), vi.X_cov.clone(), vi.elbo_terms())
    (va, xa, sa, ta), (vb, xb, sb, tb) = runs["plain"], runs["cleared"]
    assert torch.equal(xa, xb) and torch.equal(sa, sb)
    for k in ta:
        assert abs(ta[k] - tb[k]) <= 1e-12 * abs(ta[k]), (k, ta[k], tb[k])
    for eng in (va.engine, vb.engine):
        assert not eng.binary and not eng.refill
        for attr in ("Bt", "stat", "probit_work", "Yt_raw"):
            assert not hasattr(eng, attr), attr
    with pytest.raises(ValueError):
        va.predict_proba(0)
    # the Gaussian oracle still describes the plain fit
    import ame_oracle as O
    X, S = c["X0"].copy(), c["S0"].copy()
    for _ in range(3):
        O.sweep_stats(c["Y"], X, S, c["params"], "good", E2E_LR)
    assert np.abs(xb.numpy() - X).max() <= 1e-4


def test_unsupported_combinations_say_which(gpu_device):
    import torch
    import covar_ref as CR
    from ame_amd import TemporalAMEModel
    from ame_amd.engine import DeviceEngine, Shard
    n, T, r = 12, 4, 2
    B = torch.from_numpy(np.random.default_rng(0).random((n, n, T)) < 0.4)

    def model(covariates=False):
        m = TemporalAMEModel(n, T, r, seed=3)
        if covariates:
            m.set_covariates(torch.from_numpy(CR.make_w(n, T, 2)), beta=(0.3, -0.2))
        m.generate_data_fast(seed=4)
        m.set_binary(B, rho=0.2)
        return m

    m = model()
    vi = _vi(m)
    with pytest.raises(NotImplementedError, match="time-sharded"):
        DeviceEngine(m, "good", 0.5, vi.X_mean, vi.X_cov, device=torch.device("cuda", 0), shard=Shard(0, 2, T))
    with pytest.raises(NotImplementedError, match="covariates"):
        _vi(model(covariates=True)).fit(max_iter=1, tolerance=0.0, verbose=False)
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    x = vi.X_mean.clone()
    for call in (lambda: vi.fit_em(1, 1, verbose=False), lambda: vi.m_step(), lambda: vi.m_step_statistics(),
                 lambda: vi.smooth(), lambda: vi.predictive_check(smoothed=True), lambda: vi.forecast(1, smoothed=True),
                 lambda: vi.gof(n_sim=1), lambda: vi.network_statistics(),
                 lambda: vi.forecast_check(torch.zeros(n, n, 1, 2))):
        with pytest.raises(NotImplementedError, match="binary"):
            call()
    assert torch.equal(vi.X_mean, x)          # the refusals left the fit alone
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    assert len(vi.history["elbo"]) == 2 and np.isfinite(float(vi.history["elbo"][-1]))
    # without a mask every pair is observed
    chk = vi.predictive_check()
    assert (chk["pairs"] == n * (n - 1) // 2).all()
    with pytest.raises(ValueError):
        vi.predictive_check(subset="held_out")


# ---------------------------------------------------------------------------
# 5. the tails: exact pair means against the mpmath fixture
# ---------------------------------------------------------------------------
# probit_ref.grid_case: r = 1, u = v = 0 and a, b on a 2^-10 grid, so the device
# forms every pair mean exactly (fp64 adds in the fill kernel, fp32 MFMA in the
# score kernel) and everything after it is fp64: held to 4 x TAIL_TAU0 of
# tests/golden/probit_tails.npz (mpmath), TAIL_TAU0 = 3.6e-15 being the scipy
# reference's own deviation from it.  One slice per regime of s m, so the worst
# ratio names the function and the argument range.
TAIL_TOL = 4.0 * BR.TAIL_TAU0


@functools.lru_cache(maxsize=None)
def _tails():
    from conftest import golden
    fx = golden("probit_tails.npz")
    return {k: fx[k] for k in fx.files}


@functools.lru_cache(maxsize=None)
def _grid_device(n, cov):
    g = BR.grid_case(n, 0.0)
    return _Device((n, g["T"], g["r"]), state=(g["X"], g["S"][cov], g["B"]))


@pytest.mark.parametrize("n", BR.GRID_SHAPES, ids=lambda n: f"n{n}")
def test_fill_on_the_tail_grid(n, gpu_device):
    """stat[0] exact, stat[1..3] within 4 x TAIL_TAU0 x the sum of |elementary
    term| of the fixture; every observed entry within 2^-24 |value| + 2^-40 (1 +
    |d|) of own mean + d (the one fp32 rounding the kernel promises, plus slack for
    d's last bits; d from the fixture at n = 20, from the scipy reference at 65).
    Measured on an MI355X, worst |stat - fixture| / (4 TAIL_TAU0 sum|terms|) per
    slice 0..5 over both shapes, both masks and the five rho: 0.022, 0.015, 0.011,
    0.190, 0.011, 0.029; entries at most 0.999 of their bound."""
    fx, dv = _tails(), _grid_device(n, "unit")
    g = BR.grid_case(n, 0.0)
    T = g["T"]
    X64 = g["X"].astype(np.float64)
    # (T, n, n, 2): row i holds (a_i, b_i), its own-perspective mean with p = q = 0
    own = np.stack([X64[:, :, 0].T[:, :, None].repeat(n, 2), X64[:, :, 1].T[:, :, None].repeat(n, 2)], -1)
    eye = np.eye(n, dtype=bool)
    worst = np.zeros(T)
    for rho in BR.GRID_RHOS:
        if n == BR.GRID_SHAPES[0]:
            d = fx[BR.grid_key(n, rho, "d")].transpose(2, 0, 1, 3)
        else:
            d = np.stack([BR.corrections(X64[:, t], g["B"][:, :, t], rho, 1)[1] for t in range(T)])
        for name in BR.GRID_MASKS:
            mask = g["masks"][name]
            Mt = dv.packed(name)
            got, stat = dv.fill(rho, Mt)
            tag = f"n{n} {name} rho={rho}"
            want, mag = fx[BR.grid_key(n, rho, "stat", name)], fx[BR.grid_key(n, rho, "statmag", name)]
            assert np.isnan(got[:, :, :n][:, eye]).all() and np.isnan(got[:, :, n:]).all(), tag
            assert np.isfinite(got[:, :, :n][:, ~eye]).all() and np.isfinite(stat).all(), tag
            assert np.array_equal(stat[:, 0], want[:, 0]), tag
            ratio = np.abs(stat - want)[:, 1:] / (TAIL_TOL * mag[:, 1:])
            print(f"{tag}: |stat - fixture| / allowance per slice {ratio.max(1).tolist()}")
            worst = np.maximum(worst, ratio.max(1))
            assert (ratio <= 1.0).all(), (tag, ratio.tolist())
            obs = ~eye[None] & (~MR.clean(mask).transpose(2, 0, 1) if mask is not None else True)
            value = own + d
            err = np.abs(got[:, :, :n].astype(np.float64) - value)
            bound = 2.0 ** -24 * np.abs(value) + 2.0 ** -40 * (1.0 + np.abs(d))
            r_e = (err / bound)[np.broadcast_to(obs, err.shape[:3])]
            print(f"{tag}: observed entries, max err / bound = {r_e.max():.3f}")
            assert (r_e <= 1.0).all(), (tag, float(r_e.max()))
            if mask is not None:
                hid = MR.clean(mask).transpose(2, 0, 1)
                assert np.array_equal(got[:, :, :n][hid], own.astype(np.float32)[hid]), tag
            # the same bits from a second call and from every two-way split of the slices
            got2, stat2 = dv.fill(rho, Mt)
            assert np.array_equal(stat2.view(np.uint64), stat.view(np.uint64)), tag
            assert np.array_equal(_i32(got2), _i32(got)), tag
            for k in range(1, T):
                ga, sa = dv.fill(rho, Mt, 0, k)
                gb, sb = dv.fill(rho, Mt, k, T)
                assert np.array_equal(np.concatenate([sa, sb]).view(np.uint64), stat.view(np.uint64)), (tag, k)
                assert np.array_equal(_i32(np.concatenate([ga, gb])), _i32(got)), (tag, k)
    print(f"n{n}: worst |stat - fixture| / (4 tau0 sum|terms|) per slice {[f'{w:.3f}' for w in worst]}")


@pytest.mark.parametrize("cov", BR.GRID_COVS)
@pytest.mark.parametrize("n", BR.GRID_SHAPES, ids=lambda n: f"n{n}")
def test_score_on_the_tail_grid(n, cov, gpu_device):
    """Pairs, ties and hits exact (no pi lies near 1/2: |t| >= 2^-11); the sums
    [1], [2], [5] within 4 x TAIL_TAU0 x the sum of |summand| of the fixture, over
    every pair and over the observed and the hidden pairs of a 30 % mask, with
    t = m ("unit") and t = m or m / 2 by the row node ("scaled").  Measured on an
    MI355X, worst |sums - fixture| / (4 TAIL_TAU0 sum|summand|) per slice 0..5:
    unit 0.022, 0.015, 0.010, 0.202, 0.015, 0.013; scaled 0.020, 0.013, 0.015,
    0.050, 0.015, 0.013."""
    fx, dv = _tails(), _grid_device(n, cov)
    T = BR.GRID_T
    Mt = dv.packed("random30")
    worst = np.zeros(T)
    for sel in BR.GRID_SELECTS:
        got = dv.score(Mt if sel else None, sel)
        want, mag = fx[BR.grid_key(n, None, "score", cov, sel)], fx[BR.grid_key(n, None, "scoremag", cov, sel)]
        tag = f"n{n} {cov} select {sel}"
        assert np.isfinite(got).all(), tag
        assert np.array_equal(got[:, [0, 3, 4]], want[:, [0, 3, 4]]), (tag, got, want)
        ratio = np.abs(got - want)[:, [1, 2, 5]] / (TAIL_TOL * mag[:, [1, 2, 5]])
        print(f"{tag}: |sums - fixture| / allowance per slice {ratio.max(1).tolist()}")
        worst = np.maximum(worst, ratio.max(1))
        assert (ratio <= 1.0).all(), (tag, ratio.tolist())
        assert np.array_equal(dv.score(Mt if sel else None, sel).view(np.uint64), got.view(np.uint64)), tag
        for k in range(1, T):
            both = np.concatenate([dv.score(Mt if sel else None, sel, 0, k), dv.score(Mt if sel else None, sel, k, T)])
            assert np.array_equal(both.view(np.uint64), got.view(np.uint64)), (tag, k)
    print(f"n{n} {cov}: worst |sums - fixture| / (4 tau0 sum|summand|) per slice {[f'{w:.3f}' for w in worst]}")
