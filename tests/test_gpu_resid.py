"""Residual diagnostics of a Gaussian fit on the GPU: ame_resid_nodes /
ame_resid_hist / ame_resid_select through the C ABI and node_check /
residual_histogram / top_residuals / forecast_residuals, against the fp64
reference tests/resid_ref.py.

Bounds (derived in resid_ref's docstring from predictive_ref.TOL, the bound the
fp32 MFMA products are held to; nothing is measured on the kernels).
  Node sums: ``pairs`` exact; every other slot within the sum of its pairs'
  bounds; summed over the nodes they equal twice predictive_check's sums to
  1e-10 of the sum of |term| (ten thousand times above an fp64 reordering of
  these term counts, ten thousand times below one fp32 rounding: the same
  per-pair values in another order, not other products).
  Histogram (256 bins to m2_max = 32, where at most 1 % of the reference m2 lie
  within their bound of an edge, test_resid_ref.py): totals exact and for every
  interior edge #{m2 + d < edge} <= cumulative device count <= #{m2 - d < edge}.
  Top-k: with D the largest d(m2) of the slice, every returned pair has m2_ref >=
  (k-th m2_ref) - 2 D and every other pair m2_ref <= (k-th) + 2 D; m2 and z within
  their bounds; rows sorted; the planted pairs first, in order.
  Smoothed states, covariates and forecasts: against the same formulas on
  predict_dyads' / forecast_dyads' dense moments (resid_ref.host_scores).
"""
import ctypes
import functools

import numpy as np
import pytest

import missing_ref as MR
import resid_ref as RR

pytestmark = pytest.mark.gpu

IDS = lambda c: "n%d_T%d_r%d" % c
OBS, HID = MR.OBSERVED, MR.HIDDEN
SUBSETS = {0: None, OBS: "observed", HID: "held_out"}
SELECTS = ((False, 0), (True, OBS), (True, HID))
SLOTS = ("pairs", "log_score", "mahalanobis", "z2 sent", "z2 received", "resid sent", "resid received",
         "sq_err sent", "sq_err received")
TOP_FIELDS = ("i", "j", "m2", "p_value", "z")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@functools.lru_cache(maxsize=None)
def _case(shape):
    """resid_ref.make_case with the reference scores of every slice; with a mask
    node 1 loses every pair of slice 0, so that a node without a pair occurs (n > 2)."""
    c = RR.make_case(shape)
    c["ref"] = RR.case_scores(c, shape[2])
    c["mask"] = c["mask"].copy()
    if shape[0] > 2:
        c["mask"][1, :, 0] = c["mask"][:, 1, 0] = True
    else:                   # one pair: hiding it would leave nothing to fit; "held_out" is then empty
        c["mask"][:] = False
    return c


@functools.lru_cache(maxsize=None)
def _vi(shape, masked):
    """A Gaussian model holding the case's network (and mask) at noise
    resid_ref.NOISE with the case's state assigned: nothing is fitted."""
    import torch
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI
    n, T, r = shape
    c = _case(shape)
    m = TemporalAMEModel(n, T, r, seed=5)
    m.Y = torch.from_numpy(c["Y"].copy())
    m.R = torch.from_numpy(RR.NOISE.astype(np.float32))
    m.R_inv = torch.linalg.inv(m.R)
    if masked:
        m.set_missing(torch.from_numpy(c["mask"]))
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.5, device=torch.device("cuda", 0))
    vi.X_mean = torch.from_numpy(c["X"].copy())
    vi.X_cov = torch.from_numpy(c["S"].copy())
    return vi


def _ref(shape, select):
    c = _case(shape)
    return [RR.subset(d, c["mask"][:, :, t], select) for t, d in enumerate(c["ref"])]


def _node_array(nc):
    """node_check's dictionary back as (T, n, 9)."""
    return np.concatenate([nc["pairs"][..., None].astype(np.float64), nc["log_score"][..., None],
                           nc["mahalanobis"][..., None], nc["z2"], nc["resid"], nc["sq_err"]], -1)


def _assert_nodes(nc, ref, n, tag):
    """Node sums against per-slice reference scores; returns the worst used share of each slot's bound."""
    got = _node_array(nc)
    assert nc["pairs"].dtype == np.int64 and got.shape == (len(ref), n, 9), tag
    worst = np.zeros(9)
    for t, d in enumerate(ref):
        want, bound = RR.node_sums(d, n), RR.node_bounds(d, n)
        assert np.array_equal(got[t, :, 0], want[:, 0]), (tag, t)
        err = np.abs(got[t] - want)
        assert (err <= bound).all(), (tag, t, np.argwhere(err > bound)[:5], (err / np.maximum(bound, 1e-300)).max())
        share = np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0).max(0)
        worst = np.maximum(worst, share)
        none = want[:, 0] == 0
        assert not got[t, none].any(), (tag, t, "a node without a pair must hold exact zeros")
        assert np.isnan(nc["mean_mahalanobis"][t, none]).all(), (tag, t)
        assert np.array_equal(nc["mean_mahalanobis"][t, ~none], got[t, ~none, 2] / got[t, ~none, 0]), (tag, t)
    return worst


def _assert_node_totals(nc, check, ref, n, tag):
    """Summed over the nodes: twice predictive_check's sums, to 1e-10 of sum |term|."""
    got = _node_array(nc)
    for t, d in enumerate(ref):
        tot, scale = got[t].sum(0), RR.node_abs(d, n).sum(0)
        zz, qq = check["z2"][t].sum(), check["sq_err"][t].sum()
        want = np.array([2 * check["pairs"][t], 2 * check["log_score"][t], 2 * check["mahalanobis"][t], zz, zz,
                         np.nan, np.nan, qq, qq])
        for k in (0, 1, 2, 3, 4, 7, 8):
            assert abs(tot[k] - want[k]) <= 1e-10 * scale[k], (tag, t, SLOTS[k], tot[k], want[k], scale[k])
        # the signed residuals: every entry is sent once and received once
        assert abs(tot[5] - tot[6]) <= 1e-10 * scale[5], (tag, t)


# ---------------------------------------------------------------------------
# 1. node sums
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RR.SHAPES, ids=IDS)
def test_node_sums(shape, gpu_device):
    n, T, r = shape
    for masked, select in SELECTS:
        vi, ref = _vi(shape, masked), _ref(shape, select)
        nc = vi.node_check(subset=SUBSETS[select])
        tag = f"{IDS(shape)} select {select}"
        worst = _assert_nodes(nc, ref, n, tag)
        print(f"{tag}: worst used share of the bound " + ", ".join(f"{s} {w:.3f}" for s, w in zip(SLOTS[1:], worst[1:])))
        _assert_node_totals(nc, vi.predictive_check(subset=SUBSETS[select]), ref, n, tag)
    if n > 2:   # the mask took every pair of node 1 in slice 0
        assert _vi(shape, True).node_check(subset="observed")["pairs"][0, 1] == 0


@pytest.mark.parametrize("r", [r for r in range(1, 33) if (65, 2, r) not in RR.SHAPES], ids=lambda r: f"r{r}")
def test_node_sums_at_every_compiled_r(r, gpu_device):
    shape = (65, 2, r)
    worst = _assert_nodes(_vi(shape, False).node_check(), _ref(shape, 0), 65, IDS(shape))
    print(f"{IDS(shape)}: worst used share of the bound {worst[1:].max():.3f}")


# ---------------------------------------------------------------------------
# 2. the histogram of m2
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RR.SHAPES, ids=IDS)
def test_histogram(shape, gpu_device):
    n, T, r = shape
    from ame_amd import residuals
    for masked, select in SELECTS:
        vi, ref = _vi(shape, masked), _ref(shape, select)
        rh = vi.residual_histogram(bins=RR.BINS, m2_max=RR.M2_MAX, subset=SUBSETS[select])
        tag = f"{IDS(shape)} select {select}"
        assert rh["hist"].dtype == np.int64 and rh["hist"].shape == (T, RR.BINS), tag
        assert np.array_equal(rh["edges"], RR.edges()), tag
        assert np.array_equal(rh["pairs"], [len(d["i"]) for d in ref]), tag
        assert np.array_equal(rh["pairs"], vi.predictive_check(subset=SUBSETS[select])["pairs"]), tag
        assert np.allclose(rh["expected"].sum(1), rh["pairs"], rtol=1e-12), tag
        assert np.array_equal(rh["expected"], residuals.expected(rh["pairs"], RR.BINS, RR.M2_MAX)), tag
        exact = 0
        for t, d in enumerate(ref):
            ok, detail = RR.sandwich(rh["hist"][t], d)
            assert ok, (tag, t, detail)
            exact += int(np.array_equal(rh["hist"][t], RR.histogram(d)))
            # the planted m2 = 40, 90, 200 (those selected) are all the end bin holds
            assert rh["hist"][t, -1] == (d["m2"] >= 39.0).sum(), (tag, t)
        print(f"{tag}: slices whose histogram equals the reference's exactly: {exact} of {T}")
    full = _vi(shape, False).residual_histogram(bins=RR.BINS, m2_max=RR.M2_MAX)["hist"]
    assert np.array_equal(full[:, -1], [sum(v >= RR.M2_MAX for _, _, v in pl) for pl in _case(shape)["planted"]])


# ---------------------------------------------------------------------------
# 3. the most surprising pairs
# ---------------------------------------------------------------------------
def _assert_top_within_bounds(top, ref, k, tag):
    for t, d in enumerate(ref):
        P = len(d["i"])
        m = min(k, P)
        i, j, m2, z, pv = top["i"][t], top["j"][t], top["m2"][t], top["z"][t], top["p_value"][t]
        assert (i[m:] == -1).all() and (j[m:] == -1).all(), (tag, t)
        assert np.isnan(m2[m:]).all() and np.isnan(z[m:]).all() and np.isnan(pv[m:]).all(), (tag, t)
        if m == 0:
            continue
        i, j, m2, z, pv = i[:m], j[:m], m2[:m], z[:m], pv[:m]
        assert (i < j).all() and (i >= 0).all(), (tag, t)
        n = int(max(d["j"].max(), j.max())) + 1
        index = np.full((n, n), -1)
        index[d["i"], d["j"]] = np.arange(P)
        at = index[i, j]
        assert (at >= 0).all(), (tag, t, "a pair that is not selected")
        assert len(set(at.tolist())) == m, (tag, t, "a pair twice")
        assert (np.abs(m2 - d["m2"][at]) <= d["d_m2"][at]).all(), (tag, t)
        assert (np.abs(z - d["z"][at]) <= d["d_z"][at]).all(), (tag, t)
        assert np.array_equal(pv, np.exp(-0.5 * m2)), (tag, t)
        assert np.array_equal(np.lexsort((j, i, -m2)), np.arange(m)), (tag, t, "not sorted by (-m2, i, j)")
        D = float(d["d_m2"].max())
        kth = np.sort(d["m2"])[::-1][m - 1]
        assert (d["m2"][at] >= kth - 2 * D).all(), (tag, t)
        rest = np.ones(P, bool)
        rest[at] = False
        assert (d["m2"][rest] <= kth + 2 * D).all(), (tag, t)


@pytest.mark.parametrize("shape", RR.SHAPES, ids=IDS)
def test_top_residuals(shape, gpu_device):
    n, T, r = shape
    c = _case(shape)
    for masked, select in SELECTS:
        vi, ref = _vi(shape, masked), _ref(shape, select)
        for k, bins, m2_max in ((1, 1024, 64.0), (5, 1024, 64.0), (40, 64, 32.0), (7, 2048, 250.0)):
            top = vi.top_residuals(k=k, bins=bins, m2_max=m2_max, subset=SUBSETS[select])
            assert top["i"].shape == (T, k) and top["z"].shape == (T, k, 2)
            assert top["i"].dtype == np.int64 and top["j"].dtype == np.int64
            _assert_top_within_bounds(top, ref, k, f"{IDS(shape)} select {select} k {k} bins {bins}")
    # the planted pairs come first, in order, with their exact (i, j)
    top = _vi(shape, False).top_residuals(k=5)
    for t, pl in enumerate(c["planted"]):
        pl = pl[::-1]
        assert [(int(a), int(b)) for a, b in zip(top["i"][t, :len(pl)], top["j"][t, :len(pl)])] == \
            [(i, j) for i, j, _ in pl], (t, top["i"][t], top["j"][t], pl)
        assert np.allclose(top["m2"][t, :len(pl)], [v for _, _, v in pl], rtol=1e-3), (t, top["m2"][t])
        assert (top["i"][t, len(pl):] == -1).all() if n * (n - 1) // 2 < 5 else (top["i"][t] >= 0).all()


# ---------------------------------------------------------------------------
# 4. other states: smoothed, covariates, forecasts (against predict_dyads' moments)
# ---------------------------------------------------------------------------
def _host_ref(mean, second, Y, mask=None, select=0, model=None, W=None):
    """resid_ref.host_scores of every slice of dense moments (n, n, S, .); with
    covariates W (p, n, n, S, 2) the residuals' bound also allows for the fp32 sums
    with beta_k W_k on both sides."""
    out = []
    extra = None
    if W is not None:
        extra = np.einsum("k,kijtc->ijtc", np.abs(model.beta.numpy().astype(np.float64)), np.abs(W.numpy()))
    for t in range(mean.shape[2]):
        d = RR.host_scores(mean[:, :, t], second[:, :, t], Y[:, :, t], extra=None if extra is None else extra[:, :, t])
        out.append(RR.subset(d, mask[:, :, t], select) if select else d)
    return out


def _assert_all_three(nc, rh, top, ref, n, k, tag):
    worst = _assert_nodes(nc, ref, n, tag)
    print(f"{tag}: worst used share of the host bound {worst[1:].max():.3f}")
    for t, d in enumerate(ref):
        ok, detail = RR.sandwich(rh["hist"][t], d, rh["hist"].shape[1], float(rh["edges"][-1]))
        assert ok, (tag, t, detail)
    _assert_top_within_bounds(top, ref, k, tag)


@functools.lru_cache(maxsize=None)
def _fitted(covariates, masked):
    import torch
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI
    n, T, r = 33, 3, 2
    m = TemporalAMEModel(n, T, r, seed=3)
    if covariates:
        g = torch.Generator().manual_seed(5)
        W = torch.randn(2, n, n, T, 2, generator=g)
        W[:, :, :, :, 1] = W[:, :, :, :, 0].transpose(1, 2)
        m.set_covariates(W, beta=[0.7, -0.4])
    m.generate_data_fast(seed=4)
    mask = MR.random_mask(n, T, 0.3, seed=3) if masked else None
    if masked:
        m.set_missing(torch.from_numpy(mask))
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.5, device=torch.device("cuda", 0))
    vi.fit(max_iter=5, tolerance=0.0, verbose=False)
    return m, mask, vi


def test_smoothed_state(gpu_device):
    import torch
    for masked, smoothed, select in ((False, True, 0), (True, "observed", HID)):
        m, mask, vi = _fitted(False, masked)
        X0, S0, hist0 = vi.X_mean.clone(), vi.X_cov.clone(), {k: list(v) for k, v in vi.history.items()}
        kw = dict(smoothed=smoothed, subset=SUBSETS[select])
        nc, rh = vi.node_check(**kw), vi.residual_histogram(bins=RR.BINS, m2_max=RR.M2_MAX, **kw)
        top = vi.top_residuals(k=6, **kw)
        mean, second = vi.predict_dyads(slice(None), smoothed=smoothed)
        ref = _host_ref(mean.numpy(), second.numpy(), m.Y.numpy(), mask, select)
        _assert_all_three(nc, rh, top, ref, m.n, 6, f"smoothed={smoothed!r} select {select}")
        # a smoothed score is not the fit's: the state really was exchanged
        assert not np.array_equal(nc["mahalanobis"], vi.node_check(subset=SUBSETS[select])["mahalanobis"])
        # no disturbance
        assert torch.equal(vi.X_mean, X0) and torch.equal(vi.X_cov, S0)
        assert {k: list(v) for k, v in vi.history.items()} == hist0


def test_covariates_score_the_residual_network(gpu_device):
    m, _, vi = _fitted(True, False)
    nc, rh = vi.node_check(), vi.residual_histogram(bins=RR.BINS, m2_max=RR.M2_MAX)
    top = vi.top_residuals(k=6)
    mean, second = vi.predict_dyads(slice(None))          # the means carry sum_k beta_k w_k
    ref = _host_ref(mean.numpy(), second.numpy(), m.Y.numpy(), model=m, W=m.W)
    _assert_all_three(nc, rh, top, ref, m.n, 6, "covariates")
    plain = _host_ref((mean - m.covariate_effect()).numpy(), second.numpy(), m.Y.numpy(), model=m, W=m.W)
    assert not (np.abs(_node_array(nc)[0] - RR.node_sums(plain[0], m.n)) <= RR.node_bounds(plain[0], m.n)).all()


def test_forecast_residuals(gpu_device):
    import torch
    for covariates in (False, True):
        m, _, vi = _fitted(covariates, False)
        n, h = m.n, 2
        g = torch.Generator().manual_seed(8)
        Yf = torch.randn(n, n, h, 2, generator=g)
        Yf[:, :, :, 1] = Yf[:, :, :, 0].transpose(0, 1)
        Wf = None
        if covariates:
            Wf = torch.randn(2, n, n, h, 2, generator=g)
            Wf[:, :, :, :, 1] = Wf[:, :, :, :, 0].transpose(1, 2)
        mf = MR.random_mask(n, h, 0.3, seed=9)
        for missing, select in ((None, 0), (mf, OBS)):
            fr = vi.forecast_residuals(Yf, k=6, W_future=Wf, missing_future=missing, bins=RR.BINS, m2_max=RR.M2_MAX)
            mean, second = vi.forecast_dyads(h, W_future=Wf)
            ref = _host_ref(mean.numpy(), second.numpy(), Yf.numpy(), mf, select, model=m, W=Wf)
            tag = f"forecast covariates={covariates} select {select}"
            _assert_all_three(fr["nodes"], fr["histogram"], fr["top"], ref, n, 6, tag)
            fc = vi.forecast_check(Yf, W_future=Wf, missing_future=missing)
            assert np.array_equal(fr["histogram"]["pairs"], fc["pairs"]), tag
            _assert_node_totals(fr["nodes"], fc, ref, n, tag)
        assert vi.forecast_residuals(Yf, k=0, W_future=Wf)["top"] is None
    with pytest.raises(ValueError):
        vi.forecast_residuals(Yf[:, :5], W_future=Wf)


# ---------------------------------------------------------------------------
# 5. the C ABI: a NaN pair
# ---------------------------------------------------------------------------
class _Direct:
    """The three entry points on an engine's device tensors, through ctypes."""

    def __init__(self, vi):
        from ame_amd import _lib
        self.eng, self.L, self._lib = vi.engine, vi.engine.L, _lib
        self.eng.discard_speculation()
        import torch
        torch.cuda.synchronize()
        self.noise = (ctypes.c_double * 4)(*RR.NOISE.ravel())

    def dims(self, S):
        e = self.eng
        return self._lib.ame_dims(e.n, e.r, S, 0, S, e.vcode)

    def _work(self, query, S):
        import torch
        ws = int(query(ctypes.byref(self.dims(S))))
        return torch.empty(ws, dtype=torch.float64, device=self.eng.dev), ws

    def nodes(self, x, cov, Yt):
        import torch
        S = int(x.shape[0])
        work, ws = self._work(self.L.ame_resid_nodes_work_size, S)
        node = torch.full((S, self.eng.n, 9), -7.0, dtype=torch.float64, device=self.eng.dev)   # overwritten
        a = self._lib.ame_resid_nodes_args(x=_ptr(x), cov=_ptr(cov), Yt=_ptr(Yt), noise=self.noise, node=_ptr(node),
                                           work=_ptr(work), work_doubles=ws)
        self._lib.check(self.L.ame_resid_nodes(ctypes.byref(self.dims(S)), ctypes.byref(a), None), "ame_resid_nodes")
        torch.cuda.synchronize()
        return node.cpu().numpy()

    def hist(self, x, cov, Yt, bins, m2_max):
        import torch
        from ame_amd import residuals
        S = int(x.shape[0])
        work, ws = self._work(self.L.ame_resid_hist_work_size, S)
        hist = torch.full((S, bins), -1, dtype=torch.int64, device=self.eng.dev)                # overwritten
        a = self._lib.ame_resid_hist_args(x=_ptr(x), cov=_ptr(cov), Yt=_ptr(Yt), noise=self.noise, hist=_ptr(hist),
                                          work=_ptr(work), work_doubles=ws, nbins=bins,
                                          scale=residuals.scale(bins, m2_max))
        self._lib.check(self.L.ame_resid_hist(ctypes.byref(self.dims(S)), ctypes.byref(a), None), "ame_resid_hist")
        torch.cuda.synchronize()
        return hist.cpu().numpy()

    def select(self, x, cov, Yt, bins, m2_max, bin_min, cap, slice0=0):
        import torch
        from ame_amd import residuals
        S = int(x.shape[0])
        work, ws = self._work(self.L.ame_resid_select_work_size, S)
        off = np.concatenate([[0], np.cumsum(cap)]).astype(np.int64)
        dev = self.eng.dev
        d_off, d_bin = torch.from_numpy(off).to(dev), torch.from_numpy(np.asarray(bin_min, np.int32)).to(dev)
        rec = torch.zeros(max(1, int(off[-1])) * 5, dtype=torch.int64, device=dev)
        count = torch.full((S,), -1, dtype=torch.int64, device=dev)
        a = self._lib.ame_resid_select_args(x=_ptr(x), cov=_ptr(cov), Yt=_ptr(Yt), noise=self.noise, work=_ptr(work),
                                            work_doubles=ws, nbins=bins, scale=residuals.scale(bins, m2_max),
                                            bin_min=_ptr(d_bin), slice0=slice0, offset=_ptr(d_off), count=_ptr(count),
                                            records=_ptr(rec))
        self._lib.check(self.L.ame_resid_select(ctypes.byref(self.dims(S)), ctypes.byref(a), None), "ame_resid_select")
        torch.cuda.synchronize()
        return rec.cpu().numpy().view(residuals.RECORD)[:int(off[-1])], off, count.cpu().numpy()


def test_c_abi_nan_pair(gpu_device):
    from ame_amd import residuals
    shape = (65, 2, 5)
    n, T, r = shape
    dv = _Direct(_vi(shape, False))
    eng = dv.eng
    x, cov, Yt = eng.x_a, eng.cov, eng.Yt.clone()
    i0, j0 = 3, 64                                   # a pair of the one-wide edge tile
    Yt[0, i0, j0, 0] = float("nan")
    bins, m2_max = RR.BINS, RR.M2_MAX
    clean = dv.hist(x, cov, eng.Yt, bins, m2_max)
    hist = dv.hist(x, cov, Yt, bins, m2_max)
    assert (hist >= 0).all() and np.array_equal(hist.sum(1), [n * (n - 1) // 2] * T)
    assert hist[0, -1] == clean[0, -1] + 1 and np.array_equal(hist[1], clean[1])
    assert np.array_equal(clean, _vi(shape, False).residual_histogram(bins=bins, m2_max=m2_max)["hist"])
    bin_min, cap = residuals.threshold(hist, 3)
    rec, off, count = dv.select(x, cov, Yt, bins, m2_max, bin_min, cap)
    assert np.array_equal(count, cap) and (rec["pad"] == 0).all()
    assert all((rec["slice"][off[t]:off[t + 1]] == t).all() for t in range(T))
    top = residuals.top_k(rec, off, 3)
    assert (top["i"][0, 0], top["j"][0, 0]) == (i0, j0) and np.isnan(top["m2"][0, 0]) and np.isnan(top["z"][0, 0, 0])
    assert np.isfinite(top["z"][0, 0, 1]) and np.isfinite(top["m2"][0, 1:]).all() and np.isfinite(top["m2"][1]).all()
    # a region that is too small: the pairs beyond it are counted, not written
    rec1, off1, count1 = dv.select(x, cov, Yt, bins, m2_max, bin_min, np.minimum(cap, 1))
    assert np.array_equal(count1, cap) and len(rec1) == T
    node = dv.nodes(x, cov, Yt)
    bad = np.isnan(node).any(2)
    want = np.zeros((T, n), bool)
    want[0, [i0, j0]] = True
    assert np.array_equal(bad, want), np.argwhere(bad != want)
    assert np.array_equal(node[:, :, 0], np.full((T, n), n - 1.0))
    good = dv.nodes(x, cov, eng.Yt)
    assert np.array_equal(_bits(good[~want]), _bits(node[~want]))
    assert np.array_equal(_bits(good), _bits(_node_array(_vi(shape, False).node_check())))


# ---------------------------------------------------------------------------
# 6. determinism
# ---------------------------------------------------------------------------
def _all_three(vi, **kw):
    return (_node_array(vi.node_check(**kw)), vi.residual_histogram(bins=1024, **kw)["hist"],
            vi.top_residuals(k=40, **kw))


def _assert_same(a, b, tag):
    assert np.array_equal(_bits(a[0]), _bits(b[0])), (tag, "node")
    assert np.array_equal(a[1], b[1]), (tag, "hist")
    for f in TOP_FIELDS:
        assert np.array_equal(_bits(a[2][f]), _bits(b[2][f])), (tag, f)


def test_second_call_and_chunked_slices_give_the_same_bits(gpu_device):
    shape = (70, 8, 3)
    vi = _vi(shape, True)
    kw = dict(subset="held_out")
    first, second = _all_three(vi, **kw), _all_three(vi, **kw)
    eng = vi.engine
    from ame_amd import _lib
    one = _lib.ame_dims(eng.n, eng.r, 1, 0, 1, eng.vcode)
    eng.PREDICT_WORK_DOUBLES = int(eng.L.ame_resid_nodes_work_size(ctypes.byref(one))) * 3   # chunks of 3, 3, 2
    try:
        for q in (eng.L.ame_resid_nodes_work_size, eng.L.ame_resid_hist_work_size, eng.L.ame_resid_select_work_size):
            assert 1 <= eng._slice_chunk(q, shape[1])[0] < shape[1]
        assert eng._slice_chunk(eng.L.ame_resid_nodes_work_size, shape[1])[0] == 3
        chunked = _all_three(vi, **kw)
    finally:
        del eng.PREDICT_WORK_DOUBLES
    assert eng._slice_chunk(eng.L.ame_resid_nodes_work_size, shape[1])[0] == shape[1]
    _assert_same(first, second, "second call")
    _assert_same(first, chunked, "chunked")


def test_both_slice_mappings_give_the_same_bits(gpu_device):
    """8 slices take the multiple-of-8 workgroup -> (slice, tile) mapping, 3 and 5 the
    slice-major one: every slice's node sums, histogram and records are the same."""
    from ame_amd import residuals
    shape = (70, 8, 3)
    n, T, r = shape
    dv = _Direct(_vi(shape, False))
    eng = dv.eng
    x, cov, Yt = eng.x_a, eng.cov, eng.Yt
    bins, m2_max = 1024, 64.0
    node, hist = dv.nodes(x, cov, Yt), dv.hist(x, cov, Yt, bins, m2_max)
    bin_min, cap = residuals.threshold(hist, 25)
    rec, off, count = dv.select(x, cov, Yt, bins, m2_max, bin_min, cap)
    assert np.array_equal(count, cap) and (cap >= 25).all()
    top = residuals.top_k(rec, off, 25)
    for t0, t1 in ((0, 3), (3, 8)):
        sl = slice(t0, t1)
        assert np.array_equal(_bits(dv.nodes(x[sl], cov[sl], Yt[sl])), _bits(node[sl])), (t0, t1)
        assert np.array_equal(dv.hist(x[sl], cov[sl], Yt[sl], bins, m2_max), hist[sl]), (t0, t1)
        r2, o2, c2 = dv.select(x[sl], cov[sl], Yt[sl], bins, m2_max, bin_min[sl], cap[sl], slice0=t0)
        assert np.array_equal(c2, cap[sl]) and all((r2["slice"][o2[k]:o2[k + 1]] == t0 + k).all() for k in range(t1 - t0))
        part = residuals.top_k(r2, o2, 25)
        for f in TOP_FIELDS:
            assert np.array_equal(_bits(part[f]), _bits(top[f][sl])), (t0, t1, f)


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals(gpu_device):
    import torch
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI
    n, T, r = 12, 3, 2
    dev = torch.device("cuda", 0)
    Yf = torch.zeros(n, n, 1, 2)
    calls = lambda v: (lambda: v.node_check(), lambda: v.residual_histogram(), lambda: v.top_residuals(k=3),
                       lambda: v.forecast_residuals(Yf))
    b = TemporalAMEModel(n, T, r, seed=3)
    b.set_binary(torch.from_numpy(np.random.default_rng(0).random((n, n, T)) < 0.4), rho=0.2)
    vb = TemporalAMEStructuredMFVI(b, factorization="good", learning_rate=0.5, device=dev)
    for call in calls(vb):
        with pytest.raises(NotImplementedError, match="binary"):
            call()
    g = TemporalAMEModel(n, T, r, seed=3)
    g.generate_data_fast(seed=4)
    sharded = TemporalAMEStructuredMFVI(g, factorization="good", learning_rate=0.5, distributed=True)
    for call in calls(sharded):
        with pytest.raises(NotImplementedError, match="time-sharded"):
            call()
        assert sharded._engine is None
    vi = TemporalAMEStructuredMFVI(g, factorization="good", learning_rate=0.5, device=dev)
    vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    x, s, hist = vi.X_mean.clone(), vi.X_cov.clone(), {k: list(v) for k, v in vi.history.items()}
    for call in (lambda: vi.node_check(subset="held_out"), lambda: vi.residual_histogram(subset="observed"),
                 lambda: vi.top_residuals(k=0), lambda: vi.top_residuals(k=-2), lambda: vi.top_residuals(k=2.5),
                 lambda: vi.residual_histogram(bins=0), lambda: vi.residual_histogram(bins=2049),
                 lambda: vi.top_residuals(k=3, bins=4096), lambda: vi.residual_histogram(m2_max=0.0),
                 lambda: vi.top_residuals(k=3, m2_max=float("inf")), lambda: vi.forecast_residuals(Yf, k=-1),
                 lambda: vi.node_check(smoothed="observed")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="m2_max.*bins|bins.*m2_max"):     # one bin: every pair is a candidate
        vi.top_residuals(k=1, bins=1, max_records=10)
    assert vi.top_residuals(k=1, bins=1)["m2"].shape == (T, 1)
    # the calls and the refusals left the fit alone
    vi.node_check(), vi.residual_histogram(), vi.top_residuals(k=4)
    assert torch.equal(vi.X_mean, x) and torch.equal(vi.X_cov, s)
    assert {k: list(v) for k, v in vi.history.items()} == hist
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    assert np.isfinite(float(vi.history["elbo"][-1]))
