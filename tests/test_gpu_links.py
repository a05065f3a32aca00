"""Link ranking of binary networks on the GPU: ame_probit_rank / ame_probit_select
through the C ABI and link_roc / top_links / forecast_links on a binary model,
against the fp64 reference tests/links_ref.py.

Bounds.
  Exact grid (probit_ref.grid_case): every score is exact (m or m / 2, a
  multiple of 2^-11) and with t_max = 8 and 64 or 1024 bins the edges are
  multiples of 2^-2 / 2^-6, so histograms equal numpy's integer for integer and
  top_links equals the brute-force top-k bit for bit, through exact ties.
  Random states: class totals and pairs exact; for every class and interior
  edge #{t_ref + delta < edge} <= cumulative device count <= #{t_ref - delta <
  edge}, delta being links_ref's per-entry bound derived from the bounds of the
  fp32 MFMA products (predictive_ref.TOL); at most 1 % of the reference scores
  lie within delta of an edge (checked without a GPU in test_links_ref.py).
  Top-k: with D the largest delta of the slice's candidates, every returned
  entry has t_ref >= (k-th t_ref) - 2 D, every other candidate t_ref <= (k-th
  t_ref) + 2 D, |score - t_ref| <= delta, tie exact, rows sorted.
  Reproducibility: the same bits from a second call, from slices forced
  through more than one chunk and under both slice mappings.
"""
import ctypes
import functools

import numpy as np
import pytest

import links_ref as LR
import missing_ref as MR
import predictive_ref as PR
import probit_ref as BR
from test_links_ref import CASES, RANDOM_BINS, random_scores

pytestmark = pytest.mark.gpu

IDS = lambda c: "n%d_T%d_r%d" % c
OBS, HID = MR.OBSERVED, MR.HIDDEN
SUBSETS = {0: None, OBS: "observed", HID: "held_out"}
TOP_FIELDS = ("sender", "receiver", "tie", "score", "prob")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _vi(n, T, r, X, S, B, mask=None, **kw):
    """A binary model holding the ties B (and the mask) with the state (X, S)
    assigned: nothing is fitted, the calls under test read this state."""
    import torch
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI
    m = TemporalAMEModel(n, T, r, seed=1)
    m.set_binary(torch.from_numpy(np.ascontiguousarray(B)))
    if mask is not None:
        m.set_missing(torch.from_numpy(mask))
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.5, device=torch.device("cuda", 0), **kw)
    vi.X_mean = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).clone()
    vi.X_cov = torch.from_numpy(np.ascontiguousarray(S, dtype=np.float32)).clone()
    return vi


def _assert_top_equal(got, want_rows, tag):
    """top_links' dict against links_ref.top_k's per-slice rows, bit for bit."""
    for t, w in enumerate(want_rows):
        for k in ("sender", "receiver", "tie"):
            assert np.array_equal(got[k][t], w[k]), (tag, t, k, got[k][t], w[k])
        assert np.array_equal(_bits(got["score"][t]), _bits(w["score"])), (tag, t, got["score"][t], w["score"])
        pad = w["sender"] < 0
        assert np.isnan(got["prob"][t][pad]).all(), (tag, t)
        assert np.allclose(got["prob"][t][~pad], BR.phi_cdf(w["score"][~pad]), rtol=1e-13, atol=1e-300), (tag, t)


# ---------------------------------------------------------------------------
# 1. the exact grid
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid(n, cov, masked):
    g = BR.grid_case(n, 0.0)
    mask = g["masks"]["random30"] if masked else None
    vi = _vi(n, g["T"], g["r"], g["X"], g["S"][cov], g["B"], mask)
    sc = LR.scores(g["X"], g["S"][cov], g["r"], g["B"])
    return g, mask, vi, sc


@pytest.mark.parametrize("cov", BR.GRID_COVS)
@pytest.mark.parametrize("n", BR.GRID_SHAPES, ids=lambda n: f"n{n}")
def test_exact_grid_histograms_and_top_links(n, cov, gpu_device):
    for select in BR.GRID_SELECTS:
        g, mask, vi, full = _grid(n, cov, bool(select))
        sc = [LR.subset(d, mask[:, :, t], select) if select else d for t, d in enumerate(full)]
        tag = f"n{n} {cov} select {select}"
        # both clamps run
        tt = np.concatenate([d["t"].ravel() for d in sc])
        assert tt.max() > 8.0 and tt.min() < -8.0, tag
        assert np.array_equal(tt * 2048, np.round(tt * 2048)), tag
        for bins in (64, 1024):
            roc = vi.link_roc(subset=SUBSETS[select], bins=bins, t_max=8.0)
            want = LR.histograms(sc, bins)
            assert roc["hist"].dtype == np.int64 and np.array_equal(roc["hist"], want), (tag, bins)
            assert np.array_equal(roc["pairs"], [len(d["i"]) for d in sc]), (tag, bins)
            assert np.array_equal(roc["edges"], LR.edges(bins)), (tag, bins)
        most = max(2 * len(d["i"]) for d in sc)
        for ties in (None, 0, 1):
            for k in (1, 7, most + 5):
                got = vi.top_links(k=k, subset=SUBSETS[select], ties=ties, bins=1024 if k != 7 else 64, t_max=8.0)
                _assert_top_equal(got, [LR.top_k(d, k, ties) for d in sc], f"{tag} ties {ties} k {k}")
    # the grid is full of exact ties: the tie-break decided rows
    d = full[0]
    t0 = LR.top_k(d, 2 * len(d["i"]))["score"]
    assert (np.diff(t0) == 0).any()


def test_scores_on_an_edge_go_to_the_upper_bin(gpu_device):
    """a, b multiples of 1/4 (the grid's own means are odd multiples of 2^-10 and
    never meet an edge): every score is an edge of both bin counts."""
    n, T = 20, 2
    rng = np.random.default_rng(5)
    X = np.zeros((n, T, 4), np.float32)
    X[:, :, 0], X[:, :, 1] = rng.integers(-20, 21, (n, T)) / 4.0, rng.integers(-20, 21, (n, T)) / 4.0
    S = np.zeros((n, T, 4, 4), np.float32)
    B = rng.random((n, n, T)) < 0.5
    B[np.arange(n), np.arange(n)] = False
    vi = _vi(n, T, 1, X, S, B)
    sc = LR.scores(X, S, 1, B)
    tt = np.concatenate([d["t"].ravel() for d in sc])
    assert np.array_equal(tt * 4, np.round(tt * 4)) and tt.max() >= 8.0 and tt.min() < -8.0
    for bins in (64, 1024):
        hist = vi.link_roc(bins=bins)["hist"]
        assert np.array_equal(hist, LR.histograms(sc, bins)), bins
        ed = LR.edges(bins)
        inside = tt[(tt >= -8.0) & (tt < 8.0)]
        assert np.array_equal(ed[LR.bin_of(inside, bins)], inside)      # the bin whose lower edge the score is
    for k in (3, 50):
        _assert_top_equal(vi.top_links(k=k, bins=64), [LR.top_k(d, k) for d in sc], f"edges k {k}")


# ---------------------------------------------------------------------------
# 2, 3. random states
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random(case, masked):
    n, T, r = case
    X, S, B, full = random_scores(case)
    mask = MR.random_mask(n, T, 0.3, seed=7) if masked else None
    return X, S, B, mask, full, _vi(n, T, r, X, S, B, mask)


def _selected(case, masked, select):
    X, S, B, mask, full, vi = _random(case, masked)
    return [LR.subset(d, mask[:, :, t], select) if select else d for t, d in enumerate(full)], vi, B


def _assert_sandwich(hist, sc, bins, tag):
    for t, d in enumerate(sc):
        assert hist[t, 1].sum() == d["y"].sum() and hist[t, 0].sum() == (~d["y"]).sum(), (tag, t)
        ok, detail = LR.sandwich(hist[t], d, bins)
        assert ok, (tag, t, detail)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_state_histograms(case, gpu_device):
    for masked, select in ((False, 0), (True, OBS), (True, HID)):
        sc, vi, _ = _selected(case, masked, select)
        for bins in RANDOM_BINS:
            roc = vi.link_roc(subset=SUBSETS[select], bins=bins)
            tag = f"{IDS(case)} select {select} bins {bins}"
            assert np.array_equal(roc["pairs"], [len(d["i"]) for d in sc]), tag
            assert np.array_equal(roc["positives"], [d["y"].sum() for d in sc]), tag
            assert np.array_equal(roc["negatives"], [(~d["y"]).sum() for d in sc]), tag
            _assert_sandwich(roc["hist"], sc, bins, tag)
            exact = [LR.auc_exact(d["t"][d["y"]], d["t"][~d["y"]])[3] for d in sc] if case[0] <= 65 else None
            print(f"{tag}: auc {roc['auc'].tolist()} bracket width {(roc['auc_hi'] - roc['auc_lo']).max():.2e}"
                  f" exact AUC of the reference scores {exact}")


def _assert_top_within_bounds(got, sc, B, k, ties, tag):
    n = B.shape[0]
    for t, d in enumerate(sc):
        ts, snd, rcv, tie = LR.entries(d, ties)
        dl = LR.entries(dict(d, t=d["delta"]), ties)[0]
        tref, dref = np.full((n, n), np.nan), np.zeros((n, n))
        tref[snd, rcv], dref[snd, rcv] = ts, dl
        m = min(k, len(ts))
        s, r_, sc_, ti = got["sender"][t], got["receiver"][t], got["score"][t], got["tie"][t]
        assert (s[m:] == -1).all() and (r_[m:] == -1).all() and (ti[m:] == -1).all(), (tag, t)
        assert np.isnan(sc_[m:]).all() and np.isnan(got["prob"][t][m:]).all(), (tag, t)
        if m == 0:
            continue
        s, r_, sc_, ti = s[:m], r_[:m], sc_[:m], ti[:m]
        assert np.isfinite(tref[s, r_]).all(), (tag, t, "an entry that is no candidate")
        assert len(set(zip(s.tolist(), r_.tolist()))) == m, (tag, t, "an entry twice")
        assert np.array_equal(ti, B[s, r_, t].astype(np.int64)), (tag, t)
        assert (np.abs(sc_ - tref[s, r_]) <= dref[s, r_]).all(), (tag, t)
        assert np.allclose(got["prob"][t][:m], BR.phi_cdf(sc_), rtol=1e-13, atol=1e-300), (tag, t)
        order = np.lexsort((r_, s, -sc_))
        assert np.array_equal(order, np.arange(m)), (tag, t, "not sorted by (-score, sender, receiver)")
        D = float(dl.max())
        kth = np.sort(ts)[::-1][m - 1]
        assert (tref[s, r_] >= kth - 2 * D).all(), (tag, t)
        rest = np.ones(len(ts), bool)
        rest[np.nonzero(np.isin(snd * n + rcv, s * n + r_))[0]] = False
        assert (ts[rest] <= kth + 2 * D).all(), (tag, t)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_state_top_links(case, gpu_device):
    for masked, select in ((False, 0), (True, HID)):
        sc, vi, B = _selected(case, masked, select)
        for k, ties, bins in ((1, None, 1024), (10, 0, 1024), (300, None, 37), (50, 1, 2048)):
            got = vi.top_links(k=k, subset=SUBSETS[select], ties=ties, bins=bins)
            assert all(got[f].shape == (case[1], k) for f in TOP_FIELDS)
            _assert_top_within_bounds(got, sc, B, k, ties, f"{IDS(case)} select {select} k {k} ties {ties}")


# ---------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------
def test_second_call_and_chunked_slices_give_the_same_bits(gpu_device):
    case = (65, 4, 5)
    X, S, B, mask, full, vi = _random(case, True)
    kw = dict(subset="held_out", bins=1024)
    roc, top = vi.link_roc(**kw), vi.top_links(k=40, **kw)
    roc2, top2 = vi.link_roc(**kw), vi.top_links(k=40, **kw)
    eng = vi.engine
    from ame_amd import _lib
    per = int(eng.L.ame_probit_rank_work_size(ctypes.byref(_lib.ame_dims(eng.n, eng.r, 1, 0, 1, eng.vcode))))
    eng.PREDICT_WORK_DOUBLES = per            # one slice per call: four chunks
    try:
        assert eng._slice_chunk(eng.L.ame_probit_rank_work_size, case[1])[0] == 1
        roc3, top3 = vi.link_roc(**kw), vi.top_links(k=40, **kw)
    finally:
        del eng.PREDICT_WORK_DOUBLES
    assert eng._slice_chunk(eng.L.ame_probit_rank_work_size, case[1])[0] == case[1]
    for other_roc, other_top in ((roc2, top2), (roc3, top3)):
        assert np.array_equal(other_roc["hist"], roc["hist"])
        for f in TOP_FIELDS:
            assert np.array_equal(_bits(other_top[f]), _bits(top[f])), f


def test_both_slice_mappings_give_the_same_bits(gpu_device):
    """A slice count that is a multiple of 8 takes the other workgroup -> (slice,
    tile) mapping: each slice's histogram and records equal a one-slice call's."""
    import torch
    from ame_amd import _lib, links
    from test_gpu_probit import _Device
    dv = _Device((70, 8, 2))
    n, T, r = dv.case
    L, Mt = dv.lib, dv.packed("random30")
    bins, t_max = 256, 8.0

    def rank(t0, t1):
        dims = dv.dims(t0, t1)
        ws = int(L.ame_probit_rank_work_size(ctypes.byref(dims)))
        work = torch.empty(ws, dtype=torch.float64, device=dv.dev)
        hist = torch.full((t1 - t0, 2, bins), -1, dtype=torch.int64, device=dv.dev)   # overwritten, not added to
        a = _lib.ame_probit_rank_args(x=_ptr(dv.x[t0:t1]), cov=_ptr(dv.cov[t0:t1]), Yt=_ptr(dv.Y01[t0:t1]),
                                      hist=_ptr(hist), work=_ptr(work), work_doubles=ws, Mt=_ptr(Mt[t0:t1]),
                                      mask_select=HID, nbins=bins, t_max=t_max, scale=links.scale(bins, t_max))
        _lib.check(L.ame_probit_rank(ctypes.byref(dims), ctypes.byref(a), None), "ame_probit_rank")
        torch.cuda.synchronize()
        return hist.cpu().numpy()

    def select(t0, t1, bin_min, cap, slice0):
        S = t1 - t0
        dims = dv.dims(t0, t1)
        ws = int(L.ame_probit_select_work_size(ctypes.byref(dims)))
        work = torch.empty(ws, dtype=torch.float64, device=dv.dev)
        off = np.concatenate([[0], np.cumsum(cap)]).astype(np.int64)
        d_off, d_bin = torch.from_numpy(off).to(dv.dev), torch.from_numpy(bin_min.astype(np.int32)).to(dv.dev)
        rec = torch.zeros(max(1, int(off[-1])) * 3, dtype=torch.int64, device=dv.dev)
        count = torch.full((S,), -1, dtype=torch.int64, device=dv.dev)
        a = _lib.ame_probit_select_args(x=_ptr(dv.x[t0:t1]), cov=_ptr(dv.cov[t0:t1]), Yt=_ptr(dv.Y01[t0:t1]),
                                        work=_ptr(work), work_doubles=ws, Mt=_ptr(Mt[t0:t1]), mask_select=HID,
                                        nbins=bins, t_max=t_max, scale=links.scale(bins, t_max), bin_min=_ptr(d_bin),
                                        tie_filter=-1, slice0=slice0, offset=_ptr(d_off), count=_ptr(count),
                                        records=_ptr(rec))
        _lib.check(L.ame_probit_select(ctypes.byref(dims), ctypes.byref(a), None), "ame_probit_select")
        torch.cuda.synchronize()
        recs = rec.cpu().numpy().view(links.RECORD)[:int(off[-1])]
        return [np.sort(recs[off[s]:off[s + 1]], order=["sender", "receiver"]) for s in range(S)], count.cpu().numpy()

    hist = rank(0, T)
    assert (hist >= 0).all() and np.array_equal(hist.sum((1, 2)), 2 * MR.pack(dv.masks["random30"])[1])
    bin_min, cap = links.threshold(hist, 25)
    recs, count = select(0, T, bin_min, cap, 0)
    assert np.array_equal(count, cap)
    for t in (0, 3, 7):
        assert np.array_equal(rank(t, t + 1)[0], hist[t]), t
        r1, c1 = select(t, t + 1, bin_min[t:t + 1], cap[t:t + 1], t)
        assert c1[0] == cap[t] and np.array_equal(r1[0], recs[t]), t
        assert (recs[t]["slice"] == t).all() and len(recs[t]) == cap[t] >= 25
    # a region that is too small: the entries beyond it are counted, not written
    small = np.minimum(cap, 5)
    recs5, count5 = select(0, T, bin_min, small, 0)
    assert np.array_equal(count5, cap) and all(len(r) == 5 for r in recs5)
    for t in range(T):
        keys = set(zip(recs[t]["sender"].tolist(), recs[t]["receiver"].tolist()))
        assert set(zip(recs5[t]["sender"].tolist(), recs5[t]["receiver"].tolist())) <= keys


# ---------------------------------------------------------------------------
# 5. end to end
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e():
    import torch
    from ame_amd import TemporalAMEStructuredMFVI
    n, T, r, rho = 40, 4, 2, 0.5
    c = BR.make_binary_case(n, T, r, rho, seed=31, lr=0.5)
    mask = MR.random_mask(n, T, 0.2, seed=2)
    m = c["model"]
    m.set_binary(torch.from_numpy(c["B"]), rho=rho)
    m.set_missing(torch.from_numpy(mask))
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.5, device=torch.device("cuda", 0))
    vi.fit(max_iter=30, tolerance=0.0, verbose=False)
    return c, mask, vi


def test_end_to_end_held_out_roc(gpu_device):
    from ame_amd import links
    c, mask, vi = _e2e()
    n, T, r = 40, 4, 2
    X0 = vi.X_mean.clone()
    roc = vi.link_roc(subset="held_out")
    bins = 1024
    # t on the host from predict_dyads' moments of the mean (the same fp32 products): each side is
    # within links_ref's delta of the fp64 value of the state, so the two are within 2 delta
    mean, second = vi.predict_dyads(slice(0, T), include_noise=False)
    mean, second = mean.numpy().astype(np.float64), second.numpy().astype(np.float64)
    X, S = vi.X_mean.numpy(), vi.X_cov.numpy()
    full = LR.scores(X, S, r, c["B"], with_delta=True)
    tight = 0
    for t in range(T):
        d = LR.subset(full[t], mask[:, :, t], HID)
        i, j = d["i"], d["j"]
        host = np.stack([mean[i, j, t, 0] / np.sqrt(1.0 + second[i, j, t, 0]),
                         mean[i, j, t, 1] / np.sqrt(1.0 + second[i, j, t, 1])], -1)
        assert (np.abs(host - d["t"]) <= d["delta"]).all(), t
        dh = dict(d, t=host, delta=2.0 * d["delta"])
        assert LR.near_edge_share(dh, bins) <= 0.01, t
        ok, detail = LR.sandwich(roc["hist"][t], dh, bins)
        assert ok, (t, detail)
        tight += int(np.array_equal(LR.histograms([dict(d, t=host)], bins)[0], roc["hist"][t]))
    print(f"slices whose histogram equals the one of the host's t exactly: {tight} of {T}")
    again = links.roc(roc["hist"], bins, 8.0)
    assert sorted(again) == sorted(roc)
    for k, v in again.items():
        if k == "pooled":
            assert sorted(v) == sorted(roc[k])
            for kk, vv in v.items():
                assert np.array_equal(np.asarray(roc[k][kk]), np.asarray(vv), equal_nan=True), kk
        else:
            assert np.array_equal(roc[k], v, equal_nan=True), k
    assert (roc["auc_lo"] <= roc["auc"]).all() and (roc["auc"] <= roc["auc_hi"]).all()
    assert roc["pooled"]["auc_lo"] <= roc["pooled"]["auc"] <= roc["pooled"]["auc_hi"]
    assert np.array_equal(roc["pairs"], vi.predictive_check(subset="held_out")["pairs"])
    assert np.array_equal(roc["pairs"], MR.pack(mask)[1])
    top = vi.top_links(k=20, subset="held_out", ties=0)
    assert (top["tie"] == 0).all() and (np.diff(top["score"], axis=1) <= 0).all()
    import torch
    assert torch.equal(vi.X_mean, X0)
    print(f"held-out AUC per step {roc['auc'].tolist()} (bracket {(roc['auc_hi'] - roc['auc_lo']).max():.1e}), "
          f"pooled {roc['pooled']['auc']:.4f}, average precision {roc['average_precision'].tolist()}, "
          f"base rate {(roc['positives'] / (2 * roc['pairs'])).tolist()}")


# ---------------------------------------------------------------------------
# 6. forecast_links
# ---------------------------------------------------------------------------
def test_forecast_links(gpu_device):
    case = (33, 3, 2)
    n, T, r = case
    X, S, B, mask, full, vi = _random(case, False)
    h = 2
    Bf = np.random.default_rng(77).random((n, n, h)) < 0.3
    Bf[np.arange(n), np.arange(n)] = True          # self ties are ignored, as set_binary ignores them
    fl = vi.forecast_links(Bf, k=15)
    Xp, Sp = vi.forecast(h)
    Bc = Bf.copy()
    Bc[np.arange(n), np.arange(n)] = False
    sc = LR.scores(Xp.numpy(), Sp.numpy(), r, Bc, with_delta=True)
    assert fl["hist"].shape == (h, 2, 1024) and np.array_equal(fl["pairs"], [n * (n - 1) // 2] * h)
    for d in sc:
        assert LR.near_edge_share(d, 1024) <= 0.01
    _assert_sandwich(fl["hist"], sc, 1024, "forecast_links")
    _assert_top_within_bounds(fl, sc, Bc, 15, None, "forecast_links top")
    plain = vi.forecast_links(Bf.astype(np.uint8), bins=64)
    assert "sender" not in plain and plain["hist"].shape == (h, 2, 64)
    _assert_sandwich(plain["hist"], sc, 64, "forecast_links 64")
    for bad in (Bf[:, :5], Bf.astype(np.float32), Bf[:, :, 0]):
        with pytest.raises(ValueError):
            vi.forecast_links(bad)


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals(gpu_device):
    import torch
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI
    n, T, r = 12, 3, 2
    dev = torch.device("cuda", 0)
    B = torch.from_numpy(np.random.default_rng(0).random((n, n, T)) < 0.4)
    g = TemporalAMEModel(n, T, r, seed=3)
    g.generate_data_fast(seed=4)
    vg = TemporalAMEStructuredMFVI(g, factorization="good", learning_rate=0.5, device=dev)
    for call in (lambda: vg.link_roc(), lambda: vg.top_links(k=3), lambda: vg.forecast_links(B[:, :, :1])):
        with pytest.raises(ValueError, match="binary"):
            call()
    m = TemporalAMEModel(n, T, r, seed=3)
    m.generate_data_fast(seed=4)
    m.set_binary(B, rho=0.2)
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.5, device=dev)
    vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    x = vi.X_mean.clone()
    for call in (lambda: vi.link_roc(subset="held_out"), lambda: vi.top_links(k=3, subset="observed"),
                 lambda: vi.top_links(k=0), lambda: vi.top_links(k=-2), lambda: vi.top_links(k=2.5),
                 lambda: vi.top_links(k=3, ties=2), lambda: vi.link_roc(bins=0), lambda: vi.link_roc(bins=2049),
                 lambda: vi.top_links(k=3, bins=4096), lambda: vi.forecast_links(B[:, :, :1], bins=-1),
                 lambda: vi.forecast_links(B[:, :, :1], k=-1), lambda: vi.link_roc(t_max=0.0)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="t_max.*bins|bins.*t_max"):     # one bin: every entry is a candidate
        vi.top_links(k=1, bins=1, max_records=10)
    assert vi.top_links(k=1, bins=1)["score"].shape == (T, 1)
    assert torch.equal(vi.X_mean, x)               # the refusals left the fit alone
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    assert np.isfinite(float(vi.history["elbo"][-1]))
    sharded = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.5, distributed=True)
    for call in (lambda: sharded.link_roc(), lambda: sharded.top_links(k=3),
                 lambda: sharded.forecast_links(B[:, :, :1])):
        with pytest.raises(NotImplementedError, match="time-sharded"):
            call()
        assert sharded._engine is None
