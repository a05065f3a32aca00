"""ame_smooth over observed partners (`Mt` set) and the calls built on it
(vi.smooth(partners="observed"), smoothed="observed") on the GPU, against the
fp64 reference tests/smooth_masked_ref.py.

Tolerance (derived, not fitted): that of tests/test_gpu_smooth.py,

    |out - ref| <= 2^-24 |ref| + 8 (T d) 2^-52 cond_2(Lambda_i) scale_i,

plus (n + 2) 2^-52 ||S_i||_2 a_i scale_i for the three-way difference
(G - w_i w_i') - H that replaces the partner sum: each of its terms is a sum of
at most n products bounded entrywise by a_i = max_t || sum_{j != i} |J_j|'
|sym R_inv| |J_j| ||_2, and an error E in the precision moves the outputs by
S_i E S_i.  (smooth_masked_ref.tolerance.)
"""
import ctypes
import functools

import numpy as np
import pytest

import missing_ref as MR
import mstep_ref as M
import predictive_ref as PR
import smooth_masked_ref as SMR
import smooth_ref as SR

pytestmark = pytest.mark.gpu

IDS = lambda s: "n%d_T%d_r%d" % s
KEYS = SMR.KEYS
PSET = "gen"
LEVELS = (0.5, 0.9, 0.95)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _device(shape):
    """One VI (no mask: its Yt is the raw packed network) per shape, means = the case's."""
    import torch
    from ame_amd import TemporalAMEStructuredMFVI
    case = SR.make_case(shape, PSET)
    vi = TemporalAMEStructuredMFVI(case["model"], factorization="good", learning_rate=0.5,
                                   device=torch.device("cuda", 0))
    vi.X_mean = torch.from_numpy(case["X"].copy())
    eng = vi.engine
    eng.discard_speculation()
    torch.cuda.synchronize()
    return case, vi, eng


@functools.lru_cache(maxsize=None)
def _packed(shape, name):
    import torch
    case, vi, eng = _device(shape)
    n, T, r = shape
    Mt, _, _ = eng.pack_mask(torch.from_numpy(SMR.make_mask(name, n, T)))
    torch.cuda.synchronize()
    return Mt


def _call(shape, Mt, chunk=None):
    """ame_smooth through the C ABI over node chunks of `chunk` (all nodes by default):
    dict of (n, ...) numpy arrays."""
    import torch
    from ame_amd import _lib as L
    lib = L.lib()
    case, vi, eng = _device(shape)
    n, T, r = shape
    d = 2 + 2 * r
    dev = eng.dev
    chunk = n if chunk is None else chunk
    dims = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
    size = lib.ame_smooth_masked_work_size if Mt is not None else lib.ame_smooth_work_size
    ws = int(size(ctypes.byref(dims), min(chunk, n)))
    assert ws > 0
    work = torch.empty(ws, dtype=torch.float64, device=dev)
    mean = torch.zeros(T, n, d, device=dev)
    cov = torch.zeros(T, n, d, d, device=dev)
    cross = torch.zeros(T, n, d, d, device=dev)
    lag = torch.zeros(T, d, d, dtype=torch.float64, device=dev)
    fail = torch.zeros(L.AME_SMOOTH_FAIL_WORDS, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for i0 in range(0, n, chunk):
        a = L.ame_smooth_args(x=_ptr(eng.x_a), Yt=_ptr(eng.Yt), consts=_ptr(eng.consts), rinv=eng.C.rinv4(),
                              i0=i0, i1=min(n, i0 + chunk), stages=0, mean=_ptr(mean), cov=_ptr(cov),
                              cross=_ptr(cross), lag_sum=_ptr(lag), fail=_ptr(fail), work=_ptr(work),
                              work_doubles=ws, Mt=_ptr(Mt))
        rc = lib.ame_smooth(ctypes.byref(dims), ctypes.byref(a), None)
        assert rc == 0, lib.ame_last_error()
    torch.cuda.synchronize()
    assert fail.cpu().tolist()[0] == 0
    return dict(mean=mean.permute(1, 0, 2).cpu().numpy(), cov=cov.permute(1, 0, 2, 3).cpu().numpy(),
                cross=cross.permute(1, 0, 2, 3).cpu().numpy(), lag_sum=lag.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _unmasked(shape):
    return _call(shape, None)


def _assert_parity(shape, name):
    n, T, r = shape
    d = 2 + 2 * r
    ref = SMR.make_case(shape, PSET, name)["mref"]
    tol = SMR.tolerance(ref, n, T, d)
    got = _call(shape, _packed(shape, name))
    for k in KEYS:
        assert got[k].shape == ref[k].shape, k
        assert np.isfinite(got[k]).all(), k
        err = np.abs(got[k].astype(np.float64) - ref[k])
        frac = float((err / np.where(tol[k] > 0, tol[k], 1.0)).max())
        print(f"{IDS(shape)} {name} {k}: max err / bound = {frac:.3f}")
        assert (err <= tol[k]).all(), (k, frac)
    assert got["lag_sum"].dtype == np.float64
    assert (got["cross"][:, 0] == 0).all() and (got["lag_sum"][0] == 0).all()
    # hiding partners never narrows: against the Mt = NULL call on the same raw network
    tr_obs = np.trace(got["cov"].astype(np.float64), axis1=2, axis2=3)
    tr_all = np.trace(_unmasked(shape)["cov"].astype(np.float64), axis1=2, axis2=3)
    assert (tr_obs >= tr_all * (1.0 - 2.0 ** -20)).all(), float((tr_obs / tr_all).min())
    return got


@pytest.mark.parametrize("name", SMR.MASKS)
@pytest.mark.parametrize("shape", SMR.SHAPES, ids=IDS)
def test_parity_with_dense_reference(shape, name, gpu_device):
    got = _assert_parity(shape, name)
    if name == "all_of_one":    # the node with no observed partner in slice 1 keeps the prior blocks only
        n, T, r = shape
        tr_obs = np.trace(got["cov"][n // 2, 1].astype(np.float64))
        assert tr_obs > np.trace(_unmasked(shape)["cov"][n // 2, 1].astype(np.float64))


@pytest.mark.parametrize("shape", SMR.EVERY_R_SHAPES, ids=IDS)
def test_parity_at_every_latent_dim(shape, gpu_device):
    """Tile count and d are what changes with r: every r from 1 to 32 at (9, 2, r)."""
    _assert_parity(shape, SMR.EVERY_R_MASK)


BIT_SHAPES = ((65, 3, 8), (130, 2, 16), (70, 2, 17), (34, 2, 32))


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=IDS)
def test_all_false_mask_has_the_bits_of_the_unmasked_call(shape, gpu_device):
    got, plain = _call(shape, _packed(shape, "none")), _unmasked(shape)
    for k in KEYS:
        assert np.array_equal(got[k], plain[k]), k


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=IDS)
def test_bit_identity_across_chunking_and_runs(shape, gpu_device):
    Mt = _packed(shape, "random30")
    one, again, chunks = _call(shape, Mt), _call(shape, Mt), _call(shape, Mt, chunk=32)
    for k in KEYS:
        assert np.array_equal(again[k], one[k]), k
        assert np.array_equal(chunks[k], one[k]), k
    assert not np.array_equal(one["cov"], _unmasked(shape)["cov"])


def test_capi_argument_errors(gpu_device):
    import torch
    from test_smooth_masked_capi import check_argument_errors
    check_argument_errors()
    torch.cuda.synchronize()   # nothing was queued that could fault


# ---------------------------------------------------------------------------
# the VI layer
# ---------------------------------------------------------------------------
E2E = (33, 3, 2)
E2E_LR, E2E_ITERS = 0.5, 6


def _vi(model, lr=E2E_LR):
    import torch
    from ame_amd import TemporalAMEStructuredMFVI
    return TemporalAMEStructuredMFVI(model, factorization="good", learning_rate=lr,
                                     device=torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def _fitted():
    """A masked fit at (33, 3, 2), 30 % hidden, and the fp64 reference of its observed-partner
    smoothed state (from the fit's fp32 means)."""
    import torch
    n, T, r = E2E
    c = MR.make_case(n, T, r, seed=41, lr=E2E_LR)
    mask = MR.random_mask(n, T, 0.3, seed=5)
    m = c["model"]
    m.set_missing(torch.from_numpy(mask))
    vi = _vi(m)
    vi.fit(max_iter=E2E_ITERS, tolerance=0.0, verbose=False)
    X = vi.X_mean.numpy().astype(np.float64)
    p = c["params"]
    ref = SMR.smooth(c["Y"], X, p["R_inv"], SMR.consts_from(p), mask)
    return dict(c, mask=mask, vi=vi, ref=ref)


def test_smooth_observed_matches_reference(gpu_device):
    c = _fitted()
    vi, ref = c["vi"], c["ref"]
    n, T, r = E2E
    sm = vi.smooth(partners="observed")
    tol = SMR.tolerance(ref, n, T, 2 + 2 * r)
    for k in KEYS:
        err = np.abs(getattr(sm, k).numpy().astype(np.float64) - ref[k])
        assert (err <= tol[k]).all(), (k, float((err / tol[k]).max()))
    assert not np.array_equal(sm.cov.numpy(), vi.X_cov.numpy())


def test_every_entry_point_takes_observed_and_leaves_vi_unchanged(gpu_device):
    import torch
    c = _fitted()
    vi = c["vi"]
    n, T, r = E2E
    before = (vi.X_mean.clone(), vi.X_cov.clone(), vi.m_step_statistics())
    sm = vi.smooth(partners="observed")
    assert tuple(sm.mean.shape) == (n, T, 2 + 2 * r) and tuple(sm.lag_sum.shape) == (T, 2 + 2 * r, 2 + 2 * r)
    seen = vi.predictive_check(levels=LEVELS, smoothed="observed")
    assert np.array_equal(vi.predictive_check(levels=LEVELS, smoothed="observed", subset="observed")["log_score"],
                          seen["log_score"])
    held = vi.predictive_check(levels=LEVELS, smoothed="observed", subset="held_out")
    hid = MR.pack(c["mask"])[1].astype(np.float64)
    assert np.array_equal(held["pairs"], hid) and np.array_equal(seen["pairs"], n * (n - 1) // 2 - hid)
    assert not np.array_equal(held["log_score"], vi.predictive_check(levels=LEVELS, subset="held_out")["log_score"])
    mean, second = vi.predict_dyads(slice(0, T), rows=range(0, 8), cols=range(4, 12), smoothed="observed")
    assert tuple(mean.shape) == (8, 8, T, 2) and tuple(second.shape) == (8, 8, T, 3)
    plain_second = vi.predict_dyads(slice(0, T), rows=range(0, 8), cols=range(4, 12))[1]
    off = ~np.eye(n, dtype=bool)[0:8, 4:12]
    assert np.isfinite(second.numpy()[off]).all() and (second.numpy()[off][..., :2] > 0).all()
    assert not np.array_equal(second.numpy()[off], plain_second.numpy()[off])    # the smoothed state's, not the fit's
    Xp, Sp = vi.forecast(2, smoothed="observed")
    assert tuple(Xp.shape) == (n, 2, 2 + 2 * r) and torch.isfinite(Sp).all()
    # the smoothed last slice is where the forecast starts
    Phi = c["params"]["Phi"]
    assert np.abs(Xp[:, 0].numpy() - c["ref"]["mean"][:, -1] @ Phi.T).max() <= 2e-6 * max(
        1.0, np.abs(c["ref"]["mean"][:, -1]).max())
    Yf = torch.randn(n, n, 2, 2, generator=torch.Generator().manual_seed(3))
    fc = vi.forecast_check(Yf, levels=LEVELS, smoothed="observed")
    assert np.array_equal(fc["pairs"], np.full(2, n * (n - 1) // 2)) and np.isfinite(fc["log_score"]).all()
    fm, fs = vi.forecast_dyads(2, rows=range(0, 4), cols=range(0, 4), smoothed="observed")
    assert tuple(fm.shape) == (4, 4, 2, 2) and tuple(fs.shape) == (4, 4, 2, 3)
    st = vi.m_step_statistics(smoothed="observed")
    assert st["hidden_pairs"] == float(hid.sum())
    res = vi.m_step(update=("R",), apply=False, smoothed="observed")
    assert torch.isfinite(res["R"]).all()
    assert res["objective_after"] >= res["objective_before"] - 2.0 ** -40 * res["objective_scale"]
    after = (vi.X_mean.clone(), vi.X_cov.clone(), vi.m_step_statistics())
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    for k in ("A0", "A11", "A00", "A10", "Rss"):
        assert torch.equal(before[2][k], after[2][k]), k


def _assert_sums(check, want, per, levels):
    """The per-sum rules of test_gpu_predictive._assert_sums."""
    zsq, csq = PR.thresholds(levels)
    for t in range(len(per)):
        s, d = want[t], per[t]
        pairs = check["pairs"][t]
        assert pairs == s[0]
        got = {1: check["log_score"][t], 2: check["mahalanobis"][t], 3: check["z2"][t, 0],
               4: check["z2"][t, 1], 5: check["mean_var"][t, 0], 6: check["mean_var"][t, 1],
               7: check["sq_err"][t, 0], 8: check["sq_err"][t, 1]}
        for k in range(2, 9):
            rel = abs(got[k] - s[k]) / abs(s[k])
            print(f"t={t} slot {k}: rel err {rel:.3e}")
            assert rel <= 5e-6, (t, k, got[k], s[k])
        bound = 5e-6 * np.abs(d["logp"]).sum()
        assert abs(got[1] - s[1]) <= bound, (t, got[1], s[1])
        for l in range(len(levels)):
            for name, cnt, vals, thr in (
                    ("z0", check["coverage"][t, l, 0] * pairs, d["z2"][:, 0], zsq[l]),
                    ("z1", check["coverage"][t, l, 1] * pairs, d["z2"][:, 1], zsq[l]),
                    ("m2", check["joint_coverage"][t, l] * pairs, d["m2"], csq[l])):
                lo = (vals <= thr * (1.0 - 4.0 * PR.TOL)).sum()
                hi = (vals <= thr * (1.0 + 4.0 * PR.TOL)).sum()
                assert lo <= round(cnt) <= hi and abs(cnt - round(cnt)) < 1e-6, (t, l, name, cnt, lo, hi)


@pytest.mark.parametrize("subset,select", (("held_out", MR.HIDDEN), ("observed", MR.OBSERVED)))
def test_predictive_check_scores_the_reference_state(subset, select, gpu_device):
    c = _fitted()
    vi, ref = c["vi"], c["ref"]
    zsq, csq = PR.thresholds(LEVELS)
    want, per = MR.score_rows(ref["mean"], ref["cov"], E2E[2], c["Y"], c["params"]["R"], zsq, csq, c["mask"], select)
    chk = vi.predictive_check(levels=LEVELS, subset=subset, smoothed="observed")
    _assert_sums(chk, want, per, LEVELS)


def test_m_step_statistics_observed(gpu_device):
    c = _fitted()
    vi, ref = c["vi"], c["ref"]
    n, T, r = E2E
    want = MR.statistics(ref["mean"], ref["cov"], r, c["Y"], c["mask"])
    want["A10"] = want["A10"] + ref["lag_sum"][1:].sum(0)
    st = vi.m_step_statistics(smoothed="observed")
    assert st["pairs"] == want["pairs"] and st["hidden_pairs"] == want["hidden_pairs"]
    for k in ("A0", "A11", "A00", "A10", "Rss"):
        err = np.abs(st[k].numpy() - want[k]).max()
        print(f"{k}: max err / max|ref| = {err / np.abs(want[k]).max():.3e}")
        assert err <= 1e-5 * np.abs(want[k]).max(), k
    plain = vi.m_step_statistics()
    assert not np.array_equal(plain["A10"].numpy(), st["A10"].numpy())


def test_fit_em_observed_end_to_end(gpu_device):
    """One round, update R, M-step on the observed-partner smoothed statistics, against the fp64
    CPU round; allowance: 4 x the deviation of the same CPU round on fp32 state arrays."""
    import torch
    from test_smooth_masked_ref import E2E_SWEEPS, em_runs
    e = em_runs()
    m = e["case"]["model"]
    m.set_missing(torch.from_numpy(e["mask"]))
    vi = _vi(m)
    h = vi.fit_em(1, E2E_SWEEPS, update=("R",), tolerance=0.0, verbose=False, smoothed="observed")
    got = {"R": h["em"][0]["R"].numpy()}
    own = MR.relative_deviation(e["em64"], e["em32"], ("R",))
    dev = MR.relative_deviation(e["em64"], got, ("R",))
    print(f"R after round 1: GPU vs fp64 EM {dev:.3e}; fp32 vs fp64 EM {own:.3e}; allowance {4 * own:.3e}")
    assert dev <= 4.0 * own, (dev, own)
    assert torch.equal(m.R, h["em"][0]["R"].float())
    # the plain masked round learns another R
    assert not np.array_equal(got["R"], _plain_round_R(e))


def _plain_round_R(e):
    import torch
    from test_smooth_masked_ref import E2E_SWEEPS
    n, T, r = E2E
    c = MR.make_case(n, T, r, seed=43, lr=E2E_LR)
    c["model"].set_missing(torch.from_numpy(e["mask"]))
    h = _vi(c["model"]).fit_em(1, E2E_SWEEPS, update=("R",), tolerance=0.0, verbose=False)
    return h["em"][0]["R"].numpy()


def test_refusals_and_value_errors(gpu_device):
    import torch
    c = _fitted()
    vi = c["vi"]
    n, T, r = E2E
    # over all partners: refused as before, and the message names the option
    for call in (lambda: vi.smooth(), lambda: vi.predictive_check(smoothed=True),
                 lambda: vi.m_step_statistics(smoothed=True), lambda: vi.engine.smooth(),
                 lambda: vi.forecast(1, smoothed=True),
                 lambda: vi.fit_em(1, 1, update=("R",), verbose=False, smoothed=True)):
        with pytest.raises(NotImplementedError, match="smooth") as ei:
            call()
        assert "observed" in str(ei.value)
    with pytest.raises(ValueError):
        vi.smooth(partners="hidden")
    with pytest.raises(ValueError):
        vi.predictive_check(smoothed="hidden")
    # without a mask
    c0 = MR.make_case(n, T, r, seed=41, lr=E2E_LR)
    v0 = _vi(c0["model"])
    v0.fit(max_iter=1, tolerance=0.0, verbose=False)
    Yf = torch.zeros(n, n, 1, 2)
    for call in (lambda: v0.smooth(partners="observed"), lambda: v0.engine.smooth(observed=True),
                 lambda: v0.predictive_check(smoothed="observed"),
                 lambda: v0.predict_dyads(0, smoothed="observed"), lambda: v0.forecast(1, smoothed="observed"),
                 lambda: v0.forecast_check(Yf, smoothed="observed"),
                 lambda: v0.forecast_dyads(1, smoothed="observed"),
                 lambda: v0.m_step_statistics(smoothed="observed"),
                 lambda: v0.m_step(apply=False, smoothed="observed"),
                 lambda: v0.fit_em(1, 1, verbose=False, smoothed="observed")):
        with pytest.raises(ValueError, match="mask"):
            call()
    # the default call of an unmasked fit is today's
    assert torch.equal(v0.smooth().mean, v0.smooth(partners=None).mean)
