"""ame_smooth and the calls built on it (vi.smooth, smoothed=True) on the GPU,
against the fp64 reference tests/smooth_ref.py (dense inverse of each node's
joint precision).

Tolerance (derived, not fitted).  The kernels compute in fp64 from the same
fp32 inputs as the reference; what remains is the single fp32 rounding of the
output plus the fp64 solve error:

    |out - ref| <= 2^-24 |ref| + 8 (T d) 2^-52 cond_2(Lambda_i) scale_i

scale_i the largest |entry| of node i's output array, cond_2 from the
reference's dense Lambda_i.  lag_sum (fp64, never rounded to fp32) is held to
n 2^-52 sum_i |X_it| plus the solve term summed over the nodes.
"""
import ctypes
import functools

import numpy as np
import pytest

import em_case
import mstep_ref as M
import smooth_ref as SR

pytestmark = pytest.mark.gpu

IDS = lambda s: "n%d_T%d_r%d" % s
KEYS = ("mean", "cov", "cross", "lag_sum")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _vi_of(case, lr=0.5):
    """A structured VI on the case's model whose means are the case's."""
    import torch
    from ame_amd import TemporalAMEStructuredMFVI
    vi = TemporalAMEStructuredMFVI(case["model"], factorization="good", learning_rate=lr,
                                   device=torch.device("cuda", 0))
    vi.X_mean = torch.from_numpy(case["X"].copy())
    return vi


def _arrays(sm):
    return {k: getattr(sm, k).numpy() for k in KEYS}


@functools.lru_cache(maxsize=None)
def _run(shape, pset):
    case = SR.make_case(shape, pset)
    vi = _vi_of(case)
    return case, vi, _arrays(vi.smooth())


@pytest.mark.parametrize("pset", SR.PSETS)
@pytest.mark.parametrize("shape", SR.SHAPES, ids=IDS)
def test_parity_with_dense_reference(shape, pset, gpu_device):
    case, vi, got = _run(shape, pset)
    n, T, r = shape
    d = 2 + 2 * r
    ref = case["ref"]
    tol = SR.tolerance(ref, T, d)
    for k in KEYS:
        assert got[k].shape == ref[k].shape, k
        assert np.isfinite(got[k]).all(), k
        err = np.abs(got[k].astype(np.float64) - ref[k])
        frac = float((err / np.where(tol[k] > 0, tol[k], 1.0)).max())
        print(f"{IDS(shape)} {pset} {k}: max err / bound = {frac:.3f}")
        assert (err <= tol[k]).all(), (k, frac)
    assert got["lag_sum"].dtype == np.float64
    assert (got["cross"][:, 0] == 0).all() and (got["lag_sum"][0] == 0).all()
    if T > 1:
        assert np.abs(got["cross"][:, 1:]).min() > 0


@pytest.mark.parametrize("shape", SR.EVERY_R_SHAPES, ids=IDS)
def test_parity_at_every_latent_dim(shape, gpu_device):
    """d is a runtime value in the kernels; every r from 1 to 32 at (5, 3, r)."""
    test_parity_with_dense_reference(shape, "gen", gpu_device)


@pytest.mark.parametrize("shape", [(33, 5, 16), (130, 3, 23), (65, 4, 5)], ids=IDS)
def test_bit_identity_across_chunking_and_runs(shape, gpu_device):
    """A scratch budget that forces 32-node chunks and one that allows a single
    launch give the same bits; so does a second run."""
    case, vi, got = _run(shape, "gen")
    eng = vi.engine
    assert eng.smooth_chunk() == shape[0]
    again = _arrays(vi.smooth())
    budget = eng.PREDICT_WORK_DOUBLES
    try:
        eng.PREDICT_WORK_DOUBLES = 1
        assert eng.smooth_chunk() == 32
        small = _arrays(vi.smooth())
    finally:
        eng.PREDICT_WORK_DOUBLES = budget
    for k in KEYS:
        assert np.array_equal(again[k], got[k]), k
        assert np.array_equal(small[k], got[k]), k


def test_no_side_effects(gpu_device):
    """After smooth(): X_mean, X_cov, the next sweep's means and
    m_step_statistics() equal those of a twin that never smoothed."""
    import torch

    def run(smooth):
        case = SR.make_case((65, 4, 5), "gen")
        vi = _vi_of(case)
        vi.fit(max_iter=2, tolerance=0.0, verbose=False)
        if smooth:
            vi.smooth()
            vi.m_step_statistics(smoothed=True)
        out = [vi.X_mean.clone(), vi.X_cov.clone()]
        st = vi.m_step_statistics()
        vi.fit(max_iter=1, tolerance=0.0, verbose=False)
        return out + [vi.X_mean.clone()] + [st[k] for k in ("A0", "A11", "A00", "A10", "Rss")]

    for a, b in zip(run(True), run(False)):
        assert torch.equal(a, b)


def test_side_calls_share_one_scratch(gpu_device):
    """predictive_check, m_step_statistics(smoothed=True), smooth and
    predictive_check again on ONE fitted object (n=48, T=6, r=3): the calls
    share the engine's one grow-only scratch buffer, and every result has the
    bits of the same call made first on a fresh twin."""
    def fitted():
        vi = _vi_of(SR.make_case((48, 6, 3), "gen"))
        vi.fit(max_iter=2, tolerance=0.0, verbose=False)
        return vi

    calls = (("predictive_check", lambda v: v.predictive_check()),
             ("m_step_statistics", lambda v: v.m_step_statistics(smoothed=True)),
             ("smooth", lambda v: _arrays(v.smooth())),
             ("predictive_check again", lambda v: v.predictive_check()))
    vi = fitted()
    for name, call in calls:
        got, want = call(vi), call(fitted())
        assert set(got) == set(want) and len(got) >= 4, name
        for k in want:
            a, b = np.asarray(got[k]), np.asarray(want[k])
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, k)


def test_smoothed_interfaces(gpu_device):
    import torch
    import predictive_ref as PR
    case, vi, got = _run((33, 5, 16), "gen")
    n, T, r = case["shape"]
    eng = vi.engine
    sm = vi.smooth()
    # predictive_check(smoothed=True) is engine.predict on the smoothed state
    levels, zsq, csq = vi._thresholds((0.5, 0.9))
    sums, _ = eng.predict(sm.d_mean, sm.d_cov, Yt=eng.Yt, zsq=zsq, csq=csq)
    want = vi._check_dict(sums, levels)
    chk = vi.predictive_check(levels=(0.5, 0.9), smoothed=True)
    for k in ("pairs", "log_score", "mahalanobis", "z2", "mean_var", "sq_err", "coverage"):
        assert np.array_equal(chk[k], want[k]), k
    plain = vi.predictive_check(levels=(0.5, 0.9))
    assert not np.array_equal(plain["log_score"], chk["log_score"])
    # forecast(2, smoothed=True): the fp64 recursion from the reference's last slice
    Phi = case["C"].Phi.numpy()
    Q = case["C"].Q.numpy()
    m = case["ref"]["mean"][:, -1]
    S = case["ref"]["cov"][:, -1]
    Xp, Sp = vi.forecast(2, smoothed=True)
    for h in range(2):
        m = m @ Phi.T
        S = Phi @ S @ Phi.T + Q
        # the bounds of test_gpu_predictive.test_forecast_matches_recursion
        assert np.abs(Xp[:, h].numpy() - m).max() <= 2e-6 * max(1.0, np.abs(m).max())
        assert np.abs(Sp[:, h].numpy() - S).max() <= 1e-6 * max(1.0, np.abs(S).max())
    # A10 = the mean part + lag_sum[1:] added in time order
    st = vi.m_step_statistics(smoothed=True)
    state, _ = eng.mstep_stats(sm.d_mean, sm.d_cov)
    state = state.cpu()
    lag = sm.lag_sum
    A10 = torch.zeros_like(state[0, 1])
    for t in range(1, T):
        A10 += state[t, 1]
    for t in range(1, T):
        A10 += lag[t]
    assert torch.equal(st["A10"], A10)
    assert not torch.equal(st["A10"], vi.m_step_statistics()["A10"])
    ref = M.state_rows(case["ref"]["mean"], case["ref"]["cov"])[0]
    assert np.abs(st["A0"].numpy() - ref[0, 0]).max() <= 1e-5 * np.abs(ref[0, 0]).max()


def test_fit_em_smoothed_end_to_end(gpu_device):
    """The experiment of em_case with smoothed=True against the fp64 CPU EM that
    uses smooth_ref; allowance after round 1: 4 x the deviation of the same CPU
    EM on fp32 state arrays from the fp64 run (measured on the CPU)."""
    import torch
    from ame_amd import TemporalAMEStructuredMFVI
    from test_smooth_ref import em_runs
    m = em_case.make_model()
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=M.EM_LR,
                                   device=torch.device("cuda", 0))
    h = vi.fit_em(M.EM_ROUNDS, M.EM_SWEEPS, update=M.EM_UPDATE, tolerance=0.0, verbose=False,
                  smoothed=True)
    em = h["em"]
    assert len(em) == M.EM_ROUNDS
    for rd in em:
        assert rd["objective_after"] >= rd["objective_before"] - 2.0 ** -40 * rd["objective_scale"]
    cpu = em_runs()
    own = em_case.relative_deviation(cpu["sm64"][0], cpu["sm32"][0])
    got = em_case.relative_deviation(cpu["sm64"][0], {k: em[0][k].numpy() for k in ("Phi", "Q", "R")})
    print(f"round 1: GPU vs fp64 CPU EM {got:.3e}; CPU EM fp32 vs fp64 {own:.3e}; allowance {4 * own:.3e}")
    assert got <= 4.0 * own, (got, own)


def test_failed_pivot_is_reported_not_faulted(gpu_device):
    """C ABI at (4, 2, 1) with S0inv = -I: every node reports a failed pivot, the
    outputs are NaN, the call returns normally; the Python layer raises.  The
    model has a wide process noise and a wide R, so that P_obs + PtQiP < 1 on
    the diagonal and D_0 = P_obs - I + PtQiP has a negative first pivot."""
    import torch
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI, _lib as L
    lib = L.lib()
    n, T, r, d = 4, 2, 1, 4
    m = TemporalAMEModel(n, T, r, process_noise_scale=100.0, seed=5)
    m.generate_data_fast(seed=9)
    m.R = (1000.0 * m.R).clone()
    m.R_inv = torch.linalg.inv(m.R)
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.5,
                                   device=torch.device("cuda", 0))
    eng = vi.engine
    dev = eng.dev
    consts = eng.consts.clone()
    consts[0] = -torch.eye(d, dtype=torch.float64, device=dev)
    dims = L.ame_dims(n, r, T, 0, T, L.AME_GOOD)
    ws = int(lib.ame_smooth_work_size(ctypes.byref(dims), n))
    work = torch.empty(ws, dtype=torch.float64, device=dev)
    mean = torch.zeros(T, n, d, device=dev)
    cov = torch.zeros(T, n, d, d, device=dev)
    cross = torch.zeros(T, n, d, d, device=dev)
    lag = torch.zeros(T, d, d, dtype=torch.float64, device=dev)
    fail = torch.zeros(L.AME_SMOOTH_FAIL_WORDS, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    a = L.ame_smooth_args(x=_ptr(eng.x_a), Yt=_ptr(eng.Yt), consts=_ptr(consts), rinv=eng.C.rinv4(),
                          i0=0, i1=n, stages=0, mean=_ptr(mean), cov=_ptr(cov), cross=_ptr(cross),
                          lag_sum=_ptr(lag), fail=_ptr(fail), work=_ptr(work), work_doubles=ws)
    assert lib.ame_smooth(ctypes.byref(dims), ctypes.byref(a), None) == 0
    torch.cuda.synchronize()
    words = fail.cpu().tolist()
    assert words[0] == n and words[1] == 1 and 0 <= words[2] < n and words[3] == 0
    assert torch.isnan(mean).all() and torch.isnan(cov).all() and torch.isnan(cross).all()
    assert torch.isnan(lag[1:]).all()
    eng.consts.copy_(consts)
    with pytest.raises(RuntimeError, match="non-positive pivot"):
        vi.smooth()


def test_capi_argument_errors(gpu_device):
    import torch
    from test_smooth_capi import check_argument_errors
    check_argument_errors()
    torch.cuda.synchronize()   # nothing was queued that could fault
