"""CPU checks of the smoothing reference tests/smooth_ref.py and of the inputs
the GPU tests (tests/test_gpu_smooth.py) run: the two routes agree, the
smoothed marginals dominate the mean-field blocks, every listed kernel mistake
is visible on every GPU input, the M-step's closed forms stay stationary with
the lag-one term in A10, and the figures DESIGN.md §7e / §7d quote."""
import functools

import numpy as np
import pytest

import em_case
import mstep_ref as M
import smooth_ref as SR

IDS = lambda s: "n%d_T%d_r%d" % s
CASES = [(s, p) for s in SR.SHAPES for p in SR.PSETS] + [(s, "gen") for s in SR.EVERY_R_SHAPES]
CASE_IDS = [f"{IDS(s)}-{p}" for s, p in CASES]

# the output a mistake is named after (the one it must move)
NAMED = {"drop_O": "cross", "no_exclusion_P": "cov", "no_exclusion_h": "mean", "Qinv_at_0": "mean",
         "PtQiP_at_end": "mean", "transpose_O": "cross", "transpose_cross": "cross"}
NEEDS_T2 = ("drop_O", "PtQiP_at_end", "transpose_O", "transpose_cross")
# Q^-1 Phi is symmetric at the default parameters (Phi = 0.8 I): transposing O
# changes nothing there, which is why the `gen` set (dense non-symmetric Phi) runs too
NEEDS_GEN = ("transpose_O",)


@functools.lru_cache(maxsize=None)
def _routes(shape, pset):
    c = SR.make_case(shape, pset)
    rec = SR.smooth(c["Y"], c["X"], c["R_inv"], c["consts"], route="recursion")
    err = {k: float(np.abs(rec[k] - c["ref"][k]).max()) for k in ("mean", "cov", "cross", "lag_sum")}
    return c, rec, err


@pytest.mark.parametrize("shape,pset", CASES, ids=CASE_IDS)
def test_recursion_matches_dense_inverse(shape, pset):
    """Both routes are fp64; they differ by their solve errors, each within the
    solve term of the GPU bound, 8 (T d) 2^-52 cond_2 scale."""
    c, rec, err = _routes(shape, pset)
    n, T, r = shape
    d = 2 + 2 * r
    ref = c["ref"]
    for k in ("mean", "cov", "cross"):
        scale = np.abs(ref[k].reshape(n, -1)).max(1)
        bound = 2 * 8.0 * T * d * 2.0 ** -52 * ref["cond"] * scale
        e = np.abs(rec[k] - ref[k]).reshape(n, -1).max(1)
        assert (e <= bound).all(), (k, float((e / np.where(bound > 0, bound, 1)).max()))
    assert (ref["cross"][:, 0] == 0).all()


@pytest.mark.parametrize("shape,pset", CASES, ids=CASE_IDS)
def test_marginals_dominate_mean_field_blocks(shape, pset):
    """S_tt - D_t^-1 is positive semidefinite; the threshold is the measured
    recursion-vs-dense error of the covariances (times d: an eigenvalue moves by
    at most the 2-norm of the perturbation)."""
    c, rec, err = _routes(shape, pset)
    n, T, r = shape
    d = 2 + 2 * r
    thr = d * max(err["cov"], np.finfo(np.float64).tiny)
    for i in range(min(n, 6)):
        D, Ob, h = SR.blocks(c["Y"], c["X"], c["R_inv"], c["consts"], i)
        for t in range(T):
            gap = c["ref"]["cov"][i, t] - np.linalg.inv(D[t])
            ev = np.linalg.eigvalsh(0.5 * (gap + gap.T))
            assert ev.min() >= -thr - 2.0 ** -52 * d * np.abs(c["ref"]["cov"][i, t]).max(), (i, t, ev.min())


def test_single_slice_is_the_block_inverse():
    c = SR.make_case((9, 1, 1), "gen")
    for i in range(9):
        D, Ob, h = SR.blocks(c["Y"], c["X"], c["R_inv"], c["consts"], i)
        assert np.allclose(c["ref"]["cov"][i, 0], np.linalg.inv(D[0]), rtol=1e-13, atol=0)
        assert np.allclose(c["ref"]["mean"][i, 0], np.linalg.solve(D[0], h[0]), rtol=1e-12, atol=0)
    assert (c["ref"]["cross"] == 0).all() and (c["ref"]["lag_sum"] == 0).all()


@pytest.mark.parametrize("shape,pset", CASES, ids=CASE_IDS)
def test_inputs_tell_kernel_mistakes_apart(shape, pset):
    """Each mistake moves at least half the entries of its named output by more
    than 100 x the GPU tolerance (first 6 nodes)."""
    c, _, _ = _routes(shape, pset)
    n, T, r = shape
    d = 2 + 2 * r
    tol = SR.tolerance(c["ref"], T, d)
    nodes = list(range(min(n, 6)))
    for mut in SR.MUTATIONS:
        if (T == 1 and mut in NEEDS_T2) or (pset == "default" and mut in NEEDS_GEN):
            continue
        k = NAMED[mut]
        got = SR.smooth(c["Y"], c["X"], c["R_inv"], c["consts"], mutation=mut, nodes=nodes)
        moved = np.abs(got[k] - c["ref"][k][nodes]) > 100 * tol[k][nodes]
        if k == "cross":
            moved = moved[:, 1:]
        frac = float(moved.mean())
        assert frac >= 0.5, (mut, k, frac)
    Phi = c["C"].Phi.numpy()
    if pset == "gen":
        assert np.abs(Phi - Phi.T).max() > 0.01 and np.abs(Phi - Phi[0, 0] * np.eye(d)).max() > 0.01


# ---- the em_case experiment ----
@functools.lru_cache(maxsize=None)
def em_state():
    """em_case's model, its start parameters and the fp64 state after 5 sweeps."""
    import ame_oracle as O
    from ame_amd import TemporalAMEStructuredMFVI
    m = em_case.make_model()
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=M.EM_LR)
    X0 = vi.X_mean.numpy().astype(np.float64)
    S0 = vi.X_cov.numpy().astype(np.float64)
    Y = m.Y.numpy().astype(np.float64)
    p = em_case.start_params(m)
    X, S = X0.copy(), S0.copy()
    q = dict(p, R_inv=np.linalg.inv(p["R"]))
    for _ in range(M.EM_SWEEPS):
        O.sweep_stats(Y, X, S, q, "good", M.EM_LR)
    return dict(Y=Y, X0=X0, S0=S0, p=p, X=X, S=S, r=m.r)


@functools.lru_cache(maxsize=None)
def em_runs():
    """The fp64 EM with smoothed statistics, and the same on fp32 state arrays."""
    e = em_state()
    return dict(sm64=SR.oracle_em_smoothed(e["Y"], e["X0"], e["S0"], e["p"]),
                sm32=SR.oracle_em_smoothed(e["Y"], e["X0"], e["S0"], e["p"], dtype=np.float32))


def test_smoothed_posterior_of_the_em_state():
    """The figures of DESIGN.md §7e at n = 40, T = 16, r = 2 after 5 sweeps."""
    e = em_state()
    n, T, d = e["X"].shape
    st, sm = SR.smoothed_statistics(e["Y"], e["X"], e["r"], e["p"])
    p = e["p"]
    Qinv = np.linalg.inv(p["Q"])
    consts = dict(S0inv=np.linalg.inv(M.blockdiag(p["Sigma"], p["Psi"])), Qinv=Qinv,
                  PtQiP=p["Phi"].T @ Qinv @ p["Phi"], QiPhi=Qinv @ p["Phi"])
    D, Ob, h = SR.blocks(e["Y"], e["X"], np.linalg.inv(p["R"]), consts, 3)
    mf = np.stack([np.linalg.inv(D[t]) for t in range(T)])
    ratio = np.trace(sm["cov"][3], axis1=1, axis2=2).sum() / np.trace(mf, axis1=1, axis2=2).sum()
    gap_min = min(np.linalg.eigvalsh(sm["cov"][3, t] - mf[t]).min() for t in range(T))
    lag_rel = np.abs(sm["cross"][3]).max() / np.abs(sm["cov"][3]).max()
    rec = SR.recursion(D, Ob, h)
    rec_err = max(np.abs(rec[1] - sm["cov"][3]).max(), np.abs(rec[2] - sm["cross"][3]).max())
    print(f"trace ratio {ratio:.4f}; min eig of S_tt - D_t^-1 {gap_min:.3e}; lag-one / marginal "
          f"{lag_rel:.4f}; recursion vs dense {rec_err:.3e}; cond {sm['cond'][3]:.1f}")
    assert 1.2 <= ratio <= 1.4
    assert gap_min > 0
    assert 0.3 <= lag_rel <= 0.5
    assert rec_err <= 1e-13
    assert sm["cond"][3] <= 100


def test_closed_forms_stay_stationary_with_cross_in_A10():
    """F is linear in the statistics: with the lag-one term in A10 the closed
    forms of mstep_ref.m_step still maximise it (no perturbed parameter set does
    better, and the gradient in Phi vanishes)."""
    e = em_state()
    n, T, d = e["X"].shape
    st, sm = SR.smoothed_statistics(e["Y"], e["X"], e["r"], e["p"])
    plain = M.statistics(e["X"], e["S"], e["r"], e["Y"])
    assert np.abs(st["A10"] - plain["A10"]).max() > 1e-3 * np.abs(plain["A10"]).max()
    new = M.m_step(st, e["p"], n, T)
    f0 = M.objective(st, new, n, T)
    assert f0 >= M.objective(st, e["p"], n, T)
    rng = np.random.default_rng(0)
    slack = 2.0 ** -40 * M.objective_magnitude(st, new, n, T)
    for k in ("Phi", "Q", "R"):
        for _ in range(4):
            E = rng.standard_normal(new[k].shape)
            if k != "Phi":
                E = 0.5 * (E + E.T)
            for eps in (1e-3, -1e-3):
                assert M.objective(st, dict(new, **{k: new[k] + eps * E}), n, T) <= f0 + slack, k
    # dF/dPhi = Q^-1 (A10 - Phi A00) = 0 at Phi = A10 A00^-1
    G = np.linalg.inv(new["Q"]) @ (st["A10"] - new["Phi"] @ st["A00"])
    assert np.abs(G).max() <= 1e-9 * np.abs(np.linalg.inv(new["Q"]) @ st["A10"]).max()


def test_em_with_and_without_smoothing():
    """What smoothing does to the EM of em_case (6 rounds of 5 sweeps): R stays
    where the mean-field EM leaves it (so its bias does not come from the time
    factorisation) and Q's U-block diagonal moves only part of the way to the
    truth.  These are the figures README.md and DESIGN.md §7d quote."""
    plain = em_case.cpu_runs()["em64"][-1]
    sm = em_runs()["sm64"][-1]
    r00 = (plain["R"][0, 0], sm["R"][0, 0])
    qu = (plain["Q"][2, 2], sm["Q"][2, 2])
    print(f"R00 mean-field {r00[0]:.5f} smoothed {r00[1]:.5f} (truth {M.TRUE_R[0]}); "
          f"Q[U0,U0] mean-field {qu[0]:.4f} smoothed {qu[1]:.4f} (truth 0.036)")
    assert abs(r00[0] - 0.1199) <= 5e-4 and abs(r00[1] - 0.1200) <= 5e-4
    assert abs(r00[1] - r00[0]) <= 1e-3            # smoothing does not move R
    assert abs(qu[0] - 0.0830) <= 1e-3 and abs(qu[1] - 0.0762) <= 1e-3
    assert 0.036 < qu[1] < qu[0]
    own = em_case.relative_deviation(em_runs()["sm64"][0], em_runs()["sm32"][0])
    print(f"round 1: smoothed CPU EM fp32 vs fp64 {own:.3e} (GPU allowance {4 * own:.3e})")
    assert 0 < own < 1e-3


def test_time_sharded_smooth_is_refused_before_any_launch():
    """smooth() and smoothed=True raise NotImplementedError on a time-sharded
    instance before the engine (and so any launch or collective) exists."""
    import torch
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI
    m = TemporalAMEModel(6, 3, 1, seed=1)
    m.generate_data_fast(seed=2)
    vi = TemporalAMEStructuredMFVI(m, distributed=True)
    calls = [lambda: vi.smooth(), lambda: vi.predictive_check(smoothed=True),
             lambda: vi.predict_dyads(0, smoothed=True), lambda: vi.forecast(1, smoothed=True),
             lambda: vi.forecast_check(torch.zeros(6, 6, 1, 2), smoothed=True),
             lambda: vi.forecast_dyads(1, smoothed=True), lambda: vi.m_step_statistics(smoothed=True),
             lambda: vi.m_step(smoothed=True), lambda: vi.fit_em(1, 1, verbose=False, smoothed=True)]
    for call in calls:
        with pytest.raises(NotImplementedError):
            call()
        assert vi._engine is None


def test_combine_adds_cross_in_time_order():
    import torch
    from ame_amd import mstep
    g = torch.Generator().manual_seed(0)
    state = torch.randn(5, 2, 4, 4, generator=g, dtype=torch.float64)
    dyad = torch.rand(5, 4, generator=g, dtype=torch.float64)
    cross = torch.randn(5, 4, 4, generator=g, dtype=torch.float64)
    a, b = mstep.combine(state, dyad), mstep.combine(state, dyad, cross=cross)
    want = a["A10"].clone()
    for t in range(1, 5):
        want += cross[t]
    assert torch.equal(b["A10"], want)
    for k in ("A0", "A11", "A00", "Rss"):
        assert torch.equal(a[k], b[k])
    assert a["pairs"] == b["pairs"]
