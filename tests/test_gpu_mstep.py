"""ame_mstep_stats and the EM calls built on it (m_step_statistics, m_step,
fit_em) on the GPU, against the fp64 reference tests/mstep_ref.py.

Bounds.
  State rows (P_t, C_t): every product and sum on the device is fp64 on the
  same fp32 inputs the reference reads, so the two differ by re-association
  only: |got - want| <= N 2^-52 sum|summand| per entry, N the number of
  summands (2n for P_t: n outer products and n covariances; n for C_t).  fp32
  products would miss this by eight orders of magnitude.
  Dyad sums: the five tile products are fp32 MFMA, as in ame_predict.  Rss00 and
  Rss11 (non-negative summands) are held to the 5e-6 relative bound
  test_gpu_predictive.py holds such sums to, Rss01 to 5e-6 x sum|summand| (its
  log-score rule); the pair count is exact.  Against ame_predict with zero
  noise on the same state (same products, same e), Rss00 = sums[5] + sums[7] and
  Rss11 = sums[6] + sums[8] up to re-association: N 2^-52 sum|summand| with
  N = 2 pairs.
  Parameter parity after EM round 1: the allowance is 4 x the deviation of the
  oracle EM run on fp32 state arrays from the fp64 run (em_case.relative_deviation:
  max over Phi, Q, R of max|difference| / max|parameter|), measured in the test.

Room under the bounds, measured on an MI355X over the cases added for every
compiled r (EVERY_R and (63, 3, 20)); for information, no bound comes from them.
Worst error / bound: state rows P 2.2e-2, C 2.3e-2 (of N 2^-52 sum|summand|);
Rss00 / Rss11 against the reference 1.7e-3 (8.5e-9 relative, of 5e-6); Rss01
1.2e-3 (of 5e-6 sum|summand|); Rss00 / Rss11 against ame_predict at zero noise
3.5e-4 (of 2 pairs 2^-52 x the sum).  tests/test_mstep_ref.py shows on the same
inputs that fp32 arithmetic alone stays under a tenth of the dyad bounds and
that a lost latent column moves every Rss entry by 26 x its bound or more.
"""
import ctypes
import functools

import numpy as np
import pytest

import em_case
import mstep_ref as M
import predictive_ref as PR

pytestmark = pytest.mark.gpu

# (63, 3, 20): a 31-node chunk (the one-node-ahead prefetch stops one short of a
# full chunk), a single tile of 63, the K = 10 state instance, a middle slice
# (70, 8, 3): 8 slices, so the single call takes the pair kernel's XCD-aware
# slice mapping and test_bit_identity's split calls (1..7 slices) the plain one;
# two tile rows, an edge tile 6 wide
SHAPES = ((5, 1, 1), (33, 3, 2), (64, 2, 3), (65, 4, 5), (130, 3, 16), (70, 2, 32), (200, 5, 8),
          (63, 3, 20), (70, 8, 3))
# every other compiled r at predictive_ref.GPU_SHAPES_EVERY_R's shape: two tile
# rows with a one-wide edge tile, chunks of 32, 32 and 1 nodes, one slice without
# a previous slice and one with.  ame_predict_pairs_kernel<R, 2> is one instance
# per r; ame_mstep_state_kernel<K> has K = 1, 2, 5, 10, 18 by ceil(d^2 / 256):
# r = 7 fills K = 1 exactly, 8 is the first r on K = 2, 11 on K = 5, 17 on K = 10
# (which serves r = 17..24), 25 on K = 18 (test_every_r_guard.py pins the map).
EVERY_R = tuple((65, 2, r) for r in range(1, 33) if r not in {s[2] for s in SHAPES})
IDS = lambda s: "n%d_T%d_r%d" % s
EPS = 2.0 ** -52


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Device:
    """make_state's random state and a generated network on the device, in the
    layouts of include/ame_amd.h, with raw C-ABI calls over slice ranges."""

    def __init__(self, shape):
        import torch
        from ame_amd import _lib
        self.L, self.lib = _lib, _lib.lib()
        n, T, r = self.shape = shape
        self.dev = torch.device("cuda", 0)
        self.X, self.S = PR.make_state(n, T, r)
        Y32 = M.gpu_network(n, T, r)
        self.Y = Y32.astype(np.float64)
        self.x = torch.from_numpy(self.X).permute(1, 0, 2).contiguous().to(self.dev)
        self.cov = torch.from_numpy(self.S).permute(1, 0, 2, 3).contiguous().to(self.dev)
        dims = self.dims(0, T)
        ysz = int(self.lib.ame_pack_y_size(ctypes.byref(dims)))
        self.ny = ysz // (2 * T * n)
        self.Yt = torch.zeros(T, n, self.ny, 2, dtype=torch.float32, device=self.dev)
        mm = torch.zeros(1, dtype=torch.int64, device=self.dev)
        Yd = torch.from_numpy(Y32).to(self.dev)
        _lib.check(self.lib.ame_pack_y(_ptr(Yd), _ptr(self.Yt), ctypes.byref(dims), _ptr(mm), None),
                   "ame_pack_y")
        torch.cuda.synchronize()

    def dims(self, t0, t1):
        n, T, r = self.shape
        return self.L.ame_dims(n, r, t1 - t0, t0, T, self.L.AME_GOOD)

    def stats(self, t0=None, t1=None, state=True, dyad=True):
        import torch
        n, T, r = self.shape
        t0, t1 = 0 if t0 is None else t0, T if t1 is None else t1
        d = 2 + 2 * r
        dims = self.dims(t0, t1)
        ws = int(self.lib.ame_mstep_work_size(ctypes.byref(dims)))
        assert ws > 0
        work = torch.empty(ws, dtype=torch.float64, device=self.dev)
        st = torch.full((t1 - t0, 2, d, d), float("nan"), dtype=torch.float64, device=self.dev)
        dy = torch.full((t1 - t0, 4), float("nan"), dtype=torch.float64, device=self.dev)
        a = self.L.ame_mstep_args(
            x=_ptr(self.x[t0:t1]), cov=_ptr(self.cov[t0:t1]),
            prev_final=_ptr(self.x[t0 - 1]) if t0 > 0 else None, Yt=_ptr(self.Yt[t0:t1]),
            state=_ptr(st) if state else None, dyad=_ptr(dy) if dyad else None, work=_ptr(work))
        self.L.check(self.lib.ame_mstep_stats(ctypes.byref(dims), ctypes.byref(a), None), "ame_mstep_stats")
        torch.cuda.synchronize()
        return st.cpu().numpy(), dy.cpu().numpy()

    def predict_sums(self):
        """ame_predict's per-slice scoring sums with zero noise and no levels."""
        import torch
        n, T, r = self.shape
        dims = self.dims(0, T)
        ws = int(self.lib.ame_predict_work_size(ctypes.byref(dims)))
        work = torch.empty(ws, dtype=torch.float64, device=self.dev)
        sums = torch.zeros(T, self.L.AME_PREDICT_SUMS, dtype=torch.float64, device=self.dev)
        a = self.L.ame_predict_args(x=_ptr(self.x), cov=_ptr(self.cov), Yt=_ptr(self.Yt), n_levels=0,
                                    sums=_ptr(sums), work=_ptr(work))
        self.L.check(self.lib.ame_predict(ctypes.byref(dims), ctypes.byref(a), None), "ame_predict")
        torch.cuda.synchronize()
        return sums.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Device results and the reference of one shape, computed once."""
    dv = _Device(shape)
    n, T, r = shape
    before = dv.predict_sums()
    st, dy = dv.stats()
    after = dv.predict_sums()
    srows, smag = M.state_rows(dv.X, dv.S)
    drows, dmag = M.dyad_rows(dv.X, dv.S, r, dv.Y)
    return dict(dv=dv, state=st, dyad=dy, predict_before=before, predict_after=after,
                srows=srows, smag=smag, drows=drows, dmag=dmag)


@pytest.mark.parametrize("shape", SHAPES + EVERY_R, ids=IDS)
def test_state_rows_match_fp64_reference(shape, gpu_device):
    c = _case(shape)
    n, T, r = shape
    got, want, mag = c["state"], c["srows"], c["smag"]
    assert got.shape == want.shape == (T, 2, 2 + 2 * r, 2 + 2 * r)
    assert np.isfinite(got).all()
    for which, N in ((0, 2 * n), (1, n)):
        err = np.abs(got[:, which] - want[:, which])
        bound = N * EPS * mag[:, which]
        ratio = (err / np.where(bound > 0, bound, 1.0)).max()
        print(f"{'PC'[which]}: max err / (N 2^-52 sum|summand|) = {ratio:.3e}")
        assert (err <= bound).all(), (which, ratio)
    assert (got[0, 1] == 0.0).all(), "C_t of global slice 0 must be exactly zero"
    assert np.abs(got[1:, 1]).min() > 0.0 if T > 1 else True


@pytest.mark.parametrize("shape", SHAPES + EVERY_R, ids=IDS)
def test_dyad_rows_match_reference_and_ame_predict(shape, gpu_device):
    c = _case(shape)
    n, T, r = shape
    got, want, mag = c["dyad"], c["drows"], c["dmag"]
    pairs = n * (n - 1) // 2
    for t in range(T):
        assert got[t, 0] == want[t, 0] == pairs
        for k in (1, 2):
            rel = abs(got[t, k] - want[t, k]) / abs(want[t, k])
            print(f"t={t} Rss{k - 1}{k - 1}: rel err {rel:.3e}")
            assert rel <= 5e-6, (t, k, got[t, k], want[t, k])
        bound = 5e-6 * mag[t, 3]
        print(f"t={t} Rss01: err {abs(got[t, 3] - want[t, 3]):.3e} bound {bound:.3e}")
        assert abs(got[t, 3] - want[t, 3]) <= bound, (t, got[t, 3], want[t, 3])
        # the same products and residuals as ame_predict at zero noise
        s = c["predict_before"][t]
        assert s[0] == pairs
        for k, (a, b) in ((1, (5, 7)), (2, (6, 8))):
            ref = s[a] + s[b]
            bound = 2 * pairs * EPS * ref          # every summand is non-negative
            print(f"t={t} Rss{k - 1}{k - 1} vs ame_predict: err {abs(got[t, k] - ref):.3e} bound {bound:.3e}")
            assert abs(got[t, k] - ref) <= bound, (t, k, got[t, k], ref)


@pytest.mark.parametrize("shape", SHAPES + EVERY_R, ids=IDS)
def test_bit_identity(shape, gpu_device):
    """Two runs agree bit for bit; one call over [0, T) equals two calls, the
    second with t_begin > 0 and prev_final; state-only and dyad-only calls give
    the same rows; ame_predict's sums are untouched by an ame_mstep_stats call."""
    c = _case(shape)
    dv = c["dv"]
    n, T, r = shape
    st2, dy2 = dv.stats()
    assert np.array_equal(st2, c["state"]) and np.array_equal(dy2, c["dyad"])
    assert np.array_equal(c["predict_before"], c["predict_after"])
    st_only, dy_nan = dv.stats(dyad=False)
    assert np.array_equal(st_only, c["state"]) and np.isnan(dy_nan).all()
    st_nan, dy_only = dv.stats(state=False)
    assert np.array_equal(dy_only, c["dyad"]) and np.isnan(st_nan).all()
    for k in range(1, T):
        sa, da = dv.stats(0, k)
        sb, db = dv.stats(k, T)
        assert np.array_equal(np.concatenate([sa, sb]), c["state"]), k
        assert np.array_equal(np.concatenate([da, db]), c["dyad"]), k


def test_capi_argument_errors(gpu_device):
    import torch
    from test_mstep_capi import check_argument_errors
    check_argument_errors()
    torch.cuda.synchronize()   # nothing was queued that could fault


# ---------------------------------------------------------------------------
# the VI layer
# ---------------------------------------------------------------------------
def _vi(n=30, T=5, r=2, lr=0.5, method="good", seed=11, model=None):
    import torch
    from ame_amd import TemporalAMEModel, TemporalAMENaiveMFVI, TemporalAMEStructuredMFVI
    if model is None:
        model = TemporalAMEModel(n, T, r, seed=seed)
        model.generate_data_fast(seed=seed + 1)
    dev = torch.device("cuda", 0)
    if method == "naive":
        return model, TemporalAMENaiveMFVI(model, learning_rate=lr, device=dev)
    return model, TemporalAMEStructuredMFVI(model, factorization=method, learning_rate=lr, device=dev)


def _history(vi):
    return ([float(e) for e in vi.history["elbo"]], [float(e) for e in vi.history["reconstruction_error"]])


@pytest.mark.parametrize("method,T,r", [("good", 4, 3), ("bad", 4, 3), ("naive", 4, 3), ("good", 3, 20)],
                         ids=["good", "bad", "naive", "good_T3_r20"])
def test_statistics_of_a_fitted_state(method, T, r, gpu_device):
    """m_step_statistics of every VI class against the reference on the
    downloaded state; a one-slice scratch budget changes no bit.  r = 20: the
    engine's own buffers, work-size query and scratch chunking on the K = 10
    state instance."""
    m, vi = _vi(n=40, T=T, r=r, method=method)
    vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    st = vi.m_step_statistics()
    X, S = vi.X_mean.numpy(), vi.X_cov.numpy()
    ref = M.statistics(X, S, m.r, m.Y.numpy())
    smag = M.state_rows(X, S)[1]
    for k, mg, N in (("A0", smag[0, 0], 2 * m.n), ("A11", smag[1:, 0].sum(0), 2 * m.n * (m.T - 1)),
                     ("A00", smag[:-1, 0].sum(0), 2 * m.n * (m.T - 1)),
                     ("A10", smag[1:, 1].sum(0), m.n * (m.T - 1))):
        assert st[k].dtype.is_floating_point and st[k].element_size() == 8 and not st[k].is_cuda
        assert (np.abs(st[k].numpy() - ref[k]) <= N * EPS * mg).all(), k
    assert st["pairs"] == ref["pairs"] == m.T * m.n * (m.n - 1) // 2
    assert np.abs(st["Rss"].numpy() - ref["Rss"]).max() <= 5e-6 * np.abs(ref["Rss"]).max()
    eng = vi.engine
    budget = eng.PREDICT_WORK_DOUBLES
    try:
        eng.PREDICT_WORK_DOUBLES = 1
        again = vi.m_step_statistics()
    finally:
        eng.PREDICT_WORK_DOUBLES = budget
    for k in ("A0", "A11", "A00", "A10", "Rss"):
        assert np.array_equal(again[k].numpy(), st[k].numpy()), k


def test_statistics_do_not_disturb_fit(gpu_device):
    """fit -> m_step_statistics -> fit has the bits of fit -> fit."""
    def run(check):
        m, vi = _vi(n=40, T=4, r=3)
        vi.fit(max_iter=3, tolerance=0.0, verbose=False)
        if check:
            vi.m_step_statistics()
            vi.m_step(apply=False)
        vi.fit(max_iter=3, tolerance=0.0, verbose=False)
        return vi.X_mean.numpy().copy(), vi.X_cov.numpy().copy(), _history(vi)

    a, b = run(True), run(False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2] == b[2]


def test_apply_equals_a_fresh_instance_on_the_updated_model(gpu_device):
    import torch
    m, vi = _vi()
    vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    old = {k: getattr(m, k).clone() for k in ("Phi", "Q", "R", "R_inv", "Sigma", "Psi")}
    res = vi.m_step(apply=True)
    for k in ("Phi", "Q", "R", "Sigma", "Psi"):
        new = getattr(m, k)
        assert new.dtype == torch.float32 and not torch.equal(new, old[k]), k
        assert torch.equal(new, res[k].to(torch.float32)), k
    assert torch.equal(m.R_inv, torch.linalg.inv(m.R))
    assert res["objective_after"] >= res["objective_before"]
    X, S = vi.X_mean.clone(), vi.X_cov.clone()
    _, fresh = _vi(model=m)
    fresh.X_mean, fresh.X_cov = X.clone(), S.clone()
    assert torch.equal(vi.engine.consts.cpu(), fresh.engine.consts.cpu())
    assert torch.equal(vi.engine.phi.cpu(), fresh.engine.phi.cpu())
    assert list(vi.engine.C.rinv4()) == list(fresh.engine.C.rinv4())
    n0 = len(vi.history["elbo"])
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    fresh.fit(max_iter=1, tolerance=0.0, verbose=False)
    assert torch.equal(vi.X_mean, fresh.X_mean) and torch.equal(vi.X_cov, fresh.X_cov)
    assert float(vi.history["elbo"][n0]) == float(fresh.history["elbo"][0])
    assert vi.history["reconstruction_error"][n0] == fresh.history["reconstruction_error"][0]


def test_update_subset_and_refusal(gpu_device):
    import torch
    m, vi = _vi()
    vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    names = ("Phi", "Q", "R", "R_inv", "Sigma", "Psi")
    old = {k: getattr(m, k).clone() for k in names}
    consts = vi.engine.consts.cpu().clone()
    res = vi.m_step(update=("R",))
    for k in ("Phi", "Q", "Sigma", "Psi"):
        assert torch.equal(getattr(m, k), old[k]), k
        assert torch.equal(res[k], old[k].double()), k
    assert not torch.equal(m.R, old["R"]) and not torch.equal(m.R_inv, old["R_inv"])
    assert torch.equal(vi.engine.consts.cpu(), consts)   # none of them depends on R
    with pytest.raises(ValueError):
        vi.m_step(update=("Phi", "Sigma"))
    with pytest.raises(ValueError):
        vi.m_step(phi_structure="diagonal")
    # a non-finite result raises and applies nothing
    now = {k: getattr(m, k).clone() for k in names}
    bad = vi.X_mean.clone()
    bad[0, 0, 0] = float("inf")
    vi.X_mean = bad
    with pytest.raises(ValueError):
        vi.m_step()
    for k in names:
        assert torch.equal(getattr(m, k), now[k]), k


@pytest.mark.parametrize("phi_structure", ["full", "scalar"])
def test_objective_never_decreases(phi_structure, gpu_device):
    """objective_after >= objective_before in every EM round, on the GPU
    statistics, up to the evaluation error of F: 2^12 terms at most (d <= 66),
    so 2^-40 x the sum of the |terms| of F."""
    m, vi = _vi(n=30, T=6, r=3)
    for k in range(3):
        vi.fit(max_iter=3, tolerance=0.0, verbose=False)
        st = {k2: (v.numpy() if hasattr(v, "numpy") else v) for k2, v in vi.m_step_statistics().items()}
        res = vi.m_step(phi_structure=phi_structure)
        new = {k2: res[k2].numpy() for k2 in M.PARAMS}
        mag = M.objective_magnitude(st, new, m.n, m.T)
        assert abs(res["objective_scale"] - mag) <= 1e-9 * mag
        slack = 2.0 ** -40 * mag
        print(f"round {k}: F {res['objective_before']:.6f} -> {res['objective_after']:.6f} (slack {slack:.1e})")
        assert res["objective_after"] >= res["objective_before"] - slack, k
        # the returned objective is the reference's F of the returned parameters
        assert abs(res["objective_after"] - M.objective(st, new, m.n, m.T)) <= slack
        if phi_structure == "scalar":
            phi = res["Phi"].numpy()
            assert np.array_equal(phi, phi[0, 0] * np.eye(m.d))


def test_fit_em_end_to_end(gpu_device):
    """The experiment of em_case: the GPU run recovers the parameters (both
    additive diagonal entries of Phi within 0.1 of 0.8, every R entry within
    0.05 of the truth) and after round 1 agrees with the fp64 CPU EM within 4 x
    the CPU EM's own fp32 sensitivity."""
    import torch
    from ame_amd import TemporalAMEStructuredMFVI
    m = em_case.make_model()
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=M.EM_LR,
                                   device=torch.device("cuda", 0))
    h = vi.fit_em(M.EM_ROUNDS, M.EM_SWEEPS, update=M.EM_UPDATE, tolerance=0.0, verbose=False)
    em = h["em"]
    assert len(em) == M.EM_ROUNDS
    assert len(h["elbo"]) == len(h["reconstruction_error"]) == M.EM_ROUNDS * M.EM_SWEEPS
    for k, rd in enumerate(em):
        print(f"round {k}: Phi diag {rd['Phi'].diagonal()[:2].tolist()} R "
              f"{rd['R'].flatten()[[0, 1, 3]].tolist()} F {rd['objective_before']:.3f} -> "
              f"{rd['objective_after']:.3f}")
        assert rd["objective_after"] >= rd["objective_before"] - 2.0 ** -40 * rd["objective_scale"]
    last = em[-1]
    assert np.abs(last["Phi"].diagonal()[:2].numpy() - M.TRUE_AR).max() <= 0.1
    assert np.abs(last["R"].flatten()[[0, 1, 3]].numpy() - np.array(M.TRUE_R)).max() <= 0.05
    assert torch.equal(m.Phi, last["Phi"].float()) and torch.equal(m.R, last["R"].float())
    cpu = em_case.cpu_runs()
    own = em_case.relative_deviation(cpu["em64"][0], cpu["em32"][0])
    got = em_case.relative_deviation(cpu["em64"][0], {k: em[0][k].numpy() for k in ("Phi", "Q", "R")})
    print(f"round 1: GPU vs fp64 CPU EM {got:.3e}; CPU EM fp32 vs fp64 {own:.3e}; allowance {4 * own:.3e}")
    assert got <= 4.0 * own, (got, own)
