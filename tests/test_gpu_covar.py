"""ame_covar_stats / ame_covar_resid and the covariate regression built on them
(set_covariates, m_step(update=(..., "beta")), fit_em, predictions) on the GPU,
against the fp64 reference tests/covar_ref.py.

Bounds.
  H: products of fp32 inputs are exact in fp64, so device and reference differ
  by re-association only: |got - want| <= N 2^-52 sum|summand|, N the pairs of a
  slice.  H[k][l][a][b] == H[l][k][b][a] exactly.
  G: e comes from the fp32 MFMA products and an fp32 subtraction, then signed
  fp64 sums: 5e-6 x sum|w_a||e_b|, the rule test_gpu_mstep.py applies to Rss01.
  ame_covar_resid: bit-equal to numpy's fp64 evaluation rounded once to fp32.
  Consistency of Rss after set_beta(beta + delta) with the host identity:
  test_gpu_mstep.py's Rss bounds (5e-6 of the sums of |summand|) at the new beta
  plus the fp32 re-rounding of the residual buffer, 2^-24 |y~| per element:
  2^-24 (|y~_a||e_b| + |e_a||y~_b|) per summand of Rss[a][b], which is
  2 x 2^-24 |y~||e| on the diagonal.
  End to end: beta after EM round 1 against the fp64 oracle EM within 4 x the
  oracle's own fp32-vs-fp64 deviation (covar_ref.relative_deviation, over beta
  and R), measured in the test.

Room under the bounds, measured on an MI355X over the cases added for every
compiled r and p (EVERY_R_P and SMALL_P); for information, no bound comes from
them.  Worst error / bound: H 4.0e-2 (of N 2^-52 sum|summand|); G 2.7e-3
(1.4e-8 of sum|w_a||e_b|, of 5e-6); the residual is bit-equal.
tests/test_covar_ref.py shows on the same inputs that fp32 arithmetic alone
stays under a tenth of the G bound and that a lost latent column moves an entry
of G in every slice by 750 x its bound or more.
"""
import ctypes
import functools

import numpy as np
import pytest

import covar_ref as CR
import mstep_ref as M

pytestmark = pytest.mark.gpu

# (n, T, r, p): one partial tile with odd n; a pad column; exactly one tile; a
# tile edge plus a pad column; three tile rows; r over the compiled split parts;
# p = 1, 3 and 8
CASES = ((5, 1, 1, 1), (33, 3, 2, 3), (64, 2, 3, 8), (65, 4, 5, 1), (130, 3, 16, 3), (70, 2, 32, 8))
# every compiled r, so every MFMA step count pad4(r + 2) / 4 = 1..9 of the G
# kernel and every residue of r + 2 mod 4 before its zero padding, on two tile
# rows with a one-wide edge tile and a pad column; p cycles through 1..8, so each
# instance <P> of the G, H and residual kernels runs at four r
EVERY_R_P = tuple((65, 2, r, 1 + (r - 1) % 8) for r in range(1, 33))
# the p that CASES leaves out, on a single partial diagonal tile: with EVERY_R_P
# every p = 1..8 runs on two shapes
SMALL_P = tuple((20, 3, 3, p) for p in (2, 4, 5, 6, 7))
ALL_CASES = CASES + EVERY_R_P + SMALL_P
IDS = lambda c: "n%d_T%d_r%d_p%d" % c
EPS = 2.0 ** -52


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class _Device:
    """make_state's means, a generated network and covariates on the device in
    the layouts of include/ame_amd.h, with raw C-ABI calls over slice ranges."""

    def __init__(self, case):
        import torch
        from ame_amd import _lib
        self.L, self.lib = _lib, _lib.lib()
        n, T, r, p = self.case = case
        self.dev = torch.device("cuda", 0)
        self.X, self.Y, self.W, self.beta = CR.gpu_inputs(case)
        self.x = torch.from_numpy(self.X).permute(1, 0, 2).contiguous().to(self.dev)
        dims = self.dims(0, T)
        self.ny = int(self.lib.ame_pack_y_size(ctypes.byref(dims))) // (2 * T * n)
        self.Yraw = self._pack(self.Y)
        self.Wt = torch.stack([self._pack(self.W[k]) for k in range(p)]).contiguous()
        self.Yt = self.resid(self.beta)
        torch.cuda.synchronize()

    def dims(self, t0, t1):
        n, T, r, _ = self.case
        return self.L.ame_dims(n, r, t1 - t0, t0, T, self.L.AME_GOOD)

    def _pack(self, A):
        import torch
        n, T, _, _ = self.case
        src = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).to(self.dev)
        out = torch.zeros(T, n, self.ny, 2, dtype=torch.float32, device=self.dev)
        mm = torch.zeros(1, dtype=torch.int64, device=self.dev)
        dims = self.dims(0, T)
        self.L.check(self.lib.ame_pack_y(_ptr(src), _ptr(out), ctypes.byref(dims), _ptr(mm), None), "ame_pack_y")
        torch.cuda.synchronize()
        return out

    def resid(self, beta):
        import torch
        n, T, _, p = self.case
        out = torch.full_like(self.Yraw, float("nan"))
        dims = self.dims(0, T)
        cb = (ctypes.c_double * p)(*[float(b) for b in beta])
        self.L.check(self.lib.ame_covar_resid(ctypes.byref(dims), _ptr(self.Yraw), _ptr(self.Wt), cb, p,
                                              _ptr(out), None), "ame_covar_resid")
        torch.cuda.synchronize()
        return out

    def stats(self, t0=None, t1=None, want_g=True, want_h=True):
        import torch
        n, T, r, p = self.case
        t0, t1 = 0 if t0 is None else t0, T if t1 is None else t1
        dims = self.dims(t0, t1)
        ws = int(self.lib.ame_covar_work_size(ctypes.byref(dims), p))
        assert ws > 0
        work = torch.empty(ws, dtype=torch.float64, device=self.dev)
        G = torch.full((t1 - t0, p, 2, 2), float("nan"), dtype=torch.float64, device=self.dev)
        H = torch.full((t1 - t0, p, p, 2, 2), float("nan"), dtype=torch.float64, device=self.dev)
        Wt = self.Wt[:, t0:t1].contiguous()
        a = self.L.ame_covar_args(x=_ptr(self.x[t0:t1]), Yt=_ptr(self.Yt[t0:t1]), Wt=_ptr(Wt), p=p,
                                  G=_ptr(G) if want_g else None, H=_ptr(H) if want_h else None,
                                  work=_ptr(work), work_doubles=ws)
        self.L.check(self.lib.ame_covar_stats(ctypes.byref(dims), ctypes.byref(a), None), "ame_covar_stats")
        torch.cuda.synchronize()
        return G.cpu().numpy(), H.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(case):
    """Device results and the reference of one case, computed once."""
    dv = _Device(case)
    n, T, r, p = case
    G, H = dv.stats()
    Yres = CR.resid(dv.Y, dv.W, dv.beta)
    rG, rGm, rH, rHm = CR.gh_rows(dv.X, r, Yres, dv.W)
    return dict(dv=dv, G=G, H=H, Yres=Yres, rG=rG, rGm=rGm, rH=rH, rHm=rHm)


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_H_matches_fp64_reference(case, gpu_device):
    c = _case(case)
    n, T, r, p = case
    got, want, mag = c["H"], c["rH"], c["rHm"]
    assert got.shape == want.shape == (T, p, p, 2, 2) and np.isfinite(got).all()
    N = n * (n - 1) // 2
    err, bound = np.abs(got - want), N * EPS * mag
    print(f"H: max err / (N 2^-52 sum|summand|) = {(err / bound).max():.3e}")
    assert (err <= bound).all()
    assert np.array_equal(got, got.transpose(0, 2, 1, 4, 3)), "H[k][l][a][b] != H[l][k][b][a]"
    assert (got[:, np.arange(p), np.arange(p), 0, 0] > 0).all()


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_G_matches_fp64_reference(case, gpu_device):
    c = _case(case)
    n, T, r, p = case
    got, want, mag = c["G"], c["rG"], c["rGm"]
    assert got.shape == want.shape == (T, p, 2, 2) and np.isfinite(got).all()
    err, bound = np.abs(got - want), 5e-6 * mag
    print(f"G: max err / sum|w_a||e_b| = {(err / mag).max():.3e} (bound 5e-6)")
    assert (err <= bound).all()
    # a real test of e: G changes by far more than the bound when the means are left out
    assert (np.abs(want) > 0).all()


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_slice_split_invariance(case, gpu_device):
    """Two runs agree bit for bit; one call over [0, T) equals two calls, the
    second with t_begin > 0; G-only and H-only calls give the same rows."""
    c = _case(case)
    dv = c["dv"]
    n, T, r, p = case
    G2, H2 = dv.stats()
    assert np.array_equal(G2, c["G"]) and np.array_equal(H2, c["H"])
    G_only, H_nan = dv.stats(want_h=False)
    assert np.array_equal(G_only, c["G"]) and np.isnan(H_nan).all()
    G_nan, H_only = dv.stats(want_g=False)
    assert np.array_equal(H_only, c["H"]) and np.isnan(G_nan).all()
    for k in range(1, T):
        Ga, Ha = dv.stats(0, k)
        Gb, Hb = dv.stats(k, T)
        assert np.array_equal(np.concatenate([Ga, Gb]), c["G"]), k
        assert np.array_equal(np.concatenate([Ha, Hb]), c["H"]), k


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_resid_is_fp64_rounded_once(case, gpu_device):
    c = _case(case)
    dv = c["dv"]
    n, T, r, p = case
    raw, Wt = dv.Yraw.cpu().numpy(), dv.Wt.cpu().numpy()
    got = dv.Yt.cpu().numpy()
    s = np.zeros(raw.shape, dtype=np.float64)
    for k in range(p):
        s += np.float64(dv.beta[k]) * Wt[k].astype(np.float64)
    want = (raw.astype(np.float64) - s).astype(np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    # the packed values are the reference layout's
    assert np.array_equal(_bits(got[:, :, :n]), _bits(c["Yres"].transpose(2, 0, 1, 3)))
    if dv.ny > n:
        assert np.array_equal(_bits(got[:, :, n:]), _bits(raw[:, :, n:]))
        assert (Wt[:, :, :, n:] == 0).all()
    zero = dv.resid(np.zeros(p)).cpu().numpy()
    assert np.array_equal(_bits(zero), _bits(raw))


def test_resid_is_not_contracted(gpu_device):
    """covar_ref.contraction_probe: an element (p = 2) whose fused and unfused
    evaluations round to different fp32 values, in every position of a small
    packed plane (n = 3: a pad column too)."""
    import torch
    from ame_amd import _lib
    lib = _lib.lib()
    w, beta, unfused, fused = CR.contraction_probe()
    assert unfused != fused
    dev = torch.device("cuda", 0)
    dims = _lib.ame_dims(3, 1, 2, 0, 2, _lib.AME_GOOD)
    ny = int(lib.ame_pack_y_size(ctypes.byref(dims))) // (2 * 2 * 3)
    raw = torch.zeros(2, 3, ny, 2, dtype=torch.float32, device=dev)
    Wt = torch.from_numpy(w).to(dev)[:, None, None, None, None].expand(2, 2, 3, ny, 2).contiguous()
    out = torch.full_like(raw, float("nan"))
    cb = (ctypes.c_double * 2)(*beta.tolist())
    _lib.check(lib.ame_covar_resid(ctypes.byref(dims), _ptr(raw), _ptr(Wt), cb, 2, _ptr(out), None),
               "ame_covar_resid")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(np.full(got.shape, unfused, dtype=np.float32))), \
        (float(got.flat[0]), float(unfused), float(fused))


def test_capi_argument_errors(gpu_device):
    import torch
    from test_covar_capi import check_argument_errors
    check_argument_errors()
    torch.cuda.synchronize()   # nothing was queued that could fault


# ---------------------------------------------------------------------------
# the VI layer
# ---------------------------------------------------------------------------
def _model(n=30, T=4, r=2, p=2, seed=11, beta=(0.5, -0.3), covariates=True):
    import torch
    from ame_amd import TemporalAMEModel
    m = TemporalAMEModel(n, T, r, seed=seed)
    if covariates:
        m.set_covariates(torch.from_numpy(CR.make_w(n, T, p, seed=seed)), beta=beta[:p])
    m.generate_data_fast(seed=seed + 1)
    return m


def _vi(model, lr=0.5):
    import torch
    from ame_amd import TemporalAMEStructuredMFVI
    return TemporalAMEStructuredMFVI(model, factorization="good", learning_rate=lr,
                                     device=torch.device("cuda", 0))


def test_rss_after_set_beta_matches_host_identity(gpu_device):
    import torch
    from ame_amd import mstep
    m = _model(n=40, T=3, r=3, p=3, beta=(0.5, -0.3, 0.2))
    m.beta = torch.tensor([0.3, 0.1, -0.2])            # not the generating beta: delta is not small
    vi = _vi(m)
    vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    st = vi.m_step_statistics()
    assert set(("G", "H", "beta")) <= set(st) and torch.equal(st["beta"], m.beta.double())
    delta = mstep.beta_step(st, m.R.double())
    want = mstep.rss_at(st, delta).numpy()
    vi.engine.set_beta(st["beta"] + delta)
    got = vi.m_step_statistics()["Rss"].numpy()
    # the issue's allowance, from the downloaded state: test_gpu_mstep.py's Rss
    # bounds (5e-6 of the sums of |summand|; Rss00 / Rss11 have non-negative
    # summands, so that is their 5e-6 relative rule) at the new beta, plus the fp32
    # re-rounding of the residual buffer, 2^-24 |y~| per element: 2 x 2^-24 |y~||e|
    # per summand on the diagonal, 2^-24 (|y~_a||e_b| + |e_a||y~_b|) off it
    X, S, r = vi.X_mean.numpy(), vi.X_cov.numpy(), m.r
    Y, W = m.Y.numpy().astype(np.float64), m.W.numpy()
    iu = np.triu_indices(m.n, 1)
    Yres = Y - CR.effect(W, (st["beta"] + delta).numpy())
    mag = M.dyad_rows(X, S, r, Yres)[1].sum(0)
    bound = 5e-6 * np.array([[mag[1], mag[3]], [mag[3], mag[2]]])
    for t in range(m.T):
        y = np.abs(Yres[iu[0], iu[1], t])
        e = np.abs(Yres[iu[0], iu[1], t] - CR.mean_mu(X[:, t], r)[iu[0], iu[1]])
        bound += 2.0 ** -24 * (np.einsum("na,nb->ab", y, e) + np.einsum("na,nb->ab", e, y))
    err = np.abs(got - want)
    print(f"Rss(beta + delta): err {err.tolist()} allowance {bound.tolist()} ratio {(err / bound).max():.3e}")
    assert (err <= bound).all()
    # and the step did something: Rss moved by far more than the allowance
    assert np.abs(st["Rss"].numpy() - got).max() > 100 * bound.max()


def test_statistics_chunking_and_cached_H(gpu_device):
    m = _model(n=40, T=4, r=3, p=2)
    vi = _vi(m)
    vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    st = vi.m_step_statistics()
    eng = vi.engine
    H_first = eng._covar_H
    budget = eng.PREDICT_WORK_DOUBLES
    try:
        eng.PREDICT_WORK_DOUBLES = 1
        eng._covar_H = None
        again = vi.m_step_statistics()
    finally:
        eng.PREDICT_WORK_DOUBLES = budget
    for k in ("G", "H", "Rss"):
        assert np.array_equal(again[k].numpy(), st[k].numpy()), k
    assert np.array_equal(H_first.cpu().numpy(), eng._covar_H.cpu().numpy())
    H_obj = eng._covar_H
    vi.m_step_statistics()
    assert eng._covar_H is H_obj                         # computed once per engine


def test_fit_em_end_to_end(gpu_device):
    import torch
    m = CR.make_model()
    assert torch.equal(m.beta, torch.zeros(CR.EM_P))
    vi = _vi(m, lr=CR.EM_LR)
    h = vi.fit_em(CR.EM_ROUNDS, CR.EM_SWEEPS, update=CR.EM_UPDATE, tolerance=0.0, verbose=False)
    em = h["em"]
    assert len(em) == CR.EM_ROUNDS
    for k, rd in enumerate(em):
        print(f"round {k}: beta {rd['beta'].tolist()} R {rd['R'].flatten()[[0, 1, 3]].tolist()} "
              f"F {rd['objective_before']:.4f} -> {rd['objective_after']:.4f}")
        # (b)
        assert rd["objective_after"] >= rd["objective_before"] - 4 * EPS * rd["objective_scale"], k
    # (a)
    cpu = CR.cpu_runs()
    own = CR.relative_deviation(cpu["em64"][0], cpu["em32"][0])
    got = CR.relative_deviation(cpu["em64"][0], {k: em[0][k].numpy() for k in ("beta", "R")})
    print(f"round 1: GPU vs fp64 CPU EM {got:.3e}; CPU EM fp32 vs fp64 {own:.3e}; allowance {4 * own:.3e}")
    assert got <= 4.0 * own, (got, own)
    dev_b = lambda x, y: float(np.abs(np.asarray(x["beta"]) - np.asarray(y["beta"])).max()
                               / np.abs(np.asarray(x["beta"])).max())
    own_b = dev_b(cpu["em64"][0], cpu["em32"][0])
    got_b = dev_b(cpu["em64"][0], {"beta": em[0]["beta"].numpy()})
    print(f"round 1, beta alone: GPU vs fp64 CPU EM {got_b:.3e}; CPU EM fp32 vs fp64 {own_b:.3e}; "
          f"allowance {4 * own_b:.3e}")
    assert got_b <= 4.0 * own_b, (got_b, own_b)
    # (c)
    true = np.array(CR.EM_BETA)
    err = np.abs(em[-1]["beta"].numpy() - true).max()
    print(f"final |beta_hat - beta|_inf = {err:.3e}")
    assert err < 0.5 * np.abs(true).min()
    assert torch.equal(m.beta, em[-1]["beta"].float()) and m.beta.dtype == torch.float32
    assert torch.equal(vi.engine.beta, m.beta.double())
    # (d) predict_dyads = the no-covariate means + sum_k beta_k W_k of the block
    eng = vi.engine
    rows, cols, t0, t1 = range(3, 20), range(10, 41), 1, 4
    base, second0 = vi._dense(eng, eng.x_a[t0:t1], eng.cov[t0:t1], rows, cols, True, 2 ** 27)
    mean, second = vi.predict_dyads(slice(t0, t1), rows=rows, cols=cols)
    eff = CR.effect(m.W.numpy()[:, 3:20, 10:41, t0:t1], m.beta.numpy().astype(np.float64))
    assert torch.equal(second, second0) or np.array_equal(np.isnan(second.numpy()), np.isnan(second0.numpy()))
    want = base.numpy().astype(np.float64) + eff
    # fp32 on the host: p products and p - 1 partial sums, each within 2^-24 of
    # sum_k |beta_k w_k|, and one rounding of the final sum (one more term for
    # the second-order parts)
    Wb = np.abs(m.W.numpy()[:, 3:20, 10:41, t0:t1].astype(np.float64))
    effabs = np.einsum("k,kijtc->ijtc", np.abs(m.beta.numpy().astype(np.float64)), Wb)
    tol = 2.0 ** -24 * (np.abs(want) + (2 * CR.EM_P + 1) * effabs)
    ratio = (np.abs(mean.numpy() - want) / tol).max()
    print(f"predict_dyads means: max err / fp32 rounding bound = {ratio:.3f}")
    assert np.abs(eff).max() > 0.1 and ratio <= 1.0


def test_forecasts_need_future_covariates(gpu_device):
    import torch
    m = _model()
    vi = _vi(m)
    vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    h = 2
    Wf = torch.from_numpy(CR.make_w(m.n, h, 2, seed=99))
    Yf = torch.randn(m.n, m.n, h, 2)
    with pytest.raises(ValueError):
        vi.forecast_dyads(h)
    with pytest.raises(ValueError):
        vi.forecast_check(Yf)
    with pytest.raises(ValueError):
        vi.forecast_dyads(h, W_future=Wf[:, :, :, :1])
    mean, _ = vi.forecast_dyads(h, W_future=Wf)
    zero, _ = vi.forecast_dyads(h, W_future=torch.zeros_like(Wf))
    eff = m.covariate_effect(Wf)
    assert torch.allclose(mean, zero + eff, rtol=0, atol=1e-5)
    a = vi.forecast_check(Yf, W_future=Wf)
    b = vi.forecast_check(Yf - eff, W_future=torch.zeros_like(Wf))
    assert np.array_equal(a["log_score"], b["log_score"])
    # a model without covariates refuses W_future and "beta"
    plain = _vi(_model(covariates=False))
    plain.fit(max_iter=1, tolerance=0.0, verbose=False)
    with pytest.raises(ValueError):
        plain.forecast_dyads(h, W_future=Wf)
    with pytest.raises(ValueError):
        plain.m_step(update=("beta", "R"))
    with pytest.raises(ValueError):
        plain.fit_em(1, 1, update=("beta",), verbose=False)


def test_singular_beta_system_applies_nothing(gpu_device):
    import torch
    m = _model(p=2)
    W = m.W.clone()
    W[1] = 2.0 * W[0]
    m.set_covariates(W, beta=[0.1, 0.2])
    vi = _vi(m)
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    R, beta, Yt = m.R.clone(), m.beta.clone(), vi.engine.Yt.clone()
    with pytest.raises(ValueError):
        vi.m_step(update=("beta", "R"))
    assert torch.equal(m.R, R) and torch.equal(m.beta, beta) and torch.equal(vi.engine.Yt, Yt)


def test_no_covariate_path_is_untouched(gpu_device):
    """Without covariates the engine holds no Yt_raw / Wt and Yt is the packed
    network; two fresh engines agree bit for bit; and a model whose covariates
    have beta = 0 (residual == Y, through the separate buffer) fits to the same
    bits as the model without."""
    import torch
    def run(covariates):
        m = _model(covariates=False)
        if covariates:
            m.set_covariates(torch.from_numpy(CR.make_w(m.n, m.T, 2)))
        vi = _vi(m)
        vi.fit(max_iter=4, tolerance=0.0, verbose=False)
        return vi, (vi.X_mean.clone(), vi.X_cov.clone(), [float(e) for e in vi.history["elbo"]],
                    list(vi.history["reconstruction_error"]))

    va, a = run(False)
    vb, b = run(False)
    vc, c = run(True)
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
        assert a[2] == other[2] and a[3] == other[3]
    for vi in (va, vb):
        eng = vi.engine
        assert not hasattr(eng, "Yt_raw") and not hasattr(eng, "Wt") and eng.p == 0 and eng.beta is None
        with pytest.raises(ValueError):
            eng.covar_stats()
        with pytest.raises(ValueError):
            eng.set_beta([0.0])
    assert vc.engine.Yt.data_ptr() != vc.engine.Yt_raw.data_ptr()
    assert torch.equal(vc.engine.Yt, vc.engine.Yt_raw) and torch.equal(va.engine.Yt, vc.engine.Yt_raw)


def test_time_sharded_engine_refuses_covariates(gpu_device):
    import torch
    from ame_amd.engine import DeviceEngine, Shard
    m = _model()
    vi = _vi(m)
    with pytest.raises(NotImplementedError):
        DeviceEngine(m, "good", 0.5, vi.X_mean, vi.X_cov, device=torch.device("cuda", 0),
                     shard=Shard(0, 2, m.T))
