"""ame_net_moments / ame_net_triads / ame_simulate and the goodness-of-fit calls
built on them (network_statistics, sample_states, gof) on the GPU, against the
fp64 reference tests/gof_ref.py.

Bounds.
  Moments: every summand is an fp32 value or an exact product of two, so device
  and reference differ by re-association only: |got - want| <= N 2^-52
  sum|summand|, N = n (n - 1).
  Triads: the reference centres by the fp32 number the kernel is given; each e
  carries one fp32 rounding and a K = n term fp32 MFMA accumulation at most
  K 2^-24 of sum|a_k b_k|: (n + 3) 2^-24 sum_ijk |E_ik E_kj E_ji|, and the same
  with E_jk for the transitive sum.
  Simulate: against gof_ref.simulate, fp64 from the same Philox integers (the
  fp32 uniforms are reproduced exactly).  Mean: the fill kernel's rule,
  2 (r + 1) 2^-24 (|a| + |b| + sum_k |u_k v_k|).  Noise: NOISE_REL |l| (1 + |z|)
  per term, NOISE_REL = 4 x the largest deviation measured over CASES with zero
  states (test_noise_deviation_is_within_the_measured_margin prints it).
  End to end: gof() is checked stage by stage, each stage against its own
  bound: every simulated network (engine.simulate with gof()'s arguments, the
  same bits gof() reduces) against gof_ref.simulate within the simulate bounds,
  and gof()'s statistics against the fp64 statistics of exactly those networks
  within the moment and triad bounds propagated through the statistics
  (gof_ref.statistic_bounds: first order, doubled, plus the fp64 evaluation).

Room under the bounds, measured on an MI355X (for information, no bound comes
from them except NOISE_REL as stated): see DESIGN.md section 7h.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import gof_ref as R

pytestmark = pytest.mark.gpu

# (n, T, r): a single partial tile; odd n with a pad column, one over the triad
# kernel's k chunk (32); the dyad tile's edge (64), K pad 5 -> 8; one over it,
# odd; one over the triad tile's edge (128), several dyad tiles, ragged; the
# widest state; eight slices, where the triad kernel takes ame_tile.h's other
# slice mapping (all workgroups of a slice on one XCD)
CASES = ((5, 1, 1), (33, 3, 2), (64, 2, 3), (65, 4, 5), (130, 3, 16), (70, 2, 32), (20, 8, 1))
KINDS = ("plain", "nan", "offset")
IDS = lambda c: "n%d_T%d_r%d" % c
CHOL = (1.1, 0.35, 0.8)
SEED = 0x9E3779B97F4A7C15          # both key words in use
SAMPLE, T_BEGIN = 3, 2
# 4 x the largest |got - fp64| / (|l| (1 + |z|)) measured on an MI355X over CASES
# with zero states (1.404e-7)
NOISE_REL = 4 * 1.404e-7


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int64 if t.dtype.itemsize == 8 else np.int32)


class _Device:
    """Raw C-ABI calls over slice ranges of one case."""

    def __init__(self, case):
        import torch
        from ame_amd import _lib
        self.L, self.lib, self.torch = _lib, _lib.lib(), torch
        self.case = case
        self.dev = torch.device("cuda", 0)
        self.ny = case[0] + (case[0] & 1)

    def dims(self, S, t0=0, T=None):
        n, _, r = self.case
        return self.L.ame_dims(n, r, S, t0, t0 + S if T is None else T, self.L.AME_GOOD)

    def up(self, a):
        return self.torch.from_numpy(np.array(a)).to(self.dev)   # a copy: the cached arrays are read-only

    def moments(self, Yt):
        torch, S, n = self.torch, int(Yt.shape[0]), self.case[0]
        dm = self.dims(S)
        need = int(self.lib.ame_net_moments_work_size(ctypes.byref(dm)))
        work = torch.full((need,), float("nan"), dtype=torch.float64, device=self.dev)
        node = torch.full((S, n, 2), float("nan"), dtype=torch.float64, device=self.dev)
        sl = torch.full((S, 2), float("nan"), dtype=torch.float64, device=self.dev)
        a = self.L.ame_moments_args(Yt=_ptr(Yt), node=_ptr(node), slice=_ptr(sl), work=_ptr(work), work_doubles=need)
        self.L.check(self.lib.ame_net_moments(ctypes.byref(dm), ctypes.byref(a), None), "ame_net_moments")
        torch.cuda.synchronize()
        return node, sl

    def triads(self, Yt, center):
        torch, S = self.torch, int(Yt.shape[0])
        dm = self.dims(S)
        need = int(self.lib.ame_net_triads_work_size(ctypes.byref(dm)))
        work = torch.full((need,), float("nan"), dtype=torch.float64, device=self.dev)
        tri = torch.full((S, 2), float("nan"), dtype=torch.float64, device=self.dev)
        a = self.L.ame_triads_args(Yt=_ptr(Yt), center=_ptr(center), tri=_ptr(tri), work=_ptr(work),
                                   work_doubles=need)
        self.L.check(self.lib.ame_net_triads(ctypes.byref(dm), ctypes.byref(a), None), "ame_net_triads")
        torch.cuda.synchronize()
        return tri

    def simulate(self, x, chol=CHOL, seed=SEED, sample=SAMPLE, t_begin=T_BEGIN):
        torch, S, n = self.torch, int(x.shape[0]), self.case[0]
        out = torch.full((S, n, self.ny, 2), float("nan"), dtype=torch.float32, device=self.dev)
        a = self.L.ame_simulate_args(x=_ptr(x), lr=(ctypes.c_double * 3)(*chol), seed=seed, sample=sample,
                                     Yt_out=_ptr(out))
        dm = self.dims(S, t_begin)
        self.L.check(self.lib.ame_simulate(ctypes.byref(dm), ctypes.byref(a), None), "ame_simulate")
        torch.cuda.synchronize()
        return out


@functools.lru_cache(maxsize=None)
def _net(case, kind):
    """(packed fp32 network, dense fp64 network, fp32 centre, reference raw sums); read-only."""
    n, T, _ = case
    y = R.make_network(n, T, 1000 + n, "offset" if kind == "offset" else "plain")
    Yd = R.dense_from_directed(y)
    Yt = R.pack(Yd)
    if kind == "nan":   # what the kernels must never read as data
        Yt[:, np.arange(n), np.arange(n)] = np.nan
        Yt[:, :, n:] = np.nan
    raw0 = R.raw_sums(Yd, np.zeros(T, dtype=np.float32))
    from ame_amd import gof as G
    center = G.center32(raw0["node"], n)
    raw = R.raw_sums(Yd, center)
    for v in (Yt, center, *raw.values()):
        v.setflags(write=False)
    return Yt, Yd, center, raw


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_moments_within_reassociation_bound(gpu_device, case, kind):
    n, T, _ = case
    Yt, _, _, raw = _net(case, kind)
    D = _Device(case)
    node, sl = D.moments(D.up(Yt))
    b = R.moment_bounds(raw, n)
    en, es = np.abs(node.cpu().numpy() - raw["node"]), np.abs(sl.cpu().numpy() - raw["slice"])
    print(f"moments {case} {kind}: worst error / bound node {np.max(en / np.maximum(b['node'], 1e-300)):.3g} "
          f"slice {np.max(es / np.maximum(b['slice'], 1e-300)):.3g}")
    assert np.all(en <= b["node"]) and np.all(es <= b["slice"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_triads_within_derived_bound(gpu_device, case, kind):
    n, T, _ = case
    Yt, _, center, raw = _net(case, kind)
    D = _Device(case)
    tri = D.triads(D.up(Yt), D.up(center)).cpu().numpy()
    if n < 3:
        return
    bound = R.triad_bounds(raw, n)
    err = np.abs(tri - raw["tri"])
    print(f"triads {case} {kind}: worst error / bound {np.max(err / bound):.3g}")
    assert np.all(np.isfinite(tri)) and np.all(err <= bound)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_moments_and_triads_bits_do_not_depend_on_split_or_run(gpu_device, case):
    n, T, _ = case
    Yt, _, center, _ = _net(case, "plain")
    D = _Device(case)
    y, c = D.up(Yt), D.up(center)
    node, sl = D.moments(y)
    tri = D.triads(y, c)
    node2, sl2 = D.moments(y)
    tri2 = D.triads(y, c)
    for a, b in ((node, node2), (sl, sl2), (tri, tri2)):
        assert np.array_equal(_bits(a), _bits(b))
    for t0, t1 in ((0, 1), (1, T)):
        if t1 <= t0:
            continue
        pn, ps = D.moments(y[t0:t1])
        pt = D.triads(y[t0:t1], c[t0:t1].contiguous())
        assert np.array_equal(_bits(pn), _bits(node[t0:t1]))
        assert np.array_equal(_bits(ps), _bits(sl[t0:t1]))
        assert np.array_equal(_bits(pt), _bits(tri[t0:t1]))


@functools.lru_cache(maxsize=None)
def _sim(case, zero_states=False):
    n, T, r = case
    x = R.make_states(n, T, r, 2000 + n)
    if zero_states:
        x = np.zeros_like(x)
    ref = R.simulate(x, CHOL, SEED, SAMPLE, T_BEGIN)
    x.setflags(write=False)
    return x, ref


def test_noise_deviation_is_within_the_measured_margin(gpu_device):
    """With zero states the output is the noise alone: the largest |got - fp64| /
    (|l| (1 + |z|)) over CASES is printed, and stays within NOISE_REL (4 x the
    figure measured when the test was written)."""
    worst = 0.0
    for case in CASES:
        n, T, r = case
        x, ref = _sim(case, True)
        D = _Device(case)
        got = R.unpack(D.simulate(D.up(x)).cpu().numpy(), n).astype(np.float64)
        unit = R.simulate_bounds(ref, r, CHOL, 1.0)      # mu_abs = 0: the noise scale alone
        up = np.triu(np.ones((n, n), dtype=bool), 1)[None, :, :, None] & np.ones(got.shape, dtype=bool)
        worst = max(worst, float(np.max(np.abs(got - ref["Y"])[up] / unit[up])))
    print(f"simulate noise: largest |got - fp64| / (|l| (1 + |z|)) = {worst:.3e}")
    assert worst <= NOISE_REL


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_simulate_matches_reference_and_layout(gpu_device, case):
    n, T, r = case
    x, ref = _sim(case)
    D = _Device(case)
    xd = D.up(x)
    out = D.simulate(xd)
    packed = out.cpu().numpy()
    assert not np.isnan(packed).any()                     # every element of Yt_out is written
    got = R.unpack(packed, n)
    assert np.all(packed[:, :, n:] == 0.0)                # the pad pair
    assert np.all(got[:, np.arange(n), np.arange(n)] == 0.0)
    assert np.array_equal(got[..., 0].view(np.int32), np.swapaxes(got[..., 1], 1, 2).copy().view(np.int32))
    bound = R.simulate_bounds(ref, r, CHOL, NOISE_REL)
    err = np.abs(got.astype(np.float64) - ref["Y"])
    off = ~np.eye(n, dtype=bool)
    print(f"simulate {case}: worst error / bound {np.max(err[:, off] / bound[:, off]):.3g}")
    assert np.all(err <= bound)
    # the counter names the dyad: any split with the matching t_begin, and a second run
    assert np.array_equal(_bits(D.simulate(xd)), _bits(out))
    if T > 1:
        a = D.simulate(xd[:1].contiguous(), t_begin=T_BEGIN)
        b = D.simulate(xd[1:].contiguous(), t_begin=T_BEGIN + 1)
        assert np.array_equal(_bits(a), _bits(out[:1])) and np.array_equal(_bits(b), _bits(out[1:]))
    # another sample, seed or slice index changes every pair
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    for kw in (dict(sample=SAMPLE + 1), dict(seed=SEED + 1), dict(seed=SEED ^ (1 << 40)), dict(t_begin=T_BEGIN + 1)):
        other = R.unpack(D.simulate(xd, **kw).cpu().numpy(), n)
        assert np.all((other != got)[:, up])
    # lr = 0: the mean alone
    mean = R.unpack(D.simulate(xd, chol=(0.0, 0.0, 0.0)).cpu().numpy(), n).astype(np.float64)
    ref0 = R.simulate(x, (0.0, 0.0, 0.0), SEED, SAMPLE, T_BEGIN)
    assert np.all(np.abs(mean - ref0["Y"]) <= R.simulate_bounds(ref0, r, (0.0, 0.0, 0.0), 0.0))


# ---------------------------------------------------------------------------
# the VI layer
# ---------------------------------------------------------------------------
E2E = (48, 3, 2)


def _model(covariates=False, seed=31):
    import torch
    import covar_ref as CR
    from ame_amd import TemporalAMEModel
    n, T, r = E2E
    m = TemporalAMEModel(n, T, r, seed=seed)
    if covariates:
        m.set_covariates(torch.from_numpy(CR.make_w(n, T, 2, seed=seed)), beta=(0.5, -0.3))
    m.generate_data_fast(seed=seed + 1)
    return m


def _vi(model, lr=0.5, **kw):
    import torch
    from ame_amd import TemporalAMEStructuredMFVI
    return TemporalAMEStructuredMFVI(model, factorization="good", learning_rate=lr,
                                     device=torch.device("cuda", 0), **kw)


def _chol(model):
    Rm = model.R.detach().double().numpy()
    L = np.linalg.cholesky(0.5 * (Rm + Rm.T))
    return (float(L[0, 0]), float(L[1, 0]), float(L[1, 1]))


def _check_statistics(got, Yt_dev, center, n, what):
    """got (T, 5) against the fp64 statistics of the packed device network, within
    the propagated moment and triad bounds; the centre within one fp32 rounding
    of the mean."""
    Yd = R.unpack(Yt_dev.cpu().numpy(), n).astype(np.float64)
    raw = R.raw_sums(Yd, center)
    bm, bt = R.moment_bounds(raw, n), R.triad_bounds(raw, n)
    worst = 0.0
    for t in range(Yd.shape[0]):
        want = R.statistics_from_raw(raw["node"][t], raw["slice"][t], raw["tri"][t], n)
        direct = R.direct_statistics(Yd[t, :, :, 0], center=center[t])
        tol = R.statistic_bounds(raw["node"][t], raw["slice"][t], raw["tri"][t], n, bm["node"][t],
                                 bm["slice"][t], bt[t])
        assert abs(float(center[t]) - want["mean"]) <= 2.0 ** -24 * abs(want["mean"]) * 1.0000001 + 1e-300
        for q, k in enumerate(R.NAMES):
            assert abs(want[k] - direct[k]) <= tol[k], (what, t, k)      # the two reference forms
            err = abs(got[t, q] - want[k])
            worst = max(worst, err / tol[k])
            assert err <= tol[k], (what, t, k, got[t, q], want[k], tol[k])
    return worst


@pytest.mark.parametrize("covariates", (False, True), ids=("plain", "covariates"))
def test_gof_matches_reference_pipeline(gpu_device, covariates):
    import torch
    n, T, r = E2E
    m = _model(covariates)
    vi = _vi(m)
    vi.fit(max_iter=3, tolerance=0.0, verbose=False)
    eng = vi.engine
    # the observed network: model.Y, or the residual the fit reads
    obs = vi.network_statistics()
    assert set(obs) == set(R.NAMES) | {"mean", "sd"} and all(v.shape == (T,) for v in obs.values())
    Yfit = R.unpack(eng.Yt.cpu().numpy(), n)
    Yexp = m.Y.detach().double().numpy()
    if covariates:
        Yexp = Yexp - np.einsum("k,kijtc->ijtc", m.beta.detach().double().numpy(), m.W.detach().double().numpy())
    Yexp = np.transpose(Yexp, (2, 0, 1, 3))
    off = ~np.eye(n, dtype=bool)
    assert np.all(np.abs(Yfit - Yexp)[:, off] <= 2.0 ** -23 * (np.abs(Yexp)[:, off] + 1.0))
    raw_obs = eng.net_statistics(eng.Yt)
    from ame_amd import gof as G
    worst = _check_statistics(G.stack(obs), eng.Yt, raw_obs["center"].cpu().numpy(), n, "observed")

    S, _ = R.gof_states(5, n, T, r, n_sim=8)
    seed = 1234567
    res = vi.gof(states=torch.from_numpy(S), seed=seed)
    assert tuple(res["names"]) == R.NAMES
    assert res["observed"].shape == (T, 5) and res["simulated"].shape == (8, T, 5) and res["quantile"].shape == (T, 5)
    assert np.array_equal(res["observed"], G.stack(obs))
    assert np.array_equal(res["quantile"], (res["simulated"] <= res["observed"][None]).mean(axis=0))
    chol = _chol(m)
    for k in range(8):
        xk = torch.from_numpy(np.ascontiguousarray(S[k].transpose(1, 0, 2))).to(eng.dev)
        Yk = eng.simulate(xk, chol, seed, k)                              # the network gof() reduced
        ref = R.simulate(S[k].transpose(1, 0, 2), chol, seed, k)
        got = R.unpack(Yk.cpu().numpy(), n).astype(np.float64)
        assert np.all(np.abs(got - ref["Y"]) <= R.simulate_bounds(ref, r, chol, NOISE_REL)), k
        ck = eng.net_statistics(Yk)["center"].cpu().numpy()
        worst = max(worst, _check_statistics(res["simulated"][k], Yk, ck, n, f"simulation {k}"))
        # and the reference pipeline's own statistics are close: same model, same noise
        mine = R.direct_statistics(ref["Y"][0, :, :, 0])
        assert abs(mine["dyad_dep"] - res["simulated"][k, 0, 2]) < 1e-4
    print(f"gof statistics: worst error / bound {worst:.3g}")
    mean_only = vi.gof(states=torch.from_numpy(S[:2]), seed=seed, include_noise=False)
    ref0 = R.simulate(S[0].transpose(1, 0, 2), (0.0, 0.0, 0.0), seed, 0)
    d0 = R.direct_statistics(ref0["Y"][1, :, :, 0])
    assert abs(mean_only["simulated"][0, 1, 3] - d0["cycle_dep"]) < 1e-4 * (1 + abs(d0["cycle_dep"]))
    assert not np.array_equal(mean_only["simulated"], res["simulated"][:2])


def test_sample_states_moments_and_seed(gpu_device):
    from ame_amd import TemporalAMEModel
    n, T, r, n_sim = 6, 2, 1, 4096
    m = TemporalAMEModel(n, T, r, seed=8)
    m.generate_data_fast(seed=9)
    vi = _vi(m)
    vi.fit(max_iter=3, tolerance=0.0, verbose=False)
    X = vi.sample_states(n_sim, seed=17)
    assert tuple(X.shape) == (n_sim, n, T, 2 + 2 * r)
    assert np.array_equal(X.numpy(), vi.sample_states(n_sim, seed=17).numpy())
    assert not np.array_equal(X.numpy(), vi.sample_states(n_sim, seed=18).numpy())
    x = X.double().numpy()
    mean, cov = vi.X_mean.double().numpy(), vi.X_cov.double().numpy()
    sd = np.sqrt(np.einsum("ntii->nti", cov))
    assert np.all(np.abs(x.mean(axis=0) - mean) <= 6 * sd / math.sqrt(n_sim))
    c = np.einsum("knti,kntj->ntij", x - mean, x - mean) / n_sim
    # Var of a sample covariance entry of a Gaussian: (S_ii S_jj + S_ij^2) / n_sim
    se = np.sqrt((sd[..., :, None] ** 2 * sd[..., None, :] ** 2 + cov ** 2) / n_sim)
    assert np.all(np.abs(c - cov) <= 6 * se)


def test_smoothed_gof_and_sensitivity_to_the_multiplicative_term(gpu_device):
    import torch
    n, T, r = E2E
    vi = _vi(_model())
    vi.fit(max_iter=3, tolerance=0.0, verbose=False)
    a = vi.gof(n_sim=3, seed=2)
    b = vi.gof(n_sim=3, seed=2, smoothed=True)
    assert np.all(np.isfinite(a["simulated"])) and np.all(np.isfinite(b["simulated"]))
    assert not np.array_equal(a["simulated"], b["simulated"])
    assert np.array_equal(a["simulated"], vi.gof(n_sim=3, seed=2)["simulated"])
    S, S0 = R.gof_states(R.GOF_SENSITIVITY_SEED, n, T, r)
    full = vi.gof(states=torch.from_numpy(S), seed=R.GOF_SENSITIVITY_SEED)["simulated"]
    flat = vi.gof(states=torch.from_numpy(S0), seed=R.GOF_SENSITIVITY_SEED)["simulated"]
    assert np.all(np.abs(flat[..., 3]) < np.abs(full[..., 3]))
    assert np.all(np.abs(flat[..., 4]) < np.abs(full[..., 4]))


def test_refusals_and_the_fit_is_untouched(gpu_device):
    import torch
    import missing_ref as MR
    n, T, r = E2E
    with pytest.raises(NotImplementedError, match="time-sharded"):
        _vi(_model(), distributed=True).gof(n_sim=1)
    with pytest.raises(NotImplementedError, match="time-sharded"):
        _vi(_model(), distributed=True).network_statistics()
    m = _model()
    m.set_missing(torch.from_numpy(MR.random_mask(n, T, 0.2)))
    with pytest.raises(NotImplementedError, match="missing"):
        _vi(m).gof(n_sim=1)
    with pytest.raises(NotImplementedError, match="missing"):
        _vi(m).network_statistics()
    m = _model()
    m.Y[1, 2, 0, 0] += 1.0            # Y[2, 1] no longer the swap of Y[1, 2]
    with pytest.raises(ValueError, match="swap-consistent"):
        _vi(m).network_statistics()
    with pytest.raises(ValueError, match="swap-consistent"):
        _vi(m).gof(n_sim=1)
    with pytest.raises(ValueError, match="states"):
        _vi(_model()).gof(states=torch.zeros(2, n, T, 3))
    # a fit with the calls in its middle ends where a fit without them ends
    one, two = _vi(_model()), _vi(_model())
    for vi in (one, two):
        vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    before = one.X_mean.clone()
    one.network_statistics()
    one.gof(n_sim=2, seed=4)
    one.gof(n_sim=1, seed=4, smoothed=True)
    one.sample_states(3, seed=1)
    assert torch.equal(one.X_mean, before)
    for vi in (one, two):
        vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    assert torch.equal(one.X_mean, two.X_mean) and torch.equal(one.X_cov, two.X_cov)
