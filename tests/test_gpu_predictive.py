"""ame_predict on the GPU (posterior-predictive dyad moments, scoring sums,
forecasts) against the fp64 reference tests/predictive_ref.py.

Elementwise tolerance.  predictive_ref.DELTA0 = 2.3e-6 is the largest error of
an np.float32 evaluation of the same formulas (products and sums one after
another) against the fp64 reference over the inputs used here (measured 2.366e-6
at (65, 2, 31), re-measured by tests/test_predictive_ref.py), relative to the
dyad's sum of |products|.  The kernel's bound is TOL = 4 x DELTA0 = 9.2e-6 of
that sum (the margin is for the MFMA chain's different summation order over up
to ~2200 terms).  Sums of non-negative summands (slots 2-8) are held to 5e-6
relative and the log score to 5e-6 x sum|summand| (the fp32-vs-fp64 bound of
test_gpu_parity.py); the pair count is exact; every coverage count lies between
the reference's counts at threshold x (1 -+ 4 TOL).
"""
import functools

import numpy as np
import pytest

import predictive_ref as R

pytestmark = pytest.mark.gpu

LEVELS = (0.5, 0.9, 0.95)
IDS = lambda s: "n%d_T%d_r%d" % s


def _model(n, T, r):
    from ame_amd import TemporalAMEModel
    m = TemporalAMEModel(n, T, r, seed=5)
    m.generate_data_fast(seed=9)
    if (n, T, r) == (200, 3, 8):   # swap-inconsistent Y, as in test_gpu_pairs.py
        m.Y[1, n - 1, 0, 0] += 0.75
        m.Y[n - 2, 0, T - 1, 1] -= 0.5
    return m


def _reference(X, S, r, Y, noise, levels):
    """Per slice: moments, |product| sums, scores and the 21 sums, in fp64."""
    zsq, csq = R.thresholds(levels)
    out = []
    for t in range(X.shape[1]):
        mean, V0, C01 = R.moments(X[:, t], S[:, t], r)
        sm, sv, sc = R.abs_sums(X[:, t], S[:, t], r)
        d = R.dyad_scores(mean, V0, C01, Y[:, :, t], noise)
        out.append(dict(mean=mean, V0=V0, C01=C01, sm=sm, sv=sv, sc=sc, d=d,
                        sums=R.sums_from_scores(d, zsq, csq)))
    return out


@functools.lru_cache(maxsize=None)
def _case(shape):
    """A "good" instance with the random state of predictive_ref.make_state
    assigned after one fit iteration (the setters' upload path), its device
    results and the reference, computed once per shape."""
    import torch
    from ame_amd import TemporalAMEStructuredMFVI
    n, T, r = shape
    m = _model(n, T, r)
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.3,
                                   device=torch.device("cuda", 0))
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    X, S = R.make_state(n, T, r)
    vi.X_mean = torch.from_numpy(X.copy())
    vi.X_cov = torch.from_numpy(S.copy())
    noise = m.R.numpy().astype(np.float64)
    check = vi.predictive_check(levels=LEVELS)
    mean, second = vi.predict_dyads(slice(None))
    ref = _reference(X, S, r, m.Y.numpy(), noise, LEVELS)
    return dict(vi=vi, model=m, X=X, S=S, noise=noise, check=check, mean=mean.numpy(),
                second=second.numpy(), ref=ref)


def _assert_dense(mean, second, ref, noise, n):
    off = ~np.eye(n, dtype=bool)
    dg = np.eye(n, dtype=bool)
    for t, rf in enumerate(ref):
        for c, (want, scale) in enumerate(((rf["mean"][..., 0], rf["sm"]),
                                           (rf["mean"][..., 1], rf["sm"].T))):
            err = np.abs(mean[:, :, t, c] - want) / scale
            print(f"t={t} mean{c}: max err / sum|products| = {err[off].max():.3e}")
            assert err[off].max() <= R.TOL, (t, c, err[off].max())
        for c, (want, scale) in enumerate((
                (rf["V0"] + noise[0, 0], rf["sv"] + abs(noise[0, 0])),
                (rf["V0"].T + noise[1, 1], rf["sv"].T + abs(noise[1, 1])),
                (rf["C01"] + 0.5 * (noise[0, 1] + noise[1, 0]), rf["sc"] + abs(noise[0, 1])))):
            got = second[:, :, t, c]
            assert np.isnan(got[dg]).all(), "diagonal second moments must be NaN"
            assert not np.isnan(got[off]).any()
            err = np.abs(got - want) / scale
            print(f"t={t} second{c}: max err / sum|products| = {err[off].max():.3e}")
            assert err[off].max() <= R.TOL, (t, c, err[off].max())


def _band(values, thr):
    lo = (values <= thr * (1.0 - 4.0 * R.TOL)).sum()
    hi = (values <= thr * (1.0 + 4.0 * R.TOL)).sum()
    return lo, hi


def _assert_sums(check, ref, levels):
    zsq, csq = R.thresholds(levels)
    for t, rf in enumerate(ref):
        s, d = rf["sums"], rf["d"]
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
        print(f"t={t} slot 1: err {abs(got[1] - s[1]):.3e} bound {bound:.3e}")
        assert abs(got[1] - s[1]) <= bound, (t, got[1], s[1])
        for l in range(len(levels)):
            for name, cnt, vals, thr in (
                    ("z0", check["coverage"][t, l, 0] * pairs, d["z2"][:, 0], zsq[l]),
                    ("z1", check["coverage"][t, l, 1] * pairs, d["z2"][:, 1], zsq[l]),
                    ("m2", check["joint_coverage"][t, l] * pairs, d["m2"], csq[l])):
                lo, hi = _band(vals, thr)
                assert lo <= round(cnt) <= hi and abs(cnt - round(cnt)) < 1e-6, (t, l, name, cnt, lo, hi)


@pytest.mark.parametrize("shape", R.GPU_SHAPES + R.GPU_SHAPES_EVERY_R, ids=IDS)
def test_dense_moments_match_reference(shape, gpu_device):
    c = _case(shape)
    n, T, r = shape
    assert c["mean"].shape == (n, n, T, 2) and c["second"].shape == (n, n, T, 3)
    _assert_dense(c["mean"], c["second"], c["ref"], c["noise"], n)
    # the diagonal means are compute_mean's (two fp32 evaluations of one formula)
    import torch
    X = torch.from_numpy(c["X"])
    for t in range(T):
        mu = c["model"].compute_mean(X[:, t, :2], X[:, t, 2:]).numpy()
        for i in range(n):
            for ch in range(2):
                assert abs(c["mean"][i, i, t, ch] - mu[i, i, ch]) <= 2 * R.TOL * c["ref"][t]["sm"][i, i]


@pytest.mark.parametrize("shape", R.GPU_SHAPES, ids=IDS)
def test_noise_adds_exactly_R(shape, gpu_device):
    """include_noise=False differs from True by R's entries, to the fp32
    rounding of the one addition (2^-24 relative, on the sum and on (float) R)."""
    c = _case(shape)
    n = shape[0]
    mean0, second0 = c["vi"].predict_dyads(slice(None), include_noise=False)
    assert np.array_equal(mean0.numpy(), c["mean"])
    off = ~np.eye(n, dtype=bool)
    N = c["noise"]
    for ch, add in enumerate((N[0, 0], N[1, 1], 0.5 * (N[0, 1] + N[1, 0]))):
        a = c["second"][..., ch].astype(np.float64)[off]
        b = second0.numpy()[..., ch].astype(np.float64)[off]
        assert (np.abs(a - b - add) <= 2.0 ** -23 * np.maximum(np.abs(a), abs(add))).all()


@pytest.mark.parametrize("shape", R.GPU_SHAPES + R.GPU_SHAPES_EVERY_R, ids=IDS)
def test_scoring_sums_match_reference(shape, gpu_device):
    c = _case(shape)
    assert c["check"]["levels"] == LEVELS
    assert c["check"]["coverage"].shape == (shape[1], 3, 2)
    assert c["check"]["joint_coverage"].shape == (shape[1], 3)
    _assert_sums(c["check"], c["ref"], LEVELS)


@pytest.mark.parametrize("shape", R.GPU_SHAPES, ids=IDS)
def test_check_is_consistent_with_dense(shape, gpu_device):
    """The coverage counts equal those recomputed on the host from predict_dyads
    and Y, within the threshold band."""
    c = _case(shape)
    n, T, r = shape
    zsq, csq = R.thresholds(LEVELS)
    Y = c["model"].Y.numpy()
    for t in range(T):
        V0 = c["second"][:, :, t, 0].astype(np.float64)
        d = R.dyad_scores(c["mean"][:, :, t].astype(np.float64), V0,
                          c["second"][:, :, t, 2].astype(np.float64), Y[:, :, t], np.zeros((2, 2)))
        pairs = c["check"]["pairs"][t]
        assert pairs == n * (n - 1) // 2
        for l in range(3):
            for cnt, vals, thr in ((c["check"]["coverage"][t, l, 0] * pairs, d["z2"][:, 0], zsq[l]),
                                   (c["check"]["coverage"][t, l, 1] * pairs, d["z2"][:, 1], zsq[l]),
                                   (c["check"]["joint_coverage"][t, l] * pairs, d["m2"], csq[l])):
                lo, hi = _band(vals, thr)
                assert lo <= round(cnt) <= hi, (t, l, cnt, lo, hi)


@pytest.mark.parametrize("shape", [(65, 2, 5), (130, 3, 16)], ids=IDS)
def test_sums_are_deterministic(shape, gpu_device):
    c = _case(shape)
    again = c["vi"].predictive_check(levels=LEVELS)
    for k, v in c["check"].items():
        if k != "levels":
            assert np.array_equal(v, again[k]), k


def test_sub_blocks_and_level_subsets(gpu_device):
    """A dense sub-block equals the same entries of the full block bit for bit;
    unused levels leave their slots zero; include_noise=False changes the sums."""
    c = _case((130, 3, 16))
    vi = c["vi"]
    mean, second = vi.predict_dyads(1, rows=range(60, 101), cols=slice(3, 70))
    assert mean.shape == (41, 67, 1, 2) and second.shape == (41, 67, 1, 3)
    assert np.array_equal(mean.numpy()[:, :, 0], c["mean"][60:101, 3:70, 1])
    assert np.array_equal(second.numpy()[:, :, 0], c["second"][60:101, 3:70, 1], equal_nan=True)
    one = vi.predictive_check(levels=(0.9,))
    assert one["coverage"].shape == (3, 1, 2)
    assert np.array_equal(one["coverage"][:, 0], c["check"]["coverage"][:, 1])
    assert np.array_equal(one["log_score"], c["check"]["log_score"])
    # a scratch budget of one slice per call (chunked launches) changes nothing
    eng = vi.engine
    budget = eng.PREDICT_WORK_DOUBLES
    try:
        eng.PREDICT_WORK_DOUBLES = 1
        chunked = vi.predictive_check(levels=LEVELS)
        mean_c, second_c = vi.predict_dyads(slice(None))
    finally:
        eng.PREDICT_WORK_DOUBLES = budget
    for k, v in c["check"].items():
        if k != "levels":
            assert np.array_equal(v, chunked[k]), k
    assert np.array_equal(mean_c.numpy(), c["mean"])
    assert np.array_equal(second_c.numpy(), c["second"], equal_nan=True)
    none = vi.predictive_check(levels=(), include_noise=False)
    assert none["coverage"].shape == (3, 0, 2)
    assert (none["mean_var"] < c["check"]["mean_var"]).all()
    with pytest.raises(ValueError):
        vi.predictive_check(levels=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError):
        vi.predictive_check(levels=(1.0,))
    with pytest.raises(ValueError):
        vi.predict_dyads(slice(None), max_elements=1000)
    with pytest.raises(ValueError):
        vi.predict_dyads(0, rows=range(0, 131))


@pytest.mark.parametrize("method", ["bad", "naive"])
def test_fitted_bad_and_naive_states(method, gpu_device):
    """The kernel is variant-agnostic: the fitted covariances of the bad and
    naive factorisations (zero blocks) against the reference on the same state."""
    import torch
    from ame_amd import TemporalAMENaiveMFVI, TemporalAMEStructuredMFVI
    n, T, r = 65, 2, 5
    m = _model(n, T, r)
    dev = torch.device("cuda", 0)
    if method == "naive":
        vi = TemporalAMENaiveMFVI(m, learning_rate=0.3, device=dev)
    else:
        vi = TemporalAMEStructuredMFVI(m, factorization="bad", learning_rate=0.3, device=dev)
    vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    X, S = vi.X_mean.numpy().copy(), vi.X_cov.numpy().copy()
    noise = m.R.numpy().astype(np.float64)
    ref = _reference(X, S, r, m.Y.numpy(), noise, LEVELS)
    mean, second = vi.predict_dyads(slice(None))
    _assert_dense(mean.numpy(), second.numpy(), ref, noise, n)
    _assert_sums(vi.predictive_check(levels=LEVELS), ref, LEVELS)


def test_check_does_not_disturb_fit(gpu_device):
    """fit -> predictive_check -> fit gives bit-equal means to fit -> fit."""
    import torch
    from ame_amd import TemporalAMEStructuredMFVI

    def run(check):
        m = _model(40, 4, 3)
        vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.5,
                                       device=torch.device("cuda", 0))
        vi.fit(max_iter=3, tolerance=0.0, verbose=False)
        if check:
            vi.predictive_check()
            vi.predict_dyads(0)
            vi.forecast_dyads(2)
        vi.fit(max_iter=3, tolerance=0.0, verbose=False)
        return vi.X_mean.numpy().copy(), vi.X_cov.numpy().copy()

    a, b = run(True), run(False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _forecast_vi(method, n=20, T=3, r=4):
    import torch
    from ame_amd import TemporalAMEModel, TemporalAMENaiveMFVI, TemporalAMEStructuredMFVI
    m = TemporalAMEModel(n, T, r, seed=3)
    g = torch.Generator().manual_seed(1)
    m.Phi = m.Phi + 0.02 * torch.randn(m.d, m.d, generator=g)   # asymmetric transition
    m.generate_data_fast(seed=2)
    dev = torch.device("cuda", 0)
    if method == "naive":
        vi = TemporalAMENaiveMFVI(m, learning_rate=0.3, device=dev)
    else:
        vi = TemporalAMEStructuredMFVI(m, factorization=method, learning_rate=0.3, device=dev)
    vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    return m, vi


def test_forecast_matches_recursion(gpu_device):
    m, vi = _forecast_vi("good")
    Xp, Sp = vi.forecast(3)
    assert tuple(Xp.shape) == (m.n, 3, m.d) and tuple(Sp.shape) == (m.n, 3, m.d, m.d)
    Xr, Sr = R.forecast(vi.X_mean.numpy()[:, -1], vi.X_cov.numpy()[:, -1], m.Phi.numpy(), m.Q.numpy(), 3)
    em = np.abs(Xp.numpy() - Xr).max()
    es = np.abs(Sp.numpy() - Sr).max()
    print(f"forecast: max|dm| {em:.3e}, max|dS| {es:.3e}")
    assert em <= 2e-6 * max(1.0, np.abs(Xr).max())
    assert es <= 1e-6 * max(1.0, np.abs(Sr).max())


def test_forecast_check_equals_host_scoring_of_forecast_dyads(gpu_device):
    import torch
    m, vi = _forecast_vi("good")
    h, n = 3, m.n
    Xp, _ = vi.forecast(h)
    g = torch.Generator().manual_seed(7)
    LR = torch.linalg.cholesky(m.R)
    Yf = torch.zeros(n, n, h, 2)
    for k in range(h):   # drawn from the model around the forecast means
        Yf[:, :, k] = m.compute_mean(Xp[:, k, :2], Xp[:, k, 2:]) + torch.randn(n, n, 2, generator=g) @ LR.T
    chk = vi.forecast_check(Yf, levels=LEVELS)
    mean, second = vi.forecast_dyads(h)
    assert mean.shape == (n, n, h, 2) and second.shape == (n, n, h, 3)
    zsq, csq = R.thresholds(LEVELS)
    ref = []
    for k in range(h):
        d = R.dyad_scores(mean.numpy()[:, :, k].astype(np.float64),
                          second.numpy()[:, :, k, 0].astype(np.float64),
                          second.numpy()[:, :, k, 2].astype(np.float64), Yf.numpy()[:, :, k],
                          np.zeros((2, 2)))
        ref.append(dict(d=d, sums=R.sums_from_scores(d, zsq, csq)))
    assert chk["pairs"].shape == (h,)
    _assert_sums(chk, ref, LEVELS)


def test_naive_forecast_agrees_with_predict_forward(gpu_device):
    m, vi = _forecast_vi("naive")
    want = vi.predict_forward(2).numpy()
    got = vi.forecast(2)[0].numpy()
    assert np.abs(got - want).max() <= 2e-6 * max(1.0, np.abs(want).max())


def test_capi_argument_errors(gpu_device):
    """Every listed misuse returns negative with a message, before any launch."""
    import torch
    from test_predict_capi import check_argument_errors
    check_argument_errors()
    torch.cuda.synchronize()   # nothing was queued that could fault
