"""CPU checks of tests/predictive_ref.py, the fp64 reference the GPU tests of
ame_predict compare with: (a) its closed forms against Monte Carlo, (b) the GPU
tests' inputs make every term of V0 and C01 visible above the comparison
tolerance, (c) the forecast recursion against a direct Phi^h evaluation.

The elementwise tolerance of the GPU tests (tests/test_gpu_predictive.py) is
derived here: DELTA0 is the largest error, over the GPU tests' inputs and
dyads, of an np.float32 evaluation of the formulas (products and sums one after
another) against the fp64 reference, relative to the dyad's sum of |products|;
the kernel's bound is 4 x DELTA0.  Measured: 2.366e-6 (at (65, 2, 31)); the
constant predictive_ref.DELTA0 = 2.3e-6 rounds it down, bound 9.2e-6.
"""
import functools

import numpy as np
import pytest

import predictive_ref as R


DELTA0_SHAPES = R.GPU_SHAPES + R.GPU_SHAPES_EVERY_R


@functools.lru_cache(maxsize=None)
def delta0():
    """Largest fp32-vs-fp64 relative error over the GPU tests' inputs."""
    worst = 0.0
    for n, T, r in DELTA0_SHAPES:
        m, S = R.make_state(n, T, r)
        for t in range(T):
            worst = max(worst, R.f32_relative_error(m[:, t], S[:, t], r))
    return worst


def test_monte_carlo_pins_closed_forms():
    """(a) n = 3, r = 2: mean, V0, C01 of every dyad within 6 standard errors
    of their Monte Carlo estimates (standard error from the same sample)."""
    n, r, N = 3, 2, 400_000
    d = 2 + 2 * r
    rng = np.random.default_rng(11)
    m = rng.standard_normal((n, d))
    A = rng.standard_normal((n, d, d))
    S = 0.3 * A @ np.swapaxes(A, 1, 2) + 0.1 * np.eye(d)
    mean, V0, C01 = R.moments(m, S, r)
    Lc = np.linalg.cholesky(S)
    x = m[None] + np.einsum("nkl,snl->snk", Lc, rng.standard_normal((N, n, d)))
    a, b, U, V = x[..., 0], x[..., 1], x[..., 2:2 + r], x[..., 2 + r:]
    checked = 0
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            mu0 = a[:, i] + b[:, j] + (U[:, i] * V[:, j]).sum(-1)
            mu1 = a[:, j] + b[:, i] + (U[:, j] * V[:, i]).sum(-1)
            for name, stat, want in (
                    ("mean0", mu0, mean[i, j, 0]), ("mean1", mu1, mean[i, j, 1]),
                    ("V0", (mu0 - mean[i, j, 0]) ** 2, V0[i, j]),
                    ("V0'", (mu1 - mean[i, j, 1]) ** 2, V0[j, i]),
                    ("C01", (mu0 - mean[i, j, 0]) * (mu1 - mean[i, j, 1]), C01[i, j])):
                se = stat.std(ddof=1) / np.sqrt(N)
                assert abs(stat.mean() - want) <= 6.0 * se, (i, j, name, stat.mean(), want, se)
                checked += 1
    assert checked == 5 * n * (n - 1)
    # C01 is symmetric in (i, j)
    np.testing.assert_allclose(C01, C01.T, rtol=1e-12, atol=1e-12)


_DROPS = [(k,) for k in R.V0_TERMS + R.C01_TERMS] + list(R.GROUPS.values())


@pytest.mark.parametrize("shape", R.GPU_SHAPES, ids=lambda s: "n%d_T%d_r%d" % s)
def test_gpu_inputs_show_every_term(shape):
    """(b) On the GPU tests' inputs, leaving out any single term (and any of the
    issue's term groups) moves V0 or C01 by more than 100 x the elementwise
    tolerance (4 x DELTA0 x sum|products|) for at least half the dyads i != j."""
    n, T, r = shape
    tol = R.TOL
    m, S = R.make_state(n, T, r)
    off = ~np.eye(n, dtype=bool)
    for t in range(T):
        _, V0, C01 = R.moments(m[:, t], S[:, t], r)
        _, sv, sc = R.abs_sums(m[:, t], S[:, t], r)
        for drop in _DROPS:
            _, V0d, C01d = R.moments(m[:, t], S[:, t], r, drop=drop)
            if drop[0] in R.V0_TERMS:
                moved = np.abs(V0d - V0) > 100.0 * tol * sv
            else:
                moved = np.abs(C01d - C01) > 100.0 * tol * sc
            frac = moved[off].mean()
            assert frac >= 0.5, (shape, t, drop, frac)


def test_delta0_is_what_the_documents_quote():
    d0 = delta0()
    print(f"DELTA0 = {d0:.3e}, kernel bound 4 x DELTA0 = {4 * d0:.3e}")
    # the constant the GPU tests use is never wider than what was measured
    assert R.DELTA0 <= d0 <= 1.1 * R.DELTA0
    assert R.TOL == 4.0 * R.DELTA0


def test_forecast_recursion_matches_direct_powers():
    """(c) m_k = Phi m_{k-1}, S_k = Phi S_{k-1} Phi' + Q against Phi^k in closed form,
    with an asymmetric Phi."""
    n, r, h = 4, 3, 5
    d = 2 + 2 * r
    rng = np.random.default_rng(5)
    Phi = 0.7 * np.eye(d) + 0.1 * rng.standard_normal((d, d))
    B = rng.standard_normal((d, d))
    Q = 0.05 * B @ B.T + 0.01 * np.eye(d)
    m = rng.standard_normal((n, d))
    A = rng.standard_normal((n, d, d))
    S = 0.3 * A @ np.swapaxes(A, 1, 2) + 0.1 * np.eye(d)
    Xp, Sp = R.forecast(m, S, Phi, Q, h)
    assert Xp.shape == (n, h, d) and Sp.shape == (n, h, d, d)
    for k in range(1, h + 1):
        mk, Sk = R.forecast_direct(m, S, Phi, Q, k)
        np.testing.assert_allclose(Xp[:, k - 1], mk, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(Sp[:, k - 1], Sk, rtol=1e-12, atol=1e-12)


def test_scoring_sums_against_scipy_free_formula():
    """The scoring sums: log density and Mahalanobis distance of each pair from
    numpy's own 2 x 2 inverse / determinant, counts at the chi-square thresholds."""
    n, r = 5, 2
    m, S = R.make_state(n, 1, r, seed=3)
    m, S = m[:, 0], S[:, 0]
    rng = np.random.default_rng(2)
    Y = rng.standard_normal((n, n, 2))
    N = np.array([[0.1, 0.05], [0.05, 0.1]])
    zsq, csq = R.thresholds((0.5, 0.9))
    assert abs(zsq[1] - 1.6448536269514722 ** 2) < 1e-12 and abs(csq[0] - 2 * np.log(2)) < 1e-12
    sums, _ = R.score_slice(m, S, r, Y, N, zsq, csq)
    mean, V0, C01 = R.moments(m, S, r)
    want = np.zeros(R.N_SUMS)
    for i in range(n):
        for j in range(i + 1, n):
            Sg = np.array([[V0[i, j], C01[i, j]], [C01[i, j], V0[j, i]]]) + N
            e = Y[i, j] - mean[i, j]
            m2 = e @ np.linalg.inv(Sg) @ e
            z = e ** 2 / np.diag(Sg)
            want[0] += 1
            want[1] += -0.5 * (np.log(np.linalg.det(Sg)) + m2 + 2 * R.LOG2PI)
            want[2] += m2
            want[3:5] += z
            want[5:7] += np.diag(Sg)
            want[7:9] += e ** 2
            for l in range(2):
                want[9 + 3 * l:11 + 3 * l] += z <= zsq[l]
                want[11 + 3 * l] += m2 <= csq[l]
    np.testing.assert_allclose(sums, want, rtol=1e-10, atol=1e-10)
