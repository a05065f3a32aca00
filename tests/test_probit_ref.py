"""The fp64 reference of the probit scheme (tests/probit_ref.py), on the CPU:
the bound against the exact orthant probability, the normal-distribution
functions over [-40, 40], and the quality of the scheme against the +-1 coding
and against E[z] written into both rows (DESIGN.md §7i records the figures).
"""
import math

import numpy as np
import pytest

import probit_ref as BR


def _exact_log_orthant(m, s, rho):
    """log P(s_a z_a > 0, a = 0, 1) for z ~ N(m, [[1, rho], [rho, 1]])."""
    from scipy.stats import multivariate_normal as mvn
    D = np.diag(-np.asarray(s, float))
    R = np.array([[1.0, rho], [rho, 1.0]])
    return math.log(mvn(mean=D @ m, cov=D @ R @ D).cdf(np.zeros(2)))


def test_bound_is_below_the_exact_orthant_probability():
    rng = np.random.default_rng(0)
    worst = -np.inf
    for _ in range(300):
        rho = rng.uniform(-0.9, 0.9)
        m = rng.normal(0.0, 1.5, 2)
        s = rng.choice([-1.0, 1.0], 2)
        l = float(BR.bound(m, s, rho, K=2))
        exact = _exact_log_orthant(m, s, rho)
        worst = max(worst, l - exact)
        # mvn.cdf integrates numerically: its default absolute error is 1e-5 on the probability
        assert l <= exact + 2e-5 / math.exp(exact), (rho, m, s, l, exact)
    print(f"max(l - exact) over 300 draws = {worst:.3e}")


def test_bound_at_rho_zero_is_the_sum_of_log_phi():
    rng = np.random.default_rng(1)
    m = rng.normal(0.0, 2.0, (200, 2))
    s = rng.choice([-1.0, 1.0], (200, 2))
    want = BR.log_phi(s * m).sum(-1)
    for K in (1, 2, 3):
        got = BR.bound(m, s, 0.0, K=K)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), K
    # and the correction is s kappa(s m): E[z] of the unit-variance truncated normal
    e, _, _ = BR.recursion(m, s, 0.0)
    assert np.abs(e - (m + s * BR.kappa(s * m))).max() <= 1e-14


def test_kappa_and_log_phi_are_finite_and_monotone():
    x = np.linspace(-40.0, 40.0, 16001)
    k, l = BR.kappa(x), BR.log_phi(x)
    assert np.isfinite(k).all() and np.isfinite(l).all()
    assert (k >= 0).all() and (np.diff(k) <= 0).all()          # the inverse Mills ratio falls
    assert (l <= 0).all() and (np.diff(l) >= 0).all()
    from scipy.special import log_ndtr
    assert np.abs(l - log_ndtr(x)).max() <= 1e-12 * np.abs(log_ndtr(x)).max() + 1e-15
    # both branches of log Phi meet at 0, and kappa's tails: -x - 1 / x and phi(x)
    assert abs(float(BR.log_phi(-1e-300)) - float(BR.log_phi(0.0))) <= 1e-15
    assert abs(float(BR.kappa(-40.0)) - (40.0 + 1.0 / 40.0)) < 1e-3 and float(BR.kappa(40.0)) == 0.0


@pytest.mark.parametrize("rho", (0.0, 0.5))
def test_scheme_beats_the_pm1_coding_on_held_out_links(rho):
    own = BR.quality_case(rho, "own")
    pm1 = BR.quality_case(rho, "pm1")
    print(f"rho={rho}: held-out mean log score own {own['held_out']:.4f} pm1 {pm1['held_out']:.4f}; "
          f"corr own {own['corr']:.3f} pm1 {pm1['corr']:.3f}; mean|mu| own {own['abs_mu']:.3f} "
          f"pm1 {pm1['abs_mu']:.3f} truth {own['abs_true']:.3f}")
    assert own["diverged"] is None and pm1["diverged"] is None
    assert own["held_out"] > pm1["held_out"]


def test_expected_z_in_both_rows_diverges():
    ez = BR.quality_case(0.0, "ez")
    print(f"E[z] in both rows: mean|mu| {ez['abs_mu']:.2f} held-out {ez['held_out']:.2f} diverged {ez['diverged']}")
    assert ez["diverged"] is not None or ez["abs_mu"] > 5.0


def test_working_network_of_a_hidden_pair_is_the_own_perspective_mean():
    import missing_ref as MR
    rng = np.random.default_rng(3)
    n, T, r = 7, 2, 2
    X = rng.normal(0, 0.7, (n, T, 2 + 2 * r))
    B = rng.random((n, n, T)) < 0.4
    mask = MR.random_mask(n, T, 0.3, seed=1)
    Yw = BR.working_network(X, B, mask, 0.5)
    own = MR.own_fill(np.zeros((n, n, T, 2)), X, np.ones((n, n, T), bool))
    h = MR.clean(mask)
    assert np.array_equal(Yw[h], own[h])
    off = ~h & ~np.eye(n, dtype=bool)[:, :, None]
    # at rho = 0 an observed entry is pushed to the side of its tie: d has the sign s
    s = np.where(BR.y_of(B) > 0, 1.0, -1.0)
    assert ((BR.working_network(X, B, mask, 0.0) - own)[off] * s[off] > 0).all()
    # the two rows of a pair carry the same correction, swapped
    d = Yw - own
    od = ~np.eye(n, dtype=bool)
    assert np.allclose(d[..., 0][od], d.transpose(1, 0, 2, 3)[..., 1][od], atol=1e-15)
    rows, mag = BR.stat_rows(X, B, mask, 0.5)
    assert np.array_equal(rows[:, 0], n * (n - 1) // 2 - MR.pack(mask)[1].astype(float))
    assert (mag[:, 1] >= np.abs(rows[:, 1])).all() and (rows[:, 2] > 0).all()
