"""The fp64 reference of the probit scheme (tests/probit_ref.py), on the CPU:
the bound against the exact orthant probability, the normal-distribution
functions over [-40, 40], and the quality of the scheme against the +-1 coding
and against E[z] written into both rows (DESIGN.md §7i records the figures).
"""
import math

import numpy as np
import pytest

import missing_ref as MR
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


# ---------------------------------------------------------------------------
# the tail grid (probit_ref.grid_case) against tests/golden/probit_tails.npz
# ---------------------------------------------------------------------------
def _fixture():
    from conftest import golden
    return golden("probit_tails.npz")


def test_grid_is_what_the_fixture_was_made_from():
    fx = _fixture()
    assert int(fx["seed"]) == BR.GRID_SEED and tuple(fx["rhos"]) == BR.GRID_RHOS
    for n in BR.GRID_SHAPES:
        g = BR.grid_case(n, 0.5)
        off = ~np.eye(n, dtype=bool)
        X = g["X"].astype(np.float64)
        assert not X[:, :, 2:].any() and np.abs(X[:, :, :2]).max() <= 19.0
        assert np.array_equal(X[:, :, :2] * 1024, np.round(X[:, :, :2] * 1024))
        m = g["means"]
        assert (m[:, off] != 0).all() and np.array_equal(m.astype(np.float32), m)
        sm = np.where(BR.y_of(g["B"]).transpose(2, 0, 1, 3) > 0, 1.0, -1.0) * m
        for t, (lo, hi) in enumerate(((-3, 3), (-12, -3), (-38, -12), (3, 38))):
            assert lo <= sm[t][off].min() and sm[t][off].max() <= hi
        up = np.triu(off)
        assert (sm[4, ..., 0][up] < 0).all() and (sm[4, ..., 1][up] > 0).all()      # ij against, ji with
        assert sm[4].min() < -20 and sm[4].max() > 20
        got = set(m[5][off].ravel().tolist())
        assert set(BR.GRID_SPECIAL) <= got
        for cov in BR.GRID_COVS:      # V0 = S_aa(row node) in {0, 3} and nothing else
            S = g["S"][cov].astype(np.float64)
            Saa = S[:, :, 0, 0].copy()
            S[:, :, 0, 0] = 0
            assert not S.any() and set(np.unique(Saa)) <= {0.0, 3.0}
        assert g["S"]["scaled"].any() and not g["S"]["unit"].any()
        # the fixture's exact columns
        for name, mask in g["masks"].items():
            hidden = 0 if mask is None else MR.pack(mask)[1].astype(np.float64)
            assert (fx[BR.grid_key(n, 0.5, "stat", name)][:, 0] == n * (n - 1) // 2 - hidden).all()


def test_recipe_regenerates_the_fixture():
    """The whole of n = 20 and, of n = 65, one slice of the fill rows and one of
    the score rows (the recipe takes minutes on all of it): to the last bit."""
    pytest.importorskip("mpmath")
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_probit_tails as G
    fx = _fixture()
    n = BR.GRID_SHAPES[0]
    made = G.score_arrays(n)
    for rho in BR.GRID_RHOS:
        made.update(G.fill_arrays(n, rho))
    assert len(made) == 12 + 5 * len(BR.GRID_RHOS)
    for k, v in made.items():
        assert np.array_equal(v.view(np.uint64), fx[k].view(np.uint64)), k
    n, t = BR.GRID_SHAPES[1], 4
    for k, v in list(G.fill_arrays(n, 0.95, slices=(t,)).items()) + list(G.score_arrays(n, slices=(5,)).items()):
        row = 5 if "score" in k else t
        assert np.array_equal(v[row].view(np.uint64), fx[k][row].view(np.uint64)), k
    names = {k for n in BR.GRID_SHAPES for rho in BR.GRID_RHOS for k in BR.grid_reference(n, rho)}
    assert set(fx.files) == names | {"seed", "rhos"}


def test_reference_stays_within_tail_tau0_of_the_fixture():
    fx = _fixture()
    worst = {}
    for n in BR.GRID_SHAPES:
        for rho in BR.GRID_RHOS:
            for k, dev in BR.grid_deviation(BR.grid_reference(n, rho), fx).items():
                what = k.split("_")[2 if "rho" in k else 1]
                key = (n, rho if "rho" in k else None, what)
                worst[key] = max(worst.get(key, 0.0), float(dev.max()))
    for key, v in sorted(worst.items(), key=str):
        print(f"n={key[0]} rho={key[1]} {key[2]}: scipy reference vs mpmath fixture {v:.3e}")
    tau = max(worst.values())
    print(f"measured tau0 = {tau:.3e} at {max(worst, key=worst.get)}; TAIL_TAU0 = {BR.TAIL_TAU0:.3e}")
    assert tau <= BR.TAIL_TAU0
    assert BR.TAIL_TAU0 <= 1.5 * tau          # pinned at the measurement, not above it


def _variant(monkeypatch, name):
    """Patches probit_ref into a wrong kernel; returns the K to run it with."""
    kap, lph = BR.kappa, BR.log_phi
    f32 = lambda f: (lambda x: np.asarray(f(x), np.float64).astype(np.float32).astype(np.float64))
    if name == "fp32":
        monkeypatch.setattr(BR, "kappa", f32(kap))
        monkeypatch.setattr(BR, "log_phi", f32(lph))
    elif name == "upper_formula_below_zero":
        from scipy.special import erfc
        monkeypatch.setattr(BR, "log_phi", lambda x: np.log1p(-0.5 * erfc(np.asarray(x, np.float64) * math.sqrt(0.5))))
    elif name == "wrong_constant":
        monkeypatch.setattr(BR, "SQRT_2_PI", math.sqrt(1.0 / (2.0 * math.pi)))
    return {"K1": 1, "K3": 3}.get(name, BR.K_STEPS)


@pytest.mark.parametrize("name", ("K1", "K3", "fp32", "upper_formula_below_zero", "wrong_constant"))
def test_tail_tolerance_rejects_a_wrong_kernel(name, monkeypatch):
    """Each variant of the reference misses 4 x TAIL_TAU0 by at least 10 x on at
    least one slice of the grid (n = 20); were one to pass, the grid would be too tame."""
    fx = _fixture()
    K = _variant(monkeypatch, name)
    n = BR.GRID_SHAPES[0]
    worst, where, by_rho = 0.0, None, {}
    with np.errstate(all="ignore"):
        for rho in BR.GRID_RHOS:
            for k, dev in BR.grid_deviation(BR.grid_reference(n, rho, K=K), fx).items():
                per_slice = dev.max(axis=(0, 1, 3)) if dev.ndim == 4 else dev.max(axis=1)
                print(f"{name} {k}: per slice / (4 tau0) = {(per_slice / (4 * BR.TAIL_TAU0)).tolist()}")
                by_rho[rho] = max(by_rho.get(rho, 0.0), float(per_slice.max()))
                if per_slice.max() > worst:
                    worst, where = float(per_slice.max()), (k, int(per_slice.argmax()))
    print(f"{name}: worst deviation {worst:.3e} = {worst / (4 * BR.TAIL_TAU0):.3e} x the allowance, at {where}; "
          f"by rho {by_rho}")
    assert worst >= 10 * 4 * BR.TAIL_TAU0, (name, worst)
    # a wrong step count shows at every rho != 0 (at rho = 0 the steps change nothing); the others at every rho
    for rho in BR.GRID_RHOS:
        if rho != 0.0 or name not in ("K1", "K3"):
            assert by_rho[rho] >= 10 * 4 * BR.TAIL_TAU0, (name, rho, by_rho[rho])


def test_formulas_against_mpmath_over_a_dense_grid():
    """kappa, log Phi and Phi over [-38, 38] in steps of 1 / 8 and at the special
    points.  Each of the three is exp(-x^2 / 2) times something tame in one of
    its tails, and fp64 forms that exponent from a rounded x / sqrt 2 and rounds
    it again before exp: either rounding moves the value by up to x^2 2^-53 of
    itself, whatever the library.  The allowance is (8 + 4 x^2) 2^-53 of the
    value: those two, as much again for erfc / erfcx themselves (scipy states no
    bound in the tails), and 8 ulp for the few operations around them.  Below the
    smallest normal number (kappa past x = 37.66, Phi below x = -37.5) a value
    carries no relative precision: that is the floor."""
    mpmath = pytest.importorskip("mpmath")
    mp, mpf = mpmath.mp, mpmath.mpf
    x = np.concatenate([np.arange(-38.0, 38.0 + 1e-9, 0.125), BR.GRID_SPECIAL, [-1.0 / 1024, 1.0 / 1024],
                        [37.65, 37.67, -37.65, -37.67, -38.5, 38.5, 8.29, 8.3, -220.0, 220.0, 0.0]])
    want = np.zeros((3, len(x)))
    with mp.workdps(80):
        for q, xv in enumerate(x):
            xm, s2 = mpf(float(xv)), mp.sqrt(2)
            Phi = mp.erfc(-xm / s2) / 2
            want[0, q] = float(mp.npdf(xm) / Phi)
            want[1, q] = float(mp.log(Phi) if xm <= 0 else mp.log1p(-mp.erfc(xm / s2) / 2))
            want[2, q] = float(Phi)
    got = np.stack([BR.kappa(x), BR.log_phi(x), BR.phi_cdf(x)])
    assert np.isfinite(got).all()
    tol = (8.0 + 4.0 * x * x) * 2.0 ** -53 * np.abs(want) + 2.0 ** -1022
    ratio = np.abs(got - want) / tol
    for q, nm in enumerate(("kappa", "log_phi", "phi_cdf")):
        print(f"{nm}: max err / allowance {ratio[q].max():.3f} at x = {x[ratio[q].argmax()]}; "
              f"max relative error {np.max(np.abs(got[q] - want[q]) / np.maximum(np.abs(want[q]), 1e-300)):.3e}")
    assert (ratio <= 1.0).all()


def test_ties_against_the_means_reach_the_tail_and_keep_the_score_rule():
    """The "against" ties of the GPU tests' random states: s m goes below -20 at
    r = 16 and 32, and the score rule's cap on entries with pi within 1e-6 of 1/2
    (0.1 %) holds on the reference for them."""
    import predictive_ref as PR
    from test_gpu_probit import CASES
    for case in CASES:
        n, T, r = case
        X, S = PR.make_state(n, T, r)
        drawn, B = BR.state_ties(X, case, "drawn"), BR.state_ties(X, case, "against")
        mu = np.stack([MR.mean_mu(X[:, t].astype(np.float64), r)[:, :, 0] for t in range(T)], 2)
        off = ~np.eye(n, dtype=bool)
        sm = (np.where(B, 1.0, -1.0) * mu)[off]
        flipped = (B != drawn)[off].mean()
        print(f"n{n}_T{T}_r{r}: s m in [{sm.min():.2f}, {sm.max():.2f}], {100 * (sm < 0).mean():.1f} % of the ties "
              f"against their means, {100 * flipped:.1f} % differ from the draw")
        assert 0.3 <= (sm < 0).mean() and flipped >= 0.25
        if r >= 16:
            assert sm.min() < -20.0
        rows, mag, near = BR.score_rows(X, S, r, B)
        assert (near <= 1e-3 * 2 * rows[:, 0]).all(), (case, near)
        assert np.isfinite(rows).all() and np.isfinite(BR.stat_rows(X, B, None, -0.7)[0]).all()
