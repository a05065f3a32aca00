"""CPU checks of tests/smooth_masked_ref.py (the smoother over observed
partners) and of the inputs tests/test_gpu_smooth_masked.py runs: the two
routes agree, hiding partners never narrows a covariance, an all-False mask is
smooth_ref, every listed kernel mistake is visible on every GPU parity shape,
and the figures DESIGN.md §7e / §7g quote."""
import functools

import numpy as np
import pytest

import missing_ref as MR
import predictive_ref as PR
import smooth_masked_ref as SMR
import smooth_ref as SR

IDS = lambda s: "n%d_T%d_r%d" % s
PSET = "gen"
ALL_SHAPES = SMR.SHAPES + SMR.EVERY_R_SHAPES
@functools.lru_cache(maxsize=None)
def _dense_case(shape):
    """The shape's inputs with its 30 % random mask, the reference and its tolerance."""
    base = SR.make_case(shape, PSET)
    n, T, r = shape
    mask = SMR.make_mask("random30", n, T)
    ref = SMR.smooth(base["Y"], base["X"], base["R_inv"], base["consts"], mask)
    return base, mask, ref, SMR.tolerance(ref, n, T, 2 + 2 * r)


@pytest.mark.parametrize("shape", SMR.SHAPES, ids=IDS)
def test_recursion_matches_dense_inverse(shape):
    """Both routes are fp64 and differ by their solve errors, each within the solve term of the
    GPU bound (as test_smooth_ref.test_recursion_matches_dense_inverse)."""
    base, mask, ref, _ = _dense_case(shape)
    n, T, r = shape
    d = 2 + 2 * r
    rec = SMR.smooth(base["Y"], base["X"], base["R_inv"], base["consts"], mask, route="recursion")
    for k in ("mean", "cov", "cross"):
        scale = np.abs(ref[k].reshape(n, -1)).max(1)
        bound = 2 * 8.0 * T * d * 2.0 ** -52 * ref["cond"] * scale
        e = np.abs(rec[k] - ref[k]).reshape(n, -1).max(1)
        assert (e <= bound).all(), (k, float((e / np.where(bound > 0, bound, 1)).max()))


@pytest.mark.parametrize("shape", SMR.SHAPES[:4] + SMR.EVERY_R_SHAPES[:3], ids=IDS)
def test_gram_route_is_the_partner_sum(shape):
    """sym(R_inv) (.) ((G - w_i w_i') - H) is the sum over the observed partners."""
    base, mask, ref, _ = _dense_case(shape)
    n, T, r = shape
    X = base["X"].astype(np.float64)
    Rs = 0.5 * (base["R_inv"] + base["R_inv"].T)
    m = MR.clean(mask)
    for i in range(0, n, max(1, n // 7)):
        for t in range(T):
            obs = np.nonzero((np.arange(n) != i) & ~m[i, :, t])[0]
            P, _ = MR._obs_terms(base["Y"].astype(np.float64), X, Rs, i, t, obs)
            G = SMR.gram_route(X, Rs, m, i, t)
            assert np.abs(G - P).max() <= (n + 2) * 2.0 ** -52 * ref["a"][i] * 4, (i, t)


@pytest.mark.parametrize("shape", SMR.SHAPES + SR.SHAPES[2:6], ids=IDS)
def test_hiding_partners_never_narrows(shape):
    """S_observed - S_all-partners is positive semidefinite at every (node, slice): smallest
    eigenvalue >= -1e-10 max|entry|."""
    base, mask, ref, _ = _dense_case(shape)
    full = base["ref"]["cov"]
    worst, ratios = 0.0, []
    for i in range(shape[0]):
        for t in range(shape[1]):
            dlt = ref["cov"][i, t] - full[i, t]
            ev = np.linalg.eigvalsh(0.5 * (dlt + dlt.T)).min()
            worst = min(worst, ev / np.abs(ref["cov"][i, t]).max())
            ratios.append(np.trace(ref["cov"][i, t]) / np.trace(full[i, t]))
    print(f"{IDS(shape)}: smallest eigenvalue / max|entry| = {worst:.2e}; tr ratio mean {np.mean(ratios):.2f} "
          f"max {np.max(ratios):.2f}")
    assert worst >= -1e-10
    assert min(ratios) >= 1.0 - 1e-10


@pytest.mark.parametrize("shape", SMR.SHAPES, ids=IDS)
def test_all_false_mask_is_smooth_ref(shape):
    c = SMR.make_case(shape, PSET, "none")
    n, T, r = shape
    for k in SMR.KEYS:
        a, b = c["mref"][k], c["ref"][k]
        assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max(), k


@pytest.mark.parametrize("name", [m for m in SMR.MASKS if m not in ("random30", "none")])
def test_structured_masks_are_what_they_say(name):
    for n, T, r in SMR.SHAPES:
        m = SMR.make_mask(name, n, T)
        assert m.shape == (n, n, T) and np.array_equal(m, m.transpose(1, 0, 2)) and not m[np.arange(n), np.arange(n)].any()
        assert all(m[:, :, t].any() for t in range(T))
        assert all(not np.array_equal(m[:, :, 0], m[:, :, t]) for t in range(1, T))
        deg = m.sum(1)                      # hidden partners (n, T)
        if name == "one_pair":
            assert (m.sum((0, 1)) == 2).all()
        if name == "last_pair":
            assert m[n - 2, n - 1, 0] and (m.sum((0, 1)) == 2).all()
        if name == "cols63_64":
            c0, c1 = (63, 64) if n >= 65 else (n - 2, n - 1)
            assert m[0, c0, 0] and m[0, c1, 0]
        if name == "counts1345" and n >= 9:
            assert [int(deg[k, 0]) for k in range(4)] == [1, 3, 4, 5]
        if name == "all_of_one":
            assert deg[n // 2, 1] == n - 1


@pytest.mark.parametrize("mutation", SMR.MUTATIONS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=IDS)
def test_every_mutation_shows(shape, mutation):
    """On every GPU parity shape, under its 30 % random mask, each mistake moves at least half
    the entries of `cov` (of `mean` for drop_mask_h, which leaves the covariances alone) by more
    than 100 x the GPU tolerance."""
    base, mask, ref, tol = _dense_case(shape)
    mut = SMR.smooth(base["Y"], base["X"], base["R_inv"], base["consts"], mask, mutation=mutation)
    key = "mean" if mutation == "drop_mask_h" else "cov"
    moved = np.abs(mut[key] - ref[key]) > 100.0 * tol[key]
    print(f"{IDS(shape)} {mutation}: {moved.mean():.3f} of {key} moved")
    assert moved.mean() >= 0.5, (mutation, float(moved.mean()))
    if mutation == "drop_mask_h":
        assert np.array_equal(mut["cov"], ref["cov"])


# ---- the figures DESIGN.md quotes ----
@functools.lru_cache(maxsize=None)
def heldout_scores():
    """missing_ref.heldout_case's fit (n = 24, T = 3, r = 2, 20 % hidden, 25 sweeps): the held-out
    mean z^2 and 90 % coverage with the fit's covariances and with the observed-partner ones."""
    c = MR.make_case(24, 3, 2, seed=31, lr=0.5)
    mask = MR.random_mask(24, 3, 0.2, seed=2)
    Y, p = c["Y"], c["params"]
    fit = MR.oracle_fit(Y, c["X0"], c["S0"], p, mask, "good", 0.5, 25)
    X32 = fit["X"].astype(np.float32).astype(np.float64)
    sm = SMR.smooth(Y, X32, p["R_inv"], SMR.consts_from(p), mask)
    zsq, csq = PR.thresholds((0.9,))
    out = {}
    for name, (X, S) in (("fit", (fit["X"], fit["S"])), ("observed", (sm["mean"], sm["cov"]))):
        rows, per = MR.score_rows(X, S, 2, Y, p["R"], zsq, csq, mask, MR.HIDDEN)
        z2 = np.concatenate([d["z2"].reshape(-1) for d in per])
        out[name] = dict(z2=float(z2.mean()), cover=float((z2 <= zsq[0]).mean()), pairs=int(rows[:, 0].sum()))
    return out


def test_heldout_scores_figures():
    s = heldout_scores()
    print("held-out dyads of missing_ref.heldout_case: " + "; ".join(
        f"{k}: mean z^2 {v['z2']:.3f}, 90 % coverage {v['cover']:.3f} ({v['pairs']} pairs)" for k, v in s.items()))
    for v in s.values():
        assert np.isfinite(v["z2"]) and 0.0 <= v["cover"] <= 1.0 and v["pairs"] > 0


E2E = (33, 3, 2)
E2E_SWEEPS, E2E_LR = 5, 0.5


@functools.lru_cache(maxsize=None)
def em_runs():
    """One EM round (update R) at (33, 3, 2), 30 % hidden, M-step on the observed-partner
    smoothed statistics: the fp64 CPU run and the same with fp32 state arrays."""
    n, T, r = E2E
    c = MR.make_case(n, T, r, seed=43, lr=E2E_LR)
    mask = MR.random_mask(n, T, 0.3, seed=6)
    run = lambda dt: SMR.oracle_em_round(c["Y"], c["X0"], c["S0"], c["params"], mask, dtype=dt,
                                         sweeps=E2E_SWEEPS, lr=E2E_LR)
    return dict(case=c, mask=mask, em64=run(np.float64), em32=run(np.float32))


def test_em_round_allowance_is_measurable():
    e = em_runs()
    own = MR.relative_deviation(e["em64"], e["em32"], ("R",))
    print(f"R after one round: CPU EM fp32 vs fp64 {own:.3e}")
    assert 0.0 < own < 1e-3
    assert np.linalg.eigvalsh(e["em64"]["R"]).min() > 0
