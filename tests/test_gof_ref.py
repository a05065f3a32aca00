"""The goodness-of-fit reference (tests/gof_ref.py) and the host arithmetic of
ame_amd/gof.py, on the CPU: Philox known answers, the raw-sum form against the
obvious dense form, a 4-node network worked by hand, and the sensitivity of
the reference to the mistakes the GPU bounds are meant to catch."""
import math

import numpy as np
import pytest

import gof_ref as R
from ame_amd import gof as G


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = R.philox4x32_10([np.uint32(c) for c in ctr], key)
        assert tuple(int(v) for v in got) == want
    # vectorised over counters: the same words
    ctr = [np.array([0, 0x243f6a88], dtype=np.uint32), np.array([0, 0x85a308d3], dtype=np.uint32),
           np.array([0, 0x13198a2e], dtype=np.uint32), np.array([0, 0x03707344], dtype=np.uint32)]
    got = R.philox4x32_10(ctr, (0, 0))
    assert int(got[0][0]) == 0x6627e8d5 and int(got[3][0]) == 0x9b00dbd8


def test_uniforms_lie_in_the_unit_interval_and_normals_are_standard():
    u = R.uniform24(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32 and u[0] == np.float32(2.0 ** -25) and u[1] == u[0]
    assert u[2] == np.float32(1.5 * 2.0 ** -24) and 0.0 < u.min() and u.max() <= 1.0
    z0, z1 = R.pair_normals(200, 3, 12345, 7)
    z = np.concatenate([z0[np.triu_indices(200, 1)], z1[np.triu_indices(200, 1)]])
    se = 1.0 / math.sqrt(z.size)
    assert abs(z.mean()) < 6 * se and abs(z.var() - 1.0) < 6 * math.sqrt(2.0) * se
    assert abs(np.corrcoef(z0[np.triu_indices(200, 1)], z1[np.triu_indices(200, 1)])[0, 1]) < 6 * math.sqrt(2) * se


def _network(n, T, seed, offset=0.0):
    """A directed network with sender / receiver effects, reciprocity and a
    rank-2 term, on a grid of 1/8 so that y - centre is exact in fp32."""
    rng = np.random.default_rng(seed)
    a, b = rng.normal(size=(T, n, 1)), rng.normal(size=(T, 1, n))
    U = rng.normal(size=(T, n, 2))
    e = rng.normal(size=(T, n, n))
    y = a + b + np.einsum("tik,tjk->tij", U, U + 0.3 * rng.normal(size=(T, n, 2))) + e + 0.5 * np.swapaxes(e, 1, 2)
    return np.round(8.0 * y) / 8.0 + offset


@pytest.mark.parametrize("n,T,offset", [(3, 2, 0.0), (5, 1, 0.0), (33, 3, 0.0), (64, 2, 16.0), (20, 2, -40.0)])
def test_raw_sum_form_matches_direct_form(n, T, offset):
    y = _network(n, T, 100 + n, offset)
    Yd = R.dense_from_directed(y)
    off = ~np.eye(n, dtype=bool)
    # a centre on the grid near the mean: y - centre is exact in fp32
    center = np.array([round(8.0 * y[t][off].mean()) / 8.0 for t in range(T)], dtype=np.float32)
    raw = R.raw_sums(Yd, center)
    st_raw = R.statistics_from_raw(raw["node"], raw["slice"], raw["tri"], n)
    st_lib = G.combine(raw["node"], raw["slice"], raw["tri"], n)
    for t in range(T):
        d = R.direct_statistics(y[t], center=center[t])
        for k in R.NAMES + ("mean", "sd"):
            # fp64 on both sides; the centred sums lose log2(kappa) bits, kappa <= 2e3 here
            assert st_raw[k][t] == pytest.approx(d[k], rel=1e-9, abs=1e-9), (k, t)
            assert st_lib[k][t] == pytest.approx(d[k], rel=1e-9, abs=1e-9), (k, t)
    assert G.stack(st_lib).shape == (T, 5)


def test_two_nodes_have_no_triads():
    y = _network(2, 1, 5)
    raw = R.raw_sums(R.dense_from_directed(y), np.zeros(1, dtype=np.float32))
    for st in (G.combine(raw["node"], raw["slice"], raw["tri"], 2),
               R.statistics_from_raw(raw["node"], raw["slice"], raw["tri"], 2), R.direct_statistics(y[0])):
        assert np.all(np.isnan(st["cycle_dep"])) and np.all(np.isnan(st["trans_dep"]))
        assert np.all(np.isfinite(st["sd_rowmean"]))


def test_hand_built_four_node_network():
    """ybar = 1, E = Y - 1 off the diagonal, sum E^2 = 10, s^2 = 10 / 11.
    Rows 4 3 3 2 and columns 2 4 3 3: row means 4/3 1 1 2/3, variance
    (1/9 + 1/9) / 3 = 2/27, the same for the columns.  sum E_ij E_ji = 2 (1 + 1)
    = 4 (the pairs {0, 2} and {1, 3}): dyad_dep = 4 / 10.  tr(E^3) = -9 and
    tr(E E' E) = -3 (rows of E E, E E' against the columns of E), over
    4 3 2 s^3."""
    y = np.array([[9., 3., 0., 1.],
                  [1., 9., 2., 0.],
                  [0., 1., 9., 2.],
                  [1., 0., 1., 9.]])   # the diagonal must not matter
    s3 = (10.0 / 11.0) ** 1.5
    want = {"mean": 1.0, "sd": math.sqrt(10.0 / 11.0), "sd_rowmean": math.sqrt(2.0 / 27.0),
            "sd_colmean": math.sqrt(2.0 / 27.0), "dyad_dep": 0.4, "cycle_dep": -9.0 / (24.0 * s3),
            "trans_dep": -3.0 / (24.0 * s3)}
    d = R.direct_statistics(y)
    raw = R.raw_sums(R.dense_from_directed(y[None]), np.ones(1, dtype=np.float32))
    assert raw["tri"][0].tolist() == [-9.0, -3.0] and raw["slice"][0].tolist() == [22.0, 16.0]
    lib = G.combine(raw["node"], raw["slice"], raw["tri"], 4)
    for k, v in want.items():
        assert d[k] == pytest.approx(v, rel=1e-13), k
        assert lib[k][0] == pytest.approx(v, rel=1e-13), k


def test_reference_is_sensitive_to_what_the_gpu_bounds_guard():
    """Keeping the diagonal in E, exchanging the cycle and the transitive
    operand, or centring by another mean (the mean over all n^2 cells) moves a
    triad statistic by far more than the GPU bound on it."""
    n = 33
    y = _network(n, 1, 77, offset=2.0)[0]
    np.fill_diagonal(y, 0.0)
    off = ~np.eye(n, dtype=bool)
    c = np.float32(y[off].mean())
    raw = R.raw_sums(R.dense_from_directed(y[None]), np.array([c]))
    good = R.direct_statistics(y, center=c)
    den = n * (n - 1) * (n - 2) * good["sd"] ** 3
    bound = R.triad_bounds(raw, n)[0] / den          # on cycle_dep, trans_dep
    broken = [R.direct_statistics(y, center=c, zero_diagonal=False),
              R.direct_statistics(y, center=c, swap_triads=True),
              R.direct_statistics(y, center=np.float32(y.sum() / n ** 2))]
    for b in broken:
        moved = max(abs(b["cycle_dep"] - good["cycle_dep"]) / bound[0],
                    abs(b["trans_dep"] - good["trans_dep"]) / bound[1])
        assert moved > 100.0, moved


def test_multiplicative_term_shows_in_the_triad_statistics():
    """The reference's networks from states without U, V have smaller |cycle_dep|
    and |trans_dep| than those from the full states, in every simulation and
    slice, at the seed the GPU test uses."""
    S, S0 = R.gof_states(R.GOF_SENSITIVITY_SEED)
    chol = (1.0, 0.3, 0.9)
    for k in range(S.shape[0]):
        full = R.simulate(S[k].transpose(1, 0, 2), chol, R.GOF_SENSITIVITY_SEED, k)["Y"]
        flat = R.simulate(S0[k].transpose(1, 0, 2), chol, R.GOF_SENSITIVITY_SEED, k)["Y"]
        for t in range(S.shape[2]):
            a, b = R.direct_statistics(full[t, :, :, 0]), R.direct_statistics(flat[t, :, :, 0])
            assert abs(b["cycle_dep"]) < 0.5 * abs(a["cycle_dep"]), (k, t)
            assert abs(b["trans_dep"]) < 0.5 * abs(a["trans_dep"]), (k, t)


def test_simulated_reference_network_is_swap_consistent():
    S, _ = R.gof_states(3, n=7, T=2, r=1, n_sim=1)
    out = R.simulate(S[0].transpose(1, 0, 2), (1.0, -0.4, 0.8), 99, 5, t_begin=4)
    Y = out["Y"]
    assert np.array_equal(Y[..., 0], np.swapaxes(Y[..., 1], 1, 2))
    assert np.all(Y[:, np.arange(7), np.arange(7)] == 0.0)
    again = R.simulate(S[0].transpose(1, 0, 2)[1:], (1.0, -0.4, 0.8), 99, 5, t_begin=5)["Y"]
    assert np.array_equal(again[0], Y[1])
