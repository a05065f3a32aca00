"""Pin the CPU oracle to the reference's own runs at model parameters off the
constructor defaults, and check that the generic draws the GPU parity tests use
(tests/test_gpu_model_params.py) can tell a mixed-up constant from a right one.

At the defaults Phi = ar I, R / Sigma have equal variances, Psi has identical
U / V blocks and Q is block-diagonal, so Q^-1 Phi == Phi^T Q^-1, R_inv[0,0] ==
R_inv[1,1], ...: a transposed read or a swapped block changes nothing.  The
gp_* fixtures (tests/golden/make_golden_params.py: the reference with its six
parameter attributes overwritten, tests/generic_params.py) have none of these
symmetries.

* fp64: the oracle reproduces the reference's fp64 trajectory to 1e-10
  relative (means, covariances, ELBO, MSE, each of the four ELBO terms);
* fp32: within test_oracle_golden.py's fp32 bound (5e-6 on the means, 5e-6
  relative on the ELBO);
* the statistics form of the sweep and the fast ELBO equal the direct forms on
  the `gen` set (ame_oracle._p_obs has separate R_inv[0,1] / R_inv[1,0] paths
  and e0 / e1 blocks that symmetric inputs never separate);
* discriminating power: for every draw the GPU file runs, each single mutation
  (Phi -> Phi^T, R's diagonal swapped, Sigma's diagonal swapped, Psi's U / V
  blocks exchanged, Q conjugated by a<->b, U<->V) moves the fp64 oracle's
  two-iteration means by at least 1e-2, 1000 times the GPU bound, so no later
  edit can turn a failing GPU case green by picking symmetric inputs;
* conditioning: for every such draw the fp32 oracle stays within
  1e-4 max(1, max|mu|) of the fp64 oracle; a draw that does not is replaced
  here, on the CPU.
"""
import glob
import os

import numpy as np
import pytest

import ame_oracle as O
import generic_params as GP
from conftest import GOLDEN, golden

FIXTURES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "gp_*.npz")))
F64 = [f for f in FIXTURES if f.endswith("_f64.npz")]
F32 = [f for f in FIXTURES if not f.endswith("_f64.npz")]


def test_fixture_sets_complete():
    sets = ["gen", "phi", "rinv"] + list(GP.CTOR)
    want = sorted(f"gp_{s}_{m}{x}.npz" for s in sets for m in ("good", "bad", "naive")
                  for x in ("", "_f64"))
    assert FIXTURES == want
    assert not glob.glob(os.path.join(GOLDEN, "gp_*_lr*.npz"))


def test_fixture_parameters_are_generic():
    """The stored parameters really lack the symmetries (and the recipe that
    the GPU draws use reproduces the stored `gen` / `phi` / `rinv` sets)."""
    z = golden("gp_gen_good_f64.npz")
    Phi, Q, R_inv, Sigma, Psi = (z[k].astype(np.float64) for k in ("Phi", "Q", "R_inv", "Sigma", "Psi"))
    r = int(z["r"])
    Qi = np.linalg.inv(Q)
    assert np.abs(Qi @ Phi - Phi.T @ Qi).max() > 0.1
    assert np.abs(Phi - Phi.T).max() > 0.05
    assert abs(np.abs(np.linalg.eigvals(Phi)).max() - 0.7) < 1e-5
    assert abs(R_inv[0, 0] - R_inv[1, 1]) > 1.0
    assert abs(Sigma[0, 0] - Sigma[1, 1]) > 0.05
    assert np.abs(Psi[:r, :r] - Psi[r:, r:]).max() > 0.05 and np.abs(Psi[:r, r:]).max() > 0.05
    assert np.abs(Q[:2, 2:]).max() > 1e-3
    for M, lo, hi in ((Q, 0.05, 0.2), (Sigma, 0.5, 2.0), (Psi, 0.5, 2.0)):
        ev = np.linalg.eigvalsh(M)
        assert np.array_equal(M, M.T) and ev.min() > lo * (1 - 1e-5) and ev.max() < hi * (1 + 1e-5)
    default = O.model_params(r)
    for pset, seed in (("gen", 20261), ("phi", 20262), ("rinv", 20263)):
        z = golden(f"gp_{pset}_bad.npz")
        want = dict(O.model_params(int(z["r"])), **GP.generic_params(int(z["r"]), seed, GP.SETS[pset]))
        for k in GP.PKEYS:
            assert np.array_equal(z[k], want[k]), (pset, k)
    assert default["Phi"][0, 0] == np.float32(0.8)


def _replay(name, dt):
    z = golden(name)
    method = name.split("_")[2].replace(".npz", "")
    P = {k: z[k].astype(dt) for k in GP.PKEYS}
    Y = z["Y"].astype(dt)
    Xm, Xc = z["init_mean"].astype(dt).copy(), z["init_cov"].astype(dt).copy()
    lr = float(z["lr"])
    res = []
    for it in range(1, int(z["iters"]) + 1):
        O.sweep(Y, Xm, Xc, P, method, lr)
        res.append((it, Xm.copy(), Xc.copy(), O.elbo_split(Y, Xm, Xc, P, method),
                    O.recon_error(Y, Xm)))
    return z, res


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.mark.parametrize("name", F64)
def test_oracle_fp64_reproduces_reference(name):
    z, res = _replay(name, np.float64)
    assert int(z["iters"]) == 2
    for it, Xm, Xc, sp, rec in res:
        assert _rel(Xm, z[f"mean_{it}"]) <= 1e-10, it
        if f"cov_{it}" in z:
            assert _rel(Xc, z[f"cov_{it}"]) <= 1e-10, it
        e = z["elbo"][it - 1]
        assert abs(sp.sum() - e) <= 1e-10 * abs(e)
        assert np.all(np.abs(sp - z["elbo_split"][it - 1]) <= 1e-10 * np.abs(z["elbo_split"][it - 1])), it
        assert abs(rec - z["recon"][it - 1]) <= 1e-10 * z["recon"][it - 1]
    assert "cov_2" in z


@pytest.mark.parametrize("name", F32)
def test_oracle_fp32_close_to_reference(name):
    z, res = _replay(name, np.float32)
    for it, Xm, Xc, sp, rec in res:
        assert np.abs(Xm - z[f"mean_{it}"]).max() < 5e-6
        assert abs(sp.sum() - z["elbo"][it - 1]) <= 5e-6 * abs(z["elbo"][it - 1])


@pytest.mark.parametrize("method", ["good", "bad", "naive"])
def test_stats_forms_equal_direct_on_gen(method):
    """sweep_stats == sweep and elbo_recon_fast == elbo_split / recon_error at
    the `gen` parameters, from the reference's fp64 trajectory."""
    z = golden(f"gp_gen_{method}_f64.npz")
    P = {k: z[k].astype(np.float64) for k in GP.PKEYS}
    Y = z["Y"].astype(np.float64)
    lr = float(z["lr"])
    A = (z["init_mean"].astype(np.float64), z["init_cov"].astype(np.float64))
    B = (A[0].copy(), A[1].copy())
    for it in (1, 2):
        O.sweep(Y, A[0], A[1], P, method, lr)
        O.sweep_stats(Y, B[0], B[1], P, method, lr)
        assert _rel(B[0], z[f"mean_{it}"]) <= 1e-10
    assert np.abs(A[0] - B[0]).max() <= 1e-12 * max(1.0, np.abs(A[0]).max())
    assert np.abs(A[1] - B[1]).max() <= 1e-13 * max(1.0, np.abs(A[1]).max())
    split, rec = O.elbo_recon_fast(Y, A[0], A[1], P, method)
    ref = O.elbo_split(Y, A[0], A[1], P, method)
    assert np.allclose(split, ref, rtol=1e-11, atol=1e-9)
    assert np.all(np.abs(split - z["elbo_split"][-1]) <= 1e-10 * np.abs(z["elbo_split"][-1]))
    assert abs(rec - O.recon_error(Y, A[0])) <= 1e-12 * rec


# ----------------------------------------------------------------------------
# discriminating power and conditioning of every draw the GPU file runs
# ----------------------------------------------------------------------------
MOVE = 1e-2        # 1000 x the GPU parity bound on the means


def _two_sweeps(Y, Xm0, Xc0, P, method, lr, fast):
    Xm, Xc = Xm0.copy(), Xc0.copy()
    for _ in range(2):
        (O.sweep_stats if fast else O.sweep)(Y, Xm, Xc, P, method, lr)
    return Xm


def _mutation_moves(Y, Xm, Xc, P, method, lr, pset):
    base = _two_sweeps(Y, Xm, Xc, P, method, lr, True)
    return {name: np.abs(_two_sweeps(Y, Xm, Xc, fn(P), method, lr, True) - base).max()
            for name, fn in GP.mutations(pset).items()}


@pytest.mark.parametrize("name", [f for f in F64 if GP.mutations(f.split("_")[1])])
def test_fixture_discriminates(name):
    z = golden(name)
    pset, method = name.split("_")[1:3]
    P = {k: z[k].astype(np.float64) for k in GP.PKEYS}
    moves = _mutation_moves(z["Y"].astype(np.float64), z["init_mean"].astype(np.float64),
                            z["init_cov"].astype(np.float64), P, method, float(z["lr"]), pset)
    print(name, {k: f"{v:.2e}" for k, v in moves.items()})
    assert moves and all(v >= MOVE for v in moves.values()), moves


def _case_state(case):
    m, vi = GP.build_case(case)
    P = {k: getattr(m, k).numpy().astype(np.float64) for k in GP.PKEYS}
    return m.Y.numpy(), vi.X_mean.numpy().copy(), vi.X_cov.numpy().copy(), P


@pytest.mark.parametrize("case", [c for c in GP.CASES if GP.mutations(c.pset)], ids=lambda c: c.id)
def test_draw_discriminates(case):
    Y, Xm, Xc, P = _case_state(case)
    moves = _mutation_moves(Y.astype(np.float64), Xm.astype(np.float64), Xc.astype(np.float64),
                            P, case.method, case.lr, case.pset)
    print(case.id, {k: f"{v:.2e}" for k, v in moves.items()})
    assert moves and all(v >= MOVE for v in moves.values()), moves


@pytest.mark.parametrize("case", GP.CASES, ids=lambda c: c.id)
def test_draw_is_well_conditioned(case):
    """fp32 oracle within 1e-4 max(1, max|mu|) of the fp64 oracle after the two
    iterations the GPU test runs (the direct sweep, as its helper uses; the
    statistics form, pinned to it above, at n = 300)."""
    assert case.lr <= 0.7
    Y, Xm, Xc, P = _case_state(case)
    fast = case.n > 100
    ref = _two_sweeps(Y.astype(np.float64), Xm.astype(np.float64), Xc.astype(np.float64), P,
                      case.method, case.lr, fast)
    P32 = {k: v.astype(np.float32) for k, v in P.items()}
    got = _two_sweeps(Y, Xm, Xc, P32, case.method, case.lr, fast)
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"{case.id}: fp32 oracle vs fp64 oracle {err:.2e}, max|mu| {np.abs(ref).max():.2f}")
    assert err <= 1e-4 * max(1.0, np.abs(ref).max()), err


def test_cases_cover_every_path():
    kinds = {(c.kind, c.method) for c in GP.CASES if c.pset == "gen"}
    for k in (GP.V3, GP.V2_LDS, GP.V2_HBM, GP.V2_WORKERS):
        assert {(k, m) for m in ("good", "bad", "naive")} <= kinds
    for k in (GP.V2_PIPE, GP.V2_W6):
        assert {(k, "good"), (k, "naive")} <= kinds
    for k in (GP.V3, GP.V2_LDS, GP.V2_HBM, GP.V2_WORKERS, GP.V2_PIPE, GP.V2_W6):
        assert any(c.kind == k and c.T == 2 for c in GP.CASES)
        assert any(c.kind == k and c.T >= 3 for c in GP.CASES)
    assert {c.opts.get("pairs_kernel") for c in GP.CASES} >= {GP.PAIRS_V1, GP.PAIRS_V2}
    assert len({c.id for c in GP.CASES}) == len(GP.CASES)
