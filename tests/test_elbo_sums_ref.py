"""CPU checks of tests/elbo_sums_ref.py, the fp64 reference the GPU tests of
ame_elbo and ame_pack_y compare with.

(a) Folded through the host's own assembly (engine.assemble, what
    vi.elbo_terms() uses), the eight sums reproduce the oracle's elbo_split and
    reconstruction error to 1e-12 relative per term, at two shapes, each with
    the constructor's parameters and with an asymmetric Phi / Q / R_inv draw.
(b) The sums of [0, k) and [k, T) add up to those of [0, T) within
    8 x 2^-52 x mag.
(c) The mismatch rule compares bit patterns.
"""
import numpy as np
import pytest

import elbo_sums_ref as E
import predictive_ref as PR
from generic_params import assign, generic_params

SHAPES = ((12, 4, 2), (37, 3, 5))
EPS = 2.0 ** -52


def _cov_terms(S, S0inv, Qinv):
    """(T, n, 4) from covariances (n, T, d, d) in numpy: slogdet, trace,
    tr(Qinv S), tr(S0inv S)."""
    S = np.swapaxes(S.astype(np.float64), 0, 1)
    sign, ld = np.linalg.slogdet(S)
    assert (sign > 0).all()
    return np.stack([ld, np.trace(S, axis1=-2, axis2=-1), np.einsum("ab,tnba->tn", Qinv, S),
                     np.einsum("ab,tnba->tn", S0inv, S)], axis=-1)


def _model(shape, generic):
    from ame_amd import TemporalAMEModel
    n, T, r = shape
    m = TemporalAMEModel(n, T, r, seed=5)
    if generic:
        assign(m, generic_params(r, 1000 * n + 10 * r + T))
    m.generate_data_fast(seed=9)
    return m


@pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_T%d_r%d" % s)
def test_sums_fold_to_the_oracle_terms(shape, generic):
    import ame_oracle as O
    from ame_amd.engine import Constants, assemble
    n, T, r = shape
    d = 2 + 2 * r
    m = _model(shape, generic)
    C = Constants(m)
    X, S = PR.make_state(n, T, r)
    Y = m.Y.numpy()
    S0inv, Qinv, Phi = C.S0inv.numpy(), C.Qinv.numpy(), C.Phi.numpy()
    rinv = C.R_inv.numpy().flatten()
    if generic:
        assert not np.allclose(Phi, Phi.T) and rinv[0] != rinv[3]
    ct = _cov_terms(S, S0inv, Qinv)
    out, mag, rows, mags = E.elbo_sums(X, ct, Y, S0inv, Qinv, Phi, rinv, 0, T)
    assert rows.shape == mags.shape == (T, 8) and (np.abs(out) <= mag).all()
    assert (rows[1:, 2:4] == 0).all() and (rows[0, 4:6] == 0).all() and (rows[1:, 4:6] != 0).all()
    P = {k: getattr(m, k).numpy().astype(np.float64) for k in ("R", "R_inv", "Sigma", "Psi", "Phi", "Q")}
    X64, S64, Y64 = X.astype(np.float64), S.astype(np.float64), Y.astype(np.float64)
    for variant in ("good", "naive"):
        t = assemble(out, n, T, d, variant, C)
        ref = O.elbo_split(Y64, X64, S64, P, variant)
        for k, want in zip(("loglik", "prior0", "trans", "entropy"), ref):
            rel = abs(t[k] - want) / abs(want)
            print(f"{variant} {k}: rel err {rel:.2e}")
            assert rel <= 1e-12, (variant, k, t[k], want)
        want = O.recon_error(Y64, X64)
        assert abs(t["recon"] - want) <= 1e-12 * want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_T%d_r%d" % s)
def test_sums_are_additive_over_slice_ranges(shape):
    n, T, r = shape
    p = E.make_params(r)
    X, _ = PR.make_state(n, T, r)
    Y = _model(shape, False).Y.numpy()
    ct = E.synthetic_cov_terms(n, T, 0)
    args = (X, ct, Y, p["S0inv"], p["Qinv"], p["Phi"], p["rinv"])
    whole, mag, _, _ = E.elbo_sums(*args, 0, T)
    for k in range(1, T):
        a, ma, _, _ = E.elbo_sums(*args, 0, k)
        b, mb, _, _ = E.elbo_sums(*args, k, T)
        assert (a[2:4] == whole[2:4]).all() and (b[2:4] == 0).all()     # slice 0 only
        assert (np.abs(a + b - whole) <= 8 * EPS * mag).all(), k
        assert (np.abs(ma + mb - mag) <= 8 * EPS * mag).all(), k
    # the previous mean comes from the full X: a range's sums do not change when
    # slices outside [t0 - 1, t1) do
    X2 = X.copy()
    X2[:, 0] += 1.0
    if T >= 3:
        c, _, _, _ = E.elbo_sums(X2, *args[1:], 2, T)
        b, _, _, _ = E.elbo_sums(*args, 2, T)
        assert np.array_equal(b, c)
    c, _, _, _ = E.elbo_sums(X2, *args[1:], 1, T)
    b, _, _, _ = E.elbo_sums(*args, 1, T)
    assert c[4] != b[4] and np.array_equal(np.delete(c, 4), np.delete(b, 4))


def test_synthetic_inputs_discriminate():
    """The synthetic cov_terms tell columns and slices apart, and the parameter
    draw is off the fp32 grid."""
    ct = E.synthetic_cov_terms(37, 3, 0)
    sums = ct.sum(1)                                   # (T, 4)
    mag = np.abs(ct).sum(1)
    gap = np.abs(sums.reshape(-1)[:, None] - sums.reshape(-1)[None, :])
    gap[np.eye(12, dtype=bool)] = np.inf
    assert gap.min() > 1e-3 * mag.max()
    assert (ct < 0).any() and (ct > 0).any() and np.abs(ct).max() / np.abs(ct).min() > 1e4
    p = E.make_params(2)
    assert p["rinv"][1] != p["rinv"][2]
    assert not E.is_fp32(p["Qinv"]).all() and not E.is_fp32(p["S0inv"][:2, :2]).any()


def test_mismatch_rule_compares_bits():
    Y = np.zeros((3, 3, 2, 2), dtype=np.float32)
    Y[0, 1, 0], Y[1, 0, 0] = (1.0, 2.0), (2.0, 1.0)              # consistent
    assert E.pack_mismatches(Y, 0, 2) == 0
    Y[0, 2, 1], Y[2, 0, 1] = (0.0, 3.0), (3.0, -0.0)             # equal as floats, not as bits
    assert E.pack_mismatches(Y, 0, 2) == 1 and E.pack_mismatches(Y, 0, 1) == 0
    nan = np.array([0x7FC01234], dtype=np.uint32).view(np.float32)[0]
    Y[1, 2, 0], Y[2, 1, 0] = (nan, 5.0), (5.0, nan)              # same bits on both sides
    Y[1, 1, 0] = (9.0, nan)                                      # the diagonal is not a pair
    assert E.pack_mismatches(Y, 0, 2) == 1
    lay = E.pack_layout(Y, 1, 2)
    assert lay.shape == (1, 3, 4, 2) and (lay[:, :, 3] == 0).all()
    assert lay[0, 2, 0, 1] == 0x80000000 and lay[0, 0, 2, 1] == np.float32(3.0).view(np.uint32)
