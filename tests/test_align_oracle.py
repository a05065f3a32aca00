"""CPU: the alignment restatement in oracle/ame_oracle.py against the reference's
own outputs (tests/golden/*_align.npz, written by make_golden_align.py from
src/utils/alignment.py).  The reference computes in fp32, the oracle in fp64:
agreement within 2e-5 * max(1, |x|)."""
import numpy as np
import pytest

import ame_oracle as O
from conftest import golden


@pytest.mark.parametrize("tag", ["c1", "mid", "wide"])
def test_alignment_oracle_vs_reference(tag):
    z = golden(f"{tag}_align.npz")
    r = int(z["r"])
    Xt = z["X_true"].astype(np.float64)
    for name in [k[:-4] for k in z.files if k.endswith("_est")]:
        Xe = z[f"{name}_est"].astype(np.float64)
        tol = 2e-5 * max(1.0, np.abs(Xt).max())
        each = O.align_temporal_states(Xe, Xt, r, True)
        assert np.abs(each - z[f"{name}_each"]).max() <= tol, name
        glob = O.align_temporal_states(Xe, Xt, r, False)
        assert np.abs(glob - z[f"{name}_global"]).max() <= tol, name
        err, _ = O.compute_alignment_error(Xe, Xt, r)
        assert abs(err - z[f"{name}_err"]) <= 1e-5 * z[f"{name}_err"]
        err0, _ = O.compute_alignment_error(Xe, Xt, r, align=False)
        assert abs(err0 - z[f"{name}_err_noalign"]) <= 1e-5 * z[f"{name}_err_noalign"]
        assert abs(O.correlation_after_alignment(Xe, Xt, r) - z[f"{name}_corr"]) <= 1e-6


def _sign_margins(Xe, Xt, r, each):
    """(row length k, |x.t| / (|x|^2 + |t|^2)) of every row whose sign
    align_signs_rows decides (|-x - t| < |x - t| <=> x.t < 0), in fp64: the
    additive pairs and the rotated U and V rows (each time step, or with the
    global rotation)."""
    out = []
    rows = lambda X, Tr: out.append(
        (X.shape[-1], np.abs((X * Tr).sum(-1)) / ((X * X).sum(-1) + (Tr * Tr).sum(-1))))
    RM = None if each else O.procrustes_alignment(Xe.mean(axis=1)[:, 2:], Xt.mean(axis=1)[:, 2:])[1]
    for t in range(Xe.shape[1]):
        rows(Xe[:, t, :2], Xt[:, t, :2])
        if each:
            for blk in (slice(2, 2 + r), slice(2 + r, 2 + 2 * r)):
                rows(O.procrustes_alignment(Xe[:, t, blk], Xt[:, t, blk])[0], Xt[:, t, blk])
        else:
            rows(Xe[:, t, 2:] @ RM, Xt[:, t, 2:])
    return out


def test_gpu_align_inputs_have_no_sign_ties():
    """tests/test_gpu_align.py::test_align_vs_oracle_large holds an fp32 kernel
    to the fp64 oracle and relies on no row sitting on a sign tie.  For its
    inputs: (a) the oracle evaluated in fp32 takes the same decisions as in fp64
    (outputs within that test's 2e-5 bound; a flipped row would differ by 2 |x|);
    (b) every decided row is further from a tie than fp32 sums can blur.  The
    decision compares dp = |x - t|^2 and dn = |x + t|^2, each a sum of k
    squares: dp - dn = -4 x.t, dp + dn = 2 (|x|^2 + |t|^2).  An fp32 FMA chain
    errs by at most (k + 1) u of each sum, u = 2^-24, and the fp32 rounding of
    the rotated row moves x.t by at most u (|x|^2 + |t|^2) / 2, so the sign is
    safe when |x.t| / (|x|^2 + |t|^2) > (k + 3) u / 2; required here: twice that."""
    from test_gpu_align import ORACLE_SHAPES, oracle_inputs
    worst = np.inf
    for n, T, r in ORACLE_SHAPES:
        Xe, Xt = oracle_inputs(n, T, r)
        Xe64, Xt64 = Xe.astype(np.float64), Xt.astype(np.float64)
        for each in (True, False):
            ref = O.align_temporal_states(Xe64, Xt64, r, each)
            f32 = O.align_temporal_states(Xe, Xt, r, each)
            assert f32.dtype == np.float32
            assert np.abs(f32 - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), (n, T, r, each)
            for k, margin in _sign_margins(Xe64, Xt64, r, each):
                need = (k + 3) * 2.0 ** -24
                worst = min(worst, margin.min() / need)
                assert margin.min() > need, (n, T, r, each, k, margin.min(), need)
    print(f"smallest sign margin / required margin: {worst:.2f}")


def test_alignment_of_truth_is_identity():
    """Property: X_true^T X_true is symmetric PSD, so R = U Vt = I and every row
    keeps its sign -- aligning the truth to itself returns it unchanged."""
    rng = np.random.default_rng(3)
    Xt = rng.standard_normal((30, 4, 8))
    for each in (True, False):
        assert np.abs(O.align_temporal_states(Xt, Xt, 3, each) - Xt).max() < 1e-12
    assert O.compute_alignment_error(Xt, Xt, 3)[0] < 1e-24
