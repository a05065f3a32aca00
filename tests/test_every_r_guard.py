"""Completeness guard (no GPU) for the every-latent-dim matrix of the GPU suite.

libame_amd.so compiles one template instance per r = 1..32 for every kernel
path, and the instances differ in lane mapping, padding and LDS layout.  The
GPU tests run each path at every r; this file holds their parameter lists to
that, so an edit cannot thin the matrix without a test failing, and pins the
host-side facts the lists rest on (the compiled r set, the v3 fit bound, the
LDS overflow reach), which the library answers without a device.
"""
import ctypes

import predictive_ref as R
import test_gpu_align as A
import test_gpu_cov_terms as C
import test_gpu_every_r as E
import test_gpu_pairs as P

ALL_R = set(range(1, 33))
VARIANTS = {"good", "bad", "naive"}


def _v3_accepts(n, T, r, variant=0, request=3):
    from ame_amd import _lib
    d = _lib.ame_dims(n, r, T, 0, T, variant)
    return int(_lib.lib().ame_sweep_kind(ctypes.byref(d), request)) == 3


def _params(fn, name):
    """The argvalues of the parametrize mark of `fn` whose argnames are `name`."""
    for mark in fn.pytestmark:
        if mark.name == "parametrize" and mark.args[0] == name:
            return list(mark.args[1])
    raise AssertionError(f"{fn.__name__} has no parametrize mark {name!r}")


def test_library_compiles_r_1_to_32():
    from ame_amd import _lib
    assert set(_lib.supported_r()) == ALL_R == set(E.ALL_R)


def test_v3_bound_is_r_23():
    """v3 accepts exactly r = 1..23 at the matrix shape, in every variant;
    r = 23 ends at n = 128, r = 22 at n = 384 (Lay<R>::total within 160 KiB)."""
    n, T = E.V3_SHAPE
    for v in range(3):
        assert {r for r in ALL_R if _v3_accepts(n, T, r, v)} == set(E.V3_R) == set(range(1, 24))
    assert _v3_accepts(128, 1, 23) and not _v3_accepts(129, 1, 23)
    assert _v3_accepts(384, 1, 22) and not _v3_accepts(385, 1, 22)
    assert not any(_v3_accepts(2, 1, r) for r in range(24, 33))


def test_sweep_matrix_covers_every_cell():
    assert _params(E.test_v3_every_r_every_variant, "r,method") == \
        [(r, v) for r in range(1, 24) for v in E.VARIANTS]
    assert _params(E.test_workers_every_r_every_variant, "r,method") == \
        [(r, v) for r in range(1, 33) for v in E.VARIANTS]
    waves = _params(E.test_v3_all_helper_waves, "n,T,r,method")
    assert [(n, T, r) for n, T, r, _ in waves] == \
        [(460, 2, r) for r in range(1, 22)] + [(380, 2, 22)]
    for n, T, r, v in waves:
        assert v == E.VARIANTS[r % 3]
        # all 7 helper waves and a second slot (r = 22: six waves, all it fits), registers only
        assert (448 < n if r < 22 else 320 < n) and n <= 448 * E.nsreg(r) and _v3_accepts(n, T, r)
    other = _params(E.test_other_v2_kinds_every_r, "kind,r,method")
    assert len(other) == 4 * 32 == len(set(other))
    for kind in (20, 21, 23, 24):
        cells = [(r, v) for k, r, v in other if k == kind]
        assert [r for r, _ in cells] == list(range(1, 33))
        assert all(v == E.VARIANTS[(r + kind) % 3] for r, v in cells)
        for v in VARIANTS:   # each (kind, variant) sees every residue of r mod 4
            assert {r % 4 for r, vv in cells if vv == v} == {0, 1, 2, 3}, (kind, v)
    assert set(E.VARIANTS) == VARIANTS and E.FP32_CAP == 1e-4 and E.LR == 0.5


def test_overflow_cases_reach_the_lds_slots():
    """Each case is accepted by v3 under AME_SWEEP_AUTO and has nodes past the
    register slots; NSREG restated from Cfg<R>::NSREG (csrc/ame_sweep3.hip)."""
    assert [E.nsreg(r) for r in (1, 3, 4, 6, 8, 10, 13, 16, 24, 25, 32)] == \
        [16, 16, 12, 8, 6, 4, 3, 3, 2, 1, 1]
    cases = _params(E.test_v3_lds_overflow_slots, "n,T,r,method")
    assert cases == [(1400, 2, 13, "good"), (1400, 2, 13, "bad"), (1400, 2, 13, "naive"),
                     (2200, 2, 10, "bad"), (2900, 1, 8, "naive")]
    for n, T, r, v in cases:
        assert n > 448 * E.nsreg(r)
        assert _v3_accepts(n, T, r, E.VARIANTS.index(v), request=0)
    # the r whose overflow slots fit the LDS at all
    reach = {r for r in range(1, 24) if _v3_accepts(448 * E.nsreg(r) + 1, 1, r)}
    assert reach == {7, 8, 9, 10, 11, 13}


def test_direct_kernel_tests_cover_every_r():
    assert set(_params(C.test_cov_terms_random_spd, "r")) == ALL_R
    assert set(_params(C.test_cov_terms_random_spd, "t_begin")) == {0, 1}
    assert set(_params(C.test_cov_terms_indefinite, "r")) >= {2, 4, 6, 16, 17, 19, 21, 23, 24, 31, 32}
    pairs = _params(P.test_pairs_v2_matches_v1_and_oracle, "n,T,r,swap")
    assert {r for _, _, r, _ in pairs} == ALL_R
    assert {(n, T, r, s) for n, T, r, s in pairs if n == 70} == \
        {(70, 2, r, r % 2 == 0) for r in ALL_R - {1, 2, 3, 5, 8, 16, 32}}
    align = _params(A.test_align_vs_oracle_large, "n,T,r")
    assert {r for _, _, r in align} == ALL_R
    assert {s for s in align if s[0] == 77} == {(77, 3, r) for r in ALL_R - {16, 32}}


def test_predictive_tests_cover_every_r():
    import test_gpu_predictive as G
    import test_predictive_ref as M
    assert set(R.GPU_SHAPES_EVERY_R) == {(65, 2, r) for r in ALL_R - {1, 2, 3, 5, 8, 16, 32}}
    for fn in (G.test_dense_moments_match_reference, G.test_scoring_sums_match_reference):
        shapes = _params(fn, "shape")
        assert {s[2] for s in shapes} == ALL_R
        assert set(shapes) == set(R.GPU_SHAPES) | set(R.GPU_SHAPES_EVERY_R)
    # DELTA0 is measured over the same inputs
    assert set(M.DELTA0_SHAPES) == set(R.GPU_SHAPES) | set(R.GPU_SHAPES_EVERY_R)


def mstep_state_k(r):
    """The instance of ame_mstep_state_kernel<K> that serves r, restated from
    ame_mstep_state_dispatch (csrc/ame_mstep.hip): the first of K = 1, 2, 5, 10,
    18 with 256 K >= d^2, d = 2 + 2 r."""
    need = -(-(2 + 2 * r) ** 2 // 256)
    return next(k for k in (1, 2, 5, 10, 18) if need <= k)


def test_em_kernel_tests_cover_every_instance():
    """The M-step, covariate and missing-dyad kernels: every instance per r
    (ame_predict_pairs_kernel<R, 2>, the mask selector of <R, 0> / <R, 2>, the K
    loop counts of ame_covar_g_kernel and ame_fill_kernel), per K
    (ame_mstep_state_kernel<K>) and per p (ame_covar_{g,h,resid}_kernel<P>)."""
    import test_gpu_covar as CV
    import test_gpu_missing as MS
    import test_gpu_mstep as MT
    import test_covar_ref as CVR
    import test_mstep_ref as MTR
    # M-step
    for fn in (MT.test_state_rows_match_fp64_reference, MT.test_dyad_rows_match_reference_and_ame_predict,
               MT.test_bit_identity):
        shapes = _params(fn, "shape")
        assert {s[2] for s in shapes} == ALL_R, fn.__name__
        assert (63, 3, 20) in shapes and len(set(shapes)) == len(shapes), fn.__name__
        assert set(shapes) >= {(65, 2, r) for r in ALL_R - {1, 2, 3, 5, 8, 16, 20, 32}}, fn.__name__
    assert (63 % 32, 65 % 32) == (31, 1)           # the chunk that stops the prefetch one short; a one-node chunk
    fitted = _params(MT.test_statistics_of_a_fitted_state, "method,T,r")
    assert {m for m, _, r in fitted if r == 3} == VARIANTS and ("good", 3, 20) in fitted
    # the instance map the list rests on: if the thresholds of the dispatch move,
    # these are the r to look at again
    assert [mstep_state_k(r) for r in (1, 7, 8, 10, 11, 16, 17, 24, 25, 32)] == [1, 1, 2, 2, 5, 5, 10, 10, 18, 18]
    assert {mstep_state_k(r) for r in ALL_R} == {1, 2, 5, 10, 18}
    assert {r for r in ALL_R if mstep_state_k(r) == 10} == set(range(17, 25))
    assert (2 + 2 * 7) ** 2 == 256 and (2 + 2 * 24) ** 2 == 2500 and (2 + 2 * 32) ** 2 <= 18 * 256
    # covariates
    for fn in (CV.test_H_matches_fp64_reference, CV.test_G_matches_fp64_reference,
               CV.test_slice_split_invariance, CV.test_resid_is_fp64_rounded_once):
        cases = _params(fn, "case")
        assert len(set(cases)) == len(cases), fn.__name__
        assert {c[2] for c in cases} == ALL_R, fn.__name__
        assert set(cases) >= {(65, 2, r, 1 + (r - 1) % 8) for r in ALL_R}, fn.__name__
        for p in range(1, 9):
            assert len({(n, T) for n, T, _, pp in cases if pp == p}) >= 2, (fn.__name__, p)
        # every MFMA step count of the G kernel's K loop, pad4(r + 2) / 4
        assert {(r + 2 + 3) // 4 for _, _, r, _ in cases} == set(range(1, 10))
    # missing dyads
    for fn in (MS.test_fill_writes_hidden_entries_only, MS.test_fill_correction_sums,
               MS.test_predict_and_mstep_select_pairs):
        cases = _params(fn, "case")
        assert len(set(cases)) == len(cases), fn.__name__
        assert {c[2] for c in cases} == ALL_R, fn.__name__
        assert set(cases) >= set(MS.CASES) | {(65, 3, r) for r in ALL_R - {1, 2, 3, 16, 32}}, fn.__name__
    assert {(r + 3) // 4 for r in ALL_R} == set(range(1, 9))      # the fill kernel's K loop counts
    for case in MS.EVERY_R:
        assert MS.fill_masks(case, ()) == ("random30", "cols63_64", "tile")
        assert MS.select_masks(case) == ("random30",)
        assert set(MS.fill_masks(case, ())) <= set(MS.masks_for(*case[:2]))
    for case in MS.CASES:   # the hand-picked cases keep every mask
        names = tuple(MS.masks_for(*case[:2]))
        assert MS.fill_masks(case, names) == names
        assert set(names) - {"cols63_64"} <= set(MS.select_masks(case)) <= set(names)
    # the references' sensitivity (test_mstep_ref.py, test_covar_ref.py) is
    # measured over the inputs of the new cases
    assert set(MTR.GPU_NEW_SHAPES) == {(63, 3, 20)} | set(MT.EVERY_R)
    assert set(CVR.GPU_NEW_CASES) == set(CV.EVERY_R_P) | set(CV.SMALL_P)
