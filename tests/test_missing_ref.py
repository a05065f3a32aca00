"""Hidden dyads on the CPU: model.set_missing, the fixed point of the
fill-then-sweep iteration, and what the scheme is worth on held-out dyads
(tests/missing_ref.py; no GPU)."""
import numpy as np
import pytest
import torch

import missing_ref as MR


def _model(n=6, T=3, r=1):
    from ame_amd import TemporalAMEModel
    m = TemporalAMEModel(n, T, r, seed=1)
    m.generate_data_fast(seed=2)
    return m


def test_set_missing_validation():
    m = _model()
    assert m.missing is None
    good = MR.random_mask(6, 3, 0.4)
    m.set_missing(good)
    assert m.missing.dtype == torch.bool and tuple(m.missing.shape) == (6, 6, 3)
    assert np.array_equal(m.missing.numpy(), good)
    # uint8 and torch inputs; the diagonal is ignored
    u8 = torch.from_numpy(good.astype(np.uint8))
    u8[2, 2, 1] = 1
    m.set_missing(u8)
    assert np.array_equal(m.missing.numpy(), good)
    # Y is untouched and stays finite
    assert bool(torch.isfinite(m.Y).all())
    # clearing
    m.set_missing(None)
    assert m.missing is None
    # shape, dtype, asymmetry
    with pytest.raises(ValueError, match="shape"):
        m.set_missing(np.zeros((6, 6, 2), dtype=bool))
    with pytest.raises(ValueError, match="shape"):
        m.set_missing(np.zeros((6, 5, 3), dtype=bool))
    with pytest.raises(ValueError, match="dtype"):
        m.set_missing(np.zeros((6, 6, 3), dtype=np.float32))
    bad = good.copy()
    bad[0, 1, 0] = not bad[0, 1, 0]
    with pytest.raises(ValueError, match="symmetric"):
        m.set_missing(bad)
    assert m.missing is None                       # a refused mask changes nothing


def test_pack_reference_layout():
    """missing_ref.pack: bit j & 63 of word j >> 6, nothing at j >= n or j == i."""
    mask = MR.sym_mask(66, 2, [(0, 63, 0), (0, 64, 0), (64, 65, 1), (3, 5, 1)])
    w, pairs, deg = MR.pack(mask)
    assert w.shape == (2, 66, 2) and w.dtype == np.uint64
    assert int(w[0, 0, 0]) == 1 << 63 and int(w[0, 0, 1]) == 1
    assert int(w[0, 63, 0]) == 1 and int(w[0, 64, 0]) == 1
    assert int(w[1, 64, 1]) == 1 << 1 and int(w[1, 65, 1]) == 1 << 0
    assert pairs.tolist() == [2, 2]
    assert deg[0, 0] == 63 and deg[0, 1] == 65 and deg[1, 3] == 64
    assert MR.asym_entries(mask) == 0
    mask[7, 9, 0] = True
    assert MR.asym_entries(mask) == 2


def test_own_fill_removes_a_hidden_partner_from_the_update():
    """With row i's hidden entries at J_j m_i, the hidden partners' part of h
    is exactly P_hid m_i: the full system is the masked one plus P_hid on both
    sides."""
    c = MR.make_case(10, 2, 2, seed=5)
    mask = MR.random_mask(10, 2, 0.4, seed=3)
    X = c["X0"]
    Yw = MR.own_fill(c["Y"], X, mask)
    assert np.array_equal(Yw[~MR.clean(mask)], c["Y"][~MR.clean(mask)])
    for i, t in ((0, 0), (4, 1), (9, 0)):
        P_all, h_all = MR.node_system(Yw, X, c["params"], mask, i, t, "all")
        P_obs, h_obs = MR.node_system(c["Y"], X, c["params"], mask, i, t, "observed")
        P_hid, h_hid = MR.node_system(Yw, X, c["params"], mask, i, t, "hidden")
        assert np.allclose(P_all, P_obs + P_hid, rtol=1e-13, atol=1e-13)
        assert np.allclose(h_hid, P_hid @ X[i, t], rtol=1e-12, atol=1e-12)
        assert np.allclose(h_all, h_obs + P_hid @ X[i, t], rtol=1e-12, atol=1e-12)


def test_fixed_point_is_the_masked_rule_up_to_the_jitter():
    """At a fixed point m of fill-then-sweep (lr = 1) node i's mean satisfies
        m = (P^-1 + eps I) h,   P = P_m + P_hid,   h = h_m + P_hid m,
    P_m, h_m the system over observed partners (plus prior terms), P_hid the
    hidden partners' precision, eps = 1e-6.  Multiplying by P:
        P m = h + eps P h   =>   P_m m = h_m + eps P h   =>   h_m = P_m m - eps P h.
    The masked rule's new mean is m' = (P_m^-1 + eps I) h_m, hence
        m' = m + eps (P_m m - P_m^-1 P h) - eps^2 P h,
    the converged mean plus a term that vanishes with the jitter.  Checked on
    node 0 at slice 0 to 1e-8 of max|m|."""
    c = MR.fixed_point_case()
    fit, mask, p = c["fit"], c["mask"], c["params"]
    assert fit["change"] < 1e-10, fit
    X = fit["X"]
    i, t = 0, 0
    assert mask[i, :, t].sum() >= 1                # node 0 has hidden partners at slice 0
    Yw = MR.own_fill(c["Y"], X, mask)
    P, h = MR.node_system(Yw, X, p, mask, i, t, "all")
    P_m, h_m = MR.node_system(c["Y"], X, p, mask, i, t, "observed")
    m = X[i, t]
    scale = np.abs(m).max()
    # m is a fixed point of the full rule on the working network
    assert np.abs(MR.jittered_solve(P, h) - m).max() <= 1e-8 * scale
    new = MR.masked_update(c["Y"], X, p, mask, i, t)
    eps = MR.JITTER
    term = eps * (P_m @ m - np.linalg.solve(P_m, P @ h)) - eps ** 2 * (P @ h)
    err = np.abs(new - (m + term)).max()
    print(f"sweeps {fit['sweeps']}, |m' - m| {np.abs(new - m).max():.3e}, |term| {np.abs(term).max():.3e}, "
          f"identity error {err:.3e} (max|m| {scale:.3f})")
    assert err <= 1e-8 * scale
    # the identity is not vacuous: without the term it fails by orders of magnitude
    assert np.abs(new - m).max() > 100 * 1e-8 * scale


def test_hidden_dyad_error_beats_zero_fill():
    e = MR.heldout_case()
    print("hidden-dyad MSE: zero-fill {zero_fill:.3f}, scheme {scheme:.3f}, full {full:.3f}".format(**e))
    assert e["scheme"] < e["zero_fill"]
    assert e["full"] <= e["scheme"]                # seeing everything cannot be worse here


def test_masked_terms_without_hidden_pairs_are_the_oracles():
    import ame_oracle as O
    c = MR.make_case(9, 3, 2, seed=8)
    none = np.zeros((9, 9, 3), dtype=bool)
    got = MR.masked_terms(c["Y"], c["X0"], c["S0"], c["params"], "good", none)
    split, recon = O.elbo_recon_fast(c["Y"], c["X0"], c["S0"], c["params"], "good")
    for k, v in zip(("loglik", "prior0", "trans", "entropy"), split):
        assert abs(got[k] - v) <= 1e-12 * abs(v), k
    assert abs(got["recon"] - recon) <= 1e-12 * recon
