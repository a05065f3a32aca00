"""The reference of the residual diagnostics (tests/resid_ref.py) checked without
a GPU: its bounds hold an fp32 evaluation of the same formulas, few reference m2
lie within their bound of a bin edge, the node sums add up to the slice sums,
the planted pairs are the exact top of every slice, and the mutations a kernel
could plausibly make miss the bounds.
"""
import functools

import numpy as np
import pytest

import missing_ref as MR
import predictive_ref as PR
import resid_ref as RR

IDS = lambda c: "n%d_T%d_r%d" % c
FIELDS = (("m2", "d_m2"), ("z2", "d_z2"), ("e", "d_e"), ("logp", "d_logp"), ("z", "d_z"))


@functools.lru_cache(maxsize=None)
def case(shape):
    c = RR.make_case(shape)
    c["ref"] = RR.case_scores(c, shape[2])
    return c


def _f32(c, r, t):
    return PR.moments_f32(c["X"][:, t], c["S"][:, t], r)


@pytest.mark.parametrize("shape", RR.CPU_SHAPES, ids=IDS)
def test_fp32_evaluation_stays_inside_every_bound(shape):
    n, T, r = shape
    c = case(shape)
    for t in range(T):
        ref = c["ref"][t]
        f32 = RR.slice_scores(c["X"][:, t], c["S"][:, t], r, c["Y"][:, :, t], moments=_f32(c, r, t))
        shares = {a: float((np.abs(f32[a] - ref[a]) / ref[b]).max()) for a, b in FIELDS}
        print(f"{IDS(shape)} t={t}: worst used share of the bound {shares}")
        assert max(shares.values()) <= 1.0, (t, shares)
        assert (np.abs(f32["e"] ** 2 - ref["e"] ** 2) <= ref["d_q"]).all(), t
        got, want, bound = RR.node_sums(f32, n), RR.node_sums(ref, n), RR.node_bounds(ref, n)
        assert np.array_equal(got[:, 0], want[:, 0])
        assert (np.abs(got - want) <= bound).all(), t


@pytest.mark.parametrize("shape", RR.CPU_SHAPES, ids=IDS)
def test_few_reference_m2_lie_near_an_edge(shape):
    c = case(shape)
    share = max(RR.near_edge_share(d) for d in c["ref"])
    fine = max(RR.near_edge_share(d, 1024, 32.0) for d in c["ref"])
    print(f"{IDS(shape)}: share within d_m2 of an interior edge {share:.4f} at {RR.BINS} bins, {fine:.4f} at 1024")
    assert share <= 0.01


@pytest.mark.parametrize("shape", RR.CPU_SHAPES + ((2, 1, 1), (3, 2, 2)), ids=IDS)
def test_node_sums_add_up_to_twice_the_slice_sums(shape):
    n, T, r = shape
    c = case(shape)
    zsq, csq = PR.thresholds((0.5,))
    for t, d in enumerate(c["ref"]):
        for select in (0, MR.OBSERVED, MR.HIDDEN):
            ds = RR.subset(d, c["mask"][:, :, t], select)
            node, s = RR.node_sums(ds, n), PR.sums_from_scores(ds, zsq, csq)
            tot = node.sum(0)
            scale = RR.node_abs(ds, n).sum(0) + 1.0
            want = 2.0 * np.array([s[0], s[1], s[2], 0.5 * (s[3] + s[4]), 0.5 * (s[3] + s[4]), np.nan, np.nan,
                                   0.5 * (s[7] + s[8]), 0.5 * (s[7] + s[8])])
            want[5] = want[6] = ds["e"].sum()
            assert tot[0] == want[0]
            assert (np.abs(tot - want) <= 1e-12 * scale).all(), (t, select, tot, want)
            # sent and received are the two entries seen from the two ends
            assert abs(node[:, 3].sum() - node[:, 4].sum()) <= 1e-12 * scale[3]
            # a node whose pairs are all left out has exact zeros
            alone = np.setdiff1d(np.arange(n), np.concatenate([ds["i"], ds["j"]]))
            assert not node[alone].any()


@pytest.mark.parametrize("shape", RR.SHAPES, ids=IDS)
def test_planted_pairs_are_the_exact_top(shape):
    n, T, r = shape
    c = case(shape)
    for t, d in enumerate(c["ref"]):
        pl = c["planted"][t][::-1]                       # most surprising first
        top = RR.top_k(d, len(pl) + 1)
        got = [(int(d["i"][p]), int(d["j"][p])) for p in top[:len(pl)]]
        assert got == [(i, j) for i, j, _ in pl], (t, got, pl)
        m2 = d["m2"][top]
        assert np.allclose(m2[:len(pl)], [v for _, _, v in pl], rtol=1e-5), (t, m2)
        D = float(d["d_m2"].max())
        assert (-np.diff(m2) > 2.0 * D).all(), (t, m2, D)
        if len(m2) > len(pl):
            assert m2[-1] <= RR.CEILING
        # the end bin of the histogram holds m2 = 40, 90, 200
        assert RR.histogram(d)[-1] == sum(v >= RR.M2_MAX for _, _, v in pl)


@pytest.mark.parametrize("shape", RR.CPU_SHAPES, ids=IDS)
def test_mutations_miss_the_bounds(shape):
    n, T, r = shape
    c = case(shape)
    t = T - 1
    ref = c["ref"][t]
    args = (c["X"][:, t], c["S"][:, t], r, c["Y"][:, :, t])
    want, bound = RR.node_sums(ref, n), RR.node_bounds(ref, n)
    muts = {"no C01": RR.node_sums(RR.slice_scores(*args, drop_c01=True), n),
            "no noise": RR.node_sums(RR.slice_scores(*args, noise=np.zeros((2, 2))), n),
            "sent and received exchanged": RR.node_sums(ref, n, exchange=True)}
    for name, got in muts.items():
        over = np.abs(got - want) / np.maximum(bound, 1e-300)
        print(f"{IDS(shape)} {name}: worst |difference| / bound per slot {over.max(0)[1:]}")
        assert over[:, 1:].max() > 10.0, name
    assert (np.abs(RR.slice_scores(*args, drop_c01=True)["m2"] - ref["m2"]) > ref["d_m2"]).any()


def test_bin_rule():
    assert RR.bin_of([0.0, 0.124, 0.125, 31.99, 32.0, 1e9, -1.0, np.nan, np.inf]).tolist() == \
        [0, 0, 1, 255, 255, 255, 0, 255, 255]
