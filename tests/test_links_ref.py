"""The host finish of link ranking (ame_amd/links.py) against brute force, and
the conditions tests/test_gpu_links.py relies on, checked on the reference
alone (no GPU)."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import links_ref as LR
import predictive_ref as PR
import probit_ref as BR

from ame_amd import links

# the random states and the bin counts of tests/test_gpu_links.py
CASES = ((5, 1, 1), (33, 3, 2), (65, 4, 5), (130, 3, 16), (70, 2, 32))
RANDOM_BINS = (1024, 37)


@functools.lru_cache(maxsize=None)
def random_scores(case):
    n, T, r = case
    X, S = PR.make_state(n, T, r)
    B = BR.state_ties(X, case)
    return X, S, B, LR.scores(X, S, r, B, with_delta=True)


def _hists(seed, T=4, bins=16, top=30):
    rng = np.random.default_rng(seed)
    return rng.integers(0, top, (T, 2, bins)).astype(np.int64)


def test_bin_rule_matches_the_reference_and_puts_an_edge_score_into_the_upper_bin():
    for bins in (1, 2, 37, 64, 1024, 2048):
        ed = links.edges(bins, 8.0)
        assert ed.shape == (bins + 1,) and ed[0] == -8.0 and abs(ed[-1] - 8.0) <= 1e-12
        t = np.concatenate([np.random.default_rng(bins).normal(0, 5, 4000), [-1e300, 1e300, -8.0, 8.0, 0.0, -0.0]])
        assert np.array_equal(links.bin_of(t, bins, 8.0), LR.bin_of(t, bins, 8.0))
        assert links.bin_of([-9.0, 9.0, np.nan], bins, 8.0).tolist() == [0, bins - 1, 0]
    for bins in (64, 1024):      # edges are exact: multiples of 2^-2 and 2^-6
        ed = links.edges(bins, 8.0)
        assert np.array_equal(ed, LR.edges(bins)) and np.array_equal(ed * 64, np.round(ed * 64))
        assert np.array_equal(links.bin_of(ed[:-1], bins, 8.0), np.arange(bins))
        # just below an edge (further than the rounding of t + t_max, 2^-50): the lower bin
        assert np.array_equal(links.bin_of(ed[1:] - 2.0 ** -40, bins, 8.0), np.arange(bins))
    assert links.scale(1024, 8.0) == 64.0
    for bad in (0, 2049, 1.5, True):
        with pytest.raises(ValueError):
            links.check_bins(bad, 8.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            links.check_bins(16, bad)


@pytest.mark.parametrize("seed", range(3))
def test_curves_and_auc_bounds_equal_brute_force_exactly(seed):
    h = _hists(seed)
    if seed == 2:
        h[:, :, ::2] = 0          # empty bins, also at the ends
    got = links.curves(h)
    for t in range(h.shape[0]):
        w = LR.curves_brute(h[t])
        P, N = w["P"], w["N"]
        assert got["positives"][t] == P and got["negatives"][t] == N
        assert got["auc_lo"][t] == float(Fraction(w["num_lo"], P * N))
        assert got["auc_hi"][t] == float(Fraction(w["num_lo"] + w["num_tie"], P * N))
        assert got["auc"][t] == 0.5 * (got["auc_lo"][t] + got["auc_hi"][t])
        assert got["auc_lo"][t] <= got["auc"][t] <= got["auc_hi"][t]
        tpr = np.array([float(Fraction(v, P)) for v in w["tp"]])
        fpr = np.array([float(Fraction(v, N)) for v in w["fp"]])
        prec = np.array([float(Fraction(a, a + b)) if a + b else 1.0 for a, b in zip(w["tp"], w["fp"])])
        assert np.array_equal(got["tpr"][t], tpr) and np.array_equal(got["recall"][t], tpr)
        assert np.array_equal(got["fpr"][t], fpr) and np.array_equal(got["precision"][t], prec)
        B = h.shape[2]
        ap = 0.0
        for e in range(B - 1, -1, -1):       # thresholds from the top
            ap += (tpr[e] - tpr[e + 1]) * prec[e]
        assert got["average_precision"][t] == ap
        assert tpr[0] == fpr[0] == 1.0 and tpr[-1] == fpr[-1] == 0.0
    full = links.roc(h, h.shape[2], 8.0)
    assert np.array_equal(full["pairs"], h.sum((1, 2)) // 2) and np.array_equal(full["hist"], h)
    pooled = links.curves(h.sum(0, keepdims=True))
    for k, v in pooled.items():
        assert np.array_equal(np.asarray(full["pooled"][k]), v[0], equal_nan=True), k
    assert np.array_equal(full["pooled"]["hist"], h.sum(0))


@pytest.mark.parametrize("seed", range(4))
def test_the_bracket_contains_the_exact_auc_of_the_unbinned_scores(seed):
    rng = np.random.default_rng(seed)
    npos, nneg = 300 + 50 * seed, 700
    tp = rng.normal(0.8, 1.0 + seed, npos)
    tn = rng.normal(0.0, 1.0 + seed, nneg)
    tp[:40] = np.round(tp[:40], 1)           # exact ties between and within the classes
    tn[:90] = np.round(tn[:90], 1)
    wins, ties, pairs, exact = LR.auc_exact(tp, tn)
    assert ties > 0
    for bins in (1, 2, 7, 64, 1024, 2048):
        h = np.zeros((1, 2, bins), np.int64)
        np.add.at(h[0, 1], LR.bin_of(tp, bins), 1)
        np.add.at(h[0, 0], LR.bin_of(tn, bins), 1)
        c = links.curves(h)
        assert c["auc_lo"][0] <= exact <= c["auc_hi"][0], (bins, c["auc_lo"][0], exact, c["auc_hi"][0])
        if bins == 1:
            assert c["auc_lo"][0] == 0.0 and c["auc_hi"][0] == 1.0 and c["auc"][0] == 0.5


def test_the_bracket_when_every_score_ties_in_one_bin():
    tp, tn = np.full(50, 0.3), np.full(70, 0.3)
    _, ties, pairs, exact = LR.auc_exact(tp, tn)
    assert ties == pairs and exact == 0.5
    h = np.zeros((1, 2, 64), np.int64)
    b = int(LR.bin_of(0.3, 64))
    h[0, 1, b], h[0, 0, b] = 50, 70
    c = links.curves(h)
    assert c["auc_lo"][0] == 0.0 and c["auc_hi"][0] == 1.0 and c["auc"][0] == exact
    # beyond t_max every score shares the clamped end bin: the bracket says so
    h = np.zeros((1, 2, 64), np.int64)
    np.add.at(h[0, 1], LR.bin_of(np.linspace(9, 20, 50), 64), 1)
    np.add.at(h[0, 0], LR.bin_of(np.linspace(8.5, 30, 70), 64), 1)
    c = links.curves(h)
    assert c["auc_lo"][0] == 0.0 and c["auc_hi"][0] == 1.0


def test_one_class_slices_give_nan():
    h = _hists(5, T=3)
    h[0, 1] = 0          # no tie
    h[1, 0] = 0          # nothing but ties
    c = links.curves(h)
    for t in (0, 1):
        for k in links.SCALARS:
            assert np.isnan(c[k][t]), (t, k)
        for k in links.CURVES:
            assert np.isnan(c[k][t]).all(), (t, k)
    assert np.isfinite(c["auc"][2]) and np.isfinite(c["tpr"][2]).all()
    assert c["positives"].tolist() == [0, int(h[1, 1].sum()), int(h[2, 1].sum())]
    empty = links.roc(np.zeros((2, 2, 8), np.int64), 8, 8.0)
    assert np.isnan(empty["auc"]).all() and np.isnan(empty["pooled"]["auc"]) and empty["pairs"].tolist() == [0, 0]


def test_threshold_bin_and_capacity():
    h = _hists(9, T=5, bins=12, top=6)
    h[3] = 0
    for ties in (None, 0, 1):
        hh = h.sum(1) if ties is None else h[:, ties]
        for k in (1, 7, 40, 10 ** 6):
            bin_min, cap = links.threshold(h, k, ties)
            assert bin_min.dtype == np.int32 and cap.dtype == np.int64
            for t in range(h.shape[0]):
                above = [int(hh[t, b:].sum()) for b in range(12)]
                ok = [b for b in range(12) if above[b] >= k]
                want = max(ok) if ok else 0
                assert bin_min[t] == want and cap[t] == above[want], (ties, k, t)
                if ok:       # the k-th best lies in bin_min, and one bin less would not do
                    assert cap[t] >= k and (want == 11 or above[want + 1] < k)
                else:        # fewer than k candidates: all of them
                    assert cap[t] == int(hh[t].sum()) < k
    for bad in (0, -3):
        with pytest.raises(ValueError):
            links.threshold(h, bad)
    with pytest.raises(ValueError):
        links.threshold(h, 3, ties=2)


def test_top_k_orders_by_score_then_sender_then_receiver_and_pads():
    rng = np.random.default_rng(3)
    n0, n1 = 40, 3
    rec = np.zeros(n0 + n1, links.RECORD)
    rec["t"] = np.round(rng.normal(0, 1, n0 + n1), 1)          # many exact ties
    rec["sender"], rec["receiver"] = rng.integers(0, 6, n0 + n1), rng.integers(0, 6, n0 + n1)
    rec["tie"] = rng.integers(0, 2, n0 + n1)
    off = np.array([0, n0, n0, n0 + n1])
    got = links.top_k(rec, off, 5)
    assert got["score"].shape == (3, 5)
    for t in range(3):
        r = rec[off[t]:off[t + 1]]
        order = sorted(range(len(r)), key=lambda e: (-r["t"][e], r["sender"][e], r["receiver"][e]))[:5]
        m = len(order)
        assert np.array_equal(got["score"][t, :m], r["t"][order]) and np.isnan(got["score"][t, m:]).all()
        for k in ("sender", "receiver", "tie"):
            assert np.array_equal(got[k][t, :m], r[k][order]) and (got[k][t, m:] == -1).all()
    shuffled = rec.copy()
    shuffled[:n0] = rec[:n0][rng.permutation(n0)]
    again = links.top_k(shuffled, off, 5)
    for k in ("sender", "receiver", "score"):     # the order inside a region is free (duplicates aside)
        assert np.array_equal(again[k], got[k], equal_nan=True)
    assert np.allclose(links.phi(np.array([0.0, -40.0, 9.0])), [0.5, 0.0, 1.0]) and np.isnan(links.phi(np.array([np.nan]))[0])


def test_reference_top_k_and_histograms_on_a_small_case():
    X, S, B, sc = random_scores(CASES[0])
    h = LR.histograms(sc, 64)
    assert h.sum() == 5 * 4 and h[0, 1].sum() == B[:, :, 0].sum()
    top = LR.top_k(sc[0], 25)
    assert (top["sender"][20:] == -1).all() and np.isnan(top["score"][20:]).all()
    assert (np.diff(top["score"][:20]) <= 0).all()
    only = LR.top_k(sc[0], 3, ties=0)
    assert (only["tie"] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_T%d_r%d" % c)
def test_few_reference_scores_lie_within_delta_of_an_edge(case):
    """The condition of the GPU sandwich test: at most 1 % of a slice's entries
    lie within their bound of a bin edge, so the sandwich cannot go slack."""
    X, S, B, sc = random_scores(case)
    for bins in RANDOM_BINS:
        for t, d in enumerate(sc):
            share = LR.near_edge_share(d, bins)
            print(f"{case} bins {bins} slice {t}: {share:.4f} of the entries within delta of an edge; "
                  f"largest delta {d['delta'].max():.2e}")
            assert share <= 0.01, (case, bins, t, share)
            assert d["delta"].max() < 0.1 * (16.0 / bins)
