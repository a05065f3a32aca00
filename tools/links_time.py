"""Cost of ranking the links of a binary network on the GPU: one ame_probit_rank
pass (the class histograms behind link_roc), one ame_probit_select pass (the
records behind top_links) and, as the yardstick, one ame_probit_score pass of
the same run: the same feature rows and tile products with a heavier fp64
epilogue.  link_roc and top_links themselves by the host clock (they add the
copy of the histograms, the host finish and, for top_links, both passes and
the sort).

    python3 tools/links_time.py [--n 1024 --T 128 --r 16 --bins 1024 --k 1000] [--out profiles/links_config3.json]

HIP events around each call, warm-up, median of repeated calls.  Reported, not
gated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-temporal-ame-svi_amd"))

import torch  # noqa: E402


def _time(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def _host_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--t-max", type=float, default=8.0)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "links_config3.json"))
    a = ap.parse_args()
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI, _lib, links
    n, T, r = a.n, a.T, a.r
    dev = torch.device("cuda", 0)
    m = TemporalAMEModel(n, T, r, seed=42)
    m.generate_data_fast(device=dev)
    ties = (m.Y[..., 0] > 0).to("cpu")   # the sign of the generated Gaussian network
    m.set_binary(ties, rho=0.0)
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.01, device=dev)
    vi.fit(max_iter=a.iters, tolerance=0.0, verbose=False)
    eng = vi.engine
    eng.discard_speculation()
    Yt, Mt, sel = eng.mask_args(0)
    x, cov = eng.x_a, eng.cov
    res = {"config": [n, T, r], "bins": a.bins, "t_max": a.t_max, "k": a.k, "fit_iters": a.iters,
           "reps": a.reps, "warmup": a.warmup}
    res["score_ms_median"], res["score_ms_min"] = _time(
        lambda: eng.probit_score(x, cov, Yt, Mt=Mt, mask_select=sel), a.warmup, a.reps)
    res["rank_ms_median"], res["rank_ms_min"] = _time(
        lambda: eng.probit_rank(x, cov, Yt, a.bins, a.t_max, Mt=Mt, mask_select=sel), a.warmup, a.reps)
    hist = eng.probit_rank(x, cov, Yt, a.bins, a.t_max, Mt=Mt, mask_select=sel).to("cpu").numpy()
    bin_min, cap = links.threshold(hist, a.k)
    off = [0]
    for c in cap.tolist():
        off.append(off[-1] + int(c))
    res["select_records"] = off[-1]
    res["select_ms_median"], res["select_ms_min"] = _time(
        lambda: eng.probit_select(x, cov, Yt, a.bins, a.t_max, bin_min, off, Mt=Mt, mask_select=sel),
        a.warmup, a.reps)
    res["link_roc_host_ms_median"], res["link_roc_host_ms_min"] = _host_ms(
        lambda: vi.link_roc(bins=a.bins, t_max=a.t_max), a.warmup, a.reps)
    res["top_links_host_ms_median"], res["top_links_host_ms_min"] = _host_ms(
        lambda: vi.top_links(k=a.k, bins=a.bins, t_max=a.t_max), a.warmup, a.reps)
    res["rank_over_score"] = res["rank_ms_median"] / res["score_ms_median"]
    res["select_over_score"] = res["select_ms_median"] / res["score_ms_median"]
    # what the rank pass adds to the tile products: LDS atomics (entries) and the global flush
    res["entries"] = int(hist.sum())
    res["nonzero_bins_per_slice_mean"] = float((hist > 0).sum((1, 2)).mean())
    roc = links.roc(hist, a.bins, a.t_max)
    res["pooled_auc"] = roc["pooled"]["auc"]
    res["pooled_auc_bracket"] = roc["pooled"]["auc_hi"] - roc["pooled"]["auc_lo"]
    res["device"] = torch.cuda.get_device_name(dev)
    res["lib"] = _lib.build_hash()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
