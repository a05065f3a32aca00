"""Cost of the residual diagnostics of a Gaussian fit on the GPU: one
ame_resid_nodes pass (the per-node sums behind node_check), one ame_resid_hist
pass (residual_histogram), one ame_resid_select pass (the records behind
top_residuals) and, as the yardstick, ame_predict's scoring pass (MODE 0) of
the same run: the same feature rows and tile products.  node_check,
residual_histogram and top_residuals themselves by the host clock (they add the
copies, the host finish and, for top_residuals, both passes and the sort).

    python3 tools/resid_time.py [--n 1024 --T 128 --r 16 --bins 1024 --k 100] [--out profiles/resid_config3.json]

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
    ap.add_argument("--m2-max", type=float, default=64.0)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resid_config3.json"))
    a = ap.parse_args()
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI, _lib, residuals
    n, T, r = a.n, a.T, a.r
    dev = torch.device("cuda", 0)
    m = TemporalAMEModel(n, T, r, seed=42)
    m.generate_data_fast(device=dev)
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.01, device=dev)
    vi.fit(max_iter=a.iters, tolerance=0.0, verbose=False)
    eng = vi.engine
    eng.discard_speculation()
    Yt, Mt, sel = eng.mask_args(0)
    x, cov = eng.x_a, eng.cov
    res = {"config": [n, T, r], "bins": a.bins, "m2_max": a.m2_max, "k": a.k, "fit_iters": a.iters,
           "reps": a.reps, "warmup": a.warmup}
    res["score_ms_median"], res["score_ms_min"] = _time(
        lambda: eng.predict(x, cov, Yt=Yt, Mt=Mt, mask_select=sel), a.warmup, a.reps)
    res["nodes_ms_median"], res["nodes_ms_min"] = _time(
        lambda: eng.resid_nodes(x, cov, Yt, Mt=Mt, mask_select=sel), a.warmup, a.reps)
    res["hist_ms_median"], res["hist_ms_min"] = _time(
        lambda: eng.resid_hist(x, cov, Yt, a.bins, a.m2_max, Mt=Mt, mask_select=sel), a.warmup, a.reps)
    hist = eng.resid_hist(x, cov, Yt, a.bins, a.m2_max, Mt=Mt, mask_select=sel).to("cpu").numpy()
    bin_min, cap = residuals.threshold(hist, a.k)
    off = [0]
    for c in cap.tolist():
        off.append(off[-1] + int(c))
    res["select_records"] = off[-1]
    res["select_ms_median"], res["select_ms_min"] = _time(
        lambda: eng.resid_select(x, cov, Yt, a.bins, a.m2_max, bin_min, off, Mt=Mt, mask_select=sel),
        a.warmup, a.reps)
    kw = dict(bins=a.bins, m2_max=a.m2_max)
    res["node_check_host_ms_median"], res["node_check_host_ms_min"] = _host_ms(
        lambda: vi.node_check(), a.warmup, a.reps)
    res["residual_histogram_host_ms_median"], res["residual_histogram_host_ms_min"] = _host_ms(
        lambda: vi.residual_histogram(**kw), a.warmup, a.reps)
    res["top_residuals_host_ms_median"], res["top_residuals_host_ms_min"] = _host_ms(
        lambda: vi.top_residuals(k=a.k, **kw), a.warmup, a.reps)
    for name in ("nodes", "hist", "select"):
        res[f"{name}_over_score"] = res[f"{name}_ms_median"] / res["score_ms_median"]
    res["chunks"] = {name: -(-T // eng._slice_chunk(getattr(eng.L, f"ame_{q}_work_size"), T)[0])
                     for name, q in (("score", "predict"), ("nodes", "resid_nodes"), ("hist", "resid_hist"),
                                     ("select", "resid_select"))}
    res["pairs"] = int(hist.sum())
    res["end_bin_pairs"] = int(hist[:, -1].sum())
    res["nonzero_bins_per_slice_mean"] = float((hist > 0).sum(1).mean())
    res["device"] = torch.cuda.get_device_name(dev)
    res["lib"] = _lib.build_hash()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
