"""Time of ame_covar_stats (G alone, as every M-step runs it; G and H, the first
call of an engine) and of ame_covar_resid alone on the GPU, beside the dyad
pass of ame_mstep_stats in the same run: HIP events around each launch,
warm-up, median of repeated launches.

    python3 tools/covar_time.py [--n 1024 --T 128 --r 16 --p 4] [--out profiles/covar_config3.json]

Bytes are the algorithmic reads: the upper half of the residual plane and of
each of the p covariate planes for the G pass ((1 + p) / 2 packed planes), p
half planes for H counted once, 1 + p planes read and one written for the
residual pass; against the HBM peak (8.0 TB/s spec, 6.29 TB/s measured float4
copy).  Reported, not gated."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-temporal-ame-svi_amd"))

import torch  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--p", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covar_config3.json"))
    a = ap.parse_args()
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI, _lib
    n, T, r, p = a.n, a.T, a.r, a.p
    dev = torch.device("cuda", 0)
    m = TemporalAMEModel(n, T, r, seed=42)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    W = torch.randn(p, n, n, T, 2, generator=g, device=dev)
    m.set_covariates(W, beta=[0.5 * (-1) ** k / (k + 1) for k in range(p)])
    del W
    m.generate_data_fast(device=dev)
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.01, device=dev)
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    eng = vi.engine
    eng.discard_speculation()
    torch.cuda.synchronize()
    L = _lib.lib()
    dims = eng.dims
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ws = int(L.ame_covar_work_size(ctypes.byref(dims), p))
    work = torch.empty(ws, dtype=torch.float64, device=dev)
    G = torch.empty(T, p, 2, 2, dtype=torch.float64, device=dev)
    H = torch.empty(T, p, p, 2, 2, dtype=torch.float64, device=dev)
    out = torch.empty_like(eng.Yt)
    beta = (ctypes.c_double * p)(*eng.beta.tolist())

    def covar(with_g, with_h):
        args = _lib.ame_covar_args(x=_ptr(eng.x_a), Yt=_ptr(eng.Yt), Wt=_ptr(eng.Wt), p=p,
                                   G=_ptr(G) if with_g else None, H=_ptr(H) if with_h else None,
                                   work=_ptr(work), work_doubles=ws)
        _lib.check(L.ame_covar_stats(ctypes.byref(dims), ctypes.byref(args), sp), "ame_covar_stats")

    def resid():
        _lib.check(L.ame_covar_resid(ctypes.byref(dims), _ptr(eng.Yt_raw), _ptr(eng.Wt), beta, p,
                                     _ptr(out), sp), "ame_covar_resid")

    mwork = torch.empty(int(L.ame_mstep_work_size(ctypes.byref(dims))), dtype=torch.float64, device=dev)
    dyad = torch.empty(T, 4, dtype=torch.float64, device=dev)

    def mstep_dyad():
        args = _lib.ame_mstep_args(x=_ptr(eng.x_a), cov=_ptr(eng.cov), Yt=_ptr(eng.Yt), state=None,
                                   dyad=_ptr(dyad), work=_ptr(mwork))
        _lib.check(L.ame_mstep_stats(ctypes.byref(dims), ctypes.byref(args), sp), "ame_mstep_stats")

    g_med, g_min = _time(lambda: covar(True, False), a.warmup, a.reps)
    gh_med, gh_min = _time(lambda: covar(True, True), a.warmup, a.reps)
    h_med, h_min = _time(lambda: covar(False, True), a.warmup, a.reps)
    rs_med, rs_min = _time(resid, a.warmup, a.reps)
    dy_med, dy_min = _time(mstep_dyad, a.warmup, a.reps)
    plane = 4.0 * T * n * eng.ny * 2          # bytes of one packed plane
    g_bytes = (1 + p) / 2.0 * plane
    h_bytes = p / 2.0 * plane
    rs_bytes = (2 + p) * plane

    def bw(nbytes, ms):
        tbs = nbytes / (ms * 1e-3) / 1e12
        return {"bytes": nbytes, "tbs": tbs, "frac_8tbs": tbs * 1e12 / HBM_SPEC,
                "frac_6.29tbs": tbs * 1e12 / HBM_COPY}

    res = {"config": [n, T, r], "p": p, "rounds": a.reps, "warmup": a.warmup,
           "stats_g_ms_median": g_med, "stats_g_ms_min": g_min, "stats_g": bw(g_bytes, g_med),
           "stats_gh_ms_median": gh_med, "stats_gh_ms_min": gh_min,
           "stats_gh": bw(g_bytes + h_bytes, gh_med),
           "stats_h_ms_median": h_med, "stats_h_ms_min": h_min, "stats_h": bw(h_bytes, h_med),
           "resid_ms_median": rs_med, "resid_ms_min": rs_min, "resid": bw(rs_bytes, rs_med),
           "mstep_dyad_ms_median": dy_med, "mstep_dyad_ms_min": dy_min,
           "device": torch.cuda.get_device_name(dev), "lib": _lib.build_hash()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
