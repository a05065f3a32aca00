"""Time of the three goodness-of-fit kernels (ame_net_moments, ame_net_triads,
ame_simulate) on the GPU and of one vi.gof(n_sim=...) by the host clock: HIP
events around each launch, warm-up, median of repeated launches.

    python3 tools/gof_time.py [--n 1024 --T 128 --r 16 --n-sim 8] [--out profiles/gof_config3.json]

Bytes are the algorithmic traffic: one packed network read by the moments pass,
one written by the simulate pass (the states are n d floats per slice, counted
too); against the HBM peak (8.0 TB/s spec, 6.29 TB/s measured float4 copy).
Flops of the triad pass: two n x n x n products per slice, 4 n^3 T, against the
157.3 TFLOP/s fp32-MFMA peak; its compulsory bytes are one network.  Reported,
not gated."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-temporal-ame-svi_amd"))

import torch  # noqa: E402

HBM_SPEC, HBM_COPY, MFMA_F32 = 8.0e12, 6.29e12, 157.3e12


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
    ap.add_argument("--n-sim", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gof_config3.json"))
    a = ap.parse_args()
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI, _lib
    n, T, r = a.n, a.T, a.r
    dev = torch.device("cuda", 0)
    m = TemporalAMEModel(n, T, r, seed=42)
    m.generate_data_fast(device=dev)
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.01, device=dev)
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    eng = vi.engine
    eng.discard_speculation()
    torch.cuda.synchronize()
    L = _lib.lib()
    dims = eng.dims
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    mw = int(L.ame_net_moments_work_size(ctypes.byref(dims)))
    tw = int(L.ame_net_triads_work_size(ctypes.byref(dims)))
    mwork = torch.empty(mw, dtype=torch.float64, device=dev)
    twork = torch.empty(tw, dtype=torch.float64, device=dev)
    node = torch.empty(T, n, 2, dtype=torch.float64, device=dev)
    sl = torch.empty(T, 2, dtype=torch.float64, device=dev)
    tri = torch.empty(T, 2, dtype=torch.float64, device=dev)
    sim = torch.empty_like(eng.Yt)
    lr = (ctypes.c_double * 3)(1.0, 0.3, 0.9)

    def moments():
        args = _lib.ame_moments_args(Yt=_ptr(eng.Yt), node=_ptr(node), slice=_ptr(sl), work=_ptr(mwork),
                                     work_doubles=mw)
        _lib.check(L.ame_net_moments(ctypes.byref(dims), ctypes.byref(args), sp), "ame_net_moments")

    moments()
    center = (node[:, :, 0].sum(dim=1) / float(n * (n - 1))).float().contiguous()

    def triads():
        args = _lib.ame_triads_args(Yt=_ptr(eng.Yt), center=_ptr(center), tri=_ptr(tri), work=_ptr(twork),
                                    work_doubles=tw)
        _lib.check(L.ame_net_triads(ctypes.byref(dims), ctypes.byref(args), sp), "ame_net_triads")

    def simulate():
        args = _lib.ame_simulate_args(x=_ptr(eng.x_a), lr=lr, seed=7, sample=1, Yt_out=_ptr(sim))
        _lib.check(L.ame_simulate(ctypes.byref(dims), ctypes.byref(args), sp), "ame_simulate")

    mo_med, mo_min = _time(moments, a.warmup, a.reps)
    tr_med, tr_min = _time(triads, a.warmup, a.reps)
    si_med, si_min = _time(simulate, a.warmup, a.reps)
    vi.gof(n_sim=1, seed=0)          # warm-up: buffers, Cholesky factors' kernels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vi.gof(n_sim=a.n_sim, seed=0)
    torch.cuda.synchronize()
    gof_s = time.perf_counter() - t0
    plane = 4.0 * T * n * eng.ny * 2          # bytes of one packed network
    flops = 4.0 * float(n) ** 3 * T

    def bw(nbytes, ms):
        tbs = nbytes / (ms * 1e-3) / 1e12
        return {"bytes": nbytes, "tbs": tbs, "frac_8tbs": tbs * 1e12 / HBM_SPEC,
                "frac_6.29tbs": tbs * 1e12 / HBM_COPY}

    tf = flops / (tr_med * 1e-3)
    res = {"config": [n, T, r], "rounds": a.reps, "warmup": a.warmup,
           "moments_ms_median": mo_med, "moments_ms_min": mo_min, "moments": bw(plane, mo_med),
           "triads_ms_median": tr_med, "triads_ms_min": tr_min,
           "triads": {"flops": flops, "tflops": tf / 1e12, "frac_157.3tf": tf / MFMA_F32, **bw(plane, tr_med)},
           "simulate_ms_median": si_med, "simulate_ms_min": si_min,
           "simulate": bw(plane + 4.0 * T * n * eng.d, si_med),
           "gof_n_sim": a.n_sim, "gof_host_s": gof_s, "gof_host_s_per_network": gof_s / (a.n_sim + 1),
           "device": torch.cuda.get_device_name(dev), "lib": _lib.build_hash()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
