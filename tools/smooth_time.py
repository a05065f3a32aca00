"""Time of the two stages of ame_smooth alone on the GPU: HIP events around each
launch, warm-up, median of repeated launches, after one fit() iteration.

    python3 tools/smooth_time.py [--n 1024 --T 128 --r 16] [--out profiles/smooth_config3.json]

Observation stage (AME_SMOOTH_STAGE_OBS): the per-slice Gram statistics and
h_obs of every node, one pass over Yt; its bytes are Yt read once plus the
means and the h_obs rows written, against the HBM peak (8.0 TB/s spec, 6.29 TB/s
measured float4 copy).  Solve stage (AME_SMOOTH_STAGE_SOLVE): one workgroup per
node, forward and backward over t, then the lag_sum reduction; its flops are
counted as 12 d^3 per node and slice (six d x d x d products).  Both stages
run as ONE call over all nodes on a scratch buffer sized for that; `smooth_ms`
is vi.smooth() as the library chunks it within its scratch budget.
Reported, not gated."""
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
FP64_VECTOR_PEAK = 78.6e12


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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_config3.json"))
    a = ap.parse_args()
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI, _lib
    n, T, r = a.n, a.T, a.r
    d = 2 + 2 * r
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
    ws = int(L.ame_smooth_work_size(ctypes.byref(dims), n))
    work = torch.empty(ws, dtype=torch.float64, device=dev)
    mean = torch.empty(T, n, d, device=dev)
    cov = torch.empty(T, n, d, d, device=dev)
    cross = torch.empty(T, n, d, d, device=dev)
    lag = torch.empty(T, d, d, dtype=torch.float64, device=dev)
    fail = torch.zeros(_lib.AME_SMOOTH_FAIL_WORDS, dtype=torch.int32, device=dev)

    def stage(which):
        args = _lib.ame_smooth_args(
            x=_ptr(eng.x_a), Yt=_ptr(eng.Yt), consts=_ptr(eng.consts), rinv=eng.C.rinv4(), i0=0, i1=n,
            stages=which, mean=_ptr(mean), cov=_ptr(cov), cross=_ptr(cross), lag_sum=_ptr(lag),
            fail=_ptr(fail), work=_ptr(work), work_doubles=ws)
        _lib.check(L.ame_smooth(ctypes.byref(dims), ctypes.byref(args), sp), "ame_smooth")

    ob_med, ob_min = _time(lambda: stage(_lib.AME_SMOOTH_STAGE_OBS), a.warmup, a.reps)
    so_med, so_min = _time(lambda: stage(_lib.AME_SMOOTH_STAGE_SOLVE), a.warmup, a.reps)
    failed = int(fail.cpu()[0])
    all_med, all_min = _time(lambda: eng.smooth(check=False), 1, max(3, a.reps // 4))
    y_bytes = 4.0 * T * n * eng.ny * 2
    obs_bytes = y_bytes + 4.0 * T * n * d + 8.0 * T * n * d
    flops = 12.0 * d ** 3 * n * T
    # J^-1 written and read once, X written and read once (lag_sum), three fp32 outputs
    solve_bytes = 8.0 * n * T * d * d * 4 + 4.0 * n * T * d * d * 2
    res = {"config": [n, T, r], "rounds": a.reps, "warmup": a.warmup,
           "obs_ms_median": ob_med, "obs_ms_min": ob_min, "obs_bytes": obs_bytes, "y_bytes": y_bytes,
           "obs_tbs": obs_bytes / (ob_med * 1e-3) / 1e12,
           "obs_frac_6.29tbs": obs_bytes / (ob_med * 1e-3) / HBM_COPY,
           "obs_flop": 2.0 * T * n * n * d, "obs_tflops": 2.0 * T * n * n * d / (ob_med * 1e-3) / 1e12,
           "solve_ms_median": so_med, "solve_ms_min": so_min, "solve_flop": flops,
           "solve_tflops": flops / (so_med * 1e-3) / 1e12,
           "solve_frac_fp64_vector_peak": flops / (so_med * 1e-3) / FP64_VECTOR_PEAK,
           "solve_bytes": solve_bytes, "solve_tbs": solve_bytes / (so_med * 1e-3) / 1e12,
           "solve_lds_bytes": int(L.ame_smooth_lds_bytes(r)), "failed_nodes": failed,
           "smooth_ms_median": all_med, "smooth_ms_min": all_min, "smooth_chunk_nodes": eng.smooth_chunk(),
           "work_doubles_all_nodes": ws,
           "device": torch.cuda.get_device_name(dev), "lib": _lib.build_hash()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
