"""Time of the two passes of ame_mstep_stats alone on the GPU: HIP events
around each launch, warm-up, median of repeated launches.

    python3 tools/mstep_time.py [--n 1024 --T 128 --r 16] [--out profiles/mstep_config3.json]

State pass (state != NULL, dyad == NULL): bytes = the covariances and means
read once plus the chunk partials written and read, against the HBM peak
(8.0 TB/s spec, 6.29 TB/s measured float4 copy).  Dyad pass (dyad != NULL,
state == NULL): beside ame_predict's scoring pass (sums, three levels) on the
same state, with which it shares the feature kernel and the five tile products.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mstep_config3.json"))
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
    work = torch.empty(int(L.ame_mstep_work_size(ctypes.byref(dims))), dtype=torch.float64, device=dev)
    state = torch.empty(T, 2, d, d, dtype=torch.float64, device=dev)
    dyad = torch.empty(T, 4, dtype=torch.float64, device=dev)

    def mstep(with_state, with_dyad):
        args = _lib.ame_mstep_args(x=_ptr(eng.x_a), cov=_ptr(eng.cov), Yt=_ptr(eng.Yt),
                                   state=_ptr(state) if with_state else None,
                                   dyad=_ptr(dyad) if with_dyad else None, work=_ptr(work))
        _lib.check(L.ame_mstep_stats(ctypes.byref(dims), ctypes.byref(args), sp), "ame_mstep_stats")

    pwork = torch.empty(int(L.ame_predict_work_size(ctypes.byref(dims))), dtype=torch.float64, device=dev)
    sums = torch.empty(T, _lib.AME_PREDICT_SUMS, dtype=torch.float64, device=dev)
    _, zsq, csq = vi._thresholds((0.5, 0.9, 0.95))

    def predict():
        args = _lib.ame_predict_args(
            x=_ptr(eng.x_a), cov=_ptr(eng.cov), Yt=_ptr(eng.Yt), noise=eng.noise4(True), n_levels=3,
            zsq=(ctypes.c_double * _lib.AME_PREDICT_MAX_LEVELS)(*zsq),
            csq=(ctypes.c_double * _lib.AME_PREDICT_MAX_LEVELS)(*csq), sums=_ptr(sums), work=_ptr(pwork))
        _lib.check(L.ame_predict(ctypes.byref(dims), ctypes.byref(args), sp), "ame_predict")

    st_med, st_min = _time(lambda: mstep(True, False), a.warmup, a.reps)
    dy_med, dy_min = _time(lambda: mstep(False, True), a.warmup, a.reps)
    pr_med, pr_min = _time(predict, a.warmup, a.reps)
    chunks = (n + 31) // 32
    read = 4.0 * T * n * d * d + 2 * 4.0 * T * n * d
    partial = 8.0 * T * chunks * 2 * d * d
    out_bytes = 8.0 * T * 2 * d * d
    total = read + 2 * partial + out_bytes
    res = {"config": [n, T, r], "rounds": a.reps, "warmup": a.warmup,
           "state_ms_median": st_med, "state_ms_min": st_min,
           "state_bytes": total, "state_cov_bytes": 4.0 * T * n * d * d,
           "state_tbs": total / (st_med * 1e-3) / 1e12,
           "state_frac_8tbs": total / (st_med * 1e-3) / HBM_SPEC,
           "state_frac_6.29tbs": total / (st_med * 1e-3) / HBM_COPY,
           "dyad_ms_median": dy_med, "dyad_ms_min": dy_min,
           "predict_scoring_ms_median": pr_med, "predict_scoring_ms_min": pr_min,
           "dyad_over_predict": dy_med / pr_med,
           "device": torch.cuda.get_device_name(dev), "lib": _lib.build_hash()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
