"""Time of ame_smooth's stages with a mask (observed partners only) beside the
unmasked stages, in one run on the GPU: HIP events around each launch, warm-up,
median of repeated launches, after one fit() iteration.

    python3 tools/smooth_masked_time.py [--n 1024 --T 128 --r 16 --hidden 0.1]
                                        [--out profiles/smooth_masked_config3.json]

Observation stage with `Mt` set: the unmasked stage's two kernels (h_obs now
also reads one mask word per 64 partners) plus ame_smooth_hgram_kernel, which
gathers each node's hidden partners' (U, V) rows and writes H, (1+2r)^2 doubles
per (node, slice).  Its useful flops are counted as hidden ordered pairs x
2r (2r + 1) (one multiply-add per lower-triangle entry); what the MFMA steps
issue is chunks x tiles x 2 * 16 * 16 * 4.  Its bytes: the gathered rows (4 * 2r
each, mostly from L2: a slice's means are n * d * 4 bytes) and H written once.
The stage is timed with the 10 % mask and with an all-False mask (the walk over
the mask words and the write of a zero H alone).  The solve stage reads H once
more than the unmasked one.  Reported, not gated."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-temporal-ame-svi_amd"))

import torch  # noqa: E402

HBM_COPY = 6.29e12
FP64_MATRIX_PEAK = 78.6e12


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


def _random_mask(n, T, frac, dev):
    """(n, n, T) uint8 on the device: each unordered pair of each slice hidden with probability frac."""
    g = torch.Generator(device=dev).manual_seed(7)
    up = torch.triu(torch.ones(n, n, dtype=torch.bool, device=dev), 1)[:, :, None]
    m = (torch.rand(n, n, T, device=dev, generator=g) < frac) & up
    return (m | m.transpose(0, 1)).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--hidden", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_masked_config3.json"))
    a = ap.parse_args()
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI, _lib
    n, T, r = a.n, a.T, a.r
    d, W = 2 + 2 * r, 1 + 2 * r
    dev = torch.device("cuda", 0)
    m = TemporalAMEModel(n, T, r, seed=42)
    m.generate_data_fast(device=dev)
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.01, device=dev)
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    eng = vi.engine
    eng.discard_speculation()
    Mt_hid, pairs, deg = eng.pack_mask(_random_mask(n, T, a.hidden, dev))
    Mt_none, _, _ = eng.pack_mask(torch.zeros(n, n, T, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    hidden_ordered = 2 * int(pairs.sum().item())
    # chunks of four partners per (node, slice)
    chunks = int((((n - 1) - deg.long()) + 3).div(4, rounding_mode="floor").sum().item())
    L = _lib.lib()
    dims = eng.dims
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ws = int(L.ame_smooth_masked_work_size(ctypes.byref(dims), n))
    ws_plain = int(L.ame_smooth_work_size(ctypes.byref(dims), n))
    work = torch.empty(ws, dtype=torch.float64, device=dev)
    mean = torch.empty(T, n, d, device=dev)
    cov = torch.empty(T, n, d, d, device=dev)
    cross = torch.empty(T, n, d, d, device=dev)
    lag = torch.empty(T, d, d, dtype=torch.float64, device=dev)
    fail = torch.zeros(_lib.AME_SMOOTH_FAIL_WORDS, dtype=torch.int32, device=dev)

    def stage(which, Mt):
        args = _lib.ame_smooth_args(
            x=_ptr(eng.x_a), Yt=_ptr(eng.Yt), consts=_ptr(eng.consts), rinv=eng.C.rinv4(), i0=0, i1=n,
            stages=which, mean=_ptr(mean), cov=_ptr(cov), cross=_ptr(cross), lag_sum=_ptr(lag),
            fail=_ptr(fail), work=_ptr(work), work_doubles=ws, Mt=_ptr(Mt))
        _lib.check(L.ame_smooth(ctypes.byref(dims), ctypes.byref(args), sp), "ame_smooth")

    OBS, SOLVE = _lib.AME_SMOOTH_STAGE_OBS, _lib.AME_SMOOTH_STAGE_SOLVE
    res = {"config": [n, T, r], "hidden_fraction": a.hidden, "rounds": a.reps, "warmup": a.warmup}
    for key, which, Mt in (("obs_unmasked", OBS, None), ("solve_unmasked", SOLVE, None),
                           ("obs_all_false", OBS, Mt_none), ("obs_hidden", OBS, Mt_hid),
                           ("solve_hidden", SOLVE, Mt_hid)):
        if which == SOLVE:      # the solve stage reads what an observation stage of the same call left
            stage(OBS, Mt)
        med, mn = _time(lambda: stage(which, Mt), a.warmup, a.reps)
        res[key + "_ms_median"], res[key + "_ms_min"] = med, mn
    failed = int(fail.cpu()[0])
    ntl = (2 * r + 15) // 16
    ntl = ntl * (ntl + 1) // 2
    extra = max(res["obs_hidden_ms_median"] - res["obs_unmasked_ms_median"], 1e-9) * 1e-3
    flop = float(hidden_ordered) * 2 * r * (2 * r + 1)
    issued = float(chunks) * ntl * 2 * 16 * 16 * 4
    gather_bytes = float(hidden_ordered) * 4 * 2 * r
    h_bytes = 8.0 * n * T * W * W
    res.update({
        "hidden_ordered_pairs": hidden_ordered, "chunks_of_four": chunks, "lower_triangle_tiles": ntl,
        "hgram_flop": flop, "hgram_flop_issued": issued, "hgram_gather_bytes": gather_bytes,
        "hgram_H_bytes": h_bytes, "mask_bytes": 8.0 * T * n * ((n + 63) // 64),
        "obs_extra_ms_hidden": extra * 1e3,
        "obs_extra_ms_all_false": res["obs_all_false_ms_median"] - res["obs_unmasked_ms_median"],
        "hgram_tflops_useful": flop / extra / 1e12, "hgram_tflops_issued": issued / extra / 1e12,
        "hgram_frac_fp64_matrix_peak_issued": issued / extra / FP64_MATRIX_PEAK,
        "hgram_H_write_tbs": h_bytes / extra / 1e12, "hgram_H_write_frac_6.29tbs": h_bytes / extra / HBM_COPY,
        "dense_masked_gemm_flop": float(T) * n * n * 2 * r * (2 * r + 1),
        "solve_extra_ms_hidden": res["solve_hidden_ms_median"] - res["solve_unmasked_ms_median"],
        "failed_nodes": failed, "work_doubles_all_nodes": ws, "work_doubles_unmasked": ws_plain,
        "device": torch.cuda.get_device_name(dev), "lib": _lib.build_hash()})
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
