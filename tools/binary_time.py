"""Cost of a binary (probit) fit on the GPU: one ame_probit_fill call, one
ame_probit_score pass and the per-iteration fit() time, each at rho = 0 and at
rho = 0.5, with no mask and with the given share of the pairs hidden, beside the
unmasked Gaussian run with pipeline=False, speculate=False (a binary run sweeps
in order, so that run separates the cost of in-order sweeps from the cost of
the fill).  The Gaussian path is the code and the bits of the commit before
binary networks.

    python3 tools/binary_time.py [--n 1024 --T 128 --r 16 --hidden 0.1] [--out profiles/binary_config3.json]

HIP events around each launch, warm-up, median of repeated launches; fit() by
the host clock around fit(max_iter=iters) after a warm-up fit.  Reported, not
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


def _mask(n, T, frac, seed):
    g = torch.Generator()
    g.manual_seed(seed)
    m = torch.zeros(n, n, T, dtype=torch.bool)
    for t in range(T):   # slice by slice: the full (n, n, T) draw is not needed at once
        up = torch.triu(torch.rand(n, n, generator=g) < frac, 1)
        m[:, :, t] = up | up.T
    return m


def _fit_ms(vi, iters, rounds):
    vi.fit(max_iter=3, tolerance=0.0, verbose=False)
    torch.cuda.synchronize()
    per = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        vi.fit(max_iter=iters, tolerance=0.0, verbose=False)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3 / iters)
    return statistics.median(per), min(per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--hidden", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binary_config3.json"))
    a = ap.parse_args()
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI, _lib
    n, T, r = a.n, a.T, a.r
    dev = torch.device("cuda", 0)
    m = TemporalAMEModel(n, T, r, seed=42)
    m.generate_data_fast(device=dev)
    ties = (m.Y[..., 0] > 0).to("cpu")   # the sign of the generated Gaussian network

    def vi_of(**opts):
        vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.01, device=dev,
                                       engine_options=opts or None)
        vi.engine   # built now, while the model carries these settings
        return vi

    res = {"config": [n, T, r], "hidden_share": a.hidden, "iters": a.iters, "rounds": a.rounds,
           "reps": a.reps, "warmup": a.warmup}
    # the Gaussian network, unmasked, sweeps in order
    vi = vi_of(pipeline=False, speculate=False)
    res["fit_gaussian_inorder_ms_per_iter_median"], res["fit_gaussian_inorder_ms_per_iter_min"] = \
        _fit_ms(vi, a.iters, a.rounds)
    del vi
    mask = _mask(n, T, a.hidden, seed=11)
    for rho in (0.0, 0.5):
        for key, mk in (("nomask", None), ("hidden", mask)):
            m.set_binary(ties, rho=rho)
            m.set_missing(mk)
            vi = vi_of()
            eng = vi.engine
            tag = f"rho{rho:g}_{key}"
            res[f"fit_{tag}_ms_per_iter_median"], res[f"fit_{tag}_ms_per_iter_min"] = _fit_ms(vi, a.iters, a.rounds)
            res[f"fill_{tag}_ms_median"], res[f"fill_{tag}_ms_min"] = _time(eng.probit_fill, a.warmup, a.reps)
            res[f"score_{tag}_ms_median"], res[f"score_{tag}_ms_min"] = _time(vi.predictive_check, a.warmup, a.reps)
            if mk is not None:
                res["hidden_pairs"] = int(sum(eng.hidden_pairs))
            del vi, eng
    # bytes one fill writes: every off-diagonal float2 of the working network
    res["fill_bytes_written"] = T * n * (n - 1) * 8
    res["device"] = torch.cuda.get_device_name(dev)
    res["lib"] = _lib.build_hash()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
