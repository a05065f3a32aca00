"""Cost of hidden dyads on the GPU: one ame_fill_missing call (at the given share
of hidden pairs and at 0 %, which is the mask scan alone), ame_elbo with
swap_consistent = 0 beside the swap-consistent call, and the per-iteration
fit() time of a masked run beside the unmasked run with default options and
with pipeline=False, speculate=False (a masked run sweeps in order, so the
second separates the cost of in-order sweeps from the cost of the fill).  The
unmasked path is the code and the bits of the commit before hidden dyads.

    python3 tools/missing_time.py [--n 1024 --T 128 --r 16 --hidden 0.1] [--out profiles/missing_config3.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "missing_config3.json"))
    a = ap.parse_args()
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI, _lib
    n, T, r = a.n, a.T, a.r
    dev = torch.device("cuda", 0)
    m = TemporalAMEModel(n, T, r, seed=42)
    m.generate_data_fast(device=dev)

    def vi_of(mask, **opts):
        m.set_missing(mask)
        vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.01, device=dev,
                                       engine_options=opts or None)
        vi.engine   # built now, while the model carries this mask
        return vi

    res = {"config": [n, T, r], "hidden_share": a.hidden, "iters": a.iters, "rounds": a.rounds,
           "reps": a.reps, "warmup": a.warmup}
    # unmasked: default options, then in-order sweeps
    for key, opts in (("fit_unmasked_default", {}),
                      ("fit_unmasked_inorder", dict(pipeline=False, speculate=False))):
        vi = vi_of(None, **opts)
        med, lo = _fit_ms(vi, a.iters, a.rounds)
        res[key + "_ms_per_iter_median"], res[key + "_ms_per_iter_min"] = med, lo
        if key == "fit_unmasked_default":
            eng = vi.engine
            eng.discard_speculation()
            assert eng.swap_consistent
            res["elbo_swap1_ms_median"], res["elbo_swap1_ms_min"] = _time(eng.launch_elbo, a.warmup, a.reps)
        del vi
    # masked at the given share, then nothing hidden (the mask scan alone)
    for key, frac in (("hidden", a.hidden), ("none", 0.0)):
        vi = vi_of(_mask(n, T, frac, seed=11))
        eng = vi.engine
        res[f"hidden_pairs_{key}"] = int(sum(eng.hidden_pairs))
        if key == "hidden":
            med, lo = _fit_ms(vi, a.iters, a.rounds)
            res["fit_masked_ms_per_iter_median"], res["fit_masked_ms_per_iter_min"] = med, lo
            assert not eng.swap_consistent
            res["elbo_swap0_ms_median"], res["elbo_swap0_ms_min"] = _time(eng.launch_elbo, a.warmup, a.reps)
        else:
            vi.fit(max_iter=1, tolerance=0.0, verbose=False)
        med, lo = _time(eng.fill_missing, a.warmup, a.reps)
        res[f"fill_{key}_ms_median"], res[f"fill_{key}_ms_min"] = med, lo
        del vi, eng
    res["device"] = torch.cuda.get_device_name(dev)
    res["lib"] = _lib.build_hash()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
