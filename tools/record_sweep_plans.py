"""Record the sweep launch plan a real DeviceEngine makes, case by case, on the GPU.

    python3 tools/record_sweep_plans.py --out plans.json
    python3 tools/record_sweep_plans.py --fixture tests/golden/sweep_plans.json --out new.json

Without --fixture: builds the engine of every case below (zero data: nothing is
launched), records its plan as ``parent_plan`` beside the case's inputs, frees
it and goes on.  Run on the commit whose plans are to be pinned; it reads only
the engine's public plan attributes, ``sweep_work``, ``elbo_stream`` and _lib.

With --fixture (a tree that has ame_amd.plan): builds each engine again, stops
if its plan differs from the fixture's ``parent_plan``, and stores beside each
case the ``caps_log``: every question plan_sweeps asked LibCaps and the answer.
tests/test_sweep_plan.py replays that log on the CPU.

One process; each case runs under its own time limit (SIGALRM) and the first
failure ends the run."""
import argparse
import gc
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-temporal-ame-svi_amd"))

import torch  # noqa: E402

# (name, n, r, T_local, T_total, t_begin, device_sharers, options)
CASES = [
    ("config3", 1024, 16, 128, 128, 0, 1, {}),
    ("config4_one_gpu", 1024, 16, 512, 512, 0, 1, {}),
    ("round6_clamp_rank0", 1024, 16, 256, 512, 0, 2, {"slice_group": 128}),
    ("round6_clamp_rank1", 1024, 16, 256, 512, 256, 2, {"slice_group": 128}),
    ("config5_full", 4096, 32, 256, 256, 0, 1, {}),
    ("config5_rank_auto", 4096, 32, 32, 256, 0, 1, {"sweep_kernel": 0}),
    ("config5_rank_k22", 4096, 32, 32, 256, 0, 1, {"sweep_kernel": 22}),
    ("config5_rank_k23", 4096, 32, 32, 256, 0, 1, {"sweep_kernel": 23}),
    ("config5_rank_k24", 4096, 32, 32, 256, 0, 1, {"sweep_kernel": 24}),
    ("config5_rank_k24_elbo_cus", 4096, 32, 32, 256, 0, 1, {"sweep_kernel": 24, "elbo_cus": 32}),
    ("tiny", 128, 4, 8, 8, 0, 1, {}),
    ("n90_depth3", 90, 4, 40, 40, 0, 1, {"spec_depth": 3}),
    ("n90_no_pipeline_depth2", 90, 4, 40, 40, 0, 1, {"pipeline": False, "spec_depth": 2}),
    ("n90_group2", 90, 4, 40, 40, 0, 1, {"slice_group": 2}),
    # shapes of tests/test_gpu_large.py
    ("v2_hbm_request", 50, 4, 4, 4, 0, 1, {"sweep_kernel": 21}),
    ("v2_lds_request", 64, 8, 5, 5, 0, 1, {"sweep_kernel": 20}),
    ("v2_single_request", 3400, 16, 1, 1, 0, 1, {"sweep_kernel": 1}),
]


class StubHalo:
    """The three calls DeviceEngine.__init__ makes on a halo."""

    def __init__(self, sharers):
        self.sharers = sharers

    def agree_max(self, eng, value):
        return value

    def device_sharers(self, eng):
        return self.sharers

    def agree(self, eng, flag):
        return flag


def build_engine(n, r, T_local, T_total, t_begin, sharers, options, dev):
    from ame_amd import TemporalAMEModel
    from ame_amd.engine import DeviceEngine, Shard
    m = TemporalAMEModel(n, T_total, r, seed=1)
    m.Y = torch.zeros(n, n, T_total, 2, device=dev)
    x = torch.zeros(n, T_total, m.d, device=dev)
    c = torch.zeros(n, T_total, m.d, m.d, device=dev)
    shard = halo = None
    if sharers > 1 or T_local != T_total:
        shard = Shard(t_begin, T_local, T_total, rank=t_begin // T_local, world=T_total // T_local)
        halo = StubHalo(sharers)
    return DeviceEngine(m, "good", 0.01, x, c, device=dev, shard=shard, halo=halo, options=options)


def engine_plan(eng):
    split = None
    if eng.elbo_stream is not None:
        split = [int(eng.options.elbo_cus),
                 int(torch.cuda.get_device_properties(eng.dev).multi_processor_count)]
    launches = int(eng.coresident_launches)
    return {"max_slices": int(eng.max_slices), "groups": [list(g) for g in eng.groups],
            "group_kinds": {str(k): int(v) for k, v in sorted(eng.group_kinds.items())},
            "sweep_kind": int(eng.sweep_kind), "resident_slots": int(eng.resident_slots),
            "pipelined": bool(eng.pipelined), "coresident_launches": launches,
            "spec_depth": int(eng.spec_depth), "work_doubles": eng.sweep_work.numel() // launches,
            "cu_split": split, "device_sharers": int(eng.device_sharers),
            "elbo_first": bool(eng.elbo_first), "speculation": bool(eng.speculation)}


def caps_log(n, r, T_local, T_total, t_begin, sharers, options, dev):
    from ame_amd import _lib
    from ame_amd.engine import EngineOptions
    from ame_amd.plan import LibCaps, SweepCaps, plan_sweeps
    real = LibCaps(n, r, t_begin, T_total, _lib.AME_GOOD, dev)
    log = []

    class Logging(SweepCaps):
        r = real.r

        @property
        def cus(self):
            log.append(["cus", [], real.cus])
            return log[-1][2]

        refuse = real.refuse

    def ask(name):
        def q(self, *args):
            log.append([name, list(args), int(getattr(real, name)(*args))])
            return log[-1][2]
        return q
    for name in ("max_slices", "kind", "orders_slices", "slice_workgroups", "work_size"):
        setattr(Logging, name, ask(name))
    plan_sweeps(Logging(), n, T_local, T_total, EngineOptions.coerce(options), sharers)
    return log


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--fixture", default=None)
    ap.add_argument("--case-timeout", type=int, default=120)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    want = None
    if args.fixture:
        with open(args.fixture) as fh:
            want = {c["name"]: c for c in json.load(fh)["cases"]}

    def expired(*_):
        raise TimeoutError("case exceeded its time limit")
    signal.signal(signal.SIGALRM, expired)
    out = []
    for name, n, r, TL, TT, t0, sharers, options in CASES:
        if want is not None and name not in want:
            continue
        signal.alarm(args.case_timeout)
        eng = build_engine(n, r, TL, TT, t0, sharers, options, dev)
        plan = engine_plan(eng)
        del eng
        gc.collect()
        torch.cuda.empty_cache()
        case = {"name": name, "n": n, "r": r, "T_local": TL, "T_total": TT, "t_begin": t0,
                "device_sharers": sharers, "options": options, "parent_plan": plan}
        if want is not None:
            case["parent_plan"] = want[name]["parent_plan"]
            if plan != case["parent_plan"]:
                raise SystemExit(f"{name}: plan {plan} differs from the fixture's "
                                 f"{case['parent_plan']}")
            case["caps_log"] = caps_log(n, r, TL, TT, t0, sharers, options, dev)
        signal.alarm(0)
        print(name, json.dumps(plan), flush=True)
        out.append(case)
        with open(args.out, "w") as fh:   # one case per line
            fh.write('{"cases": [\n' + ",\n".join(json.dumps(c) for c in out) + "\n]}\n")


if __name__ == "__main__":
    main()
