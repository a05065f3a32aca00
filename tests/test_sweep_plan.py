"""The sweep launch planner (ame_amd/plan.py) on the CPU.

* Replay: for every case of tests/golden/sweep_plans.json (recorded on an
  MI355X by tools/record_sweep_plans.py) plan_sweeps, answered from the case's
  ``caps_log`` alone, makes the plan the engine made before the planner was
  split out of DeviceEngine.__init__ (``parent_plan``).  A question the log
  does not hold fails the test.
* Policy: a hand-written capability table.  Its numbers are test inputs, not
  measurements: 256 CUs, v3 one slice per CU, kind 22 eight workgroups per
  slice (kind 23 five, kind 24 seven).
"""
import json
import os
import random

import pytest

from ame_amd import _lib
from ame_amd.engine import EngineOptions
from ame_amd.plan import SweepCaps, SweepPlan, plan_sweeps

AUTO, SINGLE, V2_AUTO, V3 = (_lib.AME_SWEEP_AUTO, _lib.AME_SWEEP_V2_SINGLE, _lib.AME_SWEEP_V2_AUTO,
                             _lib.AME_SWEEP_V3)
LDS, HBM, W, PIPE, W6 = (_lib.AME_SWEEP_V2_LDS, _lib.AME_SWEEP_V2_HBM, _lib.AME_SWEEP_V2_WORKERS,
                         _lib.AME_SWEEP_V2_PIPE, _lib.AME_SWEEP_V2_W6)

with open(os.path.join(os.path.dirname(__file__), "golden", "sweep_plans.json")) as _fh:
    CASES = json.load(_fh)["cases"]


def plan_dict(plan):
    """A SweepPlan in the fixture's JSON form."""
    return {"max_slices": plan.max_slices, "groups": [list(g) for g in plan.groups],
            "group_kinds": {str(k): v for k, v in plan.group_kinds.items()},
            "sweep_kind": plan.sweep_kind, "resident_slots": plan.resident_slots,
            "pipelined": plan.pipelined, "coresident_launches": plan.coresident_launches,
            "spec_depth": plan.spec_depth, "work_doubles": plan.work_doubles,
            "cu_split": None if plan.cu_split is None else list(plan.cu_split)}


class ReplayCaps(SweepCaps):
    """Answers from a recorded caps_log; anything else fails the test."""

    def __init__(self, r, log):
        self.r = r
        self.answers = {(name, tuple(args)): ans for name, args, ans in log}

    def _answer(self, name, *args):
        if (name, args) not in self.answers:
            pytest.fail(f"plan_sweeps asked {name}{args}, which the recorded run did not")
        return self.answers[(name, args)]

    cus = property(lambda self: self._answer("cus"))

    def max_slices(self, request):
        return self._answer("max_slices", request)

    def kind(self, group_size, request):
        return self._answer("kind", group_size, request)

    def orders_slices(self, kind):
        return bool(self._answer("orders_slices", kind))

    def slice_workgroups(self, kind):
        return self._answer("slice_workgroups", kind)

    def work_size(self, group_size, kind):
        return self._answer("work_size", group_size, kind)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_replay_makes_the_parent_plan(case):
    plan = plan_sweeps(ReplayCaps(case["r"], case["caps_log"]), case["n"], case["T_local"],
                       case["T_total"], EngineOptions.coerce(case["options"]),
                       case["device_sharers"])
    got = plan_dict(plan)
    for field, want in case["parent_plan"].items():
        if field in got:   # the rest (device_sharers, elbo_first, speculation) is the engine's
            assert got[field] == want, (field, got[field], want)
    assert set(got) <= set(case["parent_plan"])


def test_fixture_holds_the_issue_cases():
    names = {c["name"] for c in CASES}
    assert len(CASES) == 17 and len(names) == 17
    for c in CASES:
        assert c["caps_log"], c["name"]


# ---------------------------------------------------------------------------
# policy, on a hand-written table
# ---------------------------------------------------------------------------
class TableCaps(SweepCaps):
    """kinds: {kind: (slots, workgroups per slice, orders slices, scratch
    doubles per slice)}; slots = slices of the kind the whole chip holds.  A
    worker kind (22, 23, 24) runs a launch of up to `slots` slices.  Requests
    resolve as include/ame_amd.h says: AUTO takes v3, else the workers when
    the launch fits, else the single-workgroup kinds (LDS before HBM)."""
    DEFAULT = {V3: (256, 1, True, 0), LDS: (512, 1, False, 0), HBM: (256, 1, False, 100),
               W: (32, 8, False, 1000), PIPE: (51, 5, True, 900), W6: (36, 7, False, 950)}

    def __init__(self, kinds=None, cus=256, r=16):
        self.kinds = dict(self.DEFAULT if kinds is None else kinds)
        self.cus, self.r = cus, r
        self.asked = []

    def _single(self):
        return LDS if LDS in self.kinds else HBM if HBM in self.kinds else None

    def max_slices(self, request):
        self.asked.append(("max_slices", request))
        if request == AUTO and V3 in self.kinds:
            request = V3
        elif request in (AUTO, V2_AUTO, SINGLE):
            request = self._single()
        return self.kinds[request][0] if request in self.kinds else 0

    def kind(self, group_size, request):
        self.asked.append(("kind", group_size, request))
        if request == AUTO and V3 in self.kinds:
            return V3
        if request in (AUTO, V2_AUTO) and W in self.kinds and group_size <= self.kinds[W][0]:
            return W
        if request in (AUTO, V2_AUTO, SINGLE):
            return -1 if self._single() is None else self._single()
        if request not in self.kinds:
            return -1
        if request in (W, PIPE, W6) and group_size > self.kinds[request][0]:
            return -1
        return request

    def orders_slices(self, kind):
        return self.kinds[kind][2]

    def slice_workgroups(self, kind):
        return self.kinds[kind][1] if kind in self.kinds else -1

    def work_size(self, group_size, kind):
        return group_size * self.kinds[kind][3]


def _plan(caps=None, n=1024, T_local=128, T_total=None, sharers=1, **options):
    return plan_sweeps(caps or TableCaps(), n, T_local, T_total or T_local,
                       EngineOptions.coerce(options), sharers)


def _random_table(rng):
    cus = rng.choice((64, 128, 256, 304))
    kinds = {}
    if rng.random() < 0.7:
        kinds[V3] = (cus * rng.choice((1, 1, 2)), 1, True, rng.choice((0, 0, 7)))
    if rng.random() < 0.7:
        kinds[LDS] = (cus * rng.choice((1, 2)), 1, False, 0)
    if LDS not in kinds or rng.random() < 0.7:
        kinds[HBM] = (cus * rng.choice((1, 2)), 1, False, rng.randrange(1, 200))
    for kind, wgs, orders in ((W, 8, False), (PIPE, 5, True), (W6, 7, False)):
        kinds[kind] = (cus * rng.choice((1, 2)) // wgs, wgs, orders, rng.randrange(1, 2000))
    return TableCaps(kinds, cus=cus, r=rng.choice((4, 16, 32)))


def test_random_tables_obey_the_coresidency_rule():
    rng = random.Random(20240611)
    drawn, skipped = 600, 0
    for _ in range(drawn):
        caps = _random_table(rng)
        T_local = rng.choice((1, 2, 7, 20, 31, 32, 33, 40, 128, 129, 256, 512, 600))
        world = rng.choice((1, 1, 2, 4))
        sharers = rng.choice((1, 1, 1, 2, 4)) if world > 1 else 1
        req = rng.choice((AUTO, AUTO, AUTO, SINGLE, V2_AUTO, V3, LDS, HBM, W, PIPE, W6))
        opts = {"sweep_kernel": req, "pipeline": rng.random() < 0.8,
                "slice_group": rng.choice((0, 0, 3, 128)), "spec_depth": rng.choice((None, None, 1, 3))}
        try:
            plan = _plan(caps, n=rng.choice((90, 1024, 4096)), T_local=T_local,
                         T_total=T_local * world, sharers=sharers, **opts)
        except (RuntimeError, ValueError):
            skipped += 1
            continue
        ctx = (caps.kinds, caps.cus, T_local, world, sharers, opts, plan)
        sizes = [sz for _, sz in plan.groups]
        assert sharers * plan.coresident_launches * max(sizes) <= plan.resident_slots, ctx
        assert plan.groups[0][0] == 0 and sum(sizes) == T_local and min(sizes) >= 1, ctx
        assert all(b[0] == a[0] + a[1] for a, b in zip(plan.groups, plan.groups[1:])), ctx
        assert set(plan.group_kinds) == set(sizes), ctx
        assert plan.sweep_kind == plan.group_kinds[sizes[0]], ctx
        assert plan.work_doubles == max(1, caps.work_size(max(sizes), plan.group_kinds[max(sizes)])), ctx
        assert plan.coresident_launches == (2 if plan.pipelined else 1), ctx
        assert plan.spec_depth >= 1 and (plan.pipelined or plan.spec_depth == 1), ctx
    assert skipped <= drawn // 10, (skipped, drawn)


def test_round6_clamp():
    """2 ranks on one GPU, forced group 128, 256 one-per-CU slots, pipelined:
    2 ranks x 2 launches x 128 would ask for 512 of 256 CUs."""
    plan = _plan(T_local=256, T_total=512, sharers=2, slice_group=128)
    assert plan.pipelined and plan.resident_slots == 256
    assert max(sz for _, sz in plan.groups) <= 64
    assert plan.groups == [(0, 64), (64, 64), (128, 64), (192, 64)]


def test_auto_workers_on_a_shared_gpu():
    """Beyond v3 AUTO budgets for the single-workgroup sweep (256 slices) and
    takes kind 22 when the launch fits the whole chip (32 slices): two ranks of
    20 slices each get their half of kind 22's slots, not 40 of 32."""
    caps = TableCaps({k: v for k, v in TableCaps.DEFAULT.items() if k != V3})
    plan = _plan(caps, n=4096, T_local=20, T_total=40, sharers=2)
    assert plan.sweep_kind == W and plan.resident_slots == 32 and not plan.pipelined
    assert plan.groups == [(0, 10), (10, 10)] and plan.max_slices == 16
    alone = _plan(caps, n=4096, T_local=20, T_total=40, sharers=1)
    assert alone.groups == [(0, 20)] and alone.sweep_kind == W


def test_spec_depth():
    assert _plan(n=90, T_local=40, pipeline=False, spec_depth=2).spec_depth == 1
    assert _plan(n=90, T_local=40, spec_depth=3).spec_depth == 3
    with pytest.raises(ValueError, match="spec_depth must be >= 1"):
        _plan(spec_depth=0)
    with pytest.raises(ValueError, match="spec_depth must be >= 1"):
        _plan(pipeline=False, spec_depth=0)   # before the non-pipelined clamp to 1


def test_elbo_cus():
    for bad in (AUTO, V3, PIPE, HBM):
        with pytest.raises(ValueError, match=r"elbo_cus needs sweep_kernel 22 or 24 and 0 < elbo_cus < "
                                             rf"256 CUs \(got 32, kernel {bad}\)"):
            _plan(T_local=32, sweep_kernel=bad, elbo_cus=32)
    for bad in (256, 300, -1):
        with pytest.raises(ValueError, match=rf"elbo_cus needs sweep_kernel 22 or 24 .*got {bad}, kernel 24"):
            _plan(T_local=32, sweep_kernel=W6, elbo_cus=bad)
    plan = _plan(T_local=32, T_total=256, n=4096, sweep_kernel=W6, elbo_cus=32)
    assert plan.max_slices == 32 == (256 - 32) // 7 and plan.cu_split == (32, 256)
    assert not plan.pipelined and plan.resident_slots == 36
    assert _plan(T_local=32, sweep_kernel=W6).max_slices == 36
    with pytest.raises(ValueError, match="elbo_cus=250 leaves no room for a slice"):
        _plan(T_local=32, sweep_kernel=W6, elbo_cus=250)


def test_sharers_leaving_no_slice():
    kinds = dict(TableCaps.DEFAULT)
    kinds[HBM] = (3, 1, False, 100)
    with pytest.raises(RuntimeError, match=r"ame_amd: 4 ranks share this GPU and one sweep slice "
                                           r"\(n=1024, r=16\) does not fit 1/4 of it"):
        _plan(TableCaps(kinds), T_local=8, T_total=32, sharers=4, sweep_kernel=HBM)
    del kinds[V3]
    with pytest.raises(RuntimeError, match=r"no sweep kernel fits n=1024, r=16 \(request 3\)"):
        _plan(TableCaps(kinds), sweep_kernel=V3)


def test_serial():
    plan = _plan(T_local=512)
    assert plan.pipelined and plan.coresident_launches == 2 and plan.spec_depth == 2
    s = plan.serial()
    assert isinstance(s, SweepPlan)
    assert (s.pipelined, s.coresident_launches, s.spec_depth) == (False, 1, 1)
    assert (s.groups, s.group_kinds, s.max_slices, s.work_doubles) == (
        plan.groups, plan.group_kinds, plan.max_slices, plan.work_doubles)
    with pytest.raises(Exception):
        s.spec_depth = 2   # frozen


@pytest.mark.parametrize("req", [AUTO, V2_AUTO])
def test_auto_worker_group_override(req):
    """max_slices becomes kind 22's w exactly when 1 <= w < min(T_local,
    max_slices) and a launch of w slices resolves to kind 22."""
    base = {k: v for k, v in TableCaps.DEFAULT.items() if k != V3 or req == V2_AUTO}
    for w in (0, 1, 31, 32, 33, 255, 256, 300):
        for T_local in (1, 32, 33, 256, 257, 600):
            kinds = dict(base)
            kinds[W] = (w, 8, False, 1000)
            caps = TableCaps(kinds)
            plan = _plan(caps, n=4096, T_local=T_local, sweep_kernel=req)
            single = kinds[LDS][0]                      # what the request's max_slices answers
            trigger = 1 <= w < min(T_local, single)     # the probe at w resolves to 22 (it fits w)
            assert plan.max_slices == (w if trigger else single), (w, T_local, plan)
    # the probe decides: same window, but a launch of w slices does not get kind 22
    class NoWorkers(TableCaps):
        def kind(self, group_size, request):
            k = super().kind(group_size, request)
            return self._single() if k == W else k
    plan = _plan(NoWorkers(base), n=4096, T_local=256, sweep_kernel=req)
    assert plan.max_slices == base[LDS][0] and plan.sweep_kind == LDS
    # AUTO with v3 in reach never asks about the workers
    if req == AUTO:
        caps = TableCaps()
        assert _plan(caps, T_local=600).sweep_kind == V3
        assert ("max_slices", W) not in caps.asked
