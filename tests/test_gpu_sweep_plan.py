"""plan_sweeps answered by the live library and device (LibCaps) makes, for every
case of tests/golden/sweep_plans.json, the plan the engine made before the
planner was split out of DeviceEngine.__init__.  Nothing is allocated: the
planner only asks the C-ABI's size and kind queries."""
import pytest

from test_sweep_plan import CASES, plan_dict

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_live_plan_is_the_parent_plan(case, gpu_device):
    import torch
    from ame_amd import _lib
    from ame_amd.engine import EngineOptions
    from ame_amd.plan import LibCaps, plan_sweeps
    caps = LibCaps(case["n"], case["r"], case["t_begin"], case["T_total"], _lib.AME_GOOD, gpu_device)
    before = torch.cuda.memory_allocated(gpu_device)
    plan = plan_sweeps(caps, case["n"], case["T_local"], case["T_total"],
                       EngineOptions.coerce(case["options"]), case["device_sharers"])
    assert torch.cuda.memory_allocated(gpu_device) == before
    got = plan_dict(plan)
    for field, want in got.items():
        assert want == case["parent_plan"][field], (field, want, case["parent_plan"][field])
