"""Sweep launch planning: which kernel each slice group gets, how many slices
co-reside, how they are grouped, whether consecutive launches pipeline, how
deep the speculation queue is, how much scratch a launch needs and how the CUs
are split for ``elbo_cus``.

:func:`plan_sweeps` is a pure function of the shape, the options and the
answers of a :class:`SweepCaps`; :class:`LibCaps` answers from the C-ABI and
the device and is the only code here that touches either, so every decision
can be driven on the CPU with a table of answers (tests/test_sweep_plan.py).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, replace
from typing import Optional

from . import _lib

# Queue-depth model.  In the pipelined steady state with period
# P (about one slice's chain of n node steps) the host reads iteration k's ELBO
# once sweep k has finished on the LAST slice of the LAST rank, i.e. after the
# wavefront's fill over all T_total slices plus one chain plus the ELBO kernels
# and the all_reduce; by then sweep k + 1 + depth must already be queued:
#     (1 + depth) P >= fill + C + delta,   fill = F (T_total - 1) steps.
# F = node steps of lag per slice: 2.94 measured in round 4 (lane start offset
# 890 us over 127 slices at 2.38 us per step, profiles/r04_v3_stamps_head.txt;
# 2.6 in round 1), rounded up to 3.0 -- a deeper queue only costs a state slot;
# delta ~ 128 steps (0.33 ms).
FILL_STEPS_PER_SLICE = 3.0
ELBO_READ_STEPS = 128
MAX_SPEC_DEPTH = 8


def derive_spec_depth(n: int, T_total: int) -> int:
    """Smallest queue depth the model above needs, at least 2 (measured best on
    one GPU), at most MAX_SPEC_DEPTH."""
    need = math.ceil((FILL_STEPS_PER_SLICE * (T_total - 1) + ELBO_READ_STEPS) / max(1, n))
    return max(2, min(MAX_SPEC_DEPTH, need))


def slice_groups(T_local: int, max_slices: int, force: int = 0):
    """Consecutive groups [(offset, size)] of the local slices that each fit on
    the chip at once (a sweep's slices spin on each other, so all slices of one
    launch must be co-resident).  The groups of one sweep run one after another
    on one stream; group g+1's first slice takes slice (g's last)'s new means
    from the hand-off granules group g left behind, so the Gauss-Seidel order
    is the same as one launch over all slices (reference: the t loop of
    structured_mf.py:240 has no limit on T)."""
    cap = max_slices if force <= 0 else min(force, max_slices)
    if cap < 1:
        raise RuntimeError("ame_amd: no sweep workgroup fits on this device")
    k = -(-T_local // cap)
    base, extra = divmod(T_local, k)
    out, off = [], 0
    for g in range(k):
        sz = base + (1 if g < extra else 0)
        out.append((off, sz))
        off += sz
    return out


class SweepCaps:
    """What the planner may ask about the sweep kernels of one problem (fixed
    n, r, t_begin, T_total, variant) on one device.  ``request`` is a request
    code and ``kind`` a concrete kind of include/ame_amd.h; a group size is a
    launch's number of slices."""
    cus: int   # compute units of the device
    r: int     # latent dim (error texts only)

    def max_slices(self, request: int) -> int:
        """Slices of this request the whole chip holds at once (< 1: none fits)."""
        raise NotImplementedError

    def kind(self, group_size: int, request: int) -> int:
        """The concrete kind a launch of group_size slices gets, or negative."""
        raise NotImplementedError

    def orders_slices(self, kind: int) -> bool:
        """Whether the kind orders itself slice by slice on the device."""
        raise NotImplementedError

    def slice_workgroups(self, kind: int) -> int:
        """Workgroups (one CU each) per slice of the kind, or negative."""
        raise NotImplementedError

    def work_size(self, group_size: int, kind: int) -> int:
        """Scratch doubles of one launch, or negative."""
        raise NotImplementedError

    def refuse(self, what: str):
        """Raise for a negative answer to `what` that the plan cannot do without."""
        raise RuntimeError(f"{what} failed (-1)")


class LibCaps(SweepCaps):
    """The answers of libame_amd.so and the device."""

    def __init__(self, n, r, t_begin, T_total, variant, device):
        self.L = _lib.lib()
        self.n, self.r, self.t_begin, self.T_total, self.variant = n, r, t_begin, T_total, variant
        self.device = device

    def _dims(self, group_size):
        return ctypes.byref(_lib.ame_dims(self.n, self.r, group_size, self.t_begin, self.T_total,
                                          self.variant))

    @property
    def cus(self):
        import torch
        return int(torch.cuda.get_device_properties(self.device).multi_processor_count)

    def max_slices(self, request):
        return int(self.L.ame_sweep_max_slices(self.n, self.r, request))

    def kind(self, group_size, request):
        return int(self.L.ame_sweep_kind(self._dims(group_size), request))

    def orders_slices(self, kind):
        return bool(self.L.ame_sweep_orders_slices(self.n, self.r, kind))

    def slice_workgroups(self, kind):
        return int(self.L.ame_sweep_slice_workgroups(kind))

    def work_size(self, group_size, kind):
        return int(self.L.ame_sweep_work_size(self._dims(group_size), kind))

    def refuse(self, what):   # the library's own message of its last negative answer
        _lib.check(-1, what)


@dataclass(frozen=True)
class SweepPlan:
    max_slices: int            # slices one launch may hold, after every clamp
    groups: list               # [(offset, size)] of the local slices, in order
    group_kinds: dict          # group size -> concrete kind
    sweep_kind: int            # the first group's kind
    resident_slots: int        # slice workgroups of sweep_kind the whole chip holds at once
    pipelined: bool            # consecutive launches run two at a time
    coresident_launches: int   # launches of this process that may spin at once
    spec_depth: int            # sweeps kept started ahead of the committed state
    work_doubles: int          # scratch per launch (the largest group's need)
    cu_split: Optional[tuple]  # (elbo_cus, cus) or None

    def serial(self) -> "SweepPlan":
        """This plan run one launch at a time (the ranks did not all pipeline)."""
        return replace(self, pipelined=False, coresident_launches=1, spec_depth=1)


def plan_sweeps(caps: SweepCaps, n: int, T_local: int, T_total: int, options,
                device_sharers: int = 1) -> SweepPlan:
    """The sweep launches of one engine (``options``: EngineOptions) under the
    co-residency rule
        device_sharers * coresident_launches * largest group <= resident_slots."""
    opt, req = options, options.sweep_kernel
    max_slices = caps.max_slices(req)
    if max_slices < 1:
        raise RuntimeError(f"ame_amd: no sweep kernel fits n={n}, r={caps.r} (request {req})")
    cu_split = None
    if opt.elbo_cus:
        # ELBO beside the sweep: the sweep's launch must fit the CUs left to it
        # (workgroups per slice from the library, one CU each)
        per_slice = None
        if req in (_lib.AME_SWEEP_V2_WORKERS, _lib.AME_SWEEP_V2_W6):
            per_slice = caps.slice_workgroups(req)
        cus = caps.cus
        if per_slice is None or per_slice < 1 or not 0 < int(opt.elbo_cus) < cus:
            raise ValueError("elbo_cus needs sweep_kernel 22 or 24 and 0 < elbo_cus < "
                             f"{cus} CUs (got {opt.elbo_cus}, kernel {req})")
        max_slices = min(max_slices, (cus - int(opt.elbo_cus)) // per_slice)
        if max_slices < 1:
            raise ValueError(f"elbo_cus={opt.elbo_cus} leaves no room for a slice")
        cu_split = (int(opt.elbo_cus), cus)
    if req in (_lib.AME_SWEEP_AUTO, _lib.AME_SWEEP_V2_AUTO) and (
            req == _lib.AME_SWEEP_V2_AUTO or caps.max_slices(_lib.AME_SWEEP_V3) < 1):
        # beyond v3's reach the GEMV-worker sweep (kind 22) in slice groups of
        # what co-resides beats ONE launch of the single-workgroup sweep over
        # all slices: config 5 at T = 256 on one GPU, 8 groups of 32 vs kind 21,
        # 285-302 vs 580 ms per iteration; the pipelined kind 23 in overlapping
        # groups measured the same, 274-291 ms, and loses at
        # T_local = 32, so kind 22 stays the choice.  AUTO picks kind 22
        # whenever T_local fits one launch
        w = caps.max_slices(_lib.AME_SWEEP_V2_WORKERS)
        if 1 <= w < min(T_local, max_slices) and caps.kind(w, req) == _lib.AME_SWEEP_V2_WORKERS:
            max_slices = w
    # Ranks of one time-sharded run that share this GPU share its CUs, and a
    # spinning launch of one rank can wait on a slice of another (halo, back
    # channel): all of them must be co-resident at once, so each rank
    # budgets for 1/k of the chip (co-residency rule)
    if device_sharers > 1:
        max_slices //= device_sharers
        if max_slices < 1:
            raise RuntimeError(f"ame_amd: {device_sharers} ranks share this GPU and one "
                               f"sweep slice (n={n}, r={caps.r}) does not fit 1/"
                               f"{device_sharers} of it")
    # Pipelined layout: a kernel that orders itself slice by slice on the
    # device (done flags) runs with TWO launches co-resident -- consecutive
    # sweeps, and consecutive slice groups of one sweep -- so each launch gets
    # at most half of what co-resides; the launches alternate over two
    # streams
    pipe_cap = 0
    if opt.pipeline and max_slices >= 2:
        half = max_slices // 2
        pk = caps.kind(max(1, min(T_local, half)), req)
        if pk >= 0 and caps.orders_slices(pk):
            pipe_cap = half
    cap = pipe_cap or max_slices
    while True:
        groups = slice_groups(T_local, cap, opt.slice_group)
        # the kernel of each group size is resolved ONCE here and passed with
        # every launch (ame_sweep rejects a launch whose buffers were sized for
        # another kind); groups that run one after another share the scratch,
        # pipelined launches alternate between two halves of it
        group_kinds = {}
        work_doubles = 1
        for size in sorted({sz for _, sz in groups}):
            k = caps.kind(size, req)
            if k < 0:
                caps.refuse("ame_sweep_kind")
            w = caps.work_size(size, k)
            if w < 0:
                caps.refuse("ame_sweep_work_size")
            group_kinds[size] = k
            work_doubles = max(work_doubles, w)
        sweep_kind = group_kinds[groups[0][1]]
        # slice workgroups of this kind the whole chip holds at once
        resident_slots = caps.max_slices(sweep_kind)
        largest = max(sz for _, sz in groups)
        if device_sharers * largest <= resident_slots:
            break
        # The request's budget counted slices of another kind than the launch
        # resolved to: AUTO beyond v3 budgets for the single-workgroup sweep and
        # takes kind 22 (8 workgroups per slice) when the launch fits the chip,
        # which it need not share evenly with the other ranks on this GPU.
        # Regroup within this kind's share
        cap = max_slices = resident_slots // device_sharers
        if cap < 1:
            raise RuntimeError(f"ame_amd: {device_sharers} ranks share this GPU and a launch of "
                               f"kind {sweep_kind} (n={n}, r={caps.r}) does not fit 1/"
                               f"{device_sharers} of it")
    pipelined = (len(set(group_kinds.values())) == 1 and pipe_cap > 0
                 and caps.orders_slices(sweep_kind)
                 and 2 * largest * device_sharers <= resident_slots
                 and bool(opt.pipeline))
    # How many sweeps may run ahead of the committed state.  Pipelined sweeps
    # overlap slice by slice, so a deeper queue keeps the wavefront full when
    # its fill over all T slices (all ranks) exceeds one iteration: the host
    # reads iteration k's ELBO only after sweep k has finished everywhere, and
    # sweep k+depth must already be queued by then.
    if opt.spec_depth is None:
        spec_depth = derive_spec_depth(n, T_total) if pipelined else 1
    else:
        spec_depth = int(opt.spec_depth)
    if spec_depth < 1:
        raise ValueError("spec_depth must be >= 1")
    if not pipelined:
        # A sweep that does not order itself slice by slice on the device must
        # not start before the sweep that writes its input slot has finished;
        # with more than one queued that is a serial chain anyway, so the
        # queue is one deep (_launch_sweep also orders after the last one).
        spec_depth = 1
    return SweepPlan(max_slices=max_slices, groups=groups, group_kinds=group_kinds,
                     sweep_kind=sweep_kind, resident_slots=resident_slots, pipelined=pipelined,
                     coresident_launches=2 if pipelined else 1, spec_depth=spec_depth,
                     work_doubles=work_doubles, cu_split=cu_split)
