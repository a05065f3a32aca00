"""Device engine: HBM-resident VI state + the per-iteration kernel sequence.

One engine per process / GPU.  It owns, for the local time slices
[t_begin, t_begin + T_local):

    Yt        [T_local][n][ny][2] fp32  observed network, time-major, rows padded to
                                        even length (ame_pack_y)
    xs[k]     [T_local][n][d]    fp32   means: ring of spec_depth + 1 states
    covs[k]   [T_local][n][d][d] fp32   covariances: same ring (x_a / cov = current)
    hand      [T_local][n][d]    u64    lane-to-lane {epoch,value} granules
    cov_terms [T_local][n][4]    fp64   per-(node,time) covariance ELBO terms

and runs, per fit() iteration (reference base.py:170-181):

    ame_sweep   (means + covariances)       structured_mf.py:211-326
    ame_cov     (covariance ELBO terms)     structured_mf.py:142-144, 166, 193, 202-209
    ame_elbo    (pair + node sums)          structured_mf.py:115-200, temporal_ame.py:255-291

The host then assembles ELBO and MSE from 8 fp64 sums (+ the analytic
constants) exactly as the reference's formulas define them.

A sweep reads the current state and writes the spare buffers, which become
current when the sweep is committed.  While fit() has another iteration to
go, the next sweep does not depend on this iteration's ELBO, so it is started
on a high-priority stream of its own before this iteration's ELBO kernels,
which then run beside it on the main stream (they read only the current
state); the next update_step merely commits it.  When fit() stops instead
(convergence or max_iter) the started sweep is dropped: it never touched the
current state.  On one GPU, when both sweeps' workgroups fit on the chip,
the next sweep is queued while the previous one still runs (pipelined): each
of its slices waits on the device for the previous sweep to finish slices t
and t+1, so consecutive sweeps overlap and the wavefront fill is paid once per
fit() instead of once per iteration.  Results are bit-identical to running
the kernels in order (tests/test_gpu_parity.py::test_speculative_sweep_is_exact).

On a binary model (model.set_binary) the engine owns Bt (the packed ties), a
working network Yt beside Yt_raw and stat, and runs ame_probit_fill where the
masked path runs ame_fill_missing (with a mask: in its place).
With hidden dyads (model.set_missing) the engine also owns Yt_raw (the packed
observations; Yt is then a separate working network), Mt / pairs / deg (the
packed mask, ame_pack_mask) and corr, and runs ame_fill_missing on the main
stream after every committed sweep, before that state's ELBO; sweeps then run
in order, none started ahead.
"""
from __future__ import annotations

import collections
import ctypes
import math
import time
from dataclasses import dataclass, fields, replace
from typing import Optional

import torch

from . import _lib
from .plan import (ELBO_READ_STEPS, FILL_STEPS_PER_SLICE, MAX_SPEC_DEPTH,  # noqa: F401 (re-exported)
                   LibCaps, derive_spec_depth, plan_sweeps, slice_groups)

LOG2PI = math.log(2.0 * math.pi)
VARIANTS = {"good": _lib.AME_GOOD, "bad": _lib.AME_BAD, "naive": _lib.AME_NAIVE}


@dataclass
class Shard:
    """Contiguous block of time slices held by this rank."""
    t_begin: int
    T_local: int
    T_total: int
    rank: int = 0
    world: int = 1


# CU-masked streams (EngineOptions.elbo_cus), per (device, first CU, CUs, slot)
_CU_STREAMS = {}


@dataclass
class EngineOptions:
    """Execution choices of one engine.  Nothing is read from the environment:
    the defaults are the production path, tests and A/B runs pass these
    explicitly (``engine_options=`` of the VI classes).

    sweep_kernel  request code of include/ame_amd.h (``_lib.AME_SWEEP_*``):
                  AUTO picks v3 when the shape fits it, else v2 (with GEMV
                  workers when they are co-resident)
    pipeline      queue the next sweep while this one runs (kernels that order
                  themselves slice by slice on the device)
    speculate     start the next sweep before this iteration's ELBO is read
    spec_depth    sweeps kept started ahead of the committed state when
                  pipelined; None derives it from the global slice count
                  (:func:`derive_spec_depth`)
    slice_group   at most this many local slices per launch (0: as many as fit)
    pairs_kernel  ELBO pair kernel (``_lib.AME_PAIRS_*``; 0 = default)
    elbo_cus      > 0: run the ELBO kernels on their own CU-masked stream over
                  compute units [0, elbo_cus) and the sweep streams over the
                  rest (ame_stream_create_cu_range), so iteration k's ELBO runs
                  beside sweep k+1 instead of queueing behind its workgroups.
                  Needs a non-pipelined GEMV-worker kind (sweep_kernel 22 or 24)
                  whose launch fits the remaining CUs (kind 24 at config 5's
                  rank shape: 32 slices x 7 workgroups = 224 CUs, elbo_cus 32)
    elbo_first    queue this iteration's ELBO kernels before the speculative
                  next sweep and order that sweep after them (default: after
                  it).  Same results; measured at config 5's rank shape (kind
                  22) no faster: 32.8-35.5 vs 33.0-34.0 ms per iteration
                  (profiles/r05_c5_elbo_first_ab.txt), so off
    """
    sweep_kernel: int = 0
    pipeline: bool = True
    speculate: bool = True
    spec_depth: Optional[int] = None
    slice_group: int = 0
    pairs_kernel: int = 0
    elbo_cus: int = 0
    elbo_first: bool = False

    @classmethod
    def coerce(cls, opts) -> "EngineOptions":
        if opts is None:
            return cls()
        if isinstance(opts, cls):
            return opts
        names = {f.name for f in fields(cls)}
        bad = set(opts) - names
        if bad:
            raise ValueError(f"unknown engine option(s) {sorted(bad)}; known: {sorted(names)}")
        return cls(**opts)


# Sweep epochs are unique within the process: every engine starts above the
# highest epoch any earlier engine launched.  A buffer the caching allocator
# recycles from an older engine (done flags, hand-off granules) then only
# holds epochs BELOW every epoch this engine waits for, so a stale word makes
# a waiter wait instead of passing; the device additionally flags any word
# ABOVE the epoch window (AME_STATUS_STALE_EPOCH, include/ame_amd.h).
_EPOCH_HIGH = 0


def _epoch_base() -> int:
    return _EPOCH_HIGH


def _note_epoch(e: int) -> None:
    global _EPOCH_HIGH
    _EPOCH_HIGH = max(_EPOCH_HIGH, int(e))


_STATUS_TEXT = (
    (_lib.AME_STATUS_SPIN_TIMEOUT, "a hand-off between slices timed out (workgroups not co-resident?)"),
    (_lib.AME_STATUS_HALO_TIMEOUT, "a hand-off from a neighbouring rank timed out"),
    (_lib.AME_STATUS_LDS_TIMEOUT, "an intra-workgroup hand-off timed out (internal error)"),
    (_lib.AME_STATUS_STALE_EPOCH, "a hand-off word carried an epoch outside the protocol's "
                                  "window (stale buffer or an unordered write): results of "
                                  "this sweep are not trusted"),
)


def status_text(st: int) -> str:
    parts = [txt for bit, txt in _STATUS_TEXT if st & bit]
    return "; ".join(parts) if parts else "unknown"


def status_report(words) -> str:
    """Text of a status block (include/ame_amd.h, AME_STATUS_WORDS uint32):
    the bits, then the record of the FIRST failing wait (site, slice, node,
    word seen vs expected, time waited, sweep epoch) and how many later waits
    gave up quietly because of it."""
    w = [int(x) & 0xFFFFFFFF for x in words]
    w += [0] * (_lib.AME_STATUS_WORDS - len(w))
    msg = f"device status {w[0]:#x}: {status_text(w[0])}"
    if w[1]:
        node = "prologue" if w[4] == 0xFFFFFFFF else f"node {w[4]}"
        site = _lib.AME_WAIT_SITES.get(w[2], f"site {w[2]}")
        msg += (f"; first failure: {site}, slice {w[3]}, {node}, saw {w[5]} expected {w[6]}, "
                f"after {w[7] / 1e3:.1f} ms, sweep epoch {w[8]}")
    if w[10]:
        msg += f"; {w[10]} later wait(s) gave up quietly"
    return msg


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _blockdiag(Sigma, Psi):
    d = 2 + Psi.shape[0]
    S = torch.zeros(d, d, dtype=torch.float64)
    S[:2, :2] = Sigma.double()
    S[2:, 2:] = Psi.double()
    return S


def _sym(a):
    return 0.5 * (a + a.T)


class Constants:
    """fp64 model constants, built from the fp32 model attributes the reference reads."""

    def __init__(self, model):
        d = model.d
        self.R = model.R.detach().double().cpu()
        self.R_inv = model.R_inv.detach().double().cpu()
        S0 = _blockdiag(model.Sigma.detach().cpu(), model.Psi.detach().cpu())
        Q = model.Q.detach().double().cpu()
        Phi = model.Phi.detach().double().cpu()
        self.S0inv = _sym(torch.linalg.inv(S0))
        self.Qinv = _sym(torch.linalg.inv(Q))
        self.PtQiP = _sym(Phi.T @ self.Qinv @ Phi)
        self.QiPhi = self.Qinv @ Phi
        self.PhiTQi = Phi.T @ self.Qinv
        self.Phi = Phi
        self.Q = Q
        self.logdetR = float(torch.logdet(self.R))
        self.trRinv = float(torch.trace(self.R_inv))
        self.logdetS0 = float(torch.logdet(S0))
        self.logdetQ = float(torch.logdet(Q))
        self.stack = torch.stack([self.S0inv, self.Qinv, self.PtQiP, self.QiPhi,
                                  self.PhiTQi]).contiguous()
        self.d = d

    def rinv4(self):
        r = self.R_inv.flatten().tolist()
        return (ctypes.c_double * 4)(*r)


def assemble(out, n, T, d, variant, C: Constants, hidden=None, pairs_obs=None, deg_trace=None, binary=None):
    """ELBO pieces and MSE from the 8 device sums (see include/ame_amd.h).

    Formulas: structured_mf.py:124-209 / naive_mf.py:114-191 and
    temporal_ame.py:290 with the pairwise correction collapsed as
    sum_{i<j}(tr_i + tr_j) = (n-1) sum_i tr_i.

    With hidden dyads (all three optional arguments): ``hidden`` = the two
    correction sums of ame_fill_missing added over the slices, which out[0] and
    out[7] accumulated at the hidden entries of the working network and are
    taken off again; ``pairs_obs`` = observed pairs; ``deg_trace`` = sum_{i,t}
    deg[t][i] tr(S_it), each node's trace counted once per observed partner
    ((n - 1) out[1] when nothing is hidden).  The formulas are then the
    reference's over observed pairs.

    On a binary model (``binary`` = (sum_t stat[t][1], sum_t stat[t][2]) of
    ame_probit_fill, with ``pairs_obs`` and ``deg_trace``; ``hidden`` unused):
    loglik = the probit bound of the observed pairs minus half the same
    heuristic variance term, recon = the mean squared error of Phi(E[mu])
    against the ties; none of ame_elbo's pair sums (out[0], out[7]) is read.
    """
    if pairs_obs is None:
        npairs = T * n * (n - 1) / 2.0
        corr = 0.0 if variant == "naive" else 0.1 * C.trRinv / d * (n - 1) * out[1]
        quad, sq = out[0], out[7]
    else:
        npairs = float(pairs_obs)
        corr = 0.0 if variant == "naive" else 0.1 * C.trRinv / d * deg_trace
        quad, sq = (0.0, binary[1]) if binary is not None else (out[0] - hidden[0], out[7] - hidden[1])
    if binary is not None:
        loglik = binary[0] - 0.5 * corr
    else:
        loglik = -0.5 * (npairs * (C.logdetR + 2 * LOG2PI) + quad + corr)
    prior0 = -0.5 * (n * (C.logdetS0 + d * LOG2PI) + out[2] + out[3])
    trans = -0.5 * (n * (T - 1) * (C.logdetQ + d * LOG2PI) + out[4] + out[5])
    ent = 0.5 * (n * T * d * (1 + LOG2PI) + out[6])
    recon = sq / (n * (n - 1) * T) if pairs_obs is None else sq / (2.0 * npairs)
    return {"loglik": loglik, "prior0": prior0, "trans": trans, "entropy": ent,
            "elbo": loglik + prior0 + trans + ent, "recon": recon}


class _ElboCall:
    """The with-block of DeviceEngine._elbo_call: the CU-masked ELBO stream is
    ordered after everything queued on the main one, and later main-stream
    work (reading out) after it.  A class, not a generator: this runs twice per
    fit() iteration on the host's critical path.  A launch that raises leaves
    the block without the closing event, as the caller's exception is the news."""
    __slots__ = ("eng", "name", "st", "tok")

    def __init__(self, eng, name):
        self.eng, self.name = eng, name

    def __enter__(self):
        eng = self.eng
        st = self.st = eng._elbo_stream()
        if st is not eng.stream:
            ev = torch.cuda.Event()
            ev.record(eng.stream)
            st.wait_event(ev)
        self.tok = eng._tic(self.name, st) if eng.timing else None
        return ctypes.c_void_p(st.cuda_stream)

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            eng = self.eng
            if self.tok is not None:
                eng._toc(self.tok)
            if self.st is not eng.stream:
                ev = torch.cuda.Event()
                ev.record(self.st)
                eng.stream.wait_event(ev)
        return False


def _plan_field(name):
    return property(lambda self: getattr(self.plan, name), doc=f"SweepPlan.{name} of this engine")


class DeviceEngine:
    """HBM-resident state of one VI run on one GPU (one time shard)."""

    max_slices = _plan_field("max_slices")
    groups = _plan_field("groups")
    group_kinds = _plan_field("group_kinds")
    sweep_kind = _plan_field("sweep_kind")
    resident_slots = _plan_field("resident_slots")
    pipelined = _plan_field("pipelined")
    coresident_launches = _plan_field("coresident_launches")
    spec_depth = _plan_field("spec_depth")

    def __init__(self, model, variant: str, lr: float, X_mean: torch.Tensor,
                 X_cov: torch.Tensor, device=None, shard: Optional[Shard] = None,
                 halo=None, options: Optional[EngineOptions] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("ame_amd: no GPU visible; the HIP path has no CPU fallback")
        self.L = _lib.lib()
        if variant not in VARIANTS:
            raise ValueError(f"Unknown factorization '{variant}'")
        self.variant = variant
        self.vcode = VARIANTS[variant]
        self.n, self.T, self.d, self.r = int(model.n), int(model.T), int(model.d), int(model.r)
        if self.r not in _lib.supported_r():
            raise RuntimeError(f"ame_amd: latent_dim={self.r} not compiled "
                               f"(supported {_lib.supported_r()})")
        self.dev = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        self.shard = shard or Shard(0, self.T, self.T)
        self.halo = halo
        if getattr(model, "W", None) is not None and (
                halo is not None or self.shard.T_local != self.shard.T_total):
            raise NotImplementedError("dyadic covariates are not available on a time-sharded run")
        self.options = opt = EngineOptions.coerce(options)
        # hidden dyads (model.set_missing): the working network is refilled from
        # the new means after every sweep, so sweeps run in order, none started
        # ahead
        self.masked = getattr(model, "missing", None) is not None
        if self.masked:
            if halo is not None or self.shard.T_local != self.shard.T_total:
                raise NotImplementedError("missing dyads are not available on a time-sharded run")
            if getattr(model, "W", None) is not None:
                raise NotImplementedError("missing dyads together with dyadic covariates are not "
                                          "available (ame_covar_stats does not select pairs)")
            self.options = opt = replace(opt, pipeline=False, speculate=False)
        # binary network (model.set_binary): the working network is rewritten from
        # the new means after every sweep, as in the masked path
        self.binary = getattr(model, "binary", None) is not None
        if self.binary:
            if halo is not None or self.shard.T_local != self.shard.T_total:
                raise NotImplementedError("binary networks are not available on a time-sharded run")
            if getattr(model, "W", None) is not None:
                raise NotImplementedError("binary networks together with dyadic covariates are not "
                                          "available (the residual of a 0 / 1 network has no meaning)")
            self.options = opt = replace(opt, pipeline=False, speculate=False)
        self.refill = self.masked or self.binary   # the working network follows the means
        self.lr = float(lr)
        self.C = Constants(model)
        sh = self.shard
        self.dims = _lib.ame_dims(self.n, self.r, sh.T_local, sh.t_begin, sh.T_total, self.vcode)
        dev = self.dev
        with torch.cuda.device(dev):
            self.stream = torch.cuda.current_stream(dev)
            self.consts = self.C.stack.to(dev)
            self.phi = self.C.Phi.contiguous().to(dev)
            self._pack_y(model.Y)
            t0, t1 = sh.t_begin, sh.t_begin + sh.T_local
            x0 = X_mean[:, t0:t1].detach().float().permute(1, 0, 2).contiguous().to(dev)
            c0 = X_cov[:, t0:t1].detach().float().permute(1, 0, 2, 3).contiguous().to(dev)
            self.xs, self.covs = [x0], [c0]
            self._cur = 0
            n, d, TL = self.n, self.d, sh.T_local
            self.hand = torch.zeros(TL * n * d, dtype=torch.int64, device=dev)
            self.cov_terms = torch.zeros(TL * n * 4, dtype=torch.float64, device=dev)
            ws = int(self.L.ame_elbo_work_size(ctypes.byref(self.dims)))
            if ws < 0:
                _lib.check(-1, "ame_elbo_work_size")
            self.work = torch.empty(ws, dtype=torch.float64, device=dev)
            self.out = torch.zeros(8, dtype=torch.float64, device=dev)
            self.status = torch.zeros(_lib.AME_STATUS_WORDS, dtype=torch.int32, device=dev)
        self.last_status = None   # the status block of the last failure _check_status raised
        self.epoch = _epoch_base()
        if self.halo is not None:   # every rank's sweep k carries the same epoch
            self.epoch = self.halo.agree_max(self, self.epoch)
        # the sweep launches (ame_amd/plan.py); ranks that share this GPU share
        # its CUs, and every rank must take the same path
        caps = LibCaps(self.n, self.r, sh.t_begin, sh.T_total, self.vcode, dev)
        self.device_sharers = self.halo.device_sharers(self) if self.halo is not None else 1
        self.plan = plan_sweeps(caps, self.n, sh.T_local, sh.T_total, opt, self.device_sharers)
        if self.halo is not None and not self.halo.agree(self, self.plan.pipelined):
            self.plan = self.plan.serial()
        # ELBO before the speculative sweep (EngineOptions.elbo_first)
        self.elbo_first = bool(opt.elbo_first)
        if self.halo is not None:   # the collectives of sums() keep one order on every rank
            self.elbo_first = self.halo.agree(self, self.elbo_first)
        self._out_host = None
        self._out_valid = False
        self._cov_terms_valid = False
        self._fill_valid = False
        self._hidden_host = None
        self.timing = False       # record HIP events around each kernel launch
        self.events = []          # (name, start, end) while timing
        self.speculation = bool(opt.speculate)
        self._specs = collections.deque()   # (done events, ring slot) of sweeps started ahead
        # consecutive sweeps (or, pipelined, consecutive launches) alternate
        # between two high-priority streams
        self.elbo_stream = None
        if self.plan.cu_split is None:
            self.sweep_streams = [torch.cuda.Stream(device=dev, priority=-1) for _ in range(2)]
        else:
            ec, cus = self.plan.cu_split
            self.elbo_stream = self._cu_stream(0, ec)
            self.sweep_streams = [self._cu_stream(ec, cus - ec, slot) for slot in range(2)]
        self._launch_ctr = 0
        with torch.cuda.device(dev):
            self.done = torch.zeros(max(sh.T_local, 1), dtype=torch.int32, device=dev)
            # scratch per launch; pipelined, two launches run at once: two halves
            self.sweep_work = torch.empty(self.plan.work_doubles * self.coresident_launches,
                                          dtype=torch.float64, device=dev)
            while len(self.xs) < self.spec_depth + 1:
                self.xs.append(torch.empty_like(self.xs[0]))
                self.covs.append(torch.empty_like(self.covs[0]))
        # Scratch of the calls that run beside the sweep (predict, mstep_stats,
        # smooth), grown to the largest need so far.  One buffer serves all
        # three: they run one after another on the ELBO stream, none reads what
        # it has not written in the same call (the buffer starts uninitialised),
        # and none keeps a result there -- outputs are separate tensors, also
        # those of smooth() that are fed back into mstep_stats / predict.
        self._side_work = None
        self._sim_buf = None    # one slice chunk of a simulated network (simulated_statistics)
        self._host_ready = None
        # test hook only (tests/test_gpu_stale_epoch.py): False lets a pipelined
        # launch skip the wait for host-issued writes, to show the device's
        # epoch-window check catching the resulting stale flags
        self._order_after_host_writes = True
        # test hook only (tests/test_gpu_skew.py): seconds this rank sleeps before
        # its first sweep launch, after that sweep's collectives -- a rank that
        # arrives late, as host jitter or a slow first collective makes it
        self._first_launch_delay_s = 0.0
        # dyadic covariates (include/ame_amd.h): none -> no buffers, Yt as packed
        self.p = 0
        self.beta = None
        self._covar_H = None
        if getattr(model, "W", None) is not None:
            self._init_covariates(model)
        if self.masked:
            self._init_missing(model.missing)
        if self.binary:
            self._init_binary(model)
        self._mark_host_writes()

    # ------------------------------------------------------------------
    # missing dyads (ame_pack_mask / ame_fill_missing)
    # ------------------------------------------------------------------
    def pack_mask(self, mask, what="mask", symmetric=True):
        """(n, n, S) bool / uint8 mask -> (Mt [S][n][nw] int64, pairs [S] int64,
        deg [S][n] int32) on the device (ame_pack_mask); an asymmetric mask
        raises ValueError unless symmetric=False (the ties of a binary network:
        only the words mean anything then)."""
        m = torch.as_tensor(mask)
        if m.dim() != 3 or tuple(m.shape[:2]) != (self.n, self.n) or m.shape[2] < 1:
            raise ValueError(f"{what} has shape {tuple(m.shape)}, expected ({self.n}, {self.n}, S)")
        if m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"{what} has dtype {m.dtype}, expected bool or uint8")
        S = int(m.shape[2])
        nw = (self.n + 63) // 64
        dims = _lib.ame_dims(self.n, self.r, S, 0, S, self.vcode)
        with torch.cuda.device(self.dev):
            src = m.detach().to(torch.uint8).to(self.dev).contiguous()
            Mt = torch.empty(S, self.n, nw, dtype=torch.int64, device=self.dev)
            pairs = torch.empty(S, dtype=torch.int64, device=self.dev)
            deg = torch.empty(S, self.n, dtype=torch.int32, device=self.dev)
            asym = torch.empty(1, dtype=torch.int64, device=self.dev)
        _lib.check(self.L.ame_pack_mask(_ptr(src), _ptr(Mt), ctypes.byref(dims), _ptr(pairs), _ptr(deg),
                                        _ptr(asym), self._sp()), "ame_pack_mask")
        bad = int(asym.item())
        del src
        if bad and symmetric:
            raise ValueError(f"{what} is not symmetric: {bad // 2} pair(s) with mask[i, j, t] != "
                             "mask[j, i, t] (the unit is the unordered pair)")
        return Mt, pairs, deg

    def _init_missing(self, mask):
        """Pack the mask once, keep the packed observations as Yt_raw and make Yt
        a separate working buffer (a copy: observed entries are never written
        again, hidden ones are overwritten by every fill)."""
        if tuple(mask.shape) != (self.n, self.n, self.T):
            raise ValueError(f"mask has shape {tuple(mask.shape)}, expected ({self.n}, {self.n}, {self.T})")
        self.Mt, self.pairs, self.deg = self.pack_mask(mask)
        self.hidden_pairs = [int(v) for v in self.pairs.cpu().tolist()]
        self.pairs_obs = self.T * self.n * (self.n - 1) // 2 - sum(self.hidden_pairs)
        if self.pairs_obs < 1:
            raise ValueError("every dyad is hidden: nothing to fit")
        with torch.cuda.device(self.dev):
            self.Yt_raw = self.Yt
            self.Yt = self.Yt_raw.clone()
            self.corr = torch.zeros(self.T, 2, dtype=torch.float64, device=self.dev)
            ws = int(self.L.ame_fill_work_size(ctypes.byref(self.dims)))
            if ws < 0:
                _lib.check(-1, "ame_fill_work_size")
            self.fill_work = torch.empty(ws, dtype=torch.float64, device=self.dev)
            self._deg64 = self.deg.double()
        if sum(self.hidden_pairs):   # the two rows of a hidden pair hold different values
            self.swap_consistent = False
        self._fill_valid = False
        self._hidden_host = None

    def fill_missing(self):
        """Refill the hidden entries of the working network from the current
        means, on the main stream (ame_fill_missing): after the sweep that
        produced them has been committed there, before the ELBO of that state and
        before the next sweep, which is ordered after the main stream."""
        a = _lib.ame_fill_args(x=_ptr(self.x_a), Mt=_ptr(self.Mt), Yt=_ptr(self.Yt), rinv=self.C.rinv4(),
                               corr=_ptr(self.corr), work=_ptr(self.fill_work))
        tok = self._tic("fill")
        _lib.check(self.L.ame_fill_missing(ctypes.byref(self.dims), ctypes.byref(a), self._sp()),
                   "ame_fill_missing")
        self._toc(tok)
        self._fill_valid = True
        self._hidden_host = None

    # ------------------------------------------------------------------
    # binary networks (ame_probit_fill / ame_probit_score)
    # ------------------------------------------------------------------
    def _init_binary(self, model):
        """Pack the ties once (ame_pack_mask's layout), keep the packed 0 / 1
        network as Yt_raw and make Yt the working network every sweep reads (a
        copy: the diagonal and the pad column are never written again)."""
        B = model.binary
        if tuple(B.shape) != (self.n, self.n, self.T):
            raise ValueError(f"B has shape {tuple(B.shape)}, expected ({self.n}, {self.n}, {self.T})")
        self.rho = float(model.binary_rho)
        self.Bt, _, _ = self.pack_mask(B, "B", symmetric=False)
        with torch.cuda.device(self.dev):
            if not self.masked:
                self.Yt_raw = self.Yt
                self.Yt = self.Yt_raw.clone()
                self.Mt = None
                self.pairs_obs = self.T * self.n * (self.n - 1) // 2
            self.stat = torch.zeros(self.T, _lib.AME_PROBIT_STATS, dtype=torch.float64, device=self.dev)
            ws = int(self.L.ame_probit_fill_work_size(ctypes.byref(self.dims)))
            if ws < 0:
                _lib.check(-1, "ame_probit_fill_work_size")
            self.probit_work = torch.empty(ws, dtype=torch.float64, device=self.dev)
        self.swap_consistent = False   # the two rows of a pair hold different values
        self._fill_valid = False
        self._hidden_host = None

    def probit_fill(self):
        """Rewrite the working network from the current means on the main stream
        (ame_probit_fill), where the masked path runs fill_missing."""
        a = _lib.ame_probit_fill_args(x=_ptr(self.x_a), Bt=_ptr(self.Bt),
                                      Mt=_ptr(self.Mt) if self.Mt is not None else None, rho=self.rho,
                                      Yt=_ptr(self.Yt), stat=_ptr(self.stat), work=_ptr(self.probit_work),
                                      work_doubles=self.probit_work.numel())
        tok = self._tic("probit_fill")
        _lib.check(self.L.ame_probit_fill(ctypes.byref(self.dims), ctypes.byref(a), self._sp()),
                   "ame_probit_fill")
        self._toc(tok)
        self._fill_valid = True
        self._hidden_host = None

    def _refill(self):
        if self.binary:
            self.probit_fill()
        else:
            self.fill_missing()

    def probit_score(self, x, cov, Yt, Mt=None, mask_select=0):
        """ame_probit_score over a stack of slices: per-slice sums
        [S][AME_PROBIT_SUMS] (fp64, device) of the 0 / 1 network Yt against
        pi = Phi(E[mu] / sqrt(1 + V0)).  Runs on the ELBO stream; the caller has
        dropped speculation."""
        S = int(x.shape[0])
        n, d = self.n, self.d
        assert tuple(x.shape) == (S, n, d) and tuple(cov.shape) == (S, n, d, d)
        assert x.is_contiguous() and cov.is_contiguous()
        chunk, wk = self._slice_chunk(self.L.ame_probit_score_work_size, S)
        with torch.cuda.device(self.dev):
            sums = torch.zeros(S, _lib.AME_PROBIT_SUMS, dtype=torch.float64, device=self.dev)
        with self._elbo_call("probit_score") as sp:
            for s0 in range(0, S, chunk):
                s1 = min(S, s0 + chunk)
                dm = _lib.ame_dims(n, self.r, s1 - s0, 0, s1 - s0, self.vcode)
                a = _lib.ame_probit_score_args(
                    x=_ptr(x[s0:s1]), cov=_ptr(cov[s0:s1]), Yt=_ptr(Yt[s0:s1]), sums=_ptr(sums[s0:s1]),
                    work=_ptr(wk), work_doubles=wk.numel(),
                    Mt=_ptr(Mt[s0:s1]) if Mt is not None else None, mask_select=int(mask_select))
                _lib.check(self.L.ame_probit_score(ctypes.byref(dm), ctypes.byref(a), sp), "ame_probit_score")
        return sums

    def probit_rank(self, x, cov, Yt, nbins, t_max, Mt=None, mask_select=0):
        """ame_probit_rank over a stack of slices: the class histograms
        [S][2][nbins] (int64, device) of the scores t = E[mu] / sqrt(1 + V0) of
        the 0 / 1 network Yt.  Whole slices at a time within the scratch budget
        of predict(); integer counts, so a slice's row does not depend on the
        split.  Runs on the ELBO stream; the caller has dropped speculation."""
        from . import links
        S = int(x.shape[0])
        n, d = self.n, self.d
        assert tuple(x.shape) == (S, n, d) and tuple(cov.shape) == (S, n, d, d)
        assert x.is_contiguous() and cov.is_contiguous()
        nbins, t_max = links.check_bins(nbins, t_max)
        chunk, wk = self._slice_chunk(self.L.ame_probit_rank_work_size, S)
        with torch.cuda.device(self.dev):
            hist = torch.empty(S, 2, nbins, dtype=torch.int64, device=self.dev)
        with self._elbo_call("probit_rank") as sp:
            for s0 in range(0, S, chunk):
                s1 = min(S, s0 + chunk)
                dm = _lib.ame_dims(n, self.r, s1 - s0, 0, s1 - s0, self.vcode)
                a = _lib.ame_probit_rank_args(
                    x=_ptr(x[s0:s1]), cov=_ptr(cov[s0:s1]), Yt=_ptr(Yt[s0:s1]), hist=_ptr(hist[s0:s1]),
                    work=_ptr(wk), work_doubles=wk.numel(),
                    Mt=_ptr(Mt[s0:s1]) if Mt is not None else None, mask_select=int(mask_select),
                    nbins=nbins, t_max=t_max, scale=links.scale(nbins, t_max))
                _lib.check(self.L.ame_probit_rank(ctypes.byref(dm), ctypes.byref(a), sp), "ame_probit_rank")
        return hist

    def probit_select(self, x, cov, Yt, nbins, t_max, bin_min, offset, tie_filter=-1, Mt=None, mask_select=0):
        """ame_probit_select over a stack of slices: every selected entry whose
        bin is at least bin_min[s] (and whose class is tie_filter, if 0 or 1)
        as a record in slice s's region [offset[s], offset[s + 1]).  bin_min
        (S,) and offset (S + 1,) are host integers.  Returns (records: int64
        words on the device, 3 per record, links.RECORD; count (S,) int64:
        the entries that passed, which exceeds a region's size where some were
        dropped).  Chunked like probit_rank; runs on the ELBO stream."""
        from . import links
        S = int(x.shape[0])
        n, d = self.n, self.d
        assert tuple(x.shape) == (S, n, d) and tuple(cov.shape) == (S, n, d, d)
        assert x.is_contiguous() and cov.is_contiguous()
        nbins, t_max = links.check_bins(nbins, t_max)
        off = torch.as_tensor(offset, dtype=torch.int64).reshape(-1)
        bmin = torch.as_tensor(bin_min, dtype=torch.int32).reshape(-1)
        if off.numel() != S + 1 or bmin.numel() != S or int(off[0]) < 0 or bool((off[1:] < off[:-1]).any()):
            raise ValueError("probit_select: offset must hold S + 1 non-decreasing record offsets from >= 0 "
                             "and bin_min S bins")
        chunk, wk = self._slice_chunk(self.L.ame_probit_select_work_size, S)
        with torch.cuda.device(self.dev):
            rec = torch.zeros(max(1, int(off[-1])) * (links.RECORD.itemsize // 8), dtype=torch.int64,
                              device=self.dev)
            count = torch.empty(S, dtype=torch.int64, device=self.dev)
            d_off, d_bmin = off.to(self.dev), bmin.to(self.dev)
        with self._elbo_call("probit_select") as sp:
            for s0 in range(0, S, chunk):
                s1 = min(S, s0 + chunk)
                dm = _lib.ame_dims(n, self.r, s1 - s0, 0, s1 - s0, self.vcode)
                a = _lib.ame_probit_select_args(
                    x=_ptr(x[s0:s1]), cov=_ptr(cov[s0:s1]), Yt=_ptr(Yt[s0:s1]), work=_ptr(wk),
                    work_doubles=wk.numel(), Mt=_ptr(Mt[s0:s1]) if Mt is not None else None,
                    mask_select=int(mask_select), nbins=nbins, t_max=t_max, scale=links.scale(nbins, t_max),
                    bin_min=_ptr(d_bmin[s0:s1]), tie_filter=int(tie_filter), slice0=s0,
                    offset=_ptr(d_off[s0:s1 + 1]), count=_ptr(count[s0:s1]), records=_ptr(rec))
                _lib.check(self.L.ame_probit_select(ctypes.byref(dm), ctypes.byref(a), sp), "ame_probit_select")
        return rec, count

    # ------------------------------------------------------------------
    # residual diagnostics (ame_resid_nodes / ame_resid_hist / ame_resid_select)
    # ------------------------------------------------------------------
    def _resid_chunks(self, x, cov, work_size):
        S = int(x.shape[0])
        assert tuple(x.shape) == (S, self.n, self.d) and tuple(cov.shape) == (S, self.n, self.d, self.d)
        assert x.is_contiguous() and cov.is_contiguous()
        chunk, wk = self._slice_chunk(work_size, S)
        return S, chunk, wk

    def resid_nodes(self, x, cov, Yt, include_noise=True, Mt=None, mask_select=0):
        """ame_resid_nodes over a stack of slices: the per-node sums
        [S][n][AME_NODE_SUMS] (fp64, device) of the dyad scores of Yt.  Whole
        slices at a time within the scratch budget of predict(); a slice's rows
        do not depend on the split.  Runs on the ELBO stream; the caller has
        dropped speculation."""
        S, chunk, wk = self._resid_chunks(x, cov, self.L.ame_resid_nodes_work_size)
        n = self.n
        with torch.cuda.device(self.dev):
            node = torch.empty(S, n, _lib.AME_NODE_SUMS, dtype=torch.float64, device=self.dev)
        with self._elbo_call("resid_nodes") as sp:
            for s0 in range(0, S, chunk):
                s1 = min(S, s0 + chunk)
                dm = _lib.ame_dims(n, self.r, s1 - s0, 0, s1 - s0, self.vcode)
                a = _lib.ame_resid_nodes_args(
                    x=_ptr(x[s0:s1]), cov=_ptr(cov[s0:s1]), Yt=_ptr(Yt[s0:s1]),
                    noise=self.noise4(include_noise), node=_ptr(node[s0:s1]), work=_ptr(wk),
                    work_doubles=wk.numel(), Mt=_ptr(Mt[s0:s1]) if Mt is not None else None,
                    mask_select=int(mask_select))
                _lib.check(self.L.ame_resid_nodes(ctypes.byref(dm), ctypes.byref(a), sp), "ame_resid_nodes")
        return node

    def resid_hist(self, x, cov, Yt, nbins, m2_max, include_noise=True, Mt=None, mask_select=0):
        """ame_resid_hist over a stack of slices: the histograms [S][nbins]
        (int64, device) of the pairs' m^2.  Chunked like resid_nodes; integer
        counts, so a slice's row does not depend on the split."""
        from . import residuals
        nbins, m2_max = residuals.check_bins(nbins, m2_max)
        S, chunk, wk = self._resid_chunks(x, cov, self.L.ame_resid_hist_work_size)
        n = self.n
        with torch.cuda.device(self.dev):
            hist = torch.empty(S, nbins, dtype=torch.int64, device=self.dev)
        with self._elbo_call("resid_hist") as sp:
            for s0 in range(0, S, chunk):
                s1 = min(S, s0 + chunk)
                dm = _lib.ame_dims(n, self.r, s1 - s0, 0, s1 - s0, self.vcode)
                a = _lib.ame_resid_hist_args(
                    x=_ptr(x[s0:s1]), cov=_ptr(cov[s0:s1]), Yt=_ptr(Yt[s0:s1]),
                    noise=self.noise4(include_noise), hist=_ptr(hist[s0:s1]), work=_ptr(wk),
                    work_doubles=wk.numel(), Mt=_ptr(Mt[s0:s1]) if Mt is not None else None,
                    mask_select=int(mask_select), nbins=nbins, scale=residuals.scale(nbins, m2_max))
                _lib.check(self.L.ame_resid_hist(ctypes.byref(dm), ctypes.byref(a), sp), "ame_resid_hist")
        return hist

    def resid_select(self, x, cov, Yt, nbins, m2_max, bin_min, offset, include_noise=True, Mt=None,
                     mask_select=0):
        """ame_resid_select over a stack of slices: every selected pair whose bin
        of m^2 is at least bin_min[s] as a record in slice s's region
        [offset[s], offset[s + 1]).  bin_min (S,) and offset (S + 1,) are host
        integers.  Returns (records: int64 words on the device, 5 per record,
        residuals.RECORD; count (S,) int64: the pairs that passed, which exceeds
        a region's size where some were dropped).  Chunked like resid_hist."""
        from . import residuals
        nbins, m2_max = residuals.check_bins(nbins, m2_max)
        S, chunk, wk = self._resid_chunks(x, cov, self.L.ame_resid_select_work_size)
        n = self.n
        off = torch.as_tensor(offset, dtype=torch.int64).reshape(-1)
        bmin = torch.as_tensor(bin_min, dtype=torch.int32).reshape(-1)
        if off.numel() != S + 1 or bmin.numel() != S or int(off[0]) < 0 or bool((off[1:] < off[:-1]).any()):
            raise ValueError("resid_select: offset must hold S + 1 non-decreasing record offsets from >= 0 "
                             "and bin_min S bins")
        with torch.cuda.device(self.dev):
            rec = torch.zeros(max(1, int(off[-1])) * (residuals.RECORD.itemsize // 8), dtype=torch.int64,
                              device=self.dev)
            count = torch.empty(S, dtype=torch.int64, device=self.dev)
            d_off, d_bmin = off.to(self.dev), bmin.to(self.dev)
        with self._elbo_call("resid_select") as sp:
            for s0 in range(0, S, chunk):
                s1 = min(S, s0 + chunk)
                dm = _lib.ame_dims(n, self.r, s1 - s0, 0, s1 - s0, self.vcode)
                a = _lib.ame_resid_select_args(
                    x=_ptr(x[s0:s1]), cov=_ptr(cov[s0:s1]), Yt=_ptr(Yt[s0:s1]),
                    noise=self.noise4(include_noise), work=_ptr(wk), work_doubles=wk.numel(),
                    Mt=_ptr(Mt[s0:s1]) if Mt is not None else None, mask_select=int(mask_select),
                    nbins=nbins, scale=residuals.scale(nbins, m2_max), bin_min=_ptr(d_bmin[s0:s1]),
                    slice0=s0, reserved=0, offset=_ptr(d_off[s0:s1 + 1]), count=_ptr(count[s0:s1]),
                    records=_ptr(rec))
                _lib.check(self.L.ame_resid_select(ctypes.byref(dm), ctypes.byref(a), sp), "ame_resid_select")
        return rec, count

    def mask_args(self, select):
        """(Yt, Mt, mask_select) for predict / mstep_stats: the packed observations
        (never the working network) with the mask and a selector, or the
        network every kernel reads when nothing is masked."""
        if not self.masked:
            if select:
                raise ValueError("a subset needs a mask (model.set_missing)")
            return (self.Yt_raw if self.binary else self.Yt), None, 0
        return self.Yt_raw, self.Mt, int(select)

    # ------------------------------------------------------------------
    # dyadic covariates (ame_covar_stats / ame_covar_resid)
    # ------------------------------------------------------------------
    def _init_covariates(self, model):
        """Pack the covariates W (p, n, n, T, 2) plane by plane as Y is packed,
        keep the packed observations as Yt_raw and make Yt a separate buffer
        holding the residual Y - sum_k beta_k W_k at the model's beta: every
        launch keeps reading self.Yt."""
        sh = self.shard   # the whole time axis: __init__ refused a time-sharded run
        W = model.W.detach()
        p = int(W.shape[0])
        if W.dim() != 5 or tuple(W.shape[1:]) != (self.n, self.n, self.T, 2) \
                or not 1 <= p <= _lib.AME_MAX_COVARIATES:
            raise ValueError(f"covariates have shape {tuple(W.shape)}, expected (p, {self.n}, {self.n}, "
                             f"{self.T}, 2) with 1 <= p <= {_lib.AME_MAX_COVARIATES}")
        with torch.cuda.device(self.dev):
            self.Wt = torch.empty(p, sh.T_local, self.n, self.ny, 2, dtype=torch.float32, device=self.dev)
            mm = torch.zeros(1, dtype=torch.int64, device=self.dev)
            for k in range(p):
                src = W[k].float().to(self.dev).contiguous()
                _lib.check(self.L.ame_pack_y(_ptr(src), _ptr(self.Wt[k]), ctypes.byref(self.dims),
                                             _ptr(mm), self._sp()), "ame_pack_y")
                del src
            # the residual is swap-consistent when Y and every covariate are
            self.swap_consistent = self.swap_consistent and int(mm.item()) == 0
            self.Yt_raw = self.Yt
            self.Yt = torch.empty_like(self.Yt_raw)
        self.p = p
        self.set_beta(model.beta)

    def set_beta(self, beta):
        """Rebuild the residual Yt = Yt_raw - sum_k beta_k Wt[k] (ame_covar_resid)
        from the raw observations -- never incrementally, so nothing drifts --
        ordered after any dropped speculative sweep."""
        if not self.p:
            raise ValueError("set_beta: the model has no covariates")
        b = [float(v) for v in torch.as_tensor(beta).detach().double().flatten().tolist()]
        if len(b) != self.p:
            raise ValueError(f"beta has {len(b)} entries, expected {self.p}")
        self.discard_speculation()
        cb = (ctypes.c_double * self.p)(*b)
        _lib.check(self.L.ame_covar_resid(ctypes.byref(self.dims), _ptr(self.Yt_raw), _ptr(self.Wt), cb,
                                          self.p, _ptr(self.Yt), self._sp()), "ame_covar_resid")
        self.beta = torch.tensor(b, dtype=torch.float64)
        self._mark_host_writes()
        self.invalidate()

    def covar_stats(self, x=None):
        """Per-slice covariate statistics of the current means (or the given
        [T_local][n][d] means) against the residual Yt: ``G`` [T_local][p][2][2]
        and ``H`` [T_local][p][p][2][2], fp64 on the device (ame_covar_stats).
        H depends on the data alone: it is computed by the first call and kept.
        Whole slices at a time within the scratch budget of predict(); a slice's
        row does not depend on the split."""
        if not self.p:
            raise ValueError("covar_stats: the model has no covariates")
        self.discard_speculation()
        n, p, TL = self.n, self.p, self.shard.T_local
        if x is None:
            x = self.x_a
        assert tuple(x.shape) == (TL, n, self.d) and x.is_contiguous()

        def ame_covar_work_size(dm):   # the one-argument query _slice_chunk takes, at this p
            return self.L.ame_covar_work_size(dm, p)

        chunk, wk = self._slice_chunk(ame_covar_work_size, TL)
        want_h = self._covar_H is None
        with torch.cuda.device(self.dev):
            G = torch.empty(TL, p, 2, 2, dtype=torch.float64, device=self.dev)
            H = torch.empty(TL, p, p, 2, 2, dtype=torch.float64, device=self.dev) if want_h else None
            # the p planes of a slice range are not contiguous: a chunked call gets a
            # copy, made on the main stream before the ELBO stream is ordered after it
            wparts = [self.Wt if chunk >= TL else self.Wt[:, s0:min(TL, s0 + chunk)].contiguous()
                      for s0 in range(0, TL, chunk)]
        with self._elbo_call("covar") as sp:
            for c, s0 in enumerate(range(0, TL, chunk)):
                s1 = min(TL, s0 + chunk)
                dm = _lib.ame_dims(n, self.r, s1 - s0, self.shard.t_begin + s0, self.shard.T_total,
                                   self.vcode)
                a = _lib.ame_covar_args(
                    x=_ptr(x[s0:s1]), Yt=_ptr(self.Yt[s0:s1]), Wt=_ptr(wparts[c]), p=p,
                    G=_ptr(G[s0:s1]), H=_ptr(H[s0:s1]) if want_h else None, work=_ptr(wk),
                    work_doubles=wk.numel())
                _lib.check(self.L.ame_covar_stats(ctypes.byref(dm), ctypes.byref(a), sp),
                           "ame_covar_stats")
        for t in (x, self.Yt, self.Wt, wk, G, *wparts):
            t.record_stream(self._elbo_stream())
        if want_h:
            H.record_stream(self._elbo_stream())
            self._covar_H = H
        return G, self._covar_H

    def _cu_stream(self, first, num, slot=0):
        """A stream over compute units [first, first + num) (C-ABI, HIP CU mask),
        shared by every engine of the process and never destroyed: the caching
        allocator keeps events on the streams its blocks were used on
        (record_stream), so a stream must outlive every tensor an engine drops."""
        key = (self.dev.index, int(first), int(num), int(slot))
        st = _CU_STREAMS.get(key)
        if st is None:
            p = ctypes.c_void_p()
            with torch.cuda.device(self.dev):
                _lib.check(self.L.ame_stream_create_cu_range(int(first), int(num), ctypes.byref(p)),
                           "ame_stream_create_cu_range")
            st = _CU_STREAMS[key] = torch.cuda.ExternalStream(p.value, device=self.dev)
        return st

    def _elbo_stream(self):
        """The stream the ELBO kernels run on: the main stream, or (elbo_cus) the
        CU-masked ELBO stream."""
        return self.stream if self.elbo_stream is None else self.elbo_stream

    def _elbo_call(self, name):
        """``with self._elbo_call(name) as sp:`` launches on the ELBO stream (handle
        sp), timed as `name` (kernel_ms)."""
        return _ElboCall(self, name)

    def _scratch(self, need):
        """The shared scratch of the calls beside the sweep, at least `need` doubles."""
        if self._side_work is None or self._side_work.numel() < need:
            with torch.cuda.device(self.dev):
                self._side_work = torch.empty(need, dtype=torch.float64, device=self.dev)
        return self._side_work

    def _slice_chunk(self, work_size, S):
        """(slices per call, scratch) for S independent slices scored in whole
        slices within PREDICT_WORK_DOUBLES; work_size is the library's query."""
        one = _lib.ame_dims(self.n, self.r, 1, 0, 1, self.vcode)
        per = int(work_size(ctypes.byref(one)))
        if per < 0:
            _lib.check(-1, work_size.__name__)
        chunk = max(1, min(S, self.PREDICT_WORK_DOUBLES // per))
        dims = _lib.ame_dims(self.n, self.r, chunk, 0, chunk, self.vcode)
        return chunk, self._scratch(int(work_size(ctypes.byref(dims))))

    def _mark_host_writes(self):
        """Record the main-stream position after host-issued writes to the state
        or the sweep's flags (uploads, zero fills, set_means / set_covs).  A
        pipelined launch orders itself on the device against the previous sweep
        only; this event orders it after these writes as well (its stream has no
        other tie to the main stream)."""
        ev = torch.cuda.Event()
        ev.record(self.stream)
        self._host_ready = ev

    # current state (ring slot _cur)
    @property
    def x_a(self) -> torch.Tensor:
        return self.xs[self._cur]

    @property
    def cov(self) -> torch.Tensor:
        return self.covs[self._cur]

    # ------------------------------------------------------------------
    def _sp(self):
        return ctypes.c_void_p(self.stream.cuda_stream)

    def _tic(self, name, stream=None):
        if not self.timing:
            return None
        s = self.stream if stream is None else stream
        e = torch.cuda.Event(enable_timing=True)
        e.record(s)
        return (name, e, s)

    def _toc(self, tok, stream=None):
        if tok is None:
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record(tok[2] if stream is None else stream)
        self.events.append((tok[0], tok[1], e))

    def kernel_ms(self):
        """Average device ms per launch of each timed kernel (synchronises)."""
        torch.cuda.synchronize(self.dev)
        acc = {}
        for name, a, b in self.events:
            acc.setdefault(name, []).append(a.elapsed_time(b))
        return {k: sum(v) / len(v) for k, v in acc.items()}, {k: len(v) for k, v in acc.items()}

    def _pack_y(self, Y):
        if Y is None:
            raise ValueError("No data generated yet. Call generate_data() first.")
        sh = self.shard
        src = Y.detach()
        if src.dtype != torch.float32:
            src = src.float()
        src = src.to(self.dev).contiguous()
        ysz = int(self.L.ame_pack_y_size(ctypes.byref(self.dims)))
        if ysz < 0:
            _lib.check(-1, "ame_pack_y_size")
        self.ny = ysz // (2 * sh.T_local * self.n)   # row stride: n rounded up to even
        self.Yt = torch.empty(sh.T_local, self.n, self.ny, 2, dtype=torch.float32, device=self.dev)
        mm = torch.zeros(1, dtype=torch.int64, device=self.dev)
        rc = self.L.ame_pack_y(_ptr(src), _ptr(self.Yt), ctypes.byref(self.dims), _ptr(mm),
                               self._sp())
        _lib.check(rc, "ame_pack_y")
        self.swap_consistent = int(mm.item()) == 0
        del src

    # ------------------------------------------------------------------
    def _launch_sweep(self, spec=False):
        """Enqueue one sweep from the newest state (the last queued sweep's
        output, or the current state) into the next ring slot; returns
        (done-events, slot).
        A speculative sweep in pipelined mode is queued while the previous sweep
        (epoch - 1) still runs and orders itself slice by slice on the device;
        any other sweep is ordered after everything queued on the main stream.
        Pipelined engines alternate their launches -- sweeps and slice groups --
        over the two sweep streams, so launch j + 1 runs beside launch j and
        launch j + 2 queues behind launch j (at most two co-resident); otherwise
        a sweep's groups run in order on one stream."""
        plan = self.plan
        src = self._specs[-1][1] if self._specs else self._cur
        dst = (src + 1) % len(self.xs)
        self.epoch += 1
        _note_epoch(self.epoch)
        pipe = spec and plan.pipelined and self.speculation
        halo_in = halo_out = next_old = back_in = back_out = None
        if self.halo is not None:
            # a pipelined launch takes next_old from the back channel instead of a
            # collective that would wait for the running sweep
            next_old, halo_in, halo_out = self.halo.before_sweep(
                self, gather=not pipe, first=self.xs[src][0])
            back_in, back_out = self.halo.back_channels(self)
        if self._first_launch_delay_s:
            time.sleep(self._first_launch_delay_s)
            self._first_launch_delay_s = 0.0
        wait = self.epoch - 1 if pipe else 0
        ready = None
        if not pipe:
            ready = torch.cuda.Event()
            ready.record(self.stream)
        prev = self._specs[-1][0] if self._specs else []
        used = []

        def order(stream):   # first launch of this sweep on `stream`
            if stream in used:
                return
            used.append(stream)
            if pipe:
                if self._order_after_host_writes:
                    stream.wait_event(self._host_ready)
            else:
                stream.wait_event(ready)
                for ev in prev:   # its input slot is the output of the last queued sweep
                    stream.wait_event(ev)

        tok = None
        n, d, sh = self.n, self.d, self.shard
        last = len(plan.groups) - 1
        stream = None
        for g, (off, size) in enumerate(plan.groups):
            if plan.pipelined:
                par = self._launch_ctr & 1
                self._launch_ctr += 1
            else:
                par = 0
            stream = self.sweep_streams[par if plan.pipelined else (self.epoch & 1)]
            order(stream)
            if tok is None:
                tok = self._tic("sweep", stream)

            def at(t, slices, per_slice, esize):   # pointer to local slice `slices` of t
                return ctypes.c_void_p(t.data_ptr() + slices * per_slice * esize)
            nd, ndd, nn2 = n * d, n * d * d, n * self.ny * 2
            g_halo_in = halo_in if g == 0 else at(self.hand, off - 1, nd, 8)
            g_halo_out = halo_out if g == last else None
            g_next_old = next_old if g == last else at(self.xs[src], off + size, nd, 4)
            dims = _lib.ame_dims(n, self.r, size, sh.t_begin + off, sh.T_total, self.vcode)
            a = _lib.ame_sweep_args(
                kind=plan.group_kinds[size], work_doubles=plan.work_doubles,
                Yt=at(self.Yt, off, nn2, 4), x_old=at(self.xs[src], off, nd, 4),
                x_new=at(self.xs[dst], off, nd, 4), next_old=g_next_old,
                hand=at(self.hand, off, nd, 8), halo_in=g_halo_in, halo_out=g_halo_out,
                cov=at(self.covs[src], off, ndd, 4), consts=_ptr(self.consts),
                rinv=self.C.rinv4(), lr=self.lr, one_minus_lr=float(1.0 - self.lr),
                epoch=self.epoch, status=_ptr(self.status),
                work=at(self.sweep_work, par, plan.work_doubles, 8),
                cov_new=at(self.covs[dst], off, ndd, 4), done=at(self.done, off, 1, 4),
                wait_epoch=wait, back_out=back_out if g == 0 else None,
                back_in=back_in if g == last else None,
                flags=(_lib.AME_SWEEP_FLAG_NEXT_GROUP if g < last else 0)
                | (_lib.AME_SWEEP_FLAG_PREV_GROUP if g > 0 else 0))
            _lib.check(self.L.ame_sweep(ctypes.byref(dims), ctypes.byref(a),
                                        ctypes.c_void_p(stream.cuda_stream)), "ame_sweep")
        self._toc(tok, stream)
        # the kernels take raw pointers: tell the caching allocator these streams
        # use the buffers, so a dropped engine's memory is not handed out again
        # while a sweep still reads or writes it
        done = []
        for st in used:
            for t in (self.xs[src], self.xs[dst], self.covs[src], self.covs[dst], self.hand,
                      self.done, self.status, self.sweep_work, self.Yt, self.consts):
                t.record_stream(st)
            ev = torch.cuda.Event()
            ev.record(st)
            done.append(ev)
        return done, dst

    def _commit(self, slot):
        self._cur = slot
        self._out_valid = False
        self._cov_terms_valid = False
        self._fill_valid = False

    def sweep(self):
        """One Gauss-Seidel sweep + covariance update (reference _update_step).
        A sweep already started from this state (speculate) is only committed."""
        if self._specs:
            done, slot = self._specs.popleft()
        else:
            if self.refill and not self._fill_valid:   # first sweep, or after set_means
                self._refill()
            done, slot = self._launch_sweep()
        for ev in done:
            self.stream.wait_event(ev)
        self._commit(slot)
        if self.refill:   # one fill serves this state's ELBO correction and the next sweep
            self._refill()
        if self.halo is not None:
            self.halo.after_sweep(self)

    def speculate(self, ahead=1):
        """Keep min(ahead, spec_depth) sweeps started beyond the current state.
        Each reads the previous one's output ring slot; none touches the current
        state, and the oldest slot it overwrites belongs to a state whose ELBO
        the host has already read."""
        if not self.speculation:
            return
        want = min(int(ahead), self.plan.spec_depth)
        while len(self._specs) < want:
            self._specs.append(self._launch_sweep(spec=True))

    def discard_speculation(self):
        """Drop started sweeps that will not be committed.  They write only
        spare ring slots; later main-stream work is ordered after them."""
        while self._specs:
            done, _ = self._specs.popleft()
            for ev in done:
                self.stream.wait_event(ev)

    def refresh_cov_terms(self):
        """Covariance ELBO terms of the current covariances (no update)."""
        c = _lib.ame_cov_args(cov=_ptr(self.cov), consts=_ptr(self.consts),
                              cov_terms=_ptr(self.cov_terms))
        with self._elbo_call("cov") as sp:
            _lib.check(self.L.ame_cov(ctypes.byref(self.dims), ctypes.byref(c), sp), "ame_cov")
        self._cov_terms_valid = True

    def launch_elbo(self, pairs_only=False):
        """The ELBO / MSE sums of the current state into self.out.  pairs_only
        (diagnostic timing): the pair kernel alone through ame_elbo_pairs_diag,
        which writes no sums."""
        if not pairs_only and not self._cov_terms_valid:
            self.refresh_cov_terms()
        if self.refill and not self._fill_valid:
            self._refill()
        prev_final = None
        if self.halo is not None and not pairs_only:
            prev_final = self.halo.prev_final(self)
        e = _lib.ame_elbo_args(
            Yt=_ptr(self.Yt), x=_ptr(self.x_a), prev_final=prev_final,
            cov_terms=_ptr(self.cov_terms), consts=_ptr(self.consts), phi=_ptr(self.phi),
            rinv=self.C.rinv4(), swap_consistent=1 if self.swap_consistent else 0,
            work=_ptr(self.work), out=_ptr(self.out), pairs_kernel=self.options.pairs_kernel)
        launch, what = ((self.L.ame_elbo_pairs_diag, "ame_elbo_pairs_diag") if pairs_only
                        else (self.L.ame_elbo, "ame_elbo"))
        with self._elbo_call("pairs" if pairs_only else "elbo") as sp:
            _lib.check(launch(ctypes.byref(self.dims), ctypes.byref(e), sp), what)

    def sums(self, speculate=0):
        """The 8 fp64 sums for the current state (all ranks reduced).  With
        speculate=k > 0 (iterations still to come) up to k next sweeps are
        started first and run beside them."""
        if not self._out_valid:
            if self.elbo_first:
                # the sweep's `ready` event (main stream) then follows the ELBO
                self.launch_elbo()
                if speculate:
                    self.speculate(int(speculate))
            else:
                if speculate:
                    self.speculate(int(speculate))
                self.launch_elbo()
            out = self.out
            if self.halo is not None:
                out = self.halo.allreduce_sums(out)
            self._out_host = out.cpu().tolist()
            self._check_status()
            self._out_valid = True
        return self._out_host

    def terms(self, speculate=0):
        out = self.sums(speculate)
        if self.binary:
            if self._hidden_host is None:
                # the bound and the Brier sum, slice by slice in time order, and each
                # node's trace once per observed partner
                rows = self.stat.cpu().tolist()
                bound = brier = 0.0
                for row in rows:
                    bound += row[1]
                    brier += row[2]
                if self.masked:
                    tr = self.cov_terms.view(self.T, self.n, 4)[:, :, 1]
                    deg_trace = float((self._deg64 * tr).sum().item())
                else:
                    deg_trace = (self.n - 1) * out[1]
                self._hidden_host = ((bound, brier), deg_trace)
            bin_sums, deg_trace = self._hidden_host
            return assemble(out, self.n, self.T, self.d, self.variant, self.C, pairs_obs=self.pairs_obs,
                            deg_trace=deg_trace, binary=bin_sums)
        if not self.masked:
            return assemble(out, self.n, self.T, self.d, self.variant, self.C)
        if self._hidden_host is None:
            # the state's correction sums, slice by slice in time order, and each
            # node's trace once per observed partner, from cov_terms on the device
            rows = self.corr.cpu().tolist()
            hid = [0.0, 0.0]
            for row in rows:
                hid[0] += row[0]
                hid[1] += row[1]
            tr = self.cov_terms.view(self.T, self.n, 4)[:, :, 1]
            self._hidden_host = (hid, float((self._deg64 * tr).sum().item()))
        hid, deg_trace = self._hidden_host
        return assemble(out, self.n, self.T, self.d, self.variant, self.C, hidden=hid,
                        pairs_obs=self.pairs_obs, deg_trace=deg_trace)

    def _check_status(self):
        words = self.status.cpu().tolist()
        if words[0]:
            self.status.zero_()
            # a later pipelined launch must not start before this zero lands (it
            # would erase that sweep's own status bits)
            self._mark_host_writes()
            self.last_status = words
            raise RuntimeError(f"ame_amd: sweep reported {status_report(words)}")

    def invalidate(self):
        self._out_valid = False
        self._cov_terms_valid = False
        self._fill_valid = False
        self._hidden_host = None

    # ------------------------------------------------------------------
    # state transfer (reference layout (n, T, d[, d]))
    # ------------------------------------------------------------------
    def means_local(self) -> torch.Tensor:
        return self.x_a.permute(1, 0, 2)

    def covs_local(self) -> torch.Tensor:
        return self.cov.permute(1, 0, 2, 3)

    def set_means(self, X_mean: torch.Tensor):
        self.discard_speculation()
        sh = self.shard
        t0, t1 = sh.t_begin, sh.t_begin + sh.T_local
        self.x_a.copy_(X_mean[:, t0:t1].detach().float().permute(1, 0, 2))
        self._mark_host_writes()
        self.invalidate()

    def set_covs(self, X_cov: torch.Tensor):
        self.discard_speculation()
        sh = self.shard
        t0, t1 = sh.t_begin, sh.t_begin + sh.T_local
        self.cov.copy_(X_cov[:, t0:t1].detach().float().permute(1, 0, 2, 3))
        self._mark_host_writes()
        self.invalidate()

    # ------------------------------------------------------------------
    # posterior-predictive dyad moments (ame_predict, include/ame_amd.h)
    # ------------------------------------------------------------------
    # scratch budget of one ame_predict call in doubles (256 MiB): longer slice
    # stacks are scored in chunks of whole slices, which changes no result (the
    # slices are independent and each keeps its own row of sums)
    PREDICT_WORK_DOUBLES = 1 << 25

    def noise4(self, include_noise: bool):
        """N of the predictive covariance: model.R (observations) or zeros (the mean)."""
        vals = self.C.R.flatten().tolist() if include_noise else [0.0] * 4
        return (ctypes.c_double * 4)(*vals)

    def pack_future(self, Y_future: torch.Tensor) -> torch.Tensor:
        """(n, n, h, 2) observations -> the packed [h][n][ny][2] layout (ame_pack_y)."""
        if Y_future.dim() != 4 or tuple(Y_future.shape[:2]) != (self.n, self.n) \
                or Y_future.shape[3] != 2 or Y_future.shape[2] < 1:
            raise ValueError(f"Y_future has shape {tuple(Y_future.shape)}, expected "
                             f"({self.n}, {self.n}, h, 2)")
        h = int(Y_future.shape[2])
        src = Y_future.detach().float().to(self.dev).contiguous()
        dims = _lib.ame_dims(self.n, self.r, h, 0, h, self.vcode)
        Yt = torch.empty(h, self.n, self.ny, 2, dtype=torch.float32, device=self.dev)
        mm = torch.zeros(1, dtype=torch.int64, device=self.dev)
        _lib.check(self.L.ame_pack_y(_ptr(src), _ptr(Yt), ctypes.byref(dims), _ptr(mm), self._sp()),
                   "ame_pack_y")
        return Yt

    def predict(self, x, cov, Yt=None, include_noise=True, zsq=(), csq=(), block=None, Mt=None,
                mask_select=0):
        """ame_predict over a stack of slices: x [S][n][d], cov [S][n][d][d]
        (device, fp32, contiguous).  Yt [S][n][ny][2] -> per-slice sums
        [S][AME_PREDICT_SUMS] (fp64, device); block = (i0, i1, j0, j1) -> dense
        [S][i1-i0][j1-j0][5] (fp32, device).  Returns (sums or None, dense or
        None).  Mt [S][n][nw] (ame_pack_mask) with mask_select = _lib.AME_MASK_OBSERVED
        / AME_MASK_HIDDEN scores only those pairs.  Runs on the ELBO stream; the
        caller has dropped speculation."""
        S = int(x.shape[0])
        n, d = self.n, self.d
        assert tuple(x.shape) == (S, n, d) and tuple(cov.shape) == (S, n, d, d)
        assert x.is_contiguous() and cov.is_contiguous()
        nl = len(zsq)
        chunk, wk = self._slice_chunk(self.L.ame_predict_work_size, S)
        with torch.cuda.device(self.dev):
            sums = torch.zeros(S, _lib.AME_PREDICT_SUMS, dtype=torch.float64,
                               device=self.dev) if Yt is not None else None
            dense = None
            if block is not None:
                i0, i1, j0, j1 = (int(v) for v in block)
                dense = torch.empty(S, i1 - i0, j1 - j0, 5, dtype=torch.float32, device=self.dev)
        with self._elbo_call("predict") as sp:
            for s0 in range(0, S, chunk):
                s1 = min(S, s0 + chunk)
                dm = _lib.ame_dims(n, self.r, s1 - s0, 0, s1 - s0, self.vcode)
                a = _lib.ame_predict_args(
                    x=_ptr(x[s0:s1]), cov=_ptr(cov[s0:s1]),
                    Yt=_ptr(Yt[s0:s1]) if Yt is not None else None,
                    noise=self.noise4(include_noise), n_levels=nl,
                    zsq=(ctypes.c_double * _lib.AME_PREDICT_MAX_LEVELS)(*zsq),
                    csq=(ctypes.c_double * _lib.AME_PREDICT_MAX_LEVELS)(*csq),
                    sums=_ptr(sums[s0:s1]) if sums is not None else None,
                    dense=_ptr(dense[s0:s1]) if dense is not None else None,
                    work=_ptr(wk), Mt=_ptr(Mt[s0:s1]) if Mt is not None else None,
                    mask_select=int(mask_select))
                if block is not None:
                    a.i0, a.i1, a.j0, a.j1 = i0, i1, j0, j1
                _lib.check(self.L.ame_predict(ctypes.byref(dm), ctypes.byref(a), sp), "ame_predict")
        return sums, dense

    # ------------------------------------------------------------------
    # M-step sufficient statistics and new constants (ame_mstep_stats)
    # ------------------------------------------------------------------
    def mstep_stats(self, x=None, cov=None):
        """Per-slice sufficient statistics of the current state (or of the given
        [T_local][n][d] means and [T_local][n][d][d] covariances) for the M-step:
        ``state`` [T_local][2][d][d] (P_t, C_t) and ``dyad`` [T_local][4] (pairs,
        Rss00, Rss11, Rss01), fp64 on the device.  Whole slices at a time within
        the scratch budget of predict(); a slice's row does not depend on the
        split.  Time-sharded: a collective (the left neighbour's last means)."""
        self.discard_speculation()
        n, d, sh = self.n, self.d, self.shard
        TL = sh.T_local
        prev_final = self.halo.prev_final(self) if self.halo is not None else None
        chunk, wk = self._slice_chunk(self.L.ame_mstep_work_size, TL)
        if x is None:
            x, cov = self.x_a, self.cov
        # with hidden dyads: the packed observations and the observed pairs only
        Yt, Mt, sel = self.mask_args(_lib.AME_MASK_OBSERVED if self.masked else 0)
        with torch.cuda.device(self.dev):
            state = torch.empty(TL, 2, d, d, dtype=torch.float64, device=self.dev)
            dyad = torch.empty(TL, 4, dtype=torch.float64, device=self.dev)
        with self._elbo_call("mstep") as sp:
            for s0 in range(0, TL, chunk):
                s1 = min(TL, s0 + chunk)
                dm = _lib.ame_dims(n, self.r, s1 - s0, sh.t_begin + s0, sh.T_total, self.vcode)
                a = _lib.ame_mstep_args(
                    x=_ptr(x[s0:s1]), cov=_ptr(cov[s0:s1]),
                    prev_final=prev_final if s0 == 0 else _ptr(x[s0 - 1]),
                    Yt=_ptr(Yt[s0:s1]), state=_ptr(state[s0:s1]), dyad=_ptr(dyad[s0:s1]),
                    work=_ptr(wk), Mt=_ptr(Mt[s0:s1]) if Mt is not None else None, mask_select=sel)
                _lib.check(self.L.ame_mstep_stats(ctypes.byref(dm), ctypes.byref(a), sp),
                           "ame_mstep_stats")
        return state, dyad

    # ------------------------------------------------------------------
    # goodness of fit (ame_net_moments / ame_net_triads / ame_simulate)
    # ------------------------------------------------------------------
    def _check_packed(self, Yt, what):
        S = int(Yt.shape[0])
        assert tuple(Yt.shape) == (S, self.n, self.ny, 2) and Yt.dtype == torch.float32 \
            and Yt.is_contiguous(), f"{what}: a packed [S][n][ny][2] fp32 network is expected"
        return S

    def net_moments(self, Yt):
        """ame_net_moments over a packed stack Yt [S][n][ny][2]: ``node`` [S][n][2]
        (row_i, col_i) and ``slice`` [S][2] (sum y^2, sum y_ij y_ji), fp64 on the
        device.  Whole slices at a time within the scratch budget of predict();
        a slice's rows do not depend on the split.  Runs on the ELBO stream."""
        S = self._check_packed(Yt, "net_moments")
        chunk, wk = self._slice_chunk(self.L.ame_net_moments_work_size, S)
        with torch.cuda.device(self.dev):
            node = torch.empty(S, self.n, 2, dtype=torch.float64, device=self.dev)
            sl = torch.empty(S, 2, dtype=torch.float64, device=self.dev)
        with self._elbo_call("net_moments") as sp:
            for s0 in range(0, S, chunk):
                s1 = min(S, s0 + chunk)
                dm = _lib.ame_dims(self.n, self.r, s1 - s0, 0, s1 - s0, self.vcode)
                a = _lib.ame_moments_args(Yt=_ptr(Yt[s0:s1]), node=_ptr(node[s0:s1]), slice=_ptr(sl[s0:s1]),
                                          work=_ptr(wk), work_doubles=wk.numel())
                _lib.check(self.L.ame_net_moments(ctypes.byref(dm), ctypes.byref(a), sp), "ame_net_moments")
        for t in (Yt, wk, node, sl):
            t.record_stream(self._elbo_stream())
        return node, sl

    def net_triads(self, Yt, center):
        """ame_net_triads over a packed stack Yt [S][n][ny][2] centred by
        ``center`` [S] (fp32, device): ``tri`` [S][2] fp64 on the device, the
        cycle and the transitive sum.  Chunked as net_moments."""
        S = self._check_packed(Yt, "net_triads")
        assert tuple(center.shape) == (S,) and center.dtype == torch.float32 and center.is_contiguous()
        chunk, wk = self._slice_chunk(self.L.ame_net_triads_work_size, S)
        with torch.cuda.device(self.dev):
            tri = torch.empty(S, 2, dtype=torch.float64, device=self.dev)
        with self._elbo_call("net_triads") as sp:
            for s0 in range(0, S, chunk):
                s1 = min(S, s0 + chunk)
                dm = _lib.ame_dims(self.n, self.r, s1 - s0, 0, s1 - s0, self.vcode)
                a = _lib.ame_triads_args(Yt=_ptr(Yt[s0:s1]), center=_ptr(center[s0:s1]), tri=_ptr(tri[s0:s1]),
                                         work=_ptr(wk), work_doubles=wk.numel())
                _lib.check(self.L.ame_net_triads(ctypes.byref(dm), ctypes.byref(a), sp), "ame_net_triads")
        for t in (Yt, center, wk, tri):
            t.record_stream(self._elbo_stream())
        return tri

    def net_statistics(self, Yt):
        """The raw sums of the five network statistics of a packed stack (which
        must be swap-consistent): {"node", "slice", "tri", "center"} on the
        device, for :func:`ame_amd.gof.combine`.  The centre of the triad sums is
        the mean of the network rounded to fp32, formed on the device from the
        row sums (no host round trip)."""
        node, sl = self.net_moments(Yt)
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            center = (node[:, :, 0].sum(dim=1) / float(self.n * (self.n - 1))).float().contiguous()
        tri = self.net_triads(Yt, center)
        return {"node": node, "slice": sl, "tri": tri, "center": center}

    def sim_chunk(self):
        """Slices of one simulated-network buffer: whole slices within the bytes of
        predict()'s scratch budget."""
        per = self.n * self.ny * 2 * 4
        return max(1, min(self.shard.T_local, self.PREDICT_WORK_DOUBLES * 8 // per))

    def simulate(self, x, noise_chol, seed, sample, out=None, t_begin=0):
        """ame_simulate: one network from the states x [S][n][d] (device, fp32,
        contiguous) of the global slices t_begin .. t_begin + S - 1 into ``out``
        [S][n][ny][2] (allocated when None).  noise_chol = (l00, l10, l11), the
        lower Cholesky factor of the noise covariance; zeros give the mean.  The
        Philox counter names (i, j, global slice, sample): the bits do not depend
        on how the slices are split over calls."""
        S = int(x.shape[0])
        assert tuple(x.shape) == (S, self.n, self.d) and x.dtype == torch.float32 and x.is_contiguous()
        if out is None:
            with torch.cuda.device(self.dev):
                out = torch.empty(S, self.n, self.ny, 2, dtype=torch.float32, device=self.dev)
        assert self._check_packed(out, "simulate") == S
        l3 = (ctypes.c_double * 3)(*(float(v) for v in noise_chol))
        dm = _lib.ame_dims(self.n, self.r, S, int(t_begin), int(t_begin) + S, self.vcode)
        a = _lib.ame_simulate_args(x=_ptr(x), lr=l3, seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                                   sample=int(sample) & 0xFFFFFFFF, Yt_out=_ptr(out))
        with self._elbo_call("simulate") as sp:
            _lib.check(self.L.ame_simulate(ctypes.byref(dm), ctypes.byref(a), sp), "ame_simulate")
        for t in (x, out):
            t.record_stream(self._elbo_stream())
        return out

    def simulated_statistics(self, x, noise_chol, seed, sample):
        """The raw sums (as net_statistics, on the host) of one network simulated
        from the states x [T_local][n][d], slice chunk by slice chunk through one
        reused buffer of sim_chunk() slices: no n^2 T allocation."""
        TL, chunk = int(x.shape[0]), self.sim_chunk()
        if self._sim_buf is None or self._sim_buf.shape[0] != chunk:
            with torch.cuda.device(self.dev):
                self._sim_buf = torch.empty(chunk, self.n, self.ny, 2, dtype=torch.float32, device=self.dev)
        parts = []
        for s0 in range(0, TL, chunk):
            s1 = min(TL, s0 + chunk)
            buf = self._sim_buf[:s1 - s0]
            self.simulate(x[s0:s1], noise_chol, seed, sample, out=buf, t_begin=self.shard.t_begin + s0)
            raw = self.net_statistics(buf)
            # the copy ends before the buffer is simulated into again
            with torch.cuda.stream(self.stream):
                parts.append({k: v.cpu() for k, v in raw.items()})
        return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}

    # ------------------------------------------------------------------
    # exact per-node smoothing across time (ame_smooth)
    # ------------------------------------------------------------------
    def smooth_chunk(self, observed=False):
        """Nodes per ame_smooth call within the scratch budget of predict(): all n,
        or a multiple of 32 (at least 32).  ``observed``: of a call with the mask
        (ame_smooth_masked_work_size)."""
        n = self.n
        size = self.L.ame_smooth_masked_work_size if observed else self.L.ame_smooth_work_size
        w1 = int(size(ctypes.byref(self.dims), 1))
        w2 = int(size(ctypes.byref(self.dims), 2)) if n >= 2 else -1
        if w1 < 0 or w2 < 0:
            _lib.check(-1, "ame_smooth_work_size")
        per, base = w2 - w1, 2 * w1 - w2
        fit = (self.PREDICT_WORK_DOUBLES - base) // per
        return n if fit >= n else min(n, max(32, fit // 32 * 32))

    def smooth(self, stages=0, check=True, observed=False):
        """Each node's exact Gaussian posterior across time given the current
        means of the others (include/ame_amd.h, ame_smooth): new device tensors
        ``mean`` [T][n][d], ``cov`` and ``cross`` [T][n][d][d] (fp32) and
        ``lag_sum`` [T][d][d] (fp64).  Reads x_a, Yt, consts and rinv; writes
        nothing the sweep reads.  Nodes go in chunks (multiples of 32) within
        the scratch budget of predict(); the result has the same bits for any
        chunking.  A node whose factorisation met a non-positive pivot raises
        RuntimeError (its outputs are NaN).  Runs on the ELBO stream.
        With hidden dyads the call is refused unless ``observed=True``: the sums
        then run over each node's observed partners only (Yt_raw and Mt), so the
        covariances widen with the number of hidden partners."""
        if self.halo is not None or self.shard.T_local != self.shard.T_total:
            raise NotImplementedError("smooth is not available on a time-sharded run")
        if observed and not self.masked:
            raise ValueError("smooth(observed=True) needs a mask (model.set_missing)")
        if self.masked and not observed:
            raise NotImplementedError("smooth over all partners is not available with missing dyads: "
                                      "its observation stage would read hidden entries; pass "
                                      "observed=True (vi.smooth(partners=\"observed\"), "
                                      "smoothed=\"observed\")")
        self.discard_speculation()
        n, d, T = self.n, self.d, self.shard.T_local
        chunk = self.smooth_chunk(observed)
        size = self.L.ame_smooth_masked_work_size if observed else self.L.ame_smooth_work_size
        wk = self._scratch(int(size(ctypes.byref(self.dims), chunk)))
        x = self.x_a
        Yt, Mt = (self.Yt_raw, self.Mt) if observed else (self.Yt, None)
        with torch.cuda.device(self.dev):
            mean =torch.empty(T, n, d, dtype=torch.float32, device=self.dev)
            cov = torch.empty(T, n, d, d, dtype=torch.float32, device=self.dev)
            cross = torch.empty(T, n, d, d, dtype=torch.float32, device=self.dev)
            lag = torch.empty(T, d, d, dtype=torch.float64, device=self.dev)
            fail = torch.zeros(_lib.AME_SMOOTH_FAIL_WORDS, dtype=torch.int32, device=self.dev)
        with self._elbo_call("smooth") as sp:
            for i0 in range(0, n, chunk):
                a = _lib.ame_smooth_args(
                    x=_ptr(x), Yt=_ptr(Yt), consts=_ptr(self.consts), rinv=self.C.rinv4(),
                    i0=i0, i1=min(n, i0 + chunk), stages=int(stages), mean=_ptr(mean), cov=_ptr(cov),
                    cross=_ptr(cross), lag_sum=_ptr(lag), fail=_ptr(fail), work=_ptr(wk),
                    work_doubles=wk.numel(), Mt=_ptr(Mt) if Mt is not None else None)
                _lib.check(self.L.ame_smooth(ctypes.byref(self.dims), ctypes.byref(a), sp),
                           "ame_smooth")
        st = self._elbo_stream()
        for t in (x, Yt, self.consts, wk, mean, cov, cross, lag, fail) + (() if Mt is None else (Mt,)):
            t.record_stream(st)
        if check:
            words = [int(w) & 0xFFFFFFFF for w in fail.cpu().tolist()]
            if words[0]:
                raise RuntimeError(f"ame_amd: smooth met a non-positive pivot at {words[0]} node(s); "
                                   f"first reported: node {words[2]}, time {words[3]} (the "
                                   "precision of that node's trajectory is not positive definite)")
        return mean, cov, cross, lag

    def set_constants(self, model):
        """Rebuild the fp64 constants from the model's (updated) fp32 attributes,
        exactly as at construction, and copy them into the device tensors the
        kernels already point to, ordered after any dropped speculative sweep."""
        self.discard_speculation()
        self.C = Constants(model)
        self.consts.copy_(self.C.stack)
        self.phi.copy_(self.C.Phi.contiguous())
        self._mark_host_writes()
        self.invalidate()

    def forecast_states(self, m_last: torch.Tensor, S_last: torch.Tensor, n_steps: int):
        """h-step forecast of the states from the last fitted slice: m_k = Phi
        m_{k-1}, S_k = Phi S_{k-1} Phi' + Q, batched over nodes in fp64 on the
        device and rounded to fp32 once.  Returns [h][n][d], [h][n][d][d]."""
        h = int(n_steps)
        if h < 1:
            raise ValueError("n_steps must be >= 1")
        Phi = self.C.Phi.to(self.dev)
        Q = self.C.Q.to(self.dev)
        m = m_last.to(self.dev).double()
        S = S_last.to(self.dev).double()
        ms, Ss = [], []
        for _ in range(h):
            m = m @ Phi.T
            S = Phi @ S @ Phi.T + Q
            ms.append(m)
            Ss.append(S)
        return torch.stack(ms).float().contiguous(), torch.stack(Ss).float().contiguous()
