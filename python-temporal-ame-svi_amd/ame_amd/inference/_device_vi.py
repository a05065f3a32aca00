"""GPU-backed temporal VI: state lives in HBM, the reference-visible attributes
(``X_mean (n,T,d)``, ``X_cov (n,T,d,d)``, CPU fp32) are lazily synchronised views.

Synchronisation rule: after a device step the device copy is authoritative;
reading ``vi.X_mean`` downloads it once, INTO the host tensor handed out
before (so a reference a caller kept, ``X = vi.X_mean``, sees the fitted
values once the attribute has been read again, like the reference's live
tensor), and remembers the tensor's version counter.  Assigning
``vi.X_mean = ...`` or mutating the host tensor in place (which bumps
``tensor._version``) makes the host copy authoritative again and it is
uploaded before the next device step.

Time-sharded runs: reading ``X_mean`` / ``X_cov`` after a device step is a
COLLECTIVE (every rank's slices are all-gathered), so every rank must read
it, e.g. not only ``if rank == 0``.  ``local_means()`` / ``local_covs()``
return this rank's own slices without communication.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

from .base import BaseTemporalVariationalInference
from ..engine import DeviceEngine, EngineOptions


def default_device():
    if not torch.cuda.is_available():
        return None
    lr = os.environ.get("LOCAL_RANK")
    if lr is not None and torch.cuda.device_count() > 1:
        return torch.device("cuda", int(lr) % torch.cuda.device_count())
    return torch.device("cuda", torch.cuda.current_device())


class SmoothResult:
    """What ``vi.smooth()`` returns: each node's exact Gaussian posterior across
    time given the other nodes' means.  Holds the device tensors (time-major,
    ``d_mean`` [T][n][d], ``d_cov`` / ``d_cross`` [T][n][d][d] fp32, ``d_lag_sum``
    [T][d][d] fp64) and hands out CPU copies in the reference's layout:
    ``mean`` (n, T, d), ``cov`` (n, T, d, d), ``cross`` (n, T, d, d) with
    cross[i, t] = Cov(x_it, x_i,t-1) (zero at t = 0) and ``lag_sum`` (T, d, d)
    = sum_i cross[i, t] in fp64."""

    def __init__(self, mean, cov, cross, lag_sum):
        self.d_mean, self.d_cov, self.d_cross, self.d_lag_sum = mean, cov, cross, lag_sum

    @property
    def mean(self):
        return self.d_mean.permute(1, 0, 2).to("cpu").contiguous()

    @property
    def cov(self):
        return self.d_cov.permute(1, 0, 2, 3).to("cpu").contiguous()

    @property
    def cross(self):
        return self.d_cross.permute(1, 0, 2, 3).to("cpu").contiguous()

    @property
    def lag_sum(self):
        return self.d_lag_sum.to("cpu")


class DeviceTemporalVI(BaseTemporalVariationalInference):
    _variant = "good"

    def __init__(self, model, learning_rate, seed, device=None, distributed=None,
                 engine_options=None):
        self._device = device
        self._distributed = distributed
        self._engine_options = EngineOptions.coerce(engine_options)
        self._engine: Optional[DeviceEngine] = None
        self._halo = None       # the engine's TimeShardHalo (time-sharded runs)
        self._spec_next = 0     # iterations fit() still has to go (speculation window)
        self._host = {"mean": None, "cov": None}
        self._ver = {"mean": None, "cov": None}
        self._stale = {"mean": False, "cov": False}
        super().__init__(model, learning_rate, seed)

    # ---------------- reference-visible state ----------------
    def _get(self, key):
        eng = self._engine
        if eng is not None and self._stale[key]:
            if key == "mean":
                t = self._gather(eng.means_local(), axis=1)
            else:
                t = self._gather(eng.covs_local(), axis=1)
            h = self._host[key]
            if h is not None and h.shape == t.shape and h.dtype == t.dtype and not h.is_inference():
                # refresh in place: a tensor a caller took earlier (X = vi.X_mean)
                # sees the update, as the reference's live attribute does
                # (structured_mf.py:282-287, 332-338)
                h.copy_(t)
                t = h
            self._host[key] = t
            self._ver[key] = t._version
            self._stale[key] = False
        return self._host[key]

    def _set(self, key, value):
        self._host[key] = value
        self._ver[key] = None     # force upload before the next device step
        self._stale[key] = False

    @property
    def X_mean(self):
        return self._get("mean")

    @X_mean.setter
    def X_mean(self, v):
        self._set("mean", v)

    @property
    def X_cov(self):
        return self._get("cov")

    @X_cov.setter
    def X_cov(self, v):
        self._set("cov", v)

    def _host_dirty(self, key):
        h = self._host[key]
        return (not self._stale[key]) and h is not None and (
            self._ver[key] is None or h._version != self._ver[key])

    # ---------------- engine lifecycle ----------------
    def _time_sharded(self) -> bool:
        """Whether this run is (or, before the engine exists, will be) time-sharded;
        decided without a collective."""
        if self._engine is not None:
            return self._halo is not None
        return self._wants_halo()

    def _wants_halo(self) -> bool:
        import torch.distributed as dist
        use = self._distributed
        if use is None:
            use = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        return bool(use)

    def _make_halo(self):
        use = self._distributed
        if not self._wants_halo():
            return None, None
        if use is None:
            use = True
        from ..distributed import TimeShardHalo
        # distributed=True / None: defaults; a dict: TimeShardHalo options (peer_mode)
        halo = TimeShardHalo.create(self.T, **(use if isinstance(use, dict) else {}))
        return halo.shard, halo

    def _ensure_engine(self) -> DeviceEngine:
        if self._engine is None:
            dev = self._device if self._device is not None else default_device()
            shard, halo = self._make_halo()
            self._engine = DeviceEngine(self.model, self._variant, self.lr, self._host["mean"],
                                        self._host["cov"], device=dev, shard=shard, halo=halo,
                                        options=self._engine_options)
            self._ver["mean"] = self._host["mean"]._version
            self._ver["cov"] = self._host["cov"]._version
            self._halo = halo
        else:
            eng = self._engine
            if self._host_dirty("mean"):
                eng.set_means(self._host["mean"])
                self._ver["mean"] = self._host["mean"]._version
            if self._host_dirty("cov"):
                eng.set_covs(self._host["cov"])
                self._ver["cov"] = self._host["cov"]._version
        return self._engine

    def _gather(self, local, axis):
        halo = self._halo
        if halo is None:
            return local.detach().to("cpu").contiguous()
        return halo.gather_time(local, axis)

    # ---------------- hooks ----------------
    def _update_step(self) -> None:
        eng = self._ensure_engine()
        eng.sweep()
        self._stale["mean"] = True
        self._stale["cov"] = True

    # ---------------- fit() hooks: the speculation window ----------------
    def _fit_iteration(self, iteration: int, max_iter: int) -> None:
        # iterations that follow this one unless fit() converges first: that many
        # sweeps may be started ahead (bounded by the engine's spec_depth)
        self._spec_next = max(0, max_iter - 1 - iteration)

    def _fit_end(self, ok: bool = True) -> None:
        self._spec_next = 0
        if self._engine is None:
            return
        halo = self._halo
        if not ok:
            # fit() is raising: the peers may sit in a collective this rank never
            # enters (the ELBO all_reduce, agree()), so no barrier here, and a
            # faulted device must not replace the original exception.  The peer
            # buffers stay mapped until close() at exit.
            try:
                self._engine.discard_speculation()
                if halo is not None:
                    halo.quiesce_local(self._engine)
            except Exception:
                pass
            return
        self._engine.discard_speculation()
        if halo is not None:
            # no rank leaves fit() while a neighbour's dropped sweep may still
            # store into its peer buffers (they are freed at close / exit)
            halo.quiesce(self._engine)

    def _terms(self):
        return self._ensure_engine().terms(speculate=self._spec_next)

    def _compute_elbo(self):
        # the reference returns a 0-d fp32 tensor (python float + fp32 tensors)
        return torch.tensor(self._terms()["elbo"], dtype=torch.float32)

    def _compute_expected_log_likelihood(self):
        return torch.tensor(self._terms()["loglik"], dtype=torch.float32)

    def _compute_log_prior_initial(self):
        return torch.tensor(self._terms()["prior0"], dtype=torch.float32)

    def _compute_log_prior_transitions(self):
        return torch.tensor(self._terms()["trans"], dtype=torch.float32)

    def _compute_entropy(self):
        return torch.tensor(self._terms()["entropy"], dtype=torch.float32)

    def _compute_reconstruction_error(self) -> float:
        return float(self._terms()["recon"])

    def elbo_terms(self) -> dict:
        """fp64 ELBO pieces + MSE of the current state (extension)."""
        return dict(self._terms())

    def local_means(self) -> torch.Tensor:
        """This rank's slices (n, T_local, d) of the current means, on the CPU,
        without a collective (extension; equals X_mean on one process)."""
        return self._ensure_engine().means_local().detach().to("cpu").contiguous()

    def local_covs(self) -> torch.Tensor:
        """This rank's slices (n, T_local, d, d) of the current covariances."""
        return self._ensure_engine().covs_local().detach().to("cpu").contiguous()

    # ---------------- posterior-predictive checks and forecasts (extensions) ----------------
    # The reference's calibration_error / compute_coverage /
    # temporal_prediction_metrics (src/utils/metrics.py:350-518) take predictive
    # intervals of the dyads; these calls produce them from (X_mean, X_cov) on the
    # device (ame_predict), as per-time-step sums or as dense blocks.
    @staticmethod
    def _thresholds(levels):
        """zsq = Phi^-1((1 + p) / 2)^2 (marginal) and csq = -2 ln(1 - p) (joint, 2 dof)."""
        from statistics import NormalDist
        from .. import _lib
        levels = tuple(float(p) for p in levels)
        if len(levels) > _lib.AME_PREDICT_MAX_LEVELS:
            raise ValueError(f"at most {_lib.AME_PREDICT_MAX_LEVELS} levels (got {len(levels)})")
        for p in levels:
            if not 0.0 < p < 1.0:
                raise ValueError(f"coverage level {p} outside (0, 1)")
        nd = NormalDist()
        return (levels, [nd.inv_cdf((1.0 + p) / 2.0) ** 2 for p in levels],
                [-2.0 * math.log1p(-p) for p in levels])

    @staticmethod
    def _check_dict(sums, levels):
        """The public dictionary from per-slice sum rows (S, AME_PREDICT_SUMS), fp64 numpy."""
        s = sums.detach().to("cpu", torch.float64).numpy()
        L = len(levels)
        pairs = s[:, 0].copy()
        cnt = s[:, 9:9 + 3 * L].reshape(s.shape[0], L, 3)
        return {"levels": levels, "pairs": pairs, "log_score": s[:, 1].copy(),
                "mahalanobis": s[:, 2].copy(), "z2": s[:, 3:5].copy(), "mean_var": s[:, 5:7].copy(),
                "sq_err": s[:, 7:9].copy(), "coverage": cnt[:, :, :2] / pairs[:, None, None],
                "joint_coverage": cnt[:, :, 2] / pairs[:, None]}

    def _range(self, sel, size, what):
        """A contiguous index range from None, an int, a range or a slice."""
        if sel is None:
            return 0, size
        if isinstance(sel, int):
            k = sel + size if -size <= sel < 0 else sel
            sel = range(k, k + 1)
        if isinstance(sel, slice):
            sel = range(*sel.indices(size))
        if not isinstance(sel, range) or sel.step != 1 or len(sel) < 1 or sel.start < 0 or sel.stop > size:
            raise ValueError(f"{what} must be a non-empty contiguous range within [0, {size})")
        return sel.start, sel.stop

    def _predict_engine(self):
        eng = self._ensure_engine()
        eng.discard_speculation()
        return eng

    # ---------------- binary networks (extension, model.set_binary) ----------------
    def _binary(self) -> bool:
        return getattr(self.model, "binary", None) is not None

    def _refuse_binary(self, what, why):
        if self._binary():
            raise NotImplementedError(f"{what} is not available on a binary model (model.set_binary): {why}")

    def _binary_check(self, subset) -> dict:
        """predictive_check of a binary model: Bernoulli scores of the ties under
        pi = Phi(E[mu] / sqrt(1 + V0)), the exact marginal P(y = 1) under q."""
        select = self._subset(subset)
        eng = self._predict_engine()
        Yt, Mt, select = eng.mask_args(select)
        s = eng.probit_score(eng.x_a, eng.cov, Yt, Mt=Mt, mask_select=select)
        s = s.detach().to("cpu", torch.float64).numpy()
        pairs = s[:, 0].copy()
        ent = 2.0 * pairs
        return {"pairs": pairs, "log_score": s[:, 1].copy(), "brier": s[:, 2] / ent,
                "accuracy": s[:, 3] / ent, "base_rate": s[:, 4] / ent, "mean_prob": s[:, 5] / ent}

    def predict_proba(self, times, rows=None, cols=None, max_elements=2 ** 27) -> torch.Tensor:
        """P(y_ij = 1) of a binary model for a block, (ni, nj, S, 2) fp32 on the
        CPU in Y's (ij, ji) layout: pi = Phi(E[mu] / sqrt(1 + V0)) from
        predict_dyads' moments of the mean, formed on the device.  The diagonal
        is NaN.  ``times`` is an int or a slice, ``rows`` / ``cols`` contiguous
        ranges or slices."""
        if not self._binary():
            raise ValueError("predict_proba needs a binary model (model.set_binary)")
        eng = self._predict_engine()
        t0, t1 = self._range(times, self.T, "times")
        i0, i1 = self._range(rows, self.n, "rows")
        j0, j1 = self._range(cols, self.n, "cols")
        count = (t1 - t0) * (i1 - i0) * (j1 - j0) * 5
        if count > int(max_elements):
            raise ValueError(f"{count} device floats exceed max_elements={int(max_elements)}; "
                             "ask for fewer times, rows or columns")
        _, dense = eng.predict(eng.x_a[t0:t1], eng.cov[t0:t1], include_noise=False, block=(i0, i1, j0, j1))
        dd = dense.double()
        pi = 0.5 * torch.erfc(-(dd[..., 0:2] / torch.sqrt(1.0 + dd[..., 2:4])) * math.sqrt(0.5))
        return pi.float().permute(1, 2, 0, 3).to("cpu").contiguous()

    # ---------------- ranking the links of a binary network (extension) ----------------
    # ROC / precision-recall curves, AUC and ranked lists from the scores
    # t = E[mu] / sqrt(1 + V0) (pi = Phi(t) is monotone in t), formed tile by
    # tile on the device (ame_probit_rank / ame_probit_select); no probability
    # is moved to the host.  The host finish is ame_amd/links.py.
    def _links_engine(self, what):
        if not self._binary():
            raise ValueError(f"{what} needs a binary model (model.set_binary)")
        if self._time_sharded():
            raise NotImplementedError(f"{what} is not available on a time-sharded run: fit on one process")
        return self._predict_engine()

    @staticmethod
    def _top_links(eng, x, cov, Yt, Mt, select, hist, k, ties, bins, t_max, max_records):
        """top_links' fields for a stack of slices whose histograms are `hist`."""
        import numpy as np
        from .. import links
        bin_min, capacity = links.threshold(hist, k, ties)
        total = int(capacity.sum())
        if total > int(max_records):
            raise ValueError(f"{total} candidate records exceed max_records={int(max_records)}: too many scores "
                             f"share the threshold bin (they saturate the clamped end bin beyond t_max={t_max}, or "
                             f"bins={bins} is too coarse); raise t_max or bins, or ask for fewer slices")
        offset = np.concatenate([[0], np.cumsum(capacity)]).astype(np.int64)
        rec, count = eng.probit_select(x, cov, Yt, bins, t_max, bin_min, offset,
                                       tie_filter=-1 if ties is None else int(ties), Mt=Mt, mask_select=select)
        count = count.to("cpu").numpy()
        if not np.array_equal(count, capacity):   # the two passes bin the same scores: cannot differ
            raise RuntimeError(f"ame_probit_select passed {count.tolist()} entries, the histograms "
                               f"promise {capacity.tolist()}")
        records = rec.to("cpu").numpy().view(links.RECORD)[:total]
        out = links.top_k(records, offset, k)
        out["prob"] = links.phi(out["score"])
        return out

    def link_roc(self, subset=None, bins=1024, t_max=8.0) -> dict:
        """ROC and precision-recall curves and the AUC of the ties of a binary
        model, per time step, from device histograms of the score t = E[mu] /
        sqrt(1 + V0) (pi = Phi(t) is monotone in it; class 1 is a tie).  ``subset``
        as in :meth:`predictive_check` ("held_out": the hidden pairs against
        ``model.Y``, out of sample).  ``bins`` (1 .. 2048) equal bins cover
        [-t_max, t_max); the end bins also hold what lies beyond.  Returns
        ``edges`` (bins + 1,), ``hist`` (T, 2, bins) int64, ``pairs`` /
        ``positives`` / ``negatives`` (T,), ``auc``, ``auc_lo``, ``auc_hi``,
        ``average_precision`` (T,), ``fpr`` / ``tpr`` / ``precision`` / ``recall``
        (T, bins + 1) and the same over all steps under ``pooled``
        (:func:`ame_amd.links.curves`).  The exact AUC of the scores lies in
        [auc_lo, auc_hi]; a step with one class only gives NaN."""
        from .. import links
        eng = self._links_engine("link_roc")
        bins, t_max = links.check_bins(bins, t_max)
        select = self._subset(subset)
        Yt, Mt, select = eng.mask_args(select)
        hist = eng.probit_rank(eng.x_a, eng.cov, Yt, bins, t_max, Mt=Mt, mask_select=select)
        return links.roc(hist.to("cpu").numpy(), bins, t_max)

    def top_links(self, k=100, subset=None, ties=None, bins=1024, t_max=8.0, max_records=2 ** 24) -> dict:
        """The k most probable directed links of every time step of a binary
        model, best first by (-score, sender, receiver): ``sender``, ``receiver``,
        ``tie`` (T, k) int64, ``score`` (T, k) fp64 = t and ``prob`` = Phi(score);
        a step with fewer than k candidates is padded with -1 / NaN.  ``ties=0``
        ranks the absent links only (recommendation on an observed network),
        ``ties=1`` the present ones.  The device keeps the entries at or above
        the histogram bin that holds the k-th score; more than ``max_records``
        of them is a ValueError (many scores saturate the clamped top bin: raise
        ``t_max`` or ``bins``)."""
        from .. import links
        eng = self._links_engine("top_links")
        bins, t_max = links.check_bins(bins, t_max)
        if isinstance(k, bool) or int(k) != k or int(k) < 1:
            raise ValueError(f"k must be an integer >= 1 (got {k!r})")
        if ties not in (None, 0, 1):
            raise ValueError(f"ties must be None, 0 or 1 (got {ties!r})")
        select = self._subset(subset)
        Yt, Mt, select = eng.mask_args(select)
        hist = eng.probit_rank(eng.x_a, eng.cov, Yt, bins, t_max, Mt=Mt, mask_select=select)
        return self._top_links(eng, eng.x_a, eng.cov, Yt, Mt, select, hist.to("cpu").numpy(), int(k), ties,
                               bins, t_max, max_records)

    def forecast_links(self, B_future, bins=1024, t_max=8.0, k=0, max_records=2 ** 24) -> dict:
        """:meth:`link_roc` of held-out steps: ``B_future`` (n, n, h) bool / uint8
        ties scored against the h-step forecast of the states (:meth:`forecast`);
        the same dictionary with h rows, every future pair observed, plus
        :meth:`top_links`' fields (both classes) when k > 0."""
        from .. import links
        eng = self._links_engine("forecast_links")
        bins, t_max = links.check_bins(bins, t_max)
        if isinstance(k, bool) or int(k) != k or int(k) < 0:
            raise ValueError(f"k must be an integer >= 0 (got {k!r})")
        B = torch.as_tensor(B_future)
        if B.dim() != 3 or tuple(B.shape[:2]) != (self.n, self.n) or B.shape[2] < 1:
            raise ValueError(f"B_future has shape {tuple(B.shape)}, expected ({self.n}, {self.n}, h)")
        if B.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"B_future has dtype {B.dtype}, expected bool or uint8")
        # the 0 / 1 network as set_binary builds model.Y: no self ties, entry (ij, ji)
        Bc = (B.to("cpu") != 0) & ~torch.eye(self.n, dtype=torch.bool).unsqueeze(2)
        Y01 = torch.stack([Bc, Bc.transpose(0, 1)], dim=-1).float()
        eng, (m, S) = self._forecast_states(int(B.shape[2]))
        Yt = eng.pack_future(Y01)
        hist = eng.probit_rank(m, S, Yt, bins, t_max).to("cpu").numpy()
        out = links.roc(hist, bins, t_max)
        if int(k) > 0:
            out.update(self._top_links(eng, m, S, Yt, None, 0, hist, int(k), None, bins, t_max, max_records))
        return out

    # ---------------- exact smoothing across time (extension) ----------------
    def smooth(self, partners=None) -> SmoothResult:
        """Each node's exact Gaussian posterior over its whole trajectory given
        the current means of the other nodes (ame_smooth): smoothed means, the
        time-marginal covariances (never smaller than the fit's mean-field
        blocks) and the lag-one cross-covariances.  Does not modify this object.
        Not available on a time-sharded run.
        With hidden dyads (model.set_missing) the default call is refused;
        ``partners="observed"`` conditions each node on the dyads it has observed
        only, so its covariances widen with the number of hidden partners."""
        if partners not in (None, "observed"):
            raise ValueError(f'partners must be None or "observed" (got {partners!r})')
        self._refuse_binary("smooth / smoothed=", "the smoother conditions on Gaussian observations")
        if self._time_sharded():
            raise NotImplementedError("smooth is not available on a time-sharded run: the forward "
                                      "pass would have to carry (J_t^-1, g_t) across ranks")
        masked = getattr(self.model, "missing", None) is not None
        if partners == "observed" and not masked:
            raise ValueError('partners="observed" / smoothed="observed" need a mask (model.set_missing)')
        if masked and partners is None:
            raise NotImplementedError("smooth() / smoothed=True over all partners are not available "
                                      "with missing dyads: use smooth(partners=\"observed\") / "
                                      "smoothed=\"observed\"")
        eng = self._predict_engine()
        return SmoothResult(*eng.smooth(observed=partners == "observed"))

    @staticmethod
    def _partners(smoothed):
        """The ``partners`` of :meth:`smooth` a ``smoothed`` argument asks for:
        "observed" by name, None for any other true value."""
        if isinstance(smoothed, str):
            if smoothed != "observed":
                raise ValueError(f'smoothed must be False, True or "observed" (got {smoothed!r})')
            return "observed"
        return None

    def _state(self, smoothed):
        """(engine, means, covariances, smoothing result or None) the extension
        calls work from: the fit's state, or its smoothed counterpart
        (smoothed=True, or "observed" with hidden dyads)."""
        if smoothed:
            sm = self.smooth(partners=self._partners(smoothed))
            return self._engine, sm.d_mean, sm.d_cov, sm
        eng = self._predict_engine()
        return eng, eng.x_a, eng.cov, None

    _SUBSETS = {"observed": 1, "held_out": 2}   # AME_MASK_OBSERVED / AME_MASK_HIDDEN

    def _subset(self, subset):
        """mask_select of a predictive_check subset: "observed" by default with a
        mask (model.set_missing); any subset without one is a ValueError."""
        if getattr(self.model, "missing", None) is None:
            if subset is not None:
                raise ValueError(f"subset={subset!r} needs a mask (model.set_missing)")
            return 0
        if subset is None:
            subset = "observed"
        if subset not in self._SUBSETS:
            raise ValueError(f"subset must be one of {sorted(self._SUBSETS)} (got {subset!r})")
        return self._SUBSETS[subset]

    def predictive_check(self, levels=(0.5, 0.9, 0.95), include_noise=True, smoothed=False,
                         subset=None) -> dict:
        """Score the observed network against the posterior-predictive moments of
        every dyad, in-sample.  fp64 arrays of length T: ``pairs``, ``log_score``
        (sum of log N(y_ij; E mu_ij, Sigma_ij) over pairs i < j), ``mahalanobis``,
        ``z2`` (T, 2), ``mean_var`` (T, 2), ``sq_err`` (T, 2), ``coverage``
        (T, L, 2) and ``joint_coverage`` (T, L) as fractions, and ``levels``.
        include_noise=False scores against the credible region of the mean.
        smoothed=True scores the smoothed means and covariances (:meth:`smooth`)
        instead of the fit's (with hidden dyads: smoothed="observed", the
        smoother over each node's observed partners, whose covariances widen with
        the number of hidden partners).  Time-sharded: a collective, every rank
        returns all T steps.  With hidden dyads (model.set_missing) ``subset`` chooses the
        pairs: "observed" (the default) scores the pairs the fit has seen,
        "held_out" the hidden ones against ``model.Y``, out of sample; ``pairs``
        counts the chosen ones.
        On a binary model (model.set_binary) the scores are Bernoulli: fp64 arrays
        of length T ``pairs``, ``log_score`` (sum over both entries of the chosen
        pairs of log P(y_ij)), and per entry ``brier``, ``accuracy`` (share with
        (pi > 1/2) == y), ``base_rate`` (share of ties) and ``mean_prob``, with
        pi = Phi(E[mu] / sqrt(1 + V0)); levels / include_noise are not used."""
        if self._binary():
            if smoothed:
                self._refuse_binary("smoothed=", "the smoother conditions on Gaussian observations")
            return self._binary_check(subset)
        levels, zsq, csq = self._thresholds(levels)
        select = self._subset(subset)
        eng, x, cov, _ = self._state(smoothed)
        Yt, Mt, select = eng.mask_args(select)
        sums, _ = eng.predict(x, cov, Yt=Yt, include_noise=include_noise,
                              zsq=zsq, csq=csq, Mt=Mt, mask_select=select)
        if self._halo is not None:
            sums = self._halo.gather_time(sums.unsqueeze(0), 1)[0]
        return self._check_dict(sums, levels)

    def _dense(self, eng, x, cov, rows, cols, include_noise, max_elements):
        i0, i1 = self._range(rows, self.n, "rows")
        j0, j1 = self._range(cols, self.n, "cols")
        count = int(x.shape[0]) * (i1 - i0) * (j1 - j0) * 5
        if count > int(max_elements):
            raise ValueError(f"{count} output floats exceed max_elements={int(max_elements)}; "
                             "ask for fewer times, rows or columns")
        _, dense = eng.predict(x, cov, include_noise=include_noise, block=(i0, i1, j0, j1))
        dense = dense.permute(1, 2, 0, 3).to("cpu")
        return dense[..., :2].contiguous(), dense[..., 2:].contiguous()

    def predict_dyads(self, times, rows=None, cols=None, include_noise=True, max_elements=2 ** 27,
                      smoothed=False):
        """Dense predictive moments ``(mean, second)`` on the CPU: (ni, nj, S, 2)
        = E[mu_ij] (plus sum_k beta_k w_k,ij when the model has covariates) and (ni, nj, S, 3) = Var of entry 0, Var of entry 1 and their
        covariance (with model.R added when include_noise).  ``times`` is an int
        or a slice, ``rows`` / ``cols`` contiguous ranges or slices.  The diagonal
        holds compute_mean's means and NaN second moments.  smoothed=True: of the
        smoothed state (:meth:`smooth`)."""
        eng, x, cov, _ = self._state(smoothed)
        if self._halo is not None:
            raise NotImplementedError("predict_dyads is not available on a time-sharded run: "
                                      "score with predictive_check, or fit on one process")
        t0, t1 = self._range(times, self.T, "times")
        mean, second = self._dense(eng, x[t0:t1], cov[t0:t1], rows, cols, include_noise, max_elements)
        if getattr(self.model, "W", None) is not None:
            mean = mean + self._covariate_block(self.model.W[:, :, :, t0:t1], rows, cols)
        return mean, second

    def _covariate_block(self, W, rows, cols):
        """sum_k beta_k W_k of the block rows x cols, (ni, nj, S, 2) fp32 on the CPU."""
        i0, i1 = self._range(rows, self.n, "rows")
        j0, j1 = self._range(cols, self.n, "cols")
        return self.model.covariate_effect(W[:, i0:i1, j0:j1].to("cpu"))

    def _future_covariates(self, W_future, h):
        """The (p, n, n, h, 2) covariates of held-out steps: required exactly when
        the model has covariates (None otherwise)."""
        W = getattr(self.model, "W", None)
        if W is None:
            if W_future is not None:
                raise ValueError("W_future given but the model has no covariates")
            return None
        if W_future is None:
            raise ValueError("the model has covariates: W_future (p, n, n, h, 2) is required")
        Wf = torch.as_tensor(W_future, dtype=torch.float32)
        if Wf.dim() == 4:
            Wf = Wf.unsqueeze(0)
        want = (int(W.shape[0]), self.n, self.n, int(h), 2)
        if tuple(Wf.shape) != want:
            raise ValueError(f"W_future has shape {tuple(Wf.shape)}, expected {want}")
        return Wf

    def _forecast_states(self, n_steps, smoothed=False):
        if smoothed:   # the smoothed last slice is the filtered one
            eng, x, cov, _ = self._state(smoothed)
            return eng, eng.forecast_states(x[-1], cov[-1], n_steps)
        eng = self._predict_engine()
        if self._halo is None:
            m, S = eng.x_a[-1], eng.cov[-1]
        else:   # collective getters: every rank reads the last slice and computes the same
            m, S = self.X_mean[:, -1], self.X_cov[:, -1]
        return eng, eng.forecast_states(m, S, n_steps)

    def forecast(self, n_steps: int = 1, smoothed=False):
        """h-step forecast of the states from the last fitted slice, ``(X_pred
        (n, h, d), S_pred (n, h, d, d))`` on the CPU: m_k = Phi m_{k-1}, S_k = Phi
        S_{k-1} Phi' + Q (the means are naive_mf.py:386-396's predict_forward).
        smoothed=True starts from the smoothed last slice (:meth:`smooth`), which
        is the filtered one."""
        _, (m, S) = self._forecast_states(n_steps, smoothed)
        return m.permute(1, 0, 2).to("cpu").contiguous(), S.permute(1, 0, 2, 3).to("cpu").contiguous()

    def forecast_check(self, Y_future, levels=(0.5, 0.9, 0.95), include_noise=True,
                       smoothed=False, W_future=None, missing_future=None) -> dict:
        """predictive_check of held-out steps: ``Y_future`` (n, n, h, 2) scored
        against the h-step forecast; the same dictionary, of length h.  A model
        with covariates needs theirs for those steps, ``W_future`` (p, n, n, h,
        2): the residual Y_future - sum_k beta_k W_future[k] is scored.
        ``missing_future`` (n, n, h), bool or uint8 and symmetric as in
        model.set_missing: only the observed future pairs are scored."""
        levels, zsq, csq = self._thresholds(levels)
        self._refuse_binary("forecast_check", "it scores Gaussian observations; forecast() and "
                            "predict_proba() give the states and the in-sample probabilities")
        Y_future = torch.as_tensor(Y_future)
        Wf = self._future_covariates(W_future, Y_future.shape[2] if Y_future.dim() == 4 else 1)
        if Wf is not None:
            Y_future = Y_future.to("cpu", torch.float32) - self.model.covariate_effect(Wf)
        eng, (m, S) = self._forecast_states(int(Y_future.shape[2]) if Y_future.dim() == 4 else 1,
                                            smoothed)
        Yt = eng.pack_future(Y_future)
        Mt, select = None, 0
        if missing_future is not None:
            mf = torch.as_tensor(missing_future)
            if mf.dim() != 3 or int(mf.shape[2]) != int(Yt.shape[0]):
                raise ValueError(f"missing_future has shape {tuple(mf.shape)}, expected "
                                 f"({self.n}, {self.n}, {int(Yt.shape[0])})")
            Mt, _, _ = eng.pack_mask(mf, "missing_future")
            select = self._SUBSETS["observed"]
        sums, _ = eng.predict(m, S, Yt=Yt, include_noise=include_noise, zsq=zsq, csq=csq, Mt=Mt,
                              mask_select=select)
        return self._check_dict(sums, levels)

    # ---------------- residual diagnostics of a Gaussian fit (extension) ----------------
    # predictive_check reduces a fit to sums per time step; these calls keep the
    # node and the pair: per-node sums of the dyad scores, the distribution of the
    # Mahalanobis distance m2 = e' Sigma^-1 e and the k most surprising pairs, all
    # formed tile by tile on the device (ame_resid_nodes / ame_resid_hist /
    # ame_resid_select); no dyad moment is moved to the host.  The host finish is
    # ame_amd/residuals.py.
    def _resid_refuse(self, what):
        self._refuse_binary(what, "it scores Gaussian observations; link_roc and top_links rank the "
                            "links of a binary model")
        if self._time_sharded():
            raise NotImplementedError(f"{what} is not available on a time-sharded run: fit on one process")

    def _resid_state(self, what, subset, smoothed):
        """(engine, means, covariances, Yt, Mt, mask_select) of the in-sample calls,
        chosen as predictive_check chooses them."""
        self._resid_refuse(what)
        select = self._subset(subset)
        eng, x, cov, _ = self._state(smoothed)
        Yt, Mt, select = eng.mask_args(select)
        return eng, x, cov, Yt, Mt, select

    @staticmethod
    def _check_k(k, least=1):
        if isinstance(k, bool) or int(k) != k or int(k) < least:
            raise ValueError(f"k must be an integer >= {least} (got {k!r})")
        return int(k)

    @staticmethod
    def _top_residuals(eng, x, cov, Yt, Mt, select, hist, k, bins, m2_max, include_noise, max_records):
        """top_residuals' fields for a stack of slices whose histograms are `hist`."""
        import numpy as np
        from .. import residuals
        bin_min, capacity = residuals.threshold(hist, k)
        total = int(capacity.sum())
        if total > int(max_records):
            raise ValueError(f"{total} candidate records exceed max_records={int(max_records)}: too many pairs "
                             f"share the threshold bin (they saturate the open last bin beyond m2_max={m2_max}, "
                             f"or bins={bins} is too coarse); raise m2_max or bins, or ask for fewer slices")
        offset = np.concatenate([[0], np.cumsum(capacity)]).astype(np.int64)
        rec, count = eng.resid_select(x, cov, Yt, bins, m2_max, bin_min, offset, include_noise=include_noise,
                                      Mt=Mt, mask_select=select)
        count = count.to("cpu").numpy()
        if not np.array_equal(count, capacity):   # the two passes bin the same m2: cannot differ
            raise RuntimeError(f"ame_resid_select passed {count.tolist()} pairs, the histograms "
                               f"promise {capacity.tolist()}")
        records = rec.to("cpu").numpy().view(residuals.RECORD)[:total]
        return residuals.top_k(records, offset, k)

    def node_check(self, include_noise=True, smoothed=False, subset=None) -> dict:
        """:meth:`predictive_check` per node: for every time step and node the
        sums over the chosen pairs that contain it.  ``pairs`` (T, n) int64;
        ``log_score`` and ``mahalanobis`` (T, n), the pair's log N(y; E mu,
        Sigma) and m2; ``z2``, ``resid`` (the signed bias) and ``sq_err``
        (T, n, 2), last axis [the entries the node sends, the entries it
        receives]; ``mean_mahalanobis`` = mahalanobis / pairs (2 under the
        model; NaN where pairs == 0).  ``include_noise``, ``smoothed`` and
        ``subset`` as in :meth:`predictive_check`; with covariates the residual
        network the fit reads is scored.  Summed over the nodes every field is
        twice predictive_check's.  Not available on a binary model or a
        time-sharded run.  Does not modify this object."""
        from .. import residuals
        eng, x, cov, Yt, Mt, select = self._resid_state("node_check", subset, smoothed)
        node = eng.resid_nodes(x, cov, Yt, include_noise=include_noise, Mt=Mt, mask_select=select)
        return residuals.node_dict(node.to("cpu").numpy())

    def residual_histogram(self, bins=1024, m2_max=64.0, subset=None, smoothed=False,
                           include_noise=True) -> dict:
        """The distribution of the pairs' Mahalanobis distance m2 per time step:
        ``edges`` (bins + 1,), ``hist`` (T, bins) int64, ``expected`` (T, bins)
        fp64, the counts of a chi-square with 2 degrees of freedom (what a
        calibrated fit gives), and ``pairs`` (T,).  ``bins`` (1 .. 2048) equal
        bins cover [0, m2_max); the last one also holds what lies beyond and any
        NaN.  The other arguments as in :meth:`node_check`."""
        from .. import residuals
        bins, m2_max = residuals.check_bins(bins, m2_max)
        eng, x, cov, Yt, Mt, select = self._resid_state("residual_histogram", subset, smoothed)
        hist = eng.resid_hist(x, cov, Yt, bins, m2_max, include_noise=include_noise, Mt=Mt, mask_select=select)
        return residuals.histogram(hist.to("cpu").numpy(), bins, m2_max)

    def top_residuals(self, k=100, bins=1024, m2_max=64.0, subset=None, smoothed=False, include_noise=True,
                      max_records=2 ** 24) -> dict:
        """The k most surprising pairs of every time step, most surprising first
        by (NaN first, -m2, i, j): ``i``, ``j`` (T, k) int64 with i < j, ``m2``
        and ``p_value`` = exp(-m2 / 2) (T, k), ``z`` (T, k, 2) the signed
        standardised residuals of the entries i -> j and j -> i; a step with
        fewer than k pairs is padded with -1 / NaN.  The device keeps the pairs
        at or above the histogram bin that holds the k-th m2; more than
        ``max_records`` of them is a ValueError (many pairs lie beyond
        ``m2_max``: raise ``m2_max`` or ``bins``).  The other arguments as in
        :meth:`node_check`."""
        from .. import residuals
        bins, m2_max = residuals.check_bins(bins, m2_max)
        k = self._check_k(k)
        eng, x, cov, Yt, Mt, select = self._resid_state("top_residuals", subset, smoothed)
        hist = eng.resid_hist(x, cov, Yt, bins, m2_max, include_noise=include_noise, Mt=Mt, mask_select=select)
        return self._top_residuals(eng, x, cov, Yt, Mt, select, hist.to("cpu").numpy(), k, bins, m2_max,
                                   include_noise, max_records)

    def forecast_residuals(self, Y_future, k=100, W_future=None, missing_future=None, bins=1024, m2_max=64.0,
                           smoothed=False, include_noise=True, max_records=2 ** 24) -> dict:
        """:meth:`node_check`, :meth:`residual_histogram` and :meth:`top_residuals`
        of held-out steps: ``Y_future`` (n, n, h, 2) against the h-step forecast,
        packed and (``W_future``, ``missing_future``) prepared as
        :meth:`forecast_check` does.  Returns ``{"nodes": ..., "histogram": ...,
        "top": ...}`` with h rows each; ``top`` is None when k == 0."""
        from .. import residuals
        bins, m2_max = residuals.check_bins(bins, m2_max)
        k = self._check_k(k, least=0)
        self._resid_refuse("forecast_residuals")
        Y_future = torch.as_tensor(Y_future)
        if Y_future.dim() != 4 or tuple(Y_future.shape[:2]) != (self.n, self.n) or Y_future.shape[3] != 2 \
                or Y_future.shape[2] < 1:
            raise ValueError(f"Y_future has shape {tuple(Y_future.shape)}, expected ({self.n}, {self.n}, h, 2)")
        Wf = self._future_covariates(W_future, Y_future.shape[2] if Y_future.dim() == 4 else 1)
        if Wf is not None:
            Y_future = Y_future.to("cpu", torch.float32) - self.model.covariate_effect(Wf)
        eng, (m, S) = self._forecast_states(int(Y_future.shape[2]) if Y_future.dim() == 4 else 1, smoothed)
        Yt = eng.pack_future(Y_future)
        Mt, select = None, 0
        if missing_future is not None:
            mf = torch.as_tensor(missing_future)
            if mf.dim() != 3 or int(mf.shape[2]) != int(Yt.shape[0]):
                raise ValueError(f"missing_future has shape {tuple(mf.shape)}, expected "
                                 f"({self.n}, {self.n}, {int(Yt.shape[0])})")
            Mt, _, _ = eng.pack_mask(mf, "missing_future")
            select = self._SUBSETS["observed"]
        kw = dict(include_noise=include_noise, Mt=Mt, mask_select=select)
        node = eng.resid_nodes(m, S, Yt, **kw)
        hist = eng.resid_hist(m, S, Yt, bins, m2_max, **kw).to("cpu").numpy()
        top = self._top_residuals(eng, m, S, Yt, Mt, select, hist, k, bins, m2_max, include_noise,
                                  max_records) if k else None
        return {"nodes": residuals.node_dict(node.to("cpu").numpy()),
                "histogram": residuals.histogram(hist, bins, m2_max), "top": top}

    def forecast_dyads(self, n_steps: int = 1, rows=None, cols=None, include_noise=True,
                       max_elements=2 ** 27, smoothed=False, W_future=None):
        """predict_dyads of the h-step forecast: (ni, nj, h, 2) and (ni, nj, h, 3).
        A model with covariates needs ``W_future`` (p, n, n, h, 2); sum_k beta_k
        W_future[k] of the block is added to the means."""
        Wf = self._future_covariates(W_future, n_steps)
        eng, (m, S) = self._forecast_states(n_steps, smoothed)
        mean, second = self._dense(eng, m, S, rows, cols, include_noise, max_elements)
        if Wf is not None:
            mean = mean + self._covariate_block(Wf, rows, cols)
        return mean, second

    # ---------------- variational EM: learn Phi, Q, R, Sigma, Psi (extension) ----------------
    # The reference never estimates the model parameters.  The E-step is the
    # sweep; the M-step is closed-form (ame_amd/mstep.py) given sufficient
    # statistics of q that the device computes (ame_mstep_stats).  q is
    # mean-field across time, so posterior variances are underestimated and the
    # estimates of Q and R are biased; at small n the Phi of the multiplicative
    # block is poorly identified (U V' is rotation-invariant): update=("R", "Q")
    # or phi_structure="scalar" restrict the step.
    def m_step_statistics(self, smoothed=False) -> dict:
        """fp64 CPU tensors ``A0, A11, A00, A10`` (d, d), ``Rss`` (2, 2) and the
        pair count ``pairs`` of the current q.  Time-sharded: a collective; every
        rank adds all T slices in time order and returns the same bits.
        With hidden dyads (model.set_missing) ``Rss`` and ``pairs`` run over the
        observed pairs only, so the M-step's R = Rss / pairs is theirs, and
        ``hidden_pairs`` counts the rest.
        smoothed=True: the statistics of the smoothed posterior (:meth:`smooth`):
        its means and marginals in place of the fit's, and its lag-one
        cross-covariances added into A10."""
        from .. import mstep
        self._refuse_binary("fit_em / m_step", "no M-step is defined for probit data (rho is fixed)")
        if smoothed:
            eng, x, cov, sm = self._state(smoothed)
            state, dyad = eng.mstep_stats(x, cov)
            stats = mstep.combine(state, dyad, cross=sm.d_lag_sum)
            if eng.p:
                stats.update(mstep.combine_covar(*eng.covar_stats(x), eng.beta))
            if eng.masked:
                stats["hidden_pairs"] = float(sum(eng.hidden_pairs))
            return stats
        eng = self._predict_engine()
        state, dyad = eng.mstep_stats()
        if self._halo is not None:
            state = self._halo.gather_time(state.unsqueeze(0), 1)[0]
            dyad = self._halo.gather_time(dyad.unsqueeze(0), 1)[0]
        stats = mstep.combine(state, dyad)
        if eng.p:   # covariates: G, H and the beta the residual Yt was taken at
            stats.update(mstep.combine_covar(*eng.covar_stats(), eng.beta))
        if eng.masked:   # Rss and pairs run over the observed pairs only
            stats["hidden_pairs"] = float(sum(eng.hidden_pairs))
        return stats

    def _model_params64(self) -> dict:
        m = self.model
        out = {k: getattr(m, k).detach().to("cpu", torch.float64).clone()
               for k in ("Phi", "Q", "R", "Sigma", "Psi")}
        if getattr(m, "W", None) is not None:
            out["beta"] = m.beta.detach().to("cpu", torch.float64).clone()
        return out

    def m_step(self, update=("Phi", "Q", "R", "Sigma0"), phi_structure="full", apply=True,
               smoothed=False) -> dict:
        """One closed-form M-step on the current q.  Returns the new fp64 ``Phi,
        Q, R, Sigma, Psi`` (those not in ``update`` unchanged) with
        ``objective_before`` / ``objective_after``: the expected complete-data
        log-likelihood F (ame_amd/mstep.py) at the model's parameters and at the
        returned ones, and ``objective_scale``, the sum of the |terms| of F (its
        evaluation error is a small multiple of 2^-52 of that).  ``apply`` writes them to the model as fp32 (``R_inv``
        with ``R``) and rebuilds the engine's constants from those attributes,
        as a fresh VI on the updated model would.  A non-finite or
        non-positive-definite result raises ValueError and applies nothing.
        With covariates (model.set_covariates) ``update`` may name "beta": the
        regression coefficients get their closed-form step first and R is then
        taken at the new beta; the statistics carry ``G``, ``H`` and the ``beta``
        they were taken at, the result ``beta``.  Applying writes ``model.beta``
        (fp32) and rebuilds the engine's residual network.  A singular system
        for beta raises ValueError and applies nothing."""
        from .. import mstep
        self._refuse_binary("fit_em / m_step", "no M-step is defined for probit data (rho is fixed)")
        update = tuple(update)
        if "beta" in update and getattr(self.model, "W", None) is None:
            raise ValueError('update has "beta" but the model has no covariates (set_covariates)')
        stats = self.m_step_statistics(smoothed=smoothed)
        old = self._model_params64()
        new = mstep.solve(stats, old, self.n, self.T, update, phi_structure)
        new32 = {k: v.to(torch.float32) for k, v in new.items()}
        mstep.validate(new)
        mstep.validate({k: v.double() for k, v in new32.items()})
        out = dict(new)
        out["objective_before"] = mstep.objective(stats, old, self.n, self.T)
        out["objective_after"] = mstep.objective(stats, new, self.n, self.T)
        out["objective_scale"] = mstep.objective_scale(stats, new, self.n, self.T)
        if apply:
            m = self.model
            changed = {"Phi": ("Phi",), "Q": ("Q",), "R": ("R",), "Sigma0": ("Sigma", "Psi"),
                       "beta": ("beta",)}
            for u in update:
                for k in changed[u]:
                    setattr(m, k, new32[k])
            if "R" in update:
                m.R_inv = torch.linalg.inv(m.R)
            self._ensure_engine().set_constants(m)
            if "beta" in update:   # the residual network every kernel reads, at the new beta
                self._engine.set_beta(m.beta)
        return out

    def fit_em(self, n_rounds: int = 10, inner_iter: int = 10,
               update=("Phi", "Q", "R", "Sigma0"), phi_structure="full",
               tolerance: float = 1e-4, verbose: bool = True, smoothed=False):
        """Variational EM: ``n_rounds`` rounds of ``fit(max_iter=inner_iter)``
        followed by ``m_step(update, phi_structure)``.  ``history["em"]`` gains
        one m_step dictionary per round; ``history["elbo"]`` and
        ``history["reconstruction_error"]`` keep growing as repeated fit() calls
        make them.  smoothed=True: every M-step uses the statistics of the
        smoothed posterior; F and the closed forms are the same (F is linear in
        the statistics)."""
        self._refuse_binary("fit_em / m_step", "no M-step is defined for probit data (rho is fixed)")
        if smoothed and self._time_sharded():
            raise NotImplementedError("smoothed=True is not available on a time-sharded run")
        masked = getattr(self.model, "missing", None) is not None
        if smoothed and self._partners(smoothed) is None and masked:
            raise NotImplementedError("smoothed=True is not available with missing dyads: use "
                                      "smoothed=\"observed\"")
        if smoothed and self._partners(smoothed) == "observed" and not masked:
            raise ValueError('smoothed="observed" needs a mask (model.set_missing)')
        em = self.history.setdefault("em", [])
        for k in range(int(n_rounds)):
            self.fit(max_iter=inner_iter, tolerance=tolerance, verbose=False)
            res = self.m_step(update=update, phi_structure=phi_structure, apply=True,
                              smoothed=smoothed)
            em.append(res)
            if verbose:
                print(f"EM round {k:3d} | F: {res['objective_before']:.4f} -> "
                      f"{res['objective_after']:.4f} | ELBO: {float(self.history['elbo'][-1]):10.2f}")
        return self.history

    # ---------------- goodness of fit by network statistics (extension) ----------------
    def _gof_engine(self):
        """The engine, after the refusals of the goodness-of-fit calls (raised
        before anything is launched for them)."""
        self._refuse_binary("gof / network_statistics", "the simulated networks would be Gaussian")
        if self._time_sharded():
            raise NotImplementedError("network statistics are not available on a time-sharded run: "
                                      "every rank would simulate and reduce its own slices only")
        if getattr(self.model, "missing", None) is not None:
            raise NotImplementedError("network statistics are not available with missing dyads: a hidden "
                                      "pair has no observed value (the complete-case statistics are not "
                                      "implemented)")
        eng = self._predict_engine()
        if not eng.swap_consistent:
            raise ValueError("network statistics need a swap-consistent network: Y[j, i, t] must be "
                             "Y[i, j, t] with its two entries exchanged (the kernels read y_ji from row i)")
        return eng

    @staticmethod
    def _stat_dict(raw, n):
        from .. import gof as G
        return G.combine(raw["node"].cpu().numpy(), raw["slice"].cpu().numpy(), raw["tri"].cpu().numpy(), n)

    def network_statistics(self) -> dict:
        """The five network statistics of the GOF panel of ``amen``, per slice, of
        the network the fit reads: fp64 (T,) arrays ``sd_rowmean``,
        ``sd_colmean``, ``dyad_dep``, ``cycle_dep``, ``trans_dep``, plus ``mean``
        and ``sd`` (:mod:`ame_amd.gof`).  With covariates that network is the
        residual Y - sum_k beta_k W_k at the current beta, so the statistics are
        the residual's.  Needs a fully observed, swap-consistent network; not
        available on a time-sharded run.  Does not modify this object."""
        eng = self._gof_engine()
        return self._stat_dict(eng.net_statistics(eng.Yt), self.n)

    @staticmethod
    def _factor(cov):
        """Lower Cholesky factors of [T][n][d][d] covariances (symmetrised), fp32
        on the covariances' device: factored there when this torch build can,
        otherwise on the CPU in fp64."""
        c = 0.5 * (cov + cov.transpose(-1, -2))
        try:
            return torch.linalg.cholesky(c)
        except RuntimeError:
            return torch.linalg.cholesky(c.to("cpu", torch.float64)).to(cov.device, torch.float32)

    def _state_draws(self, n_sim, seed, smoothed):
        """Generator of n_sim draws [T][n][d] (device, fp32) from q: every (node,
        slice) an independent N(m, S).  The statistics are per slice and q
        factorises over nodes, so the time marginals are all they need."""
        eng, x, cov, _ = self._state(smoothed)
        L = self._factor(cov)
        g = torch.Generator(device=x.device)
        g.manual_seed(int(seed))
        for _ in range(int(n_sim)):
            z = torch.randn(x.shape, generator=g, device=x.device, dtype=torch.float32)
            yield (x + torch.einsum("tnij,tnj->tni", L, z)).contiguous()

    def sample_states(self, n_sim: int, seed: int = 0, smoothed=False) -> torch.Tensor:
        """``n_sim`` draws (n_sim, n, T, d) of the states from q (CPU fp32): every
        (node, slice) is an independent N(m, S) from a Cholesky factor of its
        covariance block, drawn with a seeded generator (the same seed gives the
        same draws).  smoothed=True draws from the smoothed marginals
        (:meth:`smooth`); the lag-one correlations are not reproduced, which no
        per-slice statistic can see."""
        if self._time_sharded():
            raise NotImplementedError("sample_states is not available on a time-sharded run")
        draws = [xk.permute(1, 0, 2).to("cpu") for xk in self._state_draws(n_sim, seed, smoothed)]
        return torch.stack(draws).contiguous()

    def gof(self, n_sim: int = 100, seed: int = 0, smoothed=False, states=None,
            include_noise: bool = True) -> dict:
        """Goodness of fit: the five network statistics (:meth:`network_statistics`)
        of the observed network against those of ``n_sim`` networks simulated
        from the fit, y_ij = mu_ij(x) + eps with x drawn from q
        (:meth:`sample_states`; smoothed=True from the smoothed marginals) and
        eps ~ N(0, sym(R)) (include_noise=False: mu alone).  Returns ``names``,
        ``observed`` (T, 5), ``simulated`` (n_sim, T, 5) and ``quantile`` (T, 5),
        the share of simulations at or below the observed value.  ``states``
        (n_sim, n, T, d) replaces the internal draws; ``seed`` also keys the
        noise (Philox counter: pair, slice, simulation).  With covariates the
        observed network is the residual and the simulated ones are residual
        networks too (mu + eps, no beta W).  Needs a fully observed,
        swap-consistent network; not available on a time-sharded run.  Does not
        modify this object."""
        import numpy as np
        from .. import gof as G
        eng = self._gof_engine()
        if states is not None:
            states = torch.as_tensor(states)
            if states.dim() != 4 or tuple(states.shape[1:]) != (self.n, self.T, self.d):
                raise ValueError(f"states have shape {tuple(states.shape)}, expected "
                                 f"(n_sim, {self.n}, {self.T}, {self.d})")
            n_sim = int(states.shape[0])
            draws = (states[k].detach().float().permute(1, 0, 2).to(eng.dev).contiguous()
                     for k in range(n_sim))
        else:
            draws = self._state_draws(n_sim, seed, smoothed)
        chol = (0.0, 0.0, 0.0)
        if include_noise:
            R = self.model.R.detach().to("cpu", torch.float64)
            Lr = torch.linalg.cholesky(0.5 * (R + R.T))
            chol = (float(Lr[0, 0]), float(Lr[1, 0]), float(Lr[1, 1]))
        observed = G.stack(self._stat_dict(eng.net_statistics(eng.Yt), self.n))
        sims = [G.stack(self._stat_dict(eng.simulated_statistics(xk, chol, seed, k), self.n))
                for k, xk in enumerate(draws)]
        simulated = np.stack(sims) if sims else np.zeros((0,) + observed.shape)
        return {"names": G.NAMES, "observed": observed, "simulated": simulated,
                "quantile": G.quantile(observed, simulated) if sims else np.full(observed.shape, np.nan)}

    def get_variational_means(self) -> torch.Tensor:
        return self.X_mean

    def get_variational_covariances(self) -> torch.Tensor:
        return self.X_cov

    @property
    def engine(self) -> DeviceEngine:
        return self._ensure_engine()
