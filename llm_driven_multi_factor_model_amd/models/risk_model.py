"""Tensor-native Barra risk model: CS-WLS factor returns -> Newey-West -> eigen adjustment -> VRA.

Equivalent of ``Barra-master/mfm/MFM.py`` (``reg_by_time`` :48-76, ``Newey_West_by_time``
:80-101, ``eigen_risk_adj_by_time`` :105-126, ``vol_regime_adj_by_time`` :130-167) and the
diagnostics of ``mfm/utils.py`` (``eigenfactor_bias_stat`` :97-117, ``bayes_shrink`` :153-168),
re-designed for MI355X:

* no per-date Python loop: every stage is one batched launch over all dates of the shard;
* data-parallel over dates: a ``RiskPanel`` shard with ``date_offset`` runs on each rank; the
  factor-return series is all-gathered once (RCCL) and the Newey-West scan emits only the
  rank's own dates; the eigen adjustment of a date needs only that date's covariance; the VRA
  bias series is all-gathered once;
* outputs stay on the device as float64 tensors; pandas objects are built only on request;
* every stage is traced (ROCTX range, HIP-event GPU time, JSONL metrics: utils/trace.py);
* checkpoint / resume: :meth:`RiskModel.state_dict` exports the O(T K) history the scans need and
  :meth:`RiskModel.resume` appends new dates without re-running the old ones (utils/checkpoint.py).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from ..ops import cross_section as xs
from ..ops import ew_scan, eigen
from ..parallel import dist as pdist
from ..utils import checkpoint as ckpt
from ..utils import trace
from ..utils.config import RiskConfig
from .panel import RiskPanel


class MinVariance(NamedTuple):
    """:meth:`RiskModel.min_variance`: ``weights`` [D_loc, N], ``variance`` [D_loc] (float64)."""
    weights: torch.Tensor
    variance: torch.Tensor


class Portfolio(NamedTuple):
    """:meth:`RiskModel.optimize`: ``weights`` [D_loc, N], ``variance`` [D_loc] (float64),
    ``passes`` / ``status`` [D_loc] (int32, the codes of :mod:`ops.box_qp`), ``active_variance``
    [D_loc] (None without a benchmark), ``expected_return`` [D_loc] (None without alpha);
    with ``neutral``: ``exposure_gap`` [D_loc] = max |x_S - t| and ``eta`` [D_loc, m], the
    multipliers of the exposure constraints (:mod:`ops.exposure_qp`), None otherwise; with
    ``tcost``: ``turnover`` [D_loc] = sum |h - prev| and ``cost`` [D_loc] = sum tcost |h - prev|
    (:class:`ops.box_qp.BoxQPCost`), None otherwise."""
    weights: torch.Tensor
    variance: torch.Tensor
    passes: torch.Tensor
    status: torch.Tensor
    active_variance: torch.Tensor | None
    expected_return: torch.Tensor | None
    exposure_gap: torch.Tensor | None = None
    eta: torch.Tensor | None = None
    turnover: torch.Tensor | None = None
    cost: torch.Tensor | None = None


class EvalSummary(NamedTuple):
    """:class:`ops.factor_eval.ICSummary` of ``ic`` and of ``rank_ic`` ([S, H] fields)."""
    ic: ICSummary
    rank_ic: ICSummary


class FactorEval(NamedTuple):
    """:meth:`RiskModel.factor_ic`: ``n`` int32, ``ic`` / ``rank_ic`` [D_loc, S, H]; ``q_ret`` /
    ``q_count`` [D_loc, S, H, G]; ``spread`` = ``q_ret[..., -1] - q_ret[..., 0]`` (None when G =
    0); ``summary`` over the global dates (the same on every rank)."""
    n: torch.Tensor
    ic: torch.Tensor
    rank_ic: torch.Tensor
    q_ret: torch.Tensor
    q_count: torch.Tensor
    spread: torch.Tensor | None
    summary: EvalSummary


class RiskModel:
    """Barra risk model over a (possibly date-sharded) panel.

    Attributes after the stages run (rank-local date block unless stated):
      factor_ret [D_loc, K], specific_ret [D_loc, N], r2 [D_loc], status [D_loc]
      factor_ret_global [T, K] (all ranks' dates), nw_cov / eigen_cov / vra_cov [D_loc, K, K],
      vra_lambda [D_loc]
    """

    def __init__(self, panel: RiskPanel, config: RiskConfig | None = None,
                 T_global: int | None = None, ctx: pdist.DistContext | None = None,
                 history: dict | None = None, sync_stages: bool = True):
        self.panel = panel
        self.cfg = config or RiskConfig()
        self.ctx = ctx or pdist.context()
        # dates already processed by an earlier run (checkpoint): global index offset
        self.history = history
        self.T_hist = int(history["T"]) if history is not None else 0
        # every rank's date-block length, exchanged once: the per-stage all-gathers then run
        # as single collectives without host synchronisation
        self.sizes = pdist.shard_sizes(panel.D, self.ctx)
        T_new = sum(self.sizes)
        if T_global is not None and int(T_global) != T_new:
            raise ValueError(f"T_global={T_global} but the ranks' date blocks sum to {T_new}")
        self.T = self.T_hist + T_new
        self.times = trace.Timer()
        self.sync_stages = sync_stages
        self.factor_ret = self.specific_ret = self.r2 = self.status = self.stats = None
        self.factor_ret_global = None
        self.nw_cov = self.eigen_cov = self.vra_cov = self.vra_lambda = None
        self.eigen_bias = None
        self.B2_global = self.B2 = None
        self.nw_params = None     # (q, tau) of the last newey_west() call
        self.spec_vra_lambda = None   # [D_loc], set by specific_risk_use4()
        self._est_cov = None          # (stats it was formed from, EstCov), set by estimator_cov()

    def _stage(self, name: str):
        return trace.stage(name, self.times, self.device, sync=self.sync_stages,
                           dates=self.panel.D, K=self.K)

    @property
    def device(self):
        return self.panel.device

    @property
    def K(self) -> int:
        return self.panel.K

    @property
    def t_lo(self) -> int:
        """Global index of this rank's first date (history dates come first)."""
        return self.T_hist + self.panel.date_offset

    # --------------------------------------------------------------- stage 1: regression
    def regress(self, want_resid: bool = True):
        p = self.panel
        with self._stage("regress"):
            res = xs.xs_wls(p.styles, p.cap, p.ret, p.ind, p.P, pivot_mode=self.cfg.pivot_mode,
                            want_resid=want_resid, deterministic=self.cfg.deterministic)
        self.factor_ret, self.specific_ret, self.r2 = res.f, res.resid, res.r2
        self.status, self.stats = res.status, res.stats
        self.factor_ret_global = None
        if self.cfg.time_scan == "gather":
            self._gather_f()
        return self.factor_ret, self.specific_ret, self.r2

    def _gather_f(self) -> torch.Tensor:
        """[T, K] factor returns of every date (history first).  Collective."""
        if self.factor_ret_global is None:
            with self._stage("allgather_f"):
                F = pdist.all_gather_rows(self.factor_ret, self.ctx, self.sizes)
                if self.history is not None:
                    F = torch.cat([self.history["factor_ret"].to(F.device, F.dtype), F])
                self.factor_ret_global = F
        return self.factor_ret_global

    def _hist(self, key: str):
        if self.history is None:
            return None
        return self.history[key].to(self.device, torch.float64)

    # --------------------------------------------------------------- stage 2: Newey-West
    def newey_west(self, q: int | None = None, tau: float | None = None):
        if self.factor_ret is None:
            raise RuntimeError("please run regress() to get factor returns first")
        q = self.cfg.nw_lags if q is None else q
        tau = self.cfg.nw_half_life if tau is None else tau
        lo = self.t_lo
        self.nw_params = (int(q), float(tau))
        with self._stage("newey_west"):
            if self.cfg.time_scan == "carry":  # own dates only, block states carried across ranks
                self.nw_cov = ew_scan.newey_west_series_sharded(
                    self.factor_ret, q, tau, self.ctx, self.sizes, history=self._hist("factor_ret"))
            else:
                self.nw_cov = ew_scan.newey_west_series(self._gather_f(), q, tau, lo,
                                                        lo + self.panel.D)
        return self.nw_cov

    # --------------------------------------------------------------- stage 3: eigen adjustment
    def eigen_adjust(self, M: int | None = None, scale_coef: float | None = None,
                     T_sim: int | None = None, seed: int | None = None):
        if self.nw_cov is None:
            raise RuntimeError("please run newey_west() first")
        M = self.cfg.eigen_sims if M is None else M
        scale_coef = self.cfg.eigen_scale if scale_coef is None else scale_coef
        T_sim = T_sim or self.cfg.eigen_sim_length or self.T
        seed = self.cfg.eigen_seed if seed is None else seed
        with self._stage("eigen_adjust"):
            if self.cfg.eigen_shard == "sims":
                # Simulations sharded over ranks (10k-bootstrap configuration): every rank needs
                # the Newey-West covariances of ALL new dates, runs its block of sims on all of
                # them, and one all_reduce of the [T, K] bias sums (C5) completes the mean over M.
                lo_new = self.T_hist
                if self.cfg.time_scan == "carry":
                    # each rank scanned only its own dates: gather those blocks (no rescan, no
                    # factor-return gather), so the SP scan composes with C5 sharding
                    nw_all = pdist.all_gather_rows(self.nw_cov.contiguous(), self.ctx,
                                                   self.sizes)
                else:
                    # the gathered series is already on every rank: an O(T K^2) rescan is
                    # cheaper than gathering [T, K, K]
                    q_nw, tau_nw = self.nw_params  # the (q, tau) newey_west() actually used
                    nw_all = ew_scan.newey_west_series(self._gather_f(), q_nw, tau_nw, lo_new,
                                                       self.T)
                Fh, vb = eigen.eigen_risk_adjust_sharded(
                    nw_all, M=M, scale_coef=scale_coef, T_sim=T_sim, seed=seed,
                    chunk=self.cfg.eigen_chunk, ctx=self.ctx, psd_tol=self.cfg.psd_tol,
                    return_bias=True, date0=lo_new)
                a = self.t_lo - lo_new
                self.eigen_cov = Fh[a:a + self.panel.D].contiguous()
                self.eigen_bias = vb[a:a + self.panel.D].contiguous()
            else:
                self.eigen_cov, self.eigen_bias = eigen.eigen_risk_adjust(
                    self.nw_cov, M=M, scale_coef=scale_coef, T_sim=T_sim, seed=seed,
                    psd_tol=self.cfg.psd_tol, return_bias=True, date0=self.t_lo)
        return self.eigen_cov

    # --------------------------------------------------------------- stage 4: VRA
    def vol_regime_adjust(self, tau: float | None = None):
        """lambda_t^2 = EW mean of B_s^2 over valid s <= t; B_t^2 = mean_k f_tk^2 / sigma_tk^2.

        ``sigma_t`` is the eigen-adjusted forecast of date t itself (in-sample, quirk Q10); with
        ``config.vra_out_of_sample`` the forecast made at t-1 is used instead (USE4 practice).
        """
        if self.eigen_cov is None:
            raise RuntimeError("please run eigen_adjust() first")
        tau = self.cfg.vra_half_life if tau is None else tau
        with self._stage("vra"):
            var = torch.diagonal(self.eigen_cov, dim1=-2, dim2=-1)        # [D_loc, K]
            if self.cfg.vra_out_of_sample:
                var_all = pdist.all_gather_rows(var.contiguous(), self.ctx, self.sizes)
                if self.history is not None and "last_var" in self.history:
                    prev0 = self.history["last_var"].to(var.device, var.dtype)[None]
                else:
                    prev0 = torch.full_like(var_all[:1], float("nan"))
                prev = torch.cat([prev0, var_all[:-1]])
                lo = self.panel.date_offset
                var = prev[lo:lo + self.panel.D]
            B2 = (self.factor_ret ** 2 / var).mean(-1)                    # NaN where ER empty
            self.B2 = B2
            self.B2_global = None
            if self.cfg.time_scan == "carry":
                lam2 = ew_scan.ew_prefix_mean_sharded(B2, tau, self.ctx, self.sizes,
                                                      history=self._hist("B2"))
            else:
                lam2 = ew_scan.ew_prefix_mean(self._gather_b2(), tau)[
                    self.t_lo:self.t_lo + self.panel.D]
            # no valid date yet: the reference's sum over an empty selection gives lambda = 0
            lam2 = torch.nan_to_num(lam2, nan=0.0)
            self.vra_lambda = torch.sqrt(lam2)
            self.vra_cov = self.eigen_cov * lam2[:, None, None]
        return self.vra_cov, self.vra_lambda

    def _gather_b2(self) -> torch.Tensor:
        """[T] VRA bias statistics of every date (history first).  Collective."""
        if self.B2_global is None:
            B2_all = pdist.all_gather_rows(self.B2, self.ctx, self.sizes)
            if self.history is not None:
                B2_all = torch.cat([self.history["B2"].to(B2_all.device, B2_all.dtype), B2_all])
            self.B2_global = B2_all
        return self.B2_global

    def run(self):
        self.regress()
        self.newey_west()
        self.eigen_adjust()
        self.vol_regime_adjust()
        return self

    # --------------------------------------------------------------- checkpoint / resume
    def state_dict(self) -> dict:
        """History needed to append dates later (identical on every rank), plus artifacts.

        Call after :meth:`run`.  Collective in distributed mode (every rank must call it).
        """
        if self.vra_cov is None:
            raise RuntimeError("run all four stages before exporting a checkpoint")
        F_all, B2_all = self._gather_f(), self._gather_b2()
        r2 = pdist.all_gather_rows(self.r2, self.ctx, self.sizes)
        status = pdist.all_gather_rows(self.status, self.ctx, self.sizes)
        var = torch.diagonal(self.eigen_cov, dim1=-2, dim2=-1).contiguous()
        var_all = pdist.all_gather_rows(var, self.ctx, self.sizes)
        vra_last = pdist.all_gather_rows(self.vra_cov[-1:].contiguous(), self.ctx)[-1]
        if self.history is not None:
            r2 = torch.cat([self.history["r2"].to(r2.device), r2])
            status = torch.cat([self.history["status"].to(status.device), status])
        dates = [str(d) for d in self._global_dates()]
        if self.history is not None:
            dates = list(self.history["dates"]) + dates
        cfg = self.cfg.to_dict()
        return {
            "T": int(F_all.shape[0]), "K": int(self.K),
            "factor_names": list(self.panel.factor_names), "dates": dates,
            "config": {k: v for k, v in cfg.items()}, "config_hash": ckpt.config_hash(cfg),
            "factor_ret": F_all, "B2": B2_all,
            "r2": r2, "status": status, "last_var": var_all[-1], "last_vra_cov": vra_last,
        }

    def save(self, path) -> None:
        """Write a checkpoint (rank 0 writes; collective in distributed mode)."""
        st = self.state_dict()
        if self.ctx.rank == 0:
            ckpt.save_state(st, path)
        pdist.barrier(self.ctx)

    @classmethod
    def resume(cls, state, panel: RiskPanel, config: RiskConfig | None = None,
               T_global: int | None = None, ctx: pdist.DistContext | None = None, **kw):
        """A model for the NEW dates of ``panel`` continuing the run saved in ``state`` (a dict
        from :meth:`state_dict` or a checkpoint path).  Old dates are not recomputed: their
        factor returns feed the Newey-West prefix scan and the VRA series.  Results for the
        new dates equal those of one run over all dates (the eigen simulation length follows
        the total number of dates, quirk Q9, as in a full run)."""
        if not isinstance(state, dict):
            state = ckpt.load_state(state)
        stored = dict(state["config"])
        fv = int(state.get("format_version", ckpt.FORMAT_VERSION))
        if ckpt.config_hash(stored, fv) != state["config_hash"]:
            raise ValueError("checkpoint config does not match its hash (corrupt file?)")
        # fields a format-1 file predates take their defaults; unknown keys are ignored
        import dataclasses
        known = {f.name for f in dataclasses.fields(RiskConfig)}
        saved = RiskConfig(**{k: v for k, v in stored.items() if k in known})
        cfg = config or saved
        if ckpt.model_config(cfg.to_dict()) != ckpt.model_config(saved.to_dict()):
            raise ValueError("checkpoint was produced with a different RiskConfig")
        if int(state["K"]) != panel.K or list(state["factor_names"]) != list(panel.factor_names):
            raise ValueError("factor set of the new panel differs from the checkpoint")
        if len(panel.dates) and len(state["dates"]):
            import pandas as pd
            if pd.Timestamp(str(panel.dates[0])) <= pd.Timestamp(str(state["dates"][-1])):
                raise ValueError("resume panel must start after the last checkpointed date")
        return cls(panel, cfg, T_global=T_global, ctx=ctx, history=state, **kw)

    def diagnostics(self) -> dict:
        """Counters of the run (rank-local dates): solver status bits and NaN rates."""
        st = self.status.cpu() if self.status is not None else torch.zeros(0, dtype=torch.int32)
        out = {"dates": int(st.numel())}
        for name, bit in (("no_rows", xs.XS_NO_ROWS), ("pivot_empty", xs.XS_PIVOT_EMPTY),
                          ("near_singular", xs.XS_NEAR_SINGULAR), ("zero_pivot", xs.XS_ZERO_PIVOT),
                          ("pinv_cut", xs.XS_PINV_CUT), ("bad_sigma", xs.XS_BAD_SIGMA)):
            out[name] = int(((st & bit) != 0).sum())
        for name, t in (("factor_ret", self.factor_ret), ("nw_cov", self.nw_cov),
                        ("eigen_cov", self.eigen_cov), ("vra_cov", self.vra_cov)):
            if t is not None and t.numel():
                bad = ~torch.isfinite(t.reshape(t.shape[0], -1)).all(-1)
                out[f"{name}_nan_dates"] = int(bad.sum())
        return out

    # --------------------------------------------------------------- diagnostics
    def eigenfactor_bias(self, which: str = "eigen", start: int = 0, predlen: int = 1):
        """Eigenfactor bias statistic (``MFM.py:203-204`` runs it with predlen=21 on dates >=
        1000) of the chosen covariance series over GLOBAL dates t >= ``start`` with
        t + predlen < T.  Collective: each rank forms the z-scores of its own dates (the
        realised returns of later dates come from the gathered factor-return series), the z rows
        are all-gathered in calendar order and the std runs over all of them, so the result is
        the same on every rank and for every world size.  After :meth:`resume` only dates
        computed in this run have covariances: dates before the checkpoint's end are skipped
        with a RuntimeWarning."""
        cov = {"nw": self.nw_cov, "eigen": self.eigen_cov, "vra": self.vra_cov}[which]
        if cov is None:
            raise RuntimeError(f"covariance series {which!r} not computed yet")
        F = self._gather_f()                     # [T, K] with history first
        T, lo, D = self.T, self.t_lo, self.panel.D
        if self.T_hist > start and self.ctx.rank == 0:
            # a checkpoint keeps no covariance series: resumed runs cover their own dates only
            import warnings
            warnings.warn(f"eigenfactor_bias: dates [{start}, {self.T_hist}) precede this resumed "
                          f"run (no stored covariances); the statistic covers dates >= "
                          f"{self.T_hist} only", RuntimeWarning, stacklevel=2)
        a, b = max(start, lo), min(lo + D, T - predlen)
        z = torch.empty(0, self.K, dtype=torch.float64, device=self.device)
        if b > a:
            z = eigenfactor_z(cov[a - lo:b - lo], F[a + 1:b + predlen], predlen)
        Z = pdist.all_gather_rows(z.contiguous(), self.ctx)
        if Z.shape[0] == 0:
            return torch.full((self.K,), float("nan"), dtype=torch.float64)
        Z = Z[torch.isfinite(Z).all(-1)]
        return Z.std(0, unbiased=False)

    def specific_vol_series(self, window: int = 252, min_periods: int = 1) -> torch.Tensor:
        """[D_loc, N] trailing specific volatility, point in time: for date t the ddof-0 std of
        each stock's specific returns over the ``window`` dates ENDING at t (dates before t
        only; no later date enters).  The window crosses rank boundaries through a halo of the
        preceding window-1 rows (one collective), and every window is summed in the same fixed
        order whatever the sharding, so the result is bitwise rank-invariant.  Checkpoints keep
        no specific returns: after a resume the first window-1 new dates see only new dates."""
        e = self.specific_ret.double()
        D = e.shape[0]
        h = window - 1
        halo = pdist.halo_prev_rows(e, h, self.ctx, self.sizes)
        if e.is_cuda:  # HIP kernel, bitwise the loop below (csrc/attribution.hip)
            from ..ops.attribution import trailing_vol
            return trailing_vol(halo, e, window, min_periods)
        ext = torch.cat([halo, e])
        ok = torch.isfinite(ext)
        x = torch.where(ok, ext, torch.zeros((), dtype=torch.float64, device=e.device))
        okd = ok.double()
        n = torch.zeros_like(e)
        s1 = torch.zeros_like(e)
        s2 = torch.zeros_like(e)
        for j in range(window):  # fixed summation order: newest date first
            sl = slice(h - j, h - j + D)
            n += okd[sl]
            s1 += x[sl]
            s2 += x[sl] * x[sl]
        mean = s1 / n
        var = s2 / n - mean * mean
        vol = torch.sqrt(torch.clamp(var, min=0.0))
        return torch.where(n >= max(1, min_periods), vol,
                           torch.full_like(vol, float("nan")))

    def specific_risk_shrunk(self, window: int = 252, ngroup: int = 10, q: float = 1.0,
                             per_date: bool = True):
        """Cap-decile Bayesian shrinkage (``utils.bayes_shrink``, utils.py:153-168) of the
        point-in-time trailing specific volatility.  ``per_date``: [D_loc, N], date t shrunk
        with its own window and caps; otherwise [N] of the LAST global date, on every rank
        (broadcast from the rank that owns it).  Collective in distributed mode."""
        from ..ops.xs_reduce import bayes_shrink
        vol = self.specific_vol_series(window)
        s = bayes_shrink(vol, self.panel.cap.double(), ngroup, q).double()
        if per_date:
            return s
        return pdist.broadcast_last_row(s, self.ctx, self.sizes)

    def specific_vol_ewnw(self, window: int = 252, half_life: float = 84.0, lags: int = 5,
                          min_periods: int = 1) -> torch.Tensor:
        """[D_loc, N] exponentially weighted, Newey-West corrected trailing specific volatility
        (:func:`ops.specific_risk.ewnw_vol`): weights ``0.5 ** (age / half_life)`` and ``lags``
        Bartlett-weighted autocovariances over the ``window`` dates ENDING at each date, with the
        half-life and lag semantics of the factor covariance.  Point in time; the halo of the
        preceding window - 1 rows crosses rank boundaries (one collective) and every window is
        summed in its own fixed order, so the result is bitwise rank-invariant.  GPU: ``lags <=
        5`` and ``window <= 1024``.  Checkpoints keep no specific returns: after a resume the
        first window - 1 new dates see only new dates."""
        from ..ops.specific_risk import ewnw_vol
        e = self.specific_ret.double()
        halo = pdist.halo_prev_rows(e, window - 1, self.ctx, self.sizes)
        return ewnw_vol(halo, e, window, half_life, lags, min_periods)

    def specific_risk_use4(self, window: int = 252, half_life: float = 84.0, lags: int = 5,
                           ngroup: int = 10, q: float = 1.0, vra_half_life: float | None = None,
                           out_of_sample: bool = True, per_date: bool = True):
        """USE4-style specific risk: the cap-decile Bayesian shrinkage of
        :meth:`specific_vol_ewnw`, times the specific volatility-regime multiplier lambda_S.

        ``B2[t] = sum_n cap_n (e_tn / s_n)^2 / sum_n cap_n`` (:func:`ops.specific_risk.
        spec_bias2`) tests the shrunk forecast ``s`` against the specific returns of date t:
        the forecast made at t - 1 by default (``out_of_sample``; the first global date has
        none, its B2 is NaN), that of date t itself otherwise.  ``lambda_S[t]^2`` is the
        exponentially weighted mean (``vra_half_life``, default ``config.vra_half_life``) of
        the B2 of all valid dates <= t, 1 while there is none; ``config.time_scan`` chooses the
        carried scan or one all-gather, as for the factor VRA.  Returns ``s * lambda_S`` as
        [D_loc, N] and keeps ``spec_vra_lambda`` [D_loc]; ``per_date=False``: [N] of the LAST
        global date on every rank.  Collective in distributed mode.

        A checkpoint keeps neither specific returns nor the B2 history of this model: after a
        resume the windows and lambda_S start from the new dates."""
        from ..ops.specific_risk import spec_bias2
        from ..ops.xs_reduce import bayes_shrink
        cap = self.panel.cap
        s = bayes_shrink(self.specific_vol_ewnw(window, half_life, lags), cap.double(), ngroup,
                         q).double()
        e = self.specific_ret.double()
        fc = s
        if out_of_sample:
            fc = torch.cat([pdist.halo_prev_rows(s, 1, self.ctx, self.sizes), s])[:s.shape[0]]
        B2 = spec_bias2(e, fc, cap if cap.dtype == torch.float64 else cap.float())
        tau = self.cfg.vra_half_life if vra_half_life is None else vra_half_life
        if self.cfg.time_scan == "carry":
            lam2 = ew_scan.ew_prefix_mean_sharded(B2, tau, self.ctx, self.sizes)
        else:
            lo = self.panel.date_offset
            lam2 = ew_scan.ew_prefix_mean(pdist.all_gather_rows(B2, self.ctx, self.sizes), tau)[
                lo:lo + self.panel.D]
        lam2 = torch.nan_to_num(lam2, nan=1.0)   # no valid date yet: no adjustment
        self.spec_vra_lambda = torch.sqrt(lam2)
        out = s * self.spec_vra_lambda[:, None]
        if per_date:
            return out
        return pdist.broadcast_last_row(out, self.ctx, self.sizes)

    def _specific_vol_named(self, name: str) -> torch.Tensor:
        """``specific_vol`` given as a string: ``"use4"`` is :meth:`specific_risk_use4`, every
        other string :meth:`specific_risk_shrunk`."""
        return self.specific_risk_use4() if name == "use4" else self.specific_risk_shrunk()

    def risk_attribution(self, h: torch.Tensor, which: str = "vra",
                         specific_vol: torch.Tensor | str | None = "shrunk"):
        """Risk decomposition of holdings ``h`` ([N] held every date, or [D_loc, N]) on this
        rank's dates against the chosen covariance series (``nw`` / ``eigen`` / ``vra``).

        ``specific_vol``: per-stock specific volatility [N] or [D_loc, N]; ``"shrunk"`` uses
        :meth:`specific_risk_shrunk` (cap-decile Bayesian shrinkage of each date's own trailing
        residual vol: point in time, identical for every world size; collective), ``"use4"``
        :meth:`specific_risk_use4` (EW Newey-West vol, shrunk, times the specific
        volatility-regime multiplier; collective); None ignores specific risk.  Returns :class:`ops.attribution.RiskAttribution`.
        """
        from ..ops import attribution as attr
        if self.stats is None:
            raise RuntimeError("run regress() first")
        p = self.panel
        h = h.to(device=p.device, dtype=torch.float64)
        if h.dim() == 1:
            h = h[None, :].expand(p.D, -1)
        cov = {"nw": self.nw_cov, "eigen": self.eigen_cov, "vra": self.vra_cov}[which]
        if cov is None:
            raise RuntimeError(f"covariance series {which!r} not computed yet")
        x = attr.portfolio_exposure(p.styles, p.cap, p.ret, p.ind, h.contiguous(), self.stats, p.P)
        if isinstance(specific_vol, str):
            specific_vol = self._specific_vol_named(specific_vol)
        svar = None if specific_vol is None else attr.portfolio_specific_var(h, specific_vol)
        return attr.risk_attribution(x, cov, svar)

    # --------------------------------------------------------------- portfolio construction
    def _cov_inputs(self, which: str, specific_vol):
        """(factor covariance series, specific volatility) for the asset-covariance methods."""
        if self.stats is None:
            raise RuntimeError("run regress() first")
        cov = {"nw": self.nw_cov, "eigen": self.eigen_cov, "vra": self.vra_cov}[which]
        if cov is None:
            raise RuntimeError(f"covariance series {which!r} not computed yet")
        if specific_vol is None:
            raise ValueError("the asset covariance needs specific volatilities: pass a tensor "
                             "[N] / [D_loc, N], 'shrunk' or 'use4'")
        if isinstance(specific_vol, str):
            specific_vol = self._specific_vol_named(specific_vol)
        return cov, specific_vol.to(self.device)

    def _rows(self, h: torch.Tensor) -> torch.Tensor:
        h = h.to(device=self.device, dtype=torch.float64)
        return h[None, :].expand(self.panel.D, -1) if h.dim() == 1 else h

    def solve_cov(self, b: torch.Tensor, which: str = "vra",
                  specific_vol: torch.Tensor | str = "shrunk",
                  universe: torch.Tensor | None = None) -> torch.Tensor:
        """``Sigma_d^-1 b`` on this rank's dates for the asset covariance ``Sigma_d = X_d F_d X_d^T
        + diag(s_d^2)`` (:mod:`ops.factor_cov`: Woodbury, no N x N matrix).  ``b`` is [N] (the
        same every date), [D_loc, N] or [D_loc, NB, N]; ``which`` / ``specific_vol`` as in
        :meth:`risk_attribution`; ``universe`` an optional [D_loc, N] bool mask.  Stocks outside
        the universe get 0, dates with an invalid covariance NaN.  Per date: the only collective
        is the one ``"shrunk"`` makes."""
        from ..ops import factor_cov as fc
        cov, sv = self._cov_inputs(which, specific_vol)
        p = self.panel
        return fc.solve_cov(p.styles, p.cap, p.ret, p.ind, self.stats, p.P, cov, sv,
                            self._rows(b), universe)

    def apply_cov(self, h: torch.Tensor, which: str = "vra",
                  specific_vol: torch.Tensor | str = "shrunk",
                  universe: torch.Tensor | None = None) -> torch.Tensor:
        """``Sigma_d h`` restricted to the universe; arguments as :meth:`solve_cov`."""
        from ..ops import factor_cov as fc
        cov, sv = self._cov_inputs(which, specific_vol)
        p = self.panel
        return fc.apply_cov(p.styles, p.cap, p.ret, p.ind, self.stats, p.P, cov, sv,
                            self._rows(h), universe)

    def min_variance(self, which: str = "vra", specific_vol: torch.Tensor | str = "shrunk",
                     universe: torch.Tensor | None = None):
        """Fully invested, unconstrained minimum-variance portfolio of every date:
        ``weights`` [D_loc, N] = y / sum(y) with y = Sigma^-1 1_U, and its ``variance`` [D_loc]
        = 1 / sum(y).  NaN on dates with an invalid covariance or an empty universe."""
        p = self.panel
        ones = torch.ones(p.D, p.N, dtype=torch.float64, device=self.device)
        y = self.solve_cov(ones, which, specific_vol, universe)
        tot = y.sum(-1)
        tot = torch.where(tot > 0, tot, torch.full_like(tot, float("nan")))
        return MinVariance(weights=y / tot[:, None], variance=1.0 / tot)

    def optimize(self, alpha: torch.Tensor | None = None, risk_aversion: float = 1.0,
                 lower=0.0, upper=1.0, benchmark: torch.Tensor | None = None, budget=1.0,
                 which: str = "vra", specific_vol: torch.Tensor | str = "shrunk",
                 universe: torch.Tensor | None = None, neutral=None, exposure=None,
                 prev=None, tcost=None, dates: tuple[int, int] | None = None,
                 **solver) -> Portfolio:
        """Box-constrained portfolio of every date (:func:`ops.box_qp.box_qp`): minimise
        ``1/2 h^T Sigma h - q^T h`` subject to ``sum h = budget`` and ``lower <= h <= upper`` on
        the universe, with ``q = alpha / risk_aversion`` (+ ``Sigma h_b`` when a ``benchmark`` is
        given: minimum tracking error, or a mean-variance tilt around it).  ``alpha`` /
        ``benchmark`` are [N] or [D_loc, N]; ``lower`` / ``upper`` a scalar, [N] or [D_loc, N];
        ``which`` / ``specific_vol`` / ``universe`` as in :meth:`min_variance`; ``solver``
        passes ``tol``, ``max_passes`` and ``check_every`` on.  Infeasible dates and dates with
        an invalid covariance give NaN rows (see ``status``).  Per date: the only collective is
        the one ``"shrunk"`` makes.

        ``neutral`` adds the equality constraints ``(X^T h)_k = t_k`` on a set of factors
        (:func:`ops.exposure_qp.exposure_qp`): an index list into the K factors without the
        country, or ``"industries"``, ``"styles"``, ``"all"`` (every factor but the country).
        ``exposure`` [m] or [D_loc, m] are the targets; None means the exposures of
        ``benchmark`` restricted to the universe (active-neutral; ``ValueError`` without a
        benchmark).  ``neutral=None`` is the box-constrained problem alone.

        ``prev`` / ``tcost`` (a scalar, [N] or [D_loc, N] each; both or neither) add the linear
        trading cost ``sum_n tcost_n |h_n - prev_n|`` to the objective (:mod:`ops.tcost_qp`):
        ``prev`` are the holdings before the trade, ``tcost`` = +inf freezes a name; the result
        carries ``turnover`` and ``cost``.  ``dates`` = (a, b) solves the local dates a..b-1
        only: every per-date argument is still given for the whole block and is cut to those
        rows, and the result has b - a rows (:meth:`rebalance` solves one date at a time)."""
        from ..ops import box_qp as bq
        from ..ops import factor_cov as fc
        cov, sv = self._cov_inputs(which, specific_vol)
        p, stats = self.panel, self.stats
        if dates is not None:
            a0, b0 = dates
            D_all = p.D
            p, stats, cov = p.slice_dates(a0, b0), stats[a0:b0], cov[a0:b0]

            def cut(t, per_date_dim=2):
                if isinstance(t, torch.Tensor) and t.dim() >= per_date_dim \
                        and t.shape[0] == D_all:
                    return t[a0:b0]
                return t
            sv, alpha, benchmark, lower, upper, universe, exposure, prev, tcost = map(
                cut, (sv, alpha, benchmark, lower, upper, universe, exposure, prev, tcost))
            budget = cut(budget, 1)
        rows = lambda t: t.to(device=self.device, dtype=torch.float64).expand(p.D, -1)  # noqa: E731
        args = (p.styles, p.cap, p.ret, p.ind, stats, p.P)
        q = torch.zeros(p.D, p.N, dtype=torch.float64, device=self.device)
        al = hb = Shb = None
        tc = {} if tcost is None and prev is None else dict(prev=prev, tcost=tcost)
        if alpha is not None:
            al = torch.nan_to_num(rows(alpha), nan=0.0, posinf=0.0, neginf=0.0)
            q = q + al / risk_aversion
        if benchmark is not None:
            hb = rows(benchmark)
            Shb = fc.apply_cov(*args, cov, sv, hb, universe)
            q = q + Shb
        gap = eta = None
        if neutral is None:
            if exposure is not None:
                raise ValueError("exposure needs neutral, the factors it constrains")
            r = bq.box_qp(*args, cov, sv, q, lower, upper, budget, universe, **solver, **tc)
        else:
            from ..ops import exposure_qp as eq
            sel = self._neutral_factors(neutral)
            if exposure is None:
                if hb is None:
                    raise ValueError("neutral without exposure targets needs a benchmark")
                m = fc.universe_mask(p.styles, p.cap, p.ret, p.ind, p.P, sv, universe)
                hz = torch.where(m, torch.nan_to_num(hb, nan=0.0, posinf=0.0, neginf=0.0),
                                 torch.zeros_like(q))
                exposure = fc.factor_xty(*args, hz[:, None])[:, 0][:, sel]
            else:
                exposure = torch.as_tensor(exposure, dtype=torch.float64, device=self.device)
            r = eq.exposure_qp(*args, cov, sv, sel, exposure, q, lower, upper, budget, universe,
                               **solver, **tc)
            gap, eta = r.exposure_gap, r.eta
        active = ret = None
        if hb is not None:   # (h - h_b)^T Sigma (h - h_b), h_b restricted to the universe
            m = fc.universe_mask(p.styles, p.cap, p.ret, p.ind, p.P, sv, universe)
            hz = torch.where(m, torch.nan_to_num(hb, nan=0.0, posinf=0.0, neginf=0.0),
                             torch.zeros_like(q))
            e = r.weights - hz   # formed from the difference: no cancellation of variances
            active = (e * fc.apply_cov(*args, cov, sv, e, universe)).sum(-1)
        if al is not None:
            ret = (al * r.weights).sum(-1)
        return Portfolio(r.weights, r.variance, r.passes, r.status, active, ret, gap, eta,
                         *((r.turnover, r.cost) if tc else ()))

    def risk_budget(self, budgets=None, budget=1.0, which: str = "vra",
                    specific_vol: torch.Tensor | str = "shrunk",
                    universe: torch.Tensor | None = None,
                    dates: tuple[int, int] | None = None, **solver):
        """Risk-budgeting (risk-parity) portfolio of every date
        (:func:`ops.risk_budget.risk_budget`): the long-only, fully invested ``h`` with
        ``h_n (Sigma h)_n / h^T Sigma h = b_n / sum b`` on the stocks with a budget ``b_n > 0``.
        ``budgets``: None (equal risk contribution), [N] or [D_loc, N]; ``budget`` (the sum of
        the weights) a scalar or [D_loc]; ``which`` / ``specific_vol`` / ``universe`` /
        ``dates`` as in :meth:`optimize`; ``solver`` passes ``tol``, ``max_passes``,
        ``check_every`` and ``theta`` on.  Returns :class:`ops.risk_budget.RiskBudget`; dates
        with an empty universe or an invalid covariance give NaN rows (see ``status``).  Per
        date: the only collective is the one ``"shrunk"`` makes."""
        from ..ops import risk_budget as rbm
        cov, sv = self._cov_inputs(which, specific_vol)
        p, stats = self.panel, self.stats
        if dates is not None:
            a0, b0 = dates
            D_all = p.D
            p, stats, cov = p.slice_dates(a0, b0), stats[a0:b0], cov[a0:b0]

            def cut(t, per_date_dim=2):
                if isinstance(t, torch.Tensor) and t.dim() >= per_date_dim \
                        and t.shape[0] == D_all:
                    return t[a0:b0]
                return t
            sv, budgets, universe = map(cut, (sv, budgets, universe))
            budget = cut(budget, 1)
        return rbm.risk_budget(p.styles, p.cap, p.ret, p.ind, stats, p.P, cov, sv, budgets,
                               budget, universe, **solver)

    def asset_cov(self, stocks, which: str = "vra", specific_vol: torch.Tensor | str = "shrunk",
                  universe: torch.Tensor | None = None,
                  dates: tuple[int, int] | None = None, correlation: bool = False):
        """Dense asset covariance (``correlation``: correlation) block ``Sigma_d[S, S]`` of a
        basket on every local date (:func:`ops.asset_cov.asset_cov`).  ``stocks``: a list of
        names of ``panel.stocks`` (``KeyError`` names an unknown one), or an index tensor [M]
        (the same basket every date) / [D_loc, M] (a basket per date, -1 = padding).  ``which``
        / ``specific_vol`` / ``universe`` / ``dates`` as in :meth:`optimize`.  Returns
        :class:`ops.asset_cov.AssetCov`: ``cov`` [D, M, M], ``vol`` / ``valid`` [D, M]; members
        outside the universe give NaN rows and columns.  Per date: the only collective is the
        one ``"shrunk"`` makes."""
        from ..ops import asset_cov as ac
        cov, sv = self._cov_inputs(which, specific_vol)
        p, stats = self.panel, self.stats
        if isinstance(stocks, torch.Tensor):
            index = stocks
        else:
            pos = {str(s): i for i, s in enumerate(p.stocks)}
            missing = [str(s) for s in stocks if str(s) not in pos]
            if missing:
                raise KeyError(f"unknown stock name(s): {', '.join(missing)}")
            index = torch.tensor([pos[str(s)] for s in stocks], dtype=torch.int64)
        if index.dim() == 2 and index.shape[0] != p.D:
            raise ValueError(f"a per-date index must have {p.D} rows, got {index.shape[0]}")
        if dates is not None:
            a0, b0 = dates
            D_all = p.D
            p, stats, cov = p.slice_dates(a0, b0), stats[a0:b0], cov[a0:b0]

            def cut(t):
                if isinstance(t, torch.Tensor) and t.dim() >= 2 and t.shape[0] == D_all:
                    return t[a0:b0]
                return t
            sv, universe, index = map(cut, (sv, universe, index))
        return ac.asset_cov(p.styles, p.cap, p.ret, p.ind, stats, p.P, cov, sv,
                            index.to(self.device), universe, correlation)

    def rebalance(self, start: torch.Tensor | None = None, drift: bool = True,
                  **optimize_kwargs) -> Portfolio:
        """A path of holdings over the local dates: date t is solved by :meth:`optimize`
        (``optimize_kwargs``, which must hold ``tcost``) with ``prev`` = the holdings that date
        t - 1 ended with; the first date starts from ``start`` [N] (zeros: from cash).

        With ``drift`` the carried weights first move with the market: p = h o (1 + r) / (1 +
        sum h r) with r = ``nan_to_num(ret[t - 1])``, the panel's return row of the date the
        holdings come from.  These are fractions of the net asset value, valid for any budget,
        0 included.  A date that ends ``INFEASIBLE`` or ``INVALID`` (a NaN row) does not trade:
        the holdings are carried through it.  Returns the stacked :class:`Portfolio`; its
        ``turnover`` / ``cost`` are those of every date's trade.

        This is a sequential loop, one date after the other: D_loc times the launches-per-pass
        sequence of a one-date :meth:`optimize`, not a batched path, so a workgroup-per-date
        kernel runs on one CU.  Each date depends on the one before, so the method is
        single-process only (``RuntimeError`` with more than one rank).  ``specific_vol`` is
        resolved once, before the loop."""
        from ..ops import box_qp as bq
        if self.ctx.world > 1:
            raise RuntimeError("rebalance walks the dates in order and is single-process only; "
                               f"this run has {self.ctx.world} ranks")
        if optimize_kwargs.get("tcost") is None:
            raise ValueError("rebalance needs tcost (0.0 for none)")
        if "prev" in optimize_kwargs or "dates" in optimize_kwargs:
            raise ValueError("rebalance sets prev and dates itself")
        p = self.panel
        kw = dict(optimize_kwargs)
        sv = kw.get("specific_vol", "shrunk")
        if isinstance(sv, str):
            kw["specific_vol"] = self._specific_vol_named(sv).to(self.device)
        hold = torch.zeros(p.N, dtype=torch.float64, device=self.device) if start is None \
            else start.to(device=self.device, dtype=torch.float64).clone()
        out = []
        for t in range(p.D):
            if drift and t > 0:
                r = torch.nan_to_num(p.ret[t - 1].double(), nan=0.0, posinf=0.0, neginf=0.0)
                hold = hold * (1.0 + r) / (1.0 + (hold * r).sum())
            res = self.optimize(prev=hold, dates=(t, t + 1), **kw)
            out.append(res)
            if int(res.status[0]) < bq.INFEASIBLE:
                hold = res.weights[0]
        if not out:
            return self.optimize(prev=hold, dates=(0, 0), **kw)
        return Portfolio(*(None if f[0] is None else torch.cat(f) for f in zip(*out)))

    def _neutral_factors(self, neutral) -> list[int]:
        P, K = self.panel.P, self.K
        if isinstance(neutral, str):
            named = {"industries": list(range(1, 1 + P)), "styles": list(range(1 + P, K)),
                     "all": list(range(1, K))}
            if neutral not in named:
                raise ValueError(f"neutral must be an index list or one of {sorted(named)}, got "
                                 f"{neutral!r}")
            return named[neutral]
        return [int(k) for k in neutral]

    def predicted_beta(self, h_bench: torch.Tensor, which: str = "vra",
                       specific_vol: torch.Tensor | str = "shrunk",
                       universe: torch.Tensor | None = None) -> torch.Tensor:
        """Predicted beta of every stock to the benchmark holdings ``h_bench`` ([N] or
        [D_loc, N]): ``Sigma h_b / (h_b^T Sigma h_b)`` [D_loc, N], NaN outside the universe."""
        from ..ops import factor_cov as fc
        cov, sv = self._cov_inputs(which, specific_vol)
        p = self.panel
        h = self._rows(h_bench)
        Sh = fc.apply_cov(p.styles, p.cap, p.ret, p.ind, self.stats, p.P, cov, sv, h, universe)
        m = fc.universe_mask(p.styles, p.cap, p.ret, p.ind, p.P, sv, universe)
        hz = torch.where(m, torch.nan_to_num(h, nan=0.0, posinf=0.0, neginf=0.0),
                         torch.zeros_like(Sh))
        beta = Sh / (hz * Sh).sum(-1, keepdim=True)
        return torch.where(m, beta, torch.full_like(beta, float("nan")))

    # --------------------------------------------------------------- model validation
    def bias_test(self, h: torch.Tensor, which: str = "vra",
                  specific_vol: torch.Tensor | str = "shrunk", per_date: bool = False,
                  out_of_sample: bool = True, universe: torch.Tensor | None = None,
                  window: int = 252, min_periods: int = 63, start: int = 0):
        """Portfolio bias test (:mod:`ops.bias_test`) of the chosen covariance series and
        specific-risk model on test portfolios ``h``: [N] or [B, N] held on every date, with
        ``per_date`` [D_loc, N] or [D_loc, B, N].  ``which`` / ``specific_vol`` / ``universe`` as
        in :meth:`min_variance`.

        ``out_of_sample`` (default): row t is tested with the forecast made at t - 1, ``cov[t -
        1]`` and the specific volatility of t - 1, against the exposures ``X_t`` and the return
        ``ret[t]`` that follows them (``cov[t]`` and the specific volatility of row t already
        contain that return): the alignment of :meth:`specific_risk_use4`.  The first global
        date of a run has no forecast; its z is NaN.  Otherwise row t's own forecasts are used
        (a diagnostic).

        Returns :class:`ops.bias_test.BiasTest`: ``z``, ``forecast_vol``, ``realised`` and
        ``coverage`` (= held / gross weight) [D_loc, B], and the statistics of z over the global
        dates >= ``start``: ``bias``, ``n_obs``, ``q_stat`` and ``mrad_mean`` come from the
        all-gathered z rows and are the same on every rank and for every world size,
        ``rolling_bias`` / ``mrad`` cover this rank's dates (windows cross rank boundaries
        through a halo).  Collectives: the two forecast halos, the z halo, the z gather, and
        what the named ``specific_vol`` makes."""
        from ..ops import bias_test as bt
        cov, sv = self._cov_inputs(which, specific_vol)
        p = self.panel
        D, K = p.D, self.K
        s = sv.to(torch.float64)
        s = (s[None, :].expand(D, -1) if s.dim() == 1 else s).contiguous()
        F = cov.to(torch.float64)
        if out_of_sample:
            Ff = F.reshape(D, K * K).contiguous()
            F = torch.cat([pdist.halo_prev_rows(Ff, 1, self.ctx, self.sizes), Ff])[:D]
            F = F.reshape(D, K, K)
            s = torch.cat([pdist.halo_prev_rows(s, 1, self.ctx, self.sizes), s])[:D]
        fc = bt.portfolio_forecast(p.styles, p.cap, p.ret, p.ind, self.stats, p.P,
                                   h.to(self.device), F, s, per_date=per_date, universe=universe)
        z = bt.standardised(fc)
        var = fc.factor_var + fc.specific_var
        nan = torch.full_like(var, float("nan"))
        vol = torch.sqrt(torch.where(torch.isfinite(var) & (var > 0), var, nan))
        # the statistics see the global dates >= start only
        t = self.t_lo + torch.arange(D, device=z.device)
        zs = torch.where((t >= start)[:, None], z, nan).contiguous()
        halo = pdist.halo_prev_rows(zs, window - 1, self.ctx, self.sizes)
        zg = pdist.all_gather_rows(zs, self.ctx, self.sizes)
        st = bt.bias_stats(zs, halo, zg, window, min_periods)
        return bt.BiasTest(z=z, forecast_vol=vol, realised=fc.realised,
                           coverage=fc.held / fc.gross, stats=st)

    # --------------------------------------------------------------- the regression as an estimator
    def _panel_args(self):
        if self.stats is None:
            raise RuntimeError("run regress() first")
        p = self.panel
        return p.styles, p.cap, p.ret, p.ind, self.stats, p.P

    def estimator_cov(self):
        """:class:`ops.pure_factor.EstCov` of this rank's dates: the estimator covariance ``C``
        [D_loc, K, K] of the regression (``Var(f_d) = sigma_d^2 C_d``, ``Omega_d = C_d X_d^T
        W_d``), the ``rank`` the pseudo-inverse kept and the stock count ``n``, with
        ``config.pivot_mode``.  Per date: no collective.  Kept for the two methods below until
        :meth:`regress` runs again."""
        from ..ops import pure_factor as pf
        args = self._panel_args()
        if self._est_cov is None or self._est_cov[0] is not self.stats:
            self._est_cov = (self.stats, pf.estimator_cov(*args, pivot_mode=self.cfg.pivot_mode))
        return self._est_cov[1]

    def factor_tstats(self):
        """:class:`ops.pure_factor.FactorStats` of this rank's dates: standard errors ``se`` and
        t-statistics ``t`` [D_loc, K] of the factor returns, the residual variance ``sigma2`` and
        the degrees of freedom ``dof`` [D_loc].  Needs the specific returns of ``regress()``.
        Per date: no collective."""
        from ..ops import pure_factor as pf
        args = self._panel_args()
        if self.specific_ret is None:
            raise RuntimeError("factor_tstats needs specific returns: regress(want_resid=True)")
        return pf.factor_return_stats(*args, self.factor_ret, self.specific_ret,
                                      self.estimator_cov())

    def pure_factor_portfolios(self, factors=None) -> torch.Tensor:
        """Pure factor portfolios ``Omega`` [D_loc, S, N] float64 of the selected factors: row j
        of date d holds the stock weights whose return on date d is the factor return
        ``f[d, sel_j]`` (unit exposure to that factor, none to the others).  ``factors``: an index
        list into the K factors, or ``"country"``, ``"industries"``, ``"styles"``, ``"all"`` /
        None.  The output feeds :meth:`bias_test` as ``bias_test(H, per_date=True)``, the USE4
        test of the model on its own factor portfolios.  Per date: no collective.

        Memory: ``D_loc S N 8`` bytes; an all-factor call at 2520 dates x 5000 stocks x K = 42 is
        4.2 GB, the ten styles alone 1.0 GB."""
        from ..ops import pure_factor as pf
        args = self._panel_args()
        P, K = self.panel.P, self.K
        if isinstance(factors, str):
            named = {"country": [0], "industries": list(range(1, 1 + P)),
                     "styles": list(range(1 + P, K)), "all": None}
            if factors not in named:
                raise ValueError(f"factors must be an index list or one of {sorted(named)}, got "
                                 f"{factors!r}")
            factors = named[factors]
        return pf.pure_factor_weights(*args, self.estimator_cov().C, factors)

    # --------------------------------------------------------------- factor evaluation
    def _eval_inputs(self, signals, universe):
        p = self.panel
        x = p.styles if signals is None else signals.to(self.device)
        if x.dim() != 3 or x.shape[0] != p.D or x.shape[2] != p.N:
            raise ValueError(f"signals must be [D_loc, S, N] = [{p.D}, S, {p.N}], got "
                             f"{tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
        u = p.valid()
        if universe is not None:
            u = u & universe.to(device=self.device, dtype=torch.bool)
        return x, u

    def factor_ic(self, horizons=(1, 5, 20), quantiles: int = 5,
                  signals: torch.Tensor | None = None, universe: torch.Tensor | None = None,
                  start: int = 0) -> FactorEval:
        """Per-date IC, rank IC and quantile-bucket forward returns (:mod:`ops.factor_eval`) of
        ``signals`` [D_loc, S, N] (default: the panel's raw styles; IC and ranks are invariant to
        the per-date z-scoring) against the compounded forward returns over ``horizons`` dates,
        ``panel.ret[d]`` being the first of them.  The universe is ``panel.valid()`` AND the
        optional ``universe`` [D_loc, N].  Needs no :meth:`regress`.

        Collectives: the ``max(h) - 1`` return rows that follow this rank's block
        (:func:`parallel.dist.halo_next_rows`), and one gather each of the ``ic`` / ``rank_ic``
        rows for ``summary``, the :class:`ops.factor_eval.ICSummary` over the global dates >=
        ``start``, which is the same on every rank and for every world size.  The last ``h - 1``
        global dates have no ``h``-date forward return: their n is 0."""
        from ..ops import factor_eval as fe
        hz = [int(h) for h in horizons]
        x, u = self._eval_inputs(signals, universe)
        ret = self.panel.ret.to(torch.float64)
        tail = pdist.halo_next_rows(ret, max(hz) - 1, self.ctx, self.sizes)
        y = fe.forward_returns(ret, hz, tail)
        r = fe.factor_ic(x, y, u, quantiles)
        s0 = max(0, int(start) - self.T_hist)
        summ = EvalSummary(*(fe.ic_summary(pdist.all_gather_rows(v.contiguous(), self.ctx,
                                                                 self.sizes), s0)
                             for v in (r.ic, r.rank_ic)))
        spread = r.q_ret[..., -1] - r.q_ret[..., 0] if quantiles > 0 else None
        return FactorEval(r.n, r.ic, r.rank_ic, r.q_ret, r.q_count, spread, summ)

    def rank_autocorr(self, lag: int = 1, signals: torch.Tensor | None = None,
                      universe: torch.Tensor | None = None) -> torch.Tensor:
        """[D_loc, S] Spearman correlation of ``signals[d]`` with ``signals[d - lag]`` (default:
        the panel's raw styles) over the stocks of date d's universe (``panel.valid()`` AND
        ``universe``) with both values finite; NaN on the first ``lag`` global dates.  One
        collective: the ``lag`` signal rows that precede this rank's block."""
        from ..ops import factor_eval as fe
        if lag < 1:
            raise ValueError(f"lag must be >= 1, got {lag}")
        x, u = self._eval_inputs(signals, universe)
        D, S, N = x.shape
        xf = x.reshape(D, S * N)
        halo = pdist.halo_prev_rows(xf, lag, self.ctx, self.sizes)
        prev = torch.cat([halo, xf])[:D].reshape(D, S, N).to(torch.float64)
        return fe.factor_ic(x, prev, u, 0, paired=True).rank_ic

    # --------------------------------------------------------------- pandas views
    def factor_returns_frame(self):
        import pandas as pd
        F = pdist.gather_to_root(self.factor_ret, self.ctx)
        if F is None:
            return None
        dates = self._global_dates()
        return pd.DataFrame(F.cpu().numpy(), index=pd.DatetimeIndex(dates), columns=self.panel.factor_names)

    def _global_dates(self):
        d = self.panel.dates
        if self.ctx.enabled:
            import torch.distributed as dist
            objs = [None] * self.ctx.world
            dist.all_gather_object(objs, np.asarray(d))
            d = np.concatenate(objs)
        return d


def eigenfactor_z(cov: torch.Tensor, fwd: torch.Tensor, predlen: int) -> torch.Tensor:
    """z-scores [n, K] of the eigen-factor portfolios of ``cov`` [n, K, K] (utils.py:103-110):
    U / colsum(U), sigma = sqrt(predlen diag(U^T cov U)), realised = U^T (prod(1 + f) - 1) over
    the next predlen dates.  ``fwd`` [n + predlen - 1, K] holds the factor returns of the
    dates after cov's first date."""
    cov = cov.double()
    n = cov.shape[0]
    w, U = eigen.eigh(cov)
    U = U / U.sum(-2, keepdim=True)
    sig = torch.sqrt(predlen * torch.einsum("dki,dkl,dli->di", U, cov, U))
    growth = (fwd.double()[:n + predlen - 1] + 1.0).unfold(0, predlen, 1).prod(-1) - 1.0  # [n, K]
    r = torch.einsum("dki,dk->di", U, growth)
    return r / sig


def eigenfactor_bias_stat(cov: torch.Tensor, ret: torch.Tensor, predlen: int = 1) -> torch.Tensor:
    """Bias statistic of eigen-factor portfolios (``utils.eigenfactor_bias_stat``, utils.py:97-117).

    For date i: eigen-portfolios U / colsum(U) of cov[i]; forecast sigma = sqrt(predlen *
    diag(U^T cov U)); realised = U^T (prod(1 + f[i+1 : i+1+predlen]) - 1); z = realised/sigma.
    Returns std over dates (ddof 0) per eigenfactor; dates with NaN covariances are skipped (the
    reference's bare ``except: pass``).  Eigenfactors ordered by descending variance.
    """
    cov = cov.double()
    ret = ret.double()
    n = cov.shape[0] - predlen
    if n <= 0:
        return torch.full((cov.shape[-1],), float("nan"), dtype=torch.float64)
    z = eigenfactor_z(cov[:n], ret[1:n + predlen], predlen)
    ok = torch.isfinite(z).all(-1)
    z = z[ok]
    return z.std(0, unbiased=False)
