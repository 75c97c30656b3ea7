"""Portfolio bias test: out-of-sample risk forecasts against realised returns (USE4 practice).

For a set of test portfolios the model's forecast variance of date d is

    factor_var + specific_var = x^T F_fc[d] x + sum_n h_n^2 s_fc[d, n]^2,   x = X_d^T h,

and the standardised return ``z = realised / sqrt(forecast variance)`` has unit standard deviation
over time when the forecasts are right.  :func:`portfolio_forecast` forms the sums for every date
and portfolio in one pass (``csrc/portfolio_batch.hip``); :func:`standardised` gives ``z``;
:func:`bias_stats` the bias statistic (std of z), its rolling version, the mean rolling absolute
deviation (MRAD) and the Q-statistic ``mean(z^2 - ln z^2)``.

Test set ``T_d``: stocks that enter the regression (:func:`..cross_section.valid_mask`) with a
finite ``spec_vol[d, n] > 0`` and, optionally, the caller's ``universe`` bit.  A position outside
``T_d``, or with a non-finite weight, is dropped from every sum, so the forecast and the realised
return describe the same holdings; ``held / gross`` says how much of the portfolio that is.
Inputs are row-aligned: shifting the forecasts by one date is the caller's job
(:meth:`RiskModel.bias_test` does it).  CPU tensors take the float64 torch transcription (any
K; also the tests' oracle); device tensors run the HIP kernel, for K = 1 + P + Q <= 64 and
Q <= 16 styles.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from .. import _native
from . import factor_cov as fcov
from .cross_section import valid_mask

_vp, _i, _ll = C.c_void_p, C.c_int, C.c_longlong
_SIG = [_vp] * 6 + [_ll] + [_vp] * 3 + [_i] * 5 + [_vp] * 7
_native.register("mfa_portfolio_batch", _SIG)
_native.register("mfa_portfolio_batch_f64", _SIG)


class PortfolioForecast(NamedTuple):
    """:func:`portfolio_forecast`: float64 [D, B] sums over the test set (``gross``: over every
    finite weight); ``exposure`` [D, B, K] or None."""
    factor_var: torch.Tensor
    specific_var: torch.Tensor
    realised: torch.Tensor
    held: torch.Tensor
    gross: torch.Tensor
    exposure: torch.Tensor | None


class BiasStats(NamedTuple):
    """:func:`bias_stats`: ``bias`` / ``n_obs`` / ``q_stat`` [B], ``rolling_bias`` [D_loc, B],
    ``mrad`` [D_loc], ``mrad_mean`` scalar."""
    bias: torch.Tensor
    n_obs: torch.Tensor
    q_stat: torch.Tensor
    rolling_bias: torch.Tensor
    mrad: torch.Tensor
    mrad_mean: torch.Tensor


class BiasTest(NamedTuple):
    """:meth:`RiskModel.bias_test`: ``z`` / ``forecast_vol`` / ``realised`` / ``coverage``
    [D_loc, B] and the :class:`BiasStats` over the global dates."""
    z: torch.Tensor
    forecast_vol: torch.Tensor
    realised: torch.Tensor
    coverage: torch.Tensor
    stats: BiasStats


def _weights3(H: torch.Tensor, D: int, N: int, per_date: bool, device) -> torch.Tensor:
    """``H`` as float64 [B, N] (static) or [D, B, N] (per date)."""
    H = H.to(device=device, dtype=torch.float64)
    if per_date:
        if H.dim() == 2:
            H = H[:, None, :]
        if H.dim() != 3 or H.shape[0] != D or H.shape[2] != N:
            raise ValueError(f"H must be [D, N] or [D, B, N] with (D, N) = {(D, N)}, got "
                             f"{tuple(H.shape)}")
    else:
        if H.dim() == 1:
            H = H[None, :]
        if H.dim() != 2 or H.shape[1] != N:
            raise ValueError(f"H must be [N] or [B, N] with N = {N}, got {tuple(H.shape)}")
    return H.contiguous()


def _forecast_reference(X, cap, ret, ind, stats, P, H, F, s, universe, return_exposure):
    """Dense float64 transcription (O(D B N) memory)."""
    D, Q, N = X.shape
    zero = torch.zeros((), dtype=torch.float64)
    m = valid_mask(X, cap, ret, ind, P) & torch.isfinite(s) & (s > 0)
    if universe is not None:
        m = m & universe
    Xd = fcov.design_matrix(X, cap, ret, ind, torch.nan_to_num(stats), P, m)   # [D, N, K]
    hz = torch.where(torch.isfinite(H), H, zero)
    hz = hz if hz.dim() == 3 else hz[None].expand(D, -1, -1)
    hm = torch.where(m[:, None, :], hz, zero)                                   # [D, B, N]
    x = torch.einsum("dbn,dnk->dbk", hm, Xd)
    s2 = torch.where(m, s * s, zero)
    r = torch.where(m, ret.double(), zero)
    spec = torch.einsum("dbn,dn->db", hm * hm, s2)
    real = torch.einsum("dbn,dn->db", hm, r)
    fv = torch.full_like(real, float("nan"))
    bad_stats = ~fcov._stats_ok(stats, Q) | ~(stats[:, Q] > 0)
    if F is not None:
        fv = torch.einsum("dbk,dkl,dbl->db", x, torch.nan_to_num(F), x)
        fv[~torch.isfinite(F).all(-1).all(-1) | bad_stats] = float("nan")
    x[bad_stats] = float("nan")
    return PortfolioForecast(fv, spec, real, hm.abs().sum(-1), hz.abs().sum(-1),
                             x if return_exposure else None)


def portfolio_forecast(X, cap, ret, ind, stats, P, H, F, spec_vol, *, per_date: bool = False,
                       universe=None, return_exposure: bool = False) -> PortfolioForecast:
    """Forecast variance and realised return of every portfolio on every date.

    ``X`` [D, Q, N], ``cap`` / ``ret`` [D, N], ``ind`` [D, N] int16 (None when P == 0) and
    ``stats`` [D, Q+2] are the regression's panel and :attr:`XsResult.stats`.  ``H``: weights held
    on every date, [N] or [B, N] (read in place on the GPU, never expanded over dates); with
    ``per_date`` [D, N] or [D, B, N].  ``F`` [D, K, K] factor-covariance forecasts (None: no
    factor variance, NaN), ``spec_vol`` [N] or [D, N] specific-volatility forecasts, ``universe``
    an optional [D, N] bool mask.  A date whose ``F`` is not finite gets NaN ``factor_var``, one
    whose ``stats`` row is not finite (or whose pooled sigma is not > 0) NaN ``factor_var`` and
    ``exposure``; the other sums are still formed.  GPU: K <= 64 and Q <= 16 (``ValueError``); one launch, bitwise reproducible,
    and the value of (d, b) depends on row b and date d alone."""
    D, Q, N = X.shape
    K = 1 + P + Q
    fcov._check_limits(X, P)
    dev = X.device
    H = _weights3(H, D, N, per_date, dev)
    B = H.shape[-2]
    stats = fcov._f64(stats, (D, Q + 2), "stats")
    s = spec_vol.to(device=dev, dtype=torch.float64)
    if s.dim() == 1:
        s = s[None, :].expand(D, -1)
    s = fcov._f64(s, (D, N), "spec_vol")
    if F is not None:
        F = fcov._f64(F.to(dev), (D, K, K), "F")
    if universe is not None:
        universe = universe.to(device=dev, dtype=torch.bool)
        if tuple(universe.shape) != (D, N):
            raise ValueError(f"universe must be {(D, N)}, got {tuple(universe.shape)}")
        universe = universe.contiguous()
    if not X.is_cuda:
        return _forecast_reference(X, cap, ret, ind, stats, P, H, F, s, universe,
                                   return_exposure)
    dt, X, cap, ret, ind = fcov._panel_args(X, cap, ret, ind, P)
    out = torch.empty(5, D, B, dtype=torch.float64, device=dev)
    expo = torch.empty(D, B, K, dtype=torch.float64, device=dev) if return_exposure else None
    if D > 0 and B > 0:
        uni = universe.view(torch.uint8) if universe is not None else None
        _native.call("mfa_portfolio_batch_f64" if dt == torch.float64 else "mfa_portfolio_batch",
                     _native.ptr(X), _native.ptr(cap), _native.ptr(ret), _native.ptr(ind),
                     _native.ptr(stats), _native.ptr(H), B * N if per_date else 0,
                     _native.ptr(s), _native.ptr(F), _native.ptr(uni), D, N, P, Q, B,
                     *(_native.ptr(out[i]) for i in range(5)), _native.ptr(expo),
                     _native.stream(dev))
    return PortfolioForecast(out[0], out[1], out[2], out[3], out[4], expo)


def standardised(fc: PortfolioForecast) -> torch.Tensor:
    """``z = realised / sqrt(factor_var + specific_var)`` [D, B]; NaN where the forecast variance
    is not finite or <= 0."""
    var = fc.factor_var + fc.specific_var
    ok = torch.isfinite(var) & (var > 0)
    nan = torch.full_like(var, float("nan"))
    return torch.where(ok, fc.realised / torch.sqrt(torch.where(ok, var, torch.ones_like(var))),
                       nan)


def _rolling_std(halo: torch.Tensor, z: torch.Tensor, window: int, min_periods: int):
    """ddof-0 std of the finite values in the ``window`` rows ending at each row of ``z``
    (``halo``: the window - 1 rows before it).  GPU: :func:`..attribution.trailing_vol`; CPU: the
    same sums in the same order (newest date first) as ``RiskModel.specific_vol_series``."""
    D, h = z.shape[0], window - 1
    if tuple(halo.shape) != (h,) + tuple(z.shape[1:]):
        raise ValueError(f"halo must be [{h}, {z.shape[1]}], got {tuple(halo.shape)}")
    if z.is_cuda:
        from .attribution import trailing_vol
        return trailing_vol(halo, z.contiguous(), window, min_periods)
    ext = torch.cat([halo.to(z), z])
    ok = torch.isfinite(ext)
    x = torch.where(ok, ext, torch.zeros((), dtype=z.dtype))
    okd = ok.to(z.dtype)
    n, s1, s2 = torch.zeros_like(z), torch.zeros_like(z), torch.zeros_like(z)
    for j in range(window):
        sl = slice(h - j, h - j + D)
        n += okd[sl]
        s1 += x[sl]
        s2 += x[sl] * x[sl]
    mean = s1 / n
    vol = torch.sqrt(torch.clamp(s2 / n - mean * mean, min=0.0))
    return torch.where(n >= max(1, min_periods), vol, torch.full_like(vol, float("nan")))


def _nanmean(x: torch.Tensor, dim=None) -> torch.Tensor:
    ok = torch.isfinite(x)
    x = torch.where(ok, x, torch.zeros((), dtype=x.dtype, device=x.device))
    if dim is None:
        return x.sum() / ok.sum()
    return x.sum(dim) / ok.sum(dim)


def bias_stats(z_local: torch.Tensor, halo: torch.Tensor, z_global: torch.Tensor,
               window: int = 252, min_periods: int = 63) -> BiasStats:
    """Bias statistics of standardised returns.  ``z_local`` [D_loc, B] are this rank's dates,
    ``halo`` [window - 1, B] the rows before them (NaN where none) and ``z_global`` [T, B] every
    date's rows (``z_local`` itself in one process); non-finite z are skipped everywhere.

    ``bias`` [B]: ddof-0 std of each portfolio's z (mean removed); ``n_obs`` [B] their number;
    ``q_stat`` [B]: mean of ``z^2 - ln z^2`` over the non-zero z (1 for a perfect forecast);
    ``rolling_bias`` [D_loc, B]: the std over the ``window`` dates ending at each date, NaN
    below ``min_periods`` values; ``mrad`` [D_loc]: mean over portfolios of ``|rolling_bias -
    1|``; ``mrad_mean``: the same mean over all dates of ``z_global`` and all portfolios.  The
    statistics of ``z_global`` are the same on every rank."""
    z_local, z_global = z_local.to(torch.float64), z_global.to(torch.float64)
    zero = torch.zeros((), dtype=torch.float64, device=z_global.device)
    fin = torch.isfinite(z_global)
    n = fin.sum(0)
    mean = torch.where(fin, z_global, zero).sum(0) / n
    dev = torch.where(fin, z_global - mean, zero)
    bias = torch.sqrt((dev * dev).sum(0) / n)
    nz = fin & (z_global != 0)
    z2 = torch.where(nz, z_global * z_global, torch.ones_like(z_global))
    q = torch.where(nz, z2 - torch.log(z2), zero).sum(0) / nz.sum(0)
    rb = _rolling_std(halo, z_local, window, min_periods)
    if z_global is z_local:
        rb_all = rb
    else:
        nan = torch.full((window - 1, z_global.shape[1]), float("nan"), dtype=torch.float64,
                         device=z_global.device)
        rb_all = _rolling_std(nan, z_global, window, min_periods)
    return BiasStats(bias=bias, n_obs=n, q_stat=q, rolling_bias=rb,
                     mrad=_nanmean((rb - 1.0).abs(), 1), mrad_mean=_nanmean((rb_all - 1.0).abs()))
