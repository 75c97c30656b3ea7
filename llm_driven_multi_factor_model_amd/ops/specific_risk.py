"""Specific-risk model in the USE4 / CNE5 style: exponentially weighted, Newey-West corrected
trailing volatility of the specific returns, and the cross-sectional bias statistic behind the
specific volatility-regime multiplier (:meth:`RiskModel.specific_risk_use4`).

The reference stops at the never-called ``bayes_shrink`` (``mfm/utils.py:153-168``); the weights
and lag semantics here are those of its factor-side ``Newey_West`` (``mfm/utils.py``): weight
``0.5 ** (age / half_life)``, a lag product carries the weight of its newer row, Bartlett
coefficients ``1 - l / (lags + 1)``.

``ewnw_vol`` for local date t and stock n, over ``ext = cat([halo, e])`` with row j = 0 the date
itself and j = window - 1 the oldest row of its window::

    w_j  = 0.5 ** (j / half_life)                 (float64 table built once on the host)
    S_w  = sum_j w_j,  mean = sum_j w_j e_j / S_w (finite rows only)
    d_j  = e_j - mean                             (0 for a NaN / infinite row)
    C_0  = sum_j w_j d_j^2 / S_w
    C_l  = sum_j w_j d_j d_{j+l} / S_w            (pairs inside the window, l = 1..lags)
    v    = C_0 + sum_l 2 (1 - l / (lags + 1)) C_l;   v <= 0 -> C_0;   vol = sqrt(v)

NaN below ``max(1, min_periods)`` finite rows.  Both paths sum newest row first with one
rounding per operation: the HIP kernel (``csrc/specific_risk.hip``) agrees with the CPU path to
an ulp, and on either path a date shard that holds its halo returns the bits of the whole series.

GPU limits: ``lags <= MAX_LAGS_GPU`` (5) and ``window <= MAX_WINDOW_GPU`` (1024); beyond them
``ewnw_vol`` raises ``ValueError`` before any launch.  The CPU path takes any value.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native

_native.register("mfa_ewnw_vol", [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
_native.register("mfa_spec_bias2", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p])
_native.register("mfa_spec_bias2_f64", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p])

MAX_LAGS_GPU = 5       # template instantiations of ewnw_vol_kernel
MAX_WINDOW_GPU = 1024  # its LDS weight table

_tables: dict = {}


def ew_weights(window: int, half_life: float, device=None) -> torch.Tensor:
    """[window] float64 ``0.5 ** (j / half_life)``, j = 0 the newest row; ``half_life = inf``
    gives exactly 1.  Computed on the host (the CPU path and the kernel read the same numbers)
    and kept per (window, half_life, device)."""
    hl = float(half_life)
    if not hl > 0.0:
        raise ValueError(f"half_life must be > 0 (inf allowed), got {half_life}")
    dev = torch.device(device or "cpu")
    key = (int(window), hl, dev.type, dev.index)
    w = _tables.get(key)
    if w is None:
        w = torch.tensor([0.5 ** (j / hl) for j in range(window)], dtype=torch.float64).to(dev)
        if len(_tables) >= 64:
            _tables.clear()
        _tables[key] = w
    return w


def ewnw_vol(halo: torch.Tensor, e: torch.Tensor, window: int, half_life: float, lags: int = 0,
             min_periods: int = 1) -> torch.Tensor:
    """[D, N] float64 trailing EW Newey-West specific volatility (module docstring) over the
    ``window`` rows ending at each date of ``cat([halo, e])``; ``halo`` = the window - 1
    preceding rows, NaN where none."""
    D, N = e.shape
    window, lags = int(window), int(lags)
    h = window - 1
    if window < 1 or lags < 0:
        raise ValueError(f"need window >= 1 and lags >= 0, got {window}, {lags}")
    if halo.shape != (h, N):
        raise ValueError(f"halo must be [{h}, {N}], got {tuple(halo.shape)}")
    if not e.is_cuda:
        return _ewnw_vol_cpu(halo.double(), e.double(), window,
                             ew_weights(window, half_life).tolist(), lags, min_periods)
    if lags > MAX_LAGS_GPU:
        raise ValueError(f"ewnw_vol on the GPU supports lags <= {MAX_LAGS_GPU}, got {lags}")
    if window > MAX_WINDOW_GPU:
        raise ValueError(f"ewnw_vol on the GPU supports window <= {MAX_WINDOW_GPU}, got {window}")
    if (D + 5) // 6 > 65535:
        raise ValueError(f"ewnw_vol on the GPU supports at most {6 * 65535} dates per call")
    e = _native.check_device_tensor(e, torch.float64, "e")
    halo = halo.to(device=e.device, dtype=torch.float64).contiguous()
    w = ew_weights(window, half_life, e.device)
    vol = torch.empty(D, N, dtype=torch.float64, device=e.device)
    _native.call("mfa_ewnw_vol", _native.ptr(halo) if h > 0 else None, h, _native.ptr(e), D, N,
                 window, lags, int(min_periods), _native.ptr(w), _native.ptr(vol),
                 _native.stream(e.device))
    return vol


def _ewnw_vol_cpu(halo, e, window, w, lags, min_periods):
    """The definition as tensor loops over the window, newest row first (the order and the
    roundings of the kernel)."""
    D = e.shape[0]
    h = window - 1
    ext = torch.cat([halo, e])
    ok = torch.isfinite(ext)
    zero = torch.zeros((), dtype=torch.float64)
    x = torch.where(ok, ext, zero)
    okd = ok.double()
    cnt = torch.zeros_like(e)
    sw = torch.zeros_like(e)
    s1 = torch.zeros_like(e)
    for j in range(window):
        sl = slice(h - j, h - j + D)
        wf = okd[sl] * w[j]
        cnt += okd[sl]
        sw += wf
        s1 += wf * x[sl]
    mean = s1 / sw
    c = [torch.zeros_like(e) for _ in range(lags + 1)]
    hist: list = []   # u of the rows before (newer than) row j, newest last
    for j in range(window):
        sl = slice(h - j, h - j + D)
        d = torch.where(ok[sl], x[sl] - mean, zero)
        u = d * w[j]
        c[0] += u * d
        for l in range(1, min(lags, j) + 1):
            c[l] += hist[-l] * d
        hist.append(u)
        if len(hist) > lags:
            hist.pop(0)
    c0 = c[0] / sw
    v = c0.clone()
    for l in range(1, lags + 1):
        v = v + (2.0 * (1.0 - l / (lags + 1))) * (c[l] / sw)
    v = torch.where(v > 0, v, c0)
    vol = torch.sqrt(v)
    return torch.where(cnt >= max(1, int(min_periods)), vol, torch.full_like(vol, float("nan")))


def spec_bias2(e: torch.Tensor, sigma: torch.Tensor, cap: torch.Tensor) -> torch.Tensor:
    """[D] float64 cap-weighted cross-sectional bias of the specific forecasts:
    ``sum_n cap_n (e_n / sigma_n)^2 / sum_n cap_n`` over stocks with finite ``e``, finite
    ``sigma > 0`` and finite ``cap > 0``; NaN for a date without one.  ``cap`` keeps the panel's
    storage type (fp32 or fp64) on the GPU path; fixed summation order, no atomics."""
    D, N = e.shape
    if sigma.shape != (D, N) or cap.shape != (D, N):
        raise ValueError(f"sigma and cap must be [D, N] = {(D, N)}, got {tuple(sigma.shape)}, "
                         f"{tuple(cap.shape)}")
    if not e.is_cuda:
        return _spec_bias2_cpu(e.double(), sigma.double(), cap.double())
    e = _native.check_device_tensor(e.double(), torch.float64, "e")
    sigma = _native.check_device_tensor(sigma.double(), torch.float64, "sigma")
    dt = torch.float64 if cap.dtype == torch.float64 else torch.float32
    cap = _native.check_device_tensor(cap.to(dt), dt, "cap")
    out = torch.empty(D, dtype=torch.float64, device=e.device)
    _native.call("mfa_spec_bias2_f64" if dt == torch.float64 else "mfa_spec_bias2",
                 _native.ptr(e), _native.ptr(sigma), _native.ptr(cap), D, N, _native.ptr(out),
                 _native.stream(e.device))
    return out


def _spec_bias2_cpu(e, sigma, cap):
    ok = torch.isfinite(e) & torch.isfinite(sigma) & (sigma > 0) & torch.isfinite(cap) & (cap > 0)
    zero = torch.zeros((), dtype=torch.float64)
    z = torch.where(ok, e, zero) / torch.where(ok, sigma, torch.ones((), dtype=torch.float64))
    c = torch.where(ok, cap, zero)
    num, den = (c * (z * z)).sum(1), c.sum(1)
    return torch.where(den > 0, num / den, torch.full_like(den, float("nan")))
