"""Factor evaluation: per-date information coefficient, rank IC and quantile-bucket returns.

Inputs are signals ``x`` [D, S, N] (float32 or float64), targets ``y`` [D, H, N] (float64) and a
``universe`` [D, N] (bool).  For a triple (d, s, h) the **pair set** is the stocks with
``universe[d, n]`` true and ``x[d, s, n]``, ``y[d, h, n]`` finite (NaN and +-inf are invalid); it
has ``n`` members, and everything about a triple depends on that triple's data only.

* ``ic``: Pearson correlation over the pair set: the fp64 means first, then ``Sxy / sqrt(Sxx *
  Syy)`` of the deviations; NaN when ``n < 2`` or ``Sxx * Syy`` is not > 0.
* ``rank_ic``: the same formula on the average ranks within the pair set (1..n, tied values share
  the mean of their positions as ``scipy.stats.rankdata(method="average")``, -0.0 ties with
  +0.0).  The deviations ``r - (n + 1) / 2`` are half-integers, so for n <= 8192 their products
  and sums are exact in fp64 in any order and ``rank_ic`` carries three roundings.
* quantile buckets, ``G`` groups by the signal: group = the number of inner edges ``e_1 ..
  e_{G-1}`` strictly below the value, the edges being ``np.quantile(values of the pair set,
  linspace(0, 1, G + 1))`` (method "linear") in numpy's own arithmetic on the float64 values
  (as :func:`..xs_reduce.bayes_shrink`).  On tie-free data this is ``pd.qcut(x, G,
  labels=False)``; tied values share a group.  ``q_ret`` is the equal-weighted mean of ``y`` over
  the group (NaN for an empty group), ``q_count`` its size.

CPU tensors take the float64 torch transcription below (any N; also the tests' oracle); device
tensors run the kernels of ``csrc/factor_eval.hip``, for N <= 8192, H <= 8 and G <= 32
(``ValueError`` before any launch).  :func:`forward_returns` and :func:`ic_summary` are small
torch code with a fixed order on either device.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Sequence

import torch

from .. import _native

MAX_N, MAX_H, MAX_G = 8192, 8, 32
_CPU_CHUNK = 1 << 22   # elements of one [dates, S, H, N] block of the CPU path

_vp, _i = C.c_void_p, C.c_int
_native.register("mfa_factor_ic", [_vp] * 3 + [_i] * 6 + [_vp] * 6)
_native.register("mfa_factor_ic_f64", [_vp] * 3 + [_i] * 6 + [_vp] * 6)
_native.register("mfa_xs_rank", [_vp, _vp, _i, _i, _i, _vp, _vp])
_native.register("mfa_xs_rank_f64", [_vp, _vp, _i, _i, _i, _vp, _vp])


class FactorIC(NamedTuple):
    """:func:`factor_ic`: ``n`` int32, ``ic`` / ``rank_ic`` float64 [D, S, H]; ``q_ret`` float64
    and ``q_count`` int32 [D, S, H, G] (G = 0: empty).  ``paired``: without the H axis."""
    n: torch.Tensor
    ic: torch.Tensor
    rank_ic: torch.Tensor
    q_ret: torch.Tensor
    q_count: torch.Tensor


class ICSummary(NamedTuple):
    """:func:`ic_summary` over the dates with a finite value: ``mean``, ``std`` (ddof 1),
    ``icir = mean / std``, ``t = icir sqrt(n_dates)``, ``hit`` (share > 0) float64 and
    ``n_dates`` int64, each of the value's shape without its date axis."""
    mean: torch.Tensor
    std: torch.Tensor
    icir: torch.Tensor
    t: torch.Tensor
    hit: torch.Tensor
    n_dates: torch.Tensor


# ------------------------------------------------------------------ float64 torch transcription
def _sorted_ranks(v: torch.Tensor, m: torch.Tensor):
    """Rows ``v`` [..., N] float64 with member mask ``m``: (sorted keys with +inf for the others,
    average ranks [..., N] in the original order: garbage outside ``m``)."""
    N = v.shape[-1]
    key = torch.where(m, v, torch.full((), float("inf"), dtype=v.dtype, device=v.device))
    sk, order = torch.sort(key, dim=-1)
    pos = torch.arange(N, device=v.device).expand(sk.shape)
    new = torch.ones_like(m)
    new[..., 1:] = sk[..., 1:] != sk[..., :-1]
    last = torch.ones_like(m)
    last[..., :-1] = new[..., 1:]
    start = torch.cummax(torch.where(new, pos, torch.zeros_like(pos)), dim=-1).values
    end = torch.cummin(torch.where(last, pos, torch.full_like(pos, N)).flip(-1), dim=-1).values
    r = 0.5 * (start + end.flip(-1)).to(torch.float64) + 1.0
    return sk, torch.empty_like(r).scatter_(-1, order, r)


def _corr(a, b, m, n):
    """``Sab / sqrt(Saa Sbb)`` of the deviations of a, b from their means over ``m``."""
    zero = torch.zeros((), dtype=torch.float64, device=a.device)
    nf = n.to(torch.float64)
    ma = torch.where(m, a, zero).sum(-1) / nf
    mb = torch.where(m, b, zero).sum(-1) / nf
    da = torch.where(m, a - ma[..., None], zero)
    db = torch.where(m, b - mb[..., None], zero)
    den = (da * da).sum(-1) * (db * db).sum(-1)
    ok = (n >= 2) & (den > 0)
    return torch.where(ok, (da * db).sum(-1) / torch.sqrt(torch.where(ok, den, zero + 1.0)),
                       zero + float("nan"))


def _quantile_edges(sk: torch.Tensor, n: torch.Tensor, G: int) -> torch.Tensor:
    """Inner edges [..., G - 1] of rows whose first ``n`` sorted keys ``sk`` are the members:
    np.quantile(..., method="linear"), every operation rounded on its own."""
    g = torch.arange(1, G, dtype=torch.float64, device=sk.device) * (1.0 / G)
    n1 = (n - 1).clamp(min=0)
    pos = n1[..., None].to(torch.float64) * g
    lo = torch.minimum(torch.floor(pos).to(torch.int64), n1[..., None])
    hi = torch.minimum(lo + 1, n1[..., None])
    fr = pos - lo.to(torch.float64)
    a, b = sk.gather(-1, lo), sk.gather(-1, hi)
    ba = b - a
    return torch.where(fr >= 0.5, b - ba * (1.0 - fr), a + ba * fr)


def _factor_ic_block(x, y, u, G, paired):
    """The CPU path on one block of dates: x [D, S, N], y [D, H, N] float64, u [D, N]."""
    if paired:
        xb, yb = x, y                                    # [D, S, N] against [D, S, N]
        m = u[:, None, :] & torch.isfinite(xb) & torch.isfinite(yb)
    else:
        xb, yb = x[:, :, None, :], y[:, None, :, :]      # [D, S, H, N]
        m = u[:, None, None, :] & torch.isfinite(xb) & torch.isfinite(yb)
        xb, yb = xb.expand(m.shape), yb.expand(m.shape)
    n = m.sum(-1)
    ic = _corr(xb, yb, m, n)
    skx, rx = _sorted_ranks(xb, m)
    _, ry = _sorted_ranks(yb, m)
    ric = _corr(rx, ry, m, n)
    q_ret = torch.empty(m.shape[:-1] + (G,), dtype=torch.float64, device=x.device)
    q_cnt = torch.empty(m.shape[:-1] + (G,), dtype=torch.int32, device=x.device)
    if G > 0:
        edges = _quantile_edges(skx, n, G)
        grp = torch.zeros(m.shape, dtype=torch.int64, device=x.device)
        for k in range(G - 1):
            grp += xb > edges[..., k:k + 1]
        zero = torch.zeros((), dtype=torch.float64, device=x.device)
        for g in range(G):
            sel = m & (grp == g)
            c = sel.sum(-1)
            q_cnt[..., g] = c
            q_ret[..., g] = torch.where(c > 0, torch.where(sel, yb, zero).sum(-1) / c,
                                        zero + float("nan"))
    return n.to(torch.int32), ic, ric, q_ret, q_cnt


def _check(x, y, universe, paired):
    if x.dim() != 3 or x.dtype not in (torch.float32, torch.float64):
        raise ValueError("x must be [D, S, N] float32 or float64")
    D, S, N = x.shape
    if y is not None:
        if y.dim() != 3 or y.shape[0] != D or y.shape[2] != N or not y.is_floating_point():
            raise ValueError(f"y must be [D, H, N] with D = {D}, N = {N}, got {tuple(y.shape)}")
        if paired and y.shape[1] != S:
            raise ValueError(f"paired needs H == S, got H = {y.shape[1]}, S = {S}")
    if tuple(universe.shape) != (D, N) or universe.dtype != torch.bool:
        raise ValueError(f"universe must be bool {(D, N)}")
    return D, S, N


def factor_ic(x: torch.Tensor, y: torch.Tensor, universe: torch.Tensor, quantiles: int = 0,
              paired: bool = False) -> FactorIC:
    """IC, rank IC and ``quantiles`` = G bucket returns of every (date, signal, target) triple;
    definitions in the module docstring.  ``paired`` (needs H == S): only the triples (d, s, s)
    are formed and the outputs lose their H axis.

    GPU: one workgroup per (date, signal) sorts (value, stock) pairs of x and of y in LDS,
    forms the average ranks by binary searches for the tie runs and the exact rank sums on the
    fly; every floating sum in a fixed order, no atomics: two calls give the same bits, and a
    triple's result is the same computed alone or inside any call.  N <= 8192, G <= 32, and
    (unless ``paired``, where a workgroup sees one target) H <= 8."""
    D, S, N = _check(x, y, universe, paired)
    H, G = y.shape[1], int(quantiles)
    if G < 0:
        raise ValueError(f"quantiles must be >= 0, got {G}")
    dev = x.device
    y = y.to(device=dev, dtype=torch.float64)
    universe = universe.to(dev)
    lead = (D, S) if paired else (D, S, H)
    if x.is_cuda and (N > MAX_N or G > MAX_G or (H > MAX_H and not paired)):
        raise ValueError(f"factor_ic on the GPU: N <= {MAX_N}, H <= {MAX_H}, quantiles <= {MAX_G}; "
                         f"got N = {N}, H = {H}, quantiles = {G}")
    n = torch.zeros(lead, dtype=torch.int32, device=dev)
    ic = torch.full(lead, float("nan"), dtype=torch.float64, device=dev)
    ric = torch.full(lead, float("nan"), dtype=torch.float64, device=dev)
    q_ret = torch.full(lead + (G,), float("nan"), dtype=torch.float64, device=dev)
    q_cnt = torch.zeros(lead + (G,), dtype=torch.int32, device=dev)
    if n.numel() == 0 or N == 0:
        return FactorIC(n, ic, ric, q_ret, q_cnt)
    if not x.is_cuda:
        xd = x.double()
        step = max(1, _CPU_CHUNK // (S * (1 if paired else H) * N))
        parts = [_factor_ic_block(xd[a:a + step], y[a:a + step], universe[a:a + step], G, paired)
                 for a in range(0, D, step)]
        return FactorIC(*(torch.cat([p[k] for p in parts]) for k in range(5)))
    x, y, universe = x.contiguous(), y.contiguous(), universe.contiguous()
    _native.call("mfa_factor_ic_f64" if x.dtype == torch.float64 else "mfa_factor_ic",
                 _native.ptr(x), _native.ptr(y), _native.ptr(universe), D, S, H, N, G,
                 int(bool(paired)), _native.ptr(n), _native.ptr(ic), _native.ptr(ric),
                 _native.ptr(q_ret), _native.ptr(q_cnt), _native.stream(dev))
    return FactorIC(n, ic, ric, q_ret, q_cnt)


def xs_rank(x: torch.Tensor, universe: torch.Tensor) -> torch.Tensor:
    """Average ranks [D, S, N] float64 of every (date, signal) row of ``x`` within ``universe &
    finite``: 1..n, ties share the mean of their positions (``scipy.stats.rankdata(method=
    "average")``), -0.0 ties with +0.0; NaN outside the set.  GPU: N <= 8192."""
    D, S, N = _check(x, None, universe, False)
    universe = universe.to(x.device)
    if not x.is_cuda:
        xd = x.double()
        if xd.numel() == 0:
            return xd
        m = universe[:, None, :] & torch.isfinite(xd)
        _, r = _sorted_ranks(xd, m)
        return torch.where(m, r, torch.full((), float("nan"), dtype=torch.float64))
    if N > MAX_N:
        raise ValueError(f"xs_rank on the GPU: N <= {MAX_N}, got N = {N}")
    out = torch.empty(D, S, N, dtype=torch.float64, device=x.device)
    if out.numel() == 0:
        return out
    x, universe = x.contiguous(), universe.contiguous()
    _native.call("mfa_xs_rank_f64" if x.dtype == torch.float64 else "mfa_xs_rank",
                 _native.ptr(x), _native.ptr(universe), D, S, N, _native.ptr(out),
                 _native.stream(x.device))
    return out


# ------------------------------------------------------------------ targets and summaries
def forward_returns(ret: torch.Tensor, horizons: Sequence[int],
                    tail: torch.Tensor | None = None) -> torch.Tensor:
    """Compounded forward returns [D, H, N] float64 of ``ret`` [D, N]:

        fwd[d, j] = (1 + ret[d]) (1 + ret[d + 1]) ... (1 + ret[d + h_j - 1]) - 1,

    multiplied in that order in fp64; NaN if any term is non-finite or the window runs past the
    last row.  ``tail`` holds the ``max(h) - 1`` rows that follow the block (None: there are
    none).  ``ret[d]`` being the return that follows the exposures of row d, h = 1 is ``ret`` (to
    the rounding of ``(1 + r) - 1``)."""
    hz = [int(h) for h in horizons]
    if not hz or min(hz) < 1:
        raise ValueError(f"horizons must be positive integers, got {list(horizons)}")
    if ret.dim() != 2:
        raise ValueError("ret must be [D, N]")
    D, N = ret.shape
    hmax = max(hz)
    r = ret.to(torch.float64)
    nan = torch.full((hmax - 1, N), float("nan"), dtype=torch.float64, device=r.device)
    if tail is not None:
        if tuple(tail.shape) != (hmax - 1, N):
            raise ValueError(f"tail must be {(hmax - 1, N)}, got {tuple(tail.shape)}")
        nan = tail.to(device=r.device, dtype=torch.float64)
    ext = torch.cat([r, nan])
    out = torch.empty(D, len(hz), N, dtype=torch.float64, device=r.device)
    acc = bad = None
    for k in range(hmax):
        term = ext[k:k + D]
        b = ~torch.isfinite(term)
        acc = 1.0 + term if acc is None else acc * (1.0 + term)
        bad = b if bad is None else bad | b
        for j, h in enumerate(hz):
            if h == k + 1:
                out[:, j] = torch.where(bad, torch.full_like(acc, float("nan")), acc - 1.0)
    return out


def ic_summary(values: torch.Tensor, start: int = 0) -> ICSummary:
    """Summary over the date axis (the first) of ``values`` [Dg, ...], e.g. the gathered ``ic``
    [Dg, S, H], over the dates >= ``start`` with a finite value."""
    v = values.to(torch.float64)
    t = torch.arange(v.shape[0], device=v.device).reshape((-1,) + (1,) * (v.dim() - 1))
    ok = torch.isfinite(v) & (t >= start)
    zero = torch.zeros((), dtype=torch.float64, device=v.device)
    nan = zero + float("nan")
    n = ok.sum(0)
    nf = n.to(torch.float64)
    mean = torch.where(n > 0, torch.where(ok, v, zero).sum(0) / nf, nan)
    dv = torch.where(ok, v - mean, zero)
    std = torch.where(n > 1, torch.sqrt((dv * dv).sum(0) / (nf - 1.0)), nan)
    icir = mean / std
    hit = torch.where(n > 0, (ok & (v > 0)).sum(0) / nf, nan)
    return ICSummary(mean, std, icir, icir * torch.sqrt(nf), hit, n)
