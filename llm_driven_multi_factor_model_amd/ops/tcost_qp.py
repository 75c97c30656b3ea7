"""Linear trading costs for the box-constrained optimisers: the projection step.

For every date d, with p the holdings before the trade and kappa >= 0 a per-stock cost:

    minimise   1/2 h^T Sigma_d h - q^T h + sum_n kappa_n |h_n - p_n|
    subject to sum_U h_n = budget,   lo_n <= h_n <= hi_n  (n in U),   h_n = 0  (n not in U)

(and, through :mod:`.exposure_qp`, ``(X_d^T h)_k = t_k`` on a set of factors).  The cost is
separable per stock, so the reduced dual of :mod:`.box_qp` keeps its shape and only the inner
per-stock minimiser, the projection, changes.  With ``v = u + gamma a``, ``a = 1 / s^2``:

    h_n(gamma) = clip( median(v_n - kappa_n a_n, p_n, v_n + kappa_n a_n), lo_n, hi_n )

* ``h_n(gamma)`` is nondecreasing and piecewise linear (breakpoints where ``v -+ kappa a`` meets
  lo, hi or p; flat on the no-trade piece h = p), so the exact budget root find carries over;
* ``grad phi = B^T h - nu`` is unchanged;
* the generalised Hessian keeps its form with the free set "strictly inside the bounds and
  ``h_n != p_n``" (``w = a`` there, 0 elsewhere);
* ``phi`` gains ``+ sum kappa |h - p|``: the projection reports ``stats[:, 1] = q^T h - cost``, so
  :func:`.box_qp.box_step` and :func:`.exposure_qp.eq_step` take the result as it is.

:func:`.box_qp.run_trial` calls :func:`tc_project` in place of :func:`.box_qp.box_project` when the
problem carries ``prev`` / ``kappa``.  GPU: ``csrc/tcost_qp.hip``, one workgroup per date; CPU
tensors take the float64 torch transcription below, which is also the tests' oracle.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from .. import _native
from . import box_qp as bq
from . import factor_cov as fc
from .box_qp import ROOT_ITERS, RUNNING, _EPS, _INF, Projection

_vp, _i = C.c_void_p, C.c_int
_native.register("mfa_tc_project", [_vp] * 9 + [_i] * 3 + [_vp] * 6 + [_vp])


class TcProjection(NamedTuple):
    """:func:`tc_project`: ``proj`` (a :class:`.box_qp.Projection` whose ``stats[:, 1]`` is
    ``q^T h - cost``) and ``cost`` [D] = sum over the universe of kappa |h - p|."""
    proj: Projection
    cost: torch.Tensor


def new_tc_projection(D: int, N: int, device) -> TcProjection:
    return TcProjection(bq.new_projection(D, N, device),
                        torch.zeros(D, dtype=torch.float64, device=device))


def _tc_project_torch(u, a, lo, hi, q, bud, p, kap, gam, run):
    D, N = u.shape
    zero = torch.zeros((), dtype=torch.float64, device=u.device)
    part = torch.isfinite(a) & (a > 0) & ~torch.isnan(lo) & ~torch.isnan(hi)
    kbad = ~((kap >= 0) & (kap < _INF))
    inval = (part & (~torch.isfinite(u) | kbad)).any(-1) | ~torch.isfinite(bud)
    a_ = torch.where(part, a, zero)
    u_ = torch.where(part & torch.isfinite(u), u, zero)
    lo_, hi_ = torch.where(part, lo, zero), torch.where(part, hi, zero)
    p_ = torch.where(part & torch.isfinite(p), p, zero)
    k_ = torch.where(part & ~kbad, kap, zero)
    bad = (part & (~(lo_ <= hi_) | (lo_ == _INF) | (hi_ == -_INF))).any(-1)
    slo, shi = lo_.sum(-1), hi_.sum(-1)
    infeas = bad | ~part.any(-1) | (slo > bud) | (shi < bud)
    flag = torch.where(inval, 2, torch.where(infeas, 1, 0)).to(torch.int32)
    # the range of the finite breakpoints: v -+ kappa a = x  at  gamma = (x - u) / a +- kappa
    a1 = torch.where(part, a, zero + 1.0)
    bmin = torch.full_like(bud, _INF)
    bmax = torch.full_like(bud, -_INF)
    for x in (lo_, hi_, p_):
        fin = part & torch.isfinite(x)
        t = (x - u_) / a1
        bmin = torch.minimum(bmin, torch.where(fin, t - k_, zero + _INF).amin(-1))
        bmax = torch.maximum(bmax, torch.where(fin, t + k_, zero - _INF).amax(-1))
    none = ~(bmin <= bmax)
    bmin, bmax = torch.where(none, zero, bmin), torch.where(none, zero, bmax)
    ka = k_ * a_

    def hold(g):
        v = u_ + g[:, None] * a_
        m = torch.minimum(torch.maximum(p_, v - ka), v + ka)
        free = (m > lo_) & (m < hi_) & (m != p_)
        return torch.minimum(torch.maximum(m, lo_), hi_), torch.where(free, a_, zero)

    gam = torch.where(torch.isfinite(gam), gam, zero).clone()
    L = torch.full_like(gam, -_INF)
    H = torch.full_like(gam, _INF)
    act = run & (flag == 0)
    for _ in range(ROOT_ITERS):
        if not bool(act.any()):
            break
        h, w = hold(gam)
        S, T, W = h.sum(-1), h.abs().sum(-1), w.sum(-1)
        s = S - bud
        act = act & ~(s.abs() <= 4.0 * _EPS * (T + bud.abs()))
        L = torch.where(act & (s < 0), gam, L)
        H = torch.where(act & ~(s < 0), gam, H)
        closed = (L > -_INF) & (H < _INF)
        act = act & ~(closed & (H - L <= 4.0 * _EPS * torch.maximum(L.abs(), H.abs())))
        gn = gam - s / W
        newton = (W > 0) & (gn > L) & (gn < H)
        mid = 0.5 * (L + H)
        act = act & ~(~newton & closed & ~((mid > L) & (mid < H)))
        below = torch.minimum(gam, bmin) - torch.maximum(
            torch.ones_like(gam), torch.maximum(gam.abs(), bmin.abs()))
        above = torch.maximum(gam, bmax) + torch.maximum(
            torch.ones_like(gam), torch.maximum(gam.abs(), bmax.abs()))
        gn = torch.where(newton, gn, torch.where(closed, mid, torch.where(L == -_INF, below,
                                                                         above)))
        gam = torch.where(act, gn, gam)
    h, w = hold(gam)
    qz = torch.where(part, torch.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0), zero)
    cost = (k_ * (h - p_).abs()).sum(-1)
    stats = torch.stack([(h * h / a1).sum(-1), (qz * h).sum(-1) - cost, h.abs().sum(-1)], -1)
    return h, w, gam, stats, flag, cost


def _tc_project_into(out: TcProjection, u, a, lo, hi, q, bud, p, kap, status) -> None:
    """The torch projection written into ``out`` as the kernel does: running, feasible dates."""
    pj = out.proj
    run = torch.ones_like(bud, dtype=torch.bool) if status is None else status == RUNNING
    h, w, gam, stats, flag, cost = _tc_project_torch(u, a, lo, hi, q, bud, p, kap, pj.gamma, run)
    keep = run & (flag == 0)
    pj.h.copy_(torch.where(keep[:, None], h, pj.h))
    pj.w.copy_(torch.where(keep[:, None], w, pj.w))
    pj.gamma.copy_(torch.where(keep, gam, pj.gamma))
    pj.stats.copy_(torch.where(keep[:, None], stats, pj.stats))
    pj.flag.copy_(torch.where(run, flag, pj.flag))
    out.cost.copy_(torch.where(keep, cost, out.cost))


def tc_project(u, a, lo, hi, budget, p, kappa, q=None, gamma0=None, status=None, *, out=None,
               stream_rows: bool = False) -> TcProjection:
    """The projection step with linear trading costs for every date: the root ``gamma`` of
    ``sum_U h_n(gamma) = budget`` with ``h_n(gamma) = clip(median(v_n - kappa_n a_n, p_n, v_n +
    kappa_n a_n), lo_n, hi_n)``, ``v = u + gamma a``, and ``h`` at that root.

    Arguments as :func:`.box_qp.box_project`, plus ``p`` [D, N] (the holdings before the trade;
    a non-finite entry is 0, a name not held before) and ``kappa`` [D, N] (the cost per unit
    traded, finite and >= 0 on the universe).  A stock outside the universe gets h = 0 and adds
    nothing to ``cost``.  ``flag`` as in ``box_project``, and also 2 when a stock of the universe
    has a NaN, negative or infinite kappa (:func:`.box_qp.box_qp` resolves kappa = +inf before it
    gets here).  ``w`` is ``a`` where the median is strictly inside (lo, hi) and differs from p,
    0 elsewhere; ``stats`` = (sum s^2 h^2, q^T h - cost, sum |h|).  Rows of dates whose ``status``
    is not ``RUNNING``, or whose flag is not 0, keep what ``out`` (a previous
    :class:`TcProjection`) held (zeros without it).  With kappa = 0, ``h`` is the ``h`` of
    ``box_project``.  GPU: one workgroup per date; for N <= 5120 the date's rows stay on chip
    (u, a, lo, hi in registers, p and kappa in LDS) and are re-read from L2 above that
    (``stream_rows`` forces the latter); the reductions run in a fixed order and both variants
    use the same operations, so they give the same bits, and so do two calls.
    """
    D, N = u.shape
    dev = u.device
    u, a = fc._f64(u, (D, N), "u"), fc._f64(a, (D, N), "a")
    lo, hi = fc._f64(lo, (D, N), "lo"), fc._f64(hi, (D, N), "hi")
    p, kappa = fc._f64(p, (D, N), "p"), fc._f64(kappa, (D, N), "kappa")
    q = torch.zeros_like(u) if q is None else fc._f64(q, (D, N), "q")
    bud = torch.as_tensor(budget, dtype=torch.float64, device=dev).expand(D).contiguous()
    if out is None:
        out = new_tc_projection(D, N, dev)
    elif out.proj.h.shape != (D, N) or out.proj.h.device != dev or out.cost.shape != (D,) \
            or not all(t.is_contiguous() for t in (*out.proj, out.cost)):
        raise ValueError("out must be a contiguous TcProjection of the same (D, N) and device")
    if status is not None and (status.shape != (D,) or status.dtype != torch.int32
                               or status.device != dev):
        raise ValueError("status must be an int32 [D] tensor on the same device")
    pj = out.proj
    if gamma0 is not None:
        pj.gamma.copy_(gamma0)
    if D == 0:
        return out
    if not u.is_cuda:
        _tc_project_into(out, u, a, lo, hi, q, bud, p, kappa, status)
        return out
    if N <= 0:
        raise ValueError("tc_project needs N >= 1")
    _native.call("mfa_tc_project", _native.ptr(u), _native.ptr(a), _native.ptr(lo),
                 _native.ptr(hi), _native.ptr(q), _native.ptr(p), _native.ptr(kappa),
                 _native.ptr(bud), _native.ptr(status), D, N, 1 if stream_rows else 0,
                 _native.ptr(pj.gamma), _native.ptr(pj.h), _native.ptr(pj.w),
                 _native.ptr(pj.stats), _native.ptr(pj.flag), _native.ptr(out.cost),
                 _native.stream(dev))
    return out
