"""Box-constrained portfolio optimisation on the factor-structured asset covariance.

For every date d, over the universe ``U_d`` of :func:`.factor_cov.universe_mask`:

    minimise   1/2 h^T Sigma_d h - q^T h
    subject to sum_U h_n = budget,   lo_n <= h_n <= hi_n  (n in U),   h_n = 0  (n not in U)

with ``Sigma_d = X_d F_d X_d^T + diag(s_d^2)`` (``q = 0``: minimum variance; ``q = Sigma h_b``:
minimum tracking error to ``h_b``; ``q = alpha / lambda + Sigma h_b``: mean-variance tilt).

Semismooth Newton on the reduced dual.  With ``a = 1 / s^2``, ``F = R R^T`` as in
:func:`.factor_cov.woodbury_coef`, ``B = X R`` and ``nu`` in R^K the multiplier of ``y = B^T h``:

    phi(nu) = 1/2 sum s_n^2 h_n^2 - q^T h + nu^T B^T h - 1/2 |nu|^2        (maximised)
    u_n = a_n (q_n - x_n . R nu),    h_n = clip(u_n + gamma a_n, lo_n, hi_n),
    gamma = root of  s(gamma) = sum_U h_n(gamma) - budget   (nondecreasing, piecewise linear),
    grad phi = B^T h - nu,   -H a generalised Hessian,   H = I + R^T (G_f - g_f g_f^T / sigma_f) R

where ``G_f = X^T diag(a 1_free) X`` is the Gram over the free set (strictly inside the bounds);
the country column of X is 1, so ``g_f`` is column 0 of ``G_f`` and ``sigma_f = G_f[0, 0]``.
``H >= I``, so its Cholesky never fails.  Each trial ``nu`` ("pass") re-solves ``gamma``, so every
iterate is primal feasible; the step ``H dn = grad phi`` is followed by Armijo backtracking on
``phi``: a rejected step is cut to the maximiser of the parabola through ``phi(0)``, ``phi'(0)``
and ``phi(step)``, kept in [0.1, 0.5] of the step (plain halving left three times as many dates
unfinished after 32 passes on model covariances of short history).  A date stops when

    max |grad phi| <= tol * max(1, sum |h|) * sqrt(max_k F_kk)

(``sqrt(F_kk)`` is the norm of ``B``'s row for a stock with unit exposure to factor k alone; it
stands in for ``max |B|``, has the same units and needs no extra pass over the panel).

One pass on the GPU is five launches with no host synchronisation: ``factor_apply`` (u),
``box_project`` (gamma, h, w), ``factor_gram`` (G_f), ``factor_xty`` (X^T h) and ``box_step``
(``csrc/box_qp.hip``); K = 1 + P + Q <= 64 and Q <= 16 as in :mod:`.factor_cov`.  CPU tensors take
the float64 torch transcription below (dense ``X_d``; any K), which is also the tests' oracle.

With ``prev`` / ``tcost`` the objective gains the linear trading cost ``sum_n kappa_n |h_n -
p_n|``; only the projection changes (:mod:`.tcost_qp`), the step is the one below.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from .. import _native
from . import eigen
from . import factor_cov as fc

OK, MAX_PASSES, INFEASIBLE, INVALID = 0, 1, 2, 3
RUNNING = -1           # internal: a date that still iterates
ARMIJO = 1e-4
ROOT_ITERS = 100       # cap of the inner root find (kRootIters in csrc/box_qp.hip)
_EPS = 2.220446049250313e-16
_INF = float("inf")

_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
_native.register("mfa_box_project", [_vp] * 7 + [_i] * 3 + [_vp] * 6)
_native.register("mfa_box_step", [_vp] * 6 + [_d, _i, _i] + [_vp] * 9)


class BoxQP(NamedTuple):
    """:func:`box_qp`: ``weights`` [D, N], ``gamma`` / ``variance`` [D] (float64), ``passes`` /
    ``status`` [D] (int32; ``OK``, ``MAX_PASSES``, ``INFEASIBLE``, ``INVALID``)."""
    weights: torch.Tensor
    gamma: torch.Tensor
    variance: torch.Tensor
    passes: torch.Tensor
    status: torch.Tensor


class BoxQPCost(NamedTuple):
    """:func:`box_qp` with ``prev`` / ``tcost``: the fields of :class:`BoxQP`, then ``turnover``
    [D] = sum_n |h_n - p_n| over all N stocks (a non-finite p counts as 0, so the forced sale of
    a name that left the universe is counted) and ``cost`` [D], the same sum weighted by kappa
    (a stock with a non-finite kappa counts 0); NaN where the weights are."""
    weights: torch.Tensor
    gamma: torch.Tensor
    variance: torch.Tensor
    passes: torch.Tensor
    status: torch.Tensor
    turnover: torch.Tensor
    cost: torch.Tensor


class Projection(NamedTuple):
    """:func:`box_project`: ``h`` / ``w`` [D, N] (weights; Gram weight ``a`` on the free set, 0
    elsewhere), ``gamma`` [D], ``stats`` [D, 3] = (sum s^2 h^2, q^T h, sum |h|), ``flag`` [D]
    int32 (0 feasible, 1 infeasible, 2 non-finite input)."""
    h: torch.Tensor
    w: torch.Tensor
    gamma: torch.Tensor
    stats: torch.Tensor
    flag: torch.Tensor


class StepState(NamedTuple):
    """Per-date solver state, updated in place by :func:`box_step`: ``nu`` / ``grad`` / ``dn`` /
    ``c`` [D, K]; ``ds`` [D, 4] = (phi, step, variance of the last trial, unused); ``passes`` /
    ``status`` / ``accepted`` [D] int32."""
    nu: torch.Tensor
    grad: torch.Tensor
    dn: torch.Tensor
    c: torch.Tensor
    ds: torch.Tensor
    passes: torch.Tensor
    status: torch.Tensor
    accepted: torch.Tensor

    def clone(self) -> "StepState":
        return StepState(*(t.clone() for t in self))

    def to(self, device) -> "StepState":
        return StepState(*(t.to(device) for t in self))


def new_state(D: int, K: int, device) -> StepState:
    """The state before the first pass: nu = 0, phi = -inf (the first trial is accepted)."""
    z = lambda: torch.zeros(D, K, dtype=torch.float64, device=device)   # noqa: E731
    ds = torch.zeros(D, 4, dtype=torch.float64, device=device)
    ds[:, 0] = -_INF
    ds[:, 1] = 1.0
    zi = lambda: torch.zeros(D, dtype=torch.int32, device=device)       # noqa: E731
    return StepState(z(), z(), z(), z(), ds, zi(), zi() + RUNNING, zi())


def _rows(t, D: int, N: int, device, name: str) -> torch.Tensor:
    """A scalar, [N] or [D, N] as a contiguous float64 [D, N]."""
    t = torch.as_tensor(t, dtype=torch.float64, device=device)
    if t.dim() > 2 or (t.dim() >= 1 and t.shape[-1] != N) or (t.dim() == 2 and t.shape[0] != D):
        raise ValueError(f"{name} must be a scalar, [N] or [D, N] with (D, N) = {(D, N)}, got "
                         f"{tuple(t.shape)}")
    return t.expand(D, N).contiguous()


# --------------------------------------------------------------------------------- projection
def _project_torch(u, a, lo, hi, q, bud, gam, run):
    D, N = u.shape
    zero = torch.zeros((), dtype=torch.float64, device=u.device)
    part = torch.isfinite(a) & (a > 0) & ~torch.isnan(lo) & ~torch.isnan(hi)
    inval = (part & ~torch.isfinite(u)).any(-1) | ~torch.isfinite(bud)
    a_ = torch.where(part, a, zero)
    u_ = torch.where(part & torch.isfinite(u), u, zero)
    lo_, hi_ = torch.where(part, lo, zero), torch.where(part, hi, zero)
    bad = (part & (~(lo_ <= hi_) | (lo_ == _INF) | (hi_ == -_INF))).any(-1)
    slo, shi = lo_.sum(-1), hi_.sum(-1)
    infeas = bad | ~part.any(-1) | (slo > bud) | (shi < bud)
    flag = torch.where(inval, 2, torch.where(infeas, 1, 0)).to(torch.int32)
    a1 = torch.where(part, a, zero + 1.0)
    tl = torch.where(part & torch.isfinite(lo_), (lo_ - u_) / a1, zero + _INF)
    th = torch.where(part & torch.isfinite(hi_), (hi_ - u_) / a1, zero + _INF)
    bmin = torch.minimum(tl.amin(-1), th.amin(-1))
    bmax = torch.maximum(torch.where(tl == _INF, -tl, tl).amax(-1),
                         torch.where(th == _INF, -th, th).amax(-1))
    none = ~(bmin <= bmax)
    bmin, bmax = torch.where(none, zero, bmin), torch.where(none, zero, bmax)

    def clip(g):
        v = u_ + g[:, None] * a_
        return v, torch.minimum(torch.maximum(v, lo_), hi_)

    gam = torch.where(torch.isfinite(gam), gam, zero).clone()
    L = torch.full_like(gam, -_INF)
    H = torch.full_like(gam, _INF)
    act = run & (flag == 0)
    for _ in range(ROOT_ITERS):
        if not bool(act.any()):
            break
        v, h = clip(gam)
        S, T = h.sum(-1), h.abs().sum(-1)
        W = torch.where((v > lo_) & (v < hi_), a_, zero).sum(-1)
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
    v, h = clip(gam)
    w = torch.where((v > lo_) & (v < hi_), a_, zero)
    qz = torch.where(part, torch.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0), zero)
    stats = torch.stack([(h * h / a1).sum(-1), (qz * h).sum(-1), h.abs().sum(-1)], -1)
    return h, w, gam, stats, flag


def box_project(u, a, lo, hi, budget, q=None, gamma0=None, status=None, *, out=None,
                stream_rows: bool = False) -> Projection:
    """Exact projection step of the solver for every date: the root ``gamma`` of
    ``sum_U clip(u_n + gamma a_n, lo_n, hi_n) = budget`` and ``h`` at that root.

    ``u`` / ``a`` / ``lo`` / ``hi`` [D, N] float64 (``a <= 0`` or not finite, or a NaN bound: the
    stock takes no part and gets h = 0; infinite bounds are legal), ``budget`` [D] or a scalar,
    ``q`` [D, N] (only for ``stats``), ``gamma0`` [D] a warm start.  ``flag`` is 1 (infeasible)
    when sum lo > budget, sum hi < budget, lo > hi for a stock of the universe or the universe
    is empty, and 2 when ``u`` or ``budget`` is not finite.  Rows of dates whose ``status`` is
    not ``RUNNING``, or whose flag is not 0, keep what ``out`` (a previous :class:`Projection`)
    held (zeros without it).  GPU: one workgroup per date; the date's four rows stay in
    registers for N <= 5120 and are re-read from L2 above that (``stream_rows`` forces the
    latter); the reductions run in a fixed order, so two calls give the same bits.
    """
    D, N = u.shape
    dev = u.device
    u, a = fc._f64(u, (D, N), "u"), fc._f64(a, (D, N), "a")
    lo, hi = fc._f64(lo, (D, N), "lo"), fc._f64(hi, (D, N), "hi")
    q = torch.zeros_like(u) if q is None else fc._f64(q, (D, N), "q")
    bud = torch.as_tensor(budget, dtype=torch.float64, device=dev).expand(D).contiguous()
    if out is None:
        out = new_projection(D, N, dev)
    elif out.h.shape != (D, N) or out.h.device != dev or not all(t.is_contiguous() for t in out):
        raise ValueError("out must be a contiguous Projection of the same (D, N) and device")
    if status is not None and (status.shape != (D,) or status.dtype != torch.int32
                               or status.device != dev):
        raise ValueError("status must be an int32 [D] tensor on the same device")
    if gamma0 is not None:
        out.gamma.copy_(gamma0)
    if D == 0:
        return out
    if not u.is_cuda:
        _project_into(out, u, a, lo, hi, q, bud, status)
        return out
    if N <= 0:
        raise ValueError("box_project needs N >= 1")
    _native.call("mfa_box_project", _native.ptr(u), _native.ptr(a), _native.ptr(lo),
                 _native.ptr(hi), _native.ptr(q), _native.ptr(bud), _native.ptr(status), D, N,
                 1 if stream_rows else 0, _native.ptr(out.gamma), _native.ptr(out.h),
                 _native.ptr(out.w), _native.ptr(out.stats), _native.ptr(out.flag),
                 _native.stream(dev))
    return out


# --------------------------------------------------------------------------------------- step
def _step_torch(G, lam, U, x, pstats, pflag, st: StepState, tol: float) -> None:
    D, K = x.shape
    dev = x.device
    run = st.status == RUNNING
    eye = torch.eye(K, dtype=torch.float64, device=dev)
    R = U * torch.sqrt(lam.clamp(min=0.0))[:, None, :]
    bad = ~(torch.isfinite(G).all(-1).all(-1) & torch.isfinite(R).all(-1).all(-1)
            & torch.isfinite(x).all(-1))
    bad = bad | ((pflag == 0) & ~torch.isfinite(pstats[:, :2]).all(-1))
    stop = run & ((pflag != 0) | bad)
    st.status[stop] = torch.where(pflag == 1, INFEASIBLE, INVALID).to(torch.int32)[stop]
    st.accepted[stop] = 0
    run = run & ~stop
    Rz, Gz = torch.nan_to_num(R), torch.nan_to_num(G)
    xz, ps = torch.nan_to_num(x), torch.nan_to_num(pstats)
    phi, step = st.ds[:, 0], st.ds[:, 1]
    nut = st.nu + step[:, None] * st.dn
    by = torch.einsum("djk,dj->dk", Rz, xz)
    gt = by - nut
    phit = 0.5 * ps[:, 0] - ps[:, 1] + (nut * by).sum(-1) - 0.5 * (nut * nut).sum(-1)
    gmax = gt.abs().amax(-1)
    gd = (st.grad * st.dn).sum(-1)
    bscale = torch.sqrt((Rz * Rz).sum(-1).amax(-1))
    nonfin = run & ~(torch.isfinite(phit) & torch.isfinite(gmax))
    st.status[nonfin] = INVALID
    st.accepted[nonfin] = 0
    run = run & ~nonfin
    conv = gmax <= tol * ps[:, 2].clamp(min=1.0) * bscale
    acc = conv | (phit >= phi + ARMIJO * step * gd - 4.0 * _EPS * phit.abs())
    A, newton = run & acc, run & acc & ~conv
    if bool(newton.any()):
        Tm = Gz @ Rz
        p = Tm[:, 0, :]
        sigma = Gz[:, 0, 0]
        isg = torch.where(sigma > 0, 1.0 / sigma.clamp(min=1e-300), torch.zeros_like(sigma))
        Hm = eye + Rz.transpose(1, 2) @ Tm - isg[:, None, None] * p[:, :, None] * p[:, None, :]
        Hm = torch.where(newton[:, None, None], Hm, eye)
        Lc, info = torch.linalg.cholesky_ex(Hm)
        fail = newton & (info != 0)
        Lc = torch.where(fail[:, None, None], eye, Lc)
        dn_new = torch.cholesky_solve(gt[..., None], Lc)[..., 0]
        st.status[fail] = INVALID
        st.accepted[fail] = 0
        run, A, newton = run & ~fail, A & ~fail, newton & ~fail
        st.dn[newton] = dn_new[newton]
    # rejected: the maximiser of the parabola through phi(0), phi'(0) and phi(step), kept in
    # [0.1, 0.5] step (plain halving when the parabola has no maximum)
    den = 2.0 * (phi + gd * step - phit)
    cut = torch.where(den > 0, gd * step * step / den.clamp(min=1e-300), 0.5 * step)
    cut = torch.minimum(torch.maximum(torch.nan_to_num(cut, nan=0.0), 0.1 * step), 0.5 * step)
    nstep = torch.where(acc, torch.where(conv, 0.0, 1.0).to(cut.dtype), cut)
    st.nu[A] = nut[A]
    st.grad[A] = gt[A]
    st.ds[:, 0] = torch.where(A, phit, phi)
    st.ds[:, 1] = torch.where(run, nstep, step)
    st.ds[:, 2] = torch.where(run, ps[:, 0] + (by * by).sum(-1), st.ds[:, 2])
    cn = torch.einsum("dik,dk->di", Rz, st.nu + st.ds[:, 1, None] * st.dn)
    st.c[run] = cn[run]
    st.passes[run] += 1
    st.accepted[run] = acc[run].to(torch.int32)
    st.status[run & conv] = OK


def box_step(G, lam, U, x, pstats, pflag, state: StepState, tol: float) -> StepState:
    """One outer step for every running date, in place on ``state``: form ``grad phi`` and
    ``phi`` at the trial, accept it (Armijo) or cut the step; on accept build H from ``G``
    [D, K, K] (the Gram with the free set's weights), factor it and solve for the new direction;
    test convergence; write the next trial's ``c = R (nu + step dn)``.  ``lam`` / ``U`` are the
    eigenpairs of F from :func:`..eigen.eigh`, ``x`` [D, K] = X^T h, ``pstats`` / ``pflag`` come
    from :func:`box_project`.  Finished dates are left untouched; non-finite F, G or stats give
    ``INVALID``.  GPU: K <= 64, one workgroup per date (H and its Cholesky factor in LDS)."""
    D, K = x.shape
    if x.is_cuda and K > fc.MAX_K:
        raise ValueError(f"box_step on the GPU supports K <= {fc.MAX_K}, got K = {K}")
    G, U = fc._f64(G, (D, K, K), "G"), fc._f64(U, (D, K, K), "U")
    lam, x = fc._f64(lam, (D, K), "lam"), fc._f64(x, (D, K), "x")
    if D == 0:
        return state
    if not x.is_cuda:
        _step_torch(G, lam, U, x, pstats, pflag, state, tol)
        return state
    _native.call("mfa_box_step", _native.ptr(G), _native.ptr(lam), _native.ptr(U), _native.ptr(x),
                 _native.ptr(pstats), _native.ptr(pflag), float(tol), D, K,
                 _native.ptr(state.nu), _native.ptr(state.grad), _native.ptr(state.dn),
                 _native.ptr(state.c), _native.ptr(state.ds), _native.ptr(state.passes),
                 _native.ptr(state.status), _native.ptr(state.accepted), _native.stream(x.device))
    return state


# ------------------------------------------------------------------------------------- driver
class Problem(NamedTuple):
    """What every pass of :func:`box_qp` reads: the panel, ``a`` (0 outside the universe), the
    bounds, ``q``, ``budget`` [D] and the eigenpairs of F; with trading costs also ``prev`` and
    ``kappa`` [D, N] (:mod:`.tcost_qp`), None without."""
    panel: tuple
    a: torch.Tensor
    lo: torch.Tensor
    hi: torch.Tensor
    q: torch.Tensor
    budget: torch.Tensor
    lam: torch.Tensor
    U: torch.Tensor
    Xd: torch.Tensor | None    # dense design matrix (torch path only)
    prev: torch.Tensor | None = None
    kappa: torch.Tensor | None = None


def make_problem(X, cap, ret, ind, stats, P, F, spec_vol, q=None, lower=0.0, upper=1.0,
                 budget=1.0, universe=None, dense: bool | None = None, prev=None,
                 tcost=None) -> Problem:
    """The per-call set-up of :func:`box_qp` (same arguments): broadcast bounds and ``q``, ``a``
    masked to the universe, ``eigh(F)``; ``dense`` also builds the design matrix (default: on
    the CPU).  With ``prev`` / ``tcost``: a non-finite prev becomes 0, and a stock with kappa =
    +inf ("do not trade") gets lo = hi = clip(prev, lo, hi) and kappa = 0, so that no infinity
    reaches the projection."""
    D, Q, N = X.shape
    K = 1 + P + Q
    dev = X.device
    dense = (not X.is_cuda) if dense is None else dense
    lo, hi = _rows(lower, D, N, dev, "lower"), _rows(upper, D, N, dev, "upper")
    pv = kap = None
    if tcost is not None:
        pv = torch.nan_to_num(_rows(prev, D, N, dev, "prev"), nan=0.0, posinf=0.0, neginf=0.0)
        kap = _rows(tcost, D, N, dev, "tcost")
        frozen = kap == _INF
        pin = torch.minimum(torch.maximum(pv, lo), hi)
        fix = frozen & (lo <= hi)          # lo > hi stays what it is: infeasible
        lo, hi = torch.where(fix, pin, lo), torch.where(fix, pin, hi)
        kap = torch.where(frozen, torch.zeros_like(kap), kap).contiguous()
    q = _rows(0.0 if q is None else q, D, N, dev, "q")
    bud = torch.as_tensor(budget, dtype=torch.float64, device=dev).expand(D).contiguous()
    a, _ = fc._weights(X, cap, ret, ind, P, spec_vol, universe)
    m = fc.universe_mask(X, cap, ret, ind, P, spec_vol, universe)
    m = m & ~torch.isnan(lo) & ~torch.isnan(hi)
    a = torch.where(m, a, torch.zeros((), dtype=torch.float64, device=dev)).contiguous()
    stats = fc._f64(stats, (D, Q + 2), "stats")
    F = fc._f64(F.to(dev), (D, K, K), "F")
    if D:
        lam, U = eigen.eigh(F)
    else:
        lam, U = F.new_empty(0, K), F.new_empty(0, K, K)
    Xd = fc.design_matrix(X, cap, ret, ind, torch.nan_to_num(stats), P, m) if dense else None
    return Problem((X, cap, ret, ind, stats, P), a, lo, hi, q, bud, lam.contiguous(),
                   U.contiguous(), Xd, pv, kap)


def run_trial(pb: Problem, st: StepState, pj: Projection, *, stream_rows: bool = False):
    """The trial ``c`` of ``st`` for every running date: u, the projection (into ``pj``), and
    ``(G_f, X^T h)``.  On the GPU: four launches (apply, project, Gram, X^T h).  A problem
    with ``prev`` / ``kappa`` takes the projection of :mod:`.tcost_qp`."""
    X, cap, ret, ind, stats, P = pb.panel
    if pb.kappa is not None:
        from . import tcost_qp as tc
        tcp = tc.TcProjection(pj, pj.gamma.new_zeros(pj.gamma.shape))
    if pb.Xd is None:
        u = fc.factor_apply(*pb.panel, pb.a, -pb.a, pb.q[:, None], st.c[:, None, :])[:, 0]
        if pb.kappa is not None:
            tc.tc_project(u, pb.a, pb.lo, pb.hi, pb.budget, pb.prev, pb.kappa, pb.q, None,
                          st.status, out=tcp, stream_rows=stream_rows)
        else:
            box_project(u, pb.a, pb.lo, pb.hi, pb.budget, pb.q, None, st.status, out=pj,
                        stream_rows=stream_rows)
        G = fc.factor_gram(*pb.panel, pj.w)
        x = fc.factor_xty(*pb.panel, pj.h[:, None])[:, 0]
        return G, x
    ok = fc._stats_ok(stats, X.shape[1])
    u = pb.a * (torch.nan_to_num(pb.q, nan=0.0, posinf=0.0, neginf=0.0)
                - torch.einsum("dnk,dk->dn", pb.Xd, st.c))
    u[~ok] = float("nan")
    if pb.kappa is not None:
        tc._tc_project_into(tcp, u, pb.a, pb.lo, pb.hi, pb.q, pb.budget, pb.prev, pb.kappa,
                            st.status)
    else:
        _project_into(pj, u, pb.a, pb.lo, pb.hi, pb.q, pb.budget, st.status)
    G = torch.einsum("dnk,dn,dnl->dkl", pb.Xd, pj.w, pb.Xd)
    G[~ok] = float("nan")
    return G, torch.einsum("dnk,dn->dk", pb.Xd, pj.h)


def run_pass(pb: Problem, st: StepState, pj: Projection, tol: float, *,
             stream_rows: bool = False) -> None:
    """One pass for every running date: :func:`run_trial`, then the step.  On the GPU: five
    launches, no host synchronisation."""
    G, x = run_trial(pb, st, pj, stream_rows=stream_rows)
    if pb.Xd is None:
        box_step(G, pb.lam, pb.U, x, pj.stats, pj.flag, st, tol)
    else:
        _step_torch(G, pb.lam, pb.U, x, pj.stats, pj.flag, st, tol)


def _project_into(pj, u, a, lo, hi, q, bud, status):
    """The torch projection on whatever device ``u`` lives, written into ``pj`` as the kernel
    does: running, feasible dates only."""
    run = torch.ones_like(bud, dtype=torch.bool) if status is None else status == RUNNING
    h, w, gam, stats, flag = _project_torch(u, a, lo, hi, q, bud, pj.gamma, run)
    keep = run & (flag == 0)
    pj.h.copy_(torch.where(keep[:, None], h, pj.h))
    pj.w.copy_(torch.where(keep[:, None], w, pj.w))
    pj.gamma.copy_(torch.where(keep, gam, pj.gamma))
    pj.stats.copy_(torch.where(keep[:, None], stats, pj.stats))
    pj.flag.copy_(torch.where(run, flag, pj.flag))


def check_tcost(prev, tcost) -> None:
    if (prev is None) != (tcost is None):
        raise ValueError("prev and tcost go together: the trading cost is sum tcost |h - prev|, "
                         f"got only {'prev' if tcost is None else 'tcost'}")


def trade_stats(weights, prev, tcost) -> tuple[torch.Tensor, torch.Tensor]:
    """``(turnover, cost)`` [D] of :class:`BoxQPCost` for ``weights`` [D, N]."""
    D, N = weights.shape
    dev = weights.device
    pv = torch.nan_to_num(_rows(prev, D, N, dev, "prev"), nan=0.0, posinf=0.0, neginf=0.0)
    kap = _rows(tcost, D, N, dev, "tcost")
    kap = torch.where(torch.isfinite(kap), kap, torch.zeros_like(kap))
    trade = (weights - pv).abs()
    return trade.sum(-1), (kap * trade).sum(-1)


def new_projection(D: int, N: int, device) -> Projection:
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=device)   # noqa: E731
    return Projection(z(D, N), z(D, N), z(D), z(D, 3),
                      torch.zeros(D, dtype=torch.int32, device=device))


def box_qp(X, cap, ret, ind, stats, P, F, spec_vol, q=None, lower=0.0, upper=1.0, budget=1.0,
           universe=None, tol: float = 1e-10, max_passes: int = 32, check_every: int = 4, *,
           torch_ops: bool = False, stream_rows: bool = False, prev=None,
           tcost=None) -> BoxQP | BoxQPCost:
    """Solve the box-constrained QP of the module docstring for every date.

    Panel arguments, ``F`` [D, K, K], ``spec_vol`` and ``universe`` as in
    :func:`.factor_cov.solve_cov`; ``q`` / ``lower`` / ``upper`` a scalar, [N] or [D, N]
    (infinite bounds are legal, a NaN bound takes the stock out of the universe); ``budget`` a
    scalar or [D].  Up to ``max_passes`` passes are launched; every ``check_every`` passes the
    number of unfinished dates is read back (one number) to stop early, ``check_every=0`` never
    reads back.  ``status``: ``OK``; ``MAX_PASSES`` (the last trial, which is feasible, is
    returned); ``INFEASIBLE`` and ``INVALID`` (non-finite F or stats) give an all-NaN row.
    ``variance`` = h^T Sigma h = sum s^2 h^2 + |B^T h|^2 of the returned weights.  GPU: K <= 64
    and Q <= 16 (``ValueError`` before any launch).  ``torch_ops`` runs the dense torch
    transcription on the tensors' device (the CPU path; on the GPU only as a timing
    comparison); ``stream_rows`` forces the projection kernel's re-streaming variant.

    ``prev`` / ``tcost`` (a scalar, [N] or [D, N] each; both or neither, ``ValueError``
    otherwise) add the linear trading cost ``sum_n tcost_n |h_n - prev_n|`` to the objective
    (:mod:`.tcost_qp`) and return a :class:`BoxQPCost`.  A non-finite ``prev`` is 0; ``tcost`` =
    +inf means "do not trade this name" (it ends at ``clip(prev, lower, upper)``); a NaN or
    negative ``tcost`` on a stock of the universe makes the date ``INVALID``.  Without them the
    call is what it was.
    """
    check_tcost(prev, tcost)
    D, Q, N = X.shape
    K = 1 + P + Q
    dev = X.device
    dense = torch_ops or not X.is_cuda
    if not dense:
        fc._check_limits(X, P)
    if D == 0:
        e = torch.empty(0, dtype=torch.float64, device=dev)
        ei = torch.empty(0, dtype=torch.int32, device=dev)
        r = BoxQP(torch.empty(0, N, dtype=torch.float64, device=dev), e, e.clone(), ei,
                  ei.clone())
        return r if tcost is None else BoxQPCost(*r, e.clone(), e.clone())
    pb = make_problem(X, cap, ret, ind, stats, P, F, spec_vol, q, lower, upper, budget, universe,
                      dense, prev, tcost)
    st, pj = new_state(D, K, dev), new_projection(D, N, dev)
    for it in range(1, max_passes + 1):
        run_pass(pb, st, pj, tol, stream_rows=stream_rows)
        if check_every and it % check_every == 0 and it < max_passes \
                and int((st.status == RUNNING).sum()) == 0:
            break
    status = torch.where(st.status == RUNNING, MAX_PASSES, st.status).to(torch.int32)
    dead = status >= INFEASIBLE
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    r = BoxQP(weights=torch.where(dead[:, None], nan, pj.h),
              gamma=torch.where(dead, nan, pj.gamma),
              variance=torch.where(dead, nan, st.ds[:, 2]),
              passes=st.passes, status=status)
    return r if tcost is None else BoxQPCost(*r, *trade_stats(r.weights, prev, tcost))
