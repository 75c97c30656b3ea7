"""Risk-budgeting (equal risk contribution, risk parity) portfolios on the factor-structured
asset covariance.

For every date d, over ``U_d`` = the universe of :func:`.factor_cov.universe_mask` restricted to
the stocks with a budget ``b_n > 0``, the long-only, fully invested ``h`` whose risk
contributions are in proportion to the budgets:

    h_n (Sigma_d h)_n / h^T Sigma_d h = b_n / sum_m b_m     (n in U),     h_n = 0  (n not in U)

with ``Sigma_d = X_d F_d X_d^T + diag(s_d^2)``.  It is not a QP.  Spinu's formulation: with the
budgets scaled to ``sum_U b = |U|``, y > 0 minimises the smooth convex

    phi(y) = 1/2 y^T Sigma y - sum_U b_n ln y_n,

the minimiser is unique, satisfies ``y_n (Sigma y)_n = b_n`` and ``h = budget y / sum y``.  The
Hessian ``Sigma + diag(b / y^2)`` is again "factor part + diagonal", so a Newton step is the
Woodbury solve of :mod:`.factor_cov` with a changed diagonal.  At an iterate y, with
``x = X^T y`` and ``z = F x``:

    Sy_n = s_n^2 y_n + x_n . z      g_n = Sy_n - b_n / y_n      a_n = 1 / (s_n^2 + b_n / y_n^2)
    G = X^T diag(a) X    v = X^T (a o g)    sigma = sum a g^2    r = max_U |y_n Sy_n / b_n - 1|
    c = R (I + R^T G R)^-1 R^T v   (F = R R^T)      lambda = sqrt(max(sigma - v^T c, 0))
    delta_n = -a_n (g_n - x_n . c)

The trial step is clamped by coordinate, ``y+ = max(y + delta, theta y)``, which keeps y > 0
without a line search.  The next pass evaluates ``phi(y+)``; a trial with ``phi(y+) > phi(y) +
1e-12 |phi(y)|`` is rejected and the date takes, from the saved y, the damped Newton step
``y + delta / (1 + M lambda)`` with ``M = 1 / sqrt(min_U b)``, which self-concordance keeps
positive and descending, so it is accepted unconditionally.  A date stops when ``r <= tol``: r is
the relative error of the risk contributions, returned as ``rc_gap``.  The start is
``y0 = sqrt(b) / s`` scaled along its ray to ``y0^T Sigma y0 = |U|``.

Every date keeps two iterates, ``y`` [2, D, N] and ``x`` [2, D, K]; ``sel`` names the saved (last
accepted) one and ``1 - sel`` the trial, since dates accept and reject independently.  One pass
on the GPU is three launches with no host synchronisation (``csrc/risk_budget.hip``):
``rb_moments`` (one stream over the panel: G, v and the scalars at the trial), ``rb_step``
(accept / reject / converged, c and lambda) and ``rb_update`` (a second stream: the next trial
and its ``X^T y``); K = 1 + P + Q <= 64 and Q <= 16 as in :mod:`.factor_cov`.  CPU tensors take
the float64 torch transcription below (dense ``X_d``; any K), which is also the tests' oracle.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from .. import _native
from . import eigen
from . import factor_cov as fc
from .box_qp import INFEASIBLE, INVALID, MAX_PASSES, OK, RUNNING, _rows

CLAMPED, DAMPED = 0, 1     # how a date's trial was formed (kClamped / kDamped)
REJECT = 1e-12             # a trial is rejected when phi rises by more than this, relative
_INF = float("inf")

_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
_native.register("mfa_rb_moments", [_vp] * 12 + [_i] * 4 + [_vp] * 4)
_native.register("mfa_rb_moments_f64", [_vp] * 12 + [_i] * 4 + [_vp] * 4)
_native.register("mfa_rb_step", [_vp] * 6 + [_d, _i, _i] + [_vp] * 8)
_native.register("mfa_rb_update", [_vp] * 15 + [_d] + [_i] * 4 + [_vp])
_native.register("mfa_rb_update_f64", [_vp] * 15 + [_d] + [_i] * 4 + [_vp])


class RiskBudget(NamedTuple):
    """:func:`risk_budget`: ``weights`` [D, N], ``variance`` = h^T Sigma h and ``rc_gap`` = max_U
    |RC share / budget share - 1| [D] (float64), ``passes`` / ``rejected`` / ``status`` [D]
    (int32; ``OK``, ``MAX_PASSES``, ``INFEASIBLE``, ``INVALID``)."""
    weights: torch.Tensor
    variance: torch.Tensor
    rc_gap: torch.Tensor
    passes: torch.Tensor
    rejected: torch.Tensor
    status: torch.Tensor


class Problem(NamedTuple):
    """What every pass reads: the panel, the scaled budgets ``bt`` and ``s2`` = s^2 [D, N] (both
    0 outside U), ``F`` and its eigenpairs, ``M`` = 1 / sqrt(min_U bt) and ``budget`` [D],
    ``status0`` [D] (``RUNNING``, or why the date cannot be solved), ``nU`` [D] = |U| and the
    dense design matrix (torch path only)."""
    panel: tuple
    bt: torch.Tensor
    s2: torch.Tensor
    F: torch.Tensor
    lam: torch.Tensor
    U: torch.Tensor
    M: torch.Tensor
    budget: torch.Tensor
    status0: torch.Tensor
    nU: torch.Tensor
    Xd: torch.Tensor | None


class State(NamedTuple):
    """Per-date solver state, updated in place: the two iterates ``y`` [2, D, N] and their
    exposures ``x`` [2, D, K]; ``c`` [D, K] (Newton coefficients at the saved iterate); ``ds``
    [D, 5] = (phi, lambda, damped step length, y^T Sigma y, r) of the saved iterate; ``sel`` (the
    saved iterate's buffer), ``mode`` (``CLAMPED`` / ``DAMPED`` trial), ``passes``, ``rejected``,
    ``status`` [D] int32."""
    y: torch.Tensor
    x: torch.Tensor
    c: torch.Tensor
    ds: torch.Tensor
    sel: torch.Tensor
    mode: torch.Tensor
    passes: torch.Tensor
    rejected: torch.Tensor
    status: torch.Tensor

    def clone(self) -> "State":
        return State(*(t.clone() for t in self))

    def to(self, device) -> "State":
        return State(*(t.to(device) for t in self))


class Moments(NamedTuple):
    """:func:`rb_moments`: ``G`` [D, K, K], ``v`` [D, K], ``sc`` [D, 4] = (sigma, r, phi,
    y^T Sigma y) at the trial iterate."""
    G: torch.Tensor
    v: torch.Tensor
    sc: torch.Tensor

    def to(self, device) -> "Moments":
        return Moments(*(t.to(device) for t in self))


def new_moments(D: int, K: int, device) -> Moments:
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=device)   # noqa: E731
    return Moments(z(D, K, K), z(D, K), z(D, 4))


def _pick(t: torch.Tensor, which: torch.Tensor) -> torch.Tensor:
    """Row ``which[d]`` (0 or 1) of ``t`` [2, D, ...] for every date."""
    w = which.bool().reshape(-1, *([1] * (t.dim() - 2)))
    return torch.where(w, t[1], t[0])


def _put(t: torch.Tensor, which: torch.Tensor, rows: torch.Tensor, val: torch.Tensor) -> None:
    """``t[which[d], d] = val[d]`` for the dates of the boolean ``rows``."""
    shape = (-1, *([1] * (t.dim() - 2)))
    for k in (0, 1):
        m = (rows & (which == k)).reshape(shape)
        t[k] = torch.where(m, val, t[k])


def _dates(fn, *ts: torch.Tensor) -> torch.Tensor:
    """``fn`` on every date's slices, stacked.  The torch path forms its matrix products date by
    date: a batched product picks its kernel, and with it the order of its sums, by the number
    of dates, and a date's result must not depend on the other dates of the call."""
    return torch.stack([fn(*(t[d] for t in ts)) for d in range(ts[0].shape[0])])


def _xty(Xd: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """``X_d^T h`` [D, K]."""
    return _dates(lambda X, v: X.T @ v, Xd, h)


def _xdot(Xd: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """``X_d c`` [D, N]."""
    return _dates(lambda X, v: X @ v, Xd, c)


# ---------------------------------------------------------------------------------- set-up
def make_problem(X, cap, ret, ind, stats, P, F, spec_vol, budgets=None, budget=1.0,
                 universe=None, dense: bool | None = None) -> Problem:
    """The per-call set-up of :func:`risk_budget` (same arguments): U, the scaled budgets,
    ``eigh(F)`` and the dates that cannot be solved; ``dense`` also builds the design matrix
    (default: on the CPU)."""
    D, Q, N = X.shape
    K = 1 + P + Q
    dev = X.device
    dense = (not X.is_cuda) if dense is None else dense
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    b = _rows(1.0 if budgets is None else budgets, D, N, dev, "budgets")
    bud = torch.as_tensor(budget, dtype=torch.float64, device=dev).expand(D).contiguous()
    m = fc.universe_mask(X, cap, ret, ind, P, spec_vol, universe)
    okb = torch.isfinite(b) & (b >= 0)
    Um = m & okb & (b > 0)
    bz = torch.where(Um, b, zero)
    if dense:
        nU, sb = Um.sum(-1).double(), bz.sum(-1)
    elif D:   # sums over U in the kernels' fixed order: the country column of X^T h
        nU, sb = fc.factor_xty(X, cap, ret, ind, stats, P,
                               torch.stack([Um.double(), bz], 1))[:, :, 0].unbind(1)
    else:
        nU = sb = b.new_zeros(0)
    bt = torch.where(Um, b * (nU / sb.clamp(min=1e-300))[:, None], zero)
    _, s2 = fc._weights(X, cap, ret, ind, P, spec_vol, universe)
    s2 = torch.where(Um, s2, zero).contiguous()
    bmin = torch.where(Um, bt, zero + _INF).amin(-1)
    stats = fc._f64(stats, (D, Q + 2), "stats")
    F = fc._f64(F.to(dev), (D, K, K), "F")
    invalid = (m & ~okb).any(-1) | ~torch.isfinite(F).all(-1).all(-1) | ~fc._stats_ok(stats, Q) \
        | ~torch.isfinite(bt).all(-1)
    infeas = (nU == 0) | ~(torch.isfinite(bud) & (bud > 0))
    status0 = torch.where(invalid, INVALID, torch.where(infeas, INFEASIBLE, RUNNING)).to(
        torch.int32)
    run = status0 == RUNNING
    bt = torch.where(run[:, None], bt, zero).contiguous()
    M = torch.where(run, 1.0 / torch.sqrt(bmin), zero + 1.0).contiguous()
    if D:
        lam, U = eigen.eigh(F)
    else:
        lam, U = F.new_empty(0, K), F.new_empty(0, K, K)
    Xd = fc.design_matrix(X, cap, ret, ind, torch.nan_to_num(stats), P, Um) if dense else None
    return Problem((X, cap, ret, ind, stats, P), bt, s2, F, lam.contiguous(), U.contiguous(), M,
                   bud, status0, nU.contiguous(), Xd)


def new_state(pb: Problem) -> State:
    """The state before the first pass: the trial is ``y0 = sqrt(b) / s`` scaled along its ray to
    ``y0^T Sigma y0 = |U|``, and phi = +inf, so the first trial is accepted.  One
    :func:`.factor_cov.factor_xty` and torch ops."""
    D, N = pb.bt.shape
    K = pb.F.shape[-1]
    dev = pb.bt.device
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    run = pb.status0 == RUNNING
    m = pb.bt > 0
    y0 = torch.where(m, torch.sqrt(pb.bt / torch.where(m, pb.s2, zero + 1.0)), zero)
    Fz = torch.where(run[:, None, None], pb.F, zero)
    if pb.Xd is not None:
        x0 = torch.where(run[:, None], _xty(pb.Xd, y0), zero)
        q = (pb.s2 * y0 * y0).sum(-1) + (x0 * _xdot(Fz, x0)).sum(-1)
    elif D:
        # every sum in a fixed order that does not depend on D: sum s^2 y0^2 is the country
        # column of a second right-hand side, x0' F x0 is accumulated term by term
        xs = fc.factor_xty(*pb.panel, torch.stack([y0, pb.s2 * y0 * y0], 1))
        x0 = torch.where(run[:, None], xs[:, 0], zero)
        q = torch.where(run, xs[:, 1, 0], zero)
        z = torch.zeros_like(x0)
        for k in range(K):
            z = torch.addcmul(z, Fz[:, :, k], x0[:, k:k + 1])
        for k in range(K):
            q = torch.addcmul(q, x0[:, k], z[:, k])
    else:
        x0, q = y0.new_zeros(0, K), y0.new_zeros(0)
    scale = torch.where(run & (q > 0), torch.sqrt(pb.nU / q.clamp(min=1e-300)), zero)
    y = torch.zeros(2, D, N, dtype=torch.float64, device=dev)
    x = torch.zeros(2, D, K, dtype=torch.float64, device=dev)
    y[1], x[1] = y0 * scale[:, None], x0 * scale[:, None]
    ds = torch.zeros(D, 5, dtype=torch.float64, device=dev)
    ds[:, 0] = _INF
    ds[:, 2] = 1.0
    zi = lambda: torch.zeros(D, dtype=torch.int32, device=dev)            # noqa: E731
    return State(y, x, torch.zeros(D, K, dtype=torch.float64, device=dev), ds, zi(), zi(), zi(),
                 zi(), pb.status0.clone())


# --------------------------------------------------------------------------------- moments
def _at(pb: Problem, y, x):
    """(m, Sy, g, a) of the method at the iterate (y, x); 0 outside U."""
    zero = torch.zeros((), dtype=torch.float64, device=y.device)
    m = (pb.bt > 0) & (y > 0)
    y1 = torch.where(m, y, zero + 1.0)
    z = _xdot(torch.nan_to_num(pb.F), x)
    Sy = torch.where(m, pb.s2 * y + _xdot(pb.Xd, z), zero)
    by = pb.bt / y1
    g = torch.where(m, Sy - by, zero)
    a = torch.where(m, 1.0 / (pb.s2 + by / y1), zero)
    return m, y1, Sy, g, a


def _moments_torch(pb: Problem, st: State, out: Moments) -> None:
    zero = torch.zeros((), dtype=torch.float64, device=pb.bt.device)
    run = st.status == RUNNING
    y, x = _pick(st.y, 1 - st.sel), _pick(st.x, 1 - st.sel)
    m, y1, Sy, g, a = _at(pb, y, x)
    G = _dates(lambda X, w: X.T @ (w[:, None] * X), pb.Xd, a)
    v = _xty(pb.Xd, a * g)
    bt1 = torch.where(m, pb.bt, zero + 1.0)
    r = torch.where(m, (y * Sy / bt1 - 1.0).abs(), zero).amax(-1)
    ysy = (y * Sy).sum(-1)
    phi = 0.5 * ysy - torch.where(m, pb.bt * torch.log(y1), zero).sum(-1)
    sc = torch.stack([(a * g * g).sum(-1), r, phi, ysy], -1)
    out.G.copy_(torch.where(run[:, None, None], G, out.G))
    out.v.copy_(torch.where(run[:, None], v, out.v))
    out.sc.copy_(torch.where(run[:, None], sc, out.sc))


def _check_gpu(pb: Problem):
    """The panel as the kernels take it: (dtype, X, cap, ret, ind, stats, P)."""
    X, cap, ret, ind, stats, P = pb.panel
    fc._check_limits(X, P)
    stats = fc._f64(stats, (X.shape[0], X.shape[1] + 2), "stats")
    return (*fc._panel_args(X, cap, ret, ind, P), stats, P)


def rb_moments(pb: Problem, st: State, out: Moments | None = None) -> Moments:
    """G, v and (sigma, r, phi, y^T Sigma y) at the trial iterate of every running date, in one
    stream over the panel; the rows of finished dates keep what ``out`` held (zeros without
    it).  GPU: one workgroup per date (two from 11 styles on), order-fixed sums."""
    D, N = pb.bt.shape
    K = pb.F.shape[-1]
    out = new_moments(D, K, pb.bt.device) if out is None else out
    if D == 0:
        return out
    if pb.Xd is not None:
        _moments_torch(pb, st, out)
        return out
    dt, X, cap, ret, ind, stats, P = _check_gpu(pb)
    _native.call("mfa_rb_moments_f64" if dt == torch.float64 else "mfa_rb_moments",
                 _native.ptr(X), _native.ptr(cap), _native.ptr(ret), _native.ptr(ind),
                 _native.ptr(st.y), _native.ptr(st.x), _native.ptr(st.sel), _native.ptr(pb.bt),
                 _native.ptr(pb.s2), _native.ptr(pb.F), _native.ptr(stats),
                 _native.ptr(st.status), D, N, P, X.shape[1], _native.ptr(out.G),
                 _native.ptr(out.v), _native.ptr(out.sc), _native.stream(X.device))
    return out


# ------------------------------------------------------------------------------------ step
def _step_torch(mo: Moments, lam, U, M, st: State, tol: float) -> None:
    D, K = mo.v.shape
    dev = mo.v.device
    run = st.status == RUNNING
    eye = torch.eye(K, dtype=torch.float64, device=dev)
    R = U * torch.sqrt(lam.clamp(min=0.0))[:, None, :]
    bad = ~(torch.isfinite(mo.G).all(-1).all(-1) & torch.isfinite(U).all(-1).all(-1)
            & torch.isfinite(lam).all(-1) & torch.isfinite(mo.v).all(-1)
            & torch.isfinite(mo.sc).all(-1) & torch.isfinite(M))
    st.status[run & bad] = INVALID
    run = run & ~bad
    Rz, Gz, vz = torch.nan_to_num(R), torch.nan_to_num(mo.G), torch.nan_to_num(mo.v)
    sigma, r, phit, ysy = torch.nan_to_num(mo.sc).unbind(-1)
    phi = st.ds[:, 0]
    acc = (st.mode == DAMPED) | ~(phit > phi + REJECT * phi.abs())
    rej = run & ~acc
    conv = run & acc & (r <= tol)
    newton = run & acc & ~(r <= tol)
    if bool(newton.any()):
        Mm = torch.where(newton[:, None, None], eye + _dates(lambda R_, G_: R_.T @ G_ @ R_, Rz, Gz),
                         eye)
        L, info = torch.linalg.cholesky_ex(Mm)
        fail = newton & (info != 0)
        L = torch.where(fail[:, None, None], eye, L)
        p = _xty(Rz, vz)
        c = _xdot(Rz, torch.cholesky_solve(p[..., None], L)[..., 0])
        st.status[fail] = INVALID
        newton = newton & ~fail
        st.c.copy_(torch.where(newton[:, None], c, st.c))
        l2 = (sigma - (vz * c).sum(-1)).clamp(min=0.0)
        st.ds[:, 1] = torch.where(newton, torch.sqrt(l2), st.ds[:, 1])
    A = conv | newton
    st.sel.copy_(torch.where(A, 1 - st.sel, st.sel))
    st.ds[:, 0] = torch.where(A, phit, phi)
    st.ds[:, 3] = torch.where(A, ysy, st.ds[:, 3])
    st.ds[:, 4] = torch.where(A, r, st.ds[:, 4])
    st.ds[:, 2] = torch.where(rej, 1.0 / (1.0 + M * st.ds[:, 1]), st.ds[:, 2])
    mode = torch.where(newton, CLAMPED, torch.where(rej, DAMPED, st.mode))
    st.mode.copy_(mode.to(torch.int32))
    st.rejected[rej] += 1
    st.passes[A | rej] += 1
    st.status[conv] = OK


def rb_step(mo: Moments, lam, U, M, state: State, tol: float) -> State:
    """The accept / reject / converged decision for every running date, in place on ``state``.
    A trial is accepted when it was a damped step or phi did not rise; it becomes the saved
    iterate (``sel`` flips, phi / y^T Sigma y / r are saved), the date stops with ``OK`` when
    ``r <= tol``, otherwise c and lambda are computed from ``mo`` and the next trial is
    clamped.  A rejected trial leaves the saved iterate, its c and lambda, sets the next trial
    to damped with the step length ``1 / (1 + M lambda)`` and counts in ``rejected``.  Either
    way ``passes`` goes up by one.  A non-finite input or a non-positive Cholesky pivot gives
    ``INVALID``.  ``lam`` / ``U`` are the eigenpairs of F.  GPU: K <= 64, one workgroup per date
    (I + R^T G R and its Cholesky factor in LDS)."""
    D, K = mo.v.shape
    if mo.v.is_cuda and K > fc.MAX_K:
        raise ValueError(f"rb_step on the GPU supports K <= {fc.MAX_K}, got K = {K}")
    U = fc._f64(U, (D, K, K), "U")
    lam, M = fc._f64(lam, (D, K), "lam"), fc._f64(M, (D,), "M")
    if D == 0:
        return state
    if not mo.v.is_cuda:
        _step_torch(mo, lam, U, M, state, tol)
        return state
    _native.call("mfa_rb_step", _native.ptr(mo.G), _native.ptr(mo.v), _native.ptr(mo.sc),
                 _native.ptr(lam), _native.ptr(U), _native.ptr(M), float(tol), D, K,
                 _native.ptr(state.c), _native.ptr(state.ds), _native.ptr(state.sel),
                 _native.ptr(state.mode), _native.ptr(state.passes), _native.ptr(state.rejected),
                 _native.ptr(state.status), _native.stream(mo.v.device))
    return state


# ---------------------------------------------------------------------------------- update
def _update_torch(pb: Problem, st: State, theta: float) -> None:
    zero = torch.zeros((), dtype=torch.float64, device=pb.bt.device)
    run = st.status == RUNNING
    y, x = _pick(st.y, st.sel), _pick(st.x, st.sel)
    m, y1, Sy, g, a = _at(pb, y, x)
    delta = -a * (g - _xdot(pb.Xd, torch.nan_to_num(st.c)))
    yt = torch.where((st.mode == DAMPED)[:, None], y + st.ds[:, 2, None] * delta,
                     torch.maximum(y + delta, theta * y))
    yt = torch.where(m, yt, zero)
    _put(st.y, 1 - st.sel, run, yt)
    _put(st.x, 1 - st.sel, run, _xty(pb.Xd, yt))


def rb_update(pb: Problem, state: State, theta: float = 0.1) -> State:
    """The next trial of every running date, written to the buffer that ``1 - sel`` names:
    ``max(y + delta, theta y)`` (clamped) or ``y + ds[2] delta`` (damped) from the saved iterate
    and its c, 0 outside U, with ``x = X^T y_trial`` summed in the same stream over the panel."""
    D, N = pb.bt.shape
    if D == 0:
        return state
    if pb.Xd is not None:
        _update_torch(pb, state, theta)
        return state
    dt, X, cap, ret, ind, stats, P = _check_gpu(pb)
    _native.call("mfa_rb_update_f64" if dt == torch.float64 else "mfa_rb_update",
                 _native.ptr(X), _native.ptr(cap), _native.ptr(ret), _native.ptr(ind),
                 _native.ptr(state.y), _native.ptr(state.x), _native.ptr(state.sel),
                 _native.ptr(state.mode), _native.ptr(state.c), _native.ptr(state.ds),
                 _native.ptr(pb.bt), _native.ptr(pb.s2), _native.ptr(pb.F), _native.ptr(stats),
                 _native.ptr(state.status), float(theta), D, N, P, X.shape[1],
                 _native.stream(X.device))
    return state


# ---------------------------------------------------------------------------------- driver
def run_pass(pb: Problem, st: State, tol: float = 1e-9, theta: float = 0.1,
             mo: Moments | None = None) -> Moments:
    """One pass for every running date: moments at the trial, the step, the next trial.  On the
    GPU: three launches, no host synchronisation."""
    mo = rb_moments(pb, st, mo)
    rb_step(mo, pb.lam, pb.U, pb.M, st, tol)
    rb_update(pb, st, theta)
    return mo


def result(pb: Problem, st: State) -> RiskBudget:
    """The :class:`RiskBudget` of a state: weights from every date's saved iterate."""
    dev = pb.bt.device
    status = torch.where(st.status == RUNNING, MAX_PASSES, st.status).to(torch.int32)
    dead = (status >= INFEASIBLE) | (st.passes == 0)
    y = _pick(st.y, st.sel)
    tot = _pick(st.x, st.sel)[:, 0]   # the country exposure of y: sum_U y in a fixed order
    tot1 = torch.where(tot > 0, tot, torch.ones_like(tot))
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    w = pb.budget[:, None] * y / tot1[:, None]
    var = pb.budget * pb.budget * st.ds[:, 3] / (tot1 * tot1)
    return RiskBudget(weights=torch.where(dead[:, None], nan, w),
                      variance=torch.where(dead, nan, var),
                      rc_gap=torch.where(dead, nan, st.ds[:, 4]),
                      passes=st.passes, rejected=st.rejected, status=status)


def risk_budget(X, cap, ret, ind, stats, P, F, spec_vol, budgets=None, budget=1.0,
                universe=None, *, tol: float = 1e-9, max_passes: int = 32,
                check_every: int = 4, theta: float = 0.1) -> RiskBudget:
    """The risk-budgeting portfolio of the module docstring for every date.

    Panel arguments, ``F`` [D, K, K], ``spec_vol`` and ``universe`` as in
    :func:`.factor_cov.solve_cov`.  ``budgets``: None (equal risk contribution), [N] or [D, N];
    b = 0 excludes a stock (weight 0); a NaN, infinite or negative budget on a stock of
    ``universe_mask`` makes the date ``INVALID``.  ``budget`` (the sum of the weights): a scalar
    or [D]; not finite or not > 0 gives ``INFEASIBLE``.  Up to ``max_passes`` passes are
    launched; every ``check_every`` passes the number of unfinished dates is read back (one
    number) to stop early, ``check_every=0`` never reads back.  ``status``: ``OK``;
    ``MAX_PASSES`` (the weights are those of the last accepted iterate); ``INFEASIBLE`` (an
    empty universe, a bad ``budget``) and ``INVALID`` (a non-finite F or ``stats``, a bad budget
    entry) give NaN rows.  Stocks outside U get exactly 0.  GPU: K <= 64 and Q <= 16
    (``ValueError`` before any launch); two calls give the same bits, and a date's result does
    not depend on the other dates of the call.
    """
    D, Q, N = X.shape
    dev = X.device
    fc._check_limits(X, P)
    if D == 0:
        e = torch.empty(0, dtype=torch.float64, device=dev)
        ei = torch.empty(0, dtype=torch.int32, device=dev)
        return RiskBudget(torch.empty(0, N, dtype=torch.float64, device=dev), e, e.clone(),
                          ei, ei.clone(), ei.clone())
    pb = make_problem(X, cap, ret, ind, stats, P, F, spec_vol, budgets, budget, universe)
    st = new_state(pb)
    mo = new_moments(D, 1 + P + Q, dev)
    for it in range(1, max_passes + 1):
        run_pass(pb, st, tol, theta, mo)
        if check_every and it % check_every == 0 and it < max_passes \
                and int((st.status == RUNNING).sum()) == 0:
            break
    return result(pb, st)
