"""Box-constrained portfolio optimisation with factor-exposure equality constraints.

For every date d, over the universe ``U_d`` of :func:`.factor_cov.universe_mask`:

    minimise   1/2 h^T Sigma_d h - q^T h
    subject to sum_U h_n = budget,   lo_n <= h_n <= hi_n  (n in U),   h_n = 0  (n not in U),
               (X_d^T h)_k = t_{d,k}   for k in S

``S`` is a set of m factor indices 1 <= k < K, the same for every date of a call (the country
column 0 is the budget and is refused); ``X_d^T h`` are the model's exposures as
:func:`.factor_cov.factor_xty` returns them (industry weight sums, z-scored styles).  "Long-only,
2 % cap, industry- and size-neutral to the benchmark" is ``S`` = industries + SIZE with ``t`` the
benchmark's exposures.

The method keeps the shape of :mod:`.box_qp`: a semismooth Newton method on a K-dimensional dual
with the budget multiplier gamma eliminated by the exact projection, so every iterate is box-
and budget-feasible.  Let T be the factors not in S (KT = K - m >= 1, T holds the country).  On
the feasible set x_S = t, so the factor risk is 1/2 x_T^T F_TT x_T + x_T^T F_TS t + const; only
``y_T = R_T^T x_T`` is dualised, ``F_TT = R_T R_T^T`` from ``eigen.eigh``.  The multipliers are
``lambda = (nu_T in R^KT, mu in R^m)``; with J [K, K] holding R_T on rows T x the first KT columns
and the identity on rows S x the last m columns, d = (1..1, 0..0), tau = (0..0, t) and
``q' = q - X_T F_TS t``:

    c = J lambda,   u = a (q' - X c),   h = clip(u + gamma a, lo, hi)   (gamma: box_project)
    phi(lambda) = 1/2 sum s^2 h^2 - q'^T h + c^T x - 1/2 sum d_k lambda_k^2 - tau^T lambda
    grad phi = J^T x - d o lambda - tau        (nu: R_T^T x_T - nu_T;   mu: x_S - t),   x = X^T h
    H = diag(d) + J^T (G_f - g_f g_f^T / sigma_f) J + rho diag_mu(D_U)

The mu block of H has no identity: it is singular whenever the free set is small, or when S
holds every industry (their columns sum to the country column).  ``D_U`` is the diagonal of
``J^T (G_U - g_U g_U^T / sigma_U) J`` with ``G_U`` the Gram over the whole universe (one
``factor_gram`` pass per call); ``rho`` is a per-date state that starts at 1, is divided by 10
(floor 1e-14) after a step accepted at full length and multiplied by 4 (cap 1) when the step had
to be cut.  The Newton step ``H dl = grad phi`` is followed by the Armijo backtracking of
:mod:`.box_qp`.  A date stops when the nu block passes the test of :mod:`.box_qp` (with F_TT) and

    max |x_S - t| <= tol * max(1, sum |h|)

Multipliers of the original problem, written when a date converges:
``eta = -mu + (F x)_S``.  Sign convention: with r = Sigma h - q,

    r_n = gamma + (X_S eta)_n   on stocks strictly inside their bounds,
    r_n >= gamma + (X_S eta)_n  at the lower bound,   r_n <= gamma + (X_S eta)_n  at the upper.

A target that no portfolio in the box reaches never converges: the date ends as ``MAX_PASSES``
with ``exposure_gap`` = max |x_S - t| of the returned trial.  Its mu grows without bound (phi is
unbounded), and with it u = a (q' - X c), until the projection, which holds the budget to a few
eps of max |u|, can no longer hold it to a few eps of sum |h|.  So the step tests every trial's
budget on x_0 = sum h: a date whose trial misses 5e-13 (sum |h| + |budget|) is stopped there
(internal status ``STALLED``, reported as ``MAX_PASSES``) with all of its state untouched, and
the driver, which alternates between two projection buffers, returns the trial before it.  Every
returned row therefore holds the budget to 1e-12 (sum |h| + |budget|).  One pass on the GPU is the
four panel launches of :func:`.box_qp.run_trial` and ``eq_step`` (``csrc/box_qp.hip``); K <= 64
and Q <= 16.  CPU tensors take the float64 torch transcription below (any K), the tests' oracle.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from .. import _native
from . import box_qp as bq
from . import eigen
from . import factor_cov as fc
from .box_qp import INFEASIBLE, INVALID, MAX_PASSES, OK, RUNNING  # noqa: F401

RHO0, RHO_MIN, RHO_DOWN, RHO_UP = 1.0, 1e-14, 10.0, 4.0
STALLED = 4             # internal: a trial lost the budget (kStalled in csrc/box_qp.hip)
BUDGET_TOL = 5e-13      # of sum |h| + |budget|: half of what a returned row has to meet

_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
_native.register("mfa_eq_step", [_vp] * 10 + [_d, _i, _i, _i] + [_vp] * 12)


class ExposureQP(NamedTuple):
    """:func:`exposure_qp`: ``weights`` [D, N], ``gamma`` [D], ``eta`` [D, m] (multipliers of the
    exposure constraints, NaN unless ``OK``), ``exposure_gap`` [D] = max |x_S - t| of the returned
    weights, ``variance`` [D] (float64), ``passes`` / ``status`` [D] (int32, the codes of
    :mod:`.box_qp`)."""
    weights: torch.Tensor
    gamma: torch.Tensor
    eta: torch.Tensor
    exposure_gap: torch.Tensor
    variance: torch.Tensor
    passes: torch.Tensor
    status: torch.Tensor


class ExposureQPCost(NamedTuple):
    """:func:`exposure_qp` with ``prev`` / ``tcost``: the fields of :class:`ExposureQP`, then
    ``turnover`` and ``cost`` [D] as in :class:`.box_qp.BoxQPCost`."""
    weights: torch.Tensor
    gamma: torch.Tensor
    eta: torch.Tensor
    exposure_gap: torch.Tensor
    variance: torch.Tensor
    passes: torch.Tensor
    status: torch.Tensor
    turnover: torch.Tensor
    cost: torch.Tensor


class EqProblem(NamedTuple):
    """What :func:`eq_step` reads besides the trial: ``J`` / ``F`` [D, K, K], ``d`` [K] (1 on the
    nu slots, 0 on the mu slots), ``tau`` / ``DU`` [D, K], ``budget`` [D]; ``KT`` = number of nu
    slots."""
    J: torch.Tensor
    d: torch.Tensor
    tau: torch.Tensor
    DU: torch.Tensor
    F: torch.Tensor
    budget: torch.Tensor
    KT: int


class EqState(NamedTuple):
    """Per-date solver state of :func:`eq_step`: ``step`` (a :class:`.box_qp.StepState` whose
    ``nu`` holds lambda and whose ``ds`` [D, 4] = (phi, step, variance, exposure gap of the last
    trial that held the budget)), ``rho`` [D], ``eta`` [D, K] (slot order: 0 on the nu slots)
    and ``which`` [D] int32, the ``parity`` of the last step whose trial held the budget."""
    step: bq.StepState
    rho: torch.Tensor
    eta: torch.Tensor
    which: torch.Tensor

    def clone(self) -> "EqState":
        return EqState(self.step.clone(), self.rho.clone(), self.eta.clone(), self.which.clone())

    def to(self, device) -> "EqState":
        return EqState(self.step.to(device), self.rho.to(device), self.eta.to(device),
                       self.which.to(device))


def new_eq_state(D: int, K: int, device) -> EqState:
    return EqState(bq.new_state(D, K, device),
                   torch.full((D,), RHO0, dtype=torch.float64, device=device),
                   torch.zeros(D, K, dtype=torch.float64, device=device),
                   torch.zeros(D, dtype=torch.int32, device=device))


def check_factors(factors, K: int) -> list[int]:
    """``factors`` as a list of distinct ints in 1..K-1 (``ValueError`` otherwise)."""
    sel = [int(k) for k in (factors.tolist() if isinstance(factors, torch.Tensor) else factors)]
    if any(k == 0 for k in sel):
        raise ValueError("factor 0 (the country) cannot be constrained: it is the budget")
    if any(k < 1 or k >= K for k in sel):
        raise ValueError(f"factors must lie in 1..{K - 1}, got {sel}")
    if len(set(sel)) != len(sel):
        raise ValueError(f"factors must be distinct, got {sel}")
    return sel


# --------------------------------------------------------------------------------------- step
def _eq_step_torch(G, ep: EqProblem, x, pstats, pflag, es: EqState, tol: float,
                   parity: int = 0) -> None:
    st, rho = es.step, es.rho
    D, K = x.shape
    dev = x.device
    dv = ep.d
    mu_slot = dv == 0
    run = st.status == RUNNING
    eye = torch.eye(K, dtype=torch.float64, device=dev)
    fin2 = lambda t: torch.isfinite(t).all(-1).all(-1)   # noqa: E731
    bad = ~(fin2(G) & fin2(ep.J) & fin2(ep.F) & torch.isfinite(x).all(-1)
            & torch.isfinite(ep.tau).all(-1) & torch.isfinite(ep.DU).all(-1)
            & torch.isfinite(rho))
    bad = bad | ((pflag == 0) & ~torch.isfinite(pstats[:, :2]).all(-1))
    stop = run & ((pflag != 0) | bad)
    st.status[stop] = torch.where(pflag == 1, INFEASIBLE, INVALID).to(torch.int32)[stop]
    st.accepted[stop] = 0
    run = run & ~stop
    Jz, Gz, Fz = torch.nan_to_num(ep.J), torch.nan_to_num(G), torch.nan_to_num(ep.F)
    xz, ps = torch.nan_to_num(x), torch.nan_to_num(pstats)
    tz, Dz = torch.nan_to_num(ep.tau), torch.nan_to_num(ep.DU)
    phi, step = st.ds[:, 0], st.ds[:, 1]
    lt = st.nu + step[:, None] * st.dn
    by = torch.einsum("djk,dj->dk", Jz, xz)
    gt = by - dv * lt - tz
    phit = 0.5 * ps[:, 0] - ps[:, 1] + (lt * by).sum(-1) - 0.5 * (dv * lt * lt).sum(-1) \
        - (tz * lt).sum(-1)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    gmax = torch.where(mu_slot, zero, gt.abs()).amax(-1)
    gap = torch.where(mu_slot, gt.abs(), zero).amax(-1)
    gd = (st.grad * st.dn).sum(-1)
    bscale = torch.sqrt((Jz * Jz * dv).sum(-1).amax(-1))
    nonfin = run & ~(torch.isfinite(phit) & torch.isfinite(gmax) & torch.isfinite(gap))
    st.status[nonfin] = INVALID
    st.accepted[nonfin] = 0
    run = run & ~nonfin
    # a trial that lost the budget stops the date; nothing else of its state changes
    lost = run & (st.passes > 0) & ~((xz[:, 0] - ep.budget).abs()
                                     <= BUDGET_TOL * (ps[:, 2] + ep.budget.abs()))
    st.status[lost] = STALLED
    st.accepted[lost] = 0
    st.passes[lost] += 1
    run = run & ~lost
    hs = ps[:, 2].clamp(min=1.0)
    conv = (gmax <= tol * hs * bscale) & (gap <= tol * hs)
    acc = conv | (phit >= phi + bq.ARMIJO * step * gd - 4.0 * bq._EPS * phit.abs())
    rh = torch.where(acc, torch.where(step == 1.0, (rho / RHO_DOWN).clamp(min=RHO_MIN), rho),
                     (RHO_UP * rho).clamp(max=1.0))
    rho.copy_(torch.where(run, rh, rho))
    A, newton = run & acc, run & acc & ~conv
    if bool(newton.any()):
        Tm = Gz @ Jz
        p = Tm[:, 0, :]
        sigma = Gz[:, 0, 0]
        isg = torch.where(sigma > 0, 1.0 / sigma.clamp(min=1e-300), torch.zeros_like(sigma))
        Hd = torch.where(mu_slot, rho[:, None] * Dz, dv.expand(D, K))
        Hm = torch.diag_embed(Hd) + Jz.transpose(1, 2) @ Tm \
            - isg[:, None, None] * p[:, :, None] * p[:, None, :]
        Hm = torch.where(newton[:, None, None], Hm, eye)
        Lc, info = torch.linalg.cholesky_ex(Hm)
        fail = newton & (info != 0)
        Lc = torch.where(fail[:, None, None], eye, Lc)
        dn_new = torch.cholesky_solve(gt[..., None], Lc)[..., 0]
        st.status[fail] = INVALID
        st.accepted[fail] = 0
        run, A, newton = run & ~fail, A & ~fail, newton & ~fail
        st.dn[newton] = dn_new[newton]
    den = 2.0 * (phi + gd * step - phit)
    cut = torch.where(den > 0, gd * step * step / den.clamp(min=1e-300), 0.5 * step)
    cut = torch.minimum(torch.maximum(torch.nan_to_num(cut, nan=0.0), 0.1 * step), 0.5 * step)
    nstep = torch.where(acc, torch.where(conv, 0.0, 1.0).to(cut.dtype), cut)
    st.nu[A] = lt[A]
    st.grad[A] = gt[A]
    Fx = torch.einsum("dkl,dl->dk", Fz, xz)
    st.ds[:, 0] = torch.where(A, phit, phi)
    st.ds[:, 1] = torch.where(run, nstep, step)
    st.ds[:, 2] = torch.where(run, ps[:, 0] + (xz * Fx).sum(-1), st.ds[:, 2])
    st.ds[:, 3] = torch.where(run, gap, st.ds[:, 3])
    cn = torch.einsum("dik,dk->di", Jz, st.nu + st.ds[:, 1, None] * st.dn)
    st.c[run] = cn[run]
    st.passes[run] += 1
    st.accepted[run] = acc[run].to(torch.int32)
    es.which[run] = parity
    done = run & conv
    en = torch.where(mu_slot, torch.einsum("djk,dj->dk", Jz, Fx) - lt, zero)
    es.eta[done] = en[done]
    st.status[done] = OK


def eq_step(G, ep: EqProblem, x, pstats, pflag, state: EqState, tol: float, *,
            parity: int = 0, torch_ops: bool = False) -> EqState:
    """One outer step with exposure equalities for every running date, in place on ``state``:
    :func:`.box_qp.box_step` generalised to ``lambda = (nu_T, mu)`` (module docstring).  ``G``
    [D, K, K] is the Gram with the free set's weights, ``x`` [D, K] = X^T h, ``pstats`` /
    ``pflag`` come from :func:`.box_qp.box_project`.  Also writes the variance
    ``sum s^2 h^2 + x^T F x`` of the trial from the true x and the exposure gap (``ds[:, 2:4]``),
    updates ``rho`` and, when a date converges, writes ``eta``.  A date whose trial misses the
    budget (x_0 against ``ep.budget``, ``BUDGET_TOL``) becomes ``STALLED`` and keeps its state;
    every other running date gets ``which = parity``.  Finished dates are left untouched; a
    non-finite F, J, G, target or stats gives ``INVALID``.  GPU: K <= 64, one
    workgroup per date (``eq_step_kernel``); ``torch_ops`` runs the transcription instead."""
    D, K = x.shape
    if x.is_cuda and not torch_ops and K > fc.MAX_K:
        raise ValueError(f"eq_step on the GPU supports K <= {fc.MAX_K}, got K = {K}")
    G, x = fc._f64(G, (D, K, K), "G"), fc._f64(x, (D, K), "x")
    ep = EqProblem(fc._f64(ep.J, (D, K, K), "J"), fc._f64(ep.d, (K,), "d"),
                   fc._f64(ep.tau, (D, K), "tau"), fc._f64(ep.DU, (D, K), "DU"),
                   fc._f64(ep.F, (D, K, K), "F"), fc._f64(ep.budget, (D,), "budget"), ep.KT)
    if D == 0:
        return state
    if torch_ops or not x.is_cuda:
        _eq_step_torch(G, ep, x, pstats, pflag, state, tol, parity)
        return state
    st = state.step
    _native.call("mfa_eq_step", _native.ptr(G), _native.ptr(ep.J), _native.ptr(ep.d),
                 _native.ptr(ep.tau), _native.ptr(ep.DU), _native.ptr(ep.F), _native.ptr(x),
                 _native.ptr(pstats), _native.ptr(pflag), _native.ptr(ep.budget), float(tol), D,
                 K, int(parity), _native.ptr(st.nu), _native.ptr(st.grad), _native.ptr(st.dn),
                 _native.ptr(st.c), _native.ptr(st.ds), _native.ptr(state.rho),
                 _native.ptr(state.eta), _native.ptr(st.passes), _native.ptr(st.status),
                 _native.ptr(st.accepted), _native.ptr(state.which), _native.stream(x.device))
    return state


# ------------------------------------------------------------------------------------- driver
def make_eq_problem(pb: bq.Problem, F, sel: list[int], targets) -> tuple[bq.Problem, EqProblem]:
    """The per-call set-up on top of :func:`.box_qp.make_problem`: ``eigh(F_TT)``, J, d, tau,
    D_U, and ``pb`` with ``q`` replaced by ``q' = q - X_T F_TS t``."""
    X, cap, ret, ind, stats, P = pb.panel
    D, Q, N = X.shape
    K = 1 + P + Q
    dev = X.device
    m, KT = len(sel), K - len(sel)
    F = fc._f64(F.to(dev), (D, K, K), "F")
    t = torch.as_tensor(targets, dtype=torch.float64, device=dev)
    if t.dim() not in (1, 2) or t.shape[-1] != m or (t.dim() == 2 and t.shape[0] != D):
        raise ValueError(f"targets must be [m] or [D, m] with (D, m) = {(D, m)}, got "
                         f"{tuple(t.shape)}")
    t = t.expand(D, m)
    S = torch.tensor(sel, dtype=torch.long, device=dev)
    T = torch.tensor([k for k in range(K) if k not in set(sel)], dtype=torch.long, device=dev)
    lamT, UT = eigen.eigh(F[:, T][:, :, T].contiguous())
    RT = UT * torch.sqrt(lamT.clamp(min=0.0))[:, None, :]
    J = torch.zeros(D, K, K, dtype=torch.float64, device=dev)
    J[:, T[:, None], torch.arange(KT, device=dev)[None, :]] = RT
    J[:, S, KT + torch.arange(m, device=dev)] = 1.0
    dv = torch.cat([torch.ones(KT, dtype=torch.float64, device=dev),
                    torch.zeros(m, dtype=torch.float64, device=dev)])
    tau = torch.cat([torch.zeros(D, KT, dtype=torch.float64, device=dev), t], 1).contiguous()
    # q' = q - X_T F_TS t
    cq = torch.zeros(D, K, dtype=torch.float64, device=dev)
    cq[:, T] = torch.einsum("dts,ds->dt", F[:, T][:, :, S], torch.nan_to_num(t))
    cq = torch.nan_to_num(cq, nan=0.0, posinf=0.0, neginf=0.0)
    if pb.Xd is None:
        one = (pb.a > 0).double()
        qp = fc.factor_apply(*pb.panel, one, -one, pb.q[:, None], cq[:, None, :])[:, 0]
        GU = fc.factor_gram(*pb.panel, pb.a)
    else:
        qp = torch.nan_to_num(pb.q, nan=0.0, posinf=0.0, neginf=0.0) \
            - torch.einsum("dnk,dk->dn", pb.Xd, cq)
        GU = torch.einsum("dnk,dn,dnl->dkl", pb.Xd, pb.a, pb.Xd)
    # D_U = diag(J' (G_U - g g' / sigma) J), floored so that a factor no stock of the universe
    # loads on (an empty industry) keeps a positive pivot; its gradient entry is -t
    GU = torch.nan_to_num(GU, nan=0.0, posinf=0.0, neginf=0.0)
    Jz = torch.nan_to_num(J, nan=0.0, posinf=0.0, neginf=0.0)
    sig = GU[:, 0, 0]
    isg = torch.where(sig > 0, 1.0 / sig.clamp(min=1e-300), torch.zeros_like(sig))
    Gh = GU - isg[:, None, None] * GU[:, :, 0, None] * GU[:, None, 0, :]
    DU = torch.einsum("dji,djk,dki->di", Jz, Gh, Jz)
    top = DU.amax(-1, keepdim=True)
    top = torch.where(top > 0, top, torch.ones_like(top))
    DU = torch.maximum(DU, bq._EPS * top).contiguous()
    return pb._replace(q=qp.contiguous()), EqProblem(J, dv, tau, DU, F, pb.budget, KT)


def exposure_qp(X, cap, ret, ind, stats, P, F, spec_vol, factors, targets, q=None, lower=0.0,
                upper=1.0, budget=1.0, universe=None, tol: float = 1e-10, max_passes: int = 128,
                check_every: int = 4, *, torch_ops: bool = False, prev=None,
                tcost=None) -> ExposureQP | ExposureQPCost:
    """Solve the QP of the module docstring for every date.

    Panel arguments, ``F``, ``spec_vol``, ``q`` / ``lower`` / ``upper`` / ``budget`` /
    ``universe`` and the solver controls as :func:`.box_qp.box_qp`.  ``factors``: a list of m
    distinct factor indices in 1..K-1; ``targets`` [m] or [D, m] (a NaN target makes that date
    ``INVALID``).  ``factors=[]`` returns exactly what ``box_qp`` returns for the same arguments
    (mind the defaults: ``max_passes`` is 128 here and 32 there).  ``status`` as ``box_qp``;
    ``MAX_PASSES`` returns the last trial that held the budget, which is box- and
    budget-feasible, with its ``exposure_gap`` (an unattainable target ends this way).  ``ValueError`` before any
    launch for index 0, duplicates, indices out of range and, on the GPU, K > 64 or Q > 16.
    ``torch_ops`` runs the dense torch transcription on the tensors' device (the CPU path; on
    the GPU only as a timing comparison).  ``prev`` / ``tcost`` add linear trading costs as in
    :func:`.box_qp.box_qp` and return an :class:`ExposureQPCost`; with the multipliers ``eta``
    the sign convention of the module docstring holds with the cost's subgradient added."""
    bq.check_tcost(prev, tcost)
    D, Q, N = X.shape
    K = 1 + P + Q
    dev = X.device
    sel = check_factors(factors, K)
    m = len(sel)
    dense = torch_ops or not X.is_cuda
    if not dense:
        fc._check_limits(X, P)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    if m == 0:
        r = bq.box_qp(X, cap, ret, ind, stats, P, F, spec_vol, q, lower, upper, budget, universe,
                      tol, max_passes, check_every, torch_ops=torch_ops, prev=prev, tcost=tcost)
        gap = torch.where(r.status >= INFEASIBLE, nan, torch.zeros_like(r.variance))
        e = ExposureQP(r.weights, r.gamma, r.variance.new_zeros(D, 0), gap, r.variance,
                       r.passes, r.status)
        return e if tcost is None else ExposureQPCost(*e, r.turnover, r.cost)
    if D == 0:
        e = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)   # noqa: E731
        ei = lambda: torch.empty(0, dtype=torch.int32, device=dev)        # noqa: E731
        r = ExposureQP(e(0, N), e(0), e(0, m), e(0), e(0), ei(), ei())
        return r if tcost is None else ExposureQPCost(*r, e(0), e(0))
    pb = bq.make_problem(X, cap, ret, ind, stats, P, F, spec_vol, q, lower, upper, budget,
                         universe, dense, prev, tcost)
    pb, ep = make_eq_problem(pb, F, sel, targets)
    es = new_eq_state(D, K, dev)
    pjs = (bq.new_projection(D, N, dev), bq.new_projection(D, N, dev))
    st = es.step
    for it in range(1, max_passes + 1):
        # trial `it` goes into buffer it & 1, so that the trial before it survives it; gamma of
        # the running dates is carried over as the root find's warm start
        pj, last = pjs[it & 1], pjs[(it & 1) ^ 1]
        pj.gamma.copy_(torch.where(st.status == RUNNING, last.gamma, pj.gamma))
        G, x = bq.run_trial(pb, st, pj)
        eq_step(G, ep, x, pj.stats, pj.flag, es, tol, parity=it & 1, torch_ops=dense)
        if check_every and it % check_every == 0 and it < max_passes \
                and int((st.status == RUNNING).sum()) == 0:
            break
    status = torch.where((st.status == RUNNING) | (st.status == STALLED), MAX_PASSES,
                         st.status).to(torch.int32)
    dead = status >= INFEASIBLE
    odd = es.which == 1
    h = torch.where(odd[:, None], pjs[1].h, pjs[0].h)
    gam = torch.where(odd, pjs[1].gamma, pjs[0].gamma)
    r = ExposureQP(weights=torch.where(dead[:, None], nan, h),
                   gamma=torch.where(dead, nan, gam),
                   eta=torch.where((status != OK)[:, None], nan, es.eta[:, ep.KT:]),
                   exposure_gap=torch.where(dead, nan, st.ds[:, 3]),
                   variance=torch.where(dead, nan, st.ds[:, 2]),
                   passes=st.passes, status=status)
    return r if tcost is None else ExposureQPCost(*r, *bq.trade_stats(r.weights, prev, tcost))
