"""Pure factor portfolios and factor-return t-statistics of the cross-sectional regression.

For date d the regression of :func:`..cross_section.xs_wls` is the linear estimator
``f_d = Omega_d r_d``.  Everything about it comes from one K x K matrix, the estimator covariance

    C_d = R_d (R_d^T X_d^T W_d X_d R_d)^+ R_d^T,

with ``W = diag(sqrt(cap))`` on the regression-valid stocks, ``R_d`` the industry-neutral
constraint matrix of :func:`..cross_section.xs_wls_reference` (the identity with one pivot row) and
``^+`` the pseudo-inverse that drops eigenvalues <= 1e-15 lambda_max:

    Omega_d  = C_d X_d^T W_d                  the K x N pure factor portfolios (row k has unit
                                              exposure to factor k and none to the others),
    Var(f_d) = sigma_d^2 C_d,                 sigma_d^2 = sum w e^2 / (n - rank).

:func:`estimator_cov` forms ``C``, :func:`pure_factor_weights` any rows of ``Omega`` for every
date in one pass over the raw panel, :func:`factor_return_stats` standard errors and t-statistics.
Every function takes the panel arguments ``(X, cap, ret, ind, stats, P)`` of :mod:`.factor_cov`.
CPU tensors take the float64 torch transcription below (dense ``design_matrix``, batched
``pinv``, any K; also the tests' oracle); device tensors run the kernels of
``csrc/pure_factor.hip``, for K = 1 + P + Q <= 64 and Q <= 16 styles (``ValueError``).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from .. import _native
from . import factor_cov as fcov
from .cross_section import valid_mask

ROWS_NB = 64   # rows of C per mfa_pure_factor_weights launch (they live in LDS)

_vp, _i = C.c_void_p, C.c_int
_native.register("mfa_est_cov", [_vp] * 3 + [_i] * 4 + [_vp] * 3)
_native.register("mfa_pure_factor_weights", [_vp] * 7 + [_i] * 7 + [_vp, _vp])
_native.register("mfa_pure_factor_weights_f64", [_vp] * 7 + [_i] * 7 + [_vp, _vp])
_native.register("mfa_factor_stats", [_vp] * 9 + [_i] * 4 + [_vp] * 5)
_native.register("mfa_factor_stats_f64", [_vp] * 9 + [_i] * 4 + [_vp] * 5)


class EstCov(NamedTuple):
    """:func:`estimator_cov`: ``C`` [D, K, K] float64 (symmetric), ``rank`` [D] int32 (eigenvalues
    kept by the pseudo-inverse), ``n`` [D] float64 (stocks in the regression,
    ``stats[:, Q + 1]``)."""
    C: torch.Tensor
    rank: torch.Tensor
    n: torch.Tensor


class FactorStats(NamedTuple):
    """:func:`factor_return_stats`: ``se`` / ``t`` [D, K], ``sigma2`` / ``dof`` [D] (float64)."""
    se: torch.Tensor
    t: torch.Tensor
    sigma2: torch.Tensor
    dof: torch.Tensor


def _bad_stats(stats: torch.Tensor, Q: int) -> torch.Tensor:
    return ~fcov._stats_ok(stats, Q) | ~(stats[:, Q] > 0)


def _safe_stats(stats: torch.Tensor, Q: int) -> torch.Tensor:
    """``stats`` with the rows of :func:`_bad_stats` replaced by (mu 0, sigma 1), so that the dense
    design matrix of such a date holds no NaN (its outputs are overwritten afterwards)."""
    st = stats.clone()
    bad = _bad_stats(stats, Q)
    st[bad] = 0.0
    st[bad, Q] = 1.0
    return st


def _dense(X, cap, ret, ind, stats, P):
    """(X_d [D, N, K], w [D, N]): the dense design matrix and the regression weights sqrt(cap),
    both zero outside the regression."""
    Q = X.shape[1]
    m = valid_mask(X, cap, ret, ind, P)
    zero = torch.zeros((), dtype=torch.float64)
    w = torch.where(m, torch.sqrt(torch.where(m, cap.double(), zero)), zero)
    return fcov.design_matrix(X, cap, ret, ind, _safe_stats(stats, Q), P, m), w


def constraint_matrix(s: torch.Tensor, pivot_mode: int = 0):
    """The constraint of every date from its raw industry caps ``s`` [D, P].

    Returns ``(piv, ratio, ok)``: the pivot industry of every date (pivot_mode 0: the last with
    ``s_j > 0``; 1: the last), ``ratio[d, j] = -s_j / s_pivot`` and whether the pivot is
    non-empty, exactly the choices of :func:`..cross_section.xs_wls_reference`."""
    D, P = s.shape
    if pivot_mode == 1:
        piv = torch.full((D,), P - 1, dtype=torch.long)
    else:
        idx = torch.where(s > 0, torch.arange(P).expand(D, P), torch.full((D, P), -1))
        piv = idx.max(1).values
        piv = torch.where(piv < 0, torch.full_like(piv, P - 1), piv)
    sp = s.gather(1, piv[:, None]).squeeze(1)
    ok = torch.isfinite(sp) & (sp > 0)
    ratio = -s / torch.where(ok, sp, torch.ones_like(sp))[:, None]
    return piv, ratio, ok


def _constraint_dense(piv, ratio, K: int, P: int) -> torch.Tensor:
    """R [D, K, K - 1]: the identity with row 1 + piv replaced by ``ratio`` over the industry
    columns, and column 1 + piv dropped."""
    D = piv.shape[0]
    Rm = torch.eye(K, dtype=torch.float64).repeat(D, 1, 1)
    rows = 1 + piv
    Rm[torch.arange(D), rows, 1:1 + P] = ratio
    keep = torch.ones(D, K, dtype=torch.bool)
    keep[torch.arange(D), rows] = False
    return Rm[keep[:, None, :].expand(-1, K, -1)].view(D, K, K - 1)


def _estimator_cov_reference(X, cap, ret, ind, stats, P, pivot_mode):
    D, Q, N = X.shape
    K = 1 + P + Q
    Xd, w = _dense(X, cap, ret, ind, stats, P)
    G = torch.einsum("dnk,dn,dnl->dkl", Xd, w, Xd)
    bad = _bad_stats(stats, Q) | ~(G[:, 0, 0] > 0) | ~torch.isfinite(G).all(-1).all(-1)
    Rm = None
    if P > 0:
        capz = torch.where(w > 0, cap.double(), torch.zeros((), dtype=torch.float64))
        s = torch.einsum("dnp,dn->dp", Xd[:, :, 1:1 + P], capz)
        piv, ratio, ok = constraint_matrix(torch.nan_to_num(s), pivot_mode)
        bad = bad | ~ok
        Rm = _constraint_dense(piv, ratio, K, P)
    eye = torch.eye(K, dtype=torch.float64)
    G = torch.where(bad[:, None, None], eye, G)
    A = Rm.transpose(1, 2) @ G @ Rm if Rm is not None else G
    A = 0.5 * (A + A.transpose(1, 2))
    Ai = torch.linalg.pinv(A, rtol=1e-15, hermitian=True)
    # an empty industry is an exact zero row and column of A: so it is of the pseudo-inverse
    # (LAPACK leaves rounding noise there, which would make its standard error 1e-17, not 0)
    z = (A == 0).all(-1)
    Ai = torch.where(z[:, :, None] | z[:, None, :], torch.zeros((), dtype=torch.float64), Ai)
    rank = torch.linalg.matrix_rank(A, rtol=1e-15, hermitian=True).to(torch.int32)
    Cm = Rm @ Ai @ Rm.transpose(1, 2) if Rm is not None else Ai
    Cm = 0.5 * (Cm + Cm.transpose(1, 2))
    Cm[bad] = float("nan")
    rank[bad] = 0
    return Cm, rank


def estimator_cov(X, cap, ret, ind, stats, P, pivot_mode: int = 0) -> EstCov:
    """Estimator covariance ``C_d = R (R^T X^T W X R)^+ R^T`` of every date.

    ``X`` [D, Q, N], ``cap`` / ``ret`` [D, N], ``ind`` [D, N] int16 (None when P == 0) and
    ``stats`` [D, Q+2] are the regression's panel and :attr:`XsResult.stats`; ``pivot_mode`` as
    :func:`..cross_section.xs_wls` (0: the last non-empty industry is eliminated, 1: the last).
    A date gets NaN ``C`` and rank 0 when its ``stats`` row is not finite, its sigma is not > 0,
    it has no valid stock (no weight), or its pivot industry is empty (pivot_mode 1).

    GPU: two :func:`.factor_cov.factor_gram` passes over the panel (``a = sqrt(cap)`` for
    ``G = X^T W X``; ``a = cap`` for the raw industry caps the constraint needs, row 0 of that
    Gram; skipped when P == 0; each pass takes 0.28 ms at 2520 x 5000 x 42 on an MI355X,
    ``profiles/r11/pure_factor_bench.log``), then one workgroup per date: ``A = R^T G R`` in LDS, one-wave
    Jacobi, products in a fixed order (bitwise reproducible)."""
    D, Q, N = X.shape
    K = 1 + P + Q
    fcov._check_limits(X, P)
    if pivot_mode not in (0, 1):
        raise ValueError(f"pivot_mode must be 0 or 1, got {pivot_mode}")
    stats = fcov._f64(stats, (D, Q + 2), "stats")
    n = stats[:, Q + 1].clone()
    if not X.is_cuda:
        Cm, rank = _estimator_cov_reference(X, cap, ret, ind, stats, P, pivot_mode)
        return EstCov(Cm, rank, n)
    Cm = torch.empty(D, K, K, dtype=torch.float64, device=X.device)
    rank = torch.empty(D, dtype=torch.int32, device=X.device)
    if D == 0:
        return EstCov(Cm, rank, n)
    c64 = cap.to(torch.float64)
    G = fcov.factor_gram(X, cap, ret, ind, stats, P, torch.sqrt(c64))
    Gs = fcov.factor_gram(X, cap, ret, ind, stats, P, c64) if P > 0 else None
    _native.call("mfa_est_cov", _native.ptr(G), _native.ptr(Gs), _native.ptr(stats), D, P, Q,
                 pivot_mode, _native.ptr(Cm), _native.ptr(rank), _native.stream(X.device))
    return EstCov(Cm, rank, n)


def _selection(factors, K: int, device) -> torch.Tensor:
    if factors is None:
        return torch.arange(K, dtype=torch.int64, device=device)
    sel = torch.as_tensor(factors, dtype=torch.int64).reshape(-1)
    if sel.numel() and (int(sel.min()) < 0 or int(sel.max()) >= K):
        raise ValueError(f"factors must index the K = {K} factors, got {sel.tolist()}")
    return sel.to(device)


def pure_factor_weights(X, cap, ret, ind, stats, P, C, factors=None) -> torch.Tensor:
    """Pure factor portfolios ``Omega`` [D, S, N] float64 of the selected factors:
    ``Omega[d, j, n] = sqrt(cap_n) sum_k C[d, sel_j, k] x_{n, k}`` on the regression-valid stocks,
    0 on the others, so that ``Omega[d] @ ret[d]`` (over the valid stocks) is the factor return.

    ``C`` [D, K, K] is :attr:`EstCov.C`; ``factors`` an int64 index list into K (None: all K
    factors).  A date whose ``C`` or ``stats`` row is not finite (or whose sigma is not > 0) gets
    NaN for every stock.  The output takes ``D S N 8`` bytes.

    GPU: one pass over the raw panel per ``ROWS_NB`` = 64 rows, the selected rows of ``C`` in LDS
    with the z-scoring folded in, non-temporal stores; bitwise reproducible, and row j depends
    neither on the other rows asked for nor on its place in ``factors``."""
    D, Q, N = X.shape
    K = 1 + P + Q
    fcov._check_limits(X, P)
    stats = fcov._f64(stats, (D, Q + 2), "stats")
    Cm = fcov._f64(C.to(X.device), (D, K, K), "C")
    sel = _selection(factors, K, X.device)
    S = sel.numel()
    if not X.is_cuda:
        Xd, w = _dense(X, cap, ret, ind, stats, P)
        out = torch.einsum("dsk,dnk->dsn", torch.nan_to_num(Cm[:, sel]), Xd) * w[:, None, :]
        out[~torch.isfinite(Cm).all(-1).all(-1) | _bad_stats(stats, Q)] = float("nan")
        return out
    dt, X, cap, ret, ind = fcov._panel_args(X, cap, ret, ind, P)
    out = torch.empty(D, S, N, dtype=torch.float64, device=X.device)
    if D == 0 or S == 0:
        return out
    sel32 = sel.to(torch.int32).contiguous()
    name = "mfa_pure_factor_weights_f64" if dt == torch.float64 else "mfa_pure_factor_weights"
    for b0 in range(0, S, ROWS_NB):
        _native.call(name, _native.ptr(X), _native.ptr(cap), _native.ptr(ret), _native.ptr(ind),
                     _native.ptr(stats), _native.ptr(Cm), _native.ptr(sel32), D, N, P, Q, S, b0,
                     min(ROWS_NB, S - b0), _native.ptr(out), _native.stream(X.device))
    return out


def factor_return_stats(X, cap, ret, ind, stats, P, f, resid, est: EstCov) -> FactorStats:
    """Standard errors and t-statistics of the factor returns ``f`` [D, K] with residuals
    ``resid`` [D, N] (:attr:`XsResult.f` / :attr:`XsResult.resid`) and ``est`` from
    :func:`estimator_cov`:

        dof = n - rank,  sigma2 = sum_valid sqrt(cap) e^2 / dof,  se_k = sqrt(sigma2 C_kk),
        t_k = f_k / se_k.

    ``dof <= 0`` gives NaN ``sigma2``, ``se`` and ``t``; ``se_k == 0`` (an empty industry, whose
    ``f_k`` is 0) NaN ``t_k``.  The sum runs over the regression-valid stocks with a finite
    residual.  GPU: one workgroup per date, a fixed-order reduction (bitwise reproducible)."""
    D, Q, N = X.shape
    K = 1 + P + Q
    fcov._check_limits(X, P)
    dev = X.device
    f = fcov._f64(f.to(dev), (D, K), "f")
    Cm = fcov._f64(est.C.to(dev), (D, K, K), "est.C")
    n = fcov._f64(est.n.to(dev), (D,), "est.n")
    rank = est.rank.to(device=dev, dtype=torch.int32).contiguous()
    if tuple(resid.shape) != (D, N):
        raise ValueError(f"resid must be {(D, N)}, got {tuple(resid.shape)}")
    if tuple(rank.shape) != (D,):
        raise ValueError(f"est.rank must be {(D,)}, got {tuple(rank.shape)}")
    if not X.is_cuda:
        e = resid.double()
        m = valid_mask(X, cap, ret, ind, P) & torch.isfinite(e)
        zero = torch.zeros((), dtype=torch.float64)
        w = torch.sqrt(torch.where(m, cap.double(), zero))
        dof = n - rank.double()
        nan = torch.full_like(dof, float("nan"))
        ok = torch.isfinite(dof) & (dof > 0)
        sigma2 = torch.where(ok, torch.where(m, w * e * e, zero).sum(1)
                             / torch.where(ok, dof, torch.ones_like(dof)), nan)
        se = torch.sqrt(sigma2[:, None] * torch.diagonal(Cm, dim1=-2, dim2=-1))
        t = torch.where(se > 0, f / se, torch.full_like(se, float("nan")))
        return FactorStats(se, t, sigma2, dof)
    dt, X, cap, ret, ind = fcov._panel_args(X, cap, ret, ind, P)
    resid = _native.check_device_tensor(resid.to(device=dev, dtype=dt), dt, "resid")
    se = torch.empty(D, K, dtype=torch.float64, device=dev)
    t = torch.empty(D, K, dtype=torch.float64, device=dev)
    sigma2 = torch.empty(D, dtype=torch.float64, device=dev)
    dof = torch.empty(D, dtype=torch.float64, device=dev)
    if D > 0:
        _native.call("mfa_factor_stats_f64" if dt == torch.float64 else "mfa_factor_stats",
                     _native.ptr(X), _native.ptr(cap), _native.ptr(ret), _native.ptr(ind),
                     _native.ptr(resid), _native.ptr(Cm), _native.ptr(f), _native.ptr(rank),
                     _native.ptr(n), D, N, P, Q, _native.ptr(se), _native.ptr(t),
                     _native.ptr(sigma2), _native.ptr(dof), _native.stream(dev))
    return FactorStats(se, t, sigma2, dof)
