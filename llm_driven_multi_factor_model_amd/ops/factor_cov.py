"""Solve and product with the factor-structured asset covariance, without an N x N matrix.

For date d the model's asset covariance over the stock universe ``U_d`` is

    Sigma_d = X_d F_d X_d^T + diag(s_d^2)

with ``X_d`` the regression's design matrix [country | one-hot industries | cap-weighted
z-scored styles] (never materialised on the GPU: the kernels of ``csrc/factor_cov.hip`` stream
the raw panel and fold the z-scoring in from :attr:`XsResult.stats`), ``F_d`` a K x K factor
covariance and ``s_d`` the specific volatilities.  ``U_d`` = stocks that enter the regression
(:func:`..cross_section.valid_mask`) with a finite specific volatility > 0 and, optionally, a
caller's boolean ``universe``.  With ``a = 1 / s^2`` on ``U_d`` (0 elsewhere):

    G = X^T diag(a) X,   g = X^T (a o b),   F = R R^T  (R = U sqrt(max(lambda, 0)) from eigh),
    c = R (I + R^T G R)^-1 R^T g            (Cholesky of the always-SPD inner matrix; the only
                                             positive semi-definite F is never inverted),
    Sigma^-1 b = a o (b - X c),             Sigma h = s^2 o h + X (F (X^T h)).

Stocks outside ``U_d`` get 0; non-finite entries of ``b`` / ``h`` count as 0; a date whose ``F_d``
or ``stats`` row is not finite gets an all-NaN row.  CPU tensors take the float64 torch
transcription below (dense ``X_d``; also the tests' oracle); device tensors run the HIP kernels,
for K = 1 + P + Q <= 64 and Q <= 16 styles.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native
from . import eigen
from .attribution import portfolio_exposure
from .cross_section import valid_mask

MAX_K = eigen.WIDE_K   # the one-wave tier: M = I + R^T G R is factored in one workgroup's LDS
MAX_Q = 16
APPLY_NB = 8           # right-hand sides per mfa_factor_apply launch
XTY_NB = 4             # right-hand sides per mfa_factor_xty launch

_vp, _i = C.c_void_p, C.c_int
_native.register("mfa_factor_gram", [_vp] * 6 + [_i] * 4 + [_vp, _vp])
_native.register("mfa_factor_gram_f64", [_vp] * 6 + [_i] * 4 + [_vp, _vp])
_native.register("mfa_factor_xty", [_vp] * 6 + [_i] * 7 + [_vp, _vp])
_native.register("mfa_factor_xty_f64", [_vp] * 6 + [_i] * 7 + [_vp, _vp])
_native.register("mfa_woodbury_coef", [_vp] * 4 + [_i] * 3 + [_vp, _vp])
_native.register("mfa_factor_apply", [_vp] * 9 + [_i] * 7 + [_vp, _vp])
_native.register("mfa_factor_apply_f64", [_vp] * 9 + [_i] * 7 + [_vp, _vp])


def _check_limits(X: torch.Tensor, P: int) -> None:
    Q = X.shape[1]
    if X.is_cuda and (1 + P + Q > MAX_K or Q > MAX_Q):
        raise ValueError(f"factor_cov on the GPU supports K = 1 + P + Q <= {MAX_K} factors and "
                         f"Q <= {MAX_Q} styles; got K = {1 + P + Q}, Q = {Q}")


def _panel_args(X, cap, ret, ind, P):
    dt = X.dtype if X.dtype == torch.float64 else torch.float32
    X = _native.check_device_tensor(X, dt, "X")
    cap = _native.check_device_tensor(cap, dt, "cap")
    ret = _native.check_device_tensor(ret, dt, "ret")
    if P > 0:
        ind = _native.check_device_tensor(ind, torch.int16, "ind")
    return dt, X, cap, ret, (ind if P > 0 else None)


def _f64(t: torch.Tensor, shape, name: str) -> torch.Tensor:
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t.to(torch.float64).contiguous()


def universe_mask(X, cap, ret, ind, P, spec_vol, universe=None) -> torch.Tensor:
    """[D, N] bool: regression-valid stocks with a finite specific volatility > 0 (``spec_vol``
    [N] or [D, N]) that the optional boolean ``universe`` [D, N] keeps."""
    D, Q, N = X.shape
    s = spec_vol.to(device=X.device, dtype=torch.float64)
    s = s[None, :].expand(D, N) if s.dim() == 1 else s
    m = valid_mask(X, cap, ret, ind, P) & torch.isfinite(s) & (s > 0)
    if universe is not None:
        m = m & universe.to(device=X.device, dtype=torch.bool)
    return m


def _weights(X, cap, ret, ind, P, spec_vol, universe):
    """(a, s2) [D, N] float64: 1 / s^2 and s^2 where the specific volatility is finite and > 0
    and ``universe`` keeps the stock, 0 elsewhere.  The regression's validity rule is not applied
    here: :func:`factor_gram`, :func:`factor_xty` and :func:`factor_apply` apply it while
    they stream the panel, so the panel is not read an extra time for it."""
    D, Q, N = X.shape
    s = spec_vol.to(device=X.device, dtype=torch.float64)
    m = torch.isfinite(s) & (s > 0)
    zero = torch.zeros((), dtype=torch.float64, device=X.device)
    a, s2 = torch.where(m, 1.0 / (s * s), zero), torch.where(m, s * s, zero)
    if s.dim() == 1:
        a, s2 = a[None, :].expand(D, N), s2[None, :].expand(D, N)
    if universe is not None:
        u = universe.to(device=X.device, dtype=torch.bool)
        a, s2 = torch.where(u, a, zero), torch.where(u, s2, zero)
    return a, s2


def design_matrix(X, cap, ret, ind, stats, P, mask=None) -> torch.Tensor:
    """Dense float64 ``X_d`` [D, N, K] (zero rows for stocks outside ``mask``, default the
    regression's validity rule).  The CPU path and the tests' oracle; O(D N K) memory."""
    D, Q, N = X.shape
    m = valid_mask(X, cap, ret, ind, P) if mask is None else mask
    mu, sig = stats[:, :Q].double(), stats[:, Q].double()
    zero = torch.zeros((), dtype=torch.float64, device=X.device)
    Z = (X.double() - mu[:, :, None]) / sig[:, None, None]
    Z = torch.where(m[:, None, :], Z, zero)
    cols = [m.double()[..., None]]
    if P > 0:
        cols.append(torch.nn.functional.one_hot(ind.long().clamp(0, P - 1), P).double()
                    * m[..., None])
    cols.append(Z.transpose(1, 2))
    return torch.cat(cols, 2)


def _stats_ok(stats, Q):
    return torch.isfinite(stats[:, :Q + 1]).all(-1)


def factor_gram(X, cap, ret, ind, stats, P, a) -> torch.Tensor:
    """``G`` [D, K, K] float64 = X_d^T diag(a_d) X_d over the regression-valid stocks with a
    finite ``a`` [D, N] > 0.  NaN for a date whose ``stats`` row is not finite.  GPU: one
    workgroup per date, block-structured sums in a fixed order (bitwise reproducible)."""
    D, Q, N = X.shape
    K = 1 + P + Q
    _check_limits(X, P)
    a = _f64(a, (D, N), "a")
    stats = _f64(stats, (D, Q + 2), "stats")
    if not X.is_cuda:
        m = valid_mask(X, cap, ret, ind, P) & torch.isfinite(a) & (a > 0)
        Xd = design_matrix(X, cap, ret, ind, torch.nan_to_num(stats), P, m)
        G = torch.einsum("dnk,dn,dnl->dkl", Xd, torch.where(m, a, torch.zeros_like(a)), Xd)
        G[~_stats_ok(stats, Q)] = float("nan")
        return G
    dt, X, cap, ret, ind = _panel_args(X, cap, ret, ind, P)
    G = torch.empty(D, K, K, dtype=torch.float64, device=X.device)
    _native.call("mfa_factor_gram_f64" if dt == torch.float64 else "mfa_factor_gram",
                 _native.ptr(X), _native.ptr(cap), _native.ptr(ret), _native.ptr(ind),
                 _native.ptr(a), _native.ptr(stats), D, N, P, Q, _native.ptr(G),
                 _native.stream(X.device))
    return G


def woodbury_coef(G: torch.Tensor, F: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """``c`` [D, NB, K] = R (I + R^T G R)^-1 R^T g with F = R R^T from :func:`..eigen.eigh`
    (negative eigenvalues clamped to 0).  ``G`` / ``F`` [D, K, K], ``g`` [D, NB, K].  A date with
    a non-finite input gives NaN.  GPU: K <= 64, one workgroup per date (Cholesky in LDS)."""
    D, K = G.shape[0], G.shape[-1]
    NB = g.shape[1]
    if G.is_cuda and K > MAX_K:
        raise ValueError(f"woodbury_coef on the GPU supports K <= {MAX_K}, got K = {K}")
    G = _f64(G, (D, K, K), "G")
    g = _f64(g, (D, NB, K), "g")
    F = _f64(F, (D, K, K), "F")
    if D == 0 or NB == 0:
        return torch.empty(D, NB, K, dtype=torch.float64, device=G.device)
    w, U = eigen.eigh(F)
    if not G.is_cuda:
        R = U * torch.sqrt(w.clamp(min=0.0))[:, None, :]
        ok = (torch.isfinite(G).all(-1).all(-1) & torch.isfinite(R).all(-1).all(-1)
              & torch.isfinite(g).all(-1).all(-1))
        eye = torch.eye(K, dtype=torch.float64)
        M = torch.where(ok[:, None, None], eye + R.transpose(1, 2) @ G @ R, eye)
        L, info = torch.linalg.cholesky_ex(M)
        ok = ok & (info == 0)
        L = torch.where(ok[:, None, None], L, eye)
        p = torch.einsum("dji,dbj->dib", torch.nan_to_num(R), torch.nan_to_num(g))
        c = torch.einsum("dik,dkb->dbi", R, torch.cholesky_solve(p, L))
        c[~ok] = float("nan")
        return c
    c = torch.empty(D, NB, K, dtype=torch.float64, device=G.device)
    _native.call("mfa_woodbury_coef", _native.ptr(G), _native.ptr(w.contiguous()),
                 _native.ptr(U.contiguous()), _native.ptr(g), D, NB, K, _native.ptr(c),
                 _native.stream(G.device))
    return c


def factor_apply(X, cap, ret, ind, stats, P, u, v, rhs, c) -> torch.Tensor:
    """``out[d, b, n] = u[d, n] rhs[d, b, n] + v[d, n] (x_n . c[d, b])`` [D, NB, N] float64 on the
    regression-valid stocks with ``v != 0``; 0 elsewhere; non-finite ``rhs`` entries count as 0;
    NaN for every stock of a (date, rhs) whose ``c`` or ``stats`` is not finite.  GPU: one pass
    over the panel per block of up to ``APPLY_NB`` right-hand sides."""
    D, Q, N = X.shape
    K = 1 + P + Q
    NB = rhs.shape[1]
    _check_limits(X, P)
    u, v = _f64(u, (D, N), "u"), _f64(v, (D, N), "v")
    rhs, c = _f64(rhs, (D, NB, N), "rhs"), _f64(c, (D, NB, K), "c")
    stats = _f64(stats, (D, Q + 2), "stats")
    if not X.is_cuda:
        m = valid_mask(X, cap, ret, ind, P) & torch.isfinite(u) & torch.isfinite(v) & (v != 0)
        Xd = design_matrix(X, cap, ret, ind, torch.nan_to_num(stats), P, m)
        xc = torch.einsum("dnk,dbk->dbn", Xd, torch.nan_to_num(c))
        zero = torch.zeros((), dtype=torch.float64)
        out = torch.where(m, u, zero)[:, None] * torch.nan_to_num(rhs, nan=0.0, posinf=0.0,
                                                                   neginf=0.0) \
            + torch.where(m, v, zero)[:, None] * xc
        bad = ~torch.isfinite(c).all(-1) | ~_stats_ok(stats, Q)[:, None]
        out[bad] = float("nan")
        return out
    dt, X, cap, ret, ind = _panel_args(X, cap, ret, ind, P)
    out = torch.empty(D, NB, N, dtype=torch.float64, device=X.device)
    name = "mfa_factor_apply_f64" if dt == torch.float64 else "mfa_factor_apply"
    for b0 in range(0, NB, APPLY_NB):
        _native.call(name, _native.ptr(X), _native.ptr(cap), _native.ptr(ret), _native.ptr(ind),
                     _native.ptr(u), _native.ptr(v), _native.ptr(stats), _native.ptr(rhs),
                     _native.ptr(c), D, N, P, Q, NB, b0, min(APPLY_NB, NB - b0),
                     _native.ptr(out), _native.stream(X.device))
    return out


def _rhs3(rhs: torch.Tensor, D: int, N: int, device) -> tuple[torch.Tensor, bool]:
    rhs = rhs.to(device=device, dtype=torch.float64)
    flat = rhs.dim() == 2
    if flat:
        rhs = rhs[:, None, :]
    if rhs.dim() != 3 or rhs.shape[0] != D or rhs.shape[2] != N:
        raise ValueError(f"rhs must be [D, N] or [D, NB, N] with (D, N) = {(D, N)}, got "
                         f"{tuple(rhs.shape)}")
    return rhs.contiguous(), flat


def factor_xty(X, cap, ret, ind, stats, P, H) -> torch.Tensor:
    """``X_d^T h`` [D, NB, K] float64 for every right-hand side of ``H`` [D, NB, N]: the
    exposures of :func:`..attribution.portfolio_exposure` (invalid stocks and non-finite entries
    contribute nothing).  GPU: one pass over the panel per block of ``XTY_NB`` right-hand sides,
    sums in a fixed order (bitwise reproducible)."""
    D, Q, N = X.shape
    K = 1 + P + Q
    NB = H.shape[1]
    _check_limits(X, P)
    H = _f64(H, (D, NB, N), "H")
    stats = _f64(stats, (D, Q + 2), "stats")
    if not X.is_cuda:
        if NB == 0:
            return torch.empty(D, 0, K, dtype=torch.float64)
        return torch.stack([portfolio_exposure(X, cap, ret, ind, H[:, b], stats, P)
                            for b in range(NB)], 1)
    dt, X, cap, ret, ind = _panel_args(X, cap, ret, ind, P)
    out = torch.empty(D, NB, K, dtype=torch.float64, device=X.device)
    name = "mfa_factor_xty_f64" if dt == torch.float64 else "mfa_factor_xty"
    for b0 in range(0, NB, XTY_NB):
        _native.call(name, _native.ptr(X), _native.ptr(cap), _native.ptr(ret), _native.ptr(ind),
                     _native.ptr(H), _native.ptr(stats), D, N, P, Q, NB, b0,
                     min(XTY_NB, NB - b0), _native.ptr(out), _native.stream(X.device))
    return out


def solve_cov(X, cap, ret, ind, stats, P, F, spec_vol, rhs, universe=None) -> torch.Tensor:
    """``Sigma_d^-1 b`` for every date and right-hand side.

    ``X`` [D, Q, N], ``cap`` / ``ret`` [D, N], ``ind`` [D, N] int16 (None when P == 0) and
    ``stats`` [D, Q+2] are the regression's panel and :attr:`XsResult.stats`; ``F`` [D, K, K];
    ``spec_vol`` [N] or [D, N]; ``rhs`` [D, N] or [D, NB, N] (the result has the same shape),
    any NB; ``universe`` an optional [D, N] bool mask.  Stocks outside the universe get 0, dates
    with a non-finite ``F`` or ``stats`` row NaN.  GPU: K <= 64 and Q <= 16 (``ValueError``).
    """
    D, Q, N = X.shape
    _check_limits(X, P)
    rhs, flat = _rhs3(rhs, D, N, X.device)
    NB = rhs.shape[1]
    if D == 0 or NB == 0:
        out = torch.empty(D, NB, N, dtype=torch.float64, device=X.device)
        return out[:, 0] if flat else out
    a, _ = _weights(X, cap, ret, ind, P, spec_vol, universe)
    ab = a[:, None] * torch.nan_to_num(rhs, nan=0.0, posinf=0.0, neginf=0.0)
    G = factor_gram(X, cap, ret, ind, stats, P, a)
    g = factor_xty(X, cap, ret, ind, stats, P, ab)
    c = woodbury_coef(G, F.to(X.device), g)
    out = factor_apply(X, cap, ret, ind, stats, P, a, -a, rhs, c)
    return out[:, 0] if flat else out


def apply_cov(X, cap, ret, ind, stats, P, F, spec_vol, h, universe=None) -> torch.Tensor:
    """``Sigma_d h = s^2 o h + X (F (X^T h))`` restricted to the universe; arguments and
    conventions as :func:`solve_cov`."""
    D, Q, N = X.shape
    _check_limits(X, P)
    h, flat = _rhs3(h, D, N, X.device)
    NB = h.shape[1]
    if D == 0 or NB == 0:
        out = torch.empty(D, NB, N, dtype=torch.float64, device=X.device)
        return out[:, 0] if flat else out
    a, s2 = _weights(X, cap, ret, ind, P, spec_vol, universe)
    hu = (a > 0).double()[:, None] * torch.nan_to_num(h, nan=0.0, posinf=0.0, neginf=0.0)
    x = factor_xty(X, cap, ret, ind, stats, P, hu)
    c = torch.einsum("dkl,dbl->dbk", F.to(device=X.device, dtype=torch.float64), x)
    out = factor_apply(X, cap, ret, ind, stats, P, s2, (a > 0).double(), h, c)
    return out[:, 0] if flat else out
