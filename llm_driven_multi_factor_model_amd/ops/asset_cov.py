"""Dense asset covariance and correlation blocks of a basket of stocks.

Every portfolio method of this package applies the model's asset covariance

    Sigma_d = X_d F_d X_d^T + diag(s_d^2)

(:mod:`.factor_cov`) without forming it.  :func:`asset_cov` forms the block a user asks for,
``Sigma_d[S, S]`` for a basket ``S`` of M stocks: an index's constituents, a hedge set, the input
of an optimiser or a clustering of one's own.  For two valid members i, j of date d, with
``n_i = index[d, i]``:

    cov[d, i, j] = x_{n_i}^T F_d x_{n_j} + s_{n_i}^2 [n_i == n_j]

(the specific term is keyed on the stock, not the position: a name listed twice is the same
asset).  A member is *valid* when ``n_i >= 0`` and stock ``n_i`` is in the optimisers' universe
(:func:`.factor_cov.universe_mask`: the regression's validity rule, a finite specific volatility
> 0, the optional ``universe`` bit); rows and columns of the other members are NaN, and a date
whose ``F_d`` or ``stats`` row is not finite is all NaN with no valid member.  Only the entries
with i >= j are computed and mirrored, so ``cov[d]`` is symmetric bit for bit.  ``F`` is used as
given (no ``eigh``), which is what :func:`.factor_cov.apply_cov` applies.

CPU tensors take the float64 torch transcription (any K; also the tests' oracle); device
tensors run ``csrc/asset_cov.hip`` for K = 1 + P + Q <= 64 and Q <= 16 styles: the design rows
are gathered from the raw panel by stock index, the M x M block is an fp64 MFMA product written
once, whole rows at a time.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from .. import _native
from . import factor_cov as fcov
from .cross_section import valid_mask

SCRATCH_BYTES = 256 << 20   # bound on the (Z, Z F) scratch of one chunk of dates
MAX_CHUNK = 65535           # dates per launch (grid y)

_vp, _i, _ll = C.c_void_p, C.c_int, C.c_longlong
_SIG = [_vp] * 7 + [_ll, _vp, _ll, _vp] + [_i] * 7 + [_vp] * 7 + [_vp]
_native.register("mfa_asset_cov", _SIG)
_native.register("mfa_asset_cov_f64", _SIG)
_native.register("mfa_asset_cov_date_bytes", [_i, _i])


class AssetCov(NamedTuple):
    """:func:`asset_cov`: ``cov`` [D, M, M] float64 (the correlation when asked for), ``vol``
    [D, M] float64 total volatility, ``valid`` [D, M] bool, ``index`` as given ([M] or [D, M])."""
    cov: torch.Tensor
    vol: torch.Tensor
    valid: torch.Tensor
    index: torch.Tensor


def _check_index(index: torch.Tensor, D: int, N: int, device) -> torch.Tensor:
    if index.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64):
        raise TypeError(f"index must be an integer tensor, got {index.dtype}")
    if index.dim() not in (1, 2) or (index.dim() == 2 and index.shape[0] != D):
        raise ValueError(f"index must be [M] or [D, M] with D = {D}, got {tuple(index.shape)}")
    index = index.to(device)
    if index.numel() and (int(index.min()) < -1 or int(index.max()) >= N):
        raise ValueError(f"index entries must lie in [-1, {N}) (-1 = padding); got "
                         f"[{int(index.min())}, {int(index.max())}]")
    return index


def _reference(X, cap, ret, ind, stats, P, F, s, index, universe, correlation):
    """Dense float64 transcription on the gathered members (O(D M (K + M)) memory)."""
    D, Q, N = X.shape
    idx = index.long()
    idx = idx[None, :].expand(D, -1) if idx.dim() == 1 else idx
    M = idx.shape[1]
    at = idx.clamp(min=0)
    Xg = X.gather(2, at[:, None, :].expand(D, Q, M))
    capg, retg, sg = cap.gather(1, at), ret.gather(1, at), s.gather(1, at)
    indg = ind.gather(1, at) if P > 0 else None
    date_ok = fcov._stats_ok(stats, Q) & torch.isfinite(F).all(-1).all(-1)
    valid = (idx >= 0) & valid_mask(Xg, capg, retg, indg, P) & torch.isfinite(sg) & (sg > 0) \
        & date_ok[:, None]
    if universe is not None:
        valid = valid & universe.gather(1, at)
    Z = fcov.design_matrix(Xg, capg, retg, indg, torch.nan_to_num(stats), P, valid)  # [D, M, K]
    low = torch.tril((Z @ torch.nan_to_num(F)) @ Z.transpose(1, 2))   # i >= j only ...
    cov = low + torch.tril(low, -1).transpose(1, 2)                   # ... and its mirror
    zero = torch.zeros((), dtype=torch.float64)
    s2 = torch.where(valid, sg * sg, zero)
    cov = cov + torch.where(idx[:, :, None] == idx[:, None, :], s2[:, :, None], zero)
    nan = torch.full((), float("nan"), dtype=torch.float64)
    vol = torch.where(valid, torch.sqrt(torch.diagonal(cov, dim1=1, dim2=2)), nan)
    if correlation:
        cov = cov / (vol[:, :, None] * vol[:, None, :])
        torch.diagonal(cov, dim1=1, dim2=2).fill_(1.0)
    cov = torch.where(valid[:, :, None] & valid[:, None, :], cov, nan)
    return cov, vol, valid


def asset_cov(X, cap, ret, ind, stats, P, F, spec_vol, index, universe=None,
              correlation: bool = False) -> AssetCov:
    """The asset covariance (``correlation``: correlation) block of a basket on every date.

    ``X`` [D, Q, N], ``cap`` / ``ret`` [D, N], ``ind`` [D, N] int16 (None when P == 0) and
    ``stats`` [D, Q+2] are the regression's panel and :attr:`XsResult.stats`; ``F`` [D, K, K];
    ``spec_vol`` [N] or [D, N]; ``universe`` an optional [D, N] bool mask.  ``index`` holds stock
    positions: [M] is the same basket on every date (read in place, never expanded over the
    dates), [D, M] a basket per date with -1 as padding; any other value outside [-1, N) is a
    ``ValueError``; duplicates are legal.  With ``correlation`` the block holds
    ``cov_ij / (vol_i vol_j)`` and exactly 1.0 where i == j.  GPU: K <= 64 and Q <= 16
    (``ValueError``); bitwise reproducible, and date d does not depend on the other dates."""
    D, Q, N = X.shape
    K = 1 + P + Q
    fcov._check_limits(X, P)
    dev = X.device
    index = _check_index(index, D, N, dev)
    M = index.shape[-1]
    stats = fcov._f64(stats, (D, Q + 2), "stats")
    F = fcov._f64(F.to(dev), (D, K, K), "F")
    s = spec_vol.to(device=dev, dtype=torch.float64)
    if s.dim() == 1:
        s = fcov._f64(s, (N,), "spec_vol")
    else:
        s = fcov._f64(s, (D, N), "spec_vol")
    if universe is not None:
        universe = universe.to(device=dev, dtype=torch.bool)
        if tuple(universe.shape) != (D, N):
            raise ValueError(f"universe must be {(D, N)}, got {tuple(universe.shape)}")
        universe = universe.contiguous()
    if D == 0 or M == 0:
        return AssetCov(torch.empty(D, M, M, dtype=torch.float64, device=dev),
                        torch.empty(D, M, dtype=torch.float64, device=dev),
                        torch.empty(D, M, dtype=torch.bool, device=dev), index)
    if not X.is_cuda:
        sd = s[None, :].expand(D, N) if s.dim() == 1 else s
        return AssetCov(*_reference(X, cap, ret, ind, stats, P, F, sd, index, universe,
                                    correlation), index)
    dt, X, cap, ret, ind = fcov._panel_args(X, cap, ret, ind, P)
    idx32 = index.to(torch.int32).contiguous()
    cov = torch.empty(D, M, M, dtype=torch.float64, device=dev)
    vol = torch.empty(D, M, dtype=torch.float64, device=dev)
    valid = torch.empty(D, M, dtype=torch.bool, device=dev)
    # dates run in chunks, so that the scratch (Z, Z F, s^2, stock id per member) stays bounded;
    # the chunks queue on one stream, with no host synchronisation between them
    per_date = _native.query("mfa_asset_cov_date_bytes", M, K)
    chunk = max(1, min(D, MAX_CHUNK, SCRATCH_BYTES // per_date))
    KP = 16 * ((K + 15) // 16)
    zy = torch.empty(2, chunk, M, KP, dtype=torch.float64, device=dev)
    s2 = torch.empty(chunk, M, dtype=torch.float64, device=dev)
    nid = torch.empty(chunk, M, dtype=torch.int32, device=dev)
    uni = universe.view(torch.uint8) if universe is not None else None
    name = "mfa_asset_cov_f64" if dt == torch.float64 else "mfa_asset_cov"
    for d0 in range(0, D, chunk):
        _native.call(name, _native.ptr(X), _native.ptr(cap), _native.ptr(ret), _native.ptr(ind),
                     _native.ptr(stats), _native.ptr(F), _native.ptr(s),
                     0 if s.dim() == 1 else N, _native.ptr(idx32),
                     0 if idx32.dim() == 1 else M, _native.ptr(uni), d0, min(chunk, D - d0), N,
                     P, Q, M, int(bool(correlation)), _native.ptr(zy[0]), _native.ptr(zy[1]),
                     _native.ptr(s2), _native.ptr(nid), _native.ptr(cov), _native.ptr(vol),
                     _native.ptr(valid), _native.stream(dev))
    return AssetCov(cov, vol, valid, index)
