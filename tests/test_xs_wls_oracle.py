"""Cross-sectional WLS regression (``ops/cross_section.py::xs_wls``, kernels in
``csrc/xs_wls_impl.h``) against a per-date high-precision numpy oracle, at the edges of the
kernels' control flow: sizes around the 64-stock wave tile, the 256-stock workgroup step, the
residual pass's prefetched tail (768 fp64 / 1536 fp32 stocks) and its main block (1024 / 3072),
the 513-date shard that moves fp64 panels onto the LDS-DMA ring, every validity channel alone,
empty tiles and dates, rank-deficient and degenerate dates, the shapes at which the industry table
and the solve change, and a raw-SIZE-like style column whose mean is 13 standard deviations from 0.

The oracle (``oracle_date``) is written from the semantics of the reference's ``CrossSection``
(cap-weighted style means, one pooled ddof-0 sigma, design ``[1 | one-hot | z]``, the industry
constraint with the last non-empty industry as pivot, weights sqrt(cap), minimum-norm solution,
``e = r - X f``, unweighted R^2), not from the package's own CPU path: inputs as stored (float32
values are exact), every moment in ``np.longdouble`` with two-pass deviations, and no normal
equations -- ``sqrt(w) Xt g = sqrt(w) r`` by float64 ``lstsq`` (rcond 3e-8, the square root of
pinv's 1e-15 on the normal matrix) refined four times with longdouble residuals.  It asserts
itself that the singular values of the scaled design are either above 1e-5 or below 1e-12 of the
largest, so no rank decision depends on which cut is used.  Every case runs against the oracle
twice: through the CPU path (unmarked) and through the HIP kernels (``gpu``), production library
only.

Tolerance rule.  ``atol_case`` is measured here, on the CPU, from the inputs alone: the same
regression computed a second, independent way in plain float64 numpy, the way a float64
raw-moment implementation is entitled to (raw Gram and cross moments of ``[1 | one-hot | x]``
accumulated sequentially, algebraic centring and scaling, ``pinv(A, rcond=1e-15)``, one-pass R^2
sums), 8 x its largest deviation from the oracle over the case, separately for f, e, r2 and the
stats (mu, sigma).  Then, per date d,

    f:              |got - oracle| <= 4 eps64 max|f_d| + atol_f
    e, fp64 panel:  |got - oracle| <= 4 eps64 max|r_d| + atol_e
    e, fp32 panel:  |got - oracle| <= 2**-24 |oracle| + atol_e      (float64 rounded once)
    r2:             |got - oracle| <= 4 eps64 + atol_r2
    mu, sigma:      |got - oracle| <= 4 eps64 |oracle| + atol_stats

n, the NaN positions and ``status & (NO_ROWS | PIVOT_EMPTY | BAD_SIGMA)`` must match exactly; on
the GPU a rank-deficient date must carry ``XS_REFINED`` and a well-conditioned one status 0.  The
bound is never derived from the output under test; the values measured when the cases were written
stand beside each case and the assertion message prints the one in force.  No date and no output
is left out, except r2 of a date whose oracle var(r) is exactly 0.
"""
import functools

import numpy as np
import pytest
import torch

from llm_driven_multi_factor_model_amd.ops import cross_section as X
from llm_driven_multi_factor_model_amd.ops import xs_sharded as S

LD = np.longdouble
F64 = np.float64
EPS = float(np.finfo(np.float64).eps)
U32 = 2.0 ** -24
BAD = X.XS_NO_ROWS | X.XS_PIVOT_EMPTY | X.XS_BAD_SIGMA
DT = {"f32": np.float32, "f64": np.float64}
NAN, INF = float("nan"), float("inf")
PRE = {"f32": 1536, "f64": 768}       # stocks of the residual pass's prefetched tail


@pytest.fixture(params=[pytest.param("cpu"), pytest.param("hip", marks=pytest.mark.gpu)])
def dev(request):
    if request.param == "cpu":
        return torch.device("cpu")
    return request.getfixturevalue("cuda")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


# ============================================================================== the oracle
def _valid(x, cap, ret, ind, P):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(cap) & (cap >= 0) & np.isfinite(ret) & np.isfinite(x).all(0)
    if P > 0:
        ok &= (ind >= 0) & (ind < P)
    return ok


def _pivot(s, P, pivot_mode):
    if pivot_mode == 1:
        return P - 1
    nz = np.nonzero(s > 0)[0]
    return int(nz[-1]) if nz.size else P - 1


def _constraint(s, piv, P, Q, T):
    """``R`` of ``CrossSection.reg``: identity with the pivot industry's row replaced by
    ``-s_j / s_pivot`` and the pivot's column deleted (identity when there are no industries)."""
    K = 1 + P + Q
    R = np.eye(K, dtype=T)
    if P > 0:
        R[1 + piv, 1:1 + P] = -s / s[piv]
        R = np.delete(R, 1 + piv, axis=1)
    return R


def _empty(Q, N, K, T):
    return dict(f=np.full(K, np.nan, dtype=T), e=np.full(N, np.nan, dtype=T), r2=T(np.nan),
                mu=np.full(Q, np.nan, dtype=T), sigma=T(np.nan), n=0, bad=0, deficient=False,
                rmax=0.0, r2_defined=True)


def oracle_date(x, cap, ret, ind, P, pivot_mode=0):
    """One date: x [Q, N], cap / ret [N] as stored, ind [N] int16 (None when P == 0)."""
    Q, N = x.shape
    K = 1 + P + Q
    o = _empty(Q, N, K, LD)
    ok = _valid(x, cap, ret, ind, P)
    n = o["n"] = int(ok.sum())
    if n == 0:      # the pooled sigma of no entries is NaN and no industry has capital
        o["bad"] = X.XS_NO_ROWS | X.XS_BAD_SIGMA | (X.XS_PIVOT_EMPTY if P > 0 else 0)
        return o
    c, r, xv = cap[ok].astype(LD), ret[ok].astype(LD), x[:, ok].astype(LD)
    o["rmax"] = float(np.abs(r).max())
    mu = o["mu"] = (xv * c).sum(1) / c.sum()
    m = xv.sum() / LD(xv.size)
    sigma = o["sigma"] = np.sqrt(((xv - m) ** 2).sum() / LD(xv.size))
    if not (sigma > 0 and np.isfinite(sigma)):
        o["bad"] |= X.XS_BAD_SIGMA
    oh = np.zeros((n, P), dtype=LD)
    piv = 0
    if P > 0:
        oh[np.arange(n), ind[ok].astype(np.int64)] = 1
        s = (oh * c[:, None]).sum(0)
        piv = _pivot(s, P, pivot_mode)
        if not s[piv] > 0:
            o["bad"] |= X.XS_PIVOT_EMPTY
    else:
        s = np.zeros(0, dtype=LD)
    rm = r.sum() / LD(n)
    var_r = ((r - rm) ** 2).sum() / LD(n)
    o["r2_defined"] = bool(var_r != 0)
    if o["bad"]:
        return o
    Xf = np.concatenate([np.ones((n, 1), dtype=LD), oh, ((xv - mu[:, None]) / sigma).T], 1)
    R = _constraint(s, piv, P, Q, LD)
    sw = np.sqrt(np.sqrt(c))                 # WLS weights sqrt(cap): rows scaled by their root
    M, y = sw[:, None] * (Xf @ R), sw * r
    M64 = M.astype(F64)
    sv = np.linalg.svd(M64, compute_uv=False)
    assert ((sv > 1e-5 * sv[0]) | (sv < 1e-12 * sv[0])).all(), \
        f"singular values too close to the rank cut: {sv / sv[0]}"
    o["deficient"] = bool((sv > 1e-5 * sv[0]).sum() < np.count_nonzero(np.abs(M64).max(0)))
    g = np.linalg.lstsq(M64, y.astype(F64), rcond=3e-8)[0].astype(LD)
    for _ in range(4):
        g = g + np.linalg.lstsq(M64, (y - M @ g).astype(F64), rcond=3e-8)[0].astype(LD)
    f = o["f"] = R @ g
    ev = r - Xf @ f
    o["e"][ok] = ev
    o["r2"] = 1 - (((ev - ev.sum() / LD(n)) ** 2).sum() / LD(n)) / var_r if var_r != 0 else LD(np.nan)
    return o


def _seq(a):
    """Sequential (left to right, not pairwise) float64 sum over axis 0."""
    return np.cumsum(a, axis=0)[-1]


def second_date(x, cap, ret, ind, P, pivot_mode=0):
    """The second opinion: float64 raw moments, algebraic centring, pinv of the normal matrix."""
    Q, N = x.shape
    K = 1 + P + Q
    o = _empty(Q, N, K, F64)
    ok = _valid(x, cap, ret, ind, P)
    n = int(ok.sum())
    if n == 0:
        return o
    c, r, xv = cap[ok].astype(F64), ret[ok].astype(F64), x[:, ok].astype(F64).T
    oh = np.zeros((n, P))
    if P > 0:
        oh[np.arange(n), ind[ok].astype(np.int64)] = 1
    U = np.concatenate([np.ones((n, 1)), oh, xv], 1)
    w = np.sqrt(c)
    G = np.stack([_seq(U * (w * U[:, i])[:, None]) for i in range(K)])
    h = _seq(U * (w * r)[:, None])
    s = _seq(oh * c[:, None]) if P > 0 else np.zeros(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = o["mu"] = _seq(c[:, None] * xv) / _seq(c)
        nq = float(n * Q)
        sigma = o["sigma"] = np.sqrt(max(_seq((xv * xv).reshape(-1)) / nq - (_seq(xv.reshape(-1)) / nq) ** 2, 0.0))
    piv = _pivot(s, P, pivot_mode) if P > 0 else 0
    if not (sigma > 0 and np.isfinite(sigma)) or (P > 0 and not s[piv] > 0):
        return o
    T = np.eye(K)
    T[0, 1 + P:] = -mu / sigma
    T[1 + P:, 1 + P:] = np.eye(Q) / sigma
    R = _constraint(s, piv, P, Q, F64)
    TR = T @ R
    g = np.linalg.pinv(TR.T @ G @ TR, rcond=1e-15) @ (TR.T @ h)
    o["f"] = R @ g
    ev = r - U @ (TR @ g)
    o["e"][ok] = ev
    vr = _seq(r * r) / n - (_seq(r) / n) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        o["r2"] = 1.0 - (_seq(ev * ev) / n - (_seq(ev) / n) ** 2) / vr if vr != 0 else np.nan
    return o


def _dev(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    fin = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a[fin] - b[fin]))) if fin.any() else 0.0


class Case:
    """A panel, its oracle and its measured ``atol_case``."""

    def __init__(self, x, cap, ret, ind, P, pivot_mode=0):
        self.x, self.cap, self.ret, self.ind, self.P, self.pivot_mode = x, cap, ret, ind, P, pivot_mode
        self.D, self.Q, self.N = x.shape
        self.fp32 = x.dtype == np.float32
        dates = [(x[d], cap[d], ret[d], ind[d] if P > 0 else None, P, pivot_mode) for d in range(self.D)]
        o = [oracle_date(*a) for a in dates]
        s = [second_date(*a) for a in dates]
        st = lambda L, k: np.stack([np.asarray(v[k]) for v in L])       # noqa: E731
        self.f, self.e, self.r2 = st(o, "f"), st(o, "e"), st(o, "r2")
        self.stats = np.concatenate([st(o, "mu"), st(o, "sigma")[:, None]], 1)
        self.n = np.array([v["n"] for v in o])
        self.bad = np.array([v["bad"] for v in o])
        self.deficient = np.array([v["deficient"] for v in o])
        self.rmax = np.array([v["rmax"] for v in o])
        self.r2_defined = np.array([v["r2_defined"] for v in o])
        s_stats = np.concatenate([st(s, "mu"), st(s, "sigma")[:, None]], 1)
        self.atol = dict(f=8 * _dev(st(s, "f"), self.f), e=8 * _dev(st(s, "e"), self.e),
                         r2=8 * _dev(st(s, "r2"), self.r2), stats=8 * _dev(s_stats, self.stats))

    def tensors(self, dev, idx=None):
        sel = (lambda a: a) if idx is None else (lambda a: a[idx])
        return (_t(sel(self.x), dev), _t(sel(self.cap), dev), _t(sel(self.ret), dev),
                _t(sel(self.ind), dev) if self.P > 0 else None)

    def run(self, dev, idx=None, fn=None, **kw):
        out = (fn or X.xs_wls)(*self.tensors(dev, idx), self.P, pivot_mode=self.pivot_mode, **kw)
        if dev.type != "cpu":
            torch.cuda.synchronize()
        return out


def _cmp(got, want, bound, what, atol):
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=LD)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), \
        f"{what}: NaN positions differ at {np.argwhere(np.isnan(got) != nan)[:5].tolist()}"
    err = np.abs(got.astype(LD) - want)
    bound = np.broadcast_to(bound, want.shape)
    if (~nan).any():      # the figures, before any assertion on them (shown with ``pytest -s``)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = float(np.nanmax(np.append(err[~nan] / bound[~nan], LD(0))))
        print(f"{what}: max |err| {float(err[~nan].max()):.3g}, max |err| / bound {worst:.3g}")
    bad = ~nan & ~(err <= bound)
    if bad.any():
        ex = np.where(nan, -np.inf, (err - bound).astype(F64))
        i = np.unravel_index(int(np.argmax(ex)), ex.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {int((~nan).sum())} outside the bound with measured "
                             f"atol_case {atol:.3g}; worst at {tuple(int(k) for k in i)}: |err| {float(err[i]):.3g} "
                             f"> {float(bound[i]):.3g} (oracle {float(want[i]):.6g})")


def check(out, case, dev, what, idx=None, resid=True):
    """Every output of every date of ``out`` against the oracle of ``case`` (``idx``: the case's
    date behind each date of the call)."""
    idx = np.arange(case.D) if idx is None else idx
    a = case.atol
    what = f"{what} [{dev.type}] atol_case f {a['f']:.2g} e {a['e']:.2g} r2 {a['r2']:.2g} stats {a['stats']:.2g}"
    f, r2, stats, n = case.f[idx], case.r2[idx], case.stats[idx], case.n[idx]
    assert out.f.dtype == torch.float64 and out.r2.dtype == torch.float64
    got_stats = _np(out.stats)
    assert np.array_equal(got_stats[:, -1], n.astype(F64)), f"{what}: n {got_stats[:, -1]} != {n}"
    st = _np(out.status).astype(np.int64)
    assert np.array_equal(st & BAD, case.bad[idx]), f"{what}: bad status bits {st & BAD} != {case.bad[idx]}"
    if dev.type != "cpu":
        dfc = case.deficient[idx]
        assert ((st[dfc] & X.XS_REFINED) != 0).all(), f"{what}: rank-deficient dates not refined: {st}"
        fine = ~dfc & (case.bad[idx] == 0)
        assert (st[fine] == 0).all(), f"{what}: well-conditioned dates flagged: {st}"
    fmax = np.abs(np.nan_to_num(f.astype(F64))).max(1)
    _cmp(_np(out.f), f, 4 * EPS * fmax[:, None] + a["f"], what + " f", a["f"])
    _cmp(got_stats[:, :-1], stats, 4 * EPS * np.abs(np.nan_to_num(stats.astype(F64))) + a["stats"],
         what + " mu|sigma", a["stats"])
    got_r2, df = _np(out.r2), case.r2_defined[idx]
    _cmp(got_r2[df], r2[df], 4 * EPS + a["r2"], what + " r2", a["r2"])
    if resid:
        e = case.e[idx]
        assert out.resid.dtype == (torch.float32 if case.fp32 else torch.float64)
        if case.fp32:
            bound = U32 * np.abs(np.nan_to_num(e.astype(F64))) + a["e"]
        else:
            bound = 4 * EPS * case.rmax[idx][:, None] + a["e"]
        _cmp(_np(out.resid), e, bound, what + " e", a["e"])
    else:
        assert out.resid is None


def _bits(t):
    return None if t is None else t.nan_to_num(7.0, 8.0, 9.0)


def assert_bitwise(a, b, what, sl=slice(None), resid=True):
    for k in ("f", "r2", "stats", "status") + (("resid",) if resid else ()):
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k)[sl])), f"{what}: {k} differs bitwise"


# ============================================================================== panels
def _panel(D, N, P, Q, dtype, seed, absent=0.02, offset=None):
    """A planted-factor panel in storage dtype ``dtype``: N(0, 1) styles with means up to +-0.4
    (``offset`` = (style, mean, sd) overrides one), lognormal caps, uniform industries, and
    ``absent`` of the stocks missing (odd stocks by a NaN return, even ones by ind = -1, or by a
    NaN cap when there are no industries)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((D, Q, N)) + rng.uniform(-0.4, 0.4, (D, Q, 1))
    if offset is not None:
        q, mean, sd = offset
        x[:, q] = mean + sd * rng.standard_normal((D, N))
    cap = np.exp(rng.standard_normal((D, N)) * 1.3 + 10)
    ind = rng.integers(0, max(P, 1), (D, N)).astype(np.int16)
    fc = rng.standard_normal((D, 1)) * 0.01
    fi = rng.standard_normal((D, max(P, 1))) * 0.02
    fs = rng.standard_normal((D, Q)) * 0.01
    ret = fc + (np.take_along_axis(fi, ind.astype(np.int64), 1) if P > 0 else 0.0) \
        + np.einsum("dq,dqn->dn", fs, x - x.mean(2, keepdims=True)) + rng.standard_normal((D, N)) * 0.02
    x, cap, ret = x.astype(dtype), cap.astype(dtype), ret.astype(dtype)
    gone = rng.random((D, N)) < absent
    odd = (np.arange(N) % 2 == 1)[None, :]
    ret[gone & odd] = NAN
    if P > 0:
        ind[gone & ~odd] = -1
    else:
        cap[gone & ~odd] = NAN
    return x, cap, ret, ind


# ------------------------------------------------------------------------------ 1. sizes
SIZES = [5, 8, 64, 72, 256, 264, 504, 512, 520]
SIZES64 = [760, 768, 769, 776, 1792, 1800]
SIZES32 = [1528, 1536, 1537, 1544, 4608, 4616]


@functools.lru_cache(maxsize=None)
def _size_case(dt, N):
    return Case(*_panel(5, N, 6, 4, DT[dt], 100 + N), 6)


# measured atol_case when written (f / e / r2 / stats), smallest and largest N of each dtype:
#   f32: N = 5: 5.6e-15 / 6.7e-16 / 0 / 1.7e-15      N = 4616: 2.0e-15 / 3.1e-15 / 8.2e-14 / 1.1e-13
#   f64: N = 5: 1.1e-14 / 4.2e-15 / 0 / 1.2e-15      N = 1800: 9.0e-16 / 3.6e-15 / 6.7e-15 / 1.8e-14
# in between f <= 1.9e-14 (N = 8, exact fits) and otherwise <= 2.5e-15, e <= 4.0e-15; r2 and the
# stats grow with N (sequential sums).  r2 = 0 at N = 5, 8: both give an exact fit's R^2 = 1.
@pytest.mark.parametrize("dt,N", [("f32", n) for n in SIZES + SIZES32] + [("f64", n) for n in SIZES + SIZES64])
def test_sizes(dev, dt, N):
    """(P, Q) = (6, 4), 5 dates, 2 % absent: N around the 64-stock tile, the 4-wave step of 256,
    the prefetched tail and the main residual block; N % 8 != 0 goes through the wrapper's padding.
    N = 5 and 8 have fewer stocks than factors (K = 11): minimum-norm dates."""
    case = _size_case(dt, N)
    if N <= 8:      # (an N = 8 date with 4 industries present has 8 columns: an exact, full-rank fit)
        assert case.deficient.sum() >= 3
    elif N >= 64:
        assert not case.deficient.any() and not case.bad.any()
    check(case.run(dev), case, dev, f"sizes {dt} N={N}")


@pytest.mark.parametrize("N", [8, 264, 520, 776, 1800])
def test_sizes_ring(dev, N):
    """fp64, 513 dates (the 5 distinct dates repeated cyclically): more than 512 dates put the
    production kernel on the LDS-DMA ring, which streams the tile validity words too.  All 513
    dates are compared with the oracle of their date.  On the GPU (deterministic kernel) every
    repetition equals its first occurrence bitwise, across 511 / 512 too, and the first 5 dates
    equal the 5-date (plain-load) call bitwise: a date-sharded regression is rank-invariant."""
    case = _size_case("f64", N)
    idx = np.arange(513) % 5
    out = case.run(dev, idx)
    check(out, case, dev, f"ring N={N}", idx)
    if dev.type != "cpu":
        for k in ("f", "r2", "stats", "status", "resid"):
            t = _bits(getattr(out, k))
            for d in range(5):
                assert torch.equal(t[d::5], t[d:d + 1].expand_as(t[d::5])), f"ring N={N}: {k} of date {d} varies"
        assert_bitwise(case.run(dev), out, f"ring N={N}: 5-date call vs dates 0..4 of 513", slice(0, 5))


# ------------------------------------------------------------------------------ 2. validity
EDGE = [0, 63, 64, 255, 256, -1]


def _knock(x, cap, ret, ind, d, stocks, ch, P):
    """Make ``stocks`` of date d absent through validity channel ``ch`` alone."""
    Q = x.shape[1]
    if ch == 0: ind[d, stocks] = -1
    elif ch == 1: ind[d, stocks] = P
    elif ch == 2: ind[d, stocks] = 32767
    elif ch == 3: cap[d, stocks] = NAN
    elif ch == 4: cap[d, stocks] = -cap[d, stocks]
    elif ch == 5: ret[d, stocks] = INF
    elif ch == 6: x[d, 0, stocks] = NAN
    elif ch == 7: x[d, Q - 1, stocks] = -INF


def _knock_all_but(x, cap, ret, ind, d, keep, P):
    """Only the stocks ``keep`` stay valid on date d; stock n leaves through channel n % 8."""
    n = np.arange(x.shape[2])
    for ch in range(8):
        _knock(x, cap, ret, ind, d, n[(n % 8 == ch) & ~keep], ch, P)


@functools.lru_cache(maxsize=None)
def _validity_case(dt):
    N, P, Q = 264, 6, 4
    x, cap, ret, ind = _panel(13, N, P, Q, DT[dt], 200, absent=0.0)
    n = np.arange(N)
    for ch in range(8):                                   # dates 0..7: one channel each
        _knock(x, cap, ret, ind, ch, EDGE, ch, P)
    cap[8, [1, 63, 64, 200]] = 0.0                        # date 8: zero caps on valid stocks
    cap[8, [2, 128, 263]] = -0.0
    _knock_all_but(x, cap, ret, ind, 9, (n < 128) | (n >= 192), P)     # a middle tile absent
    _knock_all_but(x, cap, ret, ind, 10, n < 64, P)                    # valid only in tile 0
    _knock_all_but(x, cap, ret, ind, 11, n >= 256, P)                  # only in the partial tile
    _knock_all_but(x, cap, ret, ind, 12, n < 0, P)                     # nobody
    return Case(x, cap, ret, ind, P)


# measured atol_case when written (f / e / r2 / stats):
#   f32: 4.0e-15 / 4.3e-15 / 7.3e-15 / 1.2e-14      f64: 4.0e-15 / 4.6e-15 / 4.9e-15 / 6.5e-15
# tail test below: f32 2.2e-15 / 2.8e-15 / 2.2e-14 / 5.8e-14, f64 2.4e-16 / 1.0e-15 / 1.1e-14 / 4.8e-15
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_validity_channels(dev, dt):
    """N = 264, (P, Q) = (6, 4), one pattern per date: dates 0-7 take stocks 0, 63, 64, 255, 256
    and N - 1 out through one channel each (ind = -1, ind = P, ind = 32767, NaN cap, cap < 0, +inf
    ret, NaN in style 0 only, -inf in style Q - 1 only); date 8 has +0.0 and -0.0 caps on valid
    stocks (weight 0, but counted in n, sigma and R^2); date 9 has a whole middle tile absent;
    dates 10 / 11 have valid stocks only in tile 0 / only in the last, partial tile (8 stocks:
    minimum norm); date 12 has none (XS_NO_ROWS: f, r2 and e NaN, n = 0)."""
    case = _validity_case(dt)
    assert (case.n == [258] * 8 + [264, 200, 64, 8, 0]).all(), case.n
    assert np.isnan(case.e[:8][:, EDGE]).all() and np.isfinite(case.e[8]).all()
    assert (case.bad[:12] == 0).all() and case.bad[12] & X.XS_NO_ROWS
    assert case.deficient[11] and not case.deficient[:11].any()
    assert np.isnan(case.f[12]).all() and np.isnan(case.e[12]).all() and np.isnan(case.r2[12])
    check(case.run(dev), case, dev, f"validity {dt}")


@functools.lru_cache(maxsize=None)
def _tail_case(dt):
    N = {"f32": 4616, "f64": 1800}[dt]
    x, cap, ret, ind = _panel(2, N, 6, 4, DT[dt], 250, absent=0.0)
    n = np.arange(N)
    _knock_all_but(x, cap, ret, ind, 0, n >= N - PRE[dt], 6)
    _knock_all_but(x, cap, ret, ind, 1, n < N - PRE[dt], 6)
    return Case(x, cap, ret, ind, 6)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_valid_only_inside_or_outside_prefetched_tail(dev, dt):
    """N = 1800 (fp64) / 4616 (fp32): date 0 has valid stocks only in the last 768 / 1536 stocks
    (the tail that waves 1-3 prefetch during the solve), date 1 only before them."""
    case = _tail_case(dt)
    assert (case.n == [PRE[dt], case.N - PRE[dt]]).all() and not case.bad.any() and not case.deficient.any()
    check(case.run(dev), case, dev, f"tail {dt}")


# ------------------------------------------------------------------------------ 3. rank, status
@functools.lru_cache(maxsize=None)
def _rank_case(dt, pivot_mode):
    N, P, Q = 264, 6, 4
    K = 1 + P + Q
    x, cap, ret, ind = _panel(8, N, P, Q, DT[dt], 300, absent=0.0)
    n = np.arange(N)
    if pivot_mode == 1:      # date 0 ordinary, date 1 with the last industry empty
        x, cap, ret, ind = x[:2].copy(), cap[:2].copy(), ret[:2].copy(), ind[:2].copy()
        ind[1][ind[1] == P - 1] = P - 2
        ind[:, [3, 64, 263]] = -1
        return Case(x, cap, ret, ind, P, pivot_mode=1)
    ind[2:, [3, 64, 200, 263]] = -1                       # a few absent stocks on dates 2..7
    _knock_all_but(x, cap, ret, ind, 0, np.isin(n, [7, 70, 260]), P)                  # n = 3
    nine = [0, 5, 63, 64, 100, 130, 255, 256, 263]        # n = K - 2 in all 6 industries: 10 columns
    ind[1, nine] = [0, 1, 2, 3, 4, 5, 0, 1, 2]
    _knock_all_but(x, cap, ret, ind, 1, np.isin(n, nine), P)
    x[2, 3] = x[2, 1]                                     # a duplicated style
    ind[3][ind[3] == 2] = 1                               # a singleton industry
    ind[3, 100] = 2
    cap[4][ind[4] == 1] = 0.0                             # an industry with zero caps only
    ind[5][ind[5] == P - 1] = P - 2                       # last industry empty (pivot moves)
    x[6] = 1.0                                            # pooled sigma exactly 0
    assert (K - 2 == 9) and ind[3, 100] == 2
    return Case(x, cap, ret, ind, P)


# measured atol_case when written (f / e / r2 / stats):
#   f32: 2.9e-14 / 6.9e-15 / 5.9e-15 / 1.1e-14      f64: 2.0e-14 / 5.6e-15 / 6.1e-15 / 1.1e-14
# reference-pivot test below: f32 2.6e-16 / 8.5e-16 / 4.8e-16 / 8.8e-15, f64 4.7e-16 / 9.0e-16 / 2.0e-15 / 2.2e-15
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_rank_and_status_edges(dev, dt):
    """N = 264, (P, Q) = (6, 4), K = 11.  Date 0: 3 valid stocks; 1: K - 2 = 9; 2: a duplicated
    style; 3: an industry with one stock; 4: an industry whose stocks all have cap 0 (f_j = 0,
    not singular); 5: the last industry empty, pivot_mode 0 (the pivot moves to industry P - 2);
    6: every style entry exactly 1.0 (sums of squares are exact: sigma = 0 in any arithmetic,
    XS_BAD_SIGMA); 7: an ordinary date."""
    case = _rank_case(dt, 0)
    assert (case.n[:2] == [3, 9]).all() and (case.deficient == [1, 1, 1, 0, 0, 0, 0, 0]).all()
    assert (case.bad == [0] * 6 + [X.XS_BAD_SIGMA, 0]).all(), case.bad
    # f_j = 0 for the weightless and the empty industry (lstsq leaves 1e-18 in a zero column)
    assert abs(case.f[4, 2]) < 1e-16 and abs(case.f[5, 6]) < 1e-16 and np.isfinite(case.f[:6]).all()
    assert case.stats[6, -1] == 0 and np.isnan(case.f[6]).all() and np.isnan(case.e[6]).all()
    check(case.run(dev), case, dev, f"rank {dt}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_last_industry_empty_reference_pivot(dev, dt):
    """pivot_mode 1 (the reference's choice: always the last industry): on date 1 it is empty --
    XS_PIVOT_EMPTY, f NaN and e NaN on the valid rows too; date 0 is an ordinary date."""
    case = _rank_case(dt, 1)
    assert (case.bad == [0, X.XS_PIVOT_EMPTY]).all() and case.n[1] > 250
    assert np.isnan(case.f[1]).all() and np.isnan(case.e[1]).all() and np.isfinite(case.f[0]).all()
    check(case.run(dev), case, dev, f"reference pivot {dt}")


# ------------------------------------------------------------------------------ 4. shapes
SHAPES = [(0, 1), (1, 3), (2, 1), (31, 10), (57, 10), (58, 10), (31, 11), (40, 16), (128, 16), (129, 4),
          (256, 16)]


@functools.lru_cache(maxsize=None)
def _shape_case(dt, P, Q):
    return Case(*_panel(3, 520, P, Q, DT[dt], 400 + 20 * P + Q), P)


# measured atol_case when written (f / e / r2 / stats; the larger of f32 and f64):
#   (0, 1)    2.9e-16 / 5.0e-16 / 1.6e-14 / 4.3e-15      (1, 3)    3.3e-16 / 1.3e-15 / 6.3e-14 / 4.6e-15
#   (2, 1)    1.6e-16 / 4.4e-16 / 2.6e-14 / 6.5e-15      (31, 10)  4.9e-15 / 8.4e-15 / 4.5e-15 / 4.2e-14
#   (57, 10)  7.9e-15 / 8.0e-15 / 6.0e-15 / 3.9e-14      (58, 10)  2.1e-14 / 2.6e-14 / 2.8e-15 / 3.8e-14
#   (31, 11)  3.2e-15 / 4.1e-15 / 3.6e-15 / 4.1e-14      (40, 16)  5.5e-15 / 6.6e-15 / 4.6e-15 / 5.3e-14
#   (128, 16) 3.3e-11 / 3.3e-11 / 2.8e-13 / 6.2e-14      (129, 4)  1.2e-12 / 1.2e-12 / 1.8e-13 / 1.5e-14
#   (256, 16) 2.1e-12 / 2.2e-12 / 7.5e-14 / 7.4e-14
# From 128 industries on, 520 stocks leave 2 to 4 per industry and the design is nearly saturated
# (K = 145 .. 273 columns): the float64 normal equations lose that much.
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("P,Q", SHAPES)
def test_table_and_solve_shapes(dev, dt, P, Q):
    """N = 520, 3 dates: no industries, P = 1, the deterministic 8-replica table up to its limit
    (57 industries at Q = 10) and the single-replica table beyond, the Q > 10 register budget,
    the fused maximum of 128 industries and the split kernels above it (129, 256)."""
    case = _shape_case(dt, P, Q)
    assert not case.bad.any()
    check(case.run(dev), case, dev, f"shape {dt} P={P} Q={Q}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_shared_replica_table(dev, dt):
    """(31, 10) with ``deterministic=False``: the replicas shared across waves."""
    case = _shape_case(dt, 31, 10)
    check(case.run(dev, deterministic=False), case, dev, f"shape {dt} P=31 Q=10 deterministic=False")


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("P,Q", [(6, 4), (129, 4)])
def test_stock_sharded_direct(dev, dt, P, Q):
    """``xs_wls_stock_sharded`` called directly (world size 1): moments, solve, device pinv and
    residual kernels, below and above the fused kernel's industry limit."""
    case = _shape_case(dt, P, Q)
    out = case.run(dev, fn=lambda x, c, r, i, P_, **kw: S.xs_wls_stock_sharded(x, c, r, i, P_, None, **kw))
    check(out, case, dev, f"stock-sharded {dt} P={P} Q={Q}")


# ------------------------------------------------------------------------------ 5. cancellation
@functools.lru_cache(maxsize=None)
def _offset_case(dt):
    return Case(*_panel(2, 784, 12, 10, DT[dt], 500, offset=(0, 20.0, 1.5)), 12)


# measured atol_case when written (f / e / r2 / stats):
#   f32: 2.4e-13 / 2.0e-13 / 3.0e-15 / 3.6e-13      f64: 2.4e-13 / 1.7e-13 / 6.1e-15 / 6.4e-14
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_raw_size_style_cancellation(dev, dt):
    """(P, Q) = (12, 10), N = 784: style 0 is a raw SIZE column (mean 20, sd 1.5), so the
    algebraic centring of the raw moments (``acc - mu_q mu_s Sw`` in ``solve_body``) cancels
    three digits.  The bound is the rule's: what a float64 raw-moment solve is entitled to."""
    case = _offset_case(dt)
    assert (np.abs(case.stats[:, 0] - 20) < 0.5).all() and not case.bad.any() and not case.deficient.any()
    check(case.run(dev), case, dev, f"offset-20 {dt}")


# ------------------------------------------------------------------------------ 6. buffers
@functools.lru_cache(maxsize=None)
def _buffer_cases(dt, N):
    a = Case(*_panel(5, N, 6, 4, DT[dt], 600 + N), 6)
    x, cap, ret, ind = _panel(5, N, 6, 4, DT[dt], 700 + N, absent=0.1)
    n = np.arange(N)
    _knock_all_but(x, cap, ret, ind, 1, (n < 64) | (n >= 128), 6)     # tile 1 absent
    _knock_all_but(x, cap, ret, ind, 2, n < 0, 6)                     # an empty date
    _knock_all_but(x, cap, ret, ind, 3, n >= 256, 6)                  # only the last tile
    return a, Case(x, cap, ret, ind, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N", [264, 261])
def test_buffer_reuse(cuda, dt, N):
    """One ``workspace`` and one ``out`` reused for panel A, panel B (other absence patterns: a
    tile, a date, all but the last tile absent) and A again give the bits of fresh calls -- no
    stale validity words or moments -- also with N % 8 != 0, where ``out.resid`` is filled from
    the padded buffer; ``want_resid=False`` gives the same f, r2, stats and status."""
    a, b = _buffer_cases(dt, N)
    fresh = {id(c): c.run(cuda) for c in (a, b)}
    check(fresh[id(a)], a, cuda, f"buffers {dt} N={N} A")
    check(fresh[id(b)], b, cuda, f"buffers {dt} N={N} B")
    D, K, Q = 5, 11, 4
    tdt = torch.float32 if dt == "f32" else torch.float64
    out = X.XsResult(f=torch.full((D, K), 3.0, dtype=torch.float64, device=cuda),
                     resid=torch.full((D, N), 3.0, dtype=tdt, device=cuda),
                     r2=torch.full((D,), 3.0, dtype=torch.float64, device=cuda),
                     stats=torch.full((D, Q + 2), 3.0, dtype=torch.float64, device=cuda),
                     status=torch.full((D,), 3, dtype=torch.int32, device=cuda))
    ws = X.xs_wls_workspace(D, 6, Q, cuda, N)
    ws.fill_(0xFF)
    for k, c in enumerate((a, b, a)):
        got = c.run(cuda, out=out, workspace=ws)
        assert got is out
        assert_bitwise(fresh[id(c)], out, f"buffers {dt} N={N}: reuse {k}")
    for c in (a, b):
        nr = c.run(cuda, want_resid=False)
        check(nr, c, cuda, f"buffers {dt} N={N} want_resid=False", resid=False)
        assert_bitwise(fresh[id(c)], nr, f"buffers {dt} N={N}: want_resid=False", resid=False)
