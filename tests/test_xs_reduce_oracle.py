"""Cross-sectional reduction kernels (``csrc/xs_reduce.hip``) against plain high-precision numpy
oracles, at the edges of every kernel: sizes around the wave / block / tile boundaries, empty and
single-row dates, NaN / inf masks, rank-deficient regressions, the LDS limits of the shrink.

The oracles below are written from the semantics of the reference (pandas ``clip`` / ``mean`` /
``std``, ``sm.OLS`` residuals, ``np.std``, ``pd.qcut`` codes), not from the package's own CPU
path: float32 inputs as given, ``np.longdouble`` arithmetic, two-pass moments, ``lstsq`` for the
regression (refined once in longdouble), ``np.quantile(..., method="linear")`` for the edges.
Every case runs against the oracle twice: through the CPU path (unmarked) and through the HIP
kernels (``gpu``).

Tolerance rule.  Every output is a float64 result rounded once to float32, so

    |got - oracle| <= 2**-23 * |oracle| + atol_case

``atol_case`` is 0 for winsorize and composite (selection, or one fma chain of at most 8 terms).
For ``ols_resid``, ``style_norm`` and ``bayes_shrink`` it is measured here, on the CPU, from the
inputs alone: the same operation computed a second, independent way in plain float64 numpy
(normal equations; one-pass moments; naive float64 sums), 8 x its largest deviation from the
longdouble oracle on that case (the 8 covers a block tree's summation order against numpy's).
It is the accuracy a float64 implementation is entitled to and is never derived from the output
under test.  The values measured when the cases were written stand beside each case; the
assertion message prints the one in force.  NaN (and inf) positions must match exactly.
"""
import numpy as np
import pytest
import torch

from llm_driven_multi_factor_model_amd.ops import xs_reduce as R

LD = np.longdouble
U32 = 2.0 ** -23
EPS = np.finfo(np.float64).eps
NAN = np.float32("nan")


@pytest.fixture(params=[pytest.param("cpu"), pytest.param("hip", marks=pytest.mark.gpu)])
def dev(request):
    if request.param == "cpu":
        return torch.device("cpu")
    return request.getfixturevalue("cuda")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _close(got, want, atol, what, rtol=U32):
    """``got`` (array) against the oracle ``want`` (float64 / longdouble) under the module's rule."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), \
        f"{what}: NaN positions differ at {np.argwhere(np.isnan(got) != np.isnan(want))[:5].tolist()}"
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), f"{what}: inf positions"
    f = np.isfinite(want)
    err = np.abs(got[f] - want[f])
    bound = rtol * np.abs(want[f]) + atol
    bad = err > bound
    if bad.any():
        i = int(np.argmax(err - bound))
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(f.sum())} outside rtol {rtol:.3g} + measured "
                             f"atol_case {atol:.3g}; worst |err| {err[i]:.3g} at oracle {want[f][i]:.6g} "
                             f"(bound {bound[i]:.3g}), max |err| {err.max():.3g}")


def _dev(a, b):
    """Largest deviation of the float64 second opinion ``a`` from the oracle ``b`` (finite entries)."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    f = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a[f] - b[f]))) if f.any() else 0.0


# ============================================================================== winsorize
def oracle_winsorize(x, n_std):
    """pandas ``x.clip(mean - n std, mean + n std)`` per row: NaN skipped, ddof 1; NaN bounds
    (fewer than 2 values, or an infinite value in the row) clip nothing."""
    out = x.astype(LD)
    for r in range(x.shape[0]):
        lo, hi = _winsor_bounds(x[r], n_std)
        v = out[r]
        with np.errstate(invalid="ignore"):
            out[r] = np.where(v < lo, lo, np.where(v > hi, hi, v))
    return out


def _winsor_bounds(row, n_std):
    v = row[~np.isnan(row)].astype(LD)
    if v.size < 2:
        return LD("nan"), LD("nan")
    with np.errstate(invalid="ignore", over="ignore"):
        mean = v.sum(dtype=LD) / LD(v.size)
        dv = v - mean
        sd = np.sqrt((dv * dv).sum(dtype=LD) / LD(v.size - 1))
        return mean - LD(n_std) * sd, mean + LD(n_std) * sd


def _f32_above(b):
    f = np.float32(b)
    return f if LD(f) > b else np.nextafter(f, np.float32(np.inf))


def _f32_below(b):
    f = np.float32(b)
    return f if LD(f) < b else np.nextafter(f, np.float32(-np.inf))


def _winsor_edge_row(N, rng, n_std):
    """A row whose entries 0..3 are the float32 neighbours of the clip bounds (the smallest above
    and the largest below each), as a fixed point of the bounds they themselves move."""
    x = (rng.standard_normal(N) * 2 + 1).astype(np.float32)
    for _ in range(100):
        lo, hi = _winsor_bounds(x, n_std)
        new = np.array([_f32_above(hi), _f32_below(hi), _f32_above(lo), _f32_below(lo)], dtype=np.float32)
        if np.array_equal(new, x[:4]):
            break
        x[:4] = new
    else:
        raise AssertionError("edge row did not settle")
    lo, hi = _winsor_bounds(x, n_std)
    ulp_hi, ulp_lo = np.spacing(np.float32(abs(hi))), np.spacing(np.float32(abs(lo)))
    assert LD(x[1]) < hi < LD(x[0]) and float(x[0]) - float(x[1]) <= 2 * ulp_hi
    assert LD(x[3]) < lo < LD(x[2]) and float(x[2]) - float(x[3]) <= 2 * ulp_lo
    return x


def _winsor_panel(N, n_std=2.5):
    rng = np.random.default_rng(1000 + N)
    rows = []
    rows.append(np.full(N, NAN))                                   # all NaN
    r = np.full(N, NAN); r[N // 2] = 3.25; rows.append(r)          # exactly one value
    if N >= 2:
        r = np.full(N, NAN); r[0] = -1.5; r[N - 1] = 7.0; rows.append(r)   # exactly two values
    rows.append(np.full(N, np.float32(0.3)))                       # constant row: sd = 0
    r = (rng.standard_normal(N) * 2 + 1).astype(np.float32)        # +inf: bounds NaN, unchanged
    r[N // 3] = np.inf
    rows.append(r)
    r = (1e4 + rng.uniform(-1, 1, N)).astype(np.float32)           # mean >> sd
    if N >= 63:
        r[5] = 1e4 + 40
        r[7] = 1e4 - 35
    rows.append(r)
    r = (rng.standard_normal(N) * 2 + 1).astype(np.float32)        # NaNs and far outliers
    r[rng.random(N) < 0.1] = NAN
    if N >= 63:
        r[:3] = [50.0, -40.0, 30.0]
    rows.append(r)
    if N >= 63:
        rows.append(_winsor_edge_row(N, rng, n_std))
    return np.stack(rows).astype(np.float32)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_winsorize_oracle(dev, N):
    x = _winsor_panel(N)
    want = oracle_winsorize(x, 2.5)
    if N >= 63:  # the cases do clip: both outliers and the neighbours beyond the bounds move
        assert (want[-1, [0, 3]] != x[-1, [0, 3]].astype(LD)).all() and (want[-1, [1, 2]] == x[-1, [1, 2]]).all()
        assert (want[-2, :3] != x[-2, :3].astype(LD)).all()
    xt = _t(x, dev)
    got = R.winsorize(xt, 2.5)
    assert got.dtype == torch.float32 and got.data_ptr() != xt.data_ptr()
    assert np.array_equal(_np(xt), x, equal_nan=True), "winsorize changed its input"
    _close(_np(got), want, 0.0, f"winsorize N={N}")   # atol_case 0: selection
    ret = R.winsorize_(xt, 2.5)
    assert ret.data_ptr() == xt.data_ptr()
    _close(_np(xt), want, 0.0, f"winsorize_ N={N}")
    assert torch.equal(xt.nan_to_num(7.0), got.nan_to_num(7.0)), "winsorize_ and winsorize differ"


# ============================================================================== composite
def oracle_composite(xs, ws):
    num = np.zeros(xs[0].shape, dtype=LD)
    den = np.zeros(xs[0].shape, dtype=LD)
    for x, w in zip(xs, ws):
        ok = ~np.isnan(x)
        num += np.where(ok, x.astype(LD), LD(0)) * LD(w)
        den += ok * LD(w)
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / den


def _composite_inputs(C, n, seed):
    rng = np.random.default_rng(seed)
    xs = []
    for _ in range(C):
        x = (rng.standard_normal(n) * 2 + 1).astype(np.float32)
        x[rng.random(n) < 0.2] = NAN
        xs.append(x)
    for x in xs:
        x[n // 2] = NAN           # one element with every component missing
    ws = [0.7] if C == 1 else list(rng.uniform(0.05, 1.0, C))
    return xs, ws


@pytest.mark.parametrize("C, shape", [(1, (3, 257)), (8, (3, 257)), (2, (4096 * 256 + 257,))])
def test_composite_oracle(dev, C, shape):
    """C = 1 and C = 8 on a small panel; C = 2 on 4096 * 256 + 257 elements, one more than one
    trip of the kernel's grid-stride loop (grid 4096 x 256 threads) covers."""
    n = int(np.prod(shape))
    xs, ws = _composite_inputs(C, n, 2000 + C)
    want = oracle_composite(xs, ws).reshape(shape)
    assert np.isnan(want.reshape(-1)[n // 2])
    got = R.composite([_t(x.reshape(shape), dev) for x in xs], ws)
    assert got.dtype == torch.float32
    _close(_np(got), want, 0.0, f"composite C={C} n={n}")   # atol_case 0: one fma chain


# ============================================================================== ols_resid
def _ols_design(y, xs, d, log_x0, ypow):
    with np.errstate(invalid="ignore", divide="ignore"):
        cols = [x[d].astype(LD) for x in xs]
        if log_x0:
            cols[0] = np.log(cols[0])
        yv = cols[0] ** ypow if ypow > 0 else y[d].astype(LD)
    N = yv.shape[0]
    Z = np.stack([np.ones(N, dtype=LD)] + cols, 1)
    ok = np.isfinite(yv) & np.isfinite(Z).all(1)
    return Z, yv, ok


def oracle_ols(y, xs, min_rows, sign, log_x0=False, ypow=0):
    """``sign * (y - Z lstsq(Z, y))`` on the rows where y and every regressor are finite (numpy's
    default ``rcond`` decides the rank, as for ``sm.OLS``' pinv), one refinement step in
    longdouble; dates with fewer than ``min_rows`` such rows, and the other rows, are NaN."""
    D, N = (xs[0] if xs else y).shape
    out = np.full((D, N), np.nan, dtype=LD)
    for d in range(D):
        Z, yv, ok = _ols_design(y, xs, d, log_x0, ypow)
        if ok.sum() < min_rows:
            continue
        Zv, yo = Z[ok], yv[ok]
        Z64 = Zv.astype(np.float64)
        b = np.linalg.lstsq(Z64, yo.astype(np.float64), rcond=None)[0].astype(LD)
        e = yo - Zv @ b
        b = b + np.linalg.lstsq(Z64, e.astype(np.float64), rcond=None)[0].astype(LD)
        out[d, ok] = LD(sign) * (yo - Zv @ b)
    return out


def second_ols(y, xs, min_rows, sign, log_x0=False, ypow=0):
    """The second opinion: float64 normal equations.  Their entries carry up to n eps of summation
    error, so n eps is the rank tolerance such a solve can use."""
    D, N = (xs[0] if xs else y).shape
    out = np.full((D, N), np.nan)
    for d in range(D):
        Z, yv, ok = _ols_design(y, xs, d, log_x0, ypow)
        if ok.sum() < min_rows:
            continue
        Z64, y64 = Z[ok].astype(np.float64), yv[ok].astype(np.float64)
        b = np.linalg.lstsq(Z64.T @ Z64, Z64.T @ y64, rcond=int(ok.sum()) * EPS)[0]
        out[d, ok] = sign * (y64 - Z64 @ b)
    return out


def _run_ols(dev, y, xs, what, **kw):
    want = oracle_ols(y, xs, **kw)
    atol = 8 * _dev(second_ols(y, xs, **kw), want)
    got = R.ols_resid(None if y is None else _t(y, dev), [_t(x, dev) for x in xs], **kw)
    assert got.dtype == torch.float32
    _close(_np(got), want, atol, what)
    return atol, want


def _ols_panel(p, N, seed):
    """Dates: 0 all rows valid; 1 exactly p + 2 valid rows; 2 exactly p + 1; 3 NaN in y only;
    4 NaN in one regressor only; 5 +-inf in a regressor (dates 1, 2 mask y; with N = p + 1 no
    date reaches min_rows = p + 2)."""
    rng = np.random.default_rng(seed)
    D = 6
    xs = [(rng.standard_normal((D, N)) * 2 + 1).astype(np.float32) for _ in range(p)]
    y = (rng.standard_normal((D, N)) + sum(0.5 * (k + 1) * x for k, x in enumerate(xs)) + 0.25).astype(np.float32)
    for d, keep in ((1, p + 2), (2, p + 1)):
        drop = rng.permutation(N)[min(keep, N):]
        y[d, drop] = NAN
    y[3, rng.random(N) < 0.1] = NAN
    if N > 3:
        y[3, 0] = NAN
    if p:
        xs[p - 1][4, rng.random(N) < 0.1] = NAN
        xs[p - 1][4, N - 1] = NAN
        xs[0][5, 0] = np.inf
        xs[p - 1][5, N // 2] = -np.inf
    return y, xs


# measured atol_case (8 x |normal equations - oracle|) when written, N = p + 2 / 64 / 257 / 1000
# (N = p + 1 has no valid date: 0):
#   p = 0: 2.0e-15 / 2.0e-15 / 1.2e-15 / 1.0e-15      p = 1: 1.5e-14 / 1.2e-14 / 3.9e-14 / 4.2e-14
#   p = 2: 4.9e-13 / 4.1e-13 / 4.9e-13 / 3.1e-13      p = 3: 5.0e-14 / 1.1e-13 / 1.6e-13 / 1.3e-13
#   p = 4: 1.7e-13 / 1.7e-13 / 4.1e-13 / 4.6e-13
@pytest.mark.parametrize("p", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("Nk", ["p+1", "p+2", 64, 257, 1000])
def test_ols_resid_oracle(dev, p, Nk):
    N = {"p+1": p + 1, "p+2": p + 2}.get(Nk, Nk)
    y, xs = _ols_panel(p, N, 3000 + 10 * p + N)
    for sign in (1.0, -1.0):
        _, want = _run_ols(dev, y, xs, f"ols_resid p={p} N={N} sign={sign}", min_rows=p + 2, sign=sign)
    fin = np.isfinite(want)
    assert not fin[2].any(), "min_rows - 1 valid rows: a NaN date"
    if N >= p + 2:
        assert fin[0].all() and fin[1].sum() == p + 2
    else:
        assert not fin.any()
    if p and N > 3:
        assert not fin[5, 0] and not fin[5, N // 2] and not fin[4, N - 1] and not fin[3, 0]


def test_ols_resid_default_min_rows(dev):
    """``min_rows`` defaults to p + 2."""
    y, xs = _ols_panel(2, 64, 7)
    got = R.ols_resid(_t(y, dev), [_t(x, dev) for x in xs])
    want = oracle_ols(y, xs, 4, 1.0)
    _close(_np(got), want, 8 * _dev(second_ols(y, xs, 4, 1.0), want), "ols_resid default min_rows")


# measured atol_case when written: N = 2: 3.2e-08, 257: 2.4e-08, 1000: 5.4e-08 (residuals up to 1500:
# the normal equations of [1, ln cap] with ln cap = 23 +- 1.2 and y around 12000 are not centred)
@pytest.mark.parametrize("N", [2, 257, 1000])
def test_ols_resid_nlsize_oracle(dev, N):
    """NLSIZE: -(residual of ln(cap)^3 on [1, ln(cap)]), logs and cubes formed in float64 from the
    float32 caps.  Date 0: lognormal caps around e^23 with a zero, a negative and a NaN cap
    (excluded rows); date 1: exactly two valid rows (an exact fit: residual 0 up to the measured
    term); date 2: one valid row (NaN date)."""
    rng = np.random.default_rng(3500 + N)
    cap = np.exp(23 + 1.2 * rng.standard_normal((3, N))).astype(np.float32)
    if N > 2:
        cap[0, 1], cap[0, 2], cap[0, 3] = 0.0, -cap[0, 2], NAN
    cap[1, :] = NAN
    cap[1, 0], cap[1, N - 1] = np.float32(np.exp(21.0)), np.float32(np.exp(25.0))
    cap[2, 1:] = NAN
    atol, want = _run_ols(dev, None, [cap], f"NLSIZE N={N}", min_rows=2, sign=-1.0, log_x0=True, ypow=3)
    fin = np.isfinite(want)
    assert fin[1].sum() == 2 and not fin[2].any()
    if N > 2:
        assert not fin[0, 1:4].any() and fin[0].sum() == N - 3
    assert np.abs(want[1][fin[1]]).max() <= 1e-12    # two rows, two coefficients


def _rank_deficient(kind, N, seed):
    """Six dates each, with their own missing rows (date 0: one) and, for ``constant``, their own
    value: where the roundoff of the Gram sums falls differs from date to date."""
    rng = np.random.default_rng(seed)
    D = 6
    x1 = (rng.standard_normal((D, N)) * 2 + 1).astype(np.float32)
    y = (rng.standard_normal((D, N)) + 0.5 * x1 + 0.25).astype(np.float32)
    y[1:][rng.random((D - 1, N)) < 0.1] = NAN
    y[:, 3] = NAN
    if kind == "constant":
        c = np.array([0.3, 0.3, 1.7, -2.9, 1e-3, 123.456], dtype=np.float32)
        return y, [np.repeat(c[:, None], N, 1)]
    if kind == "duplicate":
        return y, [x1, x1.copy()]
    if kind == "scaled":
        return y, [x1, (np.float32(2.5) * x1).astype(np.float32)]
    assert kind == "zero"
    return y, [x1, np.zeros((D, N), dtype=np.float32)]


# measured atol_case when written (N = 120 / 1000 / 5000):
#   constant   1.5e-14 / 2.9e-14 / 5.5e-14      duplicate  3.5e-14 / 7.1e-14 / 1.1e-13
#   zero       3.7e-14 / 8.8e-14 / 1.0e-13      scaled     3.9 / 1.4 / 1.9 (see the test's docstring)
@pytest.mark.parametrize("N", [120, 1000, 5000])
@pytest.mark.parametrize("kind", ["constant", "duplicate", "scaled", "zero"])
def test_ols_resid_rank_deficient_oracle(dev, kind, N):
    """Rank-deficient dates: a regressor constant at 0.3 (collinear with the intercept), an exactly
    duplicated regressor, x2 = fl32(2.5 x1) and an all-zero regressor; the oracle is the lstsq
    residual, i.e. the projection residual.  Whether roundoff leaves a pivot of the normal
    equations at 1e-17 of its scale or at exactly 0 depends on N, hence three sizes.

    ``scaled``: fl32(2.5 x1) differs from 2.5 x1 by float32 rounding, so Z has a smallest
    singular value around 1e-8 of the largest: lstsq keeps it (coefficients of +-1e6 fitted to the
    rounding noise) while no float64 normal-equation solve can resolve it (its Gram eigenvalue is
    1e-16 of the largest).  The measured atol_case says so: 3.9 / 1.4 / 1.9 when written,
    against 1e-13 for the other three kinds, so for this kind the test checks little more than
    the NaN mask and that the residual stays of the order of y."""
    y, xs = _rank_deficient(kind, N, 4000 + N)
    atol, want = _run_ols(dev, y, xs, f"ols_resid {kind} N={N}", min_rows=len(xs) + 2, sign=1.0)
    assert np.isfinite(want[0]).sum() == N - 1 and np.isfinite(want).sum() > 5 * N
    if kind != "scaled":
        assert atol < 1e-11, atol     # the second opinion does reach the projection residual


@pytest.mark.reference
def test_orthogonalize_rank_deficient_matches_reference(ref, capsys):
    """``orthogonalize_factors`` of the reference (recorded) on a panel with a full-rank date, a
    date whose second regressor is constant and a date whose regressors are duplicates."""
    import pandas as pd
    rng = np.random.default_rng(4500)
    D, N = 3, 120
    b = (rng.standard_normal((D, N)) * 2 + 1).astype(np.float32)
    s = (rng.standard_normal((D, N)) * 2 + 1).astype(np.float32)
    y = (rng.standard_normal((D, N)) + 0.5 * b - 0.3 * s).astype(np.float32)
    y[rng.random((D, N)) < 0.1] = NAN
    s[1] = np.float32(0.3)
    s[2] = b[2]
    df = pd.DataFrame({"trade_date": np.repeat(np.arange(D), N), "ts_code": np.tile(np.arange(N), D),
                       "y": y.astype(np.float64).reshape(-1), "b": b.astype(np.float64).reshape(-1),
                       "s": s.astype(np.float64).reshape(-1)})
    exp = ref.post_processing.orthogonalize_factors(df, {"y": ["b", "s"]})["y"].values.reshape(D, N)
    want = oracle_ols(y, [b, s], 4, 1.0)
    atol = 8 * _dev(second_ols(y, [b, s], 4, 1.0), want)
    _close(exp, want, atol, "reference vs oracle", rtol=2.0 ** -40)
    devs = [torch.device("cpu")] + ([torch.device("cuda:0")] if torch.cuda.is_available() else [])
    for dv in devs:
        got = R.ols_resid(_t(y, dv), [_t(b, dv), _t(s, dv)])
        _close(_np(got), exp, atol, f"orthogonalize vs reference on {dv}")


# ============================================================================== style_norm
def oracle_style_norm(X, cap):
    """``(x - cap-weighted mean_q) / np.std(all valid x)`` per date; a row enters the moments when
    its cap and all its styles are finite; every entry is transformed (NaN stays NaN)."""
    D, Q, N = X.shape
    Z = np.full((D, Q, N), np.nan, dtype=LD)
    mu = np.full((D, Q), np.nan, dtype=LD)
    sig = np.full(D, np.nan, dtype=LD)
    for d in range(D):
        ok = np.isfinite(cap[d]) & np.isfinite(X[d]).all(0)
        if ok.any():
            w = cap[d][ok].astype(LD)
            xv = X[d][:, ok].astype(LD)
            mu[d] = (xv * w).sum(1, dtype=LD) / w.sum(dtype=LD)
            m = xv.sum(dtype=LD) / LD(xv.size)
            dv = xv - m
            sig[d] = np.sqrt((dv * dv).sum(dtype=LD) / LD(xv.size))
        with np.errstate(invalid="ignore", divide="ignore"):
            Z[d] = (X[d].astype(LD) - mu[d][:, None]) / sig[d]
    return Z, mu, sig


def second_style_norm(X, cap):
    """One-pass float64 moments (E x^2 - (E x)^2), naive sums."""
    D, Q, N = X.shape
    Z = np.full((D, Q, N), np.nan)
    mu = np.full((D, Q), np.nan)
    sig = np.full(D, np.nan)
    for d in range(D):
        ok = np.isfinite(cap[d]) & np.isfinite(X[d]).all(0)
        if ok.any():
            w = cap[d][ok].astype(np.float64)
            xv = X[d][:, ok].astype(np.float64)
            mu[d] = (xv * w).sum(1) / w.sum()
            m = xv.sum() / xv.size
            sig[d] = np.sqrt(max((xv * xv).sum() / xv.size - m * m, 0.0))
        with np.errstate(invalid="ignore", divide="ignore"):
            Z[d] = (X[d].astype(np.float64) - mu[d][:, None]) / sig[d]
    return Z, mu, sig


def _style_panel(Q, N, seed):
    """Dates: 0 clean; 1 NaN in cap only; 2 NaN in a single style only; 3 no valid row;
    4 pooled sd 0 (every valid style value 0.5: all sums exact, Z = 0 / 0); 5 mean 100, sd 0.1."""
    rng = np.random.default_rng(seed)
    D = 6
    X = rng.standard_normal((D, Q, N)).astype(np.float32)
    cap = np.exp(rng.standard_normal((D, N)) * 1.3 + 10).astype(np.float32)
    cap[1, rng.random(N) < 0.1] = NAN
    cap[1, N - 1] = NAN
    X[2, Q // 2, rng.random(N) < 0.1] = NAN
    X[2, Q // 2, 0] = NAN
    cap[3, :] = NAN
    X[4] = 0.5
    if N > 1:
        cap[4, 0] = NAN
    X[5] = (100 + 0.1 * rng.standard_normal((Q, N))).astype(np.float32)
    return X, cap


# measured atol_case when written, (Z, mu, sig), largest over Q at each N -- dominated by date 5
# (mean 100, sd 0.1: the one-pass variance loses 6 digits):
#   N = 1: (0, 0, 3.8e-11)   63: (4.2e-09, 4.6e-13, 1.7e-10)
#   257: (2.7e-09, 9.3e-13, 1.1e-10)   1000: (4.7e-09, 1.8e-12, 1.1e-10)
# Smallest: Q = 64, N = 63: sig 4.1e-12 and Q = 64, N = 1000: sig 1.5e-11 -- a kernel that takes
# the variance as E x^2 - m^2 with block-tree sums misses these (2.3e-11 and 1.2e-10 measured on
# an MI355X), which is why it takes squared deviations from the mean.
@pytest.mark.parametrize("Q", [1, 10, 64])
@pytest.mark.parametrize("N", [1, 63, 257, 1000])
def test_style_norm_oracle(dev, Q, N):
    X, cap = _style_panel(Q, N, 5000 + 100 * Q + N)
    Zo, muo, so = oracle_style_norm(X, cap)
    Z2, mu2, s2 = second_style_norm(X, cap)
    aZ, amu, asig = 8 * _dev(Z2, Zo), 8 * _dev(mu2, muo), 8 * _dev(s2, so)
    Xt = _t(X, dev)
    Z, mu, sig = R.style_norm(Xt, _t(cap, dev))
    assert Z.dtype == torch.float32 and mu.dtype == torch.float64 and sig.dtype == torch.float64
    assert np.array_equal(_np(Xt), X, equal_nan=True), "style_norm changed its input"
    what = f"style_norm Q={Q} N={N}"
    _close(_np(mu), muo, amu, what + " mu", rtol=2.0 ** -40)
    _close(_np(sig), so, asig, what + " sig", rtol=2.0 ** -40)
    _close(_np(Z), Zo, aZ, what + " Z")
    # the edges are what they are meant to be
    assert np.isnan(so[3]) and np.isnan(muo[3]).all() and np.isnan(Zo[3]).all()
    assert so[4] == 0 and (muo[4] == 0.5).all() and np.isnan(Zo[4]).all()
    if N > 1:   # excluded rows with finite styles are still transformed; NaN entries stay NaN
        assert np.isfinite(Zo[1, :, N - 1]).all()
        assert np.isnan(Zo[2, Q // 2, 0]) and (Q == 1 or np.isfinite(Zo[2, 0, 0]))


@pytest.mark.gpu
def test_style_norm_q65_raises(cuda):
    X = torch.zeros(1, 65, 8, device=cuda)
    with pytest.raises(ValueError):
        R.style_norm(X, torch.ones(1, 8, device=cuda))
    torch.cuda.synchronize()


# ============================================================================== bayes_shrink
def _bayes_groups(cd, ok, G):
    cs = cd[ok].astype(np.float64)
    edges = np.quantile(cs, np.linspace(0, 1, G + 1), method="linear")
    g = np.zeros(cs.size, dtype=np.int64)
    for k in range(1, G):          # right-closed bins, the first includes the minimum
        g[cs > edges[k]] = k
    return g


def _bayes(v, c, G, q, T):
    """``T`` = longdouble: the oracle; float64: the second opinion (naive float64 sums)."""
    D, N = v.shape
    out = np.full((D, N), np.nan, dtype=T)
    grp = np.full((D, N), -1, dtype=np.int32)
    for d in range(D):
        ok = np.isfinite(v[d]) & np.isfinite(c[d])
        if not ok.any():
            continue
        g = _bayes_groups(c[d], ok, G)
        vv, cc = v[d][ok].astype(T), c[d][ok].astype(T)
        res = np.empty(vv.size, dtype=T)
        for k in np.unique(g):
            s = g == k
            m = (vv[s] * cc[s]).sum(dtype=T) / cc[s].sum(dtype=T)
            sd = np.sqrt(((vv[s] - m) ** 2).sum(dtype=T) / T(s.sum()))
            a = T(q) * np.abs(vv[s] - m)
            with np.errstate(invalid="ignore"):
                w = a / (a + sd)       # a one-member group: 0 / 0
            res[s] = w * m + (1 - w) * np.abs(vv[s])
        out[d, ok] = res
        grp[d, ok] = g
    return out, grp


def _bayes_panel(N, seed):
    """Date 0: lognormal caps, NaN in vol only and NaN in cap only (from N = 9 on), two negative
    vols; date 1: 30 % of the stocks share one cap (equal edges, empty groups)."""
    rng = np.random.default_rng(seed)
    vol = (rng.random((2, N)) * 0.05 + 0.01).astype(np.float32)
    cap = np.exp(rng.standard_normal((2, N)) * 1.3 + 10).astype(np.float32)
    if N >= 9:
        vol[0, rng.random(N) < 0.05] = NAN
        vol[0, 4] = NAN
        cap[0, rng.random(N) < 0.05] = NAN
        cap[0, 7] = NAN
        vol[0, 1], vol[0, 2] = -vol[0, 1], -vol[0, 2]
        tie = rng.random(N) < 0.3
        tie[:3] = True
        cap[1, tie] = np.float32(np.exp(10.5))
    return vol, cap


def _run_bayes(dev, vol, cap, G, q, what):
    want, gw = _bayes(vol, cap, G, q, LD)
    second, _ = _bayes(vol, cap, G, q, np.float64)
    atol = 8 * _dev(second, want)
    got, gg = R.bayes_shrink(_t(vol, dev), _t(cap, dev), G, q, return_groups=True)
    assert got.dtype == torch.float32 and got.shape == vol.shape
    assert np.array_equal(_np(gg).astype(np.int64), gw.astype(np.int64)), \
        f"{what}: {int((_np(gg) != gw).sum())} group codes differ"
    _close(_np(got), want, atol, what)
    return want, gw


# measured atol_case when written: 0 (N = 1) to 1.4e-16 (N = 8193, G = 64); the float32 rounding of
# outputs around 0.03 (3.6e-09) is what decides
BAYES_N = [1, 2, 9, 10, 11, 64, 65, 1023, 1025, 8192, 16385]


@pytest.mark.parametrize("G", [1, 10, 64])
@pytest.mark.parametrize("N", BAYES_N)
def test_bayes_shrink_oracle(dev, N, G):
    """Sizes around the group count, the wave, the block, the LDS sort's power-of-two padding and
    its limit (16385: the presorted path).  8193 and 16384 have tests of their own below."""
    vol, cap = _bayes_panel(N, 6000 + N)
    want, gw = _run_bayes(dev, vol, cap, G, 0.7, f"bayes_shrink N={N} G={G}")
    if N >= 64 and G == 10:
        assert len(np.unique(gw[1][gw[1] >= 0])) < G, "the tied date has empty groups"
        assert len(np.unique(gw[0][gw[0] >= 0])) == G


@pytest.mark.parametrize("N", [8193, 16384])
def test_bayes_shrink_oracle_large_lds(dev, N):
    """8192 < N <= 16384: the LDS sort needs 64 KB of dynamic LDS beside the kernel's static LDS,
    above the default per-launch limit; one call per size."""
    vol, cap = _bayes_panel(N, 6000 + N)
    _run_bayes(dev, vol, cap, 10, 0.7, f"bayes_shrink N={N} G=10")


def test_bayes_shrink_sparse_dates_oracle(dev):
    """Date 0: exactly one valid pair; date 1: 5 valid pairs for 10 groups; date 2: none."""
    rng = np.random.default_rng(6500)
    N = 64
    vol = (rng.random((3, N)) * 0.05 + 0.01).astype(np.float32)
    cap = np.exp(rng.standard_normal((3, N)) * 1.3 + 10).astype(np.float32)
    vol[0, :40] = NAN
    cap[0, 30:] = NAN
    cap[0, 50], vol[0, 50] = 3.0e4, 0.02
    cap[1, 5:] = NAN
    vol[2, :] = NAN
    want, gw = _run_bayes(dev, vol, cap, 10, 0.7, "bayes_shrink sparse dates")
    assert (gw[0] >= 0).sum() == 1 and (gw[1] >= 0).sum() == 5 and (gw[2] == -1).all()
    assert np.isnan(want[0]).all()     # a one-member group shrinks 0 / 0


# ============================================================================== determinism
@pytest.mark.gpu
def test_bayes_shrink_repeats_bitwise(cuda):
    """Five calls on one [32, 5000] input give the same bits (output and groups), and so do two
    calls of ``RiskModel.specific_risk_shrunk``.

    This guard cannot reliably catch a floating-point atomic in the group sums: an order-dependent
    wobble of 1e-16 in a float64 sum rarely crosses a float32 rounding boundary.  That the kernel
    has none is established by reading it (fixed-order lane-strided partial sums and a wave
    butterfly); the test only keeps it that way where a change would show."""
    g = torch.Generator().manual_seed(9)
    vol = (torch.rand(32, 5000, generator=g) * 0.05 + 0.01)
    cap = torch.exp(torch.randn(32, 5000, generator=g) * 1.3 + 10)
    vol[torch.rand(32, 5000, generator=g) < 0.02] = float("nan")
    vol, cap = vol.to(cuda), cap.to(cuda)
    o0, g0 = R.bayes_shrink(vol, cap, 10, 1.0, return_groups=True)
    for _ in range(4):
        o, gg = R.bayes_shrink(vol, cap, 10, 1.0, return_groups=True)
        assert torch.equal(o.nan_to_num(7.0), o0.nan_to_num(7.0)) and torch.equal(gg, g0)

    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(80, 600, 31, 10, seed=11, device=cuda, missing_frac=0.02)
    m = RiskModel(p, preset("reference", eigen_sims=2)).run()
    a = m.specific_risk_shrunk(window=40)
    b = m.specific_risk_shrunk(window=40)
    assert a.shape == (80, 600) and torch.isfinite(a).any()
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))
