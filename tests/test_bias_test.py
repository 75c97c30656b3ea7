"""Portfolio bias test: ``ops.bias_test`` (``csrc/portfolio_batch.hip``) and
``RiskModel.bias_test``.

The GPU tests compare the kernel with the CPU path; the CPU path is checked on its own against a
per-(date, portfolio) loop written from ``design_matrix``, against the attribution methods, and
by a calibration experiment with a known answer.

Bound of the kernel tests: every sum is within ``1e-12 * scale`` of the oracle, ``scale`` being
the same sum with the absolute value of every term (for a style exposure the unfolded form
``(sum |h x_q| + |mu_q| sum |h|) / sigma``): both sides sum at most N = 517 terms in float64, so
their rounding errors stay below N eps = 517 * 1.1e-16 = 6e-14 of the scale; 1e-12 leaves a 16x
margin.  ``factor_var`` and ``z`` are checked at rtol 1e-10 on long-only weights with
``F = A A^T + 0.1 I``, where the oracle's own cancellation is mild.
"""
import functools
import math
import os
import subprocess
import sys

import pandas as pd
import pytest
import torch

from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
from llm_driven_multi_factor_model_amd.ops import bias_test as bt
from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
from llm_driven_multi_factor_model_amd.ops.cross_section import valid_mask, xs_wls
from tests._design_row_cases import (SWEEP_D, SWEEP_N, assert_finite, planted_panel,
                                     planted_stats, sweep_params)

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 3, 63, 65, 203, 517)
BS = (1, 5, 16, 17, 33, 70)
PQS = ((0, 1), (3, 3), (2, 13), (31, 10), (5, 16), (47, 16))
BMAX = max(BS)


class Case:
    """Seeded inputs over D = 5 dates: panel (missing_frac = 0.2) + stats, F = A A^T + 0.1 I,
    s with NaN / 0 / negative / inf entries, a universe mask, long-only weights [5, 70, N] with
    NaN entries.  Date 1 has no valid stock (no specific-risk forecast), date 2 a NaN F, date 3
    a NaN stats row.  ``planted``: D = 2 dates of the Q sweeps' panel
    (tests/_design_row_cases.py) with none of the three, so that every output is finite."""

    def __init__(self, N, P, Q, dtype, signed=False, planted=False):
        D = SWEEP_D if planted else 5
        if planted:
            p, _ = planted_panel(D, N, P, Q, dtype)
            self.stats = planted_stats(p)
        else:
            p = synthetic_panel(D, N, P, Q, seed=11 + N, missing_frac=0.2, dtype=dtype)
            self.stats = xs_wls(p.styles, p.cap, p.ret, p.ind, P).stats.to(F64).clone()
            self.stats[3, 0] = float("nan")
        self.p, self.D, self.N, self.P, self.Q, self.K = p, D, N, P, Q, 1 + P + Q
        K = self.K
        g = torch.Generator().manual_seed(500 + N)
        A = torch.randn(D, K, K, generator=g, dtype=F64) / math.sqrt(K)
        self.F = A @ A.transpose(1, 2) + 0.1 * torch.eye(K, dtype=F64)
        s = 0.01 + 0.03 * torch.rand(D, N, generator=g, dtype=F64)
        s[0, 0::11] = float("nan")
        s[0, 1::13] = 0.0
        if not planted:
            self.F[2, K // 2, 0] = float("nan")
            s[4, 2::7] = -0.02
            s[4, 3::17] = float("inf")
            s[1] = float("nan")
        self.s = s
        self.universe = torch.rand(D, N, generator=g) < 0.8
        if signed:
            H = torch.randn(D, BMAX, N, generator=g, dtype=F64)
        else:
            H = torch.rand(D, BMAX, N, generator=g, dtype=F64)
        H[torch.rand(D, BMAX, N, generator=g) < 0.03] = float("nan")
        H[0, 0, -1] = float("inf")
        self.H = H

    def args(self, dev, d0=0, d1=None):
        p = self.p.slice_dates(d0, self.D if d1 is None else d1).to(dev)
        return p.styles, p.cap, p.ret, p.ind, self.stats[d0:d1].to(dev), self.P

    def rest(self, dev, d0=0, d1=None):
        return dict(F=self.F[d0:d1].to(dev), spec_vol=self.s[d0:d1].to(dev),
                    universe=self.universe[d0:d1].to(dev))


@functools.lru_cache(maxsize=None)
def _case(*a, **kw):
    return Case(*a, **kw)


def _forecast(c, dev, H, per_date, d0=0, d1=None, expo=True):
    r = c.rest(dev, d0, d1)
    return bt.portfolio_forecast(*c.args(dev, d0, d1), H.to(dev), r["F"], r["spec_vol"],
                                 per_date=per_date, universe=r["universe"], return_exposure=expo)


def _scales(c, H, per_date, d0=0, d1=None):
    """The sums with absolute values of every term: (exposure [D, B, K], realised [D, B])."""
    X, cap, ret, ind, stats, P = c.args("cpu", d0, d1)
    D, Q, N = X.shape
    s, u = c.s[d0:d1], c.universe[d0:d1]
    m = valid_mask(X, cap, ret, ind, P) & torch.isfinite(s) & (s > 0) & u
    h = H if per_date else H[None].expand(D, -1, -1)
    ha = torch.where(torch.isfinite(h) & m[:, None, :], h, torch.zeros((), dtype=F64)).abs()
    held = ha.sum(-1)
    cols = [held[..., None]]
    if P > 0:
        oh = torch.nn.functional.one_hot(ind.long().clamp(0, P - 1), P).double()
        cols.append(torch.einsum("dbn,dnp->dbp", ha, oh))
    xa = torch.nan_to_num(X.double()).abs()
    mu, sig = stats[:, :Q], stats[:, Q]
    cols.append((torch.einsum("dbn,dqn->dbq", ha, xa) + mu.abs()[:, None, :] * held[..., None])
                / sig[:, None, None])
    r = torch.einsum("dbn,dn->db", ha, torch.nan_to_num(ret.double()).abs())
    return torch.cat(cols, -1), r


def _close(got, want, scale, name):
    got = got.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{name}: NaN pattern"
    ok = ~torch.isnan(want)
    err = (got - want)[ok].abs()
    bound = 1e-12 * scale[ok]
    assert (err <= bound).all(), f"{name}: {float((err - bound).max()):.3e} over the bound"


def _check(c, dev, H, per_date, d0=0, d1=None, variance=True):
    got = _forecast(c, dev, H, per_date, d0, d1)
    want = _forecast(c, "cpu", H, per_date, d0, d1)
    xs, rs = _scales(c, H, per_date, d0, d1)
    _close(got.exposure, want.exposure, xs, "exposure")
    _close(got.realised, want.realised, rs, "realised")
    _close(got.specific_var, want.specific_var, want.specific_var, "specific_var")
    _close(got.held, want.held, want.held, "held")
    _close(got.gross, want.gross, want.gross, "gross")
    cov_g, cov_w = (got.held / got.gross).cpu(), want.held / want.gross
    torch.testing.assert_close(cov_g, cov_w, rtol=0, atol=1e-12, equal_nan=True)
    assert torch.equal(torch.isnan(got.factor_var.cpu()), torch.isnan(want.factor_var))
    if variance:
        torch.testing.assert_close(got.factor_var.cpu(), want.factor_var, rtol=1e-10, atol=0,
                                   equal_nan=True)
        torch.testing.assert_close(bt.standardised(got).cpu(), bt.standardised(want), rtol=1e-10,
                                   atol=0, equal_nan=True)
    return want


# ------------------------------------------------------------------ kernel against the CPU path
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("P,Q", PQS)
def test_kernel_matches_cpu_path(cuda, P, Q, dtype):
    for N in NS:
        c = _case(N, P, Q, dtype)
        for B in BS:
            Hd = c.H[:, :B].contiguous()
            want = _check(c, cuda, Hd, True)                    # D = 5, per-date
            _check(c, cuda, Hd[0], False)                       # D = 5, static
            _check(c, cuda, Hd[:1], True, 0, 1)                 # D = 1
            _check(c, cuda, Hd[0], False, 0, 1)
    # at the largest N, the planted dates do what they are there for
    assert (want.held[1] == 0).all() and (want.gross[1] > 0).all()
    assert torch.isnan(want.factor_var[2]).all() and not torch.isnan(want.exposure[2]).any()
    assert torch.isnan(want.factor_var[3]).all() and torch.isnan(want.exposure[3]).all()
    assert torch.isfinite(want.factor_var[[0, 1, 4]]).all() and (want.factor_var[1] == 0).all()
    assert torch.isfinite(want.realised).all() and torch.isfinite(want.specific_var).all()


@pytest.mark.gpu
@pytest.mark.parametrize("P,Q,dtype", sweep_params())
def test_kernel_q_sweep(cuda, P, Q, dtype):
    """Every Q the dispatch knows at N = 300 (five 64-stock chunks, the last one ragged) and
    B = 17 (a second wave with one portfolio), on the planted panel."""
    c = _case(SWEEP_N, P, Q, dtype, planted=True)
    Hd = c.H[:, :17].contiguous()
    assert_finite(*_forecast(c, "cpu", Hd, True))   # before any GPU run
    _check(c, cuda, Hd, True)
    _check(c, cuda, Hd[0], False)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("P,Q", PQS)
def test_kernel_sums_signed_weights(cuda, P, Q, dtype):
    """Long-short weights: the sums cancel, the bound (absolute-value scale) does not."""
    c = _case(517, P, Q, dtype, signed=True)
    _check(c, cuda, c.H[:, :33].contiguous(), True, variance=False)
    _check(c, cuda, c.H[1, :17].contiguous(), False, variance=False)


@pytest.mark.gpu
def test_kernel_no_universe_no_exposure_1d_weights(cuda):
    c = _case(203, 3, 3, torch.float32)
    a = bt.portfolio_forecast(*c.args(cuda), c.H[0, 0].to(cuda), c.F.to(cuda), c.s[0].to(cuda))
    b = bt.portfolio_forecast(*c.args("cpu"), c.H[0, 0], c.F, c.s[0])
    assert a.exposure is None and a.factor_var.shape == (5, 1)
    for x, y in zip(a[:5], b[:5]):
        torch.testing.assert_close(x.cpu(), y, rtol=1e-10, atol=1e-14, equal_nan=True)
    n = bt.portfolio_forecast(*c.args(cuda), c.H[0, :3].to(cuda), None, c.s.to(cuda))
    assert torch.isnan(n.factor_var).all() and torch.isfinite(n.specific_var).all()


# --------------------------------------------------------------------------------------- bitwise
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_kernel_bitwise(cuda, dtype):
    c = _case(517, 31, 10, dtype)
    H = c.H[:, :33].contiguous()

    def same(a, b):
        for x, y in zip(a, b):
            assert torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0))

    full = _forecast(c, cuda, H, True)
    same(full, _forecast(c, cuda, H, True))                                  # two calls agree
    for b in (0, 15, 16, 20, 32):                                            # a row on its own
        one = _forecast(c, cuda, H[:, b:b + 1].contiguous(), True)
        same(one, [t[:, b:b + 1] for t in full])
    static = _forecast(c, cuda, H[4], False)                                 # static == expanded
    same(static, _forecast(c, cuda, H[4][None].expand(5, -1, -1), True))
    part = _forecast(c, cuda, H[2:5].contiguous(), True, 2, 5)               # dates [2:5]
    same(part, [t[2:5] for t in full])


# ---------------------------------------------------------------------------------------- limits
@pytest.mark.gpu
@pytest.mark.parametrize("P,Q", [(48, 16), (3, 17)])
def test_gpu_limits_raise_before_launch(cuda, P, Q):
    p = synthetic_panel(2, 40, P, Q, seed=2)
    K = 1 + P + Q
    stats = xs_wls(p.styles, p.cap, p.ret, p.ind, P).stats
    H, F, s = torch.rand(3, 40, dtype=F64), torch.eye(K, dtype=F64).expand(2, K, K), \
        torch.full((40,), 0.02, dtype=F64)
    r = bt.portfolio_forecast(p.styles, p.cap, p.ret, p.ind, stats, P, H, F, s)   # CPU: any K
    assert torch.isfinite(r.factor_var).all()
    g = p.to(cuda)
    with pytest.raises(ValueError, match="K = 1 \\+ P \\+ Q"):
        bt.portfolio_forecast(g.styles, g.cap, g.ret, g.ind, stats.to(cuda), P, H.to(cuda),
                              F.to(cuda), s.to(cuda))


def test_wrong_shapes_raise():
    p = synthetic_panel(3, 20, 2, 2, seed=2)
    stats = xs_wls(p.styles, p.cap, p.ret, p.ind, 2).stats
    a = (p.styles, p.cap, p.ret, p.ind, stats, 2)
    H, F, s = torch.rand(4, 20, dtype=F64), torch.eye(5, dtype=F64).expand(3, 5, 5), \
        torch.full((20,), 0.02, dtype=F64)
    bt.portfolio_forecast(*a, H, F, s)
    with pytest.raises(ValueError, match="H must be"):
        bt.portfolio_forecast(*a, H[:, :19], F, s)
    with pytest.raises(ValueError, match="H must be"):
        bt.portfolio_forecast(*a, H, F, s, per_date=True)
    with pytest.raises(ValueError, match="F must be"):
        bt.portfolio_forecast(*a, H, F[:, :4, :4], s)
    with pytest.raises(ValueError, match="spec_vol must be"):
        bt.portfolio_forecast(*a, H, F, torch.ones(2, 20, dtype=F64))
    with pytest.raises(ValueError, match="stats must be"):
        bt.portfolio_forecast(*a[:4], stats[:, :3], 2, H, F, s)
    with pytest.raises(ValueError, match="universe must be"):
        bt.portfolio_forecast(*a, H, F, s, universe=torch.ones(3, 19, dtype=torch.bool))


# ---------------------------------------------------------------- the CPU path, independently
@pytest.mark.parametrize("per_date", [False, True])
def test_cpu_path_matches_python_loop(per_date):
    c = _case(63, 3, 3, torch.float64, signed=True)
    B = 4
    H = c.H[:, :B].contiguous() if per_date else c.H[0, :B].contiguous()
    got = _forecast(c, "cpu", H, per_date)
    X, cap, ret, ind, stats, P = c.args("cpu")
    m = valid_mask(X, cap, ret, ind, P) & torch.isfinite(c.s) & (c.s > 0) & c.universe
    Xd = fc.design_matrix(X, cap, ret, ind, torch.nan_to_num(stats), P, m)
    for d in range(c.D):
        for b in range(B):
            h = H[d, b] if per_date else H[b]
            fin = torch.isfinite(h)
            idx = torch.nonzero(m[d] & fin).flatten()
            hv = h[idx]
            x = Xd[d, idx].T @ hv
            stats_ok = bool(torch.isfinite(stats[d, :c.Q + 1]).all())
            want = dict(specific_var=(hv * hv * c.s[d, idx] ** 2).sum(),
                        realised=(hv * ret[d, idx].double()).sum(), held=hv.abs().sum(),
                        gross=h[fin].abs().sum(),
                        factor_var=x @ c.F[d] @ x if stats_ok else torch.tensor(float("nan")))
            for k, v in want.items():
                torch.testing.assert_close(getattr(got, k)[d, b], v.to(F64), rtol=1e-12,
                                           atol=1e-15, equal_nan=True, msg=f"{k} {d} {b}")
            if stats_ok:
                torch.testing.assert_close(got.exposure[d, b], x, rtol=1e-11, atol=1e-13)
            else:
                assert torch.isnan(got.exposure[d, b]).all()


def _model(seed=21, D=37):
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(D, 64, 4, 3, seed=seed, missing_frac=0.05)
    return RiskModel(p, preset("reference", eigen_sims=5)).run()


@functools.lru_cache(maxsize=None)
def _shared_model():
    return _model()


@pytest.mark.parametrize("which,specific_vol", [("vra", "shrunk"), ("eigen", "use4")])
def test_in_sample_forecast_equals_risk_attribution(which, specific_vol):
    from llm_driven_multi_factor_model_amd.ops.attribution import portfolio_specific_var
    m = _shared_model()
    p = m.panel
    s = m._specific_vol_named(specific_vol)
    ok = valid_mask(p.styles, p.cap, p.ret, p.ind, p.P) & torch.isfinite(s) & (s > 0)
    g = torch.Generator().manual_seed(4)
    h = torch.where(ok, torch.rand(p.D, p.N, generator=g, dtype=F64), torch.zeros((), dtype=F64))
    r = m.bias_test(h, which, specific_vol, per_date=True, out_of_sample=False, window=10,
                    min_periods=3)
    ra = m.risk_attribution(h, which, specific_vol)
    fin = torch.isfinite(ra.total_vol) & (ra.total_var > 0)
    assert fin.sum() > 20
    torch.testing.assert_close(r.forecast_vol[:, 0][fin], ra.total_vol[fin], rtol=1e-12, atol=0)
    fcst = bt.portfolio_forecast(p.styles, p.cap, p.ret, p.ind, m.stats, p.P, h,
                                 {"vra": m.vra_cov, "eigen": m.eigen_cov}[which], s,
                                 per_date=True)
    torch.testing.assert_close(fcst.specific_var[:, 0], portfolio_specific_var(h, s), rtol=1e-12,
                               atol=0)
    held = ok.any(1)   # a date with no forecast holds nothing: coverage 0 / 0
    assert torch.equal(torch.isnan(r.coverage[:, 0]), ~held)
    torch.testing.assert_close(r.coverage[held, 0], torch.ones(int(held.sum()), dtype=F64),
                               rtol=0, atol=1e-12)


# ---------------------------------------------------------------------- alignment, calibration
def _planted(scale=1.0, D=400, N=60, B=8, P=3, Q=2, seed=5):
    """ret = X f + e with f ~ N(0, F), e ~ N(0, s^2); stats = (mu 0, sigma 1), so X_d is the raw
    [1 | one-hot | styles].  Forecasts passed: ``scale`` times the true F and s^2."""
    g = torch.Generator().manual_seed(seed)
    K = 1 + P + Q
    X = torch.randn(D, Q, N, generator=g, dtype=F64)
    ind = torch.randint(0, P, (D, N), generator=g).to(torch.int16)
    cap = torch.ones(D, N, dtype=F64)
    stats = torch.zeros(D, Q + 2, dtype=F64)
    stats[:, Q], stats[:, Q + 1] = 1.0, N
    A = 0.01 * torch.randn(K, K, generator=g, dtype=F64)
    F = A @ A.T
    s = 0.01 + 0.02 * torch.rand(N, generator=g, dtype=F64)
    Xd = fc.design_matrix(X, cap, cap, ind, stats, P)
    f = torch.randn(D, K, generator=g, dtype=F64) @ torch.linalg.cholesky(
        F + 1e-14 * torch.eye(K, dtype=F64)).T
    ret = torch.einsum("dnk,dk->dn", Xd, f) + s * torch.randn(D, N, generator=g, dtype=F64)
    H = torch.randn(B, N, generator=g, dtype=F64)
    H[:B // 2] = H[:B // 2].abs()
    fcst = bt.portfolio_forecast(X, cap, ret, ind, stats, P, H, (scale * F).expand(D, K, K),
                                 math.sqrt(scale) * s)
    z = bt.standardised(fcst)
    return bt.bias_stats(z, torch.full((251, B), float("nan"), dtype=F64), z)


def test_calibration_bias_is_one_for_the_true_model():
    band = 4.0 / math.sqrt(2 * 400)   # four standard errors of a std over 400 dates
    st = _planted(1.0)
    assert (st.n_obs == 400).all()
    assert ((st.bias - 1.0).abs() < band).all(), st.bias
    half = _planted(4.0)               # variances 4x too large: z halves
    assert ((half.bias - 0.5).abs() < band).all(), half.bias
    torch.testing.assert_close(half.bias, 0.5 * st.bias, rtol=1e-12, atol=0)


def test_out_of_sample_alignment():
    m = _shared_model()
    p = m.panel
    g = torch.Generator().manual_seed(9)
    H = torch.rand(3, p.N, generator=g, dtype=F64)
    r = m.bias_test(H, "vra", "shrunk", window=10, min_periods=3)
    assert torch.isnan(r.z[0]).all() and torch.isnan(r.forecast_vol[0]).all()
    s = m.specific_risk_shrunk()
    q = p.slice_dates(1, p.D)
    hand = bt.portfolio_forecast(q.styles, q.cap, q.ret, q.ind, m.stats[1:], p.P, H,
                                 m.vra_cov[:-1], s[:-1])
    torch.testing.assert_close(r.z[1:], bt.standardised(hand), rtol=0, atol=0, equal_nan=True)
    torch.testing.assert_close(r.realised[1:], hand.realised, rtol=0, atol=0)
    assert torch.isfinite(r.z[-1]).all()
    # start: the statistics drop the earlier dates, the per-date outputs do not
    r2 = m.bias_test(H, "vra", "shrunk", window=10, min_periods=3, start=20)
    torch.testing.assert_close(r2.z, r.z, rtol=0, atol=0, equal_nan=True)
    fin = torch.isfinite(r.z[20:]).sum(0)
    assert torch.equal(r2.stats.n_obs, fin)
    torch.testing.assert_close(r2.stats.bias, r.z[20:].std(0, unbiased=False), rtol=1e-12, atol=0)


def test_bias_test_errors_match_siblings():
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    m = _shared_model()
    h = torch.ones(m.panel.N, dtype=F64)
    with pytest.raises(KeyError):
        m.bias_test(h, which="nope")
    with pytest.raises(ValueError, match="specific volatilities"):
        m.bias_test(h, specific_vol=None)
    fresh = RiskModel(m.panel, m.cfg)
    with pytest.raises(RuntimeError, match="regress"):
        fresh.bias_test(h)


# ------------------------------------------------------------------------------------ statistics
def test_statistics_of_unit_z():
    z = torch.ones(40, 3, dtype=F64)
    z[1::2] = -1.0
    z[5, 1] = float("nan")
    z[6, 1] = float("nan")
    halo = torch.full((9, 3), float("nan"), dtype=F64)
    st = bt.bias_stats(z, halo, z, window=10, min_periods=4)
    assert torch.equal(st.q_stat, torch.ones(3, dtype=F64))
    assert torch.equal(st.n_obs, torch.tensor([40, 38, 40]))
    torch.testing.assert_close(st.bias, torch.ones(3, dtype=F64), rtol=1e-15, atol=0)
    st2 = bt.bias_stats(2 * z, halo, 2 * z, window=10, min_periods=4)
    torch.testing.assert_close(st2.bias, 2 * st.bias, rtol=1e-15, atol=0)
    torch.testing.assert_close(st2.q_stat, torch.full((3,), 4 - math.log(4.0), dtype=F64))
    zz = z.clone()
    zz[3, 0] = 0.0      # a zero z counts for the bias, not for Q (ln 0)
    st3 = bt.bias_stats(zz, halo, zz, window=10, min_periods=4)
    assert st3.n_obs[0] == 40 and st3.q_stat[0] == 1.0


def test_rolling_bias_matches_naive_loop():
    g = torch.Generator().manual_seed(3)
    z = torch.randn(60, 5, generator=g, dtype=F64)
    z[torch.rand(60, 5, generator=g) < 0.15] = float("nan")
    z[10:19, 2] = float("nan")
    W, MP = 12, 5
    halo = torch.randn(W - 1, 5, generator=g, dtype=F64)
    halo[:4] = float("nan")
    st = bt.bias_stats(z, halo, z, window=W, min_periods=MP)
    ext = torch.cat([halo, z])
    want = torch.full_like(z, float("nan"))
    for t in range(60):
        for b in range(5):
            w = ext[t:t + W, b]
            w = w[torch.isfinite(w)]
            if len(w) >= MP:
                want[t, b] = w.std(unbiased=False)
    torch.testing.assert_close(st.rolling_bias, want, rtol=1e-12, atol=1e-12, equal_nan=True)
    assert torch.isnan(want).any() and torch.isfinite(want).any()
    dev = (want - 1).abs()
    for t in range(60):
        row = dev[t][torch.isfinite(dev[t])]
        if len(row):
            torch.testing.assert_close(st.mrad[t], row.mean(), rtol=1e-12, atol=1e-14)
        else:
            assert torch.isnan(st.mrad[t])
    torch.testing.assert_close(st.mrad_mean, dev[torch.isfinite(dev)].mean(), rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_rolling_bias_gpu_uses_trailing_vol(cuda):
    g = torch.Generator().manual_seed(3)
    z = torch.randn(50, 7, generator=g, dtype=F64)
    z[torch.rand(50, 7, generator=g) < 0.1] = float("nan")
    halo = torch.full((11, 7), float("nan"), dtype=F64)
    a = bt.bias_stats(z, halo, z, window=12, min_periods=5)
    zc = z.to(cuda)
    b = bt.bias_stats(zc, halo.to(cuda), zc, window=12, min_periods=5)
    for x, y in zip(a, b):
        torch.testing.assert_close(y.cpu(), x, rtol=1e-12, atol=1e-14, equal_nan=True)


@pytest.mark.gpu
def test_model_bias_test_gpu_matches_cpu(cuda):
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    m = _shared_model()
    gm = RiskModel(m.panel.to(cuda), m.cfg).run()
    g = torch.Generator().manual_seed(9)
    H = torch.rand(5, m.panel.N, generator=g, dtype=F64)
    b = gm.bias_test(H.to(cuda), window=10, min_periods=3)
    # the device model's own forecasts (its eigen adjustment draws other random numbers than the
    # CPU model's), shifted by hand and sent through the CPU path
    p = m.panel
    q = p.slice_dates(1, p.D)
    hand = bt.portfolio_forecast(q.styles, q.cap, q.ret, q.ind, gm.stats[1:].cpu(), p.P, H,
                                 gm.vra_cov[:-1].cpu(), gm.specific_risk_shrunk()[:-1].cpu())
    z = bt.standardised(hand)
    assert torch.isnan(b.z[0]).all() and torch.isfinite(z[-1]).all()
    torch.testing.assert_close(b.z[1:].cpu(), z, rtol=1e-10, atol=0, equal_nan=True)
    torch.testing.assert_close(b.realised[1:].cpu(), hand.realised, rtol=1e-10, atol=1e-15)
    nan = torch.full((9, 5), float("nan"), dtype=F64)
    zc = b.z.cpu()
    want = bt.bias_stats(zc, nan, zc, window=10, min_periods=3)
    for x, y in zip(b.stats, want):
        torch.testing.assert_close(x.cpu(), y, rtol=1e-12, atol=1e-14, equal_nan=True)


# ------------------------------------------------------------------------------------------- CLI
def test_cli_bias_test(tmp_path):
    d = str(tmp_path)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")

    def cli(*args):
        return subprocess.run([sys.executable, "-m", "llm_driven_multi_factor_model_amd.cli",
                               *args], cwd=ROOT, capture_output=True, text=True, timeout=600,
                              env=env)

    r = cli("synth", "--out", d, "--dates", "45", "--stocks", "70", "--industries", "5")
    assert r.returncode == 0, r.stderr
    stocks = pd.read_csv(f"{d}/barra_data_csi.csv")["stocknames"].astype(str).unique()
    g = torch.Generator().manual_seed(1)
    w = pd.DataFrame({"stocknames": stocks,
                      "random": torch.rand(len(stocks), generator=g).numpy(),
                      "first_half": [1.0 if i < len(stocks) // 2 else 0.0
                                     for i in range(len(stocks))],
                      "long_short": torch.randn(len(stocks), generator=g).numpy()})
    w.to_csv(f"{d}/portfolios.csv", index=False)
    r = cli("risk", "--data", f"{d}/barra_data_csi.csv", "--industry", f"{d}/industry_info.csv",
            "--out", f"{d}/res", "--sims", "4", "--bias-test", f"{d}/portfolios.csv",
            "--bias-test-window", "12", "--specific-model", "use4", "--device", "cpu")
    assert r.returncode == 0, r.stderr[-3000:]
    out = pd.read_csv(f"{d}/res/bias_test.csv", index_col=0)
    assert list(out.index) == ["random", "first_half", "long_short"]
    assert list(out.columns) == ["bias", "n_obs", "q_stat", "mrad", "coverage"]
    assert pd.notna(out["bias"]).all() and (out["bias"] > 0).all()
    # the first date has no forecast (nor have the dates before the covariance series starts)
    assert ((out["n_obs"] > 10) & (out["n_obs"] <= 44)).all()
    assert ((out["coverage"] > 0) & (out["coverage"] <= 1)).all()
