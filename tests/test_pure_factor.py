"""Pure factor portfolios and factor-return t-statistics: ``ops.pure_factor``
(``csrc/pure_factor.hip``), the three ``RiskModel`` methods and ``cli risk --factor-stats``.

The CPU path (dense ``design_matrix``, batched ``pinv``) is checked against the single-date
``pure_factor_portfolio``, against ``xs_wls``, by the identities of the estimator covariance, by a
closed form and by a planted panel; the GPU tests compare the kernels with the CPU path.

Panels: ``synthetic_panel(seed=7, missing_frac=0.05)`` with, where P > 0, industry 0 (never the
pivot) emptied on date 1 and the last industry emptied on date 2: both dates are rank-deficient
by exactly 1, through an exact zero row of the constrained normal matrix.
"""
import dataclasses
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
from llm_driven_multi_factor_model_amd.ops import bias_test as bt
from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
from llm_driven_multi_factor_model_amd.ops import pure_factor as pf
from llm_driven_multi_factor_model_amd.ops.cross_section import (pure_factor_portfolio,
                                                                 valid_mask, xs_wls)
from tests._design_row_cases import (SWEEP_D, SWEEP_N, assert_finite, planted_panel,
                                     sweep_params)

F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_SHAPES = ((6, 203, 5, 4, F64), (4, 517, 31, 10, F64), (5, 65, 3, 2, F32), (3, 64, 0, 1, F64))
GPU_PQS = ((0, 1), (5, 4), (31, 10), (47, 16))
GPU_NS = (3, 63, 65, 203, 517)


def _empty(p, d, j):
    ind = p.ind.clone()
    ind[d][ind[d] == j] = -1
    return dataclasses.replace(p, ind=ind)


class Case:
    """Panel, regression and CPU-path results of one shape.  ``planted``: the panel of the Q
    sweeps (tests/_design_row_cases.py), every date of full rank with finite results."""

    def __init__(self, D, N, P, Q, dtype, nan_stats_date=None, planted=False):
        if planted:
            p, _ = planted_panel(D, N, P, Q, dtype)
        else:
            p = synthetic_panel(D, N, P, Q, seed=7, missing_frac=0.05, dtype=dtype)
        if P > 1 and D >= 3:
            p = _empty(_empty(p, 1, 0), 2, P - 1)
        self.p, self.D, self.N, self.P, self.Q, self.K = p, D, N, P, Q, 1 + P + Q
        self.xs = xs_wls(p.styles, p.cap, p.ret, p.ind, P)
        self.stats = self.xs.stats.to(F64).clone()
        if nan_stats_date is not None:
            self.stats[nan_stats_date, 0] = float("nan")
        self.est = pf.estimator_cov(*self.args("cpu"))
        self.omega = pf.pure_factor_weights(*self.args("cpu"), self.est.C)
        self.fs = pf.factor_return_stats(*self.args("cpu"), self.xs.f, self.xs.resid, self.est)
        if planted:
            assert_finite(self.stats, self.est.C, self.omega, *self.fs)

    def args(self, dev, d0=0, d1=None):
        p = self.p.slice_dates(d0, self.D if d1 is None else d1).to(dev)
        return p.styles, p.cap, p.ret, p.ind, self.stats[d0:d1].to(dev), self.P

    def valid(self):
        p = self.p
        return valid_mask(p.styles, p.cap, p.ret, p.ind, self.P)

    def pivot(self, d):
        """Last industry with a positive cap sum on date d (pivot_mode 0)."""
        p, m = self.p, self.valid()[d]
        s = torch.zeros(self.P, dtype=F64).index_add_(0, p.ind[d][m].long(), p.cap[d][m].double())
        return int(torch.nonzero(s > 0).max())

    def normal_matrix(self, d):
        """(G, A, R) of date d from the dense design matrix: G = X^T W X, A = R^T G R."""
        p, m = self.p, self.valid()[d]
        Xd = fc.design_matrix(*self.args("cpu"))[d][m]
        c = p.cap[d][m].double()
        G = Xd.T @ (Xd * torch.sqrt(c)[:, None])
        K, P = self.K, self.P
        R = torch.eye(K, dtype=F64)
        if P > 0:
            s = (Xd[:, 1:1 + P] * c[:, None]).sum(0)
            pv = self.pivot(d)
            R[1 + pv, 1:1 + P] = -s / s[pv]
            R = torch.cat([R[:, :1 + pv], R[:, 2 + pv:]], 1)
        return G, R.T @ G @ R, R


@functools.lru_cache(maxsize=None)
def _case(*a, **kw):
    return Case(*a, **kw)


def _close_per_date(got, want, bound, name):
    """|got - want| <= bound * max |want[d]| for every date d; equal NaN patterns."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, f"{name}: {tuple(got.shape)} vs {tuple(want.shape)}"
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{name}: NaN pattern"
    D = want.shape[0]
    g, w = torch.nan_to_num(got.reshape(D, -1)), torch.nan_to_num(want.reshape(D, -1))
    scale = w.abs().amax(1)
    err = (g - w).abs().amax(1)
    print(f"{name}: worst err / max = {float((err / scale.clamp(min=1e-300)).max()):.3e}")
    assert (err <= bound * scale).all(), \
        f"{name}: {float((err / scale.clamp(min=1e-300)).max()):.3e} of the date's max > {bound}"


def _same_bits(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


# ------------------------------------------------------------------ the CPU path, independently
@pytest.mark.parametrize("D,N,P,Q,dtype", CPU_SHAPES)
def test_oracle_matches_single_date_function(D, N, P, Q, dtype):
    c = _case(D, N, P, Q, dtype)
    m = c.valid()
    for d in range(D):
        idx = torch.nonzero(m[d]).flatten()
        want, _ = pure_factor_portfolio(c.p.styles[d][:, idx], c.p.cap[d, idx],
                                        c.p.ind[d, idx] if P > 0 else None, P, c.stats[d, :Q],
                                        float(c.stats[d, Q]), c.pivot(d) if P > 0 else None)
        got = c.omega[d]
        scale = float(want.abs().max())
        assert float((got[:, idx] - want).abs().max()) <= 1e-10 * scale, d
        assert (got[:, ~m[d]] == 0).all()


@pytest.mark.parametrize("D,N,P,Q,dtype", CPU_SHAPES)
def test_weights_give_the_factor_returns(D, N, P, Q, dtype):
    c = _case(D, N, P, Q, dtype)
    r = torch.where(c.valid(), c.p.ret.double(), torch.zeros((), dtype=F64))
    torch.testing.assert_close(torch.einsum("dkn,dn->dk", c.omega, r), c.xs.f, rtol=1e-9,
                               atol=1e-12)
    if P > 1:   # an emptied industry has a zero portfolio and f = 0
        assert (c.omega[1, 1] == 0).all() and abs(float(c.xs.f[1, 1])) < 1e-15
        assert (c.omega[2, P] == 0).all() and abs(float(c.xs.f[2, P])) < 1e-15


@pytest.mark.parametrize("D,N,P,Q,dtype", CPU_SHAPES)
def test_identities_and_rank(D, N, P, Q, dtype):
    c = _case(D, N, P, Q, dtype)
    m = c.valid()
    w = torch.sqrt(torch.where(m, c.p.cap.double(), torch.zeros((), dtype=F64)))
    winv = torch.where(w > 0, 1.0 / w, torch.zeros_like(w))
    assert torch.equal(c.est.C, c.est.C.transpose(1, 2))
    _close_per_date(torch.einsum("din,dn,djn->dij", c.omega, winv, c.omega), c.est.C, 1e-10,
                    "Omega W^-1 Omega^T")
    for d in range(D):
        G, A, _ = c.normal_matrix(d)
        Cd = c.est.C[d]
        assert float((Cd @ G @ Cd - Cd).abs().max()) <= 1e-10 * float(Cd.abs().max()), d
        assert int(c.est.rank[d]) == int(torch.linalg.matrix_rank(A, rtol=1e-15)), d
    full = c.K - (1 if P > 0 else 0)
    want = [full - (1 if (P > 1 and d in (1, 2)) else 0) for d in range(D)]
    assert c.est.rank.tolist() == want
    assert torch.equal(c.est.n, c.valid().sum(1).double())


@pytest.mark.parametrize("D,N,P,Q,dtype", CPU_SHAPES[:3])
def test_style_portfolios_through_the_forecast_call(D, N, P, Q, dtype):
    c = _case(D, N, P, Q, dtype)
    styles = list(range(1 + P, c.K))
    H = c.omega[:, styles].contiguous()
    r = bt.portfolio_forecast(*c.args("cpu"), H, None, torch.ones(N, dtype=F64), per_date=True)
    torch.testing.assert_close(r.realised, c.xs.f[:, styles], rtol=1e-10, atol=1e-14)


def test_standard_errors_closed_form_without_industries():
    D, N, P, Q, dtype = CPU_SHAPES[3]
    c = _case(D, N, P, Q, dtype)
    m = c.valid()
    Xd = fc.design_matrix(*c.args("cpu"))
    for d in range(D):
        w = np.sqrt(c.p.cap[d][m[d]].double().numpy())
        Xt = Xd[d][m[d]].numpy() * np.sqrt(w)[:, None]
        e = c.xs.resid[d][m[d]].double().numpy()
        n, K = Xt.shape
        s2 = float((w * e * e).sum() / (n - K))
        se = np.sqrt(np.diag(s2 * np.linalg.inv(Xt.T @ Xt)))
        np.testing.assert_allclose(c.fs.se[d].numpy(), se, rtol=1e-10, atol=0)
        np.testing.assert_allclose(float(c.fs.sigma2[d]), s2, rtol=1e-10, atol=0)
        np.testing.assert_allclose(c.fs.t[d].numpy(), c.xs.f[d].numpy() / se, rtol=1e-10, atol=0)
        assert float(c.fs.dof[d]) == n - K


def test_planted_panel_t_has_unit_spread():
    """ret = X f + sigma eps / sqrt(w) with one style's true return 0: that style's t is Student
    t with about 190 degrees of freedom, so its std over 400 dates is 1 within four standard
    errors, 4 / sqrt(2 * 400) = 0.14; and t does not move when cap is scaled."""
    D, N, P, Q = 400, 200, 3, 3
    g = torch.Generator().manual_seed(12)
    X = torch.randn(D, Q, N, generator=g, dtype=F64)
    ind = torch.randint(0, P, (D, N), generator=g).to(torch.int16)
    cap = torch.exp(torch.randn(D, N, generator=g, dtype=F64))
    st0 = torch.zeros(D, Q + 2, dtype=F64)
    st0[:, Q], st0[:, Q + 1] = 1.0, N
    Xd = fc.design_matrix(X, cap, cap, ind, st0, P)       # raw [1 | one-hot | styles]
    f_true = 0.01 * torch.randn(D, 1 + P + Q, generator=g, dtype=F64)
    f_true[:, 1 + P + 1] = 0.0
    ret = torch.einsum("dnk,dk->dn", Xd, f_true) \
        + 0.02 * torch.randn(D, N, generator=g, dtype=F64) / cap ** 0.25
    band = 4.0 / math.sqrt(2 * D)
    ts = []
    for scale in (1.0, 100.0):
        cp = cap * scale
        r = xs_wls(X, cp, ret, ind, P)
        a = (X, cp, ret, ind, r.stats, P)
        fs = pf.factor_return_stats(*a, r.f, r.resid, pf.estimator_cov(*a))
        t = fs.t[:, 1 + P + 1]
        assert torch.isfinite(t).all() and (fs.dof == N - (P + Q)).all()
        assert abs(float(t.std(unbiased=False)) - 1.0) < band, float(t.std(unbiased=False))
        ts.append(fs.t)
    torch.testing.assert_close(ts[1], ts[0], rtol=1e-9, atol=1e-12)
    # the other styles' true returns are not zero: their t is wider
    assert float(ts[0][:, 1 + P].std()) > 1.5


def test_edges_nan_patterns():
    D, N, P, Q = 5, 40, 4, 2
    p = synthetic_panel(D, N, P, Q, seed=3, missing_frac=0.05, dtype=F64)
    ind = p.ind.clone()
    ind[1] = -1                              # date 1: no valid stock
    ind[2][ind[2] == P - 1] = -1             # date 2: empty last industry
    p = dataclasses.replace(p, ind=ind)
    r = xs_wls(p.styles, p.cap, p.ret, p.ind, P)
    stats = r.stats.clone()
    stats[3, 1] = float("nan")               # date 3: NaN stats row
    a = (p.styles, p.cap, p.ret, p.ind, stats, P)
    for mode, bad in ((0, [1, 3]), (1, [1, 2, 3])):
        est = pf.estimator_cov(*a, pivot_mode=mode)
        good = [d for d in range(D) if d not in bad]
        assert torch.isnan(est.C[bad]).all() and (est.rank[bad] == 0).all()
        assert torch.isfinite(est.C[good]).all() and (est.rank[good] > 0).all()
        om = pf.pure_factor_weights(*a, est.C)
        assert torch.isnan(om[bad]).all() and torch.isfinite(om[good]).all()
        rm = xs_wls(p.styles, p.cap, p.ret, p.ind, P, pivot_mode=mode)
        fs = pf.factor_return_stats(*a, rm.f, rm.resid, est)
        assert torch.isnan(fs.se[bad]).all() and torch.isnan(fs.t[bad]).all()
        assert torch.isfinite(fs.se[good]).all() and torch.isfinite(fs.sigma2[good]).all()
        # an empty industry: f = 0, se = 0, t NaN
        if mode == 0:
            assert fs.se[2, P] == 0 and torch.isnan(fs.t[2, P]) and abs(float(rm.f[2, P])) < 1e-15
            assert torch.isfinite(fs.t[2, :P]).all()
    # a NaN C (of any date) is a NaN date of the weights, whatever rows are asked for
    Cn = pf.estimator_cov(*a).C.clone()
    Cn[0, 0, 1] = float("nan")
    assert torch.isnan(pf.pure_factor_weights(*a, Cn, [P + 1])[0]).all()


def test_edge_fewer_stocks_than_factors():
    """N = 3 stocks, P = 5 industries: n <= rank, no degrees of freedom; C is still returned."""
    p = synthetic_panel(4, 3, 5, 2, seed=7, dtype=F64)
    r = xs_wls(p.styles, p.cap, p.ret, p.ind, 5)
    a = (p.styles, p.cap, p.ret, p.ind, r.stats, 5)
    est = pf.estimator_cov(*a)
    ok = torch.isfinite(r.stats[:, 2]) & (r.stats[:, 2] > 0)
    assert ok.any()
    fs = pf.factor_return_stats(*a, r.f, r.resid, est)
    assert torch.isfinite(est.C[ok]).all() and (est.rank[ok] > 0).all()
    assert (fs.dof[ok] <= 0).all() and (est.rank[ok] <= 3).all()
    assert torch.isnan(fs.sigma2).all() and torch.isnan(fs.se).all() and torch.isnan(fs.t).all()


def test_wrong_arguments_raise():
    c = _case(*CPU_SHAPES[2])
    a = c.args("cpu")
    with pytest.raises(ValueError, match="pivot_mode"):
        pf.estimator_cov(*a, pivot_mode=2)
    with pytest.raises(ValueError, match="factors must index"):
        pf.pure_factor_weights(*a, c.est.C, [c.K])
    with pytest.raises(ValueError, match="C must be"):
        pf.pure_factor_weights(*a, c.est.C[:, :2, :2])
    with pytest.raises(ValueError, match="resid must be"):
        pf.factor_return_stats(*a, c.xs.f, c.xs.resid[:, :-1], c.est)
    with pytest.raises(ValueError, match="f must be"):
        pf.factor_return_stats(*a, c.xs.f[:, :-1], c.xs.resid, c.est)


# ----------------------------------------------------------------------------- selection, model
def _model(dev="cpu", pivot_mode=0):
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.utils.config import preset
    c = _case(*CPU_SHAPES[0])
    m = RiskModel(c.p.to(dev), preset("reference", pivot_mode=pivot_mode))
    m.regress()
    return m


def test_factor_subsets_and_model_selectors():
    c = _case(*CPU_SHAPES[0])
    P, K = c.P, c.K
    sub = pf.pure_factor_weights(*c.args("cpu"), c.est.C, [K - 1, 0, 3, K - 1])
    torch.testing.assert_close(sub, c.omega[:, [K - 1, 0, 3, K - 1]], rtol=1e-12, atol=1e-18)
    assert pf.pure_factor_weights(*c.args("cpu"), c.est.C, []).shape == (c.D, 0, c.N)
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    with pytest.raises(RuntimeError, match="regress"):
        RiskModel(c.p).pure_factor_portfolios()
    m = _model()
    om = m.pure_factor_portfolios()
    torch.testing.assert_close(om, c.omega, rtol=0, atol=0)
    def same(a, b):   # the CPU path's matrix product rounds differently for another S
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-18)

    same(m.pure_factor_portfolios("all"), om)
    same(m.pure_factor_portfolios("country"), om[:, :1])
    same(m.pure_factor_portfolios("industries"), om[:, 1:1 + P])
    same(m.pure_factor_portfolios("styles"), om[:, 1 + P:])
    same(m.pure_factor_portfolios([2, 1]), om[:, [2, 1]])
    with pytest.raises(ValueError, match="factors must be"):
        m.pure_factor_portfolios("style")
    assert torch.equal(m.estimator_cov().rank, c.est.rank)
    ts = m.factor_tstats()
    torch.testing.assert_close(ts.t, c.fs.t, rtol=0, atol=0, equal_nan=True)
    # config.pivot_mode reaches the estimator: date 2 has an empty last industry
    m1 = _model(pivot_mode=1)
    assert torch.isnan(m1.estimator_cov().C[2]).all() and torch.isnan(m1.factor_tstats().t[2]).all()
    assert torch.isfinite(m1.estimator_cov().C[[0, 1, 3]]).all()


def test_cli_factor_stats(tmp_path):
    d = str(tmp_path)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")

    def cli(*args):
        return subprocess.run([sys.executable, "-m", "llm_driven_multi_factor_model_amd.cli",
                               *args], cwd=ROOT, capture_output=True, text=True, timeout=600,
                              env=env)

    r = cli("synth", "--out", d, "--dates", "30", "--stocks", "60", "--industries", "4")
    assert r.returncode == 0, r.stderr
    r = cli("risk", "--data", f"{d}/barra_data_csi.csv", "--industry", f"{d}/industry_info.csv",
            "--out", f"{d}/res", "--sims", "4", "--factor-stats", "--device", "cpu")
    assert r.returncode == 0, r.stderr[-3000:]
    ts = pd.read_csv(f"{d}/res/factor_tstats.csv")
    assert list(ts.columns) == ["date", "factor", "f", "se", "t"]
    K = ts["factor"].nunique()
    assert len(ts) == 30 * K and K == 1 + 4 + 10
    ok = ts["se"] > 0
    assert ok.mean() > 0.9
    np.testing.assert_allclose(ts["t"][ok], (ts["f"] / ts["se"])[ok], rtol=1e-9)
    sig = pd.read_csv(f"{d}/res/factor_significance.csv", index_col=0)
    assert list(sig.columns) == ["mean_abs_t", "share_abs_t_gt_2", "n_obs"]
    assert list(sig.index) == list(ts["factor"][:K])
    assert ((sig["share_abs_t_gt_2"] >= 0) & (sig["share_abs_t_gt_2"] <= 1)).all()
    by = ts.assign(a=ts["t"].abs()).groupby("factor", sort=False)["a"]
    np.testing.assert_allclose(sig["mean_abs_t"].to_numpy(), by.mean().to_numpy(), rtol=1e-9)


# ------------------------------------------------------------------ kernels against the CPU path
def _gpu_cases(P, Q, dtype):
    """(case, d0, d1) over the grid: D = 5 (dates 1 and 2 with an emptied industry, date 3 with a
    NaN stats row) and D = 1 (date 1 alone)."""
    for N in GPU_NS:
        c = _case(5, N, P, Q, dtype, nan_stats_date=3)
        yield c, 0, 5
        yield c, 1, 2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("P,Q", GPU_PQS)
def test_estimator_cov_kernel_matches_cpu_path(cuda, P, Q, dtype):
    for c, d0, d1 in _gpu_cases(P, Q, dtype):
        got = pf.estimator_cov(*c.args(cuda, d0, d1))
        name = f"C N={c.N} D={d1 - d0}"
        print(name, "rank", got.rank.tolist(), "cpu", c.est.rank[d0:d1].tolist())
        _close_per_date(got.C, c.est.C[d0:d1], 1e-9, name)
        assert torch.equal(got.rank.cpu(), c.est.rank[d0:d1]), name
        assert _same_bits(got.C, got.C.transpose(1, 2))
        again = pf.estimator_cov(*c.args(cuda, d0, d1))
        assert _same_bits(again.C, got.C) and torch.equal(again.rank, got.rank)
        torch.testing.assert_close(got.n.cpu(), c.est.n[d0:d1], rtol=0, atol=0, equal_nan=True)
    assert torch.isnan(c.est.C[3]).all() and c.est.rank[3] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("pivot_mode", [0, 1])
def test_estimator_cov_kernel_pivot_modes(cuda, pivot_mode):
    c = _case(*CPU_SHAPES[0])
    want = pf.estimator_cov(*c.args("cpu"), pivot_mode=pivot_mode)
    got = pf.estimator_cov(*c.args(cuda), pivot_mode=pivot_mode)
    _close_per_date(got.C, want.C, 1e-9, "C")
    assert torch.equal(got.rank.cpu(), want.rank)
    assert bool(torch.isnan(want.C[2]).all()) == (pivot_mode == 1)


def _check_weights(c, cuda, d0=0, d1=None):
    """One row, nine rows and all K rows of Omega against the CPU path (both sides use its C);
    returns the S = K result."""
    d1 = c.D if d1 is None else d1
    K = c.K
    Cg = c.est.C[d0:d1].to(cuda)
    for sel in ([K // 2], [int(i) % K for i in range(3, 12)], None):
        got = pf.pure_factor_weights(*c.args(cuda, d0, d1), Cg, sel)
        want = c.omega[d0:d1] if sel is None else c.omega[d0:d1][:, sel]
        _close_per_date(got, want, 1e-11, f"Omega N={c.N} D={d1 - d0} S={want.shape[1]}")
        assert _same_bits(pf.pure_factor_weights(*c.args(cuda, d0, d1), Cg, sel), got)
    return got


def _check_stats(c, cuda, d0=0, d1=None):
    d1 = c.D if d1 is None else d1
    est = pf.EstCov(*(t[d0:d1].to(cuda) for t in c.est))
    a = (*c.args(cuda, d0, d1), c.xs.f[d0:d1].to(cuda), c.xs.resid[d0:d1].to(cuda), est)
    got = pf.factor_return_stats(*a)
    want = pf.FactorStats(*(t[d0:d1] for t in c.fs))
    for x, y, nm in zip(got, want, got._fields):
        torch.testing.assert_close(x.cpu(), y, rtol=1e-10, atol=0, equal_nan=True,
                                   msg=lambda s: f"{nm} N={c.N} D={d1 - d0}: {s}")
    again = pf.factor_return_stats(*a)
    assert all(_same_bits(x, y) for x, y in zip(got, again))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("P,Q", GPU_PQS)
def test_weights_kernel_matches_cpu_path(cuda, P, Q, dtype):
    """Bound: 1e-11 of each date's max |Omega| (both sides use the CPU path's C)."""
    K = 1 + P + Q
    for c, d0, d1 in _gpu_cases(P, Q, dtype):
        Cg = c.est.C[d0:d1].to(cuda)
        got = _check_weights(c, cuda, d0, d1)
        if d1 - d0 == 5:   # got is the S = K call: a row alone, and dates [2:5] alone
            for j in (0, K // 2, K - 1):
                one = pf.pure_factor_weights(*c.args(cuda), Cg, [j])
                assert _same_bits(one[:, 0], got[:, j]), (c.N, j)
            part = pf.pure_factor_weights(*c.args(cuda, 2, 5), Cg[2:5].contiguous())
            assert _same_bits(part, got[2:5]), c.N
            assert torch.isnan(got[3]).all() and not torch.isnan(got[[0, 4]]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("P,Q", GPU_PQS)
def test_factor_stats_kernel_matches_cpu_path(cuda, P, Q, dtype):
    for c, d0, d1 in _gpu_cases(P, Q, dtype):
        _check_stats(c, cuda, d0, d1)


# Every Q the dispatch knows, on the planted panel; and N = 2100, which crosses the weights
# kernel's 2048-stock chunk and leaves its last 52 stocks without a second stock per thread.
SWEEP = [*(pytest.param(SWEEP_N, *s.values, id=s.id) for s in sweep_params()),
         pytest.param(2100, 3, 4, F32, id="p3-q4-f32-n2100")]


@pytest.mark.gpu
@pytest.mark.parametrize("N,P,Q,dtype", SWEEP)
def test_weights_kernel_q_sweep(cuda, N, P, Q, dtype):
    _check_weights(_case(SWEEP_D, N, P, Q, dtype, planted=True), cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("N,P,Q,dtype", SWEEP)
def test_factor_stats_kernel_q_sweep(cuda, N, P, Q, dtype):
    _check_stats(_case(SWEEP_D, N, P, Q, dtype, planted=True), cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("P,Q", [(48, 16), (3, 17)])
def test_gpu_limits_raise_before_launch(cuda, P, Q):
    p = synthetic_panel(2, 80, P, Q, seed=2, dtype=F64)
    r = xs_wls(p.styles, p.cap, p.ret, p.ind, P)
    a = (p.styles, p.cap, p.ret, p.ind, r.stats, P)
    est = pf.estimator_cov(*a)                                        # CPU: any K
    om = pf.pure_factor_weights(*a, est.C, [0])
    fs = pf.factor_return_stats(*a, r.f, r.resid, est)
    assert torch.isfinite(est.C).all() and torch.isfinite(om).all() and torch.isfinite(fs.se).all()
    g = p.to(cuda)
    ga = (g.styles, g.cap, g.ret, g.ind, r.stats.to(cuda), P)
    with pytest.raises(ValueError, match="K = 1 \\+ P \\+ Q"):
        pf.estimator_cov(*ga)
    with pytest.raises(ValueError, match="K = 1 \\+ P \\+ Q"):
        pf.pure_factor_weights(*ga, est.C.to(cuda), [0])
    with pytest.raises(ValueError, match="K = 1 \\+ P \\+ Q"):
        pf.factor_return_stats(*ga, r.f.to(cuda), r.resid.to(cuda), est)


@pytest.mark.gpu
def test_model_methods_gpu_match_cpu(cuda):
    m, g = _model(), _model(cuda)
    P = m.panel.P
    ce, ge = m.estimator_cov(), g.estimator_cov()
    _close_per_date(ge.C, ce.C, 1e-8, "C")
    assert torch.equal(ge.rank.cpu(), ce.rank) and torch.equal(ge.n.cpu(), ce.n)
    ct, gt = m.factor_tstats(), g.factor_tstats()
    for x, y in zip(gt, ct):
        torch.testing.assert_close(x.cpu(), y, rtol=1e-8, atol=1e-14, equal_nan=True)
    for sel in (None, "styles", [P, 0]):
        _close_per_date(g.pure_factor_portfolios(sel), m.pure_factor_portfolios(sel), 1e-8,
                        f"Omega {sel}")
    # the style portfolios through the bias test's forecast kernel give the style returns back
    H = g.pure_factor_portfolios("styles")
    p = g.panel
    r = bt.portfolio_forecast(p.styles, p.cap, p.ret, p.ind, g.stats, p.P, H, None,
                              torch.ones(p.N, dtype=F64, device=cuda), per_date=True)
    torch.testing.assert_close(r.realised.cpu(), m.factor_ret[:, 1 + P:], rtol=1e-8, atol=1e-12)
