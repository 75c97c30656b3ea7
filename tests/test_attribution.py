"""Portfolio risk attribution: exposure kernel vs dense oracle, decomposition identities, and
the link to the reference's pure-factor-portfolio exposures (CrossSection.py:76,104)."""
import pytest
import torch

from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
from llm_driven_multi_factor_model_amd.ops import attribution as attr
from llm_driven_multi_factor_model_amd.ops.cross_section import (pure_factor_portfolio, valid_mask,
                                                                 xs_wls)
from tests._design_row_cases import (SWEEP_D, SWEEP_N, SWEEP_QS, assert_finite, planted_panel,
                                     planted_stats, sweep_params)


def _panel(D=6, N=120, P=5, Q=4, seed=3):
    return synthetic_panel(D, N, P, Q, seed=seed, missing_frac=0.05)


def test_pure_factor_portfolio_has_unit_exposure():
    """Holding row k of Omega gives exactly row k of Omega X (the reference's returned
    pure_factor_portfolio_exposure), which the constraint makes != e_k only in the industries."""
    p = _panel()
    out = xs_wls(p.styles, p.cap, p.ret, p.ind, p.P)
    d = 2
    m = valid_mask(p.styles, p.cap, p.ret, p.ind, p.P)[d]
    Q = p.Q
    omega, omx = pure_factor_portfolio(p.styles[d][:, m], p.cap[d][m], p.ind[d][m], p.P,
                                       out.stats[d, :Q], float(out.stats[d, Q]))
    K = 1 + p.P + Q
    h = torch.zeros(K, p.D, p.N, dtype=torch.float64)
    h[:, d, m] = omega
    for k in (0, 2, 1 + p.P, K - 1):
        x = attr.portfolio_exposure(p.styles, p.cap, p.ret, p.ind, h[k], out.stats, p.P)
        torch.testing.assert_close(x[d], omx[k], rtol=1e-9, atol=1e-10)
    # styles of a style pure-factor portfolio: unit exposure, zero on the other styles
    x = attr.portfolio_exposure(p.styles, p.cap, p.ret, p.ind, h[1 + p.P], out.stats, p.P)[d]
    torch.testing.assert_close(x[1 + p.P:], torch.eye(Q, dtype=torch.float64)[0], rtol=0, atol=1e-9)


def test_decomposition_identities():
    g = torch.Generator().manual_seed(1)
    D, K = 5, 7
    A = torch.randn(D, 40, K, generator=g, dtype=torch.float64)
    F = A.transpose(1, 2) @ A / 40
    x = torch.randn(D, K, generator=g, dtype=torch.float64)
    sv = torch.rand(D, generator=g, dtype=torch.float64) * 1e-2
    r = attr.risk_attribution(x, F, sv)
    torch.testing.assert_close(r.total_var, torch.einsum("dk,dkl,dl->d", x, F, x) + sv)
    torch.testing.assert_close(r.contrib.sum(1), r.factor_var / r.total_vol)
    torch.testing.assert_close(r.pct_var.sum(1) + sv / r.total_var, torch.ones(D, dtype=torch.float64))
    gr = r.grouped(3)
    torch.testing.assert_close(gr["country"] + gr["industry"] + gr["style"] + gr["specific"],
                               torch.ones(D, dtype=torch.float64))


def test_risk_model_attribution_cpu():
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(60, 80, 4, 3, seed=5, missing_frac=0.02)
    m = RiskModel(p, preset("reference", eigen_sims=5)).run()
    h = torch.full((p.N,), 1.0 / p.N, dtype=torch.float64)
    r = m.risk_attribution(h)
    ok = torch.isfinite(r.total_var)
    assert ok[-10:].all()
    assert (r.specific_var[ok] > 0).all() and (r.factor_var[ok] > 0).all()


# The 40-date panel with missing cells, then every Q the dispatch knows and the blocked path of
# wider style sets (17: one style in the second block; 32: two full blocks; 33: a third block) on
# the planted panel.
EXPOSURE_CASES = [pytest.param(40, 1000, 31, 10, torch.float32, False, id="k42-missing-cells"),
                  *(pytest.param(SWEEP_D, SWEEP_N, *s.values, True, id=s.id)
                    for s in sweep_params(SWEEP_QS + (17, 32, 33)))]


@pytest.mark.gpu
@pytest.mark.parametrize("D,N,P,Q,dtype,planted", EXPOSURE_CASES)
def test_hip_portfolio_exposure_matches_oracle(cuda, D, N, P, Q, dtype, planted):
    if planted:
        p, _ = planted_panel(D, N, P, Q, dtype)
        stats = planted_stats(p)
    else:
        p = synthetic_panel(D, N, P, Q, seed=8, missing_frac=0.03, dtype=dtype)
        stats = xs_wls(p.styles, p.cap, p.ret, p.ind, p.P).stats
    g = torch.Generator().manual_seed(2)
    h = torch.rand(p.D, p.N, generator=g, dtype=torch.float64) / p.N
    h[:, ::7] = float("nan")
    ref = attr.portfolio_exposure(p.styles, p.cap, p.ret, p.ind, h, stats, p.P)
    assert_finite(ref)
    gp = p.to(cuda)
    got = attr.portfolio_exposure(gp.styles, gp.cap, gp.ret, gp.ind, h.to(cuda), stats.to(cuda), p.P)
    torch.testing.assert_close(got.cpu(), ref, rtol=1e-11, atol=1e-14)


def _trailing_vol_loop(halo, e, window, min_periods=1):
    """The newest-first tensor loop of RiskModel.specific_vol_series (its CPU path)."""
    D = e.shape[0]
    h = window - 1
    ext = torch.cat([halo, e])
    ok = torch.isfinite(ext)
    okd = ok.double()
    n, s1, s2 = torch.zeros_like(e), torch.zeros_like(e), torch.zeros_like(e)
    x = torch.where(ok, ext, torch.zeros((), dtype=torch.float64, device=e.device))
    for j in range(window):
        sl = slice(h - j, h - j + D)
        n += okd[sl]
        s1 += x[sl]
        s2 += x[sl] * x[sl]
    mean = s1 / n
    vol = torch.sqrt(torch.clamp(s2 / n - mean * mean, min=0.0))
    return torch.where(n >= max(1, min_periods), vol, torch.full_like(vol, float("nan")))


@pytest.mark.gpu
@pytest.mark.parametrize("D,N,window,minp", [(300, 777, 252, 1), (37, 300, 10, 4), (5, 64, 1, 1),
                                             (2520, 520, 252, 20)])
def test_trailing_vol_kernel_is_bitwise_the_loop(cuda, D, N, window, minp):
    """The HIP trailing-vol kernel equals the newest-first tensor loop on the GPU bit for bit
    (NaN rows, NaN halo, partial windows, a tile tail): rank-invariance of the point-in-time
    specific vol rests on that fixed order.  (Against the CPU loop only to 1 ulp: torch's CPU
    sqrt is SLEEF's 0.5001-ulp vector sqrt, not the correctly rounded one.)"""
    g = torch.Generator().manual_seed(D + N)
    e = torch.randn(D, N, generator=g, dtype=torch.float64) * 0.02
    e[torch.rand(D, N, generator=g) < 0.05] = float("nan")
    halo = torch.randn(window - 1, N, generator=g, dtype=torch.float64) * 0.02
    halo[: (window - 1) // 2] = float("nan")
    ref = _trailing_vol_loop(halo.to(cuda), e.to(cuda), window, minp).cpu()
    got = attr.trailing_vol(halo.to(cuda), e.to(cuda), window, minp).cpu()
    assert torch.equal(got.isnan(), ref.isnan())
    assert torch.equal(got.nan_to_num(-1.0), ref.nan_to_num(-1.0))
    cpu = _trailing_vol_loop(halo, e, window, minp)
    torch.testing.assert_close(got, cpu, rtol=4e-16, atol=0, equal_nan=True)
