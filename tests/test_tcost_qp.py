"""Linear trading costs in the optimisers (``ops.tcost_qp``, ``csrc/tcost_qp.hip``,
``box_qp`` / ``exposure_qp`` / ``RiskModel.optimize`` with ``prev`` / ``tcost`` and
``RiskModel.rebalance``).

The algorithm-independent oracle is the KKT conditions of

    min 1/2 h' Sigma h - q' h + sum kappa |h - p|,   sum_U h = budget,   lo <= h <= hi

against the dense ``Sigma_d`` of each date: with r = Sigma h - q (- X_S eta with exposure
constraints), s- = -kappa if h <= p else kappa and s+ = kappa if h >= p else -kappa (the ends of
the cost's subdifferential), there is one gamma with gamma >= r + s- - eps on stocks strictly
inside the box and at the upper bound, and gamma <= r + s+ + eps on stocks strictly inside the
box and at the lower bound, eps = 10 tol max(max|r|, max kappa) (the solver's tol = 1e-10 with
the x10 margin of ``test_box_qp``); the box holds exactly, the budget to 1e-12 (sum|h| +
|budget|), and weights off the universe are 0.  The GPU tests check the kernel against the CPU
transcription and the GPU's weights against the CPU's and the same KKT check.
"""
import functools

import pytest
import torch

from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
from llm_driven_multi_factor_model_amd.ops import box_qp as bq
from llm_driven_multi_factor_model_amd.ops import exposure_qp as eq
from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
from llm_driven_multi_factor_model_amd.ops import tcost_qp as tc
from tests.test_box_qp import (E2E, SCENARIOS, Case, _assert_matches_cpu, _case, _dense_sigma,
                               _project_inputs, _risk_model)

F64 = torch.float64
INF = float("inf")
NAN = float("nan")
TOL = 1e-10
KAPPAS = (2e-5, 2e-4)
SHAPES = [((4, 203, 5, 4), torch.float32), ((3, 1000, 31, 10), torch.float64)]


def _full(t, D, N):
    return torch.as_tensor(0.0 if t is None else t, dtype=F64).expand(D, N)


@functools.lru_cache(maxsize=None)
def _prev(c: Case, scenario):
    """"Yesterday": the cost-free solution of the scenario rolled by one date."""
    q, lo, hi = c.scenario(scenario)
    r = bq.box_qp(*c.panel_args, c.F, c.s, q, lo, hi)
    assert (r.status == bq.OK).all()
    return r.weights.roll(1, 0)


@functools.lru_cache(maxsize=None)
def _cpu(c: Case, scenario, kappa):
    q, lo, hi = c.scenario(scenario)
    return bq.box_qp(*c.panel_args, c.F, c.s, q, lo, hi, max_passes=64, prev=_prev(c, scenario),
                     tcost=kappa)


def _check_kkt(c: Case, weights, q, lo, hi, prev, kappa, budget=1.0, tol=TOL, dates=None,
               what="", shift=None):
    """``shift`` [D, N]: what the exposure constraints add to r (X_S eta), None without."""
    q, lo, hi = _full(q, c.D, c.N), _full(lo, c.D, c.N), _full(hi, c.D, c.N)
    prev = torch.nan_to_num(_full(prev, c.D, c.N), nan=0.0, posinf=0.0, neginf=0.0)
    kappa = _full(kappa, c.D, c.N)
    for d, ds in enumerate(_dense_sigma(c)):
        if ds is None or (dates is not None and d not in dates):
            continue
        idx, Sig = ds
        h, l, u, p, k = weights[d, idx], lo[d, idx], hi[d, idx], prev[d, idx], kappa[d, idx]
        out = torch.ones(c.N, dtype=torch.bool)
        out[idx] = False
        assert (weights[d, out] == 0).all(), f"{what} date {d}: weight outside the universe"
        assert ((h >= l) & (h <= u)).all(), f"{what} date {d}: box"
        berr = abs(h.sum().item() - budget)
        r = Sig @ h - q[d, idx]
        if shift is not None:
            r = r - shift[d, idx]
        eps = 10 * tol * max(r.abs().max().item(), k.max().item())
        sm = torch.where(h <= p, -k, k)
        sp = torch.where(h >= p, k, -k)
        # a stock pinned by lo = hi has no condition: any r is met by its two bound multipliers
        free, atl, atu = (h > l) & (h < u), (h <= l) & (l < u), (h >= u) & (l < u)
        g_lo = max([-INF] + [(r + sm)[m].max().item() - eps for m in (free, atu) if m.any()])
        g_hi = min([INF] + [(r + sp)[m].min().item() + eps for m in (free, atl) if m.any()])
        print(f"{what} date {d}: free {int(free.sum())}/{len(idx)}, untraded "
              f"{int((h == p).sum())}, KKT gap {(g_lo - g_hi) / eps:.2e} eps, budget error "
              f"{berr:.1e}")
        assert berr <= 1e-12 * (h.abs().sum().item() + abs(budget)), f"{what} date {d}: budget"
        assert g_lo <= g_hi, f"{what} date {d}: no gamma satisfies KKT ({g_lo} > {g_hi})"


# ------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("shape,dtype", SHAPES)
def test_kkt_against_dense_sigma(shape, dtype, scenario, kappa):
    c = _case(*shape, dtype=dtype)
    q, lo, hi = c.scenario(scenario)
    p = _prev(c, scenario)
    r = _cpu(c, scenario, kappa)
    print("passes", r.passes.tolist(), "turnover", r.turnover.tolist())
    assert (r.status == bq.OK).all() and (r.passes <= 64).all()
    _check_kkt(c, r.weights, q, lo, hi, p, kappa, what=f"{scenario} {kappa}")
    # the fields match their definitions; variance stays h' Sigma h
    trade = (r.weights - p).abs().sum(-1)
    assert torch.equal(r.turnover, trade)
    torch.testing.assert_close(r.cost, kappa * trade, rtol=1e-13, atol=0)
    for d, (idx, Sig) in enumerate(_dense_sigma(c)):
        h = r.weights[d, idx]
        assert abs(r.variance[d].item() - (h @ Sig @ h).item()) <= 1e-12 * r.variance[d].item()


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("shape,dtype", SHAPES)
def test_zero_cost_equals_box_qp(shape, dtype, scenario):
    c = _case(*shape, dtype=dtype)
    q, lo, hi = c.scenario(scenario)
    ref = bq.box_qp(*c.panel_args, c.F, c.s, q, lo, hi)
    r = bq.box_qp(*c.panel_args, c.F, c.s, q, lo, hi, prev=_prev(c, scenario),
                  tcost=torch.zeros(c.D, c.N, dtype=F64))
    assert (r.status == bq.OK).all() and (r.cost == 0).all()
    err = (r.weights - ref.weights).abs().amax(-1)
    print("kappa = 0 vs box_qp:", (err / ref.weights.abs().amax(-1)).max().item())
    assert (err <= 1e-9 * ref.weights.abs().amax(-1)).all()
    # tcost=None is the call it was
    r0 = bq.box_qp(*c.panel_args, c.F, c.s, q, lo, hi, prev=None, tcost=None)
    assert type(r0) is bq.BoxQP
    for a, b in zip(r0, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("scenario", ("cap", "long-short"))
def test_turnover_nonincreasing_in_kappa(scenario):
    c = _case(3, 1000, 31, 10, dtype=torch.float64)
    q, lo, hi = c.scenario(scenario)
    p = _prev(c, scenario)
    last = first = None
    for f in (0.0, 0.01, 0.1, 1.0):
        r = bq.box_qp(*c.panel_args, c.F, c.s, q, lo, hi, max_passes=64, prev=p, tcost=2e-4 * f)
        assert (r.status == bq.OK).all()
        print(f"kappa {2e-4 * f:g}: turnover {r.turnover.tolist()}")
        if last is not None:
            assert (r.turnover <= last + 1e-8).all(), (f, r.turnover, last)
        last = r.turnover
        first = last if first is None else first
    assert (last < first).all()          # and the cost does bite


@pytest.mark.parametrize("shape,dtype", SHAPES)
def test_large_kappa_freezes_a_feasible_book(shape, dtype):
    c = _case(*shape, dtype=dtype)
    _, lo, hi = c.scenario("long-short")
    p = bq.box_qp(*c.panel_args, c.F, c.s, c.alpha / 20, lo, hi).weights     # feasible
    q = c.alpha / 50
    kap = torch.zeros(c.D, dtype=F64)
    for d, (idx, Sig) in enumerate(_dense_sigma(c)):
        r = Sig @ p[d, idx] - q[d, idx]
        kap[d] = r.max() - r.min()
    r = bq.box_qp(*c.panel_args, c.F, c.s, q, lo, hi, prev=p,
                  tcost=kap[:, None].expand(c.D, c.N))
    print("frozen: turnover", r.turnover.tolist(), "passes", r.passes.tolist())
    assert (r.status == bq.OK).all()
    assert (r.turnover <= 1e-12 * (p.abs().sum(-1) + 1.0)).all()


def test_edge_cases():
    c = _case(4, 203, 5, 4)
    q, lo, hi = c.scenario("long-short")
    args = (*c.panel_args, c.F, c.s, q, lo, hi)
    # prev outside the box, NaN, and nonzero off the universe: the box still holds exactly
    g = torch.Generator().manual_seed(5)
    p = 0.02 * torch.randn(c.D, c.N, generator=g, dtype=F64)
    p[:, 3::19] = NAN
    off = torch.ones(c.D, c.N, dtype=torch.bool)
    for d, (idx, _) in enumerate(_dense_sigma(c)):
        off[d, idx] = False
    assert (p[off] != 0).any() and ((p < lo) | (p > hi)).any()
    r = bq.box_qp(*args, max_passes=64, prev=p, tcost=2e-5)
    assert (r.status == bq.OK).all()
    _check_kkt(c, r.weights, q, lo, hi, p, 2e-5, what="wild prev")
    pz = torch.nan_to_num(p, nan=0.0)
    assert torch.equal(r.turnover, (r.weights - pz).abs().sum(-1))   # off-universe sales count
    # kappa = +inf on some names: they end at clip(prev, lo, hi); cost counts them 0
    kap = torch.full((c.D, c.N), 2e-5, dtype=F64)
    kap[:, 1::7] = INF
    r = bq.box_qp(*args, max_passes=64, prev=p, tcost=kap)
    assert (r.status == bq.OK).all() and torch.isfinite(r.cost).all()
    pin = pz.clamp(lo, hi)
    on = ~off
    assert torch.equal(r.weights[:, 1::7][on[:, 1::7]], pin[:, 1::7][on[:, 1::7]])
    lo2, hi2 = _full(lo, c.D, c.N).clone(), _full(hi, c.D, c.N).clone()
    lo2[:, 1::7], hi2[:, 1::7] = pin[:, 1::7], pin[:, 1::7]
    _check_kkt(c, r.weights, q, lo2, hi2, p, torch.where(kap == INF, 0.0, kap), what="frozen")
    kf = torch.where(kap == INF, 0.0, kap)
    torch.testing.assert_close(r.cost, (kf * (r.weights - pz).abs()).sum(-1), rtol=1e-13, atol=0)
    # a NaN or a negative kappa on a stock of the universe: that date is INVALID
    for badk in (NAN, -1e-5):
        kap = torch.full((c.D, c.N), 2e-5, dtype=F64)
        kap[1, _dense_sigma(c)[1][0][3]] = badk
        kap[2, torch.nonzero(off[2])[0]] = badk          # off the universe: ignored
        r = bq.box_qp(*args, max_passes=64, prev=p, tcost=kap)
        assert r.status.tolist() == [bq.OK, bq.INVALID, bq.OK, bq.OK]
        assert torch.isnan(r.weights[1]).all() and torch.isnan(r.turnover[1])
    # the edge case of test_box_qp: INVALID / INFEASIBLE where box_qp gives them
    e = _case(4, 203, 5, 4, edge=True)
    pe = torch.full((e.N,), 1.0 / e.N, dtype=F64)
    r = bq.box_qp(*e.panel_args, e.F, e.s, None, 0.0, 1.0, universe=e.universe, max_passes=64,
                  prev=pe, tcost=2e-5)
    assert r.status.tolist() == [bq.OK, bq.OK, bq.INVALID, bq.OK]
    assert torch.isnan(r.weights[2]).all() and torch.isnan(r.cost[2])
    _check_kkt(e, r.weights, None, 0.0, 1.0, pe, 2e-5, what="edge")
    r = bq.box_qp(*e.panel_args, e.F, e.s, None, 0.0, 1.0 / (2 * e.N), universe=e.universe,
                  prev=pe, tcost=2e-5)
    assert (r.status == bq.INFEASIBLE).all() and torch.isnan(r.weights).all()
    # one date does not depend on the others
    full = _cpu(c, "long-short", 2e-5)
    pp = _prev(c, "long-short")
    p1 = c.p.slice_dates(2, 3)
    r1 = bq.box_qp(p1.styles, p1.cap, p1.ret, p1.ind, c.stats[2:3], c.P, c.F[2:3], c.s, q[2:3],
                   lo, hi, max_passes=64, prev=pp[2:3], tcost=2e-5)
    assert torch.equal(r1.status, full.status[2:3]) and torch.equal(r1.passes, full.passes[2:3])
    torch.testing.assert_close(r1.weights, full.weights[2:3], rtol=0, atol=1e-15)
    # prev and tcost go together
    with pytest.raises(ValueError, match="tcost"):
        bq.box_qp(*args, prev=p)
    with pytest.raises(ValueError, match="prev"):
        bq.box_qp(*args, tcost=2e-5)
    with pytest.raises(ValueError):
        eq.exposure_qp(*c.panel_args, c.F, c.s, [2], torch.zeros(1, dtype=F64), tcost=2e-5)
    # a zero-date block
    p0 = c.p.slice_dates(0, 0)
    r = bq.box_qp(p0.styles, p0.cap, p0.ret, p0.ind, c.stats[:0], c.P, c.F[:0], c.s, prev=0.0,
                  tcost=0.0)
    assert r.weights.shape == (0, c.N) and r.turnover.shape == (0,)


def _neutral_setup(c: Case):
    """Industries + SIZE (the first style) neutral to a cap-weighted benchmark, 2 % cap."""
    U = fc.universe_mask(c.p.styles, c.p.cap, c.p.ret, c.p.ind, c.P, c.s)
    hb = torch.where(U, c.p.cap.double(), torch.zeros((), dtype=F64))
    hb = hb / hb.sum(-1, keepdim=True)
    sel = list(range(1, 2 + c.P))
    t = fc.factor_xty(*c.panel_args, hb[:, None])[:, 0][:, sel]
    q = fc.apply_cov(*c.panel_args, c.F, c.s, hb)
    return sel, t, q


def test_exposure_qp_with_costs():
    c = _case(3, 1000, 31, 10, dtype=torch.float64)
    sel, t, q = _neutral_setup(c)
    base = eq.exposure_qp(*c.panel_args, c.F, c.s, sel, t, q, 0.0, 0.02)
    assert (base.status == eq.OK).all()
    p = base.weights.roll(1, 0)
    r = eq.exposure_qp(*c.panel_args, c.F, c.s, sel, t, q, 0.0, 0.02, prev=p, tcost=2e-5)
    print("passes", r.passes.tolist(), "gap", r.exposure_gap.tolist(), "turnover",
          r.turnover.tolist(), "cost-free turnover", (base.weights - p).abs().sum(-1).tolist())
    assert (r.status == eq.OK).all()
    habs = r.weights.abs().sum(-1)
    Xd = torch.nan_to_num(fc.design_matrix(*c.panel_args))
    x = torch.einsum("dnk,dn->dk", Xd, r.weights)[:, sel]
    assert (r.exposure_gap <= 1e-10 * habs.clamp(min=1.0)).all()
    # from the dense design matrix, with the bound of test_exposure_qp
    assert ((x - t).abs().amax(-1) <= 1e-9 * habs.clamp(min=1.0)).all()
    shift = torch.einsum("dnk,dk->dn", Xd[:, :, sel], r.eta)
    _check_kkt(c, r.weights, q, 0.0, 0.02, p, 2e-5, what="neutral", shift=shift)
    assert (r.turnover < (base.weights - p).abs().sum(-1)).all()
    # no factors: box_qp with the same prev / tcost
    c = _case(4, 203, 5, 4)
    q, lo, hi = c.scenario("long-short")
    pv = _prev(c, "long-short")
    r = eq.exposure_qp(*c.panel_args, c.F, c.s, [], torch.zeros(0), q, lo, hi, max_passes=64,
                       prev=pv, tcost=2e-5)
    b = _cpu(c, "long-short", 2e-5)
    for name in ("weights", "gamma", "variance", "passes", "status", "turnover", "cost"):
        assert torch.equal(getattr(r, name), getattr(b, name)), name


def test_risk_model_optimize_and_rebalance_cpu():
    m = _risk_model()
    p = m.panel
    sv = m.specific_risk_shrunk()
    kw = dict(upper=0.05, specific_vol=sv)
    base = m.optimize(**kw)
    assert base.turnover is None and base.cost is None
    fin = base.status == bq.OK
    first = int(torch.nonzero(fin)[0])
    # tcost = 0: rebalance is the per-date optimum
    r0 = m.rebalance(tcost=0.0, **kw)
    assert torch.equal(r0.status, base.status) and r0.weights.shape == (p.D, p.N)
    err = (r0.weights - base.weights)[fin].abs().amax(-1)
    assert (err <= 1e-9 * base.weights[fin].abs().amax(-1)).all()
    # the fields match their definitions, with [N] and [D, N] costs
    kap = 1e-4 * (1.0 + torch.arange(p.N, dtype=F64) / p.N)
    prev = base.weights[-1]
    r = m.optimize(prev=prev, tcost=kap, **kw)
    assert torch.equal(r.status, base.status)
    trade = (r.weights - prev).abs()
    assert torch.equal(r.turnover[fin], trade.sum(-1)[fin])
    torch.testing.assert_close(r.cost[fin], (kap * trade).sum(-1)[fin], rtol=1e-13, atol=0)
    assert torch.isnan(r.turnover[~fin]).all()
    w, var, passes, status, active, ret, gap, eta = r[:8]     # the earlier fields as before
    assert gap is None and eta is None and r[8] is r.turnover and r[9] is r.cost
    # kappa > 0: row t is a one-date optimize from the drifted row t - 1; dead dates carry
    # the holdings through
    start = torch.full((p.N,), 1.0 / p.N, dtype=F64)
    rb = m.rebalance(start=start, tcost=kap, **kw)
    assert torch.equal(rb.status, base.status) and not fin[0]      # the first dates are INVALID
    hold = start
    for t in range(p.D):
        if t > 0:
            ret_t = torch.nan_to_num(p.ret[t - 1].double())
            hold = hold * (1 + ret_t) / (1 + (hold * ret_t).sum())
        if t <= first + 4 or t >= p.D - 5:      # each row stands on the row before: a few do
            one = m.optimize(prev=hold, tcost=kap, dates=(t, t + 1), **kw)
            assert one.weights.shape == (1, p.N)
            assert torch.equal(one.weights[0], rb.weights[t]) or not fin[t]
            assert torch.equal(one.turnover[0], rb.turnover[t]) or not fin[t]
        if fin[t]:
            hold = rb.weights[t]
        else:
            assert torch.isnan(rb.weights[t]).all()
    # the drifted start reached the first live date untouched by the dead dates before it
    assert rb.turnover[first] > 0
    nd = m.rebalance(start=start, drift=False, tcost=kap, **kw)
    one = m.optimize(prev=start, tcost=kap, dates=(first, first + 1), **kw)
    assert torch.equal(nd.weights[first], one.weights[0])
    # neutral goes through the same field
    U = fc.universe_mask(p.styles, p.cap, p.ret, p.ind, p.P, sv)
    hb = torch.where(U, p.cap.double(), torch.zeros((), dtype=F64))
    hb = hb / hb.sum(-1, keepdim=True)
    rn = m.optimize(benchmark=hb, neutral="industries", upper=0.1, specific_vol=sv, prev=prev,
                    tcost=1e-4)
    assert (rn.status[-10:] == bq.OK).all() and rn.eta is not None
    assert torch.equal(rn.turnover[-10:], (rn.weights - prev).abs().sum(-1)[-10:])
    with pytest.raises(ValueError):
        m.optimize(prev=prev, **kw)
    with pytest.raises(ValueError):
        m.rebalance(**kw)


# ------------------------------------------------------------------------------------ GPU
TIERS = (1024, 3072, 5120)        # the resident tiers of tc_project_kernel: E = 4, 12, 20
PROJECT_N = [1, 63, 64, 65, 257, 1000, 5000] + [b + k for b in TIERS for k in (-1, 0, 1)]


@functools.lru_cache(maxsize=None)
def _tc_inputs(N, zero_cost):
    u, a, lo, hi, bud, q = _project_inputs(N)
    g = torch.Generator().manual_seed(99 + N)
    p = 0.5 * (lo + hi) + 0.3 * (hi - lo + 1e-3) * torch.randn(3, N, generator=g, dtype=F64)
    p[:, 2::13] = NAN
    p[:, 4::9] += 2.0                                   # outside the box
    kap = torch.zeros(3, N, dtype=F64) if zero_cost else \
        1e-5 * torch.rand(3, N, generator=g, dtype=F64)
    ref = tc.tc_project(u, a, lo, hi, bud, p, kap, q)
    return (u, a, lo, hi, bud, p, kap, q), ref


@pytest.mark.gpu
@pytest.mark.parametrize("zero_cost", [True, False], ids=["kappa0", "kappa"])
@pytest.mark.parametrize("N", PROJECT_N)
def test_hip_tc_project_matches_cpu(cuda, N, zero_cost):
    inp, ref = _tc_inputs(N, zero_cost)
    u, a, lo, hi, bud, p, kap, q = inp
    dev = tuple(t.to(cuda) for t in inp)
    got = tc.tc_project(*dev)
    streamed = tc.tc_project(*dev, stream_rows=True)
    for x, y in zip((*got.proj, got.cost), (*streamed.proj, streamed.cost)):
        assert torch.equal(x, y)                         # resident and streamed: the same bits
    assert torch.equal(got.proj.flag.cpu(), ref.proj.flag), (got.proj.flag, ref.proj.flag)
    if N >= 63:
        assert (ref.proj.flag == 0).all()
    box = bq.box_project(*dev[:5], dev[7]) if zero_cost else None
    eps = torch.finfo(F64).eps
    pz = torch.nan_to_num(p, nan=0.0)
    for d in range(3):
        if ref.proj.flag[d] != 0:
            continue
        h, hr, w = got.proj.h[d].cpu(), ref.proj.h[d], got.proj.w[d].cpu()
        bound = 16 * N * eps * (hr.abs().sum().item() + abs(bud[d].item()))
        err = (h - hr).abs().max().item()
        berr = abs(h.sum().item() - bud[d].item())
        print(f"N {N} date {d}: |h - h_cpu| {err:.2e}, budget error {berr:.2e}, bound "
              f"{bound:.2e}, untraded {int((h == pz[d]).sum())}")
        assert err <= bound and berr <= bound
        part = (a[d] > 0) & ~torch.isnan(hi[d])
        assert (h[~part] == 0).all() and (w[~part] == 0).all()
        l, up = lo[d][part], hi[d][part]
        assert ((h[part] >= l) & (h[part] <= up)).all()
        inside = (h > torch.nan_to_num(lo[d])) & (h < torch.nan_to_num(hi[d])) & (h != pz[d])
        assert (w[~inside] == 0).all() and torch.equal(w[w != 0], a[d][w != 0])
        if box is not None:
            assert (h - box.h[d].cpu()).abs().max().item() <= bound
        # sum h^2 / a, q' h - cost, sum |h|, cost: 1e-12 of the sums of their terms' magnitudes
        qa = (q[d].abs() * hr.abs())[part].sum().item()
        cr = ref.cost[d].item()
        st, sr = got.proj.stats[d].cpu(), ref.proj.stats[d]
        for k, mag in enumerate((sr[0].item(), qa + cr, sr[2].item())):
            assert abs(st[k].item() - sr[k].item()) <= 1e-12 * mag + bound, (k, st, sr)
        # kappa <= 1e-5, so the cost of the difference in h is far below `bound`
        assert abs(got.cost[d].item() - cr) <= 1e-12 * cr + bound
    if N >= 63:   # date 2: nothing is free
        assert (got.proj.w[2] == 0).all() and (got.proj.h[2].cpu()[a[2] > 0] == 2.0 ** -13).all()


@pytest.mark.gpu
def test_hip_tc_project_flags_and_kept_rows(cuda):
    inp, _ = _tc_inputs(257, False)
    u, a, lo, hi, bud, p, kap, q = (t.clone() for t in inp)
    n_on = int(torch.nonzero(a[0] > 0)[0])
    kap[0, n_on] = NAN                       # date 0: flag 2
    kap[1, n_on] = -1e-6                     # date 1: flag 2
    kap[2, 5] = NAN                          # off the universe (a = 0): ignored
    assert a[2, 5] == 0
    ref = tc.tc_project(u, a, lo, hi, bud, p, kap, q)
    got = tc.tc_project(*(t.to(cuda) for t in (u, a, lo, hi, bud, p, kap, q)))
    assert ref.proj.flag.tolist() == [2, 2, 0] == got.proj.flag.tolist()
    assert (got.proj.h[:2] == 0).all() and (got.cost[:2] == 0).all()     # rows kept (zeros)
    # a finished date keeps what `out` held
    status = torch.tensor([bq.RUNNING, bq.OK, bq.OK], dtype=torch.int32, device=cuda)
    out = tc.new_tc_projection(3, 257, cuda)
    out.proj.h.fill_(7.0)
    out.cost.fill_(7.0)
    tc.tc_project(*(t.to(cuda) for t in inp), None, status, out=out)
    assert (out.proj.h[1:] == 7.0).all() and (out.cost[1:] == 7.0).all()
    assert (out.proj.h[0] != 7.0).all() and out.cost[0] != 7.0


@pytest.mark.gpu
@pytest.mark.parametrize("scenario", ("cap", "long-short"))
@pytest.mark.parametrize("shape,dtype", E2E)
def test_hip_box_qp_with_costs_end_to_end(cuda, shape, dtype, scenario):
    c = _case(*shape, dtype=dtype)
    q, lo, hi = c.scenario(scenario)
    p = _prev(c, scenario)
    ref = _cpu(c, scenario, 2e-5)
    got = bq.box_qp(*c.on(cuda), c.F.to(cuda), c.s.to(cuda), None if q is None else q.to(cuda),
                    lo, hi, max_passes=64, prev=p.to(cuda), tcost=2e-5)
    assert (ref.status == bq.OK).all()
    _assert_matches_cpu(got, ref, scenario)
    for name in ("turnover", "cost"):
        a, b = getattr(got, name).cpu(), getattr(ref, name)
        assert ((a - b).abs() <= 1e-8 * b.abs().clamp(min=1e-300)).all(), (name, a, b)
    _check_kkt(c, got.weights.cpu(), q, lo, hi, p, 2e-5, what=f"GPU {scenario}")


@pytest.mark.gpu
def test_hip_box_qp_with_costs_reproducible_and_limits(cuda):
    c = _case(3, 1000, 31, 10, dtype=torch.float64)
    args = (*c.on(cuda), c.F.to(cuda), c.s.to(cuda))
    kw = dict(max_passes=64, prev=_prev(c, "cap").to(cuda), tcost=2e-5)
    r1 = bq.box_qp(*args, None, 0.0, 0.05, **kw)
    r2 = bq.box_qp(*args, None, 0.0, 0.05, **kw)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    r3 = bq.box_qp(*args, None, 0.0, 0.05, stream_rows=True, **kw)
    assert torch.equal(r3.weights, r1.weights)
    # tcost=None launches what it launched: the same bits as a plain call
    r0 = bq.box_qp(*args, None, 0.0, 0.05, prev=None, tcost=None)
    for a, b in zip(r0, bq.box_qp(*args, None, 0.0, 0.05)):
        assert torch.equal(a, b)
    # the K / Q limits are raised before any launch
    D, N, P, Q = 1, 16, 54, 10   # K = 65
    K = 1 + P + Q
    X = torch.zeros(D, Q, N, device=cuda)
    v = torch.zeros(D, N, device=cuda)
    ind = torch.zeros(D, N, dtype=torch.int16, device=cuda)
    st = torch.ones(D, Q + 2, dtype=F64, device=cuda)
    F = torch.eye(K, dtype=F64, device=cuda)[None]
    s = torch.ones(N, dtype=F64, device=cuda)
    with pytest.raises(ValueError, match="64"):
        bq.box_qp(X, v, v, ind, st, P, F, s, prev=0.0, tcost=1e-5)
    with pytest.raises(ValueError, match="64"):
        eq.exposure_qp(X, v, v, ind, st, P, F, s, [3], torch.zeros(1, dtype=F64, device=cuda),
                       prev=0.0, tcost=1e-5)
    X17 = torch.zeros(D, 17, N, device=cuda)   # Q = 17 > 16 styles
    with pytest.raises(ValueError, match="16"):
        bq.box_qp(X17, v, v, None, torch.ones(D, 19, dtype=F64, device=cuda), 0,
                  torch.eye(18, dtype=F64, device=cuda)[None], s, prev=0.0, tcost=1e-5)


@pytest.mark.gpu
def test_risk_model_optimize_with_costs_gpu_matches_cpu(cuda):
    """As ``test_box_qp.test_risk_model_optimize_gpu_matches_cpu``: the CPU model is given the
    GPU model's eigen and VRA covariances."""
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(80, 520, 31, 10, seed=5, missing_frac=0.03)
    cfg = preset("reference", eigen_sims=5)
    mc = RiskModel(p, cfg).run()
    mg = RiskModel(p.to(cuda), cfg).run()
    mc.eigen_cov, mc.vra_cov = mg.eigen_cov.cpu(), mg.vra_cov.cpu()
    svc, svg = mc.specific_risk_shrunk(), mg.specific_risk_shrunk()
    U = fc.universe_mask(p.styles, p.cap, p.ret, p.ind, p.P, svc)
    hb = torch.where(U, p.cap.double(), torch.zeros((), dtype=F64))
    hb = hb / hb.sum(-1, keepdim=True)
    prev = torch.nan_to_num(mc.optimize(upper=0.02, specific_vol=svc).weights).roll(1, 0)
    for neutral in (None, "industries"):
        kw = dict(upper=0.02, tcost=2e-5, max_passes=128)
        if neutral:
            kw.update(neutral=neutral)
        rc = mc.optimize(benchmark=hb if neutral else None, specific_vol=svc, prev=prev, **kw)
        rg = mg.optimize(benchmark=hb.to(cuda) if neutral else None, specific_vol=svg,
                         prev=prev.to(cuda), **kw)
        fin_c = torch.isfinite(rc.weights).all(-1)
        assert torch.equal(fin_c, torch.isfinite(rg.weights).all(-1).cpu()), neutral
        assert (rc.status[-10:] == bq.OK).all() and (rg.status[-10:] == bq.OK).all()
        both = (rc.status == bq.OK) & (rg.status.cpu() == bq.OK)
        w, wr = rg.weights.cpu()[both], rc.weights[both]
        err, scale = (w - wr).abs().amax(-1), wr.abs().amax(-1)
        print(f"neutral {neutral}: weights {(err / scale).max().item():.2e} on "
              f"{int(both.sum())}, passes {rg.passes.max().item()}")
        assert (err <= 1e-8 * scale).all()
        t, tr = rg.turnover.cpu()[both], rc.turnover[both]
        assert ((t - tr).abs() <= 1e-8 * tr.abs().clamp(min=1e-300)).all()
