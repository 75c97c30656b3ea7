"""Risk-budgeting portfolios (``ops.risk_budget``, ``csrc/risk_budget.hip``) and
``RiskModel.risk_budget``.

The algorithm-independent oracle is the definition itself against the dense ``Sigma_d`` of each
date (N_U x N_U, explicit design matrix): with RC_n = h_n (Sigma h)_n, the shares RC_n / sum RC
agree with b_n / sum b to 10 tol relative (the solver stops at ``rc_gap <= tol`` = 1e-9; x10
margin), sum h is the budget to 1e-12, h > 0 on U and exactly 0 off it, and ``variance`` is
h^T Sigma h to 1e-12 relative.  The GPU tests check each kernel against its CPU function to 1e-12
of each date's array's largest magnitude, and the GPU's weights against the same oracle.
"""
import functools

import pytest
import torch

from llm_driven_multi_factor_model_amd.ops import risk_budget as rb
from tests.test_box_qp import Case, _case, _dense_sigma, _risk_model   # noqa: F401

F64 = torch.float64
TOL = 1e-9
KINDS = ("equal", "spread")

# (D, N, P, Q), panel dtype, edge
CASES = [
    pytest.param((4, 203, 5, 4), torch.float32, False, id="baseline-f32"),
    pytest.param((2, 77, 0, 3), torch.float64, False, id="no-industries-f64"),
    pytest.param((3, 1000, 31, 10), torch.float64, False, id="k42-f64"),
    pytest.param((2, 300, 3, 13), torch.float64, False, id="q13-split-f64"),
    pytest.param((2, 37, 1, 1), torch.float32, False, id="sub-wave-q1-f32"),
    pytest.param((4, 203, 5, 4), torch.float32, True, id="edge-f32"),
]


def _budgets(c: Case, kind: str):
    """None (equal risk contribution) or 10^(4 rand), eight decades of budget ratios squared."""
    if kind == "equal":
        return None
    g = torch.Generator().manual_seed(4000 + c.N)
    return 10.0 ** (4.0 * torch.rand(c.D, c.N, generator=g, dtype=F64))


@functools.lru_cache(maxsize=None)
def _cpu(c: Case, kind: str):
    return rb.risk_budget(*c.panel_args, c.F, c.s, _budgets(c, kind), universe=c.universe)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise equal, NaN rows included."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) \
        and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _check_oracle(c: Case, res, b=None, budget=1.0, tol=TOL, dates=None, what=""):
    b = torch.ones(c.D, c.N, dtype=F64) if b is None else torch.as_tensor(
        b, dtype=F64).expand(c.D, c.N)
    w, var = res.weights.cpu(), res.variance.cpu()
    worst = 0.0
    for d, ds in enumerate(_dense_sigma(c)):
        if ds is None or (dates is not None and d not in dates):
            continue
        idx, Sig = ds
        keep = b[d, idx] > 0
        idx, Sig = idx[keep], Sig[keep][:, keep]
        h = w[d, idx]
        off = torch.ones(c.N, dtype=torch.bool)
        off[idx] = False
        assert (w[d, off] == 0).all(), f"{what} date {d}: weight outside U"
        assert (h > 0).all(), f"{what} date {d}: h > 0 on U"
        assert abs(h.sum().item() - budget) <= 1e-12 * budget, f"{what} date {d}: budget"
        rc = h * (Sig @ h)
        share, bs = rc / rc.sum(), b[d, idx] / b[d, idx].sum()
        gap = (share / bs - 1.0).abs().max().item()
        v = (h @ Sig @ h).item()
        verr = abs(var[d].item() - v) / v
        print(f"{what} date {d}: |U| {len(idx)}, RC share error {gap:.2e}, variance error "
              f"{verr:.1e}, rc_gap {res.rc_gap[d].item():.2e}, passes {int(res.passes[d])}")
        assert gap <= 10 * tol, f"{what} date {d}: risk contributions"
        assert verr <= 1e-12, f"{what} date {d}: variance"
        worst = max(worst, gap)
    return worst


def _valid(c: Case):
    return [d for d, ds in enumerate(_dense_sigma(c)) if ds is not None]


# ------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,dtype,edge", CASES)
def test_oracle_against_dense_sigma(shape, dtype, edge, kind):
    c = _case(*shape, dtype=dtype, edge=edge)
    r = _cpu(c, kind)
    ok = _valid(c)
    print("passes", r.passes.tolist(), "rejected", r.rejected.tolist())
    assert (r.status[ok] == rb.OK).all() and (r.passes[ok] <= 16).all()
    assert (r.rc_gap[ok] <= TOL).all()
    _check_oracle(c, r, _budgets(c, kind), what=kind)
    for d in range(c.D):
        if d not in ok:   # the NaN-F date
            assert r.status[d] == rb.INVALID
            assert torch.isnan(r.weights[d]).all() and torch.isnan(r.variance[d]) \
                and torch.isnan(r.rc_gap[d])
    if edge:
        w = r.weights[ok]
        assert (w[:, ::3] == 0).all() and (w[:, 5::17] == 0).all() and (w[:, 9::23] == 0).all()


def test_scaling_invariance():
    c = _case(4, 203, 5, 4)
    b = _budgets(c, "spread")
    r = _cpu(c, "spread")
    top = r.weights.amax(-1, keepdim=True)
    r7 = rb.risk_budget(*c.panel_args, c.F, c.s, 7.0 * b)
    assert (r7.status == rb.OK).all()
    assert ((r7.weights - r.weights).abs() <= 1e-12 * top).all()
    r25 = rb.risk_budget(*c.panel_args, c.F, c.s, b, 2.5)
    assert (r25.status == rb.OK).all()
    assert ((r25.weights - 2.5 * r.weights).abs() <= 1e-12 * 2.5 * top).all()
    assert ((r25.variance - 6.25 * r.variance).abs() <= 1e-12 * 6.25 * r.variance).all()
    _check_oracle(c, r25, b, budget=2.5, what="budget 2.5")
    # a budget per date
    bud = torch.tensor([1.0, 2.5, 0.5, 1.0], dtype=F64)
    rd = rb.risk_budget(*c.panel_args, c.F, c.s, b, bud)
    assert ((rd.weights - bud[:, None] * r.weights).abs() <= 1e-12 * bud[:, None] * top).all()


def test_degenerate_dates():
    c = _case(4, 203, 5, 4)
    sig = _dense_sigma(c)
    # date 0: one stock; date 1: b = 0 on every third name; date 2: all zero; date 3: equal
    b = torch.ones(c.D, c.N, dtype=F64)
    one = int(sig[0][0][7])
    b[0] = 0.0
    b[0, one] = 3.0
    b[1, ::3] = 0.0
    b[2] = 0.0
    r = rb.risk_budget(*c.panel_args, c.F, c.s, b, 2.0)
    assert r.status.tolist() == [rb.OK, rb.OK, rb.INFEASIBLE, rb.OK]
    assert r.weights[0, one] == 2.0 and r.weights[0].sum() == 2.0
    assert torch.isnan(r.weights[2]).all() and torch.isnan(r.variance[2])
    assert (r.weights[1, ::3] == 0).all()
    _check_oracle(c, r, b, budget=2.0, dates=(0, 1, 3), what="zero budgets")
    # a NaN, an infinite or a negative budget entry on the universe: that date only
    for bad in (float("nan"), float("inf"), -1.0):
        b = torch.ones(c.D, c.N, dtype=F64)
        b[1, int(sig[1][0][3])] = bad
        r = rb.risk_budget(*c.panel_args, c.F, c.s, b)
        assert r.status.tolist() == [rb.OK, rb.INVALID, rb.OK, rb.OK], bad
        assert torch.isnan(r.weights[1]).all()
        assert _same(r.weights[[0, 2, 3]], _cpu(c, "equal").weights[[0, 2, 3]])
    # ... outside the universe it is ignored
    off = torch.ones(c.N, dtype=torch.bool)
    off[sig[1][0]] = False
    b = torch.ones(c.D, c.N, dtype=F64)
    b[1, torch.nonzero(off).flatten()[0]] = float("nan")
    r = rb.risk_budget(*c.panel_args, c.F, c.s, b)
    assert (r.status == rb.OK).all() and _same(r.weights, _cpu(c, "equal").weights)
    # the sum of the weights must be finite and > 0
    bud = torch.tensor([1.0, 0.0, float("nan"), -1.0], dtype=F64)
    r = rb.risk_budget(*c.panel_args, c.F, c.s, None, bud)
    assert r.status.tolist() == [rb.OK] + [rb.INFEASIBLE] * 3
    assert torch.isnan(r.weights[1:]).all() and torch.isfinite(r.weights[0]).all()
    # the NaN-F date
    e = _case(4, 203, 5, 4, edge=True)
    assert _cpu(e, "equal").status.tolist() == [rb.OK, rb.OK, rb.INVALID, rb.OK]
    # max_passes: the last accepted iterate, long-only and fully invested
    r = rb.risk_budget(*c.panel_args, c.F, c.s, max_passes=3)
    assert (r.status == rb.MAX_PASSES).all() and (r.passes == 3).all()
    assert torch.isfinite(r.weights).all() and (r.weights >= 0).all()
    assert ((r.weights.sum(-1) - 1).abs() <= 1e-12).all() and (r.rc_gap > TOL).all()
    # a zero-date block
    p = c.p.slice_dates(0, 0)
    r = rb.risk_budget(p.styles, p.cap, p.ret, p.ind, c.stats[:0], c.P, c.F[:0], c.s)
    assert r.weights.shape == (0, c.N) and r.status.shape == (0,)


@pytest.mark.parametrize("shape,kind,drop", [
    # two passes in, the third trial lowers phi by 0.92 and 0.87 on this shape: 1 forces it
    pytest.param((2, 37, 1, 1), "equal", 1.0, id="sub-wave-q1-drop-1"),
    # ... and by 8 to 13 on this one (phi is of the order of |U|), so the saved phi is put out
    # of every trial's reach
    pytest.param((4, 203, 5, 4), "spread", 1e6, id="baseline-spread-drop-1e6"),
])
def test_forced_rejection_takes_the_damped_step(shape, kind, drop):
    c = _case(*shape)
    b = _budgets(c, kind)
    pb = rb.make_problem(*c.panel_args, c.F, c.s, b)
    st = rb.new_state(pb)
    for _ in range(2):
        rb.run_pass(pb, st)
    assert (st.status == rb.RUNNING).all() and (st.passes == 2).all()
    y_saved = rb._pick(st.y, st.sel).clone()
    st.ds[:, 0] -= drop           # the next trial cannot reach this phi: it is rejected
    rb.run_pass(pb, st)
    assert (st.rejected == 1).all() and (st.mode == rb.DAMPED).all()
    assert torch.equal(rb._pick(st.y, st.sel), y_saved)     # the saved iterate stayed
    t = st.ds[:, 2]
    assert ((t > 0) & (t < 1)).all()
    for _ in range(20):
        if not (st.status == rb.RUNNING).any():
            break
        rb.run_pass(pb, st)
    r = rb.result(pb, st)
    print("passes", r.passes.tolist(), "against", _cpu(c, kind).passes.tolist())
    assert (r.status == rb.OK).all() and (r.rejected == 1).all()
    _check_oracle(c, r, b, what="forced rejection")


def test_risk_model_risk_budget_cpu():
    m = _risk_model()
    p = m.panel
    sv = m.specific_risk_shrunk()
    r = m.risk_budget()
    ref = rb.risk_budget(p.styles, p.cap, p.ret, p.ind, m.stats, p.P, m.vra_cov, sv)
    for a, b in zip(r, ref):
        assert _same(a, b)
    assert (r.status[-10:] == rb.OK).all() and (r.status <= rb.MAX_PASSES).sum() >= 10
    assert torch.equal(r.status <= rb.MAX_PASSES, torch.isfinite(r.weights).all(-1))
    # dates = (a, b): rows a .. b-1 of the full call, bit for bit
    for a0 in (1, p.D - 3):
        r1 = m.risk_budget(dates=(a0, a0 + 1))
        assert r1.weights.shape == (1, p.N)
        for a, b in zip(r1, r):
            assert _same(a, b[a0:a0 + 1]), a0
    # budgets [D, N] and a named specific volatility are cut and passed on
    g = torch.Generator().manual_seed(9)
    b = 10.0 ** torch.rand(p.D, p.N, generator=g, dtype=F64)
    r2 = m.risk_budget(b, 2.0, which="nw", specific_vol=sv, tol=1e-8)
    ref = rb.risk_budget(p.styles, p.cap, p.ret, p.ind, m.stats, p.P, m.nw_cov, sv, b, 2.0,
                         tol=1e-8)
    assert _same(r2.weights, ref.weights) and torch.equal(r2.status, ref.status)
    r3 = m.risk_budget(b, 2.0, which="nw", specific_vol=sv, tol=1e-8, dates=(p.D - 2, p.D))
    assert _same(r3.weights, r2.weights[-2:])


# ------------------------------------------------------------------------------------ GPU
def _close(got, ref, rows, what, scalars=False):
    """1e-12 of each date's array's largest magnitude (``scalars``: of each entry's own)."""
    got, ref = got.cpu(), ref.cpu()
    for d in rows:
        err = (got[d] - ref[d]).abs()
        mag = ref[d].abs() if scalars else ref[d].abs().max()
        rel = (err / mag.clamp(min=1e-300)).max().item() if err.numel() else 0.0
        print(f"{what} date {d}: {rel:.2e}")
        assert (err <= 1e-12 * mag).all(), (what, d, rel)


def _gpu_problem(c: Case, pb: rb.Problem, cuda) -> rb.Problem:
    """The CPU problem's arrays on the device (the same eigenpairs), without the dense X."""
    return rb.Problem(c.on(cuda), *(t.to(cuda) for t in pb[1:-1]), None)


INTS = ("sel", "mode", "passes", "rejected", "status")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape,_dt,edge", CASES)
def test_hip_kernels_match_cpu(cuda, shape, _dt, edge, dtype):
    """Each kernel against its CPU function on the same inputs, two passes in, once with the
    accepted (clamped) and once with a rejected (damped) trial; the last date is finished."""
    c = _case(*shape, dtype=dtype, edge=edge)
    b = _budgets(c, "spread")
    pb = rb.make_problem(*c.panel_args, c.F, c.s, b, universe=c.universe)
    base = rb.new_state(pb)
    for _ in range(2):
        rb.run_pass(pb, base)
    base.status[c.D - 1] = rb.OK
    run = [d for d in range(c.D) if base.status[d] == rb.RUNNING]
    idle = [d for d in range(c.D) if d not in run]
    assert run and idle
    pg = _gpu_problem(c, pb, cuda)
    for damped in (False, True):
        s0 = base.clone()
        if damped:
            s0.ds[:, 0] -= 1e6      # out of every trial's reach: the trial is rejected
        tag = "damped" if damped else "clamped"
        # moments at the trial
        mc, mg = rb.rb_moments(pb, s0), rb.rb_moments(pg, s0.to(cuda))
        _close(mg.G, mc.G, run, f"{tag} G")
        _close(mg.v, mc.v, run, f"{tag} v")
        _close(mg.sc, mc.sc, run, f"{tag} (sigma, r, phi, ySy)", scalars=True)
        for t in mg:
            assert (t.cpu()[idle] == 0).all()
        # the step, on the CPU's moments
        sc, sg = s0.clone(), s0.to(cuda)
        rb.rb_step(mc, pb.lam, pb.U, pb.M, sc, TOL)
        rb.rb_step(mc.to(cuda), pg.lam, pg.U, pg.M, sg, TOL)
        for name in INTS:
            assert torch.equal(getattr(sg, name).cpu(), getattr(sc, name)), (tag, name)
        assert (sc.mode[run] == (rb.DAMPED if damped else rb.CLAMPED)).all()
        assert (sc.rejected[run] == int(damped)).all() and (sc.passes[run] == 3).all()
        _close(sg.c, sc.c, run, f"{tag} c")
        _close(sg.ds, sc.ds, run, f"{tag} ds", scalars=True)
        # the next trial, from the CPU's state
        uc, ug = sc.clone(), sc.to(cuda)
        rb.rb_update(pb, uc)
        rb.rb_update(pg, ug)
        yt, xt = rb._pick(uc.y, 1 - uc.sel), rb._pick(uc.x, 1 - uc.sel)
        _close(rb._pick(ug.y, 1 - ug.sel), yt, run, f"{tag} trial y")
        _close(rb._pick(ug.x, 1 - ug.sel), xt, run, f"{tag} trial x")
        assert torch.equal(rb._pick(ug.y, ug.sel).cpu(), rb._pick(sc.y, sc.sel))   # saved: kept
        assert torch.equal((rb._pick(ug.y, 1 - ug.sel) == 0).cpu(), yt == 0)
        # the finished and the invalid dates: nothing moved
        for got in (sg, ug):
            for a, bb in zip(got, s0):
                a = a.cpu()
                a = a[:, idle] if a.shape[0] == 2 and a.dim() == 3 else a[idle]
                bb = bb[:, idle] if bb.shape[0] == 2 and bb.dim() == 3 else bb[idle]
                assert torch.equal(a, bb)


def _gpu(c: Case, kind: str, cuda, **kw):
    b = _budgets(c, kind)
    uni = None if c.universe is None else c.universe.to(cuda)
    return rb.risk_budget(*c.on(cuda), c.F.to(cuda), c.s.to(cuda),
                          None if b is None else b.to(cuda), universe=uni, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,dtype,edge", CASES)
def test_hip_risk_budget_end_to_end(cuda, shape, dtype, edge, kind):
    """Statuses as the CPU's, the oracle on the GPU's own weights, and the CPU's weights.  The
    worst GPU-to-CPU difference measured on these twelve cases on an MI355X is 1.69e-15 of a
    date's largest weight (k42-f64, spread budgets; every case is below 2e-15 and takes the
    CPU's number of passes); the bound is ten times that, far inside the 1e-7 ceiling."""
    c = _case(*shape, dtype=dtype, edge=edge)
    ref, got = _cpu(c, kind), _gpu(c, kind, cuda)
    assert torch.equal(got.status.cpu(), ref.status)
    ok = _valid(c)
    assert (got.status.cpu()[ok] == rb.OK).all() and (got.passes.cpu()[ok] <= 16).all()
    dead = [d for d in range(c.D) if d not in ok]
    assert torch.isnan(got.weights.cpu()[dead]).all()
    _check_oracle(c, got, _budgets(c, kind), what=f"GPU {kind}")
    w, wr = got.weights.cpu()[ok], ref.weights[ok]
    rel = ((w - wr).abs().amax(-1) / wr.amax(-1)).max().item()
    print(f"GPU vs CPU weights {rel:.2e} of the largest weight, passes "
          f"{got.passes.tolist()} / {ref.passes.tolist()}")
    assert rel <= 1.7e-14


@pytest.mark.gpu
def test_hip_risk_budget_bitwise(cuda):
    c = _case(3, 1000, 31, 10, dtype=torch.float64)
    r1, r2 = _gpu(c, "spread", cuda), _gpu(c, "spread", cuda)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    r0 = _gpu(c, "spread", cuda, check_every=0, max_passes=12)
    assert torch.equal(r0.weights, r1.weights) and torch.equal(r0.status, r1.status)
    # a date solved alone equals its row in the batch
    for cc in (c, _case(2, 300, 3, 13, dtype=torch.float64)):
        full = _gpu(cc, "spread", cuda)
        d = cc.D - 1
        p = cc.p.slice_dates(d, d + 1).to(cuda)
        b = _budgets(cc, "spread")[d:d + 1].to(cuda)
        alone = rb.risk_budget(p.styles, p.cap, p.ret, p.ind, cc.stats[d:d + 1].to(cuda), cc.P,
                               cc.F[d:d + 1].to(cuda), cc.s.to(cuda), b)
        for a, bb in zip(alone, full):
            assert torch.equal(a, bb[d:d + 1])


@pytest.mark.gpu
def test_hip_risk_budget_limits_raise_before_launch(cuda):
    D, N, P, Q = 1, 16, 54, 10   # K = 65
    K = 1 + P + Q
    X = torch.zeros(D, Q, N, device=cuda)
    v = torch.zeros(D, N, device=cuda)
    ind = torch.zeros(D, N, dtype=torch.int16, device=cuda)
    st = torch.ones(D, Q + 2, dtype=F64, device=cuda)
    F = torch.eye(K, dtype=F64, device=cuda)[None]
    s = torch.ones(N, dtype=F64, device=cuda)
    with pytest.raises(ValueError, match="64"):
        rb.risk_budget(X, v, v, ind, st, P, F, s)
    mo = rb.new_moments(D, K, cuda)
    with pytest.raises(ValueError, match="64"):
        rb.rb_step(mo, F[:, 0], F, F[:, 0, 0], None, TOL)
    X17 = torch.zeros(D, 17, N, device=cuda)   # Q = 17 > 16 styles
    with pytest.raises(ValueError, match="16"):
        rb.risk_budget(X17, v, v, None, torch.ones(D, 19, dtype=F64, device=cuda), 0,
                       torch.eye(18, dtype=F64, device=cuda)[None], s)


@pytest.mark.gpu
def test_risk_model_risk_budget_gpu_matches_cpu(cuda):
    """As ``test_risk_model_optimize_gpu_matches_cpu``: the CPU model is given the GPU model's
    eigen and VRA covariances, and the two are held to the bound of that test, 1e-8 of a date's
    largest weight (the specific volatilities of the two devices differ in their last bits)."""
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(80, 520, 31, 10, seed=5, missing_frac=0.03)
    cfg = preset("reference", eigen_sims=5)
    mc = RiskModel(p, cfg).run()
    mg = RiskModel(p.to(cuda), cfg).run()
    mc.eigen_cov, mc.vra_cov = mg.eigen_cov.cpu(), mg.vra_cov.cpu()
    svc, svg = mc.specific_risk_shrunk(), mg.specific_risk_shrunk()
    g = torch.Generator().manual_seed(2)
    b = 10.0 ** (2.0 * torch.rand(p.N, generator=g, dtype=F64))
    for which, bud in (("nw", None), ("vra", b)):
        rc = mc.risk_budget(bud, which=which, specific_vol=svc)
        rg = mg.risk_budget(None if bud is None else bud.to(cuda), which=which, specific_vol=svg)
        assert torch.equal(rc.status, rg.status.cpu()), which
        fin = rc.status == rb.OK
        assert fin[-10:].all()
        assert torch.equal(fin, torch.isfinite(rg.weights).all(-1).cpu())
        w, wr = rg.weights.cpu()[fin], rc.weights[fin]
        err, scale = (w - wr).abs().amax(-1), wr.amax(-1)
        print(f"{which}: weights {(err / scale).max().item():.2e}")
        assert (err <= 1e-8 * scale).all()
        v, vr = rg.variance.cpu()[fin], rc.variance[fin]
        assert ((v - vr).abs() <= 1e-8 * vr).all()
