"""Box-constrained portfolio optimisation (``ops.box_qp``, ``csrc/box_qp.hip``) and
``RiskModel.optimize``.

The algorithm-independent oracle is the KKT conditions against the dense ``Sigma_d`` of each
date (N_U x N_U, explicit design matrix): with r = Sigma h - q there is one gamma with
|r_n - gamma| <= eps on stocks strictly inside their bounds, r_n >= gamma - eps at the lower and
r_n <= gamma + eps at the upper bound, eps = 10 tol max|r| (the solver's own tol = 1e-10 with a
x10 margin); the box holds exactly and the budget to 1e-12 (sum|h| + |budget|).  The GPU tests
check the kernels against the CPU functions and the GPU's weights against the same KKT check.
"""
import functools
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
from llm_driven_multi_factor_model_amd.ops import box_qp as bq
from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
from llm_driven_multi_factor_model_amd.ops.cross_section import valid_mask, xs_wls

F64 = torch.float64
INF = float("inf")
TOL = 1e-10


class Case:
    """Seeded inputs as ``test_factor_cov.Case``: panel + stats, F = A^T A / (3K) with
    A = 0.01 randn(3K, K), s = 0.01 + 0.03 rand(N), alpha = 0.02 randn(D, N)."""

    def __init__(self, D, N, P, Q, dtype=torch.float32, seed=3, edge=False):
        p = synthetic_panel(D, N, P, Q, seed=seed, missing_frac=0.03, dtype=dtype)
        self.p, self.D, self.N, self.P, self.Q = p, D, N, P, Q
        self.K = K = 1 + P + Q
        self.stats = xs_wls(p.styles, p.cap, p.ret, p.ind, P).stats
        g = torch.Generator().manual_seed(1000 + seed)
        A = 0.01 * torch.randn(D, 3 * K, K, generator=g, dtype=F64)
        self.F = A.transpose(1, 2) @ A / (3 * K)
        self.s = 0.01 + 0.03 * torch.rand(N, generator=g, dtype=F64)
        self.alpha = 0.02 * torch.randn(D, N, generator=g, dtype=F64)
        self.universe = None
        if edge:
            w, U = torch.linalg.eigh(self.F[1])
            w[:5] = 0.0
            self.F[1] = (U * w) @ U.T                  # rank-deficient by 5
            self.F[2] = float("nan")                   # an invalid date
            self.s = self.s.clone()
            self.s[5::17] = float("nan")
            self.s[9::23] = 0.0
            self.universe = torch.ones(D, N, dtype=torch.bool)
            self.universe[:, ::3] = False

    @property
    def panel_args(self):
        p = self.p
        return p.styles, p.cap, p.ret, p.ind, self.stats, self.P

    def on(self, dev):
        p = self.p.to(dev)
        return p.styles, p.cap, p.ret, p.ind, self.stats.to(dev), self.P

    def scenario(self, name):
        """(q, lower, upper)."""
        return {"long-only": (None, 0.0, 1.0), "cap": (None, 0.0, 0.05),
                "vertex": (self.alpha / 5, 0.0, 0.05),
                "long-short": (self.alpha / 50, -0.01, 0.02)}[name]


SCENARIOS = ("long-only", "cap", "vertex", "long-short")


@functools.lru_cache(maxsize=None)
def _case(*a, **kw):
    return Case(*a, **dict(kw))


@functools.lru_cache(maxsize=None)
def _dense_sigma(c: Case):
    """Per date (index of the universe, dense Sigma on it), None for a non-finite F."""
    X = c.p.styles
    D, Q, N = X.shape
    m = valid_mask(X, c.p.cap, c.p.ret, c.p.ind, c.P) & torch.isfinite(c.s) & (c.s > 0)
    if c.universe is not None:
        m = m & c.universe
    mu, sig = c.stats[:, :Q].double(), c.stats[:, Q].double()
    Z = (X.double() - mu[:, :, None]) / sig[:, None, None]
    cols = [torch.ones(D, N, 1, dtype=F64)]
    if c.P > 0:
        cols.append(torch.nn.functional.one_hot(c.p.ind.long().clamp(0, c.P - 1), c.P).double())
    cols.append(Z.transpose(1, 2))
    Xd = torch.cat(cols, 2)
    out = []
    for d in range(D):
        if not torch.isfinite(c.F[d]).all():
            out.append(None)
            continue
        idx = torch.nonzero(m[d]).flatten()
        Xu = Xd[d, idx]
        out.append((idx, Xu @ c.F[d] @ Xu.T + torch.diag(c.s[idx] ** 2)))
    return out


def _full(t, D, N):
    return torch.as_tensor(0.0 if t is None else t, dtype=F64).expand(D, N)


def _check_kkt(c: Case, weights, q, lo, hi, budget=1.0, tol=TOL, dates=None, what=""):
    q, lo, hi = _full(q, c.D, c.N), _full(lo, c.D, c.N), _full(hi, c.D, c.N)
    for d, ds in enumerate(_dense_sigma(c)):
        if ds is None or (dates is not None and d not in dates):
            continue
        idx, Sig = ds
        h, l, u = weights[d, idx], lo[d, idx], hi[d, idx]
        out = torch.ones(c.N, dtype=torch.bool)
        out[idx] = False
        assert (weights[d, out] == 0).all(), f"{what} date {d}: weight outside the universe"
        assert ((h >= l) & (h <= u)).all(), f"{what} date {d}: box"
        berr = abs(h.sum().item() - budget)
        r = Sig @ h - q[d, idx]
        eps = 10 * tol * r.abs().max().item()
        free, atl, atu = (h > l) & (h < u), h <= l, h >= u
        g_lo = max([-INF] + [(r[k] - eps).max().item() for k in (free, atu) if k.any()])
        g_hi = min([INF] + [(r[k] + eps).min().item() for k in (free, atl) if k.any()])
        print(f"{what} date {d}: free {int(free.sum())}/{len(idx)}, KKT gap "
              f"{(g_lo - g_hi) / eps:.2e} eps, budget error {berr:.1e}")
        assert berr <= 1e-12 * (h.abs().sum().item() + abs(budget)), f"{what} date {d}: budget"
        assert g_lo <= g_hi, f"{what} date {d}: no gamma satisfies KKT ({g_lo} > {g_hi})"


# ------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("shape,dtype", [((4, 203, 5, 4), torch.float32),
                                         ((2, 77, 0, 3), torch.float64)])
def test_kkt_against_dense_sigma(shape, dtype, scenario):
    c = _case(*shape, dtype=dtype)
    q, lo, hi = c.scenario(scenario)
    r = bq.box_qp(*c.panel_args, c.F, c.s, q, lo, hi)
    print("passes", r.passes.tolist())
    assert (r.status == bq.OK).all() and (r.passes <= 32).all()
    _check_kkt(c, r.weights, q, lo, hi, what=scenario)
    # variance = h' Sigma h
    for d, (idx, Sig) in enumerate(_dense_sigma(c)):
        h = r.weights[d, idx]
        assert abs(r.variance[d].item() - (h @ Sig @ h).item()) <= 1e-12 * r.variance[d].item()


@pytest.mark.parametrize("shape,dtype", [((4, 203, 5, 4), torch.float32),
                                         ((2, 77, 0, 3), torch.float64)])
def test_unbounded_equals_min_variance(shape, dtype):
    c = _case(*shape, dtype=dtype)
    r = bq.box_qp(*c.panel_args, c.F, c.s, None, -INF, INF)
    y = fc.solve_cov(*c.panel_args, c.F, c.s, torch.ones(c.D, c.N, dtype=F64))
    w = y / y.sum(-1, keepdim=True)
    assert (r.status == bq.OK).all()
    err = (r.weights - w).abs().amax(-1)
    print("unbounded vs y / sum y:", (err / w.abs().amax(-1)).max().item(), r.passes.tolist())
    assert (err <= 1e-9 * w.abs().amax(-1)).all()
    var = 1.0 / y.sum(-1)
    assert ((r.variance - var).abs() <= 1e-9 * var).all()


def test_edge_cases():
    c = _case(4, 203, 5, 4, edge=True)
    r = bq.box_qp(*c.panel_args, c.F, c.s, None, 0.0, 1.0, universe=c.universe)
    assert r.status.tolist() == [bq.OK, bq.OK, bq.INVALID, bq.OK]
    assert torch.isnan(r.weights[2]).all() and torch.isnan(r.variance[2])
    assert torch.isfinite(r.weights[[0, 1, 3]]).all()
    _check_kkt(c, r.weights, None, 0.0, 1.0, what="edge")      # date 1 is rank-deficient
    ok = [0, 1, 3]
    assert (r.weights[ok][:, ::3] == 0).all() and (r.weights[ok][:, 5::17] == 0).all() \
        and (r.weights[ok][:, 9::23] == 0).all()
    # sum of the upper bounds below the budget: infeasible everywhere
    for cc, uni in ((c, c.universe), (_case(4, 203, 5, 4), None)):
        r = bq.box_qp(*cc.panel_args, cc.F, cc.s, None, 0.0, 1.0 / (2 * cc.N), universe=uni)
        assert (r.status == bq.INFEASIBLE).all() and torch.isnan(r.weights).all()
    # one stock with lo > hi: that date only
    c = _case(4, 203, 5, 4)
    idx0 = _dense_sigma(c)[1][0]
    lo = torch.zeros(c.D, c.N, dtype=F64)
    lo[1, idx0[3]] = 2.0
    r = bq.box_qp(*c.panel_args, c.F, c.s, None, lo, 1.0)
    assert r.status.tolist() == [bq.OK, bq.INFEASIBLE, bq.OK, bq.OK]
    assert torch.isnan(r.weights[1]).all()
    _check_kkt(c, r.weights, None, lo, 1.0, dates=(0, 2, 3), what="lo > hi elsewhere")
    # one pass: the first iterate, feasible
    r = bq.box_qp(*c.panel_args, c.F, c.s, None, 0.0, 1.0, max_passes=1)
    assert (r.status == bq.MAX_PASSES).all() and (r.passes == 1).all()
    w = r.weights
    assert torch.isfinite(w).all() and ((w >= 0) & (w <= 1)).all()
    assert ((w.sum(-1) - 1).abs() <= 1e-12 * (w.abs().sum(-1) + 1)).all()
    # a zero-date block
    p = c.p.slice_dates(0, 0)
    r = bq.box_qp(p.styles, p.cap, p.ret, p.ind, c.stats[:0], c.P, c.F[:0], c.s)
    assert r.weights.shape == (0, c.N) and r.status.shape == (0,)


def test_one_date_does_not_depend_on_the_others():
    c = _case(4, 203, 5, 4)
    q, lo, hi = c.scenario("long-short")
    r = bq.box_qp(*c.panel_args, c.F, c.s, q, lo, hi)
    p = c.p.slice_dates(2, 3)
    r1 = bq.box_qp(p.styles, p.cap, p.ret, p.ind, c.stats[2:3], c.P, c.F[2:3], c.s, q[2:3], lo, hi)
    assert torch.equal(r1.status, r.status[2:3]) and torch.equal(r1.passes, r.passes[2:3])
    torch.testing.assert_close(r1.weights, r.weights[2:3], rtol=0, atol=1e-15)


def _risk_model(device="cpu"):
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(60, 80, 4, 3, seed=5, missing_frac=0.02)
    return RiskModel(p.to(device), preset("reference", eigen_sims=5)).run()


def test_risk_model_optimize_cpu():
    m = _risk_model()
    p = m.panel
    sv = m.specific_risk_shrunk()
    U = fc.universe_mask(p.styles, p.cap, p.ret, p.ind, p.P, sv)
    hb = torch.where(U, p.cap.double(), torch.zeros((), dtype=F64))
    hb = hb / hb.sum(-1, keepdim=True)
    r = m.optimize(benchmark=hb, lower=0.0, upper=1.0)
    fin = r.status == bq.OK
    assert fin[-10:].all() and r.expected_return is None
    assert torch.equal(fin, torch.isfinite(r.weights).all(-1))
    err = (r.weights - hb).abs().amax(-1)[fin]
    print("benchmark recovered to", (err / hb.amax(-1)[fin]).max().item())
    assert (err <= 1e-9 * hb.amax(-1)[fin]).all()
    assert (r.active_variance[fin] <= 1e-16 * r.variance[fin]).all()
    # capped minimum variance passes KKT on every finite date (per-date specific volatilities)
    r = m.optimize(upper=0.05)
    assert (r.status[-10:] == bq.OK).all() and r.active_variance is None
    X = p.styles
    mu, sig = m.stats[:, :p.Q].double(), m.stats[:, p.Q].double()
    Z = ((X.double() - mu[:, :, None]) / sig[:, None, None]).transpose(1, 2)
    Xd = torch.cat([torch.ones(p.D, p.N, 1, dtype=F64),
                    torch.nn.functional.one_hot(p.ind.long().clamp(0, p.P - 1), p.P).double(),
                    Z], 2)
    checked = 0
    for d in range(p.D):
        if r.status[d] != bq.OK:
            continue
        idx = torch.nonzero(U[d]).flatten()
        Xu, h = Xd[d, idx], r.weights[d, idx]
        Sig = Xu @ m.vra_cov[d] @ Xu.T + torch.diag(sv[d, idx] ** 2)
        g = Sig @ h
        eps = 10 * TOL * g.abs().max().item()
        free, atl, atu = (h > 0) & (h < 0.05), h <= 0, h >= 0.05
        assert ((h >= 0) & (h <= 0.05)).all() and (r.weights[d][~U[d]] == 0).all()
        assert abs(h.sum().item() - 1) <= 1e-12 * (h.abs().sum().item() + 1)
        g_lo = max([-INF] + [(g[k] - eps).max().item() for k in (free, atu) if k.any()])
        g_hi = min([INF] + [(g[k] + eps).min().item() for k in (free, atl) if k.any()])
        assert g_lo <= g_hi, d
        checked += 1
    assert checked >= 10
    # a tilt reports its expected return
    alpha = torch.linspace(-0.01, 0.01, p.N, dtype=F64)
    r = m.optimize(alpha=alpha, risk_aversion=5.0, upper=0.05)
    ok = r.status == bq.OK
    torch.testing.assert_close(r.expected_return[ok], (r.weights[ok] * alpha).sum(-1))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dist_panel():
    return synthetic_panel(37, 64, 4, 3, seed=21, missing_frac=0.05)


def _dist_outputs(m):
    r = m.optimize(upper=0.1)
    return dict(weights=r.weights, variance=r.variance, passes=r.passes, status=r.status)


def _dist_worker(rank, world, port, path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.parallel import dist as pdist
    from llm_driven_multi_factor_model_amd.utils.config import preset
    ctx = pdist.init_distributed(device="cpu")
    full = _dist_panel()
    a, b = pdist.shard_range(full.D, ctx.rank, ctx.world)
    m = RiskModel(full.slice_dates(a, b), preset("reference", eigen_sims=5), T_global=full.D,
                  ctx=ctx).run()
    got = {k: pdist.gather_to_root(v.contiguous(), ctx) for k, v in _dist_outputs(m).items()}
    if ctx.rank == 0:
        torch.save(got, path)
    pdist.barrier(ctx)
    torch.distributed.destroy_process_group()


def test_optimize_rank_invariant():
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.utils.config import preset
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "bq.pt")
        mp.spawn(_dist_worker, args=(2, _free_port(), path), nprocs=2, join=True)
        got = torch.load(path, weights_only=True)
    ref = _dist_outputs(RiskModel(_dist_panel(), preset("reference", eigen_sims=5)).run())
    assert (ref["status"][-5:] == bq.OK).all()
    assert torch.equal(got["status"], ref["status"])
    for k in ("weights", "variance"):
        torch.testing.assert_close(got[k], ref[k], rtol=1e-12, atol=1e-15, equal_nan=True, msg=k)


# ------------------------------------------------------------------------------------ GPU
def _project_inputs(N, seed=11):
    """D = 3: long-only, long-short, and a date whose stocks all sit at a bound (lo = hi = 2^-13
    with budget N 2^-13, exact in every summation order)."""
    g = torch.Generator().manual_seed(seed + N)
    D = 3
    a = 1e2 + (1e4 - 1e2) * torch.rand(D, N, generator=g, dtype=F64)
    u = a * 1e-4 * torch.randn(D, N, generator=g, dtype=F64)
    lo = torch.zeros(D, N, dtype=F64)
    hi = torch.ones(D, N, dtype=F64)
    lo[1], hi[1] = -0.01, 0.02
    lo[2] = hi[2] = 2.0 ** -13
    bud = torch.tensor([1.0, 1.0, N * 2.0 ** -13], dtype=F64)
    if N >= 63:   # stocks outside the universe and a NaN bound
        a[:, 5::11] = 0.0
        hi[0, 7] = float("nan")
        bud[2] = float((a[2] > 0).sum()) * 2.0 ** -13
    q = 1e-4 * torch.randn(D, N, generator=g, dtype=F64)
    return u, a, lo, hi, bud, q


@pytest.mark.gpu
@pytest.mark.parametrize("stream_rows", [False, True], ids=["auto", "streamed"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000, 5000])
def test_hip_box_project_matches_cpu(cuda, N, stream_rows):
    u, a, lo, hi, bud, q = _project_inputs(N)
    ref = bq.box_project(u, a, lo, hi, bud, q)
    got = bq.box_project(*(t.to(cuda) for t in (u, a, lo, hi, bud, q)), stream_rows=stream_rows)
    assert torch.equal(got.flag.cpu(), ref.flag), (got.flag, ref.flag)
    if N >= 63:
        assert (ref.flag == 0).all()
    eps = torch.finfo(F64).eps
    for d in range(3):
        if ref.flag[d] != 0:
            continue
        h, hr = got.h[d].cpu(), ref.h[d]
        bound = 16 * N * eps * (hr.abs().sum().item() + abs(bud[d].item()))
        err = (h - hr).abs().max().item()
        berr = abs(h.sum().item() - bud[d].item())
        print(f"N {N} date {d}: |h - h_cpu| {err:.2e}, budget error {berr:.2e}, bound {bound:.2e}")
        assert err <= bound and berr <= bound
        assert ((h >= torch.nan_to_num(lo[d], nan=0.0)) | (a[d] <= 0)).all()
        assert (h[(a[d] <= 0) | torch.isnan(hi[d])] == 0).all()
        # sum h^2 / a, q' h, sum |h|: 1e-12 of the sums of their terms' magnitudes
        part = a[d] > 0
        qa = (q[d].abs() * hr.abs())[part].sum().item()
        st, sr = got.stats[d].cpu(), ref.stats[d]
        for k, mag in enumerate((sr[0].item(), qa, sr[2].item())):
            assert abs(st[k].item() - sr[k].item()) <= 1e-12 * mag + bound, (k, st, sr)
    if N >= 63:   # date 2: nothing is free
        assert (got.w[2] == 0).all() and (got.h[2].cpu()[a[2] > 0] == 2.0 ** -13).all()


def _drive(c, scenario, cuda, universe=None, lo_override=None, passes=8):
    """Run the CPU path pass by pass; at every pass run the CPU and the HIP step on the same
    inputs and compare."""
    q, lo, hi = c.scenario(scenario)
    if lo_override is not None:
        lo = lo_override
    pb = bq.make_problem(*c.panel_args, c.F, c.s, q, lo, hi, universe=universe)
    st, pj = bq.new_state(c.D, c.K, "cpu"), bq.new_projection(c.D, c.N, "cpu")
    lam, U = pb.lam.to(cuda), pb.U.to(cuda)
    seen = set()
    for it in range(passes):
        G, x = bq.run_trial(pb, st, pj)
        sg = st.clone().to(cuda)
        bq.box_step(G.to(cuda), lam, U, x.to(cuda), pj.stats.to(cuda), pj.flag.to(cuda), sg, TOL)
        bq.box_step(G, pb.lam, pb.U, x, pj.stats, pj.flag, st, TOL)
        sg = sg.to("cpu")
        assert torch.equal(sg.status, st.status), (it, sg.status, st.status)
        assert torch.equal(sg.accepted, st.accepted), (it, sg.accepted, st.accepted)
        assert torch.equal(sg.passes, st.passes)
        for name in ("c", "nu"):
            a, b = getattr(sg, name), getattr(st, name)
            live = (st.status == bq.RUNNING) | (st.status == bq.OK)
            err = (a - b).abs().amax(-1)[live]
            scale = b.abs().amax(-1)[live]
            print(f"pass {it} {name}: {(err / scale.clamp(min=1e-300)).max().item():.2e}")
            assert (err <= 1e-9 * scale).all(), (it, name)
        rows = st.status <= bq.OK          # running or converged: phi, step, variance
        a, b = sg.ds[rows, :3], st.ds[rows, :3]
        assert ((a - b).abs() <= 1e-9 * b.abs()).all(), (it, a, b)
        seen.update(zip(st.accepted.tolist(), st.status.tolist()))
        if not (st.status == bq.RUNNING).any():
            break
    return seen


@pytest.mark.gpu
def test_hip_box_step_matches_cpu(cuda):
    c = _case(3, 1000, 31, 10, dtype=torch.float64)
    seen = _drive(c, "long-short", cuda, passes=16)
    assert (1, bq.OK) in seen and (1, bq.RUNNING) in seen
    e = _case(4, 203, 5, 4, edge=True)
    lo = torch.zeros(e.D, e.N, dtype=F64)
    lo[0, _dense_sigma(e)[0][0][3]] = 2.0        # date 0 infeasible, date 2 invalid
    seen = _drive(e, "cap", cuda, universe=e.universe, lo_override=lo)
    assert {s for _, s in seen} >= {bq.OK, bq.INFEASIBLE, bq.INVALID}
    _drive(_case(2, 300, 53, 10), "vertex", cuda)   # K = 64


E2E = [
    pytest.param((4, 203, 5, 4), torch.float32, id="baseline"),
    pytest.param((3, 1000, 31, 10), torch.float64, id="k42-f64"),
    pytest.param((2, 257, 0, 16), torch.float32, id="q16-gram-split"),
    pytest.param((2, 300, 53, 10), torch.float32, id="k64"),
]


def _assert_matches_cpu(got, ref, what):
    assert torch.equal(got.status.cpu(), ref.status), (what, got.status, ref.status)
    ok = ref.status <= bq.MAX_PASSES
    assert torch.isnan(got.weights.cpu()[~ok]).all()
    err = (got.weights.cpu() - ref.weights)[ok].abs().amax(-1)
    scale = ref.weights[ok].abs().amax(-1)
    print(f"{what}: GPU vs CPU weights {(err / scale).max().item():.2e}, passes "
          f"{got.passes.tolist()} / {ref.passes.tolist()}")
    assert (err <= 1e-8 * scale).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("shape,dtype", E2E)
def test_hip_box_qp_end_to_end(cuda, shape, dtype, scenario):
    c = _case(*shape, dtype=dtype)
    q, lo, hi = c.scenario(scenario)
    ref = bq.box_qp(*c.panel_args, c.F, c.s, q, lo, hi)
    got = bq.box_qp(*c.on(cuda), c.F.to(cuda), c.s.to(cuda), None if q is None else q.to(cuda),
                    lo, hi)
    assert (ref.status == bq.OK).all()
    _assert_matches_cpu(got, ref, scenario)
    _check_kkt(c, got.weights.cpu(), q, lo, hi, what=f"GPU {scenario}")
    v, vr = got.variance.cpu(), ref.variance
    assert ((v - vr).abs() <= 1e-8 * vr).all()


@pytest.mark.gpu
def test_hip_box_qp_edge_cases(cuda):
    c = _case(4, 203, 5, 4, edge=True)
    args = (*c.on(cuda), c.F.to(cuda), c.s.to(cuda))
    uni = c.universe.to(cuda)
    ref = bq.box_qp(*c.panel_args, c.F, c.s, None, 0.0, 1.0, universe=c.universe)
    got = bq.box_qp(*args, None, 0.0, 1.0, universe=uni)
    assert got.status.tolist() == [bq.OK, bq.OK, bq.INVALID, bq.OK]
    _assert_matches_cpu(got, ref, "edge")
    w = got.weights.cpu()
    _check_kkt(c, w, None, 0.0, 1.0, what="GPU edge")
    ok = [0, 1, 3]
    assert (w[ok][:, ::3] == 0).all() and (w[ok][:, 5::17] == 0).all() \
        and (w[ok][:, 9::23] == 0).all()
    got = bq.box_qp(*args, None, 0.0, 1.0 / (2 * c.N), universe=uni)
    assert (got.status == bq.INFEASIBLE).all() and torch.isnan(got.weights).all()
    lo = torch.zeros(c.D, c.N, dtype=F64)
    lo[1, _dense_sigma(c)[1][0][3]] = 2.0
    got = bq.box_qp(*args, None, lo.to(cuda), 1.0, universe=uni)
    assert got.status.tolist() == [bq.OK, bq.INFEASIBLE, bq.INVALID, bq.OK]
    got = bq.box_qp(*args, None, 0.0, 1.0, universe=uni, max_passes=1)
    assert got.status.tolist() == [bq.MAX_PASSES, bq.MAX_PASSES, bq.INVALID, bq.MAX_PASSES]
    w = got.weights.cpu()[ok]
    assert torch.isfinite(w).all() and ((w >= 0) & (w <= 1)).all()
    assert ((w.sum(-1) - 1).abs() <= 1e-12 * (w.abs().sum(-1) + 1)).all()


@pytest.mark.gpu
def test_hip_box_qp_bitwise_reproducible(cuda):
    c = _case(3, 1000, 31, 10, dtype=torch.float64)
    args = (*c.on(cuda), c.F.to(cuda), c.s.to(cuda))
    r1 = bq.box_qp(*args, None, 0.0, 1.0)
    r2 = bq.box_qp(*args, None, 0.0, 1.0)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    r0 = bq.box_qp(*args, None, 0.0, 1.0, check_every=0)
    assert torch.equal(r0.weights, r1.weights) and torch.equal(r0.status, r1.status)
    # the register-resident and the re-streaming projection sum in the same order
    r3 = bq.box_qp(*args, None, 0.0, 1.0, stream_rows=True)
    assert torch.equal(r3.weights, r1.weights)


@pytest.mark.gpu
def test_hip_box_qp_limits_raise_before_launch(cuda):
    D, N, P, Q = 1, 16, 54, 10   # K = 65
    K = 1 + P + Q
    X = torch.zeros(D, Q, N, device=cuda)
    v = torch.zeros(D, N, device=cuda)
    ind = torch.zeros(D, N, dtype=torch.int16, device=cuda)
    st = torch.ones(D, Q + 2, dtype=F64, device=cuda)
    F = torch.eye(K, dtype=F64, device=cuda)[None]
    s = torch.ones(N, dtype=F64, device=cuda)
    with pytest.raises(ValueError, match="64"):
        bq.box_qp(X, v, v, ind, st, P, F, s)
    with pytest.raises(ValueError, match="64"):
        bq.box_step(F, F[:, 0], F, F[:, 0], None, None, None, TOL)
    X17 = torch.zeros(D, 17, N, device=cuda)   # Q = 17 > 16 styles
    with pytest.raises(ValueError, match="16"):
        bq.box_qp(X17, v, v, None, torch.ones(D, 19, dtype=F64, device=cuda), 0,
                  torch.eye(18, dtype=F64, device=cuda)[None], s)


@pytest.mark.gpu
def test_risk_model_optimize_gpu_matches_cpu(cuda):
    """As ``test_risk_model_gpu_matches_cpu``: the CPU model is given the GPU model's eigen and
    VRA covariances (the simulations draw from different generators on the two devices)."""
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(80, 520, 31, 10, seed=5, missing_frac=0.03)
    cfg = preset("reference", eigen_sims=5)
    mc = RiskModel(p, cfg).run()
    mg = RiskModel(p.to(cuda), cfg).run()
    mc.eigen_cov, mc.vra_cov = mg.eigen_cov.cpu(), mg.vra_cov.cpu()
    svc, svg = mc.specific_risk_shrunk(), mg.specific_risk_shrunk()
    for which in ("nw", "vra"):
        for upper in (1.0, 0.02):
            rc = mc.optimize(upper=upper, which=which, specific_vol=svc)
            rg = mg.optimize(upper=upper, which=which, specific_vol=svg)
            fin_c = torch.isfinite(rc.weights).all(-1)
            assert torch.equal(fin_c, torch.isfinite(rg.weights).all(-1).cpu()), which
            assert (rc.status[-10:] == bq.OK).all() and (rg.status[-10:] == bq.OK).all()
            w, wr = rg.weights.cpu()[fin_c], rc.weights[fin_c]
            err, scale = (w - wr).abs().amax(-1), wr.abs().amax(-1)
            print(f"{which} upper {upper}: weights {(err / scale).max().item():.2e}")
            assert (err <= 1e-8 * scale).all()
            v, vr = rg.variance.cpu()[fin_c], rc.variance[fin_c]
            assert ((v - vr).abs() <= 1e-8 * vr).all()
