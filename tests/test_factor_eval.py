"""Factor evaluation (ops/factor_eval.py, csrc/factor_eval.hip): average ranks, IC, rank IC and
quantile-bucket returns.

CPU: the float64 torch path against scipy (``rankdata``, ``spearmanr``), numpy (``corrcoef``)
and pandas (``qcut``, groupby mean); ``forward_returns`` against a per-stock Python loop,
``ic_summary`` against numpy, the CLI files against the method.

GPU: the kernels against the CPU path on the same inputs at the wave and block edges of N
(NP = N and NP = 2N), N = 5000 and the limit 8192.  Bounds: ``n``, ``q_count`` and ``xs_rank``
exact; ``rank_ic`` 1e-14 absolute (the rank sums are exact in fp64, three roundings remain: the
product, the square root, the division); ``ic`` 1e-11 absolute (N eps = 1e-12 at N = 8192 for a
reordered sum of deviations, times 10); ``q_ret`` 1e-12 relative + 1e-15 absolute.
"""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.stats as ss
import torch

from llm_driven_multi_factor_model_amd.ops import factor_eval as fe

F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pairs(x, y, u, d, s, h):
    m = (u[d] & torch.isfinite(x[d, s]) & torch.isfinite(y[d, h])).numpy()
    return x[d, s].double().numpy()[m], y[d, h].numpy()[m], m


# ------------------------------------------------------------------ CPU: ranks
def _rank_rows():
    g = _gen(1)
    N = 257
    x = torch.randn(1, 5, N, generator=g, dtype=F64)
    x[0, 1] = torch.round(x[0, 1]).clamp(-2, 2)              # 5 levels
    x[0, 2] = 0.75                                           # all equal
    x[0, 3, ::2] = 0.0
    x[0, 3, 1::4] = -0.0                                     # -0.0 next to +0.0
    x[0, 4, 3] = float("nan")
    x[0, 4, 5] = float("inf")
    x[0, 4, 7] = float("-inf")
    u = torch.ones(1, N, dtype=torch.bool)
    u[0, 11::13] = False
    return x, u


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_xs_rank_equals_scipy_rankdata(dtype):
    x, u = _rank_rows()
    x = x.to(dtype)
    r = fe.xs_rank(x, u)
    assert r.dtype == F64 and r.shape == x.shape
    for s in range(x.shape[1]):
        m = (u[0] & torch.isfinite(x[0, s])).numpy()
        want = ss.rankdata(x[0, s].double().numpy()[m], method="average")
        assert np.array_equal(r[0, s].numpy()[m], want), s
        assert np.isnan(r[0, s].numpy()[~m]).all(), s
    assert (r[0, 2][u[0]] == (u[0].sum() + 1) / 2).all()          # the all-equal row
    z = r[0, 3][u[0] & (x[0, 3] == 0)]
    assert (z == z[0]).all()                                      # -0.0 ties with +0.0


# ------------------------------------------------------------------ CPU: correlations
@pytest.mark.parametrize("N", [2, 3, 50, 1000, 8192])
def test_ic_and_rank_ic_equal_numpy_and_scipy(N):
    g = _gen(N)
    D, S, H = 2, 3, 2
    x = torch.randn(D, S, N, generator=g, dtype=F64)
    y = torch.randn(D, H, N, generator=g, dtype=F64) + 0.3 * x[:, :H]
    x[:, 1] = torch.round(x[:, 1]).clamp(-2, 2)                   # tied signal
    y[1, 1] = torch.round(y[1, 1] * 2)                            # tied target
    u = torch.rand(D, N, generator=g) < 0.9
    if N > 10:
        x[0, 0, 1] = float("nan")
        y[0, 0, 2] = float("inf")
    r = fe.factor_ic(x, y, u)
    assert r.q_ret.shape == (D, S, H, 0) and r.q_count.shape == (D, S, H, 0)
    for d in range(D):
        for s in range(S):
            for h in range(H):
                xv, yv, m = _pairs(x, y, u, d, s, h)
                assert int(r.n[d, s, h]) == m.sum()
                if m.sum() < 2 or np.ptp(xv) == 0 or np.ptp(yv) == 0:
                    assert torch.isnan(r.ic[d, s, h]) and torch.isnan(r.rank_ic[d, s, h])
                    continue
                assert abs(float(r.ic[d, s, h]) - np.corrcoef(xv, yv)[0, 1]) <= 1e-12
                assert abs(float(r.rank_ic[d, s, h]) - ss.spearmanr(xv, yv)[0]) <= 1e-12


def test_degenerate_pair_sets_give_nan():
    x = torch.tensor([[[1.0, 2.0, 3.0, 4.0], [2.0, 2.0, 2.0, 2.0]]], dtype=F64)
    y = torch.tensor([[[0.1, 0.3, 0.2, 0.4], [float("nan")] * 3 + [1.0]]], dtype=F64)
    u = torch.ones(1, 4, dtype=torch.bool)
    r = fe.factor_ic(x, y, u, quantiles=2)
    assert r.n.tolist() == [[[4, 1], [4, 1]]]
    assert torch.isfinite(r.ic[0, 0, 0]) and torch.isfinite(r.rank_ic[0, 0, 0])
    assert torch.isnan(r.ic[0, 0, 1]) and torch.isnan(r.rank_ic[0, 0, 1])      # n = 1
    assert torch.isnan(r.ic[0, 1, 0]) and torch.isnan(r.rank_ic[0, 1, 0])      # zero variance
    assert r.q_count[0, 0, 1].tolist() == [1, 0] and r.q_count[0, 1, 0].tolist() == [4, 0]
    e = fe.factor_ic(x, y, torch.zeros(1, 4, dtype=torch.bool), quantiles=2)
    assert (e.n == 0).all() and torch.isnan(e.ic).all() and torch.isnan(e.q_ret).all()
    assert (e.q_count == 0).all()


# ------------------------------------------------------------------ CPU: buckets
@pytest.mark.parametrize("N", [7, 10, 64, 5000])
@pytest.mark.parametrize("G", [1, 2, 5, 10])
def test_buckets_equal_pandas_qcut(N, G):
    g = _gen(100 * N + G)
    x = torch.randn(1, 1, N, generator=g, dtype=F64)
    idx = torch.arange(N, dtype=F64)
    # positive targets: the condition number of a bucket mean is 1, so a relative bound on it
    # is a bound on the summation (a zero-mean target would measure its cancellation instead)
    y = torch.stack([0.5 + torch.rand(N, generator=g, dtype=F64), idx, idx * idx])[None]
    u = torch.ones(1, N, dtype=torch.bool)
    if N > 7:
        u[0, 3] = False
        x[0, 0, 5] = float("nan")
    r = fe.factor_ic(x, y, u, quantiles=G)
    for h in range(3):   # the means of i and i^2 pin the membership, not only the size
        xv, yv, m = _pairs(x, y, u, 0, 0, h)
        codes = pd.qcut(xv, G, labels=False)
        by = pd.Series(yv).groupby(codes)
        assert r.q_count[0, 0, h].tolist() == by.size().reindex(range(G), fill_value=0).tolist()
        np.testing.assert_allclose(r.q_ret[0, 0, h].numpy(), by.mean().reindex(range(G)).values,
                                   rtol=1e-14, atol=0)


def test_more_buckets_than_stocks_and_ties():
    x = torch.tensor([[[3.0, 1.0, 2.0], [1.0, 1.0, 2.0]]], dtype=F64)
    y = torch.tensor([[[10.0, 20.0, 40.0]]], dtype=F64)
    r = fe.factor_ic(x, y, torch.ones(1, 3, dtype=torch.bool), quantiles=10)
    for s in range(2):
        xv = x[0, s].numpy()
        edges = np.quantile(xv, np.linspace(0, 1, 11))[1:-1]
        grp = (xv[:, None] > edges[None, :]).sum(1)
        cnt = np.bincount(grp, minlength=10)
        assert r.q_count[0, s, 0].tolist() == cnt.tolist()
        for k in range(10):
            if cnt[k] == 0:
                assert torch.isnan(r.q_ret[0, s, 0, k])
            else:
                assert float(r.q_ret[0, s, 0, k]) == y[0, 0].numpy()[grp == k].mean()
    assert (r.q_count[0, 0, 0] == 0).sum() == 7
    assert r.q_count[0, 1, 0, 0] == 2           # the tied pair shares a group


def test_paired_is_the_diagonal_cpu():
    g = _gen(5)
    x = torch.randn(3, 4, 40, generator=g, dtype=F64)
    y = torch.randn(3, 4, 40, generator=g, dtype=F64)
    y[1, 2, ::3] = float("nan")
    u = torch.rand(3, 40, generator=g) < 0.8
    f, p = fe.factor_ic(x, y, u, 3), fe.factor_ic(x, y, u, 3, paired=True)
    for a, b in zip(f[:3], p[:3]):
        assert _same(torch.diagonal(a, dim1=1, dim2=2).contiguous(), b)
    assert torch.equal(torch.diagonal(f.q_count, dim1=1, dim2=2).permute(0, 2, 1), p.q_count)
    with pytest.raises(ValueError):
        fe.factor_ic(x, y[:, :3], u, paired=True)


# ------------------------------------------------------------------ CPU: targets and summary
def test_forward_returns_against_a_python_loop():
    g = _gen(9)
    D, N, hz = 11, 6, (1, 2, 5)
    ret = 0.05 * torch.randn(D, N, generator=g, dtype=F64)
    ret[4, 2] = float("nan")
    ret[7, 3] = float("inf")
    tail = 0.05 * torch.randn(4, N, generator=g, dtype=F64)
    tail[1, 0] = float("nan")
    for tl in (None, tail):
        got = fe.forward_returns(ret, hz, tl)
        assert got.shape == (D, 3, N) and got.dtype == F64
        ext = torch.cat([ret, tl if tl is not None else torch.full((4, N), float("nan"),
                                                                   dtype=F64)]).tolist()
        for d in range(D):
            for j, h in enumerate(hz):
                for n in range(N):
                    terms = [ext[d + k][n] for k in range(h)]
                    if not all(np.isfinite(t) for t in terms):
                        assert torch.isnan(got[d, j, n]), (d, h, n)
                        continue
                    acc = 1.0 + terms[0]
                    for t in terms[1:]:
                        acc = acc * (1.0 + t)
                    assert float(got[d, j, n]) == acc - 1.0, (d, h, n)
    nt = fe.forward_returns(ret, hz)
    assert torch.isnan(nt[-4:, 2]).all() and torch.isnan(nt[-1:, 1]).all()
    assert torch.isfinite(nt[-1, 0, 0])
    assert torch.isnan(nt[3, 1, 2]) and torch.isnan(nt[0, 2, 2]) and torch.isfinite(nt[5, 1, 2])
    with pytest.raises(ValueError):
        fe.forward_returns(ret, hz, tail[:2])


def test_ic_summary_against_numpy():
    g = _gen(3)
    v = torch.randn(30, 3, 2, generator=g, dtype=F64)
    v[5] = float("nan")
    v[11, 1, 0] = float("nan")
    v[:, 2, 1] = float("nan")
    v[:29, 2, 0] = float("nan")                    # one date: std NaN
    sm = fe.ic_summary(v, start=4)
    a = v.numpy()[4:]
    for s in range(3):
        for h in range(2):
            col = a[:, s, h]
            col = col[np.isfinite(col)]
            assert int(sm.n_dates[s, h]) == len(col)
            if len(col) == 0:
                assert torch.isnan(sm.mean[s, h]) and torch.isnan(sm.hit[s, h])
                continue
            np.testing.assert_allclose(float(sm.mean[s, h]), col.mean(), rtol=1e-13)
            np.testing.assert_allclose(float(sm.hit[s, h]), (col > 0).mean(), rtol=1e-15)
            if len(col) < 2:
                assert torch.isnan(sm.std[s, h]) and torch.isnan(sm.t[s, h])
                continue
            sd = col.std(ddof=1)
            np.testing.assert_allclose(float(sm.std[s, h]), sd, rtol=1e-13)
            np.testing.assert_allclose(float(sm.icir[s, h]), col.mean() / sd, rtol=1e-12)
            np.testing.assert_allclose(float(sm.t[s, h]), col.mean() / sd * np.sqrt(len(col)),
                                       rtol=1e-12)


# ------------------------------------------------------------------ CPU: model and CLI
def test_model_methods_cpu():
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    p = synthetic_panel(12, 80, P=5, Q=4, seed=2, missing_frac=0.05)
    m = RiskModel(p)
    ev = m.factor_ic(horizons=(1, 3), quantiles=5, start=2)
    y = fe.forward_returns(p.ret, (1, 3))
    want = fe.factor_ic(p.styles, y, p.valid(), 5)
    for k in ("n", "ic", "rank_ic", "q_ret", "q_count"):
        assert torch.allclose(getattr(ev, k), getattr(want, k), rtol=0, atol=0, equal_nan=True)
    assert torch.allclose(ev.spread, want.q_ret[..., -1] - want.q_ret[..., 0], rtol=0, atol=0,
                          equal_nan=True)
    assert (ev.n[-2:, :, 1] == 0).all() and (ev.n[:, :, 0] > 50).all()
    sm = fe.ic_summary(want.rank_ic, 2)
    assert torch.equal(ev.summary.rank_ic.mean, sm.mean)
    assert ev.summary.ic.n_dates.tolist() == [[10, 8]] * 4
    # a caller's candidate factors and a narrower universe
    cand = torch.randn(12, 2, 80, generator=_gen(4), dtype=F64)
    uni = torch.rand(12, 80, generator=_gen(5)) < 0.7
    ev2 = m.factor_ic(horizons=(2,), quantiles=0, signals=cand, universe=uni)
    w2 = fe.factor_ic(cand, fe.forward_returns(p.ret, (2,)), p.valid() & uni)
    assert torch.allclose(ev2.rank_ic, w2.rank_ic, rtol=0, atol=0, equal_nan=True)
    assert ev2.spread is None
    # rank autocorrelation: Spearman of x[d] against x[d - lag] on date d's universe
    ac = m.rank_autocorr(lag=2)
    assert ac.shape == (12, 4) and torch.isnan(ac[:2]).all() and torch.isfinite(ac[2:]).all()
    v = p.valid()
    for d, s in ((2, 0), (7, 3)):
        a, b = p.styles[d, s].double(), p.styles[d - 2, s].double()
        mm = (v[d] & torch.isfinite(a) & torch.isfinite(b)).numpy()
        assert abs(float(ac[d, s]) - ss.spearmanr(a.numpy()[mm], b.numpy()[mm])[0]) <= 1e-12


def test_cli_factor_ic_files_hold_the_methods_numbers(tmp_path):
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.utils.io import panel_from_barra_csv
    from tests.test_attribution_dist import _cli
    d = str(tmp_path)
    r = _cli(["synth", "--out", d, "--dates", "30", "--stocks", "60", "--industries", "4",
              "--styles", "3"])
    assert r.returncode == 0, r.stderr
    r = _cli(["risk", "--data", f"{d}/barra_data_csi.csv", "--industry", f"{d}/industry_info.csv",
              "--out", f"{d}/res", "--sims", "3", "--device", "cpu", "--factor-ic",
              "--ic-horizons", "1,4", "--ic-quantiles", "3"])
    assert r.returncode == 0, r.stderr[-3000:]
    per = pd.read_csv(f"{d}/res/factor_ic.csv")
    summ = pd.read_csv(f"{d}/res/factor_ic_summary.csv")
    assert list(per.columns) == ["date", "factor", "horizon", "n", "ic", "rank_ic"]
    panel = panel_from_barra_csv(f"{d}/barra_data_csi.csv", f"{d}/industry_info.csv", device="cpu")
    ev = RiskModel(panel).factor_ic(horizons=(1, 4), quantiles=3)
    D, S, H = ev.ic.shape
    assert len(per) == D * S * H and len(summ) == S * H
    assert per["factor"].tolist()[:H * S] == list(np.repeat(panel.style_names, H))
    assert per["horizon"].tolist()[:H] == [1, 4]
    assert per["n"].tolist() == ev.n.reshape(-1).tolist()
    for k in ("ic", "rank_ic"):
        np.testing.assert_allclose(per[k].values, getattr(ev, k).reshape(-1).numpy(), rtol=1e-12,
                                   atol=1e-15, equal_nan=True)
        for f in fe.ICSummary._fields:
            np.testing.assert_allclose(summ[f"{k}_{f}"].values,
                                       getattr(getattr(ev.summary, k), f).reshape(-1).numpy(),
                                       rtol=1e-12, atol=1e-15, equal_nan=True)
    q = torch.nan_to_num(ev.q_ret).sum(0) / torch.isfinite(ev.q_ret).sum(0)
    for g in range(3):
        np.testing.assert_allclose(summ[f"q{g + 1}"].values, q[..., g].reshape(-1).numpy(),
                                   rtol=1e-12, atol=1e-15)
    sp = torch.nan_to_num(ev.spread).sum(0) / torch.isfinite(ev.spread).sum(0)
    np.testing.assert_allclose(summ["spread"].values, sp.reshape(-1).numpy(), rtol=1e-12,
                               atol=1e-15)


# ------------------------------------------------------------------ GPU against the CPU path
GPU_N = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 5000, 8192]
GPU_G = [0, 1, 2, 10]
SHAPES = {"wide": (7, 11, 4), "one": (1, 1, 1)}


@functools.lru_cache(maxsize=None)
def _case(N, shape, kind, dtype):
    """Inputs (x, y, universe) on the CPU: tie-free or 5-level signals, stocks invalid in x but
    valid in y and the reverse, pair sets that differ per horizon (also horizons without their
    last rows), and with 7 dates an empty universe, a one-stock universe, an all-equal row and
    -0.0 next to +0.0."""
    D, S, H = SHAPES[shape]
    g = _gen(7 * N + D)
    x = torch.randn(D, S, N, generator=g, dtype=F64)
    y = 0.02 * torch.randn(D, H, N, generator=g, dtype=F64) + 0.004 * x[:, :1]
    if kind == "levels":
        x = torch.round(x).clamp(-2, 2)
        y[:, -1] = torch.round(y[:, -1] * 50)
    u = torch.rand(D, N, generator=g) < 0.9
    if N <= 3:
        u[:] = True
    x[..., 1::17] = float("nan")
    x[:, 0, 2::19] = float("inf")
    y[..., 5::23] = float("nan")
    y[:, 0, 6::29] = float("-inf")
    for h in range(1, H):
        y[:, h, 3 + h::13] = float("nan")
        y[D - h:, h] = float("nan")
    if D == 7:
        u[2] = False
        u[3] = False
        u[3, N // 2] = True
        x[3, :, N // 2] = 0.5
        y[3, 0, N // 2] = 0.01
        x[4, 0] = 1.5
        x[5, 0, ::2] = 0.0
        x[5, 0, 1::4] = -0.0
    return x.to(dtype), y, u


@functools.lru_cache(maxsize=None)
def _want(N, shape, kind, dtype, G):
    return fe.factor_ic(*_case(N, shape, kind, dtype), quantiles=G)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        torch.equal(torch.nan_to_num(a.cpu(), nan=-7.0), torch.nan_to_num(b.cpu(), nan=-7.0)) and \
        torch.equal(torch.isnan(a.cpu()), torch.isnan(b.cpu()))


def _compare(got, want, tag):
    assert torch.equal(got.n.cpu(), want.n), tag
    assert torch.equal(got.q_count.cpu(), want.q_count), tag
    torch.testing.assert_close(got.rank_ic.cpu(), want.rank_ic, rtol=0, atol=1e-14,
                               equal_nan=True, msg=lambda m: f"{tag} rank_ic: {m}")
    torch.testing.assert_close(got.ic.cpu(), want.ic, rtol=0, atol=1e-11, equal_nan=True,
                               msg=lambda m: f"{tag} ic: {m}")
    torch.testing.assert_close(got.q_ret.cpu(), want.q_ret, rtol=1e-12, atol=1e-15,
                               equal_nan=True, msg=lambda m: f"{tag} q_ret: {m}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["tiefree", "levels"])
@pytest.mark.parametrize("shape", ["wide", "one"])
@pytest.mark.parametrize("N", GPU_N)
def test_factor_ic_kernel_matches_cpu_path(cuda, N, shape, kind, dtype):
    x, y, u = (t.to(cuda) for t in _case(N, shape, kind, dtype))
    for G in GPU_G:   # one CPU reference per (case, G), kept for the tests below
        got = fe.factor_ic(x, y, u, quantiles=G)
        _compare(got, _want(N, shape, kind, dtype, G), (N, shape, kind, G))
        again = fe.factor_ic(x, y, u, quantiles=G)
        assert all(_same(a, b) for a, b in zip(got, again)), (N, G)
    if shape == "wide":
        assert int(got.n[2].max()) == 0 and int(got.n[3, :, 0].max()) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["tiefree", "levels"])
@pytest.mark.parametrize("N", GPU_N)
def test_xs_rank_kernel_equals_cpu_path(cuda, N, kind, dtype):
    x, _, u = _case(N, "wide", kind, dtype)
    want = fe.xs_rank(x, u)
    got = fe.xs_rank(x.to(cuda), u.to(cuda))
    assert _same(got, want)
    assert _same(fe.xs_rank(x.to(cuda), u.to(cuda)), got)


@pytest.mark.gpu
@pytest.mark.parametrize("N,step", [(65, 1), (1025, 37), (5000, 101)])
def test_triple_alone_equals_triple_in_the_full_call(cuda, N, step):
    x, y, u = (t.to(cuda) for t in _case(N, "wide", "tiefree", torch.float64))
    D, S, H = SHAPES["wide"]
    full = fe.factor_ic(x, y, u, quantiles=10)
    for t in range(0, D * S * H, step):
        d, s, h = t // (S * H), (t // H) % S, t % H
        one = fe.factor_ic(x[d:d + 1, s:s + 1], y[d:d + 1, h:h + 1], u[d:d + 1], quantiles=10)
        for a, b in zip(one, full):
            assert _same(a[0, 0, 0], b[d, s, h]), (d, s, h)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [65, 1025])
@pytest.mark.parametrize("kind", ["tiefree", "levels"])
def test_paired_equals_the_diagonal(cuda, N, kind):
    x, y, u = (t.to(cuda) for t in _case(N, "wide", kind, torch.float32))
    x = x[:, :4].contiguous()
    full = fe.factor_ic(x, y, u, quantiles=2)
    pair = fe.factor_ic(x, y, u, quantiles=2, paired=True)
    for a, b in zip(full[:3], pair[:3]):
        assert _same(torch.diagonal(a, dim1=1, dim2=2).contiguous(), b)
    for a, b in zip(full[3:], pair[3:]):
        assert _same(torch.diagonal(a, dim1=1, dim2=2).permute(0, 2, 1).contiguous(), b)
    _compare(pair, fe.factor_ic(x.cpu(), y.cpu(), u.cpu(), quantiles=2, paired=True), (N, kind))


@pytest.mark.gpu
def test_gpu_limits_raise_before_any_launch(cuda):
    def args(N, H):
        return (torch.zeros(1, 1, N, device=cuda), torch.zeros(1, H, N, dtype=F64, device=cuda),
                torch.ones(1, N, dtype=torch.bool, device=cuda))
    with pytest.raises(ValueError):
        fe.factor_ic(*args(8193, 1))
    with pytest.raises(ValueError):
        fe.factor_ic(*args(16, 9))
    with pytest.raises(ValueError):
        fe.factor_ic(*args(16, 1), quantiles=33)
    with pytest.raises(ValueError):
        fe.xs_rank(torch.zeros(1, 1, 8193, device=cuda),
                   torch.ones(1, 8193, dtype=torch.bool, device=cuda))
    r = fe.factor_ic(*args(16, 8), quantiles=32)     # the limits themselves run
    assert r.q_count.shape == (1, 1, 8, 32) and int(r.n.min()) == 16


@pytest.mark.gpu
def test_model_factor_ic_on_device_equals_cpu(cuda):
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    p = synthetic_panel(12, 300, P=5, Q=4, seed=6, missing_frac=0.03)
    want = RiskModel(p).factor_ic(horizons=(1, 3), quantiles=5)
    got = RiskModel(p.to(cuda)).factor_ic(horizons=(1, 3), quantiles=5)
    _compare(got, want, "model")
    # a difference of two bucket means, each within 1e-12 relative + 1e-15 absolute
    tol = 2 * (1e-12 * float(torch.nan_to_num(want.q_ret).abs().max()) + 1e-15)
    torch.testing.assert_close(got.spread.cpu(), want.spread, rtol=0, atol=tol, equal_nan=True)
    assert torch.equal(got.summary.ic.n_dates.cpu(), want.summary.ic.n_dates)
    torch.testing.assert_close(got.summary.ic.mean.cpu(), want.summary.ic.mean, rtol=0, atol=1e-11)
    torch.testing.assert_close(got.summary.rank_ic.mean.cpu(), want.summary.rank_ic.mean, rtol=0,
                               atol=1e-14)
    ac_w = RiskModel(p).rank_autocorr(lag=1)
    ac_g = RiskModel(p.to(cuda)).rank_autocorr(lag=1)
    torch.testing.assert_close(ac_g.cpu(), ac_w, rtol=0, atol=1e-14, equal_nan=True)
