"""Dense asset covariance / correlation blocks (``ops.asset_cov``, ``csrc/asset_cov.hip``),
``RiskModel.asset_cov``, ``RiskService.covariance`` / ``POST /cov`` and ``cli risk --asset-cov``.

Bound, as in ``tests/test_bias_test.py``: every entry is within ``1e-12 * S_ij`` of the oracle,

    S_ij = sum_kl |x_ik| |F_kl| |x_jl| + s_i^2 [n_i == n_j],

the same sum with the absolute value of every term.  The two chained K-term sums round to at most
(2 K + 2) eps S = 1.4e-14 S at K = 64, so 1e-12 leaves about 70x margin; ``vol^2`` is held to the
same bound against the diagonal.  The oracle of the CPU path is ``tests.test_box_qp._dense_sigma``
(an explicit design matrix); the GPU tests compare the kernels with the CPU path.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from llm_driven_multi_factor_model_amd.ops import asset_cov as ac
from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
from tests.test_box_qp import Case, _case, _dense_sigma, _risk_model   # noqa: F401
from tests.test_factor_cov import _assert_rel

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-12


# ------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _model():
    """``tests.test_box_qp._risk_model()``, fitted once for this file (never modified)."""
    return _risk_model()


def _rows(index, D):
    return index[None, :].expand(D, -1) if index.dim() == 1 else index


def _scale(styles, cap, ret, ind, stats, P, F, s, universe, index):
    """S [D, M, M] of the bound (0 on rows / columns of members outside the universe)."""
    D = styles.shape[0]
    m = fc.universe_mask(styles, cap, ret, ind, P, s, universe)
    Xa = fc.design_matrix(styles, cap, ret, ind, stats, P, m).abs()
    idx = _rows(index, D)
    at = idx.clamp(min=0)
    Z = Xa[torch.arange(D)[:, None], at] * (idx >= 0)[..., None]
    s2 = torch.nan_to_num(s.double() if s.dim() == 2 else s.double()[None, :].expand(D, -1)) ** 2
    same = idx[:, :, None] == idx[:, None, :]
    return Z @ torch.nan_to_num(F).abs() @ Z.transpose(1, 2) \
        + torch.where(same, s2.gather(1, at)[:, :, None], torch.zeros((), dtype=F64))


def _case_scale(c: Case, index):
    return _scale(*c.panel_args, c.F, c.s, c.universe, index)


def _within(got, ref, S, what):
    """NaN pattern equal; |got - ref| <= 1e-12 S on the rest.  Prints the worst ratio."""
    got, ref = got.cpu(), ref.cpu()
    assert got.shape == ref.shape, what
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaN pattern"
    fin = ~torch.isnan(ref)
    err = (got - ref).abs()[fin]
    worst = (err / S[fin].clamp(min=1e-300)).max().item() if err.numel() else 0.0
    print(f"{what}: worst error {worst:.2e} S (bound {REL:.0e})")
    assert (err <= REL * S[fin]).all(), f"{what}: {worst:.3e} S > {REL:.0e} S"
    return worst


def _symmetric(cov):
    nan = torch.isnan(cov)
    return torch.equal(nan, nan.transpose(-1, -2)) \
        and torch.equal(torch.nan_to_num(cov), torch.nan_to_num(cov).transpose(-1, -2))


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) \
        and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _cpu_call(c: Case, index, correlation=False):
    return ac.asset_cov(*c.panel_args, c.F, c.s, index, universe=c.universe,
                        correlation=correlation)


# ------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("edge", [False, True], ids=["plain", "edge"])
@pytest.mark.parametrize("shape,dtype", [((4, 203, 5, 4), torch.float64),
                                         ((2, 77, 0, 3), torch.float32)])
def test_dense_oracle(shape, dtype, edge):
    if edge and shape[0] < 3:
        # Case(edge=True) plants its NaN F on date 2: the two-date shape gets a third date
        shape = (3,) + shape[1:]
    c = _case(*shape, dtype=dtype, edge=edge)
    index = torch.arange(c.N)
    r = _cpu_call(c, index)
    S = _case_scale(c, index)
    assert r.cov.shape == (c.D, c.N, c.N) and r.vol.shape == (c.D, c.N)
    assert r.valid.dtype == torch.bool and r.cov.dtype == F64 and _symmetric(r.cov)
    seen_nan_date = False
    for d, ds in enumerate(_dense_sigma(c)):
        if ds is None:   # the NaN-F date
            assert torch.isnan(r.cov[d]).all() and torch.isnan(r.vol[d]).all()
            assert not r.valid[d].any()
            seen_nan_date = True
            continue
        idx, Sig = ds
        on = torch.zeros(c.N, dtype=torch.bool)
        on[idx] = True
        assert torch.equal(r.valid[d], on)
        blk = r.cov[d][idx][:, idx]
        err = (blk - Sig).abs()
        Sb = S[d][idx][:, idx]
        print(f"date {d}: |U| {len(idx)}, worst {(err / Sb).max().item():.2e} S")
        assert (err <= REL * Sb).all()
        off = ~(on[:, None] & on[None, :])
        assert torch.isnan(r.cov[d][off]).all() and torch.isfinite(blk).all()
        assert torch.isnan(r.vol[d][~on]).all()
        dg = torch.diagonal(Sig)
        assert ((r.vol[d][idx] ** 2 - dg).abs() <= REL * torch.diagonal(Sb)).all()
    assert seen_nan_date == edge


@pytest.mark.parametrize("edge", [False, True], ids=["plain", "edge"])
def test_against_apply_cov(edge):
    c = _case(4, 203, 5, 4, edge=edge)
    g = torch.Generator().manual_seed(7)
    index = torch.randperm(c.N, generator=g)[:40]
    r = _cpu_call(c, index)
    h = torch.zeros(c.D, c.N, dtype=F64)
    hv = torch.randn(c.D, 40, generator=g, dtype=F64)
    h[:, index] = torch.where(r.valid, hv, torch.zeros((), dtype=F64))
    ref = fc.apply_cov(*c.panel_args, c.F, c.s, h, universe=c.universe)[:, index]
    got = torch.einsum("dij,dj->di", torch.nan_to_num(r.cov), h[:, index])
    dates = [d for d in range(c.D) if torch.isfinite(c.F[d]).all()]
    assert len(dates) == (3 if edge else 4) and r.valid[dates].any(-1).all()
    _assert_rel(got[dates], ref[dates], 1e-12, "cov @ h vs apply_cov")


def test_index_handling():
    c = _case(4, 203, 5, 4)
    g = torch.Generator().manual_seed(8)
    index = torch.randperm(c.N, generator=g)[:50]
    r = _cpu_call(c, index)
    assert r.index is index or torch.equal(r.index, index)
    # static [M] == the same basket given per date
    rd = _cpu_call(c, index[None, :].expand(c.D, -1).contiguous())
    assert _same(r.cov, rd.cov) and _same(r.vol, rd.vol) and torch.equal(r.valid, rd.valid)
    # -1 padding: NaN rows and columns, valid False, the rest untouched
    pad = index.clone()
    pad[[3, 17, 49]] = -1
    rp = _cpu_call(c, pad)
    assert not rp.valid[:, [3, 17, 49]].any() and torch.isnan(rp.vol[:, [3, 17, 49]]).all()
    assert torch.isnan(rp.cov[:, [3, 17, 49], :]).all() and torch.isnan(rp.cov[:, :, [3, 17, 49]]).all()
    keep = torch.ones(50, dtype=torch.bool)
    keep[[3, 17, 49]] = False
    assert _same(rp.cov[:, keep][:, :, keep], r.cov[:, keep][:, :, keep])
    assert torch.equal(rp.valid[:, keep], r.valid[:, keep])
    # a name listed twice is the same asset: off-diagonal = diagonal, within the bound
    dup = index.clone()
    dup[30] = dup[4]
    rdup = _cpu_call(c, dup)
    S = _case_scale(c, dup)
    v = rdup.valid[:, 4]
    assert v.any() and torch.equal(rdup.valid[:, 30], v)
    for a, b in ((4, 30), (30, 4)):
        err = (rdup.cov[:, a, b] - rdup.cov[:, 4, 4]).abs()[v]
        assert (err <= REL * S[:, a, b][v]).all()
        assert (rdup.cov[:, a, b][v] > 0).all()
    # a permuted basket gives the permuted block
    perm = torch.randperm(50, generator=g)
    rperm = _cpu_call(c, index[perm])
    _within(rperm.cov, r.cov[:, perm][:, :, perm], _case_scale(c, index[perm]), "permuted")
    assert torch.equal(rperm.valid, r.valid[:, perm])
    # index N (and anything below -1) is refused
    for bad in (c.N, -2):
        badidx = index.clone()
        badidx[1] = bad
        with pytest.raises(ValueError, match="index"):
            _cpu_call(c, badidx)
    # empty baskets and zero-date blocks
    e = _cpu_call(c, index[:0])
    assert e.cov.shape == (c.D, 0, 0) and e.vol.shape == (c.D, 0) and e.valid.shape == (c.D, 0)
    p = c.p.slice_dates(0, 0)
    z = ac.asset_cov(p.styles, p.cap, p.ret, p.ind, c.stats[:0], c.P, c.F[:0], c.s, index)
    assert z.cov.shape == (0, 50, 50) and z.vol.shape == (0, 50) and z.valid.shape == (0, 50)


@pytest.mark.parametrize("shape,edge", [((4, 203, 5, 4), False), ((4, 203, 5, 4), True),
                                        ((2, 130, 3, 16), False)])
def test_structure(shape, edge):
    c = _case(*shape, edge=edge)
    g = torch.Generator().manual_seed(9)
    index = torch.randperm(c.N, generator=g)[:90]
    r, rc = _cpu_call(c, index), _cpu_call(c, index, correlation=True)
    assert _symmetric(r.cov) and _symmetric(rc.cov)
    assert torch.equal(r.valid, rc.valid) and _same(r.vol, rc.vol)
    for d in range(c.D):
        v = r.valid[d]
        if not v.any():
            assert not torch.isfinite(c.F[d]).all()
            continue
        blk = r.cov[d][v][:, v]
        w = torch.linalg.eigvalsh(blk)      # F is PSD: so is the block
        top = torch.diagonal(blk).max().item()
        print(f"date {d}: smallest eigenvalue {w[0].item() / top:.2e} of the largest variance")
        assert w[0].item() >= -1e-12 * top
        cor = rc.cov[d][v][:, v]
        assert (torch.diagonal(cor) == 1.0).all()
        assert (cor.abs() <= 1 + 1e-12).all()
        vol = r.vol[d][v]
        torch.testing.assert_close(cor, blk / (vol[:, None] * vol[None, :]), rtol=1e-12, atol=0)
    assert torch.equal(torch.isnan(r.cov), torch.isnan(rc.cov))


def test_date_does_not_depend_on_the_others():
    c = _case(4, 203, 5, 4, edge=True)
    index = torch.arange(0, c.N, 2)
    r = _cpu_call(c, index)
    for d in (1, 3):
        p = c.p.slice_dates(d, d + 1)
        one = ac.asset_cov(p.styles, p.cap, p.ret, p.ind, c.stats[d:d + 1], c.P, c.F[d:d + 1],
                           c.s, index, universe=c.universe[d:d + 1])
        assert _same(one.cov, r.cov[d:d + 1]) and _same(one.vol, r.vol[d:d + 1])


def test_risk_model_asset_cov_cpu():
    m = _model()
    p = m.panel
    g = torch.Generator().manual_seed(10)
    index = torch.randperm(p.N, generator=g)[:25]
    names = [str(p.stocks[i]) for i in index.tolist()]
    r = m.asset_cov(names)
    ri = m.asset_cov(index)
    assert r.cov.shape == (p.D, 25, 25)
    assert _same(r.cov, ri.cov) and _same(r.vol, ri.vol) and torch.equal(r.valid, ri.valid)
    assert r.valid[-10:].any(-1).all() and _symmetric(r.cov)
    ref = ac.asset_cov(p.styles, p.cap, p.ret, p.ind, m.stats, p.P, m.vra_cov,
                       m.specific_risk_shrunk(), index)
    assert _same(r.cov, ref.cov)
    # dates = (t, t + 1): row t of the full call, bit for bit; per-date baskets are cut too
    per_date = index[None, :].expand(p.D, -1).clone()
    per_date[:, 0] = -1
    rpd = m.asset_cov(per_date)
    for t in (1, p.D - 3, p.D - 1):
        r1 = m.asset_cov(names, dates=(t, t + 1))
        assert r1.cov.shape == (1, 25, 25)
        assert _same(r1.cov, r.cov[t:t + 1]) and _same(r1.vol, r.vol[t:t + 1])
        assert torch.equal(r1.valid, r.valid[t:t + 1])
        assert _same(m.asset_cov(per_date, dates=(t, t + 1)).cov, rpd.cov[t:t + 1])
    # vol = the total volatility risk_attribution reports for the one-hot holding of the name
    for i in (0, 7, 24):
        h = torch.zeros(p.N, dtype=F64)
        h[index[i]] = 1.0
        tv = torch.sqrt(m.risk_attribution(h).total_var)
        v = r.valid[:, i]
        assert v.any()
        torch.testing.assert_close(r.vol[:, i][v], tv[v], rtol=1e-12, atol=0)
    # correlation, other covariance series and a given specific volatility are passed on
    sv = m.specific_risk_shrunk()
    rc = m.asset_cov(names, which="nw", specific_vol=sv, correlation=True)
    ref = ac.asset_cov(p.styles, p.cap, p.ret, p.ind, m.stats, p.P, m.nw_cov, sv, index,
                       correlation=True)
    assert _same(rc.cov, ref.cov)
    with pytest.raises(KeyError, match="NOT_A_STOCK"):
        m.asset_cov(names + ["NOT_A_STOCK"])
    e = m.asset_cov([])
    assert e.cov.shape == (p.D, 0, 0) and e.valid.shape == (p.D, 0)
    z = m.asset_cov(names, dates=(5, 5))
    assert z.cov.shape == (0, 25, 25) and z.vol.shape == (0, 25)


# ----------------------------------------------------------------------------- serving, CLI
def _service():
    from llm_driven_multi_factor_model_amd.serving import RiskService
    return RiskService(_model())


def test_service_covariance():
    svc = _service()
    ok = svc.held_ok.tolist()
    held = [s for s, k in zip(svc.stocks, ok) if k]
    names = held[3:15] + ["NOT_A_STOCK"] + held[:2]
    r = svc.covariance(names)
    kept = held[3:15] + held[:2]
    assert r.kept == kept and r.ignored == ["NOT_A_STOCK"]
    idx = torch.tensor([svc._pos[s] for s in kept])
    Xs = svc.X[idx]
    ref = Xs @ svc.F @ Xs.T + torch.diag(svc.s2[idx])
    assert r.cov.shape == (14, 14) and torch.equal(r.cov, r.cov.T)
    torch.testing.assert_close(r.cov, ref, rtol=1e-12, atol=1e-12 * ref.abs().max().item())
    rc = svc.covariance(names, correlation=True)
    vol = torch.sqrt(torch.diagonal(r.cov))
    assert (torch.diagonal(rc.cov) == 1.0).all() and torch.equal(rc.cov, rc.cov.T)
    torch.testing.assert_close(rc.cov, r.cov / (vol[:, None] * vol[None, :]), rtol=1e-12, atol=0)
    # a name given twice is the same asset
    rd = svc.covariance([kept[0], kept[1], kept[0]])
    assert rd.cov[0, 2] == rd.cov[0, 0] == rd.cov[2, 2]
    # the model's own block on the snapshot date (the service's universe is wider: no return
    # needed), where the model's member is valid
    m = _model()
    mr = m.asset_cov(kept, dates=(m.panel.D - 1, m.panel.D))
    v = mr.valid[0]
    assert v.sum() >= 10
    torch.testing.assert_close(r.cov[v][:, v], mr.cov[0][v][:, v], rtol=1e-10,
                               atol=1e-12 * r.cov.abs().max().item())


def test_http_cov():
    from fastapi.testclient import TestClient

    from llm_driven_multi_factor_model_amd.serving import make_app
    svc = _service()
    client = TestClient(make_app(svc))
    held = [s for s, k in zip(svc.stocks, svc.held_ok.tolist()) if k]
    names = held[:6] + ["NOT_A_STOCK"]
    out = client.post("/cov", json={"stocks": names}).json()
    assert out["date"] == svc.date and out["stocks"] == held[:6]
    assert out["ignored"] == ["NOT_A_STOCK"]
    ref = svc.covariance(names).cov
    assert np.array_equal(np.asarray(out["cov"], dtype=np.float64), ref.numpy())
    cor = client.post("/cov", json={"stocks": names, "correlation": True}).json()["cov"]
    assert np.array_equal(np.asarray(cor, dtype=np.float64),
                          svc.covariance(names, correlation=True).cov.numpy())
    assert client.post("/cov", json={}).status_code == 422


def test_cli_asset_cov(tmp_path):
    d = str(tmp_path)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")

    def cli(*args):
        return subprocess.run([sys.executable, "-m", "llm_driven_multi_factor_model_amd.cli",
                               *args], cwd=ROOT, capture_output=True, text=True, timeout=600,
                              env=env)

    r = cli("synth", "--out", d, "--dates", "45", "--stocks", "70", "--industries", "5")
    assert r.returncode == 0, r.stderr
    data = pd.read_csv(f"{d}/barra_data_csi.csv")
    last = data[data["date"] == data["date"].iloc[-1]]
    names = list(last["stocknames"].astype(str).unique()[:12][::-1])
    pd.DataFrame({"stocknames": names}).to_csv(f"{d}/names.csv", index=False)
    r = cli("risk", "--data", f"{d}/barra_data_csi.csv", "--industry", f"{d}/industry_info.csv",
            "--out", f"{d}/res", "--sims", "4", "--asset-cov", f"{d}/names.csv",
            "--specific-model", "use4", "--device", "cpu")
    assert r.returncode == 0, r.stderr[-3000:]
    out = pd.read_csv(f"{d}/res/asset_cov.csv", index_col=0)
    assert list(out.index.astype(str)) == names and list(out.columns.astype(str)) == names
    a = out.to_numpy(dtype=np.float64)
    assert a.shape == (12, 12)
    assert np.array_equal(a, a.T, equal_nan=True)
    fin = np.isfinite(np.diagonal(a))
    assert fin.sum() >= 6 and (np.diagonal(a)[fin] > 0).all()


def test_write_asset_cov_date_and_correlation(tmp_path):
    from llm_driven_multi_factor_model_amd.cli import _write_asset_cov
    m = _model()
    p = m.panel
    names = [str(s) for s in p.stocks[:9]]
    pd.DataFrame({"stocknames": names}).to_csv(tmp_path / "names.csv", index=False)
    t = p.D - 4
    date = str(np.datetime_as_string(np.asarray(p.dates)[t], unit="D"))
    path = _write_asset_cov(m, str(tmp_path / "names.csv"), str(tmp_path), m.ctx, "trailing",
                            date, True)
    out = pd.read_csv(path, index_col=0, float_precision="round_trip").to_numpy(dtype=np.float64)
    ref = m.asset_cov(names, dates=(t, t + 1), correlation=True).cov[0].numpy()
    assert np.array_equal(out, ref, equal_nan=True)
    with pytest.raises(SystemExit):
        _write_asset_cov(m, str(tmp_path / "names.csv"), str(tmp_path), m.ctx, "trailing",
                         "1901-01-01")


# ------------------------------------------------------------------------------------ GPU
def _basket(c: Case, kind: str) -> torch.Tensor:
    g = torch.Generator().manual_seed(6000 + c.N)
    if kind == "all":
        return torch.arange(c.N)
    if kind == "per-date-130":      # [D, 130]: -1 pads, one duplicate inside a tile and one
        idx = torch.stack([torch.randperm(c.N, generator=g)[:130] for _ in range(c.D)])
        idx[:, 100] = idx[:, 7]     # ... across two tile rows (an off-diagonal tile)
        idx[:, 21] = idx[:, 20]
        idx[:, [0, 63, 64, 129]] = -1
        idx[1, 40:50] = -1
        return idx
    return torch.randperm(c.N, generator=g)[:int(kind)]


# (D, N, P, Q), dtype, edge, basket
GPU_CASES = [
    pytest.param((3, 203, 5, 4), torch.float32, False, "all", id="k10-all-203-f32"),
    pytest.param((3, 203, 5, 4), torch.float64, True, "per-date-130", id="edge-per-date-f64"),
    pytest.param((2, 300, 53, 10), torch.float32, False, "65", id="k64-m65-f32"),
    pytest.param((2, 130, 3, 16), torch.float32, False, "64", id="q16-m64-f32"),
    pytest.param((2, 77, 0, 3), torch.float32, False, "1", id="k4-m1-f32"),
    pytest.param((2, 77, 0, 3), torch.float32, False, "all", id="k4-all-77-f32"),
]


@functools.lru_cache(maxsize=None)
def _cpu_ref(c: Case, kind: str, correlation: bool):
    index = _basket(c, kind)
    return index, _cpu_call(c, index, correlation), _case_scale(c, index)


def _gpu_call(c: Case, index, cuda, correlation=False):
    uni = None if c.universe is None else c.universe.to(cuda)
    return ac.asset_cov(*c.on(cuda), c.F.to(cuda), c.s.to(cuda), index.to(cuda), universe=uni,
                        correlation=correlation)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype,edge,kind", GPU_CASES)
def test_hip_matches_cpu(cuda, shape, dtype, edge, kind):
    c = _case(*shape, dtype=dtype, edge=edge)
    index, ref, S = _cpu_ref(c, kind, False)
    got = _gpu_call(c, index, cuda)
    assert got.cov.is_cuda and got.cov.shape == ref.cov.shape
    assert torch.equal(got.valid.cpu(), ref.valid)
    assert ref.valid.any()
    _within(got.cov, ref.cov, S, "cov")
    assert _symmetric(got.cov)
    Sd = torch.diagonal(S, dim1=1, dim2=2)
    _within(got.vol ** 2, ref.vol ** 2, Sd, "vol^2")
    _within(got.vol.cpu() ** 2, torch.diagonal(got.cov.cpu(), dim1=1, dim2=2), Sd,
            "vol^2 vs the diagonal")
    if edge:
        assert torch.isnan(got.cov[2]).all() and not got.valid[2].any()   # the NaN-F date
        pads = (index < 0)
        assert torch.isnan(got.cov.cpu()[pads]).all() and not got.valid.cpu()[pads].any()
    # correlation: the same against the CPU path, the bound carried through the division
    # (1e-12 S_ij / (vol_i vol_j)); rtol 1e-12 of each entry against the kernel's own
    # cov / (vol x vol); the diagonal exactly 1.  An entrywise rtol against the CPU path is no
    # check of the kernel: x_i^T F x_j cancels, and on the first case (ZF)Z^T and Z(FZ^T) in
    # float64 on the CPU already differ by 2.4e-12 of the smallest entries (3.8e-16 S); the
    # kernel measured 3.4e-12 of such an entry there (3.2e-16 S).
    _, refc, _ = _cpu_ref(c, kind, True)
    gotc = _gpu_call(c, index, cuda, correlation=True)
    assert torch.equal(gotc.valid.cpu(), ref.valid) and _same(gotc.vol, got.vol)
    cc, rc = gotc.cov.cpu(), refc.cov
    assert _symmetric(gotc.cov)
    vv = ref.vol[:, :, None] * ref.vol[:, None, :]
    _within(cc, rc, S / vv.nan_to_num(nan=1.0), "correlation")
    fin = ~torch.isnan(rc)
    gv = got.vol.cpu()
    own = got.cov.cpu() / (gv[:, :, None] * gv[:, None, :])
    off = fin & ~torch.eye(cc.shape[-1], dtype=torch.bool)[None]
    torch.testing.assert_close(cc[off], own[off], rtol=1e-12, atol=0)
    dg = torch.diagonal(cc, dim1=1, dim2=2)
    assert (dg[ref.valid] == 1.0).all()
    assert (cc[fin].abs() <= 1 + 1e-12).all()


@pytest.mark.gpu
def test_hip_bitwise_and_date_slices(cuda):
    c = _case(3, 203, 5, 4, dtype=torch.float64, edge=True)
    index = _basket(c, "per-date-130")
    for corr in (False, True):
        r1, r2 = _gpu_call(c, index, cuda, corr), _gpu_call(c, index, cuda, corr)
        for a, b in zip(r1[:3], r2[:3]):
            assert _same(a, b)
        assert _symmetric(r1.cov)
        # dates (1, 2): row 1 of the full call
        p = c.p.slice_dates(1, 2).to(cuda)
        one = ac.asset_cov(p.styles, p.cap, p.ret, p.ind, c.stats[1:2].to(cuda), c.P,
                           c.F[1:2].to(cuda), c.s.to(cuda), index[1:2].to(cuda),
                           universe=c.universe[1:2].to(cuda), correlation=corr)
        for a, b in zip(one[:3], r1[:3]):
            assert _same(a, b[1:2])
    # a static basket equals the same basket given per date; small date chunks change nothing
    c = _case(3, 203, 5, 4)
    index = _basket(c, "all")
    r = _gpu_call(c, index, cuda)
    rd = _gpu_call(c, index[None, :].expand(c.D, -1).contiguous(), cuda)
    assert _same(r.cov, rd.cov) and _same(r.vol, rd.vol) and torch.equal(r.valid, rd.valid)
    old = ac.SCRATCH_BYTES
    try:
        ac.SCRATCH_BYTES = 1       # one date per chunk
        rs = _gpu_call(c, index, cuda)
    finally:
        ac.SCRATCH_BYTES = old
    assert _same(r.cov, rs.cov) and _same(r.vol, rs.vol) and torch.equal(r.valid, rs.valid)


@pytest.mark.gpu
def test_hip_asset_cov_limits_raise_before_launch(cuda):
    D, N, P, Q = 1, 16, 54, 10   # K = 65
    K = 1 + P + Q
    X = torch.zeros(D, Q, N, device=cuda)
    v = torch.zeros(D, N, device=cuda)
    ind = torch.zeros(D, N, dtype=torch.int16, device=cuda)
    st = torch.ones(D, Q + 2, dtype=F64, device=cuda)
    F = torch.eye(K, dtype=F64, device=cuda)[None]
    s = torch.ones(N, dtype=F64, device=cuda)
    index = torch.arange(N, device=cuda)
    with pytest.raises(ValueError, match="64"):
        ac.asset_cov(X, v, v, ind, st, P, F, s, index)
    X17 = torch.zeros(D, 17, N, device=cuda)   # Q = 17 > 16 styles
    with pytest.raises(ValueError, match="16"):
        ac.asset_cov(X17, v, v, None, torch.ones(D, 19, dtype=F64, device=cuda), 0,
                     torch.eye(18, dtype=F64, device=cuda)[None], s, index)
    # an index outside [-1, N) is refused on the device too
    X4 = torch.zeros(D, 4, N, device=cuda)
    with pytest.raises(ValueError, match="index"):
        ac.asset_cov(X4, v, v, None, torch.ones(D, 6, dtype=F64, device=cuda), 0,
                     torch.eye(5, dtype=F64, device=cuda)[None], s,
                     torch.tensor([0, N], device=cuda))


@pytest.mark.gpu
def test_risk_model_asset_cov_gpu_matches_cpu(cuda):
    """As ``test_risk_model_risk_budget_gpu_matches_cpu``: the CPU model is given the GPU model's
    eigen and VRA covariances; each model uses its own specific volatilities (they differ in
    their last bits, 1e-16 of s^2, far inside the bound)."""
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(80, 520, 31, 10, seed=5, missing_frac=0.03)
    cfg = preset("reference", eigen_sims=5)
    mc = RiskModel(p, cfg).run()
    mg = RiskModel(p.to(cuda), cfg).run()
    mc.eigen_cov, mc.vra_cov = mg.eigen_cov.cpu(), mg.vra_cov.cpu()
    svc, svg = mc.specific_risk_shrunk(), mg.specific_risk_shrunk()
    g = torch.Generator().manual_seed(3)
    index = torch.randperm(p.N, generator=g)[:100]
    names = [str(p.stocks[i]) for i in index.tolist()]
    S = _scale(p.styles, p.cap, p.ret, p.ind, mc.stats, p.P, mc.vra_cov, svc, None, index)
    for corr in (False, True):
        rc = mc.asset_cov(names, specific_vol=svc, correlation=corr)
        rg = mg.asset_cov(names, specific_vol=svg, correlation=corr)
        assert torch.equal(rc.valid, rg.valid.cpu()) and rc.valid[-10:].any(-1).all()
        assert _symmetric(rg.cov)
        if corr:
            vol = rc.vol
            _within(rg.cov, rc.cov, S / (vol[:, :, None] * vol[:, None, :]).nan_to_num(nan=1.0),
                    "correlation")
        else:
            _within(rg.cov, rc.cov, S, "cov")
            _within(rg.vol ** 2, rc.vol ** 2, torch.diagonal(S, dim1=1, dim2=2), "vol^2")
