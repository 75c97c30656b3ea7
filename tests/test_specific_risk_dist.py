"""Rank-invariant specific-risk model: a date-sharded gloo run reproduces the one-process
``specific_vol_ewnw``, ``specific_risk_use4`` (forecast of t - 1 and of t, gathered and carried
lambda scan), ``spec_vra_lambda`` and ``risk_attribution(h, specific_vol="use4")`` to 1e-12.
World 3 makes the blocks (about 12 dates) close to the 9-row halo; world 8 makes them (4 or 5
dates) shorter than it, so a window reaches across several rank boundaries."""
import os
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_attribution_dist import _free_port, _panel

KW = dict(window=10, lags=2, half_life=5.0)


def _cfg(scan):
    from llm_driven_multi_factor_model_amd.utils.config import preset
    return preset("reference", eigen_sims=5, time_scan=scan)


def _outputs(m):
    h = torch.full((m.panel.N,), 1.0 / m.panel.N, dtype=torch.float64)
    h[::3] *= 2.0
    out = {"ewnw": m.specific_vol_ewnw(**KW)}
    for oos in (True, False):
        out[f"use4_{oos}"] = m.specific_risk_use4(out_of_sample=oos, **KW)
        out[f"lambda_{oos}"] = m.spec_vra_lambda
    r = m.risk_attribution(h, specific_vol="use4")   # the defaults: window 252, 5 lags
    out.update(specific=r.specific_var, total=r.total_var, lambda_default=m.spec_vra_lambda)
    return out, m.specific_risk_use4(per_date=False, **KW)


def _worker(rank, world, port, path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.parallel import dist as pdist
    ctx = pdist.init_distributed(device="cpu")
    full = _panel()
    a, b = pdist.shard_range(full.D, ctx.rank, ctx.world)
    got = {}
    for scan in ("gather", "carry"):
        m = RiskModel(full.slice_dates(a, b), _cfg(scan), T_global=full.D, ctx=ctx).run()
        per, last = _outputs(m)
        got[scan] = {k: pdist.gather_to_root(v.contiguous(), ctx) for k, v in per.items()}
        lasts = pdist.all_gather_rows(last[None].contiguous(), ctx)   # returned on EVERY rank
        if ctx.rank == 0:
            got[scan]["lasts"] = lasts
    if ctx.rank == 0:
        torch.save(got, path)
    pdist.barrier(ctx)
    torch.distributed.destroy_process_group()


@pytest.fixture(scope="module")
def single():
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    return {scan: _outputs(RiskModel(_panel(), _cfg(scan)).run()) for scan in ("gather", "carry")}


@pytest.mark.parametrize("world", [2, 3, 8])
def test_specific_risk_rank_invariant(world, single):
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "sr.pt")
        mp.spawn(_worker, args=(world, _free_port(), path), nprocs=world, join=True)
        got = torch.load(path, weights_only=True)
    for scan in ("gather", "carry"):
        per, last = single[scan]
        for k, v in per.items():
            torch.testing.assert_close(got[scan][k], v, rtol=1e-12, atol=1e-15, equal_nan=True,
                                       msg=f"{scan} {k}")
        for r in range(world):
            torch.testing.assert_close(got[scan]["lasts"][r], last, rtol=1e-12, atol=1e-15,
                                       equal_nan=True)
        assert torch.isfinite(per["use4_True"][-1]).any() and (per["lambda_True"] > 0).all()
        # the window sums themselves are order-fixed: the same bits for every sharding
        assert torch.equal(torch.nan_to_num(got[scan]["ewnw"], nan=-1.0),
                           torch.nan_to_num(per["ewnw"], nan=-1.0))
