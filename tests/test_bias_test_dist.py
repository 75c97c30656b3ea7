"""Rank invariance of ``RiskModel.bias_test`` (gloo on CPU): the forecasts of date t - 1 reach
date t across rank boundaries through a one-row halo, the rolling window through a window - 1 row
halo, and the global statistics come from the all-gathered z rows.  Worlds 2, 3 and 8 on 37 dates
with ``window=10`` make blocks shorter than the window."""
import os
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_attribution_dist import _free_port, _panel

SPEC = ("shrunk", "use4")
KW = dict(window=10, min_periods=4, start=3)


def _cfg(time_scan):
    from llm_driven_multi_factor_model_amd.utils.config import preset
    return preset("reference", eigen_sims=5, time_scan=time_scan)


def _weights(N):
    g = torch.Generator().manual_seed(17)
    H = torch.rand(6, N, generator=g, dtype=torch.float64)
    H[3:] -= 0.5
    H[1, ::5] = float("nan")
    return H


def _outputs(m):
    out = {}
    for sv in SPEC:
        r = m.bias_test(_weights(m.panel.N), "vra", sv, **KW)
        out[sv] = (dict(z=r.z, forecast_vol=r.forecast_vol, rolling_bias=r.stats.rolling_bias,
                        mrad=r.stats.mrad, coverage=r.coverage),
                   torch.cat([r.stats.bias, r.stats.q_stat, r.stats.n_obs.double(),
                              r.stats.mrad_mean[None]]))
    return out


def _worker(rank, world, port, path, time_scan):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.parallel import dist as pdist
    ctx = pdist.init_distributed(device="cpu")
    full = _panel()
    a, b = pdist.shard_range(full.D, ctx.rank, ctx.world)
    m = RiskModel(full.slice_dates(a, b), _cfg(time_scan), T_global=full.D, ctx=ctx).run()
    got = {}
    for sv, (per, glob) in _outputs(m).items():
        got[sv] = ({k: pdist.gather_to_root(v.contiguous(), ctx) for k, v in per.items()},
                   pdist.all_gather_rows(glob[None].contiguous(), ctx))
    if ctx.rank == 0:
        torch.save(got, path)
    pdist.barrier(ctx)
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("time_scan", ["gather", "carry"])
def test_bias_test_rank_invariant(world, time_scan):
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "bias.pt")
        mp.spawn(_worker, args=(world, _free_port(), path, time_scan), nprocs=world, join=True)
        got = torch.load(path, weights_only=True)
    want = _outputs(RiskModel(_panel(), _cfg(time_scan)).run())
    for sv in SPEC:
        per, glob = want[sv]
        for k, v in per.items():
            torch.testing.assert_close(got[sv][0][k], v, rtol=1e-12, atol=1e-15, equal_nan=True,
                                       msg=f"{sv} {k}")
        ranks = got[sv][1]
        for r in range(1, world):   # the global statistics are identical on every rank
            assert torch.equal(ranks[r], ranks[0]), (sv, r)
        torch.testing.assert_close(ranks[0], glob, rtol=1e-12, atol=1e-15)
        assert torch.isfinite(glob).all()
        assert torch.isnan(per["z"][0]).all() and torch.isfinite(per["rolling_bias"][-1]).all()
