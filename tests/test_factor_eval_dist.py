"""Rank invariance of the factor evaluation (gloo on CPU): ``halo_next_rows`` is the slice of
the full series that follows a rank's block; ``RiskModel.factor_ic`` takes its forward returns
across rank boundaries through that halo and its summary from the gathered rows;
``rank_autocorr`` takes the lagged signals through ``halo_prev_rows``.  Worlds 2 and 3 on 37
dates with horizons up to 20 make blocks (18, 12 dates) shorter than the 19-row halo."""
import os
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_attribution_dist import _free_port, _panel

HORIZONS = (1, 5, 20)
HALO = max(HORIZONS) - 1
KW = dict(horizons=HORIZONS, quantiles=4, start=3)


def _outputs(m):
    ev = m.factor_ic(**KW)
    per = dict(n=ev.n, ic=ev.ic, rank_ic=ev.rank_ic, q_ret=ev.q_ret, q_count=ev.q_count,
               spread=ev.spread, autocorr=m.rank_autocorr(lag=2))
    glob = torch.stack([t.double() for sm in ev.summary for t in sm])   # [12, S, H]
    return per, glob


def _worker(rank, world, port, path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.parallel import dist as pdist
    ctx = pdist.init_distributed(device="cpu")
    full = _panel()
    a, b = pdist.shard_range(full.D, ctx.rank, ctx.world)
    m = RiskModel(full.slice_dates(a, b), T_global=full.D, ctx=ctx)
    ret = full.ret.double()
    halo = pdist.halo_next_rows(ret[a:b], HALO, ctx, m.sizes)
    want = torch.cat([ret[b:b + HALO], torch.full((HALO, full.N), float("nan"),
                                                  dtype=torch.float64)])[:HALO]
    halo_ok = halo.shape == want.shape and bool(
        (torch.isnan(halo) == torch.isnan(want)).all()
        and torch.equal(torch.nan_to_num(halo), torch.nan_to_num(want)))
    # an empty block in the middle is covered by the ranks after it
    mid = ret[a:b] if ctx.rank != 1 else ret[:0]
    lens = [b - a if r != 1 else 0 for r, (a, b) in
            enumerate(pdist.shard_range(full.D, r, ctx.world) for r in range(ctx.world))]
    h2 = pdist.halo_next_rows(mid, 3, ctx, lens)
    kept = torch.cat([ret[slice(*pdist.shard_range(full.D, r, ctx.world))]
                      for r in range(ctx.world) if r != 1] + [torch.full((3, full.N),
                                                                         float("nan"),
                                                                         dtype=torch.float64)])
    off = sum(lens[:ctx.rank + 1])
    w2 = kept[off:off + 3]
    halo_ok = halo_ok and bool((torch.isnan(h2) == torch.isnan(w2)).all()
                               and torch.equal(torch.nan_to_num(h2), torch.nan_to_num(w2)))
    per, glob = _outputs(m)
    got = {k: pdist.gather_to_root(v.contiguous(), ctx) for k, v in per.items()}
    globs = pdist.all_gather_rows(glob[None].contiguous(), ctx)
    oks = pdist.all_gather_rows(torch.tensor([float(halo_ok)], dtype=torch.float64), ctx)
    if ctx.rank == 0:
        got.update(globs=globs, halo_ok=oks)
        torch.save(got, path)
    pdist.barrier(ctx)
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_factor_ic_rank_invariant(world):
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "ic.pt")
        mp.spawn(_worker, args=(world, _free_port(), path), nprocs=world, join=True)
        got = torch.load(path, weights_only=True)
    assert got["halo_ok"].tolist() == [1.0] * world
    per, glob = _outputs(RiskModel(_panel()))
    for k, v in per.items():
        torch.testing.assert_close(got[k], v, rtol=1e-12, atol=1e-15, equal_nan=True, msg=k)
    for r in range(1, world):   # the summary is identical on every rank
        assert torch.equal(torch.nan_to_num(got["globs"][r]), torch.nan_to_num(got["globs"][0]))
    torch.testing.assert_close(got["globs"][0], glob, rtol=1e-12, atol=1e-15, equal_nan=True)
    assert torch.isfinite(glob[0]).all() and torch.isfinite(per["ic"][:17]).all()
    assert (per["n"][-HALO:, :, 2] == 0).all() and torch.isnan(per["autocorr"][:2]).all()


def test_halo_next_rows_without_a_process_group():
    from llm_driven_multi_factor_model_amd.parallel import dist as pdist
    x = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    h = pdist.halo_next_rows(x, 2, pdist.DistContext())
    assert h.shape == (2, 3) and torch.isnan(h).all()
    assert pdist.halo_next_rows(x, 0, pdist.DistContext()).shape == (0, 3)
