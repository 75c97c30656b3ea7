"""Timing of ops/factor_eval.py (csrc/factor_eval.hip): IC, rank IC and quantile-bucket returns,
against the same quantities from torch ops on the same GPU.

    python tools/factor_eval_bench.py [--dates 2520] [--stocks 5000]
                                      [--out profiles/r12/factor_eval_bench.log]

For an fp64 and an fp32 synthetic panel (S = 10 styles as signals, 1 % missing, horizons (1, 5,
20), G = 5 buckets) the forward returns are formed once (untimed); then, after a warm-up call,
``reps`` calls are timed between device synchronisations and the median is reported:

  * ``factor_ic`` (one kernel);
  * the torch composition: per chunk of dates a sort of every (date, signal, horizon) row of x
    and of y, tie averaging of the ranks through run ids and ``unique_consecutive`` counts, a
    scatter back to stock order, masked two-pass correlations, ``torch.nanquantile`` edges and one
    masked mean per bucket.  It must agree with the kernel (``n`` and ``q_count`` exactly, ``ic``,
    ``rank_ic`` and ``q_ret`` to 1e-10) or the run fails before anything is timed;
  * variants of the kernel call that show where its time goes (one kernel, so a kernel trace
    cannot split it): without buckets (G = 0), one horizon only (the other two add a y sort
    each, and an x sort where their pair set differs), and ``xs_rank`` (one sort and one ranking
    per (date, signal) plus a [D, S, N] fp64 store).

One JSON line per panel type goes to stdout and to ``--out``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HORIZONS, G = (1, 5, 20), 5
CHUNK = 48   # dates per block of the torch composition ([48, S, H, N] fp64 temporaries)


def _timed(fn, reps, dev):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def _ms(t):
    return {"median": round(t[0], 3), "min": round(t[1], 3), "max": round(t[2], 3)}


def _torch_ranks(v, m):
    """Average ranks of the rows of v [R, N] within m, by torch ops."""
    R, N = v.shape
    sk, order = torch.sort(torch.where(m, v, torch.full_like(v, float("inf"))), dim=1)
    new = torch.ones(R, N, dtype=torch.bool, device=v.device)
    new[:, 1:] = sk[:, 1:] != sk[:, :-1]
    ids = torch.cumsum(new.reshape(-1), 0) - 1
    _, counts = torch.unique_consecutive(ids, return_counts=True)
    ends = torch.cumsum(counts, 0)
    mid = (2 * ends - counts - 1).to(torch.float64) * 0.5          # mean flat position of a run
    row0 = (torch.arange(R, device=v.device) * N)[:, None]
    r = mid[ids].reshape(R, N) - row0 + 1.0
    return torch.empty_like(r).scatter_(1, order, r)


def _torch_corr(a, b, m, n):
    zero = torch.zeros((), dtype=torch.float64, device=a.device)
    nf = n.to(torch.float64)
    da = torch.where(m, a - (torch.where(m, a, zero).sum(1) / nf)[:, None], zero)
    db = torch.where(m, b - (torch.where(m, b, zero).sum(1) / nf)[:, None], zero)
    den = (da * da).sum(1) * (db * db).sum(1)
    c = (da * db).sum(1) / torch.sqrt(den)
    return torch.where((n >= 2) & (den > 0), c, zero + float("nan"))


def torch_composition(x, y, u):
    """(n, ic, rank_ic, q_ret, q_count) of ops.factor_eval.factor_ic from torch ops."""
    D, S, N = x.shape
    outs = []
    q = torch.arange(1, G, dtype=torch.float64, device=x.device) / G
    nan = torch.full((), float("nan"), dtype=torch.float64, device=x.device)
    for a in range(0, D, CHUNK):
        xb = x[a:a + CHUNK].double()[:, :, None, :]
        yb = y[a:a + CHUNK][:, None, :, :]
        m = u[a:a + CHUNK][:, None, None, :] & torch.isfinite(xb) & torch.isfinite(yb)
        shp = m.shape[:-1]
        m = m.reshape(-1, N)
        xb = xb.expand(shp + (N,)).reshape(-1, N)
        yb = yb.expand(shp + (N,)).reshape(-1, N)
        n = m.sum(1)
        ic = _torch_corr(xb, yb, m, n)
        ric = _torch_corr(_torch_ranks(xb, m), _torch_ranks(yb, m), m, n)
        edges = torch.nanquantile(torch.where(m, xb, nan), q, dim=1).T      # [R, G - 1]
        grp = (xb[:, :, None] > edges[:, None, :]).sum(2)
        q_ret, q_cnt = [], []
        for g in range(G):
            sel = m & (grp == g)
            c = sel.sum(1)
            q_cnt.append(c)
            q_ret.append(torch.where(c > 0, torch.where(sel, yb, torch.zeros_like(yb)).sum(1) / c,
                                     nan))
        outs.append((n.to(torch.int32).reshape(shp), ic.reshape(shp), ric.reshape(shp),
                     torch.stack(q_ret, 1).reshape(shp + (G,)),
                     torch.stack(q_cnt, 1).to(torch.int32).reshape(shp + (G,))))
    return tuple(torch.cat([o[k] for o in outs]) for k in range(5))


def _maxdiff(a, b):
    both = torch.isnan(a) & torch.isnan(b)
    d = torch.where(both, torch.zeros_like(a), (a - b).abs())
    return float(torch.nan_to_num(d, nan=float("inf")).max())


def bench(D, N, S, dtype, reps, dev):
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.ops import factor_eval as fe
    p = synthetic_panel(D, N, 31, S, seed=3, device=dev, missing_frac=0.01, dtype=dtype)
    x, u = p.styles, p.valid()
    y = fe.forward_returns(p.ret, HORIZONS)
    torch.cuda.synchronize(dev)
    out = {"D": D, "N": N, "S": S, "horizons": list(HORIZONS), "G": G,
           "panel": str(dtype).replace("torch.", ""), "reps": reps}

    got = fe.factor_ic(x, y, u, G)
    ref = torch_composition(x, y, u)
    diff = {"n_equal": bool(torch.equal(got.n, ref[0])),
            "q_count_equal": bool(torch.equal(got.q_count, ref[4])),
            "ic": _maxdiff(got.ic, ref[1]), "rank_ic": _maxdiff(got.rank_ic, ref[2]),
            "q_ret": _maxdiff(got.q_ret, ref[3])}
    out["max_diff_vs_torch"] = diff
    if not (diff["n_equal"] and diff["q_count_equal"]
            and max(diff["ic"], diff["rank_ic"], diff["q_ret"]) <= 1e-10):
        raise SystemExit(f"factor_ic differs from the torch composition: {json.dumps(diff)}")
    out["pair_sets"] = {"min": int(got.n[got.n > 0].min()), "max": int(got.n.max()),
                        "empty": int((got.n == 0).sum())}
    del ref
    torch.cuda.empty_cache()

    t1 = _timed(lambda: fe.factor_ic(x, y, u, G), reps, dev)
    out["factor_ic_ms"] = _ms(t1)
    t2 = _timed(lambda: torch_composition(x, y, u), reps, dev)
    out["torch_composition_ms"] = _ms(t2)
    out["speedup_over_torch"] = round(t2[0] / t1[0], 2)
    torch.cuda.empty_cache()
    out["factor_ic_no_buckets_ms"] = _ms(_timed(lambda: fe.factor_ic(x, y, u, 0), reps, dev))
    y1 = y[:, :1].contiguous()
    out["factor_ic_one_horizon_ms"] = _ms(_timed(lambda: fe.factor_ic(x, y1, u, G), reps, dev))
    out["xs_rank_ms"] = _ms(_timed(lambda: fe.xs_rank(x, u), reps, dev))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--dates", type=int, default=2520)
    ap.add_argument("--stocks", type=int, default=5000)
    ap.add_argument("--styles", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12",
                                                  "factor_eval_bench.log"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("factor_eval_bench needs a GPU: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for dtype in (torch.float64, torch.float32):
            r = bench(a.dates, a.stocks, a.styles, dtype, a.reps, dev)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
