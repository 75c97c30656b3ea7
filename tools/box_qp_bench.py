"""Timing of RiskModel.optimize (ops/box_qp.py, csrc/box_qp.hip) against the same algorithm
written with torch ops on the GPU.

    python tools/box_qp_bench.py [--dates 2520] [--stocks 5000]
                                 [--out profiles/r08/box_qp_bench.log]

For an fp64 and an fp32 synthetic panel (P = 31 industries, Q = 10 styles, 1 % missing) one
RiskModel is run once (untimed) and its shrunk specific volatility precomputed; then, for
long-only minimum variance (bounds [0, 1]) and the 2 % cap (bounds [0, 0.02]), after a warm-up
call ``reps`` calls of ``optimize(which="vra", specific_vol=<precomputed>)`` are timed between
device synchronisations and the median is reported, together with

  * the histogram of ``passes`` and of ``status`` over the dates;
  * the median time of each launch of one pass (apply, project with the rows in registers and
    re-streamed, Gram, X^T h, step), from separately synchronised calls on the first trial;
  * the same algorithm with torch ops (``box_qp(..., torch_ops=True)``: dense X_d, einsum,
    torch.linalg.cholesky), in chunks of dates, and its worst difference from the HIP result
    (over all finite dates, and over the dates that both solvers report as converged).
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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


def _hist(t):
    return dict(sorted(collections.Counter(t.tolist()).items()))


def torch_optimize(p, stats, F, sv, upper, chunk):
    from llm_driven_multi_factor_model_amd.ops import box_qp as bq
    ws, ss = [], []
    for lo in range(0, p.D, chunk):
        sl = slice(lo, lo + chunk)
        r = bq.box_qp(p.styles[sl], p.cap[sl], p.ret[sl], p.ind[sl], stats[sl], p.P, F[sl],
                      sv[sl], None, 0.0, upper, torch_ops=True)
        ws.append(r.weights)
        ss.append(r.status)
    return torch.cat(ws), torch.cat(ss)


def bench(D, N, P, Q, dtype, reps, dev, chunk, torch_reps):
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.ops import box_qp as bq
    from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(D, N, P, Q, seed=3, device=dev, missing_frac=0.01, dtype=dtype)
    m = RiskModel(p, preset("reference", eigen_sims=10)).run()
    sv = m.specific_risk_shrunk()
    torch.cuda.synchronize(dev)
    out = {"D": D, "N": N, "K": p.K, "panel": str(dtype).replace("torch.", ""), "reps": reps}
    args = (p.styles, p.cap, p.ret, p.ind, m.stats, p.P)
    for name, upper in (("long_only", 1.0), ("cap_2pct", 0.02)):
        res = {}
        res["optimize_ms"] = _ms(_timed(lambda: m.optimize(upper=upper, which="vra",
                                                           specific_vol=sv), reps, dev))
        res["optimize_stream_rows_ms"] = _ms(_timed(
            lambda: m.optimize(upper=upper, which="vra", specific_vol=sv, stream_rows=True),
            reps, dev))
        r = m.optimize(upper=upper, which="vra", specific_vol=sv)
        res["passes_hist"] = _hist(r.passes)
        res["status_hist"] = _hist(r.status)
        # one pass, launch by launch, on the trial after the first step
        pb = bq.make_problem(*args, m.vra_cov, sv, None, 0.0, upper)
        st, pj = bq.new_state(D, p.K, dev), bq.new_projection(D, N, dev)
        bq.run_pass(pb, st, pj, 1e-10)
        c = st.c[:, None, :].contiguous()
        u = fc.factor_apply(*args, pb.a, -pb.a, pb.q[:, None], c)[:, 0].contiguous()
        G = fc.factor_gram(*args, pj.w)
        x = fc.factor_xty(*args, pj.h[:, None])[:, 0].contiguous()
        scratch = bq.new_projection(D, N, dev)

        def step():
            bq.box_step(G, pb.lam, pb.U, x, pj.stats, pj.flag, st.clone(), 1e-10)
        steps = {
            "apply": lambda: fc.factor_apply(*args, pb.a, -pb.a, pb.q[:, None], c),
            "project (registers)": lambda: bq.box_project(u, pb.a, pb.lo, pb.hi, pb.budget,
                                                          pb.q, pj.gamma, st.status, out=scratch),
            "project (re-streamed)": lambda: bq.box_project(u, pb.a, pb.lo, pb.hi, pb.budget,
                                                            pb.q, pj.gamma, st.status,
                                                            out=scratch, stream_rows=True),
            "project (cold start, registers)": lambda: bq.box_project(
                u, pb.a, pb.lo, pb.hi, pb.budget, pb.q, torch.zeros_like(pj.gamma), st.status,
                out=scratch),
            "gram": lambda: fc.factor_gram(*args, pj.w),
            "xty": lambda: fc.factor_xty(*args, pj.h[:, None]),
            "step (incl. state clone)": step,
            "state clone": lambda: st.clone(),
        }
        res["pass_ms"] = {k: round(_timed(f, reps, dev)[0], 3) for k, f in steps.items()}
        try:
            tw, ts = torch_optimize(p, m.stats, m.vra_cov, sv, upper, chunk)
            res["torch_ops_ms"] = _ms(_timed(
                lambda: torch_optimize(p, m.stats, m.vra_cov, sv, upper, chunk), torch_reps, dev))
            res["torch_ops_date_chunk"] = chunk
            fin = torch.isfinite(r.weights).all(-1) & torch.isfinite(tw).all(-1)
            diff = ((tw - r.weights)[fin].abs().amax(-1) / r.weights[fin].abs().amax(-1)).max()
            res["torch_ops_worst_rel_diff_vs_hip"] = float(diff)
            res["finite_dates"] = int(fin.sum())
            okd = (r.status == bq.OK) & (ts == bq.OK)
            rel = (tw - r.weights)[okd].abs().amax(-1) / r.weights[okd].abs().amax(-1)
            res["torch_ops_worst_rel_diff_on_ok_dates"] = float(rel.max())
            res["ok_dates_both"] = int(okd.sum())
            res["hip_speedup_over_torch_ops"] = round(
                res["torch_ops_ms"]["median"] / res["optimize_ms"]["median"], 2)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            res["torch_ops_ms"] = "out of memory"
        out[name] = res
        print(f"[box_qp_bench] {out['panel']} {name} done", file=sys.stderr, flush=True)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--dates", type=int, default=2520)
    ap.add_argument("--stocks", type=int, default=5000)
    ap.add_argument("--industries", type=int, default=31)
    ap.add_argument("--styles", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-chunk", type=int, default=504)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "box_qp_bench.log"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("box_qp_bench needs a GPU: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for dtype in (torch.float64, torch.float32):
            r = bench(a.dates, a.stocks, a.industries, a.styles, dtype, a.reps, dev,
                      a.torch_chunk, a.torch_reps)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
