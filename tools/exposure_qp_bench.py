"""Timing of RiskModel.optimize(neutral=...) (ops/exposure_qp.py, eq_step_kernel in
csrc/box_qp.hip) against the same algorithm written with torch ops on the GPU.

    python tools/exposure_qp_bench.py [--dates 2520] [--stocks 5000]
                                      [--out profiles/r13/exposure_qp_bench.log]

For an fp64 synthetic panel (P = 31 industries, Q = 10 styles, 1 % missing) one RiskModel is run
once (untimed) and its shrunk specific volatility precomputed.  The problem is long-only with a
2 % cap, minimum tracking error to the cap-weighted benchmark, industry- and SIZE-neutral to it
(32 equality constraints).  First the HIP path and ``exposure_qp(..., torch_ops=True)`` (dense
X_d, einsum, torch.linalg.cholesky, in chunks of dates) are run once each and must agree: on the
dates both report ``OK`` the weights within 1e-8 of each date's largest weight, or the tool stops
before any timing.  Then, after a warm-up call, ``reps`` calls of ``optimize`` are timed between
device synchronisations and the median is reported with the histogram of ``passes``, the counts
of ``status``, the largest exposure gap on the ``OK`` dates, the median time of one ``eq_step``
launch and the timing of the torch-ops path.
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


def torch_optimize(p, stats, F, sv, sel, t, q, upper, chunk, max_passes):
    from llm_driven_multi_factor_model_amd.ops import exposure_qp as eq
    ws, ss = [], []
    for lo in range(0, p.D, chunk):
        sl = slice(lo, lo + chunk)
        r = eq.exposure_qp(p.styles[sl], p.cap[sl], p.ret[sl], p.ind[sl], stats[sl], p.P, F[sl],
                           sv[sl], sel, t[sl], q[sl], 0.0, upper, max_passes=max_passes,
                           torch_ops=True)
        ws.append(r.weights)
        ss.append(r.status)
    return torch.cat(ws), torch.cat(ss)


def bench(D, N, P, Q, dtype, reps, dev, chunk, torch_reps, max_passes):
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.ops import box_qp as bq
    from llm_driven_multi_factor_model_amd.ops import exposure_qp as eq
    from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(D, N, P, Q, seed=3, device=dev, missing_frac=0.01, dtype=dtype)
    m = RiskModel(p, preset("reference", eigen_sims=10)).run()
    sv = m.specific_risk_shrunk()
    args = (p.styles, p.cap, p.ret, p.ind, m.stats, p.P)
    U = fc.universe_mask(p.styles, p.cap, p.ret, p.ind, p.P, sv)
    hb = torch.where(U, p.cap.double(), torch.zeros((), dtype=torch.float64, device=dev))
    hb = hb / hb.sum(-1, keepdim=True)
    sel = list(range(1, 1 + P)) + [1 + P]          # industries + SIZE (style 0)
    upper = 0.02
    kw = dict(benchmark=hb, upper=upper, neutral=sel, which="vra", specific_vol=sv,
              max_passes=max_passes)
    torch.cuda.synchronize(dev)
    out = {"D": D, "N": N, "K": p.K, "m": len(sel), "panel": str(dtype).replace("torch.", ""),
           "reps": reps, "max_passes": max_passes}
    r = m.optimize(**kw)
    ok = r.status == bq.OK
    out["passes_hist"] = _hist(r.passes)
    out["status_counts"] = _hist(r.status)
    out["worst_exposure_gap_on_ok_dates"] = float(r.exposure_gap[ok].max()) if ok.any() else None
    # agreement with the torch-ops path before any timing
    q = fc.apply_cov(*args, m.vra_cov, sv, hb)
    t = fc.factor_xty(*args, hb[:, None])[:, 0][:, sel]
    tw, ts = torch_optimize(p, m.stats, m.vra_cov, sv, sel, t, q, upper, chunk, max_passes)
    both = ok & (ts == bq.OK)
    rel = (tw - r.weights)[both].abs().amax(-1) / r.weights[both].abs().amax(-1)
    out["ok_dates_both"] = int(both.sum())
    out["torch_ops_status_counts"] = _hist(ts)
    out["torch_ops_worst_rel_diff_on_ok_dates"] = float(rel.max()) if both.any() else None
    if not both.any() or not bool((rel <= 1e-8).all()):
        out["error"] = "the HIP and the torch-ops path disagree: nothing was timed"
        return out
    out["optimize_ms"] = _ms(_timed(lambda: m.optimize(**kw), reps, dev))
    # one eq_step launch on the second trial's inputs
    pb = bq.make_problem(*args, m.vra_cov, sv, q, 0.0, upper)
    pb, ep = eq.make_eq_problem(pb, m.vra_cov, sel, t)
    es, pj = eq.new_eq_state(D, p.K, dev), bq.new_projection(D, N, dev)
    G, x = bq.run_trial(pb, es.step, pj)
    eq.eq_step(G, ep, x, pj.stats, pj.flag, es, 1e-10)
    G, x = bq.run_trial(pb, es.step, pj)
    out["pass_ms"] = {
        "trial (apply, project, gram, xty)": round(_timed(
            lambda: bq.run_trial(pb, es.step, pj), reps, dev)[0], 3),
        "eq_step (incl. state clone)": round(_timed(
            lambda: eq.eq_step(G, ep, x, pj.stats, pj.flag, es.clone(), 1e-10), reps, dev)[0], 3),
        "state clone": round(_timed(lambda: es.clone(), reps, dev)[0], 3),
    }
    out["torch_ops_ms"] = _ms(_timed(
        lambda: torch_optimize(p, m.stats, m.vra_cov, sv, sel, t, q, upper, chunk, max_passes),
        torch_reps, dev))
    out["torch_ops_date_chunk"] = chunk
    out["hip_speedup_over_torch_ops"] = round(
        out["torch_ops_ms"]["median"] / out["optimize_ms"]["median"], 2)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--dates", type=int, default=2520)
    ap.add_argument("--stocks", type=int, default=5000)
    ap.add_argument("--industries", type=int, default=31)
    ap.add_argument("--styles", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--torch-chunk", type=int, default=504)
    ap.add_argument("--max-passes", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13",
                                                  "exposure_qp_bench.log"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("exposure_qp_bench needs a GPU: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    r = bench(a.dates, a.stocks, a.industries, a.styles, torch.float64, a.reps, dev,
              a.torch_chunk, a.torch_reps, a.max_passes)
    line = json.dumps(r)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 1 if "error" in r else 0


if __name__ == "__main__":
    raise SystemExit(main())
