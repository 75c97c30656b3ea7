"""Timing of the trading-cost path of RiskModel.optimize (ops/tcost_qp.py, csrc/tcost_qp.hip)
against the cost-free path of the same process.

    python tools/tcost_qp_bench.py [--dates 2520] [--stocks 5000]
                                   [--out profiles/r14/tcost_qp_bench.log]

One fp64 synthetic panel (P = 31 industries, Q = 10 styles, 1 % missing), one RiskModel run
(untimed), its shrunk specific volatility precomputed, ``which="vra"``.  Every figure is the
median of ``reps`` calls after a warm-up call, timed between device synchronisations.

  * projection alone, on the trial after the first step of the 2 % cap problem: ``tc_project``
    with kappa = 0 (it computes the ``h`` of ``box_project``, so the ratio is the price of the
    two extra rows) and with kappa = 2e-5 against ``box_project`` on the same inputs, with the
    rows resident and re-streamed;
  * the whole call: ``optimize(upper=0.02, prev=p, tcost=2e-5)``, p = the previous date's
    cost-free solution, against ``optimize(upper=0.02)``, with the histogram of ``passes`` and
    of ``status`` (1 = MAX_PASSES) of each and the turnover with and without the cost;
  * ``rebalance(upper=0.02, tcost=2e-5)`` over the same panel, run once: the wall time as it is
    (a sequential loop of one-date solves).
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


def bench(D, N, P, Q, reps, dev, kappa, rebalance):
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.ops import box_qp as bq
    from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
    from llm_driven_multi_factor_model_amd.ops import tcost_qp as tc
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(D, N, P, Q, seed=3, device=dev, missing_frac=0.01, dtype=torch.float64)
    m = RiskModel(p, preset("reference", eigen_sims=10)).run()
    sv = m.specific_risk_shrunk()
    torch.cuda.synchronize(dev)
    out = {"D": D, "N": N, "K": p.K, "panel": "float64", "reps": reps, "kappa": kappa,
           "upper": 0.02}
    kw = dict(upper=0.02, which="vra", specific_vol=sv)
    base = m.optimize(**kw)
    prev = torch.nan_to_num(base.weights).roll(1, 0)
    prev[0] = 0.0

    # the projection alone, on the trial after the first step
    args = (p.styles, p.cap, p.ret, p.ind, m.stats, p.P)
    pb = bq.make_problem(*args, m.vra_cov, sv, None, 0.0, 0.02)
    st, pj = bq.new_state(D, p.K, dev), bq.new_projection(D, N, dev)
    bq.run_pass(pb, st, pj, 1e-10)
    c = st.c[:, None, :].contiguous()
    u = fc.factor_apply(*args, pb.a, -pb.a, pb.q[:, None], c)[:, 0].contiguous()
    sb, stc = bq.new_projection(D, N, dev), tc.new_tc_projection(D, N, dev)
    zero, kap = torch.zeros_like(u), torch.full_like(u, kappa)
    box = (u, pb.a, pb.lo, pb.hi, pb.budget)

    def tcp(k, **kws):
        return lambda: tc.tc_project(*box, prev, k, pb.q, pj.gamma, st.status, out=stc, **kws)
    steps = {
        "box_project (resident)": lambda: bq.box_project(*box, pb.q, pj.gamma, st.status,
                                                          out=sb),
        "box_project (re-streamed)": lambda: bq.box_project(*box, pb.q, pj.gamma, st.status,
                                                            out=sb, stream_rows=True),
        "tc_project kappa=0 (resident)": tcp(zero),
        "tc_project kappa=0 (re-streamed)": tcp(zero, stream_rows=True),
        "tc_project kappa>0 (resident)": tcp(kap),
        "tc_project kappa>0 (re-streamed)": tcp(kap, stream_rows=True),
    }
    out["project_ms"] = {k: round(_timed(f, reps, dev)[0], 3) for k, f in steps.items()}
    pm = out["project_ms"]
    out["tc_over_box_resident"] = round(
        pm["tc_project kappa=0 (resident)"] / pm["box_project (resident)"], 3)
    out["tc_over_box_streamed"] = round(
        pm["tc_project kappa=0 (re-streamed)"] / pm["box_project (re-streamed)"], 3)
    hb = bq.box_project(*box, pb.q, pj.gamma, st.status).h
    ht = tc.tc_project(*box, prev, zero, pb.q, pj.gamma, st.status).proj.h
    out["kappa0_h_equals_box_project"] = bool(torch.equal(hb, ht))
    print("[tcost_qp_bench] projection done", file=sys.stderr, flush=True)

    # the whole call
    out["optimize_ms"] = _ms(_timed(lambda: m.optimize(**kw), reps, dev))
    out["optimize_tcost_ms"] = _ms(_timed(
        lambda: m.optimize(prev=prev, tcost=kappa, **kw), reps, dev))
    r = m.optimize(prev=prev, tcost=kappa, **kw)
    for name, res in (("optimize", base), ("optimize_tcost", r)):
        out[name + "_passes_hist"] = _hist(res.passes)
        out[name + "_status_hist"] = _hist(res.status)
        out[name + "_max_passes_dates"] = int((res.status == bq.MAX_PASSES).sum())
    live = (base.status == bq.OK) & (r.status == bq.OK)
    live[0] = False
    free = (base.weights - prev).abs().sum(-1)[live]
    out["turnover_median"] = {"cost_free": round(float(free.median()), 4),
                              "tcost": round(float(r.turnover[live].median()), 4)}
    print("[tcost_qp_bench] optimize done", file=sys.stderr, flush=True)

    if rebalance:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        rb = m.rebalance(tcost=kappa, **kw)
        torch.cuda.synchronize(dev)
        out["rebalance_s"] = round(time.perf_counter() - t0, 2)
        out["rebalance_status_hist"] = _hist(rb.status)
        ok = rb.status == bq.OK
        out["rebalance_turnover_median"] = round(float(rb.turnover[ok][1:].median()), 4)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--dates", type=int, default=2520)
    ap.add_argument("--stocks", type=int, default=5000)
    ap.add_argument("--industries", type=int, default=31)
    ap.add_argument("--styles", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kappa", type=float, default=2e-5)
    ap.add_argument("--no-rebalance", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "tcost_qp_bench.log"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tcost_qp_bench needs a GPU: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    r = bench(a.dates, a.stocks, a.industries, a.styles, a.reps, dev, a.kappa,
              not a.no_rebalance)
    line = json.dumps(r)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
