"""Timing of RiskModel.risk_budget (ops/risk_budget.py, csrc/risk_budget.hip) against the same
iteration composed from what the library had before.

    python tools/risk_budget_bench.py [--dates 2520] [--stocks 5000] [--panel float64]
                                      [--out profiles/r15/risk_budget_bench.f64.log]

One synthetic panel (P = 31 industries, Q = 10 styles, 1 % missing), one RiskModel run
(untimed), its shrunk specific volatility precomputed, ``which="vra"``, equal budgets and
budgets 10^(2 rand).  Every figure is the median of ``reps`` calls after a warm-up call, timed
between device synchronisations.

  * the whole call ``risk_budget()``, with the histograms of ``passes``, ``rejected`` and
    ``status`` and the worst ``rc_gap``;
  * the composed iteration: the same method, start and accept / reject rule written with
    ``factor_xty`` (x = X^T y), ``factor_apply`` (Sigma y), ``factor_gram`` (G), ``factor_xty``
    (v), ``woodbury_coef`` (c), ``factor_apply`` (X c) and torch elementwise ops: five passes
    over the panel per step instead of two.  Nothing is timed unless its weights agree with the
    kernels' to 1e-8 of each date's largest weight;
  * each kernel alone, on the state two passes in (every solvable date still running), with the
    bytes it moves (compulsory traffic: every input read once, every output written once) and
    the resulting TB/s.
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


def composed(pb, tol=1e-9, max_passes=32, check_every=4, theta=0.1):
    """The iteration of ops/risk_budget.py from the kernels of factor_cov.hip and torch ops."""
    from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
    from llm_driven_multi_factor_model_amd.ops import risk_budget as rb
    zero = torch.zeros((), dtype=torch.float64, device=pb.bt.device)
    st0 = rb.new_state(pb)
    m = pb.bt > 0
    inU = m.double()
    bt1 = torch.where(m, pb.bt, zero + 1.0)
    Fz = torch.nan_to_num(pb.F)
    yt, ys = st0.y[1].clone(), st0.y[0].clone()
    D = yt.shape[0]
    phi = torch.full((D,), float("inf"), dtype=torch.float64, device=yt.device)
    lam, ysy_s, r_s = torch.zeros_like(phi), torch.zeros_like(phi), torch.zeros_like(phi)
    delta = torch.zeros_like(yt)
    mode = torch.zeros(D, dtype=torch.int32, device=yt.device)
    passes, rejected = torch.zeros_like(mode), torch.zeros_like(mode)
    status = pb.status0.clone()
    for it in range(1, max_passes + 1):
        run = status == rb.RUNNING
        x = fc.factor_xty(*pb.panel, yt[:, None])[:, 0]
        z = torch.einsum("dkl,dl->dk", Fz, torch.nan_to_num(x))
        Sy = fc.factor_apply(*pb.panel, pb.s2, inU, yt[:, None], z[:, None])[:, 0]
        y1 = torch.where(m, yt, zero + 1.0)
        by = pb.bt / y1
        g = torch.where(m, Sy - by, zero)
        a = torch.where(m, 1.0 / (pb.s2 + by / y1), zero)
        r = torch.where(m, (yt * Sy / bt1 - 1.0).abs(), zero).amax(-1)
        ysy = torch.where(m, yt * Sy, zero).sum(-1)
        phit = 0.5 * ysy - torch.where(m, pb.bt * torch.log(y1), zero).sum(-1)
        acc = (mode == rb.DAMPED) | ~(phit > phi + rb.REJECT * phi.abs())
        A, rej = run & acc, run & ~acc
        conv, newton = A & (r <= tol), A & ~(r <= tol)
        G = fc.factor_gram(*pb.panel, a)
        v = fc.factor_xty(*pb.panel, (a * g)[:, None])
        c = fc.woodbury_coef(G, pb.F, v)
        l2 = (torch.where(m, a * g * g, zero).sum(-1) - (v * c).sum(-1)[:, 0]).clamp(min=0.0)
        Xc = fc.factor_apply(*pb.panel, pb.s2, inU, torch.zeros_like(yt)[:, None], c)[:, 0]
        dn = -a * (g - Xc)
        ys = torch.where(A[:, None], yt, ys)
        phi = torch.where(A, phit, phi)
        ysy_s, r_s = torch.where(A, ysy, ysy_s), torch.where(A, r, r_s)
        lam = torch.where(newton, torch.sqrt(l2), lam)
        delta = torch.where(newton[:, None], dn, delta)
        mode = torch.where(newton, rb.CLAMPED, torch.where(rej, rb.DAMPED, mode)).to(torch.int32)
        t = 1.0 / (1.0 + pb.M * lam)
        nxt = torch.where((mode == rb.DAMPED)[:, None], ys + t[:, None] * delta,
                          torch.maximum(ys + delta, theta * ys))
        yt = torch.where((run & ~conv)[:, None], torch.where(m, nxt, zero), yt)
        passes = passes + run.to(torch.int32)
        rejected = rejected + rej.to(torch.int32)
        status = torch.where(conv, rb.OK, status).to(torch.int32)
        if check_every and it % check_every == 0 and it < max_passes \
                and int((status == rb.RUNNING).sum()) == 0:
            break
    status = torch.where(status == rb.RUNNING, rb.MAX_PASSES, status).to(torch.int32)
    dead = status >= rb.INFEASIBLE
    tot = ys.sum(-1)
    tot1 = torch.where(tot > 0, tot, torch.ones_like(tot))
    nan = zero + float("nan")
    w = torch.where(dead[:, None], nan, pb.budget[:, None] * ys / tot1[:, None])
    return rb.RiskBudget(w, torch.where(dead, nan, pb.budget ** 2 * ysy_s / (tot1 * tot1)),
                         torch.where(dead, nan, r_s), passes, rejected, status)


def bench(D, N, P, Q, reps, dev, dtype):
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.ops import risk_budget as rb
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(D, N, P, Q, seed=3, device=dev, missing_frac=0.01, dtype=dtype)
    m = RiskModel(p, preset("reference", eigen_sims=10)).run()
    sv = m.specific_risk_shrunk()
    torch.cuda.synchronize(dev)
    K = p.K
    es = 8 if dtype == torch.float64 else 4
    out = {"D": D, "N": N, "K": K, "panel": str(dtype).replace("torch.", ""), "reps": reps}
    args = (p.styles, p.cap, p.ret, p.ind, m.stats, p.P)
    g = torch.Generator(device="cpu").manual_seed(17)
    spread = (10.0 ** (2.0 * torch.rand(N, generator=g, dtype=torch.float64))).to(dev)
    for name, b in (("equal", None), ("spread", spread)):
        kw = dict(budgets=b, which="vra", specific_vol=sv)
        r = m.risk_budget(**kw)
        pb = rb.make_problem(*args, m.vra_cov, sv, b)
        ref = composed(pb)
        live = (r.status == rb.OK) & (ref.status == rb.OK)
        err = ((r.weights - ref.weights).abs().amax(-1) / r.weights.amax(-1))[live]
        o = {"status_hist": _hist(r.status), "passes_hist": _hist(r.passes[r.status == rb.OK]),
             "rejected_hist": _hist(r.rejected[r.status == rb.OK]),
             "rc_gap_max": float(r.rc_gap[r.status == rb.OK].max()),
             "composed_status_equal": bool(torch.equal(r.status, ref.status)),
             "composed_passes_equal": bool(torch.equal(r.passes, ref.passes)),
             "composed_weight_error_max": float(err.max())}
        if not (o["composed_status_equal"] and float(err.max()) <= 1e-8):
            raise SystemExit(f"risk_budget_bench: the kernels and the composed iteration "
                             f"disagree ({name}): {json.dumps(o)}; nothing timed")
        o["risk_budget_ms"] = _ms(_timed(lambda: m.risk_budget(**kw), reps, dev))
        o["composed_ms"] = _ms(_timed(lambda: composed(pb), reps, dev))
        o["setup_ms"] = _ms(_timed(lambda: rb.new_state(rb.make_problem(
            *args, m.vra_cov, sv, b)), reps, dev))
        o["speedup"] = round(o["composed_ms"]["median"] / o["risk_budget_ms"]["median"], 3)
        out[name] = o
        print(f"[risk_budget_bench] {name} done", file=sys.stderr, flush=True)

    # each kernel alone, two passes in
    pb = rb.make_problem(*args, m.vra_cov, sv, spread)
    st = rb.new_state(pb)
    mo = rb.new_moments(D, K, dev)
    for _ in range(2):
        rb.run_pass(pb, st, mo=mo)
    live = int((st.status == rb.RUNNING).sum())
    out["kernel_dates_running"] = live
    panel = (Q + 2) * N * es + (2 * N if P > 0 else 0)
    byts = {
        "rb_moments": live * (panel + 3 * 8 * N + 8 * (2 * K * K + 2 * K + 4)),
        "rb_step": live * 8 * (2 * K * K + 4 * K + 16),
        "rb_update": live * (panel + 3 * 8 * N + 8 * N + 8 * (K * K + 3 * K)),
    }
    s1, s2 = st.clone(), st.clone()
    rb.rb_moments(pb, st, mo)
    fns = {"rb_moments": lambda: rb.rb_moments(pb, st, mo),
           "rb_step": lambda: rb.rb_step(mo, pb.lam, pb.U, pb.M, s1, 1e-9),
           "rb_update": lambda: rb.rb_update(pb, s2)}
    out["kernels"] = {}
    for name, fn in fns.items():
        t = _timed(fn, reps, dev)
        out["kernels"][name] = {"ms": round(t[0], 3), "MB": round(byts[name] / 1e6, 1),
                                "TB/s": round(byts[name] / (t[0] * 1e-3) / 1e12, 3)}
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--dates", type=int, default=2520)
    ap.add_argument("--stocks", type=int, default=5000)
    ap.add_argument("--industries", type=int, default=31)
    ap.add_argument("--styles", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--panel", choices=("float64", "float32"), default="float64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("risk_budget_bench needs a GPU: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    tag = "f64" if a.panel == "float64" else "f32"
    path = a.out or os.path.join(ROOT, "profiles", "r15", f"risk_budget_bench.{tag}.log")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    r = bench(a.dates, a.stocks, a.industries, a.styles, a.reps, dev,
              torch.float64 if a.panel == "float64" else torch.float32)
    line = json.dumps(r)
    print(line, flush=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
