"""Timing of RiskModel.min_variance (ops/factor_cov.py, csrc/factor_cov.hip) against the same
Woodbury algebra written with torch ops on the GPU.

    python tools/factor_cov_bench.py [--dates 2520] [--stocks 5000]
                                     [--out profiles/r07/factor_cov_bench.log]

For an fp64 and an fp32 synthetic panel (P = 31 industries, Q = 10 styles, 1 % missing) one
RiskModel is run once (untimed); then, after a warm-up call, ``reps`` calls of
``min_variance(which="vra", specific_vol=<precomputed shrunk vol>)`` are timed between device
synchronisations and the median is reported, together with

  * the median time of each step (a = 1 / s^2, Gram, X^T h, eigh + inner solve, apply), from
    separately synchronised calls;
  * the bytes the panel passes move (the Gram kernel, the X^T h kernel that forms g, and the
    apply kernel each stream the panel once) and the resulting TB/s over the whole call;
  * the torch-op formulation (dense X_d per chunk of dates, batched matmul, torch.linalg.eigh /
    cholesky), at the largest date chunk of the list that fits, and its worst difference from the
    HIP result.
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


def torch_min_variance(p, stats, F, sv, chunk):
    """The algebra of ops.factor_cov.solve_cov for b = 1 with torch ops, ``chunk`` dates at a time
    (materialises X_d [chunk, N, K])."""
    from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
    from llm_driven_multi_factor_model_amd.ops.cross_section import valid_mask
    D, N, K = p.D, p.N, p.K
    ys = []
    eye = torch.eye(K, dtype=torch.float64, device=F.device)
    for lo in range(0, D, chunk):
        sl = slice(lo, lo + chunk)
        X, cap, ret, ind = p.styles[sl], p.cap[sl], p.ret[sl], p.ind[sl]
        a, _ = fc._weights(X, cap, ret, ind, p.P, sv[sl], None)
        m = valid_mask(X, cap, ret, ind, p.P) & (a > 0)
        a = torch.where(m, a, torch.zeros_like(a))
        Xd = fc.design_matrix(X, cap, ret, ind, torch.nan_to_num(stats[sl]), p.P, m)
        aX = a[..., None] * Xd
        G = Xd.transpose(1, 2) @ aX
        g = aX.sum(1)
        Fc = F[sl]
        ok = torch.isfinite(Fc).all(-1).all(-1) & torch.isfinite(stats[sl]).all(-1)
        w, U = torch.linalg.eigh(torch.where(ok[:, None, None], Fc, eye))
        R = U * torch.sqrt(w.clamp(min=0.0))[:, None, :]
        M = eye + R.transpose(1, 2) @ G @ R
        L, _ = torch.linalg.cholesky_ex(torch.where(ok[:, None, None], M, eye))
        c = R @ torch.cholesky_solve(R.transpose(1, 2) @ g[..., None], L)
        y = a * (1.0 - (Xd @ c)[..., 0])
        ys.append(torch.where(ok[:, None], y, torch.full_like(y, float("nan"))))
    y = torch.cat(ys)
    tot = y.sum(-1)
    return y / tot[:, None], 1.0 / tot


def bench(D, N, P, Q, dtype, reps, dev, chunks):
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel
    from llm_driven_multi_factor_model_amd.ops import eigen
    from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
    from llm_driven_multi_factor_model_amd.utils.config import preset
    p = synthetic_panel(D, N, P, Q, seed=3, device=dev, missing_frac=0.01, dtype=dtype)
    m = RiskModel(p, preset("reference", eigen_sims=10)).run()
    sv = m.specific_risk_shrunk()
    torch.cuda.synchronize(dev)
    K, es = p.K, p.styles.element_size()
    out = {"D": D, "N": N, "K": K, "panel": str(dtype).replace("torch.", ""), "reps": reps}

    med, lo, hi = _timed(lambda: m.min_variance("vra", sv), reps, dev)
    out["min_variance_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
    # bytes per (date, stock) of the three panel passes: panel (Q styles + cap + ret) + int16
    # industry, plus a (Gram), a o b (xty), u, v, rhs in and out (apply)
    panel = (Q + 2) * es + 2
    passes = {"gram": panel + 8, "xty": panel + 8, "apply": panel + 4 * 8}
    total = sum(passes.values()) * D * N
    out["pass_bytes"] = {k: v * D * N for k, v in passes.items()}
    out["pass_bytes_total"] = total
    out["TBps_over_whole_call"] = round(total / (med * 1e-3) / 1e12, 3)

    args = (p.styles, p.cap, p.ret, p.ind, m.stats, p.P)
    a, _ = fc._weights(*args[:4], p.P, sv, None)
    ones = torch.ones(D, 1, N, dtype=torch.float64, device=dev)
    G = fc.factor_gram(*args, a)
    g = fc.factor_xty(*args, a[:, None])
    c = fc.woodbury_coef(G, m.vra_cov, g)
    steps = {
        "weights a = 1/s^2 (torch elementwise)": lambda: fc._weights(*args[:4], p.P, sv, None),
        "factor_gram": lambda: fc.factor_gram(*args, a),
        "factor_xty (g)": lambda: fc.factor_xty(*args, a[:, None]),
        "eigh(F)": lambda: eigen.eigh(m.vra_cov),
        "woodbury_coef (eigh + inner solve)": lambda: fc.woodbury_coef(G, m.vra_cov, g),
        "factor_apply": lambda: fc.factor_apply(*args, a, -a, ones, c),
    }
    out["step_ms"] = {k: round(_timed(f, reps, dev)[0], 3) for k, f in steps.items()}
    for k, name in (("gram", "factor_gram"), ("xty", "factor_xty (g)"),
                    ("apply", "factor_apply")):
        out.setdefault("pass_TBps", {})[k] = round(
            out["pass_bytes"][k] / (out["step_ms"][name] * 1e-3) / 1e12, 3)

    ref = m.min_variance("vra", sv)
    for chunk in chunks:
        try:
            tw, tv = torch_min_variance(p, m.stats, m.vra_cov, sv, chunk)
            med_t, lo_t, hi_t = _timed(lambda: torch_min_variance(p, m.stats, m.vra_cov, sv, chunk),
                                       max(3, reps // 2), dev)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            continue
        fin = torch.isfinite(ref.weights).all(-1) & torch.isfinite(tw).all(-1)
        diff = ((tw - ref.weights)[fin].abs().amax(-1) / ref.weights[fin].abs().amax(-1)).max()
        out["torch_ops"] = {"date_chunk": chunk, "median_ms": round(med_t, 3),
                            "min_ms": round(lo_t, 3), "max_ms": round(hi_t, 3),
                            "finite_dates": int(fin.sum()),
                            "worst_rel_diff_vs_hip": float(diff)}
        out["hip_speedup_over_torch_ops"] = round(med_t / med, 2)
        break
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--dates", type=int, default=2520)
    ap.add_argument("--stocks", type=int, default=5000)
    ap.add_argument("--industries", type=int, default=31)
    ap.add_argument("--styles", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "factor_cov_bench.log"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("factor_cov_bench needs a GPU: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for dtype in (torch.float64, torch.float32):
            r = bench(a.dates, a.stocks, a.industries, a.styles, dtype, a.reps, dev,
                      chunks=(256, 128, 64, 32, 16))
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
