"""Timing of ops/pure_factor.py (csrc/pure_factor.hip): estimator covariance, pure factor
portfolios and factor-return t-statistics, against what the library could do before them.

    python tools/pure_factor_bench.py [--dates 2520] [--stocks 5000]
                                      [--out profiles/r11/pure_factor_bench.log]

For an fp64 and an fp32 synthetic panel (P = 31 industries, Q = 10 styles, 1 % missing) the
regression is run once (untimed); then, after a warm-up call, ``reps`` calls of each function are
timed between device synchronisations and the median is reported:

  * ``estimator_cov`` (two Gram passes + the per-date Jacobi kernel), and the Jacobi kernel alone;
  * ``pure_factor_weights`` for the styles (S = Q) and for all factors (S = K), with the achieved
    write bandwidth ``D S N 8 / t``;
  * ``factor_return_stats``;
  * the same Omega from the kernels the library already had: ceil(S / 8) ``factor_apply`` passes
    with u = 0, v = sqrt(cap), c = the rows of C (8 right-hand sides per pass); the two results
    must agree to 1e-12 of each date's max |Omega|, or the run fails.

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


def bench(D, N, P, Q, dtype, reps, dev):
    from llm_driven_multi_factor_model_amd import _native
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
    from llm_driven_multi_factor_model_amd.ops import pure_factor as pf
    from llm_driven_multi_factor_model_amd.ops.cross_section import xs_wls
    p = synthetic_panel(D, N, P, Q, seed=3, device=dev, missing_frac=0.01, dtype=dtype)
    K = p.K
    r = xs_wls(p.styles, p.cap, p.ret, p.ind, P)
    args = (p.styles, p.cap, p.ret, p.ind, r.stats, P)
    torch.cuda.synchronize(dev)
    out = {"D": D, "N": N, "K": K, "panel": str(dtype).replace("torch.", ""), "reps": reps}

    out["estimator_cov_ms"] = _ms(_timed(lambda: pf.estimator_cov(*args), reps, dev))
    est = pf.estimator_cov(*args)
    c64 = p.cap.to(torch.float64)
    G = fc.factor_gram(*args, torch.sqrt(c64))
    Gs = fc.factor_gram(*args, c64)
    Cs, rk = torch.empty_like(est.C), torch.empty_like(est.rank)
    out["est_cov_kernel_ms"] = _ms(_timed(lambda: _native.call(
        "mfa_est_cov", _native.ptr(G), _native.ptr(Gs), _native.ptr(r.stats), D, P, Q, 0,
        _native.ptr(Cs), _native.ptr(rk), _native.stream(dev)), reps, dev))
    out["factor_gram_ms"] = _ms(_timed(lambda: fc.factor_gram(*args, c64), reps, dev))
    out["rank_hist"] = {int(k): int((est.rank == k).sum()) for k in est.rank.unique().tolist()}
    out["nan_dates"] = int(torch.isnan(est.C).any(-1).any(-1).sum())
    out["factor_return_stats_ms"] = _ms(_timed(
        lambda: pf.factor_return_stats(*args, r.f, r.resid, est), reps, dev))
    fs = pf.factor_return_stats(*args, r.f, r.resid, est)
    t = fs.t[:, 1 + P:].abs()
    out["styles_share_abs_t_gt_2"] = [round(float(x), 4) for x in (t > 2).double().mean(0)]

    zeros = torch.zeros(D, N, dtype=torch.float64, device=dev)
    v = torch.sqrt(torch.where(torch.isfinite(c64) & (c64 >= 0), c64, torch.zeros_like(c64)))
    for name, sel in (("styles", list(range(1 + P, K))), ("all", list(range(K)))):
        S = len(sel)
        res = {"S": S}
        t1 = _timed(lambda: pf.pure_factor_weights(*args, est.C, sel), reps, dev)
        res["pure_factor_weights_ms"] = _ms(t1)
        res["write_GBps"] = round(D * S * N * 8 / (t1[0] * 1e-3) / 1e9, 1)
        om = pf.pure_factor_weights(*args, est.C, sel)
        crow = est.C[:, sel].contiguous()
        rhs = torch.zeros(D, S, N, dtype=torch.float64, device=dev)

        def compose():
            return fc.factor_apply(*args, zeros, v, rhs, crow)
        t2 = _timed(compose, reps, dev)
        res["factor_apply_composition_ms"] = _ms(t2)
        res["factor_apply_passes"] = -(-S // fc.APPLY_NB)
        res["composition_write_GBps"] = round(D * S * N * 8 / (t2[0] * 1e-3) / 1e9, 1)
        res["speedup_over_composition"] = round(t2[0] / t1[0], 2)
        ref = compose()
        scale = om.abs().amax((1, 2))
        fin = torch.isfinite(scale) & (scale > 0)
        err = ((om - ref).abs().amax((1, 2)) / scale)[fin]
        res["worst_diff_vs_composition"] = float(err.max())
        res["dates_compared"] = int(fin.sum())
        if not float(err.max()) <= 1e-12:
            raise SystemExit(f"pure_factor_weights differs from the factor_apply composition by "
                             f"{float(err.max()):.3e} of a date's max (bound 1e-12)")
        del om, ref, rhs
        torch.cuda.empty_cache()
        out[name] = res
        print(f"[pure_factor_bench] {out['panel']} {name} done", file=sys.stderr, flush=True)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--dates", type=int, default=2520)
    ap.add_argument("--stocks", type=int, default=5000)
    ap.add_argument("--industries", type=int, default=31)
    ap.add_argument("--styles", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11",
                                                  "pure_factor_bench.log"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pure_factor_bench needs a GPU: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for dtype in (torch.float64, torch.float32):
            r = bench(a.dates, a.stocks, a.industries, a.styles, dtype, a.reps, dev)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
