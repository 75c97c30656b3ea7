"""Timing of ops.bias_test.portfolio_forecast (csrc/portfolio_batch.hip) against what the kernels
before it can do for the same numbers.

    python tools/bias_test_bench.py [--dates 2520] [--stocks 5000]
                                    [--out profiles/r10/bias_test_bench.log]

For an fp64 and an fp32 synthetic panel (P = 31 industries, Q = 10 styles, 1 % missing), static
weights [B, N] for B in {1, 16, 256, 1024}, a random SPD factor covariance per date and a random
specific volatility per (date, stock): after a warm-up call, ``reps`` calls are timed between
device synchronisations; median, min and max are reported, with the bytes the call has to move at
the least (the panel once per tile of 64 portfolios, s once per tile, H once) next to them.

Baseline (B = 16 and 256): blocks of 4 portfolios, each expanded and masked to [D, 4, N]
(``factor_xty`` takes per-date right-hand sides only, and applies the regression's validity rule
but not the specific-risk one), ``factor_xty`` for the exposures, torch ops for sum h^2 s^2,
sum h ret, sum |h| and the quadratic form.  B = 1024 would need 256 such passes and is not run
this way; the [D, B, N] copy that a single ``factor_xty`` call would take is 100 GB.  For B <= 4
one ``factor_xty`` pass over pre-expanded weights is timed for comparison.
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

TILE = 64


def _timed(fn, reps, dev):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
            "max": round(max(ts), 3)}


def baseline(args, H, F, s, m):
    """(factor_var, specific_var, realised, held) [D, B] through factor_xty, 4 portfolios a pass."""
    from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
    ret = args[2].double()
    s2 = s * s
    zero = torch.zeros((), dtype=torch.float64, device=H.device)
    outs = []
    for b0 in range(0, H.shape[0], fc.XTY_NB):
        Hb = torch.where(m[:, None, :], H[None, b0:b0 + fc.XTY_NB], zero)   # [D, 4, N]
        x = fc.factor_xty(*args, Hb)
        fv = torch.einsum("dbk,dkl,dbl->db", x, F, x)
        spec = torch.einsum("dbn,dn->db", Hb * Hb, s2)
        real = torch.einsum("dbn,dn->db", Hb, ret)
        outs.append((fv, spec, real, Hb.abs().sum(-1)))
    return [torch.cat(c, 1) for c in zip(*outs)]


def bench(D, N, P, Q, dtype, Bs, reps, dev):
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.ops import bias_test as bt
    from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
    from llm_driven_multi_factor_model_amd.ops.cross_section import xs_wls
    p = synthetic_panel(D, N, P, Q, seed=3, device=dev, missing_frac=0.01, dtype=dtype)
    stats = xs_wls(p.styles, p.cap, p.ret, p.ind, P, want_resid=False).stats
    args = (p.styles, p.cap, p.ret, p.ind, stats, P)
    K, es = p.K, p.styles.element_size()
    g = torch.Generator(device=dev).manual_seed(5)
    A = 0.01 * torch.randn(D, K, K, generator=g, device=dev, dtype=torch.float64)
    F = A @ A.transpose(1, 2)
    s = 0.01 + 0.03 * torch.rand(D, N, generator=g, device=dev, dtype=torch.float64)
    m = fc.universe_mask(*args[:4], P, s)
    Hall = torch.rand(max(Bs), N, generator=g, device=dev, dtype=torch.float64)
    for B in Bs:
        H = Hall[:B].contiguous()
        r = {"D": D, "N": N, "K": K, "panel": str(dtype).replace("torch.", ""), "B": B,
             "reps": reps}
        r["portfolio_forecast_ms"] = _timed(lambda: bt.portfolio_forecast(*args, H, F, s), reps,
                                            dev)
        tiles = (B + TILE - 1) // TILE
        least = tiles * D * N * ((Q + 2) * es + 2 + 8) + B * N * 8 + D * K * K * 8
        med = r["portfolio_forecast_ms"]["median"]
        r["least_bytes"] = least
        r["least_bytes_TBps"] = round(least / (med * 1e-3) / 1e12, 3)
        r["mfma_TFLOPs"] = round(2.0 * D * N * 16 * ((B + 15) // 16) * 16 * ((K + 15) // 16)
                                 / (med * 1e-3) / 1e12, 2)
        if B <= fc.XTY_NB:
            Hx = H[None].expand(D, B, N).contiguous()
            r["one_factor_xty_pass_ms"] = _timed(lambda: fc.factor_xty(*args, Hx), reps, dev)
            del Hx
        if B in (16, 256):
            r["baseline_ms"] = _timed(lambda: baseline(args, H, F, s, m), reps, dev)
            new = bt.portfolio_forecast(*args, H, F, s)
            old = baseline(args, H, F, s, m)
            r["worst_rel_diff_vs_baseline"] = max(
                float(((a - b).abs() / b.abs().clamp(min=1e-300)).max())
                for a, b in zip(new[:4], old))
            r["speedup_over_baseline"] = round(r["baseline_ms"]["median"] / med, 2)
            r["beats_baseline_beyond_spread"] = bool(
                r["baseline_ms"]["min"] > r["portfolio_forecast_ms"]["max"])
            del new, old
        yield r
        torch.cuda.empty_cache()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--dates", type=int, default=2520)
    ap.add_argument("--stocks", type=int, default=5000)
    ap.add_argument("--industries", type=int, default=31)
    ap.add_argument("--styles", type=int, default=10)
    ap.add_argument("--portfolios", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "bias_test_bench.log"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bias_test_bench needs a GPU: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for dtype in (torch.float64, torch.float32):
            for r in bench(a.dates, a.stocks, a.industries, a.styles, dtype, a.portfolios,
                           a.reps, dev):
                line = json.dumps(r)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
