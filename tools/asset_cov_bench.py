"""Timing of ops.asset_cov.asset_cov (csrc/asset_cov.hip) against the same algebra written with
torch ops on the same GPU.

    python tools/asset_cov_bench.py [--dates 2520] [--stocks 5000] [--out LOG]

One synthetic panel per dtype (P = 31 industries, Q = 10 styles, 1 % missing), its ``stats`` from
``xs_wls``, a random positive definite F per date and random specific volatilities.  For a static
basket of M = 50 / 300 / 1000 random names (all dates at M <= 300, the last tenth of them at
M = 1000, so that the output fits) and fp64 / fp32 panels, every figure is the median of 7 calls
after a warm-up call, timed between device synchronisations:

  * ``kernel``: ``asset_cov()`` (index check, scratch and output allocation, both kernels);
  * ``torch``: gather the members' raw rows, build their dense design rows (``design_matrix``),
    ``torch.bmm`` twice and a diagonal add; ``torch_bmm`` is the two ``bmm`` and the add alone,
    on design rows built beforehand.  The torch path neither mirrors a triangle nor writes NaN;
  * ``copy``: a plain ``cov.copy_()`` of the same size (one read and one write of the output),
    its rate, and ``write_floor``: the time the output write alone would take at that rate,
    with its share of the kernel's time.

Nothing is timed unless the kernel and the torch path agree within the bound of
tests/test_asset_cov.py on every entry of the valid members: 1e-12 S_ij with
S = |Z| |F| |Z|^T + s^2 on the diagonal.
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

REPS = 7
REL = 1e-12


def _timed(fn, dev):
    fn()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
            "max": round(max(ts), 3)}


def _design_rows(panel, stats, P, s, index):
    """(Z [D, M, K], s^2 [D, M], valid [D, M]) of the gathered members, with torch ops."""
    from llm_driven_multi_factor_model_amd.ops import factor_cov as fc
    from llm_driven_multi_factor_model_amd.ops.cross_section import valid_mask
    X, cap, ret, ind = panel
    D, Q, _ = X.shape
    M = index.shape[0]
    at = index[None, :].expand(D, M)
    Xg = X.gather(2, at[:, None, :].expand(D, Q, M))
    capg, retg, indg = cap.gather(1, at), ret.gather(1, at), ind.gather(1, at)
    sg = s[index][None, :].expand(D, M)
    valid = valid_mask(Xg, capg, retg, indg, P) & torch.isfinite(sg) & (sg > 0)
    Z = fc.design_matrix(Xg, capg, retg, indg, stats, P, valid)
    return Z, torch.where(valid, sg * sg, torch.zeros_like(sg)), valid


def _bmm_path(Z, F, s2):
    cov = torch.bmm(torch.bmm(Z, F), Z.transpose(1, 2))
    torch.diagonal(cov, dim1=1, dim2=2).add_(s2)
    return cov


def run(D, N, dtype, Ms, dev, log):
    from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
    from llm_driven_multi_factor_model_amd.ops import asset_cov as ac
    from llm_driven_multi_factor_model_amd.ops.cross_section import xs_wls
    P, Q = 31, 10
    K = 1 + P + Q
    p = synthetic_panel(D, N, P, Q, seed=1, device=dev, missing_frac=0.01, dtype=dtype)
    stats = xs_wls(p.styles, p.cap, p.ret, p.ind, P).stats.double()
    g = torch.Generator(device=dev).manual_seed(2)
    A = 0.01 * torch.randn(D, 3 * K, K, generator=g, device=dev, dtype=torch.float64)
    F = A.transpose(1, 2) @ A / (3 * K)
    s = 0.01 + 0.03 * torch.rand(N, generator=g, device=dev, dtype=torch.float64)
    for M in Ms:
        d0 = 0 if M <= 300 else D - max(1, D // 10)
        q = p.slice_dates(d0, D)
        panel = (q.styles, q.cap, q.ret, q.ind)
        st, Fq = stats[d0:], F[d0:].contiguous()
        Dq = D - d0
        index = torch.randperm(N, generator=g, device=dev)[:M]
        call = lambda corr=False: ac.asset_cov(*panel, st, P, Fq, s, index,   # noqa: E731
                                               correlation=corr)
        full = lambda: _torch_full(panel, st, P, s, index, Fq)                # noqa: E731
        # agreement first
        got = call()
        Z, s2, valid = _design_rows(panel, st, P, s, index)
        ref = _bmm_path(Z, Fq, s2)
        S = _bmm_path(Z.abs(), Fq.abs(), s2)
        assert torch.equal(got.valid, valid), "valid members differ"
        vv = valid[:, :, None] & valid[:, None, :]
        assert torch.equal(torch.isnan(got.cov), ~vv), "NaN pattern"
        err = torch.where(vv, (got.cov - ref).abs() / S.clamp(min=1e-300), torch.zeros_like(S))
        worst = err.max().item()
        if not worst <= REL:
            raise SystemExit(f"kernel and torch path disagree: {worst:.3e} S > {REL:.0e} S "
                             f"(M = {M}, {dtype}); nothing timed")
        sym = torch.equal(torch.nan_to_num(got.cov), torch.nan_to_num(got.cov).transpose(1, 2))
        del ref, S, err, vv
        nbytes = got.cov.numel() * 8
        dst = torch.empty_like(got.cov)
        t_copy = _timed(lambda: dst.copy_(got.cov), dev)
        del dst
        rate = 2 * nbytes / (t_copy["median"] * 1e-3)            # bytes / s, read + write
        t_k = _timed(call, dev)
        t_kc = _timed(lambda: call(True), dev)
        del got
        t_t = _timed(full, dev)
        t_b = _timed(lambda: _bmm_path(Z, Fq, s2), dev)
        floor = nbytes / rate * 1e3
        rec = {"panel": str(dtype).replace("torch.", ""), "dates": Dq, "stocks": N, "M": M,
               "K": K, "out_GB": round(nbytes / 1e9, 3), "worst_err_S": float(f"{worst:.3e}"),
               "symmetric": sym, "kernel_ms": t_k, "kernel_correlation_ms": t_kc,
               "torch_ms": t_t, "torch_bmm_ms": t_b, "copy_ms": t_copy,
               "copy_TBps": round(rate / 1e12, 3), "write_floor_ms": round(floor, 3),
               "write_floor_share": round(floor / t_k["median"], 3),
               "torch_over_kernel": round(t_t["median"] / t_k["median"], 2),
               "torch_bmm_over_kernel": round(t_b["median"] / t_k["median"], 2)}
        line = json.dumps(rec)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()
        del Z, s2, valid
        torch.cuda.empty_cache()


def _torch_full(panel, st, P, s, index, F):
    Z, s2, _ = _design_rows(panel, st, P, s, index)
    return _bmm_path(Z, F, s2)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dates", type=int, default=2520)
    ap.add_argument("--stocks", type=int, default=5000)
    ap.add_argument("--baskets", default="50,300,1000")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("asset_cov_bench needs a GPU")
    dev = torch.device("cuda")
    Ms = [int(m) for m in a.baskets.split(",") if m.strip()]
    log = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        log = open(a.out, "a")
    print(f"# {torch.cuda.get_device_name(dev)}, torch {torch.__version__}, median of {REPS} "
          f"calls after a warm-up", flush=True)
    for dtype in (torch.float64, torch.float32):
        run(a.dates, a.stocks, dtype, Ms, dev, log)
    if log:
        log.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
