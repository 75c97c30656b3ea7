"""Where the risk-attribution stage spends its time (1 GPU, 2520 x 5000 fp64 panel): each
sub-step of RiskModel.risk_attribution timed with HIP events (median of 5).

``--bayes-shrink [CALLS]``: only ``bayes_shrink`` (the cap-decile shrink kernel of
csrc/xs_reduce.hip) on the stage's own inputs, median / min / max of CALLS (7) calls after a
warm-up.

``--specific-risk``: the specific-risk model (csrc/specific_risk.hip): ``ewnw_vol`` at window
252 with 0 and 5 lags, ``spec_bias2`` and the whole ``specific_risk_use4`` call, next to two
baselines of the same run: the ``trailing_vol`` kernel and the EW Newey-West algebra written
with torch ops on the GPU (median / min / max of 7 calls after a warm-up)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel  # noqa: E402
from llm_driven_multi_factor_model_amd.models.risk_model import RiskModel  # noqa: E402
from llm_driven_multi_factor_model_amd.ops import attribution as attr  # noqa: E402
from llm_driven_multi_factor_model_amd.ops.xs_reduce import bayes_shrink  # noqa: E402
from llm_driven_multi_factor_model_amd.parallel import dist as pdist  # noqa: E402
from llm_driven_multi_factor_model_amd.utils.config import preset  # noqa: E402

dev = torch.device("cuda:0")
p = synthetic_panel(2520, 5000, 31, 10, seed=3, device=dev, missing_frac=0.01, dtype=torch.float64)
m = RiskModel(p, preset("reference")).run()
h = torch.full((p.N,), 1.0 / p.N, device=dev, dtype=torch.float64)


def t(fn, n=5, spread=False):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    v = []
    for _ in range(n):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        v.append(e0.elapsed_time(e1))
    if spread:
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                "max_ms": round(max(v), 4), "calls": n}
    return round(statistics.median(v), 3)


e = m.specific_ret.double()
halo = pdist.halo_prev_rows(e, 251, m.ctx, m.sizes)
vol = attr.trailing_vol(halo, e, 252, 1)
if "--bayes-shrink" in sys.argv:
    i = sys.argv.index("--bayes-shrink")
    calls = int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 7
    print(json.dumps({"bayes_shrink": t(lambda: bayes_shrink(vol, p.cap.double(), 10, 1.0), calls, True)}))
    sys.exit(0)
if "--specific-risk" in sys.argv:
    from llm_driven_multi_factor_model_amd.ops import specific_risk as sr

    def ewnw_torch(lags, W=252, hl=84.0):
        """The two-pass algebra of ops/specific_risk.py with torch ops on the device."""
        return sr._ewnw_vol_cpu(halo, e, W, sr.ew_weights(W, hl).tolist(), lags, 1)

    sig = m.specific_risk_use4()
    cap = p.cap
    v5 = sr.ewnw_vol(halo, e, 252, 84.0, 5)
    err = ((ewnw_torch(5) - v5).abs() / v5.abs().clamp(min=1e-300))
    res = {
        "shape": [p.D, p.N], "window": 252, "half_life": 84.0,
        "trailing_vol": t(lambda: attr.trailing_vol(halo, e, 252, 1), 7, True),
        "ewnw_vol_lags0": t(lambda: sr.ewnw_vol(halo, e, 252, 84.0, 0), 7, True),
        "ewnw_vol_lags5": t(lambda: sr.ewnw_vol(halo, e, 252, 84.0, 5), 7, True),
        "ewnw_torch_lags0": t(lambda: ewnw_torch(0), 3, True),
        "ewnw_torch_lags5": t(lambda: ewnw_torch(5), 3, True),
        "ewnw_torch_vs_kernel_max_rel": float(torch.nan_to_num(err, nan=0.0).max()),
        "spec_bias2": t(lambda: sr.spec_bias2(e, sig, cap), 7, True),
        "specific_risk_use4": t(lambda: m.specific_risk_use4(), 7, True),
        "specific_risk_shrunk": t(lambda: m.specific_risk_shrunk(), 7, True),
    }
    print(json.dumps(res))
    sys.exit(0)
H = h[None, :].expand(p.D, -1).contiguous()
sv = m.specific_risk_shrunk()
x = attr.portfolio_exposure(p.styles, p.cap, p.ret, p.ind, H, m.stats, p.P)
svar = attr.portfolio_specific_var(H, sv)
res = {
    "specific_ret_double": t(lambda: m.specific_ret.double()),
    "halo": t(lambda: pdist.halo_prev_rows(e, 251, m.ctx, m.sizes)),
    "trailing_vol": t(lambda: attr.trailing_vol(halo, e, 252, 1)),
    "bayes_shrink": t(lambda: bayes_shrink(vol, p.cap.double(), 10, 1.0)),
    "h_expand": t(lambda: h[None, :].expand(p.D, -1).contiguous()),
    "portfolio_exposure": t(lambda: attr.portfolio_exposure(p.styles, p.cap, p.ret, p.ind, H, m.stats, p.P)),
    "portfolio_specific_var": t(lambda: attr.portfolio_specific_var(H, sv)),
    "risk_attribution_math": t(lambda: attr.risk_attribution(x, m.vra_cov, svar)),
    "total": t(lambda: m.risk_attribution(h)),
}
print(json.dumps(res))
