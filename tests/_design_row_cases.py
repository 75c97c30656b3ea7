"""Panels for the Q sweeps of the kernels that stream the raw panel (``csrc/design_row.h``).

The runtime Q of those kernels picks one template instantiation each, so a wrong dispatch case
is a wrong result for one Q only: the GPU-vs-CPU tests of ``factor_cov``, ``pure_factor``,
``bias_test`` and ``attribution`` therefore run Q = 1..16 (and the blocked Q > 16 of the exposure
kernel) on a panel where, on every date, one stock fails each clause of the regression's validity
rule and nothing else, and every other stock is valid.
"""
import dataclasses

import pytest
import torch

from llm_driven_multi_factor_model_amd.models.panel import synthetic_panel
from llm_driven_multi_factor_model_amd.ops.cross_section import valid_mask, xs_wls

SWEEP_D, SWEEP_N = 2, 300   # N = 300: two trips of a 256-thread loop (the second ragged), five
                            # 64-stock chunks (the last ragged)
SWEEP_QS = tuple(range(1, 17))
SWEEP_PS = (0, 3)
SWEEP_DTYPES = (torch.float32, torch.float64)


def sweep_params(qs=SWEEP_QS):
    """pytest params (P, Q, dtype) of a sweep."""
    return [pytest.param(P, Q, dt, id=f"p{P}-q{Q}-{'f32' if dt == torch.float32 else 'f64'}")
            for Q in qs for P in SWEEP_PS for dt in SWEEP_DTYPES]


def planted_panel(D, N, P, Q, dtype, seed=5):
    """(panel, planted [D, N] bool): a panel without missing cells where date d has, from stock
    (7 + 253 d) mod (N - 6) on, one stock each with a NaN in one style, a NaN cap, a negative cap,
    a NaN ret and (P > 0) industry -1 and industry P."""
    p = synthetic_panel(D, N, P, Q, seed=seed, missing_frac=0.0, dtype=dtype)
    styles, cap, ret = p.styles.clone(), p.cap.clone(), p.ret.clone()
    ind = None if p.ind is None else p.ind.clone()
    planted = torch.zeros(D, N, dtype=torch.bool)
    nan = float("nan")
    for d in range(D):
        n0 = (7 + 253 * d) % (N - 6)
        styles[d, (d + Q // 2) % Q, n0] = nan
        cap[d, n0 + 1] = nan
        cap[d, n0 + 2] = -cap[d, n0 + 2]
        ret[d, n0 + 3] = nan
        if P > 0:
            ind[d, n0 + 4] = -1
            ind[d, n0 + 5] = P
        planted[d, n0:n0 + (6 if P > 0 else 4)] = True
    p = dataclasses.replace(p, styles=styles, cap=cap, ret=ret, ind=ind)
    # the plants are the invalid stocks, and the only ones
    assert torch.equal(valid_mask(p.styles, p.cap, p.ret, p.ind, P), ~planted)
    return p, planted


def planted_stats(p):
    """stats of ``xs_wls`` for a planted panel: a finite row with sigma > 0 on every date."""
    stats = xs_wls(p.styles, p.cap, p.ret, p.ind, p.P).stats.to(torch.float64)
    assert torch.isfinite(stats).all() and (stats[:, p.Q] > 0).all()
    return stats


def assert_finite(*tensors):
    """A sweep case that compared NaN with NaN would prove nothing."""
    for t in tensors:
        assert torch.isfinite(t).all()
