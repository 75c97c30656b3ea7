"""Time-axis scan kernels (``csrc/ew_scan.hip``: ``nw_chunk_sums``, ``nw_carry_scan``, ``nw_emit``,
``ew_cumsum_cols``, ``ew_cumsum_tail``, ``ew_prefix_mean``) against plain high-precision numpy
oracles, at the edges of every kernel: series lengths each side of the 32-date chunks and of the
64-lane partition, K^2 each side of the 256-thread workgroup, the emission rule met exactly, lag
counts around the groups of 8 and beyond a chunk's dates, the lag counts at which the chunk halves
and the LDS limit, half-lives 0.5 .. 1e9, data that stresses the one-pass algebra, non-finite
input on chunk and shard boundaries, and every kind of shard cut.

The oracles are written from the reference's semantics (``mfm/utils.py:16-50`` evaluated on every
prefix by ``mfm/MFM.py:80-101``; the VRA multiplier of ``mfm/MFM.py:149-164``), not from
``ops/ew_scan.py``, in ``np.longdouble``:

* Newey-West at date t: n = t + 1 rows, weights ``0.5**(arange(n-1,-1,-1)/tau)`` normalised, the
  weighted mean removed, ``G0 = sum_s w_s r_s r_s^T``, ``G_i = sum_{s>=i} w_s r_{s-i} r_s^T``,
  ``V = G0 + sum_{i=1..q} (1 - i/(q+1)) (G_i + G_i^T)``; NaN where ``n <= q or n <= K`` (the
  reference raises there).  O(T^2 K^2 q): evaluated on every date when T <= 130 (all cases but
  the K = 56 ones, which take the last 10 dates -- with 4-date chunks each of them lies on or
  next to a chunk edge -- and the first emitted date).
* Prefix mean at date t: the same weights over the finite entries up to t, NaN where none is.

Project rules the oracles adopt:

* +-inf in the prefix-mean input counts as missing;
* a non-finite factor return in column k makes row and column k of V NaN from that date on; every
  other entry equals the oracle computed without column k;
* a column that is exactly constant over the prefix centres to exactly 0 (the longdouble weights
  sum to 1 only to 1e-19), so its row and column of V are exactly 0.

Every case runs through the CPU path (unmarked), the HIP single-launch scan (``gpu``) and the
shard path ``..._sharded(x[cut:], ..., history=x[:cut])`` on both devices, against the same oracle.

Constants transcribed from ``csrc/ew_scan.hip`` (asserted against ``mfa_nw_max_lags`` and by every
case that is meant to hit a chunk size): ``CH = 32`` dates per chunk (line 31), ``G = 8`` lags per
launch group (line 32), the 160 KB LDS image ``nw_lds_doubles(ch, K, q) = (2 (ch + q) + q) K +
ch (1 + G)`` doubles (``nw_lds_doubles``, line 359), ``nw_chunk``: CH halved down to 4 while the
image exceeds 160 KB (line 365), ``mfa_nw_max_lags``: the largest q whose 4-date image fits
(line 388); the 64-lane partition ``per = ceil(T / 64)`` of ``ew_cumsum_cols`` (line 275) and
``ew_prefix_mean`` (line 318).

Tolerance rule (that of ``test_xs_reduce_oracle.py`` and ``test_rolling_oracle.py``; no bound comes
from the output under test):

    |got - oracle| <= rtol * |oracle| + atol_case,     NaN and inf positions exactly equal.

``rtol``: the outputs are fp64 computed in fp64.  In units of u = 2**-53: ``nw_emit`` forms
``1 / Z(n)`` from two library calls documented at 1 ulp (2 u each) and a division (u), multiplies
S0 by it (u), subtracts the mean product (u) and stores / adds the lag groups' terms (u): 8 u,
``rtol = 4 eps64``.  ``ew_prefix_mean`` ends in the last fma of num, of den and one division:
3 u, ``rtol = 2 eps64``.

``atol_case`` is measured on the CPU from the inputs alone: the same quantity computed a second,
independent way in plain float64 numpy -- for Newey-West one-pass decayed uncentred moments with
``Z`` accumulated by summation, for the prefix mean a running num / den -- and 8 x its largest
deviation from the longdouble oracle, per case and per date (prefix mean: per case).  For
Newey-West the deviation is taken twice, in absolute terms and in units of ``sqrt(Q_k Q_l)``,
``Q_k = sum_s w_s f_sk^2`` over the prefix (the magnitude of the uncentred terms an entry is
formed from, so that columns of different scale are each held to their own), and an entry takes
the smaller of the two.  The floor is the rounding of the result itself: the same 8 u as ``rtol``
on the terms the one-pass result is the difference of, ``4 eps64 sqrt(Q_k Q_l)`` (``eps64 |oracle|``
for the prefix mean).  The second opinion shares the kernels' inherent conditioning (uncentred
one-pass moments, the rounded decay ``l = 0.5**(1/tau)``); it shares neither a closed-form
normaliser nor a backward recurrence for the halo rows, so losses from those are not excused.

Where the oracle is exactly 0 by construction (a zero or constant column) the second opinion may
hit 0 by luck and is not used; the bound there is analytic, ``c eps64 sqrt(Q_k Q_l)`` with
``c = 4 (1 + 2 q) (n + 2)``: V sums 1 + 2 q moments (G0, the G_i and their transposes, Bartlett
weights <= 1), each the difference of 4 products (A_i, a_i mu^T, mu b_i^T, z_i mu mu^T over Z),
each product bounded by ``sqrt(Q_k Q_l)`` (Cauchy-Schwarz) and carrying at most one rounding per
row of its n-row decayed sums plus two for its scaling: (n + 2) eps64.  A zero column has Q = 0:
its entries must be exactly 0.

Prefix-mean gaps of missing data are kept short enough that ``l**gap`` stays far above the fp64
denormals (<= 60 dates at tau = 0.5, 2**-120); beyond that the decayed count underflows, which is
outside what is tested.

The bound in force is printed by every assertion; the values measured when the cases were written
stand beside the cases.
"""
import functools

import numpy as np
import pytest
import torch

from llm_driven_multi_factor_model_amd import _native
from llm_driven_multi_factor_model_amd.ops import ew_scan as ES

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
RTOL_NW = 4 * EPS
RTOL_PM = 2 * EPS
NAN, INF = float("nan"), float("inf")

# ------------------------------------------------------------------ csrc/ew_scan.hip, transcribed
CH, G, LDS_BYTES = 32, 8, 160 * 1024


def nw_lds_doubles(ch, K, q):
    return (2 * (ch + q) + q) * K + ch * (1 + G)


def nw_chunk(K, q):
    ch = CH
    while ch > 4 and nw_lds_doubles(ch, K, q) * 8 > LDS_BYTES:
        ch >>= 1
    return ch


def nw_max_lags(K):
    q = 0
    while nw_lds_doubles(4, K, q + 1) * 8 <= LDS_BYTES:
        q += 1
    return q


def lag_groups(q):
    return max(1, -(-q // G))


def test_transcription_figures():
    """The figures the cases below rely on, from the transcription alone."""
    assert [nw_chunk(56, q) for q in (98, 99, 110, 111, 116, 117, 119)] == [32, 16, 16, 8, 8, 4, 4]
    assert nw_max_lags(56) == 119 and nw_max_lags(42) == 159
    assert nw_chunk(288, 2) == CH and nw_chunk(289, 2) == CH // 2
    assert [lag_groups(q) for q in (0, 1, 7, 8, 9, 16, 17, 32, 40)] == [1, 1, 1, 1, 2, 2, 3, 4, 5]
    assert nw_lds_doubles(4, 56, 119) * 8 <= LDS_BYTES < nw_lds_doubles(4, 56, 120) * 8


@pytest.mark.gpu
def test_max_lags_matches_transcription(cuda):
    for K in (1, 2, 17, 42, 56, 200, 288, 289):
        assert _native.query("mfa_nw_max_lags", K) == nw_max_lags(K), K


def test_docstring_lag_limit():
    """``ops/ew_scan.py`` quotes the lag limit at K = 42: the figure is the formula's."""
    assert f"{nw_max_lags(42)} at" in " ".join(ES.__doc__.split())


# ============================================================================== helpers
@pytest.fixture(params=[pytest.param("cpu"), pytest.param("hip", marks=pytest.mark.gpu)])
def mode(request):
    return request.param


def _device(mode, request):
    return torch.device("cpu") if mode == "cpu" else request.getfixturevalue("cuda")


def _t(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _close(got, want, atol, rtol, what):
    """``got`` (fp64) against the longdouble oracle ``want``; ``atol`` scalar or per element."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=LD)
    atol = np.broadcast_to(np.asarray(atol, dtype=np.float64), want.shape)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    dn = np.isnan(got) != np.isnan(want)
    assert not dn.any(), (f"{what}: NaN positions differ at {np.argwhere(dn)[:4].tolist()} "
                          f"({int(dn.sum())} entries), got there {got[dn][:4].tolist()}, "
                          f"oracle {want[dn][:4].astype(np.float64).tolist()}")
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf].astype(np.float64)), \
        f"{what}: inf positions"
    f = np.isfinite(want)
    err = np.abs(got[f].astype(LD) - want[f]).astype(np.float64)
    bound = rtol * np.abs(want[f]).astype(np.float64) + atol[f]
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if f.any() else 0.0
    bad = err > bound
    if bad.any():
        i = int(np.argmax(err - bound))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {int(f.sum())} outside rtol {rtol:.3g} + atol_case (max "
            f"{float(atol[f].max()):.3g}); worst |err| {err[i]:.3g} at oracle {float(want[f][i]):.6g} "
            f"(entry {np.argwhere(f)[i].tolist()}, bound {bound[i]:.3g}, err / bound up to {worst:.3g})")
    return worst


# ============================================================================== Newey-West
def _series(kind, T, K, seed):
    """``plain``: N(0, 0.01^2).  ``ar``: AR(1), coefficient 0.9.  ``stress`` (K = 6): mean 1 / std
    1e-2, exact zeros, an exact constant, AR(1), and two columns of scale 1e1 and 1e-5."""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((T, K)) * 0.01
    if kind in ("ar", "stress"):
        A = F.copy()
        for t in range(1, T):
            A[t] = 0.9 * A[t - 1] + F[t]
        if kind == "ar":
            return A
        assert K == 6
        F[:, 0] += 1.0
        F[:, 1] = 0.0
        F[:, 2] = 0.37
        F[:, 3] = A[:, 3]
        F[:, 4] *= 1e3
        F[:, 5] *= 1e-3
    return F


def _case(T, K, q, tau, kind="plain", cuts=None, put=(), windows=False, last=None, seed=None):
    """One hashable case.  ``put``: ((t, k, value), ...) non-finite entries; ``last``: evaluate the
    oracle on the last ``last`` dates only; ``cuts``: shard cuts (default: one near the middle)."""
    if cuts is None:
        cuts = (min(33, T - 1),) if T > 1 else ()
    cuts = tuple(sorted({c for c in cuts if 1 <= c <= T - 1}))
    seed = 1000 * T + 10 * K + q if seed is None else seed
    return (T, K, q, float(tau), kind, cuts, tuple(put), windows, last, seed)


def _id(c):
    T, K, q, tau, kind, cuts, put, windows, last, _ = c
    s = f"T{T}-K{K}-q{q}-tau{tau:g}-{kind}"
    if put:
        s += "-" + "-".join(f"{'nan' if v != v else 'inf'}@{t}" for t, _, v in put)
    return s + ("-win" if windows else "") + (f"-cuts{len(cuts)}" if len(cuts) > 1 else "")


def _input(c):
    T, K, q, tau, kind, cuts, put, windows, last, seed = c
    F = _series(kind, T, K, seed)
    for t, k, v in put:
        F[t, k] = v
    return F


def _dates(c):
    """The dates the oracle is evaluated on: all when T <= 130, else / with ``last`` the first
    emitted date, both sides of every chunk edge among the last dates, and the last date."""
    T, K, q, tau, kind, cuts, put, windows, last, seed = c
    if last is None:
        assert T <= 130
        return tuple(range(T))
    first = max(q, K)
    d = set(range(T - last, T)) | ({first} if first < T else set())
    ch = nw_chunk(K, q)
    assert any(t % ch == 0 for t in range(T - last + 1, T)), "no chunk edge among the dates"
    return tuple(sorted(d))


def oracle_nw(F, q, tau, dates):
    """V [len(dates), K, K] in longdouble, literally the reference's Newey_West on each prefix."""
    T, K = F.shape
    fin = np.isfinite(F)
    FL = np.where(fin, F, 0.0).astype(LD)
    out = np.full((len(dates), K, K), np.nan, dtype=LD)
    for j, t in enumerate(dates):
        n = t + 1
        if n <= q or n <= K:
            continue
        w = LD(0.5) ** (np.arange(n - 1, -1, -1).astype(LD) / LD(tau))
        w = w / w.sum()
        dead = ~fin[:n].all(0)
        X = np.where(dead[None, :], LD(0), FL[:n])             # computed without the dead columns
        r = X - (w[:, None] * X).sum(0)
        r[:, (X == X[0]).all(0)] = 0                           # an exactly constant column
        V = (r * w[:, None]).T @ r
        for i in range(1, q + 1):
            Gi = (r[:n - i] * w[i:, None]).T @ r[i:]
            V = V + (1 - LD(i) / LD(q + 1)) * (Gi + Gi.T)
        V[dead, :] = np.nan
        V[:, dead] = np.nan
        out[j] = V
    return out


def second_nw(F, q, tau, dates):
    """The second opinion in float64: one-pass decayed uncentred moments, Z by summation.  Also
    Q [len(dates), K], the normalised decayed sums of squares."""
    T, K = F.shape
    X = np.where(np.isfinite(F), F, 0.0)
    lam = 0.5 ** (1.0 / tau)
    Z, m, S0 = 0.0, np.zeros(K), np.zeros((K, K))
    A, a, b, z = np.zeros((q, K, K)), np.zeros((q, K)), np.zeros((q, K)), np.zeros(q)
    coef = 1.0 - np.arange(1, q + 1) / (q + 1.0)
    want = {t: j for j, t in enumerate(dates)}
    out = np.full((len(dates), K, K), np.nan)
    Q = np.zeros((len(dates), K))
    Xp = np.concatenate([np.zeros((q, K)), X])                  # row u of X is row u + q of Xp
    for u in range(T):
        fu = X[u]
        Z = lam * Z + 1.0
        m = lam * m + fu
        S0 = lam * S0 + np.outer(fu, fu)
        if q:
            has = (u >= np.arange(1, q + 1)).astype(np.float64)
            g = Xp[u:u + q][::-1]                               # f_{u-1}, ..., f_{u-q} (0 before date 0)
            A = lam * A + g[:, :, None] * fu[None, None, :]
            a = lam * a + g
            b = lam * b + has[:, None] * fu[None, :]
            z = lam * z + has
        if u in want and u + 1 > q and u + 1 > K:
            mu = m / Z
            mm = np.outer(mu, mu)
            V = S0 / Z - mm
            if q:
                Gi = (A - a[:, :, None] * mu[None, None, :] - mu[None, :, None] * b[:, None, :]
                      + z[:, None, None] * mm[None]) / Z
                V = V + np.einsum("i,ikl->kl", coef, Gi + Gi.transpose(0, 2, 1))
            out[want[u]] = V
            Q[want[u]] = np.diag(S0) / Z
    return out, Q


def nw_bounds(F, q, want, sec, Q, dates):
    """atol per (date, k, l) under the module's rule, and the mask of exact-zero oracle entries."""
    atol = np.zeros(want.shape)
    zero = np.isfinite(want) & (want == 0)
    for j, t in enumerate(dates):
        f = np.isfinite(want[j]) & ~zero[j]
        s = np.sqrt(np.outer(Q[j], Q[j]))
        if f.any():
            d = np.abs(sec[j].astype(LD) - want[j]).astype(np.float64)
            assert np.isfinite(sec[j][f]).all() and (s[f] > 0).all()
            a = np.minimum(8 * d[f].max(), 8 * (d[f] / s[f]).max() * s)
            atol[j] = np.maximum(a, 4 * EPS * s)
        atol[j][zero[j]] = 4 * (1 + 2 * q) * (t + 3) * EPS * s[zero[j]]
    return atol, zero


@functools.lru_cache(maxsize=None)
def _nw(c):
    T, K, q, tau, kind, cuts, put, windows, last, seed = c
    F = _input(c)
    dates = _dates(c)
    want = oracle_nw(F, q, tau, dates)
    sec, Q = second_nw(F, q, tau, dates)
    atol, zero = nw_bounds(F, q, want, sec, Q, dates)
    for a in (F, want, sec, atol, zero):
        a.setflags(write=False)
    return F, dates, want, sec, atol, zero


# --- chunk edges (32 dates) and the ew_cumsum_cols lane partition (64 lanes x per); the cases with
# windows emit [t_lo, t_hi) inside a chunk, on its edges, one date and none.
# atol_case / sqrt(V_kk V_ll), largest per case when written: 4e-15 .. 3e-14 (2e-13 at T = 1)
EDGE = [_case(1, 1, 0, 42), _case(2, 1, 0, 42), _case(2, 1, 1, 42)] + \
       [_case(T, 3, 2, 42, windows=T in (33, 64, 65)) for T in (31, 32, 33, 63, 64, 65, 127, 128, 129)]
# --- workgroup tiling over K^2 (K = 16: 256 entries, K = 17: the second blockIdx.y), T just past K
# so that n = K gives NaN and n = K + 1 the first matrix.  atol_case / sqrt(V_kk V_ll): 5e-15 .. 3e-14
TILE = [_case(K + 3, K, 1, 42, cuts=(K, K + 1)) for K in (1, 2, 15, 16, 17)]
# --- the emission rule met exactly: n = q, q + 1 with q > K; q >= T (every output NaN)
EMIT = [_case(9, 2, 5, 42, cuts=(5, 6)), _case(5, 2, 5, 42, cuts=(2,)), _case(5, 2, 7, 42, cuts=(2,))]
# --- lag groups of 8, and more lags than a chunk has dates; AR(1) data: the lag terms dominate.
# atol_case / sqrt(V_kk V_ll): 2e-14 .. 2e-13
LAGS = [_case(70, 3, q, 42, "ar") for q in (0, 1, 7, 8, 9, 16, 17, 32, 40)]
# --- chunk halving and the LDS limit at K = 56 (chunk asserted per case); oracle on the last 10
# dates.  atol_case / sqrt(V_kk V_ll): 4e-11 .. 6e-9 (130 rows, 56 columns, up to 119 lags: V is
# nearly singular and its small diagonal entries carry the error of the large ones)
WIDE = [(_case(130, 56, q, 42, "ar", cuts=(123,), last=10), ch)
        for q, ch in ((98, 32), (99, 16), (110, 16), (111, 8), (116, 8), (117, 4), (119, 4))]
# --- half-lives, all dates of T = 70: both sides of the chunk edges at 32 and 64
# atol_case / sqrt(V_kk V_ll): 8e-13 (tau 0.5), 4e-14 (tau 2), 8e-15 .. 1e-14 (tau >= 42)
TAUS = [_case(70, 4, 2, tau, cuts=(31, 32, 33)) for tau in (0.5, 2, 42, 252, 1e4, 1e6, 1e9)]
# --- data that stresses the one-pass algebra.  atol_case / sqrt(V_kk V_ll): 1e-10 .. 1e-9, on the
# mean-1 column (mean^2 / var = 1e4)
DATA = [_case(65, 6, 2, tau, "stress") for tau in (42, 1e4)] + [_case(65, 6, 9, 42, "stress")]
# --- one NaN / +inf in one column: first row of a chunk, last row, within the last q rows before
# a shard cut.  atol_case / sqrt(V_kk V_ll): 1e-14
BAD = [_case(70, 3, 2, 42, put=((t, 1, v),), cuts=(50,)) for t in (32, 63, 49) for v in (NAN, INF)] + \
      [_case(70, 3, 0, 42, put=((40, 0, INF),), cuts=(41,))]
# --- shard cuts; (tau 0.5, q 10) and (tau 2, q 10) measure how the halo rows of M are rebuilt.
# atol_case / sqrt(V_kk V_ll): 5e-15 .. 5e-14 at tau 42, 8e-12 (tau 0.5), 4e-12 (tau 2).  On the MI355X
# the largest err / bound of the module was 0.86 (the stress columns at tau 1e4) when written.
SHARD = [_case(70, 4, q, 42, cuts=(1, q - 1, q, q + 1, 4, 5, 31, 32, 33, 69)) for q in (0, 2, 10)] + \
        [_case(70, 4, 10, tau, cuts=(1, 9, 10, 11, 31, 32, 33, 69)) for tau in (0.5, 2)]

NW_CASES = EDGE + TILE + EMIT + LAGS + [c for c, _ in WIDE] + TAUS + DATA + BAD + SHARD
WINDOWS = [(5, 40), (32, 64), (31, 33), (40, 64), (64, 65), (32, 32), (0, 1)]


def _check_case(c):
    T, K, q, tau, kind, cuts, put, windows, last, seed = c
    F, dates, want, sec, atol, zero = _nw(c)
    emitted = np.isfinite(want).any((1, 2))
    assert emitted.any() == (T > max(q, K)), "the case emits nothing (or should not)"
    if kind == "stress":
        assert zero[emitted][:, 1, :].all() and zero[emitted][:, 2, :].all() and (atol[:, 1, :] == 0).all()
    if put:
        (t, k, v), = put
        j = dates.index(t)
        assert np.isnan(want[j:, k, :]).all() and np.isfinite(np.delete(np.delete(want[j:], k, 1), k, 2)).all()
    return F, dates, want, atol


@pytest.mark.parametrize("c", NW_CASES, ids=_id)
def test_second_opinion_inside_its_bound(c):
    """The inputs are chosen so that the float64 second opinion itself passes the rule (the
    analytic bound on the exact zeros included)."""
    T, K, q, tau = c[:4]
    F, dates, want, atol = _check_case(c)
    sec = np.where(np.isnan(want), np.nan, _nw(c)[3])
    _close(sec, want, atol, RTOL_NW, f"second opinion {_id(c)}")


@pytest.mark.parametrize("c", NW_CASES, ids=_id)
def test_nw_series_oracle(mode, request, c):
    T, K, q, tau, kind, cuts, put, windows, last, seed = c
    dev = _device(mode, request)
    F, dates, want, atol = _check_case(c)
    for cc, ch in WIDE:
        if cc == c:
            assert nw_chunk(K, q) == ch and q <= nw_max_lags(K)
    if c in LAGS or c in EDGE or c in TAUS:
        assert nw_chunk(K, q) == CH
    Ft = _t(F, dev)
    idx = list(dates)
    got = _np(ES.newey_west_series(Ft, q, tau))
    assert got.shape == (T, K, K)
    w = _close(got[idx], want, atol, RTOL_NW, f"NW {mode} {_id(c)}")
    print(f"NW {mode} {_id(c)}: err / bound {w:.3g}, atol_case max {atol.max():.3g}")
    if windows:
        for lo, hi in WINDOWS:
            hi = min(hi, T)
            if lo > hi:
                continue
            part = _np(ES.newey_west_series(Ft, q, tau, lo, hi))
            assert part.shape == (hi - lo, K, K)
            _close(part, want[lo:hi], atol[lo:hi], RTOL_NW, f"NW {mode} {_id(c)} window [{lo}, {hi})")


@pytest.mark.parametrize("c", [c for c in NW_CASES if c[5]], ids=_id)
def test_nw_sharded_oracle(mode, request, c):
    T, K, q, tau, kind, cuts, put, windows, last, seed = c
    dev = _device(mode, request)
    F, dates, want, atol = _check_case(c)
    Ft = _t(F, dev)
    worst = 0.0
    for cut in cuts:
        got = _np(ES.newey_west_series_sharded(Ft[cut:], q, tau, history=Ft[:cut]))
        assert got.shape == (T - cut, K, K)
        j = [i for i, t in enumerate(dates) if t >= cut]
        idx = [dates[i] - cut for i in j]
        worst = max(worst, _close(got[idx], want[j], atol[j], RTOL_NW, f"NW shard {mode} {_id(c)} cut {cut}"))
    print(f"NW shard {mode} {_id(c)}: err / bound {worst:.3g}, atol_case max {atol.max():.3g}")


@pytest.mark.gpu
def test_lag_count_past_the_lds_limit_raises(cuda):
    F = _t(_series("plain", 130, 56, 1), cuda)
    assert nw_max_lags(56) == 119
    with pytest.raises(ValueError):
        ES.newey_west_series(F, 120, 42.0)
    with pytest.raises(ValueError):
        ES.newey_west_series_sharded(F[100:], 120, 42.0, history=F[:100])


# ============================================================================== prefix mean
def _pm_input(T, kind, seed):
    rng = np.random.default_rng(seed)
    x = rng.random(T) + 0.5
    per = -(-T // 64)
    if kind == "mixed":          # leading NaNs, scattered NaN and +-inf
        x[:min(3, T - 1)] = NAN
        x[rng.random(T) < 0.1] = NAN
        if T > 3:
            x[3] = 0.75
        if T > 20:
            x[[7, 11]] = INF, -INF
            x[T - 1] = 1.25
    elif kind == "allnan":
        x[:] = NAN
    elif kind == "run":          # a NaN run over whole lanes' ranges that ends mid-lane
        a = 2 * per
        b = min(a + 60, a + 3 * per + max(1, per // 2))
        assert b < T and b - a <= 60 and (per == 1 or b % per != 0)
        x[a:b] = NAN
    elif kind == "big":
        x = 1e6 + (x - 1.0) * 1e-2
    elif kind == "inf":
        x[rng.random(T) < 0.2] = INF
        x[rng.random(T) < 0.2] = -INF
        x[0] = INF
    else:
        assert kind == "plain"
    return x


def _pm(x, tau, dt):
    """Oracle (``dt`` longdouble): the reference's weights over the finite entries of each prefix."""
    T = x.size
    ok = np.isfinite(x)
    xv = np.where(ok, x, 0).astype(dt)
    age = np.arange(T)[:, None] - np.arange(T)[None, :]                      # t - s
    w = np.where((age >= 0) & ok[None, :], dt(0.5) ** (np.maximum(age, 0).astype(dt) / dt(tau)), dt(0))
    den = w.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, (w * xv[None, :]).sum(1) / den, dt("nan"))


def _pm_second(x, tau):
    lam = 0.5 ** (1.0 / tau)
    num = den = 0.0
    out = np.full(x.size, np.nan)
    for t, v in enumerate(x.tolist()):
        ok = np.isfinite(v)
        num = lam * num + (v if ok else 0.0)
        den = lam * den + (1.0 if ok else 0.0)
        if den > 0:
            out[t] = num / den
    return out


@functools.lru_cache(maxsize=None)
def _pm_case(T, kind, tau, seed):
    x = _pm_input(T, kind, seed)
    want = _pm(x, tau, LD)
    sec = _pm_second(x, tau)
    assert np.array_equal(np.isnan(sec), np.isnan(want))
    f = np.isfinite(want)
    dev = float(np.max(np.abs(sec[f].astype(LD) - want[f]))) if f.any() else 0.0
    atol = np.maximum(8 * dev, EPS * np.abs(np.where(f, want, 0)).astype(np.float64))
    for a in (x, want, atol):
        a.setflags(write=False)
    return x, want, atol


PM_T = (1, 2, 63, 64, 65, 127, 128, 129, 1025)
# (T, kind, tau, cuts); atol_case when written: 2e-16 .. 1.3e-14 (values ~1), 1e-9 .. 3e-8 ("big",
# values 1e6)
PM_CASES = [(T, "mixed", 42.0, (1, 63, 64, 65, T - 1)) for T in PM_T] + \
           [(T, "plain", 42.0, ()) for T in (1, 2, 64, 65)] + \
           [(T, kind, tau, (1, 63, 64, 65, T - 1))
            for T, kind in ((129, "run"), (1025, "run"), (129, "inf"), (129, "big"), (1025, "big"), (65, "allnan"))
            for tau in (0.5, 42.0, 1e6)]


@pytest.mark.parametrize("T, kind, tau, cuts", PM_CASES)
def test_prefix_mean_oracle(mode, request, T, kind, tau, cuts):
    dev = _device(mode, request)
    x, want, atol = _pm_case(T, kind, tau, 7 * T + len(kind))
    if kind == "allnan":
        assert np.isnan(want).all()
    if kind == "mixed" and T > 3:
        assert np.isnan(want[:3]).all() and np.isfinite(want[3:]).all()
    xt = _t(x, dev)
    w = _close(_np(ES.ew_prefix_mean(xt, tau)), want, atol, RTOL_PM, f"prefix mean {mode} T={T} {kind} tau={tau:g}")
    for cut in sorted({c for c in cuts if 1 <= c <= T - 1}):
        got = _np(ES.ew_prefix_mean_sharded(xt[cut:], tau, history=xt[:cut]))
        w = max(w, _close(got, want[cut:], atol[cut:], RTOL_PM,
                          f"prefix mean shard {mode} T={T} {kind} tau={tau:g} cut {cut}"))
    print(f"prefix mean {mode} T={T} {kind} tau={tau:g}: err / bound {w:.3g}, atol_case max {atol.max():.3g}")


@pytest.mark.parametrize("tau", [0.5, 42.0])
def test_prefix_mean_shard_cut_in_nan_run_and_nan_history(mode, request, tau):
    """A cut inside a NaN run, and a history that is all NaN (nothing carried in)."""
    dev = _device(mode, request)
    x, want, atol = _pm_case(129, "run", tau, 7 * 129 + 3)
    run = np.flatnonzero(np.isnan(x))
    cut = int(run[len(run) // 2])
    assert np.isnan(x[cut - 1]) and np.isnan(x[cut]) and np.isnan(x[cut + 1])
    xt = _t(x, dev)
    got = _np(ES.ew_prefix_mean_sharded(xt[cut:], tau, history=xt[:cut]))
    _close(got, want[cut:], atol[cut:], RTOL_PM, f"prefix mean shard {mode} cut {cut} inside the run")
    y = x.copy()
    y[:64] = NAN
    wy = _pm(y, tau, LD)
    f = np.isfinite(wy)
    ay = np.maximum(8 * float(np.max(np.abs(_pm_second(y, tau)[f].astype(LD) - wy[f]))), EPS * np.abs(np.where(f, wy, 0)))
    yt = _t(y, dev)
    for cut in (63, 64):
        got = _np(ES.ew_prefix_mean_sharded(yt[cut:], tau, history=yt[:cut]))
        _close(got, wy[cut:], ay[cut:].astype(np.float64), RTOL_PM, f"prefix mean shard {mode} all-NaN history, cut {cut}")
