// Projection step of the box-constrained QP with linear trading costs (ops/tcost_qp.py), all
// dates per launch (gfx950):
//   minimise 1/2 h' Sigma h - q' h + sum_n kappa_n |h_n - p_n|
//   s.t.  sum_U h = budget,  lo <= h <= hi on U,  h = 0 off U.
// The cost is separable per stock, so only the inner per-stock minimiser of csrc/box_qp.hip
// changes: with v_n = u_n + gamma a_n,
//   h_n(gamma) = clip( median(v_n - kappa_n a_n, p_n, v_n + kappa_n a_n), lo_n, hi_n ),
// still nondecreasing and piecewise linear in gamma (slope a_n where the median is not p_n and
// lies strictly inside the bounds, 0 on the no-trade piece and at a bound).  The root find, its
// two stopping tests and the fixed reduction order (thread-strided, lane -> wave -> the four
// waves in wave order) are those of box_project_kernel; pstats[1] = q' h - sum kappa |h - p|, so
// box_step_kernel and eq_step_kernel take the result as it is.
//
// Layout of the resident tiers (N <= E * 256, E = 4 / 12 / 20 stocks per thread): the four rows
// of box_project_kernel (u, a, lo, hi) live in registers and the two new rows (p, kappa) in LDS,
// 2 * E * 256 doubles = 16 / 48 / 80 KiB, each thread reading back only what it wrote (no
// barrier, no bank conflict: consecutive lanes, consecutive doubles).  All six rows in registers
// also fit at E = 20 without scratch (256 VGPRs + 226 AGPRs of the 512), but every use of a row
// parked in an AGPR costs a copy, and at 2520 x 5000 that layout measured 1.85 ms against 1.69 ms
// for this one (kappa = 0; 1.34 against 1.24 ms at kappa = 2e-5), so it was dropped.  The
// compiler's resource report, no scratch in any tier, is quoted in the README ("Trading
// costs").  Above 5120 stocks, or with mode 1, the rows are re-read from global memory (L2) in
// every inner iteration; both variants sum in the same order and use the same fused
// operations, so they give the same bits.
#include "common.h"

namespace {

using namespace mfa;

constexpr int kThreads = 256, kWaves = 4;
constexpr int kRunning = -1;  // ops/box_qp.py
constexpr int kRootIters = 100;
constexpr double kEps = 2.220446049250313e-16;
constexpr double kInf = __builtin_huge_val();

struct Stock {
  double u, a, lo, hi, p, k;
};

struct Rows {
  const double *u, *a, *lo, *hi, *p, *k;
};

// Stock n of a date, sanitised as load_stock of csrc/box_qp.hip: a stock outside the universe (a
// <= 0 or not finite) or with a NaN bound becomes all zeros, which gives h = 0 for every gamma,
// is never free and costs nothing.  A non-finite p is 0 (a name not held before).  `inval` is
// raised by a universe stock whose u is not finite or whose kappa is NaN, negative or infinite.
__device__ __forceinline__ Stock load_stock(const Rows& r, int n, int& inval) {
  Stock s{r.u[n], r.a[n], r.lo[n], r.hi[n], r.p[n], r.k[n]};
  const bool in = __builtin_isfinite(s.a) && s.a > 0.0 && s.lo == s.lo && s.hi == s.hi;
  if (!in) return Stock{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const bool ubad = !__builtin_isfinite(s.u), kbad = !(s.k >= 0.0 && s.k < kInf);
  inval |= ubad || kbad;
  if (ubad) s.u = 0.0;
  if (kbad) s.k = 0.0;
  if (!__builtin_isfinite(s.p)) s.p = 0.0;
  return s;
}

// h_n(gamma) and whether it moves with gamma; the same operations wherever it is evaluated
__device__ __forceinline__ double hold(const Stock& s, double gam, bool& free) {
  const double v = fma(gam, s.a, s.u);
  const double m = fmin(fmax(s.p, fma(-s.k, s.a, v)), fma(s.k, s.a, v));
  free = m > s.lo && m < s.hi && m != s.p;
  return fmin(fmax(m, s.lo), s.hi);
}

__device__ __forceinline__ void clip_terms(const Stock& s, double gam, double& S, double& W,
                                           double& T) {
  bool free;
  const double h = hold(s, gam, free);
  S += h;
  T += fabs(h);
  W += free ? s.a : 0.0;
}

// Sum of NV per-thread values over the workgroup: lane -> wave (DPP) -> the four waves in wave
// order.  `buf` [kWaves * NV]; callers alternate between two buffers so that one barrier per
// call is enough.
template <int NV>
__device__ __forceinline__ void block_sums(double (&x)[NV], double* buf) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    x[j] = wave_total(x[j]);
    if (lane == 0) buf[wid * NV + j] = x[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j)
    x[j] = ((buf[j] + buf[NV + j]) + buf[2 * NV + j]) + buf[3 * NV + j];
}

// E > 0: the date's rows are resident, E stocks per thread (N <= E * 256): u, a, lo, hi in
// registers, p and kappa in LDS; E == 0: they are re-read from global memory (L2) in every inner
// iteration, any N.
template <int E>
__global__ __launch_bounds__(kThreads) void tc_project_kernel(
    Rows rows, const double* __restrict__ q, const double* __restrict__ budget,
    const int* __restrict__ status, int N, double* __restrict__ gamma, double* __restrict__ h,
    double* __restrict__ w, double* __restrict__ pstats, int* __restrict__ pflag,
    double* __restrict__ cost) {
  __shared__ double red[2][kWaves * 4];
  __shared__ double ext[kWaves * 2];
  const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (status && status[d] != kRunning) return;  // a finished date keeps its h, w, gamma, cost
  const size_t off = (size_t)d * N;
  const Rows rd{rows.u + off, rows.a + off, rows.lo + off, rows.hi + off, rows.p + off,
                rows.k + off};
  constexpr int EE = E > 0 ? E : 1;
  __shared__ double pk[E > 0 ? 2 * E * kThreads : 1];  // p [E][256], then kappa [E][256]
  double ru[EE], ra[EE], rl[EE], rh[EE];
  auto at = [&](int i) {
    return Stock{ru[i], ra[i], rl[i], rh[i], pk[i * kThreads + tid], pk[(EE + i) * kThreads + tid]};
  };

  // set-up: feasibility, the range of the finite breakpoints of every h_n(gamma)
  double su[3] = {0.0, 0.0, 0.0};  // sum lo, sum hi, stocks
  double bmin = kInf, bmax = -kInf;
  int bad = 0, inval = 0;
  auto setup = [&](const Stock& s) {
    if (s.a > 0.0) {
      bad |= !(s.lo <= s.hi) || s.lo == kInf || s.hi == -kInf;
      su[0] += s.lo;
      su[1] += s.hi;
      su[2] += 1.0;
      auto brk = [&](double x) {  // v -+ kappa a = x  at  gamma = (x - u) / a +- kappa
        if (__builtin_isfinite(x)) {
          const double t = (x - s.u) / s.a;
          bmin = fmin(bmin, t - s.k);
          bmax = fmax(bmax, t + s.k);
        }
      };
      brk(s.lo);
      brk(s.hi);
      brk(s.p);
    }
  };
  if constexpr (E > 0) {
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int n = tid + i * kThreads;
      Stock s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (n < N) {
        s = load_stock(rd, n, inval);
        setup(s);
      }
      ru[i] = s.u, ra[i] = s.a, rl[i] = s.lo, rh[i] = s.hi;
      pk[i * kThreads + tid] = s.p, pk[(EE + i) * kThreads + tid] = s.k;
    }
  } else {
    for (int n = tid; n < N; n += kThreads) setup(load_stock(rd, n, inval));
  }
  const double bud = budget[d];
  inval |= !__builtin_isfinite(bud);
  block_sums<3>(su, red[0]);
  bmin = wave_min(bmin);
  bmax = wave_max(bmax);
  if (lane == 0) {
    ext[wid * 2] = bmin;
    ext[wid * 2 + 1] = bmax;
  }
  inval = __syncthreads_or(inval);
  bad = __syncthreads_or(bad);
  bmin = fmin(fmin(ext[0], ext[2]), fmin(ext[4], ext[6]));
  bmax = fmax(fmax(ext[1], ext[3]), fmax(ext[5], ext[7]));
  if (!(bmin <= bmax)) bmin = bmax = 0.0;  // no finite breakpoint anywhere
  const int flag = inval ? 2 : ((bad || su[2] == 0.0 || su[0] > bud || su[1] < bud) ? 1 : 0);
  if (flag) {  // uniform: h, w, gamma and cost keep what they held
    if (tid == 0) pflag[d] = flag;
    return;
  }

  // root of s(gamma): bracketed Newton, bisection when the Newton point leaves the bracket (a
  // root on a no-trade piece has W = 0); an open end is closed by a point beyond every
  // breakpoint, where s is linear
  int unused = 0;
  double gam = gamma[d];
  if (!__builtin_isfinite(gam)) gam = 0.0;
  double L = -kInf, H = kInf;
  int pp = 1;  // reduction buffer of the next block_sums
  for (int it = 0; it < kRootIters; ++it) {
    double sw[3] = {0.0, 0.0, 0.0};  // S, W, T
    if constexpr (E > 0) {
#pragma unroll
      for (int i = 0; i < E; ++i) clip_terms(at(i), gam, sw[0], sw[1], sw[2]);
    } else {
      for (int n = tid; n < N; n += kThreads)
        clip_terms(load_stock(rd, n, unused), gam, sw[0], sw[1], sw[2]);
    }
    block_sums<3>(sw, red[pp]);
    pp ^= 1;
    const double s = sw[0] - bud, W = sw[1];
    if (fabs(s) <= 4.0 * kEps * (sw[2] + fabs(bud))) break;
    if (s < 0.0) L = gam;
    else H = gam;
    const bool closed = L > -kInf && H < kInf;
    if (closed && H - L <= 4.0 * kEps * fmax(fabs(L), fabs(H))) break;
    double gn = gam - s / W;
    if (!(W > 0.0 && gn > L && gn < H)) {
      if (closed) {
        gn = 0.5 * (L + H);
        if (!(gn > L && gn < H)) break;
      } else if (L == -kInf) {
        gn = fmin(gam, bmin) - fmax(1.0, fmax(fabs(gam), fabs(bmin)));
      } else {
        gn = fmax(gam, bmax) + fmax(1.0, fmax(fabs(gam), fabs(bmax)));
      }
    }
    gam = gn;
  }

  // h, the Gram weight of the free set, sum s^2 h^2, q' h, sum |h|, sum kappa |h - p|
  const double* qd = q + off;
  double* hout = h + off;
  double* wout = w + off;
  double fs[4] = {0.0, 0.0, 0.0, 0.0};
  auto finish = [&](const Stock& s, int n) {
    bool free;
    const double hn = hold(s, gam, free);
    hout[n] = hn;
    wout[n] = free ? s.a : 0.0;
    if (s.a > 0.0) {
      const double qn = qd[n];
      fs[0] = fma(hn / s.a, hn, fs[0]);
      fs[1] = fma(__builtin_isfinite(qn) ? qn : 0.0, hn, fs[1]);
      fs[2] += fabs(hn);
      fs[3] = fma(s.k, fabs(hn - s.p), fs[3]);
    }
  };
  if constexpr (E > 0) {
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int n = tid + i * kThreads;
      if (n < N) finish(at(i), n);
    }
  } else {
    for (int n = tid; n < N; n += kThreads) finish(load_stock(rd, n, unused), n);
  }
  block_sums<4>(fs, red[pp]);
  if (tid == 0) {
    gamma[d] = gam;
    pstats[(size_t)d * 3] = fs[0];
    pstats[(size_t)d * 3 + 1] = fs[1] - fs[3];
    pstats[(size_t)d * 3 + 2] = fs[2];
    cost[d] = fs[3];
    pflag[d] = 0;
  }
}

}  // namespace

// u, a, lo, hi, q, p, kappa, h, w [D][N] f64; budget, gamma [D] (gamma: warm start in, root out);
// status [D] int or null (dates whose status is not -1 are left untouched); pstats [D][3] =
// (sum h^2 / a, q' h - cost, sum |h|); cost [D] = sum_U kappa |h - p|; pflag [D]: 0 feasible,
// 1 infeasible, 2 non-finite u or budget, or a kappa of the universe that is not in [0, inf).
// mode 0: rows resident for N <= 5120, re-streamed above; mode 1: always re-streamed.
MFA_API int mfa_tc_project(const double* u, const double* a, const double* lo, const double* hi,
                           const double* q, const double* p, const double* kappa,
                           const double* budget, const int* status, int D, int N, int mode,
                           double* gamma, double* h, double* w, double* pstats, int* pflag,
                           double* cost, void* stream) {
  if (D <= 0) return 0;
  if (N <= 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const Rows rows{u, a, lo, hi, p, kappa};
#define MFA_E(ee)                                                                          \
  hipLaunchKernelGGL((tc_project_kernel<ee>), dim3(D), dim3(kThreads), 0, s, rows, q, budget, \
                     status, N, gamma, h, w, pstats, pflag, cost)
  if (mode == 1 || N > 20 * kThreads) MFA_E(0);
  else if (N <= 4 * kThreads) MFA_E(4);
  else if (N <= 12 * kThreads) MFA_E(12);
  else MFA_E(20);
#undef MFA_E
  return (int)hipGetLastError();
}
