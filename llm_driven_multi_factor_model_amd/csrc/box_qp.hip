// Box-constrained QP on the factor-structured covariance Sigma_d = X_d F_d X_d^T + diag(s_d^2),
// all dates per launch (gfx950):
//   minimise 1/2 h' Sigma h - q' h   s.t.  sum_U h = budget,  lo <= h <= hi on U,  h = 0 off U.
// Semismooth Newton on the reduced dual phi(nu) (nu in R^K, the multiplier of y = B' h with
// B = X R, F = R R'); the budget multiplier gamma is eliminated exactly at every trial nu:
//   u_n = a_n (q_n - x_n . R nu),   h_n = clip(u_n + gamma a_n, lo_n, hi_n),   a = 1 / s^2,
//   gamma = root of the nondecreasing piecewise-linear  s(gamma) = sum_U h_n(gamma) - budget.
// One trial ("pass") = factor_apply (u) -> box_project_kernel (gamma, h, Gram weight w = a 1_free)
// -> factor_gram (G_f) + factor_xty (X' h) -> box_step_kernel (Armijo test, Newton direction,
// convergence, next trial's c = R (nu + step dn)).  One 256-thread workgroup per date in both
// kernels; every reduction runs in a fixed order, so two runs give the same bits.
#include "common.h"

namespace {

using namespace mfa;

constexpr int kThreads = 256, kWaves = 4;
constexpr int kMaxK = 64;
constexpr int kRunning = -1, kOk = 0, kInfeasible = 2, kInvalid = 3;  // ops/box_qp.py
constexpr int kStalled = 4;  // ops/exposure_qp.py: the trial's projection lost the budget
constexpr int kRootIters = 100;
constexpr double kEps = 2.220446049250313e-16;
constexpr double kInf = __builtin_huge_val();

// ----------------------------------------------------------------------------- projection
struct Stock {
  double u, a, lo, hi;
};

// Stock n of a date, sanitised: a stock outside the universe (a <= 0 or not finite) or with a
// NaN bound becomes (0, 0, 0, 0), which clips to h = 0 for every gamma and is never free.
__device__ __forceinline__ Stock load_stock(const double* __restrict__ u,
                                            const double* __restrict__ a,
                                            const double* __restrict__ lo,
                                            const double* __restrict__ hi, int n) {
  Stock s{u[n], a[n], lo[n], hi[n]};
  const bool in = __builtin_isfinite(s.a) && s.a > 0.0 && s.lo == s.lo && s.hi == s.hi;
  if (!in) s = Stock{0.0, 0.0, 0.0, 0.0};
  return s;
}

__device__ __forceinline__ void clip_terms(const Stock& s, double gam, double& S, double& W,
                                           double& T) {
  const double v = fma(gam, s.a, s.u);
  const double h = fmin(fmax(v, s.lo), s.hi);
  S += h;
  T += fabs(h);
  W += (v > s.lo && v < s.hi) ? s.a : 0.0;
}

// Sum of three per-thread values over the workgroup: lane -> wave (DPP) -> the four waves in wave
// order.  `buf` [kWaves * 3]; callers alternate between two buffers so that one barrier per call
// is enough.
__device__ __forceinline__ void block_sum3(double& x, double& y, double& z, double* buf) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  x = wave_total(x);
  y = wave_total(y);
  z = wave_total(z);
  if (lane == 0) {
    buf[wid * 3] = x;
    buf[wid * 3 + 1] = y;
    buf[wid * 3 + 2] = z;
  }
  __syncthreads();
  x = ((buf[0] + buf[3]) + buf[6]) + buf[9];
  y = ((buf[1] + buf[4]) + buf[7]) + buf[10];
  z = ((buf[2] + buf[5]) + buf[8]) + buf[11];
}

// E > 0: the date's four rows live in registers, E stocks per thread (N <= E * 256); E == 0: they
// are re-read from global memory (L2) in every inner iteration, any N.  Both sum in the same
// order (thread-strided), so they give the same bits.
template <int E>
__global__ __launch_bounds__(kThreads) void box_project_kernel(
    const double* __restrict__ u, const double* __restrict__ a, const double* __restrict__ lo,
    const double* __restrict__ hi, const double* __restrict__ q,
    const double* __restrict__ budget, const int* __restrict__ status, int N,
    double* __restrict__ gamma, double* __restrict__ h, double* __restrict__ w,
    double* __restrict__ pstats, int* __restrict__ pflag) {
  __shared__ double red[2][kWaves * 3];
  __shared__ double ext[kWaves * 2];
  const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (status && status[d] != kRunning) return;  // a finished date keeps its h, w and gamma
  const double* ud = u + (size_t)d * N;
  const double* ad = a + (size_t)d * N;
  const double* ld = lo + (size_t)d * N;
  const double* hd = hi + (size_t)d * N;
  constexpr int EE = E > 0 ? E : 1;
  Stock r[EE];

  // set-up: feasibility, the range of the finite breakpoints
  double slo = 0.0, shi = 0.0, cnt = 0.0, bmin = kInf, bmax = -kInf;
  int bad = 0, inval = 0;
  auto setup = [&](const Stock& s, double uraw) {
    if (s.a > 0.0) {
      inval |= !__builtin_isfinite(uraw);
      bad |= !(s.lo <= s.hi) || s.lo == kInf || s.hi == -kInf;
      cnt += 1.0;
      slo += s.lo;
      shi += s.hi;
      if (__builtin_isfinite(s.lo)) {
        const double t = (s.lo - s.u) / s.a;
        bmin = fmin(bmin, t);
        bmax = fmax(bmax, t);
      }
      if (__builtin_isfinite(s.hi)) {
        const double t = (s.hi - s.u) / s.a;
        bmin = fmin(bmin, t);
        bmax = fmax(bmax, t);
      }
    }
  };
  if constexpr (E > 0) {
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int n = tid + i * kThreads;
      r[i] = Stock{0.0, 0.0, 0.0, 0.0};
      if (n < N) {
        r[i] = load_stock(ud, ad, ld, hd, n);
        const double uraw = r[i].u;
        if (!__builtin_isfinite(uraw)) r[i].u = 0.0;
        setup(r[i], uraw);
      }
    }
  } else {
    for (int n = tid; n < N; n += kThreads) {
      Stock s = load_stock(ud, ad, ld, hd, n);
      const double uraw = s.u;
      if (!__builtin_isfinite(uraw)) s.u = 0.0;
      setup(s, uraw);
    }
  }
  const double bud = budget[d];
  inval |= !__builtin_isfinite(bud);
  block_sum3(slo, shi, cnt, red[0]);
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
  if (!(bmin <= bmax)) bmin = bmax = 0.0;  // no finite bound anywhere
  const int flag = inval ? 2 : ((bad || cnt == 0.0 || slo > bud || shi < bud) ? 1 : 0);
  if (flag) {  // uniform: h, w and gamma keep what they held
    if (tid == 0) pflag[d] = flag;
    return;
  }

  // root of s(gamma): bracketed Newton, bisection when the Newton point leaves the bracket; an
  // open end is closed by a point beyond every breakpoint, where s is linear
  double gam = gamma[d];
  if (!__builtin_isfinite(gam)) gam = 0.0;
  double L = -kInf, H = kInf;
  int pp = 1;  // reduction buffer of the next block_sum3
  for (int it = 0; it < kRootIters; ++it) {
    double S = 0.0, W = 0.0, T = 0.0;
    if constexpr (E > 0) {
#pragma unroll
      for (int i = 0; i < E; ++i) clip_terms(r[i], gam, S, W, T);
    } else {
      for (int n = tid; n < N; n += kThreads) {
        Stock s = load_stock(ud, ad, ld, hd, n);
        if (!__builtin_isfinite(s.u)) s.u = 0.0;
        clip_terms(s, gam, S, W, T);
      }
    }
    block_sum3(S, W, T, red[pp]);
    pp ^= 1;
    const double s = S - bud;
    if (fabs(s) <= 4.0 * kEps * (T + fabs(bud))) break;
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

  // h, the Gram weight of the free set, sum s^2 h^2, q' h, sum |h|
  const double* qd = q + (size_t)d * N;
  double* hout = h + (size_t)d * N;
  double* wout = w + (size_t)d * N;
  double sh2 = 0.0, qh = 0.0, T = 0.0;
  auto finish = [&](const Stock& s, int n) {
    const double v = fma(gam, s.a, s.u);
    const double hn = fmin(fmax(v, s.lo), s.hi);
    hout[n] = hn;
    wout[n] = (v > s.lo && v < s.hi) ? s.a : 0.0;
    if (s.a > 0.0) {
      const double qn = qd[n];
      sh2 = fma(hn / s.a, hn, sh2);
      qh = fma(__builtin_isfinite(qn) ? qn : 0.0, hn, qh);
      T += fabs(hn);
    }
  };
  if constexpr (E > 0) {
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int n = tid + i * kThreads;
      if (n < N) finish(r[i], n);
    }
  } else {
    for (int n = tid; n < N; n += kThreads) {
      Stock s = load_stock(ud, ad, ld, hd, n);
      if (!__builtin_isfinite(s.u)) s.u = 0.0;
      finish(s, n);
    }
  }
  block_sum3(sh2, qh, T, red[pp]);
  if (tid == 0) {
    gamma[d] = gam;
    pstats[(size_t)d * 3] = sh2;
    pstats[(size_t)d * 3 + 1] = qh;
    pstats[(size_t)d * 3 + 2] = T;
    pflag[d] = 0;
  }
}

// ------------------------------------------------------------------------------------ step
// Dynamic LDS: A (G_f, then H and its Cholesky factor), R = U sqrt(max(lambda, 0)), Tm = G_f R
// with the odd leading dimension K | 1 of woodbury_coef_kernel, then six K-vectors.
__host__ __device__ constexpr size_t step_lds_bytes(int K) {
  return ((size_t)3 * K * (K | 1) + 6 * kMaxK) * sizeof(double);
}

__global__ __launch_bounds__(kThreads) void box_step_kernel(
    const double* __restrict__ G, const double* __restrict__ lam, const double* __restrict__ U,
    const double* __restrict__ x, const double* __restrict__ pstats,
    const int* __restrict__ pflag, double tol, int K, double* __restrict__ nu,
    double* __restrict__ grad, double* __restrict__ dn, double* __restrict__ c,
    double* __restrict__ ds, int* __restrict__ passes, int* __restrict__ status,
    int* __restrict__ accepted) {
  extern __shared__ double st_lds[];
  const int kLD = K | 1;
  double* A = st_lds;
  double* R = A + K * kLD;
  double* Tm = R + K * kLD;
  double* nut = Tm + K * kLD;  // trial nu, then the current nu
  double* by = nut + kMaxK;    // B' h = R' (X' h)
  double* gt = by + kMaxK;     // gradient at the trial
  double* gold = gt + kMaxK;   // gradient at the accepted point
  double* dnv = gold + kMaxK;  // Newton direction
  double* rn = dnv + kMaxK;    // squared row norms of R (diagonal of F)
  const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (status[d] != kRunning) return;  // a finished date keeps its state and its c
  const double* Gd = G + (size_t)d * K * K;
  const double* Ud = U + (size_t)d * K * K;
  const double* ld = lam + (size_t)d * K;
  const double* xd = x + (size_t)d * K;
  double* dsd = ds + (size_t)d * 4;  // phi, step, variance of the last trial, spare
  const int flag = pflag[d];
  int bad = 0;
  for (int e = tid; e < K * K; e += kThreads) {
    const int i = e / K, k = e - i * K;
    const double gv = Gd[e], uv = Ud[e], lv = ld[k];
    bad |= !(__builtin_isfinite(gv) && __builtin_isfinite(uv) && __builtin_isfinite(lv));
    A[i * kLD + k] = gv;
    R[i * kLD + k] = uv * sqrt(lv > 0.0 ? lv : 0.0);
  }
  for (int e = tid; e < K; e += kThreads) bad |= !__builtin_isfinite(xd[e]);
  const double sh2 = pstats[(size_t)d * 3], qh = pstats[(size_t)d * 3 + 1],
               habs = pstats[(size_t)d * 3 + 2];
  bad = __syncthreads_or(bad);
  if (flag == 0) bad |= !(__builtin_isfinite(sh2) && __builtin_isfinite(qh));
  if (flag != 0 || bad) {
    if (tid == 0) {
      status[d] = flag == 1 ? kInfeasible : kInvalid;
      accepted[d] = 0;
    }
    return;
  }
  const double phi = dsd[0], step = dsd[1];
  if (tid < K) {
    nut[tid] = fma(step, dn[(size_t)d * K + tid], nu[(size_t)d * K + tid]);
    double s = 0.0, r2 = 0.0;
    for (int j = 0; j < K; ++j) {
      s = fma(R[j * kLD + tid], xd[j], s);
      r2 = fma(R[tid * kLD + j], R[tid * kLD + j], r2);
    }
    by[tid] = s;
    rn[tid] = r2;
    gold[tid] = grad[(size_t)d * K + tid];
    dnv[tid] = dn[(size_t)d * K + tid];
  }
  __syncthreads();
  // scalars of the trial, the same serial sums in every thread
  double nb = 0.0, nn = 0.0, bb = 0.0, gmax = 0.0, gd = 0.0, rmax = 0.0;
  for (int k = 0; k < K; ++k) {
    const double g = by[k] - nut[k];
    nb = fma(nut[k], by[k], nb);
    nn = fma(nut[k], nut[k], nn);
    bb = fma(by[k], by[k], bb);
    gmax = fmax(gmax, fabs(g));
    gd = fma(gold[k], dnv[k], gd);
    rmax = fmax(rmax, rn[k]);
  }
  const double phit = 0.5 * sh2 - qh + nb - 0.5 * nn;
  const int np = passes[d] + 1;
  if (!(__builtin_isfinite(phit) && __builtin_isfinite(gmax))) {
    if (tid == 0) {
      status[d] = kInvalid;
      accepted[d] = 0;
    }
    return;
  }
  // converged: max |grad| <= tol max(1, sum |h|) sqrt(max_k F_kk)
  const bool conv = gmax <= tol * fmax(1.0, habs) * sqrt(rmax);
  const bool acc = conv || phit >= phi + 1e-4 * step * gd - 4.0 * kEps * fabs(phit);
  __syncthreads();  // gold / dnv read by every thread before they change
  double nstep = 1.0;
  if (!acc) {  // the maximiser of the parabola through phi(0), phi'(0), phi(step), in [0.1, 0.5] step
    const double den = 2.0 * (phi + gd * step - phit);
    double cut = den > 0.0 ? gd * step * step / den : 0.5 * step;
    if (!(cut == cut)) cut = 0.0;
    nstep = fmin(fmax(cut, 0.1 * step), 0.5 * step);
  }
  if (acc) {
    if (tid < K) {
      const double g = by[tid] - nut[tid];
      gt[tid] = g;
      nu[(size_t)d * K + tid] = nut[tid];
      grad[(size_t)d * K + tid] = g;
    }
  } else if (tid < K) {
    nut[tid] = nu[(size_t)d * K + tid];
  }
  if (acc && !conv) {
    // H = I + R' (G_f - g g' / sigma) R with g = G_f[:, 0], sigma = G_f[0, 0] (the country
    // column is 1 on every stock); R' g is row 0 of Tm = G_f R
    for (int e = tid; e < K * K; e += kThreads) {
      const int i = e / K, k = e - i * K;
      double s = 0.0;
      for (int j = 0; j < K; ++j) s = fma(A[i * kLD + j], R[j * kLD + k], s);
      Tm[i * kLD + k] = s;
    }
    const double sigma = A[0];
    const double isg = sigma > 0.0 ? 1.0 / sigma : 0.0;
    __syncthreads();
    for (int e = tid; e < K * K; e += kThreads) {
      const int i = e / K, k = e - i * K;
      double s = i == k ? 1.0 : 0.0;
      for (int j = 0; j < K; ++j) s = fma(R[j * kLD + i], Tm[j * kLD + k], s);
      A[i * kLD + k] = fma(-Tm[i] * isg, Tm[k], s);
    }
    int cbad = 0;
    for (int k = 0; k < K && !cbad; ++k) {
      __syncthreads();
      const double piv = A[k * kLD + k];  // the same value in every thread
      cbad = !(piv > 0.0) || !__builtin_isfinite(piv);
      const double inv = 1.0 / sqrt(piv);
      __syncthreads();
      if (cbad) break;
      if (tid >= k && tid < K) A[tid * kLD + k] *= inv;
      __syncthreads();
      const int m = K - k - 1;
      for (int e = tid; e < m * m; e += kThreads) {
        const int i = k + 1 + e / m, j = k + 1 + e % m;
        if (j <= i) A[i * kLD + j] = fma(-A[i * kLD + k], A[j * kLD + k], A[i * kLD + j]);
      }
    }
    __syncthreads();
    if (cbad) {
      if (tid == 0) {
        status[d] = kInvalid;
        accepted[d] = 0;
      }
      return;
    }
    if (wid == 0) {  // H dn = grad, lane i holds row i
      const bool in = lane < K;
      const int li = in ? lane : 0;
      double p = in ? gt[li] : 0.0;
      for (int j = 0; j < K; ++j) {
        const double yj = __shfl(p, j, kWave) / A[j * kLD + j];
        if (lane == j) p = yj;
        else if (lane > j && in) p = fma(-A[li * kLD + j], yj, p);
      }
      for (int j = K - 1; j >= 0; --j) {
        const double xj = __shfl(p, j, kWave) / A[j * kLD + j];
        if (lane == j) p = xj;
        else if (lane < j) p = fma(-A[j * kLD + li], xj, p);
      }
      if (in) {
        dnv[lane] = p;
        dn[(size_t)d * K + lane] = p;
      }
    }
  }
  __syncthreads();
  if (conv) nstep = 0.0;  // c = R nu
  if (tid < K) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s = fma(R[tid * kLD + k], fma(nstep, dnv[k], nut[k]), s);
    c[(size_t)d * K + tid] = s;
  }
  if (tid == 0) {
    if (acc) dsd[0] = phit;
    dsd[1] = nstep;
    dsd[2] = sh2 + bb;
    passes[d] = np;
    accepted[d] = acc;
    if (conv) status[d] = kOk;
  }
}

// ------------------------------------------------------- step with exposure equalities
// The generalised step of ops/exposure_qp.py: the multiplier vector is lambda = (nu_T, mu), the
// trial's factor coefficients are c = J lambda, and
//   phi(lambda) = 1/2 sum s^2 h^2 - q'^T h + lambda . J^T x - 1/2 sum d_k lambda_k^2 - tau . lambda
//   grad = J^T x - d o lambda - tau
//   H = diag(d) + J^T (G_f - g g^T / sigma) J + rho diag((1 - d) o D_U)
// (d_k = 1 on the nu slots, 0 on the mu slots; box_step_kernel is the case J = R, d = 1, tau = 0).
// The multipliers of an unattainable target grow without bound, and with them u = a (q' - X c),
// until the projection can no longer hold the budget in double precision.  Every trial's budget
// is therefore tested on x_0 = sum h (the country exposure): a date whose trial misses it is
// stopped (kStalled) before anything of its state changes; the driver alternates between two
// projection buffers, `which` names the one that holds the date's last good trial.
// Dynamic LDS: A, J and Tm = G_f J with the leading dimension K | 1, then ten K-vectors.
__host__ __device__ constexpr size_t eq_lds_bytes(int K) {
  return ((size_t)3 * K * (K | 1) + 10 * kMaxK) * sizeof(double);
}

__global__ __launch_bounds__(kThreads) void eq_step_kernel(
    const double* __restrict__ G, const double* __restrict__ J, const double* __restrict__ dvec,
    const double* __restrict__ tau, const double* __restrict__ DU, const double* __restrict__ F,
    const double* __restrict__ x, const double* __restrict__ pstats,
    const int* __restrict__ pflag, const double* __restrict__ budget, double tol, int K,
    int parity, double* __restrict__ nu, double* __restrict__ grad, double* __restrict__ dn,
    double* __restrict__ c, double* __restrict__ ds, double* __restrict__ rho,
    double* __restrict__ eta, int* __restrict__ passes, int* __restrict__ status,
    int* __restrict__ accepted, int* __restrict__ which) {
  extern __shared__ double eq_lds[];
  const int kLD = K | 1;
  double* A = eq_lds;
  double* Jm = A + K * kLD;
  double* Tm = Jm + K * kLD;
  double* nut = Tm + K * kLD;  // trial lambda, then the current lambda
  double* by = nut + kMaxK;    // J' x
  double* gt = by + kMaxK;     // gradient at the trial
  double* gold = gt + kMaxK;   // gradient at the accepted point
  double* dnv = gold + kMaxK;  // Newton direction
  double* rn = dnv + kMaxK;    // squared norms of J's rows over the nu slots (diagonal of F_TT)
  double* dvv = rn + kMaxK;    // d
  double* tv = dvv + kMaxK;    // tau
  double* xv = tv + kMaxK;     // x = X' h
  double* fx = xv + kMaxK;     // F x
  const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (status[d] != kRunning) return;  // a finished date keeps its state and its c
  const double* Gd = G + (size_t)d * K * K;
  const double* Jd = J + (size_t)d * K * K;
  const double* Fd = F + (size_t)d * K * K;
  const double* xd = x + (size_t)d * K;
  const double* td = tau + (size_t)d * K;
  const double* dud = DU + (size_t)d * K;
  double* dsd = ds + (size_t)d * 4;  // phi, step, variance and exposure gap of the last trial
  const int flag = pflag[d];
  int bad = 0;
  for (int e = tid; e < K * K; e += kThreads) {
    const int i = e / K, k = e - i * K;
    const double gv = Gd[e], jv = Jd[e], fv = Fd[e];
    bad |= !(__builtin_isfinite(gv) && __builtin_isfinite(jv) && __builtin_isfinite(fv));
    A[i * kLD + k] = gv;
    Jm[i * kLD + k] = jv;
    Tm[i * kLD + k] = fv;  // F, until Tm is formed
  }
  for (int e = tid; e < K; e += kThreads) {
    const double xe = xd[e], te = td[e], de = dud[e], dv = dvec[e];
    bad |= !(__builtin_isfinite(xe) && __builtin_isfinite(te) && __builtin_isfinite(de) &&
             __builtin_isfinite(dv));
    xv[e] = xe;
    tv[e] = te;
    dvv[e] = dv;
  }
  const double sh2 = pstats[(size_t)d * 3], qh = pstats[(size_t)d * 3 + 1],
               habs = pstats[(size_t)d * 3 + 2];
  double rh = rho[d];
  bad |= !__builtin_isfinite(rh);
  bad = __syncthreads_or(bad);
  if (flag == 0) bad |= !(__builtin_isfinite(sh2) && __builtin_isfinite(qh));
  if (flag != 0 || bad) {
    if (tid == 0) {
      status[d] = flag == 1 ? kInfeasible : kInvalid;
      accepted[d] = 0;
    }
    return;
  }
  const double phi = dsd[0], step = dsd[1];
  if (tid < K) {
    nut[tid] = fma(step, dn[(size_t)d * K + tid], nu[(size_t)d * K + tid]);
    double s = 0.0, r2 = 0.0, f = 0.0;
    for (int j = 0; j < K; ++j) {
      s = fma(Jm[j * kLD + tid], xv[j], s);
      r2 = fma(Jm[tid * kLD + j] * dvv[j], Jm[tid * kLD + j], r2);
      f = fma(Tm[tid * kLD + j], xv[j], f);
    }
    by[tid] = s;
    rn[tid] = r2;
    fx[tid] = f;
    gold[tid] = grad[(size_t)d * K + tid];
    dnv[tid] = dn[(size_t)d * K + tid];
  }
  __syncthreads();
  // scalars of the trial, the same serial sums in every thread
  double nb = 0.0, nn = 0.0, tl = 0.0, xfx = 0.0, gmax = 0.0, gap = 0.0, gd = 0.0, rmax = 0.0;
  for (int k = 0; k < K; ++k) {
    const double g = by[k] - dvv[k] * nut[k] - tv[k];
    nb = fma(nut[k], by[k], nb);
    nn = fma(dvv[k] * nut[k], nut[k], nn);
    tl = fma(tv[k], nut[k], tl);
    xfx = fma(xv[k], fx[k], xfx);
    if (dvv[k] != 0.0) gmax = fmax(gmax, fabs(g));
    else gap = fmax(gap, fabs(g));
    gd = fma(gold[k], dnv[k], gd);
    rmax = fmax(rmax, rn[k]);
  }
  const double phit = 0.5 * sh2 - qh + nb - 0.5 * nn - tl;
  const int np = passes[d] + 1;
  if (!(__builtin_isfinite(phit) && __builtin_isfinite(gmax) && __builtin_isfinite(gap))) {
    if (tid == 0) {
      status[d] = kInvalid;
      accepted[d] = 0;
    }
    return;
  }
  // the trial's budget, half the 1e-12 (sum |h| + |budget|) that a returned row has to meet
  const double bud = budget[d];
  if (np > 1 && !(fabs(xv[0] - bud) <= 5e-13 * (habs + fabs(bud)))) {
    if (tid == 0) {  // uniform; ds, rho, which and the state keep the last good trial
      status[d] = kStalled;
      accepted[d] = 0;
      passes[d] = np;
    }
    return;
  }
  // converged: the nu block as box_step_kernel, the mu block max |x_S - t| <= tol max(1, sum |h|)
  const double hs = fmax(1.0, habs);
  const bool conv = gmax <= tol * hs * sqrt(rmax) && gap <= tol * hs;
  const bool acc = conv || phit >= phi + 1e-4 * step * gd - 4.0 * kEps * fabs(phit);
  // rho: a tenth after a step accepted at full length, four times after a cut
  if (!acc) rh = fmin(4.0 * rh, 1.0);
  else if (step == 1.0) rh = fmax(rh / 10.0, 1e-14);
  __syncthreads();  // gold / dnv read by every thread before they change
  double nstep = 1.0;
  if (!acc) {  // the maximiser of the parabola through phi(0), phi'(0), phi(step), in [0.1, 0.5] step
    const double den = 2.0 * (phi + gd * step - phit);
    double cut = den > 0.0 ? gd * step * step / den : 0.5 * step;
    if (!(cut == cut)) cut = 0.0;
    nstep = fmin(fmax(cut, 0.1 * step), 0.5 * step);
  }
  if (acc) {
    if (tid < K) {
      const double g = by[tid] - dvv[tid] * nut[tid] - tv[tid];
      gt[tid] = g;
      nu[(size_t)d * K + tid] = nut[tid];
      grad[(size_t)d * K + tid] = g;
    }
  } else if (tid < K) {
    nut[tid] = nu[(size_t)d * K + tid];
  }
  if (acc && !conv) {
    // H = diag(d) + J' (G_f - g g' / sigma) J + rho diag((1 - d) D_U); J' g is row 0 of Tm = G_f J
    for (int e = tid; e < K * K; e += kThreads) {
      const int i = e / K, k = e - i * K;
      double s = 0.0;
      for (int j = 0; j < K; ++j) s = fma(A[i * kLD + j], Jm[j * kLD + k], s);
      Tm[i * kLD + k] = s;
    }
    const double sigma = A[0];
    const double isg = sigma > 0.0 ? 1.0 / sigma : 0.0;
    __syncthreads();
    for (int e = tid; e < K * K; e += kThreads) {
      const int i = e / K, k = e - i * K;
      double s = 0.0;
      if (i == k) s = dvv[i] != 0.0 ? dvv[i] : rh * dud[i];
      for (int j = 0; j < K; ++j) s = fma(Jm[j * kLD + i], Tm[j * kLD + k], s);
      A[i * kLD + k] = fma(-Tm[i] * isg, Tm[k], s);
    }
    int cbad = 0;
    for (int k = 0; k < K && !cbad; ++k) {
      __syncthreads();
      const double piv = A[k * kLD + k];  // the same value in every thread
      cbad = !(piv > 0.0) || !__builtin_isfinite(piv);
      const double inv = 1.0 / sqrt(piv);
      __syncthreads();
      if (cbad) break;
      if (tid >= k && tid < K) A[tid * kLD + k] *= inv;
      __syncthreads();
      const int m = K - k - 1;
      for (int e = tid; e < m * m; e += kThreads) {
        const int i = k + 1 + e / m, j = k + 1 + e % m;
        if (j <= i) A[i * kLD + j] = fma(-A[i * kLD + k], A[j * kLD + k], A[i * kLD + j]);
      }
    }
    __syncthreads();
    if (cbad) {
      if (tid == 0) {
        status[d] = kInvalid;
        accepted[d] = 0;
      }
      return;
    }
    if (wid == 0) {  // H dn = grad, lane i holds row i
      const bool in = lane < K;
      const int li = in ? lane : 0;
      double p = in ? gt[li] : 0.0;
      for (int j = 0; j < K; ++j) {
        const double yj = __shfl(p, j, kWave) / A[j * kLD + j];
        if (lane == j) p = yj;
        else if (lane > j && in) p = fma(-A[li * kLD + j], yj, p);
      }
      for (int j = K - 1; j >= 0; --j) {
        const double xj = __shfl(p, j, kWave) / A[j * kLD + j];
        if (lane == j) p = xj;
        else if (lane < j) p = fma(-A[j * kLD + li], xj, p);
      }
      if (in) {
        dnv[lane] = p;
        dn[(size_t)d * K + lane] = p;
      }
    }
  }
  __syncthreads();
  if (conv) nstep = 0.0;  // c = J lambda
  if (tid < K) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s = fma(Jm[tid * kLD + k], fma(nstep, dnv[k], nut[k]), s);
    c[(size_t)d * K + tid] = s;
    if (conv) {  // eta = -mu + (F x)_S on the mu slots: (Sigma h - q)_n = gamma + (X_S eta)_n
      double e = 0.0;
      if (dvv[tid] == 0.0) {
        for (int j = 0; j < K; ++j) e = fma(Jm[j * kLD + tid], fx[j], e);
        e -= nut[tid];
      }
      eta[(size_t)d * K + tid] = e;
    }
  }
  if (tid == 0) {
    if (acc) dsd[0] = phit;
    dsd[1] = nstep;
    dsd[2] = sh2 + xfx;
    dsd[3] = gap;
    rho[d] = rh;
    passes[d] = np;
    accepted[d] = acc;
    which[d] = parity;
    if (conv) status[d] = kOk;
  }
}

}  // namespace

// u, a, lo, hi, q, h, w [D][N] f64; budget, gamma [D] (gamma: warm start in, root out);
// status [D] int or null (dates whose status is not -1 are left untouched); pstats [D][3] =
// (sum h^2 / a, q' h, sum |h|); pflag [D]: 0 feasible, 1 infeasible, 2 non-finite input.
// mode 0: rows in registers for N <= 5120, re-streamed above; mode 1: always re-streamed.
MFA_API int mfa_box_project(const double* u, const double* a, const double* lo, const double* hi,
                            const double* q, const double* budget, const int* status, int D,
                            int N, int mode, double* gamma, double* h, double* w,
                            double* pstats, int* pflag, void* stream) {
  if (D <= 0) return 0;
  if (N <= 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
#define MFA_E(ee)                                                                              \
  hipLaunchKernelGGL((box_project_kernel<ee>), dim3(D), dim3(kThreads), 0, s, u, a, lo, hi, q, \
                     budget, status, N, gamma, h, w, pstats, pflag)
  if (mode == 1 || N > 20 * kThreads) MFA_E(0);
  else if (N <= 4 * kThreads) MFA_E(4);
  else if (N <= 12 * kThreads) MFA_E(12);
  else MFA_E(20);
#undef MFA_E
  return (int)hipGetLastError();
}

// G [D][K][K] (Gram of the free set), (lam [D][K], U [D][K][K]) eigenpairs of F, x [D][K] = X' h,
// pstats / pflag of mfa_box_project; state per date: nu, grad, dn, c [D][K], ds [D][4] = (phi,
// step, variance of the last trial, spare), passes, status, accepted [D] int.  K <= 64.
MFA_API int mfa_box_step(const double* G, const double* lam, const double* U, const double* x,
                         const double* pstats, const int* pflag, double tol, int D, int K,
                         double* nu, double* grad, double* dn, double* c, double* ds, int* passes,
                         int* status, int* accepted, void* stream) {
  if (D <= 0) return 0;
  if (K < 1 || K > kMaxK) return (int)hipErrorInvalidValue;
  const size_t lds = step_lds_bytes(K);
  static size_t attr = 64 * 1024;  // raise the dynamic-LDS limit once per size
  if (attr < lds) {
    if (hipError_t err = hipFuncSetAttribute((const void*)box_step_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
      return (int)err;
    attr = lds;
  }
  hipLaunchKernelGGL(box_step_kernel, dim3(D), dim3(kThreads), lds, (hipStream_t)stream, G, lam,
                     U, x, pstats, pflag, tol, K, nu, grad, dn, c, ds, passes, status, accepted);
  return (int)hipGetLastError();
}

// The step with exposure equalities.  G, x, pstats, pflag as mfa_box_step; J, F [D][K][K]; dvec
// [K] (1 on the nu slots, 0 on the mu slots); tau, DU [D][K]; state as mfa_box_step with nu
// holding lambda and ds [D][4] = (phi, step, variance, exposure gap of the last trial), plus rho
// [D] and eta [D][K] (written when a date converges: the multipliers on the mu slots, 0 on the
// others); budget [D]; which [D] is set to `parity` for every date whose trial holds the budget,
// a date whose trial misses it gets status 4 and keeps everything else.  K <= 64.
MFA_API int mfa_eq_step(const double* G, const double* J, const double* dvec, const double* tau,
                        const double* DU, const double* F, const double* x, const double* pstats,
                        const int* pflag, const double* budget, double tol, int D, int K,
                        int parity, double* nu, double* grad, double* dn, double* c, double* ds,
                        double* rho, double* eta, int* passes, int* status, int* accepted,
                        int* which, void* stream) {
  if (D <= 0) return 0;
  if (K < 1 || K > kMaxK) return (int)hipErrorInvalidValue;
  const size_t lds = eq_lds_bytes(K);
  static size_t attr = 64 * 1024;  // raise the dynamic-LDS limit once per size
  if (attr < lds) {
    if (hipError_t err = hipFuncSetAttribute((const void*)eq_step_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
      return (int)err;
    attr = lds;
  }
  hipLaunchKernelGGL(eq_step_kernel, dim3(D), dim3(kThreads), lds, (hipStream_t)stream, G, J, dvec,
                     tau, DU, F, x, pstats, pflag, budget, tol, K, parity, nu, grad, dn, c, ds, rho,
                     eta, passes, status, accepted, which);
  return (int)hipGetLastError();
}
