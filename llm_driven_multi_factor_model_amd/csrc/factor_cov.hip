// Factor-structured asset covariance Sigma_d = X_d F_d X_d^T + diag(s_d^2): solve and product
// without an N x N matrix, all dates per launch (gfx950).
//
// X_d is the regression's design matrix [country | one-hot industries | cap-weighted z-scored
// styles] (K = 1 + P + Q columns); it is never materialised: the kernels stream the raw panel
// and fold the z-scoring in from stats = (mu_q, sigma, n) of mfa_xs_wls (design_row.h: the view
// of a date, the validity rule, the fold and its inverse).
// With a_n = 1 / s_n^2 on the universe (0 elsewhere) and F = R R^T (R = U sqrt(max(lambda, 0))),
//   Sigma^-1 b = a o (b - X c),      c = R (I + R^T G R)^-1 R^T g,
//   G = X^T diag(a) X,               g = X^T (a o b)
// (Woodbury in the form that never inverts the only positive semi-definite F), and
//   Sigma h    = s^2 o h + X (F (X^T h)).
// Four kernels, one 256-thread workgroup per date each:
//   factor_gram_kernel    raw panel + a -> G [D][K][K]       (block-structured, order-fixed sums)
//   factor_xty_kernel     X^T h for up to 4 h per pass       (g and X^T h; order-fixed sums)
//   woodbury_coef_kernel  G, eigenpairs of F, g -> c         (K <= 64: M in LDS, Cholesky)
//   factor_apply_kernel   out = u o rhs + v o (X c)          (all right-hand sides in one pass)
#include "design_row.h"

namespace {

using namespace mfa;

constexpr int kApplyNB = 8;   // right-hand sides per factor_apply launch (c lives in LDS)

// ------------------------------------------------------------------------------- factor Gram
// Dense style block: upper-triangle rows [R0, R1) of sum a x_q x_q' in registers.  Up to 12 styles
// run as one part (78 + 13 accumulators); 13..16 styles are split into two row ranges of about
// equal size that run as two workgroups per date (blockIdx.y), so no part spills.
constexpr int tri_count(int Q, int r0, int r1) {
  int n = 0;
  for (int q = r0; q < r1; ++q) n += Q - q;
  return n;
}
constexpr int gram_split(int Q) {
  if (Q <= 12) return Q;
  int s = 0;
  while (2 * tri_count(Q, 0, s) < tri_count(Q, 0, Q)) ++s;
  return s;
}
constexpr int gram_nacc_max(int Q) { return Q * (Q + 1) / 2 + Q + 1; }

__host__ __device__ constexpr size_t gram_lds_doubles(int Pseg, int Q) {
  return (size_t)kWaves * Pseg * (Q + 1) + (size_t)(kWaves + 1) * (Q * (Q + 1) / 2 + Q + 1);
}

// Sums of part [R0, R1) of date d, then this part's entries of G_d.  The part with R0 == 0 also
// owns the country / industry rows and columns.  Industry sums (sum a, sum a x_q per industry)
// go to one LDS table per wave: only that wave's atomics land in it, in program order, and the
// four tables are summed in wave order; the dense sums are reduced lane -> wave (DPP) -> waves in
// a fixed order.  Two runs therefore give the same bits.
template <int Q, int R0, int R1, typename T>
__device__ __forceinline__ void gram_body(const T* __restrict__ X, const T* __restrict__ cap,
                                          const T* __restrict__ ret,
                                          const int16_t* __restrict__ ind,
                                          const double* __restrict__ a,
                                          const double* __restrict__ stats, int N, int P,
                                          double* __restrict__ G, double* lds) {
  constexpr int NT = tri_count(Q, R0, R1), NACC = NT + Q + 1, QS = Q + 1;
  constexpr bool LEAD = R0 == 0;
  const int d = blockIdx.x, tid = threadIdx.x, wid = tid >> 6;
  const DesignDate<T> day(X, cap, ret, ind, d, N, P, Q);
  const int Pseg = day.Pseg, K = 1 + P + Q;
  double* seg = lds;                              // [kWaves][Pseg][QS]
  double* red = seg + (size_t)kWaves * Pseg * QS;  // [kWaves][NACC]
  double* tot = red + kWaves * gram_nacc_max(Q);   // [NACC]
  if (LEAD && P > 0)
    for (int i = tid; i < kWaves * Pseg * QS; i += kThreads) seg[i] = 0.0;
  __syncthreads();
  const double* ad = a + (size_t)d * N;
  double* myseg = seg + (size_t)wid * Pseg * QS;
  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
  for (int n = tid; n < N; n += kThreads) {
    T c, r, xf[Q];
    int j;
    day.load_base(n, c, r, j);
    const double an = ad[n];
    bool ok = __builtin_isfinite(an) && (an > 0.0) && day.base_ok(c, r, j);
    day.load_styles_ok(n, xf, ok);
    if (!ok) continue;
    double x[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) x[q] = (double)xf[q];
    int idx = 0;
#pragma unroll
    for (int q = R0; q < R1; ++q) {
      const double aq = an * x[q];
#pragma unroll
      for (int q2 = q; q2 < Q; ++q2) {
        acc[idx] = fma(aq, x[q2], acc[idx]);
        ++idx;
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[NT + q] = fma(an, x[q], acc[NT + q]);
    acc[NT + Q] += an;
    if (LEAD && P > 0) {
      double* s = myseg + j * QS;
#pragma unroll
      for (int q = 0; q < Q; ++q) atomicAdd(s + q, an * x[q]);
      atomicAdd(s + Q, an);
    }
  }
  wave_totals(acc, red);
  __syncthreads();
  for (int i = tid; i < NACC; i += kThreads) tot[i] = sum4(red, NACC, i);
  if (LEAD && P > 0)  // entry i of the four tables is touched by this thread only
    for (int i = tid; i < Pseg * QS; i += kThreads) seg[i] = sum4(seg, Pseg * QS, i);
  __syncthreads();
  const double* st = stats + (size_t)d * (Q + 2);
  const bool bad = !stats_finite(st, Q);
  const double isig = 1.0 / st[Q];
  const double S0 = tot[NT + Q];
  double* Gd = G + (size_t)d * K * K;
  for (int e = tid; e < K * K; e += kThreads) {
    int r = e / K, c = e - r * K;
    if (r > c) {  // symmetric: evaluate the upper-triangle twin
      const int t = r;
      r = c;
      c = t;
    }
    double v;
    if (c <= P) {  // country / industry block
      if (!LEAD) continue;
      if (r == 0) v = c == 0 ? S0 : seg[(c - 1) * QS + Q];
      else v = r == c ? seg[(r - 1) * QS + Q] : 0.0;
    } else if (r <= P) {  // country / industry x style
      if (!LEAD) continue;
      const int q = c - 1 - P;
      if (r == 0) v = unfold_zscore(tot[NT + q], st[q], S0, isig);
      else v = unfold_zscore(seg[(r - 1) * QS + q], st[q], seg[(r - 1) * QS + Q], isig);
    } else {  // style x style, owned by the part that holds the smaller row
      const int qa = r - 1 - P, qb = c - 1 - P;
      if (qa < R0 || qa >= R1) continue;
      int off = 0;
      for (int t = R0; t < qa; ++t) off += Q - t;
      const double ma = st[qa], mb = st[qb];
      v = (tot[off + qb - qa] - ma * tot[NT + qb] - mb * tot[NT + qa] + ma * mb * S0) * isig *
          isig;
    }
    Gd[e] = bad ? qnan() : v;
  }
}

template <int Q, typename T>
__global__ __launch_bounds__(kThreads) void factor_gram_kernel(
    const T* __restrict__ X, const T* __restrict__ cap, const T* __restrict__ ret,
    const int16_t* __restrict__ ind, const double* __restrict__ a,
    const double* __restrict__ stats, int N, int P, double* __restrict__ G) {
  extern __shared__ double gram_lds[];
  constexpr int S = gram_split(Q);
  if constexpr (S == Q) {
    gram_body<Q, 0, Q, T>(X, cap, ret, ind, a, stats, N, P, G, gram_lds);
  } else {
    if (blockIdx.y == 0) gram_body<Q, 0, S, T>(X, cap, ret, ind, a, stats, N, P, G, gram_lds);
    else gram_body<Q, S, Q, T>(X, cap, ret, ind, a, stats, N, P, G, gram_lds);
  }
}

template <typename T>
int factor_gram_dispatch(const T* X, const T* cap, const T* ret, const int16_t* ind,
                         const double* a, const double* stats, int D, int N, int P, int Q,
                         double* G, void* stream) {
  if (D <= 0) return 0;
  if (Q < 1 || Q > kMaxQ || P < 0 || 1 + P + Q > kMaxK || N <= 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = gram_lds_doubles(P > 0 ? P : 1, Q) * sizeof(double);
  const bool known = dispatch_q(Q, [&](auto q) {
    constexpr int QQ = decltype(q)::value;
    hipLaunchKernelGGL((factor_gram_kernel<QQ, T>), dim3(D, gram_split(QQ) == QQ ? 1 : 2),
                       dim3(kThreads), lds, s, X, cap, ret, P > 0 ? ind : nullptr, a, stats, N, P,
                       G);
  });
  return known ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

// --------------------------------------------------------------------------- X^T h, many h
// out[d, b, :] = X_d^T h[d, b, :] for nb <= kXtyNB right-hand sides [b0, b0 + nb) of NB in one pass
// over the panel: the exposures of attribution.hip's portfolio_exposure_kernel (invalid stocks
// and non-finite h contribute nothing), with the order-fixed reductions of the Gram kernel (one
// industry table per wave) instead of cross-wave LDS atomics.
constexpr int kXtyNB = 4;

__host__ __device__ constexpr size_t xty_lds_doubles(int Pseg, int Q) {
  return (size_t)kWaves * kXtyNB * Pseg + (size_t)(kWaves + 1) * kXtyNB * (Q + 1);
}

template <int Q, typename T>
__global__ __launch_bounds__(kThreads) void factor_xty_kernel(
    const T* __restrict__ X, const T* __restrict__ cap, const T* __restrict__ ret,
    const int16_t* __restrict__ ind, const double* __restrict__ h,
    const double* __restrict__ stats, int N, int P, int NB, int b0, int nb,
    double* __restrict__ out) {
  extern __shared__ double xty_lds[];
  constexpr int QS = Q + 1, NACC = kXtyNB * QS;
  const int d = blockIdx.x, tid = threadIdx.x, wid = tid >> 6;
  const int Pseg = P > 0 ? P : 1, K = 1 + P + Q;
  double* seg = xty_lds;                                   // [kWaves][kXtyNB][Pseg]
  double* red = seg + (size_t)kWaves * kXtyNB * Pseg;       // [kWaves][NACC]
  double* tot = red + kWaves * NACC;                        // [NACC]
  if (P > 0)
    for (int i = tid; i < kWaves * kXtyNB * Pseg; i += kThreads) seg[i] = 0.0;
  __syncthreads();
  // this kernel keeps its own pointers and style loop; the rule is design_row.h's
  const T* Xd = X + (size_t)d * Q * N;
  const T* cd = cap + (size_t)d * N;
  const T* rd = ret + (size_t)d * N;
  const int16_t* id = ind ? ind + (size_t)d * N : nullptr;
  const double* hd = h + ((size_t)d * NB + b0) * N;
  double* myseg = seg + (size_t)wid * kXtyNB * Pseg;
  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
  for (int n = tid; n < N; n += kThreads) {
    const T c = cd[n], r = rd[n];
    const int j = id ? (int)id[n] : 0;
    bool ok = design_base_ok(c, r, j, Pseg);
    double x[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const T xf = Xd[(size_t)q * N + n];
      ok = ok && __builtin_isfinite(xf);
      x[q] = (double)xf;
    }
    if (!ok) continue;
#pragma unroll
    for (int b = 0; b < kXtyNB; ++b) {
      if (b < nb) {
        const double hv = hd[(size_t)b * N + n];
        const double w = __builtin_isfinite(hv) ? hv : 0.0;
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[b * QS + q] = fma(w, x[q], acc[b * QS + q]);
        acc[b * QS + Q] += w;
        if (P > 0 && w != 0.0) atomicAdd(myseg + b * Pseg + j, w);
      }
    }
  }
  wave_totals(acc, red);
  __syncthreads();
  for (int i = tid; i < NACC; i += kThreads) tot[i] = sum4(red, NACC, i);
  if (P > 0)  // entry i of the four tables is touched by this thread only
    for (int i = tid; i < kXtyNB * Pseg; i += kThreads) seg[i] = sum4(seg, kXtyNB * Pseg, i);
  __syncthreads();
  const double* st = stats + (size_t)d * (Q + 2);
  const double isig = 1.0 / st[Q];
  for (int e = tid; e < nb * K; e += kThreads) {
    const int b = e / K, k = e - b * K;
    const double hs = tot[b * QS + Q];
    double v;
    if (k == 0) v = hs;
    else if (k <= P) v = seg[b * Pseg + k - 1];
    else v = unfold_zscore(tot[b * QS + k - 1 - P], st[k - 1 - P], hs, isig);
    out[((size_t)d * NB + b0 + b) * K + k] = v;
  }
}

template <typename T>
int factor_xty_dispatch(const T* X, const T* cap, const T* ret, const int16_t* ind,
                        const double* h, const double* stats, int D, int N, int P, int Q, int NB,
                        int b0, int nb, double* out, void* stream) {
  if (D <= 0 || nb <= 0) return 0;
  if (Q < 1 || Q > kMaxQ || P < 0 || 1 + P + Q > kMaxK || N <= 0 || b0 < 0 || nb > kXtyNB ||
      b0 + nb > NB)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = xty_lds_doubles(P > 0 ? P : 1, Q) * sizeof(double);
  const bool known = dispatch_q(Q, [&](auto q) {
    hipLaunchKernelGGL((factor_xty_kernel<decltype(q)::value, T>), dim3(D), dim3(kThreads), lds, s,
                       X, cap, ret, P > 0 ? ind : nullptr, h, stats, N, P, NB, b0, nb, out);
  });
  return known ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

// ------------------------------------------------------------------------ Woodbury inner solve
// c_b = R M^-1 R^T g_b with M = I + R^T G R (symmetric positive definite whatever the rank of F).
// The three K x K matrices sit in dynamic LDS with an odd leading dimension K | 1 (column reads
// conflict-free; 43 KB at K = 42, so three dates share a CU; 98 KB at K = 64);
// Cholesky is right-looking over the lower triangle; each wave then takes right-hand sides
// b = wave, wave + 4, ... with lane i holding row i of the triangular solves.  Any non-finite
// input or a non-positive pivot gives NaN for every c of the date.
__host__ __device__ constexpr size_t woodbury_lds_bytes(int K) {
  return (size_t)3 * K * (K | 1) * sizeof(double);
}

__global__ __launch_bounds__(kThreads) void woodbury_coef_kernel(
    const double* __restrict__ G, const double* __restrict__ w, const double* __restrict__ U,
    const double* __restrict__ g, int NB, int K, double* __restrict__ c) {
  extern __shared__ double wb_lds[];
  const int kLD = K | 1;
  double* A = wb_lds;         // G, then M and its Cholesky factor
  double* R = A + K * kLD;    // U sqrt(max(lambda, 0))
  double* Tm = R + K * kLD;   // G R
  const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const double* Gd = G + (size_t)d * K * K;
  const double* Ud = U + (size_t)d * K * K;
  const double* wd = w + (size_t)d * K;
  const double* gd = g + (size_t)d * NB * K;
  double* cd = c + (size_t)d * NB * K;
  int bad = 0;
  for (int e = tid; e < K * K; e += kThreads) {
    const int i = e / K, k = e - i * K;
    const double gv = Gd[e], uv = Ud[e], lam = wd[k];
    bad |= !(__builtin_isfinite(gv) && __builtin_isfinite(uv) && __builtin_isfinite(lam));
    A[i * kLD + k] = gv;
    R[i * kLD + k] = uv * sqrt(lam > 0.0 ? lam : 0.0);
  }
  for (int e = tid; e < NB * K; e += kThreads) bad |= !__builtin_isfinite(gd[e]);
  bad = __syncthreads_or(bad);
  if (!bad) {
    for (int e = tid; e < K * K; e += kThreads) {
      const int i = e / K, k = e - i * K;
      double s = 0.0;
      for (int j = 0; j < K; ++j) s = fma(A[i * kLD + j], R[j * kLD + k], s);
      Tm[i * kLD + k] = s;
    }
    __syncthreads();
    for (int e = tid; e < K * K; e += kThreads) {
      const int i = e / K, k = e - i * K;
      double s = i == k ? 1.0 : 0.0;
      for (int j = 0; j < K; ++j) s = fma(R[j * kLD + i], Tm[j * kLD + k], s);
      A[i * kLD + k] = s;
    }
    for (int k = 0; k < K && !bad; ++k) {
      __syncthreads();
      const double piv = A[k * kLD + k];  // the same value in every thread
      bad = !(piv > 0.0) || !__builtin_isfinite(piv);
      const double inv = 1.0 / sqrt(piv);
      __syncthreads();
      if (bad) break;
      if (tid >= k && tid < K) A[tid * kLD + k] *= inv;
      __syncthreads();
      const int m = K - k - 1;
      for (int e = tid; e < m * m; e += kThreads) {
        const int i = k + 1 + e / m, j = k + 1 + e % m;
        if (j <= i) A[i * kLD + j] = fma(-A[i * kLD + k], A[j * kLD + k], A[i * kLD + j]);
      }
    }
    __syncthreads();
  }
  if (bad) {
    for (int e = tid; e < NB * K; e += kThreads) cd[e] = qnan();
    return;
  }
  const bool in = lane < K;
  const int li = in ? lane : 0;
  for (int b = wid; b < NB; b += kWaves) {
    double p = 0.0;  // (R^T g)_lane
    for (int j = 0; j < K; ++j) p = fma(R[j * kLD + li], gd[b * K + j], p);
    if (!in) p = 0.0;
    for (int j = 0; j < K; ++j) {  // L y = p, column by column
      const double yj = __shfl(p, j, kWave) / A[j * kLD + j];
      if (lane == j) p = yj;
      else if (lane > j && in) p = fma(-A[li * kLD + j], yj, p);
    }
    for (int j = K - 1; j >= 0; --j) {  // L^T x = y
      const double xj = __shfl(p, j, kWave) / A[j * kLD + j];
      if (lane == j) p = xj;
      else if (lane < j) p = fma(-A[j * kLD + li], xj, p);
    }
    double s = 0.0;  // (R x)_lane
    for (int k = 0; k < K; ++k) s = fma(R[li * kLD + k], __shfl(p, k, kWave), s);
    if (in) cd[b * K + lane] = s;
  }
}

// ------------------------------------------------------------------------------------- apply
// out[d, b, n] = u[d, n] rhs[d, b, n] + v[d, n] (x_n . c[d, b]) for nb <= kApplyNB right-hand
// sides [b0, b0 + nb) of NB.  In the universe (regression-valid and v != 0); 0 outside it;
// non-finite rhs entries count as 0; a date whose c_b is not finite gets NaN for all of row b.
// The z-scoring is folded into c once per date: x . c = c0' + c_ind[j] + sum_q X_q c_q / sigma.
template <int Q, typename T>
__global__ __launch_bounds__(kThreads) void factor_apply_kernel(
    const T* __restrict__ X, const T* __restrict__ cap, const T* __restrict__ ret,
    const int16_t* __restrict__ ind, const double* __restrict__ u, const double* __restrict__ v,
    const double* __restrict__ stats, const double* __restrict__ rhs,
    const double* __restrict__ c, int N, int P, int NB, int b0, int nb,
    double* __restrict__ out) {
  __shared__ double cc[kApplyNB][kMaxK];
  __shared__ int badb[kApplyNB];
  const int d = blockIdx.x, tid = threadIdx.x;
  const DesignDate<T> day(X, cap, ret, ind, d, N, P, Q);
  const int K = 1 + P + Q;
  const double* st = stats + (size_t)d * (Q + 2);
  if (tid < nb) {  // one thread per right-hand side: fold (mu, sigma) into c, flag NaN
    const double* cb = c + ((size_t)d * NB + b0 + tid) * K;
    fold_zscore(cb, st, P, Q, cc[tid]);
    // the country coefficient as given, the industry and the folded style coefficients
    bool bad = !stats_finite(st, Q) || !__builtin_isfinite(cb[0]);
    for (int k = 1; k < K; ++k) bad = bad || !__builtin_isfinite(cc[tid][k]);
    badb[tid] = bad;
  }
  __syncthreads();
  const double* ud = u + (size_t)d * N;
  const double* vd = v + (size_t)d * N;
  const double* rb = rhs + ((size_t)d * NB + b0) * N;
  double* ob = out + ((size_t)d * NB + b0) * N;
  for (int n = tid; n < N; n += kThreads) {
    T cp, r, xf[Q];
    int j;
    day.load_base(n, cp, r, j);
    const double un = ud[n], vn = vd[n];
    bool ok = __builtin_isfinite(un) && __builtin_isfinite(vn) && (vn != 0.0) &&
              day.base_ok(cp, r, j);
    day.load_styles_ok(n, xf, ok);
    double x[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) x[q] = (double)xf[q];
    const int jj = (ok && P > 0) ? 1 + j : 0;
    for (int b = 0; b < nb; ++b) {
      double val = 0.0;
      if (ok) {
        double dot = cc[b][0] + (P > 0 ? cc[b][jj] : 0.0);
#pragma unroll
        for (int q = 0; q < Q; ++q) dot = fma(x[q], cc[b][1 + P + q], dot);
        const double h = rb[(size_t)b * N + n];
        val = fma(vn, dot, un * (__builtin_isfinite(h) ? h : 0.0));
      }
      if (badb[b]) val = qnan();
      __builtin_nontemporal_store(val, ob + (size_t)b * N + n);
    }
  }
}

template <typename T>
int factor_apply_dispatch(const T* X, const T* cap, const T* ret, const int16_t* ind,
                          const double* u, const double* v, const double* stats,
                          const double* rhs, const double* c, int D, int N, int P, int Q, int NB,
                          int b0, int nb, double* out, void* stream) {
  if (D <= 0 || nb <= 0) return 0;
  if (Q < 1 || Q > kMaxQ || P < 0 || 1 + P + Q > kMaxK || N <= 0 || b0 < 0 || nb > kApplyNB ||
      b0 + nb > NB)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const bool known = dispatch_q(Q, [&](auto q) {
    hipLaunchKernelGGL((factor_apply_kernel<decltype(q)::value, T>), dim3(D), dim3(kThreads), 0, s,
                       X, cap, ret, P > 0 ? ind : nullptr, u, v, stats, rhs, c, N, P, NB, b0, nb,
                       out);
  });
  return known ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

}  // namespace

// X [D][Q][N], cap/ret [D][N] f32 (validity only), ind [D][N] int16 (nullable when P == 0),
// a [D][N] f64 stock weights (<= 0 or non-finite: outside the universe), stats [D][Q+2] f64 from
// mfa_xs_wls.  G [D][K][K] f64 = X^T diag(a) X, K = 1 + P + Q <= 64, Q <= 16; NaN for a date
// whose stats row is not finite.
MFA_API int mfa_factor_gram(const float* X, const float* cap, const float* ret,
                            const int16_t* ind, const double* a, const double* stats, int D, int N,
                            int P, int Q, double* G, void* stream) {
  return factor_gram_dispatch<float>(X, cap, ret, ind, a, stats, D, N, P, Q, G, stream);
}

// Same with an fp64 panel.
MFA_API int mfa_factor_gram_f64(const double* X, const double* cap, const double* ret,
                                const int16_t* ind, const double* a, const double* stats, int D,
                                int N, int P, int Q, double* G, void* stream) {
  return factor_gram_dispatch<double>(X, cap, ret, ind, a, stats, D, N, P, Q, G, stream);
}

// out[d][b][:] = X_d^T h[d][b][:] for b in [b0, b0 + nb), nb <= 4; h [D][NB][N] f64 (non-finite
// entries count as 0), out [D][NB][K] f64.  Bitwise reproducible.
MFA_API int mfa_factor_xty(const float* X, const float* cap, const float* ret, const int16_t* ind,
                           const double* h, const double* stats, int D, int N, int P, int Q,
                           int NB, int b0, int nb, double* out, void* stream) {
  return factor_xty_dispatch<float>(X, cap, ret, ind, h, stats, D, N, P, Q, NB, b0, nb, out,
                                    stream);
}

// Same with an fp64 panel.
MFA_API int mfa_factor_xty_f64(const double* X, const double* cap, const double* ret,
                               const int16_t* ind, const double* h, const double* stats, int D,
                               int N, int P, int Q, int NB, int b0, int nb, double* out,
                               void* stream) {
  return factor_xty_dispatch<double>(X, cap, ret, ind, h, stats, D, N, P, Q, NB, b0, nb, out,
                                     stream);
}

// G [D][K][K], (w [D][K], U [D][K][K]) = eigenpairs of F (U's columns), g [D][NB][K];
// c [D][NB][K] = R (I + R^T G R)^-1 R^T g with R = U sqrt(max(w, 0)).  K <= 64.
MFA_API int mfa_woodbury_coef(const double* G, const double* w, const double* U, const double* g,
                              int D, int NB, int K, double* c, void* stream) {
  if (D <= 0 || NB <= 0) return 0;
  if (K < 1 || K > kMaxK) return (int)hipErrorInvalidValue;
  const size_t lds = woodbury_lds_bytes(K);
  if (hipError_t err = raise_dynamic_lds<woodbury_coef_kernel>(lds)) return (int)err;
  hipLaunchKernelGGL(woodbury_coef_kernel, dim3(D), dim3(kThreads), lds, (hipStream_t)stream, G,
                     w, U, g, NB, K, c);
  return (int)hipGetLastError();
}

// out[d][b][n] = u[d][n] rhs[d][b][n] + v[d][n] (x_n . c[d][b]) for b in [b0, b0 + nb), nb <= 8;
// rhs / out [D][NB][N], c [D][NB][K], u / v [D][N] (v == 0: outside the universe).
MFA_API int mfa_factor_apply(const float* X, const float* cap, const float* ret,
                             const int16_t* ind, const double* u, const double* v,
                             const double* stats, const double* rhs, const double* c, int D, int N,
                             int P, int Q, int NB, int b0, int nb, double* out, void* stream) {
  return factor_apply_dispatch<float>(X, cap, ret, ind, u, v, stats, rhs, c, D, N, P, Q, NB, b0,
                                      nb, out, stream);
}

// Same with an fp64 panel.
MFA_API int mfa_factor_apply_f64(const double* X, const double* cap, const double* ret,
                                 const int16_t* ind, const double* u, const double* v,
                                 const double* stats, const double* rhs, const double* c, int D,
                                 int N, int P, int Q, int NB, int b0, int nb, double* out,
                                 void* stream) {
  return factor_apply_dispatch<double>(X, cap, ret, ind, u, v, stats, rhs, c, D, N, P, Q, NB, b0,
                                       nb, out, stream);
}
