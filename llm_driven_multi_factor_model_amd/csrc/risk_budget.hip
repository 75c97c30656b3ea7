// Risk-budgeting (risk-parity) portfolios on the factor-structured covariance
// Sigma_d = X_d F_d X_d^T + diag(s_d^2), all dates per launch (gfx950).
//
// Spinu's formulation: y > 0 minimises phi(y) = 1/2 y' Sigma y - sum_U b_n ln y_n (b scaled to
// sum_U b = |U|); at the minimiser y_n (Sigma y)_n = b_n and h = budget y / sum y.  The Hessian
// Sigma + diag(b / y^2) is again "factor part + diagonal", so a Newton step is a Woodbury solve
// with the diagonal 1 / a_n = s_n^2 + b_n / y_n^2.  At an iterate y with x = X' y, z = F x:
//   Sy_n = s_n^2 y_n + x_n . z,   g_n = Sy_n - b_n / y_n,   a_n = 1 / (s_n^2 + b_n / y_n^2),
//   G = X' diag(a) X,  v = X' (a o g),  sigma = sum a g^2,  r = max |y_n Sy_n / b_n - 1|,
//   c = R (I + R' G R)^-1 R' v  (F = R R'),  lambda = sqrt(max(sigma - v' c, 0)),
//   delta_n = -a_n (g_n - x_n . c).
// One pass = three launches, one 256-thread workgroup per date each:
//   rb_moments_kernel  panel + trial y -> G, v, (sigma, r, phi, y' Sigma y)     (one stream)
//   rb_step_kernel     accept / reject / converged; on accept c and lambda      (Cholesky in LDS)
//   rb_update_kernel   panel + saved y + c -> trial y and x = X' y_trial        (one stream)
// Every date keeps two iterates, y [2][D][N] and x [2][D][K]: sel[d] names the saved (last
// accepted) one, 1 - sel[d] the trial.  Accepting a trial flips sel; a rejected trial is
// overwritten by the damped Newton step from the saved iterate.  All sums run in a fixed order
// (design_row.h), so two runs give the same bits, and a date never reads another date's data.
#include "design_row.h"

namespace {

using namespace mfa;

constexpr int kRunning = -1, kOk = 0, kInvalid = 3;  // ops/risk_budget.py
constexpr int kClamped = 0, kDamped = 1;             // how the date's trial was formed
constexpr int kDs = 5;  // ds [D][5] = (phi, lambda, damped step length, y' Sigma y, r) of the saved iterate

// ----------------------------------------------------------------------------------- moments
// The style triangle of G as gram_body of factor_cov.hip holds it: rows [R0, R1) in registers.
// The part with R0 == 0 also owns everything else (v, the scalars, the industry tables), Q + 4
// more sums and a running max per lane, so the triangle is split over two workgroups from 11
// styles on, at the row that balances the two parts' accumulators.
constexpr int tri_count(int Q, int r0, int r1) {
  int n = 0;
  for (int q = r0; q < r1; ++q) n += Q - q;
  return n;
}
constexpr int rb_extra(int Q) { return Q + 4; }  // sum w x_q, sum w, sigma, y' Sigma y, sum b ln y
constexpr int rb_split(int Q) {
  if (Q <= 10) return Q;
  int s = 0;
  while (2 * tri_count(Q, 0, s) + rb_extra(Q) < tri_count(Q, 0, Q)) ++s;
  return s;
}
constexpr int rb_nacc_max(int Q) { return Q * (Q + 1) / 2 + Q + 1 + rb_extra(Q); }

__host__ __device__ constexpr size_t moments_lds_doubles(int Pseg, int Q) {
  return (size_t)kWaves * Pseg * (Q + 2) + (size_t)(kWaves + 1) * rb_nacc_max(Q) + 2 * kMaxK +
         kWaves;
}

// z = F x by the first K threads (serial over l), then the z-scoring folded in by thread 0.
__device__ __forceinline__ void fold_Fx(const double* __restrict__ Fd, const double* __restrict__ xd,
                                        const double* st, int P, int Q, double* raw, double* zz) {
  const int K = 1 + P + Q, tid = threadIdx.x;
  if (tid < K) {
    double s = 0.0;
    for (int l = 0; l < K; ++l) s = fma(Fd[tid * K + l], xd[l], s);
    raw[tid] = s;
  }
  __syncthreads();
  if (tid == 0) fold_zscore(raw, st, P, Q, zz);
  __syncthreads();
}

template <int Q, int R0, int R1, typename T>
__device__ __forceinline__ void moments_body(
    const T* __restrict__ X, const T* __restrict__ cap, const T* __restrict__ ret,
    const int16_t* __restrict__ ind, const double* __restrict__ ybuf,
    const double* __restrict__ xbuf, const int* __restrict__ sel, const double* __restrict__ bt,
    const double* __restrict__ s2, const double* __restrict__ F, const double* __restrict__ stats,
    int N, int P, double* __restrict__ G, double* __restrict__ v, double* __restrict__ sc,
    double* lds) {
  constexpr bool LEAD = R0 == 0;
  constexpr int NT = tri_count(Q, R0, R1), V0 = NT + Q + 1;
  constexpr int NACC = V0 + (LEAD ? rb_extra(Q) : 0), QS = Q + 2;
  const int d = blockIdx.x, D = gridDim.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const DesignDate<T> day(X, cap, ret, ind, d, N, P, Q);
  const int Pseg = day.Pseg, K = 1 + P + Q;
  double* seg = lds;                               // [kWaves][Pseg][QS]: a x_q, a, a g
  double* red = seg + (size_t)kWaves * Pseg * QS;   // [kWaves][NACC]
  double* tot = red + kWaves * rb_nacc_max(Q);      // [NACC]
  double* zz = tot + rb_nacc_max(Q);                // [kMaxK] z with the z-scoring folded in
  double* raw = zz + kMaxK;                         // [kMaxK] z = F x
  double* rmx = raw + kMaxK;                        // [kWaves]
  const int tb = 1 - (sel[d] & 1);                  // the trial iterate
  const double* yd = ybuf + ((size_t)tb * D + d) * N;
  const double* bd = bt + (size_t)d * N;
  const double* sd = s2 + (size_t)d * N;
  const double* st = stats + (size_t)d * (Q + 2);
  if (LEAD && P > 0)
    for (int i = tid; i < kWaves * Pseg * QS; i += kThreads) seg[i] = 0.0;
  if constexpr (LEAD)
    fold_Fx(F + (size_t)d * K * K, xbuf + ((size_t)tb * D + d) * K, st, P, Q, raw, zz);
  else
    __syncthreads();
  double* myseg = seg + (size_t)wid * Pseg * QS;
  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
  double rmax = 0.0;
  for (int n = tid; n < N; n += kThreads) {
    T c, r, xf[Q];
    int j;
    day.load_base(n, c, r, j);
    const double b = bd[n], yn = yd[n], s2n = sd[n];
    bool ok = __builtin_isfinite(b) && (b > 0.0) && (yn > 0.0) && day.base_ok(c, r, j);
    day.load_styles_ok(n, xf, ok);
    if (!ok) continue;
    double x[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) x[q] = (double)xf[q];
    const double by = b / yn;
    const double an = 1.0 / (s2n + by / yn);
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
    if constexpr (LEAD) {
      double dot = zz[0] + (P > 0 ? zz[1 + j] : 0.0);
#pragma unroll
      for (int q = 0; q < Q; ++q) dot = fma(x[q], zz[1 + P + q], dot);
      const double Sy = fma(s2n, yn, dot);
      const double g = Sy - by;
      const double w = an * g;
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[V0 + q] = fma(w, x[q], acc[V0 + q]);
      acc[V0 + Q] += w;
      acc[V0 + Q + 1] = fma(w, g, acc[V0 + Q + 1]);
      acc[V0 + Q + 2] = fma(yn, Sy, acc[V0 + Q + 2]);
      acc[V0 + Q + 3] = fma(b, log(yn), acc[V0 + Q + 3]);
      rmax = fmax(rmax, fabs(yn * Sy / b - 1.0));
      if (P > 0) {
        double* s = myseg + j * QS;
#pragma unroll
        for (int q = 0; q < Q; ++q) atomicAdd(s + q, an * x[q]);
        atomicAdd(s + Q, an);
        atomicAdd(s + Q + 1, w);
      }
    }
  }
  wave_totals(acc, red);
  if constexpr (LEAD) {
    rmax = wave_max(rmax);
    if (lane == 0) rmx[wid] = rmax;
  }
  __syncthreads();
  for (int i = tid; i < NACC; i += kThreads) tot[i] = sum4(red, NACC, i);
  if (LEAD && P > 0)  // entry i of the four tables is touched by this thread only
    for (int i = tid; i < Pseg * QS; i += kThreads) seg[i] = sum4(seg, Pseg * QS, i);
  __syncthreads();
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
    double val;
    if (c <= P) {  // country / industry block
      if (!LEAD) continue;
      if (r == 0) val = c == 0 ? S0 : seg[(c - 1) * QS + Q];
      else val = r == c ? seg[(r - 1) * QS + Q] : 0.0;
    } else if (r <= P) {  // country / industry x style
      if (!LEAD) continue;
      const int q = c - 1 - P;
      if (r == 0) val = unfold_zscore(tot[NT + q], st[q], S0, isig);
      else val = unfold_zscore(seg[(r - 1) * QS + q], st[q], seg[(r - 1) * QS + Q], isig);
    } else {  // style x style, owned by the part that holds the smaller row
      const int qa = r - 1 - P, qb = c - 1 - P;
      if (qa < R0 || qa >= R1) continue;
      int off = 0;
      for (int t = R0; t < qa; ++t) off += Q - t;
      const double ma = st[qa], mb = st[qb];
      val = (tot[off + qb - qa] - ma * tot[NT + qb] - mb * tot[NT + qa] + ma * mb * S0) * isig *
            isig;
    }
    Gd[e] = bad ? qnan() : val;
  }
  if constexpr (LEAD) {
    const double Sw = tot[V0 + Q];
    for (int k = tid; k < K; k += kThreads) {
      double val;
      if (k == 0) val = Sw;
      else if (k <= P) val = seg[(k - 1) * QS + Q + 1];
      else val = unfold_zscore(tot[V0 + k - 1 - P], st[k - 1 - P], Sw, isig);
      v[(size_t)d * K + k] = bad ? qnan() : val;
    }
    if (tid == 0) {
      double* o = sc + (size_t)d * 4;
      const double ysy = tot[V0 + Q + 2];
      o[0] = tot[V0 + Q + 1];
      o[1] = fmax(fmax(rmx[0], rmx[1]), fmax(rmx[2], rmx[3]));
      o[2] = 0.5 * ysy - tot[V0 + Q + 3];
      o[3] = ysy;
    }
  }
}

template <int Q, typename T>
__global__ __launch_bounds__(kThreads) void rb_moments_kernel(
    const T* __restrict__ X, const T* __restrict__ cap, const T* __restrict__ ret,
    const int16_t* __restrict__ ind, const double* __restrict__ ybuf,
    const double* __restrict__ xbuf, const int* __restrict__ sel, const double* __restrict__ bt,
    const double* __restrict__ s2, const double* __restrict__ F, const double* __restrict__ stats,
    const int* __restrict__ status, int N, int P, double* __restrict__ G, double* __restrict__ v,
    double* __restrict__ sc) {
  extern __shared__ double rbm_lds[];
  if (status[blockIdx.x] != kRunning) return;  // a finished date keeps its G, v and scalars
  constexpr int S = rb_split(Q);
  if constexpr (S == Q) {
    moments_body<Q, 0, Q, T>(X, cap, ret, ind, ybuf, xbuf, sel, bt, s2, F, stats, N, P, G, v, sc,
                             rbm_lds);
  } else {
    if (blockIdx.y == 0)
      moments_body<Q, 0, S, T>(X, cap, ret, ind, ybuf, xbuf, sel, bt, s2, F, stats, N, P, G, v,
                               sc, rbm_lds);
    else
      moments_body<Q, S, Q, T>(X, cap, ret, ind, ybuf, xbuf, sel, bt, s2, F, stats, N, P, G, v,
                               sc, rbm_lds);
  }
}

template <typename T>
int rb_moments_dispatch(const T* X, const T* cap, const T* ret, const int16_t* ind,
                        const double* ybuf, const double* xbuf, const int* sel, const double* bt,
                        const double* s2, const double* F, const double* stats, const int* status,
                        int D, int N, int P, int Q, double* G, double* v, double* sc,
                        void* stream) {
  if (D <= 0) return 0;
  if (Q < 1 || Q > kMaxQ || P < 0 || 1 + P + Q > kMaxK || N <= 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = moments_lds_doubles(P > 0 ? P : 1, Q) * sizeof(double);
  const bool known = dispatch_q(Q, [&](auto q) {
    constexpr int QQ = decltype(q)::value;
    hipLaunchKernelGGL((rb_moments_kernel<QQ, T>), dim3(D, rb_split(QQ) == QQ ? 1 : 2),
                       dim3(kThreads), lds, s, X, cap, ret, P > 0 ? ind : nullptr, ybuf, xbuf, sel,
                       bt, s2, F, stats, status, N, P, G, v, sc);
  });
  return known ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

// -------------------------------------------------------------------------------------- step
// Dynamic LDS: A (G, then M = I + R' G R and its Cholesky factor), R = U sqrt(max(lambda, 0)) and
// Tm = G R with the odd leading dimension K | 1 of woodbury_coef_kernel, then two K-vectors.
__host__ __device__ constexpr size_t rb_step_lds_bytes(int K) {
  return ((size_t)3 * K * (K | 1) + 2 * kMaxK) * sizeof(double);
}

__global__ __launch_bounds__(kThreads) void rb_step_kernel(
    const double* __restrict__ G, const double* __restrict__ v, const double* __restrict__ sc,
    const double* __restrict__ w, const double* __restrict__ U, const double* __restrict__ Mv,
    double tol, int K, double* __restrict__ c, double* __restrict__ ds, int* __restrict__ sel,
    int* __restrict__ mode, int* __restrict__ passes, int* __restrict__ rejected,
    int* __restrict__ status) {
  extern __shared__ double rbs_lds[];
  const int kLD = K | 1;
  double* A = rbs_lds;
  double* R = A + K * kLD;
  double* Tm = R + K * kLD;
  double* vv = Tm + K * kLD;  // v
  double* cv = vv + kMaxK;    // c
  const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (status[d] != kRunning) return;  // a finished date keeps its state
  const double* Gd = G + (size_t)d * K * K;
  const double* Ud = U + (size_t)d * K * K;
  const double* wd = w + (size_t)d * K;
  const double* vd = v + (size_t)d * K;
  double* dsd = ds + (size_t)d * kDs;
  int bad = 0;
  for (int e = tid; e < K * K; e += kThreads) {
    const int i = e / K, k = e - i * K;
    const double gv = Gd[e], uv = Ud[e], lam = wd[k];
    bad |= !(__builtin_isfinite(gv) && __builtin_isfinite(uv) && __builtin_isfinite(lam));
    A[i * kLD + k] = gv;
    R[i * kLD + k] = uv * sqrt(lam > 0.0 ? lam : 0.0);
  }
  for (int e = tid; e < K; e += kThreads) {
    const double ve = vd[e];
    bad |= !__builtin_isfinite(ve);
    vv[e] = ve;
  }
  const double sigma = sc[(size_t)d * 4], r = sc[(size_t)d * 4 + 1], phit = sc[(size_t)d * 4 + 2],
               ysy = sc[(size_t)d * 4 + 3];
  const double phi = dsd[0], lam0 = dsd[1], M = Mv[d];
  const int md = mode[d];
  bad |= !(__builtin_isfinite(sigma) && __builtin_isfinite(r) && __builtin_isfinite(phit) &&
           __builtin_isfinite(ysy) && __builtin_isfinite(M));
  bad = __syncthreads_or(bad);  // also: every read of the state above precedes the writes below
  if (bad) {
    if (tid == 0) status[d] = kInvalid;
    return;
  }
  // a damped step is accepted unconditionally (self-concordance), a clamped one when phi did
  // not rise
  const bool acc = md == kDamped || !(phit > phi + 1e-12 * fabs(phi));
  if (!acc) {  // the saved iterate, its c and lambda stay; the next trial is the damped step
    if (tid == 0) {
      mode[d] = kDamped;
      dsd[2] = 1.0 / (1.0 + M * lam0);
      rejected[d] += 1;
      passes[d] += 1;
    }
    return;
  }
  if (r <= tol) {  // converged: the trial becomes the saved iterate
    if (tid == 0) {
      sel[d] = 1 - (sel[d] & 1);
      dsd[0] = phit;
      dsd[3] = ysy;
      dsd[4] = r;
      passes[d] += 1;
      status[d] = kOk;
    }
    return;
  }
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
    if (tid == 0) status[d] = kInvalid;
    return;
  }
  if (wid == 0) {  // c = R M^-1 R' v, lane i holds row i
    const bool in = lane < K;
    const int li = in ? lane : 0;
    double p = 0.0;  // (R' v)_lane
    for (int j = 0; j < K; ++j) p = fma(R[j * kLD + li], vv[j], p);
    if (!in) p = 0.0;
    for (int j = 0; j < K; ++j) {  // L y = p, column by column
      const double yj = __shfl(p, j, kWave) / A[j * kLD + j];
      if (lane == j) p = yj;
      else if (lane > j && in) p = fma(-A[li * kLD + j], yj, p);
    }
    for (int j = K - 1; j >= 0; --j) {  // L' x = y
      const double xj = __shfl(p, j, kWave) / A[j * kLD + j];
      if (lane == j) p = xj;
      else if (lane < j) p = fma(-A[j * kLD + li], xj, p);
    }
    double s = 0.0;  // (R x)_lane
    for (int k = 0; k < K; ++k) s = fma(R[li * kLD + k], __shfl(p, k, kWave), s);
    if (in) {
      cv[lane] = s;
      c[(size_t)d * K + lane] = s;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double vc = 0.0;
    for (int k = 0; k < K; ++k) vc = fma(vv[k], cv[k], vc);
    const double l2 = sigma - vc;
    sel[d] = 1 - (sel[d] & 1);
    mode[d] = kClamped;
    dsd[0] = phit;
    dsd[1] = sqrt(l2 > 0.0 ? l2 : 0.0);
    dsd[3] = ysy;
    dsd[4] = r;
    passes[d] += 1;
  }
}

// ------------------------------------------------------------------------------------ update
// The trial from the date's saved iterate: g_n, a_n and delta_n recomputed there (z = F x_saved
// and c with the z-scoring folded in), y_trial written to the other buffer, x_trial = X' y_trial
// summed in the same stream with the order-fixed reductions of factor_xty_kernel.
__host__ __device__ constexpr size_t update_lds_doubles(int Pseg, int Q) {
  return (size_t)kWaves * Pseg + (size_t)(kWaves + 1) * (Q + 1) + 3 * kMaxK;
}

template <int Q, typename T>
__global__ __launch_bounds__(kThreads) void rb_update_kernel(
    const T* __restrict__ X, const T* __restrict__ cap, const T* __restrict__ ret,
    const int16_t* __restrict__ ind, double* __restrict__ ybuf, double* __restrict__ xbuf,
    const int* __restrict__ sel, const int* __restrict__ mode, const double* __restrict__ c,
    const double* __restrict__ ds, const double* __restrict__ bt, const double* __restrict__ s2,
    const double* __restrict__ F, const double* __restrict__ stats,
    const int* __restrict__ status, double theta, int N, int P) {
  extern __shared__ double rbu_lds[];
  constexpr int NACC = Q + 1;
  const int d = blockIdx.x, D = gridDim.x, tid = threadIdx.x, wid = tid >> 6;
  if (status[d] != kRunning) return;  // a finished date keeps both iterates
  const DesignDate<T> day(X, cap, ret, ind, d, N, P, Q);
  const int Pseg = day.Pseg, K = 1 + P + Q;
  double* seg = rbu_lds;                         // [kWaves][Pseg]: sum y_trial per industry
  double* red = seg + (size_t)kWaves * Pseg;      // [kWaves][NACC]
  double* tot = red + kWaves * NACC;              // [NACC]
  double* zz = tot + NACC;                        // [kMaxK] F x_saved, folded
  double* cc = zz + kMaxK;                        // [kMaxK] c, folded
  double* raw = cc + kMaxK;                       // [kMaxK]
  const int sb = sel[d] & 1;
  const double* ys = ybuf + ((size_t)sb * D + d) * N;
  double* yt = ybuf + ((size_t)(1 - sb) * D + d) * N;
  const double* bd = bt + (size_t)d * N;
  const double* sd = s2 + (size_t)d * N;
  const double* st = stats + (size_t)d * (Q + 2);
  const bool damped = mode[d] == kDamped;
  const double t = ds[(size_t)d * kDs + 2];
  if (P > 0)
    for (int i = tid; i < kWaves * Pseg; i += kThreads) seg[i] = 0.0;
  fold_Fx(F + (size_t)d * K * K, xbuf + ((size_t)sb * D + d) * K, st, P, Q, raw, zz);
  if (tid == 0) fold_zscore(c + (size_t)d * K, st, P, Q, cc);
  __syncthreads();
  double* myseg = seg + (size_t)wid * Pseg;
  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
  for (int n = tid; n < N; n += kThreads) {
    T cp, r, xf[Q];
    int j;
    day.load_base(n, cp, r, j);
    const double b = bd[n], yn = ys[n], s2n = sd[n];
    bool ok = __builtin_isfinite(b) && (b > 0.0) && (yn > 0.0) && day.base_ok(cp, r, j);
    day.load_styles_ok(n, xf, ok);
    double out = 0.0;  // a stock outside the universe
    if (ok) {
      double x[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) x[q] = (double)xf[q];
      double dz = zz[0] + (P > 0 ? zz[1 + j] : 0.0), dc = cc[0] + (P > 0 ? cc[1 + j] : 0.0);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        dz = fma(x[q], zz[1 + P + q], dz);
        dc = fma(x[q], cc[1 + P + q], dc);
      }
      const double by = b / yn;
      const double an = 1.0 / (s2n + by / yn);
      const double g = fma(s2n, yn, dz) - by;
      const double dl = -an * (g - dc);
      out = damped ? fma(t, dl, yn) : fmax(yn + dl, theta * yn);
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[q] = fma(out, x[q], acc[q]);
      acc[Q] += out;
      if (P > 0) atomicAdd(myseg + j, out);
    }
    yt[n] = out;
  }
  wave_totals(acc, red);
  __syncthreads();
  for (int i = tid; i < NACC; i += kThreads) tot[i] = sum4(red, NACC, i);
  if (P > 0)  // entry i of the four tables is touched by this thread only
    for (int i = tid; i < Pseg; i += kThreads) seg[i] = sum4(seg, Pseg, i);
  __syncthreads();
  const double isig = 1.0 / st[Q];
  const double hs = tot[Q];
  double* xt = xbuf + ((size_t)(1 - sb) * D + d) * K;
  for (int k = tid; k < K; k += kThreads) {
    double val;
    if (k == 0) val = hs;
    else if (k <= P) val = seg[k - 1];
    else val = unfold_zscore(tot[k - 1 - P], st[k - 1 - P], hs, isig);
    xt[k] = val;
  }
}

template <typename T>
int rb_update_dispatch(const T* X, const T* cap, const T* ret, const int16_t* ind, double* ybuf,
                       double* xbuf, const int* sel, const int* mode, const double* c,
                       const double* ds, const double* bt, const double* s2, const double* F,
                       const double* stats, const int* status, double theta, int D, int N, int P,
                       int Q, void* stream) {
  if (D <= 0) return 0;
  if (Q < 1 || Q > kMaxQ || P < 0 || 1 + P + Q > kMaxK || N <= 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = update_lds_doubles(P > 0 ? P : 1, Q) * sizeof(double);
  const bool known = dispatch_q(Q, [&](auto q) {
    hipLaunchKernelGGL((rb_update_kernel<decltype(q)::value, T>), dim3(D), dim3(kThreads), lds, s,
                       X, cap, ret, P > 0 ? ind : nullptr, ybuf, xbuf, sel, mode, c, ds, bt, s2,
                       F, stats, status, theta, N, P);
  });
  return known ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

}  // namespace

// Panel as mfa_factor_gram.  y [2][D][N], x [2][D][K] the two iterates of every date and their
// exposures X' y, sel [D] the saved one (the trial 1 - sel is evaluated); bt [D][N] the scaled
// budgets (<= 0 or non-finite: outside the universe), s2 [D][N] = s^2, F [D][K][K], status [D]
// (dates whose status is not -1 are left untouched).  G [D][K][K], v [D][K], sc [D][4] = (sigma,
// r, phi, y' Sigma y).  K <= 64, Q <= 16.  Bitwise reproducible.
MFA_API int mfa_rb_moments(const float* X, const float* cap, const float* ret, const int16_t* ind,
                           const double* y, const double* x, const int* sel, const double* bt,
                           const double* s2, const double* F, const double* stats,
                           const int* status, int D, int N, int P, int Q, double* G, double* v,
                           double* sc, void* stream) {
  return rb_moments_dispatch<float>(X, cap, ret, ind, y, x, sel, bt, s2, F, stats, status, D, N, P,
                                    Q, G, v, sc, stream);
}

// Same with an fp64 panel.
MFA_API int mfa_rb_moments_f64(const double* X, const double* cap, const double* ret,
                               const int16_t* ind, const double* y, const double* x,
                               const int* sel, const double* bt, const double* s2, const double* F,
                               const double* stats, const int* status, int D, int N, int P, int Q,
                               double* G, double* v, double* sc, void* stream) {
  return rb_moments_dispatch<double>(X, cap, ret, ind, y, x, sel, bt, s2, F, stats, status, D, N,
                                     P, Q, G, v, sc, stream);
}

// G, v, sc of mfa_rb_moments; (w [D][K], U [D][K][K]) eigenpairs of F; M [D] = 1 / sqrt(min b);
// state per date: c [D][K], ds [D][5] = (phi, lambda, damped step length, y' Sigma y, r) of the
// saved iterate, sel, mode (0 clamped, 1 damped), passes, rejected, status [D] int.  K <= 64.
MFA_API int mfa_rb_step(const double* G, const double* v, const double* sc, const double* w,
                        const double* U, const double* M, double tol, int D, int K, double* c,
                        double* ds, int* sel, int* mode, int* passes, int* rejected, int* status,
                        void* stream) {
  if (D <= 0) return 0;
  if (K < 1 || K > kMaxK) return (int)hipErrorInvalidValue;
  const size_t lds = rb_step_lds_bytes(K);
  if (hipError_t err = raise_dynamic_lds<rb_step_kernel>(lds)) return (int)err;
  hipLaunchKernelGGL(rb_step_kernel, dim3(D), dim3(kThreads), lds, (hipStream_t)stream, G, v, sc,
                     w, U, M, tol, K, c, ds, sel, mode, passes, rejected, status);
  return (int)hipGetLastError();
}

// The trial of every running date from its saved iterate, into the other buffer of y and x:
// max(y + delta, theta y) when mode is 0, y + ds[2] delta when it is 1; 0 outside the universe.
MFA_API int mfa_rb_update(const float* X, const float* cap, const float* ret, const int16_t* ind,
                          double* y, double* x, const int* sel, const int* mode, const double* c,
                          const double* ds, const double* bt, const double* s2, const double* F,
                          const double* stats, const int* status, double theta, int D, int N,
                          int P, int Q, void* stream) {
  return rb_update_dispatch<float>(X, cap, ret, ind, y, x, sel, mode, c, ds, bt, s2, F, stats,
                                   status, theta, D, N, P, Q, stream);
}

// Same with an fp64 panel.
MFA_API int mfa_rb_update_f64(const double* X, const double* cap, const double* ret,
                              const int16_t* ind, double* y, double* x, const int* sel,
                              const int* mode, const double* c, const double* ds, const double* bt,
                              const double* s2, const double* F, const double* stats,
                              const int* status, double theta, int D, int N, int P, int Q,
                              void* stream) {
  return rb_update_dispatch<double>(X, cap, ret, ind, y, x, sel, mode, c, ds, bt, s2, F, stats,
                                    status, theta, D, N, P, Q, stream);
}
