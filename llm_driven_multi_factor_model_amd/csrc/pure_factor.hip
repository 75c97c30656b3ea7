// Pure factor portfolios and factor-return standard errors of the cross-sectional regression,
// all dates per launch (gfx950).
//
// Both come from the estimator covariance of date d,
//   C = R (R^T G R)^+ R^T,   G = X^T W X  (mfa_factor_gram with a = sqrt(cap)),
// R the industry-neutral constraint matrix of mfa_xs_wls (identity with one pivot row) and ^+ the
// pseudo-inverse that drops eigenvalues <= 1e-15 lambda_max:
//   Omega = C X^T W            the K x N pure factor portfolios, f = Omega r,
//   Var(f) = sigma^2 C         sigma^2 = sum w e^2 / (n - rank).
// Three kernels:
//   est_cov_kernel               G, industry caps -> C, rank   one workgroup per date; A = R^T G R
//                                in LDS, one-wave Jacobi (jacobi.h), fixed-order products
//   pure_factor_weights_kernel   raw panel, rows of C -> Omega one pass over the panel; the selected
//                                rows of C in LDS with (mu, sigma) folded in; non-temporal stores
//   factor_stats_kernel          residuals, C, f -> se, t      one workgroup per date; order-fixed
//                                sum (lane -> wave by DPP -> waves)
// The per-date view of the panel, the regression's validity rule and the fold of (mu, sigma)
// into a coefficient row are design_row.h's.
// hipcc --offload-arch=gfx950 -O3, scratch 0 for all of them:
//   est_cov_kernel                       62 VGPR, dynamic LDS 2 Kr (Kr + 1) + 256 + 3 K doubles
//                                        (29.9 KB at K = 42, P = 31; 68.5 KB at K = 64, P = 0)
//   pure_factor_weights_kernel<Q, T>     30 + 6 Q VGPR or fewer (84 at Q = 10, 120 at Q = 16),
//                                        dynamic LDS nb K doubles (13.8 KB at S = K = 42)
//   factor_stats_kernel<float / double>  26 VGPR, static LDS 32 B
#include "design_row.h"
#include "jacobi.h"

namespace {

using namespace mfa;

constexpr int kRowsNB = 64;    // rows of C per pure_factor_weights launch (they live in LDS)
constexpr int kChunk = 2048;   // stocks per workgroup of pure_factor_weights_kernel

// ------------------------------------------------------------------------ estimator covariance
__host__ __device__ constexpr size_t est_cov_lds_bytes(int K, int P) {
  const int Kr = P > 0 ? K - 1 : K;
  return ((size_t)2 * Kr * (Kr + 1) + 4 * 64 + 3 * K) * sizeof(double);
}

// G [D][K][K] = X^T diag(sqrt(cap)) X, Gs [D][K][K] = X^T diag(cap) X (row 0 carries the raw
// industry caps s_j; unused when P == 0).  A date whose G or stats row is not finite, whose sigma
// or sum of weights is not > 0, or whose pivot industry is empty gets NaN C and rank 0.
__global__ __launch_bounds__(kThreads) void est_cov_kernel(
    const double* __restrict__ G, const double* __restrict__ Gs, const double* __restrict__ stats,
    int P, int Q, int pivot_mode, double* __restrict__ C, int* __restrict__ rank) {
  extern __shared__ double ec_lds[];
  __shared__ int piv_s;
  __shared__ double sp_s;
  const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int K = 1 + P + Q, Kr = P > 0 ? K - 1 : K, lda = Kr + 1;
  double* A = ec_lds;            // [Kr][lda]  R^T G R, then its pseudo-inverse
  double* V = A + Kr * lda;      // [Kr][lda]  eigenvectors (columns)
  double* rot = V + Kr * lda;    // [4 * 64]   rotations of one Jacobi round
  double* alp = rot + 4 * 64;    // [K]        constraint weights -s_j / s_pivot
  double* inv = alp + K;         // [K]        1 / lambda over the kept spectrum, 0 elsewhere
  double* cp = inv + K;          // [K]        pivot row of C over the reduced columns
  const double* Gd = G + (size_t)d * K * K;
  const double* sd = Gs + (size_t)d * K * K + 1;  // s_j at sd[j]
  const double* st = stats + (size_t)d * (Q + 2);
  double* Cd = C + (size_t)d * K * K;
  int bad = 0;
  for (int e = tid; e < K * K; e += kThreads) bad |= !__builtin_isfinite(Gd[e]);
  if (tid == 0) {
    bad |= !stats_finite(st, Q) || !(st[Q] > 0.0) || !(Gd[0] > 0.0);
    int jp = -1;
    double sp = 1.0;
    if (P > 0) {
      if (pivot_mode == 1) jp = P - 1;
      else for (int j = 0; j < P; ++j) if (sd[j] > 0.0) jp = j;
      if (jp < 0) jp = P - 1;
      sp = sd[jp];
      bad |= !(sp > 0.0) || !__builtin_isfinite(sp);
    }
    piv_s = jp;
    sp_s = sp;
  }
  bad = __syncthreads_or(bad);
  if (bad) {  // uniform: the whole workgroup leaves
    for (int e = tid; e < K * K; e += kThreads) Cd[e] = qnan();
    if (tid == 0) rank[d] = 0;
    return;
  }
  const int pc = 1 + piv_s;  // pivot column (P > 0)
  const double sp = sp_s;
  auto orig = [&](int u) { return (P > 0 && u >= pc) ? u + 1 : u; };
  auto red = [&](int o) { return (P > 0 && o > pc) ? o - 1 : o; };
  for (int u = tid; u < Kr; u += kThreads) {
    const int ou = orig(u);
    alp[u] = (P > 0 && ou >= 1 && ou <= P) ? -sd[ou - 1] / sp : 0.0;
  }
  __syncthreads();
  for (int e = tid; e < Kr * Kr; e += kThreads) {
    const int u = e / Kr, v = e - u * Kr;
    if (v < u) continue;
    const int ou = orig(u), ov = orig(v);
    double a = Gd[ou * K + ov];
    if (P > 0) {
      const double au = alp[u], av = alp[v];
      a += au * Gd[pc * K + ov] + av * Gd[ou * K + pc] + au * av * Gd[pc * K + pc];
    }
    A[u * lda + v] = a;
    A[v * lda + u] = a;
  }
  __syncthreads();
  if (tid < 64) {  // wave 0: eigen-decompose, cut the spectrum
    // stop at an off-diagonal norm of 1e-15 of the diagonal's (the tolerance of ops.eigen.eigh):
    // the sweeps converge quadratically, and an eigenvalue moves by the square of what is left
    jacobi_wave(A, V, Kr, lda, rot, 40, 1e-15);
    double lmax = 0.0;
    for (int k = lane; k < Kr; k += 64) lmax = fmax(lmax, fabs(A[k * lda + k]));
    lmax = wave_max(lmax);
    const double cut = 1e-15 * lmax;
    int kept = 0;
    for (int k = lane; k < Kr; k += 64) {
      const double lk = A[k * lda + k];
      const bool keep = fabs(lk) > cut;
      inv[k] = keep ? 1.0 / lk : 0.0;
      kept += keep ? 1 : 0;
    }
    kept = wave_sum(kept);
    if (lane == 0) rank[d] = kept;
  }
  __syncthreads();
  // A <- V diag(inv) V^T, every entry summed over k in index order, the lower triangle mirrored
  for (int e = tid; e < Kr * Kr; e += kThreads) {
    const int u = e / Kr, v = e - u * Kr;
    if (v < u) continue;
    double s = 0.0;
    for (int k = 0; k < Kr; ++k) s = fma(V[u * lda + k] * inv[k], V[v * lda + k], s);
    A[u * lda + v] = s;
    A[v * lda + u] = s;
  }
  __syncthreads();
  if (P > 0) {
    for (int v = tid; v < Kr; v += kThreads) {
      double s = 0.0;
      for (int u = 0; u < Kr; ++u) s = fma(alp[u], A[u * lda + v], s);
      cp[v] = s;
    }
    __syncthreads();
  }
  for (int e = tid; e < K * K; e += kThreads) {
    const int i = e / K, j = e - i * K;
    double v;
    if (P > 0 && i == pc && j == pc) {
      v = 0.0;
      for (int u = 0; u < Kr; ++u) v = fma(alp[u], cp[u], v);
    } else if (P > 0 && i == pc) {
      v = cp[red(j)];
    } else if (P > 0 && j == pc) {
      v = cp[red(i)];
    } else {
      v = A[red(i) * lda + red(j)];
    }
    Cd[e] = v;
  }
}

// ---------------------------------------------------------------------- pure factor portfolios
// out[d, b0 + j, n] = sqrt(cap_n) (x_n . C[d, sel[b0 + j], :]) for nb <= kRowsNB rows of NB, on
// the regression-valid stocks; 0 on the others; NaN for every stock of a date whose C (any entry)
// or stats row is not finite or whose sigma is not > 0.  The z-scoring is folded into the
// coefficients once per workgroup, row by row in a fixed order, and every (row, stock) value is
// formed by the same instructions whatever nb, b0 and the chunk: a row does not depend on which
// other rows are asked for.  Two stocks per thread share each coefficient read from LDS.
template <int Q, typename T>
__global__ __launch_bounds__(kThreads) void pure_factor_weights_kernel(
    const T* __restrict__ X, const T* __restrict__ cap, const T* __restrict__ ret,
    const int16_t* __restrict__ ind, const double* __restrict__ stats,
    const double* __restrict__ C, const int* __restrict__ sel, int N, int P, int NB, int b0,
    int nb, double* __restrict__ out) {
  extern __shared__ double pf_lds[];  // [nb][K]
  const int d = blockIdx.x, tid = threadIdx.x;
  const DesignDate<T> day(X, cap, ret, ind, d, N, P, Q);
  const int K = 1 + P + Q;
  const double* st = stats + (size_t)d * (Q + 2);
  const double* Cd = C + (size_t)d * K * K;
  int bad = 0;
  for (int e = tid; e < K * K; e += kThreads) bad |= !__builtin_isfinite(Cd[e]);
  if (tid == 0) bad |= !stats_finite(st, Q) || !(st[Q] > 0.0);
  // one thread per row: fold (mu, sigma) into its coefficients
  if (tid < nb) fold_zscore(Cd + (size_t)sel[b0 + tid] * K, st, P, Q, pf_lds + tid * K);
  bad = __syncthreads_or(bad);
  double* ob = out + ((size_t)d * NB + b0) * N;
  const int n0 = blockIdx.y * kChunk;
  const int n1 = n0 + kChunk < N ? n0 + kChunk : N;
  for (int n = n0 + tid; n < n1; n += 2 * kThreads) {
    const int m = n + kThreads;
    const bool in2 = m < n1;
    const int m2 = in2 ? m : n;  // the second stock, or the first again (loads stay in bounds)
    // the pair's loads are interleaved and the rule is evaluated between them
    const T ca = day.cap[n], cb = day.cap[m2], ra = day.ret[n], rb = day.ret[m2];
    const int ja = day.industry(n), jb = day.industry(m2);
    bool oka = MFA_DESIGN_BASE_OK(T, ca, ra, ja, day.Pseg);
    bool okb = MFA_DESIGN_BASE_OK(T, cb, rb, jb, day.Pseg);
    double xa[Q], xb[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const T fa = day.X[(size_t)q * N + n], fb = day.X[(size_t)q * N + m2];
      oka = oka && __builtin_isfinite(fa);
      okb = okb && __builtin_isfinite(fb);
      xa[q] = (double)fa;
      xb[q] = (double)fb;
    }
    const int ia = (oka && P > 0) ? 1 + ja : 0, ib = (okb && P > 0) ? 1 + jb : 0;
    const double wa = oka ? sqrt((double)ca) : 0.0, wb = okb ? sqrt((double)cb) : 0.0;
    for (int j = 0; j < nb; ++j) {
      const double* cc = pf_lds + j * K;
      const double c0 = cc[0];
      double da = c0 + (P > 0 ? cc[ia] : 0.0), db = c0 + (P > 0 ? cc[ib] : 0.0);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const double cq = cc[1 + P + q];
        da = fma(xa[q], cq, da);
        db = fma(xb[q], cq, db);
      }
      double va = oka ? wa * da : 0.0, vb = okb ? wb * db : 0.0;
      if (bad) va = vb = qnan();
      __builtin_nontemporal_store(va, ob + (size_t)j * N + n);
      if (in2) __builtin_nontemporal_store(vb, ob + (size_t)j * N + m);
    }
  }
}

template <typename T>
int pure_factor_weights_dispatch(const T* X, const T* cap, const T* ret, const int16_t* ind,
                                 const double* stats, const double* C, const int* sel, int D,
                                 int N, int P, int Q, int NB, int b0, int nb, double* out,
                                 void* stream) {
  if (D <= 0 || nb <= 0) return 0;
  if (Q < 1 || Q > kMaxQ || P < 0 || 1 + P + Q > kMaxK || N <= 0 || b0 < 0 || nb > kRowsNB ||
      b0 + nb > NB || !sel)
    return (int)hipErrorInvalidValue;
  const int chunks = (N + kChunk - 1) / kChunk;
  if (chunks > 65535) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)nb * (1 + P + Q) * sizeof(double);
  const bool known = dispatch_q(Q, [&](auto q) {
    hipLaunchKernelGGL((pure_factor_weights_kernel<decltype(q)::value, T>), dim3(D, chunks),
                       dim3(kThreads), lds, s, X, cap, ret, P > 0 ? ind : nullptr, stats, C, sel, N,
                       P, NB, b0, nb, out);
  });
  return known ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

// --------------------------------------------------------------- factor-return standard errors
// sigma2[d] = sum over the regression-valid stocks with a finite residual of sqrt(cap) e^2, over
// dof[d] = n[d] - rank[d]; se[d, k] = sqrt(sigma2 C_kk), t = f / se.  dof <= 0 (or not finite):
// NaN sigma2, se and t; se == 0: NaN t.  Each thread sums its stocks in index order, the wave by
// DPP, the four waves in wave order: two runs give the same bits.
template <typename T>
__global__ __launch_bounds__(kThreads) void factor_stats_kernel(
    const T* __restrict__ X, const T* __restrict__ cap, const T* __restrict__ ret,
    const int16_t* __restrict__ ind, const T* __restrict__ resid, const double* __restrict__ C,
    const double* __restrict__ f, const int* __restrict__ rank, const double* __restrict__ nv,
    int N, int P, int Q, double* __restrict__ se, double* __restrict__ t,
    double* __restrict__ sigma2, double* __restrict__ dof) {
  __shared__ double red[4];
  const int d = blockIdx.x, tid = threadIdx.x;
  const DesignDate<T> day(X, cap, ret, ind, d, N, P, Q);
  const int K = 1 + P + Q;
  const T* ed = resid + (size_t)d * N;
  double acc[1] = {0.0};
  for (int n = tid; n < N; n += kThreads) {
    T c, r;
    int j;
    const T e = ed[n];  // ahead of the industry load and its wait
    day.load_base(n, c, r, j);
    bool ok = __builtin_isfinite(e) && day.base_ok(c, r, j);
    for (int q = 0; q < Q; ++q) ok = ok && __builtin_isfinite(day.X[(size_t)q * N + n]);
    if (!ok) continue;
    const double ev = (double)e;
    acc[0] = fma(sqrt((double)c), ev * ev, acc[0]);
  }
  wave_totals(acc, red);
  __syncthreads();
  const double df = nv[d] - (double)rank[d];
  const bool okd = __builtin_isfinite(df) && df > 0.0;
  const double s2 = okd ? sum4(red, 1, 0) / df : qnan();
  if (tid == 0) {
    sigma2[d] = s2;
    dof[d] = df;
  }
  for (int k = tid; k < K; k += kThreads) {
    const double s = sqrt(s2 * C[((size_t)d * K + k) * K + k]);
    se[(size_t)d * K + k] = s;
    t[(size_t)d * K + k] = s > 0.0 ? f[(size_t)d * K + k] / s : qnan();
  }
}

template <typename T>
int factor_stats_dispatch(const T* X, const T* cap, const T* ret, const int16_t* ind,
                          const T* resid, const double* C, const double* f, const int* rank,
                          const double* nv, int D, int N, int P, int Q, double* se, double* t,
                          double* sigma2, double* dof, void* stream) {
  if (D <= 0) return 0;
  if (Q < 1 || P < 0 || N <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(factor_stats_kernel<T>, dim3(D), dim3(kThreads), 0, (hipStream_t)stream, X,
                     cap, ret, P > 0 ? ind : nullptr, resid, C, f, rank, nv, N, P, Q, se, t,
                     sigma2, dof);
  return (int)hipGetLastError();
}

}  // namespace

// G / Gs [D][K][K] f64 from mfa_factor_gram with a = sqrt(cap) / a = cap (Gs is not read when
// P == 0), stats [D][Q+2]; C [D][K][K] f64, rank [D] i32.  K = 1 + P + Q <= 64.  pivot_mode as
// mfa_xs_wls (0: last non-empty industry, 1: last industry).
MFA_API int mfa_est_cov(const double* G, const double* Gs, const double* stats, int D, int P, int Q,
                        int pivot_mode, double* C, int* rank, void* stream) {
  if (D <= 0) return 0;
  const int K = 1 + P + Q;
  if (Q < 1 || P < 0 || K > kMaxK || (pivot_mode != 0 && pivot_mode != 1) || (P > 0 && !Gs))
    return (int)hipErrorInvalidValue;
  const size_t lds = est_cov_lds_bytes(K, P);
  if (hipError_t err = raise_dynamic_lds<est_cov_kernel>(lds)) return (int)err;
  hipLaunchKernelGGL(est_cov_kernel, dim3(D), dim3(kThreads), lds, (hipStream_t)stream, G,
                     P > 0 ? Gs : G, stats, P, Q, pivot_mode, C, rank);
  return (int)hipGetLastError();
}

// out [D][NB][N] f64 rows [b0, b0 + nb), nb <= 64: row b is sqrt(cap) o (X C[d][sel[b]]) with
// sel [NB] i32 row indices into K; X [D][Q][N], cap / ret [D][N] f32, ind [D][N] int16 (nullable
// when P == 0).  K <= 64, Q <= 16.
MFA_API int mfa_pure_factor_weights(const float* X, const float* cap, const float* ret,
                                    const int16_t* ind, const double* stats, const double* C,
                                    const int* sel, int D, int N, int P, int Q, int NB, int b0,
                                    int nb, double* out, void* stream) {
  return pure_factor_weights_dispatch<float>(X, cap, ret, ind, stats, C, sel, D, N, P, Q, NB, b0,
                                             nb, out, stream);
}

// Same with an fp64 panel.
MFA_API int mfa_pure_factor_weights_f64(const double* X, const double* cap, const double* ret,
                                        const int16_t* ind, const double* stats, const double* C,
                                        const int* sel, int D, int N, int P, int Q, int NB, int b0,
                                        int nb, double* out, void* stream) {
  return pure_factor_weights_dispatch<double>(X, cap, ret, ind, stats, C, sel, D, N, P, Q, NB, b0,
                                              nb, out, stream);
}

// resid [D][N] in the panel's type, C [D][K][K], f [D][K], rank [D] i32, nv [D] f64 (stocks in
// the regression); se / t [D][K], sigma2 / dof [D] f64.
MFA_API int mfa_factor_stats(const float* X, const float* cap, const float* ret, const int16_t* ind,
                             const float* resid, const double* C, const double* f, const int* rank,
                             const double* nv, int D, int N, int P, int Q, double* se, double* t,
                             double* sigma2, double* dof, void* stream) {
  return factor_stats_dispatch<float>(X, cap, ret, ind, resid, C, f, rank, nv, D, N, P, Q, se, t,
                                      sigma2, dof, stream);
}

// Same with an fp64 panel.
MFA_API int mfa_factor_stats_f64(const double* X, const double* cap, const double* ret,
                                 const int16_t* ind, const double* resid, const double* C,
                                 const double* f, const int* rank, const double* nv, int D, int N,
                                 int P, int Q, double* se, double* t, double* sigma2, double* dof,
                                 void* stream) {
  return factor_stats_dispatch<double>(X, cap, ret, ind, resid, C, f, rank, nv, D, N, P, Q, se, t,
                                       sigma2, dof, stream);
}
