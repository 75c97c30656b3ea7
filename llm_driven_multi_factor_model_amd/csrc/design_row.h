// One row of the regression's design matrix, for the kernels that stream the raw panel.
//
// X_d = [country | one-hot industries | cap-weighted z-scored styles] (K = 1 + P + Q columns) is
// never materialised: factor_cov.hip, attribution.hip, portfolio_batch.hip and pure_factor.hip
// read the raw panel (X, cap, ret, ind) and fold the z-scoring in from stats = (mu_q, sigma, n)
// of mfa_xs_wls.  What a design row is lives here, once:
//   * the per-date view of the panel;
//   * the regression's validity rule (the one of mfa_xs_wls): 0 <= ind < max(P, 1), cap finite
//     and >= 0, ret finite, every style finite.  Kernels AND their own clauses onto it;
//   * the z-scoring folded into a coefficient row, and its inverse on a row of sums;
//   * the order-fixed four-wave workgroup total;
//   * the runtime Q -> template dispatch, the shared limits and the dynamic-LDS limit.
#pragma once
#include <type_traits>

#include "common.h"

namespace mfa {

constexpr int kThreads = 256, kWaves = 4;  // every kernel on this panel: four waves per workgroup
constexpr int kMaxK = 64;  // one-wave tier of the eigen solvers (ops.eigen.WIDE_K, jacobi.h)
constexpr int kMaxQ = 16;  // styles held in registers per stock

// The rule's clauses on (cap, ret, industry) of one stock; Pseg = max(P, 1).  The expression form
// is for call sites that evaluate it in place, between their own loads (pure_factor_weights,
// portfolio_batch); everything else calls the function.
#define MFA_DESIGN_BASE_OK(T, c, r, j, Pseg) \
  (((j) >= 0) && ((j) < (Pseg)) && __builtin_isfinite(c) && ((c) >= T(0)) && __builtin_isfinite(r))
template <typename T>
__device__ __forceinline__ bool design_base_ok(T c, T r, int j, int Pseg) {
  return MFA_DESIGN_BASE_OK(T, c, r, j, Pseg);
}

// ------------------------------------------------------------------------------ per-date view
template <typename T>
struct DesignDate {
  const T* X;          // [Q][N] raw styles
  const T* cap;        // [N]
  const T* ret;        // [N]
  const int16_t* ind;  // [N], or null when the panel has no industries
  int N, Pseg;         // Pseg = max(P, 1): the industries a valid stock may name

  __device__ __forceinline__ DesignDate(const T* X_, const T* cap_, const T* ret_,
                                        const int16_t* ind_, int d, int N_, int P, int Q)
      : X(X_ + (size_t)d * Q * N_),
        cap(cap_ + (size_t)d * N_),
        ret(ret_ + (size_t)d * N_),
        ind(ind_ ? ind_ + (size_t)d * N_ : nullptr),
        N(N_),
        Pseg(P > 0 ? P : 1) {}

  __device__ __forceinline__ int industry(int n) const { return ind ? (int)ind[n] : 0; }

  // (cap, ret, industry) of stock n: three independent loads, issued together ...
  __device__ __forceinline__ void load_base(int n, T& c, T& r, int& j) const {
    c = cap[n];
    r = ret[n];
    j = industry(n);
  }
  // ... and the rule's clauses on them.  Callers put their own clauses first and this call last.
  __device__ __forceinline__ bool base_ok(T c, T r, int j) const {
    return design_base_ok(c, r, j, Pseg);
  }

  // Styles [q0, q0 + QB) of the date's Q for stock n (0 past Q), for a caller that checks later.
  template <int QB>
  __device__ __forceinline__ void load_styles(int n, T (&x)[QB], int q0 = 0, int Q = QB) const {
#pragma unroll
    for (int q = 0; q < QB; ++q) x[q] = q0 + q < Q ? X[(size_t)(q0 + q) * N + n] : T(0);
  }
  // The styles' clause of the rule, ANDed into the caller's `ok`: for the styles of the date's Q
  // outside a block [skip0, skip1), which a blocked caller does not keep but which still decide
  // validity (every one of them is read, whatever `ok` is) ...
  __device__ __forceinline__ void styles_outside_ok(int n, bool& ok, int Q, int skip0,
                                                    int skip1) const {
    for (int q = 0; q < Q; ++q)
      if (q < skip0 || q >= skip1) ok &= (bool)__builtin_isfinite(X[(size_t)q * N + n]);
  }
  // ... and for the styles the caller keeps, loaded and checked one by one.
  template <int QB>
  __device__ __forceinline__ void load_styles_ok(int n, T (&x)[QB], bool& ok, int q0 = 0,
                                                 int Q = QB) const {
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      x[q] = q0 + q < Q ? X[(size_t)(q0 + q) * N + n] : T(0);
      ok = ok && __builtin_isfinite(x[q]);
    }
  }
};

// ----------------------------------------------------------------------------------- z-scoring
// stats row st = (mu_0 .. mu_{Q-1}, sigma, n).  Every kernel needs (mu, sigma) finite before it
// trusts a z-score; what else it asks of the row (sigma > 0, ...) stays with the kernel.
__device__ __forceinline__ bool stats_finite(const double* st, int Q) {
  bool ok = true;
  for (int q = 0; q <= Q; ++q) ok &= (bool)__builtin_isfinite(st[q]);
  return ok;
}

// Fold (mu, sigma) into a coefficient row cb[K], so that x . c over the z-scored styles becomes
//   cc[0] + cc[1 + j] + sum_q X_q cc[1 + P + q]   on the raw styles:
// cc_q = c_q / sigma, cc[0] = c[0] - sum_q mu_q cc_q (in q order), industry entries copied.
__device__ __forceinline__ void fold_zscore(const double* cb, const double* st, int P, int Q,
                                            double* cc) {
  const double isig = 1.0 / st[Q];
  double c0 = cb[0];
  for (int k = 1; k <= P; ++k) cc[k] = cb[k];
  for (int q = 0; q < Q; ++q) {
    const double cq = cb[1 + P + q] * isig;
    cc[1 + P + q] = cq;
    c0 = fma(-st[q], cq, c0);
  }
  cc[0] = c0;
}

// The inverse on sums: sum_n h_n z_nq from sum = sum_n h_n X_nq, hs = sum_n h_n, isig = 1 / sigma.
__device__ __forceinline__ double unfold_zscore(double sum, double mu, double hs, double isig) {
  return (sum - mu * hs) * isig;
}

// ------------------------------------------------------------------- order-fixed block totals
// Lane -> wave by DPP (wave_total), one slot per wave in red [kWaves][NACC]; after a barrier
// sum4(red, NACC, i) adds the four waves in wave order.  Two runs give the same bits.
template <int NACC>
__device__ __forceinline__ void wave_totals(const double (&acc)[NACC], double* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const double t = wave_total(acc[i]);
    if (lane == 0) red[wid * NACC + i] = t;
  }
}
__device__ __forceinline__ double sum4(const double* t, int stride, int i) {
  return ((t[i] + t[stride + i]) + t[2 * stride + i]) + t[3 * stride + i];
}

// -------------------------------------------------------------------------------------- host
// Calls f(std::integral_constant<int, Q>) for a runtime Q in 1..kMaxQ; false for any other Q.
template <int Q0 = 1, typename F>
bool dispatch_q(int Q, F&& f) {
  if constexpr (Q0 > kMaxQ) {
    return false;
  } else {
    if (Q != Q0) return dispatch_q<Q0 + 1>(Q, f);
    f(std::integral_constant<int, Q0>{});
    return true;
  }
}

// Raises Kernel's dynamic-LDS limit to `lds` bytes when it was never raised that far: one
// high-water mark per kernel instantiation, starting at the 64 KB every kernel gets.
template <auto Kernel>
hipError_t raise_dynamic_lds(size_t lds) {
  static size_t high = 64 * 1024;
  if (high >= lds) return hipSuccess;
  const hipError_t err = hipFuncSetAttribute(
      (const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err == hipSuccess) high = lds;
  return err;
}

}  // namespace mfa
