// Specific-risk model kernels (gfx950): the exponentially weighted, Newey-West corrected
// trailing specific volatility and the cross-sectional bias statistic of the specific forecasts
// (USE4 / CNE5 specific risk; ops/specific_risk.py holds the definitions and the CPU paths).
//
// ---- mfa_ewnw_vol ------------------------------------------------------------------------
// For stock n and local date t, over the W rows ENDING at t of ext = [halo (W - 1 rows) ; e]
// (row j = 0 is date t, j = W - 1 the oldest; w_j from the host's float64 table):
//   pass 1   S_w = sum_j w_j [finite],  S_1 = sum_j w_j e_j,  cnt = #finite,  mean = S_1 / S_w
//   pass 2   d_j = e_j - mean (0 for a non-finite row),  u_j = w_j d_j,
//            c_0 = sum_j u_j d_j,  c_l = sum_j u_j d_{j+l}  (pairs inside the window, l <= L)
//   v = c_0 / S_w + sum_l 2 (1 - l / (L + 1)) (c_l / S_w);  not v > 0 -> c_0 / S_w;  sqrt(v)
// Two passes (deviations from the window's own weighted mean, no E x^2 - m^2 cancellation): the
// second pass re-reads rows that the first pass left in L2 / Infinity Cache.
// Layout as trailing_vol_kernel (attribution.hip): stocks contiguous, one thread per (stock,
// TD-date tile), the tile's TD + W - 1 rows walked newest first in blocks of RB rows, the next
// block's loads issued before the current block is summed.  The weight of (output k, row offset
// o) is table entry j = k - o: the table sits in LDS with zeros on both sides, so a row outside
// an output's window meets the weight 0 and every term it adds is an exact zero.  Every sum of
// an output therefore runs over its own window in row order with one rounding per operation
// (the library builds with -ffp-contract=fast; an empty asm on each product keeps it from being
// fused into the add that follows), whatever the tile the output falls in: a date shard that
// holds the halo reproduces the whole-series bits.  The CPU path performs the same operations in
// the same order: run with torch ops on the device it gives the kernel's bits, on the host it
// differs by at most one ulp (2.2e-16 relative, measured on an MI355X).
// The u_j of the last L rows stay in registers per output (L x TD doubles), so the accumulator
// count grows with L: the kernel is templated on L and TD shrinks with it.
// Limits: 0 <= L <= 5, 1 <= W <= 1024 (LDS table: TD - 1 + ceil((TD + W - 1) / RB) RB doubles,
// 8.3 KB at most), h >= W - 1, ceil(D / TD) <= 65535.
// Resource usage reported by the compiler for gfx950 (-Rpass-analysis=kernel-resource-usage;
// scratch 0 = no spill), <L, TD, RB>:
//   <0, 16, 16>  246 VGPR  0 AGPR  scratch 0      <1, 8, 8>  156 VGPR  0 AGPR  scratch 0
//   <2, 8, 8>    212 VGPR  0 AGPR  scratch 0      <3, 8, 8>  244 VGPR  0 AGPR  scratch 0
//   <4, 6, 6>    206 VGPR  0 AGPR  scratch 0      <5, 6, 6>  232 VGPR  0 AGPR  scratch 0
// (<1, 16, 16> and <5, 8, 8> fill the 256 VGPRs and park 58 / 86 values in AGPRs.)
//   spec_bias2_kernel<float / double>  28 VGPR, scratch 0
//
// ---- mfa_spec_bias2 ----------------------------------------------------------------------
// B2[t] = sum_n cap_n (e_n / sigma_n)^2 / sum_n cap_n over stocks with finite e, finite
// sigma > 0 and finite cap > 0 (NaN without one).  One 256-thread workgroup per date: thread i
// sums stocks i, i + 256, ... in order, the 64 lanes of a wave add through DPP (wave_total),
// thread 0 adds the four wave totals in wave order.  No atomics: two calls give the same bits.
#include "common.h"

namespace {

using namespace mfa;

// a product rounded on its own (see the header)
__device__ __forceinline__ double mul_rn(double a, double b) {
  double p = a * b;
  asm("" : "+v"(p));
  return p;
}

template <int L, int TD, int RB>
__global__ __launch_bounds__(256) void ewnw_vol_kernel(const double* __restrict__ halo, int h,
                                                       const double* __restrict__ e, int D, int N,
                                                       int W, int minp,
                                                       const double* __restrict__ wtab,
                                                       double* __restrict__ vol) {
  extern __shared__ double wl[];  // wl[PAD + j] = w_j for 0 <= j < W, 0.0 around it
  constexpr int PAD = TD - 1, NW = TD + RB - 1, LH = L > 0 ? L : 1;
  // row offset o = row - (t0 + h): output k holds it iff 0 <= k - o < W; rows o = TD-1 .. -(W-1)
  const int o_hi = TD - 1, nrows = TD + W - 1;
  const int nblk = (nrows + RB - 1) / RB;
  for (int i = threadIdx.x; i < PAD + nblk * RB; i += blockDim.x) {
    const int j = i - PAD;
    wl[i] = (j >= 0 && j < W) ? wtab[j] : 0.0;
  }
  __syncthreads();
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int t0 = blockIdx.y * TD;
  const int nt = D - t0 < TD ? D - t0 : TD;
  auto ld = [&](int i) -> double {  // ext row i (missing outside; only unwritten outputs see it)
    if (i < 0 || i >= h + D) return qnan();
    return i < h ? halo[(size_t)i * N + n] : e[(size_t)(i - h) * N + n];
  };
  double sw[TD], s1[TD], mean[TD];
  int cnt[TD];
#pragma unroll
  for (int k = 0; k < TD; ++k) {
    sw[k] = 0.0;
    s1[k] = 0.0;
    cnt[k] = 0;
  }
  double xb[RB], nb[RB], wv[NW];
  bool av[NW];
  // ---- pass 1: weighted mean and count of every output's window
#pragma unroll
  for (int u = 0; u < RB; ++u) xb[u] = ld(t0 + h + o_hi - u);
  for (int b = 0; b < nblk; ++b) {
    const int ob = o_hi - b * RB;  // offset of the block's first (newest) row
#pragma unroll
    for (int u = 0; u < RB; ++u) nb[u] = b + 1 < nblk ? ld(t0 + h + ob - RB - u) : 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {  // (k, u) -> table entry j = k + u - ob
      wv[i] = wl[PAD + i - ob];
      av[i] = (i - ob >= 0) && (i - ob < W);
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const double x = xb[u];
      const bool fin = __builtin_isfinite(x);
      const double xz = fin ? x : 0.0;
#pragma unroll
      for (int k = 0; k < TD; ++k) {
        const double wf = fin ? wv[k + u] : 0.0;
        cnt[k] += (fin && av[k + u]) ? 1 : 0;
        sw[k] = __dadd_rn(sw[k], wf);
        s1[k] = __dadd_rn(s1[k], mul_rn(wf, xz));
      }
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) xb[u] = nb[u];
  }
#pragma unroll
  for (int k = 0; k < TD; ++k) mean[k] = __ddiv_rn(s1[k], sw[k]);
  // ---- pass 2: weighted (auto)covariances of the deviations
  double c[L + 1][TD], hu[LH][TD];  // hu[l - 1][k]: u of the row l rows newer
#pragma unroll
  for (int k = 0; k < TD; ++k) {
#pragma unroll
    for (int l = 0; l <= L; ++l) c[l][k] = 0.0;
#pragma unroll
    for (int l = 0; l < LH; ++l) hu[l][k] = 0.0;
  }
#pragma unroll
  for (int u = 0; u < RB; ++u) xb[u] = ld(t0 + h + o_hi - u);
  for (int b = 0; b < nblk; ++b) {
    const int ob = o_hi - b * RB;
#pragma unroll
    for (int u = 0; u < RB; ++u) nb[u] = b + 1 < nblk ? ld(t0 + h + ob - RB - u) : 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      wv[i] = wl[PAD + i - ob];
      av[i] = (i - ob >= 0) && (i - ob < W);
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const double x = xb[u];
      const bool fin = __builtin_isfinite(x);
      const double xz = fin ? x : 0.0;
#pragma unroll
      for (int k = 0; k < TD; ++k) {
        const double d = (fin && av[k + u]) ? __dsub_rn(xz, mean[k]) : 0.0;
        const double uu = mul_rn(wv[k + u], d);
        c[0][k] = __dadd_rn(c[0][k], mul_rn(uu, d));
#pragma unroll
        for (int l = 1; l <= L; ++l) c[l][k] = __dadd_rn(c[l][k], mul_rn(hu[l - 1][k], d));
#pragma unroll
        for (int l = L - 1; l >= 1; --l) hu[l][k] = hu[l - 1][k];
        hu[0][k] = uu;
      }
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) xb[u] = nb[u];
  }
  const int thr = minp > 1 ? minp : 1;
#pragma unroll
  for (int k = 0; k < TD; ++k) {
    if (k < nt) {
      const double c0 = __ddiv_rn(c[0][k], sw[k]);
      double v = c0;
#pragma unroll
      for (int l = 1; l <= L; ++l) {
        constexpr double den = (double)(L + 1);
        const double coef = 2.0 * (1.0 - (double)l / den);  // folded at compile time
        v = __dadd_rn(v, mul_rn(coef, __ddiv_rn(c[l][k], sw[k])));
      }
      if (!(v > 0.0)) v = c0;
      vol[(size_t)(t0 + k) * N + n] = cnt[k] >= thr ? __dsqrt_rn(v) : qnan();
    }
  }
}

template <int L, int TD, int RB>
int ewnw_vol_launch(const double* halo, int h, const double* e, int D, int N, int W, int minp,
                    const double* wtab, double* vol, hipStream_t s) {
  const int gy = (D + TD - 1) / TD;
  if (gy > 65535) return (int)hipErrorInvalidValue;
  const int nblk = (TD + W - 1 + RB - 1) / RB;
  const size_t lds = (size_t)(TD - 1 + nblk * RB) * sizeof(double);
  hipLaunchKernelGGL((ewnw_vol_kernel<L, TD, RB>), dim3((N + 255) / 256, gy), dim3(256), lds, s,
                     halo, h, e, D, N, W, minp, wtab, vol);
  return (int)hipGetLastError();
}

template <typename T>
__global__ __launch_bounds__(256) void spec_bias2_kernel(const double* __restrict__ e,
                                                         const double* __restrict__ sigma,
                                                         const T* __restrict__ cap, int N,
                                                         double* __restrict__ out) {
  __shared__ double red[4][2];
  const int d = blockIdx.x, tid = threadIdx.x;
  const double* ed = e + (size_t)d * N;
  const double* sd = sigma + (size_t)d * N;
  const T* cd = cap + (size_t)d * N;
  double num = 0.0, den = 0.0;
  for (int n = tid; n < N; n += 256) {
    const double x = ed[n], s = sd[n], c = (double)cd[n];
    if (!(__builtin_isfinite(x) && __builtin_isfinite(s) && s > 0.0 && __builtin_isfinite(c) &&
          c > 0.0))
      continue;
    const double z = x / s;
    num += c * (z * z);
    den += c;
  }
  num = wave_total(num);
  den = wave_total(den);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = num;
    red[tid >> 6][1] = den;
  }
  __syncthreads();
  if (tid == 0) {
    const double a = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    const double b = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    out[d] = b > 0.0 ? a / b : qnan();
  }
}

}  // namespace

// Largest lag count and window of mfa_ewnw_vol (ops/specific_risk.py raises beyond them).
MFA_API int mfa_ewnw_max_lags(void) { return 5; }
MFA_API int mfa_ewnw_max_window(void) { return 1024; }

// vol [D][N] = EW Newey-West trailing specific volatility of e [D][N] over the W rows ending at
// each date, with halo [h][N] (h >= W - 1 rows preceding e, NaN where none; the last W - 1 are
// used) and wtab [W] = the weights w_j, j = 0 the date itself.
MFA_API int mfa_ewnw_vol(const double* halo, int h, const double* e, int D, int N, int W, int lags,
                         int min_periods, const double* wtab, double* vol, void* stream) {
  if (D <= 0 || N <= 0) return 0;
  if (W < 1 || W > 1024 || lags < 0 || lags > 5 || h < W - 1 || (h > 0 && !halo) || !wtab)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  switch (lags) {
    case 0: return ewnw_vol_launch<0, 16, 16>(halo, h, e, D, N, W, min_periods, wtab, vol, s);
    case 1: return ewnw_vol_launch<1, 8, 8>(halo, h, e, D, N, W, min_periods, wtab, vol, s);
    case 2: return ewnw_vol_launch<2, 8, 8>(halo, h, e, D, N, W, min_periods, wtab, vol, s);
    case 3: return ewnw_vol_launch<3, 8, 8>(halo, h, e, D, N, W, min_periods, wtab, vol, s);
    case 4: return ewnw_vol_launch<4, 6, 6>(halo, h, e, D, N, W, min_periods, wtab, vol, s);
    default: return ewnw_vol_launch<5, 6, 6>(halo, h, e, D, N, W, min_periods, wtab, vol, s);
  }
}

// B2 [D] from e, sigma [D][N] f64 and cap [D][N] f32.
MFA_API int mfa_spec_bias2(const double* e, const double* sigma, const float* cap, int D, int N,
                           double* out, void* stream) {
  if (D <= 0) return 0;
  if (N <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(spec_bias2_kernel<float>, dim3(D), dim3(256), 0, (hipStream_t)stream, e,
                     sigma, cap, N, out);
  return (int)hipGetLastError();
}

// Same with an fp64 cap.
MFA_API int mfa_spec_bias2_f64(const double* e, const double* sigma, const double* cap, int D,
                               int N, double* out, void* stream) {
  if (D <= 0) return 0;
  if (N <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(spec_bias2_kernel<double>, dim3(D), dim3(256), 0, (hipStream_t)stream, e,
                     sigma, cap, N, out);
  return (int)hipGetLastError();
}
