// Batched portfolio risk forecasts against realised returns: the sums behind the portfolio bias
// test (ops/bias_test.py), for every date d and portfolio b in one launch (gfx950).
//
// Test set T_d: stocks that pass the regression's validity rule (design_row.h), have a
// finite s_fc[d, n] > 0 and the optional universe[d, n] bit; a position outside T_d, or with a
// non-finite h, is dropped from every sum, so forecast and realised return describe the same
// holdings.  Per (d, b), all over T_d:
//   exposure x = X_d^T h, factor_var = x^T F_fc[d] x, specific_var = sum h^2 s_fc^2,
//   realised = sum h ret, held = sum |h|, and gross = sum |h| over every finite h.
//
// One 256-thread workgroup per (date, tile of 64 portfolios); wave w owns portfolios
// [16 w, 16 w + 16) of the tile over all stocks, so no sum ever crosses a wave.  The stock axis
// runs in chunks of 64: the workgroup builds the chunk's K = 1 + P + Q columns
// [ret | X_1..X_Q | one-hot industries] in LDS from the raw panel (stocks outside T_d zeroed),
// each wave stages its 16 x 64 slice of H, and the sums h . column are 16x16x4 fp64 MFMA chains
// (one accumulator tile per 16 columns, at most 4 as K <= 64): the column tile is read by all four
// waves, which is the reuse.  The sums that are not linear in h (h^2 s^2, |h|) and sum h ride in
// the lane that feeds the A operand; their four per-lane partials (stocks n = i mod 4) are added
// in a fixed order at the end.  The z-scoring is folded in from stats (design_row.h), and the
// K x K quadratic form runs in the epilogue with F_fc[d] in LDS.  Every sum has a fixed order that
// depends on the stock index alone: the value of (d, b) does not depend on B, on b's row in its
// tile, on the layout of H or on the other dates of the launch.
//
// Launch order: blockIdx.x = date, blockIdx.y = portfolio tile, so the workgroups in flight share
// one tile of a static H (64 N doubles: L2-resident) and stream different dates of the panel.
// 16x16x4 f64 layouts (tools/probes/mfma64_probe.hip): A operand lane l = A[l & 15][l >> 4],
// B operand lane l = B[l >> 4][l & 15], register e of lane l = D[(l >> 4) + 4 e][l & 15].
#include "design_row.h"

namespace {

using namespace mfa;

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;        // portfolios per workgroup (16 per wave)
constexpr int kChunk = 64;       // stocks per LDS chunk
constexpr int kLd = kChunk + 4;  // row stride = 4 mod 32 doubles: the MFMA operand reads of a
                                 // wave touch every LDS bank pair exactly twice

__host__ __device__ constexpr size_t pb_lds_doubles(int K) {
  return (size_t)(kTile + 16 * ((K + 15) / 16)) * kLd + kChunk;
}

// One chunk of 64 stocks for a wave's 16 portfolios: k-step s covers stocks s .. s + 3, lane
// (r16, k4) feeding portfolio r16 / column 16 t + r16 at stock s + k4 (the pointers are already
// offset to the lane's row and k4).
template <int CT>
__device__ __forceinline__ void pb_chunk(const double* __restrict__ Ar,
                                         const double* __restrict__ Cr,
                                         const double* __restrict__ Vr, f64x4 (&acc)[4],
                                         double& a_sum, double& a_spec, double& a_held,
                                         double& a_gross) {
#pragma unroll 2
  for (int s = 0; s < kChunk; s += 4) {
    const double a = Ar[s];
    const double sv = Vr[s];
    double b[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) b[t] = Cr[16 * t * kLd + s];
    const double am = sv > 0.0 ? a : 0.0;
    const double as = am * sv;
    a_gross += fabs(a);
    a_held += fabs(am);
    a_sum += am;
    a_spec = fma(as, as, a_spec);
#pragma unroll
    for (int t = 0; t < CT; ++t)
      acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[t], acc[t], 0, 0, 0);
  }
}

template <int Q, typename T>
__global__ __launch_bounds__(kThreads) void portfolio_batch_kernel(
    const T* __restrict__ X, const T* __restrict__ cap, const T* __restrict__ ret,
    const int16_t* __restrict__ ind, const double* __restrict__ stats,
    const double* __restrict__ H, long long h_dstride, const double* __restrict__ s_fc,
    const double* __restrict__ F, const uint8_t* __restrict__ universe, int N, int P, int B,
    double* __restrict__ factor_var, double* __restrict__ specific_var,
    double* __restrict__ realised, double* __restrict__ held, double* __restrict__ gross,
    double* __restrict__ exposure) {
  extern __shared__ double pb_lds[];
  const int d = blockIdx.x, b0 = blockIdx.y * kTile;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r16 = lane & 15, k4 = lane >> 4;
  const DesignDate<T> day(X, cap, ret, ind, d, N, P, Q);
  const int K = 1 + P + Q, CT = (K + 15) >> 4;
  double* As = pb_lds;               // [4 waves][16][kLd]: H slices; exposures in the epilogue
  double* Cs = As + kTile * kLd;     // [16 CT][kLd]: column tile; F_fc[d] in the epilogue
  double* Vs = Cs + 16 * CT * kLd;   // [kChunk]: s_fc on T_d, 0 outside
  double* Aw = As + wid * 16 * kLd;
  const bool active = b0 + 16 * wid < B;  // wave-uniform: this wave has portfolios

  const double* sd = s_fc + (size_t)d * N;
  const uint8_t* ud = universe ? universe + (size_t)d * N : nullptr;
  const double* Hw = H + (size_t)d * (size_t)h_dstride + (size_t)(b0 + 16 * wid) * N;
  const int nrow = active ? min(16, B - b0 - 16 * wid) : 0;

  // pad columns K .. 16 CT - 1 are never written again
  for (int i = K * kLd + tid; i < 16 * CT * kLd; i += kThreads) Cs[i] = 0.0;

  // the chunk in flight, in registers: loaded one chunk ahead of the MFMA loop
  // (every address is clamped into range, so no load hides behind a branch; what lies outside
  // N or the wave's rows is dropped when the registers go to LDS)
  T xr[Q], cr, rr;
  double sr, hr[16];
  int jr, ur = 1;
  bool inr;
  auto load = [&](int n0) {
    const int n = n0 + lane;
    inr = n < N;
    const int nn = inr ? n : N - 1;
    day.load_base(nn, cr, rr, jr);
    sr = sd[nn];
    if (ud) ur = ud[nn];
    day.load_styles(nn, xr);
    if (active) {
#pragma unroll
      for (int r = 0; r < 16; ++r) hr[r] = Hw[(size_t)min(r, nrow - 1) * N + nn];
    }
  };

  f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  double a_sum = 0.0, a_spec = 0.0, a_held = 0.0, a_gross = 0.0;

  load(0);
  for (int n0 = 0; n0 < N; n0 += kChunk) {
    {  // registers -> LDS: thread (lane, wid) writes the columns c = wid mod 4 of stock n0 + lane
      bool ok = inr && (ur != 0) && MFA_DESIGN_BASE_OK(T, cr, rr, jr, day.Pseg) &&
                __builtin_isfinite(sr) && (sr > 0.0);
#pragma unroll
      for (int q = 0; q < Q; ++q) ok = ok && __builtin_isfinite(xr[q]);
      if (wid == 0) {
        Cs[lane] = ok ? (double)rr : 0.0;
        Vs[lane] = ok ? sr : 0.0;
      }
#pragma unroll
      for (int q = 0; q < Q; ++q)
        if (((1 + q) & 3) == wid) Cs[(1 + q) * kLd + lane] = ok ? (double)xr[q] : 0.0;
      for (int p = (wid - 1 - Q) & 3; p < P; p += 4)
        Cs[(1 + Q + p) * kLd + lane] = (ok && p == jr) ? 1.0 : 0.0;
      if (active) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          Aw[r * kLd + lane] = (inr && r < nrow && __builtin_isfinite(hr[r])) ? hr[r] : 0.0;
      }
    }
    __syncthreads();
    if (n0 + kChunk < N) load(n0 + kChunk);
    if (active) {
      const double* Ar = Aw + r16 * kLd + k4;
      const double* Cr = Cs + r16 * kLd + k4;
      switch (CT) {  // wave-uniform; the tile count is a compile-time constant inside
        case 1: pb_chunk<1>(Ar, Cr, Vs + k4, acc, a_sum, a_spec, a_held, a_gross); break;
        case 2: pb_chunk<2>(Ar, Cr, Vs + k4, acc, a_sum, a_spec, a_held, a_gross); break;
        case 3: pb_chunk<3>(Ar, Cr, Vs + k4, acc, a_sum, a_spec, a_held, a_gross); break;
        default: pb_chunk<4>(Ar, Cr, Vs + k4, acc, a_sum, a_spec, a_held, a_gross); break;
      }
    }
    __syncthreads();
  }

  // the four partials of portfolio r16 (lanes r16, r16 + 16, + 32, + 48), in that order
  auto fold = [&](double v) {
    return ((__shfl(v, r16, kWave) + __shfl(v, r16 + 16, kWave)) + __shfl(v, r16 + 32, kWave)) +
           __shfl(v, r16 + 48, kWave);
  };
  const double hs = fold(a_sum), spec = fold(a_spec), hld = fold(a_held), grs = fold(a_gross);

  // epilogue: F_fc[d] -> Cs (the loop's last barrier has passed), exposures -> this wave's As
  const int kF = K | 1;
  const double* st = stats + (size_t)d * (Q + 2);
  // a zero pooled sigma has no z-scores either
  const int bad_stats = !stats_finite(st, Q) || !(st[Q] > 0.0);
  int bad = 0;
  if (F) {
    const double* Fd = F + (size_t)d * K * K;
    for (int e = tid; e < K * K; e += kThreads) {
      const int i = e / K, k = e - i * K;
      const double v = Fd[e];
      bad |= !__builtin_isfinite(v);
      Cs[i * kF + k] = v;
    }
  } else {
    bad = 1;
  }
  const double isig = 1.0 / st[Q];
  const size_t row = (size_t)d * B + b0 + 16 * wid;  // + portfolio within the wave
  if (active) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < CT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 16 * t + r16, b = k4 + 4 * e;
          const double hb = __shfl(hs, b, kWave);
          const double v = acc[t][e];
          if (c == 0) {
            if (b < nrow) realised[row + b] = v;
          } else if (c <= Q) {
            Aw[b * kF + P + c] = unfold_zscore(v, st[c - 1], hb, isig);
          } else if (c < K) {
            Aw[b * kF + c - Q] = v;
          }
        }
      }
    }
    if (k4 == 0) Aw[r16 * kF] = hs;
  }
  bad = __syncthreads_or(bad) | bad_stats;
  if (!active) return;
  double part = 0.0;  // rows k = k4 mod 4 of x^T F x for portfolio r16
  for (int k = k4; k < K; k += 4) {
    double y = 0.0;
    for (int l = 0; l < K; ++l) y = fma(Cs[k * kF + l], Aw[r16 * kF + l], y);
    part = fma(Aw[r16 * kF + k], y, part);
  }
  const double fv = fold(part);
  if (k4 == 0 && r16 < nrow) {
    factor_var[row + r16] = bad ? qnan() : fv;
    specific_var[row + r16] = spec;
    held[row + r16] = hld;
    gross[row + r16] = grs;
  }
  if (exposure)
    for (int e = lane; e < nrow * K; e += kWave) {
      const int b = e / K, k = e - b * K;
      exposure[(row + b) * K + k] = bad_stats ? qnan() : Aw[b * kF + k];
    }
}

template <int Q, typename T>
int portfolio_batch_launch(const T* X, const T* cap, const T* ret, const int16_t* ind,
                           const double* stats, const double* H, long long h_dstride,
                           const double* s_fc, const double* F, const uint8_t* universe, int D,
                           int N, int P, int B, double* factor_var, double* specific_var,
                           double* realised, double* held, double* gross, double* exposure,
                           hipStream_t s) {
  const size_t lds = pb_lds_doubles(1 + P + Q) * sizeof(double);
  if (hipError_t err = raise_dynamic_lds<portfolio_batch_kernel<Q, T>>(lds)) return (int)err;
  hipLaunchKernelGGL((portfolio_batch_kernel<Q, T>), dim3(D, (B + kTile - 1) / kTile),
                     dim3(kThreads), lds, s, X, cap, ret, P > 0 ? ind : nullptr, stats, H,
                     h_dstride, s_fc, F, universe, N, P, B, factor_var, specific_var, realised,
                     held, gross, exposure);
  return (int)hipGetLastError();
}

template <typename T>
int portfolio_batch_dispatch(const T* X, const T* cap, const T* ret, const int16_t* ind,
                             const double* stats, const double* H, long long h_dstride,
                             const double* s_fc, const double* F, const uint8_t* universe, int D,
                             int N, int P, int Q, int B, double* factor_var, double* specific_var,
                             double* realised, double* held, double* gross, double* exposure,
                             void* stream) {
  if (D <= 0 || B <= 0) return 0;
  if (Q < 1 || Q > kMaxQ || P < 0 || 1 + P + Q > kMaxK || N <= 0 ||
      (B + kTile - 1) / kTile > 65535 || (h_dstride != 0 && h_dstride != (long long)B * N))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  int err = (int)hipErrorInvalidValue;
  dispatch_q(Q, [&](auto q) {
    err = portfolio_batch_launch<decltype(q)::value, T>(
        X, cap, ret, ind, stats, H, h_dstride, s_fc, F, universe, D, N, P, B, factor_var,
        specific_var, realised, held, gross, exposure, s);
  });
  return err;
}

}  // namespace

// X [D][Q][N], cap / ret [D][N] f32, ind [D][N] int16 (nullable when P == 0), stats [D][Q+2] f64
// from mfa_xs_wls; H f64 weights, h_dstride = 0: [B][N] held on every date (read in place),
// h_dstride = B N: [D][B][N]; s_fc [D][N] f64 specific-volatility forecasts; F [D][K][K] f64
// factor-covariance forecasts (nullable: factor_var is then NaN); universe [D][N] bytes
// (nullable).  Outputs [D][B] f64, exposure [D][B][K] f64 (nullable).  K = 1 + P + Q <= 64,
// Q <= 16.  A date with a non-finite F gets NaN factor_var, one with a non-finite stats row (or a
// pooled sigma that is not > 0) NaN factor_var and exposure.  Bitwise reproducible.
MFA_API int mfa_portfolio_batch(const float* X, const float* cap, const float* ret,
                                const int16_t* ind, const double* stats, const double* H,
                                long long h_dstride, const double* s_fc, const double* F,
                                const uint8_t* universe, int D, int N, int P, int Q, int B,
                                double* factor_var, double* specific_var, double* realised,
                                double* held, double* gross, double* exposure, void* stream) {
  return portfolio_batch_dispatch<float>(X, cap, ret, ind, stats, H, h_dstride, s_fc, F, universe,
                                         D, N, P, Q, B, factor_var, specific_var, realised, held,
                                         gross, exposure, stream);
}

// Same with an fp64 panel.
MFA_API int mfa_portfolio_batch_f64(const double* X, const double* cap, const double* ret,
                                    const int16_t* ind, const double* stats, const double* H,
                                    long long h_dstride, const double* s_fc, const double* F,
                                    const uint8_t* universe, int D, int N, int P, int Q, int B,
                                    double* factor_var, double* specific_var, double* realised,
                                    double* held, double* gross, double* exposure, void* stream) {
  return portfolio_batch_dispatch<double>(X, cap, ret, ind, stats, H, h_dstride, s_fc, F,
                                          universe, D, N, P, Q, B, factor_var, specific_var,
                                          realised, held, gross, exposure, stream);
}
