// Factor evaluation: per-date information coefficient, rank IC (Spearman) and quantile-bucket
// forward returns of S signals against H targets, and the average ranks themselves.
//
// Inputs: signals x [D][S][N] (fp32 or fp64), targets y [D][H][N] fp64, universe [D][N] bytes.
// The pair set of a triple (d, s, h): universe[d][n] != 0 and x[d][s][n], y[d][h][n] finite.
//   n        members of the pair set
//   ic       Sxy / sqrt(Sxx Syy) of the deviations from the fp64 means (two passes)
//   rank_ic  the same of the average ranks within the pair set (ties share the mean of their
//            positions, -0.0 ties with +0.0); the deviations r - (n + 1) / 2 are half-integers,
//            so the three sums are exact in fp64 whatever their order
//   q_ret    mean of y over G quantile groups of x: group = the number of inner edges strictly
//            below the value, edges = np.quantile(x, linspace(0, 1, G + 1)) (method "linear") in
//            numpy's own arithmetic, as bayes_shrink_kernel of xs_reduce.hip; q_count the members
// NaN: ic / rank_ic when n < 2 or Sxx Syy is not > 0, q_ret of an empty group.
//
// factor_ic_kernel: one workgroup of 16 waves per (date, signal), looping over the horizons
// (paired: only h = s, outputs [D][S]).  Per triple:
//   1. counts, means and the Pearson sums straight from global memory / L2 (no LDS);
//   2. (x key fp64, stock index u16) pairs, +inf outside the pair set, bitonic-sorted in LDS;
//   3. each sorted position finds its tie run (neighbour compare, then lower / upper bound binary
//      searches in the sorted keys: log N steps also on an all-equal date) and stores the
//      average rank rx[stock] as fp32 in LDS (ranks up to 8192.5 are exact);
//   4. the G - 1 inner edges from the sorted keys;
//   5. the key / index arrays are reused for y: each sorted position forms ry, reads rx[stock]
//      and accumulates the rank sums; no ry array is kept;
//   6. bucket sums: x and y once more from L2, per-thread partial sums in registers over chunks
//      of kGC groups.
// Steps 2-4 are skipped when the pair set equals that of the horizon x was last sorted for
// (counted per triple, so the results stay those of the per-triple definition).
// Every floating sum runs lane -> wave (DPP, wave_total) -> the 16 waves in wave order; no
// atomics; two calls give the same bits, and a triple's results do not depend on S, H, D or on
// the other signals and horizons of the call.
//
// Dynamic LDS: NP 8 (keys) + N 4 (rx) + NP 2 (idx) bytes, NP = N rounded up to a power of two:
// 112 KB at N = 8192 (the launcher raises the kernel's dynamic-LDS limit), 100 KB at N = 5000,
// next to 2.8 KB static.  Limits: N <= 8192, G <= 32 (H <= 8 is the Python side's).
//
// One workgroup per CU above N = 4096, and the sorts are the time: at 2520 x 5000, S = 10, three
// horizons, G = 5 the call takes 62.2 ms, one horizon 21.0 ms, without buckets 60.7 ms, and
// xs_rank (one sort per row) 10.0 ms (profiles/r12/factor_eval_bench.log).  Running three steps
// of the network per LDS round trip (8 pairs per thread in registers, a padded layout against
// bank conflicts: 35 round trips instead of 91) measured 63.8 ms
// (profiles/r12/factor_eval_bench_grouped_sort.log), so neither LDS traffic nor the barrier
// count bounds the sort; the plain network stays.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage:
//   factor_ic_kernel<float> / <double>  61 VGPR, 0 AGPR, 106 SGPR, no scratch, 2816 B static LDS
//   xs_rank_kernel<float>               12 VGPR, 0 AGPR,  33 SGPR, no scratch,    0 B static LDS
//   xs_rank_kernel<double>              14 VGPR, 0 AGPR,  33 SGPR, no scratch,    0 B static LDS
#include "common.h"

namespace {

using namespace mfa;

constexpr int kThreads = 1024, kWaves = kThreads / kWave;
constexpr int kMaxN = 8192, kMaxG = 32, kGC = 8;

template <typename T>
__device__ __forceinline__ bool finv(T v) { return __builtin_isfinite(v); }

// Totals of M per-thread values over the workgroup, the same bits in every thread.
template <int M>
__device__ __forceinline__ void block_totals(double (&v)[M], double (*ws)[M]) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
  for (int m = 0; m < M; ++m) v[m] = wave_total(v[m]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < M; ++m) ws[wv][m] = v[m];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < M; ++m) v[m] = 0.0;
#pragma unroll 2
  for (int w = 0; w < kWaves; ++w) {
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] += ws[w][m];
  }
}

// Ascending bitonic sort of (keys, idx) [NP] in LDS by key; NP a power of two.  Thread t owns
// the compare-exchange of elements i (bit j clear) and i | j.  Ends with a barrier.
__device__ __forceinline__ void bitonic_sort(double* keys, uint16_t* idx, int NP) {
  __syncthreads();
  for (int k = 2; k <= NP; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (NP >> 1); t += kThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), ij = i | j;
        const bool up = (i & k) == 0;
        const double a = keys[i], b = keys[ij];
        if ((a > b) == up) {
          keys[i] = b;
          keys[ij] = a;
          const uint16_t ia = idx[i];
          idx[i] = idx[ij];
          idx[ij] = ia;
        }
      }
      __syncthreads();
    }
}

// Average rank (1-based) of sorted position p among keys[0, n): the mean of the positions of
// its tie run [lo, hi).
__device__ __forceinline__ float avg_rank(const double* keys, int n, int p) {
  const double k = keys[p];
  int lo = p, hi = p + 1;
  if (p > 0 && keys[p - 1] == k) {
    int a = 0, b = p - 1;
    while (a < b) {
      const int m = (a + b) >> 1;
      if (keys[m] < k) a = m + 1; else b = m;
    }
    lo = a;
  }
  if (p + 1 < n && keys[p + 1] == k) {
    int a = p + 2, b = n;
    while (a < b) {
      const int m = (a + b) >> 1;
      if (keys[m] <= k) a = m + 1; else b = m;
    }
    hi = a;
  }
  return 0.5f * (float)(lo + hi + 1);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void factor_ic_kernel(
    const T* __restrict__ x, const double* __restrict__ y, const uint8_t* __restrict__ univ, int S,
    int H, int N, int NP, int G, int paired, int* __restrict__ n_out, double* __restrict__ ic_out,
    double* __restrict__ ric_out, double* __restrict__ qret_out, int* __restrict__ qcnt_out) {
  extern __shared__ double dyn[];
  double* keys = dyn;                                   // [NP]
  float* rx = reinterpret_cast<float*>(keys + NP);      // [N]
  uint16_t* idx = reinterpret_cast<uint16_t*>(rx + N);  // [NP]
  __shared__ double ws[kWaves][4];
  __shared__ double wq[kWaves][kGC][2];
  __shared__ double edges[kMaxG];  // edges[k], 1 <= k < G: upper edge of group k - 1
  const int tid = threadIdx.x, s = blockIdx.x % S, d = blockIdx.x / S;
  const T* xd = x + ((size_t)d * S + s) * N;
  const uint8_t* ud = univ + (size_t)d * N;
  int hs = -1;  // horizon whose pair set rx and edges were formed on
  const int h0 = paired ? s : 0, h1 = paired ? s + 1 : H;
  for (int h = h0; h < h1; ++h) {
    const double* yd = y + ((size_t)d * H + h) * N;
    const double* ys = hs >= 0 ? y + ((size_t)d * H + hs) * N : nullptr;
    const size_t o = paired ? (size_t)d * S + s : ((size_t)d * S + s) * H + h;
    // ---- 1. count, means, Pearson sums; and whether the pair set is the one x was sorted on
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < N; i += kThreads) {
      const T xv = xd[i];
      const double yv = yd[i];
      const bool base = ud[i] != 0 && finv(xv);
      if (base && finv(yv)) {
        a[0] += 1.0;
        a[1] += (double)xv;
        a[2] += yv;
      }
      if (ys && base && finv(yv) != finv(ys[i])) a[3] += 1.0;
    }
    block_totals<4>(a, ws);
    const int n = (int)a[0];
    const bool reuse = hs >= 0 && a[3] == 0.0;
    const double mx = a[1] / a[0], my = a[2] / a[0];
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < N; i += kThreads) {
      const T xv = xd[i];
      const double yv = yd[i];
      if (ud[i] != 0 && finv(xv) && finv(yv)) {
        const double dx = (double)xv - mx, dy = yv - my;
        c[0] = fma(dx, dy, c[0]);
        c[1] = fma(dx, dx, c[1]);
        c[2] = fma(dy, dy, c[2]);
      }
    }
    block_totals<4>(c, ws);
    if (tid == 0) {
      const double den = c[1] * c[2];
      n_out[o] = n;
      ic_out[o] = (n >= 2 && den > 0.0) ? c[0] / sqrt(den) : qnan();
    }
    // ---- 2-4. sort x, average ranks, quantile edges
    if (!reuse) {
      __syncthreads();
      for (int i = tid; i < NP; i += kThreads) {
        bool ok = false;
        double kv = __builtin_huge_val();
        if (i < N) {
          const T xv = xd[i];
          ok = ud[i] != 0 && finv(xv) && finv(yd[i]);
          if (ok) kv = (double)xv;
        }
        keys[i] = kv;
        idx[i] = (uint16_t)i;
      }
      bitonic_sort(keys, idx, NP);
      for (int p = tid; p < n; p += kThreads) rx[idx[p]] = avg_rank(keys, n, p);
      if (tid >= 1 && tid < G && n > 0) {
        const double pos = __dmul_rn((double)(n - 1), __dmul_rn((double)tid, 1.0 / (double)G));
        const int lo = min((int)floor(pos), n - 1);
        const int hi = min(lo + 1, n - 1);
        const double fr = pos - (double)lo;
        const double ka = keys[lo], kb = keys[hi], ba = kb - ka;
        edges[tid] = fr >= 0.5 ? __dsub_rn(kb, __dmul_rn(ba, 1.0 - fr))
                               : __dadd_rn(ka, __dmul_rn(ba, fr));
      }
      hs = h;
    }
    // ---- 5. sort y, rank sums against rx
    __syncthreads();
    for (int i = tid; i < NP; i += kThreads) {
      double kv = __builtin_huge_val();
      if (i < N) {
        const double yv = yd[i];
        if (ud[i] != 0 && finv(xd[i]) && finv(yv)) kv = yv;
      }
      keys[i] = kv;
      idx[i] = (uint16_t)i;
    }
    bitonic_sort(keys, idx, NP);
    double r[4] = {0.0, 0.0, 0.0, 0.0};
    const double mid = 0.5 * (double)(n + 1);
    for (int p = tid; p < n; p += kThreads) {
      const double ay = (double)avg_rank(keys, n, p) - mid;
      const double ax = (double)rx[idx[p]] - mid;
      r[0] += ax * ay;
      r[1] += ax * ax;
      r[2] += ay * ay;
    }
    block_totals<4>(r, ws);
    if (tid == 0) {
      const double den = r[1] * r[2];
      ric_out[o] = (n >= 2 && den > 0.0) ? r[0] / sqrt(den) : qnan();
    }
    // ---- 6. bucket sums in a fixed order: thread t owns stocks t, t + 1024, ... and keeps the
    // partial sums of kGC groups at a time, wave_total adds the lanes, thread j the 16 waves
    const int lane = tid & (kWave - 1), wv = tid / kWave;
    for (int g0 = 0; g0 < G; g0 += kGC) {
      double q0[kGC];
      int q1[kGC];
#pragma unroll
      for (int j = 0; j < kGC; ++j) { q0[j] = 0.0; q1[j] = 0; }
#pragma unroll 1
      for (int i = tid; i < N; i += kThreads) {
        const T xv = xd[i];
        const double yv = yd[i];
        if (!(ud[i] != 0 && finv(xv) && finv(yv))) continue;
        int g = 0;
#pragma unroll 1
        for (int k = 1; k < G; ++k) g += (double)xv > edges[k] ? 1 : 0;
        const int j = g - g0;
#pragma unroll
        for (int k = 0; k < kGC; ++k)
          if (j == k) { q0[k] += yv; q1[k] += 1; }
      }
#pragma unroll
      for (int j = 0; j < kGC; ++j) {
        const double t0 = wave_total(q0[j]), t1 = wave_total((double)q1[j]);
        if (lane == 0) { wq[wv][j][0] = t0; wq[wv][j][1] = t1; }
      }
      __syncthreads();
      if (tid < kGC && g0 + tid < G) {
        double s0 = 0.0, s1 = 0.0;
        for (int w = 0; w < kWaves; ++w) { s0 += wq[w][tid][0]; s1 += wq[w][tid][1]; }
        qret_out[o * G + g0 + tid] = s1 > 0.0 ? s0 / s1 : qnan();
        qcnt_out[o * G + g0 + tid] = (int)s1;
      }
      __syncthreads();
    }
  }
}

// Average ranks of x [D][S][N] within universe & finite, as fp64 [D][S][N], NaN outside.
template <typename T>
__global__ __launch_bounds__(kThreads) void xs_rank_kernel(const T* __restrict__ x,
                                                           const uint8_t* __restrict__ univ, int S,
                                                           int N, int NP, double* __restrict__ out) {
  extern __shared__ double dyn[];
  double* keys = dyn;
  float* rx = reinterpret_cast<float*>(keys + NP);
  uint16_t* idx = reinterpret_cast<uint16_t*>(rx + N);
  const int tid = threadIdx.x, s = blockIdx.x % S, d = blockIdx.x / S;
  const T* xd = x + ((size_t)d * S + s) * N;
  const uint8_t* ud = univ + (size_t)d * N;
  for (int i = tid; i < NP; i += kThreads) {
    double kv = __builtin_huge_val();
    if (i < N) {
      const T xv = xd[i];
      if (ud[i] != 0 && finv(xv)) kv = (double)xv;
    }
    keys[i] = kv;
    idx[i] = (uint16_t)i;
  }
  bitonic_sort(keys, idx, NP);
  int n = 0;  // the finite keys come first
  {
    int a = 0, b = NP;
    while (a < b) {
      const int m = (a + b) >> 1;
      if (keys[m] < __builtin_huge_val()) a = m + 1; else b = m;
    }
    n = a;
  }
  for (int p = tid; p < n; p += kThreads) rx[idx[p]] = avg_rank(keys, n, p);
  __syncthreads();
  double* od = out + ((size_t)d * S + s) * N;
  for (int i = tid; i < N; i += kThreads)
    od[i] = (ud[i] != 0 && finv(xd[i])) ? (double)rx[i] : qnan();
}

inline int pow2_at_least(int N) {
  int NP = 1;
  while (NP < N) NP <<= 1;
  return NP;
}

inline size_t lds_bytes(int N, int NP) { return (size_t)NP * 10 + (size_t)N * 4; }

// dynamic + static LDS pass 64 KB from N = 4097 on (NP = 8192): raise the kernel's limit once per size
// (a gfx950 CU has 160 KB)
template <typename K>
hipError_t raise_lds(K kernel, size_t lds, size_t& attr) {
  if (attr >= lds) return hipSuccess;
  if (hipError_t err = hipFuncSetAttribute((const void*)kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
    return err;
  attr = lds;
  return hipSuccess;
}

template <typename T>
int launch_factor_ic(const T* x, const double* y, const uint8_t* univ, int D, int S, int H, int N,
                     int G, int paired, int* n_out, double* ic, double* ric, double* qret,
                     int* qcnt, void* stream) {
  if (D <= 0 || S <= 0 || H <= 0) return 0;
  if (N < 1 || N > kMaxN || G < 0 || G > kMaxG || (long long)D * S > 0x7fffffffLL ||
      (paired && H != S))
    return (int)hipErrorInvalidValue;
  const int NP = pow2_at_least(N);
  const size_t lds = lds_bytes(N, NP);
  static size_t attr = 32 * 1024;
  if (hipError_t err = raise_lds(factor_ic_kernel<T>, lds, attr)) return (int)err;
  hipLaunchKernelGGL(factor_ic_kernel<T>, dim3((unsigned)(D * S)), dim3(kThreads), lds, (hipStream_t)stream, x,
                     y, univ, S, H, N, NP, G, paired, n_out, ic, ric, qret, qcnt);
  return (int)hipGetLastError();
}

template <typename T>
int launch_xs_rank(const T* x, const uint8_t* univ, int D, int S, int N, double* out,
                   void* stream) {
  if (D <= 0 || S <= 0) return 0;
  if (N < 1 || N > kMaxN || (long long)D * S > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const int NP = pow2_at_least(N);
  const size_t lds = lds_bytes(N, NP);
  static size_t attr = 32 * 1024;
  if (hipError_t err = raise_lds(xs_rank_kernel<T>, lds, attr)) return (int)err;
  hipLaunchKernelGGL(xs_rank_kernel<T>, dim3((unsigned)(D * S)), dim3(kThreads), lds, (hipStream_t)stream, x,
                     univ, S, N, NP, out);
  return (int)hipGetLastError();
}

}  // namespace

// x [D][S][N], y [D][H][N], univ [D][N] (bytes); n / ic / rank_ic [D][S][H] and q_ret / q_count
// [D][S][H][G], or with paired != 0 (H == S, only h = s) [D][S] and [D][S][G].  G = 0: no
// buckets (q_ret / q_count may be null).
MFA_API int mfa_factor_ic(const float* x, const double* y, const uint8_t* univ, int D, int S, int H,
                          int N, int G, int paired, int* n_out, double* ic, double* ric,
                          double* qret, int* qcnt, void* stream) {
  return launch_factor_ic<float>(x, y, univ, D, S, H, N, G, paired, n_out, ic, ric, qret, qcnt,
                                 stream);
}

MFA_API int mfa_factor_ic_f64(const double* x, const double* y, const uint8_t* univ, int D, int S,
                              int H, int N, int G, int paired, int* n_out, double* ic, double* ric,
                              double* qret, int* qcnt, void* stream) {
  return launch_factor_ic<double>(x, y, univ, D, S, H, N, G, paired, n_out, ic, ric, qret, qcnt,
                                  stream);
}

MFA_API int mfa_xs_rank(const float* x, const uint8_t* univ, int D, int S, int N, double* out,
                        void* stream) {
  return launch_xs_rank<float>(x, univ, D, S, N, out, stream);
}

MFA_API int mfa_xs_rank_f64(const double* x, const uint8_t* univ, int D, int S, int N, double* out,
                            void* stream) {
  return launch_xs_rank<double>(x, univ, D, S, N, out, stream);
}
