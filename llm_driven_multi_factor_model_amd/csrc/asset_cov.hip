// Dense asset covariance / correlation blocks of a basket of stocks (ops/asset_cov.py, gfx950):
//   cov[d, i, j] = x_{n_i}^T F_d x_{n_j} + s_{n_i}^2 [n_i == n_j],   n_i = index[d, i],
// for every date d and the M members of the date's basket, with x_n the design row of stock n
// (design_row.h: [country | one-hot industries | z-scored styles], never materialised for the
// panel) -- the matrix every portfolio method of this package applies without forming it.
//
// Member i of date d is valid when n_i >= 0 passes the regression's validity rule, has a finite
// s > 0 and the optional universe bit, and the date's F and stats row are finite.  Rows and
// columns of the other members are NaN; vol = sqrt(x F x + s^2) on the valid members.
//
// Two kernels per chunk of dates, both on the caller's stream:
//   * rows:  one workgroup per (date, 64 members).  Gathers the members' raw panel entries by
//     stock index, builds the z-scored design rows Z [64][KP] in LDS (KP = 16 ceil(K / 16), pad
//     columns 0), multiplies by F_d (LDS) on the fp64 matrix cores, Y = Z F, and writes Z, Y, s^2
//     and the member's stock id (-1 when not valid) to scratch, vol and valid to the outputs.
//   * tile:  one workgroup per (date, 64 x 64 tile with tile-row >= tile-col).  Stages the
//     tile's Y rows and Z rows in LDS, wave w owns the 16 x 64 strip of rows 16 w: four
//     accumulators, KP / 4 MFMA steps.  The epilogue adds s^2 where the stock ids agree, scales by
//     1 / (vol_i vol_j) for a correlation (1.0 exactly where i == j) and puts NaN on non-valid
//     rows and columns.  The finished tile goes through LDS, so that the tile and its mirror are
//     both stored as whole rows (a mirror stored from the accumulator layout would be 8-byte
//     stores at stride M).  A diagonal tile keeps its lower triangle and mirrors it in LDS.
// Only entries with i >= j are ever computed; cov[d] is symmetric bit for bit.  Every entry is one
// MFMA chain over k in a fixed order: two calls give the same bits and date d does not depend on
// the other dates of the call.
//
// 16x16x4 f64 layouts (as portfolio_batch.hip): A operand lane l = A[l & 15][l >> 4], B operand
// lane l = B[l >> 4][l & 15], register e of lane l = D[(l >> 4) + 4 e][l & 15].
#include "design_row.h"

namespace {

using namespace mfa;

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;       // members per workgroup row / column (16 per wave)
constexpr int kCld = kTile + 1; // row stride of the finished tile in LDS: column reads (the
                                // mirror) and row reads are both conflict-free

__host__ __device__ constexpr int ac_kp(int K) { return 16 * ((K + 15) / 16); }
// operand row stride: KP + 4 = 4 mod 16 doubles (portfolio_batch.hip's conflict-free stride)
__host__ __device__ constexpr int ac_ld(int K) { return ac_kp(K) + 4; }
__host__ __device__ constexpr size_t ac_rows_lds(int K) {  // Zs, Ys, Fs + 4 x 64 flags
  return (size_t)(2 * kTile + ac_kp(K)) * ac_ld(K) * sizeof(double) + 4 * kTile * sizeof(int);
}
__host__ __device__ constexpr size_t ac_tile_lds(int K) {  // Ys, Zs; the finished tile on top
  const size_t ops = (size_t)2 * kTile * ac_ld(K), fin = (size_t)kTile * kCld;
  return (ops > fin ? ops : fin) * sizeof(double);
}

// acc[t] += A[16 rows][KP] B[KP][16 t .. 16 t + 15]: ap -> A[r16][k4] (row stride in the
// pointer), bp -> B's entry (k = k4, column r16) with k stride bk and column-tile stride bt.
template <int CT>
__device__ __forceinline__ void ac_chain(const double* __restrict__ ap,
                                         const double* __restrict__ bp, int bk, int bt, int KP,
                                         f64x4 (&acc)[4]) {
#pragma unroll 2
  for (int k0 = 0; k0 < KP; k0 += 4) {
    const double a = ap[k0];
    double b[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) b[t] = bp[k0 * bk + t * bt];
#pragma unroll
    for (int t = 0; t < CT; ++t)
      acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[t], acc[t], 0, 0, 0);
  }
}

// ------------------------------------------------------------------------------------- rows
template <typename T>
__global__ __launch_bounds__(kThreads) void asset_cov_rows_kernel(
    const T* __restrict__ X, const T* __restrict__ cap, const T* __restrict__ ret,
    const int16_t* __restrict__ ind, const double* __restrict__ stats,
    const double* __restrict__ F, const double* __restrict__ sv, long long s_dstride,
    const int* __restrict__ index, long long i_dstride, const uint8_t* __restrict__ universe,
    int d0, int N, int P, int Q, int M, double* __restrict__ Zg, double* __restrict__ Yg,
    double* __restrict__ s2g, int* __restrict__ nidg, double* __restrict__ vol,
    uint8_t* __restrict__ valid) {
  extern __shared__ double ac_lds[];
  const int dl = blockIdx.y, d = d0 + dl, m0 = blockIdx.x * kTile;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r16 = lane & 15, k4 = lane >> 4;
  const int K = 1 + P + Q, KP = ac_kp(K), ld = ac_ld(K), CT = KP >> 4;
  double* Zs = ac_lds;              // [64][ld] design rows
  double* Ys = Zs + kTile * ld;     // [64][ld] Z F
  double* Fs = Ys + kTile * ld;     // [KP][ld] F_d, zero padded
  int* okw = (int*)(Fs + KP * ld);  // [4 waves][64]: each wave's clauses of the validity rule
  const DesignDate<T> day(X, cap, ret, ind, d, N, P, Q);
  const double* st = stats + (size_t)d * (Q + 2);

  // F_d -> LDS
  int bad = 0;
  {
    const double* Fd = F + (size_t)d * K * K;
    for (int e = tid; e < KP * KP; e += kThreads) {
      const int i = e / KP, k = e - i * KP;
      double v = 0.0;
      if (i < K && k < K) {
        v = Fd[i * K + k];
        bad |= !__builtin_isfinite(v);
      }
      Fs[i * ld + k] = v;
    }
  }

  // member = lane; wave w takes the columns c = w mod 4 of the row and their clauses
  const int i = m0 + lane;
  const int n = i < M ? index[(size_t)d * (size_t)i_dstride + i] : -1;
  const bool in = n >= 0 && n < N;
  const int nn = in ? n : 0;
  const int j = day.industry(nn);
  bool ok = in;
  double s = 0.0;
  if (wid == 0) {
    T c, r;
    int jj;
    day.load_base(nn, c, r, jj);
    s = sv[(size_t)d * (size_t)s_dstride + nn];
    ok = ok && __builtin_isfinite(s) && (s > 0.0) && (!universe || universe[(size_t)d * N + nn]) &&
         day.base_ok(c, r, jj);
    Zs[lane * ld] = 1.0;
  }
  const double isig_den = st[Q];
  for (int q = wid; q < Q; q += kWaves) {
    const T x = day.X[(size_t)q * N + nn];
    ok = ok && __builtin_isfinite(x);
    Zs[lane * ld + 1 + P + q] = ((double)x - st[q]) / isig_den;
  }
  for (int p = wid; p < P; p += kWaves) Zs[lane * ld + 1 + p] = p == j ? 1.0 : 0.0;
  for (int k = K + wid; k < KP; k += kWaves) Zs[lane * ld + k] = 0.0;
  okw[wid * kTile + lane] = ok;
  bad = __syncthreads_or(bad) | !stats_finite(st, Q);
  ok = !bad && okw[lane] && okw[kTile + lane] && okw[2 * kTile + lane] && okw[3 * kTile + lane];
  if (!ok)  // a member that is not valid carries a zero row: nothing non-finite enters the MFMA
    for (int k = wid; k < KP; k += kWaves) Zs[lane * ld + k] = 0.0;
  __syncthreads();

  // Y = Z F: wave w owns rows 16 w .. 16 w + 15
  if (!bad) {
    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double* ap = Zs + (16 * wid + r16) * ld + k4;
    const double* bp = Fs + k4 * ld + r16;
    switch (CT) {  // wave-uniform
      case 1: ac_chain<1>(ap, bp, ld, 16, KP, acc); break;
      case 2: ac_chain<2>(ap, bp, ld, 16, KP, acc); break;
      case 3: ac_chain<3>(ap, bp, ld, 16, KP, acc); break;
      default: ac_chain<4>(ap, bp, ld, 16, KP, acc); break;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < CT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) Ys[(16 * wid + k4 + 4 * e) * ld + 16 * t + r16] = acc[t][e];
      }
  } else {
    for (int e = tid; e < kTile * KP; e += kThreads) Ys[(e / KP) * ld + e % KP] = 0.0;
  }
  __syncthreads();

  // per member: x F x in k order, vol, valid, the stock id the tiles compare
  if (wid == 0 && i < M) {
    double var = 0.0;
    for (int k = 0; k < K; ++k) var = fma(Ys[lane * ld + k], Zs[lane * ld + k], var);
    const double s2 = s * s;
    const size_t o = (size_t)d * M + i, ol = (size_t)dl * M + i;
    vol[o] = ok ? sqrt(var + s2) : qnan();
    valid[o] = ok;
    s2g[ol] = ok ? s2 : 0.0;
    nidg[ol] = ok ? n : -1;
  }
  // Z, Y -> scratch [dl][M][KP], whole rows
  const int rows = min(kTile, M - m0);
  const size_t base = ((size_t)dl * M + m0) * KP;
  for (int e = tid; e < rows * KP; e += kThreads) {
    const int r = e / KP, k = e - r * KP;
    Zg[base + e] = Zs[r * ld + k];
    Yg[base + e] = Ys[r * ld + k];
  }
}

// ------------------------------------------------------------------------------------- tile
template <bool CORR>
__global__ __launch_bounds__(kThreads) void asset_cov_tile_kernel(
    const double* __restrict__ Zg, const double* __restrict__ Yg, const double* __restrict__ s2g,
    const int* __restrict__ nidg, const double* __restrict__ vol, int d0, int M, int K,
    double* __restrict__ cov) {
  extern __shared__ double ac_lds[];
  const int dl = blockIdx.y, d = d0 + dl;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r16 = lane & 15, k4 = lane >> 4;
  const int KP = ac_kp(K), ld = ac_ld(K);
  // tile (ti, tj), ti >= tj, from the linear index t = ti (ti + 1) / 2 + tj
  const long long t = blockIdx.x;
  long long tl = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((tl + 1) * (tl + 2) / 2 <= t) ++tl;
  while (tl * (tl + 1) / 2 > t) --tl;
  const int ti = (int)tl, tj = (int)(t - tl * (tl + 1) / 2);
  const int i0 = ti * kTile, j0 = tj * kTile;
  const int ni = min(kTile, M - i0), nj = min(kTile, M - j0);
  const bool diag = ti == tj;

  double* Ys = ac_lds;           // [64][ld] rows i0 .. of Y
  double* Zs = Ys + kTile * ld;  // [64][ld] rows j0 .. of Z
  double* Cs = ac_lds;           // [64][kCld] the finished tile, once the operands are used up
  {
    const double* Yt = Yg + ((size_t)dl * M + i0) * KP;
    const double* Zt = Zg + ((size_t)dl * M + j0) * KP;
    for (int e = tid; e < kTile * KP; e += kThreads) {
      const int r = e / KP, k = e - r * KP;
      Ys[r * ld + k] = r < ni ? Yt[e] : 0.0;
      Zs[r * ld + k] = r < nj ? Zt[e] : 0.0;
    }
  }
  __syncthreads();

  f64x4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = f64x4{0.0, 0.0, 0.0, 0.0};
  {
    // A[i][k] = Y[i0 + 16 w + i][k], B[k][j] = Z[j0 + 16 u + j][k]
    const double* ap = Ys + (16 * wid + r16) * ld + k4;
    const double* bp = Zs + r16 * ld + k4;
    ac_chain<4>(ap, bp, 1, 16 * ld, KP, acc);
  }
  __syncthreads();  // every wave is done with the operands: Cs may overwrite them

  // epilogue on register e of column tile u: row li = 16 w + k4 + 4 e, column lj = 16 u + r16
  const size_t row0 = (size_t)dl * M, orow0 = (size_t)d * M;
  int idj[4];
  double vj[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int lj = 16 * u + r16;
    idj[u] = lj < nj ? nidg[row0 + j0 + lj] : -1;
    vj[u] = (CORR && lj < nj) ? vol[orow0 + j0 + lj] : 1.0;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int li = 16 * wid + k4 + 4 * e;
    const bool rin = li < ni;
    const int idi = rin ? nidg[row0 + i0 + li] : -1;
    const double s2 = rin ? s2g[row0 + i0 + li] : 0.0;
    const double vi = (CORR && rin) ? vol[orow0 + i0 + li] : 1.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int lj = 16 * u + r16;
      if (diag && lj > li) continue;  // the upper triangle of a diagonal tile is the mirror
      double v = acc[u][e];
      if (idi == idj[u]) v += s2;
      if (CORR) v = (diag && li == lj) ? 1.0 : v / (vi * vj[u]);
      if (idi < 0 || idj[u] < 0) v = qnan();
      Cs[li * kCld + lj] = v;
      if (diag && lj < li) Cs[lj * kCld + li] = v;
    }
  }
  __syncthreads();

  // the tile, whole rows: wave w stores rows w, w + 4, ...
  double* out = cov + (size_t)d * M * M;
  for (int r = wid; r < ni; r += kWaves)
    if (lane < nj) out[(size_t)(i0 + r) * M + j0 + lane] = Cs[r * kCld + lane];
  // ... and its mirror, whole rows too: row c of the mirror is column c of the tile
  if (!diag)
    for (int c = wid; c < nj; c += kWaves)
      if (lane < ni) out[(size_t)(j0 + c) * M + i0 + lane] = Cs[lane * kCld + c];
}

template <typename T>
int asset_cov_dispatch(const T* X, const T* cap, const T* ret, const int16_t* ind,
                       const double* stats, const double* F, const double* sv,
                       long long s_dstride, const int* index, long long i_dstride,
                       const uint8_t* universe, int d0, int nd, int N, int P, int Q, int M,
                       int correlation, double* Zg, double* Yg, double* s2g, int* nidg,
                       double* cov, double* vol, uint8_t* valid, void* stream) {
  if (nd <= 0 || M <= 0) return 0;
  const int K = 1 + P + Q, MT = (M + kTile - 1) / kTile;
  const long long tiles = (long long)MT * (MT + 1) / 2;
  if (Q < 1 || Q > kMaxQ || P < 0 || K > kMaxK || N <= 0 || d0 < 0 || nd > 65535 ||
      tiles > 0x7fffffffLL || (s_dstride != 0 && s_dstride != N) ||
      (i_dstride != 0 && i_dstride != M))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds_r = ac_rows_lds(K), lds_t = ac_tile_lds(K);
  if (hipError_t err = raise_dynamic_lds<asset_cov_rows_kernel<T>>(lds_r)) return (int)err;
  hipLaunchKernelGGL((asset_cov_rows_kernel<T>), dim3(MT, nd), dim3(kThreads), lds_r, s, X, cap,
                     ret, P > 0 ? ind : nullptr, stats, F, sv, s_dstride, index, i_dstride,
                     universe, d0, N, P, Q, M, Zg, Yg, s2g, nidg, vol, valid);
  if (hipError_t err = hipGetLastError()) return (int)err;
  if (correlation) {
    if (hipError_t err = raise_dynamic_lds<asset_cov_tile_kernel<true>>(lds_t)) return (int)err;
    hipLaunchKernelGGL((asset_cov_tile_kernel<true>), dim3((unsigned)tiles, nd), dim3(kThreads),
                       lds_t, s, Zg, Yg, s2g, nidg, vol, d0, M, K, cov);
  } else {
    if (hipError_t err = raise_dynamic_lds<asset_cov_tile_kernel<false>>(lds_t)) return (int)err;
    hipLaunchKernelGGL((asset_cov_tile_kernel<false>), dim3((unsigned)tiles, nd), dim3(kThreads),
                       lds_t, s, Zg, Yg, s2g, nidg, vol, d0, M, K, cov);
  }
  return (int)hipGetLastError();
}

}  // namespace

// Bytes of scratch one date of an M-member basket needs (Z, Y [M][KP] f64, s^2 [M] f64, stock id
// [M] int32, in that order, each for all the chunk's dates).
MFA_API size_t mfa_asset_cov_date_bytes(int M, int K) {
  return (size_t)M * (2 * (size_t)ac_kp(K) * sizeof(double) + sizeof(double) + sizeof(int));
}

// Dates [d0, d0 + nd) of the call.  X [D][Q][N], cap / ret [D][N] f32, ind [D][N] int16 (nullable
// when P == 0), stats [D][Q+2] f64 from mfa_xs_wls, F [D][K][K] f64, sv f64 specific
// volatilities ([N], s_dstride = 0, or [D][N], s_dstride = N), index int32 stock positions in
// [-1, N) ([M], i_dstride = 0, or [D][M], i_dstride = M; -1 = padding), universe [D][N] bytes
// (nullable).  Scratch for nd dates: Zg / Yg [nd][M][KP] f64, s2g [nd][M] f64, nidg [nd][M]
// int32.  Outputs cov [D][M][M] f64 (the correlation when `correlation`), vol [D][M] f64,
// valid [D][M] bytes.  K = 1 + P + Q <= 64, Q <= 16, nd <= 65535.  Bitwise reproducible.
MFA_API int mfa_asset_cov(const float* X, const float* cap, const float* ret, const int16_t* ind,
                          const double* stats, const double* F, const double* sv,
                          long long s_dstride, const int* index, long long i_dstride,
                          const uint8_t* universe, int d0, int nd, int N, int P, int Q, int M,
                          int correlation, double* Zg, double* Yg, double* s2g, int* nidg,
                          double* cov, double* vol, uint8_t* valid, void* stream) {
  return asset_cov_dispatch<float>(X, cap, ret, ind, stats, F, sv, s_dstride, index, i_dstride,
                                   universe, d0, nd, N, P, Q, M, correlation, Zg, Yg, s2g, nidg,
                                   cov, vol, valid, stream);
}

// Same with an fp64 panel.
MFA_API int mfa_asset_cov_f64(const double* X, const double* cap, const double* ret,
                              const int16_t* ind, const double* stats, const double* F,
                              const double* sv, long long s_dstride, const int* index,
                              long long i_dstride, const uint8_t* universe, int d0, int nd, int N,
                              int P, int Q, int M, int correlation, double* Zg, double* Yg,
                              double* s2g, int* nidg, double* cov, double* vol, uint8_t* valid,
                              void* stream) {
  return asset_cov_dispatch<double>(X, cap, ret, ind, stats, F, sv, s_dstride, index, i_dstride,
                                    universe, d0, nd, N, P, Q, M, correlation, Zg, Yg, s2g, nidg,
                                    cov, vol, valid, stream);
}
