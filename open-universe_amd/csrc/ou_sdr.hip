// BSS-eval SDR with a distortion filter of L taps over ragged rows: ou_sdr of include/ouniverse.h ("scoring").  With s_l =
// ref delayed by l samples (l = 0 .. L - 1, every signal zero-extended to T + L - 1) and P the orthogonal projection onto
// span{s_l}:  c = ||P est||^2 / ||est||^2,  out = 10 log10(c / (1 - c)), clamped as ou_si_sdr clamps.  Two kernels on the
// caller's stream, no atomics, every sum in one fixed order (the conventions of ou_metrics.hip):
//
//   sdr_corr_kernel    one workgroup = one row x kSdrTile consecutive samples t of ref.  It forms, in double,
//                        r[l] = sum_t ref[t] ref[t + l]   and   x[l] = sum_t ref[t] est[t + l]     over ITS t, l = 0 .. L - 1
//                      and writes them to partial[row][tile][2][L].  Both signals are staged in LDS as the caller's fp32, est
//                      and ref with the halo behind the tile that the lags reach; zeros stand in for what lies behind the row's
//                      own length, so no zero-extended copy of a signal exists anywhere.
//   sdr_solve_kernel   one wave per row: the row's tile partials summed in ascending tile order, R h = x (R = toeplitz(r)) by
//                      the Levinson recursion in double, c = (2 x.h - h.R h) / sum est^2, the clamped score.
//
// The correlation runs on v_mfma_f64_16x16x4_f64: a product of two fp32 values is exact in double, so the only roundings
// are those of the accumulation, and its order is fixed by the tile plan:
//   D[p][n] += sum_k A[p][k] B[k][n],  A[p][k] = s[t0 + k + p + 256 j],  B[k][n] = ref[t0 + k - 16 n]
// so D[p][n] collects lag p + 16 n + 256 j of signal s (ref or est): 256 lags per accumulator tile, j = 0, 1 for L > 256.
// Column n sees the tile's samples t = t0 .. t0 + kSdrTile - 1 at k = 16 n .. 16 n + kSdrTile - 1; B is read from a copy of
// the tile with 240 zeros on either side, so k runs over kSdrTile + 240 values for all columns at once (a tenth of the k-steps
// multiply zeros; kSdrTile + 240 is a multiple of 64: four waves x groups of four k-steps).  Operand maps (16x16x4, one
// double per lane): lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; C/D register q of lane l is
// D[(l >> 4) + 4 q][l & 15] (the f64 map, as in met_stft_kernel).
// The four waves split the k range into four consecutive quarters; their accumulators meet in LDS (over the staged
// signals, which are dead by then) and are added in wave order.
// LDS banks: lane l reads A at dword k + (l & 15) + const -- 19 consecutive dwords per wave, equal addresses broadcast -- and
// B at logical index j = k - 16 (l & 15) + 240.  Sixteen columns 16 dwords apart would share two banks of the 32 that
// ds_read_b32 spreads a half-wave over, so B is stored skewed, phys(j) = j + 2 (j >> 4): column n then sits 18 n dwords
// below column 0, and 18 n mod 32 takes 16 different even values, the second k of the half-wave the odd ones.
#include "ou_internal.h"

namespace ou {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kCorrThreads = 256;
constexpr int kTile = kSdrTile;                    // samples of ref a workgroup owns
constexpr int kSpan = kTile + 240;                 // values of k: every column's 16 n .. 16 n + kTile - 1
constexpr int kStepsPerWave = kSpan / 16;          // k-steps of 4, a quarter of them per wave
constexpr int kSigWords = kSpan + 15 + 256 + 1;    // s[t0 + k + p + 256 j]: k < kSpan, p < 16, j < 2
constexpr int kRefLogical = kSpan + 240;           // B's logical index k - 16 n + 240
constexpr int kRefWords = kRefLogical + 2 * ((kRefLogical - 1) >> 4) + 2;
constexpr int kStageWords = kRefWords + 2 * kSigWords;
constexpr int kAccWords = 4 * 4 * 256 * 2;         // 4 waves x 4 accumulator tiles x 256 lags, doubles counted as float pairs
constexpr int kLdsWords = kStageWords > kAccWords ? kStageWords : kAccWords;
static_assert(kSpan % 64 == 0, "the k range splits into four quarters, each a whole number of groups of four k-steps");
static_assert(kLdsWords * 4 <= 64 * 1024, "static LDS");

__device__ inline int skew(int j) { return j + ((j >> 4) << 1); }

// grid (tiles of the longest row of the launch, rows of the launch); partial[((row0 + b) * tile_stride + tile) * 2 L ..]:
// L values of r, then L values of x.  kLagTiles = 1 for L <= 256, else 2.
template <int kLagTiles>
__global__ __launch_bounds__(kCorrThreads) void sdr_corr_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                                long long stride, MetRows rows, int row0, int L,
                                                                double* __restrict__ partial, long long tile_stride) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsWords];
  float* sB = lds;                  // the tile of ref between two runs of 240 zeros, skewed
  float* sRef = lds + kRefWords;    // ref[t0 ..] with its halo
  float* sEst = sRef + kSigWords;   // est[t0 ..] with its halo
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const long long len = rows.len[b];
  const long long t0 = (long long)blockIdx.x * kTile;
  if (t0 >= len) return;  // (uniform) this row has no such tile: its partial is never read
  const float* x = est + (size_t)(row0 + b) * (size_t)stride;
  const float* y = ref + (size_t)(row0 + b) * (size_t)stride;

  for (int j = tid; j < kSigWords; j += kCorrThreads) {
    const long long t = t0 + j;
    const bool in = t < len;
    sRef[j] = in ? y[t] : 0.0f;
    sEst[j] = in ? x[t] : 0.0f;
  }
  for (int j = tid; j < kRefLogical; j += kCorrThreads) {
    const int i = j - 240;
    sB[skew(j)] = (i >= 0 && i < kTile && t0 + i < len) ? y[t0 + i] : 0.0f;
  }
  __syncthreads();

  f64x4 acc[kLagTiles][2];
#pragma unroll
  for (int j = 0; j < kLagTiles; j++) acc[j][0] = acc[j][1] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int pn = lane & 15, kk = lane >> 4;
  const int k4_0 = wave * kStepsPerWave;
#pragma unroll 1
  for (int s = 0; s < kStepsPerWave; s += 4) {  // k ascending; four k-steps of operands in flight ahead of their MFMAs
    double bv[4], ar[4][kLagTiles], ae[4][kLagTiles];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = 4 * (k4_0 + s + u) + kk;
      bv[u] = (double)sB[skew(k - 16 * pn + 240)];
#pragma unroll
      for (int j = 0; j < kLagTiles; j++) {
        ar[u][j] = (double)sRef[k + pn + 256 * j];
        ae[u][j] = (double)sEst[k + pn + 256 * j];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int j = 0; j < kLagTiles; j++) {
        acc[j][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[u][j], bv[u], acc[j][0], 0, 0, 0);
        acc[j][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ae[u][j], bv[u], acc[j][1], 0, 0, 0);
      }
  }
  __syncthreads();  // the staged signals are dead: the accumulators of the four waves take their place

  double* sAcc = reinterpret_cast<double*>(lds);  // [wave][signal][256 kLagTiles lags]
#pragma unroll
  for (int j = 0; j < kLagTiles; j++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int lag = 256 * j + 16 * pn + kk + 4 * q;  // D[(lane >> 4) + 4 q][lane & 15]: lag = row + 16 col
      sAcc[(wave * 2 + 0) * (256 * kLagTiles) + lag] = acc[j][0][q];
      sAcc[(wave * 2 + 1) * (256 * kLagTiles) + lag] = acc[j][1][q];
    }
  __syncthreads();
  double* p = partial + ((size_t)(row0 + b) * (size_t)tile_stride + blockIdx.x) * (size_t)(2 * L);
  for (int i = tid; i < 2 * 256 * kLagTiles; i += kCorrThreads) {
    const int sig = i / (256 * kLagTiles), lag = i - sig * (256 * kLagTiles);
    if (lag < L) {
      double v = 0.0;
      for (int w = 0; w < kCorrThreads / 64; w++) v += sAcc[(w * 2 + sig) * (256 * kLagTiles) + lag];  // waves ascending
      p[sig * L + lag] = v;
    }
  }
}

// fixed-order sum over the one wave of the solver, the result in every lane
__device__ inline double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

// 10 log10(c / (1 - c)) with c clamped to [e, 1 - e] (the rule of ou_si_sdr, ou_metrics.hip)
__device__ inline float clamped_db(double coh, double e) {
  coh = coh < e ? e : (coh > 1.0 - e ? 1.0 - e : coh);
  return (float)(10.0 * log10(coh / (1.0 - coh)));
}

// grid (rows of the launch), one wave.  tsum: the 8 doubles per row of met_time_kernel (word 1: sum est^2).
//
// Levinson recursion on R h = x, R = toeplitz(r): with a the order-m prediction polynomial (a[0] = 1) and E its error,
//     k = -(sum_{i < m} a[i] r[m - i]) / E,   a'[i] = a[i] + k a[m - i],   E' = E (1 - k^2),
//     q = (x[m] - sum_{i < m} h[i] r[m - i]) / E',   h[i] += q a'[m - i]                        (i = 0 .. m)
// one pass over the m live entries for both sums, one for the two updates: O(L) words of LDS and L steps.  R is positive
// definite for every non-zero ref, so E stays positive; should rounding ever take it to zero the recursion stops at the order
// reached (h of that order is still a point of the span).
// The score is taken as c = (2 x.h - h.R h) / sum est^2, not as x.h / sum est^2: the two agree at the exact h, and the first
// is stationary there -- an error d in h moves it by d.R d, the square of what it moves x.h by -- so what the recursion loses
// at cond(R) = 1e8 (it is weakly stable only) does not reach the score.  h.R h is one Toeplitz product from r in LDS.
__global__ __launch_bounds__(64) void sdr_solve_kernel(MetRows rows, int row0, const double* __restrict__ partial,
                                                       long long tile_stride, const double* __restrict__ tsum, int L,
                                                       float clamp_db, float* __restrict__ out) {
  __shared__ double sr[kSdrMaxFilter], sx[kSdrMaxFilter], sh[kSdrMaxFilter], sa[2][kSdrMaxFilter];
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long nt = (rows.len[b] + kTile - 1) / kTile;  // = sdr_tiles(len)
  const double* p = partial + (size_t)(row0 + b) * (size_t)tile_stride * (size_t)(2 * L);
  for (int i = lane; i < 2 * L; i += 64) {
    double s = 0.0;
    for (long long t = 0; t < nt; t++) s += p[(size_t)t * (size_t)(2 * L) + i];  // tiles ascending
    if (i < L) sr[i] = s; else sx[i - L] = s;
  }
  for (int i = lane; i < L; i += 64) sh[i] = 0.0;
  __syncthreads();
  const double see = tsum[(size_t)(row0 + b) * 8 + 1], r0 = sr[0];
  double c = 0.0;
  if (r0 > 0.0 && see > 0.0) {  // (uniform)
    if (lane == 0) {
      sa[0][0] = 1.0;
      sh[0] = sx[0] / r0;
    }
    __syncthreads();
    double E = r0;
    int cur = 0;
    for (int m = 1; m < L; m++) {
      const double* a = sa[cur];
      double* an = sa[cur ^ 1];
      double s1 = 0.0, s2 = 0.0;
      for (int i = lane; i < m; i += 64) {
        const double rv = sr[m - i];
        s1 += a[i] * rv;
        s2 += sh[i] * rv;
      }
      s1 = wave_sum(s1);
      s2 = wave_sum(s2);
      const double k = -s1 / E, En = E * (1.0 - k * k);
      if (!(En > 0.0)) break;  // (uniform)
      const double q = (sx[m] - s2) / En;
      for (int i = lane; i <= m; i += 64) an[i] = (i < m ? a[i] : 0.0) + k * (i > 0 ? a[m - i] : 0.0);
      __syncthreads();  // a' is whole before h reads it mirrored; a (read above) is next written a step from now
      for (int i = lane; i <= m; i += 64) sh[i] += q * an[m - i];
      E = En;
      cur ^= 1;
    }
    __syncthreads();
    double num = 0.0;
    for (int i = lane; i < L; i += 64) {
      double g = 0.0;
      for (int j = 0; j < L; j++) g += sr[i > j ? i - j : j - i] * sh[j];
      num += sh[i] * (2.0 * sx[i] - g);
    }
    c = wave_sum(num) / see;
  }
  if (lane == 0) {
    const double pw = pow(10.0, -(double)clamp_db / 10.0);
    out[row0 + b] = clamped_db(c, pw / (1.0 + pw));
  }
}

}  // namespace

hipError_t launch_sdr_corr(const float* est, const float* ref, long long stride, const MetRows& rows, int n_rows, int row0,
                           long long len_max, int L, double* partial, long long tile_stride, hipStream_t st) {
  const dim3 grid((unsigned)sdr_tiles(len_max), (unsigned)n_rows), block(kCorrThreads);
  if (L <= 256)
    sdr_corr_kernel<1><<<grid, block, 0, st>>>(est, ref, stride, rows, row0, L, partial, tile_stride);
  else
    sdr_corr_kernel<2><<<grid, block, 0, st>>>(est, ref, stride, rows, row0, L, partial, tile_stride);
  return hipGetLastError();
}

hipError_t launch_sdr_solve(const MetRows& rows, int n_rows, int row0, const double* partial, long long tile_stride,
                            const double* tsum, int L, float clamp_db, float* out, hipStream_t st) {
  sdr_solve_kernel<<<dim3(n_rows), dim3(64), 0, st>>>(rows, row0, partial, tile_stride, tsum, L, clamp_db, out);
  return hipGetLastError();
}

}  // namespace ou
