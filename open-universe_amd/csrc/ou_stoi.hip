// STOI and extended STOI over ragged rows: ou_stoi of include/ouniverse.h ("scoring"; the definition is there and in DESIGN
// 4.22).  The caller's fp32 samples are widened on load; everything behind them -- filter table, resampled signals, frame
// energies, the overlap-added signals, spectra, band values, segment sums -- is double, up to the one fp32 store of the score.
// All on the caller's stream, no atomics, every sum in one fixed order (the conventions of ou_metrics.hip and ou_sdr.hip); a
// row's arithmetic depends on nothing but the row, so a row in a batch is bit for bit its own B = 1 call.
//
//   stoi_resample_kernel  est and ref to 10 kHz: output j = f p + ph is sum_t coef[t][ph] x[f q + first[ph] + t], taps ascending,
//                         zeros outside [0, len) (the polyphase scheme of ou_resample.hip with a double table and accumulator).
//                         Not launched at fs = 10 kHz: the later kernels then read the caller's rows.
//   stoi_basis_kernel     the cos / -sin basis of the 512-point DFT for bins 7 .. 220 and k < 256 (the upper half of the
//                         zero-padded frame is zero), in the order the MFMA B operand is read; the window hanning(258)[1:-1].
//   stoi_energy_kernel    one wave per frame of ref: 20 log10(||w ref_f|| + eps).
//   stoi_mask_kernel      one workgroup per row: the row's maximum, the keep mask E_f > max - 40, and its exclusive scan in
//                         chunks of 1024 frames with a running base -- src[k] = the k-th kept frame, count = how many.
//   stoi_stft_kernel      one workgroup = one row x kStoiFrameTile STFT frames of BOTH compacted signals.  The compacted
//                         signals are never stored: the 17 hops the tile spans are gathered into LDS, each sample the sum of at
//                         most two windowed kept frames in ascending frame order (DESIGN 4.22 says why not materialised).  The
//                         DFT is a (16 x 256) x (256 x 16 bins) GEMM per bin tile on v_mfma_f64_16x16x4_f64; |X|^2 is formed
//                         from the accumulators and summed into the fifteen bands in registers, bins ascending.
//   stoi_seg_kernel       kStoiSegTile sliding windows of 30 frames per workgroup -> one partial in double.
//   stoi_final_kernel     one thread per row: partials in ascending order, the 30-frame cut, the fp32 score.
//
// Tile plan of stoi_stft_kernel (256 threads = 4 waves): wave w owns signal w & 1 and bin half w >> 1.  The band edges are
// contiguous (7, 9, 11, .. 219), and 109 is one of them, so half 0 walks seven 16-bin tiles from bin 7 (bands 0 .. 11, bins
// 7 .. 108) and half 1 seven from bin 109 (bands 12 .. 14, bins 109 .. 218): every band is summed by ONE wave, in ascending bin
// order, with a running accumulator that crosses tile borders; bins behind a half's last edge are computed and dropped.
//   A operand: lane l holds A[l & 15][l >> 4] = z[128 (l & 15) + k] w[k], k = 4 k4 + (l >> 4), z the gathered signal in LDS
//     (doubles).  Frames lie 128 doubles apart, which is one bank for all sixteen; z is stored skewed, phys(s) = s + 4 (s >> 7),
//     so the sixteen frames of a k-step start 132 doubles = 8 dwords (mod 64 banks) apart and a ds_read_b64 of the wave takes
//     the two passes its 512 bytes need.
//   B operand (global, L2-resident: 917 KB): basis[2 tt + c][k4][l] = cos / -sin(2 pi k bin / 512), bin = base(tt) + (l & 15).
//   C/D: register r of lane l is frame (l >> 4) + 4 r, bin base + (l & 15) (the f64 map, as in met_stft_kernel).  The band walk
//     broadcasts bin c of every frame group with __shfl from lane (l & 48) | c.
// Static LDS: 2 x 2244 + 256 doubles = 37 952 bytes.
#include "ou_internal.h"

namespace ou {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr double kEps = 2.220446049250313e-16;  // 2^-52
constexpr int kThreads = 256;
constexpr int kMaskThreads = 1024;
constexpr int kK4 = kStoiFrame / 4;                                   // k-steps of the DFT
constexpr int kSpan = (kStoiFrameTile + 1) * kStoiHop;                // samples of a compacted signal one STFT tile spans
constexpr int kZWords = kSpan + 4 * (kStoiFrameTile + 1);             // ... skewed
__constant__ int kEdges[kStoiBands + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
constexpr int kHalfBand = 12, kHalfBin = 109;                         // kEdges[kHalfBand] == kHalfBin
static_assert(kStoiFrame == 2 * kStoiHop && kStoiFrameTile == 16, "the tile plan above");

__device__ inline int tile_bin0(int tt) { return tt < kStoiBinTiles / 2 ? 7 + 16 * tt : kHalfBin + 16 * (tt - kStoiBinTiles / 2); }

// sample i of signal `ref ? ref : est` of row r at 10 kHz
__device__ inline double sample(const StoiSignals& s, int ref, int r, long long i) {
  if (s.res_est) return (ref ? s.res_ref : s.res_est)[(size_t)r * (size_t)s.res_stride + i];
  return (double)(ref ? s.ref : s.est)[(size_t)r * (size_t)s.stride + i];
}

// fixed-order sum over the workgroup: lanes by shuffle, waves ascending; every thread calls it, the result is in every thread
__device__ inline double block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < nw; i++) s += red[i];
  return s;
}

// grid (ceil(longest n10 / 256), rows of the launch)
__global__ __launch_bounds__(kThreads) void stoi_resample_kernel(StoiSignals sig, StoiRows rows, int row0, int p, int q, int taps,
                                                                 const int* __restrict__ first, const double* __restrict__ coef,
                                                                 double* __restrict__ res_est, double* __restrict__ res_ref) {
  const int b = blockIdx.y, r = row0 + b;
  const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long len = rows.len[b];
  if (j >= rows.n10[b]) return;
  const long long f = j / p;
  const int ph = (int)(j - f * p);
  const long long start = f * q + first[ph];
  const float* x = sig.est + (size_t)r * (size_t)sig.stride;
  const float* y = sig.ref + (size_t)r * (size_t)sig.stride;
  const double* cp = coef + ph;
  double ax = 0.0, ay = 0.0;
  for (int t = 0; t < taps; t++, cp += p) {  // taps ascending, one multiply and one add each
    const long long i = start + t;
    if (i >= 0 && i < len) {
      const double c = *cp;
      ax += c * (double)x[i];
      ay += c * (double)y[i];
    }
  }
  res_est[(size_t)r * (size_t)sig.res_stride + j] = ax;
  res_ref[(size_t)r * (size_t)sig.res_stride + j] = ay;
}

// one thread per word of basis (kStoiBasisWords) and of window (kStoiFrame)
__global__ void stoi_basis_kernel(double* __restrict__ basis, double* __restrict__ window) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (long long)kStoiBasisWords) {
    const int l = (int)(e & 63);
    const int q = (int)(e >> 6);
    const int k4 = q % kK4, tc = q / kK4;
    const int k = 4 * k4 + (l >> 4), bin = tile_bin0(tc >> 1) + (l & 15);
    const int m = (k * bin) & 511;  // the angle, reduced exactly
    const double ang = 2.0 * M_PI * (double)m / 512.0;
    basis[e] = (tc & 1) ? -sin(ang) : cos(ang);
  } else if (e < (long long)kStoiBasisWords + kStoiFrame) {
    const int k = (int)(e - (long long)kStoiBasisWords);
    window[k] = 0.5 - 0.5 * cos(2.0 * M_PI * (double)(k + 1) / 257.0);  // hanning(258)[1:-1]
  }
}

// grid (ceil(frames of the longest row / 16), rows of the launch): wave w takes frames f0 + 4 w .. f0 + 4 w + 3
__global__ __launch_bounds__(kThreads) void stoi_energy_kernel(StoiSignals sig, StoiRows rows, int row0,
                                                               const double* __restrict__ window, double* __restrict__ energy,
                                                               long long F) {
  const int b = blockIdx.y, r = row0 + b, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long nf = stoi_frames(rows.n10[b]);
  for (int i = 0; i < 4; i++) {
    const long long f = (long long)blockIdx.x * 16 + wave * 4 + i;
    if (f >= nf) return;  // (uniform over the wave; no barrier below)
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = lane + 64 * u;
      const double v = window[k] * sample(sig, 1, r, f * kStoiHop + k);  // f * 128 + 255 < n10: stoi_frames
      s += v * v;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) energy[(size_t)r * (size_t)F + f] = 20.0 * log10(sqrt(s) + kEps);
  }
}

// grid (rows of the launch), 1024 threads
__global__ __launch_bounds__(kMaskThreads) void stoi_mask_kernel(StoiRows rows, int row0, const double* __restrict__ energy,
                                                                 long long F, int* __restrict__ src, int* __restrict__ count) {
  __shared__ double smax[kMaskThreads / 64];
  __shared__ int scnt[kMaskThreads / 64];
  const int b = blockIdx.x, r = row0 + b, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long nf = stoi_frames(rows.n10[b]);
  const double* E = energy + (size_t)r * (size_t)F;
  int* out = src + (size_t)r * (size_t)F;
  double mx = -INFINITY;
  for (long long f = tid; f < nf; f += kMaskThreads) mx = fmax(mx, E[f]);
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
  if (lane == 0) smax[wave] = mx;
  __syncthreads();
  for (int w = 0; w < kMaskThreads / 64; w++) mx = fmax(mx, smax[w]);
  const double threshold = mx - 40.0;
  int base = 0;
  for (long long c0 = 0; c0 < nf; c0 += kMaskThreads) {  // (uniform)
    const long long f = c0 + tid;
    const bool keep = f < nf && E[f] > threshold;
    const unsigned long long vote = __ballot(keep);
    if (lane == 0) scnt[wave] = __popcll(vote);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kMaskThreads / 64; w++) {
      before += w < wave ? scnt[w] : 0;
      total += scnt[w];
    }
    if (keep) out[base + before + __popcll(vote & ((1ull << lane) - 1ull))] = (int)f;  // rank < kept frames <= nf <= F
    base += total;
    __syncthreads();  // scnt is rewritten by the next chunk
  }
  if (tid == 0) count[r] = base;
}

// grid (ceil(STFT frames of the longest row / 16), rows of the launch); bands[((r * 2 + signal) * 15 + band) * F + frame],
// signal 0 = est, 1 = ref
__global__ __launch_bounds__(kThreads) void stoi_stft_kernel(StoiSignals sig, int row0, const double* __restrict__ basis,
                                                             const double* __restrict__ window, const int* __restrict__ src,
                                                             const int* __restrict__ count, long long F,
                                                             double* __restrict__ bands) {
  __shared__ double sZ[2 * kZWords];
  __shared__ double sW[kStoiFrame];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = row0 + blockIdx.y;
  const long long K = count[r];
  const long long zlen = stoi_compacted_len(K), J = stoi_frames(zlen);
  const long long m0 = (long long)blockIdx.x * kStoiFrameTile;
  if (m0 >= J) return;  // (uniform) this row has no such tile: its band values are never read
  const int* kept = src + (size_t)r * (size_t)F;

  for (int k = tid; k < kStoiFrame; k += kThreads) sW[k] = window[k];
  // the 17 hops of both overlap-added signals: sample s is w[s - 128 k] x[128 src[k] + s - 128 k] over the kept frames k that
  // cover it -- at most two, the lower one first
  for (int idx = tid; idx < 2 * kSpan; idx += kThreads) {
    const int ref = idx / kSpan, sl = idx - ref * kSpan;
    const long long s = m0 * kStoiHop + sl;
    double v = 0.0;
    if (s < zlen) {
      long long hi = s >> 7;
      if (hi > K - 1) hi = K - 1;
      const long long lo = hi - 1;
      if (lo >= 0 && s - lo * kStoiHop < kStoiFrame) {
        const int o = (int)(s - lo * kStoiHop);
        v += window[o] * sample(sig, ref, r, (long long)kept[lo] * kStoiHop + o);
      }
      const int o = (int)(s - hi * kStoiHop);  // 0 .. 255: s < 128 (K - 1) + 256
      v += window[o] * sample(sig, ref, r, (long long)kept[hi] * kStoiHop + o);
    }
    sZ[ref * kZWords + sl + 4 * (sl >> 7)] = v;
  }
  __syncthreads();

  const int signal = wave & 1, half = wave >> 1;
  const int fi = lane & 15, kk = lane >> 4;
  const double* za = sZ + signal * kZWords + 132 * fi + kk;  // z[128 fi + k] at 132 fi + k + 4 (k >> 7)
  const int last_bin = half ? kEdges[kStoiBands] : kHalfBin;  // the edge that closes this half's last band
  int band = half ? kHalfBand : 0;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  double* outp = bands + ((size_t)(r * 2 + signal) * kStoiBands) * (size_t)F;
  for (int t = 0; t < kStoiBinTiles / 2; t++) {
    const int tt = half * (kStoiBinTiles / 2) + t;
    f64x4 re = {0.0, 0.0, 0.0, 0.0}, im = re;
    const double* bc = basis + (size_t)(2 * tt) * kK4 * 64 + lane;
    const double* bs = bc + (size_t)kK4 * 64;
#pragma unroll 1
    for (int k4 = 0; k4 < kK4; k4 += 4) {  // four k-steps of operands in flight ahead of their MFMAs; k ascending all the same
      double c[4], s[4], a[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int k = 4 * (k4 + u);  // + kk: inside za and below
        c[u] = bc[(k4 + u) * 64];
        s[u] = bs[(k4 + u) * 64];
        a[u] = za[k + 4 * (k >> 7)] * sW[k + kk];  // the windowed sample: one rounding (k + kk stays in k's half: kk < 4)
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        re = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], c[u], re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], s[u], im, 0, 0, 0);
      }
    }
    double pw[4];
#pragma unroll
    for (int q = 0; q < 4; q++) pw[q] = re[q] * re[q] + im[q] * im[q];
    const int bin0 = tile_bin0(tt);
    for (int c = 0; c < 16; c++) {  // bins ascending; band, bin and every branch on them are uniform over the wave
      const int bin = bin0 + c;
      if (bin == kEdges[band + 1]) {  // the band is complete: frames (lane >> 4) + 4 q of this lane group
        if (fi == 0) {
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const long long m = m0 + kk + 4 * q;
            if (m < J) outp[(size_t)band * (size_t)F + m] = sqrt(acc[q]);
          }
        }
        band++;
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = 0.0;
      }
      if (bin >= last_bin) break;
#pragma unroll
      for (int q = 0; q < 4; q++) acc[q] += __shfl(pw[q], (lane & 48) | c, 64);
    }
  }
}

// grid (ceil(segments of the longest row / 16), rows of the launch).  Segment i of a row is frames i .. i + 29 of its band
// values ([:, m - 30 : m] with m = i + 30).  kExtended false: sum over segment and band of the correlation of x with the
// clipped, rescaled y; true: sum over segment and frame of the correlation across bands of the row- then column-normalised
// x and y.
template <bool kExtended>
__global__ __launch_bounds__(kThreads) void stoi_seg_kernel(int row0, const double* __restrict__ bands, const int* __restrict__ count,
                                                            long long F, double clip, double* __restrict__ partial,
                                                            long long seg_stride) {
  __shared__ double red[kThreads / 64];
  __shared__ double stats[kStoiSegTile * kStoiBands * 4];
  const int tid = threadIdx.x, r = row0 + blockIdx.y;
  const long long J = stoi_frames(stoi_compacted_len(count[r]));
  const long long M = J - kStoiSegment + 1;
  const long long s0 = (long long)blockIdx.x * kStoiSegTile;
  if (J < kStoiSegment || s0 >= M) return;  // (uniform) no such tile: its partial is never read
  const double* X = bands + ((size_t)(r * 2 + 1) * kStoiBands) * (size_t)F;  // the clean signal
  const double* Y = bands + ((size_t)(r * 2 + 0) * kStoiBands) * (size_t)F;  // the estimate
  double d = 0.0;
  const int seg = tid / kStoiBands, band = tid - seg * kStoiBands;
  const bool live = seg < kStoiSegTile && s0 + seg < M;
  if (live) {
    const double* x = X + (size_t)band * (size_t)F + s0 + seg;  // frames s0 + seg .. + 29 <= J - 1
    const double* y = Y + (size_t)band * (size_t)F + s0 + seg;
    if (!kExtended) {
      double nx = 0.0, ny = 0.0;
      for (int j = 0; j < kStoiSegment; j++) {
        nx += x[j] * x[j];
        ny += y[j] * y[j];
      }
      const double c = sqrt(nx) / (sqrt(ny) + kEps);
      double mx = 0.0, my = 0.0;
      for (int j = 0; j < kStoiSegment; j++) {
        mx += x[j];
        my += fmin(c * y[j], x[j] * clip);
      }
      mx /= (double)kStoiSegment;
      my /= (double)kStoiSegment;
      double vx = 0.0, vy = 0.0;
      for (int j = 0; j < kStoiSegment; j++) {
        const double a = x[j] - mx, e = fmin(c * y[j], x[j] * clip) - my;
        vx += a * a;
        vy += e * e;
      }
      const double dx = sqrt(vx) + kEps, dy = sqrt(vy) + kEps;
      for (int j = 0; j < kStoiSegment; j++) d += ((x[j] - mx) / dx) * ((fmin(c * y[j], x[j] * clip) - my) / dy);
    } else {
      double mx = 0.0, my = 0.0;
      for (int j = 0; j < kStoiSegment; j++) {
        mx += x[j];
        my += y[j];
      }
      mx /= (double)kStoiSegment;
      my /= (double)kStoiSegment;
      double vx = 0.0, vy = 0.0;
      for (int j = 0; j < kStoiSegment; j++) {
        const double a = x[j] - mx, e = y[j] - my;
        vx += a * a;
        vy += e * e;
      }
      double* st = stats + (seg * kStoiBands + band) * 4;
      st[0] = mx; st[1] = sqrt(vx) + kEps; st[2] = my; st[3] = sqrt(vy) + kEps;
    }
  }
  if (kExtended) {
    __syncthreads();
    for (int it = tid; it < kStoiSegTile * kStoiSegment; it += kThreads) {  // one (segment, frame) per pass
      const int sg = it / kStoiSegment, j = it - sg * kStoiSegment;
      if (s0 + sg >= M) continue;
      double xb[kStoiBands], yb[kStoiBands], mx = 0.0, my = 0.0;
#pragma unroll
      for (int k = 0; k < kStoiBands; k++) {
        const double* st = stats + (sg * kStoiBands + k) * 4;
        xb[k] = (X[(size_t)k * (size_t)F + s0 + sg + j] - st[0]) / st[1];
        yb[k] = (Y[(size_t)k * (size_t)F + s0 + sg + j] - st[2]) / st[3];
        mx += xb[k];
        my += yb[k];
      }
      mx /= (double)kStoiBands;
      my /= (double)kStoiBands;
      double vx = 0.0, vy = 0.0;
#pragma unroll
      for (int k = 0; k < kStoiBands; k++) {
        xb[k] -= mx;
        yb[k] -= my;
        vx += xb[k] * xb[k];
        vy += yb[k] * yb[k];
      }
      const double dx = sqrt(vx) + kEps, dy = sqrt(vy) + kEps;
      double e = 0.0;
#pragma unroll
      for (int k = 0; k < kStoiBands; k++) e += (xb[k] / dx) * (yb[k] / dy);
      d += e;
    }
  }
  d = block_sum(d, red);
  if (tid == 0) partial[(size_t)r * (size_t)seg_stride + blockIdx.x] = d;
}

__global__ void stoi_final_kernel(int n_rows, int row0, const int* __restrict__ count, const double* __restrict__ partial,
                                  long long seg_stride, int extended, float* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_rows) return;
  const int r = row0 + b;
  const long long J = stoi_frames(stoi_compacted_len(count[r]));
  if (J < kStoiSegment) {  // fewer than 30 frames: the definition's constant
    out[r] = 1e-5f;
    return;
  }
  const long long M = J - kStoiSegment + 1, nt = (M + kStoiSegTile - 1) / kStoiSegTile;
  const double* p = partial + (size_t)r * (size_t)seg_stride;
  double s = 0.0;
  for (long long t = 0; t < nt; t++) s += p[t];  // tiles ascending
  out[r] = (float)(s / ((double)(extended ? kStoiSegment : kStoiBands) * (double)M));
}

inline unsigned tiles_of(long long n, int tile) { return (unsigned)((n + tile - 1) / tile); }

}  // namespace

hipError_t launch_stoi_resample(const StoiSignals& sig, const StoiRows& rows, int n_rows, int row0, long long n10_max, int p, int q,
                                int taps, const void* table, double* res_est, double* res_ref, hipStream_t st) {
  const int* first = static_cast<const int*>(table);
  const double* coef = reinterpret_cast<const double*>(first + ((p + 1) & ~1));
  stoi_resample_kernel<<<dim3(tiles_of(n10_max, kThreads), n_rows), dim3(kThreads), 0, st>>>(sig, rows, row0, p, q, taps, first, coef,
                                                                                             res_est, res_ref);
  return hipGetLastError();
}

hipError_t launch_stoi_basis(double* basis, double* window, hipStream_t st) {
  const long long n = (long long)kStoiBasisWords + kStoiFrame;
  stoi_basis_kernel<<<dim3(tiles_of(n, 256)), dim3(256), 0, st>>>(basis, window);
  return hipGetLastError();
}

hipError_t launch_stoi_energy(const StoiSignals& sig, const StoiRows& rows, int n_rows, int row0, long long n10_max,
                              const double* window, double* energy, long long F, hipStream_t st) {
  const long long nf = stoi_frames(n10_max);
  if (nf < 1) return hipSuccess;  // no row of the launch has a frame
  stoi_energy_kernel<<<dim3(tiles_of(nf, 16), n_rows), dim3(kThreads), 0, st>>>(sig, rows, row0, window, energy, F);
  return hipGetLastError();
}

hipError_t launch_stoi_mask(const StoiRows& rows, int n_rows, int row0, const double* energy, long long F, int* src, int* count,
                            hipStream_t st) {
  stoi_mask_kernel<<<dim3(n_rows), dim3(kMaskThreads), 0, st>>>(rows, row0, energy, F, src, count);
  return hipGetLastError();
}

hipError_t launch_stoi_stft(const StoiSignals& sig, const StoiRows& rows, int n_rows, int row0, long long n10_max,
                            const double* basis, const double* window, const int* src, const int* count, long long F,
                            double* bands, hipStream_t st) {
  const long long jmax = stoi_frames(stoi_compacted_len(stoi_frames(n10_max)));  // every frame kept
  if (jmax < 1) return hipSuccess;
  stoi_stft_kernel<<<dim3(tiles_of(jmax, kStoiFrameTile), n_rows), dim3(kThreads), 0, st>>>(sig, row0, basis, window, src, count, F,
                                                                                            bands);
  return hipGetLastError();
}

hipError_t launch_stoi_segments(bool extended, const StoiRows& rows, int n_rows, int row0, long long n10_max, const double* bands,
                                const int* count, long long F, double clip, double* partial, long long seg_stride, float* out,
                                hipStream_t st) {
  const long long tiles = stoi_seg_tiles(stoi_frames(stoi_compacted_len(stoi_frames(n10_max))));
  if (tiles > 0) {
    const dim3 grid((unsigned)tiles, n_rows), block(kThreads);
    if (extended)
      stoi_seg_kernel<true><<<grid, block, 0, st>>>(row0, bands, count, F, clip, partial, seg_stride);
    else
      stoi_seg_kernel<false><<<grid, block, 0, st>>>(row0, bands, count, F, clip, partial, seg_stride);
    if (hipError_t e = hipGetLastError()) return e;
  }
  stoi_final_kernel<<<dim3(1), dim3(kStoiRowsPerLaunch), 0, st>>>(n_rows, row0, count, partial, seg_stride, extended ? 1 : 0, out);
  return hipGetLastError();
}

}  // namespace ou
