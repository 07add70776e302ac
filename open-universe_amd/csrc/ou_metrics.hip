// Scores of an estimate against a reference over ragged rows: ou_lsd, ou_spectral_mae, ou_si_sdr of include/ouniverse.h
// ("scoring").  Three kernel families, all on the caller's stream, no atomics, every sum in one fixed order:
//
//   met_time_kernel    one workgroup per row: sum xy, sum x^2, sum y^2, sum (x - y)^2 in double, alpha = sum xy / (sum x^2 + eps),
//                      then sum |alpha x - y| in a second walk of the row (alpha stays a double).
//   met_basis_kernel   the cos / -sin basis and the periodic Hann window of one n_fft in double, angles reduced in integers mod n_fft,
//                      stored in the order the MFMA B operand is read (below).
//   met_stft_kernel    one workgroup = one row x 16 consecutive STFT frames of BOTH signals.  The 32 frames are formed in LDS
//                      straight from the waveforms (centre padding by index arithmetic: reflect or zero), the real DFT is a
//                      (32 x n_fft) x (n_fft x 2 bins) GEMM on the matrix pipe, and the per-bin term is formed from the
//                      accumulators in registers and reduced to ONE double per workgroup.  No spectrogram reaches HBM.
//   met_final_*        one thread per row sums the row's partials in ascending tile order, in double, into the result.
//
// The GEMM runs on v_mfma_f64_16x16x4_f64, not on the fp32 form.  Measured with the fp32 form (v_mfma_f32_16x16x4_f32, fp32
// window product and basis): rows of two to four frames landed 2 to 7 fp32 ulps from float64, and a host emulation
// attributes that to the fp32 OPERANDS -- the window rounded to fp32 alone moves the two-frame LSD at n_fft 600 by 3.6 ulps,
// exact accumulation or not -- so no summation order on the fp32 pipe holds the 4-ulp gate of tests/test_gpu_metrics.py.  With
// double operands the same rows are within 0.4 ulp.  The f64 form has half the rate; the samples stay fp32 in LDS.
//
// Tile plan of met_stft_kernel (256 threads = 4 waves):
//   A operand: sA[k4][half][kk][i] = frame(f0 + i of signal `half`)[4 k4 + kk] as fp32 in LDS -- 32 * Kpad floats, Kpad = n_fft
//     rounded up to 4 (zeros behind n_fft).  Lane l of a wave reads sA[k4 * 128 + half * 64 + l] (lane-linear, no conflict)
//     and multiplies by the double window value of its k, w[4 k4 + (l >> 4)].
//   B operand (global, L2-resident: 1.3 MB at n_fft 400): basis[(2 t + c)][k4][l] = cos / -sin(2 pi k bin / n_fft), k = 4 k4 +
//     (l >> 4), bin = 16 t + (l & 15), zero for bin >= n_fft / 2 + 1 or k >= n_fft.  One 512-byte row per wave and k-step.
//   Wave w owns bin tiles t = w, w + 4, ...; per tile four accumulators (est / ref x re / im), n_fft / 4 k-steps of 4 MFMAs.
//   Epilogue: lane l, register r holds frame f0 + (l >> 4) + 4 r, bin 16 t + (l & 15) of all four; bins >= n_fft / 2 + 1 and
//     frames >= the row's own count are masked, never summed.
// Dynamic LDS: 128 * Kpad bytes (51 200 at n_fft 400, 131 072 at the cap of 1024 = OU_METRICS_MAX_NFFT).
#include "ou_internal.h"

namespace ou {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kStftThreads = 256;
constexpr int kTimeThreads = 1024;

// fixed-order sum over the workgroup: lanes by shuffle, waves ascending.  Every thread must call it; the result is valid in thread 0
// (and broadcast through red[0] after the trailing barrier).  red: one double per wave.
__device__ inline double block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
    for (int i = 0; i < nw; i++) s += red[i];
    red[0] = s;
  }
  __syncthreads();
  return red[0];
}

// grid (rows of this launch), 1024 threads.  tsum: 8 doubles per row (sxy, sxx, syy, sdd, sabs, alpha, -, -)
__global__ __launch_bounds__(kTimeThreads) void met_time_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                                long long stride, MetRows rows, int row0, float eps,
                                                                int scale_invariant, double* __restrict__ tsum) {
  __shared__ double red[kTimeThreads / 64];
  const int b = blockIdx.x;
  const long long len = rows.len[b];
  const float* x = est + (size_t)(row0 + b) * (size_t)stride;
  const float* y = ref + (size_t)(row0 + b) * (size_t)stride;
  double sxy = 0.0, sxx = 0.0, syy = 0.0, sdd = 0.0;
  for (long long i = threadIdx.x; i < len; i += kTimeThreads) {
    const double xv = x[i], yv = y[i], d = xv - yv;
    sxy += xv * yv;
    sxx += xv * xv;
    syy += yv * yv;
    sdd += d * d;
  }
  sxy = block_sum(sxy, red);
  sxx = block_sum(sxx, red);
  syy = block_sum(syy, red);
  sdd = block_sum(sdd, red);
  const double a = scale_invariant ? sxy / (sxx + (double)eps) : 1.0;
  double sabs = 0.0;
  for (long long i = threadIdx.x; i < len; i += kTimeThreads) sabs += fabs(a * (double)x[i] - (double)y[i]);
  sabs = block_sum(sabs, red);
  if (threadIdx.x == 0) {
    double* t = tsum + (size_t)(row0 + b) * 8;
    t[0] = sxy; t[1] = sxx; t[2] = syy; t[3] = sdd; t[4] = sabs; t[5] = a;
  }
}

// one thread per word of basis (nbt * 2 * K4 * 64 doubles) and of window (4 * K4 doubles)
__global__ void met_basis_kernel(double* __restrict__ basis, double* __restrict__ window, int n_fft, int K4, int nbt) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nb = (long long)nbt * 2 * K4 * 64;
  const int nbins = n_fft / 2 + 1;
  if (e < nb) {
    const int l = (int)(e & 63);
    const long long q = e >> 6;
    const int k4 = (int)(q % K4), tc = (int)(q / K4);
    const int k = 4 * k4 + (l >> 4), bin = 16 * (tc >> 1) + (l & 15);
    double v = 0.0;
    if (k < n_fft && bin < nbins) {
      const long long m = ((long long)k * bin) % n_fft;  // the angle, reduced exactly
      const double ang = 2.0 * M_PI * (double)m / (double)n_fft;
      v = (tc & 1) ? -sin(ang) : cos(ang);
    }
    basis[e] = v;
  } else if (e < nb + 4ll * K4) {
    const int k = (int)(e - nb);
    window[k] = k < n_fft ? 0.5 - 0.5 * cos(2.0 * M_PI * (double)k / (double)n_fft) : 0.0;  // periodic Hann
  }
}

// kL1 false: sum of (L(|X|^2 / sum w^2 + eps) - L(|alpha Y|^2 / sum w^2 + eps))^2, L = 10 log10 or ln, reflect padding;
// kL1 true : sum of | |alpha X| - |Y| |, zero padding.   X: estimate, Y: reference.
// grid (frame tiles of the longest row of the launch, rows of the launch); partial[(row0 + b) * tile_stride + tile]
template <bool kL1>
__global__ __launch_bounds__(kStftThreads) void met_stft_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                                long long stride, MetRows rows, int row0,
                                                                const double* __restrict__ basis, const double* __restrict__ window,
                                                                const double* __restrict__ tsum, int n_fft, int hop, int K4,
                                                                int nbt, double inv_w2, double eps, int natural_log,
                                                                double* __restrict__ partial, long long tile_stride) {
  extern __shared__ __attribute__((aligned(16))) float sA[];
  __shared__ double red[kStftThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const long long len = rows.len[b];
  const long long nfr = 1 + len / hop;
  const long long f0 = (long long)blockIdx.x * 16;
  if (f0 >= nfr) return;  // (uniform) this row has no such tile: its partial is never read
  const float* x = est + (size_t)(row0 + b) * (size_t)stride;
  const float* y = ref + (size_t)(row0 + b) * (size_t)stride;
  const int Kpad = 4 * K4, half_n = n_fft / 2;

  // the 32 frames, samples as they are: consecutive threads take consecutive k of one frame (coalesced reads of the waveform)
  for (int idx = tid; idx < 32 * Kpad; idx += kStftThreads) {
    const int row = idx / Kpad, k = idx - row * Kpad;
    const long long f = f0 + (row & 15);
    float v = 0.0f;
    if (k < n_fft && f < nfr) {
      long long s = f * hop + k - half_n;
      if (!kL1) {  // reflect about sample 0 and about the row's own last sample (len > n_fft / 2: one reflection is enough)
        if (s < 0) s = -s;
        if (s >= len) s = 2 * (len - 1) - s;
      }
      if (s >= 0 && s < len) v = row < 16 ? x[s] : y[s];
    }
    sA[(k >> 2) * 128 + (row >> 4) * 64 + (k & 3) * 16 + (row & 15)] = v;
  }
  __syncthreads();

  const double a = tsum[(size_t)(row0 + b) * 8 + 5];  // alpha of the row (1 without OU_MET_SCALE_INVARIANT)
  const int nbins = half_n + 1;
  double acc = 0.0;
  for (int t = wave; t < nbt; t += kStftThreads / 64) {
    f64x4 xr = {0.0, 0.0, 0.0, 0.0}, xi = xr, yr = xr, yi = xr;
    const double* bc = basis + (size_t)(2 * t) * K4 * 64 + lane;
    const double* bs = bc + (size_t)K4 * 64;
    const double* pw = window + (lane >> 4);  // w[4 k4 + (lane >> 4)]: the k of this lane's A element
    const float* pa = sA + lane;
    int k4 = 0;
    for (; k4 + 4 <= K4; k4 += 4) {  // four k-steps of operands in flight ahead of their 16 MFMAs; k ascending all the same
      double c[4], s[4], ax[4], ay[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const double w = pw[(k4 + u) * 4];
        c[u] = bc[(k4 + u) * 64];
        s[u] = bs[(k4 + u) * 64];
        ax[u] = (double)pa[(k4 + u) * 128] * w;  // the windowed sample: one rounding, in double
        ay[u] = (double)pa[(k4 + u) * 128 + 64] * w;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        xr = __builtin_amdgcn_mfma_f64_16x16x4f64(ax[u], c[u], xr, 0, 0, 0);
        xi = __builtin_amdgcn_mfma_f64_16x16x4f64(ax[u], s[u], xi, 0, 0, 0);
        yr = __builtin_amdgcn_mfma_f64_16x16x4f64(ay[u], c[u], yr, 0, 0, 0);
        yi = __builtin_amdgcn_mfma_f64_16x16x4f64(ay[u], s[u], yi, 0, 0, 0);
      }
    }
    for (; k4 < K4; k4++) {
      const double w = pw[k4 * 4], c = bc[k4 * 64], s = bs[k4 * 64];
      const double ax = (double)pa[k4 * 128] * w, ay = (double)pa[k4 * 128 + 64] * w;
      xr = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, c, xr, 0, 0, 0);
      xi = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, s, xi, 0, 0, 0);
      yr = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, c, yr, 0, 0, 0);
      yi = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, s, yi, 0, 0, 0);
    }
    const int bin = 16 * t + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const long long f = f0 + (lane >> 4) + 4 * r;  // (the f64 C/D map: row = (lane >> 4) + 4 r, not the fp32 forms' 4 (lane >> 4) + r)
      if (bin < nbins && f < nfr) {  // the partial bin tile and the partial frame tile are masked, not padded into the sum
        const double px = xr[r] * xr[r] + xi[r] * xi[r];
        const double py = yr[r] * yr[r] + yi[r] * yi[r];
        if (kL1) {
          acc += fabs(fabs(a) * sqrt(px) - sqrt(py));
        } else {
          const double lx = px * inv_w2 + eps, ly = a * a * py * inv_w2 + eps;
          const double d = natural_log ? log(lx) - log(ly) : 10.0 * log10(lx) - 10.0 * log10(ly);
          acc += d * d;
        }
      }
    }
  }
  acc = block_sum(acc, red);
  if (tid == 0) partial[(size_t)(row0 + b) * (size_t)tile_stride + blockIdx.x] = acc;
}

__device__ inline double row_partials(const double* __restrict__ partial, long long tile_stride, int row, long long nfr) {
  const long long nt = (nfr + 15) / 16;
  const double* p = partial + (size_t)row * (size_t)tile_stride;
  double s = 0.0;
  for (long long t = 0; t < nt; t++) s += p[t];
  return s;
}

__global__ void met_final_lsd_kernel(MetRows rows, int n_rows, int row0, const double* __restrict__ partial, long long tile_stride,
                                     int hop, int nbins, float* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_rows) return;
  const long long nfr = 1 + rows.len[b] / hop;
  const double s = row_partials(partial, tile_stride, row0 + b, nfr);
  out[row0 + b] = (float)sqrt(s / ((double)nfr * (double)nbins));
}

__global__ void met_final_l1_kernel(MetRows rows, int n_rows, int row0, const double* __restrict__ partial, MetSpecs specs,
                                    const double* __restrict__ tsum, float tdw, float* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_rows) return;
  const long long len = rows.len[b];
  const double td = tsum[(size_t)(row0 + b) * 8 + 4] / (double)len;
  if (specs.n == 0) {
    out[row0 + b] = (float)td;
    return;
  }
  double sp = 0.0;
  for (int i = 0; i < specs.n; i++) {
    const long long nfr = 1 + len / specs.hop[i];
    sp += row_partials(partial + specs.offset[i], specs.tile_stride[i], row0 + b, nfr) / ((double)nfr * (double)specs.nbins[i]);
  }
  out[row0 + b] = (float)((double)tdw * td + (1.0 - (double)tdw) * sp / (double)specs.n);
}

// 10 log10(c / (1 - c)) with the coherence c clamped to [e, 1 - e], e = 10^(-clamp / 10) / (1 + 10^(-clamp / 10))
__device__ inline float clamped_db(double coh, double e) {
  coh = coh < e ? e : (coh > 1.0 - e ? 1.0 - e : coh);
  return (float)(10.0 * log10(coh / (1.0 - coh)));
}

__global__ void met_final_sdr_kernel(int n_rows, int row0, const double* __restrict__ tsum, float clamp_db,
                                     float* __restrict__ out_si_sdr, float* __restrict__ out_snr) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_rows) return;
  const double* t = tsum + (size_t)(row0 + b) * 8;
  const double sxy = t[0], sxx = t[1], syy = t[2], sdd = t[3];
  const double p = pow(10.0, -(double)clamp_db / 10.0), e = p / (1.0 + p);
  if (out_si_sdr) out_si_sdr[row0 + b] = clamped_db(sxx * syy > 0.0 ? (sxy * sxy) / (sxx * syy) : 0.0, e);
  if (out_snr) out_snr[row0 + b] = clamped_db(syy + sdd > 0.0 ? syy / (syy + sdd) : 0.0, e);
}

hipError_t stft_lds_limit() {
  static hipError_t status = [] {
    const int bytes = 128 * kMetMaxNfft;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(met_stft_kernel<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(met_stft_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               bytes);
  }();
  return status;
}

}  // namespace

hipError_t launch_met_time(const float* est, const float* ref, long long stride, const MetRows& rows, int n_rows, int row0,
                           float eps, bool scale_invariant, double* tsum, hipStream_t st) {
  met_time_kernel<<<dim3(n_rows), dim3(kTimeThreads), 0, st>>>(est, ref, stride, rows, row0, eps, scale_invariant ? 1 : 0, tsum);
  return hipGetLastError();
}

hipError_t launch_met_basis(double* basis, double* window, int n_fft, hipStream_t st) {
  const int K4 = met_k4(n_fft), nbt = met_bin_tiles(n_fft);
  const long long n = (long long)nbt * 2 * K4 * 64 + 4ll * K4;
  met_basis_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(basis, window, n_fft, K4, nbt);
  return hipGetLastError();
}

hipError_t launch_met_stft(bool l1, const float* est, const float* ref, long long stride, const MetRows& rows, int n_rows, int row0,
                           long long len_max, const double* basis, const double* window, const double* tsum, int n_fft, int hop,
                           double w2, float eps, bool natural_log, double* partial, long long tile_stride, hipStream_t st) {
  hipError_t e = stft_lds_limit();
  if (e != hipSuccess) return e;
  const int K4 = met_k4(n_fft), nbt = met_bin_tiles(n_fft);
  const long long tiles = met_frame_tiles(len_max, hop);
  const dim3 grid((unsigned)tiles, (unsigned)n_rows), block(kStftThreads);
  const size_t smem = (size_t)128 * 4 * K4;
  const double inv_w2 = 1.0 / w2;
  if (l1)
    met_stft_kernel<true><<<grid, block, smem, st>>>(est, ref, stride, rows, row0, basis, window, tsum, n_fft, hop, K4, nbt, inv_w2,
                                                     (double)eps, 0, partial, tile_stride);
  else
    met_stft_kernel<false><<<grid, block, smem, st>>>(est, ref, stride, rows, row0, basis, window, tsum, n_fft, hop, K4, nbt, inv_w2,
                                                      (double)eps, natural_log ? 1 : 0, partial, tile_stride);
  return hipGetLastError();
}

hipError_t launch_met_final_lsd(const MetRows& rows, int n_rows, int row0, const double* partial, long long tile_stride, int hop,
                                int n_fft, float* out, hipStream_t st) {
  met_final_lsd_kernel<<<dim3(1), dim3(kMetRowsPerLaunch), 0, st>>>(rows, n_rows, row0, partial, tile_stride, hop, n_fft / 2 + 1, out);
  return hipGetLastError();
}

hipError_t launch_met_final_l1(const MetRows& rows, int n_rows, int row0, const double* partial, const MetSpecs& specs,
                               const double* tsum, float tdw, float* out, hipStream_t st) {
  met_final_l1_kernel<<<dim3(1), dim3(kMetRowsPerLaunch), 0, st>>>(rows, n_rows, row0, partial, specs, tsum, tdw, out);
  return hipGetLastError();
}

hipError_t launch_met_final_sdr(int n_rows, int row0, const double* tsum, float clamp_db, float* out_si_sdr, float* out_snr,
                                hipStream_t st) {
  met_final_sdr_kernel<<<dim3(1), dim3(kMetRowsPerLaunch), 0, st>>>(n_rows, row0, tsum, clamp_db, out_si_sdr, out_snr);
  return hipGetLastError();
}

}  // namespace ou
