// Segmented enhance (ou_enhance_segments): whole-file statistics, window gathers, crossfade stitch and post step over LONG
// rows.  Every index into a long row is 64-bit and no kernel here builds a buffer descriptor, so nothing wraps past 2^32 bytes
// per row.  Reductions run in a fixed order (per-block partials in double, summed in block order by whoever needs the
// total): two runs give the same bits.  With one block per row the order is exactly that of pad_normalize_kernel /
// post_kernel, so a file that fits into one window gets the whole-file call's statistics bit for bit.
// The *_var forms (ou_enhance_segments_var) do the same for rows of lengths of their own: the geometry of a row comes from a
// device table, a group's entries (row, window, length) from the kernel arguments, and every row reduces over the block
// partition of the call on that row alone.
#include "ou_internal.h"

namespace ou {
namespace {

template <typename T>
__device__ __forceinline__ T seg_wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float seg_wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
template <typename T>
__device__ T seg_block_sum(T v, T* sh) {  // blockDim multiple of 64, <= 1024 (same order as block_sum, ou_small.hip)
  v = seg_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = 0;
  for (int i = 0; i < (int)(blockDim.x >> 6); i++) r += sh[i];
  return r;
}
__device__ float seg_block_max(float v, float* sh) {
  v = seg_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); i++) r = fmaxf(r, sh[i]);
  return r;
}

// start of window k (SegGeom, ou_kernels.h): k * hop, the last one shifted to end at T_pad
__device__ __forceinline__ long long seg_start(const SegGeom& g, long long k) {
  return k < g.n_win - 1 ? k * g.hop : g.T_pad - g.L;
}

// ---- whole-file statistics (utils/norm.py:47-87, universe.py:259) ------------------------------------------------------
// pass 1: per-block sum and sum of squares of the raw row.  grid (nb, C)
__global__ __launch_bounds__(1024) void seg_stats1_kernel(const float* __restrict__ mix, double* __restrict__ part,
                                                          long long T_raw, int nb) {
  __shared__ double shd[16];
  const int j = blockIdx.x, c = blockIdx.y;
  const float* xb = mix + (size_t)c * T_raw;
  double s = 0, sq = 0;
  for (long long t = (long long)j * 1024 + threadIdx.x; t < T_raw; t += (long long)nb * 1024) {
    const double d = xb[t];
    s += d; sq += d * d;
  }
  s = seg_block_sum(s, shd);
  sq = seg_block_sum(sq, shd);
  if (threadIdx.x == 0) { part[((size_t)c * nb + j) * 3 + 0] = s; part[((size_t)c * nb + j) * 3 + 1] = sq; }
}
// pass 2: per-block sum of (x - mean)^2 around the mean of the padded row (each block sums the partials of pass 1 in order)
__global__ __launch_bounds__(1024) void seg_stats2_kernel(const float* __restrict__ mix, double* __restrict__ part,
                                                          long long T_raw, long long T_pad, int nb) {
  __shared__ double shd[16];
  const int j = blockIdx.x, c = blockIdx.y;
  const double* pc = part + (size_t)c * nb * 3;
  double s = pc[0];
  for (int i = 1; i < nb; i++) s += pc[i * 3];
  const float mean = (float)(s / (double)T_pad);  // norm.py:62  (mean over the padded signal)
  const float* xb = mix + (size_t)c * T_raw;
  double ss = 0;
  for (long long t = (long long)j * 1024 + threadIdx.x; t < T_raw; t += (long long)nb * 1024) {
    const double d = (double)(xb[t] - mean);
    ss += d * d;
  }
  ss = seg_block_sum(ss, shd);
  if (threadIdx.x == 0) part[((size_t)c * nb + j) * 3 + 2] = ss;
}
// finish: stats[c] = {mean, gain, mix_rms, 0}  (the layout of pad_normalize_kernel's stats)
__global__ void seg_stats_finish_kernel(const double* __restrict__ part, float* __restrict__ stats, long long T_raw,
                                        long long T_pad, int nb, float level) {
  const int c = blockIdx.x;
  if (threadIdx.x != 0) return;
  const double* pc = part + (size_t)c * nb * 3;
  double s = pc[0], sq = pc[1], ss = pc[2];
  for (int i = 1; i < nb; i++) { s += pc[i * 3]; sq += pc[i * 3 + 1]; ss += pc[i * 3 + 2]; }
  const float mean = (float)(s / (double)T_pad);
  ss += (double)(T_pad - T_raw) * (double)(0.f - mean) * (double)(0.f - mean);
  float sd = (float)sqrt(ss / (double)(T_pad - 1));  // unbiased std, norm.py:22-23
  sd = fmaxf(sd, 1e-5f);
  stats[c * 4 + 0] = mean;
  stats[c * 4 + 1] = level / sd;
  stats[c * 4 + 2] = (float)sqrt(sq / (double)T_raw);
  stats[c * 4 + 3] = 0.f;
}

// ---- whole-file mel normalisation (condition.py:105-106) ---------------------------------------------------------------
// The frame energies of mel_kernel over the whole normalised file, without the mel output: the normalisation (x - mean) * gain
// and the pad split are applied on the fly to the raw row.  Same arithmetic, same order as mel_kernel.  grid (L, C)
__global__ __launch_bounds__(512) void seg_mel_energy_kernel(const float* __restrict__ mix, const float* __restrict__ stats,
                                                             const float* __restrict__ win, const float* __restrict__ tw,
                                                             const float* __restrict__ fb, float* __restrict__ esum,
                                                             long long T_raw, long long T_pad, long long pad_left,
                                                             int n_fft, int hop, int mel_pad, int n_freq, int n_mels,
                                                             long long L) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* sx = sm;
  float* tc = sx + n_fft;
  float* ts = tc + n_fft;
  float* pw = ts + n_fft;
  __shared__ float shf[8];
  const long long f = blockIdx.x;
  const int c = blockIdx.y, tid = threadIdx.x;
  const float mean = stats[c * 4 + 0], gain = stats[c * 4 + 1];
  const float* xb = mix + (size_t)c * T_raw;
  for (int n = tid; n < n_fft; n += 512) {
    const long long t = f * hop + n - mel_pad;
    float v = 0.f;
    if (t >= 0 && t < T_pad) {
      const long long tr = t - pad_left;
      v = ((tr >= 0 && tr < T_raw) ? xb[tr] : 0.f);
      v = (v - mean) * gain;
    }
    sx[n] = v * win[n];
    tc[n] = tw[n];
    ts[n] = tw[n_fft + n];
  }
  __syncthreads();
  for (int k = tid; k < n_freq; k += 512) {
    float re = 0.f, im = 0.f;
    int idx = 0;
    for (int n = 0; n < n_fft; n++) {
      float v = sx[n];
      re = fmaf(v, tc[idx], re);
      im = fmaf(-v, ts[idx], im);
      idx += k;
      if (idx >= n_fft) idx -= n_fft;
    }
    pw[k] = re * re + im * im;
  }
  __syncthreads();
  float e = 0.f;
  for (int m = tid; m < n_mels; m += 512) {
    float acc = 0.f;
    for (int k = 0; k < n_freq; k++) acc = fmaf(pw[k], fb[(size_t)k * n_mels + m], acc);
    e += acc * acc;
  }
  e = seg_block_sum(e, shf);
  if (tid == 0) esum[(size_t)c * L + f] = e;
}

// ---- window gathers ----------------------------------------------------------------------------------------------------
// mixn[j][t] = (x[c_j][s_j + t - pad_left] - mean_c) * gain_c (0 outside the raw row: the whole-file pad split), and
// mel_scale[j] = the whole-file mel scale of row c_j.  Entries e0 + j past the last real one repeat it.  grid (ceil(L/1024), B)
__global__ __launch_bounds__(256) void seg_gather_input_kernel(const float* __restrict__ mix, const float* __restrict__ stats,
                                                               const float* __restrict__ row_mel_scale, float* __restrict__ mixn,
                                                               float* __restrict__ mel_scale, SegGeom g, long long e0) {
  const int j = blockIdx.y;
  long long e = e0 + j;
  if (e > g.n_entries - 1) e = g.n_entries - 1;
  const long long c = e / g.n_win, k = e - c * g.n_win;
  const long long s = seg_start(g, k);
  const float mean = stats[c * 4 + 0], gain = stats[c * 4 + 1];
  const float* xb = mix + (size_t)c * g.T_raw;
  float* yb = mixn + (size_t)j * g.L;
  for (long long t = (long long)blockIdx.x * 1024 + threadIdx.x; t < (long long)(blockIdx.x + 1) * 1024 && t < g.L; t += 256) {
    const long long tr = s + t - g.pad_left;
    const float v = (tr >= 0 && tr < g.T_raw) ? xb[tr] : 0.f;
    yb[t] = (v - mean) * gain;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) mel_scale[j] = row_mel_scale[c];
}
// z[j][t] = noise[c_j][s_j + t]   (one step's (C, T_pad) slice of the whole-file noise)
__global__ __launch_bounds__(256) void seg_gather_noise_kernel(const float* __restrict__ noise, float* __restrict__ z, SegGeom g,
                                                               long long e0) {
  const int j = blockIdx.y;
  long long e = e0 + j;
  if (e > g.n_entries - 1) e = g.n_entries - 1;
  const long long c = e / g.n_win, k = e - c * g.n_win;
  const float* src = noise + (size_t)c * g.T_pad + seg_start(g, k);
  float* dst = z + (size_t)j * g.L;
  for (long long t = (long long)blockIdx.x * 1024 + threadIdx.x; t < (long long)(blockIdx.x + 1) * 1024 && t < g.L; t += 256)
    dst[t] = src[t];
}

// ---- crossfade stitch ----------------------------------------------------------------------------------------------------
// Entry k of a row writes the samples [w_k, w_{k+1}) of the padded row (w_0 = 0, w_k = e_{k-1} - O, w_n = T_pad, e_k = end of
// window k), unpadded into out.  On [w_k, e_{k-1}) it crossfades with window k - 1 (the previous entry of the group, or `carry`
// for the first entry of a group): weight a(i) = 0.5 - 0.5 cos(pi (i + 0.5) / O) for window k, 1 - a(i) for window k - 1.
// grid (ceil(L / 1024), n_real)
__global__ __launch_bounds__(256) void seg_stitch_kernel(const float* __restrict__ y, const float* __restrict__ carry,
                                                         float* __restrict__ out, SegGeom g, long long e0) {
  const int j = blockIdx.y;
  const long long e = e0 + j;
  const long long c = e / g.n_win, k = e - c * g.n_win;
  const long long s = seg_start(g, k);
  const long long w0 = k == 0 ? 0 : seg_start(g, k - 1) + g.L - g.overlap;
  const long long w1 = k == g.n_win - 1 ? g.T_pad : s + g.L - g.overlap;
  const long long e_prev = k == 0 ? 0 : seg_start(g, k - 1) + g.L;
  const float* yk = y + (size_t)j * g.L;
  const float* yp = j > 0 ? y + (size_t)(j - 1) * g.L : carry;
  const long long s_prev = k == 0 ? 0 : seg_start(g, k - 1);
  float* ob = out + (size_t)c * g.T_raw;
  for (long long t = (long long)blockIdx.x * 1024 + threadIdx.x; t < (long long)(blockIdx.x + 1) * 1024 && t < g.L; t += 256) {
    const long long u = s + t;  // position in the padded row
    if (u < w0 || u >= w1) continue;
    const long long tr = u - g.pad_left;
    if (tr < 0 || tr >= g.T_raw) continue;
    float v = yk[t];
    if (u < e_prev) {
      const float a = 0.5f - 0.5f * cosf(3.14159265358979f * ((float)(u - w0) + 0.5f) / (float)g.overlap);
      v = (1.f - a) * yp[u - s_prev] + a * v;
    }
    ob[tr] = v;
  }
}

// ---- post step over the whole row (universe.py:349-357) ----------------------------------------------------------------
// per-block sum of squares (double) and max |x|: grid (nb, C)
__global__ __launch_bounds__(1024) void seg_post_reduce_kernel(const float* __restrict__ out, double* __restrict__ part,
                                                               long long T_raw, int nb) {
  __shared__ double shd[16];
  __shared__ float shf[16];
  const int j = blockIdx.x, c = blockIdx.y;
  const float* xb = out + (size_t)c * T_raw;
  double sq = 0;
  float mx = 0.f;
  for (long long t = (long long)j * 1024 + threadIdx.x; t < T_raw; t += (long long)nb * 1024) {
    const float v = xb[t];
    const double d = v;
    sq += d * d;
    mx = fmaxf(mx, fabsf(v));
  }
  sq = seg_block_sum(sq, shd);
  mx = seg_block_max(mx, shf);
  if (threadIdx.x == 0) { part[((size_t)c * nb + j) * 2 + 0] = sq; part[((size_t)c * nb + j) * 2 + 1] = (double)mx; }
}
// keep_rms gain g = mix_rms / max(x_rms, 1e-5), peak m = max|x| * g (rounding is monotonic: = max|x * g|), x <- x * g [/ m]
__global__ __launch_bounds__(256) void seg_post_scale_kernel(float* __restrict__ out, const double* __restrict__ part,
                                                             const float* __restrict__ stats, long long T_raw, int nb,
                                                             int keep_rms, int peak_guard) {
  const int c = blockIdx.y;
  const double* pc = part + (size_t)c * nb * 2;
  double sq = pc[0];
  float mxa = (float)pc[1];
  for (int i = 1; i < nb; i++) { sq += pc[i * 2]; mxa = fmaxf(mxa, (float)pc[i * 2 + 1]); }
  float g = 1.f;
  if (keep_rms) {
    const float x_rms = fmaxf((float)sqrt(sq / (double)T_raw), 1e-5f);
    g = stats[c * 4 + 2] / x_rms;
  }
  const float mx = mxa * g;
  const bool div = peak_guard && mx > 1.0f;
  if (!keep_rms && !div) return;
  float* xb = out + (size_t)c * T_raw;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < T_raw; t += (long long)gridDim.x * 256) {
    float v = xb[t] * g;
    if (div) v = v / mx;
    xb[t] = v;
  }
}

// ==== rows of lengths of their own (ou_enhance_segments_var) ===============================================================
// The same arithmetic in the same order as the kernels above, with the row's geometry read from the SegRow table instead of the
// kernel arguments.  Grids are sized by the longest row; a block beyond the row's own share returns before it touches memory.
// Row c reduces over seg_nb(t_raw[c]) blocks -- the partition of the call on that row alone -- so its mean, gain, mix_rms and
// mel scale have that call's bits.

// blocks of a whole-row reduction (= seg_reduce_blocks)
__device__ __forceinline__ int seg_nb(long long T_raw) {
  const long long nb = (T_raw + (1ll << 18) - 1) >> 18;
  return (int)(nb < 1 ? 1 : nb > 1024 ? 1024 : nb);
}
// start of window k of row r, whose entries are `len` long (one window: T_pad - len = 0)
__device__ __forceinline__ long long seg_start_var(const SegRow& r, long long k, long long len, long long hop) {
  return k < r.n_win - 1 ? k * hop : r.T_pad - len;
}

__global__ void seg_upload_rows_kernel(SegRow* rows, SegRowBlock blk, int n, int off, SegVar v) {
  const int i = threadIdx.x;
  if (i >= n) return;
  const long long t = blk.t_raw[i];
  const long long pad = v.tot_ds - t % v.tot_ds;  // universe.py:219-223
  SegRow r;
  r.t_raw = t;
  r.T_pad = t + pad;
  r.pad_left = pad / 2;
  r.n_win = r.T_pad <= v.S ? 1 : (r.T_pad - v.S + v.hop - 1) / v.hop + 1;
  r.first = blk.first[i];
  r.frames = r.T_pad / v.tot_ds;
  rows[off + i] = r;
}
__global__ void seg_upload_lens_kernel(int* lens, SegEntryBlock blk, int n, int j0, int B, LevelSpec lv) {
  const int i = threadIdx.x;
  if (i >= n) return;
  for (int l = 0; l < lv.n; l++) lens[l * B + j0 + i] = (int)((long long)blk.len[i] * lv.num[l] / lv.den[l]);
}

// grid (nb_max, C); part: [C][nb_max][3]
__global__ __launch_bounds__(1024) void seg_stats1_var_kernel(const float* __restrict__ mix, double* __restrict__ part,
                                                              const SegRow* __restrict__ rows, long long row_stride, int nb_max) {
  __shared__ double shd[16];
  const int j = blockIdx.x, c = blockIdx.y;
  const long long T_raw = rows[c].t_raw;
  const int nb = seg_nb(T_raw);
  if (j >= nb) return;
  const float* xb = mix + (size_t)c * row_stride;
  double s = 0, sq = 0;
  for (long long t = (long long)j * 1024 + threadIdx.x; t < T_raw; t += (long long)nb * 1024) {
    const double d = xb[t];
    s += d; sq += d * d;
  }
  s = seg_block_sum(s, shd);
  sq = seg_block_sum(sq, shd);
  if (threadIdx.x == 0) { part[((size_t)c * nb_max + j) * 3 + 0] = s; part[((size_t)c * nb_max + j) * 3 + 1] = sq; }
}
__global__ __launch_bounds__(1024) void seg_stats2_var_kernel(const float* __restrict__ mix, double* __restrict__ part,
                                                              const SegRow* __restrict__ rows, long long row_stride, int nb_max) {
  __shared__ double shd[16];
  const int j = blockIdx.x, c = blockIdx.y;
  const long long T_raw = rows[c].t_raw, T_pad = rows[c].T_pad;
  const int nb = seg_nb(T_raw);
  if (j >= nb) return;
  const double* pc = part + (size_t)c * nb_max * 3;
  double s = pc[0];
  for (int i = 1; i < nb; i++) s += pc[i * 3];
  const float mean = (float)(s / (double)T_pad);
  const float* xb = mix + (size_t)c * row_stride;
  double ss = 0;
  for (long long t = (long long)j * 1024 + threadIdx.x; t < T_raw; t += (long long)nb * 1024) {
    const double d = (double)(xb[t] - mean);
    ss += d * d;
  }
  ss = seg_block_sum(ss, shd);
  if (threadIdx.x == 0) part[((size_t)c * nb_max + j) * 3 + 2] = ss;
}
__global__ void seg_stats_finish_var_kernel(const double* __restrict__ part, float* __restrict__ stats,
                                            const SegRow* __restrict__ rows, int nb_max, float level) {
  const int c = blockIdx.x;
  if (threadIdx.x != 0) return;
  const long long T_raw = rows[c].t_raw, T_pad = rows[c].T_pad;
  const int nb = seg_nb(T_raw);
  const double* pc = part + (size_t)c * nb_max * 3;
  double s = pc[0], sq = pc[1], ss = pc[2];
  for (int i = 1; i < nb; i++) { s += pc[i * 3]; sq += pc[i * 3 + 1]; ss += pc[i * 3 + 2]; }
  const float mean = (float)(s / (double)T_pad);
  ss += (double)(T_pad - T_raw) * (double)(0.f - mean) * (double)(0.f - mean);
  float sd = (float)sqrt(ss / (double)(T_pad - 1));
  sd = fmaxf(sd, 1e-5f);
  stats[c * 4 + 0] = mean;
  stats[c * 4 + 1] = level / sd;
  stats[c * 4 + 2] = (float)sqrt(sq / (double)T_raw);
  stats[c * 4 + 3] = 0.f;
}

// grid (frames_max, C); esum[c * row_stride + f] for the row's own frames
__global__ __launch_bounds__(512) void seg_mel_energy_var_kernel(const float* __restrict__ mix, const float* __restrict__ stats,
                                                                 const float* __restrict__ win, const float* __restrict__ tw,
                                                                 const float* __restrict__ fb, float* __restrict__ esum,
                                                                 const SegRow* __restrict__ rows, long long row_stride, int n_fft,
                                                                 int hop, int mel_pad, int n_freq, int n_mels) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* sx = sm;
  float* tc = sx + n_fft;
  float* ts = tc + n_fft;
  float* pw = ts + n_fft;
  __shared__ float shf[8];
  const long long f = blockIdx.x;
  const int c = blockIdx.y, tid = threadIdx.x;
  const SegRow r = rows[c];
  if (f >= r.frames) return;
  const float mean = stats[c * 4 + 0], gain = stats[c * 4 + 1];
  const float* xb = mix + (size_t)c * row_stride;
  for (int n = tid; n < n_fft; n += 512) {
    const long long t = f * hop + n - mel_pad;
    float v = 0.f;
    if (t >= 0 && t < r.T_pad) {
      const long long tr = t - r.pad_left;
      v = ((tr >= 0 && tr < r.t_raw) ? xb[tr] : 0.f);
      v = (v - mean) * gain;
    }
    sx[n] = v * win[n];
    tc[n] = tw[n];
    ts[n] = tw[n_fft + n];
  }
  __syncthreads();
  for (int k = tid; k < n_freq; k += 512) {
    float re = 0.f, im = 0.f;
    int idx = 0;
    for (int n = 0; n < n_fft; n++) {
      float v = sx[n];
      re = fmaf(v, tc[idx], re);
      im = fmaf(-v, ts[idx], im);
      idx += k;
      if (idx >= n_fft) idx -= n_fft;
    }
    pw[k] = re * re + im * im;
  }
  __syncthreads();
  float e = 0.f;
  for (int m = tid; m < n_mels; m += 512) {
    float acc = 0.f;
    for (int k = 0; k < n_freq; k++) acc = fmaf(pw[k], fb[(size_t)k * n_mels + m], acc);
    e += acc * acc;
  }
  e = seg_block_sum(e, shf);
  if (tid == 0) esum[(size_t)c * row_stride + f] = e;
}
// scale[c] = 1 / max(sqrt(mean of the row's frame energies), 1e-5): mel_scale_kernel (ou_small.hip) over the row's own frames
__global__ __launch_bounds__(256) void seg_mel_scale_var_kernel(const float* __restrict__ esum, float* __restrict__ scale,
                                                                const SegRow* __restrict__ rows, long long row_stride) {
  __shared__ double shd[4];
  const int c = blockIdx.x;
  const long long Lb = rows[c].frames;
  double s = 0;
  for (long long f = threadIdx.x; f < Lb; f += 256) s += esum[(size_t)c * row_stride + f];
  s = seg_block_sum(s, shd);
  if (threadIdx.x == 0) scale[c] = 1.0f / fmaxf((float)sqrt(s / Lb), 1e-5f);
}

// grid (ceil(T / 1024), n): entry i of the block is row j0 + i of mixn (B, T); columns from the entry's length on are 0
__global__ __launch_bounds__(256) void seg_gather_input_var_kernel(const float* __restrict__ mix, const float* __restrict__ stats,
                                                                   const float* __restrict__ row_mel_scale,
                                                                   const SegRow* __restrict__ rows, float* __restrict__ mixn,
                                                                   float* __restrict__ mel_scale, SegEntryBlock blk, int j0,
                                                                   long long T, SegVar v) {
  const int i = blockIdx.y, j = j0 + i;
  const int c = blk.row[i];
  const long long k = blk.win[i], len = blk.len[i];
  const SegRow r = rows[c];
  const long long s = seg_start_var(r, k, len, v.hop);
  const float mean = stats[c * 4 + 0], gain = stats[c * 4 + 1];
  const float* xb = mix + (size_t)c * v.row_stride;
  float* yb = mixn + (size_t)j * T;
  for (long long t = (long long)blockIdx.x * 1024 + threadIdx.x; t < (long long)(blockIdx.x + 1) * 1024 && t < T; t += 256) {
    float y = 0.f;
    if (t < len) {
      const long long tr = s + t - r.pad_left;
      const float x = (tr >= 0 && tr < r.t_raw) ? xb[tr] : 0.f;
      y = (x - mean) * gain;
    }
    yb[t] = y;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) mel_scale[j] = row_mel_scale[c];
}
__global__ __launch_bounds__(256) void seg_gather_noise_var_kernel(const float* __restrict__ noise, const SegRow* __restrict__ rows,
                                                                   float* __restrict__ z, SegEntryBlock blk, int j0, long long T,
                                                                   SegVar v) {
  const int i = blockIdx.y, j = j0 + i;
  const int c = blk.row[i];
  const long long k = blk.win[i], len = blk.len[i];
  const SegRow r = rows[c];
  const float* src = noise + (size_t)c * v.noise_stride + seg_start_var(r, k, len, v.hop);
  float* dst = z + (size_t)j * T;
  for (long long t = (long long)blockIdx.x * 1024 + threadIdx.x; t < (long long)(blockIdx.x + 1) * 1024 && t < T; t += 256)
    dst[t] = t < len ? src[t] : 0.f;
}

// grid (ceil(T / 1024), n): seg_stitch_kernel with the row's own geometry (a one-window row: w0 = 0, w1 = T_pad, no crossfade)
__global__ __launch_bounds__(256) void seg_stitch_var_kernel(const float* __restrict__ y, const float* __restrict__ carry,
                                                             float* __restrict__ out, const SegRow* __restrict__ rows,
                                                             SegEntryBlock blk, int j0, long long T, SegVar v) {
  const int i = blockIdx.y, j = j0 + i;
  const int c = blk.row[i];
  const long long k = blk.win[i], len = blk.len[i];
  const SegRow r = rows[c];
  const long long s = seg_start_var(r, k, len, v.hop);
  const long long s_prev = k == 0 ? 0 : seg_start_var(r, k - 1, len, v.hop);
  const long long w0 = k == 0 ? 0 : s_prev + len - v.overlap;
  const long long w1 = k == r.n_win - 1 ? r.T_pad : s + len - v.overlap;
  const long long e_prev = k == 0 ? 0 : s_prev + len;
  const float* yk = y + (size_t)j * T;
  const float* yp = j > 0 ? y + (size_t)(j - 1) * T : carry;
  float* ob = out + (size_t)c * v.row_stride;
  for (long long t = (long long)blockIdx.x * 1024 + threadIdx.x; t < (long long)(blockIdx.x + 1) * 1024 && t < len; t += 256) {
    const long long u = s + t;
    if (u < w0 || u >= w1) continue;
    const long long tr = u - r.pad_left;
    if (tr < 0 || tr >= r.t_raw) continue;
    float val = yk[t];
    if (u < e_prev) {
      const float a = 0.5f - 0.5f * cosf(3.14159265358979f * ((float)(u - w0) + 0.5f) / (float)v.overlap);
      val = (1.f - a) * yp[u - s_prev] + a * val;
    }
    ob[tr] = val;
  }
}

// grid (nb_max, C); part: [C][nb_max][2].  Every block of the row's grid line also zeroes its share of out[c][t_raw_c ..).
__global__ __launch_bounds__(1024) void seg_post_reduce_var_kernel(float* __restrict__ out, double* __restrict__ part,
                                                                   const SegRow* __restrict__ rows, long long row_stride,
                                                                   int nb_max) {
  __shared__ double shd[16];
  __shared__ float shf[16];
  const int j = blockIdx.x, c = blockIdx.y;
  const long long T_raw = rows[c].t_raw;
  float* xb = out + (size_t)c * row_stride;
  for (long long t = T_raw + (long long)j * 1024 + threadIdx.x; t < row_stride; t += (long long)nb_max * 1024) xb[t] = 0.f;
  const int nb = seg_nb(T_raw);
  if (j >= nb) return;
  double sq = 0;
  float mx = 0.f;
  for (long long t = (long long)j * 1024 + threadIdx.x; t < T_raw; t += (long long)nb * 1024) {
    const float x = xb[t];
    const double d = x;
    sq += d * d;
    mx = fmaxf(mx, fabsf(x));
  }
  sq = seg_block_sum(sq, shd);
  mx = seg_block_max(mx, shf);
  if (threadIdx.x == 0) { part[((size_t)c * nb_max + j) * 2 + 0] = sq; part[((size_t)c * nb_max + j) * 2 + 1] = (double)mx; }
}
__global__ __launch_bounds__(256) void seg_post_scale_var_kernel(float* __restrict__ out, const double* __restrict__ part,
                                                                 const float* __restrict__ stats, const SegRow* __restrict__ rows,
                                                                 long long row_stride, int nb_max, int keep_rms, int peak_guard) {
  const int c = blockIdx.y;
  const long long T_raw = rows[c].t_raw;
  const int nb = seg_nb(T_raw);
  const double* pc = part + (size_t)c * nb_max * 2;
  double sq = pc[0];
  float mxa = (float)pc[1];
  for (int i = 1; i < nb; i++) { sq += pc[i * 2]; mxa = fmaxf(mxa, (float)pc[i * 2 + 1]); }
  float g = 1.f;
  if (keep_rms) {
    const float x_rms = fmaxf((float)sqrt(sq / (double)T_raw), 1e-5f);
    g = stats[c * 4 + 2] / x_rms;
  }
  const float mx = mxa * g;
  const bool div = peak_guard && mx > 1.0f;
  if (!keep_rms && !div) return;
  float* xb = out + (size_t)c * row_stride;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < T_raw; t += (long long)gridDim.x * 256) {
    float x = xb[t] * g;
    if (div) x = x / mx;
    xb[t] = x;
  }
}


// ==== member-major forms (ou_enhance_segments_ensemble) =======================================================================
// A group runs E * Bw walk rows: row e * Bw + j is member e of entry e0 + j (entries past the last real one repeat it), and the
// long rows of the members are member-major too: row e * C + c.  grid.z = e.  The arithmetic per sample is that of the kernels
// above, so E = 1 gives their bits.  Rows are moved in 16-byte accesses from the first 16-byte boundary of the DESTINATION row
// on (the source side loads 16 bytes where it is aligned there as well, else four words); the up to 3 samples in front of it
// and behind the last whole quad go word by word.

__device__ __forceinline__ bool seg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// words from p to the next 16-byte boundary (p is 4-byte aligned)
__device__ __forceinline__ int seg_head_words(const void* p) { return (int)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2; }
__device__ __forceinline__ float4 seg_load4(const float* p) {
  if (seg_aligned16(p)) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

// z[e * Bw + j][t] = noise[e * C + c_j][s_j + t]   (one step's (E * C, T_pad) slice).  grid (ceil(L / 1024), Bw, E)
__global__ __launch_bounds__(256) void seg_gather_noise_mm_kernel(const float* __restrict__ noise, float* __restrict__ z,
                                                                  SegGeom g, long long e0, int C) {
  const int j = blockIdx.y, m = blockIdx.z, Bw = gridDim.y;
  long long e = e0 + j;
  if (e > g.n_entries - 1) e = g.n_entries - 1;
  const long long c = e / g.n_win, k = e - c * g.n_win;
  const float* src = noise + ((size_t)m * C + (size_t)c) * (size_t)g.T_pad + seg_start(g, k);
  float* dst = z + ((size_t)m * Bw + j) * (size_t)g.L;
  const long long head = seg_head_words(dst) < g.L ? seg_head_words(dst) : g.L;
  const long long nq = (g.L - head) >> 2;
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q < nq) *reinterpret_cast<float4*>(dst + head + 4 * q) = seg_load4(src + head + 4 * q);
  const long long rest = g.L - 4 * nq;  // head + tail: at most 6 words
  if (blockIdx.x == 0 && threadIdx.x < rest) {
    const long long t = threadIdx.x < head ? threadIdx.x : 4 * nq + threadIdx.x;
    dst[t] = src[t];
  }
}

// seg_stitch_kernel for walk row e * Bw + j with carry e (carry: (E, L)) into members row e * C + c_j.  Window-local columns
// [t0, t1) are what the entry writes: [w_k, w_{k+1}) of the padded row, cut to the raw row.  grid (ceil(L / 1024), n_real, E)
__global__ __launch_bounds__(256) void seg_stitch_mm_kernel(const float* __restrict__ y, const float* __restrict__ carry,
                                                            float* __restrict__ members, SegGeom g, long long e0, int Bw, int C) {
  const int j = blockIdx.y, m = blockIdx.z;
  const long long e = e0 + j;
  const long long c = e / g.n_win, k = e - c * g.n_win;
  const long long s = seg_start(g, k);
  const long long s_prev = k == 0 ? 0 : seg_start(g, k - 1);
  const long long w0 = k == 0 ? 0 : s_prev + g.L - g.overlap;
  const long long w1 = k == g.n_win - 1 ? g.T_pad : s + g.L - g.overlap;
  const long long e_prev = k == 0 ? 0 : s_prev + g.L;
  const float* yk = y + ((size_t)m * Bw + j) * (size_t)g.L;
  const float* yp = j > 0 ? yk - g.L : carry + (size_t)m * (size_t)g.L;
  float* ob = members + ((size_t)m * C + (size_t)c) * (size_t)g.T_raw;
  long long u0 = w0 > g.pad_left ? w0 : g.pad_left;  // padded-row positions [u0, u1) -> ob[u - pad_left]
  long long u1 = w1 < g.pad_left + g.T_raw ? w1 : g.pad_left + g.T_raw;
  if (u0 < s) u0 = s;
  if (u1 > s + g.L) u1 = s + g.L;
  const long long n = u1 - u0;
  if (n <= 0) return;
  auto value = [&](long long u, float v) {
    if (u < e_prev) {
      const float a = 0.5f - 0.5f * cosf(3.14159265358979f * ((float)(u - w0) + 0.5f) / (float)g.overlap);
      v = (1.f - a) * yp[u - s_prev] + a * v;
    }
    return v;
  };
  float* dst = ob + (u0 - g.pad_left);
  const float* src = yk + (u0 - s);
  const long long head = seg_head_words(dst) < n ? seg_head_words(dst) : n;
  const long long nq = (n - head) >> 2;
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q < nq) {
    const long long i = head + 4 * q;
    float4 v = seg_load4(src + i);
    v.x = value(u0 + i, v.x); v.y = value(u0 + i + 1, v.y); v.z = value(u0 + i + 2, v.z); v.w = value(u0 + i + 3, v.w);
    *reinterpret_cast<float4*>(dst + i) = v;
  }
  const long long rest = n - 4 * nq;
  if (blockIdx.x == 0 && threadIdx.x < rest) {
    const long long i = threadIdx.x < head ? threadIdx.x : 4 * nq + threadIdx.x;
    dst[i] = value(u0 + i, src[i]);
  }
}

// seg_post_scale_kernel over the E * C member rows: row r restores the mix_rms of its own input, statistics row r % C.  (The
// partials come from seg_post_reduce_kernel over E * C rows: it reads no statistics.)  grid (blocks, E * C)
__global__ __launch_bounds__(256) void seg_post_scale_mm_kernel(float* __restrict__ members, const double* __restrict__ part,
                                                                const float* __restrict__ stats, long long T_raw, int nb, int C,
                                                                int keep_rms, int peak_guard) {
  const int r = blockIdx.y;
  const double* pc = part + (size_t)r * nb * 2;
  double sq = pc[0];
  float mxa = (float)pc[1];
  for (int i = 1; i < nb; i++) { sq += pc[i * 2]; mxa = fmaxf(mxa, (float)pc[i * 2 + 1]); }
  float g = 1.f;
  if (keep_rms) {
    const float x_rms = fmaxf((float)sqrt(sq / (double)T_raw), 1e-5f);
    g = stats[(r % C) * 4 + 2] / x_rms;
  }
  const float mx = mxa * g;
  const bool div = peak_guard && mx > 1.0f;
  if (!keep_rms && !div) return;
  auto scale = [&](float x) {
    x = x * g;
    if (div) x = x / mx;
    return x;
  };
  float* xb = members + (size_t)r * (size_t)T_raw;
  const long long head = seg_head_words(xb) < T_raw ? seg_head_words(xb) : T_raw;
  const long long nq = (T_raw - head) >> 2;
  float4* xq = reinterpret_cast<float4*>(xb + head);
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long long)gridDim.x * 256) {
    float4 v = xq[q];
    v.x = scale(v.x); v.y = scale(v.y); v.z = scale(v.z); v.w = scale(v.w);
    xq[q] = v;
  }
  const long long rest = T_raw - 4 * nq;
  if (blockIdx.x == 0 && threadIdx.x < rest) {
    const long long t = threadIdx.x < head ? threadIdx.x : 4 * nq + threadIdx.x;
    xb[t] = scale(xb[t]);
  }
}

}  // namespace

int seg_reduce_blocks(long long T_raw) {
  long long nb = (T_raw + (1ll << 18) - 1) >> 18;  // one block per 256 Ki samples: one block per row up to 16 s at 16 kHz
  return (int)(nb < 1 ? 1 : nb > 1024 ? 1024 : nb);
}

hipError_t launch_seg_stats(const float* mix, double* part, float* stats, int C, long long T_raw, long long T_pad, float level,
                            hipStream_t st) {
  const int nb = seg_reduce_blocks(T_raw);
  hipLaunchKernelGGL(seg_stats1_kernel, dim3(nb, C), dim3(1024), 0, st, mix, part, T_raw, nb);
  hipLaunchKernelGGL(seg_stats2_kernel, dim3(nb, C), dim3(1024), 0, st, mix, part, T_raw, T_pad, nb);
  hipLaunchKernelGGL(seg_stats_finish_kernel, dim3(C), dim3(64), 0, st, part, stats, T_raw, T_pad, nb, level);
  return hipGetLastError();
}
hipError_t launch_seg_mel_energy(const float* mix, const float* stats, const float* win, const float* tw, const float* fb,
                                 float* esum, int C, long long T_raw, long long T_pad, long long pad_left, int n_fft, int hop,
                                 int mel_pad, int n_freq, int n_mels, long long L, hipStream_t st) {
  if (L > 0x7fffffffll) return hipErrorInvalidValue;
  const size_t smem = (size_t)(3 * n_fft + n_freq) * 4;
  hipLaunchKernelGGL(seg_mel_energy_kernel, dim3((unsigned)L, C), dim3(512), smem, st, mix, stats, win, tw, fb, esum, T_raw,
                     T_pad, pad_left, n_fft, hop, mel_pad, n_freq, n_mels, L);
  return hipGetLastError();
}
hipError_t launch_seg_gather_input(const float* mix, const float* stats, const float* row_mel_scale, float* mixn,
                                   float* mel_scale, const SegGeom& g, long long e0, int B, hipStream_t st) {
  hipLaunchKernelGGL(seg_gather_input_kernel, dim3((unsigned)((g.L + 1023) / 1024), B), dim3(256), 0, st, mix, stats,
                     row_mel_scale, mixn, mel_scale, g, e0);
  return hipGetLastError();
}
hipError_t launch_seg_gather_noise(const float* noise, float* z, const SegGeom& g, long long e0, int B, hipStream_t st) {
  hipLaunchKernelGGL(seg_gather_noise_kernel, dim3((unsigned)((g.L + 1023) / 1024), B), dim3(256), 0, st, noise, z, g, e0);
  return hipGetLastError();
}
hipError_t launch_seg_stitch(const float* y, const float* carry, float* out, const SegGeom& g, long long e0, int n_real,
                             hipStream_t st) {
  hipLaunchKernelGGL(seg_stitch_kernel, dim3((unsigned)((g.L + 1023) / 1024), n_real), dim3(256), 0, st, y, carry, out, g, e0);
  return hipGetLastError();
}
hipError_t launch_seg_post(float* out, double* part, const float* stats, int C, long long T_raw, int keep_rms, int peak_guard,
                           hipStream_t st) {
  const int nb = seg_reduce_blocks(T_raw);
  hipLaunchKernelGGL(seg_post_reduce_kernel, dim3(nb, C), dim3(1024), 0, st, out, part, T_raw, nb);
  long long nsb = (T_raw + 256 * 64 - 1) / (256 * 64);  // ~64 samples per thread
  if (nsb > 8192) nsb = 8192;
  hipLaunchKernelGGL(seg_post_scale_kernel, dim3((unsigned)nsb, C), dim3(256), 0, st, out, part, stats, T_raw, nb, keep_rms,
                     peak_guard);
  return hipGetLastError();
}

// ---- rows of lengths of their own ----------------------------------------------------------------------------------------------
hipError_t launch_seg_upload_rows(SegRow* rows, const SegRowBlock& blk, int n, int off, const SegVar& v, hipStream_t st) {
  if (n < 1 || n > kSegRowsPerLaunch) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_upload_rows_kernel, dim3(1), dim3(64), 0, st, rows, blk, n, off, v);
  return hipGetLastError();
}
hipError_t launch_seg_upload_lens(int* lens, const SegEntryBlock& blk, int n, int j0, int B, const LevelSpec& lv, hipStream_t st) {
  if (n < 1 || n > kSegEntriesPerLaunch || j0 < 0 || j0 + n > B) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_upload_lens_kernel, dim3(1), dim3(64), 0, st, lens, blk, n, j0, B, lv);
  return hipGetLastError();
}
hipError_t launch_seg_stats_var(const float* mix, double* part, float* stats, const SegRow* rows, int C, long long T_raw_max,
                                float level, hipStream_t st) {
  const int nb = seg_reduce_blocks(T_raw_max);
  hipLaunchKernelGGL(seg_stats1_var_kernel, dim3(nb, C), dim3(1024), 0, st, mix, part, rows, T_raw_max, nb);
  hipLaunchKernelGGL(seg_stats2_var_kernel, dim3(nb, C), dim3(1024), 0, st, mix, part, rows, T_raw_max, nb);
  hipLaunchKernelGGL(seg_stats_finish_var_kernel, dim3(C), dim3(64), 0, st, part, stats, rows, nb, level);
  return hipGetLastError();
}
hipError_t launch_seg_mel_energy_var(const float* mix, const float* stats, const float* win, const float* tw, const float* fb,
                                     float* esum, const SegRow* rows, int C, long long row_stride, int n_fft, int hop, int mel_pad,
                                     int n_freq, int n_mels, long long frames_max, hipStream_t st) {
  if (frames_max < 1 || frames_max > 0x7fffffffll) return hipErrorInvalidValue;
  const size_t smem = (size_t)(3 * n_fft + n_freq) * 4;
  hipLaunchKernelGGL(seg_mel_energy_var_kernel, dim3((unsigned)frames_max, C), dim3(512), smem, st, mix, stats, win, tw, fb, esum,
                     rows, row_stride, n_fft, hop, mel_pad, n_freq, n_mels);
  return hipGetLastError();
}
hipError_t launch_seg_mel_scale_var(const float* esum, float* scale, const SegRow* rows, int C, long long row_stride,
                                    hipStream_t st) {
  hipLaunchKernelGGL(seg_mel_scale_var_kernel, dim3(C), dim3(256), 0, st, esum, scale, rows, row_stride);
  return hipGetLastError();
}
hipError_t launch_seg_gather_input_var(const float* mix, const float* stats, const float* row_mel_scale, const SegRow* rows,
                                       float* mixn, float* mel_scale, const SegEntryBlock& blk, int n, int j0, long long T,
                                       const SegVar& v, hipStream_t st) {
  if (n < 1 || n > kSegEntriesPerLaunch || T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_gather_input_var_kernel, dim3((unsigned)((T + 1023) / 1024), n), dim3(256), 0, st, mix, stats,
                     row_mel_scale, rows, mixn, mel_scale, blk, j0, T, v);
  return hipGetLastError();
}
hipError_t launch_seg_gather_noise_var(const float* noise, const SegRow* rows, float* z, const SegEntryBlock& blk, int n, int j0,
                                       long long T, const SegVar& v, hipStream_t st) {
  if (n < 1 || n > kSegEntriesPerLaunch || T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_gather_noise_var_kernel, dim3((unsigned)((T + 1023) / 1024), n), dim3(256), 0, st, noise, rows, z, blk,
                     j0, T, v);
  return hipGetLastError();
}
hipError_t launch_seg_stitch_var(const float* y, const float* carry, float* out, const SegRow* rows, const SegEntryBlock& blk,
                                 int n, int j0, long long T, const SegVar& v, hipStream_t st) {
  if (n < 1 || n > kSegEntriesPerLaunch || T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_stitch_var_kernel, dim3((unsigned)((T + 1023) / 1024), n), dim3(256), 0, st, y, carry, out, rows, blk, j0,
                     T, v);
  return hipGetLastError();
}
hipError_t launch_seg_post_var(float* out, double* part, const float* stats, const SegRow* rows, int C, long long T_raw_max,
                               int keep_rms, int peak_guard, hipStream_t st) {
  const int nb = seg_reduce_blocks(T_raw_max);
  hipLaunchKernelGGL(seg_post_reduce_var_kernel, dim3(nb, C), dim3(1024), 0, st, out, part, rows, T_raw_max, nb);
  long long nsb = (T_raw_max + 256 * 64 - 1) / (256 * 64);
  if (nsb > 8192) nsb = 8192;
  hipLaunchKernelGGL(seg_post_scale_var_kernel, dim3((unsigned)nsb, C), dim3(256), 0, st, out, part, stats, rows, T_raw_max, nb,
                     keep_rms, peak_guard);
  return hipGetLastError();
}

// ---- member-major forms ----------------------------------------------------------------------------------------------------------
static bool seg_mm_grid_ok(const SegGeom& g, int rows_y, int E) {
  return g.L >= 1 && (g.L + 1023) / 1024 <= 0x7fffffffll && rows_y >= 1 && rows_y <= 65535 && E >= 1 && E <= 65535;
}
hipError_t launch_seg_gather_noise_mm(const float* noise, float* z, const SegGeom& g, long long e0, int Bw, int E, int C,
                                      hipStream_t st) {
  if (!seg_mm_grid_ok(g, Bw, E) || C < 1 || e0 < 0 || e0 >= g.n_entries) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_gather_noise_mm_kernel, dim3((unsigned)((g.L + 1023) / 1024), Bw, E), dim3(256), 0, st, noise, z, g, e0,
                     C);
  return hipGetLastError();
}
hipError_t launch_seg_stitch_mm(const float* y, const float* carry, float* members, const SegGeom& g, long long e0, int n_real,
                                int Bw, int E, int C, hipStream_t st) {
  if (!seg_mm_grid_ok(g, n_real, E) || n_real > Bw || C < 1 || e0 < 0 || e0 + n_real > g.n_entries) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_stitch_mm_kernel, dim3((unsigned)((g.L + 1023) / 1024), n_real, E), dim3(256), 0, st, y, carry, members,
                     g, e0, Bw, C);
  return hipGetLastError();
}
hipError_t launch_seg_post_mm(float* members, double* part, const float* stats, int E, int C, long long T_raw, int keep_rms,
                              int peak_guard, hipStream_t st) {
  if (E < 1 || C < 1 || (long long)E * C > 65535 || T_raw < 1) return hipErrorInvalidValue;
  const int nb = seg_reduce_blocks(T_raw);
  hipLaunchKernelGGL(seg_post_reduce_kernel, dim3(nb, E * C), dim3(1024), 0, st, members, part, T_raw, nb);
  long long nsb = (T_raw + 256 * 64 - 1) / (256 * 64);  // ~64 samples per thread
  if (nsb > 8192) nsb = 8192;
  hipLaunchKernelGGL(seg_post_scale_mm_kernel, dim3((unsigned)nsb, E * C), dim3(256), 0, st, members, part, stats, T_raw, nb, C,
                     keep_rms, peak_guard);
  return hipGetLastError();
}

}  // namespace ou
