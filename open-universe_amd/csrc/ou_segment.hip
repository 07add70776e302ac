// Segmented enhance (ou_enhance_segments): whole-file statistics, window gathers, crossfade stitch and post step over LONG
// rows.  Every index into a long row is 64-bit and no kernel here builds a buffer descriptor, so nothing wraps past 2^32 bytes
// per row.  Reductions run in a fixed order (per-block partials in double, summed in block order by whoever needs the
// total): two runs give the same bits.  With one block per row the order is exactly that of pad_normalize_kernel /
// post_kernel, so a file that fits into one window gets the whole-file call's statistics bit for bit.
// Every operation is one kernel body, a template over the rows of the call (SegRowsAlike | SegRowsTable) and the entries of a
// group (SegEntriesArith | SegEntriesList), ou_kernels.h: where the rows are alike the numbers are kernel arguments, else they
// come from a device table, a group's entries (row, window, length) from the kernel arguments, and every row reduces over the
// block partition of the call on that row alone.  Grids are sized by the longest row; a block beyond the row's own share returns
// before it touches memory (with rows alike there is none).
#include "ou_dev.h"
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

// start of window k of row r, whose entries are `len` long: k * hop, the last one shifted to end at T_pad (one window: 0)
__device__ __forceinline__ long long seg_start(const SegRow& r, long long k, long long len, long long hop) {
  return k < r.n_win - 1 ? k * hop : r.T_pad - len;
}
// Entry k of a row writes the samples [w0, w1) = [w_k, w_{k+1}) of the padded row (w_0 = 0, w_k = e_{k-1} - O, w_n = T_pad,
// e_k = end of window k).  On [w0, e_prev) it crossfades with window k - 1, which starts at s_prev: weight a(i) = 0.5 - 0.5
// cos(pi (i + 0.5) / O) for window k, 1 - a(i) for window k - 1.
struct SegWindow {
  long long s, s_prev, w0, w1, e_prev, overlap;
  __device__ SegWindow(const SegRow& r, const SegEnt& e, long long hop, long long overlap_) : overlap(overlap_) {
    s = seg_start(r, e.win, e.len, hop);
    s_prev = e.win == 0 ? 0 : seg_start(r, e.win - 1, e.len, hop);
    w0 = e.win == 0 ? 0 : s_prev + e.len - overlap;
    w1 = e.win == r.n_win - 1 ? r.T_pad : s + e.len - overlap;
    e_prev = e.win == 0 ? 0 : s_prev + e.len;
  }
  // the sample at position u of the padded row: v from window k, crossfaded with window k - 1 (yp) where they overlap
  __device__ float value(long long u, float v, const float* yp) const {
    if (u < e_prev) v = crossfade(u - w0, overlap, yp[u - s_prev], v);
    return v;
  }
};

// The 16-byte row mover.  The n words at dst are written in 16-byte accesses from the first 16-byte boundary of dst on (a source
// loads 16 bytes where it is aligned there as well, else four words: seg_load4); the up to 3 words in front of it and behind the
// last whole quad go word by word, in block 0.  quad(i) -> the float4 for words [i, i + 4), word(i) -> word i.  blockDim.x = 256.
__device__ __forceinline__ bool seg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__device__ __forceinline__ float4 seg_load4(const float* p) {
  if (seg_aligned16(p)) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
template <class Quad, class Word>
__device__ __forceinline__ void seg_move_row(float* dst, long long n, Quad quad, Word word) {
  long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) >> 2;  // words to the boundary
  if (head > n) head = n;
  const long long nq = (n - head) >> 2;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long long)gridDim.x * 256)
    *reinterpret_cast<float4*>(dst + head + 4 * q) = quad(head + 4 * q);
  const long long rest = n - 4 * nq;  // head + tail: at most 6 words
  if (blockIdx.x == 0 && threadIdx.x < rest) {
    const long long i = threadIdx.x < head ? threadIdx.x : 4 * nq + threadIdx.x;
    dst[i] = word(i);
  }
}

// ---- whole-row statistics (utils/norm.py:47-87, universe.py:259) -------------------------------------------------------
// pass 1: per-block sum and sum of squares of the raw row.  grid (part_stride, C); part: [C][part_stride][3]
template <class Rows>
__global__ __launch_bounds__(1024) void seg_stats1_kernel(const float* __restrict__ mix, double* __restrict__ part, Rows rows) {
  __shared__ double shd[16];
  const int j = blockIdx.x, c = blockIdx.y;
  const SegRow r = rows.row(c);
  const int nb = rows.blocks(r);
  if (j >= nb) return;
  const float* xb = mix + (size_t)c * rows.stride();
  double s = 0, sq = 0;
  for (long long t = (long long)j * 1024 + threadIdx.x; t < r.t_raw; t += (long long)nb * 1024) {
    const double d = xb[t];
    s += d; sq += d * d;
  }
  s = seg_block_sum(s, shd);
  sq = seg_block_sum(sq, shd);
  double* pc = part + ((size_t)c * rows.part_stride() + j) * 3;
  if (threadIdx.x == 0) { pc[0] = s; pc[1] = sq; }
}
// (pass 1 is the same for every NormMode: the raw sums do not depend on it)
// pass 2: per-block sum of (x - mean)^2 around the mean of the padded row (each block sums the partials of pass 1 in order).
// GEN (any NormMode, ou_kernels.h; false: norm 2 with zero_mean, `nm` not looked at): also the block's max |x - mu|, mu = mean
// or 0, into pmax[c][j] behind the [C][part_stride][3] sums -- formed and stored for every mode that is not plain(), zero_mean
// false under norm 2 included (which never reads it); the area holds the fourth partial for every handle.  A maximum does not depend on the order it is taken in: whatever
// the number of blocks, the finish kernel's maximum over them has the bits of pad_normalize_kernel's over one.
template <class Rows, bool GEN>
__global__ __launch_bounds__(1024) void seg_stats2_kernel(const float* __restrict__ mix, double* __restrict__ part, Rows rows,
                                                          NormMode nm) {
  __shared__ double shd[16];
  __shared__ float shf[GEN ? 16 : 1];
  const int j = blockIdx.x, c = blockIdx.y;
  const SegRow r = rows.row(c);
  const int nb = rows.blocks(r);
  if (j >= nb) return;
  double* pc = part + (size_t)c * rows.part_stride() * 3;
  double s = pc[0];
  for (int i = 1; i < nb; i++) s += pc[i * 3];
  const float mean = (float)(s / (double)r.T_pad);  // norm.py:62  (mean over the padded signal)
  const float* xb = mix + (size_t)c * rows.stride();
  const float mu = GEN && !nm.zero_mean ? 0.f : mean;
  double ss = 0;
  float mx = 0.f;
  for (long long t = (long long)j * 1024 + threadIdx.x; t < r.t_raw; t += (long long)nb * 1024) {
    const double d = (double)(xb[t] - mean);
    ss += d * d;
    if constexpr (GEN) mx = fmaxf(mx, fabsf(xb[t] - mu));
  }
  ss = seg_block_sum(ss, shd);
  if (threadIdx.x == 0) pc[j * 3 + 2] = ss;
  if constexpr (GEN) {
    mx = seg_block_max(mx, shf);
    double* pmax = part + (size_t)gridDim.y * rows.part_stride() * 3;
    if (threadIdx.x == 0) pmax[(size_t)c * rows.part_stride() + j] = (double)mx;
  }
}
// finish: stats[c] = {mean, gain, mix_rms, 0}  (the layout of pad_normalize_kernel's stats)
template <class Rows, bool GEN>
__global__ void seg_stats_finish_kernel(const double* __restrict__ part, float* __restrict__ stats, Rows rows, float level,
                                        NormMode nm) {
  const int c = blockIdx.x;
  if (threadIdx.x != 0) return;
  const SegRow r = rows.row(c);
  const int nb = rows.blocks(r);
  const double* pc = part + (size_t)c * rows.part_stride() * 3;
  double s = pc[0], sq = pc[1], ss = pc[2];
  for (int i = 1; i < nb; i++) { s += pc[i * 3]; sq += pc[i * 3 + 1]; ss += pc[i * 3 + 2]; }
  const float mean = (float)(s / (double)r.T_pad);
  ss += (double)(r.T_pad - r.t_raw) * (double)(0.f - mean) * (double)(0.f - mean);
  float sd = (float)sqrt(ss / (double)(r.T_pad - 1));  // unbiased std, norm.py:22-23
  const float mu = GEN && !nm.zero_mean ? 0.f : mean;
  float gain;
  if constexpr (GEN) {
    const double* pmax = part + (size_t)gridDim.x * rows.part_stride() * 3 + (size_t)c * rows.part_stride();
    float mx = (float)pmax[0];
    for (int i = 1; i < nb; i++) mx = fmaxf(mx, (float)pmax[i]);
    if (r.T_pad > r.t_raw) mx = fmaxf(mx, fabsf(0.f - mu));  // norm.py:26-28 over the padded row
    gain = nm.gain(level, sd, mx);
  } else {
    sd = fmaxf(sd, 1e-5f);
    gain = level / sd;
  }
  stats[c * 4 + 0] = mu;
  stats[c * 4 + 1] = gain;
  stats[c * 4 + 2] = (float)sqrt(sq / (double)r.t_raw);
  stats[c * 4 + 3] = 0.f;
}

// ---- whole-row mel normalisation (condition.py:105-106) ----------------------------------------------------------------
// The frame energies of mel_kernel over the whole normalised row, without the mel output: the normalisation (x - mean) * gain
// and the pad split are applied on the fly to the raw row.  Same arithmetic, same order as mel_kernel.  grid (frames_max, C)
template <class Rows>
__global__ __launch_bounds__(512) void seg_mel_energy_kernel(const float* __restrict__ mix, const float* __restrict__ stats,
                                                             const float* __restrict__ win, const float* __restrict__ tw,
                                                             const float* __restrict__ fb, float* __restrict__ esum, Rows rows,
                                                             int n_fft, int hop, int mel_pad, int n_freq, int n_mels) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* sx = sm;
  float* tc = sx + n_fft;
  float* ts = tc + n_fft;
  float* pw = ts + n_fft;
  __shared__ float shf[8];
  const long long f = blockIdx.x;
  const int c = blockIdx.y, tid = threadIdx.x;
  const SegRow r = rows.row(c);
  if (f >= r.frames) return;
  const float mean = stats[c * 4 + 0], gain = stats[c * 4 + 1];
  const float* xb = mix + (size_t)c * rows.stride();
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
  if (tid == 0) esum[(size_t)c * rows.frame_stride() + f] = e;
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

// ---- window gathers ----------------------------------------------------------------------------------------------------
// Entry i of the launch, row j = slot(i) of mixn (.., T): mixn[j][t] = (x[c][s + t - pad_left] - mean_c) * gain_c (0 outside the
// raw row: the whole-row pad split; 0 from the entry's own length on), and mel_scale[j] = the whole-row mel scale of row c.
// Word by word: bounds and arithmetic are per sample.  grid (ceil(T / 1024), n)
template <class Rows, class Entries>
__global__ __launch_bounds__(256) void seg_gather_input_kernel(const float* __restrict__ mix, const float* __restrict__ stats,
                                                               const float* __restrict__ row_mel_scale, float* __restrict__ mixn,
                                                               float* __restrict__ mel_scale, Rows rows, Entries ents,
                                                               long long T) {
  const int j = ents.slot(blockIdx.y);
  const SegEnt e = ents.entry(blockIdx.y);
  const SegRow r = rows.row(e.row);
  const long long s = seg_start(r, e.win, e.len, ents.hop);
  const float mean = stats[e.row * 4 + 0], gain = stats[e.row * 4 + 1];
  const float* xb = mix + (size_t)e.row * rows.stride();
  float* yb = mixn + (size_t)j * T;
  for (long long t = (long long)blockIdx.x * 1024 + threadIdx.x; t < (long long)(blockIdx.x + 1) * 1024 && t < T; t += 256) {
    float y = 0.f;
    if (t < e.len) {
      const long long tr = s + t - r.pad_left;
      const float x = (tr >= 0 && tr < r.t_raw) ? xb[tr] : 0.f;
      y = (x - mean) * gain;
    }
    yb[t] = y;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) mel_scale[j] = row_mel_scale[e.row];
}
// z[m * Bw + j][t] = noise[m * C + c][s + t] for t < len, 0 from there to T   (one step's (E * C, noise_stride) slice).
// grid (ceil(T / 1024), n, E)
template <class Rows, class Entries>
__global__ __launch_bounds__(256) void seg_gather_noise_kernel(const float* __restrict__ noise, float* __restrict__ z, Rows rows,
                                                               Entries ents, long long T, int Bw, int C) {
  const int j = ents.slot(blockIdx.y), m = blockIdx.z;
  const SegEnt e = ents.entry(blockIdx.y);
  const SegRow r = rows.row(e.row);
  const float* src = noise + ((size_t)m * C + (size_t)e.row) * (size_t)rows.noise_stride() + seg_start(r, e.win, e.len, ents.hop);
  float* dst = z + ((size_t)m * Bw + j) * (size_t)T;
  auto word = [&](long long t) { return t < e.len ? src[t] : 0.f; };
  seg_move_row(dst, T, [&](long long t) {
    return t + 4 <= e.len ? seg_load4(src + t) : make_float4(word(t), word(t + 1), word(t + 2), word(t + 3));
  }, word);
}

// ---- crossfade stitch ----------------------------------------------------------------------------------------------------
// Walk row m * Bw + j (j = slot) of y, with row j - 1 in front of it or -- j = 0 -- carry row m, into long row m * C + c.  The
// entry writes the window-local columns [u0 - s, u1 - s): [w0, w1) of the padded row, cut to the raw row and to the window.
// grid (ceil(T / 1024), n, E)
template <class Rows, class Entries>
__global__ __launch_bounds__(256) void seg_stitch_kernel(const float* __restrict__ y, const float* __restrict__ carry,
                                                         float* __restrict__ out, Rows rows, Entries ents, long long T, int Bw,
                                                         int C) {
  const int j = ents.slot(blockIdx.y), m = blockIdx.z;
  const SegEnt e = ents.entry(blockIdx.y);
  const SegRow r = rows.row(e.row);
  const SegWindow w(r, e, ents.hop, ents.overlap);
  const float* yk = y + ((size_t)m * Bw + j) * (size_t)T;
  const float* yp = j > 0 ? yk - T : carry + (size_t)m * (size_t)T;
  float* ob = out + ((size_t)m * C + (size_t)e.row) * (size_t)rows.stride();
  long long u0 = w.w0 > r.pad_left ? w.w0 : r.pad_left;  // padded-row positions [u0, u1) -> ob[u - pad_left]
  long long u1 = w.w1 < r.pad_left + r.t_raw ? w.w1 : r.pad_left + r.t_raw;
  if (u0 < w.s) u0 = w.s;
  if (u1 > w.s + e.len) u1 = w.s + e.len;
  if (u1 <= u0) return;
  const float* src = yk + (u0 - w.s);
  seg_move_row(ob + (u0 - r.pad_left), u1 - u0, [&](long long i) {
    float4 v = seg_load4(src + i);
    v.x = w.value(u0 + i, v.x, yp); v.y = w.value(u0 + i + 1, v.y, yp);
    v.z = w.value(u0 + i + 2, v.z, yp); v.w = w.value(u0 + i + 3, v.w, yp);
    return v;
  }, [&](long long i) { return w.value(u0 + i, src[i], yp); });
}

// ---- post step over whole rows (universe.py:349-357) -------------------------------------------------------------------
// per-block sum of squares (double) and max |x| of long row q (its length: that of row q % C); rows shorter than the stride are
// zeroed behind their own samples by every block of the grid line.  grid (part_stride, E * C); part: [E * C][part_stride][2]
template <class Rows>
__global__ __launch_bounds__(1024) void seg_post_reduce_kernel(float* __restrict__ out, double* __restrict__ part, Rows rows,
                                                               int C) {
  __shared__ double shd[16];
  __shared__ float shf[16];
  const int j = blockIdx.x, q = blockIdx.y;
  const SegRow r = rows.row(q % C);
  float* xb = out + (size_t)q * (size_t)rows.stride();
  if (Rows::zero_tail)
    for (long long t = r.t_raw + (long long)j * 1024 + threadIdx.x; t < rows.stride(); t += (long long)gridDim.x * 1024) xb[t] = 0.f;
  const int nb = rows.blocks(r);
  if (j >= nb) return;
  double sq = 0;
  float mx = 0.f;
  for (long long t = (long long)j * 1024 + threadIdx.x; t < r.t_raw; t += (long long)nb * 1024) {
    const float v = xb[t];
    const double d = v;
    sq += d * d;
    mx = fmaxf(mx, fabsf(v));
  }
  sq = seg_block_sum(sq, shd);
  mx = seg_block_max(mx, shf);
  double* pc = part + ((size_t)q * rows.part_stride() + j) * 2;
  if (threadIdx.x == 0) { pc[0] = sq; pc[1] = (double)mx; }
}
// keep_rms gain g = mix_rms / max(x_rms, 1e-5) with the mix_rms of statistics row q % C, peak m = max|x| * g (rounding is
// monotonic: = max|x * g|), x <- x * g [/ m].  grid (blocks, E * C)
template <class Rows>
__global__ __launch_bounds__(256) void seg_post_scale_kernel(float* __restrict__ out, const double* __restrict__ part,
                                                             const float* __restrict__ stats, Rows rows, int C, int keep_rms,
                                                             int peak_guard) {
  const int q = blockIdx.y;
  const SegRow r = rows.row(q % C);
  const int nb = rows.blocks(r);
  const double* pc = part + (size_t)q * rows.part_stride() * 2;
  double sq = pc[0];
  float mxa = (float)pc[1];
  for (int i = 1; i < nb; i++) { sq += pc[i * 2]; mxa = fmaxf(mxa, (float)pc[i * 2 + 1]); }
  float g = 1.f;
  if (keep_rms) {
    const float x_rms = fmaxf((float)sqrt(sq / (double)r.t_raw), 1e-5f);
    g = stats[(q % C) * 4 + 2] / x_rms;
  }
  const float mx = mxa * g;
  const bool div = peak_guard && mx > 1.0f;
  if (!keep_rms && !div) return;
  auto scale = [&](float x) {
    x = x * g;
    if (div) x = x / mx;
    return x;
  };
  float* xb = out + (size_t)q * (size_t)rows.stride();
  seg_move_row(xb, r.t_raw, [&](long long i) {
    float4 v = *reinterpret_cast<const float4*>(xb + i);
    v.x = scale(v.x); v.y = scale(v.y); v.z = scale(v.z); v.w = scale(v.w);
    return v;
  }, [&](long long i) { return scale(xb[i]); });
}

// ---- the SegRow table and a ragged group's per-level lengths, from kernel arguments -------------------------------------------
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
// (member m = blockIdx.x writes walk rows m * Bw + j0 + i of the [level][E * Bw] table: member rows repeat their entry's lengths)
__global__ void seg_upload_lens_kernel(int* lens, SegEntryBlock blk, int n, int j0, int Bw, LevelSpec lv) {
  const int i = threadIdx.x, m = blockIdx.x, B = (int)gridDim.x * Bw;
  if (i >= n) return;
  for (int l = 0; l < lv.n; l++) lens[l * B + m * Bw + j0 + i] = (int)((long long)blk.len[i] * lv.num[l] / lv.den[l]);
}

// ---- what the launch wrappers check ------------------------------------------------------------------------------------------
// entries [0, n) of the launch exist (`real`: none of them may be a filler past the last entry)
bool seg_entries_ok(const SegEntriesArith& a, int n, bool real) {
  return a.L >= 1 && a.n_win >= 1 && a.e0 >= 0 && a.e0 < a.n_entries && (!real || a.e0 + n <= a.n_entries);
}
bool seg_entries_ok(const SegEntriesList& l, int n, bool) { return n <= kSegEntriesPerLaunch && l.j0 >= 0; }
// grid (ceil(T / 1024), n, E) of the per-entry kernels, whose walk has Bw rows per member; false: not launchable
template <class Entries>
bool seg_entry_grid(const Entries& ents, int n, bool real, long long T, int Bw, int E, int C, dim3& grid) {
  if (T < 1 || (T + 1023) / 1024 > 0x7fffffffll || n < 1 || n > 65535 || ents.slot(n - 1) >= Bw || E < 1 || E > 65535 || C < 1 ||
      !seg_entries_ok(ents, n, real))
    return false;
  grid = dim3((unsigned)((T + 1023) / 1024), n, E);
  return true;
}

}  // namespace

template <class Rows>
hipError_t launch_seg_stats(const float* mix, double* part, float* stats, const Rows& rows, int C, float level, const NormMode& nm,
                            hipStream_t st) {
  if (C < 1 || C > 65535 || rows.stride() < 1) return hipErrorInvalidValue;
  const dim3 grid(rows.part_stride(), C);
  hipLaunchKernelGGL(seg_stats1_kernel<Rows>, grid, dim3(1024), 0, st, mix, part, rows);
  if (nm.plain()) {
    hipLaunchKernelGGL((seg_stats2_kernel<Rows, false>), grid, dim3(1024), 0, st, mix, part, rows, nm);
    hipLaunchKernelGGL((seg_stats_finish_kernel<Rows, false>), dim3(C), dim3(64), 0, st, part, stats, rows, level, nm);
  } else {
    hipLaunchKernelGGL((seg_stats2_kernel<Rows, true>), grid, dim3(1024), 0, st, mix, part, rows, nm);
    hipLaunchKernelGGL((seg_stats_finish_kernel<Rows, true>), dim3(C), dim3(64), 0, st, part, stats, rows, level, nm);
  }
  return hipGetLastError();
}
template <class Rows>
hipError_t launch_seg_mel_energy(const float* mix, const float* stats, const float* win, const float* tw, const float* fb,
                                 float* esum, const Rows& rows, int C, int n_fft, int hop, int mel_pad, int n_freq, int n_mels,
                                 long long frames_max, hipStream_t st) {
  if (C < 1 || C > 65535 || frames_max < 1 || frames_max > 0x7fffffffll) return hipErrorInvalidValue;
  const size_t smem = (size_t)(3 * n_fft + n_freq) * 4;
  hipLaunchKernelGGL(seg_mel_energy_kernel<Rows>, dim3((unsigned)frames_max, C), dim3(512), smem, st, mix, stats, win, tw, fb, esum,
                     rows, n_fft, hop, mel_pad, n_freq, n_mels);
  return hipGetLastError();
}
hipError_t launch_seg_mel_scale_var(const float* esum, float* scale, const SegRow* rows, int C, long long row_stride,
                                    hipStream_t st) {
  hipLaunchKernelGGL(seg_mel_scale_var_kernel, dim3(C), dim3(256), 0, st, esum, scale, rows, row_stride);
  return hipGetLastError();
}
template <class Rows, class Entries>
hipError_t launch_seg_gather_input(const float* mix, const float* stats, const float* row_mel_scale, float* mixn,
                                   float* mel_scale, const Rows& rows, const Entries& ents, int n, long long T, hipStream_t st) {
  dim3 grid;
  if (!seg_entry_grid(ents, n, false, T, 0x7fffffff, 1, 1, grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((seg_gather_input_kernel<Rows, Entries>), grid, dim3(256), 0, st, mix, stats, row_mel_scale, mixn, mel_scale,
                     rows, ents, T);
  return hipGetLastError();
}
template <class Rows, class Entries>
hipError_t launch_seg_gather_noise(const float* noise, float* z, const Rows& rows, const Entries& ents, int n, long long T, int Bw,
                                   int E, int C, hipStream_t st) {
  dim3 grid;
  if (!seg_entry_grid(ents, n, false, T, Bw, E, C, grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((seg_gather_noise_kernel<Rows, Entries>), grid, dim3(256), 0, st, noise, z, rows, ents, T, Bw, C);
  return hipGetLastError();
}
template <class Rows, class Entries>
hipError_t launch_seg_stitch(const float* y, const float* carry, float* out, const Rows& rows, const Entries& ents, int n,
                             long long T, int Bw, int E, int C, hipStream_t st) {
  dim3 grid;
  if (!seg_entry_grid(ents, n, true, T, Bw, E, C, grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((seg_stitch_kernel<Rows, Entries>), grid, dim3(256), 0, st, y, carry, out, rows, ents, T, Bw, C);
  return hipGetLastError();
}
template <class Rows>
hipError_t launch_seg_post(float* out, double* part, const float* stats, const Rows& rows, int E, int C, int keep_rms,
                           int peak_guard, hipStream_t st) {
  if (E < 1 || C < 1 || (long long)E * C > 65535 || rows.stride() < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_post_reduce_kernel<Rows>, dim3(rows.part_stride(), E * C), dim3(1024), 0, st, out, part, rows, C);
  long long nsb = (rows.stride() + 256 * 64 - 1) / (256 * 64);  // ~64 samples per thread
  if (nsb > 8192) nsb = 8192;
  hipLaunchKernelGGL(seg_post_scale_kernel<Rows>, dim3((unsigned)nsb, E * C), dim3(256), 0, st, out, part, stats, rows, C, keep_rms,
                     peak_guard);
  return hipGetLastError();
}
// the two calls there are: rows alike with arithmetic entries, a table of rows with listed entries
#define OU_SEG_INSTANTIATE(Rows, Entries)                                                                                          \
  template hipError_t launch_seg_stats<Rows>(const float*, double*, float*, const Rows&, int, float, const NormMode&, hipStream_t);                 \
  template hipError_t launch_seg_mel_energy<Rows>(const float*, const float*, const float*, const float*, const float*, float*,    \
                                                  const Rows&, int, int, int, int, int, int, long long, hipStream_t);              \
  template hipError_t launch_seg_gather_input<Rows, Entries>(const float*, const float*, const float*, float*, float*, const Rows&, \
                                                             const Entries&, int, long long, hipStream_t);                         \
  template hipError_t launch_seg_gather_noise<Rows, Entries>(const float*, float*, const Rows&, const Entries&, int, long long,    \
                                                             int, int, int, hipStream_t);                                          \
  template hipError_t launch_seg_stitch<Rows, Entries>(const float*, const float*, float*, const Rows&, const Entries&, int,       \
                                                       long long, int, int, int, hipStream_t);                                     \
  template hipError_t launch_seg_post<Rows>(float*, double*, const float*, const Rows&, int, int, int, int, hipStream_t);
OU_SEG_INSTANTIATE(SegRowsAlike, SegEntriesArith)
OU_SEG_INSTANTIATE(SegRowsTable, SegEntriesList)
#undef OU_SEG_INSTANTIATE

hipError_t launch_seg_upload_rows(SegRow* rows, const SegRowBlock& blk, int n, int off, const SegVar& v, hipStream_t st) {
  if (n < 1 || n > kSegRowsPerLaunch) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_upload_rows_kernel, dim3(1), dim3(64), 0, st, rows, blk, n, off, v);
  return hipGetLastError();
}
hipError_t launch_seg_upload_lens(int* lens, const SegEntryBlock& blk, int n, int j0, int Bw, int E, const LevelSpec& lv,
                                  hipStream_t st) {
  if (n < 1 || n > kSegEntriesPerLaunch || j0 < 0 || j0 + n > Bw || E < 1 || E > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_upload_lens_kernel, dim3(E), dim3(64), 0, st, lens, blk, n, j0, Bw, lv);
  return hipGetLastError();
}

}  // namespace ou
