// Polyphase windowed-sinc resampler over ragged rows: ou_resample of include/ouniverse.h ("resampling").
// Output j = f * nw + p of a row reads the `taps` inputs from f * orig + first[p] on and the coefficient column p of the table
// (int first[nw], then float coef[taps][nw]: consecutive lanes = consecutive phases = consecutive words).  One accumulation order
// for every kernel below -- taps ascending, one fp32 FMA each -- so a row's result depends on neither the tiling nor the batch.
// No atomics, 64-bit row offsets, every global read of x inside [0, len[b]).
#include "ou_internal.h"

namespace ou {
namespace {

constexpr int kPer = 4;                   // outputs per thread: a workgroup of nt threads owns nt * kPer consecutive outputs
constexpr int kLdsBytes = 64 * 1024;      // dynamic LDS a launch may ask for
constexpr int kRedBytes = 64;             // 4 + 4 per-wave partial minima / maxima (long long)
constexpr int kTabLdsMax = 24 * 1024;     // a table up to this size is copied into LDS, a larger one is read through the caches
constexpr int kSpanSlack = 12;            // rounding of the first offsets (2), alignment of the staged span to 16 bytes (3 + 3), spare

struct Geometry {
  int nt;        // threads per workgroup (0: the span of 64 * kPer outputs does not fit into LDS -> resample_direct_kernel)
  int span_cap;  // floats of LDS for the staged input span (multiple of 4)
  bool tab_lds;
};

Geometry geometry(int orig, int nw, int taps) {
  Geometry g{0, 0, false};
  const size_t tab_bytes = ((size_t)taps + 1) * (size_t)nw * 4;
  g.tab_lds = tab_bytes <= (size_t)kTabLdsMax;
  const long long budget = (kLdsBytes - kRedBytes - (g.tab_lds ? (long long)tab_bytes : 0)) / 4;
  for (int nt = 256; nt >= 64; nt >>= 1) {
    // first input of output j: floor(orig * j / nw - const) + 1, so the tile's first offsets spread over at most
    // ceil((tile - 1) * orig / nw) + 1 samples; every output reads `taps` from its own
    const long long spread = ((long long)(nt * kPer - 1) * orig + nw - 1) / nw;
    const long long need = (spread + taps + kSpanSlack + 3) & ~3ll;
    if (need <= budget) {
      g.nt = nt;
      g.span_cap = (int)need;
      return g;
    }
  }
  return g;
}

// grid (ceil(cols / (nt * kPer)), rows of this launch), nt threads, dynamic LDS: sx[span_cap] | red[8] | table copy (kTabLds)
template <bool kTabLds>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, long long x_stride, float* __restrict__ y,
                                                       long long y_stride, long long cols, ResampleRows rows, int orig, int nw,
                                                       int taps, const int* __restrict__ table, int span_cap, int vec_ok) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sx = smem;
  long long* red = reinterpret_cast<long long*>(smem + span_cap);
  int* stab = reinterpret_cast<int*>(smem + span_cap) + kRedBytes / 4;

  const int nt = blockDim.x, tid = threadIdx.x;
  const int b = blockIdx.y;
  const long long j0 = (long long)blockIdx.x * (nt * kPer);
  const long long len = rows.len[b], ylen = rows.ylen[b];
  const float* xr = x + (size_t)b * (size_t)x_stride;
  float* yr = y + (size_t)b * (size_t)y_stride;
  if (j0 >= ylen) {  // (uniform over the workgroup) nothing but the zero tail of the row
#pragma unroll
    for (int r = 0; r < kPer; r++) {
      const long long j = j0 + r * nt + tid;
      if (j < cols) yr[j] = 0.f;
    }
    return;
  }

  if (kTabLds) {
    const int words = (taps + 1) * nw;
    for (int i = tid; i < words; i += nt) stab[i] = table[i];
    __syncthreads();
  }
  const int* first = kTabLds ? stab : table;
  const float* coef = reinterpret_cast<const float*>(first) + nw;

  // the phase and the first input (relative to the tile's first frame) of this thread's outputs
  const long long f0 = j0 / nw;
  const unsigned p0 = (unsigned)(j0 - f0 * nw);
  int p[kPer];
  long long start[kPer];
  long long mn = 0x7fffffffffffffffll, mx = -0x7fffffffffffffffll;
#pragma unroll
  for (int r = 0; r < kPer; r++) {
    const unsigned q = p0 + (unsigned)(r * nt + tid);
    const unsigned df = q / (unsigned)nw;
    p[r] = (int)(q - df * (unsigned)nw);
    start[r] = (long long)df * orig + first[p[r]];
    mn = start[r] < mn ? start[r] : mn;
    mx = start[r] > mx ? start[r] : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long a = __shfl_xor(mn, o), c = __shfl_xor(mx, o);
    mn = a < mn ? a : mn;
    mx = c > mx ? c : mx;
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = mn;
    red[4 + (tid >> 6)] = mx;
  }
  __syncthreads();
  for (int w = 0; w < (nt >> 6); w++) {
    mn = red[w] < mn ? red[w] : mn;
    mx = red[4 + w] > mx ? red[4 + w] : mx;
  }

  // stage [lo, hi) of the row, widened to 16-byte groups of the row, zero outside [0, len): the row's own boundary
  const long long lo = f0 * orig + mn;
  const int shift = (int)(((lo % 4) + 4) % 4);
  const long long lo_al = lo - shift;
  long long groups = (mx + taps - mn + shift + 3) / 4;
  if (groups * 4 > span_cap) groups = span_cap / 4;  // (never: span_cap covers the bound of geometry())
  for (int c = tid; c < (int)groups; c += nt) {
    const long long g = lo_al + 4ll * c;
    float4 v;
    if (vec_ok && g >= 0 && g + 4 <= len) {
      v = *reinterpret_cast<const float4*>(xr + g);
    } else {
      v.x = (g >= 0 && g < len) ? xr[g] : 0.f;
      v.y = (g + 1 >= 0 && g + 1 < len) ? xr[g + 1] : 0.f;
      v.z = (g + 2 >= 0 && g + 2 < len) ? xr[g + 2] : 0.f;
      v.w = (g + 3 >= 0 && g + 3 < len) ? xr[g + 3] : 0.f;
    }
    *reinterpret_cast<float4*>(sx + 4 * c) = v;
  }
  __syncthreads();

  int off[kPer];
  float acc[kPer];
#pragma unroll
  for (int r = 0; r < kPer; r++) {
    off[r] = (int)(start[r] - mn) + shift;
    acc[r] = 0.f;
  }
  const float* cp = coef;
  for (int t = 0; t < taps; t++, cp += nw) {
#pragma unroll
    for (int r = 0; r < kPer; r++) acc[r] = fmaf(cp[p[r]], sx[off[r] + t], acc[r]);
  }
#pragma unroll
  for (int r = 0; r < kPer; r++) {
    const long long j = j0 + r * nt + tid;
    if (j < cols) yr[j] = j < ylen ? acc[r] : 0.f;
  }
}

// A rate pair whose span of 256 outputs does not fit into LDS (a very long filter): one thread per output, x and the table
// through the caches, the row boundary checked per tap.  Same order of accumulation.
__global__ __launch_bounds__(256) void resample_direct_kernel(const float* __restrict__ x, long long x_stride,
                                                              float* __restrict__ y, long long y_stride, long long cols,
                                                              ResampleRows rows, int orig, int nw, int taps,
                                                              const int* __restrict__ table) {
  const int b = blockIdx.y;
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= cols) return;
  const long long len = rows.len[b], ylen = rows.ylen[b];
  const float* xr = x + (size_t)b * (size_t)x_stride;
  float* yr = y + (size_t)b * (size_t)y_stride;
  if (j >= ylen) {
    yr[j] = 0.f;
    return;
  }
  const long long f = j / nw;
  const long long p = j - f * nw;
  const long long start = f * orig + table[p];
  const float* cp = reinterpret_cast<const float*>(table) + nw + p;
  float acc = 0.f;
  for (int t = 0; t < taps; t++, cp += nw) {
    const long long i = start + t;
    const float v = (i >= 0 && i < len) ? xr[i] : 0.f;
    acc = fmaf(*cp, v, acc);
  }
  yr[j] = acc;
}

// equal rates: y[b][j] = j < len[b] ? x[b][j] : 0 for j < cols
__global__ __launch_bounds__(256) void resample_copy_kernel(const float* __restrict__ x, long long x_stride, float* __restrict__ y,
                                                            long long y_stride, long long cols, ResampleRows rows) {
  const int b = blockIdx.y;
  const long long len = rows.len[b];
  const float* xr = x + (size_t)b * (size_t)x_stride;
  float* yr = y + (size_t)b * (size_t)y_stride;
#pragma unroll
  for (int r = 0; r < kPer; r++) {
    const long long j = (long long)blockIdx.x * (256 * kPer) + r * 256 + threadIdx.x;
    if (j < cols) yr[j] = j < len ? xr[j] : 0.f;
  }
}

}  // namespace

int resample_tile(int orig, int nw, int taps) {
  if (orig == nw) return 256 * kPer;
  const Geometry g = geometry(orig, nw, taps);
  return g.nt ? g.nt * kPer : 256;
}

hipError_t launch_resample(const float* x, long long x_stride, float* y, long long y_stride, long long cols,
                           const ResampleRows& rows, int n_rows, int orig, int nw, int taps, const void* table,
                           hipStream_t st) {
  if (n_rows < 1 || n_rows > kResampleRowsPerLaunch || cols < 1 || y_stride < cols || orig < 1 || nw < 1)
    return hipErrorInvalidValue;
  const bool copy = orig == nw;
  if (!copy && (!table || taps < 1)) return hipErrorInvalidValue;
  const int tile = resample_tile(orig, nw, taps);
  const long long nbx = (cols + tile - 1) / tile;
  if (nbx > 0x7fffffffll) return hipErrorInvalidValue;
  const dim3 grid((unsigned)nbx, n_rows);
  if (copy) {
    hipLaunchKernelGGL(resample_copy_kernel, grid, dim3(256), 0, st, x, x_stride, y, y_stride, cols, rows);
    return hipGetLastError();
  }
  const int* tab = static_cast<const int*>(table);
  const Geometry g = geometry(orig, nw, taps);
  if (!g.nt) {
    hipLaunchKernelGGL(resample_direct_kernel, grid, dim3(256), 0, st, x, x_stride, y, y_stride, cols, rows, orig, nw, taps, tab);
    return hipGetLastError();
  }
  // 16-byte loads need every row's sample 4 k on a 16-byte boundary
  const int vec_ok = (reinterpret_cast<uintptr_t>(x) % 16 == 0) && (x_stride % 4 == 0);
  const size_t lds = (size_t)g.span_cap * 4 + kRedBytes + (g.tab_lds ? ((size_t)taps + 1) * nw * 4 : 0);
  if (g.tab_lds)
    hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(g.nt), lds, st, x, x_stride, y, y_stride, cols, rows, orig, nw, taps,
                       tab, g.span_cap, vec_ok);
  else
    hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(g.nt), lds, st, x, x_stride, y, y_stride, cols, rows, orig, nw, taps,
                       tab, g.span_cap, vec_ok);
  return hipGetLastError();
}

}  // namespace ou
