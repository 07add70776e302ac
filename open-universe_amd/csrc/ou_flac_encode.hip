// FLAC encoder for the output side of the `enhance` CLI: ou_flac_encode_frames of include/ouniverse.h ("output files of the CLI").
// The stream is the subset audio.flac_encode writes, byte for byte: fixed blocks of 4096, independent channels, per channel and
// block either the order-2 fixed predictor with one Rice partition or a verbatim subframe.
// One workgroup per (file, block).  It walks the file's channels in order and carries the bit offset from one subframe to the
// next: a subframe's length is known only after its reduction and its prefix sum, so a stage per channel would need a second
// pass that shifts every subframe by the lengths in front of it, for a unit of work (4096 samples) one workgroup finishes anyway.
// The bits of a subframe are assembled in an LDS window of big-endian 32-bit words whose first bit is a 128-bit boundary of the
// frame; after every channel the whole 16-byte groups go to the frame's slot with 16-byte stores and the open group (< 128 bits)
// moves to the front of the window.  CRC-8 of the header is computed here (eleven bytes, one thread); CRC-16 of the frame is
// left to the host stage (ou_flac_assemble), which streams every byte through MD5 and the copy anyway.
// Integers throughout: |second difference| <= 2^25, folded residual u <= 2^26, the block's sum of u in 64 bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ouniverse.h"
#include "ou_flac_layout.h"

namespace ou {
namespace {

constexpr int kFilesPerLaunch = 64;      // per-file values travel as kernel arguments
constexpr int kNt = 256;                 // threads of a workgroup
constexpr int kPer = kFlacBlock / kNt;   // consecutive samples a thread codes
constexpr int kRiceMaxQuotient = 4096;   // a longer unary part sends the subframe to verbatim
// window: the open group (<= 127 bits) or the frame header (<= 14 bytes), then one verbatim subframe of 8 + 4096 * 24 bits
constexpr int kWinWords = 3088;
static_assert(kWinWords * 32 >= 128 + 8 + kFlacBlock * 24 + 128 && kWinWords % 4 == 0, "window holds one subframe and the carry");

struct FlacFiles {
  long long len[kFilesPerLaunch];     // samples per channel
  long long row0[kFilesPerLaunch];    // first row of x
  long long frame0[kFilesPerLaunch];  // index of the file's first frame among all frames of the call
  long long slot0[kFilesPerLaunch];   // byte offset of its first slot in `frames`
  long long pcm0[kFilesPerLaunch];    // byte offset of its packed samples in `pcm`
  int blk0[kFilesPerLaunch];          // first workgroup of the file in this launch
  int ch[kFilesPerLaunch];
};
static_assert(sizeof(FlacFiles) <= 3072, "kernel arguments stay below 4 KiB");

// clip(rint(x * 2^(bps - 1))): the product with a power of two and the rounding are exact in fp32; NaN -> 0
__device__ __forceinline__ int quantise(float x, float full) {
  const float v = fminf(fmaxf(rintf(x * full), -full), full - 1.f);
  return x != x ? 0 : (int)v;
}

// sample i of a block at word i + i / 16: a thread's 16 consecutive samples start 17 words apart, on different banks
__device__ __forceinline__ int pad(int i) { return i + (i >> 4); }

// `nb` bits (1 .. 32) of v (< 2^nb) at bit `pos` of the window, most significant bit first.  The words were zero: OR
__device__ __forceinline__ void put(uint32_t* win, uint32_t pos, uint32_t v, int nb) {
  const uint32_t wi = pos >> 5;
  const int room = 32 - (int)(pos & 31);
  if (nb <= room) {
    atomicOr(&win[wi], v << (room - nb));
  } else {
    atomicOr(&win[wi], v >> (nb - room));
    atomicOr(&win[wi + 1], v << (32 - (nb - room)));
  }
}

__device__ __forceinline__ uint32_t crc8_step(uint32_t c, uint32_t byte) {
  c ^= byte;
  for (int b = 0; b < 8; b++) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
  return c;
}

// bytes of the UTF-8-style coded frame number
__device__ __forceinline__ int utf8_bytes(uint32_t n) {
  return n < 0x80 ? 1 : n < 0x800 ? 2 : n < 0x10000 ? 3 : n < 0x200000 ? 4 : n < 0x4000000 ? 5 : 6;
}

// grid: all blocks of the launch's files, file after file
__global__ __launch_bounds__(kNt) void flac_encode_kernel(const float* __restrict__ x, long long stride, FlacFiles files, int n_files,
                                                          int bps, uint8_t* __restrict__ frames, int* __restrict__ sizes,
                                                          uint8_t* __restrict__ pcm) {
  __shared__ int sq[kFlacBlock + kFlacBlock / 16];
  __shared__ __attribute__((aligned(16))) uint32_t win[kWinWords];
  __shared__ unsigned long long red_sum[kNt / 64];
  __shared__ uint32_t red_max[kNt / 64];
  __shared__ uint32_t scan[kNt];

  const int tid = threadIdx.x;
  const int wg = blockIdx.x;
  int f = 0;
  for (int i = 1; i < n_files; i++)
    if (wg >= files.blk0[i]) f = i;
  const int blk = wg - files.blk0[f];
  const int ch = files.ch[f];
  const long long len = files.len[f], s0 = (long long)blk * kFlacBlock;
  const int n = len - s0 < kFlacBlock ? (int)(len - s0) : kFlacBlock;
  const float full = (float)(1 << (bps - 1));
  const uint32_t mask = (1u << bps) - 1u;
  const float* xf = x + (size_t)files.row0[f] * (size_t)stride + (size_t)s0;
  uint8_t* slot = frames + (size_t)files.slot0[f] + (size_t)blk * (size_t)flac_slot_bytes(ch, bps);

  for (int i = tid; i < kWinWords; i += kNt) win[i] = 0;
  __syncthreads();

  // frame header: sync, fixed blocking; block size "16 bits follow", rate "see STREAMINFO"; channels, sample size; frame number;
  // block size - 1; CRC-8
  const int fno_bytes = utf8_bytes((uint32_t)blk);
  if (tid == 0) {
    uint32_t hp = 0, crc = 0;
    auto emit = [&](uint32_t byte) {
      put(win, hp, byte, 8);
      hp += 8;
      crc = crc8_step(crc, byte);
    };
    emit(0xFF);
    emit(0xF8);
    emit(0x70);
    emit(((uint32_t)(ch - 1) << 4) | ((bps == 16 ? 4u : 6u) << 1));
    const uint32_t fno = (uint32_t)blk;
    if (fno_bytes == 1) {
      emit(fno);
    } else {
      emit(((0xFFu << (8 - fno_bytes)) & 0xFF) | (fno >> (6 * (fno_bytes - 1))));
      for (int i = fno_bytes - 2; i >= 0; i--) emit(0x80 | ((fno >> (6 * i)) & 0x3F));
    }
    emit((uint32_t)(n - 1) >> 8);
    emit((uint32_t)(n - 1) & 0xFF);
    put(win, hp, crc, 8);
  }
  uint32_t pos = 8u * (uint32_t)(4 + fno_bytes + 3);  // bit of the window the next subframe starts at
  uint32_t wbase = 0;                                 // byte of the frame the window starts at (a multiple of 16)
  __syncthreads();

  for (int c = 0; c < ch; c++) {
    const float* xr = xf + (size_t)c * (size_t)stride;
#pragma unroll
    for (int j = 0; j < kPer; j++) {
      const int i = j * kNt + tid;
      if (i < n) sq[pad(i)] = quantise(xr[i], full);
    }
    __syncthreads();

    // folded second differences of this thread's samples; the first two samples of the block are the warm-up
    const int i0 = tid * kPer;
    uint32_t u[kPer];
    unsigned long long sum = 0;
    uint32_t mx = 0;
    {
      int a = (i0 >= 2 && i0 - 2 < n) ? sq[pad(i0 - 2)] : 0, b = (i0 >= 1 && i0 - 1 < n) ? sq[pad(i0 - 1)] : 0;
#pragma unroll
      for (int j = 0; j < kPer; j++) {
        const int i = i0 + j;
        const int v = i < n ? sq[pad(i)] : 0;
        const int r = v - 2 * b + a;
        uint32_t uu = r >= 0 ? 2u * (uint32_t)r : (uint32_t)(-2 * r - 1);
        if (i < 2 || i >= n) uu = 0;
        u[j] = uu;
        sum += uu;
        mx = uu > mx ? uu : mx;
        a = b;
        b = v;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o);
      const uint32_t m2 = __shfl_xor(mx, o);
      mx = m2 > mx ? m2 : mx;
    }
    if ((tid & 63) == 0) {
      red_sum[tid >> 6] = sum;
      red_max[tid >> 6] = mx;
    }
    __syncthreads();
    sum = 0;
    mx = 0;
    for (int w = 0; w < kNt / 64; w++) {
      sum += red_sum[w];
      mx = red_max[w] > mx ? red_max[w] : mx;
    }

    // one Rice parameter for the block: the largest k <= 14 with (2^k - 1) (n - 2) <= sum u.  Everything from here to the
    // choice between the two subframe forms is the same in every thread
    int k = 0;
    bool rice = n >= 3;
    uint32_t own = 0, excl = 0, total = 0;
    if (rice) {
      while (k < 14 && ((2ull << k) - 1ull) * (unsigned long long)(n - 2) <= sum) k++;
      rice = (mx >> k) <= (uint32_t)kRiceMaxQuotient;
    }
    if (rice) {  // code lengths: quotient in unary, its terminating 1, k low bits; <= 16 * (4096 + 15) per thread
#pragma unroll
      for (int j = 0; j < kPer; j++) {
        const int i = i0 + j;
        if (i >= 2 && i < n) own += (u[j] >> k) + 1u + (uint32_t)k;
      }
      scan[tid] = own;
      __syncthreads();
      for (int o = 1; o < kNt; o <<= 1) {
        const uint32_t v = tid >= o ? scan[tid - o] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
      }
      excl = scan[tid] - own;
      total = scan[kNt - 1];
      rice = 8u + 2u * (uint32_t)bps + 10u + total < 8u + (uint32_t)n * (uint32_t)bps;
    }

    uint32_t bits;
    if (rice) {
      const uint32_t body = pos + 8u + 2u * (uint32_t)bps + 10u;
      if (tid == 0) {
        put(win, pos, 0x14, 8);  // padding bit, fixed predictor of order 2, no wasted bits
        put(win, pos + 8u, (uint32_t)sq[pad(0)] & mask, bps);
        put(win, pos + 8u + (uint32_t)bps, (uint32_t)sq[pad(1)] & mask, bps);
        put(win, pos + 8u + 2u * (uint32_t)bps, (uint32_t)k, 10);  // coding method 0, partition order 0, 4-bit parameter
      }
      uint32_t at = body + excl;
      const uint32_t low = (1u << k) - 1u;
#pragma unroll
      for (int j = 0; j < kPer; j++) {
        const int i = i0 + j;
        if (i >= 2 && i < n) {
          at += u[j] >> k;  // the zeros of the unary part are there
          put(win, at, (1u << k) | (u[j] & low), k + 1);
          at += (uint32_t)k + 1u;
        }
      }
      bits = 8u + 2u * (uint32_t)bps + 10u + total;
    } else {
      if (tid == 0) put(win, pos, 0x02, 8);  // padding bit, verbatim, no wasted bits
#pragma unroll
      for (int j = 0; j < kPer; j++) {
        const int i = i0 + j;
        if (i < n) put(win, pos + 8u + (uint32_t)i * (uint32_t)bps, (uint32_t)sq[pad(i)] & mask, bps);
      }
      bits = 8u + (uint32_t)n * (uint32_t)bps;
    }
    pos += bits;
    __syncthreads();

    // whole 16-byte groups out; behind the last channel the frame is padded with zero bits to a byte and everything goes
    const bool last = c == ch - 1;
    if (last) pos = (pos + 7u) & ~7u;
    const uint32_t nvec = last ? (pos + 127u) >> 7 : pos >> 7;
    uint4* dst = reinterpret_cast<uint4*>(slot + wbase);
    for (uint32_t i = tid; i < nvec; i += kNt) {
      uint4 v = reinterpret_cast<const uint4*>(win)[i];
      v.x = __builtin_bswap32(v.x);
      v.y = __builtin_bswap32(v.y);
      v.z = __builtin_bswap32(v.z);
      v.w = __builtin_bswap32(v.w);
      dst[i] = v;
    }
    if (last) {
      if (tid == 0) sizes[files.frame0[f] + blk] = (int)(wbase + (pos >> 3) + 2u);  // the CRC-16 the host stage appends
    } else {
      const uint32_t keep = tid < 4 ? win[nvec * 4u + (uint32_t)tid] : 0u;
      const uint32_t used = ((pos + 31u) >> 5) + 1u;
      __syncthreads();
      for (uint32_t i = tid; i < used && i < (uint32_t)kWinWords; i += kNt) win[i] = i < 4u ? keep : 0u;
      wbase += nvec * 16u;
      pos -= nvec * 128u;
      __syncthreads();
    }
  }

  // the block's part of the file's packed samples (sample-major, channels interleaved, little-endian): 16 bytes per thread and
  // step.  A block starts on a 16-byte boundary of the file's part; the last group of a file is filled up with zeros
  const int nbyte = bps == 16 ? 2 : 3;
  const int blk_bytes = n * ch * nbyte;
  uint4* pd = reinterpret_cast<uint4*>(pcm + (size_t)files.pcm0[f] + (size_t)s0 * (size_t)(ch * nbyte));
  for (int g = tid; g < (blk_bytes + 15) >> 4; g += kNt) {
    const int b0 = g * 16;
    const int s = b0 / nbyte;
    int bi = b0 - s * nbyte, t = s / ch;
    int cc = s - t * ch;
    int val = quantise(xf[(size_t)cc * (size_t)stride + t], full);  // (b0 < blk_bytes: t < n)
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if (b0 + j < blk_bytes) w[j >> 2] |= (((uint32_t)val >> (8 * bi)) & 0xFFu) << (8 * (j & 3));
      if (++bi == nbyte) {
        bi = 0;
        if (++cc == ch) {
          cc = 0;
          t++;
        }
        if (b0 + j + 1 < blk_bytes) val = quantise(xf[(size_t)cc * (size_t)stride + t], full);
      }
    }
    pd[g] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace
}  // namespace ou

extern "C" int ou_flac_encode_frames(const float* x, int64_t row_stride, int32_t files, const int32_t* channels_host,
                                     const int64_t* len_host, int32_t bps, void* frames, size_t frames_bytes,
                                     int32_t* frame_bytes, void* pcm, size_t pcm_bytes, ou_stream_t stream) {
  using namespace ou;
  const std::string who = "ou_flac_encode_frames: ";
  const std::string m = flac_shape_error(files, channels_host, len_host, bps);
  if (!m.empty()) return flac_fail(OU_EINVAL, who + m);
  if (!x || !frames || !frame_bytes || !pcm) return flac_fail(OU_EINVAL, who + "null argument");
  FlacTotals tot;
  if (!flac_totals(files, channels_host, len_host, bps, tot)) return flac_fail(OU_EINVAL, who + "the buffers exceed 2^62 bytes");
  long long longest = 0;
  for (int f = 0; f < files; f++) longest = len_host[f] > longest ? len_host[f] : longest;
  if (row_stride < longest)
    return flac_fail(OU_EINVAL, who + "row_stride = " + std::to_string((long long)row_stride) + " is below the longest length " +
                                    std::to_string(longest));
  if (tot.rows > (1ll << 60) / row_stride) return flac_fail(OU_EINVAL, who + "rows * row_stride overflows the kernel's 64-bit offsets");
  if (reinterpret_cast<uintptr_t>(frames) % 16 || reinterpret_cast<uintptr_t>(pcm) % 16)
    return flac_fail(OU_EINVAL, who + "frames and pcm must be 16-byte aligned");
  if (frames_bytes < (size_t)tot.frames_bytes || pcm_bytes < (size_t)tot.pcm_bytes)
    return flac_fail(OU_ESHAPE, who + "frames of " + std::to_string(frames_bytes) + " and pcm of " + std::to_string(pcm_bytes) +
                                    " bytes, ou_flac_encode_sizes asks for " + std::to_string(tot.frames_bytes) + " and " +
                                    std::to_string(tot.pcm_bytes));

  long long row = 0, frame = 0, slot = 0, pcm_off = 0;
  for (int f0 = 0; f0 < files;) {
    FlacFiles t;
    long long blocks = 0;
    int n = 0;
    for (; n < kFilesPerLaunch && f0 + n < files; n++) {
      const int f = f0 + n;
      const long long nb = flac_blocks(len_host[f]);
      if (blocks + nb > 0x7fffffffll) break;  // (a file has at most 2^24 blocks: n >= 1)
      t.len[n] = len_host[f];
      t.row0[n] = row;
      t.frame0[n] = frame;
      t.slot0[n] = slot;
      t.pcm0[n] = pcm_off;
      t.blk0[n] = (int)blocks;
      t.ch[n] = channels_host[f];
      blocks += nb;
      row += channels_host[f];
      frame += nb;
      slot += nb * flac_slot_bytes(channels_host[f], bps);
      pcm_off += flac_pcm_bytes(channels_host[f], len_host[f], bps);
    }
    for (int i = n; i < kFilesPerLaunch; i++) {
      t.len[i] = t.row0[i] = t.frame0[i] = t.slot0[i] = t.pcm0[i] = 0;
      t.blk0[i] = 0x7fffffff;
      t.ch[i] = 1;
    }
    hipLaunchKernelGGL(flac_encode_kernel, dim3((unsigned)blocks), dim3(kNt), 0, (hipStream_t)stream, x, (long long)row_stride, t, n,
                       (int)bps, static_cast<uint8_t*>(frames), reinterpret_cast<int*>(frame_bytes), static_cast<uint8_t*>(pcm));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return flac_fail(OU_EHIP, who + hipGetErrorString(e));
    f0 += n;
  }
  return OU_OK;
}

// ---- compression levels (ou_flac_encode_frames_level) ------------------------------------------------------------
// The same unit of work and the same window as above; per channel the workgroup prices candidates and packs the cheapest:
//   constant | fixed 0 .. 4 | (level 2) one LPC candidate of order 8, precision 14 | verbatim
// and, for a winning predictor, the best Rice partition order 0 .. 6.  Everything after the LPC analysis is integer arithmetic
// whose sums do not depend on their order; the analysis (double) runs in one fixed order: 16 consecutive samples per thread, a
// 64-lane butterfly, the four waves in turn.  A thread owns 16 consecutive samples and keeps them and their 8 predecessors in
// registers; residuals are recomputed per pass.  A partition has at least 16 samples, so a thread's samples meet at most two
// partitions of any order.  Level 0 of this kernel (fixed 2, one partition) exists for the choice records of a level-0 call
// alone: its stream comes from flac_encode_kernel.
namespace ou {
namespace {

constexpr int kLpcOrder = 8, kLpcPrecision = 14, kLpcMinBlock = 64;
constexpr int kCand = 6;      // fixed 0 .. 4, lpc
constexpr int kMaxPo = 6;     // partition orders 0 .. 6
constexpr int kHist = 8;      // predecessors a thread reads

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ uint32_t fold(long long r) { return r >= 0 ? (uint32_t)(2 * r) : (uint32_t)(-2 * r - 1); }

// the largest k <= 14 with (2^k - 1) cnt <= sum
__device__ __forceinline__ int rice_k(unsigned long long sum, uint32_t cnt) {
  int k = 0;
  while (k < 14 && ((2ull << k) - 1ull) * (unsigned long long)cnt <= sum) k++;
  return k;
}

// residual of candidate c at xs[m] (xs[m - 1 - j]: its predecessors); |.| < 2^31 for the fixed orders, checked for lpc
__device__ __forceinline__ long long fixed_residual(const int* xs, int m, int p) {
  const int a = xs[m], b = xs[m - 1], c = xs[m - 2], d = xs[m - 3], e = xs[m - 4];
  return p == 0 ? a : p == 1 ? a - b : p == 2 ? a - 2 * b + c : p == 3 ? a - 3 * b + 3 * c - d : a - 4 * b + 6 * c - 4 * d + e;
}
__device__ __forceinline__ long long lpc_residual(const int* xs, int m, const int* q, int shift) {
  long long s = 0;
#pragma unroll
  for (int j = 0; j < kLpcOrder; j++) s += (long long)q[j] * (long long)xs[m - 1 - j];
  return (long long)xs[m] - (s >> shift);
}

struct LevelShared {
  unsigned long long sum[kCand];       // sum of u per candidate
  unsigned long long part[2][64];      // sum of u per finest partition: the level-1 winner, the lpc candidate
  double acf[kNt / 64][kLpcOrder + 1];
  uint32_t qsum[kCand];                // sum of u >> k per candidate
  uint32_t plen[2][kMaxPo + 1];        // bits of the partitioned residual per order, the parameters not counted
  uint32_t flags;                      // bit c: candidate c dropped; bit 8: two samples differ
  uint32_t pdrop[2];                   // bit po: a quotient above the limit at that order
  int ktab[2][128];                      // Rice parameter of partition j of order po at (1 << po) - 1 + j
  int q[kLpcOrder];
  int shift, lpc_ok;
};

__global__ __launch_bounds__(kNt) void flac_level_kernel(const float* __restrict__ x, long long stride, FlacFiles files, int n_files,
                                                         int bps, int level, long long sub0, uint8_t* __restrict__ frames,
                                                         int* __restrict__ sizes, uint8_t* __restrict__ pcm,
                                                         int* __restrict__ choices) {
  __shared__ int sq[kFlacBlock + kFlacBlock / 16];
  __shared__ __attribute__((aligned(16))) uint32_t win[kWinWords];
  __shared__ uint32_t scan[kNt];
  __shared__ LevelShared sh;

  const int tid = threadIdx.x;
  const int wg = blockIdx.x;
  int f = 0;
  long long subs = sub0;  // subframes in front of this file's in the choices buffer
  for (int i = 1; i < n_files; i++)
    if (wg >= files.blk0[i]) {
      f = i;
      subs += (long long)(files.blk0[i] - files.blk0[i - 1]) * files.ch[i - 1];
    }
  const int blk = wg - files.blk0[f];
  const int ch = files.ch[f];
  const long long len = files.len[f], s0 = (long long)blk * kFlacBlock;
  const int n = len - s0 < kFlacBlock ? (int)(len - s0) : kFlacBlock;
  const float full = (float)(1 << (bps - 1));
  const uint32_t mask = (1u << bps) - 1u;
  const float* xf = x + (size_t)files.row0[f] * (size_t)stride + (size_t)s0;
  const bool emit_stream = frames != nullptr;
  uint8_t* slot = emit_stream ? frames + (size_t)files.slot0[f] + (size_t)blk * (size_t)flac_slot_bytes(ch, bps) : nullptr;
  int* rec0 = choices ? choices + (size_t)(subs + (long long)blk * ch) * OU_FLAC_CHOICE_WORDS : nullptr;

  for (int i = tid; i < kWinWords; i += kNt) win[i] = 0;
  __syncthreads();

  const int fno_bytes = utf8_bytes((uint32_t)blk);
  if (tid == 0 && emit_stream) {
    uint32_t hp = 0, crc = 0;
    auto emit = [&](uint32_t byte) {
      put(win, hp, byte, 8);
      hp += 8;
      crc = crc8_step(crc, byte);
    };
    emit(0xFF);
    emit(0xF8);
    emit(0x70);
    emit(((uint32_t)(ch - 1) << 4) | ((bps == 16 ? 4u : 6u) << 1));
    const uint32_t fno = (uint32_t)blk;
    if (fno_bytes == 1) {
      emit(fno);
    } else {
      emit(((0xFFu << (8 - fno_bytes)) & 0xFF) | (fno >> (6 * (fno_bytes - 1))));
      for (int i = fno_bytes - 2; i >= 0; i--) emit(0x80 | ((fno >> (6 * i)) & 0x3F));
    }
    emit((uint32_t)(n - 1) >> 8);
    emit((uint32_t)(n - 1) & 0xFF);
    put(win, hp, crc, 8);
  }
  uint32_t pos = 8u * (uint32_t)(4 + fno_bytes + 3);
  uint32_t wbase = 0;

  // the finest partition order of this block: 2^po divides n and a partition keeps 16 samples
  int pmax = 0;
  if (level >= 1)
    while (pmax < kMaxPo && (n & ((2 << pmax) - 1)) == 0 && (n >> (pmax + 1)) >= 16) pmax++;
  const int i0 = tid * kPer;

  for (int c = 0; c < ch; c++) {
    const float* xr = xf + (size_t)c * (size_t)stride;
    __syncthreads();  // the tables and sq of the channel before are done with
#pragma unroll
    for (int j = 0; j < kPer; j++) {
      const int i = j * kNt + tid;
      if (i < n) sq[pad(i)] = quantise(xr[i], full);
    }
    if (tid < kCand) {
      sh.sum[tid] = 0;
      sh.qsum[tid] = 0;
    }
    if (tid < 128) sh.part[tid >> 6][tid & 63] = 0;
    if (tid < 2 * (kMaxPo + 1)) sh.plen[tid / (kMaxPo + 1)][tid % (kMaxPo + 1)] = 0;
    if (tid == 0) {
      sh.flags = 0;
      sh.pdrop[0] = sh.pdrop[1] = 0;
      sh.lpc_ok = 0;
      sh.shift = 0;
    }
    if (tid < kLpcOrder) sh.q[tid] = 0;
    __syncthreads();

    int xs[kHist + kPer];  // xs[kHist + j]: sample i0 + j
#pragma unroll
    for (int m = 0; m < kHist + kPer; m++) {
      const int i = i0 - kHist + m;
      xs[m] = (i >= 0 && i < n) ? sq[pad(i)] : 0;
    }
    const int first = sq[pad(0)];

    // ---- the LPC analysis: Welch window, autocorrelation, Levinson-Durbin, quantisation ----
    const bool try_lpc = level >= 2 && n >= kLpcMinBlock;
    if (try_lpc) {
      double xw[kHist + kPer];
      const double mid = (double)(n - 1), wid = (double)(n + 1);
#pragma unroll
      for (int m = 0; m < kHist + kPer; m++) {
        const int i = i0 - kHist + m;
        const double z = (2.0 * (double)i - mid) / wid;
        xw[m] = (double)xs[m] * (1.0 - z * z);  // (xs is zero outside the block)
      }
#pragma unroll
      for (int lag = 0; lag <= kLpcOrder; lag++) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < kPer; j++) acc = acc + xw[kHist + j] * xw[kHist + j - lag];
        acc = wave_sum(acc);
        if ((tid & 63) == 0) sh.acf[tid >> 6][lag] = acc;
      }
      __syncthreads();
      if (tid == 0) {
        double r[kLpcOrder + 1];
#pragma unroll
        for (int lag = 0; lag <= kLpcOrder; lag++) {
          double t = 0.0;
#pragma unroll
          for (int w = 0; w < kNt / 64; w++) t = t + sh.acf[w][lag];
          r[lag] = t;
        }
        bool ok = isfinite(r[0]) && r[0] > 0.0;
        double a[kLpcOrder], err = ok ? r[0] : 1.0;
#pragma unroll
        for (int j = 0; j < kLpcOrder; j++) a[j] = 0.0;
#pragma unroll
        for (int m = 0; m < kLpcOrder; m++) {
          double acc = r[m + 1];
#pragma unroll
          for (int j = 0; j < m; j++) acc = acc - a[j] * r[m - j];
          const double kk = acc / err;
          double prev[kLpcOrder];
#pragma unroll
          for (int j = 0; j < kLpcOrder; j++) prev[j] = a[j];
#pragma unroll
          for (int j = 0; j < m; j++) a[j] = prev[j] - kk * prev[m - 1 - j];
          a[m] = kk;
          err = err * (1.0 - kk * kk);
          if (!(isfinite(err) && err > 0.0)) {
            ok = false;
            err = 1.0;
          }
        }
        double cmax = 0.0;
#pragma unroll
        for (int j = 0; j < kLpcOrder; j++) {
          ok = ok && isfinite(a[j]);
          cmax = fabs(a[j]) > cmax ? fabs(a[j]) : cmax;
        }
        ok = ok && cmax > 0.0;
        if (ok) {
          int e;
          frexp(cmax, &e);
          int shift = (kLpcPrecision - 1) - e;
          shift = shift < 0 ? 0 : shift > 15 ? 15 : shift;
          const double scale = (double)(1 << shift);
#pragma unroll
          for (int j = 0; j < kLpcOrder; j++) {
            const double qv = rint(a[j] * scale);
            ok = ok && qv >= -8192.0 && qv <= 8191.0;
            sh.q[j] = ok ? (int)qv : 0;
          }
          sh.shift = shift;
        }
        sh.lpc_ok = ok ? 1 : 0;
      }
      __syncthreads();
    }
    const bool lpc_ok = try_lpc && sh.lpc_ok != 0;
    int q[kLpcOrder];
#pragma unroll
    for (int j = 0; j < kLpcOrder; j++) q[j] = sh.q[j];
    const int shift = sh.shift;

    // which candidates exist: fixed p needs n > p; level 0 knows fixed 2 alone, and only for n >= 3
    uint32_t cand = 0;
    if (level == 0) {
      cand = n >= 3 ? 1u << 2 : 0u;
    } else {
      for (int p = 0; p <= 4; p++)
        if (n > p) cand |= 1u << p;
      if (lpc_ok) cand |= 1u << 5;
    }

    // ---- pass A: sum of u per candidate; lpc residuals in range; all samples equal ----
    {
      unsigned long long sum[kCand];
      uint32_t flags = 0;
#pragma unroll
      for (int p = 0; p < kCand; p++) sum[p] = 0;
#pragma unroll
      for (int j = 0; j < kPer; j++) {
        const int i = i0 + j;
        if (i < n) {
          if (xs[kHist + j] != first) flags |= 1u << 8;
#pragma unroll
          for (int p = 0; p <= 4; p++)
            if (i >= p) sum[p] += fold(fixed_residual(xs, kHist + j, p));
          if (lpc_ok && i >= kLpcOrder) {
            const long long r = lpc_residual(xs, kHist + j, q, shift);
            if (r <= -(1ll << 31) || r >= (1ll << 31))
              flags |= 1u << 5;
            else
              sum[5] += fold(r);
          }
        }
      }
#pragma unroll
      for (int p = 0; p < kCand; p++) {
        const unsigned long long s = wave_sum(sum[p]);
        if ((tid & 63) == 0 && s) atomicAdd(&sh.sum[p], s);
      }
      flags = wave_or(flags);
      if ((tid & 63) == 0 && flags) atomicOr(&sh.flags, flags);
    }
    __syncthreads();
    int kc[kCand];
#pragma unroll
    for (int p = 0; p < kCand; p++) kc[p] = rice_k(sh.sum[p], (uint32_t)(n - (p == 5 ? kLpcOrder : p)));

    // ---- pass B: sum of the quotients per candidate, and whether one of them is too long ----
    {
      uint32_t qs[kCand], flags = 0;
#pragma unroll
      for (int p = 0; p < kCand; p++) qs[p] = 0;
#pragma unroll
      for (int j = 0; j < kPer; j++) {
        const int i = i0 + j;
        if (i < n) {
#pragma unroll
          for (int p = 0; p <= 4; p++)
            if (i >= p) {
              const uint32_t qq = fold(fixed_residual(xs, kHist + j, p)) >> kc[p];
              if (qq > (uint32_t)kRiceMaxQuotient) flags |= 1u << p;
              qs[p] += qq > (uint32_t)kRiceMaxQuotient ? 0u : qq;
            }
          if (lpc_ok && i >= kLpcOrder) {
            const long long r = lpc_residual(xs, kHist + j, q, shift);
            const bool in = r > -(1ll << 31) && r < (1ll << 31);
            const uint32_t qq = in ? fold(r) >> kc[5] : 0u;
            if (qq > (uint32_t)kRiceMaxQuotient) flags |= 1u << 5;
            qs[5] += qq > (uint32_t)kRiceMaxQuotient ? 0u : qq;
          }
        }
      }
#pragma unroll
      for (int p = 0; p < kCand; p++) {
        const uint32_t s = wave_sum(qs[p]);
        if ((tid & 63) == 0 && s) atomicAdd(&sh.qsum[p], s);
      }
      flags = wave_or(flags);
      if ((tid & 63) == 0 && flags) atomicOr(&sh.flags, flags);
    }
    __syncthreads();

    // ---- stage 1 and 2, once for the candidates of level 1 (constant, fixed 0 .. 4: the cheapest, the earlier one on a tie) and
    // once for the lpc candidate; the same in every thread ----
    const uint32_t verbatim_bits = 8u + (uint32_t)n * (uint32_t)bps;
    const uint32_t dropped = sh.flags;
    int fkind[2], forder[2], fk0[2], fpo[2];
    uint32_t fbest[2], fhead[2];
#pragma unroll
    for (int fin = 0; fin < 2; fin++) {
      int kind = OU_FLAC_KIND_VERBATIM, order = 0, k0 = 0, po = 0;
      uint32_t best = 0xFFFFFFFFu, head = 0;
      if (fin == 0 && level >= 1 && !(dropped & (1u << 8))) {
        kind = OU_FLAC_KIND_CONSTANT;
        best = 8u + (uint32_t)bps;
      }
#pragma unroll
      for (int p = (fin == 0 ? 0 : 5); p < (fin == 0 ? 5 : 6); p++) {
        if (!(cand & (1u << p)) || (dropped & (1u << p))) continue;
        const int ord = p == 5 ? kLpcOrder : p;
        const uint32_t h = 8u + (uint32_t)ord * (uint32_t)bps + (p == 5 ? 9u + (uint32_t)(kLpcOrder * kLpcPrecision) : 0u) + 6u;
        const uint32_t bits = h + 4u + (uint32_t)(n - ord) * (uint32_t)(kc[p] + 1) + sh.qsum[p];
        if (bits < best) {
          best = bits;
          head = h;
          order = ord;
          k0 = kc[p];
          kind = p == 5 ? OU_FLAC_KIND_LPC : OU_FLAC_KIND_FIXED;
        }
      }
      const bool predictor = kind == OU_FLAC_KIND_FIXED || kind == OU_FLAC_KIND_LPC;
      if (predictor && pmax > 0) {  // the partition order
        uint32_t u[kPer];
#pragma unroll
        for (int j = 0; j < kPer; j++) {
          const int i = i0 + j;
          uint32_t uu = 0;
          if (i >= order && i < n) uu = fold(fin == 1 ? lpc_residual(xs, kHist + j, q, shift) : fixed_residual(xs, kHist + j, order));
          u[j] = uu;
        }
        const int fine = n >> pmax;  // samples of a finest partition (>= 16)
        {
          const int j0 = min(i0 / fine, (1 << pmax) - 1);  // (threads behind the block add nothing)
          const int edge = (j0 + 1) * fine;
          unsigned long long sa = 0, sb = 0;
#pragma unroll
          for (int j = 0; j < kPer; j++) {
            if (i0 + j < edge)
              sa += u[j];
            else
              sb += u[j];
          }
          if (sa) atomicAdd(&sh.part[fin][j0], sa);
          if (sb) atomicAdd(&sh.part[fin][j0 + 1], sb);  // (u is zero behind the block: sb != 0 means that partition exists)
        }
        __syncthreads();
        if (tid < (2 << pmax) - 1) {
          int o = 0;
          while (tid >= (2 << o) - 1) o++;
          const int j = tid - ((1 << o) - 1);
          const int span = 1 << (pmax - o);
          unsigned long long t = 0;
          for (int w = 0; w < span; w++) t += sh.part[fin][j * span + w];
          sh.ktab[fin][tid] = rice_k(t, (uint32_t)((n >> o) - (j == 0 ? order : 0)));
        }
        __syncthreads();
        uint32_t pl[kMaxPo + 1], pdrop = 0;
#pragma unroll
        for (int o = 0; o <= kMaxPo; o++) {
          pl[o] = 0;
          if (o <= pmax) {
            const int size = n >> o;
            const int j0 = min(i0 / size, (1 << o) - 1);
            const int edge = (j0 + 1) * size;
            const int ka = sh.ktab[fin][(1 << o) - 1 + j0];
            const int kb = j0 + 1 < (1 << o) ? sh.ktab[fin][(1 << o) - 1 + j0 + 1] : 0;
#pragma unroll
            for (int j = 0; j < kPer; j++) {
              const int i = i0 + j;
              if (i >= order && i < n) {
                const int k = i < edge ? ka : kb;
                const uint32_t qq = u[j] >> k;
                if (qq > (uint32_t)kRiceMaxQuotient) pdrop |= 1u << o;
                pl[o] += (qq > (uint32_t)kRiceMaxQuotient ? 0u : qq) + (uint32_t)k + 1u;
              }
            }
          }
        }
#pragma unroll
        for (int o = 0; o <= kMaxPo; o++) {
          const uint32_t t = wave_sum(pl[o]);
          if ((tid & 63) == 0 && t) atomicAdd(&sh.plen[fin][o], t);
        }
        pdrop = wave_or(pdrop);
        if ((tid & 63) == 0 && pdrop) atomicOr(&sh.pdrop[fin], pdrop);
        __syncthreads();
        for (int o = 1; o <= pmax; o++) {
          if (sh.pdrop[fin] & (1u << o)) continue;
          const uint32_t bits = head + (4u << o) + sh.plen[fin][o];
          if (bits < best) {
            best = bits;
            po = o;
          }
        }
      }
      fkind[fin] = kind;
      forder[fin] = order;
      fk0[fin] = k0;
      fpo[fin] = po;
      fbest[fin] = best;
      fhead[fin] = head;
    }
    const bool take_lpc = fbest[1] < fbest[0];  // lpc is the last candidate: it needs to be strictly shorter
    int kind = take_lpc ? fkind[1] : fkind[0], order = take_lpc ? forder[1] : forder[0], po = take_lpc ? fpo[1] : fpo[0];
    const int k0 = take_lpc ? fk0[1] : fk0[0];
    uint32_t best = take_lpc ? fbest[1] : fbest[0];
    const uint32_t head = take_lpc ? fhead[1] : fhead[0];
    const int* ktab = take_lpc ? sh.ktab[1] : sh.ktab[0];

    // ---- stage 3 ----
    if (best >= verbatim_bits) {
      kind = OU_FLAC_KIND_VERBATIM;
      order = 0;
      po = 0;
      best = verbatim_bits;
    }
    const bool coded = kind == OU_FLAC_KIND_FIXED || kind == OU_FLAC_KIND_LPC;
    const bool lpc_out = kind == OU_FLAC_KIND_LPC;
    uint32_t u[kPer];  // folded residuals of the chosen predictor (zero where a sample is warm-up or behind the block)
#pragma unroll
    for (int j = 0; j < kPer; j++) {
      const int i = i0 + j;
      uint32_t uu = 0;
      if (coded && i >= order && i < n) uu = fold(lpc_out ? lpc_residual(xs, kHist + j, q, shift) : fixed_residual(xs, kHist + j, order));
      u[j] = uu;
    }

    if (rec0 && tid < OU_FLAC_CHOICE_WORDS) {
      int v = 0;
      if (tid == 0) v = kind;
      if (tid == 1) v = order;
      if (tid == 2) v = po;
      if (tid == 3) v = lpc_out ? kLpcPrecision : 0;
      if (tid == 4) v = lpc_out ? shift : 0;
      if (tid == 5) v = (int)best;
      if (tid >= 6 && tid < 6 + kLpcOrder) v = lpc_out ? sh.q[tid - 6] : 0;
      rec0[(size_t)c * OU_FLAC_CHOICE_WORDS + tid] = v;
    }

    if (emit_stream) {
      if (coded) {
        // Rice parameters of this thread's (at most two) partitions; code lengths; the 4-bit parameter in front of the first
        // sample of every partition but the first, whose parameter belongs to the head
        const int size = n >> po;
        const int j0 = min(i0 / size, (1 << po) - 1);
        const int edge = (j0 + 1) * size;
        int ka, kb;
        if (po == 0) {
          ka = kb = k0;
        } else {
          ka = ktab[(1 << po) - 1 + j0];
          kb = j0 + 1 < (1 << po) ? ktab[(1 << po) - 1 + j0 + 1] : 0;
        }
        uint32_t own = 0;
#pragma unroll
        for (int j = 0; j < kPer; j++) {
          const int i = i0 + j;
          if (i >= order && i < n) {
            const int k = i < edge ? ka : kb;
            own += (u[j] >> k) + 1u + (uint32_t)k + ((i == edge && i > 0) || (i > 0 && i == j0 * size) ? 4u : 0u);
          }
        }
        scan[tid] = own;
        __syncthreads();
        for (int o = 1; o < kNt; o <<= 1) {
          const uint32_t v = tid >= o ? scan[tid - o] : 0u;
          __syncthreads();
          scan[tid] += v;
          __syncthreads();
        }
        const uint32_t excl = scan[tid] - own;
        if (tid == 0) {
          uint32_t hp = pos;
          put(win, hp, (uint32_t)((lpc_out ? 31 + order : 8 + order) << 1), 8);
          hp += 8;
          for (int j = 0; j < order; j++) {
            put(win, hp, (uint32_t)sq[pad(j)] & mask, bps);
            hp += (uint32_t)bps;
          }
          if (lpc_out) {
            put(win, hp, (uint32_t)(kLpcPrecision - 1), 4);
            put(win, hp + 4u, (uint32_t)shift, 5);
            hp += 9u;
            for (int j = 0; j < kLpcOrder; j++) {
              put(win, hp, (uint32_t)sh.q[j] & ((1u << kLpcPrecision) - 1u), kLpcPrecision);
              hp += (uint32_t)kLpcPrecision;
            }
          }
          put(win, hp, (uint32_t)po, 6);  // coding method 0, the partition order
          put(win, hp + 6u, (uint32_t)(po == 0 ? ka : ktab[(1 << po) - 1]), 4);
        }
        uint32_t at = pos + head + 4u + excl;
#pragma unroll
        for (int j = 0; j < kPer; j++) {
          const int i = i0 + j;
          if (i >= order && i < n) {
            const int k = i < edge ? ka : kb;
            if ((i == edge && i > 0) || (i > 0 && i == j0 * size)) {
              put(win, at, (uint32_t)k, 4);
              at += 4u;
            }
            at += u[j] >> k;
            put(win, at, (1u << k) | (u[j] & ((1u << k) - 1u)), k + 1);
            at += (uint32_t)k + 1u;
          }
        }
      } else if (kind == OU_FLAC_KIND_CONSTANT) {
        if (tid == 0) put(win, pos + 8u, (uint32_t)first & mask, bps);  // the subframe's first byte is zero
      } else {
        if (tid == 0) put(win, pos, 0x02, 8);
#pragma unroll
        for (int j = 0; j < kPer; j++) {
          const int i = i0 + j;
          if (i < n) put(win, pos + 8u + (uint32_t)i * (uint32_t)bps, (uint32_t)xs[kHist + j] & mask, bps);
        }
      }
      pos += best;
      __syncthreads();

      const bool last = c == ch - 1;
      if (last) pos = (pos + 7u) & ~7u;
      const uint32_t nvec = last ? (pos + 127u) >> 7 : pos >> 7;
      uint4* dst = reinterpret_cast<uint4*>(slot + wbase);
      for (uint32_t i = tid; i < nvec; i += kNt) {
        uint4 v = reinterpret_cast<const uint4*>(win)[i];
        v.x = __builtin_bswap32(v.x);
        v.y = __builtin_bswap32(v.y);
        v.z = __builtin_bswap32(v.z);
        v.w = __builtin_bswap32(v.w);
        dst[i] = v;
      }
      if (last) {
        if (tid == 0) sizes[files.frame0[f] + blk] = (int)(wbase + (pos >> 3) + 2u);
      } else {
        const uint32_t keep = tid < 4 ? win[nvec * 4u + (uint32_t)tid] : 0u;
        const uint32_t used = ((pos + 31u) >> 5) + 1u;
        __syncthreads();
        for (uint32_t i = tid; i < used && i < (uint32_t)kWinWords; i += kNt) win[i] = i < 4u ? keep : 0u;
        wbase += nvec * 16u;
        pos -= nvec * 128u;
      }
    }
  }
  if (!emit_stream) return;

  // the packed samples, as in flac_encode_kernel
  const int nbyte = bps == 16 ? 2 : 3;
  const int blk_bytes = n * ch * nbyte;
  uint4* pd = reinterpret_cast<uint4*>(pcm + (size_t)files.pcm0[f] + (size_t)s0 * (size_t)(ch * nbyte));
  for (int g = tid; g < (blk_bytes + 15) >> 4; g += kNt) {
    const int b0 = g * 16;
    const int s = b0 / nbyte;
    int bi = b0 - s * nbyte, t = s / ch;
    int cc = s - t * ch;
    int val = quantise(xf[(size_t)cc * (size_t)stride + t], full);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if (b0 + j < blk_bytes) w[j >> 2] |= (((uint32_t)val >> (8 * bi)) & 0xFFu) << (8 * (j & 3));
      if (++bi == nbyte) {
        bi = 0;
        if (++cc == ch) {
          cc = 0;
          t++;
        }
        if (b0 + j + 1 < blk_bytes) val = quantise(xf[(size_t)cc * (size_t)stride + t], full);
      }
    }
    pd[g] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace
}  // namespace ou

extern "C" int ou_flac_encode_choices_bytes(int32_t files, const int32_t* channels_host, const int64_t* len_host, size_t* bytes) {
  using namespace ou;
  const std::string who = "ou_flac_encode_choices_bytes: ";
  const std::string m = flac_shape_error(files, channels_host, len_host, 24);
  if (!m.empty()) return flac_fail(OU_EINVAL, who + m);
  if (!bytes) return flac_fail(OU_EINVAL, who + "null argument");
  long long subs = 0;
  for (int f = 0; f < files; f++) subs += flac_blocks(len_host[f]) * channels_host[f];  // (< 2^24 * 8 per file)
  *bytes = (size_t)subs * OU_FLAC_CHOICE_WORDS * sizeof(int32_t);
  return OU_OK;
}

extern "C" int ou_flac_encode_frames_level(const float* x, int64_t row_stride, int32_t files, const int32_t* channels_host,
                                           const int64_t* len_host, int32_t bps, int32_t level, void* frames, size_t frames_bytes,
                                           int32_t* frame_bytes, void* pcm, size_t pcm_bytes, int32_t* choices,
                                           size_t choices_bytes, ou_stream_t stream) {
  using namespace ou;
  const std::string who = "ou_flac_encode_frames_level: ";
  const std::string m = flac_shape_error(files, channels_host, len_host, bps);
  if (!m.empty()) return flac_fail(OU_EINVAL, who + m);
  if (level < 0 || level > 2) return flac_fail(OU_EINVAL, who + "level = " + std::to_string(level) + ": 0, 1 or 2");
  if (!x || !frames || !frame_bytes || !pcm) return flac_fail(OU_EINVAL, who + "null argument");
  FlacTotals tot;
  if (!flac_totals(files, channels_host, len_host, bps, tot)) return flac_fail(OU_EINVAL, who + "the buffers exceed 2^62 bytes");
  long long longest = 0, subs = 0;
  for (int f = 0; f < files; f++) {
    longest = len_host[f] > longest ? len_host[f] : longest;
    subs += flac_blocks(len_host[f]) * channels_host[f];
  }
  if (row_stride < longest)
    return flac_fail(OU_EINVAL, who + "row_stride = " + std::to_string((long long)row_stride) + " is below the longest length " +
                                    std::to_string(longest));
  if (tot.rows > (1ll << 60) / row_stride) return flac_fail(OU_EINVAL, who + "rows * row_stride overflows the kernel's 64-bit offsets");
  if (reinterpret_cast<uintptr_t>(frames) % 16 || reinterpret_cast<uintptr_t>(pcm) % 16)
    return flac_fail(OU_EINVAL, who + "frames and pcm must be 16-byte aligned");
  if (frames_bytes < (size_t)tot.frames_bytes || pcm_bytes < (size_t)tot.pcm_bytes)
    return flac_fail(OU_ESHAPE, who + "frames of " + std::to_string(frames_bytes) + " and pcm of " + std::to_string(pcm_bytes) +
                                    " bytes, ou_flac_encode_sizes asks for " + std::to_string(tot.frames_bytes) + " and " +
                                    std::to_string(tot.pcm_bytes));
  if (choices) {
    if (reinterpret_cast<uintptr_t>(choices) % 4) return flac_fail(OU_EINVAL, who + "choices must be 4-byte aligned");
    const size_t need = (size_t)subs * OU_FLAC_CHOICE_WORDS * sizeof(int32_t);
    if (choices_bytes < need)
      return flac_fail(OU_ESHAPE, who + "choices of " + std::to_string(choices_bytes) + " bytes, ou_flac_encode_choices_bytes asks for " +
                                      std::to_string(need));
  }
  if (level == 0) {  // the stream of ou_flac_encode_frames, from its kernel; the records, if asked for, from a pass that packs nothing
    const int rc = ou_flac_encode_frames(x, row_stride, files, channels_host, len_host, bps, frames, frames_bytes, frame_bytes, pcm,
                                         pcm_bytes, stream);
    if (rc != OU_OK || !choices) return rc;
  }

  long long row = 0, frame = 0, slot = 0, pcm_off = 0, sub0 = 0;
  for (int f0 = 0; f0 < files;) {
    FlacFiles t;
    long long blocks = 0, launch_subs = 0;
    int n = 0;
    for (; n < kFilesPerLaunch && f0 + n < files; n++) {
      const int f = f0 + n;
      const long long nb = flac_blocks(len_host[f]);
      if (blocks + nb > 0x7fffffffll) break;
      t.len[n] = len_host[f];
      t.row0[n] = row;
      t.frame0[n] = frame;
      t.slot0[n] = slot;
      t.pcm0[n] = pcm_off;
      t.blk0[n] = (int)blocks;
      t.ch[n] = channels_host[f];
      blocks += nb;
      launch_subs += nb * channels_host[f];
      row += channels_host[f];
      frame += nb;
      slot += nb * flac_slot_bytes(channels_host[f], bps);
      pcm_off += flac_pcm_bytes(channels_host[f], len_host[f], bps);
    }
    for (int i = n; i < kFilesPerLaunch; i++) {
      t.len[i] = t.row0[i] = t.frame0[i] = t.slot0[i] = t.pcm0[i] = 0;
      t.blk0[i] = 0x7fffffff;
      t.ch[i] = 1;
    }
    hipLaunchKernelGGL(flac_level_kernel, dim3((unsigned)blocks), dim3(kNt), 0, (hipStream_t)stream, x, (long long)row_stride, t, n,
                       (int)bps, (int)level, sub0, level == 0 ? nullptr : static_cast<uint8_t*>(frames),
                       reinterpret_cast<int*>(frame_bytes), static_cast<uint8_t*>(pcm), reinterpret_cast<int*>(choices));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return flac_fail(OU_EHIP, who + hipGetErrorString(e));
    f0 += n;
    sub0 += launch_subs;
  }
  return OU_OK;
}
