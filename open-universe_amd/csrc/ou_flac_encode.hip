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
