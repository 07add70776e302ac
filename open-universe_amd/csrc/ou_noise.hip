// Counter-based sampler noise: z(seed, stream, draw, t), the pure function defined in include/ouniverse.h ("counter-based
// noise").  Philox4x32-10 -> four 24-bit uniforms -> two Box-Muller pairs = the four normals of one quad of positions.
// Every kernel that evaluates z must give the same bits: precise device functions only (logf, log1pf, sqrtf, sincospif), no
// fast-math, -ffp-contract=off (Makefile).  Plain pointers, 64-bit offsets, no LDS; one thread = four columns = one 16-byte
// store where the row allows it.
#include "ou_internal.h"

namespace ou {
namespace {

constexpr unsigned kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr unsigned kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

struct Quad { float z0, z1, z2, z3; };

// Philox4x32-10 block function (Salmon et al., SC'11)
__device__ __forceinline__ void philox4x32_10(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
    const unsigned hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
}

// One Box-Muller pair from two words, u = ((w >> 8) + 0.5) * 2^-24 for both.  k + 0.5 has 25 significant bits, so it is not an
// fp32 number for k >= 2^23; the upper half of the interval is therefore evaluated through its mirror image m = 2^24 - 1 - k,
// whose m + 0.5 IS exact:  ln u = log1p(-(m + 0.5) 2^-24),  cos(2 pi u) = cos(2 pi u'),  sin(2 pi u) = -sin(2 pi u')  with
// u' = (m + 0.5) 2^-24 = 1 - u.  Every argument the library functions see is the exact value of the definition.
__device__ __forceinline__ void box_muller(unsigned w_r, unsigned w_a, float& za, float& zb) {
  const unsigned kr = w_r >> 8, ka = w_a >> 8;
  const bool lo_r = kr < (1u << 23), lo_a = ka < (1u << 23);
  const float fr = (float)(lo_r ? kr : 0xFFFFFFu - kr) + 0.5f;
  const float fa = (float)(lo_a ? ka : 0xFFFFFFu - ka) + 0.5f;
  const float v = fr * 0x1p-24f;
  const float ln_u = lo_r ? logf(v) : log1pf(-v);
  const float r = sqrtf(-2.0f * ln_u);
  float s, c;
  sincospif(fa * 0x1p-23f, &s, &c);  // 2 u (or 2 u'), in units of pi
  za = r * c;
  zb = r * (lo_a ? s : -s);
}

// the four normals of quad q (positions 4 q .. 4 q + 3); the counter packing of include/ouniverse.h
__device__ __forceinline__ Quad noise_quad(unsigned long long seed, unsigned long long stream, unsigned draw,
                                           unsigned long long q) {
  unsigned c0 = (unsigned)q;
  unsigned c1 = ((unsigned)(q >> 32) & 0xFFFFu) | (draw << 16);
  unsigned c2 = (unsigned)stream;
  unsigned c3 = (unsigned)(stream >> 32);
  philox4x32_10(c0, c1, c2, c3, (unsigned)seed, (unsigned)(seed >> 32));
  Quad z;
  box_muller(c0, c1, z.z0, z.z1);
  box_muller(c2, c3, z.z2, z.z3);
  return z;
}

// grid (ceil(cols / 1024), n_rows), 256 threads; thread i of row j writes the columns 4 i .. 4 i + 3.
// A row whose t0 is not a multiple of 4 straddles two quads per thread (the shift is uniform over the row).
__global__ __launch_bounds__(256) void noise_fill_kernel(float* __restrict__ out, long long row_stride, long long cols,
                                                         NoiseRows rows, unsigned long long seed, unsigned draw, int vec_ok) {
  const int j = blockIdx.y;
  const long long col = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (col >= cols) return;
  const unsigned long long stream = rows.stream[j];
  const long long t0 = rows.t0[j], len = rows.len[j];
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (col < len) {
    const unsigned long long t = (unsigned long long)(t0 + col);
    const unsigned long long q = t >> 2;
    const int a = (int)(t & 3);
    const Quad A = noise_quad(seed, stream, draw, q);
    if (a == 0) {
      v[0] = A.z0; v[1] = A.z1; v[2] = A.z2; v[3] = A.z3;
    } else {
      const Quad Bq = noise_quad(seed, stream, draw, q + 1);
      if (a == 1) { v[0] = A.z1; v[1] = A.z2; v[2] = A.z3; v[3] = Bq.z0; }
      else if (a == 2) { v[0] = A.z2; v[1] = A.z3; v[2] = Bq.z0; v[3] = Bq.z1; }
      else { v[0] = A.z3; v[1] = Bq.z0; v[2] = Bq.z1; v[3] = Bq.z2; }
    }
    if (col + 1 >= len) v[1] = 0.f;
    if (col + 2 >= len) v[2] = 0.f;
    if (col + 3 >= len) v[3] = 0.f;
  }
  float* dst = out + (size_t)j * (size_t)row_stride + (size_t)col;
  if (vec_ok && col + 4 <= cols) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    dst[0] = v[0];
    if (col + 1 < cols) dst[1] = v[1];
    if (col + 2 < cols) dst[2] = v[2];
    if (col + 3 < cols) dst[3] = v[3];
  }
}

}  // namespace

hipError_t launch_noise_fill(float* out, long long row_stride, long long cols, const NoiseRows& rows, int n_rows,
                             unsigned long long seed, int draw, hipStream_t st) {
  if (n_rows < 1 || n_rows > kNoiseRowsPerLaunch || cols < 1 || row_stride < cols) return hipErrorInvalidValue;
  const long long nbx = (cols + 1023) / 1024;
  if (nbx > 0x7fffffffll) return hipErrorInvalidValue;
  // 16-byte stores need every row's first column on a 16-byte boundary
  const int vec_ok = (reinterpret_cast<uintptr_t>(out) % 16 == 0) && (row_stride % 4 == 0);
  hipLaunchKernelGGL(noise_fill_kernel, dim3((unsigned)nbx, n_rows), dim3(256), 0, st, out, row_stride, cols, rows, seed,
                     (unsigned)draw, vec_ok);
  return hipGetLastError();
}

}  // namespace ou
