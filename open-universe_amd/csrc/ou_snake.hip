// Alias-free Snake activation of a whole (B, C, T) tensor: ou_snake_act of include/ouniverse.h, and the launch the network walk
// puts in front of a ConvBlock body conv whose PReLU_Conv has act_type snake / snakebeta (blocks.py:176-181).
//   y[b, c, :] = Resample(2 -> 1)( snake_c( Resample(1 -> 2)(x[b, c, :]) ) )        alias_free_act.py:25-30, snake.py:53-64, 115-128
// with torchaudio's two kernels: 1 -> 2 pads (7, 8) and runs the 2 phase kernels of 15 taps, u[2 q + p] = sum_k up[p][k] x[q + k - 7];
// 2 -> 1 pads (13, 15) and runs 28 taps at stride 2, y[t] = sum_k down[k] s[2 t + k - 13].
//
// One workgroup owns kTile consecutive outputs of one (row, channel).  It stages x[t0 - 16, t0 + kTile + 16) in LDS (14 + 13
// samples of halo for the two FIRs, widened to 16-byte groups), computes the x2 signal s[2 t0 - 16, 2 t0 + 2 kTile + 16) into LDS
// and never writes it to memory, then every thread sums its four consecutive outputs from a register window of that signal.
// A value is ONE chain of fp32 FMAs over the taps in ascending order, whatever tile or batch it is computed in; sinf is the
// precise one and 1 / (beta + 1e-9) a true division (snake.py:62 -- the reciprocal blows an error up when the parameter is small).
// Row b is the call on that row alone: x counts as zero outside [0, len[b]), the x2 signal outside [0, 2 len[b]), and the output is
// zero from len[b] on.  No atomics, 64-bit row offsets, nothing read outside [0, len[b]), nothing written outside [0, T).
#include "ou_internal.h"

namespace ou {
namespace {

constexpr int kTile = 512;               // outputs of one workgroup
constexpr int kThreads = kTile / 4;      // four consecutive outputs per thread
constexpr int kXs = kTile + 32;          // sx[m] = x[t0 - 16 + m]
constexpr int kSs = 2 * kTile + 32;      // ss[j] = s[2 t0 - 16 + j]
constexpr int kPairs = kTile + 16;       // pair i = (s[2 q], s[2 q + 1]) of q = t0 - 8 + i

// kLens: 0 every row is T long, 1 lens_dev[b], 2 rows.len[b]
template <int kLens>
__global__ __launch_bounds__(kThreads) void snake_act_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int T,
                                                             long long row_stride, const int* __restrict__ lens_dev,
                                                             SnakeRows rows, const float* __restrict__ exp_alpha,
                                                             const float* __restrict__ exp_beta,
                                                             const float* __restrict__ up_k, const float* __restrict__ down_k,
                                                             int vec_x, int vec_y) {
  __shared__ __attribute__((aligned(16))) float sx[kXs];
  __shared__ __attribute__((aligned(16))) float ss[kSs];
  const int tid = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int t0 = blockIdx.x * kTile;
  int len = T;
  if (kLens == 1) len = lens_dev[b];
  if (kLens == 2) len = rows.len[b];
  len = len < 0 ? 0 : (len > T ? T : len);
  const size_t row = ((size_t)b * (size_t)C + (size_t)c) * (size_t)row_stride;
  const float* xr = x + row;
  float* yr = y + row;
  const int t = t0 + 4 * tid;  // this thread's first output

  if (t0 >= len) {  // (uniform over the workgroup) nothing but the zero tail of the row
    if (vec_y && t + 4 <= T) {
      *reinterpret_cast<float4*>(yr + t) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
      for (int r = 0; r < 4; r++)
        if (t + r < T) yr[t + r] = 0.f;
    }
    return;
  }

  // ---- x[t0 - 16, t0 + kTile + 16) -> sx, zero outside [0, len): the row's own boundary
  for (int g = tid; g < kXs / 4; g += kThreads) {
    const int u = t0 - 16 + 4 * g;
    float4 v;
    if (vec_x && u >= 0 && u + 4 <= len) {
      v = *reinterpret_cast<const float4*>(xr + u);
    } else {
      v.x = (u >= 0 && u < len) ? xr[u] : 0.f;
      v.y = (u + 1 >= 0 && u + 1 < len) ? xr[u + 1] : 0.f;
      v.z = (u + 2 >= 0 && u + 2 < len) ? xr[u + 2] : 0.f;
      v.w = (u + 3 >= 0 && u + 3 < len) ? xr[u + 3] : 0.f;
    }
    *reinterpret_cast<float4*>(sx + 4 * g) = v;
  }
  __syncthreads();

  // ---- the x2 signal: both phases of q from the 15 inputs x[q - 7 .. q + 7] = sx[i + 1 .. i + 15], then Snake (snake.py:62 /
  // :126: x + (1 / (beta + 1e-9)) * sin(x * alpha)^2, the operations in that order)
  const float a = exp_alpha[c];
  const float inv = 1.0f / ((exp_beta ? exp_beta[c] : a) + 1e-9f);
  for (int i = tid; i < kPairs; i += kThreads) {
    const int q = t0 - 8 + i;
    float u0 = 0.f, u1 = 0.f;
#pragma unroll
    for (int k = 0; k < 15; k++) {
      const float v = sx[i + 1 + k];
      u0 = fmaf(up_k[k], v, u0);
      u1 = fmaf(up_k[15 + k], v, u1);
    }
    const float s0 = sinf(u0 * a), s1 = sinf(u1 * a);
    float2 o;
    o.x = u0 + inv * (s0 * s0);
    o.y = u1 + inv * (s1 * s1);
    if (q < 0 || q >= len) o.x = o.y = 0.f;  // Resample(2 -> 1) zero-pads the 2 len samples of the x2 signal
    *reinterpret_cast<float2*>(ss + 2 * i) = o;
  }
  __syncthreads();

  // ---- outputs t .. t + 3: output t + r reads s[2 (t + r) - 13 + k] = ss[8 tid + 2 r + 3 + k], k < 28
  float w[40];
#pragma unroll
  for (int g = 0; g < 10; g++) {
    const float4 v = *reinterpret_cast<const float4*>(ss + 8 * tid + 4 * g);
    w[4 * g] = v.x; w[4 * g + 1] = v.y; w[4 * g + 2] = v.z; w[4 * g + 3] = v.w;
  }
  float acc[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    acc[r] = 0.f;
#pragma unroll
    for (int k = 0; k < 28; k++) acc[r] = fmaf(down_k[k], w[2 * r + 3 + k], acc[r]);
    if (t + r >= len) acc[r] = 0.f;
  }
  if (vec_y && t + 4 <= T) {
    *reinterpret_cast<float4*>(yr + t) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (t + r < T) yr[t + r] = acc[r];
  }
}

}  // namespace

int snake_tile() { return kTile; }

hipError_t launch_snake_act(const float* x, float* y, int B, int C, int T, long long row_stride, const int* lens_dev,
                            const SnakeRows* rows, const float* exp_alpha, const float* exp_beta, const float* up_k,
                            const float* down_k, hipStream_t st) {
  if (!x || !y || !exp_alpha || !up_k || !down_k || B < 1 || C < 1 || T < 1 || row_stride < T || C > 65535 || B > 65535)
    return hipErrorInvalidValue;
  if (!lens_dev && rows && B > kSnakeRowsPerLaunch) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((T + kTile - 1) / kTile), (unsigned)C, (unsigned)B);
  // 16-byte accesses need sample 4 k of every row on a 16-byte boundary
  const int vec_x = reinterpret_cast<uintptr_t>(x) % 16 == 0 && row_stride % 4 == 0;
  const int vec_y = reinterpret_cast<uintptr_t>(y) % 16 == 0 && row_stride % 4 == 0;
  if (lens_dev)
    hipLaunchKernelGGL(snake_act_kernel<1>, grid, dim3(kThreads), 0, st, x, y, C, T, row_stride, lens_dev, SnakeRows(), exp_alpha,
                       exp_beta, up_k, down_k, vec_x, vec_y);
  else if (rows)
    hipLaunchKernelGGL(snake_act_kernel<2>, grid, dim3(kThreads), 0, st, x, y, C, T, row_stride, nullptr, *rows, exp_alpha,
                       exp_beta, up_k, down_k, vec_x, vec_y);
  else
    hipLaunchKernelGGL(snake_act_kernel<0>, grid, dim3(kThreads), 0, st, x, y, C, T, row_stride, nullptr, SnakeRows(), exp_alpha,
                       exp_beta, up_k, down_k, vec_x, vec_y);
  return hipGetLastError();
}

}  // namespace ou
