// Streaming enhance (ou_stream_*): the two device operations around the walk of a window.  Both are word-by-word
// row movers -- a window of a stream is a few hundred KB beside a walk of milliseconds, and ring wrap, chunk stride and the
// caller's running output offset leave no common 16-byte alignment -- with one thread per word, consecutive lanes on consecutive
// words.  Every position in the stream is 64-bit.  A word of the ring and of the carry is read and then rewritten by the ONE
// thread that owns it, so neither kernel needs an order between its threads, and nothing here is an atomic.
#include "ou_dev.h"
#include "ou_internal.h"

namespace ou {
namespace {

// Thread i < S of row c owns ring slot (g.s + i) % S, and with it sample s + i of the window.
//   window (g.L > 0): win[c][i] = sample g.s + i of the stream for i < L -- 0 from g.T_valid on (the zeros behind the end at a
//     flush), chunk[c][t - P0] for t >= P0 (this push), else the ring's word of t (an earlier push: t >= P0 - S);
//   ring (g.write_ring): the slot receives the LAST sample of the chunk that maps to it, if there is one -- after the launch the
//     ring holds the last S samples of the P0 + n pushed.  The slot is read (for the window) before it is written, by the same
//     thread: a chunk longer than the ring and a window across both are safe in one launch.
// grid (ceil(S / 256), C)
__global__ __launch_bounds__(256) void stream_gather_kernel(const float* __restrict__ chunk, float* __restrict__ ring,
                                                            float* __restrict__ win, StreamGather g) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (i >= g.S) return;
  const long long slot = (g.s + i) % g.S;
  float* rs = ring + (size_t)c * (size_t)g.S + slot;
  const float* cb = chunk + (size_t)c * (size_t)g.chunk_stride;
  if (i < g.L) {
    const long long t = g.s + i;
    float v = 0.f;
    if (t < g.T_valid) {
      if (t >= g.P0) v = t - g.P0 < g.n ? cb[t - g.P0] : 0.f;
      else v = *rs;
    }
    win[(size_t)c * (size_t)g.L + i] = v;
  }
  if (g.write_ring && g.n > 0) {
    const long long last = g.P0 + g.n - 1;                            // the newest sample
    const long long t = last - ((last - slot) % g.S + g.S) % g.S;     // the newest one that lands in this slot
    if (t >= g.P0) *rs = cb[t - g.P0];
  }
}

// (1 - a) earlier + a later for the fp32 weight a in [0, 1], rounded ONCE: the rounding errors of 1 - a, of the two products and of
// their sum are recovered exactly in fp32 (Dekker's fast two-sum, fma residuals, Knuth's two-sum) and added back, so what is stored
// is the real value of the expression to within its own last place -- the stitch of ou_segment.hip rounds four times.  The weight
// is that stitch's (crossfade_weight, ou_dev.h).
__device__ __forceinline__ float stream_blend(float a, float earlier, float later) {
  const float w = 1.f - a;
  const float ew = (1.f - w) - a;                      // (1 - a) = w + ew exactly (|a| <= 1)
  const float p1 = w * earlier, e1 = fmaf(w, earlier, -p1);
  const float p2 = a * later, e2 = fmaf(a, later, -p2);
  const float s = p1 + p2;
  const float bb = s - p1;
  const float es = (p1 - (s - bb)) + (p2 - bb);        // p1 + p2 = s + es exactly
  return s + (((e1 + e2) + es) + ew * earlier);
}

// Row c, thread j:
//   emit (j < e.n_emit): the stream's sample e0 + j = res[c][e.i0 + j], over the first e.xf of them blended (stream_blend) with the carry --
//     the last V samples of the window in front, whose crossfade region starts at e0 -- and, e.clip, clamped to [-1, 1]
//     -> out[c][j] (`out` already points at the call's running offset);
//   carry (j < e.V_store): carry[c][j] = res[c][L - V + j], the raw tail of this window for the next one.  carry[c][j] is read
//     (crossfade) before it is written, by the same thread.
// The tail of a stream whose last window ran in an earlier call is the call with res = carry, L = V, i0 = 0, xf = V_store = 0.
// grid (ceil(max(n_emit, V_store) / 256), C)
__global__ __launch_bounds__(256) void stream_emit_kernel(const float* __restrict__ res, float* __restrict__ carry,
                                                          float* __restrict__ out, StreamEmit e) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  const float* rb = res + (size_t)c * (size_t)e.L;
  float* cr = carry + (size_t)c * (size_t)e.V;
  if (j < e.n_emit) {
    float v = rb[e.i0 + j];
    if (j < e.xf) v = stream_blend(crossfade_weight(j, e.V), cr[j], v);
    if (e.clip) v = fminf(fmaxf(v, -1.f), 1.f);
    out[(size_t)c * (size_t)e.out_stride + j] = v;
  }
  if (j < e.V_store) cr[j] = rb[e.L - e.V + j];
}

}  // namespace

hipError_t launch_stream_gather(const float* chunk, float* ring, float* win, const StreamGather& g, int C, hipStream_t st) {
  // what the kernel indexes with: the window inside [P0 - S, P0 + n) or behind T_valid, a chunk only where one is read
  if (C < 1 || C > 65535 || g.S < 1 || g.L < 0 || g.L > g.S || g.s < 0 || g.n < 0 || g.P0 < 0 || g.T_valid < 0 || !ring ||
      (g.L > 0 && (!win || g.s < g.P0 - g.S)) || (g.n > 0 && (!chunk || g.chunk_stride < g.n)) ||
      (g.T_valid > g.P0 + g.n) || (g.S + 255) / 256 > 0x7fffffffll)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(stream_gather_kernel, dim3((unsigned)((g.S + 255) / 256), C), dim3(256), 0, st, chunk, ring, win, g);
  return hipGetLastError();
}

hipError_t launch_stream_emit(const float* res, float* carry, float* out, const StreamEmit& e, int C, hipStream_t st) {
  const long long n = e.n_emit > e.V_store ? e.n_emit : e.V_store;
  if (C < 1 || C > 65535 || n < 1 || e.L < 1 || e.V < 0 || e.n_emit < 0 || e.i0 < 0 || e.i0 + e.n_emit > e.L || e.xf < 0 ||
      e.xf > e.V || (e.V_store != 0 && (e.V_store != e.V || e.V > e.L)) || !res || (e.n_emit > 0 && (!out || e.out_stride < e.n_emit)) ||
      ((e.xf > 0 || e.V_store > 0) && !carry) || (n + 255) / 256 > 0x7fffffffll)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(stream_emit_kernel, dim3((unsigned)((n + 255) / 256), C), dim3(256), 0, st, res, carry, out, e);
  return hipGetLastError();
}

}  // namespace ou
