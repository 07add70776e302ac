// Ensemble reduce (Universe.enhance(ensemble=E), universe.py:261-264, 359-368; utils/stats.py:22-66) and the row replication
// of ou_enhance_ensemble.  Members are member-major: row e * B + b is member e of input b.
//
// ensemble_reduce_kernel<E>: one thread = one quad of consecutive samples of one input; its E x 4 member values live in
// registers (E is a template parameter).  Order statistics come from RANK COUNTING, branch-free:
//     rank(c) = #{j : x_j < x_c} + #{j < c : x_j == x_c}
// -- the stable ascending order (ties by member index) that universe.signal_median on the Python side uses.  Inputs are
// assumed finite.  No float atomics anywhere: the mean is a sequential fp32 sum in member order, the histogram of the signal
// median is integer (LDS counters per workgroup, then one integer atomicAdd per non-zero bin).
// Plain pointers, 64-bit offsets.  Bandwidth-bound up to E ~ 16; the E^2 compares of the median show from there on.
#include "ou_internal.h"

namespace ou {
namespace {

// value of stable rank K among v[0 .. E)
template <int E>
__device__ __forceinline__ float rank_select(const float (&v)[E], int K) {
  float r = v[0];
#pragma unroll
  for (int c = 0; c < E; c++) {
    int rank = 0;
#pragma unroll
    for (int j = 0; j < E; j++) rank += (j < c) ? (v[j] <= v[c] ? 1 : 0) : (v[j] < v[c] ? 1 : 0);
    r = rank == K ? v[c] : r;
  }
  return r;
}
// stable rank of member c
template <int E>
__device__ __forceinline__ int rank_of(const float (&v)[E], int c) {
  int rank = 0;
#pragma unroll
  for (int j = 0; j < E; j++) rank += (j < c) ? (v[j] <= v[c] ? 1 : 0) : (v[j] < v[c] ? 1 : 0);
  return rank;
}

// grid (ceil(cols / 1024), rows of this launch), 256 threads.  members: (E * B, row_stride), out: (B, row_stride); the launch
// covers the inputs b0 .. b0 + gridDim.y - 1, `lens.len[i]` = valid columns of input b0 + i.
// stat 0 mean, 1 median (rank (E - 1) / 2: torch.median's lower median): writes out, 0 from len[b] on.
// stat 2 signal median: writes nothing to out; hist[b][p] += #samples whose candidate member has rank position p.
template <int E>
__global__ __launch_bounds__(256) void ensemble_reduce_kernel(const float* __restrict__ members, float* __restrict__ out,
                                                              int B, int b0, long long row_stride, long long cols,
                                                              EnsLens lens, int stat, int vec_ok, int* __restrict__ hist) {
  __shared__ int shist[E];
  const int b = b0 + blockIdx.y, tid = threadIdx.x;
  const long long col = ((long long)blockIdx.x * 256 + tid) * 4;
  const long long len = lens.len[blockIdx.y];
  if (stat == 2) {
    if (tid < E) shist[tid] = 0;
    __syncthreads();
  }
  if (col < cols) {
    const int nv = len - col >= 4 ? 4 : (len > col ? (int)(len - col) : 0);  // valid samples of this quad
    float v[4][E];
    const float* src = members + (size_t)b * (size_t)row_stride + (size_t)col;
    const size_t mstride = (size_t)B * (size_t)row_stride;
    if (nv == 4 && vec_ok) {
#pragma unroll
      for (int e = 0; e < E; e++) {
        const float4 q = *reinterpret_cast<const float4*>(src + (size_t)e * mstride);
        v[0][e] = q.x; v[1][e] = q.y; v[2][e] = q.z; v[3][e] = q.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < E; e++) {
#pragma unroll
        for (int i = 0; i < 4; i++) v[i][e] = i < nv ? src[(size_t)e * mstride + i] : 0.f;  // (nothing is read past len[b])
      }
    }
    if (stat == 2) {
      // candidates: the member(s) whose index is nearest E / 2 -- one for even E, (E - 1) / 2 and (E + 1) / 2 for odd E; the
      // smaller rank position wins
      constexpr int C0 = E % 2 ? (E - 1) / 2 : E / 2;
      constexpr bool kTwo = E % 2 == 1 && E > 1;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        int p = rank_of<E>(v[i], C0);
        if constexpr (kTwo) {
          const int p1 = rank_of<E>(v[i], (E + 1) / 2);
          p = p1 < p ? p1 : p;
        }
        if (i < nv) atomicAdd(&shist[p], 1);
      }
    } else {
      float r[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (stat == 0) {
          float s = v[i][0];
#pragma unroll
          for (int e = 1; e < E; e++) s += v[i][e];
          r[i] = s / (float)E;
        } else {
          r[i] = rank_select<E>(v[i], (E - 1) / 2);
        }
        if (i >= nv) r[i] = 0.f;
      }
      float* dst = out + (size_t)b * (size_t)row_stride + (size_t)col;
      if (vec_ok && col + 4 <= cols) {
        *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (col + i < cols) dst[i] = r[i];
      }
    }
  }
  if (stat == 2) {
    __syncthreads();
    if (tid < E) {
      const int n = shist[tid];
      if (n) atomicAdd(hist + (size_t)b * E + tid, n);
    }
  }
}

// pick[b] = first maximum of hist[b][0 .. E) (as counts.argmax); out[b] = member row pick[b], 0 from len[b] on.
// grid (ceil(cols / 1024), rows of this launch), 256 threads
__global__ __launch_bounds__(256) void ensemble_pick_kernel(const float* __restrict__ members, float* __restrict__ out, int E,
                                                            int B, int b0, long long row_stride, long long cols, EnsLens lens,
                                                            int vec_ok, const int* __restrict__ hist, int* __restrict__ pick) {
  const int b = b0 + blockIdx.y;
  const long long len = lens.len[blockIdx.y];
  int best = 0, bn = hist[(size_t)b * E];
  for (int e = 1; e < E; e++) {
    const int n = hist[(size_t)b * E + e];
    if (n > bn) { bn = n; best = e; }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) pick[b] = best;
  const long long col = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (col >= cols) return;
  const float* src = members + ((size_t)best * B + b) * (size_t)row_stride + (size_t)col;
  float* dst = out + (size_t)b * (size_t)row_stride + (size_t)col;
  if (vec_ok && col + 4 <= len) {
    *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
  } else {
    for (int i = 0; i < 4; i++)
      if (col + i < cols) dst[i] = col + i < len ? src[i] : 0.f;
  }
}

// Entry k: the 4-byte words [0, n_k) at p_k are copied to [e n_k, (e + 1) n_k) for e = 1 .. E - 1 (rows [0, B) of a tensor laid
// out for E * B rows -> the rows of every other member).  grid (blocks, entries, E - 1), grid-stride over the entry's words;
// 16-byte copies where the entry allows them (aligned base, n_k % 4 == 0), else word by word.
__global__ __launch_bounds__(256) void replicate_rows_kernel(ReplicateTable tab) {
  unsigned* p = tab.p[blockIdx.y];
  const long long n = tab.n[blockIdx.y];
  unsigned* dst = p + (size_t)(blockIdx.z + 1) * (size_t)n;
  const long long step = (long long)gridDim.x * 256;
  const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool vec = (reinterpret_cast<uintptr_t>(p) % 16 == 0) && (n % 4 == 0);
  const long long nq = vec ? n / 4 : 0;
  for (long long q = i0; q < nq; q += step) reinterpret_cast<uint4*>(dst)[q] = reinterpret_cast<const uint4*>(p)[q];
  for (long long i = nq * 4 + i0; i < n; i += step) dst[i] = p[i];  // scalar tail (everything when not aligned)
}

template <int E>
void launch_reduce_e(const float* members, float* out, int B, int b0, int nb, long long row_stride, long long cols,
                     const EnsLens& lens, int stat, int vec_ok, int* hist, hipStream_t st) {
  const unsigned nbx = (unsigned)((cols + 1023) / 1024);
  hipLaunchKernelGGL(ensemble_reduce_kernel<E>, dim3(nbx, nb), dim3(256), 0, st, members, out, B, b0, row_stride, cols, lens,
                     stat, vec_ok, hist);
}

template <int E>
void dispatch_reduce(int e, const float* members, float* out, int B, int b0, int nb, long long row_stride, long long cols,
                     const EnsLens& lens, int stat, int vec_ok, int* hist, hipStream_t st) {
  if (e == E) launch_reduce_e<E>(members, out, B, b0, nb, row_stride, cols, lens, stat, vec_ok, hist, st);
  else if constexpr (E > 1) dispatch_reduce<E - 1>(e, members, out, B, b0, nb, row_stride, cols, lens, stat, vec_ok, hist, st);
}

}  // namespace

hipError_t launch_ensemble_reduce(const float* members, float* out, int E, int B, long long row_stride, long long cols,
                                  const long long* len_host, int stat, int* hist, int* pick, hipStream_t st) {
  if (!members || !out || E < 1 || E > kMaxEnsemble || B < 1 || cols < 1 || row_stride < cols || stat < 0 || stat > 2)
    return hipErrorInvalidValue;
  if (stat == 2 && (!hist || !pick)) return hipErrorInvalidValue;
  if ((cols + 1023) / 1024 > 0x7fffffffll) return hipErrorInvalidValue;
  // 16-byte accesses need every row's first column on a 16-byte boundary, in the members and in the output
  const int vec_ok = reinterpret_cast<uintptr_t>(members) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 &&
                     row_stride % 4 == 0;
  if (stat == 2) {
    const hipError_t e = hipMemsetAsync(hist, 0, (size_t)B * E * sizeof(int), st);
    if (e != hipSuccess) return e;
  }
  for (int pass = 0; pass < (stat == 2 ? 2 : 1); pass++) {
    for (int b0 = 0; b0 < B; b0 += kEnsRowsPerLaunch) {
      const int nb = B - b0 < kEnsRowsPerLaunch ? B - b0 : kEnsRowsPerLaunch;
      EnsLens lens;
      for (int i = 0; i < kEnsRowsPerLaunch; i++) {
        long long l = i < nb ? (len_host ? len_host[b0 + i] : cols) : 0;
        lens.len[i] = l < 0 ? 0 : (l > cols ? cols : l);
      }
      if (pass == 0) {
        dispatch_reduce<kMaxEnsemble>(E, members, out, B, b0, nb, row_stride, cols, lens, stat, vec_ok, hist, st);
      } else {
        const unsigned nbx = (unsigned)((cols + 1023) / 1024);
        hipLaunchKernelGGL(ensemble_pick_kernel, dim3(nbx, nb), dim3(256), 0, st, members, out, E, B, b0, row_stride, cols,
                           lens, vec_ok, hist, pick);
      }
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

hipError_t launch_replicate_rows(const ReplicateTable& tab, int n_entries, int E, hipStream_t st) {
  if (n_entries < 1 || n_entries > kReplicateEntries || E < 1) return hipErrorInvalidValue;
  if (E == 1) return hipSuccess;
  long long mx = 0;
  for (int k = 0; k < n_entries; k++) {
    if (!tab.p[k] || tab.n[k] < 0) return hipErrorInvalidValue;
    mx = tab.n[k] > mx ? tab.n[k] : mx;
  }
  long long nbx = (mx / 4 + 255) / 256;
  nbx = nbx < 1 ? 1 : (nbx > 4096 ? 4096 : nbx);
  hipLaunchKernelGGL(replicate_rows_kernel, dim3((unsigned)nbx, n_entries, E - 1), dim3(256), 0, st, tab);
  return hipGetLastError();
}

}  // namespace ou
