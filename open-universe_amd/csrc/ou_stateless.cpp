// Entry points that take no handle: the STFT pair, the resampler (plan, table, call), the Snake activation and the scores.
#include <cmath>
#include <string>
#include <vector>

#include "ou_handle.h"

using namespace ou;

extern "C" {

int ou_transform_frames(int32_t T, int32_t n_fft, int32_t hop) {
  if (T < 1 || n_fft < 2 || hop < 1) return OU_EINVAL;
  return 1 + (T + 2 * (n_fft / 2) - n_fft) / hop;
}

int ou_transform_forward(const float* x, int32_t B, int32_t T, const float* window, int32_t n_fft, int32_t hop,
                         int32_t transform_type, float abs_exponent, float factor, float* out, ou_stream_t stream) {
  if (!x || !window || !out || B < 1) return fail(nullptr, OU_EINVAL, "bad argument");
  if (transform_type < 0 || transform_type > 2) return fail(nullptr, OU_ENOTIMPL, "transform_type must be none | exponent | log");
  hipError_t e = launch_stft_forward(x, window, out, B, T, n_fft, hop, transform_type, abs_exponent, factor, (hipStream_t)stream);
  if (e != hipSuccess) return fail(nullptr, e == hipErrorInvalidValue ? OU_EINVAL : OU_EHIP, hipGetErrorString(e));
  return OU_OK;
}

int ou_transform_inverse(const float* spec, int32_t B, int32_t n_frames, const float* window, int32_t n_fft, int32_t hop,
                         int32_t transform_type, float abs_exponent, float factor, int32_t length, float* y,
                         float* scratch, ou_stream_t stream) {
  if (!spec || !window || !y || !scratch || B < 1) return fail(nullptr, OU_EINVAL, "bad argument");
  if (transform_type < 0 || transform_type > 2) return fail(nullptr, OU_ENOTIMPL, "transform_type must be none | exponent | log");
  hipError_t e = launch_stft_inverse(spec, window, scratch, y, B, n_frames, n_fft, hop, transform_type, abs_exponent, factor,
                                     length, (hipStream_t)stream);
  if (e != hipSuccess) return fail(nullptr, e == hipErrorInvalidValue ? OU_EINVAL : OU_EHIP, hipGetErrorString(e));
  return OU_OK;
}

}  // extern "C"

namespace {
// Resampler plan (include/ouniverse.h, "resampling"): a pure host function of the two rates.
struct RsPlan {
  int fs_in = 0, fs_out = 0;
  int orig = 0, nw = 0, width = 0, taps = 0;
  double base = 0.0;
  size_t bytes = 0;
};
constexpr double kRsLowpassWidth = 6.0, kRsRolloff = 0.99;

long long gcd_ll(long long a, long long b) {
  while (b) { const long long t = a % b; a = b; b = t; }
  return a;
}
// the window argument of entry (p, u) of the dense kernel, u = i - width, before the clamp -- in the operation order of the
// definition, so the double is the one the dense kernel is computed from
inline double rs_arg(const RsPlan& pl, int p, long long u) {
  return ((double)(-p) / (double)pl.nw + (double)u / (double)pl.orig) * pl.base;
}
inline bool rs_inside(const RsPlan& pl, int p, long long u) { return std::fabs(rs_arg(pl, p, u)) < kRsLowpassWidth; }
// support of phase p: the run [first, last] of u whose argument lies strictly inside (-6, 6), within the dense range
void rs_support(const RsPlan& pl, int p, long long& first, long long& last) {
  const double c = kRsLowpassWidth / pl.base, ph = (double)p / (double)pl.nw;
  first = (long long)std::floor((double)pl.orig * (ph - c)) - 2;
  while (!rs_inside(pl, p, first)) first++;
  last = (long long)std::ceil((double)pl.orig * (ph + c)) + 2;
  while (!rs_inside(pl, p, last)) last--;
  if (first < -(long long)pl.width) first = -(long long)pl.width;
  if (last > (long long)pl.width + pl.orig - 1) last = (long long)pl.width + pl.orig - 1;
}
// false: non-positive rates, or a rate pair whose filter does not fit 32-bit table indices
bool rs_plan(int fs_in, int fs_out, RsPlan& pl) {
  thread_local RsPlan cache;
  if (fs_in < 1 || fs_out < 1) return false;
  if (cache.fs_in == fs_in && cache.fs_out == fs_out) { pl = cache; return true; }
  const long long g = gcd_ll(fs_in, fs_out);
  pl.fs_in = fs_in; pl.fs_out = fs_out;
  pl.orig = (int)(fs_in / g);
  pl.nw = (int)(fs_out / g);
  pl.base = (double)(pl.orig < pl.nw ? pl.orig : pl.nw) * kRsRolloff;
  const double w = std::ceil(kRsLowpassWidth * (double)pl.orig / pl.base);
  if (w > (double)(1 << 28)) return false;
  pl.width = (int)w;
  long long taps = 0;
  for (int p = 0; p < pl.nw; p++) {
    long long a, b;
    rs_support(pl, p, a, b);
    if (b - a + 1 > taps) taps = b - a + 1;
  }
  if ((taps + 1) * (long long)pl.nw > 0x7fffffffll / 4) return false;
  pl.taps = (int)taps;
  pl.bytes = (size_t)(taps + 1) * (size_t)pl.nw * 4;
  cache = pl;
  return true;
}
}  // namespace

extern "C" {

int ou_resample_plan(int32_t fs_in, int32_t fs_out, int32_t* orig, int32_t* new_, int32_t* width, int32_t* taps,
                     size_t* table_bytes) {
  RsPlan pl;
  if (!rs_plan(fs_in, fs_out, pl))
    return fail(nullptr, OU_EINVAL, "ou_resample_plan: rates must be positive (and their reduced ratio within 32-bit table indices)");
  if (orig) *orig = pl.orig;
  if (new_) *new_ = pl.nw;
  if (width) *width = pl.width;
  if (taps) *taps = pl.taps;
  if (table_bytes) *table_bytes = pl.bytes;
  return OU_OK;
}

int ou_resample_table(int32_t fs_in, int32_t fs_out, void* table, size_t table_bytes) {
  RsPlan pl;
  if (!rs_plan(fs_in, fs_out, pl)) return fail(nullptr, OU_EINVAL, "ou_resample_table: bad rates");
  if (!table || table_bytes != pl.bytes)
    return fail(nullptr, OU_EINVAL, "ou_resample_table: table_bytes must be what ou_resample_plan returns");
  int32_t* first = static_cast<int32_t*>(table);
  float* coef = reinterpret_cast<float*>(first + pl.nw);
  const double scale = pl.base / (double)pl.orig;
  for (int p = 0; p < pl.nw; p++) {
    long long a, b;
    rs_support(pl, p, a, b);
    first[p] = (int32_t)a;
    for (int t = 0; t < pl.taps; t++) {
      double k = 0.0;
      if (a + t <= b) {
        // audio._sinc_kernel, operation by operation (the argument is strictly inside the clamp)
        double v = rs_arg(pl, p, a + t);
        const double c = std::cos(v * M_PI / kRsLowpassWidth / 2.0);
        const double window = c * c;
        v = v * M_PI;
        k = (v == 0.0 ? 1.0 : std::sin(v) / v) * window * scale;
      }
      coef[(size_t)t * pl.nw + p] = (float)k;
    }
  }
  return OU_OK;
}

int64_t ou_resample_length(int32_t fs_in, int32_t fs_out, int64_t n) {
  if (fs_in < 1 || fs_out < 1 || n < 0) return -1;
  const long long g = gcd_ll(fs_in, fs_out);
  const long long orig = fs_in / g, nw = fs_out / g;
  if (n > (0x7fffffffffffffffll - orig) / nw) return -1;
  return (nw * n + orig - 1) / orig;
}

int32_t ou_resample_tile(int32_t fs_in, int32_t fs_out) {
  RsPlan pl;
  if (!rs_plan(fs_in, fs_out, pl)) return -1;
  return resample_tile(pl.orig, pl.nw, pl.taps);
}

int ou_resample(const float* x, int64_t x_stride, const int64_t* len_host, float* y, int64_t y_stride, int64_t cols,
                int32_t rows, int32_t fs_in, int32_t fs_out, const void* table, size_t table_bytes, ou_stream_t stream) {
  if (fs_in < 1 || fs_out < 1) return fail(nullptr, OU_EINVAL, "ou_resample: the rates must be positive");
  if (!x || !y || !len_host || rows < 1 || x_stride < 0 || cols < 0 || y_stride < cols)
    return fail(nullptr, OU_EINVAL, "ou_resample: bad argument (rows >= 1, 0 <= cols <= y_stride, x_stride >= 0)");
  RsPlan pl;
  if (!rs_plan(fs_in, fs_out, pl))
    return fail(nullptr, OU_EINVAL, "ou_resample: the reduced ratio of the rates does not fit 32-bit table indices");
  const bool copy = pl.orig == pl.nw;
  if (!copy && (!table || table_bytes != pl.bytes))
    return fail(nullptr, OU_EINVAL, "ou_resample: table / table_bytes must be those of ou_resample_plan / ou_resample_table "
                                    "for this rate pair");
  // what the kernels index with: 64-bit element offsets rows * stride and output positions nw * len + orig
  constexpr long long kMaxOffset = 1ll << 60;
  if ((x_stride && rows > kMaxOffset / x_stride) || (y_stride && rows > kMaxOffset / y_stride))
    return fail(nullptr, OU_EINVAL, "ou_resample: rows * stride overflows the kernel's 64-bit offsets");
  std::vector<long long> ylen((size_t)rows);
  for (int b = 0; b < rows; b++) {
    const long long n = len_host[b];
    if (n < 0 || n > x_stride) return fail(nullptr, OU_EINVAL, "ou_resample: 0 <= len[b] <= x_stride");
    if (n > (kMaxOffset - pl.orig) / pl.nw)
      return fail(nullptr, OU_EINVAL, "ou_resample: new * len[b] overflows the kernel's 64-bit positions");
    ylen[b] = copy ? n : ((long long)pl.nw * n + pl.orig - 1) / pl.orig;
    if (ylen[b] > cols)
      return fail(nullptr, OU_EINVAL, "ou_resample: row " + std::to_string(b) + " needs " + std::to_string(ylen[b]) +
                                          " output columns, cols = " + std::to_string(cols));
  }
  if (cols == 0) return OU_OK;  // (every row is empty and there is nothing to zero)
  const long long tile = resample_tile(pl.orig, pl.nw, pl.taps);
  if ((cols + tile - 1) / tile > 0x7fffffffll) return fail(nullptr, OU_EINVAL, "ou_resample: cols exceeds the launch grid");
  for (int off = 0; off < rows; off += kResampleRowsPerLaunch) {
    ResampleRows blk;
    const int n = rows - off < kResampleRowsPerLaunch ? rows - off : kResampleRowsPerLaunch;
    for (int i = 0; i < kResampleRowsPerLaunch; i++) {
      blk.len[i] = i < n ? len_host[off + i] : 0;
      blk.ylen[i] = i < n ? ylen[off + i] : 0;
    }
    const hipError_t e = launch_resample(x + (size_t)off * (size_t)x_stride, x_stride, y + (size_t)off * (size_t)y_stride,
                                         y_stride, cols, blk, n, pl.orig, pl.nw, pl.taps, copy ? nullptr : table,
                                         (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, OU_EHIP, std::string("HIP error at resample: ") + hipGetErrorString(e));
  }
  return OU_OK;
}

int32_t ou_snake_tile(void) { return snake_tile(); }

int ou_snake_act(const float* x, float* y, int32_t B, int32_t C, int32_t T, int64_t row_stride, const int32_t* len_host,
                 const float* exp_alpha, const float* exp_beta, const float* up_kernel, const float* down_kernel,
                 ou_stream_t stream) {
  // everything is decided here, on the host, before the first HIP call
  if (!x || !y || !exp_alpha || !up_kernel || !down_kernel) return fail(nullptr, OU_EINVAL, "ou_snake_act: null argument");
  if (B < 1 || C < 1 || T < 1) return fail(nullptr, OU_EINVAL, "ou_snake_act: B, C and T must be at least 1");
  if (C > 65535) return fail(nullptr, OU_EINVAL, "ou_snake_act: at most 65535 channels");
  if (T > 0x7fffffff - 1024) return fail(nullptr, OU_EINVAL, "ou_snake_act: T must not exceed 2^31 - 1024");
  if (row_stride < T) return fail(nullptr, OU_EINVAL, "ou_snake_act: row_stride must be at least T");
  // 64-bit offsets of the kernel: (b * C + c) * row_stride + t, in floats
  if ((long long)row_stride > (1ll << 60) / ((long long)B * C))
    return fail(nullptr, OU_EINVAL, "ou_snake_act: B * C * row_stride overflows the 64-bit offsets (at most 2^60)");
  if (len_host)
    for (int b = 0; b < B; b++)
      if (len_host[b] < 0 || len_host[b] > T) return fail(nullptr, OU_EINVAL, "ou_snake_act: 0 <= len[b] <= T");
  if (!len_host) {
    for (int off = 0; off < B; off += 65535) {  // (the grid's z extent)
      const int n = B - off < 65535 ? B - off : 65535;
      const size_t skip = (size_t)off * (size_t)C * (size_t)row_stride;
      const hipError_t e = launch_snake_act(x + skip, y + skip, n, C, T, row_stride, nullptr, nullptr, exp_alpha, exp_beta, up_kernel,
                                            down_kernel, (hipStream_t)stream);
      if (e != hipSuccess) return fail(nullptr, OU_EHIP, std::string("ou_snake_act: ") + hipGetErrorString(e));
    }
    return OU_OK;
  }
  for (int off = 0; off < B; off += kSnakeRowsPerLaunch) {
    SnakeRows blk;
    const int n = B - off < kSnakeRowsPerLaunch ? B - off : kSnakeRowsPerLaunch;
    for (int i = 0; i < kSnakeRowsPerLaunch; i++) blk.len[i] = i < n ? len_host[off + i] : 0;
    const size_t skip = (size_t)off * (size_t)C * (size_t)row_stride;
    const hipError_t e = launch_snake_act(x + skip, y + skip, n, C, T, row_stride, nullptr, &blk, exp_alpha, exp_beta, up_kernel,
                                          down_kernel, (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, OU_EHIP, std::string("ou_snake_act: ") + hipGetErrorString(e));
  }
  return OU_OK;
}

}  // extern "C"

// ---- scoring: ou_lsd, ou_spectral_mae, ou_si_sdr (include/ouniverse.h, "scoring"; kernels: ou_metrics.hip) -------------------
namespace {
constexpr long long kMetMaxLen = 0x7fffffffll;
inline size_t met_align(size_t v) { return (v + 255) & ~(size_t)255; }

// scratch of one call: | tsum (B, 8) double | window | basis (the largest n_fft) | partial of every spec |
struct MetLayout {
  size_t tsum = 0, window = 0, basis = 0, bytes = 0;
  size_t partial[kMetMaxSpecs] = {};
  long long tile_stride[kMetMaxSpecs] = {};
};

// the message of a bad spec, or empty
std::string met_spec_error(const ou_metrics_spec& s) {
  if (s.n_fft < 2 || (s.n_fft & 1))
    return "n_fft = " + std::to_string(s.n_fft) + " must be even and at least 2";
  if (s.n_fft > OU_METRICS_MAX_NFFT)
    return "n_fft = " + std::to_string(s.n_fft) + " exceeds OU_METRICS_MAX_NFFT = " + std::to_string(OU_METRICS_MAX_NFFT) +
           " (the 32 frames of a workgroup are kept in LDS)";
  if (s.hop < 1) return "hop = " + std::to_string(s.hop) + " must be at least 1";
  return std::string();
}

MetLayout met_layout(int B, long long T_max, const ou_metrics_spec* spec, int n_spec) {
  MetLayout L;
  size_t at = 0;
  L.tsum = at; at = met_align(at + (size_t)B * 8 * sizeof(double));
  int nmax = 0;
  for (int i = 0; i < n_spec; i++) nmax = spec[i].n_fft > nmax ? spec[i].n_fft : nmax;
  L.window = at; at = met_align(at + (size_t)4 * met_k4(nmax) * sizeof(double));
  L.basis = at; at = met_align(at + (nmax ? met_basis_words(nmax) : 0) * sizeof(double));
  for (int i = 0; i < n_spec; i++) {
    L.tile_stride[i] = met_frame_tiles(T_max, spec[i].hop);
    L.partial[i] = at; at = met_align(at + (size_t)B * (size_t)L.tile_stride[i] * sizeof(double));
  }
  L.bytes = at;
  return L;
}

// sum of the squares of the periodic Hann window
double met_window_power(int n_fft) {
  double s = 0.0;
  for (int k = 0; k < n_fft; k++) {
    const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)k / (double)n_fft);
    s += w * w;
  }
  return s;
}

// the checks every score shares; len_max <- the longest row
int met_check_rows(const char* who, const float* est, const float* ref, int64_t stride, const int64_t* len_host, int32_t B,
                   long long* len_max) {
  const std::string w(who);
  if (!est || !ref || !len_host) return fail(nullptr, OU_EINVAL, w + ": null argument");
  if (B < 1) return fail(nullptr, OU_EINVAL, w + ": B must be at least 1");
  if (stride < 1 || (long long)stride > (1ll << 60) / B)
    return fail(nullptr, OU_EINVAL, w + ": stride must be at least 1 and B * stride at most 2^60");
  long long mx = 0;
  for (int b = 0; b < B; b++) {
    const long long n = len_host[b];
    if (n < 1 || n > stride || n > kMetMaxLen)
      return fail(nullptr, OU_EINVAL, w + ": 1 <= len[" + std::to_string(b) + "] <= min(stride, 2^31 - 1), got " + std::to_string(n));
    mx = n > mx ? n : mx;
  }
  *len_max = mx;
  return OU_OK;
}

inline void met_rows_of(const int64_t* len_host, int B, int off, MetRows& rows, int& n, long long& len_max) {
  n = B - off < kMetRowsPerLaunch ? B - off : kMetRowsPerLaunch;
  len_max = 0;
  for (int i = 0; i < kMetRowsPerLaunch; i++) {
    rows.len[i] = i < n ? len_host[off + i] : 0;
    len_max = rows.len[i] > len_max ? rows.len[i] : len_max;
  }
}

inline int met_hip(const char* who, hipError_t e) {
  return e == hipSuccess ? OU_OK : fail(nullptr, OU_EHIP, std::string(who) + ": " + hipGetErrorString(e));
}
}  // namespace

extern "C" {

int64_t ou_metrics_frames(int64_t T, int32_t hop) {
  if (T < 0 || hop < 1) return -1;
  return 1 + T / hop;
}

int ou_metrics_scratch_bytes(int32_t B, int64_t T_max, const ou_metrics_spec* spec, int32_t n_spec, size_t* nbytes) {
  if (!nbytes || B < 1 || T_max < 1 || T_max > kMetMaxLen || n_spec < 0 || n_spec > OU_METRICS_MAX_SPECS || (n_spec && !spec))
    return fail(nullptr, OU_EINVAL, "ou_metrics_scratch_bytes: B >= 1, 1 <= T_max <= 2^31 - 1, 0 <= n_spec <= OU_METRICS_MAX_SPECS");
  for (int i = 0; i < n_spec; i++) {
    const std::string m = met_spec_error(spec[i]);
    if (!m.empty()) return fail(nullptr, OU_EINVAL, "ou_metrics_scratch_bytes: spec " + std::to_string(i) + ": " + m);
  }
  *nbytes = met_layout(B, T_max, spec, n_spec).bytes;
  return OU_OK;
}

int ou_lsd(const float* est, const float* ref, int64_t stride, const int64_t* len_host, int32_t B, const ou_metrics_spec* spec,
           float* out, void* scratch, size_t scratch_bytes, ou_stream_t stream) {
  long long len_max = 0;
  if (int rc = met_check_rows("ou_lsd", est, ref, stride, len_host, B, &len_max)) return rc;
  if (!spec || !out || !scratch) return fail(nullptr, OU_EINVAL, "ou_lsd: null argument");
  const std::string m = met_spec_error(*spec);
  if (!m.empty()) return fail(nullptr, OU_EINVAL, "ou_lsd: " + m);
  if (spec->flags & ~(OU_MET_SCALE_INVARIANT | OU_MET_NATURAL_LOG)) return fail(nullptr, OU_EINVAL, "ou_lsd: unknown flag");
  if (!(spec->eps >= 0.0f)) return fail(nullptr, OU_EINVAL, "ou_lsd: eps must not be negative");
  for (int b = 0; b < B; b++)
    if (len_host[b] <= spec->n_fft / 2)
      return fail(nullptr, OU_EINVAL, "ou_lsd: len[" + std::to_string(b) + "] = " + std::to_string((long long)len_host[b]) +
                                          " must exceed n_fft / 2 = " + std::to_string(spec->n_fft / 2) +
                                          " (the reflect padding of the centred STFT is undefined otherwise)");
  const MetLayout L = met_layout(B, len_max, spec, 1);
  if (scratch_bytes < L.bytes)
    return fail(nullptr, OU_ESHAPE, "ou_lsd: scratch of " + std::to_string(scratch_bytes) + " bytes, ou_metrics_scratch_bytes asks for " +
                                        std::to_string(L.bytes));
  char* base = static_cast<char*>(scratch);
  double* tsum = reinterpret_cast<double*>(base + L.tsum);
  double* window = reinterpret_cast<double*>(base + L.window);
  double* basis = reinterpret_cast<double*>(base + L.basis);
  double* partial = reinterpret_cast<double*>(base + L.partial[0]);
  const hipStream_t st = (hipStream_t)stream;
  const bool si = spec->flags & OU_MET_SCALE_INVARIANT;
  if (int rc = met_hip("ou_lsd", launch_met_basis(basis, window, spec->n_fft, st))) return rc;
  const double w2 = met_window_power(spec->n_fft);
  for (int off = 0; off < B; off += kMetRowsPerLaunch) {
    MetRows rows;
    int n;
    long long lm;
    met_rows_of(len_host, B, off, rows, n, lm);
    if (int rc = met_hip("ou_lsd", launch_met_time(est, ref, stride, rows, n, off, spec->eps, si, tsum, st))) return rc;
    if (int rc = met_hip("ou_lsd", launch_met_stft(false, est, ref, stride, rows, n, off, lm, basis, window, tsum, spec->n_fft,
                                                   spec->hop, w2, spec->eps, spec->flags & OU_MET_NATURAL_LOG, partial,
                                                   L.tile_stride[0], st)))
      return rc;
    if (int rc = met_hip("ou_lsd", launch_met_final_lsd(rows, n, off, partial, L.tile_stride[0], spec->hop, spec->n_fft, out, st)))
      return rc;
  }
  return OU_OK;
}

int ou_spectral_mae(const float* est, const float* ref, int64_t stride, const int64_t* len_host, int32_t B,
                   const ou_metrics_spec* spec, int32_t n_spec, float time_domain_weight, float eps, int32_t flags, float* out,
                   void* scratch, size_t scratch_bytes, ou_stream_t stream) {
  long long len_max = 0;
  if (int rc = met_check_rows("ou_spectral_mae", est, ref, stride, len_host, B, &len_max)) return rc;
  if (!out || !scratch || (n_spec && !spec)) return fail(nullptr, OU_EINVAL, "ou_spectral_mae: null argument");
  if (n_spec < 0 || n_spec > OU_METRICS_MAX_SPECS)
    return fail(nullptr, OU_EINVAL, "ou_spectral_mae: 0 <= n_spec <= OU_METRICS_MAX_SPECS = " + std::to_string(OU_METRICS_MAX_SPECS));
  for (int i = 0; i < n_spec; i++) {
    const std::string m = met_spec_error(spec[i]);
    if (!m.empty()) return fail(nullptr, OU_EINVAL, "ou_spectral_mae: spec " + std::to_string(i) + ": " + m);
  }
  if (flags & ~OU_MET_SCALE_INVARIANT) return fail(nullptr, OU_EINVAL, "ou_spectral_mae: the only flag is OU_MET_SCALE_INVARIANT");
  if (!(eps >= 0.0f) || !std::isfinite(time_domain_weight))
    return fail(nullptr, OU_EINVAL, "ou_spectral_mae: eps must not be negative and time_domain_weight must be finite");
  const MetLayout L = met_layout(B, len_max, spec, n_spec);
  if (scratch_bytes < L.bytes)
    return fail(nullptr, OU_ESHAPE, "ou_spectral_mae: scratch of " + std::to_string(scratch_bytes) +
                                        " bytes, ou_metrics_scratch_bytes asks for " + std::to_string(L.bytes));
  char* base = static_cast<char*>(scratch);
  double* tsum = reinterpret_cast<double*>(base + L.tsum);
  double* window = reinterpret_cast<double*>(base + L.window);
  double* basis = reinterpret_cast<double*>(base + L.basis);
  double* partial = reinterpret_cast<double*>(base);  // (MetSpecs.offset counts doubles from here)
  const hipStream_t st = (hipStream_t)stream;
  MetSpecs specs;
  specs.n = n_spec;
  for (int i = 0; i < kMetMaxSpecs; i++) {
    specs.hop[i] = i < n_spec ? spec[i].hop : 1;
    specs.nbins[i] = i < n_spec ? spec[i].n_fft / 2 + 1 : 1;
    specs.offset[i] = i < n_spec ? (long long)(L.partial[i] / sizeof(double)) : 0;
    specs.tile_stride[i] = L.tile_stride[i];
  }
  std::vector<MetRows> rows((size_t)(B + kMetRowsPerLaunch - 1) / kMetRowsPerLaunch);
  std::vector<int> cnt(rows.size());
  std::vector<long long> lm(rows.size());
  for (size_t c = 0; c < rows.size(); c++) {
    met_rows_of(len_host, B, (int)c * kMetRowsPerLaunch, rows[c], cnt[c], lm[c]);
    if (int rc = met_hip("ou_spectral_mae", launch_met_time(est, ref, stride, rows[c], cnt[c], (int)c * kMetRowsPerLaunch, eps,
                                                           flags & OU_MET_SCALE_INVARIANT, tsum, st)))
      return rc;
  }
  for (int i = 0; i < n_spec; i++) {  // one basis at a time in the same words: the stream orders build, use, rebuild
    if (int rc = met_hip("ou_spectral_mae", launch_met_basis(basis, window, spec[i].n_fft, st))) return rc;
    for (size_t c = 0; c < rows.size(); c++)
      if (int rc = met_hip("ou_spectral_mae",
                           launch_met_stft(true, est, ref, stride, rows[c], cnt[c], (int)c * kMetRowsPerLaunch, lm[c], basis, window,
                                           tsum, spec[i].n_fft, spec[i].hop, 1.0, 0.0f, false, partial + specs.offset[i],
                                           L.tile_stride[i], st)))
        return rc;
  }
  for (size_t c = 0; c < rows.size(); c++)
    if (int rc = met_hip("ou_spectral_mae", launch_met_final_l1(rows[c], cnt[c], (int)c * kMetRowsPerLaunch, partial, specs, tsum,
                                                               time_domain_weight, out, st)))
      return rc;
  return OU_OK;
}

int ou_si_sdr(const float* est, const float* ref, int64_t stride, const int64_t* len_host, int32_t B, float clamp_db,
              float* out_si_sdr, float* out_snr, void* scratch, size_t scratch_bytes, ou_stream_t stream) {
  long long len_max = 0;
  if (int rc = met_check_rows("ou_si_sdr", est, ref, stride, len_host, B, &len_max)) return rc;
  if (!scratch || (!out_si_sdr && !out_snr)) return fail(nullptr, OU_EINVAL, "ou_si_sdr: null argument");
  if (!(clamp_db > 0.0f) || !std::isfinite(clamp_db)) return fail(nullptr, OU_EINVAL, "ou_si_sdr: clamp_db must be positive and finite");
  const MetLayout L = met_layout(B, len_max, nullptr, 0);
  if (scratch_bytes < L.bytes)
    return fail(nullptr, OU_ESHAPE, "ou_si_sdr: scratch of " + std::to_string(scratch_bytes) +
                                        " bytes, ou_metrics_scratch_bytes asks for " + std::to_string(L.bytes));
  char* base = static_cast<char*>(scratch);
  double* tsum = reinterpret_cast<double*>(base + L.tsum);
  const hipStream_t st = (hipStream_t)stream;
  for (int off = 0; off < B; off += kMetRowsPerLaunch) {
    MetRows rows;
    int n;
    long long lm;
    met_rows_of(len_host, B, off, rows, n, lm);
    if (int rc = met_hip("ou_si_sdr", launch_met_time(est, ref, stride, rows, n, off, 0.0f, false, tsum, st))) return rc;
    if (int rc = met_hip("ou_si_sdr", launch_met_final_sdr(n, off, tsum, clamp_db, out_si_sdr, out_snr, st))) return rc;
  }
  return OU_OK;
}

}  // extern "C"

// ---- ou_sdr: the BSS-eval SDR (kernels: ou_sdr.hip) ---------------------------------------------------------------------
namespace {
// scratch of one call: | tsum (B, 8) double | partial (B, tiles of the longest row, 2, L) double |
struct SdrLayout {
  size_t tsum = 0, partial = 0, bytes = 0;
  long long tile_stride = 0;
};
SdrLayout sdr_layout(int B, long long T_max, int L) {
  SdrLayout s;
  size_t at = 0;
  s.tsum = at; at = met_align(at + (size_t)B * 8 * sizeof(double));
  s.tile_stride = sdr_tiles(T_max);
  s.partial = at; at = met_align(at + (size_t)B * (size_t)s.tile_stride * 2 * (size_t)L * sizeof(double));
  s.bytes = at;
  return s;
}
std::string sdr_filter_error(int L) {
  return "filter_length = " + std::to_string(L) + " must lie in 1 .. OU_SDR_MAX_FILTER = " + std::to_string(OU_SDR_MAX_FILTER);
}
}  // namespace

extern "C" {

int ou_sdr_scratch_bytes(int32_t B, int64_t T_max, int32_t filter_length, size_t* nbytes) {
  if (!nbytes || B < 1 || T_max < 1 || T_max > kMetMaxLen)
    return fail(nullptr, OU_EINVAL, "ou_sdr_scratch_bytes: B >= 1, 1 <= T_max <= 2^31 - 1");
  if (filter_length < 1 || filter_length > OU_SDR_MAX_FILTER)
    return fail(nullptr, OU_EINVAL, "ou_sdr_scratch_bytes: " + sdr_filter_error(filter_length));
  *nbytes = sdr_layout(B, T_max, filter_length).bytes;
  return OU_OK;
}

int ou_sdr(const float* est, const float* ref, int64_t stride, const int64_t* len_host, int32_t B, int32_t filter_length,
           float clamp_db, float* out, void* scratch, size_t scratch_bytes, ou_stream_t stream) {
  static_assert(OU_SDR_MAX_FILTER == kSdrMaxFilter, "the header's cap is the kernels'");
  long long len_max = 0;
  if (int rc = met_check_rows("ou_sdr", est, ref, stride, len_host, B, &len_max)) return rc;
  if (!scratch || !out) return fail(nullptr, OU_EINVAL, "ou_sdr: null argument");
  if (filter_length < 1 || filter_length > OU_SDR_MAX_FILTER) return fail(nullptr, OU_EINVAL, "ou_sdr: " + sdr_filter_error(filter_length));
  if (!(clamp_db > 0.0f) || !std::isfinite(clamp_db)) return fail(nullptr, OU_EINVAL, "ou_sdr: clamp_db must be positive and finite");
  const SdrLayout L = sdr_layout(B, len_max, filter_length);
  if (scratch_bytes < L.bytes)
    return fail(nullptr, OU_ESHAPE, "ou_sdr: scratch of " + std::to_string(scratch_bytes) + " bytes, ou_sdr_scratch_bytes asks for " +
                                        std::to_string(L.bytes));
  char* base = static_cast<char*>(scratch);
  double* tsum = reinterpret_cast<double*>(base + L.tsum);
  double* partial = reinterpret_cast<double*>(base + L.partial);
  const hipStream_t st = (hipStream_t)stream;
  for (int off = 0; off < B; off += kMetRowsPerLaunch) {
    MetRows rows;
    int n;
    long long lm;
    met_rows_of(len_host, B, off, rows, n, lm);
    if (int rc = met_hip("ou_sdr", launch_met_time(est, ref, stride, rows, n, off, 0.0f, false, tsum, st))) return rc;
    if (int rc = met_hip("ou_sdr", launch_sdr_corr(est, ref, stride, rows, n, off, lm, filter_length, partial, L.tile_stride, st)))
      return rc;
    if (int rc = met_hip("ou_sdr", launch_sdr_solve(rows, n, off, partial, L.tile_stride, tsum, filter_length, clamp_db, out, st)))
      return rc;
  }
  return OU_OK;
}

}  // extern "C"

// ---- ou_stoi: STOI and extended STOI (kernels: ou_stoi.hip) --------------------------------------------------------------
namespace {
// What a sample rate asks of the 10 kHz resampler (include/ouniverse.h, step 1 of the definition): a pure host function of fs.
struct StoiPlan {
  int fs = 0;
  int p = 1, q = 1, L = 0, taps = 0;  // taps per output (0: fs is 10 kHz, nothing is resampled)
  size_t table_bytes = 0;
  std::vector<char> table;            // int first[p] padded to an even count, double coef[taps][p]
  std::string error;                  // why this fs is refused, or empty
};

// I0 by its power series sum_k ((x / 2)^k / k!)^2; the terms fall below 2^-53 of the sum after about 25 of them at beta = 5.65
double stoi_i0(double x) {
  const double h = 0.5 * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; k++) {
    term *= (h / (double)k) * (h / (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}
inline long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }  // b > 0
inline long long ceil_div(long long a, long long b) { return -floor_div(-a, b); }

const StoiPlan& stoi_plan(int fs) {
  thread_local StoiPlan pl;
  thread_local bool cached = false;
  if (cached && pl.fs == fs) return pl;
  pl = StoiPlan();
  pl.fs = fs;
  cached = true;
  if (fs < 1) {
    pl.error = "fs = " + std::to_string(fs) + " must be at least 1";
    return pl;
  }
  if (fs == 10000) return pl;
  const long long g = gcd_ll(10000, fs);
  const long long p = 10000 / g, q = fs / g, mx = p > q ? p : q;
  const double fc = 1.0 / (2.0 * (double)mx);
  const double Ld = std::ceil(52.0 / (28.714 * fc / 10.0));
  const double taps_d = std::ceil((2.0 * Ld + 1.0) / (double)p);
  const double bytes_d = ((double)((p + 1) & ~1ll)) * 4.0 + taps_d * (double)p * 8.0;
  if (taps_d > (double)OU_STOI_MAX_TAPS || bytes_d > (double)OU_STOI_MAX_TABLE_BYTES) {
    pl.error = "fs = " + std::to_string(fs) + ": the 10 kHz resampling filter (10000 / " + std::to_string(fs) + " = " +
               std::to_string(p) + " / " + std::to_string(q) + ") needs " + std::to_string((long long)taps_d) +
               " taps per output and a table of " + std::to_string((long long)bytes_d) + " bytes; the caps are OU_STOI_MAX_TAPS = " +
               std::to_string(OU_STOI_MAX_TAPS) + " and OU_STOI_MAX_TABLE_BYTES = " + std::to_string(OU_STOI_MAX_TABLE_BYTES);
    return pl;
  }
  const long long L = (long long)Ld;
  pl.p = (int)p; pl.q = (int)q; pl.L = (int)L;
  // h[t + L] = 2 p fc sinc(2 fc t) kaiser(2 L + 1, beta)[t + L], normalised to sum 1, times p
  const double beta = 0.1102 * (60.0 - 8.7), i0b = stoi_i0(beta);
  std::vector<double> h((size_t)(2 * L + 1));
  double sum = 0.0;
  for (long long k = 0; k <= 2 * L; k++) {
    const double t = (double)(k - L), u = t / (double)L;
    const double x = M_PI * (2.0 * fc * t);
    const double sinc = k == L ? 1.0 : std::sin(x) / x;
    const double kaiser = stoi_i0(beta * std::sqrt(1.0 - u * u)) / i0b;
    h[(size_t)k] = 2.0 * (double)p * fc * sinc * kaiser;
    sum += h[(size_t)k];
  }
  for (double& v : h) v = v / sum * (double)p;
  // output j = f p + ph: sum_k h[k] xup[j q + L - k], xup[i p] = x[i]  ->  i = f q + i', k = ph q + L - i' p in [0, 2 L]:
  // i' from ceil((ph q - L) / p) to floor((ph q + L) / p), ascending
  long long taps = 0;
  for (long long ph = 0; ph < p; ph++) {
    const long long n = floor_div(ph * q + L, p) - ceil_div(ph * q - L, p) + 1;
    taps = n > taps ? n : taps;
  }
  pl.taps = (int)taps;
  const size_t first_words = (size_t)((p + 1) & ~1ll);
  pl.table_bytes = first_words * 4 + (size_t)taps * (size_t)p * 8;
  pl.table.assign(pl.table_bytes, 0);
  int32_t* first = reinterpret_cast<int32_t*>(pl.table.data());
  double* coef = reinterpret_cast<double*>(pl.table.data() + first_words * 4);
  for (long long ph = 0; ph < p; ph++) {
    const long long a = ceil_div(ph * q - L, p);
    first[ph] = (int32_t)a;
    for (long long t = 0; t < taps; t++) {
      const long long k = ph * q + L - (a + t) * p;
      coef[(size_t)t * (size_t)p + (size_t)ph] = (k >= 0 && k <= 2 * L) ? h[(size_t)k] : 0.0;
    }
  }
  return pl;
}

inline long long stoi_len10(long long T, const StoiPlan& pl) { return (T * pl.p + pl.q - 1) / pl.q; }  // ceil(T p / q)

// scratch of one call: | table | window | basis | res (2, B, n10) | energy (B, F) | src (B, F) | count (B) | bands (B, 2, 15, F) |
// partial (B, segment tiles) |, F = stoi_frames(n10 of the longest row)
struct StoiLayout {
  size_t table = 0, window = 0, basis = 0, res = 0, energy = 0, src = 0, count = 0, bands = 0, partial = 0, bytes = 0;
  long long n10 = 0, F = 0, seg_stride = 0;
};
StoiLayout stoi_layout(int B, long long T_max, const StoiPlan& pl) {
  StoiLayout s;
  s.n10 = stoi_len10(T_max, pl);
  s.F = stoi_frames(s.n10);
  s.seg_stride = stoi_seg_tiles(s.F);
  const size_t nb = (size_t)B, F = (size_t)s.F;
  size_t at = 0;
  s.table = at; at = met_align(at + pl.table_bytes);
  s.window = at; at = met_align(at + kStoiFrame * sizeof(double));
  s.basis = at; at = met_align(at + kStoiBasisWords * sizeof(double));
  s.res = at; at = met_align(at + (pl.taps ? 2 * nb * (size_t)s.n10 * sizeof(double) : 0));
  s.energy = at; at = met_align(at + nb * F * sizeof(double));
  s.src = at; at = met_align(at + nb * F * sizeof(int));
  s.count = at; at = met_align(at + nb * sizeof(int));
  s.bands = at; at = met_align(at + nb * 2 * kStoiBands * F * sizeof(double));
  s.partial = at; at = met_align(at + nb * (size_t)s.seg_stride * sizeof(double));
  s.bytes = at;
  return s;
}
// the message of a T_max this fs cannot take, or empty
std::string stoi_length_error(long long T_max, const StoiPlan& pl) {
  if (stoi_len10(T_max, pl) > kMetMaxLen)  // (T_max p fits 64 bits: T_max < 2^31, p <= 10000)
    return "a row of " + std::to_string(T_max) + " samples at fs = " + std::to_string(pl.fs) + " has more than 2^31 - 1 samples at 10 kHz";
  return std::string();
}
}  // namespace

extern "C" {

int32_t ou_stoi_frame_tile(void) { return kStoiFrameTile; }

int ou_stoi_scratch_bytes(int32_t B, int64_t T_max, int32_t fs, size_t* nbytes) {
  if (!nbytes || B < 1 || T_max < 1 || T_max > kMetMaxLen)
    return fail(nullptr, OU_EINVAL, "ou_stoi_scratch_bytes: B >= 1, 1 <= T_max <= 2^31 - 1");
  const StoiPlan& pl = stoi_plan(fs);
  if (!pl.error.empty()) return fail(nullptr, OU_EINVAL, "ou_stoi_scratch_bytes: " + pl.error);
  const std::string m = stoi_length_error(T_max, pl);
  if (!m.empty()) return fail(nullptr, OU_EINVAL, "ou_stoi_scratch_bytes: " + m);
  *nbytes = stoi_layout(B, T_max, pl).bytes;
  return OU_OK;
}

int ou_stoi(const float* est, const float* ref, int64_t stride, const int64_t* len_host, int32_t B, int32_t fs, int32_t extended,
            float* out, void* scratch, size_t scratch_bytes, ou_stream_t stream) {
  static_assert(kStoiRowsPerLaunch == kMetRowsPerLaunch, "one launch group per 64 rows, as the other scores");
  // everything is decided here, on the host, before the first HIP call
  if (fs < 1) return fail(nullptr, OU_EINVAL, "ou_stoi: " + stoi_plan(fs).error);
  long long len_max = 0;
  if (int rc = met_check_rows("ou_stoi", est, ref, stride, len_host, B, &len_max)) return rc;
  if (!scratch || !out) return fail(nullptr, OU_EINVAL, "ou_stoi: null argument");
  const StoiPlan& pl = stoi_plan(fs);
  if (!pl.error.empty()) return fail(nullptr, OU_EINVAL, "ou_stoi: " + pl.error);
  const std::string m = stoi_length_error(len_max, pl);
  if (!m.empty()) return fail(nullptr, OU_EINVAL, "ou_stoi: " + m);
  const StoiLayout L = stoi_layout(B, len_max, pl);
  if (scratch_bytes < L.bytes)
    return fail(nullptr, OU_ESHAPE, "ou_stoi: scratch of " + std::to_string(scratch_bytes) + " bytes, ou_stoi_scratch_bytes asks for " +
                                        std::to_string(L.bytes));
  char* base = static_cast<char*>(scratch);
  double* window = reinterpret_cast<double*>(base + L.window);
  double* basis = reinterpret_cast<double*>(base + L.basis);
  double* energy = reinterpret_cast<double*>(base + L.energy);
  int* src = reinterpret_cast<int*>(base + L.src);
  int* count = reinterpret_cast<int*>(base + L.count);
  double* bands = reinterpret_cast<double*>(base + L.bands);
  double* partial = reinterpret_cast<double*>(base + L.partial);
  StoiSignals sig{est, ref, stride, nullptr, nullptr, 0};
  double *res_est = nullptr, *res_ref = nullptr;
  const hipStream_t st = (hipStream_t)stream;
  if (pl.taps) {
    res_est = reinterpret_cast<double*>(base + L.res);
    res_ref = res_est + (size_t)B * (size_t)L.n10;
    sig.res_stride = L.n10;
    // the plan's table outlives the call (it is the thread's cache, and a pageable source is staged before the copy returns)
    if (int rc = met_hip("ou_stoi", hipMemcpyAsync(base + L.table, pl.table.data(), pl.table_bytes, hipMemcpyHostToDevice, st)))
      return rc;
  }
  if (int rc = met_hip("ou_stoi", launch_stoi_basis(basis, window, st))) return rc;
  const double clip = 1.0 + std::pow(10.0, 15.0 / 20.0);  // the estimate is clipped 15 dB above the clean band value
  for (int off = 0; off < B; off += kStoiRowsPerLaunch) {
    StoiRows rows;
    const int n = B - off < kStoiRowsPerLaunch ? B - off : kStoiRowsPerLaunch;
    long long n10_max = 0;
    for (int i = 0; i < kStoiRowsPerLaunch; i++) {
      rows.len[i] = i < n ? len_host[off + i] : 0;
      rows.n10[i] = i < n ? stoi_len10(rows.len[i], pl) : 0;
      n10_max = rows.n10[i] > n10_max ? rows.n10[i] : n10_max;
    }
    StoiSignals s = sig;  // the resampler reads the caller's rows; everything behind it the rows at 10 kHz
    if (pl.taps) {
      if (int rc = met_hip("ou_stoi", launch_stoi_resample(s, rows, n, off, n10_max, pl.p, pl.q, pl.taps, base + L.table, res_est,
                                                           res_ref, st)))
        return rc;
      s.res_est = res_est;
      s.res_ref = res_ref;
    }
    if (int rc = met_hip("ou_stoi", launch_stoi_energy(s, rows, n, off, n10_max, window, energy, L.F, st))) return rc;
    if (int rc = met_hip("ou_stoi", launch_stoi_mask(rows, n, off, energy, L.F, src, count, st))) return rc;
    if (int rc = met_hip("ou_stoi", launch_stoi_stft(s, rows, n, off, n10_max, basis, window, src, count, L.F, bands, st))) return rc;
    if (int rc = met_hip("ou_stoi", launch_stoi_segments(extended != 0, rows, n, off, n10_max, bands, count, L.F, clip, partial,
                                                         L.seg_stride, out, st)))
      return rc;
  }
  return OU_OK;
}

}  // extern "C"
