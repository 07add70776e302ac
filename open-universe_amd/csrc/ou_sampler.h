// What the segmented calls (ou_segments.cpp) use of the sampler driver (ou_sampler.cpp; private).
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ou_walk.h"

namespace ou {

// One plane of counter-based noise: dst[j][i] = i < len(j) ? z(seed, stream(j), draw, t0(j) + i) : 0 for the n_rows rows of a
// call, 64 rows per launch; `row(j, stream, t0, len)` describes row j.
template <typename RowFn>
void fill_noise_plane(Runner& r, float* dst, long long cols, int n_rows, unsigned long long seed, int draw, RowFn row) {
  for (int off = 0; off < n_rows && r.ok(); off += kNoiseRowsPerLaunch) {
    NoiseRows blk;
    const int n = n_rows - off < kNoiseRowsPerLaunch ? n_rows - off : kNoiseRowsPerLaunch;
    for (int i = 0; i < kNoiseRowsPerLaunch; i++) {
      blk.stream[i] = 0; blk.t0[i] = 0; blk.len[i] = 0;
      if (i < n) row(off + i, blk.stream[i], blk.t0[i], blk.len[i]);
    }
    r.launch("noise fill", [&] { return launch_noise_fill(dst + (size_t)off * cols, cols, cols, blk, n, seed, draw, r.st); });
  }
}

// Per-row lengths of a ragged call: every one in [1, T_max] and the longest equal to T_max.  `collapse`: when no row is shorter,
// `t_raw` becomes null -- nothing ragged about the batch: the plain path (and its fused kernels).
template <typename Len>
int check_rows(ou_handle* h, const char* who, char idx, const Len*& t_raw, int n, long long T_max, bool collapse) {
  long long mx = 0;
  bool all_whole = true;
  for (int i = 0; i < n; i++) {
    if (t_raw[i] < 1 || t_raw[i] > T_max) return fail(h, OU_EINVAL, std::string(who) + ": 1 <= t_raw[" + idx + "] <= T_raw_max");
    mx = std::max<long long>(mx, t_raw[i]);
    all_whole = all_whole && t_raw[i] == T_max;
  }
  if (mx != T_max) return fail(h, OU_EINVAL, std::string(who) + ": T_raw_max must be the length of the longest row");
  if (collapse && all_whole) t_raw = nullptr;
  return OU_OK;
}

int check_noise_source(ou_handle* h, const float* noise, int rows, const char* rows_wording, bool need_noise);
int check_steps(ou_handle* h, int n_steps, int warm_start);

// What a forward call does to the handle while it runs: the records of the previous call are dropped, and `serial` switches the
// side streams off until the call returns.
struct CallScope {
  ou_handle* h;
  bool saved_overlap;
  CallScope(ou_handle* h_, bool serial) : h(h_), saved_overlap(h_->overlap) {
    if (serial) h->overlap = false;
    h->tensors.clear();
    h->n_launch = h->n_conv = 0;
    h->ev_used = 0;
  }
  ~CallScope() { h->overlap = saved_overlap; }
  CallScope(const CallScope&) = delete;
  CallScope& operator=(const CallScope&) = delete;
};

// The sampler's constants: the sigma schedule (the caller's table where given) and one StepCoef row per step.
struct SamplerTables {
  std::vector<float> sigma;
  std::vector<StepCoef> coef;
  SamplerTables(const ou_config& cfg, int n_steps, double epsilon, const float* sigma_host) : sigma(n_steps) {
    double eta, beta;
    schedule(cfg, n_steps, epsilon, sigma.data(), &eta, &beta);
    if (sigma_host) std::memcpy(sigma.data(), sigma_host, sizeof(float) * n_steps);
    for (int n = 0; n < n_steps; n++)
      coef.push_back(make_coef(cfg, sigma[n], n == n_steps - 1, eta, beta, n + 1 < n_steps ? sigma[n + 1] : 0.f));
  }
  int n_steps() const { return (int)sigma.size(); }
  void upload_coef(Runner& r, Persist& P) const { upload_coefs(r, P.coef, coef); }
  // the FiLM rows of every step, from the uploaded coefficients (only a call that runs the score net needs them)
  void upload_film(Runner& r, Persist& P) const {
    upload_film_rows(r, P, n_steps());
  }
  void upload(Runner& r, Persist& P) const { upload_coef(r, P); upload_film(r, P); }
};

int set_levels(Runner& r, int T);

struct PostFlags {
  int keep_rms, peak;
  explicit PostFlags(uint32_t flags) : keep_rms((flags & OU_ENH_KEEP_RMS) ? 1 : 0), peak((flags & OU_ENH_NO_PEAK_GUARD) ? 0 : 1) {}
};

int check_decoupling(ou_handle* h);
void decouple(Runner& r, Persist& P);
void init_x(Runner& r, Persist& P, const float* z0, const float* warm, float sigma, int T, bool mask);
// A first score-encoder pass that already ran on side stream 2 (ou_enhance's overlap with the conditioner): its results and
// where its scratch ends.  Its init_x ran in front of it.
struct FirstPass {
  ScoreEnc E;
  size_t off_after_enc = 0;
};
// The sampler loop (universe.py:325-343) over the rows of r, steps n_start .. N - 1, every step on the same scratch.  `z(draw)`
// gives the noise plane of a draw -- 0: the initial noise, n + 1: z_n of step n -- and is called right in front of the launch
// that reads the plane, so what it enqueues (a fill, a gather) keeps its place in the stream.
template <typename NoiseFn>
void sample(Runner& r, Persist& P, int T, const SamplerTables& tab, int n_start, const float* warm, bool mask_x0, NoiseFn z,
            const FirstPass* first = nullptr) {
  const Model& m = r.h->m;
  const int n_steps = tab.n_steps();
  if (!first) init_x(r, P, z(0), warm, tab.sigma[n_start], T, mask_x0);
  const size_t step_mark = r.off;
  for (int n = n_start; n < n_steps; n++) {
    const float* zn = n == n_steps - 1 ? nullptr : z(n + 1);
    const StepCoef* cf = P.coef + n;
    const float* fr = P.film + (size_t)n * m.film.rows;
    if (first && n == n_start) {
      r.join(2, r.st);
      r.off = first->off_after_enc;
      run_score_dec(r, P, first->E, P.x.p, zn, P.x.p, OUT_UPDATE, cf, 0, fr, 0, T);
    } else {
      r.off = step_mark;
      run_score(r, P, P.x.p, zn, P.x.p, OUT_UPDATE, cf, 0, fr, 0, T);
    }
    if (!r.ok()) break;
  }
}

void replicate_conditioned(Runner& r, Persist& P, int rows, int E, bool with_stats, bool with_wav);

}  // namespace ou
