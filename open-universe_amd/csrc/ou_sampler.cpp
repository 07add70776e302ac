// The sampler driver: the pieces the enhance entry points share, ou_enhance / ou_enhance_var and
// ou_enhance_ensemble built from them, and the operator seams (ou_condition, ou_score, ou_aux_to_wav, ou_sampler_step).
#include "ou_sampler.h"

#include <cmath>

using namespace ou;

extern "C" {

int ou_schedule(const ou_config* cfg, int32_t n_steps, double epsilon, float* sigma_out, double* eta, double* beta) {
  if (!cfg || !sigma_out || !eta || !beta || n_steps < 2) return fail(nullptr, OU_EINVAL, "bad argument");
  schedule(*cfg, n_steps, epsilon, sigma_out, eta, beta);
  return OU_OK;
}

int ou_condition(ou_handle* h, const float* mix_norm, int32_t B, int32_t T, void* ws, size_t ws_bytes, ou_stream_t stream) {
  if (!h || !mix_norm || !ws || B < 1) return fail(h, OU_EINVAL, "bad argument");
  if (T % h->m.tot_ds || T <= 0) return fail(h, OU_EINVAL, "T must be a positive multiple of the total down-sampling factor");
  if (!h->ws_ok(ws, ws_bytes, B, T))
    return fail(h, OU_EINVAL, "workspace was not prepared by ou_workspace_init for this (B, T)");
  h->tensors.clear();
  h->n_launch = h->n_conv = 0;
  h->ev_used = 0;
  Runner r(h, ws, ws_bytes, false, (hipStream_t)stream, B);
  Persist P = layout_persist(r, T);
  if (r.oom) return finish(h, r);
  run_condition(r, P, mix_norm, T);
  h->cond_B = B;
  h->cond_T = T;
  return finish(h, r);
}

int ou_score(ou_handle* h, const float* x, const float* sigma_host, float* score_out, int32_t B, int32_t T, void* ws,
             size_t ws_bytes, ou_stream_t stream) {
  if (!h || !x || !sigma_host || !score_out || !ws) return fail(h, OU_EINVAL, "bad argument");
  if (B != h->cond_B || T != h->cond_T) return fail(h, OU_EINVAL, "ou_score: call ou_condition with the same (B, T) first");
  if (!h->ws_ok(ws, ws_bytes, B, T))
    return fail(h, OU_EINVAL, "workspace was not prepared by ou_workspace_init for this (B, T)");
  h->n_launch = h->n_conv = 0;
  Runner r(h, ws, ws_bytes, false, (hipStream_t)stream, B);
  auto keep = h->tensors;
  Persist P = layout_persist(r, T);
  {  // skip over the conditioner's region so that its intermediates stay inspectable
    Runner d(h, nullptr, 0, true, nullptr, B);
    Persist Pd = layout_persist(d, T);
    run_condition(d, Pd, nullptr, T);
    r.off = d.off;
  }
  for (auto& kv : keep) if (kv.first.rfind("cond.", 0) == 0) h->tensors[kv.first] = kv.second;
  std::vector<StepCoef> rows;
  for (int b = 0; b < B; b++) {
    if (!(sigma_host[b] > 0.f)) return fail(h, OU_EINVAL, "sigma must be positive");
    rows.push_back(make_coef(h->m.cfg, sigma_host[b], true, 0.0, 0.0, 0.f));
  }
  upload_coefs(r, P.coef, rows);
  const Model& m = h->m;
  upload_film_rows(r, P, B);
  run_score(r, P, x, nullptr, score_out, OUT_SCORE, P.coef, 1, P.film, m.film.rows, T);
  return finish(h, r);
}

int ou_aux_to_wav(ou_handle* h, float* wav_out, int32_t B, int32_t T, void* ws, size_t ws_bytes, ou_stream_t stream) {
  if (!h || !wav_out || !ws) return fail(h, OU_EINVAL, "bad argument");
  if (B != h->cond_B || T != h->cond_T) return fail(h, OU_EINVAL, "ou_aux_to_wav: call ou_condition with the same (B, T) first");
  const Model& m = h->m;
  if (!m.dec.present) return fail(h, OU_ENOTIMPL, "model has no signal decoupling layer (aux signal is multi-channel)");
  if (m.dec.act != OU_ACT_SNAKE) return fail(h, OU_ENOTIMPL, "only the snake signal-decoupling activation is implemented");
  Runner r(h, ws, ws_bytes, false, (hipStream_t)stream, B);
  auto keep = h->tensors;
  Persist P = layout_persist(r, T);
  h->tensors = keep;
  // scratch at the very end of the workspace
  size_t need = (size_t)B * m.C0 * 2 * T * 4;
  if (ws_bytes < need + r.off) return fail(h, OU_ENOMEM, "workspace too small");
  float* tmp = (float*)((char*)ws + ((ws_bytes - need) & ~size_t(255)));
  r.launch("decoupling", [&] {
    return launch_decoupling(P.aux.p, r.W(m.dec.alpha_off), r.W(m.dec.up_off), r.W(m.dec.down_off), r.W(m.dec.conv.w_off),
                             r.W(m.dec.conv.b_off), tmp, wav_out, B, m.C0, T, r.st);
  });
  return finish(h, r);
}

}  // extern "C"

// ---- the pieces the enhance entry points share.  ou_enhance / ou_enhance_var, ou_enhance_ensemble,
// ou_enhance_segments and ou_enhance_segments_var are these pieces plus what each adds of its own.

namespace ou {
// The caller's noise tensor against the handle's noise source (ou_set_noise_source): exactly one of them, and one stream id
// per row (`rows_wording`: how the message names the rows).  `need_noise`: the call draws noise at all.
int check_noise_source(ou_handle* h, const float* noise, int rows, const char* rows_wording, bool need_noise) {
  const bool counter = h->noise_src.on;
  if (counter && noise)
    return fail(h, OU_EINVAL, "a noise source is set on this handle (ou_set_noise_source): `noise` must be NULL");
  if (counter && (int)h->noise_src.streams.size() != rows)
    return fail(h, OU_EINVAL, "noise source: n_streams (" + std::to_string(h->noise_src.streams.size()) + ") must equal " +
                                  rows_wording + std::to_string(rows) + ")");
  if (need_noise && !noise && !counter) return fail(h, OU_EINVAL, "noise must be given");
  return OU_OK;
}
int check_steps(ou_handle* h, int n_steps, int warm_start) {
  if (n_steps < 2 || n_steps > kMaxSteps) return fail(h, OU_EINVAL, "n_steps must be in [2, 256]");
  if (warm_start >= n_steps) return fail(h, OU_EINVAL, "warm_start must be < n_steps");
  return OU_OK;
}
}  // namespace ou

namespace {
// counter mode: the two (rows, T) planes of the caller's scratch (`hint`: what the message says about its size)
int check_noise_scratch(ou_handle* h, int rows, int T, const char* hint) {
  const size_t need = (size_t)2 * rows * T * sizeof(float);
  if (!h->noise_src.scratch || h->noise_src.scratch_bytes < need)
    return fail(h, OU_ENOMEM, "noise source: scratch too small: need " + std::to_string(need) + " bytes (" + hint + ")");
  return OU_OK;
}
// the length guard (max_walk_length) of the calls that take whole rows in one pass
int check_walk_length(ou_handle* h, int T_raw, int T, bool need_wav, const char* advice) {
  const long long t_max = max_walk_length(h, need_wav);
  if (T > t_max)
    return fail(h, OU_EINVAL, "input too long for one pass: " + std::to_string(T_raw) + " samples padded to " +
                                  std::to_string(T) + " make a plane of the walk reach 2^32 bytes (at most " +
                                  std::to_string(t_max) + " padded samples)" + advice);
  return OU_OK;
}
}  // namespace

namespace ou {
// Ragged walk: the levels on which rows have lengths of their own -- T, 2 T (the decoupling layer's up-sampled grid) and
// T / (r_0 .. r_i).
int set_levels(Runner& r, int T) {
  const Model& m = r.h->m;
  LevelSpec& lv = r.lv;
  lv.n = 0;
  auto add_level = [&](int num, int den) {
    lv.num[lv.n] = num; lv.den[lv.n] = den; r.level_T[lv.n] = (int)((long long)T * num / den); lv.n++;
  };
  add_level(1, 1);
  add_level(2, 1);
  int cum = 1;
  for (int i = 0; i < m.cfg.score.n_rates && lv.n < kMaxLenLevels; i++) { cum *= m.cfg.score.rate_factors[i]; add_level(1, cum); }
  if (cum != m.tot_ds) return fail(r.h, OU_EINVAL, "internal: rate factors do not multiply to the total down-sampling factor");
  return OU_OK;
}
}  // namespace ou

namespace {
// Per-row geometry and the rows' lengths on the levels of set_levels for `n` rows of raw lengths `t_raw`.  By value through
// kernel arguments: capturable, no host memory involved.
void upload_row_lengths(Runner& r, RowInfo* rows_dst, int* lens_dst, const int32_t* t_raw, int n) {
  for (int off = 0; off < n; off += 64) {
    RowBlock blk;
    const int k = n - off < 64 ? n - off : 64;
    for (int i = 0; i < 64; i++) blk.t_raw[i] = i < k ? t_raw[off + i] : 1;
    r.launch("upload rows", [&] { return launch_upload_rows(rows_dst, lens_dst, blk, k, off, n, r.h->m.tot_ds, r.lv, r.st); });
  }
}

// universe.py:219-223 + the level normalisation of `rows` inputs of T_raw samples (a ragged walk: of their own lengths) -> P.mixn
void normalize(Runner& r, Persist& P, const float* mix, int rows, int T_raw, int T) {
  const float level = (float)std::pow(10.0, (double)r.h->m.cfg.level_db / 20.0);
  const NormMode nm = r.h->norm;
  r.launch("normalize", [&] {
    return r.ragged ? launch_pad_normalize_var(mix, P.mixn.p, P.stats, P.rows, rows, T_raw, T, level, nm, r.st)
                    : launch_pad_normalize(mix, P.mixn.p, P.stats, rows, T_raw, T, (T - T_raw) / 2, level, nm, r.st);
  });
}
// unpad, de-normalise, keep_rms and the peak guard of `rows` rows of x -> out
void post(Runner& r, Persist& P, const float* x, float* out, int rows, int T_raw, int T, PostFlags f) {
  r.launch("post", [&] {
    return r.ragged ? launch_post_var(x, P.stats, out, P.rows, rows, T_raw, T, f.keep_rms, f.peak, r.st)
                    : launch_post(x, P.stats, out, rows, T_raw, T, (T - T_raw) / 2, f.keep_rms, f.peak, r.st);
  });
}
// Noise provider of the calls whose rows are whole signals: draw d is plane (d ? d - n_start : 0) of the caller's tensor, or --
// counter mode -- filled into plane d & 1 of the scratch right in front of the launch that reads it, on the caller's stream (the
// simplest place: the launches that read a plane are untouched, and at step n_start the fill runs beside the first score-encoder
// pass on its side stream).  Row b's positions are the columns of its own padded signal, the tail of a shorter row is 0.
// `t_raw`: raw length of every row of r, or null (all T).
auto row_noise(Runner& r, const float* noise, int n_start, int T, const int32_t* t_raw) {
  return [&r, noise, n_start, T, t_raw](int draw) -> const float* {
    const ou_handle::NoiseSource& src = r.h->noise_src;
    const size_t nBT = (size_t)r.B * T;
    if (!src.on) return noise + (size_t)(draw ? draw - n_start : 0) * nBT;
    float* dst = src.scratch + (size_t)(draw & 1) * nBT;
    const int tot = r.h->m.tot_ds;
    fill_noise_plane(r, dst, T, r.B, src.seed, draw, [&](int b, unsigned long long& sid, long long& t0, long long& len) {
      sid = src.streams[b];
      t0 = 0;
      len = t_raw ? t_raw[b] + (tot - t_raw[b] % tot) : T;
    });
    return dst;
  };
}
}  // namespace

namespace ou {
// what a call that needs P.wav asks of the model, on the host before anything is launched
int check_decoupling(ou_handle* h) {
  const Model& m = h->m;
  if (!m.dec.present || m.dec.act != OU_ACT_SNAKE)
    return fail(h, OU_ENOTIMPL, "aux_to_wav needs the snake signal-decoupling layer (UNIVERSE++)");
  return OU_OK;
}
// the signal decoupling layer: P.aux -> P.wav for the rows of r (scratch from the walk's bump allocator)
void decouple(Runner& r, Persist& P) {
  const Model& m = r.h->m;
  const int T = P.wav.T;
  float* tmp = r.alloc_raw((size_t)r.B * m.C0 * 2 * T);
  r.launch("decoupling", [&] {
    return launch_decoupling(P.aux.p, r.W(m.dec.alpha_off), r.W(m.dec.up_off), r.W(m.dec.down_off), r.W(m.dec.conv.w_off),
                             r.W(m.dec.conv.b_off), tmp, P.wav.p, r.B, m.C0, T, r.st, r.lens_of(T), r.lens_of(2 * T));
  });
}

// universe.py:325-327: x = sigma * z_0 (+ the warm start's signal).  `mask`: the plane may hold noise behind a row's own end.
void init_x(Runner& r, Persist& P, const float* z0, const float* warm, float sigma, int T, bool mask) {
  r.launch("init x", [&] { return launch_init_x(z0, warm, sigma, P.x.p, (size_t)r.B * T, r.st); });
  if (mask) r.mask(P.x);
}
}  // namespace ou

namespace {
// ou_enhance / ou_enhance_var.  `t_raw`: host array of B row lengths (max = T_raw) or null (every row T_raw samples long).
// Its own: the length guard, the dry walk for `mark`, the first score-encoder pass beside the conditioner, the use_aux exit.
int enhance_impl(ou_handle* h, const float* mix, float* out, const float* noise, int32_t B, int32_t T_raw,
                 const int32_t* t_raw, int32_t n_steps, double epsilon, const float* sigma_host, int32_t warm_start,
                 uint32_t flags, void* ws, size_t ws_bytes, ou_stream_t stream) {
  if (!h || !mix || !out || !ws || B < 1 || T_raw < 1) return fail(h, OU_EINVAL, "bad argument");
  if (t_raw)
    if (const int rc = check_rows(h, "ou_enhance_var", 'b', t_raw, B, T_raw, true)) return rc;
  const bool use_aux = (flags & OU_ENH_USE_AUX_SIGNAL) != 0;
  const bool counter = h->noise_src.on;
  if (const int rc = check_noise_source(h, noise, B, "the rows of the call (", !use_aux)) return rc;
  if (const int rc = check_steps(h, n_steps, warm_start)) return rc;
  const Model& m = h->m;
  const int T = T_raw + (m.tot_ds - T_raw % m.tot_ds);  // universe.py:219-223 (a full block when already a multiple)
  const bool need_wav = use_aux || warm_start >= 0;
  if (const int rc = check_walk_length(h, T_raw, T, need_wav, "; ou_enhance_segments enhances it in windows")) return rc;
  if (!h->ws_ok(ws, ws_bytes, B, T))
    return fail(h, OU_EINVAL, "workspace was not prepared by ou_workspace_init for this (B, T_raw + pad)");
  if (counter && !use_aux)
    if (const int rc = check_noise_scratch(h, B, T, "ou_noise_scratch_bytes")) return rc;
  // Side streams inside the call only when this is the one call on the device.  With several lanes (ou_set_lanes) every lane
  // is ONE chain on its caller's stream: HIP multiplexes its streams onto a handful of hardware queues, and four lanes with
  // four streams each alias there -- measured: 4 lanes 122 utt/s with side streams (87 % of the time ONE kernel on the
  // device), 209 utt/s as four chains (serial loop: 132).
  CallScope scope(h, (flags & OU_ENH_SERIAL) || h->lanes > 1);
  hipStream_t st = (hipStream_t)stream;
  Runner r(h, ws, ws_bytes, false, st, B);
  Persist P = layout_persist(r, T);
  if (r.oom) return finish(h, r);

  const SamplerTables tab(m.cfg, n_steps, epsilon, sigma_host);
  tab.upload_coef(r, P);
  if (t_raw) {
    if (const int rc = set_levels(r, T)) return rc;
    upload_row_lengths(r, P.rows, P.lens, t_raw, B);
    r.set_ragged(P.lens, P.rows);
  }
  if (need_wav)
    if (const int rc = check_decoupling(h)) return rc;
  const int n_start = warm_start >= 0 ? warm_start : 0;
  auto z = row_noise(r, noise, n_start, T, t_raw);

  // Where the conditioner's scratch ends (= where the per-step score scratch starts): layout is a pure function of
  // (config, B, T), so a dry walk gives it before anything is launched.
  size_t mark;
  {
    auto keep = h->tensors;
    Runner d(h, nullptr, 0, true, nullptr, B);
    Persist Pd = layout_persist(d, T);
    run_condition(d, Pd, nullptr, T);
    mark = d.off;
    h->tensors = keep;
  }

  // The first score-encoder pass (+ its GRU) does not depend on the conditioner: run it on side stream 2 while
  // the conditioner runs on the caller's stream (at batch 1 most CUs idle during the GRU passes of either).
  FirstPass first;
  bool have_first = false;
  if (!use_aux) {
    tab.upload_film(r, P);
    // (only when two GRU layers fit on the machine side by side: their clusters spin on each other's publishes and must
    // all be resident)
    const int share2 = Runner::gru_share_of(h->lanes, B, true);
    const bool gru_fit = (!m.s_has_gru || gru_ring_batch_cap(m.s_gru.H, h->num_cu, share2, 0, B, h->lanes) >= 1) &&
                         gru_ring_batch_cap(m.c_gru0.H, h->num_cu, share2, 0, B, h->lanes) >= 1;
    if (warm_start < 0 && h->overlap && gru_fit) {
      r.gru_shared = true;
      init_x(r, P, z(0), nullptr, tab.sigma[n_start], T, true);
      const size_t save = r.off;
      r.fork(st, 2);
      // (behind the fork: the side stream's first kernel starts an event latency -- ~10 us -- after the fork, and this launch is
      // what the device has to do in the meantime)
      normalize(r, P, mix, B, T_raw, T);
      r.st = h->aux[2];
      r.off = mark;
      first.E = run_score_enc(r, P, P.x.p, P.coef + n_start, 0, P.film + (size_t)n_start * m.film.rows, 0, T);
      first.off_after_enc = r.off;
      r.st = st;
      r.off = save;
      have_first = true;
    }
  }
  if (!have_first) normalize(r, P, mix, B, T_raw, T);
  run_condition(r, P, P.mixn.p, T);
  r.gru_shared = false;
  if (!r.dry && r.ok() && r.off != mark) return fail(h, OU_EINVAL, "internal: workspace layout mismatch");
  h->cond_B = r.ragged ? 0 : B;  // (the operator seams ou_score / ou_aux_to_wav take whole batches only)
  h->cond_T = T;

  if (need_wav) decouple(r, P);
  if (use_aux) {
    post(r, P, P.wav.p, out, B, T_raw, T, PostFlags(flags));
    return finish(h, r);
  }
  sample(r, P, T, tab, n_start, warm_start >= 0 ? P.wav.p : nullptr, true, z, have_first ? &first : nullptr);
  post(r, P, P.x.p, out, B, T_raw, T, PostFlags(flags));
  return finish(h, r);
}
}  // namespace

extern "C" {

int ou_enhance(ou_handle* h, const float* mix, float* out, const float* noise, int32_t B, int32_t T_raw, int32_t n_steps,
               double epsilon, const float* sigma_host, int32_t warm_start, uint32_t flags, void* ws, size_t ws_bytes,
               ou_stream_t stream) {
  return enhance_impl(h, mix, out, noise, B, T_raw, nullptr, n_steps, epsilon, sigma_host, warm_start, flags, ws, ws_bytes,
                      stream);
}

int ou_enhance_var(ou_handle* h, const float* mix, float* out, const float* noise, int32_t B, int32_t T_raw_max,
                   const int32_t* t_raw, int32_t n_steps, double epsilon, const float* sigma_host, int32_t warm_start,
                   uint32_t flags, void* ws, size_t ws_bytes, ou_stream_t stream) {
  if (!t_raw) return fail(h, OU_EINVAL, "ou_enhance_var: t_raw must be given (ou_enhance takes batches of equal lengths)");
  return enhance_impl(h, mix, out, noise, B, T_raw_max, t_raw, n_steps, epsilon, sigma_host, warm_start, flags, ws, ws_bytes,
                      stream);
}

}  // extern "C"

namespace {
// bytes of the ensemble call's own area, right behind the persistent block of the (E * B)-row workspace
struct EnsArea {
  size_t lens_b, members, hist, total;
};
EnsArea ens_area(int B, int E, long long cols) {
  EnsArea a;
  size_t off = 0;
  a.lens_b = off; off += align256((size_t)B * kMaxLenLevels * 4);      // the conditioner's own [level][B] length table (ragged, shared)
  a.members = off; off += align256((size_t)E * B * (size_t)cols * 4);  // post-processed member planes (members_out == NULL)
  a.hist = off; off += align256(((size_t)B * E + B) * 4);              // signal median: histogram [B][E] + picks [B]
  a.total = off;
  return a;
}

// Replication over the members of an ensemble: the first n words at p (rows [0, rows) of a tensor laid out for E * rows rows)
// -> the E - 1 blocks behind them, kReplicateEntries tensors per launch.
class Replicator {
  Runner& r;
  const int E;
  ReplicateTable tab;
  int n = 0;

 public:
  Replicator(Runner& r_, int E_) : r(r_), E(E_) {}
  void add(void* p, size_t words) {
    if (n == kReplicateEntries) flush();
    tab.p[n] = (unsigned*)p;
    tab.n[n] = (long long)words;
    n++;
  }
  void add(const Tensor& t, int rows) { add(t.p, (size_t)rows * t.C * t.T); }
  void flush() {
    if (n) r.launch("replicate rows", [&] { return launch_replicate_rows(tab, n, E, r.st); });
    n = 0;
  }
};
}  // namespace

namespace ou {
// What the score passes read per row of a conditioner that ran over the first `rows` rows only -> the rows of the other members.
// `with_stats`: the input statistics the post step reads per member row (a call whose post step works on whole long rows keeps
// them elsewhere); `with_wav`: the decoupling layer's output (warm start).
void replicate_conditioned(Runner& r, Persist& P, int rows, int E, bool with_stats, bool with_wav) {
  Replicator rep(r, E);
  for (size_t j = 0; j < P.cond.size(); j++) { rep.add(P.cond[j], rows); rep.add(P.sc[j], rows); }
  rep.add(P.aux, rows);
  rep.add(P.latent, rows);
  rep.add(P.mixn, rows);
  if (with_stats) rep.add(P.stats, (size_t)rows * 4);
  rep.add(P.mel_scale, (size_t)rows);
  if (with_wav) rep.add(P.wav, rows);
  rep.flush();
}
}  // namespace ou

namespace {
// ou_enhance_ensemble: the shared pieces as ONE chain on the caller's stream for the E * B member rows.  Its own: the area
// behind the persistent block, the conditioner (and, for a warm start, the decoupling layer) run once over the B inputs on a
// second runner and replicated -- ens_share = 0: run over all E * B rows --, the post step per member row and the reduce.
int ensemble_impl(ou_handle* h, const float* mix, float* out, float* members_out, const float* noise, int32_t B, int32_t T_raw,
                  const int32_t* t_raw, int32_t E, int32_t stat, int32_t n_steps, double epsilon, const float* sigma_host,
                  int32_t warm_start, uint32_t flags, void* ws, size_t ws_bytes, ou_stream_t stream) {
  if (!h || !mix || !out || !ws || B < 1 || T_raw < 1) return fail(h, OU_EINVAL, "bad argument");
  if (E < 1 || E > OU_MAX_ENSEMBLE)
    return fail(h, OU_EINVAL, "ou_enhance_ensemble: 1 <= E <= " + std::to_string(OU_MAX_ENSEMBLE));
  if (stat != OU_ENS_MEAN && stat != OU_ENS_MEDIAN && stat != OU_ENS_SIGNAL_MEDIAN)
    return fail(h, OU_EINVAL, "ou_enhance_ensemble: stat must be OU_ENS_MEAN, OU_ENS_MEDIAN or OU_ENS_SIGNAL_MEDIAN");
  if (flags & OU_ENH_USE_AUX_SIGNAL)
    return fail(h, OU_EINVAL, "ou_enhance_ensemble: OU_ENH_USE_AUX_SIGNAL is refused (without noise all members are equal)");
  if ((long long)E * B > 0x7fffffffll / 64) return fail(h, OU_EINVAL, "ou_enhance_ensemble: too many rows");
  if (t_raw)
    if (const int rc = check_rows(h, "ou_enhance_ensemble", 'b', t_raw, B, T_raw, true)) return rc;
  const int EB = E * B;
  if (const int rc = check_noise_source(h, noise, EB, "the member rows of the call (E * B = ", true)) return rc;
  if (const int rc = check_steps(h, n_steps, warm_start)) return rc;
  const Model& m = h->m;
  const int T = T_raw + (m.tot_ds - T_raw % m.tot_ds);  // universe.py:219-223 (a full block when already a multiple)
  const bool need_wav = warm_start >= 0;
  if (const int rc = check_walk_length(h, T_raw, T, need_wav, "")) return rc;  // (per-row planes do not grow with E)
  if (!h->ws_ok(ws, ws_bytes, EB, T))
    return fail(h, OU_EINVAL, "workspace was not prepared by ou_workspace_init for this (E * B, T_raw + pad)");
  if (h->noise_src.on)
    if (const int rc = check_noise_scratch(h, EB, T, "ou_noise_scratch_bytes for E * B rows")) return rc;
  if (need_wav)
    if (const int rc = check_decoupling(h)) return rc;
  CallScope scope(h, true);  // one chain on the caller's stream (the conditioner || first-encoder overlap of ou_enhance is dropped)
  hipStream_t st = (hipStream_t)stream;
  const bool share = h->opt.ens_share != 0 && E > 1;
  const int Bc = share ? B : EB;  // rows of the conditioner pass

  // ---- layout: the persistent block for E * B rows (what ou_workspace_init prepared), the ensemble's own area, then the
  // conditioner's scratch (Bc rows) and the per-step score scratch (E * B rows)
  Runner r(h, ws, ws_bytes, false, st, EB);
  Persist P = layout_persist(r, T);
  const EnsArea A = ens_area(B, E, T_raw);
  char* area = (char*)r.alloc_raw(A.total / 4);
  if (r.oom) return finish(h, r);
  int* lens_b = (int*)(area + A.lens_b);
  float* members = members_out ? members_out : (float*)(area + A.members);
  int* hist = (int*)(area + A.hist);

  const SamplerTables tab(m.cfg, n_steps, epsilon, sigma_host);
  tab.upload_coef(r, P);

  std::vector<int32_t> t_rep;  // member-major lengths: row e * B + b has t_raw[b]
  if (t_raw) {
    t_rep.resize(EB);
    for (int e = 0; e < E; e++)
      for (int b = 0; b < B; b++) t_rep[(size_t)e * B + b] = t_raw[b];
    if (const int rc2 = set_levels(r, T)) return rc2;
    // E copies of the per-row geometry for the sampler loop; the length table is [level][rows], so the conditioner's B-row pass
    // gets a table of its own ([level][B]; the RowInfo entries of rows 0 .. B - 1 serve both)
    upload_row_lengths(r, P.rows, P.lens, t_rep.data(), EB);
    r.set_ragged(P.lens, P.rows);
    // (its RowInfo output goes to rows 0 .. B - 1 of P.rows once more: the same values)
    if (share) upload_row_lengths(r, P.rows, lens_b, t_raw, B);
  }
  tab.upload_film(r, P);

  // ---- pad + normalise the B inputs (one workgroup per row: what the replicated batch would give, bit for bit)
  normalize(r, P, mix, B, T_raw, T);
  if (!share && E > 1) {  // the conditioner runs over all member rows: only its input is replicated
    Replicator rep(r, E);
    rep.add(P.mixn, B);
    rep.add(P.stats, (size_t)B * 4);
    rep.flush();
  }

  // ---- conditioner (+ decoupling layer for a warm start) over Bc rows, on a runner of its own (ragged: with its own [level][B]
  // length table when it runs B of the E * B rows; the RowInfo entries of rows 0 .. B - 1 serve both)
  Runner rc = Runner::conditioner_of(r, Bc);
  if (r.ragged) rc.set_ragged(share ? lens_b : P.lens, P.rows);
  run_condition(rc, P, P.mixn.p, T);
  h->cond_B = 0;  // (the operator seams ou_score / ou_aux_to_wav do not take this layout)
  h->cond_T = T;
  if (need_wav) decouple(rc, P);
  if (!rc.ok()) return finish(h, rc);
  if (share) replicate_conditioned(r, P, B, E, true, need_wav);

  // ---- the sampler loop at E * B rows
  r.off = rc.off;
  const int n_start = need_wav ? warm_start : 0;
  sample(r, P, T, tab, n_start, need_wav ? P.wav.p : nullptr, true, row_noise(r, noise, n_start, T, t_raw ? t_rep.data() : nullptr));
  if (!r.ok()) return finish(h, r);

  // ---- per member row: unpad, keep_rms (the mix RMS of the member's own input: stats row e B + b = row b), peak guard
  post(r, P, P.x.p, members, EB, T_raw, T, PostFlags(flags));
  // ---- reduce over the members
  std::vector<long long> len64;
  if (t_raw) len64.assign(t_raw, t_raw + B);
  r.launch("ensemble reduce", [&] {
    return launch_ensemble_reduce(members, out, E, B, T_raw, T_raw, t_raw ? len64.data() : nullptr, stat, hist, hist + (size_t)B * E,
                                  st);
  });
  return finish(h, r);
}
}  // namespace

extern "C" {

int ou_ensemble_workspace_bytes(const ou_handle* hc, int32_t B, int32_t T_pad_max, int32_t E, size_t* nbytes) {
  ou_handle* h = const_cast<ou_handle*>(hc);
  if (!h || !nbytes || B < 1 || T_pad_max < 1) return fail(h, OU_EINVAL, "bad argument");
  if (E < 1 || E > OU_MAX_ENSEMBLE || (long long)E * B > 0x7fffffffll / 64)
    return fail(h, OU_EINVAL, "ou_ensemble_workspace_bytes: 1 <= E <= " + std::to_string(OU_MAX_ENSEMBLE));
  size_t walk = 0;
  const int rc = ou_workspace_bytes(h, E * B, T_pad_max, &walk);
  if (rc != OU_OK) return rc;
  // (T_pad_max bounds T_raw_max: the member planes are (E * B, T_raw_max))
  *nbytes = align256(walk) + ens_area(B, E, T_pad_max).total;
  return OU_OK;
}

int ou_enhance_ensemble(ou_handle* h, const float* mix, float* out, float* members_out, const float* noise, int32_t B,
                        int32_t T_raw_max, const int32_t* t_raw, int32_t E, int32_t stat, int32_t n_steps, double epsilon,
                        const float* sigma_host, int32_t warm_start, uint32_t flags, void* ws, size_t ws_bytes,
                        ou_stream_t stream) {
  return ensemble_impl(h, mix, out, members_out, noise, B, T_raw_max, t_raw, E, stat, n_steps, epsilon, sigma_host, warm_start,
                       flags, ws, ws_bytes, stream);
}

size_t ou_ensemble_reduce_scratch_bytes(int32_t E, int32_t B) {
  if (E < 1 || B < 1) return 0;
  return align256(((size_t)B * E + B) * sizeof(int));
}

int ou_ensemble_reduce(const float* members, float* out, int32_t E, int32_t B, int64_t row_stride, int64_t cols,
                       const int64_t* len_host, int32_t stat, void* scratch, size_t scratch_bytes, ou_stream_t stream) {
  if (!members || !out || B < 1 || cols < 1 || row_stride < cols) return fail(nullptr, OU_EINVAL, "ou_ensemble_reduce: bad argument");
  if (E < 1 || E > OU_MAX_ENSEMBLE)
    return fail(nullptr, OU_EINVAL, "ou_ensemble_reduce: 1 <= E <= " + std::to_string(OU_MAX_ENSEMBLE));
  if (stat != OU_ENS_MEAN && stat != OU_ENS_MEDIAN && stat != OU_ENS_SIGNAL_MEDIAN)
    return fail(nullptr, OU_EINVAL, "ou_ensemble_reduce: stat must be OU_ENS_MEAN, OU_ENS_MEDIAN or OU_ENS_SIGNAL_MEDIAN");
  if (len_host)
    for (int b = 0; b < B; b++)
      if (len_host[b] < 0 || len_host[b] > cols) return fail(nullptr, OU_EINVAL, "ou_ensemble_reduce: 0 <= len[b] <= cols");
  int* hist = nullptr;
  if (stat == OU_ENS_SIGNAL_MEDIAN) {
    if (!scratch || scratch_bytes < ou_ensemble_reduce_scratch_bytes(E, B) || reinterpret_cast<uintptr_t>(scratch) % 4 != 0)
      return fail(nullptr, OU_ENOMEM, "ou_ensemble_reduce: the signal median needs ou_ensemble_reduce_scratch_bytes of scratch");
    hist = (int*)scratch;
  }
  std::vector<long long> len64;
  if (len_host) len64.assign(len_host, len_host + B);
  const hipError_t e = launch_ensemble_reduce(members, out, E, B, row_stride, cols, len_host ? len64.data() : nullptr, stat, hist,
                                              hist ? hist + (size_t)B * E : nullptr, (hipStream_t)stream);
  if (e != hipSuccess) return fail(nullptr, OU_EHIP, std::string("HIP error at ensemble reduce: ") + hipGetErrorString(e));
  return OU_OK;
}

int ou_sampler_step(ou_handle* h, float* x, const float* score, const float* z, float c1, float c2, size_t n,
                    ou_stream_t stream) {
  if (!h || !x || !score) return fail(h, OU_EINVAL, "bad argument");
  hipError_t e = launch_sampler_step(x, score, z, c1, c2, n, (hipStream_t)stream);
  if (e != hipSuccess) return fail(h, OU_EHIP, hipGetErrorString(e));
  return OU_OK;
}

}  // extern "C"
