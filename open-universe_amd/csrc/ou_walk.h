// The network walk (private): Runner, the persistent part of a workspace, the conditioner and score passes
// and the sampler's scalars.  Bodies that no other file instantiates or calls in a loop are in ou_walk.cpp.
#pragma once
#include <string>
#include <vector>

#include "ou_handle.h"

namespace ou {

// The state of one walk over the network: a bump allocator over the caller's workspace and the one gate,
// launch(), through which everything a forward call enqueues goes.  In `dry` mode nothing is launched and `base` may be null:
// the same walk then only measures the footprint (ou_workspace_bytes) -> layout is a pure function of (config, B, T).
struct Runner {
  ou_handle* h;
  Options env;  // the handle's options as the call found them
  char* base;
  size_t cap;
  size_t off = 0;
  bool dry;
  hipStream_t st;       // where the next launch goes (a side stream while a branch runs there)
  hipStream_t main_st;  // the caller's stream
  int B;
  hipError_t herr = hipSuccess;
  bool oom = false;
  const char* where = "";
  size_t max_plane = 0;            // largest (C, T) plane of one batch row that alloc() handed out (length guard)
  bool mel_scale_preset = false;   // the caller wrote the per-row mel scale (segmented enhance: whole-file scale)
  // ragged batch (ou_enhance_var): per-row lengths on every level, see ou_kernels.h
  bool ragged = false;
  const int* lens_dev = nullptr;  // [lv.n][B]
  const RowInfo* rows_dev = nullptr;
  LevelSpec lv;
  int level_T[kMaxLenLevels] = {0};
  unsigned* status_words = nullptr;        // workspace header (layout_persist)
  unsigned long long* block3_bar = nullptr;
  int gru_area_rows = 0;    // rows the GRU exchange areas were laid out for when that is more than B (ou_enhance_ensemble: the
                            // conditioner runs B rows on the areas of an E * B-row workspace, as a sub-launch of a chunked batch does)
  bool gru_shared = false;  // GRU launches enqueued now may run beside another GRU layer (overlapped conditioner / score pass)

  Runner(ou_handle* h_, void* ws, size_t cap_, bool dry_, hipStream_t st_, int B_)
      : h(h_), env(h_->opt), base((char*)ws), cap(cap_), dry(dry_), st(st_), main_st(st_), B(B_) {
#ifndef OU_EXPERIMENTS
    env.dbg = 0; env.dbg_dec0_under_gru = 0;  // (switches with WRONG results by design: experiments library only)
#endif
  }
  // The conditioner's runner of a call whose score passes run more rows than its conditioner (ou_enhance_ensemble, the segmented
  // ensembles): the first Bc rows of r, on r's workspace from r's bump pointer on, with r's GRU exchange areas.
  static Runner conditioner_of(const Runner& r, int Bc) {
    Runner c(r.h, r.base, r.cap, false, r.st, Bc);
    c.status_words = r.status_words;
    c.block3_bar = r.block3_bar;
    c.gru_area_rows = r.B;
    c.off = r.off;
    c.mel_scale_preset = r.mel_scale_preset;
    c.lv = r.lv;
    for (int l = 0; l < kMaxLenLevels; l++) c.level_T[l] = r.level_T[l];
    return c;
  }
  // into ragged mode: `lens` = the rows' lengths on the levels of set_levels ([lv.n][B], device), `rows` = their geometry
  void set_ragged(const int* lens, const RowInfo* rows) {
    ragged = true;
    lens_dev = lens;
    rows_dev = rows;
  }

  bool ok() const { return herr == hipSuccess && !oom; }
  // THE launch gate: nothing is enqueued in a dry walk or after the first failure; the first error wins (finish())
  template <class F>
  void launch(const char* w, F&& enqueue) {
    if (dry || !ok()) return;
    chk(enqueue(), w);
  }

  float* alloc_raw(size_t floats) {
    size_t bytes = align256(floats * 4);
    size_t o = off;
    off += bytes;
    if (!dry && off > cap) { oom = true; return (float*)base; }
    return dry ? nullptr : (float*)(base + o);
  }
  Tensor alloc(const std::string& name, int C, int T) {
    size_t o = off;
    Tensor t;
    t.p = alloc_raw((size_t)B * C * T);
    if ((size_t)C * T * 4 > max_plane) max_plane = (size_t)C * T * 4;
    t.C = C;
    t.T = T;
    if (!name.empty()) h->tensors[name] = TensorRef{o, C, T};
    return t;
  }
  hipEvent_t next_event() {
    if (h->ev_used == h->events.size()) {
      hipEvent_t e;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
      h->events.push_back(e);
    }
    return h->events[h->ev_used++];
  }
  void wait_for(hipStream_t from, hipStream_t to, const char* w_record, const char* w_wait);
  void fork(hipStream_t from, int k) { wait_for(from, h->aux[k], "fork record", "fork wait"); }  // side stream k behind `from`
  void join(int k, hipStream_t to) { wait_for(h->aux[k], to, "join record", "join wait"); }      // `to` behind side stream k
  // per-row lengths of a (B, C, Tl) tensor (null when all rows are whole)
  const int* lens_of(int Tl) {
    if (!ragged) return nullptr;
    for (int l = 0; l < lv.n; l++)
      if (level_T[l] == Tl) return lens_dev + (size_t)l * B;
    if (herr == hipSuccess) { herr = hipErrorInvalidValue; where = "ragged batch: tensor length on no level"; }
    return nullptr;
  }
  // keep the invariant "zero from the row's own length on" after a kernel that does not keep it itself
  void mask(float* p, int C, int T) {
    if (!ragged || dry || !ok()) return;
    const int* ln = lens_of(T);
    if (ln) launch("mask tail", [&] { return launch_mask_tail(p, ln, B, C, T, st); });
  }
  void mask(const Tensor& t) { mask(t.p, t.C, t.T); }
  // A producer of a (B, C, T) tensor that can keep that invariant itself: `enqueue(lens)` launches it; handed the rows' lengths
  // (mask_fused) it zeroes behind them in its own epilogue, handed null a mask_tail launch follows.
  template <class F>
  void launch_masked(const char* w, float* p, int C, int T, F&& enqueue) {
    const int* ln = env.mask_fused ? lens_of(T) : nullptr;
    launch(w, [&] { return enqueue(ln); });
    if (!ln) mask(p, C, T);
  }
  const float* W(size_t off_floats) const { return h->W + off_floats; }

  // ---- records of the per-launch profile (ou_profile_enable).  Open one: the slot the kernel stamps, or null (profiling off, or
  // no slot left); close: the variant code the launcher chose; drop: the launch did not happen.
  unsigned long long* prof_open(double flops, double bytes, int cfg) {
    if (!h->profile || !h->prof_dev || h->prof_used >= kProfSlots) return nullptr;
    h->prof.push_back(ou_handle::ProfRec{flops, bytes, cfg});
    return h->prof_dev + 32 * h->prof_used++;
  }
  void prof_close(const unsigned long long* slot, int cfg) {
    if (slot) h->prof.back().cfg = cfg;
  }
  void prof_drop(const unsigned long long* slot) {
    if (slot) { h->prof.pop_back(); h->prof_used--; }
  }

  struct Epi {
    const float* add = nullptr;
    float add_scale = 1.f;
    const float* film = nullptr;
    int film_bstride = 0;
    const float* res = nullptr;
    float res_scale = 1.f;
    const float* in_scale = nullptr;
    bool act = true;  // apply the layer's PReLU prologue (if it has one)
    // up-path anti-alias FIR fused into the conv epilogue: taps, 2r + 1, the manual bias added after the FIR.  conv()
    // answers `supported = false` instead of failing when no kernel with that epilogue fits the layer.
    const float* fir = nullptr;
    int fir_len = 0;
    const float* fir_bias = nullptr;
    // small-K rate-change conv of a wide level on rate_down_kernel (`fir` = the filter applied BEFORE the conv, or null)
    bool rate_down = false;
    bool rate_up = false;  // the last up conv on rate_up_kernel (`fir` = the filter AFTER the conv or null, fir_bias / res)
    // store prelu(y; out_alpha) instead of y (ConvArgs::out_act): for outputs whose only reader is the next PReLU_Conv.  conv()
    // answers in `stored_act` whether the kernel that took the layer did so (else y is stored and the reader keeps its PReLU).
    bool out_act = false;
    float out_alpha = 1.f;
    bool no_mask = false;  // ragged batch: the caller fills the tail itself (GRU input projections)
  };
  // GRU launches that can meet on one XCD: this call's own two layers when they overlap, times the lanes whose clusters are
  // dealt to the same XCDs (lane l deals its 2 B clusters from XCD 2 B l on)
  static int gru_share_of(int lanes, int B, bool overlap) {
    const int ncl = 2 * B < 8 ? 2 * B : 8;
    const int by_lanes = lanes > 1 ? (ncl * lanes + 7) / 8 : 1;
    return by_lanes * (overlap ? 2 : 1);
  }

  static int conv_nq(const ConvL& L, int Tin) { return L.stride > 1 ? Tin / L.stride : Tin; }
  static int conv_tout(const ConvL& L, int Tin) { return L.stride > 1 ? Tin / L.stride : Tin * L.up; }
  // What conv() decided: the output, whether it was stored activated (Epi::out_act), and -- Epi::fir on the generic kernels
  // only -- whether a kernel with that epilogue took the layer (false: nothing was launched, the caller runs conv + launch_fir)
  struct ConvOut {
    Tensor out;
    bool stored_act = false;
    bool supported = true;
  };
  struct BlockOut { Tensor h_next, v, c1; };

  // ---- ou_walk.cpp
  ConvArgs conv_args(const ConvL& L, const Tensor& in, const Tensor& out, const Epi& e);
  ConvOut conv(const ConvL& L, const Tensor& in, const std::string& name, const Epi& e, const Tensor* dst = nullptr);
  ConvArgs rate_probe(const ConvL& rc, int Tin);
  Tensor up_path(const BlockL& Bk, const Tensor& hin, const std::string& nm, const float* res);
  ChainArgs chain_args(const BlockL& Bk, int depth, const Tensor& hu, const Tensor& c1, const Tensor& v, const Epi& e1,
                       bool need_c1);
  int plan_chain(const BlockL& Bk, const Tensor& hu, const Tensor& c1, const Tensor& v, const Epi& e1, bool need_c1);
  bool body_block3(const BlockL& Bk, const Tensor& hu, const Tensor& c1, const Tensor& c2, const Tensor& v, const std::string& nm,
                   const Epi& e1, const Epi& e3);
  Tensor activated(const ConvL& L, const Tensor& in, const Tensor& plane);
  void body(const BlockL& Bk, const Tensor& hu, const Tensor& c1, const Tensor& c2, const Tensor& v, const std::string& nm,
            Epi e1, bool need_c1, bool c1_private, const Tensor& act = Tensor());
  Tensor down_path(const BlockL& Bk, const Tensor& v, const std::string& nm);
  BlockOut block(const BlockL& Bk, const Tensor& hin, const std::string& nm, const float* film, int film_bs,
                 const float* input_cond, const float* res, bool need_c1 = false, const Tensor* c1_dst = nullptr,
                 const Tensor* v_dst = nullptr);
  Tensor gru(const GruL& G, const Tensor& in, const std::string& nm, unsigned long long* xchg, unsigned* errw,
             unsigned* epoch, const float* res, float res_scale, hipEvent_t* before = nullptr);

 private:
  void chk(hipError_t e, const char* w) {
    if (e != hipSuccess && herr == hipSuccess) { herr = e; where = w; }
    h->n_launch++;
  }
};

// Persistent part of the workspace (lives across ou_condition / ou_score / ou_enhance calls on it).
struct Persist {
  unsigned* status;
  StepCoef* coef;             // [kMaxSteps] or [B]
  float* stats;               // [B][4]
  RowInfo* rows;              // [B]   ragged batch: per-row geometry
  int* lens;                  // [kMaxLenLevels][B]   ... and lengths on every level
  unsigned long long* xchg;   // GRU granules (conditioner)
  unsigned long long* xchg2;  // GRU granules (score net; may run concurrently with the conditioner)
  float* mel_scale;           // [B]
  float* g;                   // [kMaxSteps][D]
  float* film;                // [kMaxSteps][rows]
  Tensor mixn, x, wav;        // (B,1,T)
  std::vector<Tensor> sc;     // signal_cond_proj(cond_j)   (B, C_j, T_j)
  std::vector<Tensor> cond;   // conditions
  Tensor aux, latent;
};

Persist layout_persist(Runner& r, int T);
void run_condition(Runner& r, Persist& P, const float* mix_norm, int T);

// what run_score_enc hands to run_score_dec
struct ScoreEnc {
  std::vector<Tensor> residuals;
  Tensor hg;
  bool fuse_res = false;
};
ScoreEnc run_score_enc(Runner& r, Persist& P, const float* x, const StepCoef* coef, int coef_bs,
                       const float* film_row, int film_bs, int T, hipEvent_t* pre_gru = nullptr);
void run_score_dec(Runner& r, Persist& P, const ScoreEnc& E, const float* x, const float* noise, float* out, int mode,
                   const StepCoef* coef, int coef_bs, const float* film_row, int film_bs, int T, const Tensor* dec0_done = nullptr);
void run_score(Runner& r, Persist& P, const float* x, const float* noise, float* out, int mode,
               const StepCoef* coef, int coef_bs, const float* film_row, int film_bs, int T);

StepCoef make_coef(const ou_config& cfg, float s, bool last, double eta, double beta, float s_next);
void schedule(const ou_config& cfg, int n_steps, double epsilon, float* sigma, double* eta, double* beta);
void upload_coefs(Runner& r, StepCoef* dst, const std::vector<StepCoef>& rows);
void upload_film_rows(Runner& r, Persist& P, int n);

long long max_walk_length(ou_handle* h, bool need_wav);

int finish(ou_handle* h, Runner& r);

}  // namespace ou
