// C ABI of libouniverse.so (include/ouniverse.h): packer, handle, and the forward "runner" that walks
// the model and enqueues the gfx950 kernels on the caller's stream.  No allocation, no host sync in the
// forward calls.  There is no CPU path: without a HIP device ou_create fails.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/ouniverse.h"
#include "../../include/ouniverse_tuning.h"
#include "ou_kernels.h"
#include "ou_model.h"

using namespace ou;

namespace {
thread_local std::string g_last_error;
constexpr int kMaxSteps = 256;
constexpr size_t kProfSlots = 32768;
constexpr float kInvSqrt2 = 0.70710678118654752440f;
constexpr size_t align256(size_t bytes) { return (bytes + 255) & ~size_t(255); }  // granularity of every workspace area

struct TensorRef {
  size_t off;  // bytes into the workspace
  int C, T;
};
// Tuning / test switches of a handle (ou_set_option; the table of keys is kOptions below)
struct Options {
  int dbg = 0, xcd_map = -1, conv_direct = 5, fuse = -1, fuse_nc = 0, rate_small = 1, fuse_upfir = 1, block3 = 0, d4_fir = 1,
      d4_force = 0, d4_short = 1, d2_wk = 0, wino = 1, d2_map = -1, unfuse64 = 0, preact = 1;
  int gru_v = 2, gru_bmax = 0, gru_ts = 0, gru_upw = 0, gru_backoff = 0, gru_agent = -1, gru_dbg = 0;
  int split = -1;              // ConvArgs::split
  int dbg_dec0_under_gru = 0;  // measurement only, INVALID results (see run_score); experiments library only
  int tile_prefetch = 1;
  int trace = 0, no_overlap = 0, ts = 0, deep_factor = 8, mask_fused = 1, split_wino = 1, d2_tile_rule = 1;
  int ens_share = 1;           // ou_enhance_ensemble: conditioner once over the B inputs (1) or over all E * B rows (0)
  double tile_min = -1.0;      // < 0: the launcher's default
  std::string chain_ts;        // ou_set_stamp_layer (tuning)
};
}  // namespace

struct ou_packer {
  Model m;
  std::map<std::string, HostTensor> sd;
  std::vector<float> blob;
  std::string err;
};

struct ou_handle {
  Model m;
  const float* W = nullptr;  // packed blob (device)
  int device = 0;
  int num_cu = 256;
  std::string err;
  std::map<std::string, TensorRef> tensors;
  int n_launch = 0, n_conv = 0;
  // geometry of the last ou_condition (consumed by ou_score)
  int cond_B = 0, cond_T = 0;
  bool trace = false;
  Options opt;                    // ou_set_option
  NormMode norm;                  // ou_set_normalization (as created: norm 2, zero_mean -- the kernels' plain instantiations)
  std::string plan_with_options;  // ou_plan_json's answer (the plan + the current option values)
  int last_cfg = -1;
  long long* tstamps = nullptr;
  std::map<size_t, float> alphas;  // host copies of the PReLU slopes (blob offset -> value)
  // side streams for independent branches (mel front-end, st convs, first score-encoder pass), fork/joined to the
  // caller's stream with events: still no host synchronisation, still graph-capturable
  hipStream_t aux[3] = {nullptr, nullptr, nullptr};
  std::vector<hipEvent_t> events;
  size_t ev_used = 0;
  bool overlap = true;
  int force_cfg = -1, force_sc = 0;  // micro-benchmark overrides (ou_bench_conv)
  // per-launch HIP-event profiling of the generic conv kernel (bench.py roofline)
  bool profile = false;
  struct ProfRec { double flops, bytes; int cfg; };
  std::vector<ProfRec> prof;
  size_t prof_used = 0;
  unsigned long long* prof_dev = nullptr;  // [kProfSlots][32] device-side {16 x min start, 16 x ~max end} ticks
  // workspaces that ou_workspace_init has prepared (cleared status word, GRU tag epochs and exchange areas) and the
  // shape each was prepared for: the forward calls refuse anything else -- an uninitialised buffer would feed the
  // recurrence kernels a garbage epoch and garbage tags
  struct WsRec { const void* ws; size_t bytes; int B, T; };
  std::vector<WsRec> ws_ready;
  int gru_agent_stores = 0;  // ou_set_gru_publish_mode; also set by ou_check_device_status when the safety net had to act
  // enhance calls in flight side by side in this process, one handle + stream + workspace each (ou_set_lanes): the GRU
  // launches of all lanes have to be resident together
  int lanes = 1, lane = 0;
  int lane_max_b = 0;  // ou_set_lane_batch: largest batch size any lane of the pool runs (0: every call's own B)
  // ou_set_noise_source: counter-based noise (include/ouniverse.h).  Off: the forward calls read the caller's noise tensor.
  struct NoiseSource {
    bool on = false;
    unsigned long long seed = 0;
    std::vector<unsigned long long> streams;  // host copy, one id per row
    float* scratch = nullptr;                 // two (B, T_pad) planes (caller-owned, device)
    size_t scratch_bytes = 0;
  } noise_src;
  // length guard of ou_enhance / ou_enhance_var: bytes per padded sample of the largest per-row plane of the walk (dry walk of
  // the conditioner and one score pass, every plane a multiple of T; 0 = not measured yet) and of the decoupling scratch
  double plane_per_sample = 0.0, wav_plane_per_sample = 0.0;
  // A workspace prepared for (B, T0) serves every T of the same batch size that fits into it: everything ou_workspace_init
  // prepares (status words, tag epochs, GRU exchange areas) lies in a header whose layout depends on B alone, and the tag
  // epochs advance monotonically whatever the length of a pass -- a directory of files of different lengths runs on ONE
  // workspace sized for the longest.  (Too small a buffer is caught by the walk itself: OU_ENOMEM.)
  bool ws_ok(const void* ws, size_t bytes, int B, int T) const {
    (void)T;
    for (const WsRec& r : ws_ready)
      if (r.ws == ws) return r.B == B && r.bytes <= bytes;
    return false;
  }
};

namespace {

int fail(ou_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  g_last_error = msg;
  return code;
}

struct Tensor {
  float* p = nullptr;
  int C = 0, T = 0;
};

// Tuning / test switches.  Until ABI 4 these were ~35 OU_* environment variables read by the library; since ABI 5
// the library reads NO environment variable: every switch is a typed option of the handle (ou_set_option / ou_get_option,
// include/ouniverse.h), echoed by ou_plan_json, and a forward call works on a copy taken when it starts.
struct OptDesc {
  const char* key;
  int Options::*ip;
  double Options::*dp;
  bool experiments_only;  // switches that make a call return WRONG results by design: honoured by `make EXPERIMENTS=1` builds only
  const char* doc;
};
const OptDesc kOptions[] = {
    {"conv_direct", &Options::conv_direct, nullptr, false, "kernel generations the conv launcher may use (0 .. 5, ConvArgs::direct)"},
    {"split", &Options::split, nullptr, false, "-1 rule / 0 never / 1 wherever possible: conv_split_kernel (bf16-split operands)"},
    {"split_wino", &Options::split_wino, nullptr, false, "experiments build: 0 = the plain bf16-split kernel also where its minimal-filtering form would take the layer"},
    {"wino", &Options::wino, nullptr, false, "0: never the minimal-filtering (Winograd / Cook-Toom) kernel variants"},
    {"fuse", &Options::fuse, nullptr, false, "-1 cost model / 0 never / 2 / 3: depth of the fused ConvBlock body (conv_chain kernels)"},
    {"fuse_nc", &Options::fuse_nc, nullptr, false, "128 / 256: columns per tile of the fused ConvBlock body (0: launcher's choice)"},
    {"fuse_upfir", &Options::fuse_upfir, nullptr, false, "0: up-path anti-alias FIR always as its own pass"},
    {"rate_small", &Options::rate_small, nullptr, false, "0: outermost rate-change convs on the generic kernels (no rate_down / rate_up)"},
    {"preact", &Options::preact, nullptr, false, "0: every PReLU in its consumer's operand path (ConvArgs::out_act never set)"},
    {"unfuse64", &Options::unfuse64, nullptr, false, "1: 64-channel ConvBlock bodies as three split-K launches"},
    {"block3", &Options::block3, nullptr, false, "1: the three body convs of a deep-level ConvBlock in one launch (experiments build only)"},
    {"xcd_map", &Options::xcd_map, nullptr, false, "block -> tile mapping of the LDS-tiled conv kernel (-1: launcher's choice)"},
    {"d2_map", &Options::d2_map, nullptr, false, "block -> tile mapping of the wide-load split-K kernels (-1: launcher's choice)"},
    {"d2_tile_rule", &Options::d2_tile_rule, nullptr, false, "0: round 5's 64- vs 32-column rule of the wide-load split-K kernels (ignores that only 64-column tiles have minimal filtering)"},
    {"d2_wk", &Options::d2_wk, nullptr, false, "4 / 8: K slices of conv_direct2_kernel (0: launcher's rule)"},
    {"d4_fir", &Options::d4_fir, nullptr, false, "0: up convs with a fusable FIR stay on the first-generation fused kernel"},
    {"d4_short", &Options::d4_short, nullptr, false, "0: the 401-frame levels at batch 1 stay on the first-generation kernels"},
    {"d4_force", &Options::d4_force, nullptr, false, "10 TM + log2(WK): that conv_direct4 tile shape wherever a layer admits it"},
    {"tile_min", nullptr, &Options::tile_min, false, "wave tiles per SIMD from which the no-split-K kernels take a layer (< 0: 1.2)"},
    {"tile_prefetch", &Options::tile_prefetch, nullptr, false, "0: no LDS prefetch of the epilogue operand in conv_direct3_kernel"},
    {"deep_factor", &Options::deep_factor, nullptr, false, "blocks of 64 x 128 per CU up to which a layer counts as 'deep' (split-K kernels)"},
    {"mask_fused", &Options::mask_fused, nullptr, false, "ragged batches: 0 = a separate tail-mask launch after EVERY producer (reference form of the masks)"},
    {"gru_v", &Options::gru_v, nullptr, false, "2 ring kernel / 1 polling-wave kernel (experiments build)"},
    {"gru_bmax", &Options::gru_bmax, nullptr, false, "cap on the utterances per GRU launch (forces the chunked path)"},
    {"gru_upw", &Options::gru_upw, nullptr, false, "hidden units per workgroup of the ring kernel (0: from the batch size)"},
    {"gru_backoff", &Options::gru_backoff, nullptr, false, "poll back-off experiments of the ring kernel (0: none)"},
    {"gru_agent_stores", &Options::gru_agent, nullptr, false, "-1 handle's mode / 0 plain / 1 agent-scope publishes"},
    {"gru_dbg", &Options::gru_dbg, nullptr, false, "bit 0 no republish safety net, bit 1 system-scope publishes, bit 2 FAULT INJECTION (tests)"},
    {"gru_ts", &Options::gru_ts, nullptr, false, "1: per-wave cycle stamps of the GRU kernel into the end of the workspace (tuning)"},
    {"ts", &Options::ts, nullptr, false, "1: per-wave phase stamps in ou_bench_conv (tuning)"},
    {"trace", &Options::trace, nullptr, false, "1: one line per conv launch on stderr"},
    {"no_overlap", &Options::no_overlap, nullptr, false, "1: no side streams inside a call (every kernel alone on the device)"},
    {"ens_share", &Options::ens_share, nullptr, false, "ou_enhance_ensemble: 1 = conditioner once over the B inputs, its results replicated; 0 = over all E * B rows"},
    {"dbg", &Options::dbg, nullptr, true, "phase ablation switches of the conv kernels: WRONG results by design"},
    {"dbg_dec0", &Options::dbg_dec0_under_gru, nullptr, true, "first decoder block under the GRU: upper-bound measurement, WRONG results"},
};
constexpr int kNumOptions = (int)(sizeof(kOptions) / sizeof(kOptions[0]));
const OptDesc* find_option(const char* key) {
  for (int i = 0; i < kNumOptions; i++)
    if (std::strcmp(kOptions[i].key, key) == 0) return &kOptions[i];
  return nullptr;
}

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
  // make stream `to` wait for everything enqueued so far on `from`
  void wait_for(hipStream_t from, hipStream_t to, const char* w_record, const char* w_wait) {
    if (dry || !ok()) return;
    hipEvent_t e = next_event();
    if (!e) { herr = hipErrorOutOfMemory; where = "event"; return; }
    launch(w_record, [&] { return hipEventRecord(e, from); });
    launch(w_wait, [&] { return hipStreamWaitEvent(to, e, 0); });
  }
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
  // the launch arguments of layer L reading `in`, writing `out`, with epilogue e
  ConvArgs conv_args(const ConvL& L, const Tensor& in, const Tensor& out, const Epi& e) {
    ConvArgs a;
    a.x = in.p; a.w = W(L.w_off); a.bias = W(L.b_off); a.y = out.p;
    if (L.KWP) { a.wd = W(L.wd_off); a.wu = W(L.wu_off); }
    if (L.ws_on) a.wsplit = W(L.ws_off);
    if (L.wsw_on) a.wsplitw = W(L.wsw_off);
    a.split = env.split; a.split_wino = env.split_wino;
    a.in_scale = e.in_scale;
    a.act = (L.act && e.act) ? 1 : 0;
    a.alpha_val = a.act ? h->alphas[L.a_off] : 0.f;
    a.add = e.add; a.add_scale = e.add_scale;
    a.film = e.film; a.film_bstride = e.film_bstride;
    a.res = e.res; a.res_scale = e.res_scale;
    if (e.out_act && !e.fir && !e.rate_down && !e.rate_up) { a.out_act = 1; a.out_alpha = e.out_alpha; }
    if (e.fir && !e.rate_down) { a.fir = e.fir; a.fir_len = e.fir_len; a.bias = e.fir_bias; }  // (also rate_up)
    if (e.rate_down) { a.fir = e.fir; a.fir_len = e.fir ? e.fir_len : 0; }
    a.B = B; a.Cin = L.Cin; a.Tin = in.T; a.Cout = L.Cout; a.M = L.M; a.Mp = L.Mp; a.KW = L.KW;
    a.stride = L.stride; a.pad = L.pad; a.up = L.up; a.CK = L.CK; a.Nq = conv_nq(L, in.T); a.Tout = conv_tout(L, in.T);
    a.force_cfg = h->force_cfg; a.force_sc = h->force_sc;
    a.dbg = env.dbg; a.force_xcd_map = env.xcd_map; a.direct = env.conv_direct; a.d4_fir_unfused = env.d4_fir; a.d4_force = env.d4_force; a.d4_short = env.d4_short; a.deep_factor = env.deep_factor; a.d2_tile_rule = env.d2_tile_rule; a.d2_wk = env.d2_wk; a.wino = env.wino; a.d2_map = env.d2_map;
    a.tile_min = env.tile_min; a.tile_prefetch = env.tile_prefetch;
    a.tstamps = h->tstamps;
    // ragged batch: the kernel keeps "zero behind the row's own end" in its epilogue where its family can (conv_masks_rows)
    if (ragged && env.mask_fused && !e.no_mask) a.lens = lens_of(a.Tout);
    return a;
  }

  // What conv() decided: the output, whether it was stored activated (Epi::out_act), and -- Epi::fir on the generic kernels
  // only -- whether a kernel with that epilogue took the layer (false: nothing was launched, the caller runs conv + launch_fir)
  struct ConvOut {
    Tensor out;
    bool stored_act = false;
    bool supported = true;
  };
  // one conv layer: allocate (unless `dst`), then profile, launch, mask, trace and count
  ConvOut conv(const ConvL& L, const Tensor& in, const std::string& name, const Epi& e, const Tensor* dst = nullptr) {
    ConvOut o;
    o.out = dst ? *dst : alloc(name, L.Cout, conv_tout(L, in.T));
    if (dry || !ok()) return o;
    ConvArgs a = conv_args(L, in, o.out, e);
    // algorithmic (reference, un-folded) work of this layer: dense FLOPs, activations once, weights once (the packed layers
    // carry the reference's own kernel sizes)
    a.prof = prof_open(2.0 * L.M * (double)a.Nq * L.Cin * L.KW * B,
                       4.0 * ((double)B * ((double)L.Cin * in.T + (double)L.Cout * a.Tout) + (double)L.M * L.Cin * L.KW), -1);
    int cfg = -1;
    hipError_t le;
    if (e.rate_down) {
      le = launch_rate_down(a, st, &cfg);
    } else if (e.rate_up) {
      le = launch_rate_up(a, st, &cfg);
    } else {
      le = launch_conv(a, h->num_cu, st, &cfg);
      if (le == hipErrorNotSupported && a.out_act) {  // the kernel for this layer has no activating epilogue: store y
        a.out_act = 0;
        le = launch_conv(a, h->num_cu, st, &cfg);
      }
      o.stored_act = a.out_act != 0;
      if (le == hipErrorNotSupported && e.fir) {  // not a failure and not counted: the caller falls back to conv + launch_fir
        prof_drop(a.prof);
        o.supported = false;
        return o;
      }
    }
    launch(L.name.c_str(), [le] { return le; });  // (the gate was passed above: this records the launcher's answer)
    prof_close(a.prof, cfg);
    h->last_cfg = cfg;
    if (!e.no_mask && !(a.lens && conv_masks_rows(cfg))) mask(o.out);
    if (h->trace)
      std::fprintf(stderr, "OU_TRACE conv %-64s cfg=%d M=%d Nq=%d K=%d(Cin=%d KW=%d CK=%d) stride=%d up=%d B=%d MFLOP=%.1f\n",
                   name.c_str(), cfg, L.M, a.Nq, L.Cin * L.KW, L.Cin, L.KW, L.CK, L.stride, L.up, B,
                   2.0 * L.M * a.Nq * L.Cin * L.KW * B * 1e-6);
    h->n_conv++;
    return o;
  }

  // ---- ConvBlock.forward  (blocks.py:327-412) in three parts: up_path, body, down_path; block() sequences them.

  // What rate_up_supported / rate_down_supported ask about the rate-change conv of a block reading Tin frames: the shape and
  // whether a FIR rides along (fir_mode 1: in front of the down conv, 2: behind the up conv).  Pure function of the layer shape.
  ConvArgs rate_probe(const ConvL& rc, int Tin) {
    ConvArgs a;
    a.up = rc.up; a.stride = rc.stride; a.KW = rc.KW; a.pad = rc.pad; a.Tin = Tin;
    a.Nq = conv_nq(rc, Tin); a.Tout = conv_tout(rc, Tin); a.M = rc.M; a.Cout = rc.Cout; a.Cin = rc.Cin;
    a.fir = (rc.fir_mode == 1 || rc.fir_mode == 2) ? W(rc.fir_off) : nullptr; a.fir_len = rc.fir_len;
    return a;
  }

  // blocks.py:366-376: the block's input brought to the block's rate, `res` (the skip connection) added.  `res` for dir == 0
  // blocks must already be folded into `hin`.
  Tensor up_path(const BlockL& Bk, const Tensor& hin, const std::string& nm, const float* res) {
    if (Bk.dir != 2) return hin;
    const ConvL& rc = Bk.rc;
    Epi e;
    e.res = res; e.res_scale = kInvSqrt2;  // blocks.py:374-376 fused into the up-conv epilogue
    if (rc.fir_mode == 2) { e.fir = W(rc.fir_off); e.fir_len = rc.fir_len; e.fir_bias = W(rc.fbias_off); }
    if ((rc.fir_mode == 0 || rc.fir_mode == 2) && env.rate_small != 0 && rate_up_supported(rate_probe(rc, hin.T))) {
      e.rate_up = true;
      return conv(rc, hin, nm + ".up", e).out;
    }
    // (fir_mode 4: FIR folded into 3-tap phase GEMMs by the packer, its manual bias = the conv bias)
    if (rc.fir_mode != 2) return conv(rc, hin, nm + ".up", e).out;
    // PReLU -> transposed conv (r phase GEMMs) -> FIR + bias + residual add: fused into the conv's epilogue where
    // the direct kernel takes the layer, else as one bandwidth pass after it
    const Tensor u = alloc(nm + ".upc", rc.Cout, hin.T * rc.up);
    const Tensor hu = alloc(nm + ".up", u.C, u.T);
    if (env.fuse_upfir != 0 && conv(rc, hin, nm + ".up", e, &hu).supported) return hu;
    conv(rc, hin, nm + ".upc", Epi(), &u);
    launch_masked("fir(up)", hu.p, hu.C, hu.T, [&](const int* ln) {
      return launch_fir(u.p, W(rc.fir_off), rc.fir_len, 0.f, 0, W(rc.fbias_off), res, kInvSqrt2, hu.p, B, u.C, u.T, st, ln);
    });
    return hu;
  }

  // The launch arguments of the fused body of a ConvBlock at `depth` (3: conv1 .. conv3, 2: conv2, conv3): plan_chain prices
  // them (chain_cost reads the shape, `wu` / `add` / `film` / `c1_out` as flags and `lens`), body launches them.  depth 0 in the
  // result: the layers are not a body the fused kernels take.
  ChainArgs chain_args(const BlockL& Bk, int depth, const Tensor& hu, const Tensor& c1, const Tensor& v, const Epi& e1,
                       bool need_c1) {
    ChainArgs ca;
    ca.depth = depth; ca.B = B; ca.C = Bk.C; ca.T = hu.T; ca.Mp = Bk.c1.Mp;
    ca.x = depth == 3 ? hu.p : c1.p;
    ca.y = v.p; ca.res = hu.p; ca.res_scale = kInvSqrt2;
    if (depth == 3) {
      ca.add = e1.add; ca.add_scale = e1.add_scale; ca.film = e1.film; ca.film_bstride = e1.film_bstride;
      ca.c1_out = need_c1 ? c1.p : nullptr;
    }
    const ConvL* ls[3] = {&Bk.c1, &Bk.c2, &Bk.c3};
    for (int s2 = 0; s2 < depth; s2++) {
      const ConvL& L = *ls[3 - depth + s2];
      if (!L.act || L.stride != 1 || L.up != 1 || L.Cin != Bk.C || L.Cout != Bk.C || L.pad != (L.KW - 1) / 2 || L.Mp != Bk.c1.Mp)
        ca.depth = 0;
      ChainConv& c = ca.cv[s2];
      c.w = W(L.w_off); c.bias = W(L.b_off); c.alpha = L.act ? h->alphas[L.a_off] : 0.f; c.KW = L.KW; c.CK = L.CK;
      if (L.KWP) c.wu = W(L.wu_off);
    }
    ca.force_nc = env.fuse_nc;
    ca.wino = env.wino && env.conv_direct >= 5;
    ca.lens = lens_of(hu.T);
    return ca;
  }
  // How the three body convs of a ConvBlock run: 0 = three generic launches, 3 = one fused launch, 2 = conv1 generic +
  // fused (conv2, conv3).  Pure function of (layer shapes, B, T, device, options fuse / fuse_nc) -- estimated cycles, see
  // chain_cost(); the generic launches are priced at their measured ~45 TFLOP/s with a 12 us floor.
  int plan_chain(const BlockL& Bk, const Tensor& hu, const Tensor& c1, const Tensor& v, const Epi& e1, bool need_c1) {
    const int T = hu.T;
    if (env.fuse == 0) return 0;
    // a fused body applies the PReLU of its three convs itself: not a form for a block with a Snake layer or with none
    if (!Bk.all_prelu()) return 0;
    // (ragged batch: conv_chainw_kernel zeroes its LDS tiles and its output behind every row's own end -- ChainArgs::lens)
    if (ragged && !env.mask_fused) return 0;  // (the separate-mask form has no place to mask inside a fused body)
    // Throughput regime: with >= ~2 wave tiles per SIMD the three convs run unfused on conv_direct3_kernel at 70-100 TFLOP/s
    // each, ahead of the fused body's ~75 (measured end to end: PP16 B = 4 19.2 -> 18.4 ms, OR16 B = 16 57.7 -> 55.5 ms, B = 8
    // even); below that the fused launch wins (B = 1: 24 us for all three convs).
    if (env.fuse < 0 && Bk.C % 16 == 0 && Bk.c1.KWP && Bk.c2.KWP && Bk.c3.KWP) {
      if (env.conv_direct >= 3 && direct3_tiles_per_simd(Bk.C, T, B, h->num_cu) >= 1.9 && T >= 1024) return 0;
      // Round 5, measured and left off: with minimal filtering the three split-K launches of a 64-channel body (17.0 + 11.7 +
      // 11.7 us at B = 1, back to back) look level with conv1 + the fused pair (17.0 + 24.8) -- end to end the unfused form is
      // 0.04-0.07 ms per enhance SLOWER (6.88-6.91 vs 6.83-6.85 ms, three alternating runs).  OU_UNFUSE64=1 selects it.
      if (env.unfuse64 && env.conv_direct >= 5 && env.wino && Bk.C % 64 == 0 && T >= 1024) return 0;
    }
    auto generic = [&](const ConvL& L) {
      const double cyc = 2.0 * L.M * (double)T * L.Cin * L.KW * B / 45e12 * 2.3e9;
      return cyc > 28000.0 ? cyc : 28000.0;
    };
    const double c3 = chain_cost(chain_args(Bk, 3, hu, c1, v, e1, need_c1), h->num_cu, nullptr);
    double c2 = chain_cost(chain_args(Bk, 2, hu, c1, v, e1, need_c1), h->num_cu, nullptr);
    if (c2 >= 0) c2 += generic(Bk.c1);
    if (env.fuse == 3) return c3 >= 0 ? 3 : 0;
    if (env.fuse == 2) return c2 >= 0 ? 2 : 0;
    const double c0 = generic(Bk.c1) + generic(Bk.c2) + generic(Bk.c3);
    int best = 0;
    double bc = c0;
    if (c3 >= 0 && c3 < bc) { best = 3; bc = c3; }
    if (c2 >= 0 && c2 < bc) { best = 2; bc = c2; }
    return best;
  }
  // Deep levels at batch 1: the three body convs in ONE launch (conv_block3_kernel) where the shape fits -- on the caller's
  // stream only (its workgroups wait for each other: one such kernel at a time), not while profiling per layer.  False: not
  // taken, nothing launched.  OFF by default (option block3): 41.7 / 42.3 us per fused launch (C = 512 / 256) against 44.3 /
  // 44.1 us for the three launches with their gaps, and the enhance as a whole 0.1 ms SLOWER with it.
  bool body_block3(const BlockL& Bk, const Tensor& hu, const Tensor& c1, const Tensor& c2, const Tensor& v, const std::string& nm,
                   const Epi& e1, const Epi& e3) {
    if (dry || !ok() || env.block3 == 0 || !Bk.all_prelu() || B != 1 || ragged || st != main_st || !block3_bar || h->profile || h->tstamps ||
        h->force_cfg >= 0 || env.conv_direct < 2)
      return false;
    const ConvArgs cv[3] = {conv_args(Bk.c1, hu, c1, e1), conv_args(Bk.c2, c1, c2, Epi()), conv_args(Bk.c3, c2, v, e3)};
    int cfg = -1;
    const hipError_t le = launch_conv_block3(cv, block3_bar, status_words, h->num_cu, st, &cfg);
    if (le == hipErrorInvalidConfiguration) return false;  // (not a shape for it)
    if (le != hipSuccess) { launch(nm.c_str(), [le] { return le; }); return false; }
    h->last_cfg = cfg;
    h->n_conv++;
    if (h->trace) std::fprintf(stderr, "OU_TRACE block3 %-62s cfg=%d C=%d T=%d\n", nm.c_str(), cfg, Bk.C, hu.T);
    return true;
  }
  // blocks.py:377-399: conv1 (+ cond add, FiLM: e1), conv2, conv3 (+ the block's residual), hu -> c1 -> c2 -> v.  One fused launch
  // on the wide, shallow levels (conv_chain kernels: all three, or conv1 + a fused (conv2, conv3)), else conv_block3_kernel or
  // three launches.  `need_c1`: the caller reads the raw conv1 result; `c1_private`: nobody but conv2 reads c1.
  // The input of body conv L as its conv has to read it: `in` itself, or -- act_type snake / snakebeta -- its alias-free Snake in
  // `plane` (one snake_act_kernel launch; the conv then runs with its activation off, ConvL::act = 0).  "none" and PReLU: `in`.
  Tensor activated(const ConvL& L, const Tensor& in, const Tensor& plane) {
    if (L.act_kind != OU_ACT_SNAKE && L.act_kind != OU_ACT_SNAKEBETA) return in;
    Tensor s = plane;
    s.C = in.C; s.T = in.T;
    const Model& m = h->m;
    const int* ln = lens_of(in.T);
    launch("snake", [&] {
      return launch_snake_act(in.p, s.p, B, in.C, in.T, in.T, ln, nullptr, W(L.sa_off), L.sb_off != L.sa_off ? W(L.sb_off) : nullptr,
                              W(m.snake_up_off), W(m.snake_down_off), st);
    });
    return s;
  }
  // `act`: the block's plane for activated inputs (allocated by block() when a body conv has a Snake activation)
  void body(const BlockL& Bk, const Tensor& hu, const Tensor& c1, const Tensor& c2, const Tensor& v, const std::string& nm,
            Epi e1, bool need_c1, bool c1_private, const Tensor& act = Tensor()) {
    const int depth = dry ? 0 : plan_chain(Bk, hu, c1, v, e1, need_c1);
    if (depth == 3 || depth == 2) {
      if (depth == 2) conv(Bk.c1, hu, nm + ".c1", e1, &c1);
      if (!ok()) return;
      ChainArgs ca = chain_args(Bk, depth, hu, c1, v, e1, need_c1);
      if (!env.chain_ts.empty() && nm == env.chain_ts) ca.tstamps = (long long*)(base + cap - (16u << 20));
      double flops = 0, wbytes = 0;
      for (int s2 = 0; s2 < depth; s2++) {
        flops += 2.0 * Bk.C * (double)hu.T * Bk.C * ca.cv[s2].KW * B;
        wbytes += 4.0 * Bk.C * Bk.C * ca.cv[s2].KW;
      }
      // activations: block input (also the residual) once, output once, the cond add when present
      ca.prof = prof_open(flops, 4.0 * B * (double)Bk.C * hu.T * (2 + (depth == 2 ? 1 : 0) + (ca.add ? 1 : 0)) + wbytes, -1);
      int variant = -1;
      launch(nm.c_str(), [&] { return launch_chain(ca, h->num_cu, st, &variant); });
      prof_close(ca.prof, variant);
      if (h->trace)
        std::fprintf(stderr, "OU_TRACE chain %-63s variant=%d depth=%d C=%d T=%d B=%d\n", nm.c_str(), variant, depth, Bk.C, hu.T, B);
      h->n_conv++;
      return;
    }
    Epi e3;
    e3.res = dry ? nullptr : hu.p; e3.res_scale = kInvSqrt2;  // blocks.py:399
    if (body_block3(Bk, hu, c1, c2, v, nm, e1, e3)) return;
    // c1 (unless it is exported as a condition) and c2 are read by the next conv only: stored ACTIVATED by the epilogue of the
    // conv that produces them, so that the reader's operand path has no PReLU (ConvArgs::out_act; bit-identical)
    if (env.preact && c1_private && Bk.c2.act) { e1.out_act = true; e1.out_alpha = h->alphas[Bk.c2.a_off]; }
    Epi e2;
    e2.act = !conv(Bk.c1, activated(Bk.c1, hu, act), nm + ".c1", e1, &c1).stored_act;
    if (env.preact && Bk.c3.act) { e2.out_act = true; e2.out_alpha = h->alphas[Bk.c3.a_off]; }
    e3.act = !conv(Bk.c2, activated(Bk.c2, c1, act), nm + ".c2", e2, &c2).stored_act;
    conv(Bk.c3, activated(Bk.c3, c2, act), nm + ".v", e3, &v);
  }

  // blocks.py:401-410: the block's output brought to the next block's rate
  Tensor down_path(const BlockL& Bk, const Tensor& v, const std::string& nm) {
    if (Bk.dir != 1) return v;
    const ConvL& rc = Bk.rc;
    Epi e;
    // wide levels: FIR + strided conv in one launch
    if (rc.fir_mode <= 1 && env.rate_small != 0 && rate_down_supported(rate_probe(rc, v.T))) {
      e.rate_down = true;
      if (rc.fir_mode == 1) { e.fir = W(rc.fir_off); e.fir_len = rc.fir_len; }
      return conv(rc, v, nm + ".h", e).out;
    }
    if (rc.fir_mode != 1) return conv(rc, v, nm + ".h", e).out;  // (fir_mode 3: FIR folded into the 3r-tap weights)
    const Tensor xf = alloc(nm + ".fir", v.C, v.T);
    launch("fir(down)", [&] {
      return launch_fir(v.p, W(rc.fir_off), rc.fir_len, h->alphas[rc.a_off], 1, nullptr, nullptr, 1.f, xf.p, B, v.C, v.T, st);
    });
    // (ragged batch: no mask needed -- the k = s = r conv that reads xf has no halo, and its own output is masked)
    e.act = false;  // PReLU applied by the FIR pass
    return conv(rc, xf, nm + ".h", e).out;
  }

  struct BlockOut { Tensor h_next, v, c1; };
  // `c1_dst` / `v_dst`: caller-provided (persistent) tensors for the conv1 result / the block output, so that
  // conditioner outputs are produced in place instead of being copied out of the scratch area afterwards
  BlockOut block(const BlockL& Bk, const Tensor& hin, const std::string& nm, const float* film, int film_bs,
                 const float* input_cond, const float* res, bool need_c1 = false, const Tensor* c1_dst = nullptr,
                 const Tensor* v_dst = nullptr) {
    const Tensor hu = up_path(Bk, hin, nm, res);
    Epi e1;
    if (input_cond) { e1.add = input_cond; e1.add_scale = kInvSqrt2; }  // blocks.py:384-386
    e1.film = film; e1.film_bstride = film_bs;                           // blocks.py:393-394
    BlockOut o;
    o.c1 = c1_dst ? *c1_dst : alloc(nm + ".c1", Bk.c1.Cout, hu.T);
    const Tensor c2 = alloc(nm + ".c2", Bk.c2.Cout, hu.T);
    o.v = v_dst ? *v_dst : alloc(nm + ".v", Bk.c3.Cout, hu.T);
    // (a plane per block, from the walk's own bump allocator: blocks of the conditioner and of the first score-encoder pass run
    // side by side on different streams; a model without Snake layers allocates nothing here)
    const Tensor act = Bk.has_snake() ? alloc(nm + ".act", Bk.C, hu.T) : Tensor();
    body(Bk, hu, o.c1, c2, o.v, nm, e1, need_c1, !need_c1 && !c1_dst, act);
    o.h_next = down_path(Bk, o.v, nm);
    return o;
  }

  // one bidirectional GRU layer: projection GEMM + cluster recurrence.  `before`: an event to take and record right in front of
  // the recurrence launch (null when none could be had)
  Tensor gru(const GruL& G, const Tensor& in, const std::string& nm, unsigned long long* xchg, unsigned* errw,
             unsigned* epoch, const float* res, float res_scale, hipEvent_t* before = nullptr) {
    Epi e;
    e.act = false;
    e.no_mask = true;
    Tensor gx = conv(G.proj, in, nm + ".gx", e).out;
    Tensor out = alloc(nm, 2 * G.H, in.T);
    if (dry || !ok()) return out;
    // ragged batch: frames behind a row's own end hold the state (z = 1): see launch_gru_tail_fill
    if (const int* ln = lens_of(in.T)) launch("gru tail fill", [&] { return launch_gru_tail_fill(gx.p, ln, B, G.H, in.T, st); });
    GruArgs a;
    a.gx = gx.p; a.whh = W(G.whh_off); a.bhn = W(G.bhn_off); a.out = out.p; a.res = res; a.res_scale = res_scale;
    a.xchg = xchg; a.err = errw; a.epoch = epoch; a.B = B; a.T = in.T; a.H = G.H;
    if (gru_area_rows > B) a.xchg_granules = gru_granules(gru_area_rows, G.H);
    // kernel generation: the ring kernel (every wave gathers h straight from L2, no polling wave, no workgroup barrier)
    // for every batch size; OU_GRU_V=1 selects the polling-wave kernel of round 1.  Its publishes: see below.
    a.version = env.gru_v;
    a.lanes = h->lanes;
    // (lanes whose calls differ in batch size must agree on the layout: shares and placement from the pool's largest batch)
    const int Bl = (h->lanes > 1 && h->lane_max_b > B) ? h->lane_max_b : B;
    a.share = gru_share_of(h->lanes, Bl, gru_shared);
    a.xcd_rot = h->lanes > 1 ? (2 * Bl * h->lane) % 8 : 0;
    a.force_bmax = env.gru_bmax;
    if (env.gru_ts) a.tstamps = (long long*)(base + cap - (1u << 20));
    a.force_upw = env.gru_upw;
    a.poll_backoff = env.gru_backoff;
    // publishes: PLAIN stores by default inside a cluster that shares one XCD (the L2 is that XCD's point of coherence; the
    // rendezvous proves the placement at every launch), agent-scope (sc1) stores otherwise, on request
    // (ou_set_gru_publish_mode) and -- for good -- from the moment ou_check_device_status sees that a publish really was
    // invisible to the gather's agent-scope loads on this handle (status word 33; word 20 also counts members that were
    // merely late).  A hipGraph captured before such a switch keeps the publish form it was captured with: re-capture.
    a.agent_stores = env.gru_agent >= 0 ? (env.gru_agent != 0) : h->gru_agent_stores;
    a.dbg = env.gru_dbg;
    // the recurrence proper (the input projection is a conv launch of its own): 2 directions x T steps x (3H x H) MACs;
    // variant code 1000 + steps per pass
    a.prof = prof_open(2.0 * 2.0 * 3.0 * G.H * G.H * (double)in.T * B,
                       4.0 * ((double)B * (6.0 + 2.0 + (res ? 2.0 : 0.0)) * G.H * in.T + 2.0 * 3.0 * G.H * G.H), 1000 + in.T);
    if (before && (*before = next_event())) launch("pre-gru record", [&] { return hipEventRecord(*before, st); });
    launch(G.name.c_str(), [&] { return launch_gru(a, h->num_cu, st); });
    mask(out);
    return out;
  }

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

Persist layout_persist(Runner& r, int T) {
  const Model& m = r.h->m;
  Persist P;
  // 64 status / diagnostics words + the fused ConvBlock kernel's barrier area (8 groups x 40 x 8 bytes)
  P.status = (unsigned*)r.alloc_raw(64 + 8 * 40 * 2);
  r.status_words = P.status;
  r.block3_bar = (unsigned long long*)(P.status + 64);
  int ncoef = kMaxSteps > r.B ? kMaxSteps : r.B;
  P.coef = (StepCoef*)r.alloc_raw((size_t)ncoef * 8);
  r.h->tensors["stats"] = TensorRef{r.off, 4, 1};  // (B, 4, 1): {mean removed, gain, mix_rms, 0} of each row's normalisation
  P.stats = r.alloc_raw((size_t)r.B * 4);
  P.rows = (RowInfo*)r.alloc_raw((size_t)r.B * 4);
  P.lens = (int*)r.alloc_raw((size_t)r.B * kMaxLenLevels);
  P.xchg = (unsigned long long*)r.alloc_raw(gru_granules(r.B, m.OC / 2) * 2);
  P.xchg2 = (unsigned long long*)r.alloc_raw(gru_granules(r.B, m.OC / 2) * 2);
  r.h->tensors["mel_scale"] = TensorRef{r.off, 1, 1};  // (B, 1, 1): the conditioner's mel normalisation of each row
  P.mel_scale = r.alloc_raw(r.B);
  r.h->tensors["sigma.g"] = TensorRef{r.off, m.film.D, 1};  // (B, D, 1): the noise-level embedding of the first B coefficient rows
  P.g = r.alloc_raw((size_t)ncoef * m.film.D);
  r.h->tensors["sigma.film"] = TensorRef{r.off, m.film.rows, 1};  // (B, rows, 1): their FiLM rows (gamma, beta per block)
  P.film = r.alloc_raw((size_t)ncoef * m.film.rows);
  P.mixn = r.alloc("mixn", 1, T);
  P.x = r.alloc("x", 1, T);
  P.wav = r.alloc("wav", 1, T);
  for (int j = 0; j < m.n_blocks; j++) {
    const BlockL& b = m.c_dec[j];
    int Tj = T / m.tot_ds;
    // length at the output of decoder block j
    int up = 1;
    for (int k = 0; k <= j; k++) if (m.c_dec[k].dir == 2) up *= m.c_dec[k].rate;
    Tj *= up;
    P.cond.push_back(r.alloc("cond.c" + std::to_string(j), b.C, Tj));
    P.sc.push_back(r.alloc("cond.sc" + std::to_string(j), b.C, Tj));
  }
  P.aux = r.alloc("cond.aux", m.C0, T);
  P.latent = r.alloc("cond.latent", m.OC, T / m.tot_ds);
  return P;
}

// ConditionerNetwork.forward(train=True)  condition.py:346-377
void run_condition(Runner& r, Persist& P, const float* mix_norm, int T) {
  const Model& m = r.h->m;
  const int L = T / m.tot_ds;
  const int n = m.n_levels - 1;
  hipStream_t main = r.st;
  const bool ov = r.h->overlap && !r.dry && r.h->lanes <= 1;
  // --- MelAdapter  condition.py:110-114 (independent of the encoder chain: side stream 0)
  if (ov) { r.fork(main, 0); r.st = r.h->aux[0]; }
  Tensor mel = r.alloc("cond.mel", m.mel.n_mels, L);
  float* esum = r.alloc_raw((size_t)r.B * L);
  r.launch("mel", [&] {
    return launch_mel(mix_norm, r.W(m.mel.win_off), r.W(m.mel.tw_off), r.W(m.mel.fb_off), mel.p, esum, r.B, T, m.mel.n_fft,
                      m.mel.hop, m.mel.pad_left, m.mel.n_freq, m.mel.n_mels, L, r.st);
  });
  if (!r.mel_scale_preset) r.launch("mel_scale", [&] { return launch_mel_scale(esum, P.mel_scale, r.B, L, r.st, r.lens_of(L)); });
  r.mask(mel);  // (frames behind a row's end still see its last samples)
  Runner::Epi em;
  em.in_scale = P.mel_scale;  // the global mel normalisation is linear: folded into the conv's input scale
  em.act = false;
  Tensor m0 = r.conv(m.c_melconv, mel, "cond.melconv", em).out;
  Tensor x_mel = r.block(m.c_melblock, m0, "cond.melblock", nullptr, 0, nullptr, nullptr).v;
  r.st = main;
  // --- input conv + encoder  condition.py:360, 189-206
  Tensor e0 = r.alloc("cond.in", m.C0, T);
  r.launch_masked("cond.in", e0.p, e0.C, e0.T, [&](const int* ln) {
    return launch_in_conv(mix_norm, r.W(m.c_in.w_off), r.W(m.c_in.b_off), nullptr, 0, e0.p, r.B, m.C0, T, m.c_in.KW, r.st, ln);
  });
  Tensor hcur = e0;
  std::vector<Tensor> outs;
  for (int i = 0; i < m.n_blocks; i++) {
    auto bo = r.block(m.c_enc[i], hcur, "cond.enc" + std::to_string(i), nullptr, 0, nullptr, nullptr);
    if (i < n - 1) {
      // strided "st" conv of this block's output: off the critical path (side stream 1)
      if (ov) { r.fork(main, 1); r.st = r.h->aux[1]; }
      const ConvL& S = m.c_st[i];
      const int R = S.rate, C = S.Cin / R;
      Tensor sd = r.alloc("cond.s2d" + std::to_string(i), S.Cin, bo.v.T / R);
      r.launch("s2d", [&] { return launch_s2d(bo.v.p, r.W(S.a_off), sd.p, r.B, C, bo.v.T, R, r.st); });
      Runner::Epi es;
      es.act = false;  // PReLU already applied by the space-to-depth pass
      outs.push_back(r.conv(S, sd, "cond.st" + std::to_string(i), es).out);
      r.st = main;
    }
    hcur = bo.h_next;
  }
  outs.push_back(hcur);
  if (ov) { r.join(0, main); r.join(1, main); }
  Tensor sum = r.alloc("cond.enc_sum", m.OC, L);
  if (!r.dry && r.ok() && outs.size() > 4) { r.herr = hipErrorInvalidValue; r.where = "too many encoder outputs"; return; }
  r.launch("enc_sum", [&] {
    const float* q[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < outs.size(); i++) q[i] = outs[i].p;
    return launch_sum(x_mel.p, q[0], q[1], q[2], q[3], 1.0f / std::sqrt((float)(outs.size() + 1)), sum.p, (size_t)r.B * m.OC * L,
                      r.st);
  });
  // --- conv_block1 -> 2-layer GRU (+residual) -> conv_block2   condition.py:208-216
  Tensor cb1 = r.block(m.c_cb1, sum, "cond.cb1", nullptr, 0, nullptr, nullptr).v;
  // status block: [0] error word, [2..3] / [4..5] = {tag epoch, finished-block count} of the two GRU exchange areas
  Tensor g0 = r.gru(m.c_gru0, cb1, "cond.gru0", P.xchg, P.status, P.status + 2, nullptr, 1.f);
  const bool gres = m.cfg.cond.encoder_gru_residual != 0;
  Tensor g1 = r.gru(m.c_gru1, g0, "cond.gru", P.xchg, P.status, P.status + 2, gres ? cb1.p : nullptr, kInvSqrt2);
  Tensor lat = r.block(m.c_cb2, g1, "cond.cb2", nullptr, 0, nullptr, nullptr, false, nullptr, &P.latent).v;
  // --- decoder  condition.py:264-270
  Tensor y = r.block(m.c_decin, lat, "cond.decin", nullptr, 0, nullptr, nullptr).v;
  for (int j = 0; j < m.n_blocks; j++) {
    // condition j = conv1 output of decoder block j (condition.py:264-270); the last block's output is the aux signal
    auto bo = r.block(m.c_dec[j], y, "cond.dec" + std::to_string(j), nullptr, 0, nullptr, nullptr, true, &P.cond[j],
                      j == m.n_blocks - 1 ? &P.aux : nullptr);
    y = bo.v;
    // score.py:208  sc = signal_cond_proj_j(cond_j): independent of x and sigma -> computed once here
    {
      Runner::Epi es;
      es.act = false;
      r.conv(m.s_sig[j], bo.c1, "cond.sc" + std::to_string(j), es, &P.sc[j]);
    }
  }
}

// ScoreNetwork.forward + EDM wrapper + sampler update for the coefficient rows at `coef`
//   film_row: pointer to this step's FiLM table row(s); film_bs / coef_bs: per-batch strides (0 = shared)
// Split in two halves: the encoder + GRU half does not depend on the conditioner (cond enters the decoder only),
// so the first step's encoder can run concurrently with it.
struct ScoreEnc {
  std::vector<Tensor> residuals;
  Tensor hg;
  bool fuse_res = false;
};
// `pre_gru`: an event to record right in front of the GRU launch (Runner::gru)
ScoreEnc run_score_enc(Runner& r, Persist& P, const float* x, const StepCoef* coef, int coef_bs,
                       const float* film_row, int film_bs, int T, hipEvent_t* pre_gru = nullptr) {
  const Model& m = r.h->m;
  ScoreEnc E;
  Tensor e0 = r.alloc("score.in", m.C0, T);
  // the w_in scaling of the EDM wrapper (universe.py:199,202) rides on the input conv
  r.launch_masked("score.in", e0.p, e0.C, e0.T, [&](const int* ln) {
    return launch_in_conv(x, r.W(m.s_in.w_off), r.W(m.s_in.b_off), coef, coef_bs, e0.p, r.B, m.C0, T, m.s_in.KW, r.st, ln);
  });
  Tensor hcur = e0;
  for (int i = 0; i < m.n_blocks; i++) {
    const float* fr = film_row ? film_row + m.film.enc_off[i] : nullptr;
    auto bo = r.block(m.s_enc[i], hcur, "score.enc" + std::to_string(i), fr, film_bs, nullptr, nullptr);
    E.residuals.push_back(bo.v);
    hcur = bo.h_next;
  }
  // GRU bottleneck; when decoder block 0 has no rate change its residual add (blocks.py:374-376) is fused here
  E.fuse_res = m.s_dec[0].dir == 0;
  E.hg = r.gru(m.s_gru, hcur, "score.gru", P.xchg2, P.status, P.status + 4,
               E.fuse_res && !r.dry ? E.residuals[m.n_blocks - 1].p : nullptr, kInvSqrt2, pre_gru);
  return E;
}
void run_score_dec(Runner& r, Persist& P, const ScoreEnc& E, const float* x, const float* noise, float* out, int mode,
                   const StepCoef* coef, int coef_bs, const float* film_row, int film_bs, int T, const Tensor* dec0_done = nullptr) {
  const Model& m = r.h->m;
  Tensor y = E.hg;
  for (int j = 0; j < m.n_blocks; j++) {
    if (j == 0 && dec0_done) { y = *dec0_done; continue; }
    const float* fr = film_row ? film_row + m.film.dec_off[j] : nullptr;
    const Tensor& res = E.residuals[m.n_blocks - 1 - j];
    const float* resp = (j == 0 && E.fuse_res) ? nullptr : res.p;
    auto bo = r.block(m.s_dec[j], y, "score.dec" + std::to_string(j), fr, film_bs, P.sc[j].p, resp);
    y = bo.v;
  }
  r.launch_masked("score.out", out, 1, T, [&](const int* ln) {
    return launch_out_conv(y.p, r.W(m.s_out.w_off), r.W(m.s_out.b_off), r.W(m.s_out.a_off), x, noise, out, coef, coef_bs,
                           m.cfg.has_edm, mode, r.B, m.C0, T, m.s_out.KW, r.st, ln);
  });
}
static bool m_blocks_ok(const Runner& r) { return r.h->m.n_blocks >= 1 && r.h->m.s_dec[0].dir == 0; }
void run_score(Runner& r, Persist& P, const float* x, const float* noise, float* out, int mode,
               const StepCoef* coef, int coef_bs, const float* film_row, int film_bs, int T) {
  // OU_DBG_DEC0=1 -- MEASUREMENT ONLY, RESULTS INVALID: the first decoder block is launched on a side stream that waits for
  // what precedes the GRU launch instead of the GRU itself, i.e. its three convs run UNDER the recurrence (on whatever that has
  // written so far).  The time of a forward in this mode is a lower bound for any scheme that gates those convs on the
  // recurrence's progress: the gated version can only start later and wait more.
  const bool dec0_under = r.env.dbg_dec0_under_gru != 0 && !r.dry && r.h->overlap && r.h->lanes <= 1 && m_blocks_ok(r);
  hipEvent_t pre_gru = nullptr;
  ScoreEnc E = run_score_enc(r, P, x, coef, coef_bs, film_row, film_bs, T, dec0_under ? &pre_gru : nullptr);
  if (dec0_under && pre_gru && r.ok()) {
    const Model& m = r.h->m;
    hipStream_t main = r.st;
    r.launch("dec0 wait", [&] { return hipStreamWaitEvent(r.h->aux[0], pre_gru, 0); });
    r.st = r.h->aux[0];
    const float* fr = film_row ? film_row + m.film.dec_off[0] : nullptr;
    const Tensor& res = E.residuals[m.n_blocks - 1];
    auto bo = r.block(m.s_dec[0], E.hg, "score.dec0", fr, film_bs, P.sc[0].p, E.fuse_res ? nullptr : res.p);
    r.st = main;
    r.join(0, main);
    Tensor done = bo.v;
    run_score_dec(r, P, E, x, noise, out, mode, coef, coef_bs, film_row, film_bs, T, &done);
    return;
  }
  run_score_dec(r, P, E, x, noise, out, mode, coef, coef_bs, film_row, film_bs, T);
}

// universe.py:175-189, 197-209, 333-343 scalars for one sigma, computed in fp32 like the reference's tensors
StepCoef make_coef(const ou_config& cfg, float s, bool last, double eta, double beta, float s_next) {
  StepCoef c;
  const float s2 = s * s;
  if (cfg.has_edm) {
    // universe.py:176-178: sigma_data from edm.data_level_db, else from normalization_kwargs.level_db
    const double sd = std::pow(10.0, (double)(cfg.has_edm_data_level ? cfg.edm_data_level_db : cfg.level_db) / 20.0);
    const float sd2 = (float)(sd * sd);
    const float sn2 = s2 + sd2;
    const float sn = std::sqrt(sn2);
    c.w_skip = sd2 / sn2;
    c.w_in = 1.0f / sn;
    c.w_out = (s * (float)sd) / sn;
    c.sigma_net = cfg.edm_noise * s;
  } else {
    c.w_skip = 0.f; c.w_in = 1.f; c.w_out = 1.f; c.sigma_net = s;
  }
  c.sig2 = s2;
  c.c1 = last ? s2 : s2 * (float)eta;
  c.s_next = s_next;
  c.beta = (float)beta;
  return c;
}

void schedule(const ou_config& cfg, int n_steps, double epsilon, float* sigma, double* eta, double* beta) {
  const double ratio = (double)cfg.sigma_max / (double)cfg.sigma_min;
  const double delta_t = 1.0 / (n_steps - 1);
  const double gamma = std::pow(ratio, -delta_t);
  *eta = 1.0 - std::pow(gamma, epsilon);
  *beta = std::sqrt(1.0 - std::pow(gamma, 2.0 * (epsilon - 1.0)));
  // torch.linspace(0, 1, N) (fp32, symmetric evaluation) flipped, then s_min * (s_max/s_min) ** time
  const float step = 1.0f / (float)(n_steps - 1);
  for (int n = 0; n < n_steps; n++) {
    int i = n_steps - 1 - n;
    float t = (i < n_steps / 2) ? (float)i * step : 1.0f - (float)(n_steps - 1 - i) * step;
    sigma[n] = (float)cfg.sigma_min * std::pow((float)ratio, t);  // fp32 pow like torch.pow(Scalar, fp32 Tensor)
  }
}

void upload_coefs(Runner& r, StepCoef* dst, const std::vector<StepCoef>& rows) {
  for (size_t i = 0; i < rows.size(); i += 64) {
    CoefBlock blk;
    int n = (int)std::min<size_t>(64, rows.size() - i);
    for (int k = 0; k < n; k++) blk.c[k] = rows[i + k];
    r.launch("upload coef", [&] { return launch_upload_coef(dst + i, blk, n, r.st); });
  }
}

// the FiLM rows of the first n coefficient rows at P.coef
void upload_film_rows(Runner& r, Persist& P, int n) {
  const Model& m = r.h->m;
  r.launch("sigma", [&] { return launch_sigma_embed(P.coef, n, r.W(m.sigma.p_off), m.sigma.simple, m.sigma.n_rff, m.film.D, P.g, r.st); });
  r.launch("film", [&] { return launch_film(P.g, r.W(m.film.w_off), r.W(m.film.b_off), P.film, n, m.film.rows, m.film.D, r.st); });
}

long long max_walk_length(ou_handle* h, bool need_wav);

int finish(ou_handle* h, Runner& r) {
  if (r.oom) return fail(h, OU_ENOMEM, "workspace too small: need " + std::to_string(r.off) + " bytes");
  if (r.herr != hipSuccess)
    return fail(h, OU_EHIP, std::string("HIP error at ") + r.where + ": " + hipGetErrorString(r.herr));
  return OU_OK;
}

}  // namespace

// ======================================================================================================
extern "C" {

const char* ou_version(void) {
#ifdef OU_EXPERIMENTS
  return "libouniverse 0.2 (gfx950, fp32 MFMA) +experiments";
#else
  return "libouniverse 0.2 (gfx950, fp32 MFMA)";
#endif
}
const char* ou_last_error(const ou_handle* h) { return h ? h->err.c_str() : g_last_error.c_str(); }
const char* ou_packer_last_error(const ou_packer* p) { return p ? p->err.c_str() : g_last_error.c_str(); }

int ou_packer_create(const ou_config* cfg, ou_packer** out) {
  if (!cfg || !out) return fail(nullptr, OU_EINVAL, "null argument");
  auto* p = new ou_packer();
  std::string e = build_model(*cfg, p->m);
  if (!e.empty()) { delete p; return fail(nullptr, OU_ENOTIMPL, e); }
  *out = p;
  return OU_OK;
}

int ou_packer_set(ou_packer* p, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  if (!p || !key || !data || ndim < 0 || ndim > 8) return fail(nullptr, OU_EINVAL, "bad argument to ou_packer_set");
  HostTensor t;
  size_t n = 1;
  for (int i = 0; i < ndim; i++) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
  t.data.assign(data, data + n);
  p->sd[key] = std::move(t);
  return OU_OK;
}

int ou_packer_finish(ou_packer* p, const float** blob_host, size_t* nbytes) {
  if (!p || !blob_host || !nbytes) return fail(nullptr, OU_EINVAL, "null argument");
  int code = OU_OK;
  std::string e = pack_weights(p->m, p->sd, p->blob, code);
  if (!e.empty()) { p->err = e; g_last_error = e; return code; }
  *blob_host = p->blob.data();
  *nbytes = p->blob.size() * sizeof(float);
  return OU_OK;
}

void ou_packer_destroy(ou_packer* p) { delete p; }

int ou_packed_bytes(const ou_config* cfg, size_t* nbytes) {
  if (!cfg || !nbytes) return fail(nullptr, OU_EINVAL, "null argument");
  Model m;
  std::string e = build_model(*cfg, m);
  if (!e.empty()) return fail(nullptr, OU_ENOTIMPL, e);
  *nbytes = m.total_floats * sizeof(float);
  return OU_OK;
}

const char* ou_packer_plan_json(const ou_packer* p) { return p ? p->m.json.c_str() : ""; }
const char* ou_plan_json(const ou_handle* hc) {
  if (!hc) return "";
  ou_handle* h = const_cast<ou_handle*>(hc);
  // the plan of the packed layers + the current values of the handle's options (ou_set_option)
  std::string o = "\"options\": {";
  for (int i = 0; i < kNumOptions; i++) {
    const OptDesc& d = kOptions[i];
    char buf[96];
    if (d.ip) std::snprintf(buf, sizeof buf, "%s\"%s\": %d", i ? ", " : "", d.key, h->opt.*(d.ip));
    else std::snprintf(buf, sizeof buf, "%s\"%s\": %.9g", i ? ", " : "", d.key, h->opt.*(d.dp));
    o += buf;
  }
  o += "}";
  o += std::string(", \"noise_source\": \"") + (h->noise_src.on ? "counter" : "tensor") + "\"";
  {
    char buf[96];
    std::snprintf(buf, sizeof buf, ", \"norm\": \"%s\", \"zero_mean\": %d, \"norm_eps\": %.9g",
                  h->norm.norm == OU_NORM_MAX ? "max" : h->norm.norm == OU_NORM_2MAX ? "2-max" : "2", h->norm.zero_mean, h->norm.eps);
    o += buf;
  }
  const std::string& j = h->m.json;
  const size_t close = j.rfind('}');
  h->plan_with_options = close == std::string::npos ? "{" + o + "}" : j.substr(0, close) + ", " + o + j.substr(close);
  return h->plan_with_options.c_str();
}

int ou_set_normalization(ou_handle* h, int32_t norm_mode, int32_t zero_mean, float eps) {
  if (!h) return OU_EINVAL;
  if (norm_mode != OU_NORM_2 && norm_mode != OU_NORM_MAX && norm_mode != OU_NORM_2MAX)
    return fail(h, OU_EINVAL, "ou_set_normalization: norm_mode must be OU_NORM_2, OU_NORM_MAX or OU_NORM_2MAX");
  if (zero_mean != 0 && zero_mean != 1) return fail(h, OU_EINVAL, "ou_set_normalization: zero_mean must be 0 or 1");
  if (!(eps >= 0.f) || !std::isfinite(eps)) return fail(h, OU_EINVAL, "ou_set_normalization: eps must be finite and >= 0 (0: 1e-5)");
  h->norm.norm = norm_mode;
  h->norm.zero_mean = zero_mean;
  // utils/norm.py:31-39: normalization_kwargs.eps reaches the norms in the 2-max branch only
  h->norm.eps = norm_mode == OU_NORM_2MAX && eps > 0.f ? eps : 1e-5f;
  return OU_OK;
}

int ou_set_option(ou_handle* h, const char* key, double value) {
  if (!h || !key) return fail(h, OU_EINVAL, "bad argument");
  const OptDesc* d = find_option(key);
  if (!d) return fail(h, OU_EMISSING, std::string("ou_set_option: no such option: ") + key);
#ifndef OU_EXPERIMENTS
  if (d->experiments_only && value != 0.0)
    return fail(h, OU_ENOTIMPL, std::string("ou_set_option: `") + key + "` makes calls return wrong results by design and exists in "
                "the experiments build (make EXPERIMENTS=1) only");
#endif
  if (d->ip) {
    if (value != std::floor(value) || std::fabs(value) > 2e9) return fail(h, OU_EINVAL, std::string("ou_set_option: `") + key + "` takes an integer");
    h->opt.*(d->ip) = (int)value;
  } else {
    h->opt.*(d->dp) = value;
  }
  h->trace = h->opt.trace != 0;
  h->overlap = h->opt.no_overlap == 0;
  return OU_OK;
}

int ou_get_option(const ou_handle* h, const char* key, double* value) {
  if (!h || !key || !value) return fail(const_cast<ou_handle*>(h), OU_EINVAL, "bad argument");
  const OptDesc* d = find_option(key);
  if (!d) return fail(const_cast<ou_handle*>(h), OU_EMISSING, std::string("ou_get_option: no such option: ") + key);
  *value = d->ip ? (double)(h->opt.*(d->ip)) : h->opt.*(d->dp);
  return OU_OK;
}

int ou_reset_options(ou_handle* h) {
  if (!h) return fail(h, OU_EINVAL, "bad argument");
  const std::string keep = h->opt.chain_ts;
  h->opt = Options();
  h->opt.chain_ts = keep;
  h->trace = false;
  h->overlap = true;
  return OU_OK;
}

int ou_option_count(void) { return kNumOptions; }
const char* ou_option_name(int32_t i) { return i >= 0 && i < kNumOptions ? kOptions[i].key : nullptr; }
const char* ou_option_doc(int32_t i) { return i >= 0 && i < kNumOptions ? kOptions[i].doc : nullptr; }
double ou_option_default(int32_t i) {
  if (i < 0 || i >= kNumOptions) return 0.0;
  const Options d;
  return kOptions[i].ip ? (double)(d.*(kOptions[i].ip)) : d.*(kOptions[i].dp);
}

int ou_set_stamp_layer(ou_handle* h, const char* block_name) {
  if (!h) return fail(h, OU_EINVAL, "bad argument");
  h->opt.chain_ts = block_name ? block_name : "";
  return OU_OK;
}

int ou_create(const ou_config* cfg, const void* weights_dev, size_t nbytes, int32_t device, ou_handle** out) {
  if (!cfg || !weights_dev || !out) return fail(nullptr, OU_EINVAL, "null argument");
  auto* h = new ou_handle();
  std::string e = build_model(*cfg, h->m);
  if (!e.empty()) { delete h; return fail(nullptr, OU_ENOTIMPL, e); }
  if (nbytes != h->m.total_floats * sizeof(float)) {
    size_t want = h->m.total_floats * sizeof(float);
    delete h;
    return fail(nullptr, OU_ESHAPE, "packed weight blob has " + std::to_string(nbytes) + " bytes, expected " + std::to_string(want));
  }
  int ndev = 0;
  hipError_t he = hipGetDeviceCount(&ndev);
  if (he != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    delete h;
    return fail(nullptr, OU_EHIP, "no HIP device available for ou_create (this library has no CPU path)");
  }
  hipDeviceProp_t prop;
  he = hipGetDeviceProperties(&prop, device);
  if (he != hipSuccess) { delete h; return fail(nullptr, OU_EHIP, hipGetErrorString(he)); }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    std::string arch = prop.gcnArchName;
    delete h;
    return fail(nullptr, OU_EHIP, "libouniverse is built for gfx950 (MI355X) only; device is " + arch);
  }
  h->num_cu = prop.multiProcessorCount;
  h->trace = false;
  h->device = device;
  h->W = (const float*)weights_dev;
  (void)hipSetDevice(device);
  {  // host copies of the conv PReLU slopes: passed to the kernels by value
    std::vector<const ConvL*> all;
    auto addb = [&](const BlockL& b) { if (b.dir) all.push_back(&b.rc); all.push_back(&b.c1); all.push_back(&b.c2); all.push_back(&b.c3); };
    const Model& m = h->m;
    for (auto& b : m.s_enc) addb(b);
    for (auto& b : m.s_dec) addb(b);
    addb(m.c_melblock);
    for (auto& b : m.c_enc) addb(b);
    for (auto& l : m.c_st) all.push_back(&l);
    addb(m.c_cb1); addb(m.c_cb2); addb(m.c_decin);
    for (auto& b : m.c_dec) addb(b);
    for (auto* l : all) {
      if (!l->act) continue;
      float v = 0.f;
      he = hipMemcpy(&v, h->W + l->a_off, sizeof(float), hipMemcpyDeviceToHost);
      if (he != hipSuccess) { delete h; return fail(nullptr, OU_EHIP, hipGetErrorString(he)); }
      h->alphas[l->a_off] = v;
    }
  }
  he = init_conv_kernels();
  if (he != hipSuccess) { delete h; return fail(nullptr, OU_EHIP, hipGetErrorString(he)); }
  for (int i = 0; i < 3; i++) {
    he = hipStreamCreateWithFlags(&h->aux[i], hipStreamNonBlocking);
    if (he != hipSuccess) { delete h; return fail(nullptr, OU_EHIP, hipGetErrorString(he)); }
  }
  h->overlap = true;
  *out = h;
  return OU_OK;
}

void ou_destroy(ou_handle* h) {
  if (!h) return;
  if (h->prof_dev) (void)hipFree(h->prof_dev);
  for (auto& e : h->events) (void)hipEventDestroy(e);
  for (int i = 0; i < 3; i++) if (h->aux[i]) (void)hipStreamDestroy(h->aux[i]);
  delete h;
}

int ou_workspace_bytes(const ou_handle* hc, int32_t B, int32_t T, size_t* nbytes) {
  ou_handle* h = const_cast<ou_handle*>(hc);
  if (!h || !nbytes || B < 1 || T < 1) return fail(h, OU_EINVAL, "bad argument");
  if (T % h->m.tot_ds) return fail(h, OU_EINVAL, "T must be a multiple of the total down-sampling factor");
  if (T > max_walk_length(h, false))  // (the length guard of ou_enhance: refused before a caller allocates for it)
    return fail(h, OU_EINVAL, "input too long for one pass: a plane of the walk would reach 2^32 bytes; ou_enhance_segments "
                              "enhances it in windows");
  auto saved = h->tensors;
  Runner r(h, nullptr, 0, true, nullptr, B);
  Persist P = layout_persist(r, T);
  run_condition(r, P, nullptr, T);
  size_t mark = r.off;
  run_score(r, P, nullptr, nullptr, nullptr, OUT_UPDATE, nullptr, 0, nullptr, 0, T);
  (void)mark;
  // aux_to_wav scratch (2x up-sampled aux signal)
  r.alloc_raw((size_t)B * h->m.C0 * 2 * T);
  h->tensors = saved;
  *nbytes = r.off + 4096;
  return OU_OK;
}

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

namespace {
// Length guard: the kernels of the walk address one batch row's (C, T) plane with 32-bit buffer descriptors, so no plane may
// reach 2^32 bytes.  Every plane is (channels) x (T * num / den): one dry walk (conditioner + one score pass, batch 1) gives the
// largest plane per padded sample, cached in the handle.  Returns the largest padded length the walk takes.
long long max_walk_length(ou_handle* h, bool need_wav) {
  if (h->plane_per_sample == 0.0) {
    const int T0 = h->m.tot_ds * 64;
    auto keep = h->tensors;
    Runner d(h, nullptr, 0, true, nullptr, 1);
    Persist Pd = layout_persist(d, T0);
    run_condition(d, Pd, nullptr, T0);
    run_score(d, Pd, nullptr, nullptr, nullptr, OUT_UPDATE, nullptr, 0, nullptr, 0, T0);
    h->tensors = keep;
    h->plane_per_sample = (double)d.max_plane / T0;
    h->wav_plane_per_sample = (double)h->m.C0 * 2 * 4;  // decoupling scratch: (C0, 2 T) per row
  }
  double per = h->plane_per_sample;
  if (need_wav && h->wav_plane_per_sample > per) per = h->wav_plane_per_sample;
  // (4 KiB of head room: the padded descriptors of the up-sampling kernels reach a few samples in front of the plane)
  const double lim = (4294967296.0 - 4096.0) / per;
  long long t = (long long)lim;
  return t - t % h->m.tot_ds;
}

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

// ---- the pieces the enhance entry points share.  ou_enhance / ou_enhance_var, ou_enhance_ensemble,
// ou_enhance_segments and ou_enhance_segments_var are these pieces plus what each adds of its own.

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

// A launch outside any walk, counted and reported as Runner::chk + finish do; false: it failed, enqueue nothing more.
bool launched(ou_handle* h, hipError_t e, const char* w) {
  h->n_launch++;
  if (e == hipSuccess) return true;
  fail(h, OU_EHIP, std::string("HIP error at ") + w + ": " + hipGetErrorString(e));
  return false;
}

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
struct PostFlags {
  int keep_rms, peak;
  explicit PostFlags(uint32_t flags) : keep_rms((flags & OU_ENH_KEEP_RMS) ? 1 : 0), peak((flags & OU_ENH_NO_PEAK_GUARD) ? 0 : 1) {}
};
// unpad, de-normalise, keep_rms and the peak guard of `rows` rows of x -> out
void post(Runner& r, Persist& P, const float* x, float* out, int rows, int T_raw, int T, PostFlags f) {
  r.launch("post", [&] {
    return r.ragged ? launch_post_var(x, P.stats, out, P.rows, rows, T_raw, T, f.keep_rms, f.peak, r.st)
                    : launch_post(x, P.stats, out, rows, T_raw, T, (T - T_raw) / 2, f.keep_rms, f.peak, r.st);
  });
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

// universe.py:325-327: x = sigma * z_0 (+ the warm start's signal).  `mask`: the plane may hold noise behind a row's own end.
void init_x(Runner& r, Persist& P, const float* z0, const float* warm, float sigma, int T, bool mask) {
  r.launch("init x", [&] { return launch_init_x(z0, warm, sigma, P.x.p, (size_t)r.B * T, r.st); });
  if (mask) r.mask(P.x);
}
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
  if (need_wav && (!m.dec.present || m.dec.act != OU_ACT_SNAKE))
    return fail(h, OU_ENOTIMPL, "aux_to_wav needs the snake signal-decoupling layer (UNIVERSE++)");
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
    const bool gru_fit = gru_ring_batch_cap(m.s_gru.H, h->num_cu, share2, 0, B, h->lanes) >= 1 &&
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
  if (need_wav && (!m.dec.present || m.dec.act != OU_ACT_SNAKE))
    return fail(h, OU_ENOTIMPL, "aux_to_wav needs the snake signal-decoupling layer (UNIVERSE++)");
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

}  // extern "C"

namespace {
// Segment plan (include/ouniverse.h, ou_segment_plan): a pure function of (T_raw, tot_ds, segment, overlap).
struct SegPlan {
  SegGeom g;
  std::string err;
};
bool seg_plan(int tot, long long T_raw, long long segment, long long overlap, SegPlan& p) {
  if (tot < 1 || T_raw < 1) { p.err = "segment plan: T_raw >= 1 and tot_ds >= 1"; return false; }
  const long long S = segment - segment % tot, O = overlap - overlap % tot;
  if (S < tot) { p.err = "segment must be at least one total down-sampling factor (" + std::to_string(tot) + " samples)"; return false; }
  if (O < 0 || 2 * O > S) { p.err = "overlap must lie in [0, segment / 2]"; return false; }
  SegGeom& g = p.g;
  const long long pad = tot - T_raw % tot;  // universe.py:219-223
  g.T_raw = T_raw;
  g.T_pad = T_raw + pad;
  g.pad_left = pad / 2;
  if (g.T_pad <= S) {
    g.L = g.T_pad; g.hop = g.T_pad; g.overlap = 0; g.n_win = 1;
  } else {
    g.L = S; g.hop = S - O; g.overlap = O;
    g.n_win = (g.T_pad - S + g.hop - 1) / g.hop + 1;
  }
  g.n_entries = g.n_win;  // (per row; the caller multiplies by the rows)
  return true;
}
long long seg_start_host(const SegGeom& g, long long k) { return k < g.n_win - 1 ? k * g.hop : g.T_pad - g.L; }
// batch size of every group: the entries spread evenly over ceil(E / max_batch) groups
int seg_batch(long long entries, int max_batch) {
  const long long groups = (entries + max_batch - 1) / max_batch;
  return (int)((entries + groups - 1) / groups);
}
// The segmented call's own area behind the walk's workspace (offsets in bytes): E member rows per input row, Bw entries (E * Bw
// walk rows of L samples) per group.  `with_hist`: the scratch of the ensemble reduce; `with_table`: the SegRow table and -- E > 1
// -- the [level][Bw] length table of a ragged group's shared conditioner pass (the walk's own table is [level][E * Bw]).
struct SegArea {
  size_t stats, row_scale, part, zbuf, carry, hist, geom, lens_b, total;
};
SegArea seg_area(int C, int E, int Bw, long long L, bool with_hist, bool with_table) {
  SegArea a;
  size_t off = 0;
  a.stats = off; off += align256((size_t)C * 4 * 4);
  a.row_scale = off; off += align256((size_t)C * 4);
  // the statistics' partials of the C input rows ([C][nb][3] sums and the [C][nb] block maxima behind them, nb <= 1024: the
  // fourth is reserved whatever the handle's NormMode, so the area does not depend on ou_set_normalization, called early or
  // late, and every instantiation of seg_stats2_kernel writes inside it), then the post partials of the E * C long rows ([E * C][nb][2])
  a.part = off; off += align256(std::max((size_t)C * 4, (size_t)E * C * 2) * 1024 * 8);
  a.zbuf = off; off += align256((size_t)E * Bw * L * 4);
  a.carry = off; off += align256((size_t)E * L * 4);
  a.hist = off; off += with_hist ? ou_ensemble_reduce_scratch_bytes(E, C) : 0;
  a.geom = off; off += with_table ? align256((size_t)C * sizeof(SegRow)) : 0;
  a.lens_b = off; off += with_table && E > 1 ? align256((size_t)Bw * kMaxLenLevels * 4) : 0;
  a.total = off;
  return a;
}
// what a *_workspace_bytes function answers: the walk of B rows of L samples plus the area
int seg_workspace_bytes(ou_handle* h, int B, long long L, const SegArea& A, size_t* nbytes, int32_t* batch, int32_t* length) {
  size_t walk = 0;
  if (const int rc = ou_workspace_bytes(h, B, (int32_t)L, &walk)) return rc;
  *nbytes = align256(walk) + A.total;
  if (batch) *batch = B;
  if (length) *length = (int32_t)L;
  return OU_OK;
}
// The caller's workspace against that answer (`sizer`: the name of the function that gives it), and the area's pointers.
struct SegWs {
  size_t walk;  // bytes of the walk's part
  size_t stats_off;  // `stats` in bytes from the workspace's start (ou_tensor "seg.stats")
  float *stats, *row_scale, *zbuf, *carry;
  double* part;
  int *hist, *lens_b;
  SegRow* geom;
};
int seg_workspace(ou_handle* h, void* ws, size_t ws_bytes, int B, int L, const SegArea& A, const char* sizer, SegWs& w) {
  if (const int rc = ou_workspace_bytes(h, B, L, &w.walk)) return rc;
  w.walk = align256(w.walk);
  if (ws_bytes < w.walk + A.total)
    return fail(h, OU_ENOMEM, "workspace too small: need " + std::to_string(w.walk + A.total) + " bytes (" + sizer + ")");
  if (!h->ws_ok(ws, ws_bytes, B, L))
    return fail(h, OU_EINVAL, std::string("workspace was not prepared by ou_workspace_init for (batch, length) of ") + sizer);
  char* seg = (char*)ws + w.walk;
  w.stats = (float*)(seg + A.stats);
  w.stats_off = w.walk + A.stats;
  w.row_scale = (float*)(seg + A.row_scale);
  w.part = (double*)(seg + A.part);
  w.zbuf = (float*)(seg + A.zbuf);
  w.carry = (float*)(seg + A.carry);
  w.hist = (int*)(seg + A.hist);
  w.geom = (SegRow*)(seg + A.geom);
  w.lens_b = (int*)(seg + A.lens_b);
  return OU_OK;
}
// what every entry point of the segmented ensembles refuses about its member count
int seg_ens_members(ou_handle* h, const char* who, int C, int max_batch, int E) {
  if (E < 1 || E > OU_MAX_ENSEMBLE) return fail(h, OU_EINVAL, std::string(who) + ": 1 <= E <= " + std::to_string(OU_MAX_ENSEMBLE));
  if (E > max_batch) return fail(h, OU_EINVAL, std::string(who) + ": E must not exceed max_batch (a group holds all E members of its entries)");
  if ((long long)E * C > 65535) return fail(h, OU_EINVAL, std::string(who) + ": too many member rows (E * C <= 65535)");
  return OU_OK;
}
// ... and the plan of the call on rows of one length.  Bw: entries per group
int seg_ens_plan(ou_handle* h, const char* who, int C, long long T_raw, int segment, int overlap, int max_batch, int E, SegGeom& g,
                 int& Bw) {
  if (C < 1 || T_raw < 1 || max_batch < 1) return fail(h, OU_EINVAL, "bad argument");
  if (const int rc = seg_ens_members(h, who, C, max_batch, E)) return rc;
  SegPlan plan;
  if (!seg_plan(h->m.tot_ds, T_raw, segment, overlap, plan)) return fail(h, OU_EINVAL, plan.err);
  g = plan.g;
  if (g.L > 0x7fffffffll) return fail(h, OU_EINVAL, "segment too long");
  g.n_entries = (long long)C * g.n_win;
  Bw = seg_batch(g.n_entries, max_batch / E);
  return OU_OK;
}

// Window groups of rows with lengths of their own (include/ouniverse.h, ou_segment_groups): a pure host function.
struct SegEntry { int row, win, len; };
struct SegGroups {
  std::vector<SegGeom> rows;        // the plan of every row (seg_plan)
  std::vector<long long> first;     // the row's first entry
  std::vector<SegEntry> entries;    // class FULL (row-major), then class SHORT (input order)
  std::vector<int> group_first;     // first entry of every group
  std::vector<char> group_ragged;
  long long n_full = 0;             // entries of class FULL
  long long S = 0, hop = 0, O = 0;  // window length, hop and crossfade of the long rows
  int batch = 0;
  long long length = 0;             // the longest entry = min(S, max T_pad)
  std::string err;
};
bool seg_groups(int tot, int C, const int64_t* t_raw, long long segment, long long overlap, int max_batch, SegGroups& G) {
  if (C < 1 || !t_raw || max_batch < 1) { G.err = "segment groups: C >= 1, t_raw given and max_batch >= 1"; return false; }
  G.rows.resize(C);
  G.first.assign(C, 0);
  long long n_full = 0, n_short = 0;
  for (int c = 0; c < C; c++) {
    SegPlan p;
    if (!seg_plan(tot, t_raw[c], segment, overlap, p)) { G.err = p.err; return false; }
    G.rows[c] = p.g;
    if (p.g.L > 0x7fffffffll) { G.err = "segment too long"; return false; }
    if (p.g.n_win > 1) n_full += p.g.n_win; else n_short++;
    G.length = std::max(G.length, p.g.L);
  }
  if (n_full + n_short > 0x7fffffffll) { G.err = "segment groups: too many windows"; return false; }
  G.S = segment - segment % tot;
  G.O = overlap - overlap % tot;
  G.hop = G.S - G.O;
  G.n_full = n_full;
  G.batch = std::max(n_full ? seg_batch(n_full, max_batch) : 0, n_short ? seg_batch(n_short, max_batch) : 0);
  G.entries.reserve((size_t)(n_full + n_short));
  for (int c = 0; c < C; c++)
    if (G.rows[c].n_win > 1) {
      G.first[c] = (long long)G.entries.size();
      for (long long k = 0; k < G.rows[c].n_win; k++) G.entries.push_back(SegEntry{c, (int)k, (int)G.rows[c].L});
    }
  for (int c = 0; c < C; c++)
    if (G.rows[c].n_win == 1) {
      G.first[c] = (long long)G.entries.size();
      G.entries.push_back(SegEntry{c, 0, (int)G.rows[c].L});
    }
  auto add_groups = [&](long long e0, long long e1) {
    for (long long e = e0; e < e1; e += G.batch) {
      const long long end = std::min<long long>(e + G.batch, e1);
      bool ragged = false;
      for (long long i = e + 1; i < end; i++) ragged = ragged || G.entries[i].len != G.entries[e].len;
      G.group_first.push_back((int)e);
      G.group_ragged.push_back(ragged ? 1 : 0);
    }
  };
  add_groups(0, n_full);
  add_groups(n_full, n_full + n_short);
  return true;
}

// ---- the pieces of the segmented calls ------------------------------------------------------------------------
// Whole-row statistics and frame energies of the C input rows (`esum`: the output rows hold the energies until the first stitch);
// the caller turns the energies into w.row_scale.  false: a launch failed.
template <class Rows>
bool seg_row_stats(ou_handle* h, const float* mix, float* esum, const SegWs& w, const Rows& rows, int C, long long frames_max,
                   hipStream_t st) {
  const Model& m = h->m;
  const float level = (float)std::pow(10.0, (double)m.cfg.level_db / 20.0);
  h->tensors["seg.stats"] = TensorRef{w.stats_off, 4, 1};  // rows 0 .. C - 1: {mean removed, gain, mix_rms, 0} of the input rows
  return launched(h, launch_seg_stats(mix, w.part, w.stats, rows, C, level, h->norm, st), "segment stats") &&
         launched(h, launch_seg_mel_energy(mix, w.stats, h->W + m.mel.win_off, h->W + m.mel.tw_off, h->W + m.mel.fb_off, esum, rows,
                                           C, m.mel.n_fft, m.mel.hop, m.mel.pad_left, m.mel.n_freq, m.mel.n_mels, frames_max, st),
                  "segment mel energy");
}
// One step's noise of a group's n_rows walk rows of T columns, in w.zbuf: `gather(slice)` enqueues the gather from one step's
// slice of the caller's tensor (step_noise words), or -- counter mode -- the same positions come straight from the function, no
// whole-row noise exists then: `entry(row, stream_row, t0, len)` names the long row whose stream walk row `row` reads, the first
// position and the length (0 behind it, so x needs no mask).
template <class Gather, class EntryFn>
auto seg_noise(ou_handle* h, Runner& r, const float* noise, size_t step_noise, float* zbuf, int T, int n_rows, Gather gather,
               EntryFn entry) {
  return [=, &r](int draw) -> const float* {
    if (noise) {
      gather(noise + (size_t)draw * step_noise);
      return zbuf;
    }
    fill_noise_plane(r, zbuf, T, n_rows, h->noise_src.seed, draw, [&](int row, unsigned long long& sid, long long& t0, long long& len) {
      long long stream_row = 0;
      entry(row, stream_row, t0, len);
      sid = h->noise_src.streams[(size_t)stream_row];
    });
    return zbuf;
  };
}
// every member's last real window of the group -> `carry` (E, T): the window in front of the next group
void seg_carry(Runner& r, float* carry, const float* x, int T, int Bw, int E, int n_real) {
  for (int e = 0; e < E; e++)
    r.launch("carry", [&] {
      return hipMemcpyAsync(carry + (size_t)e * T, x + ((size_t)e * Bw + n_real - 1) * T, (size_t)T * 4, hipMemcpyDeviceToDevice, r.st);
    });
}
// after the last group: what the operator seams see, and the post step over the E * C long rows
template <class Rows>
int seg_epilogue(ou_handle* h, float* long_rows, const SegWs& w, const Rows& rows, int E, int C, int L, uint32_t flags,
                 hipStream_t st) {
  h->cond_B = 0;  // (the operator seams see a whole-file batch only)
  h->cond_T = L;
  const PostFlags pf(flags);
  if (!launched(h, launch_seg_post(long_rows, w.part, w.stats, rows, E, C, pf.keep_rms, pf.peak, st), "segment post")) return OU_EHIP;
  return OU_OK;
}

// ou_enhance_segments (E = 1, members = out, no reduce) and ou_enhance_segments_ensemble behind their own refusals: the windows
// in groups of Bw entries, every group one walk of E * Bw rows (member-major) whose conditioner runs once over the Bw inputs
// (ensemble_impl's arrangement) or -- not shared, E = 1 -- over all rows; the members are stitched into the (E * C, T_raw) rows
// `members`, post-processed there and, `reduce`, reduced into `out`.
int seg_enhance(ou_handle* h, const char* who, const char* sizer, const float* mix, float* out, float* members, const float* noise,
                int C, int E, bool reduce, int stat, SegGeom g, int Bw, int n_steps, double epsilon, const float* sigma_host,
                uint32_t flags, void* ws, size_t ws_bytes, ou_stream_t stream) {
  if (g.L > max_walk_length(h, false)) return fail(h, OU_EINVAL, std::string(who) + ": segment too long for one pass of the walk");
  const int B = E * Bw;  // rows of the walk
  const int L = (int)g.L;
  SegWs w;
  if (const int rc = seg_workspace(h, ws, ws_bytes, B, L, seg_area(C, E, Bw, g.L, reduce, false), sizer, w)) return rc;

  CallScope scope(h, true);  // one chain on the caller's stream
  hipStream_t st = (hipStream_t)stream;
  const Model& m = h->m;
  const bool share = h->opt.ens_share != 0 && E > 1;
  const int Bc = share ? Bw : B;  // rows of the conditioner pass

  // ---- whole-row statistics and mel scale of the C inputs
  const long long Lf = g.T_pad / m.tot_ds;  // mel frames of the whole row (run_condition)
  if (Lf > g.T_raw) return fail(h, OU_EINVAL, "internal: mel frames do not fit into the output row");
  if (Lf > 0x7fffffffll) return fail(h, OU_EINVAL, "input too long");
  const SegRowsAlike rows{SegRow{g.T_raw, g.T_pad, g.pad_left, g.n_win, 0, Lf}};
  if (!seg_row_stats(h, mix, out, w, rows, C, Lf, st)) return OU_EHIP;
  if (!launched(h, launch_mel_scale(out, w.row_scale, C, (int)Lf, st), "segment mel scale")) return OU_EHIP;

  // ---- the groups: Bw entries at a time, E * Bw rows through the walk
  const SamplerTables tab(m.cfg, n_steps, epsilon, sigma_host);
  for (long long e0 = 0; e0 < g.n_entries; e0 += Bw) {
    const int n_real = (int)std::min<long long>(Bw, g.n_entries - e0);
    const SegEntriesArith ents{e0, g.n_entries, g.n_win, g.L, g.hop, g.overlap};
    Runner r(h, ws, w.walk, false, st, B);
    r.mel_scale_preset = true;
    Persist P = layout_persist(r, L);
    if (r.oom) return finish(h, r);
    if (e0 == 0) tab.upload(r, P);  // (the persistent area of the workspace keeps the tables from group to group)
    Runner rc = Runner::conditioner_of(r, Bc);
    // the group's inputs: once into the prefix, or -- the conditioner over all rows -- once per member
    for (int e = 0; e < (share ? 1 : E); e++)
      rc.launch("segment gather", [&] {
        return launch_seg_gather_input(mix, w.stats, w.row_scale, P.mixn.p + (size_t)e * Bw * L, P.mel_scale + (size_t)e * Bw, rows,
                                       ents, Bw, L, st);
      });
    run_condition(rc, P, P.mixn.p, L);
    // (the statistics of the post step are those of the whole long rows, w.stats: P.stats is not written; no warm start)
    if (share) replicate_conditioned(rc, P, Bw, E, false, false);
    if (const int rc2 = finish(h, rc)) return rc2;
    r.off = rc.off;
    // walk row e * Bw + j: window k of long row e * C + c, positions s_k + i of that row's noise.  The filler rows of a short
    // last group repeat their member's last real entry.
    auto z = seg_noise(h, r, noise, (size_t)E * C * g.T_pad, w.zbuf, L, B,
                       [&](const float* slice) {
                         r.launch("segment noise", [&] { return launch_seg_gather_noise(slice, w.zbuf, rows, ents, Bw, L, Bw, E, C, st); });
                       },
                       [&](int row, long long& stream_row, long long& t0, long long& len) {
                         const int e = row / Bw;
                         const SegEnt en = ents.entry(row - e * Bw);
                         stream_row = (long long)e * C + en.row;
                         t0 = seg_start_host(g, en.win);
                         len = L;
                       });
    sample(r, P, L, tab, 0, nullptr, false, z);
    r.launch("segment stitch", [&] { return launch_seg_stitch(P.x.p, w.carry, members, rows, ents, n_real, L, Bw, E, C, st); });
    if (e0 + Bw < g.n_entries) seg_carry(r, w.carry, P.x.p, L, Bw, E, n_real);
    if (const int rc2 = finish(h, r)) return rc2;
  }
  // ---- the post step over every long row (keep_rms: the mix_rms of the member's own input row), then the reduce over e
  if (const int rc = seg_epilogue(h, members, w, rows, E, C, L, flags, st)) return rc;
  if (reduce && !launched(h, launch_ensemble_reduce(members, out, E, C, g.T_raw, g.T_raw, nullptr, stat, w.hist,
                                                    w.hist + (size_t)C * E, st), "ensemble reduce"))
    return OU_EHIP;
  return OU_OK;
}

// ou_enhance_segments_var (E = 1, members = out, no reduce) and ou_enhance_segments_var_ensemble behind their own refusals: rows
// with lengths of their own, their windows in the groups `G` of Bw = G.batch entries (seg_groups at max_batch / E), every group
// one walk of E * Bw rows (member-major) -- the plain one, or the ragged one where the entries differ in length -- whose
// conditioner runs once over the Bw entries (seg_enhance's arrangement) or -- not shared, E = 1 -- over all rows; the members are
// stitched into the (E * C, T_raw_max) rows `members`, post-processed there and, `reduce`, reduced into `out` at the rows' lengths.
int seg_var_enhance(ou_handle* h, const char* who, const char* sizer, const float* mix, float* out, float* members,
                    const float* noise, int C, long long T_raw_max, const int64_t* t_raw, int E, bool reduce, int stat,
                    const SegGroups& G, int n_steps, double epsilon, const float* sigma_host, uint32_t flags, void* ws,
                    size_t ws_bytes, ou_stream_t stream) {
  const Model& m = h->m;
  const int tot = m.tot_ds;
  if (G.length > max_walk_length(h, false)) return fail(h, OU_EINVAL, std::string(who) + ": segment too long for one pass of the walk");
  const int Bw = G.batch;  // entries per group
  const int B = E * Bw;    // rows of the walk
  SegWs w;
  if (const int rc = seg_workspace(h, ws, ws_bytes, B, (int)G.length, seg_area(C, E, Bw, G.length, reduce, true), sizer, w)) return rc;

  CallScope scope(h, true);  // one chain on the caller's stream
  hipStream_t st = (hipStream_t)stream;
  const bool share = h->opt.ens_share != 0 && E > 1;
  const int Bc = share ? Bw : B;  // rows of the conditioner pass

  // ---- the geometry table, then every row's statistics and mel scale in one set of launches (the output rows hold the frame
  // energies until the first stitch -- with members of their own: until the reduce)
  long long T_pad_max = 0, frames_max = 0;
  for (int c = 0; c < C; c++) {
    T_pad_max = std::max(T_pad_max, G.rows[c].T_pad);
    const long long Lf = G.rows[c].T_pad / tot;  // mel frames of the whole row (run_condition)
    if (Lf > G.rows[c].T_raw) return fail(h, OU_EINVAL, "internal: mel frames do not fit into the output row");
    frames_max = std::max(frames_max, Lf);
  }
  if (frames_max > 0x7fffffffll) return fail(h, OU_EINVAL, "input too long");
  const SegVar v{G.S, G.hop, tot};
  for (int off = 0; off < C; off += kSegRowsPerLaunch) {
    SegRowBlock blk;
    const int n = std::min(C - off, kSegRowsPerLaunch);
    for (int i = 0; i < kSegRowsPerLaunch; i++) {
      blk.t_raw[i] = i < n ? t_raw[off + i] : 1;
      blk.first[i] = i < n ? G.first[off + i] : 0;
    }
    if (!launched(h, launch_seg_upload_rows(w.geom, blk, n, off, v, st), "segment rows")) return OU_EHIP;
  }
  const SegRowsTable rows{w.geom, T_raw_max, T_pad_max};
  if (!seg_row_stats(h, mix, out, w, rows, C, frames_max, st)) return OU_EHIP;
  if (!launched(h, launch_seg_mel_scale_var(out, w.row_scale, w.geom, C, T_raw_max, st), "segment mel scale")) return OU_EHIP;

  // ---- the groups: Bw entries at a time, E * Bw rows through the walk
  const SamplerTables tab(m.cfg, n_steps, epsilon, sigma_host);
  const long long n_entries = (long long)G.entries.size();
  for (size_t gi = 0; gi < G.group_first.size(); gi++) {
    const long long e0 = G.group_first[gi];
    const bool full = e0 < G.n_full;
    const long long e_end = std::min<long long>(e0 + Bw, full ? G.n_full : n_entries);
    const int n_real = (int)(e_end - e0);
    // entry j of the group (the filler rows of a short last group repeat the last real one) and the length of the walk
    auto entry = [&](int j) -> const SegEntry& { return G.entries[(size_t)(e0 + std::min(j, n_real - 1))]; };
    int T = 0;
    for (int j = 0; j < n_real; j++) T = std::max(T, entry(j).len);
    // fn(entries, n) for the entries [0, count) of the group, kSegEntriesPerLaunch at a time
    auto for_blocks = [&](int count, auto fn) {
      for (int j0 = 0; j0 < count; j0 += kSegEntriesPerLaunch) {
        SegEntriesList ents;
        ents.j0 = j0; ents.hop = G.hop; ents.overlap = G.O;
        const int n = std::min(count - j0, kSegEntriesPerLaunch);
        for (int i = 0; i < kSegEntriesPerLaunch; i++) {
          const SegEntry& e = entry(j0 + std::min(i, n - 1));
          ents.blk.row[i] = e.row; ents.blk.win[i] = e.win; ents.blk.len[i] = e.len;
        }
        fn(ents, n);
      }
    };
    Runner r(h, ws, w.walk, false, st, B);
    r.mel_scale_preset = true;
    Persist P = layout_persist(r, T);
    if (r.oom) return finish(h, r);
    if (gi == 0) tab.upload(r, P);  // (the persistent area keeps the tables from group to group: its layout depends on B alone)
    const bool ragged = G.group_ragged[gi] != 0;
    if (ragged) {
      // the entries' lengths on every level of the network (as ou_enhance_var; an entry is an already padded window, so its
      // length is the level-0 length itself): every member's rows in one set of launches, and the [level][Bw] table of a
      // conditioner pass over the entries alone
      if (const int rc = set_levels(r, T)) return rc;
      for_blocks(Bw, [&](const SegEntriesList& ents, int n) {
        r.launch("segment lens", [&] { return launch_seg_upload_lens(P.lens, ents.blk, n, ents.j0, Bw, E, r.lv, st); });
        if (share) r.launch("segment lens", [&] { return launch_seg_upload_lens(w.lens_b, ents.blk, n, ents.j0, Bw, 1, r.lv, st); });
      });
      r.set_ragged(P.lens, nullptr);  // (no RowInfo: the windows are gathered and stitched by their entries)
    }
    Runner rc = Runner::conditioner_of(r, Bc);
    if (ragged) rc.set_ragged(share ? w.lens_b : P.lens, nullptr);
    // the group's inputs: once into the prefix, or -- the conditioner over all rows -- once per member
    for (int e = 0; e < (share ? 1 : E); e++)
      for_blocks(Bw, [&](const SegEntriesList& ents, int n) {
        rc.launch("segment gather", [&] {
          return launch_seg_gather_input(mix, w.stats, w.row_scale, P.mixn.p + (size_t)e * Bw * T, P.mel_scale + (size_t)e * Bw, rows,
                                         ents, n, T, st);
        });
      });
    run_condition(rc, P, P.mixn.p, T);
    // (the statistics of the post step are those of the whole long rows, w.stats: P.stats is not written; no warm start)
    if (share) replicate_conditioned(rc, P, Bw, E, false, false);
    if (const int rc2 = finish(h, rc)) return rc2;
    r.off = rc.off;
    // walk row e * Bw + j: window k of long row e * C + c, positions s_k + i of that row's noise
    auto z = seg_noise(h, r, noise, (size_t)E * C * T_pad_max, w.zbuf, T, B,
                       [&](const float* slice) {
                         for_blocks(Bw, [&](const SegEntriesList& ents, int n) {
                           r.launch("segment noise", [&] { return launch_seg_gather_noise(slice, w.zbuf, rows, ents, n, T, Bw, E, C, st); });
                         });
                       },
                       [&](int row, long long& stream_row, long long& t0, long long& len) {
                         const int e = row / Bw;
                         const SegEntry& en = entry(row - e * Bw);
                         stream_row = (long long)e * C + en.row;
                         t0 = en.win < G.rows[en.row].n_win - 1 ? en.win * G.hop : G.rows[en.row].T_pad - en.len;
                         len = en.len;
                       });
    sample(r, P, T, tab, 0, nullptr, false, z);
    for_blocks(n_real, [&](const SegEntriesList& ents, int n) {
      r.launch("segment stitch", [&] { return launch_seg_stitch(P.x.p, w.carry, members, rows, ents, n, T, Bw, E, C, st); });
    });
    if (full && e_end < G.n_full) seg_carry(r, w.carry, P.x.p, T, Bw, E, n_real);  // the window in front of the next group
    if (const int rc2 = finish(h, r)) return rc2;
  }
  // ---- the post step over every long row (keep_rms: the mix_rms of the member's own input row), then the reduce over e
  if (const int rc = seg_epilogue(h, members, w, rows, E, C, (int)G.length, flags, st)) return rc;
  if (reduce) {
    const std::vector<long long> len64(t_raw, t_raw + C);
    if (!launched(h, launch_ensemble_reduce(members, out, E, C, T_raw_max, T_raw_max, len64.data(), stat, w.hist,
                                            w.hist + (size_t)C * E, st), "ensemble reduce"))
      return OU_EHIP;
  }
  return OU_OK;
}
}  // namespace

extern "C" {

int ou_segment_plan(int32_t tot_ds, int64_t T_raw, int32_t segment, int32_t overlap, int32_t capacity, int64_t* starts,
                    int32_t* lengths, int64_t* core_begin, int64_t* core_end, int32_t* n_windows, int32_t* overlap_used,
                    int64_t* T_pad) {
  SegPlan p;
  if (!seg_plan(tot_ds, T_raw, segment, overlap, p)) return fail(nullptr, OU_EINVAL, p.err);
  const SegGeom& g = p.g;
  if (g.n_win > 0x7fffffffll) return fail(nullptr, OU_EINVAL, "segment plan: too many windows");
  if (n_windows) *n_windows = (int32_t)g.n_win;
  if (overlap_used) *overlap_used = (int32_t)g.overlap;
  if (T_pad) *T_pad = g.T_pad;
  if (!starts && !lengths && !core_begin && !core_end) return OU_OK;
  if (capacity < g.n_win) return fail(nullptr, OU_EINVAL, "segment plan: capacity smaller than the number of windows");
  // core k = [m_{k-1}, m_k): m_k = the middle of the crossfade between windows k and k + 1, [e_k - O, e_k)
  for (long long k = 0; k < g.n_win; k++) {
    const long long s = seg_start_host(g, k);
    if (starts) starts[k] = s;
    if (lengths) lengths[k] = (int32_t)g.L;
    const long long m0 = k == 0 ? 0 : seg_start_host(g, k - 1) + g.L - g.overlap + g.overlap / 2;
    const long long m1 = k == g.n_win - 1 ? g.T_pad : s + g.L - g.overlap + g.overlap / 2;
    if (core_begin) core_begin[k] = m0;
    if (core_end) core_end[k] = m1;
  }
  return OU_OK;
}

int ou_segments_workspace_bytes(const ou_handle* hc, int32_t C, int64_t T_raw, int32_t segment, int32_t overlap,
                                int32_t max_batch, size_t* nbytes, int32_t* batch, int32_t* length) {
  ou_handle* h = const_cast<ou_handle*>(hc);
  if (!h || !nbytes || C < 1 || max_batch < 1) return fail(h, OU_EINVAL, "bad argument");
  SegPlan p;
  if (!seg_plan(h->m.tot_ds, T_raw, segment, overlap, p)) return fail(h, OU_EINVAL, p.err);
  if (p.g.L > 0x7fffffffll) return fail(h, OU_EINVAL, "segment too long");
  const int B = seg_batch((long long)C * p.g.n_win, max_batch);
  return seg_workspace_bytes(h, B, p.g.L, seg_area(C, 1, B, p.g.L, false, false), nbytes, batch, length);
}

int ou_enhance_segments(ou_handle* h, const float* mix, float* out, const float* noise, int32_t C, int64_t T_raw,
                        int32_t segment, int32_t overlap, int32_t max_batch, int32_t n_steps, double epsilon,
                        const float* sigma_host, int32_t warm_start, uint32_t flags, void* ws, size_t ws_bytes,
                        ou_stream_t stream) {
  if (!h || !mix || !out || !ws || C < 1 || T_raw < 1 || max_batch < 1) return fail(h, OU_EINVAL, "bad argument");
  if (const int rc = check_noise_source(h, noise, C, "the rows of the call (", true)) return rc;
  if (warm_start >= 0 || (flags & OU_ENH_USE_AUX_SIGNAL))
    return fail(h, OU_EINVAL, "ou_enhance_segments: warm_start and use_aux_signal are not supported");
  if (const int rc = check_steps(h, n_steps, warm_start)) return rc;
  SegPlan plan;
  if (!seg_plan(h->m.tot_ds, T_raw, segment, overlap, plan)) return fail(h, OU_EINVAL, plan.err);
  SegGeom g = plan.g;
  g.n_entries = (long long)C * g.n_win;
  return seg_enhance(h, "ou_enhance_segments", "ou_segments_workspace_bytes", mix, out, out, noise, C, 1, false, 0, g,
                     seg_batch(g.n_entries, max_batch), n_steps, epsilon, sigma_host, flags, ws, ws_bytes, stream);
}

int ou_segments_ensemble_workspace_bytes(const ou_handle* hc, int32_t C, int64_t T_raw, int32_t segment, int32_t overlap,
                                         int32_t max_batch, int32_t E, size_t* nbytes, int32_t* batch, int32_t* length) {
  ou_handle* h = const_cast<ou_handle*>(hc);
  if (!h || !nbytes) return fail(h, OU_EINVAL, "bad argument");
  SegGeom g;
  int Bw = 0;
  if (const int rc = seg_ens_plan(h, "ou_segments_ensemble_workspace_bytes", C, T_raw, segment, overlap, max_batch, E, g, Bw))
    return rc;
  return seg_workspace_bytes(h, E * Bw, g.L, seg_area(C, E, Bw, g.L, true, false), nbytes, batch, length);
}

int ou_enhance_segments_ensemble(ou_handle* h, const float* mix, float* out, float* members, const float* noise, int32_t C,
                                 int64_t T_raw, int32_t E, int32_t stat, int32_t segment, int32_t overlap, int32_t max_batch,
                                 int32_t n_steps, double epsilon, const float* sigma_host, int32_t warm_start, uint32_t flags,
                                 void* ws, size_t ws_bytes, ou_stream_t stream) {
  const char* who = "ou_enhance_segments_ensemble";
  if (!h || !mix || !out || !ws) return fail(h, OU_EINVAL, "bad argument");
  SegGeom g;
  int Bw = 0;
  if (const int rc = seg_ens_plan(h, who, C, T_raw, segment, overlap, max_batch, E, g, Bw)) return rc;
  if (stat != OU_ENS_MEAN && stat != OU_ENS_MEDIAN && stat != OU_ENS_SIGNAL_MEDIAN)
    return fail(h, OU_EINVAL, std::string(who) + ": stat must be OU_ENS_MEAN, OU_ENS_MEDIAN or OU_ENS_SIGNAL_MEDIAN");
  if (!members)
    return fail(h, OU_EINVAL, std::string(who) + ": `members` must be given ((E * C, T_raw): the post step runs over whole member rows)");
  if (warm_start >= 0 || (flags & OU_ENH_USE_AUX_SIGNAL))
    return fail(h, OU_EINVAL, std::string(who) + ": warm_start and use_aux_signal are not supported");
  if (const int rc = check_noise_source(h, noise, E * C, "the member rows of the call (E * C = ", true)) return rc;
  if (const int rc = check_steps(h, n_steps, warm_start)) return rc;
  return seg_enhance(h, who, "ou_segments_ensemble_workspace_bytes", mix, out, members, noise, C, E, true, stat, g, Bw, n_steps,
                     epsilon, sigma_host, flags, ws, ws_bytes, stream);
}

int ou_segment_groups(int32_t tot_ds, int32_t C, const int64_t* t_raw, int32_t segment, int32_t overlap, int32_t max_batch,
                      int32_t capacity, int32_t* entry_row, int32_t* entry_window, int32_t* entry_length, int32_t* group_first,
                      int32_t* group_ragged, int32_t* n_entries, int32_t* n_groups, int32_t* batch, int32_t* length) {
  SegGroups G;
  if (!seg_groups(tot_ds, C, t_raw, segment, overlap, max_batch, G)) return fail(nullptr, OU_EINVAL, G.err);
  const int ne = (int)G.entries.size(), ng = (int)G.group_first.size();
  if (n_entries) *n_entries = ne;
  if (n_groups) *n_groups = ng;
  if (batch) *batch = G.batch;
  if (length) *length = (int32_t)G.length;
  if (!entry_row && !entry_window && !entry_length && !group_first && !group_ragged) return OU_OK;
  if (capacity < ne) return fail(nullptr, OU_EINVAL, "segment groups: capacity smaller than the number of entries");
  for (int e = 0; e < ne; e++) {
    if (entry_row) entry_row[e] = G.entries[e].row;
    if (entry_window) entry_window[e] = G.entries[e].win;
    if (entry_length) entry_length[e] = G.entries[e].len;
  }
  for (int g = 0; g < ng; g++) {
    if (group_first) group_first[g] = G.group_first[g];
    if (group_ragged) group_ragged[g] = G.group_ragged[g];
  }
  return OU_OK;
}

int ou_segments_var_workspace_bytes(const ou_handle* hc, int32_t C, const int64_t* t_raw, int32_t segment, int32_t overlap,
                                    int32_t max_batch, size_t* nbytes, int32_t* batch, int32_t* length) {
  ou_handle* h = const_cast<ou_handle*>(hc);
  if (!h || !nbytes || !t_raw || C < 1 || max_batch < 1) return fail(h, OU_EINVAL, "bad argument");
  SegGroups G;
  if (!seg_groups(h->m.tot_ds, C, t_raw, segment, overlap, max_batch, G)) return fail(h, OU_EINVAL, G.err);
  return seg_workspace_bytes(h, G.batch, G.length, seg_area(C, 1, G.batch, G.length, false, true), nbytes, batch, length);
}

int ou_enhance_segments_var(ou_handle* h, const float* mix, float* out, const float* noise, int32_t C, int64_t T_raw_max,
                            const int64_t* t_raw, int32_t segment, int32_t overlap, int32_t max_batch, int32_t n_steps,
                            double epsilon, const float* sigma_host, int32_t warm_start, uint32_t flags, void* ws,
                            size_t ws_bytes, ou_stream_t stream) {
  // (the lengths first: what they decide needs neither the handle nor a device)
  if (!t_raw || C < 1 || C > 65535 || T_raw_max < 1) return fail(h, OU_EINVAL, "bad argument");
  if (max_batch < 1) return fail(h, OU_EINVAL, "ou_enhance_segments_var: max_batch must be at least 1");
  if (const int rc = check_rows(h, "ou_enhance_segments_var", 'c', t_raw, C, T_raw_max, false)) return rc;
  if (!h || !mix || !out || !ws) return fail(h, OU_EINVAL, "bad argument");
  if (const int rc = check_noise_source(h, noise, C, "the rows of the call (", true)) return rc;
  if (warm_start >= 0 || (flags & OU_ENH_USE_AUX_SIGNAL))
    return fail(h, OU_EINVAL, "ou_enhance_segments_var: warm_start and use_aux_signal are not supported");
  if (const int rc = check_steps(h, n_steps, warm_start)) return rc;
  SegGroups G;
  if (!seg_groups(h->m.tot_ds, C, t_raw, segment, overlap, max_batch, G)) return fail(h, OU_EINVAL, G.err);
  return seg_var_enhance(h, "ou_enhance_segments_var", "ou_segments_var_workspace_bytes", mix, out, out, noise, C, T_raw_max, t_raw,
                         1, false, 0, G, n_steps, epsilon, sigma_host, flags, ws, ws_bytes, stream);
}

int ou_segments_var_ensemble_workspace_bytes(const ou_handle* hc, int32_t C, const int64_t* t_raw, int32_t segment,
                                             int32_t overlap, int32_t max_batch, int32_t E, size_t* nbytes, int32_t* batch,
                                             int32_t* length) {
  ou_handle* h = const_cast<ou_handle*>(hc);
  if (!h || !nbytes || !t_raw || C < 1 || max_batch < 1) return fail(h, OU_EINVAL, "bad argument");
  if (const int rc = seg_ens_members(h, "ou_segments_var_ensemble_workspace_bytes", C, max_batch, E)) return rc;
  SegGroups G;
  if (!seg_groups(h->m.tot_ds, C, t_raw, segment, overlap, max_batch / E, G)) return fail(h, OU_EINVAL, G.err);
  return seg_workspace_bytes(h, E * G.batch, G.length, seg_area(C, E, G.batch, G.length, true, true), nbytes, batch, length);
}

int ou_enhance_segments_var_ensemble(ou_handle* h, const float* mix, float* out, float* members, const float* noise, int32_t C,
                                     int64_t T_raw_max, const int64_t* t_raw, int32_t E, int32_t stat, int32_t segment,
                                     int32_t overlap, int32_t max_batch, int32_t n_steps, double epsilon, const float* sigma_host,
                                     int32_t warm_start, uint32_t flags, void* ws, size_t ws_bytes, ou_stream_t stream) {
  const char* who = "ou_enhance_segments_var_ensemble";
  // (the lengths and the member count first: what they decide needs neither the handle nor a device)
  if (!t_raw || C < 1 || T_raw_max < 1) return fail(h, OU_EINVAL, std::string(who) + ": bad argument (t_raw must be given, C >= 1)");
  if (max_batch < 1) return fail(h, OU_EINVAL, std::string(who) + ": max_batch must be at least 1");
  if (const int rc = seg_ens_members(h, who, C, max_batch, E)) return rc;
  if (const int rc = check_rows(h, who, 'c', t_raw, C, T_raw_max, false)) return rc;
  if (!h || !mix || !out || !ws) return fail(h, OU_EINVAL, "bad argument");
  if (stat != OU_ENS_MEAN && stat != OU_ENS_MEDIAN && stat != OU_ENS_SIGNAL_MEDIAN)
    return fail(h, OU_EINVAL, std::string(who) + ": stat must be OU_ENS_MEAN, OU_ENS_MEDIAN or OU_ENS_SIGNAL_MEDIAN");
  if (!members)
    return fail(h, OU_EINVAL, std::string(who) + ": `members` must be given ((E * C, T_raw_max): the post step runs over whole member rows)");
  if (warm_start >= 0 || (flags & OU_ENH_USE_AUX_SIGNAL))
    return fail(h, OU_EINVAL, std::string(who) + ": warm_start and use_aux_signal are not supported");
  if (const int rc = check_noise_source(h, noise, E * C, "the member rows of the call (E * C = ", true)) return rc;
  if (const int rc = check_steps(h, n_steps, warm_start)) return rc;
  SegGroups G;
  if (!seg_groups(h->m.tot_ds, C, t_raw, segment, overlap, max_batch / E, G)) return fail(h, OU_EINVAL, G.err);
  return seg_var_enhance(h, who, "ou_segments_var_ensemble_workspace_bytes", mix, out, members, noise, C, T_raw_max, t_raw, E, true,
                         stat, G, n_steps, epsilon, sigma_host, flags, ws, ws_bytes, stream);
}

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

int ou_check_device_status(ou_handle* h, void* ws) {
  if (!h || !ws) return fail(h, OU_EINVAL, "bad argument");
  unsigned hdr[40];
  hipError_t e = hipMemcpy(hdr, ws, sizeof(hdr), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(h, OU_EHIP, hipGetErrorString(e));
  const unsigned v = hdr[0];
  // word 20: waits the GRU clusters' safety net cut short by repeating a publish (a member that was merely late counts
  // too); word 33: those among them where the awaited granule was visible to a system-scope load / an atomic but NOT to the
  // agent-scope load of the gather.  The first time word 33 moves, the cheap publish form has shown that it cannot be
  // relied upon on this device / in this process mix: agent-scope publishes from now on (+0.1 ms per GRU pass, no more
  // 0.1 ms recoveries).  Results are unaffected either way.
  if (hdr[33] != 0u && !h->gru_agent_stores) h->gru_agent_stores = 1;
  if (v) {
    (void)hipMemset(ws, 0, sizeof(v));  // sticky until read
    return fail(h, OU_ESYNC, "device-side timeout in the GRU cluster exchange (status word " + std::to_string(v) + ")");
  }
  return OU_OK;
}

int ou_workspace_init(ou_handle* h, int32_t B, int32_t T, void* ws, size_t ws_bytes, ou_stream_t stream) {
  if (!h || !ws || B < 1 || T < 1) return fail(h, OU_EINVAL, "bad argument");
  if (T % h->m.tot_ds) return fail(h, OU_EINVAL, "T must be a multiple of the total down-sampling factor");
  auto keep = h->tensors;
  Runner r(h, ws, ws_bytes, false, (hipStream_t)stream, B);
  Persist P = layout_persist(r, T);
  h->tensors = keep;
  if (r.oom) return finish(h, r);
  // header: status word, coefficient rows, statistics, both GRU exchange areas (everything in front of mel_scale)
  const size_t hdr = (size_t)((char*)P.mel_scale - (char*)ws);
  r.launch("workspace init", [&] { return hipMemsetAsync(ws, 0, hdr, r.st); });
  const int rc = finish(h, r);
  if (rc == OU_OK) {
    // remember (pointer, size, shape); a buffer that comes back at the same address is re-registered by its own init
    auto& v = h->ws_ready;
    for (size_t i = 0; i < v.size(); i++)
      if (v[i].ws == ws) { v.erase(v.begin() + i); break; }
    if (v.size() >= 64) v.erase(v.begin());
    v.push_back(ou_handle::WsRec{ws, ws_bytes, B, T});
  }
  return rc;
}

int ou_set_lanes(ou_handle* h, int32_t lanes, int32_t lane) {
  if (!h || lanes < 1 || lanes > 8 || lane < 0 || lane >= lanes) return fail(h, OU_EINVAL, "ou_set_lanes: 1 <= lanes <= 8, 0 <= lane < lanes");
  h->lanes = lanes;
  h->lane = lane;
  return OU_OK;
}

int ou_lane_capacity(const ou_handle* h, int32_t max_batch) {
  if (!h || max_batch < 1) return 0;
  // the largest number of lanes whose GRU launches -- every lane at `max_batch` -- can all be resident at the same time
  const Model& m = h->m;
  for (int lanes = 8; lanes >= 1; lanes--) {
    const int share = Runner::gru_share_of(lanes, max_batch, false);
    bool ok = true;
    for (int H : {m.s_gru.H, m.c_gru0.H, m.c_gru1.H})
      if (H > 0 && gru_ring_batch_cap(H, h->num_cu, share, 0, max_batch, lanes) < 1) ok = false;
    if (ok) return lanes;
  }
  return 1;
}

int ou_set_lane_batch(ou_handle* h, int32_t max_batch) {
  if (!h || max_batch < 0) return fail(h, OU_EINVAL, "ou_set_lane_batch: max_batch >= 0");
  h->lane_max_b = max_batch;
  return OU_OK;
}

int ou_get_gru_publish_mode(const ou_handle* h) { return h ? h->gru_agent_stores : 0; }

int ou_set_gru_publish_mode(ou_handle* h, int32_t agent_scope) {
  if (!h) return fail(h, OU_EINVAL, "bad argument");
  h->gru_agent_stores = agent_scope ? 1 : 0;
  return OU_OK;
}

int ou_set_noise_source(ou_handle* h, const ou_noise_spec* spec) {
  if (!h) return fail(h, OU_EINVAL, "bad argument");
  if (!spec) {
    h->noise_src = ou_handle::NoiseSource();
    return OU_OK;
  }
  if (!spec->streams || spec->n_streams < 1) return fail(h, OU_EINVAL, "ou_set_noise_source: one stream id per row must be given");
  if ((spec->scratch == nullptr) != (spec->scratch_bytes == 0))
    return fail(h, OU_EINVAL, "ou_set_noise_source: scratch and scratch_bytes must be given together");
  if (reinterpret_cast<uintptr_t>(spec->scratch) % 16 != 0)
    return fail(h, OU_EINVAL, "ou_set_noise_source: scratch must be 16-byte aligned");
  h->noise_src.on = true;
  h->noise_src.seed = spec->seed;
  h->noise_src.streams.assign(spec->streams, spec->streams + spec->n_streams);
  h->noise_src.scratch = (float*)spec->scratch;
  h->noise_src.scratch_bytes = spec->scratch_bytes;
  return OU_OK;
}

int ou_noise_scratch_bytes(const ou_handle* h, int32_t B, int32_t T_pad, size_t* nbytes) {
  if (!h || !nbytes || B < 1 || T_pad < 1) return fail(const_cast<ou_handle*>(h), OU_EINVAL, "bad argument");
  *nbytes = (size_t)2 * B * T_pad * sizeof(float);  // two planes, ping-pong
  return OU_OK;
}

int ou_noise_fill(float* out, int64_t row_stride, int64_t cols, int32_t rows, const uint64_t* streams_host,
                  const int64_t* t0_host, const int64_t* len_host, uint64_t seed, int32_t draw, ou_stream_t stream) {
  if (!out || !streams_host || !t0_host || !len_host || rows < 1 || cols < 1 || row_stride < cols)
    return fail(nullptr, OU_EINVAL, "ou_noise_fill: bad argument");
  if (draw < 0 || draw >= (1 << 16)) return fail(nullptr, OU_EINVAL, "ou_noise_fill: 0 <= draw < 2^16");
  for (int j = 0; j < rows; j++)
    if (len_host[j] < 0 || len_host[j] > cols || t0_host[j] < 0 || t0_host[j] > (1ll << 50) - len_host[j])
      return fail(nullptr, OU_EINVAL, "ou_noise_fill: 0 <= len[j] <= cols, t0[j] >= 0, t0[j] + len[j] <= 2^50");
  for (int off = 0; off < rows; off += kNoiseRowsPerLaunch) {
    NoiseRows blk;
    const int n = rows - off < kNoiseRowsPerLaunch ? rows - off : kNoiseRowsPerLaunch;
    for (int i = 0; i < kNoiseRowsPerLaunch; i++) {
      blk.stream[i] = i < n ? streams_host[off + i] : 0;
      blk.t0[i] = i < n ? t0_host[off + i] : 0;
      blk.len[i] = i < n ? len_host[off + i] : 0;
    }
    const hipError_t e = launch_noise_fill(out + (size_t)off * (size_t)row_stride, row_stride, cols, blk, n, seed, draw,
                                           (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, OU_EHIP, std::string("HIP error at noise fill: ") + hipGetErrorString(e));
  }
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

int ou_sampler_step(ou_handle* h, float* x, const float* score, const float* z, float c1, float c2, size_t n,
                    ou_stream_t stream) {
  if (!h || !x || !score) return fail(h, OU_EINVAL, "bad argument");
  hipError_t e = launch_sampler_step(x, score, z, c1, c2, n, (hipStream_t)stream);
  if (e != hipSuccess) return fail(h, OU_EHIP, hipGetErrorString(e));
  return OU_OK;
}

int ou_tensor(const ou_handle* h, const char* name, size_t* byte_offset, int32_t* C, int32_t* T) {
  if (!h || !name) return OU_EINVAL;
  auto it = h->tensors.find(name);
  if (it == h->tensors.end()) return OU_EMISSING;
  if (byte_offset) *byte_offset = it->second.off;
  if (C) *C = it->second.C;
  if (T) *T = it->second.T;
  return OU_OK;
}

int ou_launch_stats(const ou_handle* h, int32_t* n_launches, int32_t* n_conv_launches) {
  if (!h) return OU_EINVAL;
  if (n_launches) *n_launches = h->n_launch;
  if (n_conv_launches) *n_conv_launches = h->n_conv;
  return OU_OK;
}

// Micro-benchmark of ONE packed conv layer (measurement / tuning only): runs it `iters` times on random-ish data in
// the caller's workspace with HIP events around the batch; cfg/sc < 0: the launcher's own choice.
int ou_bench_conv(ou_handle* h, const char* layer, int32_t B, int32_t Tin, int32_t cfg, int32_t sc, int32_t with_res,
                  int32_t iters, void* ws, size_t ws_bytes, ou_stream_t stream, float* ms_per_iter, int32_t* cfg_used) {
  if (!h || !layer || !ws || !ms_per_iter) return fail(h, OU_EINVAL, "bad argument");
  const Model& m = h->m;
  std::vector<const ConvL*> all;
  auto addb = [&](const BlockL& b) { if (b.dir) all.push_back(&b.rc); all.push_back(&b.c1); all.push_back(&b.c2); all.push_back(&b.c3); };
  for (auto& b : m.s_enc) addb(b);
  for (auto& b : m.s_dec) addb(b);
  for (auto& l : m.s_sig) all.push_back(&l);
  all.push_back(&m.s_gru.proj); all.push_back(&m.c_melconv); addb(m.c_melblock);
  for (auto& b : m.c_enc) addb(b);
  for (auto& l : m.c_st) all.push_back(&l);
  all.push_back(&m.c_gru0.proj); all.push_back(&m.c_gru1.proj);
  addb(m.c_cb1); addb(m.c_cb2); addb(m.c_decin);
  for (auto& b : m.c_dec) addb(b);
  const ConvL* L = nullptr;
  for (auto* l : all) if (l->name == layer) L = l;
  if (!L) return fail(h, OU_EMISSING, std::string("no such conv layer: ") + layer);
  hipStream_t st = (hipStream_t)stream;
  Runner r(h, ws, ws_bytes, false, st, B);
  auto keep = h->tensors;
  // (kernels whose windows begin a few samples in front of a row read -- and mask -- the bytes in front of their input tensor: it
  // must not be the first bytes of the caller's allocation; in the model's own layout the status header comes first)
  r.alloc_raw(64);
  Tensor in = r.alloc("", L->Cin, Tin);
  if (r.oom) return finish(h, r);
  r.launch("fill", [&] { return hipMemsetAsync(in.p, 0x3c, (size_t)B * L->Cin * Tin * 4, st); });
  h->force_cfg = cfg; h->force_sc = sc < 0 ? 0 : sc;
  if (h->opt.ts) h->tstamps = (long long*)((char*)ws + ws_bytes - (16u << 20));
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  size_t mark = r.off;
  Runner::Epi e;
  Tensor out = r.conv(*L, in, "", e).out;  // warm-up + output allocation
  if (with_res) e.res = out.p;
  for (int w = 0; w < 2 && r.ok(); w++) { r.off = mark; r.conv(*L, in, "", e); }
  (void)hipEventRecord(e0, st);
  for (int i = 0; i < iters && r.ok(); i++) { r.off = mark; r.conv(*L, in, "", e); }
  (void)hipEventRecord(e1, st);
  h->force_cfg = -1; h->force_sc = 0;
  h->tstamps = nullptr;
  h->tensors = keep;
  int rc = finish(h, r);
  if (rc == OU_OK) {
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    *ms_per_iter = ms / (iters > 0 ? iters : 1);
    if (cfg_used) *cfg_used = h->last_cfg;
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return rc;
}

int ou_profile_enable(ou_handle* h, int32_t on) {
  if (!h) return OU_EINVAL;
  h->profile = on != 0;
  h->prof_used = 0;
  h->prof.clear();
  if (on) {
    // measurement buffer: owned by the library, allocated outside any forward call
    if (!h->prof_dev && hipMalloc((void**)&h->prof_dev, kProfSlots * 256) != hipSuccess)
      return fail(h, OU_EHIP, "hipMalloc(profile buffer) failed");
    if (hipMemset(h->prof_dev, 0xFF, kProfSlots * 256) != hipSuccess) return fail(h, OU_EHIP, "hipMemset failed");
  }
  return OU_OK;
}

// ... and the raw stamps of the same records: first block start / last block end of every launch on the device's 100 MHz
// constant clock (10 ns ticks; one clock for all handles of a process, so that the launches of several lanes can be laid on
// one timeline), plus the variant code
int ou_profile_read_ticks(ou_handle* h, int32_t max_records, uint64_t* t_start, uint64_t* t_end, int32_t* cfg,
                          int32_t* n_records) {
  if (!h || !n_records || !t_start || !t_end) return OU_EINVAL;
  int n = (int)h->prof_used;
  if (n > max_records) n = max_records;
  std::vector<unsigned long long> host((size_t)32 * (n > 0 ? n : 1));
  if (n > 0) {
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(host.data(), h->prof_dev, (size_t)n * 256, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, OU_EHIP, hipGetErrorString(e));
  }
  for (int i = 0; i < n; i++) {
    unsigned long long t0 = ~0ull, t1 = 0ull;
    for (int w = 0; w < 16; w++) {
      const unsigned long long a = host[32 * i + w], b = ~host[32 * i + 16 + w];
      if (a < t0) t0 = a;
      if (b > t1) t1 = b;
    }
    t_start[i] = t0;
    t_end[i] = t1 >= t0 ? t1 : t0;
    if (cfg) cfg[i] = h->prof[i].cfg;
  }
  *n_records = n;
  return OU_OK;
}

int ou_profile_read(ou_handle* h, int32_t max_records, float* ms, double* flops, double* bytes, int32_t* cfg,
                    int32_t* n_records) {
  if (!h || !n_records) return OU_EINVAL;
  int n = (int)h->prof_used;
  if (n > max_records) n = max_records;
  std::vector<unsigned long long> host((size_t)32 * (n > 0 ? n : 1));
  if (n > 0) {
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(host.data(), h->prof_dev, (size_t)n * 256, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, OU_EHIP, hipGetErrorString(e));
  }
  for (int i = 0; i < n; i++) {
    unsigned long long t0 = ~0ull, t1 = 0ull;
    for (int w = 0; w < 16; w++) {
      const unsigned long long a = host[32 * i + w], b = ~host[32 * i + 16 + w];
      if (a < t0) t0 = a;
      if (b > t1) t1 = b;
    }
    if (ms) ms[i] = (t1 >= t0) ? (float)((double)(t1 - t0) * 1e-5) : 0.f;  // 100 MHz constant clock: 10 ns ticks
    if (flops) flops[i] = h->prof[i].flops;
    if (bytes) bytes[i] = h->prof[i].bytes;
    if (cfg) cfg[i] = h->prof[i].cfg;
  }
  *n_records = n;
  return OU_OK;
}

}  // extern "C"
