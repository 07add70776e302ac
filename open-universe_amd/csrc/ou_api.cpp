// C ABI of libouniverse.so (include/ouniverse.h): the packer, the handle and its options, the workspace, lanes, the noise
// source, and the readers of what a call left behind (tensors, launch counts, profile).  The forward calls are in
// ou_sampler.cpp and ou_segments.cpp, the network walk they drive in ou_walk.cpp, the entry points that need no handle in
// ou_stateless.cpp.  There is no CPU path: without a HIP device ou_create fails.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "ou_variants.h"
#include "ou_walk.h"

using namespace ou;

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace ou {

int fail(ou_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  g_last_error = msg;
  return code;
}

// A launch outside any walk, counted and reported as Runner::chk + finish do; false: it failed, enqueue nothing more.
bool launched(ou_handle* h, hipError_t e, const char* w) {
  h->n_launch++;
  if (e == hipSuccess) return true;
  fail(h, OU_EHIP, std::string("HIP error at ") + w + ": " + hipGetErrorString(e));
  return false;
}

}  // namespace ou

namespace {

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
    if (m.s_sandwich) { addb(m.s_cb1); addb(m.s_cb2); }
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
  if (m.s_has_gru) all.push_back(&m.s_gru.proj);
  if (m.s_sandwich) { addb(m.s_cb1); addb(m.s_cb2); }
  all.push_back(&m.c_melconv); addb(m.c_melblock);
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

// the family a variant code names (ou_variants.h), or null: pure host code, works without a device
const char* ou_variant_family(int32_t code) { return ou::variant_family(code); }

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
