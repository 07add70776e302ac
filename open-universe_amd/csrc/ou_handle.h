// What every host file of libouniverse.so needs about a handle (private): the packer and the handle behind the opaque
// types of include/ouniverse.h, the handle's options, and the two ways a call reports a failure.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/ouniverse.h"
#include "../../include/ouniverse_tuning.h"
#include "ou_kernels.h"
#include "ou_model.h"

namespace ou {
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
}  // namespace ou

struct ou_packer {
  ou::Model m;
  std::map<std::string, ou::HostTensor> sd;
  std::vector<float> blob;
  std::string err;
};

struct ou_handle {
  ou::Model m;
  const float* W = nullptr;  // packed blob (device)
  int device = 0;
  int num_cu = 256;
  std::string err;
  std::map<std::string, ou::TensorRef> tensors;
  int n_launch = 0, n_conv = 0;
  // geometry of the last ou_condition (consumed by ou_score)
  int cond_B = 0, cond_T = 0;
  bool trace = false;
  ou::Options opt;                  // ou_set_option
  ou::NormMode norm;                // ou_set_normalization (as created: norm 2, zero_mean -- the kernels' plain instantiations)
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

namespace ou {

// the message goes to the handle (when there is one) and to the thread's last error (ou_last_error); returns `code`
int fail(ou_handle* h, int code, const std::string& msg);

struct Tensor {
  float* p = nullptr;
  int C = 0, T = 0;
};

// A launch outside any walk, counted and reported as Runner::chk + finish do; false: it failed, enqueue nothing more.
bool launched(ou_handle* h, hipError_t e, const char* w);

}  // namespace ou
