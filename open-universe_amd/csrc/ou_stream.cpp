// Streaming enhance: ou_stream_plan / ou_stream_emitted, the session behind ou_stream_create, and push / flush.
// A window of a stream IS an ou_enhance call (include/ouniverse.h), so this driver calls ou_enhance itself for every window -- on
// the window ou_stream.hip assembled, with the stream's counter source on the handle for the length of the call -- and adds only
// what lies around it: the plan, the ring, the crossfade with the carried tail and the running output offset.
#include "ou_sampler.h"

#include <mutex>
#include <set>

using namespace ou;

struct ou_stream_session {
  ou_handle* h = nullptr;
  int C = 0, tot = 0;
  long long S = 0, V = 0, hop = 0;
  int n_steps = 0, warm_start = -1;
  double epsilon = 0.0;
  std::vector<float> sigma;  // the caller's table (empty: the schedule's)
  uint32_t enh_flags = 0;
  bool clip = false;
  unsigned long long seed = 0;
  std::vector<unsigned long long> ids;
  // the workspace: the walk's part in front, then the stream's own areas
  void* ws = nullptr;
  size_t walk_bytes = 0, noise_bytes = 0;
  float *ring = nullptr, *win = nullptr, *res = nullptr, *carry = nullptr, *noise = nullptr;
  // where the stream stands: samples pushed and emitted per row, the next window of the plan
  long long pushed = 0, emitted = 0, next_win = 0;
  bool failed = false;
  bool prepared = false;  // the walk's header was cleared by THIS session (the handle's record of an address may be an older buffer's)
};

namespace {
std::mutex g_live_mutex;
std::set<const ou_stream_session*> g_live;
bool live(const ou_stream_session* s) {
  std::lock_guard<std::mutex> lock(g_live_mutex);
  return s && g_live.count(s) != 0;
}
const char* kNotLive = ": not a live stream (destroyed, or not returned by ou_stream_create)";

// S, V and the stride of a stream; false: refused, with the message
struct StreamGeom {
  long long S = 0, V = 0, hop = 0;
  std::string err;
};
bool stream_geom(int tot, long long segment, long long overlap, StreamGeom& g) {
  if (tot < 1) { g.err = "stream plan: tot_ds >= 1"; return false; }
  g.S = segment - segment % tot;
  g.V = overlap - overlap % tot;
  if (segment < 0 || g.S < 2 * (long long)tot) {
    g.err = "stream: segment must be at least two total down-sampling factors (" + std::to_string(2 * tot) + " samples)";
    return false;
  }
  if (overlap < 0 || 2 * g.V > g.S) { g.err = "stream: overlap must lie in [0, segment / 2]"; return false; }
  g.hop = g.S - g.V;
  return true;
}
long long padded(long long T, int tot) { return (T + tot - 1) / tot * tot; }
long long emitted_after(const StreamGeom& g, long long P) { return P < g.S ? 0 : (P - g.S) / g.hop * g.hop + g.hop; }

// the stream's areas behind the walk's workspace (offsets in bytes)
struct StreamArea {
  size_t ring, win, res, carry, noise, noise_bytes, total;
};
StreamArea stream_area(int C, long long S, long long V, int tot) {
  StreamArea a;
  size_t off = 0;
  a.ring = off; off += align256((size_t)C * S * 4);
  a.win = off; off += align256((size_t)C * S * 4);
  a.res = off; off += align256((size_t)C * S * 4);
  a.carry = off; off += align256((size_t)C * V * 4);
  a.noise_bytes = (size_t)2 * C * (S + tot) * 4;  // ou_noise_scratch_bytes(h, C, S + tot_ds)
  a.noise = off; off += align256(a.noise_bytes);
  a.total = off;
  return a;
}

// The handle's noise source for the length of one stream call.
struct NoiseScope {
  ou_handle* h;
  ou_handle::NoiseSource saved;
  explicit NoiseScope(ou_handle* h_) : h(h_), saved(h_->noise_src) {}
  ~NoiseScope() { h->noise_src = saved; }
  NoiseScope(const NoiseScope&) = delete;
  NoiseScope& operator=(const NoiseScope&) = delete;
};

// Window k of the plan, [s, s + L): gathered (with the ring update of a push's last window), enhanced, and its share [emitted, e1)
// of the stream emitted at column `col` of the call's output.  `xf`: it crossfades with the carry; `store`: it leaves one.
struct CallIO {
  const float* chunk;
  long long chunk_stride, n;
  float* out;
  long long out_stride;
  hipStream_t st;
};
int run_window(ou_stream_session* s, const CallIO& io, long long k, long long start, long long L, long long T_valid, bool write_ring,
               long long e1, bool store, long long col) {
  ou_handle* h = s->h;
  const StreamGather g{s->S, start, L, s->pushed, io.n, io.chunk_stride, T_valid, write_ring ? 1 : 0};
  if (!launched(h, launch_stream_gather(io.chunk, s->ring, s->win, g, s->C, io.st), "stream gather")) return OU_EHIP;
  // the walk's part of the workspace: prepared by the session's first window whatever the handle remembers about the address
  // (a freed buffer of an earlier session may have stood there), and again should the handle have forgotten it
  const int T_walk = (int)(s->S + s->tot);
  if (!s->prepared || !h->ws_ok(s->ws, s->walk_bytes, s->C, T_walk)) {
    if (const int rc = ou_workspace_init(h, s->C, T_walk, s->ws, s->walk_bytes, io.st)) return rc;
    s->prepared = true;
  }
  h->noise_src.on = true;
  h->noise_src.seed = s->seed;
  h->noise_src.streams.resize(s->ids.size());
  for (size_t c = 0; c < s->ids.size(); c++) h->noise_src.streams[c] = s->ids[c] + (unsigned long long)k;
  h->noise_src.scratch = s->noise;
  h->noise_src.scratch_bytes = s->noise_bytes;
  const uint32_t flags = s->enh_flags | OU_ENH_NO_PEAK_GUARD | OU_ENH_SERIAL;
  if (const int rc = ou_enhance(h, s->win, s->res, nullptr, s->C, (int32_t)L, s->n_steps, s->epsilon,
                                s->sigma.empty() ? nullptr : s->sigma.data(), s->warm_start, flags, s->ws, s->walk_bytes, io.st))
    return rc;
  StreamEmit e;
  e.L = L; e.V = s->V;
  e.i0 = s->emitted - start;
  e.n_emit = e1 - s->emitted;
  e.xf = k > 0 ? std::min(s->V, e.n_emit) : 0;
  e.V_store = store ? s->V : 0;
  e.out_stride = io.out_stride;
  e.clip = s->clip ? 1 : 0;
  if (e.n_emit > 0 || e.V_store > 0)
    if (!launched(h, launch_stream_emit(s->res, s->carry, io.out ? io.out + col : nullptr, e, s->C, io.st), "stream emit")) return OU_EHIP;
  s->emitted = e1;
  return OU_OK;
}

int check_call(ou_stream_session* s, const char* who, float* out, long long out_stride, long long out_capacity, int64_t* n_out) {
  if (!live(s)) return fail(nullptr, OU_EINVAL, std::string(who) + kNotLive);
  if (s->failed) return fail(s->h, OU_EINVAL, std::string(who) + ": an earlier call on this stream failed on the device; destroy it");
  if (!n_out || out_capacity < 0 || out_stride < out_capacity || (out_capacity > 0 && !out))
    return fail(s->h, OU_EINVAL, std::string(who) + ": bad argument (n_out given, out_stride >= out_capacity >= 0)");
  return OU_OK;
}
int check_capacity(ou_stream_session* s, const char* who, long long need, long long out_capacity) {
  if (out_capacity < need)
    return fail(s->h, OU_EINVAL, std::string(who) + ": out_capacity (" + std::to_string(out_capacity) + ") is below the " +
                                     std::to_string(need) + " samples this call emits");
  return OU_OK;
}
}  // namespace

extern "C" {

int ou_stream_plan(int32_t tot_ds, int64_t T, int32_t segment, int32_t overlap, int32_t capacity, int64_t* starts,
                   int32_t* lengths, int64_t* core_begin, int64_t* core_end, int32_t* n_windows, int32_t* overlap_used,
                   int64_t* T_pad) {
  StreamGeom g;
  if (!stream_geom(tot_ds, segment, overlap, g)) return fail(nullptr, OU_EINVAL, g.err);
  if (T < 0) return fail(nullptr, OU_EINVAL, "stream plan: T >= 0");
  const long long Tp = padded(T, tot_ds);
  if (Tp == 0) {
    if (n_windows) *n_windows = 0;
    if (overlap_used) *overlap_used = 0;
    if (T_pad) *T_pad = 0;
    return OU_OK;
  }
  // the geometry of ou_segment_plan applied to T_pad: that plan of a row whose padded length is T_pad (its pad is never empty)
  int64_t seg_pad = 0;
  const int rc = ou_segment_plan(tot_ds, Tp - 1, segment, overlap, capacity, starts, lengths, core_begin, core_end, n_windows,
                                 overlap_used, &seg_pad);
  if (rc != OU_OK) return rc;
  if (seg_pad != Tp) return fail(nullptr, OU_EINVAL, "internal: stream plan and segment plan disagree on the padded length");
  if (T_pad) *T_pad = Tp;
  return OU_OK;
}

int64_t ou_stream_emitted(int32_t tot_ds, int64_t P, int32_t segment, int32_t overlap) {
  StreamGeom g;
  if (!stream_geom(tot_ds, segment, overlap, g)) return fail(nullptr, OU_EINVAL, g.err);
  if (P < 0) return fail(nullptr, OU_EINVAL, "stream plan: P >= 0");
  return emitted_after(g, P);
}

int ou_stream_workspace_bytes(const ou_handle* hc, int32_t C, int32_t segment, int32_t overlap, size_t* nbytes) {
  ou_handle* h = const_cast<ou_handle*>(hc);
  if (C < 1) return fail(h, OU_EINVAL, "stream: C must be at least 1");
  if (!h || !nbytes) return fail(h, OU_EINVAL, "bad argument");
  StreamGeom g;
  if (!stream_geom(h->m.tot_ds, segment, overlap, g)) return fail(h, OU_EINVAL, g.err);
  if (g.S + h->m.tot_ds > 0x7fffffffll) return fail(h, OU_EINVAL, "stream: segment too long");
  size_t walk = 0;
  if (const int rc = ou_workspace_bytes(h, C, (int32_t)(g.S + h->m.tot_ds), &walk)) return rc;
  *nbytes = align256(walk) + stream_area(C, g.S, g.V, h->m.tot_ds).total;
  return OU_OK;
}

int ou_stream_create(ou_handle* h, const ou_stream_spec* spec, void* ws, size_t ws_bytes, ou_stream_session** out) {
  if (!spec || !out) return fail(h, OU_EINVAL, "bad argument");
  *out = nullptr;
  if (spec->C < 1) return fail(h, OU_EINVAL, "stream: C must be at least 1");
  if (!h || !ws || !spec->ids) return fail(h, OU_EINVAL, "bad argument");
  if (spec->C > 65535) return fail(h, OU_EINVAL, "stream: too many rows (C <= 65535)");
  const int tot = h->m.tot_ds;
  StreamGeom g;
  if (!stream_geom(tot, spec->segment, spec->overlap, g)) return fail(h, OU_EINVAL, g.err);
  if (spec->enh_flags & ~(uint32_t)(OU_ENH_KEEP_RMS | OU_ENH_USE_AUX_SIGNAL))
    return fail(h, OU_EINVAL, "stream: enh_flags takes OU_ENH_KEEP_RMS and OU_ENH_USE_AUX_SIGNAL only (a stream has no peak guard)");
  if (spec->stream_flags & ~(uint32_t)OU_STREAM_CLIP) return fail(h, OU_EINVAL, "stream: stream_flags takes OU_STREAM_CLIP only");
  if (const int rc = check_steps(h, spec->n_steps, spec->warm_start)) return rc;
  const bool need_wav = spec->warm_start >= 0 || (spec->enh_flags & OU_ENH_USE_AUX_SIGNAL);
  if (need_wav)
    if (const int rc = check_decoupling(h)) return rc;
  // a window that ou_enhance itself would refuse: T_raw = S pads to S + tot_ds there
  if (g.S + tot > max_walk_length(h, need_wav))
    return fail(h, OU_EINVAL, "stream: segment too long for one pass of ou_enhance (at most " +
                                  std::to_string(max_walk_length(h, need_wav) - tot) + " samples)");
  if (reinterpret_cast<uintptr_t>(ws) % 256 != 0) return fail(h, OU_EINVAL, "stream: the workspace must be 256-byte aligned");
  size_t walk = 0;
  if (const int rc = ou_workspace_bytes(h, spec->C, (int32_t)(g.S + tot), &walk)) return rc;
  walk = align256(walk);
  const StreamArea A = stream_area(spec->C, g.S, g.V, tot);
  if (ws_bytes < walk + A.total)
    return fail(h, OU_ENOMEM, "workspace too small: need " + std::to_string(walk + A.total) + " bytes (ou_stream_workspace_bytes)");
  auto* s = new ou_stream_session();
  s->h = h;
  s->C = spec->C; s->tot = tot;
  s->S = g.S; s->V = g.V; s->hop = g.hop;
  s->n_steps = spec->n_steps; s->warm_start = spec->warm_start < 0 ? -1 : spec->warm_start;
  s->epsilon = spec->epsilon;
  if (spec->sigma_host) s->sigma.assign(spec->sigma_host, spec->sigma_host + spec->n_steps);
  s->enh_flags = spec->enh_flags;
  s->clip = (spec->stream_flags & OU_STREAM_CLIP) != 0;
  s->seed = spec->seed;
  s->ids.assign(spec->ids, spec->ids + spec->C);
  s->ws = ws;
  s->walk_bytes = walk;
  s->noise_bytes = A.noise_bytes;
  char* area = (char*)ws + walk;
  s->ring = (float*)(area + A.ring);
  s->win = (float*)(area + A.win);
  s->res = (float*)(area + A.res);
  s->carry = (float*)(area + A.carry);
  s->noise = (float*)(area + A.noise);
  {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    g_live.insert(s);
  }
  *out = s;
  return OU_OK;
}

void ou_stream_destroy(ou_stream_session* s) {
  {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    if (!s || !g_live.erase(s)) {
      fail(nullptr, OU_EINVAL, std::string("ou_stream_destroy") + kNotLive);
      return;
    }
  }
  delete s;
}

int ou_stream_push(ou_stream_session* s, const float* chunk, int64_t chunk_stride, int64_t n, float* out, int64_t out_stride,
                   int64_t out_capacity, int64_t* n_out, ou_stream_t stream) {
  const char* who = "ou_stream_push";
  if (const int rc = check_call(s, who, out, out_stride, out_capacity, n_out)) return rc;
  if (n < 0 || (n > 0 && (!chunk || chunk_stride < n))) return fail(s->h, OU_EINVAL, std::string(who) + ": n >= 0, and a chunk of n samples per row, rows chunk_stride >= n apart");
  if (s->pushed > (1ll << 50) - n) return fail(s->h, OU_EINVAL, std::string(who) + ": stream too long (2^50 samples)");
  const StreamGeom g{s->S, s->V, s->hop, ""};
  const long long P1 = s->pushed + n, e_start = s->emitted;
  const long long need = emitted_after(g, P1) - e_start;
  if (const int rc = check_capacity(s, who, need, out_capacity)) return rc;
  *n_out = need;
  if (n == 0) return OU_OK;
  ou_handle* h = s->h;
  NoiseScope scope(h);
  const CallIO io{chunk, chunk_stride, n, out, out_stride, (hipStream_t)stream};
  // the grid windows this push completes; the last of them also moves the chunk into the ring
  const long long k_end = P1 < s->S ? 0 : (P1 - s->S) / s->hop + 1;
  int rc = OU_OK;
  if (s->next_win >= k_end) {
    const StreamGather rg{s->S, 0, 0, s->pushed, n, chunk_stride, P1, 1};
    if (!launched(h, launch_stream_gather(chunk, s->ring, s->win, rg, s->C, io.st), "stream ring")) rc = OU_EHIP;
  }
  for (long long k = s->next_win; k < k_end && rc == OU_OK; k++) {
    rc = run_window(s, io, k, k * s->hop, s->S, P1, k == k_end - 1, k * s->hop + s->hop, true, s->emitted - e_start);
    if (rc == OU_OK) s->next_win = k + 1;
  }
  if (rc != OU_OK) {
    s->failed = true;
    return rc;
  }
  s->pushed = P1;
  return OU_OK;
}

int ou_stream_flush(ou_stream_session* s, float* out, int64_t out_stride, int64_t out_capacity, int64_t* n_out, ou_stream_t stream) {
  const char* who = "ou_stream_flush";
  if (const int rc = check_call(s, who, out, out_stride, out_capacity, n_out)) return rc;
  const long long T = s->pushed, e_start = s->emitted;
  if (const int rc = check_capacity(s, who, T - e_start, out_capacity)) return rc;
  *n_out = T - e_start;
  ou_handle* h = s->h;
  NoiseScope scope(h);
  const CallIO io{nullptr, 0, 0, out, out_stride, (hipStream_t)stream};
  const long long Tp = padded(T, s->tot);
  // the windows of the plan for T that have not run: [0, T_pad) alone, or the grid windows and the shifted last one
  const long long n_grid = Tp <= s->S ? 1 : (Tp - s->S) / s->hop + 1;
  const long long n_win = T == 0 ? 0 : (Tp > s->S && (n_grid - 1) * s->hop + s->S < Tp ? n_grid + 1 : n_grid);
  int rc = OU_OK;
  for (long long k = s->next_win; k < n_win && rc == OU_OK && s->emitted < T; k++) {
    const long long L = std::min(Tp, s->S);
    const long long start = k < n_grid ? k * s->hop : Tp - s->S;
    const bool last = k == n_win - 1;
    rc = run_window(s, io, k, start, L, T, false, last ? T : std::min(start + L - s->V, T), !last, s->emitted - e_start);
  }
  if (rc == OU_OK && s->emitted < T) {
    // the plan's last window ran in an earlier call: what is left of it is the carry
    StreamEmit e;
    e.L = s->V; e.V = s->V; e.i0 = 0; e.n_emit = T - s->emitted; e.xf = 0; e.V_store = 0;
    e.out_stride = out_stride; e.clip = s->clip ? 1 : 0;
    if (!launched(h, launch_stream_emit(s->carry, s->carry, out + (s->emitted - e_start), e, s->C, io.st), "stream emit")) rc = OU_EHIP;
    s->emitted = T;
  }
  if (rc != OU_OK) {
    s->failed = true;
    return rc;
  }
  s->pushed = s->emitted = s->next_win = 0;
  return OU_OK;
}

}  // extern "C"
