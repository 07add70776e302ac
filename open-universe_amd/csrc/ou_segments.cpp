// The segmented calls: recordings of any length in windows, the windows in groups through the walk and the
// sampler loop, stitched into the long rows.  ou_enhance_segments, _ensemble, _var, _var_ensemble and their sizers.
#include "ou_sampler.h"

#include <algorithm>
#include <cmath>

using namespace ou;

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
  size_t row_scale_off, zbuf_off, carry_off;  // ... and "seg.row_scale", "seg.z", "seg.carry"
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
  w.row_scale_off = w.walk + A.row_scale;
  w.zbuf_off = w.walk + A.zbuf;
  w.carry_off = w.walk + A.carry;
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
  h->tensors["seg.row_scale"] = TensorRef{w.row_scale_off, 1, 1};  // rows 0 .. C - 1: the whole-row mel scale of the input rows
  return launched(h, launch_seg_stats(mix, w.part, w.stats, rows, C, level, h->norm, st), "segment stats") &&
         launched(h, launch_seg_mel_energy(mix, w.stats, h->W + m.mel.win_off, h->W + m.mel.tw_off, h->W + m.mel.fb_off, esum, rows,
                                           C, m.mel.n_fft, m.mel.hop, m.mel.pad_left, m.mel.n_freq, m.mel.n_mels, frames_max, st),
                  "segment mel energy");
}
// The cheap modes of a call, both from the window's own wav = aux_to_wav(conditioner(window)): `warm` -- the
// sampler starts at step n_start from wav + sigma[n_start] z_0 --, `aux` -- wav is the window's result, no score pass and no noise.
struct SegMode {
  int n_start;
  bool warm, aux;
  SegMode(int warm_start, uint32_t flags)
      : n_start(warm_start >= 0 ? warm_start : 0), warm(warm_start >= 0), aux((flags & OU_ENH_USE_AUX_SIGNAL) != 0) {}
  bool need_wav() const { return warm || aux; }
};
// One step's noise of a group's n_rows walk rows of T columns, in w.zbuf: `gather(slice)` enqueues the gather from one step's
// slice of the caller's tensor (step_noise words), or -- counter mode -- the same positions come straight from the function, no
// whole-row noise exists then: `entry(row, stream_row, t0, len)` names the long row whose stream walk row `row` reads, the first
// position and the length (0 behind it, so x needs no mask).  Draw d is plane (d ? d - n_start : 0) of the caller's tensor: the
// convention of ou_enhance (row_noise), (n_steps - n_start) planes.
// (the names a group leaves behind: "seg.z", E * Bw rows of T: the last step's noise of the last group; "seg.carry", E rows of T:
// the window in front of the last group that had one)
void seg_group_taps(ou_handle* h, const SegWs& w, int T, bool with_z) {
  if (with_z) h->tensors["seg.z"] = TensorRef{w.zbuf_off, 1, T};  // (the aux exit reads no noise)
  h->tensors["seg.carry"] = TensorRef{w.carry_off, 1, T};
}
template <class Gather, class EntryFn>
auto seg_noise(ou_handle* h, Runner& r, const float* noise, size_t step_noise, int n_start, float* zbuf, int T, int n_rows,
               Gather gather, EntryFn entry) {
  return [=, &r](int draw) -> const float* {
    if (noise) {
      gather(noise + (size_t)(draw ? draw - n_start : 0) * step_noise);
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
                SegMode mode, uint32_t flags, void* ws, size_t ws_bytes, ou_stream_t stream) {
  if (mode.need_wav())
    if (const int rc = check_decoupling(h)) return rc;
  if (g.L > max_walk_length(h, mode.need_wav()))
    return fail(h, OU_EINVAL, std::string(who) + ": segment too long for one pass of the walk");
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
    // (the persistent area of the workspace keeps the tables from group to group; the aux exit runs no step)
    if (e0 == 0 && !mode.aux) tab.upload(r, P);
    Runner rc = Runner::conditioner_of(r, Bc);
    // the group's inputs: once into the prefix, or -- the conditioner over all rows -- once per member
    for (int e = 0; e < (share ? 1 : E); e++)
      rc.launch("segment gather", [&] {
        return launch_seg_gather_input(mix, w.stats, w.row_scale, P.mixn.p + (size_t)e * Bw * L, P.mel_scale + (size_t)e * Bw, rows,
                                       ents, Bw, L, st);
      });
    run_condition(rc, P, P.mixn.p, L);
    // the window's own wav, its scratch behind the conditioner's (ou_workspace_bytes reserves it for the walk's rows)
    if (mode.need_wav()) decouple(rc, P);
    // (the statistics of the post step are those of the whole long rows, w.stats: P.stats is not written)
    if (share) replicate_conditioned(rc, P, Bw, E, false, false);
    if (const int rc2 = finish(h, rc)) return rc2;
    r.off = rc.off;
    // walk row e * Bw + j: window k of long row e * C + c, positions s_k + i of that row's noise.  The filler rows of a short
    // last group repeat their member's last real entry.
    auto z = seg_noise(h, r, noise, (size_t)E * C * g.T_pad, mode.n_start, w.zbuf, L, B,
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
    if (!mode.aux) sample(r, P, L, tab, mode.n_start, mode.warm ? P.wav.p : nullptr, false, z);
    const float* y = mode.aux ? P.wav.p : P.x.p;  // what the windows of this group are
    seg_group_taps(h, w, L, !mode.aux);
    r.launch("segment stitch", [&] { return launch_seg_stitch(y, w.carry, members, rows, ents, n_real, L, Bw, E, C, st); });
    if (e0 + Bw < g.n_entries) seg_carry(r, w.carry, y, L, Bw, E, n_real);
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
                    const SegGroups& G, int n_steps, double epsilon, const float* sigma_host, SegMode mode, uint32_t flags,
                    void* ws, size_t ws_bytes, ou_stream_t stream) {
  const Model& m = h->m;
  const int tot = m.tot_ds;
  if (mode.need_wav())
    if (const int rc = check_decoupling(h)) return rc;
  if (G.length > max_walk_length(h, mode.need_wav()))
    return fail(h, OU_EINVAL, std::string(who) + ": segment too long for one pass of the walk");
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
    // (the persistent area keeps the tables from group to group: its layout depends on B alone; the aux exit runs no step)
    if (gi == 0 && !mode.aux) tab.upload(r, P);
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
    // the window's own wav (seg_enhance); in a ragged group the layer writes 0 behind an entry's own length, as the noise gather
    // does, so x0 = wav + sigma z_0 and the stitched wav keep that invariant without a mask
    if (mode.need_wav()) decouple(rc, P);
    // (the statistics of the post step are those of the whole long rows, w.stats: P.stats is not written)
    if (share) replicate_conditioned(rc, P, Bw, E, false, false);
    if (const int rc2 = finish(h, rc)) return rc2;
    r.off = rc.off;
    // walk row e * Bw + j: window k of long row e * C + c, positions s_k + i of that row's noise
    auto z = seg_noise(h, r, noise, (size_t)E * C * T_pad_max, mode.n_start, w.zbuf, T, B,
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
    if (!mode.aux) sample(r, P, T, tab, mode.n_start, mode.warm ? P.wav.p : nullptr, false, z);
    const float* y = mode.aux ? P.wav.p : P.x.p;  // what the windows of this group are
    if (full) seg_group_taps(h, w, T, !mode.aux);
    else if (!mode.aux) h->tensors["seg.z"] = TensorRef{w.zbuf_off, 1, T};  // (a SHORT group reads no carry: the name keeps the FULL groups' rows)
    for_blocks(n_real, [&](const SegEntriesList& ents, int n) {
      r.launch("segment stitch", [&] { return launch_seg_stitch(y, w.carry, members, rows, ents, n, T, Bw, E, C, st); });
    });
    if (full && e_end < G.n_full) seg_carry(r, w.carry, y, T, Bw, E, n_real);  // the window in front of the next group
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
  const SegMode mode(warm_start, flags);
  if (const int rc = check_noise_source(h, noise, C, "the rows of the call (", !mode.aux)) return rc;
  if (const int rc = check_steps(h, n_steps, warm_start)) return rc;
  SegPlan plan;
  if (!seg_plan(h->m.tot_ds, T_raw, segment, overlap, plan)) return fail(h, OU_EINVAL, plan.err);
  SegGeom g = plan.g;
  g.n_entries = (long long)C * g.n_win;
  return seg_enhance(h, "ou_enhance_segments", "ou_segments_workspace_bytes", mix, out, out, noise, C, 1, false, 0, g,
                     seg_batch(g.n_entries, max_batch), n_steps, epsilon, sigma_host, mode, flags, ws, ws_bytes, stream);
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
                     epsilon, sigma_host, SegMode(-1, 0), flags, ws, ws_bytes, stream);
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
  const SegMode mode(warm_start, flags);
  if (const int rc = check_noise_source(h, noise, C, "the rows of the call (", !mode.aux)) return rc;
  if (const int rc = check_steps(h, n_steps, warm_start)) return rc;
  SegGroups G;
  if (!seg_groups(h->m.tot_ds, C, t_raw, segment, overlap, max_batch, G)) return fail(h, OU_EINVAL, G.err);
  return seg_var_enhance(h, "ou_enhance_segments_var", "ou_segments_var_workspace_bytes", mix, out, out, noise, C, T_raw_max, t_raw,
                         1, false, 0, G, n_steps, epsilon, sigma_host, mode, flags, ws, ws_bytes, stream);
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
                         stat, G, n_steps, epsilon, sigma_host, SegMode(-1, 0), flags, ws, ws_bytes, stream);
}

}  // extern "C"
