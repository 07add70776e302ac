// The network walk: what Runner does per conv layer, ConvBlock and GRU layer, the conditioner and the score
// passes built from them, and the sampler's scalars.  No allocation, no host sync: everything goes through Runner::launch.
#include "ou_walk.h"
#include "ou_internal.h"
#include "ou_variants.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "../../include/ouniverse_tuning.h"

namespace ou {

// make stream `to` wait for everything enqueued so far on `from`
void Runner::wait_for(hipStream_t from, hipStream_t to, const char* w_record, const char* w_wait) {
  if (dry || !ok()) return;
  hipEvent_t e = next_event();
  if (!e) { herr = hipErrorOutOfMemory; where = "event"; return; }
  launch(w_record, [&] { return hipEventRecord(e, from); });
  launch(w_wait, [&] { return hipStreamWaitEvent(to, e, 0); });
}

// the launch arguments of layer L reading `in`, writing `out`, with epilogue e
ConvArgs Runner::conv_args(const ConvL& L, const Tensor& in, const Tensor& out, const Epi& e) {
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

// one conv layer: allocate (unless `dst`), then profile, launch, mask, trace and count
Runner::ConvOut Runner::conv(const ConvL& L, const Tensor& in, const std::string& name, const Epi& e, const Tensor* dst) {
  ConvOut o;
  o.out = dst ? *dst : alloc(name, L.Cout, conv_tout(L, in.T));
  if (dry || !ok()) return o;
  ConvArgs a = conv_args(L, in, o.out, e);
  // algorithmic (reference, un-folded) work of this layer: dense FLOPs, activations once, weights once (the packed layers
  // carry the reference's own kernel sizes)
  a.prof = prof_open(2.0 * L.M * (double)a.Nq * L.Cin * L.KW * B,
                     4.0 * ((double)B * ((double)L.Cin * in.T + (double)L.Cout * a.Tout) + (double)L.M * L.Cin * L.KW), -1);
  // plan, then launch once (ou_internal.h): nothing is enqueued for a layer that falls back
  ConvPlan p = e.rate_down ? plan_rate_down(a) : e.rate_up ? plan_rate_up(a) : plan_conv(a, h->num_cu);
  if (!e.rate_down && !e.rate_up) {
    if (p.status == hipErrorNotSupported && a.out_act) {  // the kernel for this layer has no activating epilogue: store y
      a.out_act = 0;
      p = plan_conv(a, h->num_cu);
    }
    o.stored_act = a.out_act != 0;
    if (p.status == hipErrorNotSupported && e.fir) {  // not a failure and not counted: the caller falls back to conv + launch_fir
      prof_drop(a.prof);
      o.supported = false;
      return o;
    }
  }
  const int cfg = p.variant;
  const hipError_t le = launch_plan(p, st);
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

// What plan_rate_up / plan_rate_down are asked about the rate-change conv of a block reading Tin frames: the shape and
// whether a FIR rides along (fir_mode 1: in front of the down conv, 2: behind the up conv).  Pure function of the layer shape.
ConvArgs Runner::rate_probe(const ConvL& rc, int Tin) {
  ConvArgs a;
  a.up = rc.up; a.stride = rc.stride; a.KW = rc.KW; a.pad = rc.pad; a.Tin = Tin;
  a.Nq = conv_nq(rc, Tin); a.Tout = conv_tout(rc, Tin); a.M = rc.M; a.Cout = rc.Cout; a.Cin = rc.Cin;
  a.fir = (rc.fir_mode == 1 || rc.fir_mode == 2) ? W(rc.fir_off) : nullptr; a.fir_len = rc.fir_len;
  return a;
}

// blocks.py:366-376: the block's input brought to the block's rate, `res` (the skip connection) added.  `res` for dir == 0
// blocks must already be folded into `hin`.
Tensor Runner::up_path(const BlockL& Bk, const Tensor& hin, const std::string& nm, const float* res) {
  if (Bk.dir != 2) return hin;
  const ConvL& rc = Bk.rc;
  Epi e;
  e.res = res; e.res_scale = kInvSqrt2;  // blocks.py:374-376 fused into the up-conv epilogue
  if (rc.fir_mode == 2) { e.fir = W(rc.fir_off); e.fir_len = rc.fir_len; e.fir_bias = W(rc.fbias_off); }
  if ((rc.fir_mode == 0 || rc.fir_mode == 2) && env.rate_small != 0 && plan_rate_up(rate_probe(rc, hin.T)).status == hipSuccess) {
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
ChainArgs Runner::chain_args(const BlockL& Bk, int depth, const Tensor& hu, const Tensor& c1, const Tensor& v, const Epi& e1,
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
int Runner::plan_chain(const BlockL& Bk, const Tensor& hu, const Tensor& c1, const Tensor& v, const Epi& e1, bool need_c1) {
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
bool Runner::body_block3(const BlockL& Bk, const Tensor& hu, const Tensor& c1, const Tensor& c2, const Tensor& v, const std::string& nm,
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
Tensor Runner::activated(const ConvL& L, const Tensor& in, const Tensor& plane) {
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
void Runner::body(const BlockL& Bk, const Tensor& hu, const Tensor& c1, const Tensor& c2, const Tensor& v, const std::string& nm,
                  Epi e1, bool need_c1, bool c1_private, const Tensor& act) {
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
Tensor Runner::down_path(const BlockL& Bk, const Tensor& v, const std::string& nm) {
  if (Bk.dir != 1) return v;
  const ConvL& rc = Bk.rc;
  Epi e;
  // wide levels: FIR + strided conv in one launch
  if (rc.fir_mode <= 1 && env.rate_small != 0 && plan_rate_down(rate_probe(rc, v.T)).status == hipSuccess) {
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

// `c1_dst` / `v_dst`: caller-provided (persistent) tensors for the conv1 result / the block output, so that
// conditioner outputs are produced in place instead of being copied out of the scratch area afterwards
Runner::BlockOut Runner::block(const BlockL& Bk, const Tensor& hin, const std::string& nm, const float* film, int film_bs,
                               const float* input_cond, const float* res, bool need_c1, const Tensor* c1_dst,
                               const Tensor* v_dst) {
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
Tensor Runner::gru(const GruL& G, const Tensor& in, const std::string& nm, unsigned long long* xchg, unsigned* errw,
                   unsigned* epoch, const float* res, float res_scale, hipEvent_t* before) {
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
                     4.0 * ((double)B * (6.0 + 2.0 + (res ? 2.0 : 0.0)) * G.H * in.T + 2.0 * 3.0 * G.H * G.H), kVarRecurrence + in.T);
  if (before && (*before = next_event())) launch("pre-gru record", [&] { return hipEventRecord(*before, st); });
  launch(G.name.c_str(), [&] { return launch_gru(a, h->num_cu, st); });
  mask(out);
  return out;
}

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
  // (a score network without a GRU, OU_SEQ_NONE, has no second exchange area)
  P.xchg2 = m.s_has_gru ? (unsigned long long*)r.alloc_raw(gru_granules(r.B, m.OC / 2) * 2) : nullptr;
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
// `pre_gru`: an event to record right in front of the GRU launch (Runner::gru)
ScoreEnc run_score_enc(Runner& r, Persist& P, const float* x, const StepCoef* coef, int coef_bs,
                       const float* film_row, int film_bs, int T, hipEvent_t* pre_gru) {
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
  // The bottleneck (score.py:113-123).  Plain GRU model: when decoder block 0 has no rate change its residual add
  // (blocks.py:374-376) is fused into the GRU's epilogue.  Sandwich (conv_block1 -> GRU -> conv_block2): that add belongs behind
  // conv_block2, and with seq_model none there is no GRU to carry it: decoder block 0 then takes the residual itself
  // (run_score_dec), as the models without extra_conv_block do.
  E.fuse_res = m.s_has_gru && !m.s_sandwich && m.s_dec[0].dir == 0;
  if (!m.s_has_gru) { E.hg = hcur; return E; }
  // (conv_block1 is masked like any block; conv_block2 reads exact zeros behind a row's own end: Runner::gru masks what the
  // tail fill left there, as between cond.gru and cond.cb2)
  if (m.s_sandwich) hcur = r.block(m.s_cb1, hcur, "score.cb1", nullptr, 0, nullptr, nullptr).v;
  E.hg = r.gru(m.s_gru, hcur, "score.gru", P.xchg2, P.status, P.status + 4,
               E.fuse_res && !r.dry ? E.residuals[m.n_blocks - 1].p : nullptr, kInvSqrt2, pre_gru);
  if (m.s_sandwich) E.hg = r.block(m.s_cb2, E.hg, "score.cb2", nullptr, 0, nullptr, nullptr).v;
  return E;
}
void run_score_dec(Runner& r, Persist& P, const ScoreEnc& E, const float* x, const float* noise, float* out, int mode,
                   const StepCoef* coef, int coef_bs, const float* film_row, int film_bs, int T, const Tensor* dec0_done) {
  const Model& m = r.h->m;
  Tensor y = E.hg;
  for (int j = 0; j < m.n_blocks; j++) {
    if (j == 0 && dec0_done) { y = *dec0_done; continue; }
    const float* fr = film_row ? film_row + m.film.dec_off[j] : nullptr;
    const Tensor& res = E.residuals[m.n_blocks - 1 - j];
    const float* resp = (j == 0 && E.fuse_res) ? nullptr : res.p;
    if (!(j == 0 && E.fuse_res) && m.s_dec[j].dir == 0) {  // (not `resp`: a dry walk has no pointers, and has to see the plane)
      // a block without a rate change has no up conv whose epilogue could add its residual (up_path), and here no GRU took it
      // either (sandwich, seq_model none): (y + res) / sqrt(2) as one sum_kernel pass over OC x T / tot_ds.  Both operands are
      // zero behind a ragged row's end, so the sum is.
      const Tensor in0 = r.alloc("score.dec" + std::to_string(j) + ".in", y.C, y.T);
      r.launch("dec res", [&] {
        return launch_sum(y.p, res.p, nullptr, nullptr, nullptr, kInvSqrt2, in0.p, (size_t)r.B * y.C * y.T, r.st);
      });
      y = in0;
      resp = nullptr;
    }
    auto bo = r.block(m.s_dec[j], y, "score.dec" + std::to_string(j), fr, film_bs, P.sc[j].p, resp);
    y = bo.v;
  }
  r.launch_masked("score.out", out, 1, T, [&](const int* ln) {
    return launch_out_conv(y.p, r.W(m.s_out.w_off), r.W(m.s_out.b_off), r.W(m.s_out.a_off), x, noise, out, coef, coef_bs,
                           m.cfg.has_edm, mode, r.B, m.C0, T, m.s_out.KW, r.st, ln);
  });
}
// (the plain GRU model only: with the sandwich conv_block2 sits between the GRU and decoder block 0, with none there is no GRU)
static bool m_blocks_ok(const Runner& r) {
  const Model& m = r.h->m;
  return m.n_blocks >= 1 && m.s_dec[0].dir == 0 && m.s_has_gru && !m.s_sandwich;
}
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

int finish(ou_handle* h, Runner& r) {
  if (r.oom) return fail(h, OU_ENOMEM, "workspace too small: need " + std::to_string(r.off) + " bytes");
  if (r.herr != hipSuccess)
    return fail(h, OU_EHIP, std::string("HIP error at ") + r.where + ": " + hipGetErrorString(r.herr));
  return OU_OK;
}

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

}  // namespace ou
