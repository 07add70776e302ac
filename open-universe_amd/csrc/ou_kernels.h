// Launch wrappers of the gfx950 kernels (ou_kernels.hip).  Host-callable, everything enqueued on `stream`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ou {

// ---- generic fp32-MFMA implicit-GEMM Conv1d -------------------------------------------------------------
//   y[b][co][q*up + p] = epi( bias[co] + sum_{ci,k} W[co*up+p][ci][k] * act(in_scale[b] * x[b][ci][q*stride + k - pad]) )
//   epi(v): v = (v + add)*add_scale ; v = gamma*v + beta (FiLM) ; v = (v + res)*res_scale     (each optional)
struct ConvArgs {
  const float* x = nullptr;       // (B, Cin, Tin)
  const float* w = nullptr;       // packed [Cin/CK][KW][CK][Mp]
  const float* wd = nullptr;      // second copy, taps innermost: [Cin][Mp][4 (k3) / 8 (k5)] (conv_direct2_kernel) or null
  const float* wu = nullptr;      // third copy, Winograd domain U = G w: [Cin][Mp][4 (F(2,3)) / 8 (F(2,5): 6 used)] or null
  const void* wsplit = nullptr;   // fourth copy, three bf16 pieces per weight as MFMA A fragments: [Cin/16][KW][Mp/32][3][64][8 bf16]
                                  // (conv_split_kernel) or null
  const void* wsplitw = nullptr;  // fifth copy: the Winograd-domain weights U = G w the same way, [Cin/16][KW + 1][Mp/32][3][64][8 bf16]
                                  // (conv_splitw_kernel) or null
  int split_wino = 1;             // option split_wino: 0 = conv_split_kernel also where conv_splitw_kernel could take the layer
  const float* bias = nullptr;    // [Cout]
  float* y = nullptr;             // (B, Cout, Tout)
  const float* in_scale = nullptr;  // [B] or null
  int act = 0;                      // PReLU prologue on/off
  float alpha_val = 0.f;            // its slope (by value: no dependent scalar load at kernel entry)
  const float* add = nullptr;       // (B, Cout, Tout) or null
  const float* film = nullptr;      // gamma at film[b*film_bstride + co], beta at [.. + Cout + co]
  const float* res = nullptr;       // (B, Cout, Tout) or null
  float add_scale = 1.f, res_scale = 1.f;
  int film_bstride = 0;
  int B = 1, Cin = 0, Tin = 0, Cout = 0, M = 0, Mp = 0, KW = 1, stride = 1, pad = 0, up = 1, CK = 2;
  int Nq = 0;    // GEMM columns (output positions per row)
  int Tout = 0;  // output length (<= Nq*up)
  unsigned magic_span[3] = {0, 0, 0};  // filled by plan_conv: 2^32/span + 1 for BN = 128 / 64 / 32
  unsigned magic_up = 0;               // 2^32/up + 1 (0 when up == 1)
  int SC = 1;                          // filled by plan_conv: packed chunks per pipeline stage
  int grid_n = 1, grid_m = 1;          // filled by plan_conv: tile counts (1-D grid, XCD-aware mapping)
  int xcd_map = 0;                     // filled by plan_conv: block -> tile mapping (see the kernel)
  int force_cfg = -1, force_sc = 0;    // tuning overrides (ou_bench_conv)
  int force_xcd_map = -1;              // tuning: 0 / 1 / 2
  double tile_min = -1.0;              // OU_TILE_MIN (< 0: the launcher's default of 1.2 wave tiles per SIMD)
  int tile_prefetch = 1;               // OU_TILE_PREFETCH: LDS prefetch of the epilogue operand in conv_direct3_kernel
  int direct = 5;                      // OU_CONV_DIRECT: 0 = never use the register-direct kernels, 1 = only the first
                                       // generation (dword loads), 2 = + wide-load split-K variant where a layer has `wd`,
                                       // 3 = + the no-split-K throughput kernel (conv_direct3_kernel) for many-column launches,
                                       // 4 = + the wide-load split-K kernel for 1x1 / phase-GEMM / rate-change layers
                                       //     (conv_direct4_kernel),
                                       // 5 = + minimal filtering F(2, 3) / F(2, 5) for the k3 / k5 layers on 64-column tiles
                                       //     (conv_direct2w_kernel; default)
  int d2_map = -1;                     // OU_D2_MAP: block -> tile mapping of the wide-load split-K kernels only (tuning)
  int split = -1;                      // OU_SPLIT: -1 = the bf16-split kernel (conv_split_kernel) where the launcher's rule says so,
                                       // 0 = never, 1 = wherever a layer has the split copy (tests / tuning)
  int wino = 1;                        // OU_WINO=0: never use the minimal-filtering variants (conv_direct2w_kernel, ...)
  int d2_wk = 0;                       // OU_D2_WK = 4 / 8: K slices (waves per block) of conv_direct2_kernel (0: the launcher's rule)
  int d4_fir_unfused = 1;              // OU_D4_FIR=0: up convs with a fusable FIR stay on the first-generation fused kernel
  int d4_short = 1;                    // OU_D4_SHORT=0: the 401-frame levels at batch 1 stay on the first-generation kernels
  int d4_force = 0;                    // OU_D4_FORCE = 10 TM + log2(WK): that tile shape wherever a layer admits it (tests / tuning)
  int d2_tile_rule = 1;                // option d2_tile_rule: 0 = round 5's tile-width rule of the wide-load split-K kernels (A / B)
  int deep_factor = 8;                 // option deep_factor: up to this many blocks of 64 x 128 per CU a layer is "deep" (split-K kernels)
  // Anti-alias FIR of the up path fused into the epilogue (direct kernel, up > 1, KW == 1 only; launch_conv returns
  // hipErrorNotSupported otherwise and the caller runs launch_fir after a plain launch):
  //   y = FIR_{2 up + 1}(u) + bias ; y = res ? (y + res) * res_scale : y,   u = the transposed conv's output WITHOUT bias
  // Activation moved from the consumer's operand path to the producer's epilogue (round 5): with out_act the kernel stores
  // prelu(y; out_alpha) INSTEAD of y -- for tensors whose only reader is the next PReLU_Conv (conv1 -> conv2 -> conv3 inside a
  // ConvBlock, blocks.py:395-399); that conv then runs with act = 0 and its loop has no PReLU (every input element used to be
  // activated again by every row group and every overlapping window, and each VALU instruction beside fp32 MFMAs costs ~3 cycles
  // of the matrix pipe: tools/ubench/mfma_valu_mix.hip).  Same arithmetic on the same values: bit-identical.
  // Kernels without the epilogue form return hipErrorNotSupported (the caller stores y and keeps act = 1 downstream).
  int out_act = 0;
  float out_alpha = 1.f;
  // Ragged batch (ou_enhance_var): valid OUTPUT samples per batch row, [B] on the device, or null (all rows whole).  The kernel
  // families listed in conv_masks_rows() store 0 from lens[b] on themselves; after the others the runner launches
  // launch_mask_tail.  (Inputs need nothing: they are zero behind their rows by the same invariant.)
  const int* lens = nullptr;
  const float* fir = nullptr;
  int fir_len = 0;
  int tile_bm = 32, tile_bn = 0, tile_halo = 0;  // filled by plan_conv_direct: rows / columns a tile advances by, left halo
  int dbg = 0;                         // phase ablation switches (tuning only)
  long long* tstamps = nullptr;        // per-wave phase cycle counts (tuning only)
  unsigned long long* prof = nullptr;  // measurement: 16 x min block start, 16 x ~max block end (slot = block id & 15: 500
                                       // same-address atomics in half a microsecond stall an L2 channel), 10 ns ticks
};
// returns hipSuccess or the launch error; `cfg_out` (optional) receives the tile configuration index used
hipError_t launch_conv(const ConvArgs& a, int num_cu, hipStream_t stream, int* cfg_out = nullptr);
hipError_t init_conv_kernels();  // raises the dynamic-LDS limit of every instantiation
double direct3_tiles_per_simd(int M, int Nq, int B, int num_cu);  // wave tiles per SIMD of the no-split-K throughput kernel
// (plan_rate_down / plan_rate_up of ou_internal.h:) Small-K rate-change conv of the wide levels with the anti-alias FIR fused:
// y = conv_{k=s=r}(FIR(prelu(x))) + bias (a.fir = taps or null, a.fir_len = 2r + 1; a.act / a.alpha_val = the PReLU);
// hipErrorNotSupported = use launch_fir + launch_conv.  ... and the last up conv: y = FIR(convT_{k=s=r}(prelu(x))) + bias, then
// the residual (a.fir = taps or null, a.bias = the bias added after the filter)

// ---- small VALU kernels ------------------------------------------------------------------------------------
// Per-step scalars of the sampler / EDM wrapper (universe.py:175-209, 333-343), one row per batch element
// (or one shared row when bstride == 0).  All fp32, computed on the host in the reference's op order.
struct StepCoef {
  float w_in, sigma_net, w_skip, w_out, sig2, c1, s_next, beta;
};
enum OutMode { OUT_SCORE = 0, OUT_UPDATE = 1 };
// Conv1d(1 -> C, k) 'same' on w_in[b]*x (w_in from the coefficient row, 1 when coef == null)
//   score.py:243-245,284 ; condition.py:295-300,360
hipError_t launch_in_conv(const float* x, const float* w, const float* bias, const StepCoef* coef, int coef_bstride,
                          float* y, int B, int C, int T, int KW, hipStream_t s, const int* lens = nullptr);
// PReLU -> PReLU -> Conv1d(C -> 1, k) fused with the EDM score and the sampler update:
//   net -> score = edm ? (w_skip*x + w_out*net - x)/sig2 : net
//   OUT_SCORE : out = score ;  OUT_UPDATE : out = x + c1*score + beta*(noise*s_next)   (noise may be null)
hipError_t launch_out_conv(const float* s, const float* w, const float* bias, const float* alphas, const float* x,
                           const float* noise, float* out, const StepCoef* coef, int coef_bstride, int edm,
                           int mode, int B, int C, int T, int KW, hipStream_t st, const int* lens = nullptr);

// Noise-level embedding for S sigma rows (sigma_block.py) -> g (S, D)
hipError_t launch_sigma_embed(const StepCoef* coef, int S, const float* params, int simple, int n_rff, int D,
                              float* g, hipStream_t st);
// All FiLM projections at once: film[s][r] = W[r][:] . g[s][:] + b[r]
hipError_t launch_film(const float* g, const float* W, const float* b, float* film, int S, int rows, int D,
                       hipStream_t st);
// Upload up to 128 StepCoef rows passed by value (graph-capture safe, no host memory involved)
struct CoefBlock { StepCoef c[64]; };
hipError_t launch_upload_coef(StepCoef* dst, const CoefBlock& blk, int n, hipStream_t st);

// ---- batches whose rows have lengths of their own ("ragged": ou_enhance_var) --------------------------------------------
// Row b of the batch is the utterance it would be in a call of its own: its own pad() split (universe.py:219-223), its own
// statistics, and 'same' zero padding right behind ITS last sample on every level.  The invariant that carries this through
// the network: every activation tensor is ZERO from the row's own length on (len_l[b] = t_pad[b] * T_l / T on the level of
// length T_l), so that a halo read past a row's end sees what the reference's conv padding would supply.  Kernels that take a
// `lens` pointer keep the invariant themselves (null = all rows have the tensor's length); after the others the runner
// launches launch_mask_tail.
struct RowInfo { int t_raw, pad_left, t_pad, _r; };
// The level normalisation of a row (utils/norm.py:22-87), by value into every kernel that forms a row's mean and gain.  With
// m = the mean of the padded row, sd = its unbiased std (around m, whatever zero_mean says: torch's std removes the mean
// itself) and mx = max |x - mu| over the padded row, mu = zero_mean ? m : 0:
//   norm 2:      gain = level / max(sd, 1e-5)                        norm max:  gain = level / max(mx, 1e-5)
//   norm 2-max:  gain = min(level / max(sd, eps), 1 / max(mx, eps))  (norm.py:36-39 hands normalization_kwargs.eps to this
//                                                                     branch alone; the other two clamp at 1e-5 whatever it is)
// and y = (x - mu) * gain, stats = {mu, gain, mix_rms, 0}.  plain() = norm 2 with zero_mean: the kernels' <false>
// instantiation, which never looks at this struct -- the code every model had before the other modes existed.
struct NormMode {
  int norm = 0;        // OU_NORM_2 | OU_NORM_MAX | OU_NORM_2MAX
  int zero_mean = 1;
  float eps = 1e-5f;   // the clamp in force for `norm` (see above)
  bool plain() const { return norm == 0 && zero_mean; }
  // sd, mx: unclamped.  (fmaxf / fminf and true divisions: a row's gain has the same bits in every kernel that forms it)
  __host__ __device__ float gain(float level, float sd, float mx) const {
    if (norm == 1) return level / fmaxf(mx, eps);
    if (norm == 2) return fminf(level / fmaxf(sd, eps), 1.f / fmaxf(mx, eps));
    return level / fmaxf(sd, eps);
  }
};
constexpr int kMaxLenLevels = 8;
struct LevelSpec { int n = 0; int num[kMaxLenLevels]; int den[kMaxLenLevels]; };  // len_l[b] = t_pad[b] * num / den
struct RowBlock { int t_raw[64]; };
// rows[off .. off + n) <- {t_raw, pad_left, t_pad} (universe.py:219-223) ; lens[l * B + off + i] <- t_pad * num_l / den_l
hipError_t launch_upload_rows(RowInfo* rows, int* lens, const RowBlock& blk, int n, int off, int B, int tot_ds,
                              const LevelSpec& lv, hipStream_t st);
// y[b][c][t] = 0 for t >= lens[b]   (y: (B, C, T))
hipError_t launch_mask_tail(float* y, const int* lens, int B, int C, int T, hipStream_t st);
// GRU input projections gx (B, 6H, T) of a ragged batch, t >= lens[b]: 0 in the r / n rows and +1e4 in the z rows of both
// directions -- z = sigmoid(1e4 + ..) is exactly 1, so h' = (h - n) z + n holds the state: the backward pass reaches the row's
// last frame with h = 0 exactly, as the reference's pass over that row alone starts (the forward pass's frames past the end
// are masked afterwards).  The recurrence kernels need no per-row length.
hipError_t launch_gru_tail_fill(float* gx, const int* lens, int B, int H, int T, hipStream_t st);
// pad + normalize / unpad + post with per-row geometry (rows: RowInfo[B]); mix and out are (B, T_raw_max), y / x (B, T_pad_max)
hipError_t launch_pad_normalize_var(const float* mix, float* y, float* stats, const RowInfo* rows, int B, int T_raw_max,
                                    int T_pad_max, float level, const NormMode& nm, hipStream_t st);
hipError_t launch_post_var(const float* x, const float* stats, float* out, const RowInfo* rows, int B, int T_raw_max,
                           int T_pad_max, int keep_rms, int peak_guard, hipStream_t st);

// pad (universe.py:219-223) + normalize_batch (utils/norm.py:47-87).  stats[b] = {mean, gain, mix_rms, 0}
hipError_t launch_pad_normalize(const float* mix, float* y, float* stats, int B, int T_raw, int T_pad, int pad_left,
                                float level, const NormMode& nm, hipStream_t st);
// unpad + keep_rms + peak guard (universe.py:349-357)
hipError_t launch_post(const float* x, const float* stats, float* out, int B, int T_raw, int T_pad, int pad_left,
                       int keep_rms, int peak_guard, hipStream_t st);
// x0 = sigma0 * noise (universe.py:326) ; optionally x0 = base + sigma*noise (warm start :330)
hipError_t launch_init_x(const float* noise, const float* base, float sigma, float* x, size_t n, hipStream_t st);

// x += c1*score + c2*z  (universe.py:339,343; z may be null) -- the stand-alone form of the update that ou_enhance fuses
// into the output conv
hipError_t launch_sampler_step(float* x, const float* score, const float* z, float c1, float c2, size_t n,
                               hipStream_t st);

// CompressedMagSTFT forward / inverse (layers/dyn_range_comp.py:51-225).  type: 0 none, 1 exponent, 2 log.
//   forward: x (B, T) -> out (B, 2F, n_frames), F = n_fft/2 + 1, n_frames = 1 + T/hop-ish (center=True)
//   inverse: spec (B, 2F, n_frames) -> y (B, length); `frames` = scratch of B * n_frames * n_fft floats
hipError_t launch_stft_forward(const float* x, const float* win, float* out, int B, int T, int n_fft, int hop,
                               int type, float e, float factor, hipStream_t st);
hipError_t launch_stft_inverse(const float* spec, const float* win, float* frames, float* y, int B, int n_frames,
                               int n_fft, int hop, int type, float e, float factor, int length, hipStream_t st);

// mel front-end (condition.py:92-108): power STFT -> mel fb ; esum[b][frame] = sum_mel mel^2
hipError_t launch_mel(const float* x, const float* win, const float* tw, const float* fb, float* mel, float* esum,
                      int B, int T, int n_fft, int hop, int pad_left, int n_freq, int n_mels, int L, hipStream_t st);
// (`lens`: frames per row of a ragged batch or null -- the mean runs over the row's own frames)
hipError_t launch_mel_scale(const float* esum, float* scale, int B, int L, hipStream_t st, const int* lens = nullptr);

// ---- segmented enhance (ou_segment.hip): long rows cut into overlapping windows of L samples --------------------------------
// Window k of a row starts at k * hop (the last one at T_pad - L); the entries of a call are (row, window) pairs.  Every offset
// into a long row is 64-bit.  Each operation is ONE kernel body, a template over two small by-value descriptions (DESIGN.md
// 4.6.2): "the rows of the call" (SegRowsAlike | SegRowsTable) and "the entries of a group" (SegEntriesArith | SegEntriesList).
struct SegGeom {  // the plan of a row (host side, seg_plan)
  long long T_raw, T_pad, pad_left;
  long long L, hop, overlap;
  long long n_win, n_entries;
};
struct SegRow { long long t_raw, T_pad, pad_left, n_win, first, frames; };  // first: the row's first entry; frames: mel frames
// blocks of a whole-row reduction: one per 256 Ki samples (one block per row up to 16 s at 16 kHz), 1024 at the most
__host__ __device__ inline int seg_nb(long long T_raw) {
  const long long nb = (T_raw + (1ll << 18) - 1) >> 18;
  return (int)(nb < 1 ? 1 : nb > 1024 ? 1024 : nb);
}
// Rows of the call.  Both answer: row(c); stride() of the mix / out rows; noise_stride() of one step's noise rows;
// frame_stride() of the frame-energy rows; blocks(row), the row's own reduce blocks; part_stride(), the blocks the partials of a
// row are laid out for (= the grid of the reductions); zero_tail, whether out[c][t_raw_c, stride) exists and is to be zeroed.
// All rows alike (ou_enhance_segments, ou_enhance_segments_ensemble): the numbers by value; the frame energies are packed (C,
// frames), which is what launch_mel_scale reads.
struct SegRowsAlike {
  SegRow r;
  static constexpr bool zero_tail = false;
  __host__ __device__ SegRow row(long long) const { return r; }
  __host__ __device__ long long stride() const { return r.t_raw; }
  __host__ __device__ long long noise_stride() const { return r.T_pad; }
  __host__ __device__ long long frame_stride() const { return r.frames; }
  __host__ __device__ int blocks(const SegRow&) const { return seg_nb(r.t_raw); }
  __host__ __device__ int part_stride() const { return seg_nb(r.t_raw); }
};
// Rows of lengths of their own (ou_enhance_segments_var): row c has its SegRow in a device table (written by
// launch_seg_upload_rows, 64 rows per launch, by value: capturable, no host memory involved); mix / out and the frame energies
// are (C, row_stride), one step of noise is (C, noise_row_stride).  Grids are sized by the longest row; row c reduces over
// seg_nb(t_raw[c]) blocks whatever the other rows are, so its statistics have the bits of the call on that row alone.
struct SegRowsTable {
  const SegRow* rows;
  long long row_stride, noise_row_stride;  // T_raw_max, T_pad_max
  static constexpr bool zero_tail = true;
  __device__ SegRow row(long long c) const { return rows[c]; }
  __host__ __device__ long long stride() const { return row_stride; }
  __host__ __device__ long long noise_stride() const { return noise_row_stride; }
  __host__ __device__ long long frame_stride() const { return row_stride; }
  __host__ __device__ int blocks(const SegRow& r) const { return seg_nb(r.t_raw); }
  __host__ __device__ int part_stride() const { return seg_nb(row_stride); }
};
// Entries of a group.  Both answer entry(i) = (row, window, length) of the i-th entry of the launch, slot(i), its row in the
// walk's (Bw, T) planes, and hop / overlap of the long rows.
struct SegEnt { long long row, win, len; };
// Arithmetic: entry i is (c, k) = divmod(min(e0 + i, n_entries - 1), n_win) -- row-major over rows alike, the entries past the
// last real one repeating it -- and every entry is L long.
struct SegEntriesArith {
  long long e0, n_entries, n_win, L;
  long long hop, overlap;
  __host__ __device__ SegEnt entry(int i) const {
    long long e = e0 + i;
    if (e > n_entries - 1) e = n_entries - 1;
    const long long c = e / n_win;
    return SegEnt{c, e - c * n_win, L};
  }
  __host__ __device__ int slot(int i) const { return i; }
};
// A list: up to 64 (row, window, length) triples as kernel arguments; entry i is row j0 + i of the walk.  Entries of a long row
// have length S and start at k * hop (the last one at T_pad - S); the single entry of a row with T_pad <= S has length T_pad.
constexpr int kSegEntriesPerLaunch = 64;
struct SegEntryBlock { int row[kSegEntriesPerLaunch]; int win[kSegEntriesPerLaunch]; int len[kSegEntriesPerLaunch]; };
struct SegEntriesList {
  SegEntryBlock blk;
  int j0;
  long long hop, overlap;
  __host__ __device__ SegEnt entry(int i) const { return SegEnt{blk.row[i], blk.win[i], blk.len[i]}; }
  __host__ __device__ int slot(int i) const { return j0 + i; }
};

// stats[c] = {mean, gain, mix_rms, 0} of the padded whole row (pad_normalize_kernel's layout and arithmetic); part: [C]
// [part_stride][3] doubles and [C][part_stride] more behind them: the blocks' maxima, written for every mode but nm.plain() (the
// <true> kernels form it whatever the norm; gain() reads it for max and 2-max).  The caller reserves all four (seg_area).
template <class Rows>
hipError_t launch_seg_stats(const float* mix, double* part, float* stats, const Rows& rows, int C, float level, const NormMode& nm,
                            hipStream_t st);
// esum[c * frame_stride + f] = frame energies of the mel front-end over the whole normalised row (mel_kernel without the mel
// output), f < frames_c <= frames_max
template <class Rows>
hipError_t launch_seg_mel_energy(const float* mix, const float* stats, const float* win, const float* tw, const float* fb,
                                 float* esum, const Rows& rows, int C, int n_fft, int hop, int mel_pad, int n_freq, int n_mels,
                                 long long frames_max, hipStream_t st);
// scale[c] = the mel scale over the row's own frames of esum (C, row_stride): mel_scale_kernel's arithmetic (the rows alike go
// through launch_mel_scale itself)
hipError_t launch_seg_mel_scale_var(const float* esum, float* scale, const SegRow* rows, int C, long long row_stride,
                                    hipStream_t st);
// the first n entries of `ents`: normalised input into rows slot(i) of mixn (.., T), 0 from the entry's own length on, and each
// entry's row mel scale
template <class Rows, class Entries>
hipError_t launch_seg_gather_input(const float* mix, const float* stats, const float* row_mel_scale, float* mixn,
                                   float* mel_scale, const Rows& rows, const Entries& ents, int n, long long T, hipStream_t st);
// Members are a grid dimension of what follows: a group's walk runs E * Bw rows of T columns, row m * Bw + slot = member m of
// the entry; the long rows are (E * C, stride), row m * C + c, one step's noise (E * C, noise_stride), `carry` (E, T): member
// m's window in front of the group.  Rows move in 16-byte accesses from the destination row's first 16-byte boundary on, word by
// word in front of it and behind the last whole quad.
// one step's noise of the first n entries: z[m * Bw + slot][t] = noise[m * C + c][s + t], 0 from the entry's own length on
template <class Rows, class Entries>
hipError_t launch_seg_gather_noise(const float* noise, float* z, const Rows& rows, const Entries& ents, int n, long long T, int Bw,
                                   int E, int C, hipStream_t st);
// crossfade the window outputs y of the first n entries (entry with slot j > 0 and a window in front: with row j - 1 of y, slot
// 0: with `carry`) into the unpadded long rows
template <class Rows, class Entries>
hipError_t launch_seg_stitch(const float* y, const float* carry, float* out, const Rows& rows, const Entries& ents, int n,
                             long long T, int Bw, int E, int C, hipStream_t st);
// keep_rms + peak guard over the E * C long rows in place (universe.py:349-357); row r takes its length and mix_rms from row
// r % C.  part: [E * C][part_stride][2] doubles.  Rows of a table: out[r][t_raw, stride) <- 0 as well.
template <class Rows>
hipError_t launch_seg_post(float* out, double* part, const float* stats, const Rows& rows, int E, int C, int keep_rms,
                           int peak_guard, hipStream_t st);

// the SegRow table and the per-level lengths of a ragged group, from kernel arguments
struct SegVar {
  long long S, hop;  // window length and hop of the long rows
  int tot_ds;
};
constexpr int kSegRowsPerLaunch = 64;
struct SegRowBlock { long long t_raw[kSegRowsPerLaunch]; long long first[kSegRowsPerLaunch]; };
hipError_t launch_seg_upload_rows(SegRow* rows, const SegRowBlock& blk, int n, int off, const SegVar& v, hipStream_t st);
// lens[l * E * Bw + m * Bw + j0 + i] <- len[i] * num_l / den_l for every member m < E: the per-level lengths of a ragged group's
// E * Bw walk rows, from the entry lengths directly (an entry is an already padded window: no pad split as in launch_upload_rows)
hipError_t launch_seg_upload_lens(int* lens, const SegEntryBlock& blk, int n, int j0, int Bw, int E, const LevelSpec& lv,
                                  hipStream_t st);

// Streaming enhance (ou_stream.hip; ou_stream_* in include/ouniverse.h).  All C rows of the stream advance in lockstep, so one
// set of numbers, passed by value, describes every row of a launch.
//   gather: the window [s, s + L) of the stream -> win (C, L), from the ring (C, S) of the last S samples of the P0 pushed before
//           this call and the call's chunk (C, n; rows chunk_stride apart); 0 from T_valid on.  write_ring: the ring then takes
//           the chunk in (L = 0: nothing else happens).  L <= S, s >= P0 - S, T_valid <= P0 + n.
//   emit:   res (C, L)[i0 .. i0 + n_emit) -> out (rows out_stride apart), the first xf <= V samples crossfaded with carry (C, V),
//           clamped to [-1, 1] with `clip`; V_store = V: carry <- the last V samples of res (0: the carry stays).
struct StreamGather {
  long long S, s, L, P0, n, chunk_stride, T_valid;
  int write_ring;
};
struct StreamEmit {
  long long L, V, i0, n_emit, xf, V_store, out_stride;
  int clip;
};
hipError_t launch_stream_gather(const float* chunk, float* ring, float* win, const StreamGather& g, int C, hipStream_t st);
hipError_t launch_stream_emit(const float* res, float* carry, float* out, const StreamEmit& e, int C, hipStream_t st);

// Counter-based sampler noise (ou_noise.hip; the function z(seed, stream, draw, t) is defined in include/ouniverse.h).
// One launch fills up to 64 rows: out[j][col] = col < len[j] ? z(seed, stream[j], draw, t0[j] + col) : 0 for col < cols.
// The per-row values travel as kernel arguments (capturable, no host memory involved).
constexpr int kNoiseRowsPerLaunch = 64;
struct NoiseRows {
  unsigned long long stream[kNoiseRowsPerLaunch];
  long long t0[kNoiseRowsPerLaunch];
  long long len[kNoiseRowsPerLaunch];
};
hipError_t launch_noise_fill(float* out, long long row_stride, long long cols, const NoiseRows& rows, int n_rows,
                             unsigned long long seed, int draw, hipStream_t st);

// Ensemble reduce and row replication (ou_ensemble.hip; ou_enhance_ensemble / ou_ensemble_reduce in include/ouniverse.h).
// members: (E * B, row_stride), member-major (row e * B + b = member e of input b); out: (B, row_stride).
//   stat 0 mean (sequential fp32 sum over e, one division), 1 median (stable rank (E - 1) / 2), 2 signal median (utils/stats.py:
//   22-66: per input the member whose rank position is most often that of the middle member; needs hist [B][E] and pick [B],
//   device ints -- hist is cleared by the call).  len_host: B valid lengths on the host or null (= cols); out is 0 from there on.
// Per-row values travel as kernel arguments, 16 inputs per launch: capturable, no host memory involved.
constexpr int kMaxEnsemble = 32;
constexpr int kEnsRowsPerLaunch = 16;
struct EnsLens { long long len[kEnsRowsPerLaunch]; };
hipError_t launch_ensemble_reduce(const float* members, float* out, int E, int B, long long row_stride, long long cols,
                                  const long long* len_host, int stat, int* hist, int* pick, hipStream_t st);
// entry k: the 4-byte words [0, n[k]) at p[k] are copied to [e n[k], (e + 1) n[k]) for e = 1 .. E - 1
constexpr int kReplicateEntries = 16;
struct ReplicateTable { unsigned* p[kReplicateEntries]; long long n[kReplicateEntries]; };
hipError_t launch_replicate_rows(const ReplicateTable& tab, int n_entries, int E, hipStream_t st);

// Polyphase windowed-sinc resampler over ragged rows (ou_resample.hip; ou_resample in include/ouniverse.h).
//   y[b][j] = sum_t coef[t][p] * x[b][f * orig + first[p] + t]   (j = f * nw + p, x zero outside [0, len[b]), t ascending, fp32 FMA)
// for j < ylen[b]; 0 for ylen[b] <= j < cols.  table (device): int first[nw], then float coef[taps][nw].  orig == nw == 1 and
// table == null: plain copy with the same zeroing.  Per-row values travel as kernel arguments, 64 rows per launch.
constexpr int kResampleRowsPerLaunch = 64;
struct ResampleRows {
  long long len[kResampleRowsPerLaunch];
  long long ylen[kResampleRowsPerLaunch];
};
// consecutive outputs of one row that a workgroup owns for this rate pair (a pure host function: tests pick lengths from it)
int resample_tile(int orig, int nw, int taps);
hipError_t launch_resample(const float* x, long long x_stride, float* y, long long y_stride, long long cols,
                           const ResampleRows& rows, int n_rows, int orig, int nw, int taps, const void* table,
                           hipStream_t st);

// space-to-depth + PReLU for the conditioner's strided "st" convs: y[b][ci*R + k][q] = prelu(x[b][ci][q*R + k])
hipError_t launch_s2d(const float* x, const float* alpha, float* y, int B, int C, int T, int R, hipStream_t st);
// (`lens` of launch_in_conv / launch_out_conv / launch_fir: per-row valid lengths of a ragged batch or null, see ConvArgs::lens)
// Binomial anti-alias FIR (blocks.py:119-130, depthwise 'same' conv with 2r+1 taps), bandwidth-bound:
//   pre  (down path): y = FIR(prelu(x))                       blocks.py:211-215
//   post (up path)  : y = FIR(u) + bias[c] ; y = res ? (y + res)*res_scale : y     blocks.py:219-225, 374-376
hipError_t launch_fir(const float* x, const float* taps, int ntaps, float alpha, int act, const float* bias,
                      const float* res, float res_scale, float* y, int B, int C, int T, hipStream_t st,
                      const int* lens = nullptr);
// y = (a + b + c + d + e) * scale   (nulls skipped)   condition.py:202-206
hipError_t launch_sum(const float* a, const float* b, const float* c, const float* d, const float* e, float scale,
                      float* y, size_t n, hipStream_t st);

// Bidirectional GRU recurrence on a cluster of H/64 workgroups per (batch, direction).
//   gx : (B, 6H, T) input projection incl. biases ; out: (B, 2H, T) ; out = res ? (h + res)*scale : h
// Fused body of a ConvBlock (blocks.py:377-399) for the wide, shallow levels (C = 32 / 64): two or three stride-1
// 'same' convs chained through LDS-resident activation tiles, see conv_chain_kernel.
struct ChainConv {
  const float* wu = nullptr;    // Winograd-domain copy [C][Mp][4 | 8] (conv_chainw_kernel) or null
  const float* w = nullptr;     // packed generic-conv weights [C/CK][KW][CK][Mp]
  const float* bias = nullptr;  // [C]
  float alpha = 0.f;            // PReLU slope applied to this conv's INPUT
  int KW = 3, CK = 32;
};
struct ChainArgs {
  const float* x = nullptr;    // (B, C, T) input of the first fused conv
  float* y = nullptr;          // (B, C, T) block output
  const float* res = nullptr;  // residual added after the last conv: y = (conv + bias + res) * res_scale
  float res_scale = 1.f;
  const float* add = nullptr;  // depth 3 only: y1 = (conv1 + bias + add) * add_scale, then FiLM
  float add_scale = 1.f;
  const float* film = nullptr; // depth 3 only: [B][film_bstride] = gamma[C] | beta[C]
  int film_bstride = 0;
  float* c1_out = nullptr;     // depth 3 only: raw conv1 result, when a caller needs it
  int B = 1, C = 32, T = 0, Mp = 64;
  int depth = 3;               // number of fused convs: 3 = conv1..conv3, 2 = conv2, conv3
  ChainConv cv[3];
  int force_nc = 0;            // tuning: 128 / 256 columns per tile (0: chosen by the launcher)
  int wino = 1;                // minimal-filtering form where there is one (32 channels, depth 3); OU_WINO / OU_CONV_DIRECT < 5: 0
  const int* lens = nullptr;   // ragged batch: valid samples per row at this level (conv_chainw_kernel zeroes every stage behind them)
  unsigned long long* prof = nullptr;
  long long* tstamps = nullptr;  // tuning: per-wave phase cycle counts
};
// Shape check + cost estimate (in cycles) of the best variant; <0 when the shape is not supported.
double chain_cost(const ChainArgs& a, int num_cu, int* nc_out);
hipError_t launch_chain(const ChainArgs& a, int num_cu, hipStream_t st, int* variant);
// the three body convs of a deep-level ConvBlock (k5, k3, k3; batch 1) in one launch; hipErrorInvalidConfiguration = not a
// shape for it.  `bar`: 8 x 40 x 8 zero-initialised bytes that only this kernel touches, `err`: the status words
hipError_t launch_conv_block3(const ConvArgs* cv, unsigned long long* bar, unsigned* err, int num_cu, hipStream_t st,
                              int* cfg_out);

struct GruArgs {
  const float* gx = nullptr;
  const float* whh = nullptr;  // canonical [dir][3H][H] row-major
  const float* bhn = nullptr;
  float* out = nullptr;
  const float* res = nullptr;
  float res_scale = 1.f;
  unsigned long long* xchg = nullptr;  // exchange area: 2B clusters x (2H + 64) granules (see gru_granules())
  unsigned long long* xchg_base = nullptr;  // ring kernel: start and size of the WHOLE area of this GRU layer (filled by
  size_t xchg_granules = 0;                 // launch_gru; a chunked batch advances `xchg` per sub-launch)
  unsigned* epoch = nullptr;           // version 2: {tag epoch, finished-block count} of this exchange area (device)
  int version = 2;                     // 1: polling-wave kernel (memset per launch), 2: ring kernel (epoch tags)
  unsigned* err = nullptr;             // device status word
  long long* tstamps = nullptr;        // per-wave cycle breakdown (tuning only)
  int B = 1, T = 0, H = 0;
  int poll_backoff = 0;  // tuning: 0/1/2 x ~512 cycles of sleep before the first poll
  int agent_stores = 1;  // 1 (default): publish with agent-scope (sc1) stores; 0: plain stores when the cluster shares one XCD
  int dbg = 0;           // experiments (OU_GRU_DBG): bit 0 = no republish safety net, bit 1 = system-scope publishes from the start,
                         // bit 2 = fault injection: one workgroup drops its publishes of step 50
  int share = 1;       // GRU launches that may be resident on one XCD at the same time, this one included (2: another layer on a
                       // side stream; more: other lanes of the process, ou_set_lanes): a launch takes 1 / share of an XCD
  int lanes = 1;       // enhance calls in flight side by side in this process
  int xcd_rot = 0;     // cluster c of the launch is dealt to XCD (c + xcd_rot) % 8
  unsigned long long* prof = nullptr;  // measurement: slot [0] <- ticks before the pass, [16] <- ~ticks behind it (stamp kernels)
  int force_bmax = 0;  // testing: cap the utterances per launch (forces the chunked path at small batches)
  int force_upw = 0;  // tuning: 16 / 32 / 64 hidden units per workgroup (0: chosen from the batch size)
};
hipError_t launch_gru(const GruArgs& a, int num_cu, hipStream_t st);
// utterances one ring-kernel launch can carry with its whole grid resident (0: hidden size not supported)
int gru_ring_batch_cap(int H, int num_cu, int share, int force_upw, int B, int lanes);
// 8-byte exchange granules needed for a batch of B sequences with hidden size H (both kernel generations)
inline size_t gru_granules(int B, int H) { return (size_t)2 * B * (2 * H + 64); }

// Alias-free Snake + Conv1d(C -> 1, k3)  (universe_gan.py:117-126,145-149)
// (`lens` / `lens2`: per-row lengths of a ragged batch on the T and 2T grids, or null)
hipError_t launch_decoupling(const float* aux, const float* alpha_exp, const float* up_k, const float* down_k,
                             const float* w, const float* bias, float* tmp_up, float* out, int B, int C, int T,
                             hipStream_t st, const int* lens = nullptr, const int* lens2 = nullptr);

// Alias-free Snake of a whole (B, C, T) tensor in one launch (ou_snake.hip; ou_snake_act of include/ouniverse.h): row (b, c)
// starts at (b * C + c) * row_stride.  The rows' lengths: `lens_dev` (B ints on the device: the ragged walk), else `rows` (by
// value, B <= kSnakeRowsPerLaunch: the stateless entry point), else every row is T long.
constexpr int kSnakeRowsPerLaunch = 64;
struct SnakeRows {
  int len[kSnakeRowsPerLaunch];
};
int snake_tile();
hipError_t launch_snake_act(const float* x, float* y, int B, int C, int T, long long row_stride, const int* lens_dev,
                            const SnakeRows* rows, const float* exp_alpha, const float* exp_beta, const float* up_k,
                            const float* down_k, hipStream_t st);

// Scoring (ou_metrics.hip; "scoring" in include/ouniverse.h).  Rows of lengths of their own travel as kernel arguments, 64 per
// launch; row0 is the first row of the launch in the call's batch (scratch and results are indexed by row0 + b).
constexpr int kMetRowsPerLaunch = 64;
constexpr int kMetMaxNfft = 1024;  // = OU_METRICS_MAX_NFFT: 32 frames x n_fft floats of LDS
constexpr int kMetMaxSpecs = 8;    // = OU_METRICS_MAX_SPECS
struct MetRows {
  long long len[kMetRowsPerLaunch];
};
struct MetSpecs {  // what met_final_l1_kernel needs of every resolution: partial + offset[i] is (B, tile_stride[i]) doubles
  int n;
  int hop[kMetMaxSpecs], nbins[kMetMaxSpecs];
  long long offset[kMetMaxSpecs], tile_stride[kMetMaxSpecs];
};
inline int met_k4(int n_fft) { return (n_fft + 3) / 4; }                   // k-steps of 4
inline int met_bin_tiles(int n_fft) { return (n_fft / 2 + 1 + 15) / 16; }  // 16-bin tiles (the last one partial)
inline long long met_frame_tiles(long long len, int hop) { return (1 + len / hop + 15) / 16; }
inline size_t met_basis_words(int n_fft) { return (size_t)met_bin_tiles(n_fft) * 2 * met_k4(n_fft) * 64; }
hipError_t launch_met_time(const float* est, const float* ref, long long stride, const MetRows& rows, int n_rows, int row0,
                           float eps, bool scale_invariant, double* tsum, hipStream_t st);
// basis: met_basis_words(n_fft) doubles, window: 4 * met_k4(n_fft) doubles
hipError_t launch_met_basis(double* basis, double* window, int n_fft, hipStream_t st);
// tsum: 8 doubles per row (sum xy, x^2, y^2, (x - y)^2, |alpha x - y|, alpha, -, -), written by launch_met_time.
// l1: | |alpha X| - |Y| | with zero padding; else the squared log-spectral difference with reflect padding.  w2 = sum of window^2
hipError_t launch_met_stft(bool l1, const float* est, const float* ref, long long stride, const MetRows& rows, int n_rows, int row0,
                           long long len_max, const double* basis, const double* window, const double* tsum, int n_fft, int hop,
                           double w2, float eps, bool natural_log, double* partial, long long tile_stride, hipStream_t st);
hipError_t launch_met_final_lsd(const MetRows& rows, int n_rows, int row0, const double* partial, long long tile_stride, int hop,
                                int n_fft, float* out, hipStream_t st);
hipError_t launch_met_final_l1(const MetRows& rows, int n_rows, int row0, const double* partial, const MetSpecs& specs,
                               const double* tsum, float tdw, float* out, hipStream_t st);
hipError_t launch_met_final_sdr(int n_rows, int row0, const double* tsum, float clamp_db, float* out_si_sdr, float* out_snr,
                                hipStream_t st);

// BSS-eval SDR (ou_sdr.hip; ou_sdr of include/ouniverse.h).  partial: (B, tile_stride, 2, L) doubles -- the L autocorrelation
// lags of ref, then the L cross-correlation lags, of every tile of kSdrTile samples; tile_stride >= sdr_tiles(len_max).
// launch_sdr_solve reads tsum word 1 (sum est^2) of launch_met_time.
constexpr int kSdrTile = 2064;     // + 240 = 36 * 64 (ou_sdr.hip)
constexpr int kSdrMaxFilter = 512;  // = OU_SDR_MAX_FILTER: two accumulator tiles of 256 lags
inline long long sdr_tiles(long long len) { return (len + kSdrTile - 1) / kSdrTile; }
hipError_t launch_sdr_corr(const float* est, const float* ref, long long stride, const MetRows& rows, int n_rows, int row0,
                           long long len_max, int L, double* partial, long long tile_stride, hipStream_t st);
hipError_t launch_sdr_solve(const MetRows& rows, int n_rows, int row0, const double* partial, long long tile_stride,
                            const double* tsum, int L, float clamp_db, float* out, hipStream_t st);

// STOI / ESTOI (ou_stoi.hip; ou_stoi of include/ouniverse.h).  Everything behind the caller's fp32 samples is double.  Rows of
// a launch carry two lengths by value: len (samples at fs) and n10 (samples at 10 kHz, = len when fs is 10 kHz).  Scratch of
// row r = row0 + b, F = stoi_frames(longest n10 of the CALL):
//   res     (2, B, res_stride) doubles   est, ref at 10 kHz (absent at fs = 10 kHz: the kernels read the caller's rows)
//   energy  (B, F) doubles               20 log10(||w ref_f|| + eps) of frame f
//   src     (B, F) ints, count (B) ints  the kept frames in order, and how many
//   bands   (B, 2, 15, F) doubles        one-third-octave band values of est, ref over the frames of the compacted signals
//   partial (B, stoi_seg_tiles(F))       sums over kStoiSegTile segments
constexpr int kStoiRowsPerLaunch = 64;
constexpr int kStoiFrame = 256, kStoiHop = 128, kStoiSegment = 30, kStoiBands = 15;
constexpr int kStoiFrameTile = 16;  // STFT frames of both signals per workgroup (= ou_stoi_frame_tile())
constexpr int kStoiSegTile = 16;    // segments per workgroup of stoi_seg_kernel
constexpr int kStoiBinTiles = 14;   // 16-bin tiles of the DFT: 7 from bin 7 (bands 0 .. 11), 7 from bin 109 (bands 12 .. 14)
constexpr size_t kStoiBasisWords = (size_t)kStoiBinTiles * 2 * (kStoiFrame / 4) * 64;
struct StoiRows {
  long long len[kStoiRowsPerLaunch], n10[kStoiRowsPerLaunch];
};
struct StoiSignals {  // est / ref: (B, stride) fp32 at fs; res_est / res_ref: (B, res_stride) doubles at 10 kHz, or null
  const float *est, *ref;
  long long stride;
  const double *res_est, *res_ref;
  long long res_stride;
};
// THE frame rule: frames of 256 at hop 128 start at range(0, n - 256, 128), end exclusive -- a frame that would
// start exactly at n - 256 is not counted.  Both the silent-frame stage and the STFT of the compacted signals count with this.
__host__ __device__ inline long long stoi_frames(long long n) {
  return n > kStoiFrame ? (n - kStoiFrame + kStoiHop - 1) / kStoiHop : 0;
}
// samples of the overlap-add of K kept frames, and the STFT frames it has
__host__ __device__ inline long long stoi_compacted_len(long long K) { return K > 0 ? kStoiHop * (K - 1) + kStoiFrame : 0; }
inline long long stoi_seg_tiles(long long frames) {
  return frames >= kStoiSegment ? (frames - kStoiSegment + 1 + kStoiSegTile - 1) / kStoiSegTile : 0;
}
// table: int first[p] (padded to a multiple of 2), then double coef[taps][p]; output j = f p + ph reads x[f q + first[ph] + t]
hipError_t launch_stoi_resample(const StoiSignals& sig, const StoiRows& rows, int n_rows, int row0, long long n10_max, int p, int q,
                                int taps, const void* table, double* res_est, double* res_ref, hipStream_t st);
// basis: kStoiBasisWords doubles, window: kStoiFrame doubles
hipError_t launch_stoi_basis(double* basis, double* window, hipStream_t st);
hipError_t launch_stoi_energy(const StoiSignals& sig, const StoiRows& rows, int n_rows, int row0, long long n10_max,
                              const double* window, double* energy, long long F, hipStream_t st);
hipError_t launch_stoi_mask(const StoiRows& rows, int n_rows, int row0, const double* energy, long long F, int* src, int* count,
                            hipStream_t st);
hipError_t launch_stoi_stft(const StoiSignals& sig, const StoiRows& rows, int n_rows, int row0, long long n10_max,
                            const double* basis, const double* window, const int* src, const int* count, long long F,
                            double* bands, hipStream_t st);
hipError_t launch_stoi_segments(bool extended, const StoiRows& rows, int n_rows, int row0, long long n10_max, const double* bands,
                                const int* count, long long F, double clip, double* partial, long long seg_stride, float* out,
                                hipStream_t st);

}  // namespace ou
