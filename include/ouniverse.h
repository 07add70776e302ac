/*
 * ouniverse.h -- C ABI of libouniverse.so: MI355X (gfx950) implementation of line/open-universe's
 * `model.enhance` hot path (UNIVERSE / UNIVERSE++ reverse-diffusion sampler, score network, conditioner).
 *
 * The reference is pure Python/PyTorch and has no native interface; these entry points are what an FFI for
 * this path binds.  Each one names the reference interface it replaces (paths relative to the reference
 * checkout, tag 2024_10_08).  INTEGRATION.md shows the reference-side binding (ctypes).
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / hip types (hipStream_t is passed as void*).
 *   - all tensors are fp32, contiguous, (B, C, T) with time innermost, resident on `device`.
 *   - the caller owns every input / output / workspace / packed-weight buffer; the library owns only
 *     the plan.  No allocation and no host synchronisation inside ou_condition / ou_score / ou_enhance:
 *     everything is enqueued on the caller's stream (hipGraph-capturable).
 *   - every function returns OU_OK (0) or a negative OU_E* code; ou_last_error() gives the message.
 *     Nothing throws across the ABI.
 *   - a handle is not re-entrant: one (process, device, stream) at a time.
 */
#ifndef OUNIVERSE_H
#define OUNIVERSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OU_ABI_VERSION 7 /* 7: the bottleneck of the score encoder (ou_config.score.seq_bottleneck, OU_SEQ_*, in the slot the score network never used: additive, the number stays and so does the size of ou_config -- 0 there is the plain GRU model, blob, plan and launches bit for bit); level normalisation modes (ou_set_normalization, OU_NORM_*: additive, the number stays -- a handle nobody sets is normalization_norm 2 with zero_mean, and ou_config is what it was); Snake activations of the ConvBlock body convs (ou_config tail score_enc_act .. cond_dec_act, OU_ACT_SNAKEBETA, ou_snake_act, ou_snake_tile: additive, the number stays -- a zeroed tail is the PReLU model); ensembles of segmented rows (ou_segments_ensemble_workspace_bytes, ou_enhance_segments_ensemble: additive, the number stays); segmented enhance of rows with lengths of their own (ou_segment_groups, ou_segments_var_workspace_bytes, ou_enhance_segments_var: additive, the number stays); ensembles in the library (ou_enhance_ensemble, ou_ensemble_workspace_bytes, ou_ensemble_reduce, ou_ensemble_reduce_scratch_bytes; option ens_share); existing entry points unchanged; 6: counter-based sampler noise (ou_set_noise_source, ou_noise_scratch_bytes, ou_noise_fill); existing entry points unchanged; 5: ou_enhance_var (batches whose rows have lengths of their own), workspace header carries the per-row geometry; ou_set_option / ou_get_option replace every OU_* environment switch (the library reads no environment variable), ou_config.fir_fold; 4: the packed blob carries a bf16-split weight copy (conv_split_kernel); 3: a Winograd-domain copy (round 5), ou_set_lane_batch, ou_lane_capacity */

enum {
  OU_OK = 0,
  OU_EINVAL = -1,    /* bad argument (Python side raises ValueError) */
  OU_ENOTIMPL = -2,  /* unsupported configuration (NotImplementedError) */
  OU_EMISSING = -3,  /* tensor missing from checkpoint (KeyError) */
  OU_ESHAPE = -4,    /* tensor shape mismatch */
  OU_EHIP = -5,      /* HIP runtime error */
  OU_ENOMEM = -6,    /* workspace too small */
  OU_ESYNC = -7      /* device-side timeout flag raised (GRU cluster exchange) */
};

enum { OU_KIND_UNIVERSE = 0, OU_KIND_UNIVERSE_GAN = 1 };
enum { OU_ACT_NONE = 0, OU_ACT_PRELU = 1, OU_ACT_SNAKE = 2, OU_ACT_SNAKEBETA = 3 };
/* act_type "none" in the four *_act fields at the end of ou_config, where 0 has to mean "not set" = PReLU */
#define OU_ACT_IDENTITY (-1)
/* ou_config.score.seq_bottleneck: seq_model / encoder_gru_conv_sandwich of ScoreNetwork */
/* (1 is taken: a caller that filled `score` from its conditioner block left encoder_gru_residual = 1 there, which never meant
 * anything and still means the plain GRU) */
enum { OU_SEQ_GRU = 0, OU_SEQ_NONE = 2, OU_SEQ_GRU_SANDWICH = 3 };
/* normalization_norm (utils/norm.py:31-44) for ou_set_normalization: 2 | "max" | "2-max" */
enum { OU_NORM_2 = 0, OU_NORM_MAX = 1, OU_NORM_2MAX = 2 };

#define OU_MAX_RATES 8 /* size of ou_net_config.rate_factors (the ABI's layout); a model may have at most 4, see below */

/* One network's hyper-parameters == the constructor arguments of
 * ScoreNetwork (networks/universe/score.py:214-232) / ConditionerNetwork (condition.py:274-293).
 * Accepted (ou_packed_bytes / ou_packer_create / ou_create answer OU_ENOTIMPL with a message naming the field otherwise):
 *   n_rates 1 .. 4, every factor in [2, 8], prod(rate_factors) <= 496 with more than one factor; fb_kernel_size 1, 3, 5, 7;
 *   n_channels even, <= 64, with n_channels * 2^n_rates / 2 (the GRU's hidden size) a multiple of 64; noise_cond_dim a
 *   multiple of 64 in [64, 1024]; n_rff 1 .. 64 (random Fourier features); n_mels even, <= 256;
 *   n_mel_oversample * prod(rate_factors) (= n_fft) <= 2048; rate_factors, n_channels, fb_kernel_size and extra_conv_block the
 *   same in the score and the condition network. */
typedef struct ou_net_config {
  int32_t n_rates;
  int32_t rate_factors[OU_MAX_RATES];
  int32_t n_channels;
  int32_t fb_kernel_size;
  int32_t n_rff;
  int32_t noise_cond_dim;
  int32_t extra_conv_block;
  int32_t use_weight_norm;
  int32_t use_antialiasing;
  int32_t time_embedding_simple; /* 1: SimpleTimeEmbedding (sigma_block.py:60-78), 0: SigmaBlock RFF (:36-57) */
  int32_t n_mels;                /* conditioner only */
  int32_t n_mel_oversample;      /* conditioner only */
  /* One slot, two readings.  ou_config.cond: encoder_gru_residual of ConditionerNetwork.  ou_config.score, where that argument does
   * not exist and every caller so far left 0 (or 1, copied from its conditioner block; ignored then, the plain GRU now): what sits in the bottleneck of the score encoder (seq_model and
   * encoder_gru_conv_sandwich of ScoreNetwork, score.py:32-36, 81-102, 113-123) -- OU_SEQ_GRU (0; also 1) the bidirectional GRU, OU_SEQ_NONE
   * nothing at all (no GRU tensor of the score network is asked for or packed), OU_SEQ_GRU_SANDWICH a ConvBlock(oc) in front of
   * that GRU and one behind it (encoder.conv_block1 / conv_block2; the reference knows the sandwich in its gru branch only, so
   * there is no fourth state).  Any other value is OU_ENOTIMPL naming the field.  The plan and the blob depend on it: same value
   * for the packer and ou_create.  sizeof(ou_config) is what it was. */
  union {
    int32_t encoder_gru_residual; /* conditioner */
    int32_t seq_bottleneck;       /* score network: OU_SEQ_* */
  };
} ou_net_config;

/* == config.model of the reference (the yaml files under config/model/), inference-relevant part;
 * replaces hydra `instantiate(config.model)` at inference_utils/model_loader.py:114. */
typedef struct ou_config {
  int32_t abi_version; /* OU_ABI_VERSION */
  int32_t kind;        /* OU_KIND_* : Universe (universe.py:44) / UniverseGAN (universe_gan.py:60) */
  int32_t fs;
  float level_db;      /* normalization_kwargs.level_db */
  int32_t has_edm;     /* edm: {noise: ...} present (universe.py:85-95) */
  float edm_noise;
  double sigma_min, sigma_max; /* diffusion.* (geometric schedule, universe.py:380-386) */
  int32_t use_signal_decoupling; /* universe_gan.py:117-126 */
  int32_t signal_decoupling_act; /* OU_ACT_* */
  ou_net_config score;
  ou_net_config cond;
  int32_t has_edm_data_level; /* edm.data_level_db given (universe.py:176-178); 0: sigma_data follows level_db */
  float edm_data_level_db;
  int32_t fir_fold; /* packing choice, not a reference hyper-parameter: bit 0 / bit 1 = fold the binomial anti-alias FIR of the
                     * down / up rate-change convs (blocks.py:213-227) into their weights (one launch less per rate change for 3x
                     * that conv's FLOPs; slower on MI355X, default 0).  The plan and the blob depend on it: same value for the
                     * packer and ou_create. */
  int32_t no_split_copy; /* packing choice: 1 = leave the bf16-split weight copy (conv_split_kernel: a quarter of the blob, PP16
                          * 162 of 648 MB) out -- for handles that never run a batch of 8 or more utterances per call (the
                          * launcher's rule selects that kernel from batch 8 / 16 on).  Same value for the packer and ou_create. */
  /* encoder_act_type / decoder_act_type of ScoreNetwork (score.py:223-224) and ConditionerNetwork (condition.py:283-284): the
   * activation in front of conv1 .. conv3 of every ConvBlock of that half (blocks.py:176-187, 289-312; rate-change convs, st
   * convs and the conditioner's mel ConvBlock always keep their PReLU).  0 (a zeroed tail: every caller older than these
   * fields) or OU_ACT_PRELU: PReLU; OU_ACT_SNAKE / OU_ACT_SNAKEBETA: bigvgan.AliasFreeSnake(alpha_logscale=True[, beta=True]);
   * OU_ACT_IDENTITY: "none".  The plan and the blob depend on them: same values for the packer and ou_create. */
  int32_t score_enc_act, score_dec_act, cond_enc_act, cond_dec_act;
} ou_config;

typedef struct ou_packer ou_packer;
typedef struct ou_handle ou_handle;
typedef void* ou_stream_t; /* hipStream_t */

const char* ou_version(void);
/* Message of the last error on this handle / packer (NULL handle: last global error). */
const char* ou_last_error(const ou_handle* h);
const char* ou_packer_last_error(const ou_packer* p);

/* ---- weights: replaces model.load_state_dict + EMA copy + (never called) remove_weight_norm ------------
 * model_loader.py:117-132, universe.py:841-865, blocks.py:36-50.
 * The packer takes tensors under the reference's state-dict keys (host fp32), folds weight-norm
 * (w = g*v/||v||), keeps the binomial anti-alias FIR of the rate-change convs (blocks.py:213-227) as separate taps, lays
 * every matrix out for the gfx950 kernels and returns one contiguous fp32 blob whose layout depends on the
 * config only.  The blob is what gets broadcast over RCCL and handed to ou_create(). */
int ou_packer_create(const ou_config* cfg, ou_packer** out);
int ou_packer_set(ou_packer* p, const char* key, const float* data, const int64_t* shape, int32_t ndim);
int ou_packer_finish(ou_packer* p, const float** blob_host, size_t* nbytes); /* blob owned by the packer */
void ou_packer_destroy(ou_packer* p);
int ou_packed_bytes(const ou_config* cfg, size_t* nbytes);

/* ---- model: replaces load_model()'s returned module (model_loader.py:62-137) ----------------------------
 * `weights_dev`: device pointer to the packed blob (caller-owned, must outlive the handle). */
int ou_create(const ou_config* cfg, const void* weights_dev, size_t nbytes, int32_t device, ou_handle** out);
void ou_destroy(ou_handle* h);

/* Workspace needed for a batch of B signals of padded length T (T % prod(rate_factors) == 0). */
int ou_workspace_bytes(const ou_handle* h, int32_t B, int32_t T, size_t* nbytes);
/* Once per workspace buffer, before its first use (and after every change of B): clears the header -- the sticky
 * device status word and the GRU exchange granules (whose tags continue from launch to launch, so the forward calls
 * themselves enqueue no memset).  Enqueued on `stream`.  The handle remembers (buffer, size, B): ou_condition,
 * ou_score and ou_enhance return OU_EINVAL for a workspace that was not prepared for their batch size.  A buffer
 * prepared for (B, T) serves every shorter length of the same batch size too (the header's layout depends on B alone):
 * a set of utterances of different lengths -- the reference CLI's loop over a directory, bin/enhance.py:173-192 -- runs on
 * ONE workspace sized for the longest; a buffer that is too small for a call is refused with OU_ENOMEM. */
int ou_workspace_init(ou_handle* h, int32_t B, int32_t T, void* ws, size_t ws_bytes, ou_stream_t stream);

/* Sampler constants, universe.py:301-311: sigma[n] (fp32, n = 0..n_steps-1), eta, beta. */
int ou_schedule(const ou_config* cfg, int32_t n_steps, double epsilon, float* sigma_out, double* eta, double* beta);

/* condition_model(mix, x_wav=mix, train=True)  -- universe.py:314-316 / condition.py:346-377.
 * `mix_norm`: (B,1,T) normalised mixture.  Results (cond[5], aux signal, latent) stay in the workspace
 * (see ou_tensor()) and are consumed by ou_score(). */
int ou_condition(ou_handle* h, const float* mix_norm, int32_t B, int32_t T, void* ws, size_t ws_bytes,
                 ou_stream_t stream);

/* score_model(x, sigma, cond) -> score  -- universe.py:286,197-209 (EDM wrapper) / score.py:277-297.
 * `sigma_host`: B floats on the host.  Requires a preceding ou_condition() on the same workspace. */
int ou_score(ou_handle* h, const float* x, const float* sigma_host, float* score_out, int32_t B, int32_t T,
             void* ws, size_t ws_bytes, ou_stream_t stream);

/* aux_to_wav(aux_signal) -- universe_gan.py:145-149 (alias-free Snake -> Conv1d(C0->1,k3)).
 * Reads the conditioner's aux signal from the workspace; writes (B,1,T). */
int ou_aux_to_wav(ou_handle* h, float* wav_out, int32_t B, int32_t T, void* ws, size_t ws_bytes,
                  ou_stream_t stream);

/* Flags of ou_enhance */
#define OU_ENH_KEEP_RMS 1u       /* universe.py:352-354 */
#define OU_ENH_USE_AUX_SIGNAL 2u /* universe.py:317-319 */
#define OU_ENH_NO_PEAK_GUARD 4u  /* skip universe.py:356-357 (debug) */
#define OU_ENH_SERIAL 8u         /* everything on the caller's stream, no side streams inside the call: the form to capture
                                  * into a hipGraph (a captured fork / join replays slower than the serial chain) */

/* Universe.enhance(mix, n_steps, epsilon, rng=...) -- universe.py:231-375, for a (B, T_raw) batch.  An input whose padded length
 * would make a per-row plane of the walk reach 2^32 bytes (its kernels address a plane with 32-bit descriptors) is refused with
 * OU_EINVAL before anything is launched -- ou_enhance_segments takes it:
 * pad (:219-223) -> normalize (utils/norm.py:47-87) -> conditioner -> x0 = sigma_0 * noise[0] ->
 * N-1 x { score; x += sigma_n^2*eta*score + beta*sigma_{n+1}*noise[n+1] } -> last clean step ->
 * unpad -> [keep_rms] -> peak guard.  Ensemble replication / reduction stays with the caller of THIS entry point
 * (ou_enhance_ensemble below does both inside the library).
 *   mix, out : (B, T_raw) device
 *   noise    : (n_steps - warm_start, B, T_pad) standard-normal, device, in the reference's draw order
 *              (x0, z_0 .. z_{N-2}); T_pad = T_raw + (tot_ds - T_raw % tot_ds).  NULL when a noise source is set
 *              (ou_set_noise_source)
 *   sigma_host: n_steps floats or NULL (then computed as ou_schedule does)
 *   warm_start: -1, or the step index to start from with x = aux_to_wav(aux) + noise (universe.py:328-331) */
int ou_enhance(ou_handle* h, const float* mix, float* out, const float* noise, int32_t B, int32_t T_raw,
               int32_t n_steps, double epsilon, const float* sigma_host, int32_t warm_start, uint32_t flags,
               void* ws, size_t ws_bytes, ou_stream_t stream);

/* The same for a batch whose rows have lengths of their OWN ("exact batching"; extension).  The reference has no such call:
 * its CLI runs a directory one file at a time (bin/enhance.py:173-192) and its collator zero-pads a batch WITHOUT a mask
 * (datasets/datamodule.py:24-42), so that the padding takes part in the normalisation, the mel norm, the conv halos and the GRU
 * -- every row then differs from what the file would give alone.  Here row b IS the call on that utterance alone, batched:
 * its own pad() split (universe.py:219-223: pad_b = tot_ds - t_raw[b] % tot_ds, pad_b / 2 in front), its own mean / std
 * (utils/norm.py:47-87) and mel norm (condition.py:105-106) over its own padded length, 'same' zero padding of every conv /
 * FIR right behind its own last sample on every level, GRU passes over its own frames (the backward pass starts at its own
 * last frame with h = 0), its own RMS restore and peak guard.  Results agree with the one-by-one loop to fp32 round-off
 * (the kernels a batch selects differ from the batch-1 ones; tests: >= 100 dB).
 *   mix, out : (B, T_raw_max) device; row b holds t_raw[b] samples, the rest of the row is ignored (mix) / zeroed (out)
 *   t_raw    : B lengths on the HOST, 1 <= t_raw[b] <= T_raw_max = max_b t_raw[b]
 *   noise    : (n_steps - warm_start, B, T_pad_max) device, T_pad_max = T_raw_max + (tot_ds - T_raw_max % tot_ds); row b
 *              uses its first t_raw[b] + pad_b columns (what a call on that row alone would draw), the rest is ignored
 *   workspace: as for ou_enhance with (B, T_pad_max).  A batch whose rows all have T_raw_max samples takes the plain path. */
int ou_enhance_var(ou_handle* h, const float* mix, float* out, const float* noise, int32_t B, int32_t T_raw_max,
                   const int32_t* t_raw, int32_t n_steps, double epsilon, const float* sigma_host, int32_t warm_start,
                   uint32_t flags, void* ws, size_t ws_bytes, ou_stream_t stream);

/* ---- ensembles (universe.py:261-264, 359-368: `ensemble=E` runs E samples of every input and returns their mean, median or
 * "signal median", utils/stats.py:22-66) -------------------------------------------------------------------------------------
 * Members are MEMBER-MAJOR everywhere: row e * B + b is member e of input b -- the order torch.stack([mix] * E) produces
 * (universe.py:261-264) and the order of the stream ids of the counter-based noise (member e: the input's id + (e << 48)).
 *
 * ou_enhance_ensemble = ou_enhance / ou_enhance_var (t_raw given) of the E * B member rows, with
 *   - the conditioner -- whose result depends on the input, not on the noise -- run ONCE over the B inputs and its results
 *     replicated to the rows of the other members (option `ens_share`, default 1; 0: the conditioner runs over all E * B rows,
 *     the arithmetic of the call on the replicated batch).  A B-row conditioner pass may select other kernels than an
 *     (E * B)-row one: the members agree with those of `ens_share` = 0 to fp32 round-off (tests: >= 100 dB), not bit for bit;
 *   - the sampler loop at E * B rows, as one chain on the caller's stream (no side streams inside the call);
 *   - unpad, keep_rms and the peak guard per member row, as the reference applies them before the reduce; keep_rms restores
 *     the RMS of the member's own input b (for B = 1 the reference's result; for B > 1 the reference fails to broadcast,
 *     universe.py:354, and this per-input definition is the extension);
 *   - the reduce over e into `out`.
 *   mix, out    : (B, T_raw_max) device, the row conventions of ou_enhance_var (t_raw NULL: every row has T_raw_max samples)
 *   members_out : NULL, or (E * B, T_raw_max) device: the post-processed members (rows of a ragged batch 0 behind their end)
 *   noise       : (n_steps - max(warm_start, 0), E * B, T_pad_max) device; NULL when a noise source is set -- its n_streams
 *                 must then equal E * B and its scratch hold two (E * B, T_pad_max) planes
 *   stat        : OU_ENS_MEAN     fp32 sum over e = 0 .. E - 1 in that order, then one division by E
 *                 OU_ENS_MEDIAN   the value of stable rank (E - 1) / 2: torch.median's lower median
 *                 OU_ENS_SIGNAL_MEDIAN  per input ONE member: per sample the rank position of the member whose index is nearest
 *                   E / 2 (both neighbours for odd E, the smaller position wins), histogram of the positions over the input's
 *                   own samples, first maximum -> that member's row.  rank(c) = #{x_j < x_c} + #{j < c : x_j == x_c}
 *   flags       : OU_ENH_KEEP_RMS, OU_ENH_NO_PEAK_GUARD; OU_ENH_USE_AUX_SIGNAL is refused (OU_EINVAL: without noise all members
 *                 are equal); OU_ENH_SERIAL is implied
 *   workspace   : ou_ensemble_workspace_bytes(h, B, T_pad_max, E) bytes -- the walk's workspace for E * B rows plus the member
 *                 planes, a B x E histogram and B picks -- prepared with ou_workspace_init(h, E * B, T_pad_max, ..); a buffer
 *                 prepared for another batch size is refused (OU_EINVAL)
 * OU_EINVAL for E < 1, E > OU_MAX_ENSEMBLE, an unknown stat; the length guard of ou_enhance applies unchanged (per-row planes
 * do not grow with E).  Inputs are assumed finite.  No float atomics: results do not depend on scheduling. */
#define OU_MAX_ENSEMBLE 32
enum { OU_ENS_MEAN = 0, OU_ENS_MEDIAN = 1, OU_ENS_SIGNAL_MEDIAN = 2 };
int ou_ensemble_workspace_bytes(const ou_handle* h, int32_t B, int32_t T_pad_max, int32_t E, size_t* nbytes);
int ou_enhance_ensemble(ou_handle* h, const float* mix, float* out, float* members_out, const float* noise, int32_t B,
                        int32_t T_raw_max, const int32_t* t_raw, int32_t E, int32_t stat, int32_t n_steps, double epsilon,
                        const float* sigma_host, int32_t warm_start, uint32_t flags, void* ws, size_t ws_bytes,
                        ou_stream_t stream);
/* The reduce alone (stateless: no handle), for bindings that keep their own sampler loop:
 *   members: (E * B, row_stride) device, member-major; out: (B, row_stride) device; only the first `cols` columns of a row are
 *   touched; len_host: NULL, or B valid lengths on the HOST (0 <= len[b] <= cols) -- nothing is read past len[b], and
 *   out[b][len[b] .. cols) = 0.  scratch (OU_ENS_SIGNAL_MEDIAN only; device, >= ou_ensemble_reduce_scratch_bytes): the
 *   histogram, int32 [B][E], then the picked member of every input, int32 [B].  Enqueued on `stream`. */
size_t ou_ensemble_reduce_scratch_bytes(int32_t E, int32_t B);
int ou_ensemble_reduce(const float* members, float* out, int32_t E, int32_t B, int64_t row_stride, int64_t cols,
                       const int64_t* len_host, int32_t stat, void* scratch, size_t scratch_bytes, ou_stream_t stream);

/* ---- segmented enhance: recordings of any length in bounded memory (extension; the reference runs a whole file per call)
 * A long row is cut into overlapping windows that run as one batch through the walk of ou_enhance; whatever the reference
 * computes over the whole utterance is still computed over the whole row:
 *   - pad split, mean and gain (utils/norm.py:47-87) and mix_rms over the whole padded row; window k's input is exactly
 *     xn[s_k : s_k + L] of the normalised padded row xn;
 *   - ONE mel normalisation per row (condition.py:105-106) over the mel frames of the whole row;
 *   - window k's noise is noise[..., s_k : s_k + L] of the whole-row noise, so a generator advances as in ou_enhance;
 *   - the window outputs are crossfaded (complementary raised cosine over the last `overlap` samples of window k; the weights
 *     sum to 1) into the padded row, then unpad, keep_rms (whole-row mix_rms) and the peak guard (max over the whole row).
 * Only the network's receptive field and the bidirectional GRUs see a window instead of the row.  A row that fits into one
 * window gives the ou_enhance result.
 *
 * Plan (pure host function of T_raw, tot_ds, segment, overlap): segment and overlap are rounded down to multiples of tot_ds,
 * 0 <= overlap <= segment / 2.  T_pad = T_raw + (tot_ds - T_raw % tot_ds).  T_pad <= segment: one window [0, T_pad).  Else every
 * window has L = segment samples, window k starts at k * (segment - overlap), the last one at T_pad - L (shifted to stay inside);
 * the crossfade between windows k and k + 1 covers [s_k + L - overlap, s_k + L), and core k (the samples where window k has
 * weight >= 1/2) runs from the middle of one crossfade to the next: the cores tile [0, T_pad).
 * `capacity`: entries of the four arrays (all four may be NULL: then only n_windows / overlap_used / T_pad are returned). */
int ou_segment_plan(int32_t tot_ds, int64_t T_raw, int32_t segment, int32_t overlap, int32_t capacity, int64_t* starts,
                    int32_t* lengths, int64_t* core_begin, int64_t* core_end, int32_t* n_windows, int32_t* overlap_used,
                    int64_t* T_pad);
/* Workspace of ou_enhance_segments for C rows of T_raw samples: the workspace of the walk for (batch, length) -- batch <=
 * max_batch windows of `length` samples per group -- plus a small area for the whole-row statistics (C rows x 24 KiB), one
 * step of gathered noise (batch x length floats) and one carried window.  It depends on C, max_batch and segment, NOT on T_raw
 * (beyond T_raw's share of a segment).  Prepare the buffer with ou_workspace_init(h, batch, length, ws, nbytes, stream). */
int ou_segments_workspace_bytes(const ou_handle* h, int32_t C, int64_t T_raw, int32_t segment, int32_t overlap,
                                int32_t max_batch, size_t* nbytes, int32_t* batch, int32_t* length);
/* Universe.enhance of C independent rows of T_raw samples, in windows (see above):
 *   mix, out : (C, T_raw) device (out also serves as scratch for the whole-row mel frame energies before the first window)
 *   noise    : (n_steps - max(warm_start, 0), C, T_pad) standard-normal, device, the draw order of ou_enhance (x0, z_0 ..
 *              z_{N-2}): plane 0 is the initial draw, plane d - warm_start is draw d = n + 1 of the absolute step n.  A noise
 *              source draws 0, warm_start + 1, warm_start + 2, .. at the positions s_k + i.
 *   flags    : OU_ENH_KEEP_RMS, OU_ENH_NO_PEAK_GUARD, OU_ENH_USE_AUX_SIGNAL
 *   warm_start: -1, or 0 <= k < n_steps (OU_EINVAL otherwise)
 * The two cheap modes of ou_enhance, per window.  With wav_k = aux_to_wav(conditioner(xn[s_k : s_k + L])), the decoupling layer
 * over the window's own aux signal (the whole row's mel scale, as above):
 *   OU_ENH_USE_AUX_SIGNAL : window k's result is wav_k; no score pass runs, no noise is read (`noise` and a noise source as in
 *                           ou_enhance under this flag: `noise` may be NULL, a set source still needs n_streams == C).  Same
 *                           crossfade; unpad, keep_rms and the peak guard over the whole row.
 *   warm_start = k        : x_k = wav_k + sigma[k] * z0[s_k : s_k + L], then the steps k .. n_steps - 1, stitch and post as above.
 * Both need the snake signal-decoupling layer (UNIVERSE++): OU_ENOTIMPL otherwise, with the message of ou_enhance, decided on
 * the host before anything is launched.  The `segment too long` guard then counts the layer's (C0, 2 L) plane as ou_enhance
 * does.  Workspace: ou_segments_workspace_bytes answers what it answers for a cold start and a buffer of exactly that size runs
 * both modes (ou_workspace_bytes reserves the layer's scratch for the walk's rows); the aux exit gets no smaller workspace.
 * A row that fits one window is the ou_enhance call with the same warm_start / flags, bit for bit.  ou_tensor "wav": the last
 * group's wav rows.  With warm_start == -1 and without the flag the call enqueues what it always has.
 * Everything is enqueued on `stream` (no side streams). */
int ou_enhance_segments(ou_handle* h, const float* mix, float* out, const float* noise, int32_t C, int64_t T_raw,
                        int32_t segment, int32_t overlap, int32_t max_batch, int32_t n_steps, double epsilon,
                        const float* sigma_host, int32_t warm_start, uint32_t flags, void* ws, size_t ws_bytes,
                        ou_stream_t stream);

/* ---- segmented enhance of rows with lengths of their own (extension): ou_enhance_segments for a batch in which every row has
 * its own length, as ou_enhance_var is to ou_enhance.  Row c is, by definition, ou_enhance_segments(C = 1, T_raw = t_raw[c]) on
 * its own noise: its own pad split, whole-row mean / gain / mix_rms (bit-identical: the row's reductions use the block partition
 * of the call on that row alone), its own mel scale, crossfades only between its own consecutive windows, keep_rms and the peak
 * guard over its own samples.  What changes is the grouping: the windows of ALL rows share the window groups.
 *
 * Groups (pure host function).  Row c's windows are those of ou_segment_plan(tot_ds, t_raw[c], segment, overlap).  With S =
 * segment rounded down to a multiple of tot_ds:
 *   class FULL : every window (length S) of the rows with T_pad_c > S, in row-major order;
 *   class SHORT: the single window (length T_pad_c <= S) of every other row, in input order.
 * The entry list is FULL, then SHORT.  A group is up to `batch` consecutive entries of ONE class; batch = the larger of the two
 * classes' even spread, ceil(n / ceil(n / max_batch)) for a class of n entries, so batch <= max_batch and a class of n entries
 * makes ceil(n / batch) groups.  The walk always runs `batch` rows: a last partial group is filled by repeating its last real
 * entry (as ou_enhance_segments does).  A group is `ragged` when its entries differ in length -- SHORT groups only; it runs
 * through the ragged walk of ou_enhance_var at the length of its longest entry (entries are already padded windows: they are
 * zero from their own length on, on every level), every other group through the plain walk at its entries' length.  length =
 * the longest entry = min(S, max T_pad_c).  When all rows have one length, batch, length and the entry order are those of
 * ou_enhance_segments for (C, T_raw).
 * entry_row / entry_window / entry_length: `capacity` >= n_entries values; group_first / group_ragged: one per group (group g
 * holds the entries from group_first[g] up to group_first[g] + batch, the next group's first entry or the end of its class,
 * whichever comes first; `capacity` covers them too, n_groups <= n_entries).  All five may be NULL: only the counts are returned. */
int ou_segment_groups(int32_t tot_ds, int32_t C, const int64_t* t_raw, int32_t segment, int32_t overlap, int32_t max_batch,
                      int32_t capacity, int32_t* entry_row, int32_t* entry_window, int32_t* entry_length, int32_t* group_first,
                      int32_t* group_ragged, int32_t* n_entries, int32_t* n_groups, int32_t* batch, int32_t* length);
/* Workspace of ou_enhance_segments_var: the walk's workspace for (batch, length) plus the segment area -- the C rows'
 * statistics, scales and partials (24 KiB per row), a per-row geometry table, one step of gathered noise (batch x length floats)
 * and one carried window.  It depends on C, max_batch and segment, and on the lengths only through `length` (and through
 * `batch` where fewer than max_batch entries exist).  Prepare the buffer with ou_workspace_init(h, batch, length, ..). */
int ou_segments_var_workspace_bytes(const ou_handle* h, int32_t C, const int64_t* t_raw, int32_t segment, int32_t overlap,
                                    int32_t max_batch, size_t* nbytes, int32_t* batch, int32_t* length);
/*   mix, out : (C, T_raw_max) device; row c holds t_raw[c] samples, the rest of a mix row is ignored and the rest of an out row
 *              is zeroed (the ou_enhance_var convention; out also serves as scratch for the mel frame energies)
 *   t_raw    : HOST, C lengths, 1 <= t_raw[c] <= T_raw_max = the longest (OU_EINVAL otherwise, before anything is launched)
 *   noise    : (n_steps - max(warm_start, 0), C, T_pad_max) device; row c uses its first T_pad_c columns (what the call on row c
 *              alone would draw).  With a noise source: NULL, n_streams == C, window k of row c draws at t = s_k + i from the
 *              stream of row c.
 *   flags, warm_start: as ou_enhance_segments, both cheap modes included.  In a ragged group the window's wav is zero behind the
 *              entry's own length (the decoupling layer takes the entries' lengths), so x_k and the stitched wav are too.  Rows
 *              of one length are ou_enhance_segments with the same warm_start / flags, bit for bit.
 * Everything is enqueued on `stream`: no allocation, no host synchronisation, no side streams; the per-row geometry and every
 * group's entries reach the device as kernel arguments (capturable). */
int ou_enhance_segments_var(ou_handle* h, const float* mix, float* out, const float* noise, int32_t C, int64_t T_raw_max,
                            const int64_t* t_raw, int32_t segment, int32_t overlap, int32_t max_batch, int32_t n_steps,
                            double epsilon, const float* sigma_host, int32_t warm_start, uint32_t flags, void* ws,
                            size_t ws_bytes, ou_stream_t stream);

/* ---- ensembles of segmented rows (extension): ou_enhance_ensemble for rows of any length.  Member e of row c is, by definition,
 * ou_enhance_segments(C = 1) of row c on that member's own noise -- whole-row statistics and mel scale of row c, crossfades only
 * between consecutive windows of the row, keep_rms (the mix_rms of row c) and the peak guard over the member row's own samples --
 * and out[c] is ou_ensemble_reduce over the E post-processed members of row c.  What changes is how the work is grouped.
 *
 * Everything is MEMBER-MAJOR: member row e * C + c.
 *   mix, out : (C, T_raw) device (out also serves as scratch for the whole-row mel frame energies before the first window)
 *   members  : (E * C, T_raw) device, caller-owned and REQUIRED: the post step runs over whole member rows before the reduce (as
 *              in the reference, universe.py:352-368), so every member row has to exist whole.  THIS IS THE ONE PART OF THE CALL
 *              THAT GROWS WITH THE RECORDING (E x the output); the workspace does not depend on T_raw, as for ou_enhance_segments.
 *   noise    : (n_steps, E * C, T_pad) device; NULL when a noise source is set -- its n_streams must then equal E * C, and stream
 *              e * C + c belongs to that member row.  Window k of a member row reads the positions s_k + i of that row's noise.
 *   stat     : as ou_enhance_ensemble;  flags: OU_ENH_KEEP_RMS, OU_ENH_NO_PEAK_GUARD;  warm_start must be -1 (the cheap modes of
 *              ou_enhance_segments are not carried into the ensemble forms: OU_EINVAL).
 *
 * Groups (pure host function).  The windows are those of ou_segment_plan, the entry list is row-major (c, k) as in
 * ou_enhance_segments.  Bw = ceil(n / ceil(n / floor(max_batch / E))) entries per group for n = C * n_windows entries, and the
 * walk runs batch = E * Bw <= max_batch rows: walk row e * Bw + j is member e of entry e0 + j.  A short last group repeats its
 * last real entry per member (the filler of member e repeats member e's window and noise; fillers are never stitched).  The
 * conditioner runs ONCE over the Bw inputs of a group and its results are replicated to the other members' rows (option
 * `ens_share`, default 1, as in ou_enhance_ensemble; 0: the input is gathered E times and the conditioner runs over all E * Bw
 * rows -- the arithmetic of ou_enhance_segments on E stacked copies of the rows).  A Bw-row conditioner pass, and a walk of
 * another batch size, may select other kernels: members agree with the single-row calls to fp32 round-off, not bit for bit;
 * E = 1 is ou_enhance_segments bit for bit.
 *
 * Workspace: ou_segments_ensemble_workspace_bytes returns batch = E * Bw and length; prepare the buffer with
 * ou_workspace_init(h, batch, length, ..).  Behind the walk's workspace it holds C rows of statistics, E * C rows of post
 * partials, E * Bw * length floats of step noise, E carried windows and the reduce scratch of ou_ensemble_reduce_scratch_bytes(E, C).
 * OU_EINVAL, decided on the host before anything is launched: E < 1, E > OU_MAX_ENSEMBLE, E > max_batch, an unknown stat,
 * members == NULL, warm_start >= 0, OU_ENH_USE_AUX_SIGNAL, a non-NULL `noise` while a source is set, n_streams != E * C (and E * C >
 * 65535).  OU_ENOMEM and the unprepared-workspace refusal as in ou_enhance_segments.  Everything is enqueued on `stream`: no
 * allocation, no host synchronisation, no side streams, no float atomics. */
int ou_segments_ensemble_workspace_bytes(const ou_handle* h, int32_t C, int64_t T_raw, int32_t segment, int32_t overlap,
                                         int32_t max_batch, int32_t E, size_t* nbytes, int32_t* batch, int32_t* length);
int ou_enhance_segments_ensemble(ou_handle* h, const float* mix, float* out, float* members, const float* noise, int32_t C,
                                 int64_t T_raw, int32_t E, int32_t stat, int32_t segment, int32_t overlap, int32_t max_batch,
                                 int32_t n_steps, double epsilon, const float* sigma_host, int32_t warm_start, uint32_t flags,
                                 void* ws, size_t ws_bytes, ou_stream_t stream);

/* ---- ensembles of segmented rows with lengths of their own (extension): ou_enhance_segments_ensemble for a batch in which every
 * row has its own length, as ou_enhance_segments_var is to ou_enhance_segments.  Member e of row c is, by definition,
 * ou_enhance_segments(C = 1, T_raw = t_raw[c]) of row c on that member's own noise: the row's own pad split, whole-row mean /
 * gain / mix_rms and mel scale, crossfades only between the row's own consecutive windows, keep_rms with the mix_rms of row c and
 * the peak guard over the member row's own samples.  out[c] is ou_ensemble_reduce over the E post-processed members of row c with
 * len = t_raw[c].  Only the grouping is new.
 *
 * Everything is MEMBER-MAJOR: member row e * C + c.
 *   mix, out : (C, T_raw_max) device, the ou_enhance_segments_var conventions: the rest of a mix row is ignored, the rest of an out
 *              row is zeroed, and out holds the whole-row mel frame energies until the reduce writes it
 *   members  : (E * C, T_raw_max) device, caller-owned and REQUIRED; every row is zeroed behind its own end
 *   t_raw    : HOST, C lengths, 1 <= t_raw[c] <= T_raw_max = the longest
 *   noise    : (n_steps, E * C, T_pad_max) device; member row e * C + c uses its first T_pad_c columns, window k reads the
 *              positions s_k + i.  With a noise source: NULL, n_streams == E * C, stream e * C + c belongs to that member row.
 *   stat     : as ou_enhance_ensemble;  flags, warm_start: as ou_enhance_segments_ensemble.
 *
 * Groups.  Entries, classes (FULL, then SHORT), group boundaries and `ragged` marks are exactly those of ou_segment_groups(tot_ds,
 * C, t_raw, segment, overlap, floor(max_batch / E)); with Bw that call's `batch`, the walk runs batch = E * Bw rows, walk row e *
 * Bw + j = member e of the group's entry j.  A short last group repeats its last real entry per member (the filler of member e
 * repeats member e's own window and noise and is never stitched); a ragged group runs the ragged walk, member rows repeating
 * their entry's lengths; the window carried across a FULL group boundary is per member.  The conditioner runs ONCE over the Bw
 * entries of a group, plain or ragged, and its results and mel scales are replicated to the other members' rows (option
 * `ens_share`, default 1; 0: the input is gathered E times and the conditioner runs over all E * Bw rows -- the arithmetic of
 * ou_enhance_segments_var on E stacked copies of the rows).  Members agree with the single-row calls to fp32 round-off, not bit
 * for bit; E = 1 is ou_enhance_segments_var bit for bit, rows of one length are ou_enhance_segments_ensemble bit for bit.
 *
 * Workspace: ou_segments_var_ensemble_workspace_bytes returns batch = E * Bw and length = min(S, max T_pad_c); prepare the buffer
 * with ou_workspace_init(h, batch, length, ..).  Behind the walk's workspace it holds what ou_segments_ensemble_workspace_bytes
 * lists plus the per-row geometry table and the length table of a ragged group's conditioner pass.
 * OU_EINVAL, decided on the host before anything is launched: E < 1, E > OU_MAX_ENSEMBLE, E > max_batch, E * C > 65535, an
 * unknown stat, members == NULL, t_raw == NULL or a length outside [1, T_raw_max], warm_start >= 0, OU_ENH_USE_AUX_SIGNAL, a
 * non-NULL `noise` while a source is set or none while no source is set, n_streams != E * C, a segment too long for one pass.
 * OU_ENOMEM and the unprepared-workspace refusal as in ou_enhance_segments_var.  Everything is enqueued on `stream`: no
 * allocation, no host synchronisation, no side streams, no float atomics; geometry and entries travel as kernel arguments
 * (capturable). */
int ou_segments_var_ensemble_workspace_bytes(const ou_handle* h, int32_t C, const int64_t* t_raw, int32_t segment, int32_t overlap,
                                             int32_t max_batch, int32_t E, size_t* nbytes, int32_t* batch, int32_t* length);
int ou_enhance_segments_var_ensemble(ou_handle* h, const float* mix, float* out, float* members, const float* noise, int32_t C,
                                     int64_t T_raw_max, const int64_t* t_raw, int32_t E, int32_t stat, int32_t segment,
                                     int32_t overlap, int32_t max_batch, int32_t n_steps, double epsilon, const float* sigma_host,
                                     int32_t warm_start, uint32_t flags, void* ws, size_t ws_bytes, ou_stream_t stream);

/* ---- counter-based sampler noise (extension; the reference draws its noise with torch.randn on the model's device) --------
 * By default every enhance entry point reads its noise from a tensor the caller has drawn.  With a noise SOURCE set on the
 * handle the library produces the noise itself, one step's (B, T) plane at a time, from a pure function
 *
 *     z(seed, stream, draw, t)      -- a standard normal, fp32
 *
 * so that a row's noise depends on nothing but those four numbers: not on the batch it shares, the lane, the rank or the
 * window it is computed in, and nobody holds n_steps planes of it.  The definition (ou_noise.hip and the numpy restatement
 * open_universe_amd/noise.py follow it):
 *   - Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; multipliers D2511F53 / CD9E8D57,
 *     key increments 9E3779B9 / BB67AE85).  Key = (seed & 0xffffffff, seed >> 32).  With the quad index q = t >> 2 the counter is
 *         c0 = q & 0xffffffff    c1 = ((q >> 32) & 0xffff) | (draw << 16)    c2 = stream & 0xffffffff    c3 = stream >> 32
 *     (q < 2^48, i.e. t < 2^50; draw < 2^16).  One block (w0, w1, w2, w3) yields the normals of the positions 4q .. 4q + 3.
 *   - word -> uniform in the open interval (0, 1): u(w) = ((w >> 8) + 0.5) * 2^-24.
 *   - Box-Muller: r = sqrt(-2 ln u(w0)); z(4q) = r cos(2 pi u(w1)), z(4q + 1) = r sin(2 pi u(w1)); the same with (w2, w3) for
 *     z(4q + 2), z(4q + 3).  |z| <= sqrt(50 ln 2) = 5.887.  Evaluated with the precise fp32 device functions on exact
 *     arguments (for w >> 8 >= 2^23 through the mirror image 1 - u, whose numerator is an fp32 number: ln u = log1p(-(1 - u)),
 *     cos(2 pi u) = cos(2 pi (1 - u)), sin(2 pi u) = -sin(2 pi (1 - u))): within 1e-5 of the real-valued definition.
 *   - draw: 0 = the initial draw (x0, universe.py:326, or the warm-start noise, :330); n + 1 = z_n of the ABSOLUTE step n (:338),
 *     so a warm start at step k uses the draws 0, k + 1, k + 2, ..
 *   - t: position in the row's OWN padded signal (column of its T_pad = t_raw + pad samples): ou_enhance, a row of
 *     ou_enhance_var and a window of ou_enhance_segments (t = s_k + i) agree.
 *   - stream: one 64-bit id per row, the caller's choice (the Python layer: (utterance index << 16) | channel). */
typedef struct ou_noise_spec {
  uint64_t seed;           /* the key */
  const uint64_t* streams; /* HOST, one id per row: B of ou_enhance / ou_enhance_var, C of ou_enhance_segments (copied by the call) */
  int32_t n_streams;
  void* scratch;           /* DEVICE, caller-owned, 16-byte aligned, alive as long as the source is set: two (B, T_pad) planes */
  size_t scratch_bytes;    /* >= ou_noise_scratch_bytes(h, B, T_pad) of every ou_enhance / ou_enhance_var call that follows;
                            * ou_enhance_segments needs none (its workspace already holds one step's plane): NULL / 0 is fine */
} ou_noise_spec;
/* Noise source of the NEXT forward calls of this handle; NULL: back to the noise tensor (the default).  While a source is set
 *   - `noise` must be NULL in ou_enhance / ou_enhance_var / ou_enhance_segments (OU_EINVAL otherwise: an argument is never
 *     silently ignored), n_streams must equal the call's rows (OU_EINVAL), a scratch that is too small is OU_ENOMEM;
 *   - the library fills a plane right in front of the launch that reads it (x0 in front of the init, z_n in front of the score
 *     pass of step n) on the caller's stream, ping-pong between the two planes of the scratch -- the hot kernels read a
 *     (B, T) plane through the pointer they always got; ou_enhance_segments fills its workspace plane per window group where it
 *     gathered from the tensor before.  Stream ids and positions travel as kernel arguments: no allocation, no host
 *     synchronisation, capturable like the rest.  A captured graph keeps the source it was captured with.
 * The tensor mode enqueues exactly what it did before; ou_workspace_bytes / ou_segments_workspace_bytes are unchanged.
 * ou_plan_json reports the source as "noise_source": "tensor" | "counter". */
int ou_set_noise_source(ou_handle* h, const ou_noise_spec* spec);
int ou_noise_scratch_bytes(const ou_handle* h, int32_t B, int32_t T_pad, size_t* nbytes);
/* The function itself, for tests and for bindings that keep the reference's Python loop (cf. ou_sampler_step):
 *   out[j * row_stride + i] = i < len[j] ? z(seed, streams[j], draw, t0[j] + i) : 0      for 0 <= i < cols, 0 <= j < rows
 * out: device; streams_host / t0_host / len_host: `rows` entries on the HOST (0 <= len[j] <= cols <= row_stride, t0[j] >= 0,
 * t0[j] + len[j] <= 2^50, 0 <= draw < 2^16).  Enqueued on `stream`, 64 rows per launch. */
int ou_noise_fill(float* out, int64_t row_stride, int64_t cols, int32_t rows, const uint64_t* streams_host,
                  const int64_t* t0_host, const int64_t* len_host, uint64_t seed, int32_t draw, ou_stream_t stream);

/* ---- resampling (the two steps around enhance in the reference's CLI: torchaudio.functional.resample to the model rate and
 * back, bin/enhance.py:77-80,186-190, with its defaults sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) ------------
 * Stateless: no handle.  The definition (torchaudio's documented algorithm restated; open_universe_amd/audio.py restates the
 * same one as a dense conv1d).  With g = gcd(fs_in, fs_out):
 *     orig = fs_in / g    new = fs_out / g    base = min(orig, new) * 0.99    width = ceil(6 * orig / base)
 * and for a row x[0 .. n) (zero outside), output j = f * new + p (0 <= p < new) for 0 <= j < ceil(new * n / orig):
 *     y[j] = sum_i k[p][i] * x[f * orig - width + i]                 0 <= i < 2 * width + orig
 *     k[p][i] = sinc(pi t) cos^2(pi t / 12) base / orig,   t = clamp((-p / new + (i - width) / orig) * base, -6, 6)
 * k is evaluated in double and rounded once to fp32.  The SUPPORT of phase p is the run of i whose unclamped t lies strictly
 * inside (-6, 6); outside it k holds cos^2(pi / 2)-sized values (< 1e-30), which this path treats as zero.  So an output costs
 * `taps` (the longest support) multiply-adds instead of 2 * width + orig: 34 of 475 at 44 100 -> 16 000, 13 of 174 back.
 *
 * Coefficient table (host functions; the caller uploads it once per rate pair and owns the device copy):
 *     int32 first[new]        first input of phase p relative to f * orig (= first i of its support - width)
 *     float coef[taps][new]   coef[t][p] = k[p][first[p] + width + t], 0 behind the phase's own support
 * i.e. table_bytes = (taps + 1) * new * 4.  The values are computed in double, in the operation order of the definition, and
 * rounded once: they ARE the dense kernel's entries.  OU_EINVAL: non-positive rates, a table_bytes that is not the plan's, or
 * a reduced ratio so extreme that the table would not fit 32-bit indices (width > 2^28 or more than 2^29 words). */
int ou_resample_plan(int32_t fs_in, int32_t fs_out, int32_t* orig, int32_t* new_, int32_t* width, int32_t* taps,
                     size_t* table_bytes);
int ou_resample_table(int32_t fs_in, int32_t fs_out, void* table, size_t table_bytes);
/* ceil(new * n / orig): the outputs of a row of n samples (n itself for equal rates); -1 for a bad argument */
int64_t ou_resample_length(int32_t fs_in, int32_t fs_out, int64_t n);
/* Consecutive outputs of one row that one workgroup of ou_resample owns for this rate pair (tests choose lengths around it;
 * results do not depend on it: every output is one sum in ascending tap order).  -1 for a bad rate pair. */
int32_t ou_resample_tile(int32_t fs_in, int32_t fs_out);
/* Resample `rows` rows of lengths of their own, one launch per 64 rows:
 *   x        : (rows, x_stride) device; row b holds len[b] samples, nothing is read behind them
 *   len_host : `rows` entries on the HOST, 0 <= len[b] <= x_stride
 *   y        : (rows, y_stride) device; row b receives its ou_resample_length(fs_in, fs_out, len[b]) outputs, the columns from
 *              there up to `cols` are zeroed, nothing behind `cols` is touched (cols <= y_stride)
 *   table    : DEVICE copy of ou_resample_table's output, table_bytes = the plan's (anything else: OU_EINVAL).  A small table
 *              is kept in LDS, a large one (813 KB of coefficients at 16 000 -> 16 001) is read through the caches.
 * fs_in == fs_out: a plain copy with the same zeroing; the table is not read and may be NULL.
 * OU_EINVAL, nothing launched: non-positive rates, rows < 1, an output row that does not fit cols or y_stride, lengths or
 * strides whose products overflow the kernel's 64-bit offsets (rows * stride, new * len[b] <= 2^60).  All of that is decided
 * on the host before the first HIP call.  Enqueued on `stream`: no allocation, no host synchronisation, capturable.  The
 * accumulation is fp32 FMA in ascending tap order whatever the tiling, so a row's result does not depend on the batch it is in. */
int ou_resample(const float* x, int64_t x_stride, const int64_t* len_host, float* y, int64_t y_stride, int64_t cols,
                int32_t rows, int32_t fs_in, int32_t fs_out, const void* table, size_t table_bytes, ou_stream_t stream);

/* ---- alias-free Snake activation (bigvgan Activation1d, alias_free_act.py:25-30, around Snake / SnakeBeta, snake.py:53-64,
 * 115-128, with log-scale parameters): what a PReLU_Conv with act_type snake / snakebeta applies in front of its conv.
 * Stateless: no handle.  For row (b, c) = x[(b * C + c) * row_stride ..], with n = len[b] (T when len_host is NULL), x zero
 * outside [0, n):
 *     u[2 q + p] = sum_k up[p][k] x[q + k - 7]                      0 <= k < 15     Resample(1 -> 2): width 7, see "resampling"
 *     s[j]       = u[j] + (1 / (eb[c] + 1e-9)) * sin(u[j] * ea[c])^2   for 0 <= j < 2 n, 0 outside
 *     y[t]       = sum_k down[k] s[2 t + k - 13]                     0 <= k < 28     Resample(2 -> 1): width 13
 * for 0 <= t < n, and y[t] = 0 for n <= t < T: row b IS the call on that row alone (the ou_enhance_var convention).  ea =
 * exp(alpha), eb = exp(beta) per channel (device, C floats; exp_beta NULL: eb = ea, plain Snake); up_kernel (2, 15) and
 * down_kernel (28) are the two torchaudio kernels (device).  Every sum is one fp32 FMA per tap, taps ascending; sin is the
 * precise sinf and the reciprocal a true division, so a value depends on neither the tiling nor the batch it is in.  The x2
 * signal exists in LDS only.  y must not overlap x.
 * OU_EINVAL, decided on the host before any HIP call: a NULL tensor, B, C or T < 1, C > 65535, T > 2^31 - 1024, row_stride < T, a length outside
 * [0, T], B * C * row_stride > 2^60.  Enqueued on `stream`, 64 rows of B per launch when lengths are given (they travel as
 * kernel arguments), else one launch: no allocation, no host synchronisation, capturable. */
int ou_snake_act(const float* x, float* y, int32_t B, int32_t C, int32_t T, int64_t row_stride, const int32_t* len_host,
                 const float* exp_alpha, const float* exp_beta, const float* up_kernel, const float* down_kernel,
                 ou_stream_t stream);
/* Consecutive outputs of one (row, channel) that one workgroup of ou_snake_act owns (tests sit on its edges). */
int32_t ou_snake_tile(void);

/* ---- scoring: how close an estimate is to a reference, for batches whose rows have lengths of their own ------------------
 * The four scores of the reference's inference tooling that are arithmetic on two waveforms: the log-spectral distance and its
 * scale-invariant form (metrics/lsd.py as metrics/wrapper.py:130-153 calls it), SI-SDR (wrapper.py:197-213), the plain SNR
 * beside it, and the time-domain + multi-resolution spectral L1 (losses/multires_stft.py); and a fifth, the BSS-eval SDR
 * (wrapper.py:179-195), which the reference takes from a package but is arithmetic all the same (ou_sdr).  Stateless: no handle.
 *   est, ref : (B, stride) device; row b holds len[b] samples of each, nothing behind them is read
 *   len_host : B entries on the HOST, 1 <= len[b] <= min(stride, 2^31 - 1)
 *   out      : B floats on the device, one score per row
 *   scratch  : device, at least ou_metrics_scratch_bytes(B, longest len, the call's specs) bytes (OU_ESHAPE otherwise); no
 *              contents are kept between calls
 * Every row is scored as if it were alone at its own length: its frame count is ou_metrics_frames(len[b], hop), its own last
 * sample is the reflection point of the centred STFT, and the result is bit for bit that of a B = 1 call on the row.  Sums
 * run in one fixed order (no atomics): two runs of a call are bit-identical.
 * The STFT is centred, one-sided (n_fft / 2 + 1 bins), with the periodic Hann window of n_fft points (win_length = n_fft);
 * the DFT is a product with a cos / sin basis on the matrix pipe, in double (window, basis and sums; the samples are the
 * caller's fp32).  No spectrogram is
 * stored.  n_fft must be even, at least 2 and at most OU_METRICS_MAX_NFFT: a workgroup keeps 16 frames of both
 * signals, 128 * n_fft bytes, in the 160 KiB of LDS.  hop >= 1.  Anything else: OU_EINVAL with a message, decided on the host
 * before the first HIP call, like every other refusal below.  Enqueued on `stream`: no allocation, no host synchronisation. */
#define OU_METRICS_MAX_NFFT 1024
#define OU_METRICS_MAX_SPECS 8
#define OU_MET_SCALE_INVARIANT 1 /* rescale by alpha = sum(est ref) / (sum(est^2) + eps) first (lsd.py:95-98, multires_stft.py:97-100) */
#define OU_MET_NATURAL_LOG 2     /* ou_lsd: ln instead of 10 log10 (`db = False`) */
typedef struct ou_metrics_spec {
  int32_t n_fft, hop;
  float eps;     /* ou_lsd: inside the logarithm and in alpha.  Not read by ou_spectral_mae */
  int32_t flags; /* ou_lsd: OU_MET_*.  Not read by ou_spectral_mae */
} ou_metrics_spec;
/* 1 + T / hop: the frames of the centred STFT of T samples (n_fft even); -1 for T < 0 or hop < 1 */
int64_t ou_metrics_frames(int64_t T, int32_t hop);
/* Scratch of a call with B rows, the longest T_max samples, and these resolutions (n_spec = 0: ou_si_sdr). */
int ou_metrics_scratch_bytes(int32_t B, int64_t T_max, const ou_metrics_spec* spec, int32_t n_spec, size_t* nbytes);
/* Log-spectral distance, p = 2:  with X, Y the STFTs of est and alpha * ref (reflect padding), W = sum of window^2,
 *     out[b] = sqrt(mean over frames and bins of (L(|X|^2 / W + eps) - L(|Y|^2 / W + eps))^2),   L = 10 log10 (or ln)
 * OU_EINVAL also for len[b] <= n_fft / 2, where the reflect padding is undefined. */
int ou_lsd(const float* est, const float* ref, int64_t stride, const int64_t* len_host, int32_t B, const ou_metrics_spec* spec,
           float* out, void* scratch, size_t scratch_bytes, ou_stream_t stream);
/* out[b] = w * mean_t |alpha est - ref| + (1 - w) / n_spec * sum over specs of mean over frames and bins of | |X| - |Y| |,
 * X, Y the STFTs of alpha * est and ref with zero padding, w = time_domain_weight; n_spec = 0: the time-domain mean alone.
 * flags: OU_MET_SCALE_INVARIANT or 0; eps is the one in alpha. */
int ou_spectral_mae(const float* est, const float* ref, int64_t stride, const int64_t* len_host, int32_t B,
                   const ou_metrics_spec* spec, int32_t n_spec, float time_domain_weight, float eps, int32_t flags, float* out,
                   void* scratch, size_t scratch_bytes, ou_stream_t stream);
/* With c = (sum est ref)^2 / (sum est^2 * sum ref^2) for out_si_sdr (no mean removed) and c = sum ref^2 / (sum ref^2 +
 * sum (est - ref)^2) for out_snr, both 0 where the denominator is 0, and e = 10^(-clamp_db / 10) / (1 + 10^(-clamp_db / 10)):
 *     out = 10 log10(c' / (1 - c')),   c' = min(max(c, e), 1 - e)
 * i.e. the ratio clamped to [-clamp_db, clamp_db] (the reference passes 100).  The sums are taken in double.  Either output
 * may be NULL.  OU_EINVAL for a clamp_db that is not positive and finite. */
int ou_si_sdr(const float* est, const float* ref, int64_t stride, const int64_t* len_host, int32_t B, float clamp_db,
              float* out_si_sdr, float* out_snr, void* scratch, size_t scratch_bytes, ou_stream_t stream);
/* The BSS-eval SDR with a distortion filter of L = filter_length taps (metrics/wrapper.py:179-195 asks the fast_bss_eval
 * package for it with filter_length 512, zero_mean False, clamp_db 100).  For one row of T = len[b] samples, with s_l = ref
 * delayed by l samples (l = 0 .. L - 1), every signal zero-extended to T + L - 1, and P the orthogonal projection onto
 * span{s_0 .. s_{L-1}}:
 *     c = ||P est||^2 / ||est||^2,  0 where est or ref is all zero;   out = 10 log10(c' / (1 - c')),  c' clamped as above
 * i.e. with r[l] = sum_t ref[t] ref[t + l], x[l] = sum_t ref[t] est[t + l], R = toeplitz(r) and R h = x: c = x.h / sum est^2.
 * R is positive definite for every non-zero ref (T < L included).  L = 1 is out_si_sdr of ou_si_sdr; either signal may be
 * rescaled without changing the score.  The correlations are sums of exact products of the caller's fp32 samples, taken in
 * double on the matrix pipe; the solve (Levinson recursion) is in double; no zero-extended copy of a signal is stored.  The
 * package itself is not a dependency and not part of the reference tree: the definition above is the contract.
 * Rows, lengths, out and stream as for the other scores; scratch at least ou_sdr_scratch_bytes(B, longest len, L) bytes
 * (OU_ESHAPE otherwise).  OU_EINVAL for filter_length outside 1 .. OU_SDR_MAX_FILTER and for a clamp_db that is not positive
 * and finite.  Not done: zero_mean, load_diag, permutation solving, the conjugate-gradient solver. */
#define OU_SDR_MAX_FILTER 512
int ou_sdr_scratch_bytes(int32_t B, int64_t T_max, int32_t filter_length, size_t* nbytes);
int ou_sdr(const float* est, const float* ref, int64_t stride, const int64_t* len_host, int32_t B, int32_t filter_length,
           float clamp_db, float* out, void* scratch, size_t scratch_bytes, ou_stream_t stream);
/* STOI (Taal et al. 2011) and extended STOI (Jensen & Taal 2016) of est against the clean signal ref, both at rate fs, with
 * the constants of the authors' MATLAB code (metrics/wrapper.py:116-128 asks the pystoi package for them).  The package is not
 * a dependency and nothing is compared against it: the definition below is the contract.  EPS = 2^-52.
 *   1. fs != 10000: both signals to 10 kHz.  p = 10000 / g, q = fs / g, g = gcd; fc = 1 / (2 max(p, q)),
 *      L = ceil(52 / (28.714 fc / 10)), h[t] = 2 p fc sinc(2 fc t) kaiser(2 L + 1, 0.1102 (60 - 8.7))[t + L] for t = -L .. L,
 *      normalised to sum 1 and multiplied by p; output j = sum_k h[k] xup[j q + L - k], xup[i p] = x[i] and zero elsewhere
 *      (outside the row too); ceil(T p / q) outputs.
 *   2. Frames of 256 at hop 128 starting at range(0, n - 256, 128) -- end exclusive: a frame that would start exactly at
 *      n - 256 is NOT counted (the MATLAB rule; one function in the library) --, window w = hanning(258)[1:-1].
 *      E_f = 20 log10(||w ref_f|| + EPS); the frames with E_f > max E - 40 are kept, and the kept windowed frames of both
 *      signals are overlap-added at hop 128 in their order (K frames: 128 (K - 1) + 256 samples).
 *   3. Same frames, window and hop on both results; bins 0 .. 256 of the 512-point DFT of the zero-padded frame.
 *   4. Fifteen one-third-octave bands: the square root of the sum of |X|^2 over bins [lo, hi) = (7,9) (9,11) (11,14) (14,17)
 *      (17,22) (22,27) (27,34) (34,43) (43,55) (55,69) (69,87) (87,109) (109,138) (138,174) (174,219).
 *   5. Fewer than 30 frames after step 3: the score is 1e-5.  That is a result, not an error -- a row too short to have a
 *      single frame scores 1e-5 too.
 *   6. Segment m = 30 .. frames is band values [:, m - 30 : m], M = frames - 29 of them.
 *      extended == 0: per segment and band c = ||x|| / (||y|| + EPS), y' = min(c y, x (1 + 10^(15/20))), both with their mean
 *        over the 30 frames removed and divided by their norm + EPS; the score is sum x y' / (15 M).
 *      extended != 0: per segment and band mean removed and divided by norm + EPS over the 30 frames, then per segment and
 *        frame the same over the 15 bands, for x and y; the score is sum x y / (30 M).       (x: ref, y: est)
 * The samples enter as fp32; the filter table, the resampled and overlap-added signals, the DFT (on the f64 matrix
 * instruction), the band values and every sum are double, and out is rounded to fp32 once.
 * Rows, lengths, out and stream as for the other scores; scratch at least ou_stoi_scratch_bytes(B, longest len, fs) bytes
 * (OU_ESHAPE otherwise).  The filter table is built on the host from fs and copied into the scratch on the stream.
 * OU_EINVAL, before the first HIP call, for fs < 1, for an fs whose filter needs more than OU_STOI_MAX_TAPS taps per output
 * (ceil((2 L + 1) / p)) or a table (p ints, taps x p doubles) above OU_STOI_MAX_TABLE_BYTES -- 8000, 10000, 16000, 22050,
 * 24000, 32000, 44100, 48000, 96000 pass; a rate coprime to 10000 above about 7000 does not --, for a row with more than
 * 2^31 - 1 samples at 10 kHz, and for B < 1 or bad lengths.  ou_stoi_frame_tile: STFT frames per workgroup (for tests).
 * Not done: other internal rates, a differentiable form. */
#define OU_STOI_MAX_TAPS 2048
#define OU_STOI_MAX_TABLE_BYTES (4 << 20)
int ou_stoi_scratch_bytes(int32_t B, int64_t T_max, int32_t fs, size_t* nbytes);
int ou_stoi(const float* est, const float* ref, int64_t stride, const int64_t* len_host, int32_t B, int32_t fs, int32_t extended,
            float* out, void* scratch, size_t scratch_bytes, ou_stream_t stream);
int32_t ou_stoi_frame_tile(void);

/* ---- level normalisation: normalization_norm and normalization_kwargs.zero_mean / .eps of the model yaml (utils/norm.py:22-87):
 * how every enhance entry point (ou_enhance, _var, _ensemble, the four ou_enhance_segments*) levels a row before the networks
 * see it.  With m the mean of the padded row, sd its unbiased std (around m) and mx = max |x - mu| over the padded row,
 * mu = zero_mean ? m : 0, the row becomes (x - mu) * gain:
 *   OU_NORM_2:    gain = level / max(sd, 1e-5)          OU_NORM_MAX:  gain = level / max(mx, 1e-5)
 *   OU_NORM_2MAX: gain = min(level / max(sd, eps), 1 / max(mx, eps))
 * level = 10^(ou_config.level_db / 20).  eps: 0 = 1e-5; as in the reference it reaches the OU_NORM_2MAX branch alone.
 * A handle is created with (OU_NORM_2, 1, 0) -- every shipped config -- and then runs the kernels, launches and results it always
 * had; neither the plan, the blob, ou_workspace_bytes nor the ou_segments*_workspace_bytes answers depend on the mode (the block
 * maxima of the segmented statistics have their words in every segment workspace), so the call may come at any time between
 * two enhance calls; Universe makes it right after ou_create.  A setter and not a field of ou_config: the struct's size is part of what version 7 callers compiled against.  ou_plan_json(handle) reports
 * "norm", "zero_mean", "norm_eps".  OU_EINVAL: an unknown mode, zero_mean not 0 / 1, eps negative or not finite. */
int ou_set_normalization(ou_handle* h, int32_t norm_mode, int32_t zero_mean, float eps);

/* One sampler update on caller-owned buffers, for bindings that keep the reference's Python loop
 * (universe.py:339 `x = x + s_now^2 * eta * score + beta * z`, :343 `x = x + s_last^2 * score`):
 *   x[i] += c1 * score[i] + c2 * z[i]     over n = B*T elements; z may be NULL (last step).
 * Inside ou_enhance the same update is fused into the output conv of the score network. */
int ou_sampler_step(ou_handle* h, float* x, const float* score, const float* z, float c1, float c2, size_t n,
                    ou_stream_t stream);

/* ---- signal transform of the STFT-domain configurations: CompressedMagSTFT / CompressedMagSTFTPadded
 * (layers/dyn_range_comp.py:51-225; `model.transform`, universe.py:112-115, 274, 346).  Stateless: no handle.
 *   transform_type: 0 "none", 1 "exponent" ((1e-7 + |s|)^(e-1) s factor), 2 "log" (log(1 + |s|) sgn(s) factor)
 *   forward : x (B, T) -> out (B, 2F, n_frames), real parts then imaginary parts as channels, F = n_fft/2 + 1,
 *             STFT with center=True, zero padding, onesided, `window` (n_fft) on the device; n_frames = ou_transform_frames
 *   inverse : spec (B, 2F, n_frames) -> y (B, length): expansion, iSTFT (overlap-add / window envelope, torch.istft
 *             semantics, centre trimmed); scratch = B * n_frames * n_fft floats (device) */
int ou_transform_frames(int32_t T, int32_t n_fft, int32_t hop);
int ou_transform_forward(const float* x, int32_t B, int32_t T, const float* window, int32_t n_fft, int32_t hop,
                         int32_t transform_type, float abs_exponent, float factor, float* out, ou_stream_t stream);
int ou_transform_inverse(const float* spec, int32_t B, int32_t n_frames, const float* window, int32_t n_fft, int32_t hop,
                         int32_t transform_type, float abs_exponent, float factor, int32_t length, float* y,
                         float* scratch, ou_stream_t stream);

/* How the GRU clusters publish the hidden state (score.py:83-89,116 / condition.py:173-179,212 as a multi-workgroup
 * recurrence): 0 (default) = plain stores inside a cluster whose workgroups share one XCD (its L2 is their point of
 * coherence; verified by a rendezvous at every launch), agent-scope stores otherwise; 1 = agent-scope (sc1,
 * write-through) stores always (+0.1 ms per 401-frame pass).  Both forms are backed by a bounded-spin safety net that
 * repeats a publish system-scope and counts the event in the workspace header (word 20: every wait it cut short, late
 * members included; word 33: those where the publish was there for a system-scope load but not for the gather's
 * agent-scope load).  The library switches to 1 for good the first time word 33 moves (ou_check_device_status). */
int ou_set_gru_publish_mode(ou_handle* h, int32_t agent_scope);

/* ... and what the handle currently uses (1 after ou_set_gru_publish_mode(h, 1) or after ou_check_device_status found
 * that the safety net had to act).  A hipGraph captured earlier keeps the form it was captured with: re-capture. */
int ou_get_gru_publish_mode(const ou_handle* h);

/* K enhance calls in flight side by side in ONE process (extension; the reference's loop over files is serial,
 * bin/enhance.py:173-192): create K handles on the same weight blob, give each its own stream and workspace, and tell
 * every handle `lanes` = K and its own index `lane` (0 .. K - 1) BEFORE its first forward call.  A handle itself stays
 * non-re-entrant.  What the numbers are for: the workgroups of a GRU cluster wait for each other, so every GRU launch that
 * can be on the device at a time has to fit there whole -- the library sizes the launches of a lane to its share of the
 * XCDs and deals the clusters of lane l to XCDs of their own (2 B l, 2 B l + 1, ..).  Results do not depend on the lane:
 * a call keeps the kernels, tilings and -- as long as every cluster is still resident with it -- the split of the hidden
 * units of the single-lane call, i.e. bit-identical results (every shipped configuration at 1 .. 8 lanes; if the split does
 * not fit, the recurrence falls back to 16 units per workgroup: equal to fp32 rounding).  1 <= lanes <= 8. */
int ou_set_lanes(ou_handle* h, int32_t lanes, int32_t lane);

/* Lanes that run calls of DIFFERENT batch sizes at the same time (distributed.enhance_sharded(batch_size > 1, in_flight > 1)
 * on a ragged set, the CLI with files of different channel counts): the share of an XCD a lane's GRU launch may take and the
 * XCDs its clusters are dealt to were functions of that call's own B -- lanes that disagree about B then disagree about the
 * layout, and more cluster workgroups than an XCD holds wait for members that cannot be scheduled (a spurious device-side
 * time-out).  Tell EVERY handle of the pool the largest batch size any lane will run (`max_batch` >= 1; 0 = "this call's own
 * B", the default and the right value when all calls have one size): shares and placement are then computed from that one
 * number on all lanes.  A call smaller than max_batch may fall back to 16 hidden units per workgroup where the single call
 * takes 8 -- equal to fp32 rounding (> 100 dB), not bit-identical; calls of size max_batch are unchanged. */
int ou_set_lane_batch(ou_handle* h, int32_t max_batch);

/* How many lanes this device can carry when every lane may run a call of `max_batch` utterances: the GRU launches of all
 * lanes must be resident together (1 .. 8; e.g. UNIVERSE++ 16 kHz, H = 256: 8 lanes up to batch 2, 4 lanes at batch 4, 2 at
 * batch 8).  A pool larger than this makes the forward calls fail with OU_EHIP ("invalid configuration") -- the Python pool
 * (lanes.LanePool) clamps itself to this number. */
int ou_lane_capacity(const ou_handle* h, int32_t max_batch);

/* After the stream has been synchronised: OU_OK, or OU_ESYNC if a device-side timeout flag was raised.  The status
 * word (first 4 bytes of the workspace) is sticky: it stays raised until ou_workspace_init() / this call clears it.
 * Also reads status word 33 -- GRU publishes that were INVISIBLE to the gather's agent-scope loads (the recovery counter,
 * word 20, also counts cluster members that were merely late and does not switch anything): once word 33 has moved, the
 * handle publishes with agent-scope stores from the next call on (see ou_set_gru_publish_mode). */
int ou_check_device_status(ou_handle* h, void* ws);

/* ---- steering (tests, tuning) ---------------------------------------------------------------------------------
 * Typed options of a handle.  They replace the ~35 OU_* environment variables earlier ABI versions read: the library reads NO
 * environment variable any more, so nothing outside the caller's own code can change which kernels run.  Normal use needs
 * none of them -- the defaults are what the launchers' measured rules pick; the tests use them to force every kernel family
 * onto every layer it admits, the tools to sweep.  Keys: ou_option_name(0 .. ou_option_count() - 1), each with a one-line
 * ou_option_doc; integer-valued except `tile_min`.  Options that make a call return WRONG results by design (phase
 * ablation) exist in `make EXPERIMENTS=1` builds only (OU_ENOTIMPL otherwise).  A forward call works on the values it finds
 * when it starts; a captured hipGraph keeps the kernels it was captured with.  ou_plan_json echoes the current values. */
int ou_set_option(ou_handle* h, const char* key, double value); /* OU_EMISSING: no such key; OU_EINVAL: not an integer */
int ou_get_option(const ou_handle* h, const char* key, double* value);
int ou_reset_options(ou_handle* h); /* every option back to its default */
int ou_option_count(void);
const char* ou_option_name(int32_t index);
const char* ou_option_doc(int32_t index);
double ou_option_default(int32_t index);

/* ---- introspection (tests, profiling) ------------------------------------------------------------------- */
/* JSON description of the packed layers (for a handle: "norm": "2" | "max" | "2-max", "zero_mean", "norm_eps", see ou_set_normalization; name, kind, shapes, offsets into the blob, "activation": "prelu" | "snake" | "snakebeta" |
 * "none" with the offsets of a Snake layer's exp(alpha) / exp(beta), and the offsets of the two Snake resampling kernels); for a handle also "options": the current
 * value of every ou_set_option key. */
const char* ou_plan_json(const ou_handle* h);
const char* ou_packer_plan_json(const ou_packer* p);
/* Locate a named intermediate of the last ou_condition / ou_score / ou_enhance call in the workspace:
 * byte offset, channels, length (per batch element; layout (B, C, T)).  Names: see DESIGN.md. */
int ou_tensor(const ou_handle* h, const char* name, size_t* byte_offset, int32_t* C, int32_t* T);
/* Number of kernels the last forward enqueued, and the generic-conv launch count among them. */
int ou_launch_stats(const ou_handle* h, int32_t* n_launches, int32_t* n_conv_launches);
/* ---- input files of the CLI ------------------------------------------------------------------------------- */
/* FLAC stream decoder (pure host code).  Replaces the codec behind `torchaudio.load` in the reference's CLI
 * (open_universe/bin/enhance.py:183; AUDIO_SUFFIXES :33 lists .flac) -- torchaudio is not a dependency of this package.
 * Every checksum of the stream (frame-header CRC-8, frame CRC-16) is verified; the MD5 of the decoded audio is returned for the
 * caller to check (open_universe_amd/audio.py does).  ou_flac_last_error(): message of the last failure on this thread.
 *   ou_flac_info  : header fields; total_samples is counted by a decoding pass when the header does not carry it
 *   ou_flac_decode: out[channels][capacity_per_channel] <- the samples as integers (bits_per_sample wide, sign-extended) */
const char* ou_flac_last_error(void);
int ou_flac_info(const uint8_t* data, size_t bytes, int32_t* sample_rate, int32_t* channels, int32_t* bits_per_sample,
                 int64_t* total_samples, uint8_t* md5 /* 16 bytes, all zero = not recorded */);
int ou_flac_decode(const uint8_t* data, size_t bytes, int32_t* out, int64_t capacity_per_channel, int64_t* decoded);

/* ---- output files of the CLI ------------------------------------------------------------------------------ */
/* FLAC encoder for fp32 rows that live on the device (extension; the reference writes its results with torchaudio.save,
 * bin/enhance.py:77-80).  The stream is byte for byte the one audio.flac_encode of the Python package writes for the samples
 * q = clip(rint(x * 2^(bps - 1)), -2^(bps - 1), 2^(bps - 1) - 1) (round half to even; NaN -> 0): fixed blocks of 4096 samples,
 * independent channels, per channel and block the fixed predictor of order 2 with one Rice partition (k from the mean of the
 * folded residual) or a verbatim subframe where that is not longer, STREAMINFO with the MD5 of the samples.  Three calls:
 *   ou_flac_encode_sizes  : pure host.  frames_bytes / pcm_bytes: the device buffers of the next call (and their host copies);
 *                           n_frames: blocks of all files = entries of frame_bytes; stream_capacity[f] (may be NULL): an upper
 *                           bound of file f's stream, their sum always suffices as out_capacity.
 *   ou_flac_encode_frames : file f owns channels[f] consecutive rows of x (row_stride floats apart), each len[f] long; nothing
 *                           behind a row's length is read.  One workgroup per (file, block) quantises, codes and packs; all
 *                           files of a call go in launches of 64 files.  Writes, file after file and block after block, one
 *                           frame per slot of 16 + ceil(channels * (8 + 4096 * bps) / 8) + 2 bytes rounded up to 16 (frames), its
 *                           byte count (frame_bytes, the CRC-16 included, whose two bytes are left zero), and per file the
 *                           interleaved little-endian samples at bps / 8 bytes, rounded up to 16 bytes (pcm).  What the buffers
 *                           held before does not matter.  frames and pcm 16-byte aligned.  Enqueued on `stream`: no allocation,
 *                           no host synchronisation, capturable.
 *   ou_flac_assemble      : pure host, on host copies of the three buffers once the stream has been synchronised: CRC-16 of
 *                           every frame, MD5, STREAMINFO; stream f is out[offsets[f] .. offsets[f + 1]).
 * OU_EINVAL with a message (ou_flac_last_error), before any HIP call: files < 1, channels outside 1 .. 8, bps not 16 or 24, fs
 * outside 1 .. 2^20 - 1, a length below 1 or above 2^36 - 1, row_stride below the longest length, a null or misaligned buffer, a
 * frame size the kernel cannot have written.  OU_ESHAPE: frames_bytes, pcm_bytes or out_capacity too small. */
int ou_flac_encode_sizes(int32_t files, const int32_t* channels_host, const int64_t* len_host, int32_t bps, size_t* frames_bytes,
                         int64_t* n_frames, size_t* pcm_bytes, int64_t* stream_capacity);
int ou_flac_encode_frames(const float* x, int64_t row_stride, int32_t files, const int32_t* channels_host,
                          const int64_t* len_host, int32_t bps, void* frames, size_t frames_bytes, int32_t* frame_bytes,
                          void* pcm, size_t pcm_bytes, ou_stream_t stream);
int ou_flac_assemble(const uint8_t* frames_host, const int32_t* frame_bytes_host, const uint8_t* pcm_host, int32_t files,
                     const int32_t* channels_host, const int64_t* len_host, int32_t fs, int32_t bps, uint8_t* out,
                     size_t out_capacity, int64_t* offsets);
/* Compression levels.  Level 0 is the stream above, bit for bit, from the same kernel.  Level 1: per channel
 * and block the cheapest of a constant subframe and the fixed predictors of order 0 .. 4, priced exactly, then the best Rice
 * partition order 0 .. 6 (2^po divides the block, a partition keeps 16 samples); verbatim where that is not shorter.  Level 2
 * adds one LPC candidate of order 8 (precision 14, shift 0 .. 15; Welch window, autocorrelation and Levinson-Durbin in double,
 * in one fixed order: two runs are bit-identical).  Levels 0 and 1 are byte for byte audio.flac_encode(level=...); a level-2
 * stream is the one audio.flac_encode writes when it is handed the coefficients the device chose (lpc_override).  Blocks, frame
 * headers, slots, frame_bytes, pcm and ou_flac_assemble are those of ou_flac_encode_frames, and so is the call's contract.
 *   ou_flac_encode_choices_bytes: pure host.  Bytes of the choices buffer: one record per subframe in stream order (file, block,
 *                                 channel).
 *   choices (may be NULL)       : device, 4-byte aligned.  A record is OU_FLAC_CHOICE_WORDS int32:
 *                                 [0] kind (OU_FLAC_KIND_*)  [1] predictor order  [2] partition order  [3] coefficient precision
 *                                 [4] shift  [5] bits of the subframe  [6 ..] OU_FLAC_CHOICE_COEFS coefficients; what a kind does
 *                                 not use is 0.  Level 0 writes fixed / order 2 / partition order 0, or verbatim.
 * OU_EINVAL also for a level outside 0 .. 2 and a misaligned choices buffer; OU_ESHAPE for one that is too small. */
#define OU_FLAC_CHOICE_WORDS 18
#define OU_FLAC_CHOICE_COEFS 12
#define OU_FLAC_KIND_CONSTANT 0
#define OU_FLAC_KIND_VERBATIM 1
#define OU_FLAC_KIND_FIXED 2
#define OU_FLAC_KIND_LPC 3
int ou_flac_encode_choices_bytes(int32_t files, const int32_t* channels_host, const int64_t* len_host, size_t* bytes);
int ou_flac_encode_frames_level(const float* x, int64_t row_stride, int32_t files, const int32_t* channels_host,
                                const int64_t* len_host, int32_t bps, int32_t level, void* frames, size_t frames_bytes,
                                int32_t* frame_bytes, void* pcm, size_t pcm_bytes, int32_t* choices, size_t choices_bytes,
                                ou_stream_t stream);

/* ---- streaming enhance: push chunks, get finished audio (extension; the reference, and every entry point above, needs the whole
 * recording before it starts) ------------------------------------------------------------------------------------------------
 * A stream has C rows that advance in lockstep, a window length S (`segment` rounded down to a multiple of tot_ds, S >= 2 tot_ds),
 * an overlap V (`overlap` rounded down to a multiple of tot_ds, 0 <= V <= S / 2) and the stride S - V.  Nothing in its definition
 * needs a statistic of the whole row.  After T samples per row have been pushed and the stream is flushed:
 *
 *   Padded length.  T_pad = ceil(T / tot_ds) * tot_ds: zeros are appended at the END only (a stream does not know its length when
 *     it starts, so there is no front padding and a multiple of tot_ds gets no extra block).
 *   Windows (ou_stream_plan, pure host function).  T_pad <= S: one window [0, T_pad).  Else window k is [k (S - V), k (S - V) + S)
 *     for every k for which that fits into T_pad, and if the last of them ends before T_pad one more window follows at
 *     [T_pad - S, T_pad).  The crossfade between windows k and k + 1 covers [s_k + S - V, s_k + S); core k runs from the middle of
 *     one crossfade to the middle of the next, and the cores tile [0, T_pad).
 *     Relation to ou_segment_plan: for T_pad >= tot_ds, ou_stream_plan(tot_ds, T, segment, overlap) returns the windows, cores,
 *     overlap_used and T_pad of ou_segment_plan(tot_ds, T_pad - 1, segment, overlap) -- the segmented plan of any row whose padded
 *     length (which there always grows, T_raw + tot_ds - T_raw % tot_ds) is this T_pad.  The stream accepts less: S >= 2 tot_ds
 *     where the segmented calls take S >= tot_ds.
 *   Per-window result.  Window k is, by definition, ou_enhance(B = C, T_raw = the window's length) on the window's samples alone --
 *     the reference's `enhance` of that excerpt as if it were a file: its own pad, normalisation and mel scale, keep_rms too with
 *     OU_ENH_KEEP_RMS -- with the stream's n_steps, epsilon, sigma table, warm_start and OU_ENH_USE_AUX_SIGNAL, always with
 *     OU_ENH_NO_PEAK_GUARD and OU_ENH_SERIAL, on counter-based noise: window k of row c draws from the noise stream ids[c] + k of
 *     `seed`, at the positions of its own ou_enhance call (the Python layer spaces the ids of the rows by 2^32).  A noise tensor
 *     makes no sense for a call whose length is unknown: there is none.
 *   NO PEAK GUARD.  A whole-row maximum is not causal, so a stream never rescales; OU_STREAM_CLIP clamps the emitted samples to
 *     [-1, 1] instead (off by default: the samples are then what the windows gave).
 *   Stitching.  Outside the crossfade regions an output sample is the sample of the one window that covers it; where the shifted
 *     last window overlaps earlier windows beyond its crossfade region, the earlier window's samples are already emitted and stay.
 *     Inside [s_k + S - V, s_k + S), at offset i: (1 - a(i)) y_k + a(i) y_{k+1} with a(i) = 0.5 - 0.5 cos(pi (i + 0.5) / V), the
 *     fp32 weight of ou_enhance_segments' stitch (one shared device function); the expression is evaluated in fp32 with its
 *     rounding errors carried along, so the stored sample is its real value rounded once.
 *   Emission (ou_stream_emitted, pure host function of how much was pushed).  Once window k has run everything below s_k + S - V
 *     is final and is emitted: after P pushed samples that is 0 for P < S, else floor((P - S) / (S - V)) (S - V) + S - V.  The last
 *     V samples of the newest window are carried on the device (raw).  A flush runs the windows that are left, with zeros behind
 *     T -- one that would emit nothing below T is not run --, and emits up to T.
 * So the result of a stream differs from ou_enhance_segments of the same row (whose pad split, mean, gain, mix_rms, mel scale and
 * peak guard are those of the whole row); the worst-case delay between a sample's arrival and its emission is S samples.
 *
 * Workspace (ou_stream_workspace_bytes): the walk's workspace for (C, S + tot_ds), a ring of the last S input samples per row, one
 * assembled window, one window result, the carry (C, V) and the two (C, S + tot_ds) planes of the noise.  It depends on C, S and V,
 * never on the stream's length.  The caller owns it; the stream prepares the walk's part itself (ou_workspace_init, on the stream
 * of the first call that runs a window) and needs nothing in it initialised.
 *
 * Calls.  Every push and flush enqueues on the caller's stream only: no host synchronisation, no allocation on the device, no side
 * streams, no graphs; n_out comes from the plan alone and is known before anything is launched.  While a call runs the handle's
 * noise source is the stream's; when the call returns it is what it was before.  A handle is not re-entrant, and neither are the
 * streams on it; several streams may take turns on one handle, each on a workspace of its own.
 *   ou_stream_push : chunk (C, n) device, rows chunk_stride apart, n >= 0 samples per row (n may span several windows; NULL for
 *                    n = 0); out (C, out_capacity) device, rows out_stride apart, receives *n_out = ou_stream_emitted(P + n) -
 *                    ou_stream_emitted(P) samples per row, nothing behind them is written.  OU_EINVAL, before anything is
 *                    launched, when out_capacity is below that.
 *   ou_stream_flush: the same output arguments; *n_out = T - ou_stream_emitted(T).  Afterwards the stream is at position 0 with
 *                    window counter 0 again: a second identical run gives identical bytes.
 * Refused on the host with a message, before any HIP call: C < 1, S < 2 tot_ds, V > S / 2, n_steps / warm_start that ou_enhance
 * refuses, a window too long for one pass of ou_enhance, warm_start / OU_ENH_USE_AUX_SIGNAL on a model without the snake
 * decoupling layer (OU_ENOTIMPL, the message of ou_enhance), enhance flags other than OU_ENH_KEEP_RMS | OU_ENH_USE_AUX_SIGNAL, a
 * workspace that is too small (OU_ENOMEM) or not 256-byte aligned, and a push, flush or destroy on a pointer that is not a live
 * stream (destroyed, or never returned by ou_stream_create).  After a call that failed with OU_EHIP the stream refuses every call
 * but ou_stream_destroy. */
#define OU_STREAM_CLIP 1u
typedef struct ou_stream_session ou_stream_session;
typedef struct ou_stream_spec {
  int32_t C;               /* rows */
  int32_t segment;         /* samples; S = segment rounded down to a multiple of tot_ds */
  int32_t overlap;         /* samples; V likewise */
  int32_t n_steps;
  double epsilon;
  const float* sigma_host; /* n_steps floats or NULL, as ou_enhance (copied by ou_stream_create) */
  int32_t warm_start;      /* -1, or as ou_enhance */
  uint32_t enh_flags;      /* OU_ENH_KEEP_RMS | OU_ENH_USE_AUX_SIGNAL */
  uint32_t stream_flags;   /* OU_STREAM_CLIP */
  uint64_t seed;           /* key of the counter-based noise */
  const uint64_t* ids;     /* HOST, C noise stream ids (copied); window k of row c draws from ids[c] + k */
} ou_stream_spec;
/* `capacity`: entries of the four arrays (all four may be NULL: then only n_windows / overlap_used / T_pad are returned).  T >= 0;
 * T = 0 has no window. */
int ou_stream_plan(int32_t tot_ds, int64_t T, int32_t segment, int32_t overlap, int32_t capacity, int64_t* starts,
                   int32_t* lengths, int64_t* core_begin, int64_t* core_end, int32_t* n_windows, int32_t* overlap_used,
                   int64_t* T_pad);
/* Samples per row that are emitted once P have been pushed (before a flush); -1 for a bad argument (message in ou_last_error). */
int64_t ou_stream_emitted(int32_t tot_ds, int64_t P, int32_t segment, int32_t overlap);
int ou_stream_workspace_bytes(const ou_handle* h, int32_t C, int32_t segment, int32_t overlap, size_t* nbytes);
int ou_stream_create(ou_handle* h, const ou_stream_spec* spec, void* ws, size_t ws_bytes, ou_stream_session** out);
void ou_stream_destroy(ou_stream_session* s);
int ou_stream_push(ou_stream_session* s, const float* chunk, int64_t chunk_stride, int64_t n, float* out, int64_t out_stride,
                   int64_t out_capacity, int64_t* n_out, ou_stream_t stream);
int ou_stream_flush(ou_stream_session* s, float* out, int64_t out_stride, int64_t out_capacity, int64_t* n_out, ou_stream_t stream);

/* Measurement / tuning entry points (ou_profile_*, ou_bench_conv) are declared in ouniverse_tuning.h. */

#ifdef __cplusplus
}
#endif
#endif /* OUNIVERSE_H */
