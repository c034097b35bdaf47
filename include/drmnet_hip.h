/* drmnet_hip.h -- C ABI of the MI355X-native DRMNet reverse-diffusion hot path.
 *
 * One shared library (drmnet_amd/csrc/libdrmnet_hip.so), plain pointers and sizes, no torch types.
 * All tensor memory is BORROWED from the caller (device pointers, fp32, contiguous); the library owns
 * only the packed-weight storage behind its handles.  Every entry point takes an explicit hipStream_t
 * (passed as void*), launches asynchronously and never synchronises, except the documented per-step
 * convergence read-back inside drm_drmnet_sample.  Return value 0 = OK, non-zero = error code with the
 * text available from drm_last_error(); nothing throws across the ABI.
 *
 * The reference (kyotovision-public/DRMNet) is 100 % Python with no FFI of its own, so each entry point
 * names the reference Python interface it replaces (paths relative to the reference root).
 */
#ifndef DRMNET_HIP_H
#define DRMNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRM_ABI_VERSION 4
#define DRM_MAX_LEVELS 8

int drm_abi_version(void);
const char* drm_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * U-Net family.  Replaces ldm/modules/diffusionmodules/openaimodel.py:
 *   UNetModel.__init__/forward        :452-713 / :731-768   (kind 0; IllNet and ObsNet)
 *   EncoderUNetModel.__init__/forward :777-953 / :969-991   (kind 1; RefNet, pool="adaptive")
 * Only the configuration space the shipped YAMLs use is accepted (num_heads=1, conv_resample=False,
 * resblock_updown=False, use_scale_shift_norm=False, dims=2, fp32); anything else is rejected.
 * ------------------------------------------------------------------------------------------- */
typedef struct drm_unet_desc {
  int32_t kind;           /* 0 = UNetModel, 1 = EncoderUNetModel */
  int32_t in_channels;    /* channels of cat([x, cond], 1); 6 in every shipped config */
  int32_t model_channels;
  int32_t out_channels;
  int32_t num_res_blocks;
  int32_t n_levels;
  int32_t channel_mult[DRM_MAX_LEVELS];
  int32_t n_attn;
  int32_t attention_resolutions[DRM_MAX_LEVELS];
} drm_unet_desc;

typedef struct drm_unet drm_unet;

/* Builds the block topology and the parameter table (host only, no GPU needed). */
int drm_unet_create(const drm_unet_desc* desc, drm_unet** out);
void drm_unet_destroy(drm_unet* net);

/* Parameter table == the reference module's state_dict() order, names and shapes
 * (e.g. "input_blocks.1.0.in_layers.2.weight", [128,128,3,3]). */
int drm_unet_param_count(const drm_unet* net);
int drm_unet_param_info(const drm_unet* net, int index, char* name, int name_cap, int64_t shape[4], int* ndim);

/* Uploads/repacks all parameters. ptrs[i] = device pointer to fp32 tensor i in PyTorch layout.
 * Replaces nn.Module.load_state_dict + LitEma.copy_to (ldm/modules/ema.py:46-53): the host passes the
 * EMA tensors when sampling under ema_scope. May be called again to swap weights. */
int drm_unet_load_params(drm_unet* net, const float* const* ptrs, int count, void* stream);

/* Weight sets.  A handle keeps DRM_WEIGHT_SETS packed images side by side: set 0 for the module's live parameters, set 1 for
 * the EMA shadow that ema_scope swaps in around sampling (models/drmnet.py:242-258, ldm/models/diffusion/ddpm.py:189-202,
 * ldm/modules/ema.py:46-76).  Each set is packed (and, in the f16 modes, pre-split) once by drm_unet_load_params_set;
 * drm_unet_use_set selects the one the following forwards / sampler calls read -- entering and leaving the scope moves no
 * weights.  drm_unet_load_params loads into the currently selected set.  The selection is part of the handle's state: calls that
 * use one handle from several threads must agree on it. */
#define DRM_WEIGHT_SETS 2
int drm_unet_load_params_set(drm_unet* net, int set, const float* const* ptrs, int count, void* stream);
int drm_unet_use_set(drm_unet* net, int set);

/* Arithmetic of the convolution / projection kernels:
 *   0 = DRM_PREC_FP32 : v_mfma_f32_32x32x2_f32, exact fp32 products (default)
 *   1 = DRM_PREC_F16X3: every fp32 operand split into fp16 hi + lo, products evaluated as hi*hi + hi*lo + lo*hi on the f16
 *       matrix cores with fp32 accumulation (22-bit operands: fp32-level accuracy at 16/3 x the fp32 matrix rate).
 * Must be set before drm_unet_load_params (weights are pre-split at load time); drm_set_op_precision does the same for the
 * drm_op_* entry points. */
#define DRM_PREC_FP32 0
#define DRM_PREC_F16X3 1
/*   2 = DRM_PREC_F16  : REDUCED PRECISION.  Operands rounded to fp16 (weights after the same power-of-two pre-scaling), one
 *       f16 MFMA per product, fp32 accumulation, fp32 activations in HBM.  ~1e-3 rel-L2 on the full networks -- outside the
 *       1e-4 contract of the two modes above; offered for BASELINE configs[2] (the reference's reduced-precision sampling). */
#define DRM_PREC_F16 2
/*   3 = DRM_PREC_F16MX: DRM_PREC_F16X3 with the GroupNorm-fed 3x3 convs of the res blocks (80 % of a step's matrix work) evaluated as
 *       hi*hi on the f16 matrix cores + BOTH cross terms (hi*lo + lo*hi) in one block-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, OCP
 *       e4m3 operands with power-of-two block factors): 2/3 of the matrix-pipe cycles of F16X3.  The cross terms are 2^-11 of a product and
 *       carry an e4m3 rounding: 7e-6 rel-L2 per res block, 2.4e-5 .. 4e-5 per network against the reference -- inside the 1e-4 contract
 *       (tests/test_gpu_f16mx.py), an order of magnitude above F16X3's ~2e-6.  Every other launch runs exactly as in F16X3.
 *       RANGE LIMIT of this mode: the input of such a conv AFTER GroupNorm + SiLU is clipped to +-3584 (= 448 * 2^3, the e4m3 image's range)
 *       while it is staged -- F16X3 clips at fp16's 65504, FP32 not at all.  A GroupNorm output reaches at most sqrt(channels per group) *
 *       |gamma| + |beta| (<= 7 |gamma| + |beta| here), so |gamma| would have to exceed ~500 before a value gets there; such an input comes out
 *       finite and saturated, not wrapped or NaN.  Networks with GroupNorm gains of that size belong in F16X3. */
#define DRM_PREC_F16MX 3
/*   4 = DRM_PREC_BF16 : REDUCED PRECISION, BASELINE configs[2] as written ("DDIM 50-step, batch 256, bf16").  Operands rounded to bf16 (8
 *       significant bits, fp32's exponent range: no range guard needed), one v_mfma_f32_32x32x16_bf16 per product, fp32 accumulation, on the
 *       same kernels as DRM_PREC_F16 -- same speed, three mantissa bits fewer (~1e-2 rel-L2 per network against ~1e-3).  Outside the 1e-4
 *       contract; tests hold it to 3e-2. */
#define DRM_PREC_BF16 4
int drm_unet_set_precision(drm_unet* net, int precision);
/* drm_set_op_precision: the mode of the drm_op_* per-module entry points -- the library's only process-wide setting (an atomic word, read once at
 * the entry of every drm_op_* call; set it before the calls it is meant for, not concurrently with them).  Networks and samplers carry their own. */
int drm_set_op_precision(int precision);

/* Workspace (activations, statistics, attention scores) needed by one forward of batch N at HxW. */
size_t drm_unet_workspace_bytes(const drm_unet* net, int N, int H, int W);

/* kind 0: UNetModel.forward(cat([x, cond],1), timesteps=t | t_emb=t_emb) -> out [N,out_channels,H,W] NCHW.
 * kind 1: EncoderUNetModel.forward(cat([x, cond],1), timesteps)           -> out [N,out_channels].
 *   x    : [*, Cx, H, W] NCHW,  cond: [*, Cc, H, W] NCHW (Cx + Cc == in_channels; cond may be NULL if Cc == 0)
 *   rows : optional int32[N] gather indices into x/cond (DRMNet active-set compaction,
 *          models/drmnet.py:810-813); NULL = identity.
 *   t_emb: [N, model_channels] or NULL;  timesteps: int64[N] or NULL;  timesteps_f: fp32[N] or NULL
 *          (exactly one of the three; kind 1 needs timesteps / timesteps_f). */
int drm_unet_forward(drm_unet* net, const float* x, int Cx, const float* cond, int Cc, const int32_t* rows, const float* t_emb,
                     const int64_t* timesteps, const float* timesteps_f, float* out, int N, int H, int W, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Primitive ops on reference-layout tensors (NCHW activations, PyTorch weights).  They allocate their
 * own scratch and are meant for parity tests / per-module drop-ins, not for the timed path.
 * ------------------------------------------------------------------------------------------- */
/* nn.Linear with optional SiLU before/after: out[N,O] = act(b + act(in[N,I]) W[O,I]^T)
 * (time_embed, emb_layers: openaimodel.py:521-526,218-224; z_emb_layer: models/drmnet.py:38-45) */
int drm_linear_forward(const float* in, const float* w, const float* b, float* out, int N, int I, int O, int silu_in, int silu_out, void* stream);
/* timestep_embedding(timesteps, dim) (ldm/modules/diffusionmodules/util.py:151-171) */
int drm_timestep_embedding(const int64_t* timesteps, float* out, int N, int dim, void* stream);
/* [GroupNorm32 -> [SiLU] ->] conv2d k x k (k in {1,3}, stride 1, pad k/2) [+ emb[n,co]] [+ residual]
 * (ResBlock.in_layers / out_layers / skip_connection: openaimodel.py:201-241). gamma/beta NULL = no norm. */
int drm_op_norm_act_conv(const float* x, const float* gamma, const float* beta, int silu, const float* w, const float* b, int ksize,
                         const float* emb, const float* residual, float* out, int N, int Cin, int Cout, int H, int W, void* stream);
/* ResBlock._forward (openaimodel.py:255-275) on cat([x0 (optionally nearest-x2 upsampled), x1], 1).
 * params: 10 (or 12 with skip_connection) pointers in state_dict order. emb: [N, emb_dim]. */
int drm_op_resblock(const float* x0, int C0, int up0, const float* x1, int C1, const float* emb, int emb_dim, const float* const* params,
                    int n_params, float* out, int N, int Cout, int H, int W, void* stream);
/* AttentionBlock._forward (openaimodel.py:325-333, QKVAttentionLegacy :365-381), params: norm.w, norm.b, qkv.w, qkv.b, proj.w, proj.b */
int drm_op_attention_block(const float* x, const float* const* params, float* out, int N, int C, int H, int W, void* stream);
/* The stem kernel on its own: input_blocks.0.0 = conv3x3(cat([x, cond], 1)) (openaimodel.py:534, :757; ddpm.py:1527-1529) with the optional
 * row gather of models/drmnet.py:810-813.  x [B, Cx, H, W], cond [B, Cc, H, W] (NULL when Cc == 0), rows int32 [N] or NULL (then B = N),
 * w [Cout, Cx + Cc, 3, 3], b [Cout] or NULL -> out NCHW [N, Cout, H, W]; stat (optional) [N, Cout, 2] doubles = (sum, sum of squares) of each
 * output channel, zeroed by the call.  Op precision fp32 runs the exact fp32 form, every other the fp16 hi / lo split.  Only Cx + Cc in
 * {4, 6} with Cout == 128 is accepted. */
int drm_op_stem_conv(const float* x, int Cx, const float* cond, int Cc, const int32_t* rows, const float* w, const float* b, float* out, double* stat,
                     int N, int Cout, int H, int W, void* stream);
/* Downsample without conv = AvgPool2d(2, 2) (openaimodel.py:154-160): x NCHW [N, C, H, W] -> out NCHW [N, C, H/2, W/2]; stat (optional)
 * [N, C, 2] doubles = (sum, sum of squares) of each output channel, zeroed by the call.  C % 4 == 0, H and W even. */
int drm_op_avgpool2(const float* x, float* out, double* stat, int N, int C, int H, int W, void* stream);
/* The tail of EncoderUNetModel's head, pool="adaptive" (openaimodel.py:922-929), on GroupNorm tables the caller supplies:
 * out[n][o] = b[o] + sum_c w[o][c] mean_hw(silu(x[n][c] * scale[n][c] + shift[n][c])).  x NCHW [N, C, H, W], scale, shift [N, C], w [O, C],
 * b [O] -> out [N, O].  C % 4 == 0. */
int drm_op_encoder_head(const float* x, const float* scale, const float* shift, const float* w, const float* b, float* out, int N, int C, int H, int W,
                        int O, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Samplers.
 * ------------------------------------------------------------------------------------------- */
typedef struct drm_drmnet_cfg {
  int32_t z_dim;          /* len(z0), 6 in the shipped config */
  int32_t max_timesteps;
  double gamma;           /* double: the reference evaluates gamma^i = exp(i ln gamma) in fp64 (models/drmnet.py:494-495) */
  float epsilon, delta;   /* compared / multiplied in fp32 like the reference's tensor-scalar ops */
  float z0[8];            /* mirror-reflectance code (configs/drmnet/eval_drmnet.yaml: z0) */
} drm_drmnet_cfg;

typedef struct drm_drmnet drm_drmnet;

/* DRMNet reverse process over (RefNet, IllNet, z_emb_layer). Borrows the two nets (caller keeps them alive).
 * zemb: 6 device pointers = ZEmbDiffusionWrapper.z_emb_layer.{0,2,4}.{weight,bias} (models/drmnet.py:38-45). */
int drm_drmnet_create(drm_unet* illnet, drm_unet* refnet, const float* const* zemb, const drm_drmnet_cfg* cfg, drm_drmnet** out);
void drm_drmnet_destroy(drm_drmnet* s);
size_t drm_drmnet_workspace_bytes(const drm_drmnet* s, int N, int H, int W);
/* Batch parts of a reverse step (default 2; 1 = off; at most 4): a step over at least 64 rows per part runs its row ranges on internal streams
 * forked from and joined back into `stream`, so the sparse launches of one range (deep levels, small kernels) overlap with the other's.  The rows
 * of the reference's loop are independent (models/drmnet.py:809-839): results are those of the ranges run one after the other.  Call before
 * drm_drmnet_workspace_bytes (the workspace covers the parts' slices); a workspace that does not hold the slices makes the step run unforked, not fail.
 * NOT bitwise: a range of n / parts rows can take other tile shapes and split-K forms than the whole batch, so a row's result depends on the batch size
 * and on `parts` at the level of the arithmetic mode's rounding (f16x3: < 2e-5 rel-L2 over a recorded loop). */
int drm_drmnet_set_batch_parts(drm_drmnet* s, int parts);
/* Rows per part from which a step is forked (default 64: below it the ranges fall to the narrow conv tiles and the overlap loses, 817 vs 852 steps/s at
 * 32 rows); tests set 1 to drive tiny batches through the forked form.  Replaces the DRM_BATCH_PARTS / DRM_BATCH_PART_MIN environment reads of r5. */
int drm_drmnet_set_batch_part_min(drm_drmnet* s, int rows);

/* One reverse step on the active rows (DRMNet.p_mean_variance + the loop body, models/drmnet.py:752-770,809-839):
 *   z_out = RefNet(cat[Lr_k, LrK], i); zk = clamp(z0 + gamma^i (z_out - z0)); out = IllNet(cat[Lr_k, LrK], z_emb(zk - z0));
 *   Lr_k[rows] += out (+ delta * noise on rows that did not converge).
 * Lr_k, LrK: [B,3,H,W]; rows: int32[n_active] (device); noise: [B,3,H,W] or NULL (then Philox(seed, step));
 * zk_out / zK_out: [n_active, z_dim]; converged_out: int32[n_active] (device). */
int drm_drmnet_step(drm_drmnet* s, float* Lr_k, const float* LrK, const int32_t* rows, int n_active, int step, const float* noise,
                    uint64_t seed, float* zk_out, float* zK_out, int32_t* converged_out, int B, int H, int W, void* workspace,
                    size_t workspace_bytes, void* stream);

/* DRMNet.p_sample_loop (models/drmnet.py:782-847): LrK [B,3,H,W] (+ cond [B,3,H,W], the concat conditioning of both
 * nets; == LrK unless sigma_for_cond_xK > 0, models/drmnet.py:1037-1043) -> Lr0 [B,3,H,W], zK [B,z_dim] (NaN if never
 * converged), K int32[B].  noise0 [B,3,H,W] / step_noise [max_timesteps,B,3,H,W] or NULL (Philox).
 * early_exit = 0 keeps every row active for max_timesteps steps (countable-steps benchmark mode).
 * Synchronises the stream once per step to read the convergence flags (the reference does the same,
 * models/drmnet.py:841).  steps_done returns the number of executed steps. */
int drm_drmnet_sample(drm_drmnet* s, const float* LrK, const float* cond, const float* noise0, const float* step_noise, uint64_t seed, int early_exit,
                      float* Lr0, float* zK, int32_t* K, int32_t* steps_done, int B, int H, int W, void* workspace, size_t workspace_bytes,
                      void* stream);

/* The samplers' `mask` / `x0` arguments (known-region blending): img = q_sample(x0, t) * mask + (1 - mask) * img with
 * q_sample(x0, t) = sqrt(a_bar_t) x0 + sqrt(1 - a_bar_t) noise (ddpm.py:1052-1058).  Where and at which t it is applied differs between the three
 * reference loops, so the caller supplies the (a, b) pair of every chain step and the side of the step:
 *   DDIMSampler.ddim_sampling      ldm/models/diffusion/ddim.py:175-178   before the step's forward, at the step's t            -> when = 0
 *   ObsNetDiffusion.p_sample_loop  models/obsnet.py:545-547               before p_sample: x0 itself at t == 0, else t - 1       -> when = 0
 *   LatentDiffusion.p_sample_loop  ldm/models/diffusion/ddpm.py:1300-1302 after p_sample, at the step's t                       -> when = 1
 * (`temperature` of p_sample_ddim / p_sample, ddim.py:255 / ddpm.py:1157, needs no entry point: it scales the sigma column of `coef`.)  Passed through
 * drm_sampler_options below.
 * struct_bytes, here and in every struct a caller fills: the caller sets it to the struct's sizeof; a library that was built with another
 * size returns DRM_ERR_INVALID, naming the struct and both sizes, before it reads any other member. */
typedef struct drm_mask_blend {
  uint32_t struct_bytes;
  const float* mask;   /* [N, mask_channels, H, W], device */
  int mask_channels;   /* 1 (broadcast over the channels) or 3 */
  const float* x0;     /* [N,3,H,W], device */
  const float* qcoef;  /* float[steps][2], host: (a, b) of chain step j (j = 0 is the first executed step) */
  const float* qnoise; /* [steps][N,3,H,W] device (the draws of q_sample), or NULL: Philox(seed) under a key of its own */
  int when;            /* 0 = before the step's network forward, 1 = after its update */
} drm_mask_blend;

/* The remaining per-step options of the reference's samplers, in one struct (zero-initialise, then struct_bytes; every other member optional):
 *   blend          mask / x0 (above)
 *   uncond         DDIM only -- classifier-free guidance (p_sample_ddim, ldm/models/diffusion/ddim.py:225-232): the unconditional conditioning
 *                  [N,3,H,W]; every step evaluates the network on it as well and uses e = e_uncond + guidance_scale * (e_cond - e_uncond).  (The
 *                  reference batches both evaluations as 2 N rows; rows do not interact.)
 *   noise_dropout  F.dropout on the step noise (ddim.py:256-257, ddpm.py:1158-1159): an element is kept with probability 1 - p and scaled by
 *                  1 / (1 - p); dropout_keep [steps][N,3,H,W] holds 0 / 1 keep masks (parity runs), NULL draws them from Philox(seed) under a key of
 *                  its own.
 * Not offered: score correctors, quantize_denoised, callbacks (host hooks of the reference with no device meaning here). */
typedef struct drm_sampler_options {
  uint32_t struct_bytes;
  const drm_mask_blend* blend;
  const float* uncond;
  float guidance_scale;
  float noise_dropout;
  const float* dropout_keep;
} drm_sampler_options;

/* The reference's `intermediates` of the DDIM chain (ddim.py:171-204: after the step of `index`, (img, pred_x0) are appended when
 * index % every_t == 0 or at the first step): slot k of x / pred_x0 ([slots][N,3,H,W] each, device) receives the k-th appended pair,
 * *n_logged (host, may be NULL) the number of pairs.  The steps that log are marked in the device step table, so graph replay applies unchanged.
 * every_t <= 0: no intermediates, whatever the buffers.  every_t > 0 without both buffers and slots > 0 is DRM_ERR_INVALID. */
typedef struct drm_chain_log {
  uint32_t struct_bytes;
  int32_t every_t;
  float* x;
  float* pred_x0;
  int32_t slots;
  int32_t* n_logged;
} drm_chain_log;

/* DDIM sampling (DDIMSampler.ddim_sampling + p_sample_ddim, ldm/models/diffusion/ddim.py:128-259).
 *   timesteps: int64[S] (host) ddim_timesteps; coef: float[S][5] (host) = sqrt(a_t), sqrt(1-a_t), sqrt(a_prev),
 *   sqrt(1-a_prev-sigma^2), sigma per index; runs index S-1 .. 0 (or the first num_steps of them).  Synchronises the stream once
 *   at entry (upload of the per-step table).
 *   x: [N,3,H,W] in = x_T, out = final x;  cond: [N,3,H,W];  noise: [steps,N,3,H,W] or NULL (Philox).
 *   opt: NULL means zero options;  log: NULL means no intermediates.  Graph replay applies whatever they hold (every per-step quantity lives
 *   in a device table read through the step counter). */
int drm_ddim_sample(drm_unet* net, float* x, const float* cond, const int64_t* timesteps, const float* coef, int S, int num_steps,
                    const float* noise, uint64_t seed, const drm_sampler_options* opt, const drm_chain_log* log, int N, int H, int W,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Ancestral DDPM (LatentDiffusion.p_sample via ObsNetDiffusion.p_sample_loop, ldm/models/diffusion/ddpm.py:1079-1167,
 * models/obsnet.py:500-564).  coef: float[T][5] (host) = sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod,
 * posterior_mean_coef1, posterior_mean_coef2, exp(0.5*posterior_log_variance_clipped) for t = 0..T-1; runs t = T_start-1 .. 0.
 * x: in = x_T, out = last img; pred_x0: [N,3,H,W] out (what ObsNetDiffusion.p_sample_loop returns).
 * opt: NULL means zero options; opt->uncond must be NULL (guidance exists on the DDIM chain only). */
int drm_ddpm_sample(drm_unet* net, float* x, float* pred_x0, const float* cond, const float* coef, int T_start, int clip_denoised,
                    const float* noise, uint64_t seed, const drm_sampler_options* opt, int N, int H, int W, void* workspace, size_t workspace_bytes,
                    void* stream);

size_t drm_sampler_workspace_bytes(const drm_unet* net, int N, int H, int W);

/* drm_ddim_sample / drm_ddpm_sample keep every per-step scalar (timestep, coefficients, noise offset) in a device table indexed
 * by a device counter, so all steps issue the same launches: the first step runs eagerly, the second is captured into a hipGraph
 * and the rest of the chain replays it (BASELINE configs[2] "hipGraph-captured step").  Off by default (measured on MI355X:
 * within +-0.5 % of eager launches at batch 32 / 256, 4-8 % slower at batch 1 where the instantiation is not amortised); when on
 * it applies to chains of >= 4 steps and steps aside while the launch profiler records (events do not belong in a graph).  With replay the call returns after the chain has
 * finished (the executable graph is destroyed behind its last launch).  drm_graph_launches counts hipGraphLaunch calls so far. */
int drm_set_graph_replay(int on);

/* The in_layers conv of a ResBlock whose input is cat(nearest_x2(x0), x1) (first block of every finer decoder level) can run as two
 * launches: the four parity 2x2 convs on the stored x0 (4 taps in place of 9, pixel-shuffled into the output) and the 3x3 conv on x1
 * that adds bias, embedding and the first launch's result.  mode 0 = never, 1 = where the measured per-level rule says it is faster
 * (default), 2 = wherever the form applies (whole-tile, un-split launches, batch > 4).  Same function either way (fp32 reassociation of
 * the nine taps into four); library-level, for tests and A/B measurements. */
int drm_set_upconv_split(int mode);
int64_t drm_graph_launches(void);

/* Launch profiler (HIP events on the launch stream around each kernel family; used by bench.py for the roofline
 * object).  Kinds: 0 conv3x3 (fused GN+SiLU+conv implicit GEMM), 1 conv1x1 (skip / qkv / proj), 2 attention core,
 * 3 GroupNorm statistics, 4 other.  drm_profile_enable(1) instruments every family, (2) only kind 0 -- the dominant
 * kernel, ~90 instead of ~600 event pairs per step, which perturbs a timed region by < 0.5 % instead of ~3 %; (0) off.
 * drm_profile_collect synchronises the recorded events and returns totals since the last drm_profile_reset: each array
 * has DRM_PROFILE_KINDS entries. */
#define DRM_PROFILE_KINDS 5
void drm_profile_enable(int on);
void drm_profile_reset(void);
int drm_profile_collect(double* ms, double* flops, double* bytes, int64_t* launches);
/* Per kernel INSTANTIATION of the conv families (the name rocprofv3 prints): one text line "name\tkind\tlaunches\tms\tflops\tbytes\n" each,
 * totals since the last drm_profile_reset as of the last drm_profile_collect.  Writes at most cap - 1 characters + NUL into buf (may be
 * NULL) and returns the size needed.  Lets a per-launch PMC figure of ONE instantiation (HBM bytes) be set against the algorithmic bytes
 * of the same launches rather than a family mean. */
size_t drm_profile_variants(char* buf, size_t cap);

/* Standard-normal fill from the library's Philox4x32-10 stream (throughput mode noise source). */
int drm_randn(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream);

/* Object image -> reflectance map, the step in front of the samplers (reference: refmap_mask_make,
 * utils/img2refmap.py:6-37, with xyz2thetaphi(normal = [0,1,0], tangent = [-1,0,0]), utils/transform.py:55-89).
 *   colors  [n][channels], normals [n][3]: the object pixels (fp32, device).  res: the map is res x res texels over
 *   (theta, phi) in (0, pi)^2.  A texel takes the colour of the pixel whose colour SUM is the lower median
 *   (torch.nanmedian) among the pixels with max(|theta - theta_i|, |phi - phi_j|) <= angle_threshold (fp32 compare);
 *   fewer than min_points such pixels, or none with a non-NaN sum, leaves it zero / unmasked.
 *   refmap [res][res][channels] fp32, refmask [res][res] uint8 (0/1).
 * Synchronises the stream once (capacity check of the binning lists). */
size_t drm_refmap_workspace_bytes(int64_t n, int res, float angle_threshold);
int drm_refmap_mask_make(const float* colors, const float* normals, int64_t n, int channels, int res, float angle_threshold, int min_points,
                         float* refmap, uint8_t* refmask, void* workspace, size_t workspace_bytes, void* stream);

/* Mask erosion of scripts/estimate.py:43-50: a mask pixel is dropped when a non-mask pixel lies inside the disk
 * footprint of diameter kernel_size around it (zero "same" padding: the image border does not erode).  uint8 0/1, [H][W]. */
int drm_erode_mask(const uint8_t* mask, int H, int W, int kernel_size, uint8_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The elementwise maps either side of the samplers, and the envmap warp / tone map after them.
 * ------------------------------------------------------------------------------------------- */
/* BaseDataset.transform / rescale (dataset/basedataset.py:29-112): a transform_func string such as
 * "resize_0p1tom1p1_normalizedLogarithmic_lowerbound1e-6" is a chain of named maps (applied right to left; rescale applies
 * the inverses left to right).  drm_map_chain applies up to 8 maps per element in one pass: x, out [B][per_image] fp32
 * (out may alias x), ops[n_ops] the DRM_MAP_* codes in application order, args[n_ops] their scalar argument.
 *   lo / hi : fp32[B] per-image (log10 min, log10 max) of "normalizedLogarithmic" (NULL unless DRM_MAP_NORM_LOG / _DENORM_LOG is used)
 *   scale   : fp32[B] per-image factor of DRM_MAP_IMG_MUL / _IMG_DIV (DRMNet.normalizing_scale, models/drmnet.py:1020-1027;
 *             scripts/estimate.py:99-100) */
#define DRM_MAP_LOG_P1 0          /* "log":    log10(x + 0.1) + 1                                   basedataset.py:52-53  */
#define DRM_MAP_LOG10 1           /* "log10":  log10(x)                                             :54-55                */
#define DRM_MAP_LOWERBOUND 2      /* "lowerbound<b>": clip(x, min = arg)                            :56-58                */
#define DRM_MAP_UNIT_TO_SIGNED 3  /* "0p1tom1p1": 2 x - 1                                           :59-60                */
#define DRM_MAP_NORM_LOG 4        /* "normalizedLogarithmic": (log10 x - lo[b]) / (hi[b] - lo[b])   :61-76                */
#define DRM_MAP_EXP_M1 5          /* inverse of "log":  10^min(x - 1, arg) - 0.1  (arg = clamp_before_exp, +inf = none)  :88-92 */
#define DRM_MAP_EXP10 6           /* inverse of "log10": 10^min(x, arg)                             :93-97                */
#define DRM_MAP_SIGNED_TO_UNIT 7  /* inverse of "0p1tom1p1": (x + 1) / 2                            :100-101              */
#define DRM_MAP_DENORM_LOG 8      /* x (hi[b] - lo[b]) + lo[b]  (followed by DRM_MAP_EXP10)         :102-112              */
#define DRM_MAP_IMG_MUL 9         /* x * scale[b] */
#define DRM_MAP_IMG_DIV 10        /* x / scale[b] */
#define DRM_MAP_CLIP0 11          /* clip(x, min = 0)                                               scripts/estimate.py:97 */
int drm_map_chain(const float* x, float* out, int64_t per_image, int B, const int32_t* ops, const float* args, int n_ops, const float* lo,
                  const float* hi, const float* scale, void* stream);
/* dynamic_normalize branch of "normalizedLogarithmic" (basedataset.py:63-69): per image b of x [B][C][HW] with mask [B][HW]
 * (fp32 0/1, broadcast over channels): linearmax = max(x mask); hi[b] = log10(linearmax); lo[b] = log10(min(x mask + (1 - mask) linearmax)). */
int drm_masked_log_range(const float* x, const float* mask, int B, int C, int HW, float* lo, float* hi, void* stream);
/* models/drmnet.py:1020-1026: scale[b] = scaler / exp(mean over {L > 0} of log(clip(L, 1e-5))), L = Rec.709 luminance of x[b] ([B][3][HW]). */
int drm_luminance_scale(const float* x, int B, int HW, float scaler, float* scale, void* stream);
/* mirmap2envmap (utils/transform.py:106-144; view +z, top +y, zenith +y, left edge -z, reverse_azimuth -- the only configuration
 * the reference supports) fused with the basis_r0 division of DRMNet.r0toenvmap (models/drmnet.py:931-941; basis [C][H][W] or
 * NULL): mirmap [B][C][H][W] -> out [B][C][OH][OW], or [B][OH][OW][C] when channels_last (what r0toenvmap returns).
 * Bilinear, border padding, align_corners = False (torch.nn.functional.grid_sample arithmetic). */
int drm_mirmap2envmap(const float* mirmap, const float* basis, float* out, int B, int C, int H, int W, int OH, int OW, int log_scale_interpolation,
                      int channels_last, void* stream);
/* hdr2ldr (utils/tonemap.py:4-9): x [HW][3] one channels-last image, mask uint8[HW] or NULL -> out [HW][3] in [0, 1]. */
int drm_hdr2ldr(const float* x, const uint8_t* mask, int HW, float alpha, float gamma, float* out, void* stream);
/* The "resize" map of BaseDataset.transform (dataset/basedataset.py:44-50: torchvision.transforms.functional.resize(x, (size, size),
 * interpolation, antialias=True) = torch's anti-aliased separable bilinear / bicubic filter, align_corners = False) and the nearest
 * mask resize of ObsNetDiffusion.get_cond_for_predict (models/obsnet.py:691: torch.nn.functional.interpolate(mask, size)).
 * x [planes][IH][IW] -> out [planes][OH][OW] fp32 (planes = every leading dimension flattened).  Down-scaling factors up to 23
 * (bicubic) / 47 (bilinear); beyond that DRM_ERR_ARG. */
#define DRM_RESIZE_NEAREST 0
#define DRM_RESIZE_BILINEAR_AA 1
#define DRM_RESIZE_BICUBIC_AA 2
int drm_resize(const float* x, float* out, int planes, int IH, int IW, int OH, int OW, int mode, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The rest of the reference's sphere / environment-map warps (csrc/sphere_warp.hip): one gather-and-pool kernel, a map per warp.
 * Common to the four entries: the input is [B][C][H][W], or [B][H][W][C] when channels_last_in (what the EXR reader and the renderers
 * give); the output is always [B][C][OH][OW]; every fetch is torch.nn.functional.grid_sample(bilinear, padding_mode="border",
 * align_corners=False) arithmetic, so the azimuth seam is clamped, not wrapped, as in the reference.  `frames` is a device array
 * [B][k][3] fp32, one set of frame vectors per item, built by the caller the way the reference builds them: a binormal is
 * cross(normal, tangent), negated where the reference passes reverse_phi.  The vectors are used as given (the reference's
 * assume_normalized): a frame that is not orthonormal warps accordingly.  Item b depends on its own input and frame alone, and the
 * results are deterministic.  DRM_ERR_INVALID for a NULL pointer, B or C < 1 or a side outside [1, 16384]: nothing is launched.
 * ------------------------------------------------------------------------------------------- */
/* envmap2mirmap (utils/transform.py:201-242): a lat-long environment map and a viewer position -> the mirror reflectance map.
 * frames [B][6][3]: top (re-orthogonalised against view_from by the caller, :217-218), view_from, cross(top, view_from) (negated for
 * flip_horizontal); envmap_zenith, envmap_left_edge, cross(zenith, left_edge) (negated for reverse_azimuth_envmap).
 * With mitigate_aliasing the reference samples an S x S grid (S = min(H, W) if OH < H, else max(OH, OW)) and reduces it with
 * adaptive_avg_pool2d; here each output pixel averages its own pool window [floor(i S / OH), ceil((i + 1) S / OH)) directly and the
 * S x S intermediate never exists: one wave per pixel when every window holds 64 samples or more, one thread per pixel otherwise.
 * log_scale_interpolation: taps are log(max(t, 1e-7)), the mean is taken in the log domain, exp follows the pool. */
int drm_envmap2mirmap(const float* envmap, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int mitigate_aliasing,
                      int log_scale_interpolation, int channels_last_in, void* stream);
/* rotate_envmap (utils/transform.py:317-363): a lat-long map re-expressed in another frame.  frames [B][6][3]: tgt_envmap_zenith,
 * tgt_envmap_left_edge, -cross(of the two); src_envmap_zenith, src_envmap_left_edge, -cross(of the two). */
int drm_rotate_envmap(const float* envmap, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int channels_last_in,
                      void* stream);
/* mirimg2envmap (utils/transform.py:245-284): an orthographic mirror-ball image -> the lat-long map.  frames [B][7][3]: envmap_zenith,
 * envmap_left_edge, cross(of the two) (negated for reverse_azimuth); top (re-orthogonalised, :264-265), t = cross(view_from, top),
 * cross(top, t); view_from. */
int drm_mirimg2envmap(const float* refimg, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int log_scale_interpolation,
                      int channels_last_in, void* stream);
/* refmap2refimg_torch (utils/transform.py:170-198, with gen_sphere_normals_realcentering :147-167): a reflectance map in the (theta, phi)
 * parametrisation -> the ball image out [B][C][2 radius][2 radius]; pixels outside the disc are written 0.  mask uint8 [2 radius][2 radius]
 * (1 inside the disc) or NULL.  radius in [1, 8192]. */
int drm_refmap2refimg(const float* refmap, float* out, uint8_t* mask, int B, int C, int H, int W, int radius, int channels_last_in, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The forward model DRMNet inverts: reflectance maps of a sphere lit by an environment map (csrc/render.hip).
 * ------------------------------------------------------------------------------------------- */
/* What the B rows of any render share: a material, an environment, a view, a quadrature and optional light samples.  Zero-initialise, set
 * struct_bytes = sizeof(drm_shading), then the members in use.  All pointers are device pointers.
 *   Material: exactly one of z and tables (both, or neither, is DRM_ERR_INVALID).
 *     z: principled rows, [B][6], or [L][B][6] for the sphere.  A row is canonical: z[6] = (metallic, base colour R, G, B, roughness, specular),
 *     each clipped to [0, 1] by the kernels.  The BSDF is Mitsuba 3's "principled" with every other parameter 0 (GGX alpha =
 *     max(0.001, roughness^2), eta = 2 / (1 - sqrt(0.08 specular)) - 1).
 *     tables, NT, table_of, table_alpha, table_linear: measured BRDFs ("Measured BRDFs" below states the packed layout, the lookup and the
 *     checks made of them).  Row b is under table table_of[b] (NULL: table 0 for all); table_alpha [NT]: the proxy roughness of each table,
 *     in [0.005, 1]; table_linear: the lookup.  Under tables there are no stacks (L == 1), no light samples under a map and no bounces,
 *     and a mesh goes through drm_render_mesh_tables, not drm_render_mesh: otherwise DRM_ERR_INVALID.  1 <= B <= 65535.
 *   envmap [B][EH][EW][3]: channels-last lat-long maps (texel (i, j) looks along theta = (i + 1/2) pi / EH, psi = (j + 1/2) 2 pi / EW,
 *     (sin theta sin psi, cos theta, -sin theta cos psi); bilinear, wraps in psi, clamps in theta), or NULL for a white environment (L = 1;
 *     EH, EW and the view are then not read).
 *   view [B][9] or NULL: row-major rotations Rot.  Every light direction l of the quadrature (in the frame whose viewer is +z) is looked up
 *     in the environment at Rot l.  For the reference's look_at(origin = v, target = 0, up = +y) (utils/mitsuba3_utils.py:394-396) the columns
 *     of Rot are (right, up', back): back = v / |v|, right = normalize(+y x back), up' = back x right.  NULL and an exact identity skip the
 *     rotation (they are not multiplied by it), so the view from +z is the render without a view bit for bit.
 *   quad in [1, 1024] (32 by default in the Python layer): the integral is a deterministic quadrature, a quad x quad stratified grid per lobe
 *     (GGX-sampled half vectors for the specular lobe, cosine-weighted directions for the diffuse one); bitwise reproducible.
 *   light_samples = M: light sampling, for maps with small bright lights (a sun, a lamp) that fall between the strata of a rough lobe's
 *     quadrature.  M directions are drawn from each map's own light density and combined with the two lobe quadratures by lobe-separated
 *     multiple importance sampling, power heuristic (beta = 2).
 *     Light density.  On the dual grid of the bilinear lookup: cell (c, j), c = 0 .. EH, j = 0 .. EW - 1, spans theta in
 *     [(c - 1/2), (c + 1/2)] pi / EH clipped to [0, pi] and psi in [(j + 1/2), (j + 3/2)] 2 pi / EW; its corners are the texels
 *     (clamp(c - 1), clamp(c)) x (j, j + 1 mod EW), valued at their Rec. 709 luminance clamped at 0.  Density with respect to (theta, psi):
 *     val sc_c / (tot dpsi), val the bilinear interpolant of the corners, sc_c the sine of the row's mid colatitude, tot the sum over cells of
 *     mean4(corners) sc_c (hi_c - lo_c); p_L(w) = density / max(sin theta, 1e-6).
 *     Samples.  Sample k is the Hammersley point ((k + 1/2) / M, bitreverse32(k) 2^-32 + 1 / (2 M)) taken through the marginal CDF over rows, the
 *     row's conditional CDF over columns and the inverse of the bilinear density inside the cell.  fp64, fixed order, no atomics.
 *     Estimator.  With n_s = n_d = quad^2 (n_d = 0 for a metal) and n_L = M: each lobe sample is weighted by (n p)^2 / ((n p)^2 + (n_L p_L)^2),
 *     p = G1(v) D(h) / (4 n.v) for the specular lobe and n.l / pi for the diffuse one; light sample k with n.l_k > 0 adds
 *     L_k [f_s cos n_L p_L / ((n_s p_s)^2 + (n_L p_L)^2) + f_d cos n_L p_L / ((n_d p_d)^2 + (n_L p_L)^2)] / subpixel^2.
 *     M is 0, or a power of two in [64, 65536] (anything else is DRM_ERR_INVALID).  0, or envmap == NULL, makes exactly the launches of the
 *     render without light samples -- the same bytes -- and the light workspace is neither read nor written.  With light samples
 *     1 <= B <= 65535.  A map whose tot is 0 (black, or all non-positive) has no light technique: its rows are the plain quadrature.
 *   light_workspace: at least drm_render_light_workspace_bytes(B, EH, EW, light_samples) bytes of device memory, 8-byte aligned; one table per
 *     map b, rebuilt by every call (three small launches before the shading launch) and holding nothing the caller needs.  A missing,
 *     misaligned or short one is DRM_ERR_WORKSPACE on the sphere and DRM_ERR_INVALID for normal maps and meshes: nothing is launched. */
typedef struct drm_shading {
  uint32_t struct_bytes;
  int32_t B;
  const float* z;
  const float* tables;
  int32_t NT;
  const int32_t* table_of;
  const float* table_alpha;
  int32_t table_linear;
  const float* envmap;
  int32_t EH, EW;
  const float* view;
  int32_t quad;
  int32_t light_samples;
  void* light_workspace;
  size_t light_workspace_bytes;
} drm_shading;
size_t drm_render_light_workspace_bytes(int B, int EH, int EW, int light_samples); /* 0 for arguments the renders reject */

/* Reflectance maps of a sphere: L stacked sets of B rows, each batch item under its own map and view, in one launch.  Replaces
 * MitsubaRefMapRenderer.rendering (utils/mitsuba3_utils.py:324-430: sphere, "envmap" emitter, "direct" integrator, RefMapSensor :14-89 at +z
 * looking at -z, box filter), the basis_r0 render of DRMNet.instantiate_brdf_model (models/drmnet.py:328-347) and what DRMNet.get_input /
 * rendering_refmaps ask of the renderer (models/drmnet.py:559-569, 667-705: a Python loop of rendering(z, envmap, view_from) calls, one scene
 * update and one render per (stack, batch) item).
 *   out [L][B][3][R][R]: row (l, b) is lit by envmap[b] and seen through view[b]: the L rows of a batch item index the same map, nothing is
 *   expanded.  Pixel (i, j) is the mean over its footprint of the radiance the sphere reflects toward +z at the normal
 *   n = (cos b sin a, sin b, cos b cos a), a = (2 px - 1) pi / 2, b = (1 - 2 py) pi / 2 (flip != 0 negates n.x): subpixel x subpixel normals
 *   per pixel, each with the quadrature of the shading.  subpixel in [1, 16] (2 by default in the Python layer); L >= 1, B >= 1, L B < 2^31,
 *   1 <= R <= 8192.  One wave per pixel, fixed per-lane order and butterfly, no atomics: every row is summed in the same per-lane order
 *   whatever L is, so a stacked render equals its rows rendered one by one, and a batch its rows alone.
 *   Under tables (MitsubaRefMapRenderer.rendering with a measured BSDF): the same sensor and sub-pixel normals.  The quadrature per normal n
 *   (v = +z): the quad x quad midpoint grid mapped to the GGX visible normals of roughness alpha seen from v with l = reflect(v, h), and the
 *   same grid mapped to cosine-weighted directions (the two constructions of the principled render); a sample l of either set with n.l > 0
 *   (a GGX sample also v.h > 0 and D > 0) adds
 *     L(Rot l) f_table(n, v, l) (n.l) / (quad^2 (p_s(l) + p_d(l))),  p_s = G1(v) D(h) / (4 n.v) at h = normalize(v + l),  p_d = (n.l) / pi
 *   (the balance heuristic over both sets: consistent for any alpha, which only decides where the accuracy goes); the pixel is the sum
 *   over both sets and the subpixel^2 normals, divided by subpixel^2.  All in fp32.
 *   DRM_ERR_INVALID for a bad size, quadrature, material or light_samples, DRM_ERR_WORKSPACE for the light workspace: nothing is launched. */
int drm_render_refmap(const drm_shading* shading, int L, int R, int subpixel, int flip, float* out, void* stream);

/* Object images from a normal map: the forward model pointed at the inputs of the estimate (an object image, its normal map, a mask), with
 * no mesh behind it.  The two entries complement MitsubaOrthoRenderer (utils/mitsuba3_utils.py:433-564), which needs the mesh, and
 * DRMNet.reconstruct (models/drmnet.py:943-953), which renders the estimate back onto the sphere only.
 *   normals [Bn][H][W][3]: channel-last, as normal.npy holds them, in the view frame (right, up, back); mask [Bn][H][W] uint8 or NULL;
 *   Bn = 1 (one normal map for all B rows: one object relit B ways) or B.  n = the normal divided by its length (any length is taken).
 *   A pixel is not drawn -- image 0, alpha 0 -- where the mask is 0, where the normal is zero or has a NaN or infinite component, and
 *   where n.z <= 0 (it does not face the viewer at +z).  image [B][3][H][W]; alpha [B][H][W], 1.0 where drawn, may be NULL.
 *   Limits: 1 <= B <= 65535, H and W in [1, 4096].
 * drm_render_normals (csrc/render_shared.h, normals_pixel_kernel): every drawn pixel is the radiance its normal reflects toward +z under row b
 *   of the shading, exactly as drm_render_refmap shades the sphere point and drm_render_mesh the mesh hit with that normal: one wave per pixel,
 *   the same quad x quad grids, per-lane order and butterfly, subpixel = 1 (under tables: the per-normal sum of the sphere's table render, so a
 *   pixel whose normal is a sphere normal equals that render's pixel bit for bit).  The view turns the environment lookups only (a lobe
 *   direction l is looked up at Rot l); the normals are already in the view frame.  Light samples: the same tables, built by the same three
 *   launches, the same estimator with subpixel = 1.
 *   Bitwise reproducible; a call of B rows equals its rows alone, and Bn = 1 equals the normal map repeated B times.
 *   DRM_ERR_INVALID for Bn outside {1, B}, sizes outside the limits, a bad quadrature, material or light_samples, or a missing, misaligned
 *   or short light workspace: nothing is launched.
 * drm_image_from_refmap (csrc/refmap.hip, image_from_refmap_kernel): every drawn pixel reads a given reflectance map at its normal -- what
 *   the image would be if the reflectance-map model held exactly; the inverse of drm_refmap_mask_make's gather.  One thread per pixel.
 *   refmap [Br][3][R][R] channel-first, as drm_render_refmap writes it and the networks return it; refmask [Br][R][R] uint8 or NULL;
 *   Br = 1 or B; 1 <= R <= 8192.
 *   Texel coordinates: the inverse of the sensor's n = (cos b sin a, sin b, cos b cos a) (drm_render_refmap, flip = 0), which is also the
 *   parametrisation of drm_refmap_mask_make (theta from +y, phi = atan2(n.z, -n.x)):  a = atan2f(n.x, n.z), b = asinf(n.y) (n.y clamped to
 *   [-1, 1]);  tj = (a / pi + 0.5) R - 0.5, ti = (0.5 - b / pi) R - 0.5: texel (i, j)'s centre maps to (ti, tj) = (i, j).
 *   Bilinear over the taps (i0, i1) x (j0, j1) = (floor ti, floor ti + 1) x (floor tj, floor tj + 1), every index clamped to [0, R - 1], with
 *   fy = ti - floor ti, fx = tj - floor tj, added in this order (fp32, no contraction):
 *     top = (1 - fx) v[i0][j0] + fx v[i0][j1];  bot = (1 - fx) v[i1][j0] + fx v[i1][j1];  value = (1 - fy) top + fy bot.
 *   With a refmask a pixel is drawn only if all four clamped taps are observed (non-zero), whatever their weights: the rule depends on
 *   floor ti and floor tj alone, so it changes only where a coordinate crosses an integer.
 *   DRM_ERR_INVALID for Bn or Br outside {1, B} or sizes outside the limits: nothing is launched. */
int drm_render_normals(const drm_shading* shading, const float* normals, const uint8_t* mask, int Bn, int H, int W, float* image, float* alpha,
                       void* stream);
int drm_image_from_refmap(const float* refmap, const uint8_t* refmask, int Br, int R, const float* normals, const uint8_t* mask, int Bn, float* image,
                          float* alpha, int B, int H, int W, void* stream);

/* Ray queries against a triangle mesh through a bounding-volume hierarchy (csrc/bvh.h, csrc/bvh.hip): what the shadows and the bounce of
 * drm_render_mesh are made of, offered on their own.
 *   The intersection rule.  A ray (o, d) is given in OBJECT space; d need not be unit length.  It is occluded iff some face g satisfies all of:
 *   g != exclude; its three vertex indices are in [0, V); and with e1 = p1 - p0, e2 = p2 - p0, pv = d x e2, det = e1.pv, tv = o - p0,
 *   qv = tv x e1, U = tv.pv, V = d.qv, T = e2.qv and s = sign(det):  det != 0 and det is finite;  s U >= 0;  s V >= 0;  s (U + V) <= |det|;
 *   s T > 0.  The rule is division-free (integer-valued inputs give exact decisions), edges and vertices are inclusive, a ray lying in a face's
 *   plane misses that face (det = 0), an origin on a face does not hit that face (T = 0), and the query is any-hit: the answer does not depend
 *   on the order faces are visited in.  fp32, no contraction.  A face whose fp32 cross product e1 x e2 is exactly (0, 0, 0) occludes nothing:
 *   in exact arithmetic its det is 0 for every ray, in fp32 it would be rounding noise, and the builder leaves it out by the same arithmetic.
 *   The BVH never changes an answer: with it the result equals testing every face with the same triangle routine, for every ray.  Its boxes
 *   are padded at build time (2^-16 of the largest |coordinate|) and per query (2^-16 of the largest |o| component), the slab test's far bound
 *   has 2^-20 of slack, a direction component that is exactly 0 compares the origin with the slab instead of dividing, and a NaN slab distance
 *   constrains nothing.
 *   drm_mesh_bvh_build: pure host code (no HIP call, usable without a GPU), host pointers, over object-space positions: one blob per mesh serves
 *   all B views of a call.  Deterministic (the same input gives the same bytes), O(F log F): median split of the face centroids along the
 *   longest axis, leaves of at most 4 faces.  Faces with an index outside [0, V), a non-finite vertex or a zero cross product are left out.
 *   The buffer must hold drm_mesh_bvh_bytes(F) = 32 + 36 F bytes (0 for F outside [1, 2^24)); the bytes past the blob's own length are zeroed.
 *   Blob layout (little-endian, 16-byte aligned):  header of 32 bytes = uint32 magic "BVH1" (0x31485642), F, node_count, order_count, 16 bytes of
 *   zeros;  node_count nodes of 32 bytes in depth-first order = float box_min[3], box_max[3], int32 skip, uint32 first << 3 | count;
 *   order_count int32 face indices.  count = 0 marks an inner node, whose first child is the next node; a leaf holds the faces
 *   order[first .. first + count).  skip is the node to go to on a box miss or after a leaf.  Traversal is stackless: on a box hit an inner node
 *   goes to i + 1, everything else to skip; it ends at node_count.  The blob's length is 32 + 32 node_count + 4 order_count.
 *   Every consumer reads the header back from the device (a 32-byte copy and a synchronise of `stream`: the one wait these calls make) and
 *   returns DRM_ERR_INVALID when the magic, F or the counts do not fit; nothing is launched then.
 *   drm_mesh_occluded: one thread per ray.  All pointers are device pointers: origins, dirs [N][3], exclude [N] int32 (a face index, or any
 *   value outside [0, F) for none) or NULL, out [N] int32 0 / 1.  bvh == NULL tests all F faces per ray with the same triangle routine (the
 *   diagnostic path that shows the BVH changes nothing).  The caller vouches for the blob's length as for every other array's.
 *   The closest hit.  For a ray (o, d) and an exclude, a face g is a CANDIDATE iff the intersection rule above accepts it: its conditions are
 *   unchanged, the clause about a zero fp32 cross product included.  A candidate has, in fp32, t = T / det, u = U / det,
 *   v = V / det, each the correctly rounded quotient (the library is built without any flag that relaxes fp32 division; denormals are kept).
 *   s T > 0 and a finite non-zero det make t one of +0 .. +inf, never NaN.  The hit is the candidate that is least under the lexicographic
 *   order (t, g), t compared as an fp32 value: a total order, so the order faces are visited in cannot matter.  Cross-multiplied products are
 *   not compared (rounded products are not transitive).  No candidate: face -1.  The hit point is o + t d, with barycentric weights
 *   (1 - u - v, u, v) on the face's vertices (p0, p1, p2).  The BVH never changes an answer: the same face and the same t, u, v bits as
 *   testing every face.  Its walk is the stackless one of drm_mesh_occluded without the early return; the best t so far also bounds the far
 *   end of the slab test, under the same 2^-20 of slack.  A ray is occluded iff it has a closest hit.
 *   drm_mesh_closest_hit: one launch, one thread per ray; the arguments of drm_mesh_occluded with two outputs: out_face [N] int32 (-1: no
 *   hit) and out_tuv [N][3] float (t, u, v; zeros where there is no hit).  bvh == NULL tests all F faces per ray (the diagnostic path).  The
 *   header check and the error codes are those of drm_mesh_occluded; nothing is launched on an error. */
size_t drm_mesh_bvh_bytes(int64_t F);
int drm_mesh_bvh_build(const float* vertex_positions, const int32_t* faces, int64_t V, int64_t F, void* bvh, size_t bytes);
int drm_mesh_occluded(const float* vertex_positions, const int32_t* faces, int64_t V, int64_t F, const void* bvh, const float* origins, const float* dirs,
                      const int32_t* exclude, int32_t* out, int64_t N, void* stream);
int drm_mesh_closest_hit(const float* vertex_positions, const int32_t* faces, int64_t V, int64_t F, const void* bvh, const float* origins,
                         const float* dirs, const int32_t* exclude, int32_t* out_face, float* out_tuv, int64_t N, void* stream);

/* Object images of a triangle mesh: the input side of the chain (csrc/mesh.hip for visibility, csrc/render.hip for shading).  Replaces
 * MitsubaOrthoRenderer.rendering (utils/mitsuba3_utils.py:433-564: an orthographic camera on a smooth-shaded mesh with image, shading-normal
 * and depth AOVs).  One mesh per call, lit and seen B ways under a drm_shading with principled rows z [B][6] (tables are DRM_ERR_INVALID
 * here: a mesh under measured tables is drm_render_mesh_tables, below).
 * Every visible point is shaded exactly as drm_render_refmap shades the sphere point with the same normal: direct light from the
 * environment map, and the background is black, not the environment.  Without shadows there is no self-shadowing: it is the model the
 * reflectance map itself assumes.  Zero-initialise drm_mesh_render, set struct_bytes = sizeof(drm_mesh_render), then the members in use.
 *   The mesh: vertex_positions, vertex_normals [V][3], faces [F][3] int32 (smooth shading, no back-face culling).  1 <= F < 2^24, V >= 1.
 *   View frame.  right, up, back are the columns of the row-major Rot = view[b] of the shading.  Mesh points and normals enter the view frame
 *   as Rot^T p and Rot^T n; the environment is looked up at Rot l.  NULL or an exact identity multiplies nothing.
 *   The film: H x W pixels, S x S = subpixel^2 samples per pixel, box filter.  Sample (i, sy, j, sx) is at
 *   x = (2 (j S + sx) + 1) / (W S) - 1, y = (H / W) (1 - (2 (i S + sy) + 1) / (H S)); the ray runs along -z, and of the faces covering a
 *   sample the one with the largest view-space z is seen.  The film spans x in [-1, 1] (a mesh normalised to radius 0.9 fits).
 *   H, W in [1, 4096], subpixel in [1, 4], 1 <= B <= 65535.
 *   Coverage.  All three edge functions, oriented by the sign of the face's screen area, are >= 0 (edges inclusive).  Ties: larger z, then
 *   the lower face index, so the result does not depend on the order faces are visited in.  Faces of zero screen area are skipped, and so is
 *   a face with a vertex index outside [0, V), whose index is never dereferenced.
 *   Shading normal.  The barycentric mix of the three vertex normals, in the view frame, normalised (a zero mix stays zero).  A sample with
 *   no hit, or with n.z <= 0, contributes zero radiance.
 *   The four outputs, per row b: image [3][H][W] the mean over the S^2 samples of the radiance; normal [3][H][W] the mean of the samples' unit
 *   shading normals, zero for a miss (|normal| > 0.5 is "more than half covered", the mask the reference derives); depth [1][H][W] the mean of
 *   1.1 - z_view over the hit samples, 0 where there are none; alpha [H][W] the hit fraction.  normal, depth and alpha may each be NULL.
 *   workspace: at least drm_render_mesh_workspace_bytes = 80 B F + 16 B (H S) (W S) bytes of device memory, 16-byte aligned: one record per
 *   (row, face) and one hit per film sample, rebuilt by every call.  Three launches (mesh_setup_kernel, mesh_visibility_kernel,
 *   mesh_shade_kernel), no atomics: bitwise reproducible, and a call of B rows equals its rows rendered one by one.
 *   shadows != 0: shadow rays, any-hit queries by the intersection rule above (the same workspace, the same setup and visibility launches).
 *   bvh is a device copy of the blob, 16-byte aligned, required, bvh_bytes its length (a length shorter than the header implies is
 *   DRM_ERR_INVALID).  shadows == 0: bvh and bvh_bytes are not read.
 *   For every hit sample the ray origin is the view-space hit point (x_sample, y_sample, z_hit) taken to object space with Rot (no view:
 *   nothing is multiplied), exclude is the hit face, and every quadrature direction l with a non-zero weight is traced along Rot l, the vector
 *   the environment lookup forms: the specular direction inside its (v.h > 0, n.l > 0, D > 0) branch, the diffuse direction always.  An
 *   occluded direction contributes nothing, an open one exactly what it contributes without shadows, so a shadowed image is <= the plain
 *   one in every pixel and channel under a non-negative map.  Bitwise reproducible; rows are independent.
 *   Light samples on a mesh (light_samples > 0 of the shading, under a map), with or without shadows.
 *   Estimator (the contract).  For a hit sample with shading normal n (n.z > 0), origin o (the view-space hit point taken to object space with
 *   Rot) and hit face g the integrand is L(w) V(w) f(w) cos: V(w) = 0 iff the ray (o, w) is occluded by the intersection rule above with
 *   exclude = g; without shadows V = 1 everywhere.  Both techniques of the shading's light sampling estimate this one integrand with the SAME
 *   weights as on the sphere (n_s = n_d = quad^2, n_d = 0 for a metal, n_L = light_samples):
 *     each lobe sample keeps its power-heuristic weight (n p)^2 / ((n p)^2 + (n_L p_L)^2) and contributes only if the ray along Rot l is open;
 *     it is traced where the shadowed render traces it, before any texel fetch;
 *     each light-table entry k keeps its term L_k [f_s cos n_L p_L / ((n_s p_s)^2 + (n_L p_L)^2) + f_d cos n_L p_L / ((n_d p_d)^2 + (n_L p_L)^2)]
 *     / subpixel^2 and contributes only if the ray along its table direction is open.  The table holds world (environment-frame)
 *     directions, which in the mesh convention are also the object-space ray directions (as Rot l is for a lobe sample); it enters the
 *     view frame as Rot^T w_k for the BSDF.  It is traced only after its cheap rejections (n.l_k > 0, p_L > 0).
 *   p_L knows nothing of occlusion; the weights of a direction still sum to one, so the estimator is consistent for the shadowed integral.
 *   With shadows the image is <= the one without in every pixel and channel under a non-negative map.  A map whose tot is 0 renders as
 *   without light samples.  The tables are built by the three light launches of the sphere, after the visibility launches.
 *   The lanes keep the per-lane order of the sphere's lit kernel over the pixel's hit samples and meet in its two butterflies: bitwise
 *   reproducible, and a call of B rows equals its rows rendered one by one.
 *   bounces: 0, or 1 for one bounce of interreflection on the closest-hit query above; 1 needs shadows != 0, no light samples under a map
 *   and bounce_quad in [1, 16]; anything else is DRM_ERR_INVALID.  The launches of the shadowed render with the shading kernel's bounced
 *   instantiation in place of the shadowed one.  bounces == 0: bounce_quad is not read.
 *   Estimator (the contract).  The shadowed render, except for a lobe direction w (object space, non-zero weight) whose ray from the hit
 *   sample (origin o, exclude = the hit face g) is occluded.  It no longer drops out: in place of the map's radiance it reads
 *   L_b = the radiance its closest hit reflects toward -w under direct light, traced.  The lobe's weight and everything else about the
 *   sample are unchanged, and an open direction contributes exactly what it contributes in the shadowed render, bit for bit.  With
 *   (g', t, u, v) the closest hit of (o, w) excluding g:
 *     y = o + t w;  n_y = the normalised barycentric mix (1 - u - v, u, v) of the vertex normals of g', in object space (a zero or NaN mix:
 *     L_b = 0);  w_o = -w / |w|;  n_y.w_o <= 0: L_b = 0.
 *     Frame about n = n_y (Duff et al. 2017, with the sign term, valid for every unit n): s = 1 where n.z >= 0, else -1, a = -1 / (s + n.z),
 *     b = n.x n.y a, t = (1 + s n.x^2 a, s b, -s n.x), bt = (b, s + n.y^2 a, -n.y).
 *     K = bounce_quad^2 directions w_k, k = k1 bounce_quad + k2, from the diffuse lobe's mapping of the midpoint grid
 *     (u1, u2) = ((k1 + 1/2) / bounce_quad, (k2 + 1/2) / bounce_quad): cos_k = sqrt(1 - u1),
 *     w_k = cos_k n + sqrt(u1) (cos(2 pi u2) t + sin(2 pi u2) bt).
 *     L_b = (pi / K) sum_k V_k L(w_k) E(n_y, w_o, w_k) / cos_k.
 *     E = the principled BSDF's value times cosine, drm_brdf_eval's expression for the row z[b] evaluated in fp32, with 1 - cos^2 taken as
 *     |n x .|^2 (0 unless n.w_o > 0 and n.w_k > 0).  V_k = 0 iff the ray (y, w_k) with exclude = g' is occluded (the any-hit rule; a
 *     direction with E = 0 is not traced).  L(w_k) = the map's bilinear radiance along w_k -- an object-space direction is the world
 *     direction, as for lobe rays -- or 1 under a NULL map.
 *   Weights and radiances are non-negative under a non-negative map: a bounced image is >= the shadowed one in every pixel and channel.
 *   Each lane runs the K directions of its own bounce serially, in k order: bitwise reproducible, and a call of B rows equals its rows alone.
 *   DRM_ERR_INVALID for an argument outside the limits, a bad quadrature, material, light_samples or bounce setting, a missing, misaligned or
 *   short light workspace, a NULL, short or damaged blob under shadows; DRM_ERR_WORKSPACE for a missing, misaligned or short mesh workspace:
 *   nothing is launched. */
typedef struct drm_mesh_render {
  uint32_t struct_bytes;
  const float* vertex_positions;
  const float* vertex_normals;
  const int32_t* faces;
  int64_t V, F;
  int32_t H, W, subpixel;
  float *image, *normal, *depth, *alpha;
  void* workspace;
  size_t workspace_bytes;
  int32_t shadows;
  const void* bvh;
  size_t bvh_bytes;
  int32_t bounces, bounce_quad;
} drm_mesh_render;
size_t drm_render_mesh_workspace_bytes(int64_t F, int B, int H, int W, int subpixel); /* 0 for arguments drm_render_mesh rejects */
int drm_render_mesh(const drm_shading* shading, const drm_mesh_render* mesh, void* stream);
/* The same mesh under measured BRDFs (csrc/mesh_table.hip, mesh_table_shade_kernel): MitsubaOrthoRenderer.rendering with a measured BSDF, the
 * shapes-under-MERL-materials case.  The two structs, the workspace (drm_render_mesh_workspace_bytes), the limits, the film, the coverage
 * rule, the shading normal, the four outputs and the setup and visibility launches are drm_render_mesh's; the material of the shading is
 * its tables ("Measured BRDFs" below), row b under table table_of[b] with proxy roughness table_alpha[table_of[b]].
 *   Estimator (the contract).  For a hit sample with view-frame unit shading normal n (n.z > 0) the radiance is the per-normal sum of
 *   drm_render_refmap under tables: both sample sets at the row's table and proxy roughness, each sample l adding
 *     L(Rot l) f_table(n, v, l) (n.l) / (quad^2 (p_s(l) + p_d(l))),
 *   so a mesh point is shaded exactly as the sphere point and the normal-map pixel with the same normal.  The pixel is the sum over the
 *   subpixel^2 samples divided by subpixel^2.
 *   shadows != 0 (bvh, bvh_bytes as in drm_render_mesh): every sample with a non-zero balance weight -- a GGX sample inside its
 *   (v.h > 0, n.l > 0, D > 0) branch, a cosine sample where n.l > 0 -- is first traced by the intersection rule above along Rot l from the
 *   view-space hit point (x_sample, y_sample, z_hit) taken to object space with Rot, the hit face excluded, before the table and the
 *   environment are read.  An occluded sample contributes nothing, an open one exactly the bits it contributes without shadows: a shadowed
 *   image is <= the plain one in every pixel and channel under a non-negative map and table.
 *   fp32 throughout, one wave per pixel, the per-lane order and butterfly of drm_render_mesh, no atomics: bitwise reproducible, and a call of
 *   B rows equals its rows rendered one by one.
 *   Not built under a table: light samples, bounces, anisotropic tables.
 *   DRM_ERR_INVALID, nothing launched and no output touched, drm_last_error naming the argument: a struct_bytes of either struct; z given,
 *   or no tables (the material); light_samples > 0 under a map; bounces != 0; an argument outside the limits or a bad quadrature; a NULL,
 *   short or damaged blob under shadows; whatever "Measured BRDFs" rejects of the tables (a table_of value outside [0, NT), an alpha
 *   outside [0.005, 1] or not finite, ...).  DRM_ERR_WORKSPACE for a missing, misaligned or short mesh workspace.  Everything but the
 *   blob's header and the table_of / alpha values is decided without reading device memory. */
int drm_render_mesh_tables(const drm_shading* shading, const drm_mesh_render* mesh, void* stream);
/* The BSDF value itself, Mitsuba's eval = f(v, l) (n.l) (replaces eval_bsdf / the evaluation behind visualize_bsdf,
 * utils/mitsuba3_utils.py:610-640): z [z_rows][6] with z_rows 1 (one BSDF for every element) or N; n, v (toward the viewer),
 * l (toward the light) [N][3] unit vectors; out [N][3].  0 unless n.v > 0 and n.l > 0. */
int drm_brdf_eval(const float* z, int z_rows, const float* n, const float* v, const float* l, float* out, int64_t N, void* stream);

/* Measured BRDFs (csrc/brdf_table.hip): a material given as a MERL table instead of a principled row (the tables of a drm_shading).
 * Layout "packed table": one table is [90][90][180][4] fp32 = (theta_h, theta_d, phi_d, (r, g, b, 0)), 23 328 000 bytes, 16-byte aligned, so
 *   a lookup corner is one 16-byte load; `tables` is [NT] such blocks back to back.  Node (i, j, k) stands for theta_h = (i / 90)^2 pi / 2,
 *   theta_d = j pi / 180, phi_d = k pi / 180.  An entry without a measurement (below the horizon) has r = g = b = -1.  The values are
 *   BRDF values (load_merl's, the colour scales applied), not BRDF times cosine.  1 <= NT <= 4096.
 * The lookup f_table(n, v, l), unit n, v (toward the viewer), l (toward the light); 0 unless n.v > 0 and n.l > 0:
 *   h = normalize(v + l); theta_h = atan2(|n x h|, n.h); theta_d = atan2(|l x h|, l.h);
 *   x_h = -normalize(n - (n.h) h), y_h = h x x_h, phi_d = atan2(v.y_h, v.x_h) taken mod pi (MERL's convention: in the half-vector frame the
 *   normal lies at azimuth pi; reciprocity gives the other half); phi_d = 0 where |n - (n.h) h| < 1e-6;
 *   coordinates (90 sqrt(theta_h / (pi / 2)), 90 theta_d / (pi / 2), 180 phi_d / pi).
 *   linear = 0 ("nearest", the MERL distribution reader's rule): floor each, clamp to [0, 89], [0, 89], [0, 179]; a negative entry reads 0.
 *   linear != 0: trilinear between floor and floor + 1, clamped at 89 in theta_h and theta_d, wrapping 179 -> 0 in phi_d; corners whose
 *   entry is negative are dropped and the remaining weights renormalised; 0 where all eight are dropped.
 * table_of: int32 device array naming the table of every row / element, or NULL: table 0 for all.  It is brought to the host and checked
 *   (one stream synchronisation) before anything is launched, as is alpha.
 * DRM_ERR_INVALID, with drm_last_error naming the argument and no output touched: a NULL where data is required, tables not 16-byte aligned,
 *   NT outside [1, 4096], a table_of value outside [0, NT), an alpha outside [0.005, 1] or not finite, a bad quad / subpixel / map size.
 *
 * drm_brdf_to_merl (replaces bsdf_to_merl, utils/mitsuba3_utils.py:602-638): one packed table per principled row z [rows][6],
 *   1 <= rows <= 4096, one thread per entry, in fp64 (drm_brdf_eval's expression): in the half-vector frame h = +z,
 *   n = (-sin theta_h, 0, cos theta_h), wo = (sin theta_d cos phi_d, sin theta_d sin phi_d, cos theta_d) (the viewer), wi = wo (-1, -1, 1)
 *   (the light); entry = eval(n, wo, wi) / (n.wi); -1 where n.wo < 0 or n.wi < 0; 0 where a cosine is exactly 0 (|cos| < 1e-12: the grid's
 *   exact zeros, theta_h + theta_d = pi / 2 at phi_d = 0, as fp64 rounds them). */
int drm_brdf_to_merl(const float* z, int rows, float* tables_out, void* stream);
/* drm_merl_eval (eval_bsdf / visualize_bsdf for a measured material, utils/mitsuba3_utils.py:641-690): out [N][3] = f_table(n, v, l) (n.l)
 *   -- Mitsuba's eval convention, as drm_brdf_eval -- for N triples n, v, l [N][3]; coordinates and interpolation in fp64. */
int drm_merl_eval(const float* tables, int NT, const int32_t* table_of, const float* n, const float* v, const float* l, float* out, int64_t N, int linear,
                  void* stream);
/* drm_brdf_error_sums (csrc/brdf_error.hip; serves drmnet_amd/reflectance.py: brdf_errors, fit_principled, estimate --gt_z / --gt_merl and
 *   merl --fit / --compare): C candidate rows z [C][6], 1 <= C <= 4096, scored against ONE target on
 *   the MERL grid in one pass.  The target is `table` (one packed table, 16-byte aligned) or `z_target` (one principled row [6]); exactly one
 *   of the two is non-NULL.  At a node, a = the candidate's value there = the entry drm_brdf_to_merl stores (the same device function), b =
 *   the target's entry (a principled target's formed the same way), ci = n.wi.  A node counts where drm_brdf_to_merl stores a BRDF value
 *   (n.wo > 0 and n.wi > 0 after the 1e-12 snap) and the target entry has no negative channel; every counting node weighs one (the MERL-sample
 *   convention, no solid-angle weight) and the three channels are pooled.  sums [C][DRM_BRDF_ERROR_SUMS] fp64, over the channel values of the
 *   counting nodes:
 *     [DRM_BRDF_ERROR_N]      their count n                       [DRM_BRDF_ERROR_N_LOG]   the count with a > 0 and b > 0
 *     [DRM_BRDF_ERROR_D]      sum of d = log10 a - log10 b        [DRM_BRDF_ERROR_DD]      sum of d^2         (both over the n_log values)
 *     [DRM_BRDF_ERROR_LOG1P]  sum of (log1p(a ci) - log1p(b ci))^2
 *     [DRM_BRDF_ERROR_L2]     sum of ((a - b) ci)^2
 *     [DRM_BRDF_ERROR_AA], [DRM_BRDF_ERROR_AB], [DRM_BRDF_ERROR_BB]   sums of (a ci)^2, (a ci)(b ci), (b ci)^2
 *   Element arithmetic and sums are fp64, added in a fixed order without atomics: two calls are bitwise equal, and a row's sums do not depend
 *   on C or on its place among the candidates.  Two launches, no host synchronisation.  workspace: DRM_BRDF_ERROR_WORKSPACE_BYTES(C) of device
 *   memory, 8-byte aligned, contents irrelevant.  DRM_ERR_INVALID with drm_last_error naming the entry: both or neither target, C outside
 *   [1, 4096], a misaligned table, a NULL z / workspace / sums, a workspace too small. */
#define DRM_BRDF_ERROR_SUMS 9
#define DRM_BRDF_ERROR_N 0
#define DRM_BRDF_ERROR_N_LOG 1
#define DRM_BRDF_ERROR_D 2
#define DRM_BRDF_ERROR_DD 3
#define DRM_BRDF_ERROR_LOG1P 4
#define DRM_BRDF_ERROR_L2 5
#define DRM_BRDF_ERROR_AA 6
#define DRM_BRDF_ERROR_AB 7
#define DRM_BRDF_ERROR_BB 8
#define DRM_BRDF_ERROR_PARTS 128
#define DRM_BRDF_ERROR_WORKSPACE_BYTES(C) ((size_t)(C) * DRM_BRDF_ERROR_PARTS * DRM_BRDF_ERROR_SUMS * sizeof(double))
int drm_brdf_error_sums(const float* z, int C, const float* table, const float* z_target, double* workspace, size_t workspace_bytes, double* sums,
                        void* stream);

/* drm_image_error_sums (csrc/image_error.hip; serves drmnet_amd/relight.py: image_error_sums, image_errors_batch, and drmnet_amd/samples.py,
 *   which ranks the draws of estimate --num_samples): P pairs of images scored on a mask in one call, the image-space twin of
 *   drm_brdf_error_sums.  Zero-initialise drm_image_error, set struct_bytes = sizeof(drm_image_error), then every member.  All pointers
 *   are device pointers.
 *   a, b: two stacks of fp32 images of HW pixels and three channels; element (i, pixel q, channel c) of a stack is
 *     data[i batch_stride + q pixel_stride + c channel_stride] (strides in elements: channel-first [B][3][HW] is (3 HW, 1, HW), channel-last
 *     [B][HW][3] is (3 HW, 3, 1); a batch stride larger than an image, or 0, goes in as it is).
 *   mask: uint8 [mask_count][HW], non-zero = counted.  pairs: int32 [P][3] = (ia, ib, im), 1 <= P <= 4096: image ia of a against image ib of
 *     b on mask im.  The triples are device data and are not brought to the host: a triple outside [0, a_count) x [0, b_count) x [0, mask_count)
 *     reads nothing and gives ten NaNs (callers check their triples before the upload, as drmnet_amd.relight does).
 *   sums: double [P][DRM_IMAGE_ERROR_SUMS], over the masked pixels and their three channels, element arithmetic in fp64:
 *     [DRM_IMAGE_ERROR_N]      the masked pixels (pixels, not entries)
 *     [DRM_IMAGE_ERROR_AA], [DRM_IMAGE_ERROR_BB], [DRM_IMAGE_ERROR_AB]   sums of a^2, b^2, a b
 *     [DRM_IMAGE_ERROR_L2]     sum of (a - b)^2
 *     [DRM_IMAGE_ERROR_N_LOG]  the entries with a > 0 and b > 0
 *     [DRM_IMAGE_ERROR_D], [DRM_IMAGE_ERROR_DD]   sums of d = log10 a - log10 b and of d^2, over those entries
 *     [DRM_IMAGE_ERROR_L2_SCALED]  sum of (s a - b)^2, s = sum AB / sum AA (0 unless sum AA > 0)
 *     [DRM_IMAGE_ERROR_DD_CENTRED] sum of (d - sum D / n_log)^2 (the mean is 0 where n_log is 0)
 *   The last two are a second pass over the pixels, which forms s and the mean on the device from the first pass's parts added in the order
 *   the results are; the one-pass identities BB - AB^2 / AA and DD - D^2 / n_log cancel and are not used.  Three launches, no host
 *   synchronisation.  Sums are added in a fixed order without atomics that depends on the pixel's place alone: a pair gives the same bits
 *   alone, at any place in any list of pairs, and in two calls.  Non-finite values propagate as they do in fp64 arithmetic.
 *   workspace: DRM_IMAGE_ERROR_WORKSPACE_BYTES(P) of device memory, 8-byte aligned, contents irrelevant.
 *   DRM_ERR_INVALID, nothing launched, drm_last_error naming what is wrong: struct_bytes; a NULL a, b, mask, pairs, workspace or sums; P
 *   outside [1, 4096]; HW < 1; a count < 1; a workspace smaller than the macro; workspace or sums not 8-byte aligned. */
#define DRM_IMAGE_ERROR_SUMS 10
#define DRM_IMAGE_ERROR_N 0
#define DRM_IMAGE_ERROR_AA 1
#define DRM_IMAGE_ERROR_BB 2
#define DRM_IMAGE_ERROR_AB 3
#define DRM_IMAGE_ERROR_L2 4
#define DRM_IMAGE_ERROR_N_LOG 5
#define DRM_IMAGE_ERROR_D 6
#define DRM_IMAGE_ERROR_DD 7
#define DRM_IMAGE_ERROR_L2_SCALED 8
#define DRM_IMAGE_ERROR_DD_CENTRED 9
#define DRM_IMAGE_ERROR_PARTS 16
#define DRM_IMAGE_ERROR_WORKSPACE_BYTES(P) ((size_t)(P) * DRM_IMAGE_ERROR_PARTS * DRM_IMAGE_ERROR_SUMS * sizeof(double))
typedef struct drm_image_error {
  uint32_t struct_bytes;
  const float* a;
  int32_t a_count;
  int64_t a_batch_stride, a_pixel_stride, a_channel_stride;
  const float* b;
  int32_t b_count;
  int64_t b_batch_stride, b_pixel_stride, b_channel_stride;
  const uint8_t* mask;
  int32_t mask_count;
  int64_t HW;
  const int32_t* pairs;
  int32_t P;
  void* workspace;
  size_t workspace_bytes;
  double* sums;
} drm_image_error;
int drm_image_error_sums(const drm_image_error* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The validation losses (csrc/losses.hip).
 * ------------------------------------------------------------------------------------------- */
/* DRMNet.p_losses after the two networks, in eval mode (models/drmnet.py:432-450 with get_loss :398-411 and get_brdf_out :390-396): two
 * launches, no host synchronisation, nothing materialised.
 *   model_out, Lr_k (the noised input of the networks), Lr_km1 [B][per_row] fp32 (per_row = 3 H W); K, reversed_k int32[B];
 *   z_out, z_k, z_K [B][P] fp32; z0 fp32[P]; loss_type DRM_LOSS_L1 (|d|) or DRM_LOSS_L2 (d^2).
 *   out fp32[3] on the device = (loss_refmap, loss_refcode, loss):
 *     loss_refmap  = mean of f(model_out - (Lr_km1 - Lr_k)) over the rows with K != 0.  Rows are selected, not weighted: a NaN in a row with
 *                    K == 0 (the dataset marks its zkm1 / Lrkm1 so) does not reach the result; no selected row gives NaN (torch's empty mean)
 *     zk_out       = clamp(z0 + gamma^reversed_k (z_out - z0), 0, 1), the power as exp(reversed_k ln gamma) in fp64 cast to fp32
 *     loss_refcode = (mean f(zk_out - z_k) + mean f(clamp(z_out, 0, 1) - z_K)) / 2
 *     loss         = l_refmap_weight loss_refmap + l_refcode_weight loss_refcode
 *   Element arithmetic and sums are fp64, combined in a fixed order without atomics (two calls are bitwise equal); the three results are
 *   rounded to fp32 once.  workspace: DRM_LOSS_WORKSPACE_BYTES of device memory, contents irrelevant. */
#define DRM_LOSS_L1 0
#define DRM_LOSS_L2 1
#define DRM_LOSS_WORKSPACE_BYTES 2048
int drm_validation_losses(const float* model_out, const float* Lr_k, const float* Lr_km1, const int32_t* K, const float* z_out, const float* z_k,
                          const float* z_K, const int32_t* reversed_k, const float* z0, double gamma, int loss_type, double l_refmap_weight,
                          double l_refcode_weight, int B, int64_t per_row, int P, void* workspace, size_t workspace_bytes, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ObsNetDiffusion's validation pass around its network forward (csrc/obs_forward.hip).
 * ------------------------------------------------------------------------------------------- */
/* The forward process of a batch in one elementwise launch: the conditioning of ObsNetDiffusion.get_input for cond_key "masked_LrK"
 * (models/obsnet.py:375-398: cond = mask * LrK; cond = noisy_observe * randn_like(cond) + cond; cond += (1 - mask) * randn_like(cond)) and
 * q_sample of p_losses (ldm/models/diffusion/ddpm.py:288-294).
 *   x [B][C][H][W]: the transformed LrK; mask [B][1][mask_H][mask_W] fp32 with mask_H == H and mask_W == W (any other size is DRM_ERR_INVALID:
 *   resize it first); t int32[B] (device); sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod fp32[T] (device).
 *     cond    = mask x + noisy_observe e1 + (1 - mask) e2     the e1 term only when noisy_observe > 0, the e2 term only for DRM_PAD_NOISE;
 *                                                             a dropped term is not computed (no draw, no add)
 *     x_noisy = sqrt_alphas_cumprod[t_b] x + sqrt_one_minus_alphas_cumprod[t_b] e3
 *     noise   = e3                                            the loss target
 *   e_observe (e1), e_padding (e2), e_q (e3): [B][C][H][W] device tensors (parity runs), each or NULL.  A NULL one is drawn from the library's
 *   Philox stream of `seed`: with n = B C H W, e1 is elements [0, n), e2 [n, 2 n), e3 [2 n, 3 n) (what drm_randn(seed, offset) returns), the
 *   reference's draw order (observe, padding, q-noise).
 *   The reference's in-place "cond +=" also lands in c (IdentityFirstStage.encode returns its argument): cond here is what the network is
 *   conditioned on, after padding.  A t_b outside [0, T) is not looked up: its row of x_noisy is NaN.  fp32 arithmetic, no contraction.
 *   Either half may be left out: cond == NULL skips the conditioning (mask and its draws are not read), x_noisy == noise == NULL skips
 *   q_sample (t and the tables are not read).  The offsets of the three Philox ranges do not depend on which halves run, so two calls with one
 *   seed, one per half, give what one call gives. */
#define DRM_PAD_ZEROS 0
#define DRM_PAD_NOISE 1
int drm_obs_forward_process(const float* x, const float* mask, const int32_t* t, const float* sqrt_alphas_cumprod,
                            const float* sqrt_one_minus_alphas_cumprod, int T, float noisy_observe, int padding_mode, const float* e_observe,
                            const float* e_padding, const float* e_q, uint64_t seed, float* cond, float* x_noisy, float* noise, int B, int C, int H,
                            int W, int mask_H, int mask_W, void* stream);
/* ObsNetDiffusion.p_losses after the network, in eval mode (models/obsnet.py:469-498 with get_loss, ddpm.py:296-308): two launches, no host
 * synchronisation.
 *   model_out, target [B][per_row] fp32 (per_row = C HW); invmask [B][per_row / C] fp32 (1 - mask, broadcast over the channels) for masked_loss,
 *   or NULL; t int32[B]; logvar, lvlb_weights fp32[T]; loss_type DRM_LOSS_L1 (|d|) or DRM_LOSS_L2 (d^2), d = model_out - target.
 *     L_b         = mean of f(d) over row b                                    (invmask == NULL)
 *                 = sum f(d) invmask / (sum invmask * C)                       (masked; the second sum runs over one channel plane)
 *     loss_simple = mean_b L_b
 *     loss_vlb    = mean_b lvlb_weights[t_b] L_b
 *     loss        = l_simple_weight mean_b (L_b / exp(logvar[t_b]) + logvar[t_b]) + original_elbo_weight loss_vlb
 *   out fp32[3] on the device = (loss_simple, loss_vlb, loss); loss_simple_rows fp32[B] = L_b, or NULL.
 *   A masked row whose mask is all ones (invmask all zero) gives L_b = 0 / 0 = NaN, and with it NaN in all three scalars, as the reference does.
 *   A t_b outside [0, T) is not looked up: loss_vlb and loss are NaN.
 *   Element arithmetic and sums are fp64, every thread, tree and row in a fixed order without atomics (two calls are bitwise equal, whatever the
 *   alignment of the pointers); the results are rounded to fp32 once.  workspace: DRM_DIFFUSION_LOSS_WORKSPACE_BYTES(B) of device memory,
 *   contents irrelevant. */
#define DRM_DIFFUSION_LOSS_MAX_PARTS 32
#define DRM_DIFFUSION_LOSS_WORKSPACE_BYTES(B) ((size_t)(B) * DRM_DIFFUSION_LOSS_MAX_PARTS * 2 * sizeof(double))
int drm_diffusion_losses(const float* model_out, const float* target, const float* invmask, const int32_t* t, const float* logvar,
                         const float* lvlb_weights, int T, int loss_type, double l_simple_weight, double original_elbo_weight, int B,
                         int64_t per_row, int C, void* workspace, size_t workspace_bytes, float* out, float* loss_simple_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DRMNET_HIP_H */
