// Shared declarations for the DRMNet MI355X (gfx950) hot-path library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include <string>
#include "../../include/drmnet_hip.h"
#include "conv_forms.h"
#include "gn_fold.h"

namespace drm {

// Thread-local last error text, surfaced through drm_last_error() (C ABI never throws).
void set_error(const std::string& msg);
const char* last_error();

#define DRM_OK 0
#define DRM_ERR_INVALID 1
#define DRM_ERR_HIP 2
#define DRM_ERR_WORKSPACE 3
#define DRM_ERR_STATE 4

#define DRM_HIP_CHECK(expr)                                                                              \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess) {                                                                              \
      ::drm::set_error(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " at " + __FILE__ + ":" + \
                       std::to_string(__LINE__));                                                        \
      return DRM_ERR_HIP;                                                                                \
    }                                                                                                    \
  } while (0)

#define DRM_REQUIRE(cond, msg)                                    \
  do {                                                            \
    if (!(cond)) {                                                \
      ::drm::set_error(std::string("invalid argument: ") + (msg)); \
      return DRM_ERR_INVALID;                                     \
    }                                                             \
  } while (0)

// a struct the caller filled (include/drmnet_hip.h: struct_bytes) has the size this library was built with
#define DRM_REQUIRE_SIZE(p, T)                                                                                        \
  DRM_REQUIRE((p)->struct_bytes == sizeof(T), std::string(#T ": struct_bytes is ") + std::to_string((p)->struct_bytes) + \
                                                  ", sizeof(" #T ") is " + std::to_string(sizeof(T)))

#define DRM_TRY(expr)          \
  do {                         \
    int _s = (expr);           \
    if (_s != DRM_OK) return _s; \
  } while (0)

// The kernels are written for one device shape: gfx950 / MI355X = 256 CUs in 8 XCDs (workgroups b and b + 8 share an XCD and
// its L2), 160 KiB of LDS per CU.  device_info() reads the CURRENT device's properties once per device ordinal and returns
// null -- with the error text set -- when they do not match, so a launch on anything else fails loudly instead of running a
// mis-sized persistent grid.  Thread-safe; one process may drive several GPUs (one stream / handle set per device).
struct DeviceInfo {
  int ordinal = 0;
  int cus = 0;          // 256
  int xcds = 0;         // 8
  size_t lds_per_cu = 0;  // 163840
};
const DeviceInfo* device_info();
// The opt-in LDS size (above 48 KiB) is a per-device function attribute: one bit per device ordinal and KERNEL instantiation (a template
// argument, so kernels that share a function type keep separate state), set idempotently -- a racing second thread at worst repeats the
// call -- so the entry points stay re-entrant across streams, threads and devices.
template <auto KERNEL>
int opt_in_lds(size_t bytes, const DeviceInfo* di) {
  static std::atomic<uint64_t> attr_mask{0};
  if (bytes > 48 * 1024 && !(attr_mask.load(std::memory_order_acquire) >> di->ordinal & 1)) {
    DRM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    attr_mask.fetch_or(uint64_t(1) << di->ordinal, std::memory_order_release);
  }
  return DRM_OK;
}
template <auto KERNEL>  // (a kernel as an argument of a generic launch lambda: opt_in_lds<KERNEL> needs it as a constant)
struct KernelTag { static constexpr auto kernel = KERNEL; };
// Logical tile ids are dealt to the 8 XCDs in contiguous ranges (workgroups b and b + 8 share an XCD and its L2): the range of XCD `xcd` of `total`
struct XcdRange { int start, count; };
__host__ __device__ __forceinline__ XcdRange xcd_range(int total, int xcd) {
  const int q8 = total >> 3, r8 = total & 7;
  return {xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8, q8 + (xcd < r8 ? 1 : 0)};
}

// ---------------------------------------------------------------------------------------------
// Activation layout: NHWC fp32 ("pixels x channels", channels contiguous) everywhere inside the
// network; NCHW only at the boundary (reference tensors are NCHW).
// ---------------------------------------------------------------------------------------------

// Fused conv / GEMM descriptor (see conv.hip).
struct ConvArgs {
  const float* src0 = nullptr;  // NHWC, C0 channels; if up0, stored at (H/2, W/2) and read nearest-upsampled
  const float* src1 = nullptr;  // NHWC, C1 channels at (H, W) (skip tensor of the U-Net concat), may be null
  int C0 = 0, C1 = 0, up0 = 0;
  int N = 0, H = 0, W = 0;       // conv input == output spatial size (stride 1, pad = taps/2)
  const float* gn_scale = nullptr;  // [N][C0+C1] per-(sample,channel) GroupNorm scale (rstd*gamma) or null
  const float* gn_shift = nullptr;  // [N][C0+C1] (beta - mean*rstd*gamma)
  int silu = 0;                     // apply x*sigmoid(x) after the affine
  const float* w = nullptr;         // packed [taps][Cin/4][Cout][4]
  const float* bias = nullptr;      // [Cout]
  int taps = 9;                     // 9 (3x3, pad 1), 1 (1x1) or 4: the 3x3 conv over a nearest-x2 input as four 2x2 convs on the stored map --
                                    // Cout = 4 x the real count, parity-major (channel p * Cout/4 + co, p = 2 (y & 1) + (x & 1) of the output
                                    // pixel); out is the [N][2H][2W][Cout/4] tensor (pixel shuffle in the epilogue); no bias / emb / res / stats
  int Cout = 0;                     // padded Cout (multiple of 32)
  const float* emb = nullptr;       // optional per-(sample, cout) add: emb[n*emb_stride + co]
  int emb_stride = 0;
  const float* res = nullptr;       // optional residual NHWC [N,H,W,Cout]; may alias out
  float* out = nullptr;             // NHWC [N,H,W,Cout], or NCHW [N,cout_valid,H,W] if out_nchw
  int out_nchw = 0, cout_valid = 0;
  int cin_real = 0;                 // un-padded Cin for FLOP accounting (0 = C0 + C1)
  int ksplit = 1;                      // split-K factor (plan_conv); > 1: split k writes its raw partial sums to out + k * split_stride
  size_t split_stride = 0;             // floats between the split-K slabs (0 unless ksplit > 1)
  float* split_ws = nullptr;           // fused split-K: slab workspace ([ksplit] slabs of split_stride floats); the workgroup that arrives LAST at an output tile
  unsigned* tile_ticket = nullptr;     // (arrival counter per output tile, zero before the launch) sums the slabs in slab order and runs the full epilogue into `out`
  int terms = 3;                       // split kernels: 3 = fp16 hi/lo (fp32 accuracy), 2 = fp16 hi*hi + fp8 cross terms, 1 = plain fp16 operands, 4 = plain bf16 operands
  int mx_site = 0;                     // PREC_F16MX: this launch is one of the 3x3 convs whose weights carry the f16mx image
#ifdef DRM_S2_STAMP
  unsigned* stamp_out = nullptr;       // diagnostic build: [8 waves][120][2] (id, s_memtime low word) of one workgroup
  int stamp_block = 0, stamp_tile0 = 0;
#endif
  double2* stat_out = nullptr;         // optional [N][Cout] (sum, sum of squares) of the OUTPUT, accumulated atomically (must be zeroed)
  float* pool_out = nullptr;           // optional: the 2x2 average pool of the output, NHWC [N][H/2][W/2][Cout] (Downsample, openaimodel.py:154-160), written by the
  double2* pool_stat = nullptr;        // same epilogue, with its [N][Cout] (sum, sum of squares) (zeroed) -- plan_conv says which launches can
  const float* w_inv_scale = nullptr;  // split-precision path: device scalar 2^-k undoing the weight pre-scaling
  int ld0 = 0;                         // channel stride of src0's pixels when it is a channel slice of a wider tensor (0 = C0)
  int gn_ld = 0;                       // row stride of gn_scale / gn_shift when they are a channel slice of a wider block's tables (0 = C0 + C1)
  long long w_img_stride_f4 = 0;       // split 1x1 path: every image has its own packed weight set this many float4 apart (attention GEMMs)
  const float* w_inv_img = nullptr;    // ... and its own 2^-k weight factor [N] (replaces w_inv_scale)
  int prof_kind = -1;                  // launch-profiler family override (-1 = by tap count, PROF_KINDS = no scope of its own)
  const float* in_inv = nullptr;       // split-precision path: [N] per-image 2^-k undoing the input staging factor (launch_act_pow2_scale)
  GnFold gnf;                          // sparse launches (engine.hip gn_params): gn_scale / gn_shift (and a guard table set) are finalised by this launch's own prologue
};
// The launch profiler's work of a conv: 2 FLOP per MAC on un-padded channels; bytes = input read once + output written once (+ the residual) +
// weights once.  (the parity form, taps == 4, reports the algorithmic FLOPs of the conv it replaces: 9 taps at 4 x the pixels on a quarter
// of its GEMM columns)
struct ConvWork { double flops, bytes; };
inline ConvWork conv_work(const ConvArgs& a, int taps) {
  const double cin = a.cin_real > 0 ? a.cin_real : (a.C0 + a.C1), cout = a.out_nchw ? a.cout_valid : a.Cout;
  const double px = (double)a.N * a.H * a.W;
  const double px_in = (double)a.N * ((a.H >> a.up0) * (a.W >> a.up0)) * a.C0 + px * a.C1;
  return {2.0 * px * (taps == 4 ? 9 : taps) * cin * cout, 4.0 * (px_in + px * cout * (a.res ? 2 : 1) + (double)taps * cin * cout)};
}
// One decision per conv launch: plan_conv (conv_plan.hip) picks the kernel and its instantiation, the split-K form, and whether the 2x2 pool and
// the GroupNorm finalise fold into the launch; launch_conv carries it out.  The engine plans every conv once, in sizing and real passes alike.
enum ConvKernel : unsigned char { CONV_NONE, CONV_IGEMM, CONV_PIPELINE };  // NONE: per-image weights outside the pipeline's rule
// split-K finish: by the workgroup that arrives last at an output tile (SK instantiation, ConvArgs::tile_ticket), or by a second launch
// (splitk_reduce_small_kernel) that sums the slabs
enum SplitFinish : unsigned char { SPLIT_NONE, SPLIT_IN_LAUNCH, SPLIT_REDUCE };
struct ConvPlan {
  ConvKernel kernel = CONV_NONE;  // conv_igemm_kernel (conv.hip) or conv_split2_kernel
  int terms = 0;                  // ConvArgs::terms of a pipeline launch
  ConvTile tile = TILE_128x32;
  int th = 0, tw = 0;             // pixel tile of one image (the kernel's TH x TW)
  bool ragged = false;            // pipeline: edge tiles masked (RAG instantiations); conv_igemm_kernel masks them always
  int kc = 32;                    // conv_igemm_kernel: channels per K step (8: input channels that are not whole 32-chunks)
  int ksplit = 1;
  SplitFinish finish = SPLIT_NONE;
  size_t tickets = 0;             // SPLIT_IN_LAUNCH: the zeroed arrival counters to allocate (ConvArgs::tile_ticket)
  bool pool = false;              // the epilogue writes the 2x2 average pool (ConvArgs::pool_out / pool_stat)
  bool gn_fold = false;           // the prologue finalises the input's GroupNorm tables (ConvArgs::gnf)
  bool split() const { return kernel == CONV_PIPELINE && terms != 0; }  // split-precision operands: an un-normalised input needs its range guard
};
// `a`: the shape fields (N, H, W, C0, C1, taps, Cout, mx_site, out_nchw, w_img_stride_f4).  want_pool: a Downsample follows this conv;
// gn_foldable: the input's GroupNorm tables may be finalised by this launch
ConvPlan plan_conv(const ConvArgs& a, int precision, bool want_pool = false, bool gn_foldable = false);
// the weight image a conv with `cin` (padded) input channels reads in `precision`: the pre-split one (launch_pack_conv_weight_split) or plain fp32
bool conv_split_weights(int precision, int cin);
// the one launch entry of every conv (conv.hip): validates `a` against the plan; a split-K launch takes its slabs at a.split_ws
int launch_conv(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
template <int TAPS, int TERMS> int dispatch_s2(const ConvArgs& a, const ConvPlan& p, hipStream_t s);  // the pipeline launches of one DRM_S2_UNITS unit (conv_split2.hip)
int no_form(const ConvPlan& p);  // the error of a plan without an instantiation
size_t packed_conv_weight_split_floats(int taps, int CoutP, int CinP);
// mx: the f16mx image (fp16 hi planes + e4m3 planes of hi and lo) for the 3x3 convs that run with ConvArgs::terms == 2
int launch_pack_conv_weight_split(const float* w, float* packed, float* scales, unsigned* scratch, int Cout, int Cin, int taps, int CoutP,
                                  int CinP, hipStream_t s, bool mx = false, bool bf16 = false);
// PREC_F16MX: PREC_F16X3 with the GroupNorm-fed 3x3 convs on fp16 hi*hi + one block-scaled fp8 MFMA for both cross terms (~4e-5 per network)
// PREC_BF16: bf16 operands, fp32 accumulate (v_mfma_f32_32x32x16_bf16): BASELINE configs[2] as written; reduced precision like PREC_F16
enum Precision { PREC_FP32 = 0, PREC_F16X3 = 1, PREC_F16 = 2, PREC_F16MX = 3, PREC_BF16 = 4 };
inline bool precision_valid(int p) { return p >= PREC_FP32 && p <= PREC_BF16; }
// ConvArgs::terms of the pipeline kernel in a mode (PREC_F16MX: 3, and 2 on its mx_site launches)
inline int precision_terms(int p) { return p == PREC_F16 ? 1 : (p == PREC_BF16 ? 4 : (p == PREC_FP32 ? 0 : 3)); }
// repack PyTorch conv weight [Cout][Cin][kh][kw] -> [taps][CinP/4][CoutP][4] (zero padded)
int launch_pack_conv_weight(const float* w, float* packed, int Cout, int Cin, int taps, int CoutP, int CinP, hipStream_t s);
// one conv weight in the image its consumer reads in `precision` (engine.hip): the pre-split one where conv_split_weights says so -- f16mx for an
// mx_site in PREC_F16MX, bf16 in PREC_BF16 -- with its pre-scaling (2^k, 2^-k) at `scale`, else plain fp32; `scratch` = 1 uint on the device
int pack_conv_image(int precision, const float* w, float* packed, float* scale, unsigned* scratch, int Cout, int Cin, int taps, int CoutP, int CinP,
                    bool mx_site, hipStream_t s);
// attention parameter fold (conv_split.hip): raw qkv [3C][C] / [3C] and proj_out [C][C] / [C] -> w_out [3C][C], b_out [3C] whose v rows hold
// Wp Wv and Wp bv + bp (fp64 products, rounded once); what every attention block's qkv conv is packed from
// 3x3 conv over cat(nearest_x2(x0), x1) split by linearity (engine.hip plan_upconv_split): w [Cout][C0 + C1][3][3] -> wa [4 * Cout][C0][2][2], the
// parity-major 2x2 kernels on the stored x0 (sums of the 3x3 taps that fall on one stored pixel, fp64, rounded once), and wb [Cout][C1][3][3], the
// x1 slice; both are ordinary conv weights for the packers (taps = 4 / 9)
int launch_fold_upconv_weight(const float* w, float* wa, float* wb, int Cout, int C0, int C1, hipStream_t s);
int launch_fold_attn_params(const float* qkv_w, const float* qkv_b, const float* proj_w, const float* proj_b, float* w_out, float* b_out, int C,
                            hipStream_t s);
size_t packed_conv_weight_floats(int taps, int CoutP, int CinP);

// GroupNorm statistics (gn.hip)
// per-(n,c) first/second moments of an NHWC tensor: mom[n][c] = (mean, mean of squares)
int launch_chan_moments(const float* x, int N, int HW, int C, double* partial /*[N][splits][C][2]*/, double2* mom /*[N][C]*/, hipStream_t s);
int chan_moments_splits(int HW, int C);
// combine moments of up to two concatenated sources into per-(n,c) scale/shift (32 groups, eps 1e-5)
// inv0 / inv1: factor turning a table into per-pixel means (1 for tables of means, 1/(H*W) for tables of raw sums)
// per-image power-of-two staging factor for un-normalised inputs of the split-precision convs (gn.hip)
int launch_act_pow2_scale(const double2* mom0, int C0, int lo0, int hi0, double cnt0, const double2* mom1, int C1, double cnt1,
                          const unsigned* absmax_bits, int Ctab, int N, float* scale, float* shift, float* inv, hipStream_t s, int absmax_parts = 1);
// guard_*: optional fused range-guard tables of the same tensor (act_pow2_scale_kernel's product), cnt0 / cnt1 as there
int launch_gn_finalize(const double2* mom0, int C0, double inv0, const double2* mom1, int C1, double inv1, const float* gamma,
                       const float* beta, int N, float* scale, float* shift, hipStream_t s, double cnt0 = 0.0, double cnt1 = 0.0,
                       float* guard_scale = nullptr, float* guard_shift = nullptr, float* guard_inv = nullptr);

size_t refmap_workspace_bytes(long long n, int res, float thr);
int launch_refmap_mask_make(const float* colors, const float* normals, long long n, int C, int res, float thr, int min_points, float* refmap,
                            unsigned char* refmask, void* ws, size_t ws_bytes, hipStream_t s);
int launch_erode_mask(const unsigned char* mask, int H, int W, int k, unsigned char* out, hipStream_t s);
// the inverse of the gather (see drm_image_from_refmap): refmap [Br][3][R][R] read at the normals of normals [Bn][H][W][3]
int launch_image_from_refmap(const float* refmap, const unsigned char* refmask, int Br, int R, const float* normals, const unsigned char* mask, int Bn,
                             float* image, float* alpha, int B, int H, int W, hipStream_t s);
// attention (attn.hip): qkv [N][T][3C] (v thirds = proj_out folded into v: launch_fold_attn_params), x [N][T][C] the block's input
// -> out = x + softmax(q k^T) v [N][T][C] and out_stat [N][C] += per-channel (sum, sum of squares) of out (zeroed by the caller);
// scores workspace [group][T][T].
// One decision per attention core, like ConvPlan per conv: plan_attention (pure host code) picks the form and all that follows from it,
// launch_attention_core carries it out.
enum AttnForm : unsigned char {
  ATTN_SMALL,  // short-sequence form (qk_small / softmax / P v), and every exact-fp32 core
  ATTN_CONV,   // both GEMMs on the fused 1x1 conv pipeline (per-image weights = k, v^T): where plan_conv takes them and N * T > 1024
  ATTN_FLASH   // single-kernel form (attn_flash.hip): the long-sequence level (T >= 1024, C = 384) in the split modes, no score matrix in HBM
};
struct AttnPlan {
  AttnForm form = ATTN_SMALL;
  int N = 0, H = 0, W = 0, C = 0;
  int terms = 0;  // precision_terms: 0 = fp32 MFMA, 3 = fp16 hi/lo split, 1 = plain fp16 operands, 4 = plain bf16 operands
  // ATTN_SMALL: S on the split kernel (whole 32-chunks of C), P v too (... and of T), per-image range guard of q, k, v (attn_scales_kernel)
  bool split_qk = false, split_pv = false, guard = false;
  int group = 1;             // images per pass: the [group, T, T] scores of one pass live in `scores` (independent of the batch beyond one group)
  size_t scores_floats = 0;  // 0: ATTN_FLASH
  size_t ws_floats = 0;      // AttnTables (0: the unguarded ATTN_SMALL takes no workspace)
  bool out_stats = true;     // the last kernel accumulates out_stat (not ATTN_FLASH: one wave per SIMD on the whole register file, no room for it)
  ConvPlan qk[2], pv[2];     // ATTN_CONV: the two GEMMs of a pass of `group` images [0] and of the short last pass [1] (N % group images)
};
AttnPlan plan_attention(int N, int H, int W, int C, int precision);
// the workspace of a core (between attn.hip and attn_flash.hip only): 0, 2 or 3 packed operand images ([N] x T * C floats: fp16 hi + lo planes) ahead of the per-image factor tables
struct AttnTables {
  float *wq = nullptr, *wk = nullptr, *wv = nullptr;                 // ATTN_FLASH: q, k, v^T; ATTN_CONV: k, v^T
  float *q_tab = nullptr, *p_tab = nullptr, *zero_tab = nullptr;     // [N][C], [N][T], [N][max(C, T)]
  float *qk_inv = nullptr, *k_scale = nullptr, *k_inv = nullptr, *pv_inv = nullptr, *v_scale = nullptr, *v_inv = nullptr;  // [N] each
  float* q_scale = nullptr;                                          // [N], not ATTN_CONV
};
// scores: plan.scores_floats, ws: plan.ws_floats floats; out_stat (zeroed by the caller) where plan.out_stats
int launch_attention_core(const AttnPlan& p, const float* qkv, const double2* qkv_mom, const float* x, float* scores, float* out, double2* out_stat,
                          float* ws, hipStream_t s);
// attn_plan.hip (host code only), for the launchers of attn.hip: a GEMM of the conv-pipeline form as a 1x1 conv with per-image weights, and the one
// walk over a core's workspace (null ws: sizes only; *end = the floats it spans)
ConvArgs attention_gemm(int nb, int H, int W, int cin, int cout);
AttnTables attention_tables(const AttnPlan& p, float* ws, size_t* end = nullptr);
// the rule of ATTN_FLASH (attn_plan.hip; queries per workgroup = keys per tile = ATTN_FLASH_TILE), and, in attn_flash.hip for launch_attention_core
// alone (no other caller), its tail once the tables and the row-major images of q and k are written (v^T pack + the kernel)
constexpr int ATTN_FLASH_TILE = 128;
bool attention_flash_applicable(int T, int C, int terms);
int launch_attention_flash(const AttnPlan& p, const AttnTables& t, const float* qkv, const float* x, float* out, hipStream_t s);

// boundary maps and the envmap warp (transform.hip)
int launch_map_chain(const float* x, float* out, long long per_image, int B, const int32_t* ops, const float* args, int n_ops, const float* lo,
                     const float* hi, const float* scale, hipStream_t s);
int launch_masked_log_range(const float* x, const float* mask, int B, int C, int HW, float* lo, float* hi, hipStream_t s);
int launch_luminance_scale(const float* x, int B, int HW, float scaler, float* scale, hipStream_t s);
int launch_mirmap2envmap(const float* mir, const float* basis, float* out, int B, int C, int H, int W, int OH, int OW, int log_interp, int nhwc,
                         hipStream_t s);
int launch_hdr2ldr(const float* x, const unsigned char* mask, int HW, float alpha, float gamma, float* out, hipStream_t s);
int launch_resize(const float* x, float* out, int planes, int IH, int IW, int OH, int OW, int mode, hipStream_t s);

// the sphere / envmap warp family (sphere_warp.hip; see drm_envmap2mirmap and its neighbours): in [B][C][H][W], or [B][H][W][C] with nhwc_in,
// frames [B][k][3] fp32 on the device, out [B][C][OH][OW]
int launch_envmap2mirmap(const float* env, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int mitigate_aliasing,
                         int log_interp, int nhwc_in, hipStream_t s);
int launch_rotate_envmap(const float* env, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int nhwc_in, hipStream_t s);
int launch_mirimg2envmap(const float* img, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int log_interp, int nhwc_in,
                         hipStream_t s);
int launch_refmap2refimg(const float* refmap, float* out, unsigned char* mask, int B, int C, int H, int W, int radius, int nhwc_in, hipStream_t s);

// reflectance-map forward model (render.hip; see drm_render_refmap): every sphere render, principled rows or tables, with or without light samples
size_t render_light_workspace_bytes(int B, int EH, int EW, int light_samples);
int launch_render_refmap(const drm_shading& sh, int L, int R, int subpixel, int flip, float* out, hipStream_t s);
// object images of a triangle mesh (see drm_render_mesh): visibility in mesh.hip, shading in render.hip next to the lobe code it shares.
// The workspace holds [B][F] face records of kMeshRecordWords 32-bit words, then [B][H S][W S] hits of kMeshHitWords words.
//   record: words 0-5 the view-space (x, y) of the three vertices, 6-8 their view-space z, 9 the signed 1 / (twice the screen area),
//   10-13 the screen box (xmin, xmax, ymin, ymax; an empty box (+inf, -inf) on a skipped face), 14-16 the vertex indices (int32),
//   17 the valid flag (int32), 18-19 padding
//   hit: (face id as int32 or -1, u, v, view-space z): the point is (1 - u - v) p0 + u p1 + v p2
constexpr int kMeshRecordWords = 20, kMeshHitWords = 4;
constexpr int kMeshRecIndex = 14, kMeshRecValid = 17;
// film position of sample column c of W S and of sample row r of H S (aspect = H / W): one definition for the visibility pass and for the
// shadow-ray origins of the shading pass
__host__ __device__ __forceinline__ float mesh_sample_x(int c, int WS) { return (float)(2 * c + 1) / (float)WS - 1.0f; }
__host__ __device__ __forceinline__ float mesh_sample_y(int r, int HS, float aspect) { return aspect * (1.0f - (float)(2 * r + 1) / (float)HS); }
size_t render_mesh_workspace_bytes(long long F, int B, int H, int W, int subpixel);
// the two visibility launches: records of every (row, face), then the nearest covering face of every film sample.  view [B][9] or null.
int launch_mesh_visibility(const float* positions, const int32_t* faces, long long V, long long F, const float* view, int B, int H, int W, int subpixel,
                           float* records, float* hits, hipStream_t s);
int launch_render_mesh(const drm_shading& sh, const drm_mesh_render& m, hipStream_t s);
// the same mesh under measured tables (see drm_render_mesh_tables): the same visibility, shading in mesh_table.hip
int launch_render_mesh_tables(const drm_shading& sh, const drm_mesh_render& m, hipStream_t s);
// a normal map shaded B ways (see drm_render_normals): normals [Bn][H][W][3] in the view frame, mask uint8 [Bn][H][W] or null
int launch_render_normals(const drm_shading& sh, const float* normals, const unsigned char* mask, int Bn, int H, int W, float* image, float* alpha,
                          hipStream_t s);
// validation losses (losses.hip): see drm_validation_losses
int launch_validation_losses(const float* model_out, const float* Lr_k, const float* Lr_km1, const int32_t* K, const float* z_out, const float* z_k,
                             const float* z_K, const int32_t* reversed_k, const float* z0, double gamma, int loss_type, double w_refmap,
                             double w_refcode, int B, long long per_row, int P, double* ws, size_t ws_bytes, float* out, hipStream_t s);
// ObsNet's forward process and diffusion losses (obs_forward.hip): see drm_obs_forward_process / drm_diffusion_losses
int launch_obs_forward_process(const float* x, const float* mask, const int32_t* t, const float* sqrt_ac, const float* sqrt_1mac, int T,
                               float noisy_observe, int padding_mode, const float* e_obs, const float* e_pad, const float* e_q, uint64_t seed,
                               float* cond, float* x_noisy, float* noise, int B, int C, int H, int W, int mask_H, int mask_W, hipStream_t s);
int launch_diffusion_losses(const float* model_out, const float* target, const float* invmask, const int32_t* t, const float* logvar,
                            const float* lvlb, int T, int loss_type, double w_simple, double w_elbo, int B, long long per_row, int C, double* ws,
                            size_t ws_bytes, float* out, float* rows_out, hipStream_t s);
// principled eval (f times n.l) of N (n, v, l) triples; z [1 or N][6]; out [N][3]
int launch_brdf_eval(const float* z, int z_rows, const float* n, const float* v, const float* l, float* out, long long N, hipStream_t s);
// measured BRDFs (brdf_table.hip): tables [NT][90][90][180][4] packed (r, g, b, 0) entries; table_of int32 per row / element or null (table 0)
int launch_brdf_to_merl(const float* z, int rows, float* tables_out, hipStream_t s);
int launch_merl_eval(const float* tables, int NT, const int32_t* table_of, const float* n, const float* v, const float* l, float* out, long long N,
                     int linear, hipStream_t s);
// BRDF-space error sums of C principled rows against a packed table or a principled row (brdf_error.hip): see drm_brdf_error_sums
int launch_brdf_error_sums(const float* z, int C, const float* table, const float* z_target, double* ws, size_t ws_bytes, double* sums, hipStream_t s);
// image-space error sums of P image pairs on a mask (image_error.hip): see drm_image_error_sums
int launch_image_error_sums(const drm_image_error& args, hipStream_t s);

// misc kernels (misc.hip)
// absmax_bits (optional): [N][pack_input_absmax_parts(H, W)] words, every one written: max |element| of one block of a packed image as fp32 bits
int pack_input_absmax_parts(int H, int W);
int launch_pack_input(const float* x, const float* cond, const int* idx, float* out, int N, int H, int W, int Cx, int Cc, int CP, hipStream_t s,
                      unsigned* absmax_bits = nullptr);
// stat (optional, zeroed): [N][C] (sum, sum of squares) of the pooled tensor, accumulated with fp64 atomics
int launch_avgpool2(const float* x, float* out, int N, int H, int W, int C, hipStream_t s, double2* stat = nullptr);
int launch_linear(const float* in, const float* w, const float* b, float* out, int N, int I, int O, int silu_in, int silu_out, hipStream_t s);
int launch_timestep_embedding(const int64_t* t, const float* tf, float* out, int N, int dim, hipStream_t s);
int launch_encoder_head(const float* x, const float* scale, const float* shift, const float* w, const float* b, float* out, int N, int HW,
                        int C, int O, hipStream_t s);
// the stem of a U-Net as a kernel of its own (stemhead.hip): conv3x3(in_channels -> 128) on the NCHW boundary tensors (cat + row gather fused,
// fused output statistics)
bool stem_direct_applicable(int Cin, int Cout);
size_t stem_weight_floats();
int launch_pack_stem_weight(const float* w, float* img, int Cout, int Cin, bool exact, hipStream_t s);  // exact: fp32 operands (PREC_FP32), else fp16 hi / lo
int launch_stem_conv(const float* x, int Cx, const float* cond, int Cc, const int* rows, const float* wimg, const float* bias, float* out, double2* stat,
                     int N, int H, int W, int Cout, bool exact, hipStream_t s);
int launch_nhwc_to_nchw(const float* x, float* out, int N, int H, int W, int C, hipStream_t s);
int launch_nchw_to_nhwc(const float* x, float* out, int N, int H, int W, int C, hipStream_t s);

}  // namespace drm
