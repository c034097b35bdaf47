// The attention planner: which form of the core (common.h AttnForm), its image group, its two GEMM plans and the walk over its workspace.  Host
// code only, no kernel and no HIP call: tools/attn_plan_check.hip includes this file (and conv_plan.hip) and checks on the host what every plan
// promises its launcher (attn.hip launch_attention_core, attn_flash.hip launch_attention_flash).
#include <algorithm>

#include "common.h"
#include "profiler.h"

namespace drm {

// (T = 512 -- RefNet's 16x32 level at the metric shape, 128 workgroups at batch 32 -- measured 0.106 ms per core against 0.114 ms for the
//  conv-pipeline form: the three packing launches and the half-empty chip eat the kernel's advantage; from T = 1024 it is 0.224 vs ~0.45 ms)
#ifndef FA_MIN_T
#define FA_MIN_T 1024
#endif
bool attention_flash_applicable(int T, int C, int terms) {
  return (terms == 3 || terms == 1 || terms == 4) && C == 384 && T % ATTN_FLASH_TILE == 0 && T >= FA_MIN_T;
}

// Images per attention pass: the [T, T] score matrices of a group live in the workspace between the S GEMM, the softmax and the PV GEMM.
// The group bounds that workspace (1 GiB: 64 images at T = 2048 -- batch 256 used to need 4.3 GB per attention block) while keeping the
// launches large.  Small groups that would keep the scores in the 256 MiB Infinity Cache were measured and lose: at batch 32, T = 2048 the
// attention core takes 6.3 ms in one pass, 7.1 ms in 128 MiB groups, 8.8 ms in 64 MiB groups, 11.8 ms in 32 MiB groups (under-filled grids
// and launch tails cost more than the HBM round trips of the scores).
#ifndef DRM_ATTN_GROUP_MIB
#define DRM_ATTN_GROUP_MIB 1024
#endif
static int attention_group(int N, int T) {
  const size_t per_image = (size_t)T * T * sizeof(float);
  const size_t g = ((size_t)DRM_ATTN_GROUP_MIB << 20) / (per_image ? per_image : 1);
  return (int)std::max<size_t>(1, std::min<size_t>(g, (size_t)N));
}
// S = alpha q k^T (cin = C, cout = T) and O = P v (cin = T, cout = C) of nb images: 1x1 convs with per-image weights (k, v^T)
ConvArgs attention_gemm(int nb, int H, int W, int cin, int cout) {
  ConvArgs a;
  a.C0 = cin; a.N = nb; a.H = H; a.W = W; a.taps = 1; a.Cout = cout;
  a.w_img_stride_f4 = (long long)cin * cout / 4; a.prof_kind = PROF_KINDS;  // (inside the core's profiler scope)
  return a;
}

// The one walk over a core's workspace: the pointers for `ws`, and in *end the floats it spans -- plan_attention sizes the workspace by the same walk
// (null ws), so a size and its carve cannot disagree.
AttnTables attention_tables(const AttnPlan& p, float* ws, size_t* end) {
  AttnTables t;
  const size_t N = (size_t)p.N, T = (size_t)p.H * p.W, C = (size_t)p.C, Z = C > T ? C : T;
  const bool flash = p.form == ATTN_FLASH, conv = p.form == ATTN_CONV;
  size_t at = 0;
  auto take = [&](bool have, size_t n) { float* r = have && ws ? ws + at : nullptr; at += have ? n : 0; return r; };
  if (flash || conv || p.guard) {
    t.wq = take(flash, N * T * C);
    t.wk = take(flash || conv, N * T * C);
    t.wv = take(flash || conv, N * T * C);
    t.q_tab = take(true, N * C);
    t.p_tab = take(true, N * T);
    t.zero_tab = take(true, N * Z);
    t.qk_inv = take(true, N); t.k_scale = take(true, N); t.k_inv = take(true, N);
    t.pv_inv = take(true, N); t.v_scale = take(true, N); t.v_inv = take(true, N);
    t.q_scale = take(!conv, N);  // (the conv pipeline reads q's factor from q_tab)
    at += 64;
  }
  if (end) *end = at;
  return t;
}

AttnPlan plan_attention(int N, int H, int W, int C, int precision) {
  AttnPlan p;
  const int T = H * W;
  p.N = N; p.H = H; p.W = W; p.C = C;
  p.terms = precision_terms(precision);
  p.group = attention_group(N, T);
  if (attention_flash_applicable(T, C, p.terms)) {
    p.form = ATTN_FLASH;
    p.out_stats = false;
  } else {
    // the T >= 256 levels: both GEMMs on the conv pipeline (which kernel takes them does not depend on the image count) -- except on sparse launches
    // (the 16x16 level of a batch-1 step: six launches, 51 us, where the short-sequence form -- qk_small, softmax, P v -- takes three and ~25 us)
    const ConvPlan qk = plan_conv(attention_gemm(p.group, H, W, C, T), precision), pv = plan_conv(attention_gemm(p.group, H, W, T, C), precision);
    if (qk.kernel == CONV_PIPELINE && pv.kernel == CONV_PIPELINE && (long long)N * T > 1024) {
      p.form = ATTN_CONV;
      p.qk[0] = qk; p.pv[0] = pv;
      if (N % p.group) {  // (the tile of a launch depends on its image count)
        p.qk[1] = plan_conv(attention_gemm(N % p.group, H, W, C, T), precision);
        p.pv[1] = plan_conv(attention_gemm(N % p.group, H, W, T, C), precision);
      }
    } else {
      // S = q k^T needs whole 32-chunks of C only (rows beyond T are masked); P v needs them of T: the 4x4 level (T = 16) of a 128x128 input keeps
      // the exact-fp32 form for P v and takes the split form for S like every other level
      p.split_qk = p.guard = p.terms != 0 && C % 32 == 0;
      p.split_pv = p.split_qk && T % 32 == 0;
    }
    p.scores_floats = (size_t)p.group * T * T;
  }
  attention_tables(p, nullptr, &p.ws_floats);
  return p;
}

}  // namespace drm
