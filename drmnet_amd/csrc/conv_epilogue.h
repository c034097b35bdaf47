// The value rule of the conv epilogues, stated once, and the lane exchange / agent-scope accesses of the NHWC stores.  The library is
// built with -ffp-contract=off: the ORDER of the additions below is the contract the epilogues and every test digest rest on.
#pragma once
#include "common.h"

namespace drm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- the value rule: (acc * (w_inv * in_inv)) + bias + emb + res, in that order.  The in-launch split-K finish passes the slab sum, already scaled.
__device__ __forceinline__ float epi_scale(const ConvArgs& a, int n, float inv_scale) {
  // weight and (per image) input staging factors, all 2^-k (attention GEMMs: the "weights" are per image, and in_inv carries alpha)
  return (a.w_inv_img ? a.w_inv_img[n] : inv_scale) * (a.in_inv ? a.in_inv[n] : 1.0f);
}
__device__ __forceinline__ float epi_value(float scaled, float bias, float emb, float res) { return scaled + bias + emb + res; }

// ---- the fused GroupNorm statistics of a producer (conv_split2.hip, stemhead.hip, misc.hip avgpool2_kernel)
// Output statistics of a lane, about a pivot.  E[x^2] - E[x]^2 cancels badly when |mean| >> std (gn.hip squares in double for that reason), and an
// output channel does carry an offset: bias and emb are added right here.  Sums of x and x * x in fp32 lose the variance's low bits to the
// offset's square (2^6 on unit noise: eleven bits); sums of d = x - p and d * d about one of the lane's own values p are the size of the
// spread whatever the offset, so fp32 keeps them, and the pivot is put back exactly, in double, once per lane and row half:
//   sum x = sum d + n p,   sum x^2 = sum d^2 + p (2 sum d + n p).
__device__ __forceinline__ void stat_unpivot(float s, float q, float p, int n, double& S, double& Q) {
  const double pd = (double)p, sd = (double)s, np = (double)n * pd;
  S = sd + np;
  Q = (double)q + pd * (2.0 * sd + np);
}

// ---- the accesses and the lane exchange of the NHWC stores (conv_split2.hip, stemhead.hip)
// Agent-scope accesses of the fused split-K hand-off (sc1: coherent across the 8 XCD-private L2s by themselves, the way relaxed agent-scope atomics
// are -- LLVM AMDGPU memory model, gfx942 rows "load / store atomic monotonic agent").  The slabs move only through these, so the hand-off needs
// ordering (s_waitcnt vmcnt(0) before the ticket) but no L2 write-back / invalidate: MI355X_MICROARCH.md "Valid forms", first row of its table
// (one lane of each storing workgroup adds to ONE counter after every storing wave's vmcnt(0) wait and a barrier; the workgroup whose add came
// last loads after a barrier that lane joins; every store and every load of the bytes is a 16-byte global sc1 access).  Checked on this shape
// of hand-off by tools/probes/sc1_handoff_probe.hip: 0 stale values in 2 x 400 launches with the splits of a tile on one XCD and on different
// XCDs (plain accesses without the fences: 358 M stale values across XCDs), 9 / 15 us per launch against 33 / 57 us with the fences.
// (s_nop 1: a store of more than 8 bytes reads its data registers after issue -- the wait states the compiler inserts before it overwrites them
//  are invisible to it inside asm; without them the next quad transpose corrupted the slab)
// -DDRM_SK_FENCED=1: the conservative form of the same hand-off, kept compilable for A/Bs and as the switch to throw should a stale slab
// ever show -- plain slab stores / loads around an agent-scope release fence (one lane, before the ticket) and acquire fences (every wave of the
// finishing workgroup, after it): the LLVM memory model's documented release / acquire pair instead of per-access sc1 coherence.  19 vs 7 us per
// hand-off at the 64x64 level of the batch-1 step (profiles/r04_sc1_handoff_probe.txt); tools/skab.sh compares the two builds.
#ifdef DRM_SK_FENCED
__device__ __forceinline__ void gstore16_agent(void* p, const f32x4& v) { asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void gload16_agent(f32x4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(d) : "v"(p) : "memory"); }
#else
__device__ __forceinline__ void gstore16_agent(void* p, const f32x4& v) { asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void gload16_agent(f32x4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(d) : "v"(p) : "memory"); }
#endif

// 4 x 4 transpose across the four lanes of a quad: in, lane q holds x_k = M[q][k]; out, lane q holds x_k = M[k][q].
// Two butterfly stages (lane bit 0 with register pairs (0,1), (2,3); lane bit 1 with pairs (0,2), (1,3)); each moves one register
// per pair through a DPP quad permute and selects by lane parity.
template <int CTRL>
__device__ __forceinline__ float quad_perm(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ void quad_transpose(float& x0, float& x1, float& x2, float& x3, int lane) {
  const bool b0 = lane & 1, b1 = lane & 2;
  float t;
  t = quad_perm<0xB1>(b0 ? x0 : x1);  // [1,0,3,2]
  if (b0) x0 = t; else x1 = t;
  t = quad_perm<0xB1>(b0 ? x2 : x3);
  if (b0) x2 = t; else x3 = t;
  t = quad_perm<0x4E>(b1 ? x0 : x2);  // [2,3,0,1]
  if (b1) x0 = t; else x2 = t;
  t = quad_perm<0x4E>(b1 ? x1 : x3);
  if (b1) x1 = t; else x3 = t;
}

}  // namespace drm
