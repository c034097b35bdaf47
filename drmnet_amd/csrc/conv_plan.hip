// The conv planner: which kernel, which of its forms (conv_forms.h), the split-K form, and what folds into the launch.  Host code only, no kernel and
// no HIP call: tools/conv_plan_check.hip includes this file and checks on the host that every plan names a form that is instantiated.
#include <algorithm>
#include "common.h"

namespace drm {

constexpr long long S2_MIN_WIDE_TILES = 176;  // 256 x 128 tiles are used from this many workgroups on (of 256 CUs)
// On sparse launches (few images) the conv finalises its input's GroupNorm tables in its own prologue (ConvArgs::gnf, gn_fold.h) and no
// gn_finalize launch is made: at batch 1 a ~5 us launch per GroupNorm was 111 launches = a tenth of the DRMNet step.
constexpr int GN_FOLD_MAX_N = 4;
bool conv_split_weights(int precision, int cin) { return precision != PREC_FP32 && cin % 32 == 0; }

// Pixel-tile family of 128-row tiles for an H x W map: the one that wastes the fewest GEMM rows on masked edge pixels (ties: the larger tile).  Maps
// that are whole multiples of a tile (every shipped configuration) pick exactly what they always did; any other size the reference
// accepts (openaimodel.py:731-768 is fully convolutional) runs with masked edge tiles.  pipeline: among the families with RAG instantiations.
static PixelTile conv_tile_family(int H, int W, bool pipeline) {
  auto area = [&](const PixelTile& f) { return (long long)((H + f.th - 1) / f.th * f.th) * ((W + f.tw - 1) / f.tw * f.tw); };
  const PixelTile* best = nullptr;
  for (const PixelTile& f : PIXEL_TILES)
    if (f.th * f.tw <= 128 && (!pipeline || pixel_tile_ragged(f.th, f.tw)) && (!best || area(f) < area(*best))) best = &f;
  return *best;
}

ConvPlan plan_conv(const ConvArgs& a, int precision, bool want_pool, bool gn_foldable) {
  ConvPlan p;
  const int Ctot = a.C0 + a.C1, hw = a.H * a.W;
  const bool split = precision != PREC_FP32, chunks = Ctot % 32 == 0 && a.C0 % 32 == 0;
  const long long rows = (long long)a.N * hw;
  auto wgs = [&](int bm, int bn) { return ((rows + bm - 1) / bm) * (a.Cout / bn); };
  if (a.w_img_stride_f4 != 0) {
    // per-image weights (the attention GEMMs, attn.hip): split modes, one image per tile (maps of whole 16 x 16 tiles), 128-channel multiples
    if (!split || a.H % 16 != 0 || a.W % 16 != 0 || a.Cout % 128 != 0 || Ctot % 128 != 0) return p;
  }
  // The pipeline kernel (LDS-DMA weight ring, persistent tiles, fused output statistics) takes every conv whose channel counts are whole 32-chunks:
  // the split modes on any map, exact fp32 (TERMS = 0) on maps that are a whole number of 4x4 tiles.  The rest -- odd channel counts of the
  // per-module entry points, ragged maps in fp32 -- runs on conv_igemm_kernel (conv.hip): 128-row tiles, edge tiles masked.
  if (!chunks || (!split && (a.H % 4 != 0 || a.W % 4 != 0))) {
    const PixelTile f = conv_tile_family(a.H, a.W, false);
    p.kernel = CONV_IGEMM;
    p.th = f.th; p.tw = f.tw;
    p.tile = a.Cout % 128 == 0 ? TILE_128x128 : (a.Cout % 64 == 0 ? TILE_128x64 : TILE_128x32);
    p.kc = chunks ? 32 : 8;
    return p;
  }
  p.kernel = CONV_PIPELINE;
  p.terms = (precision == PREC_F16MX && a.mx_site) ? 2 : precision_terms(precision);
  p.gn_fold = gn_foldable && a.N <= GN_FOLD_MAX_N;
  // pixel-tile family: 256-row tiles of TH x TW pixels per image, 128-row tiles of pixel_tile_rows128 of it
  const PixelTile* fw = nullptr;
  for (const PixelTile& f : PIXEL_TILES)
    if (!fw && a.H % f.th == 0 && a.W % f.tw == 0) fw = &f;
  if (!fw) {
    // Maps that are not a whole number of tiles (any H, W the reference accepts other than the shipped sizes): 128-row tiles on 4 waves,
    // 64 or 32 channels wide, in three pixel-tile families, edge tiles masked (no split-K, no per-image weights)
    const PixelTile f = conv_tile_family(a.H, a.W, true);
    p.th = f.th; p.tw = f.tw;
    p.ragged = true;
    p.tile = a.Cout % 64 == 0 ? TILE_128x64 : TILE_128x32;
    return p;
  }
  // Split-K.  Deep levels (maps of at most 128 pixels: the 8x16 and 4x8 levels of a batch-32 step): too few GEMM rows for the 128-channel-wide
  // tiles to fill the chip, and the narrow tiles that do fill it re-stage (GroupNorm + SiLU + split) every activation tile once per 32 or 64 output
  // channels.  Split-K over the WIDE tiles instead: every split writes its slab, splitk_reduce_small_kernel finishes (two-launch form).
  // (1x1 convs of these levels on the same form measured neutral: 5.86 -> 5.54 ms of 1x1 time per step, given back by the reduction launches)
  int wide = 1;
  if (a.taps == 9 && !a.out_nchw && a.w_img_stride_f4 == 0 && a.Cout % 128 == 0 && hw <= 128 &&
      ((a.H % 8 == 0 && a.W % 16 == 0) || (a.H % 4 == 0 && a.W % 8 == 0)) && rows >= 1024) {  // (sparse launches keep the narrow tiles: a batch-1 step would fill half a wide tile)
    const int bm = (a.taps == 1 || (a.H % 8 == 0 && a.W % 16 == 0)) ? 256 : 128;  // (3x3 on 4x8 maps: 128-pixel x 128-channel tiles on 4 waves)
    const long long tiles = ((rows + bm - 1) / bm) * (a.Cout / 128);
    if (tiles < S2_MIN_WIDE_TILES) wide = (int)std::max<long long>(std::min<long long>(std::min<long long>(8, Ctot / 32 / 2), std::max<long long>(1, 256 / tiles)), 1);
  }
  // Deep U-Net levels (4x8 .. 8x16 maps) have few GEMM rows: with 256x128 tiles they launch far fewer workgroups than the chip has CUs.  Shrink
  // the tile (128 rows, then 64 / 32 channels) until the grid covers the 256 CUs.
  const bool rows256 = s2_rows256(a.taps, fw->th);
  auto tile = [&](ConvTile t, bool r256) { const PixelTile f = r256 ? *fw : pixel_tile_rows128(*fw); p.tile = t; p.th = f.th; p.tw = f.tw; };
  auto has = [&](ConvTile t, bool pool) { return s2_form(a.taps, p.terms, fw->th, fw->tw, t, false, false, pool).exists; };
  if (has(TILE_256x256, false) && a.Cout % 256 == 0 && wgs(256, 256) >= 512) {
    // 1x1 on big maps with Cout a multiple of 256: 256 output channels per tile (64 x 128 per wave, weight ring of 2).  The 1x1 form pays
    // its activation staging and its barrier once per 24 MFMAs of a wave; here per 48 (the 64x128-map skip convs: 11-15 % faster).  The
    // 1x1 kernel has the registers for it (176 -> 256 VGPRs, 2 spilled); the 3x3 kernel does not.
    tile(TILE_256x256, true);
  } else if (has(TILE_256x192, false) && a.Cout % 192 == 0 && wgs(256, 192) >= 512) {
    // 192 output channels per tile (64 x 96 per wave, one-tap weight ring of 3).  1x1 for Cout = 384 / 1152 / 1536 ...: qkv 512->1536 @16x32 and
    // the 32x64-map skip convs 12-16 % faster.  3x3 (f16x3, f16mx; the three-tap groups would not fit next to the halo tile) for Cout = 384 on
    // big maps: 12 fragment reads per 18 MFMA products instead of 8 per 12 -- 5 % faster there.  Fits since the scalar-base DMA addressing took
    // the kernel from 256 to 207 VGPRs.
    tile(TILE_256x192, true);
  } else if (a.Cout % 128 == 0 && (wgs(256, 128) >= S2_MIN_WIDE_TILES || wide > 1)) {
    // (one round of 128-wide tiles on >= 176 of the 256 CUs beats two rounds of the less efficient 64-wide ones: qkv 640->1920 @8x16 27 %,
    //  512->1536 @8x16 24 %, 3x3 384->384 @16x32 12 % faster than with the old "fill every CU" rule)
    tile(rows256 ? TILE_256x128 : TILE_128x128, rows256);
    // the Downsample behind a 3x3 conv on 16 x 16 pixel tiles, from its epilogue (split modes)
    p.pool = want_pool && !a.out_nchw && has(p.tile, true);
  } else if (a.Cout % 64 == 0 && wgs(256, 64) >= 256) {
    tile(rows256 ? TILE_256x64 : TILE_128x64, rows256);
  } else if (a.Cout % 64 == 0 && wgs(128, 64) >= 256) {
    // ([r4] 128 x 32 tiles from 512 workgroups on -- two workgroups per CU on the batch-1 step's top level instead of one: 4.74 vs 4.755 ms there,
    //  780 vs 800 steps/s at batch 32 -- not adopted: co-resident workgroups do not hide what a sparse launch waits for)
    tile(TILE_128x64, false);
  } else {
    // ([r4] a ring of 4 three-tap groups on these sparse-launch tiles: 5.31 vs 5.38 ms on the batch-1 step, later 5.06 vs 5.08 -- not adopted)
    tile(TILE_128x32, false);
  }
  // Split-K factor: the wide split above, else only the 128-row x 32-channel tiles qualify, when their grid leaves most of the 256 CUs idle and
  // the reduction is long.  (1x1 convs too [r3]: on the deep, small maps a K = 768 .. 1536 reduction is 24 .. 48 serial one-chunk steps of a
  // handful of workgroups -- 30 us at batch 1 whatever the map; split, they are ~5 chunks each plus the small-map reduction.)
  // ([r4] with the cheaper hand-off: splits of >= 2 chunks up to 1024 workgroups measured 5.13 vs 5.08 ms on the batch-1 step -- not adopted)
  p.ksplit = wide;
  if (wide == 1 && p.tile == TILE_128x32 && !a.out_nchw && a.w_img_stride_f4 == 0)
    p.ksplit = (int)std::max<long long>(std::min<long long>(std::min<long long>(8, Ctot / 32 / 4), 640 / std::max<long long>(wgs(128, 32), 1)), 1);
  if (p.ksplit > 1) {
    // Who finishes a split-K conv.  Maps of at least 128 pixels: the launch itself -- the workgroup that arrives last at an output tile sums the
    // slabs in slab order and runs the full epilogue (SK instantiation; the hand-off costs ~10 us whatever the shape).  Smaller maps:
    // splitk_reduce_small_kernel in a second launch (5.8 us on the 4x8 maps of the batch-32 step, where the fused finish measured 1 % slower on
    // the whole step; at batch 1 the maps of 128 .. 1024 pixels are where the second launch cost 12 .. 22 us: 6.64 -> 6.0 ms per step with the
    // fused finish).  ([r4] with the agent-scope hand-off the fused finish was tried on the smaller maps too: batch 1 4.79 vs 4.755 ms, batch 32
    // 759 vs 763 steps/s -- the second launch stays)
    p.finish = (hw >= 128 && wide == 1) ? SPLIT_IN_LAUNCH : SPLIT_REDUCE;
    // one arrival counter per output tile (128 GEMM rows x 32 channels; an upper bound over the pixel-tile families)
    if (p.finish == SPLIT_IN_LAUNCH) p.tickets = ((size_t)a.N * hw / 128 + (size_t)hw / 16 + 2) * (size_t)(a.Cout / 32);
  }
  return p;
}

}  // namespace drm
