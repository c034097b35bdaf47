// The forms of the conv pipeline (conv_split2_kernel), stated once: GEMM tiles, pixel-tile families, the instantiations that exist, their build units.
// plan_conv (conv_plan.hip) picks among them, dispatch_s2 (conv_split2.hip) and launch_igemm (conv.hip) instantiate from them.  Plain C++17, no HIP.
#pragma once

namespace drm {

// GEMM tiles, rows x channels: X(name, WM, WN, MT, NT) -- WM x WN waves of MT x NT 32x32 accumulators each
#define DRM_CONV_TILES(X) \
  X(TILE_256x256, 4, 2, 2, 4) X(TILE_256x192, 4, 2, 2, 3) X(TILE_256x128, 4, 2, 2, 2) X(TILE_128x128, 2, 2, 2, 2) X(TILE_256x64, 4, 2, 2, 1) \
  X(TILE_128x64, 2, 2, 2, 1) X(TILE_128x32, 4, 1, 1, 1)
#define DRM_X(name, wm, wn, mt, nt) name,
enum ConvTile : unsigned char { DRM_CONV_TILES(DRM_X) };
#undef DRM_X
struct TileShape {
  int wm, wn, mt, nt;
  constexpr int bm() const { return wm * mt * 32; }  // GEMM rows
  constexpr int bn() const { return wn * nt * 32; }  // channels
};
#define DRM_X(name, wm, wn, mt, nt) {wm, wn, mt, nt},
constexpr TileShape TILE_SHAPES[] = {DRM_CONV_TILES(DRM_X)};
#undef DRM_X
constexpr TileShape tile_shape(ConvTile t) { return TILE_SHAPES[t]; }

// Pixel-tile families, TH x TW pixels of one image, larger first: a GEMM tile of BM rows covers BM / (TH * TW) images
#define DRM_PIXEL_TILES(X) X(16, 16) X(8, 16) X(8, 8) X(4, 8) X(4, 4)
struct PixelTile { int th, tw; };
#define DRM_X(th, tw) {th, tw},
constexpr PixelTile PIXEL_TILES[] = {DRM_PIXEL_TILES(DRM_X)};
#undef DRM_X
// the family of the 128-row tiles next to a 256-row family (a 16 x 16 tile is 256 rows by itself)
constexpr PixelTile pixel_tile_rows128(PixelTile f) { return f.th * f.tw > 128 ? PixelTile{f.th / 2, f.tw} : f; }
constexpr bool pixel_tile_ragged(int th, int tw) { return th * tw <= 128 && !(th == 4 && tw == 8); }  // the families with masked-edge (RAG) instantiations
// 3x3 256-row tiles of 4-row pixel tiles (4x8 / 4x4 maps) do not exist: their multi-image halo tiles leave no room for 96 KB of weights
constexpr bool s2_rows256(int taps, int th) { return taps == 1 || th >= 8; }
// Whether conv_split2_kernel<taps, th, tw, tile_shape(tile)..., ring, tps, terms, ragged, sk, pool> is instantiated, and its weight ring (`ring` slots of
// `tps`-tap groups).  3x3: one barrier per kernel ROW (3 taps, 48 KB of weights per step, double-buffered); 1x1: one tap per step, ring of 4.  4 taps
// (the parity form of a 3x3 conv over a nearest-x2 input): one window ROW (2 taps) per step and barrier, ring of 2, on every GEMM tile of the 3x3 form
// (two-tap groups fit next to the halo tile where three-tap groups did not: 192-wide and 128x128 tiles); never ragged, split or pooled.  Those tiles of
// the other two run one-tap groups: 256x256 (1x1, f16x3) in a ring of 2, 256x192 and 128x128 in a ring of 3.  ragged: edge tiles masked, 128-row tiles
// at most 64 channels wide (exact fp32 runs ragged maps on conv_igemm_kernel); sk: split-K finished inside the launch; pool: the 2x2 average pool from
// the epilogue, split modes only.
struct S2Form { bool exists; int ring, tps; };
constexpr S2Form s2_form(int taps, int terms, int th, int tw, ConvTile tile, bool ragged, bool sk, bool pool) {
  const bool t16 = th == 16 && tw == 16, rows256 = s2_rows256(taps, th);
  const bool one_tap = taps != 4 && (tile == TILE_256x256 || tile == TILE_256x192 || tile == TILE_128x128);
  const int ring = one_tap ? (tile == TILE_256x256 ? 2 : 3) : (taps == 1 ? 4 : 2), tps = one_tap ? 1 : (taps == 9 ? 3 : (taps == 4 ? 2 : 1));
  bool e = !t16;  // (the plain forms on 128x64 and 128x32)
  if (ragged + sk + pool > (taps == 4 ? 0 : 1)) e = false;
  else if (ragged) e = terms != 0 && pixel_tile_ragged(th, tw) && (tile == TILE_128x64 || tile == TILE_128x32);
  else if (sk) e = tile == TILE_128x32 && !t16;
  else if (pool) e = tile == TILE_256x128 && taps == 9 && t16 && terms != 0;
  else if (tile == TILE_256x256) e = taps == 1 && t16 && terms == 3;
  else if (tile == TILE_256x192) e = t16 && (terms == 3 || (taps != 1 && terms == 2));
  else if (tile == TILE_256x128 || tile == TILE_256x64) e = rows256;
  else if (tile == TILE_128x128) e = !rows256;
  return {e, ring, tps};
}

// Build units: conv_split2.hip is compiled once per X(TAPS, TERMS), -DDRM_S2_UNIT=<10 * TAPS + TERMS> (drmnet_amd/build.py S2_UNITS is the same list:
// tests/test_conv_plan_cpu.py compares them).  TERMS: 0 exact fp32 operands (DRM_PREC_FP32); 1 plain fp16 operands, one MFMA per product
// (DRM_PREC_F16); 2 fp16 hi*hi + block-scaled fp8 cross terms (DRM_PREC_F16MX: the GroupNorm-fed 3x3 convs only); 3 fp16 hi / lo, three MFMAs per
// product; 4 plain bf16 operands (DRM_PREC_BF16).
#define DRM_S2_UNITS(X) X(9, 0) X(1, 0) X(9, 1) X(1, 1) X(9, 2) X(9, 3) X(1, 3) X(9, 4) X(1, 4) X(4, 0) X(4, 1) X(4, 2) X(4, 3) X(4, 4)

}  // namespace drm
