// torch.nn.functional.grid_sample(mode="bilinear", padding_mode="border", align_corners=False) on one sample position, stated once for
// the sphere / envmap warps of sphere_warp.hip and for mirmap2envmap_kernel in transform.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace drm {

// the four taps of a normalised position (u, v) in [-1, 1]^2 on an H x W image: (y0, x0) is always inside; x0 + 1 / y0 + 1 only where
// `has_x1` / `has_y1`.  Weights in ATen's order (nw, ne, sw, se).  A NaN position lands on texel 0 (fmaxf drops the NaN), so the
// taps are in bounds whatever the map computed.
struct BilinearTaps {
  int x0, y0;
  bool has_x1, has_y1;
  float w00, w01, w10, w11;
};

__device__ __forceinline__ BilinearTaps grid_sample_taps(float u, float v, int H, int W) {
  // unnormalise (align_corners = False), clip to the border, bilinear
  float ix = ((u + 1.0f) * (float)W - 1.0f) / 2.0f, iy = ((v + 1.0f) * (float)H - 1.0f) / 2.0f;
  ix = fminf((float)(W - 1), fmaxf(ix, 0.0f));
  iy = fminf((float)(H - 1), fmaxf(iy, 0.0f));
  const float fx = floorf(ix), fy = floorf(iy);
  BilinearTaps t;
  t.x0 = (int)fx;
  t.y0 = (int)fy;
  t.has_x1 = t.x0 + 1 < W;
  t.has_y1 = t.y0 + 1 < H;
  const float wx1 = ix - fx, wy1 = iy - fy, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
  t.w00 = wx0 * wy0;
  t.w01 = wx1 * wy0;
  t.w10 = wx0 * wy1;
  t.w11 = wx1 * wy1;
  return t;
}

}  // namespace drm
