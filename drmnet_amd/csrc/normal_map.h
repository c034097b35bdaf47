// Three-vectors and the reading of a normal map, shared by the kernels that go from a normal map to an image: normals_pixel_kernel
// (render_shared.h), which shades every pixel's normal, and image_from_refmap_kernel (refmap.hip), which looks it up in a reflectance map.
#pragma once
#include <hip/hip_runtime.h>

namespace drm {

struct V3 {
  float x, y, z;
};
__host__ __device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__host__ __device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// the unit vector along n, or zero where its length is zero or NaN (a NaN fails the comparison)
__host__ __device__ __forceinline__ V3 unit_or_zero(V3 n) {
  const float len2 = dot3(n, n);
  const float ninv = len2 > 0.0f ? 1.0f / sqrtf(len2) : 0.0f;
  return len2 > 0.0f ? v3(n.x * ninv, n.y * ninv, n.z * ninv) : v3(0.0f, 0.0f, 0.0f);
}

// Pixel `at` (of the H W pixels of one map) of a channel-last normal map in the view frame (right, up, back) and of its optional uint8
// mask: whether the pixel is drawn, and then n = unit_or_zero(normal).  Not drawn (image 0, alpha 0): the mask is 0 there, the normal is
// zero or NaN, or it does not face the viewer at +z (n.z <= 0; an infinite component normalises to NaN and fails the comparison too).  A
// masked-out pixel's normal is not read.
__device__ __forceinline__ bool normal_map_pixel(const float* __restrict__ normals, const unsigned char* __restrict__ mask, size_t at, V3& n) {
  if (mask && mask[at] == 0) return false;
  n = unit_or_zero(v3(normals[3 * at], normals[3 * at + 1], normals[3 * at + 2]));
  return n.z > 0.0f;
}

}  // namespace drm
