// Object images of a triangle mesh under measured BRDFs (drm_render_mesh_tables): the shapes-under-MERL-materials case of the paper's
// evaluation, with self-shadowing.  Replaces, on the inference side (paths relative to the reference root), MitsubaOrthoRenderer.rendering
// with a measured BSDF (utils/mitsuba3_utils.py:433-564).  mesh.hip finds which face every film sample sees, exactly as for
// drm_render_mesh; mesh_table_shade_kernel here is the table counterpart of mesh_shade_kernel (render.hip): it shades every hit sample with
// table_lane_sum (brdf_table.h), the per-normal body of the sphere and normal-map renders under a table, so a mesh point is shaded exactly
// as the sphere point with the same normal.  SHADOW: every sample of either set with a non-zero balance weight is first asked of the
// mesh's BVH through the Tracer (mesh_shade.h) -- before the table and environment gathers, as Occluded asks before its lookup -- and an
// occluded one contributes nothing; an open one contributes the bits it contributes without shadows.
// One wave owns one pixel: its lanes stride the quad x quad grid over the pixel's hit samples in the per-lane order of mesh_shade_kernel
// and meet in wave_sum3.  fp32 throughout, no atomics, no LDS: bitwise reproducible, and a call of B rows equals its rows alone.
// Out of scope under a table: light samples, bounces, anisotropic tables.
#include <type_traits>

#include "brdf_table.h"
#include "bvh.h"
#include "common.h"
#include "mesh_shade.h"
#include "normal_map.h"
#include "render_shared.h"

namespace drm {

namespace {

// what table_lane_sum asks of a shadowed mesh: the ray from the hit sample along the world direction, the hit face excluded
struct TracedOpen {
  Tracer trace;
  __device__ __forceinline__ bool operator()(V3 w) const { return !trace.occluded(w); }
};

// grid: ceil(B H W / 4) workgroups of 4 waves; wave = pixel (row b, i, j) of the object image, under table table_of[b] with its proxy
// roughness, lit by env[b] and seen through view[b].  The hit samples, the shading normal, the ray origin and the four outputs are
// mesh_shade_kernel's: for each of the pixel's S x S samples, in sample order, the hit (one address: a broadcast), the barycentric mix of
// the face's vertex normals taken into the view frame and normalised (a zero mix stays zero), and, where n.z > 0, the per-normal sum.
// Lane 0 writes the pixel, the means of the normals and of 1.1 - z over the hits, and the hit fraction.  rec / hits: the workspace halves
// of launch_mesh_visibility.  Without SHADOW sh is an empty struct and the kernel holds nothing of the BVH.
template <bool VIEW, bool SHADOW>
__global__ __launch_bounds__(256) void mesh_table_shade_kernel(TableArgs margs, const float* __restrict__ env, const float* __restrict__ view,
                                                               const float* __restrict__ vnormal, const float* __restrict__ rec,
                                                               const float* __restrict__ hits, float* __restrict__ image, float* __restrict__ normal,
                                                               float* __restrict__ depth, float* __restrict__ alpha, int B, long long F, int H, int W, int EH,
                                                               int EW, int Q, int S, std::conditional_t<SHADOW, ShadowArgs, NoShadowArgs> sh) {
  const long long pix = (long long)blockIdx.x * kRenderWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pix >= (long long)B * H * W) return;  // (wave-uniform)
  const int b = __builtin_amdgcn_readfirstlane((int)(pix / ((long long)H * W)));
  const int rem = (int)(pix - (long long)b * H * W);
  const int i = rem / W, j = rem - (rem / W) * W;
  const TableMaterial mat(margs, b, b, EH, Q);
  const float* e = env ? env + (size_t)b * EH * EW * 3 : nullptr;
  const ViewRot rot = view_rot(VIEW ? view + 9 * (size_t)b : nullptr);
  const float4* hit = reinterpret_cast<const float4*>(hits) + (size_t)b * H * S * W * S;
  const float* records = rec + (size_t)b * F * kMeshRecordWords;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  float nsum[3] = {0.0f, 0.0f, 0.0f}, dsum = 0.0f;
  int count = 0;
  for (int sy = 0; sy < S; ++sy) {
    for (int sx = 0; sx < S; ++sx) {
      const float4 h = hit[((size_t)i * S + sy) * W * S + (size_t)j * S + sx];
      const int f = __float_as_int(h.x);
      if (f < 0) continue;  // (wave-uniform: every lane read the same hit)
      const float* r = records + (size_t)f * kMeshRecordWords;
      const float* n0 = vnormal + 3 * (size_t)__float_as_int(r[kMeshRecIndex]);
      const float* n1 = vnormal + 3 * (size_t)__float_as_int(r[kMeshRecIndex + 1]);
      const float* n2 = vnormal + 3 * (size_t)__float_as_int(r[kMeshRecIndex + 2]);
      const V3 n = unit_or_zero(from_world<VIEW>(rot, mix_normals(n0, n1, n2, h.y, h.z)));  // (a zero or NaN mix stays a zero normal)
      nsum[0] += n.x;
      nsum[1] += n.y;
      nsum[2] += n.z;
      dsum += 1.1f - h.w;
      ++count;
      if (n.z > 0.0f) {
        if constexpr (SHADOW) {
          // (built at each hit sample, as mesh_shade_kernel builds its traced techniques: nothing is carried from one to the next)
          TracedOpen open;
          trace_mesh(open.trace, sh, F);
          open.trace.from(mesh_sample_origin<VIEW>(rot, j * S + sx, i * S + sy, W, H, S, h.w), f);
          table_lane_sum<VIEW>(mat.tab, mat.alpha, mat.linear, e, rot, EH, EW, n, Q, lane, 64, acc, open);
        } else {
          table_lane_sum<VIEW>(mat.tab, mat.alpha, mat.linear, e, rot, EH, EW, n, Q, lane, 64, acc);
        }
      }
    }
  }
  wave_sum3(acc);
  if (lane == 0) {
    const float inv_s2 = 1.0f / (float)(S * S), scale = 1.0f / ((float)(S * S) * (float)(Q * Q));
    const size_t at = (size_t)i * W + j, plane = (size_t)H * W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      image[((size_t)b * 3 + c) * plane + at] = acc[c] * scale;
      if (normal) normal[((size_t)b * 3 + c) * plane + at] = nsum[c] * inv_s2;
    }
    if (depth) depth[(size_t)b * plane + at] = count > 0 ? dsum / (float)count : 0.0f;
    if (alpha) alpha[(size_t)b * plane + at] = (float)count * inv_s2;
  }
}

}  // namespace

// drm_render_mesh_tables: the checks of launch_render_mesh with the material turned round (tables, no z), then its visibility launches and
// the table shading.  Everything up to the blob's header and check_tables is decided without touching device memory; those two copy from
// the device, and nothing is launched before both have passed.
int launch_render_mesh_tables(const drm_shading& sh, const drm_mesh_render& m, hipStream_t s) {
  const std::string who = "render_mesh_tables";
  DRM_REQUIRE_SIZE(&m, drm_mesh_render);
  bool lit;
  std::string light_fault;
  DRM_TRY(check_shading(who, sh, m.subpixel, 0, &lit, &light_fault));  // (light samples under a map: refused there, under tables)
  DRM_REQUIRE(sh.tables, who + ": the material of this entry is tables (measured); a mesh under principled rows z is drm_render_mesh");
  DRM_REQUIRE(m.vertex_positions && m.vertex_normals && m.faces && m.image, who + ": null pointer");
  DRM_REQUIRE(m.bounces == 0, who + ": bounces under tables are not built (bounces must be 0)");
  const int B = sh.B;
  MeshLaunch ml;
  DRM_TRY(plan_mesh_render(who, B, m, ml));
  if (m.shadows) DRM_TRY(check_device_bvh(m.bvh, m.bvh_bytes, true, m.F, s, who.c_str()));
  DRM_TRY(check_tables(who, sh.tables, sh.NT, sh.table_of, B, sh.table_alpha, true, s));
  DRM_TRY(launch_mesh_visibility(m.vertex_positions, m.faces, m.V, m.F, sh.view, B, m.H, m.W, m.subpixel, ml.records, ml.hits, s));
  // (a view only turns the environment and the mesh: under a white environment the mesh still turns, so the view stays)
  const auto launch = [&](auto kernel, auto shadow) {
    hipLaunchKernelGGL(kernel, dim3(ml.blocks), dim3(64 * kRenderWaves), 0, s, table_args(sh), sh.envmap, sh.view, m.vertex_normals, ml.records, ml.hits,
                       m.image, m.normal, m.depth, m.alpha, B, m.F, m.H, m.W, sh.envmap ? sh.EH : 1, sh.envmap ? sh.EW : 1, sh.quad, m.subpixel, shadow);
  };
  const ShadowArgs shadow{m.vertex_positions, m.faces, m.V, m.bvh};
  if (sh.view && m.shadows) launch(mesh_table_shade_kernel<true, true>, shadow);
  else if (sh.view) launch(mesh_table_shade_kernel<true, false>, NoShadowArgs{});
  else if (m.shadows) launch(mesh_table_shade_kernel<false, true>, shadow);
  else launch(mesh_table_shade_kernel<false, false>, NoShadowArgs{});
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

}  // namespace drm
