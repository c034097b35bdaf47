// What the two shading passes over mesh.hip's visibility share -- mesh_shade_kernel (render.hip: a principled row) and mesh_table_shade_kernel
// (mesh_table.hip: a measured table): the Tracer, through which every traced direction asks the mesh, the launch arguments that carry the
// mesh and its BVH to a shadowed kernel, and on the host the checks and the workspace carve of a drm_mesh_render.  (Device side: unnamed
// namespace.)
#pragma once
#include <string>

#include "bvh.h"
#include "common.h"
#include "render_shared.h"

namespace drm {

namespace {

// What the traced techniques ask the mesh: rays from one point of it, the face the point lies on left out.  The mesh and its tree come with
// the launch (ShadowArgs, trace_mesh); from() moves it to a hit sample.  The only place that builds a Ray for a shading pass.
struct Tracer {
  MeshRef mesh;
  BvhView tree;
  float o[3];       // the ray origin in object space
  int32_t exclude;  // the face it lies on
  __host__ __device__ __forceinline__ void from(V3 point, int32_t face) {
    o[0] = point.x;
    o[1] = point.y;
    o[2] = point.z;
    exclude = face;
  }
  __host__ __device__ __forceinline__ Ray ray(V3 w) const { return Ray{{o[0], o[1], o[2]}, {w.x, w.y, w.z}}; }
  __host__ __device__ __forceinline__ bool occluded(V3 w) const { return bvh_occluded(mesh, tree, ray(w), exclude); }
  __host__ __device__ __forceinline__ Hit closest(V3 w) const { return bvh_closest(mesh, tree, ray(w), exclude); }
};

// SHADOW: the mesh and its BVH as a shading kernel is given them.  Without it the kernel takes an empty struct and holds nothing of them.
struct NoShadowArgs {};
struct ShadowArgs {
  const float* positions;
  const int32_t* faces;
  long long V;
  const void* bvh;
};
// the mesh of F faces and its tree, as a Tracer holds them
__device__ __forceinline__ void trace_mesh(Tracer& t, const ShadowArgs& sh, long long F) {
  t.mesh = MeshRef{sh.positions, sh.faces, sh.V, F};
  t.tree = bvh_view(sh.bvh);
}
// the ray origin of film sample (column c of W S, row r of H S) of a hit at view-space depth z: the view-space hit point taken to object space
template <bool VIEW>
__device__ __forceinline__ V3 mesh_sample_origin(const ViewRot& rot, int c, int r, int W, int H, int S, float z) {
  return to_world<VIEW>(rot, v3(mesh_sample_x(c, W * S), mesh_sample_y(r, H * S, (float)H / (float)W), z));
}

}  // namespace

// What every mesh render checks of its drm_mesh_render after its own material and technique checks, without touching device memory: the
// limits, the grid, and the workspace (DRM_ERR_WORKSPACE), whose two halves it hands out.  `who` names the entry in the messages.
struct MeshLaunch {
  unsigned blocks;  // one wave per pixel, kRenderWaves to a workgroup
  float* records;   // [B][F] face records
  float* hits;      // [B][H S][W S] hits
};
static inline int plan_mesh_render(const std::string& who, int B, const drm_mesh_render& m, MeshLaunch& ml) {
  const size_t need = render_mesh_workspace_bytes(m.F, B, m.H, m.W, m.subpixel);
  DRM_REQUIRE(need != 0 && m.V >= 1 && m.V <= 0x7fffffffLL,
              who + ": 1 <= F < 2^24 faces, V >= 1 vertices, 1 <= B <= 65535 rows, H and W in [1, 4096], subpixel in [1, 4]");
  const long long blocks = pixel_blocks((long long)B * m.H * m.W);
  DRM_REQUIRE(blocks <= 0x7fffffffLL, who + ": B H W too large for one launch");
  if (!m.workspace || m.workspace_bytes < need || (reinterpret_cast<uintptr_t>(m.workspace) & 15) != 0) {
    set_error(who + ": workspace must be 16-byte aligned and hold drm_render_mesh_workspace_bytes = " + std::to_string(need) + " bytes");
    return DRM_ERR_WORKSPACE;
  }
  float* records = static_cast<float*>(m.workspace);
  ml = MeshLaunch{(unsigned)blocks, records, records + (size_t)B * m.F * kMeshRecordWords};
  return DRM_OK;
}

}  // namespace drm
