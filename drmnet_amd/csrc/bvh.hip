// The bounding-volume hierarchy behind the shadow rays of drm_render_mesh: the host builder (drm_mesh_bvh_build: no HIP call, usable
// without a GPU) and the stand-alone ray queries: any-hit (drm_mesh_occluded) and closest-hit (drm_mesh_closest_hit).  The blob layout, the
// triangle rule, the order of the closest hit and the traversal are in bvh.h.
//
// Builder.  Over object-space positions, so one tree serves every view of a call.  Kept faces (indices in [0, V), finite vertices, a non-zero
// fp32 cross product) are split at the median of their centroids along the longest axis of the centroids' box (std::nth_element, ties broken
// by the face index: the same input gives the same bytes) until a range holds at most 4: O(F log F), depth at most log2 F.  Nodes are emitted
// in depth-first order; a leaf's box is the bounds of its faces' vertices padded by 2^-16 of the largest |coordinate| of the kept faces, an
// inner node's box the union of its children's.  A range of n >= 5 faces splits into halves of at least 2, so there are at most F / 2 leaves
// and fewer than F nodes: drm_mesh_bvh_bytes = 32 + 36 F always suffices.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "bvh.h"

namespace drm {

namespace {

struct Builder {
  const float* pos;
  const int32_t* faces;
  float pad;
  std::vector<float> centroid;  // [F][3], kept faces only
  std::vector<int32_t> order;
  std::vector<BvhNode> nodes;

  void face_box(int32_t g, float lo[3], float hi[3]) const {
    for (int c = 0; c < 3; ++c) {
      const float* p = pos + 3 * (size_t)faces[3 * (size_t)g + c];
      for (int k = 0; k < 3; ++k) {
        lo[k] = std::min(lo[k], p[k]);
        hi[k] = std::max(hi[k], p[k]);
      }
    }
  }

  // nodes of order[begin, end), end - begin >= 1
  void build(size_t begin, size_t end) {
    const size_t at = nodes.size();
    nodes.push_back(BvhNode{});
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    uint32_t leaf = 0;
    if (end - begin <= (size_t)kBvhLeafFaces) {
      // (the comparison below is a strict total order, so which faces reach this leaf does not depend on the library's nth_element; their
      // order inside it would)
      std::sort(order.begin() + begin, order.begin() + end);
      for (size_t k = begin; k < end; ++k) face_box(order[k], lo, hi);
      for (int k = 0; k < 3; ++k) {
        lo[k] -= pad;
        hi[k] += pad;
      }
      leaf = (uint32_t)begin << 3 | (uint32_t)(end - begin);
    } else {
      float clo[3] = {inf, inf, inf}, chi[3] = {-inf, -inf, -inf};
      for (size_t k = begin; k < end; ++k)
        for (int a = 0; a < 3; ++a) {
          clo[a] = std::min(clo[a], centroid[3 * (size_t)order[k] + a]);
          chi[a] = std::max(chi[a], centroid[3 * (size_t)order[k] + a]);
        }
      int axis = 0;
      for (int a = 1; a < 3; ++a)
        if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
      const size_t mid = begin + (end - begin) / 2;
      std::nth_element(order.begin() + begin, order.begin() + mid, order.begin() + end, [&](int32_t x, int32_t y) {
        const float cx = centroid[3 * (size_t)x + axis], cy = centroid[3 * (size_t)y + axis];
        return cx < cy || (cx == cy && x < y);
      });
      const size_t left = nodes.size();
      build(begin, mid);
      const size_t right = nodes.size();
      build(mid, end);
      for (int k = 0; k < 3; ++k) {
        lo[k] = std::min(nodes[left].lo[k], nodes[right].lo[k]);
        hi[k] = std::max(nodes[left].hi[k], nodes[right].hi[k]);
      }
    }
    BvhNode& n = nodes[at];
    for (int k = 0; k < 3; ++k) {
      n.lo[k] = lo[k];
      n.hi[k] = hi[k];
    }
    n.skip = (int32_t)nodes.size();
    n.leaf = leaf;
  }
};

// ray k of a query and the face it leaves out (exclude null: none)
__device__ __forceinline__ Ray load_ray(const float* __restrict__ origins, const float* __restrict__ dirs, const int32_t* __restrict__ exclude, long long k,
                                        int32_t& ex) {
  const Ray r{{origins[3 * k], origins[3 * k + 1], origins[3 * k + 2]}, {dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]}};
  ex = exclude ? exclude[k] : -1;
  return r;
}

// grid ceil(N / 256): thread = ray
__global__ __launch_bounds__(256) void mesh_occluded_kernel(MeshRef m, const void* __restrict__ bvh, const float* __restrict__ origins,
                                                            const float* __restrict__ dirs, const int32_t* __restrict__ exclude,
                                                            int32_t* __restrict__ out, long long N) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= N) return;
  int32_t ex;
  const Ray r = load_ray(origins, dirs, exclude, k, ex);
  out[k] = (bvh ? bvh_occluded(m, bvh_view(bvh), r, ex) : brute_occluded(m, r, ex)) ? 1 : 0;
}

// grid ceil(N / 256): thread = ray; out_tuv [N][3] = (t, u, v), zeros where out_face is -1
__global__ __launch_bounds__(256) void mesh_closest_kernel(MeshRef m, const void* __restrict__ bvh, const float* __restrict__ origins,
                                                           const float* __restrict__ dirs, const int32_t* __restrict__ exclude,
                                                           int32_t* __restrict__ out_face, float* __restrict__ out_tuv, long long N) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= N) return;
  int32_t ex;
  const Ray r = load_ray(origins, dirs, exclude, k, ex);
  const Hit h = bvh ? bvh_closest(m, bvh_view(bvh), r, ex) : brute_closest(m, r, ex);
  out_face[k] = h.face;
  out_tuv[3 * k] = h.t;
  out_tuv[3 * k + 1] = h.u;
  out_tuv[3 * k + 2] = h.v;
}

bool faces_ok(long long F) { return F >= 1 && F < (1LL << 24); }

}  // namespace

size_t mesh_bvh_bytes(long long F) { return faces_ok(F) ? bvh_blob_bytes((uint32_t)F, (uint32_t)F) : 0; }

int mesh_bvh_build(const float* positions, const int32_t* faces, long long V, long long F, void* bvh, size_t bytes) {
  DRM_REQUIRE(positions && faces && bvh, "mesh_bvh_build: null pointer");
  DRM_REQUIRE(faces_ok(F) && V >= 1 && V <= 0x7fffffffLL, "mesh_bvh_build: 1 <= F < 2^24 faces, V >= 1 vertices");
  const size_t need = mesh_bvh_bytes(F);
  if (bytes < need) {
    set_error("mesh_bvh_build: the buffer must hold drm_mesh_bvh_bytes = " + std::to_string(need) + " bytes");
    return DRM_ERR_WORKSPACE;
  }
  Builder b{positions, faces, 0.0f, std::vector<float>(3 * (size_t)F, 0.0f), {}, {}};
  b.order.reserve((size_t)F);
  float largest = 0.0f;
  for (long long g = 0; g < F; ++g) {
    const int32_t* idx = faces + 3 * g;
    if (!(idx[0] >= 0 && idx[0] < V && idx[1] >= 0 && idx[1] < V && idx[2] >= 0 && idx[2] < V)) continue;
    const float* p0 = positions + 3 * (size_t)idx[0];
    const float* p1 = positions + 3 * (size_t)idx[1];
    const float* p2 = positions + 3 * (size_t)idx[2];
    bool finite = true;
    float big = 0.0f;
    for (int k = 0; k < 3; ++k) {
      finite = finite && std::isfinite(p0[k]) && std::isfinite(p1[k]) && std::isfinite(p2[k]);
      big = std::max(big, std::max(std::fabs(p0[k]), std::max(std::fabs(p1[k]), std::fabs(p2[k]))));
    }
    if (!finite) continue;
    const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    if (cross_is_zero(e1, e2)) continue;
    for (int k = 0; k < 3; ++k) b.centroid[3 * (size_t)g + k] = (p0[k] + p1[k] + p2[k]) * (1.0f / 3.0f);
    largest = std::max(largest, big);
    b.order.push_back((int32_t)g);
  }
  b.pad = kBvhPad * largest;
  if (!b.order.empty()) {
    b.nodes.reserve(b.order.size());
    b.build(0, b.order.size());
  }
  if (bvh_blob_bytes((uint32_t)b.nodes.size(), (uint32_t)b.order.size()) > need) {
    set_error("mesh_bvh_build: internal error: more nodes than drm_mesh_bvh_bytes allows");
    return DRM_ERR_STATE;
  }
  std::memset(bvh, 0, need);
  BvhHeader h{kBvhMagic, (uint32_t)F, (uint32_t)b.nodes.size(), (uint32_t)b.order.size(), {0, 0, 0, 0}};
  char* out = static_cast<char*>(bvh);
  std::memcpy(out, &h, sizeof(h));
  if (!b.nodes.empty()) std::memcpy(out + sizeof(h), b.nodes.data(), b.nodes.size() * sizeof(BvhNode));
  if (!b.order.empty()) std::memcpy(out + sizeof(h) + b.nodes.size() * sizeof(BvhNode), b.order.data(), b.order.size() * 4);
  return DRM_OK;
}

int check_device_bvh(const void* bvh, size_t bvh_bytes, bool have_bytes, long long F, hipStream_t s, const char* who) {
  const std::string name(who);
  DRM_REQUIRE(bvh && (reinterpret_cast<uintptr_t>(bvh) & 15) == 0, name + ": bvh must be a 16-byte aligned device pointer to a drm_mesh_bvh_build blob");
  DRM_REQUIRE(!have_bytes || bvh_bytes >= sizeof(BvhHeader), name + ": the bvh blob is shorter than its header");
  BvhHeader h;
  DRM_HIP_CHECK(hipMemcpyAsync(&h, bvh, sizeof(h), hipMemcpyDeviceToHost, s));
  DRM_HIP_CHECK(hipStreamSynchronize(s));
  DRM_REQUIRE(bvh_header_ok(h, F), name + ": the bvh blob was not built for this mesh (magic, face count or node counts do not match)");
  DRM_REQUIRE(!have_bytes || bvh_bytes >= bvh_blob_bytes(h.node_count, h.order_count), name + ": the bvh blob is shorter than its header says");
  return DRM_OK;
}

// what both ray queries check before they launch, `who` naming the entry in the messages; `pointers`: the entry's own are all there.  No
// rays: nothing is dereferenced, so neither the pointers nor the blob are looked at.
static int check_ray_query(const std::string& who, long long V, long long F, long long N, bool pointers, const void* bvh, hipStream_t s) {
  DRM_REQUIRE(N >= 0 && N <= (1LL << 31), who + ": 0 <= N <= 2^31 rays");
  DRM_REQUIRE(faces_ok(F) && V >= 1 && V <= 0x7fffffffLL, who + ": 1 <= F < 2^24 faces, V >= 1 vertices");
  if (N == 0) return DRM_OK;
  DRM_REQUIRE(pointers, who + ": null pointer");
  if (bvh) DRM_TRY(check_device_bvh(bvh, 0, false, F, s, who.c_str()));
  return DRM_OK;
}

int launch_mesh_occluded(const float* positions, const int32_t* faces, long long V, long long F, const void* bvh, const float* origins, const float* dirs,
                         const int32_t* exclude, int32_t* out, long long N, hipStream_t s) {
  DRM_TRY(check_ray_query("mesh_occluded", V, F, N, positions && faces && origins && dirs && out, bvh, s));
  if (N == 0) return DRM_OK;
  hipLaunchKernelGGL(mesh_occluded_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, MeshRef{positions, faces, V, F}, bvh, origins, dirs, exclude,
                     out, N);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

int launch_mesh_closest_hit(const float* positions, const int32_t* faces, long long V, long long F, const void* bvh, const float* origins,
                            const float* dirs, const int32_t* exclude, int32_t* out_face, float* out_tuv, long long N, hipStream_t s) {
  DRM_TRY(check_ray_query("mesh_closest_hit", V, F, N, positions && faces && origins && dirs && out_face && out_tuv, bvh, s));
  if (N == 0) return DRM_OK;
  hipLaunchKernelGGL(mesh_closest_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, MeshRef{positions, faces, V, F}, bvh, origins, dirs, exclude,
                     out_face, out_tuv, N);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

}  // namespace drm
