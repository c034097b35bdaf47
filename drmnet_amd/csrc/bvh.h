// Any-hit and closest-hit ray queries against a triangle mesh: the blob layout of drm_mesh_bvh_build, the triangle rule and the stackless
// traversal.  Shared by bvh.hip (the host builder, drm_mesh_occluded, drm_mesh_closest_hit) and render.hip (mesh_shade_kernel<VIEW, true, LIGHT, BOUNCE>).  Everything here is plain C++ compiled for host
// and device with -ffp-contract=off: the builder's box arithmetic and the kernels' triangle arithmetic round identically on both sides.
//
// The rule (the same text as include/drmnet_hip.h).  A ray (o, d) in object space, d of any length, is occluded iff some face g != exclude with
// its three vertex indices in [0, V) has, with e1 = p1 - p0, e2 = p2 - p0, pv = d x e2, det = e1.pv, tv = o - p0, qv = tv x e1, U = tv.pv,
// V = d.qv, T = e2.qv, s = sign(det):  det != 0 and finite, s U >= 0, s V >= 0, s (U + V) <= |det|, s T > 0.  No division: edges and vertices
// are inclusive, a ray in the face's plane misses it (det = 0), an origin on the face misses it (T = 0).  A face whose fp32 cross product
// e1 x e2 is exactly (0, 0, 0) occludes nothing (in exact arithmetic its det is 0 for every ray; in fp32 it is rounding noise): the builder
// leaves such a face out with the same arithmetic, so the tree and the brute-force loop agree on it for every ray.
//
// The closest hit (the same text as include/drmnet_hip.h).  A face g is a candidate of (o, d, exclude) iff the rule above accepts it
// (face_hit is the one statement of the rule, the zero-cross-product clause included, and hands out det, U, V, T; "occluded" is "has a
// candidate", so occluded is true exactly where the closest hit finds a face).  A candidate has,
// in fp32, t = T / det, u = U / det, v = V / det, each the correctly rounded quotient (IEEE division on the host; on the device hipcc's
// default, which no flag of the build relaxes: no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt, denormals kept).  s T > 0 and a
// finite non-zero det make t one of +0 .. +inf, never NaN.  The hit is the candidate that is least under the lexicographic order (t, g), t
// compared as an fp32 value: a total order, so the order faces are visited in cannot matter.  Cross-multiplied products are not compared
// (rounded products are not transitive).  No candidate: face -1 (t = u = v = 0).  The hit point is o + t d, its barycentric weights
// (1 - u - v, u, v) on (p0, p1, p2).
//
// The blob.  32-byte header (BvhHeader), node_count nodes of 32 bytes (BvhNode) in depth-first order, order_count int32 face indices.  A leaf
// holds faces order[first .. first + count), count in [1, 4]; count = 0 marks an inner node, whose first child is the next node.  skip is the
// node to go to on a box miss or after a leaf: the end of the node's subtree.  Traversal needs no stack: on a box hit an inner node goes to
// i + 1, everything else to skip, and node_count ends it.  Neither query needs an ordered traversal (the order (t, g) is total, so the
// closest hit does not depend on the order of the visits), and a per-lane stack (a runtime-indexed private array) would live in scratch.
// One walk, bvh_query<CLOSEST>, serves both questions: it stops at the first candidate, or keeps the least and visits on; brute_query<CLOSEST>
// is the same choice over the loop through all faces.  The choice is made at compile time, so an any-hit kernel holds nothing of the other.
//
// Conservative boxes.  The fp32 rule may call a hit for a ray that passes a face at a distance of a few ulps of |o| + |p|.  The builder pads
// every leaf box by 2^-16 of the largest |coordinate| of the kept faces, the query pads by 2^-16 of the largest |o| component, the slab test
// gives its far bound 2^-20 of slack, a direction component that is exactly 0 tests the origin against the slab instead of dividing, and a NaN
// slab distance (0 x inf) leaves its axis unconstrained.  The boxes only cull: the triangle routine is the same in both paths.  With
// CLOSEST the walk also bounds the far end of the slab test by the best t so far (box_may_hit<true>), under the same 2^-20 of slack (a tie in
// t must still be visited: a lower face index wins it); the box pads are what keeps a face whose fp32 t lies a few ulps before its box from
// being culled.
#pragma once
#include "common.h"

namespace drm {

constexpr uint32_t kBvhMagic = 0x31485642u;  // "BVH1"
constexpr int kBvhLeafFaces = 4;
constexpr float kBvhPad = 1.0f / 65536.0f;

struct BvhHeader {
  uint32_t magic, faces, node_count, order_count, reserved[4];
};
struct alignas(16) BvhNode {
  float lo[3], hi[3];
  int32_t skip;
  uint32_t leaf;  // first << 3 | count
};
static_assert(sizeof(BvhHeader) == 32 && sizeof(BvhNode) == 32, "blob layout");

__host__ __device__ __forceinline__ size_t bvh_blob_bytes(uint32_t nodes, uint32_t order) {
  return sizeof(BvhHeader) + (size_t)nodes * sizeof(BvhNode) + (size_t)order * 4;
}
// header of a blob that may belong to a mesh of F faces
__host__ __device__ __forceinline__ bool bvh_header_ok(const BvhHeader& h, long long F) {
  return h.magic == kBvhMagic && (long long)h.faces == F && h.order_count <= h.faces && h.node_count <= h.faces;
}

struct MeshRef {
  const float* pos;
  const int32_t* faces;
  long long V, F;
};
struct BvhView {
  const BvhNode* nodes;
  const int32_t* order;
  uint32_t node_count, order_count;
};
__host__ __device__ __forceinline__ BvhView bvh_view(const void* blob) {
  const BvhHeader* h = static_cast<const BvhHeader*>(blob);
  const BvhNode* nodes = reinterpret_cast<const BvhNode*>(h + 1);
  return BvhView{nodes, reinterpret_cast<const int32_t*>(nodes + h->node_count), h->node_count, h->order_count};
}

struct Ray {
  float o[3], d[3];
};

__host__ __device__ __forceinline__ bool cross_is_zero(const float* e1, const float* e2) {
  return e1[1] * e2[2] - e1[2] * e2[1] == 0.0f && e1[2] * e2[0] - e1[0] * e2[2] == 0.0f && e1[0] * e2[1] - e1[1] * e2[0] == 0.0f;
}

// ---- the rule, and what a closest hit is formed from
struct FaceHit {
  float det, U, V, T;
};
struct Hit {
  int32_t face;  // -1: nothing hit
  float t, u, v;
};

// the rule for face g (g in [0, F)), handing out what the quotients are formed from; a vertex index outside [0, V) is never dereferenced.
// The only statement of the rule: the any-hit and the closest-hit queries, on host and device, all ask it.
__host__ __device__ __forceinline__ bool face_hit(const MeshRef& m, long long g, const Ray& r, FaceHit& h) {
  const int32_t i0 = m.faces[3 * g], i1 = m.faces[3 * g + 1], i2 = m.faces[3 * g + 2];
  if (!(i0 >= 0 && i0 < m.V && i1 >= 0 && i1 < m.V && i2 >= 0 && i2 < m.V)) return false;
  const float* p0 = m.pos + 3 * (size_t)i0;
  const float* p1 = m.pos + 3 * (size_t)i1;
  const float* p2 = m.pos + 3 * (size_t)i2;
  const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  const float pv[3] = {r.d[1] * e2[2] - r.d[2] * e2[1], r.d[2] * e2[0] - r.d[0] * e2[2], r.d[0] * e2[1] - r.d[1] * e2[0]};
  const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
  if (!(det != 0.0f && fabsf(det) < __builtin_huge_valf())) return false;  // (a NaN fails the second comparison)
  const float tv[3] = {r.o[0] - p0[0], r.o[1] - p0[1], r.o[2] - p0[2]};
  const float qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
  const float s = det > 0.0f ? 1.0f : -1.0f;
  const float U = tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2];
  const float Vb = r.d[0] * qv[0] + r.d[1] * qv[1] + r.d[2] * qv[2];
  const float T = e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2];
  if (!(s * U >= 0.0f && s * Vb >= 0.0f && s * (U + Vb) <= fabsf(det) && s * T > 0.0f)) return false;
  h = FaceHit{det, U, Vb, T};  // (read by the caller only after true; an any-hit caller never reads it and the stores go away)
  return !cross_is_zero(e1, e2);
}

// candidate g against the best so far, under the order (t, g)
__host__ __device__ __forceinline__ void closer_of(Hit& best, int32_t g, const FaceHit& h) {
  const float t = h.T / h.det;
  if (best.face < 0 || t < best.t || (t == best.t && g < best.face)) best = Hit{g, t, h.U / h.det, h.V / h.det};
}

// Both queries are one loop over candidates, closed at compile time: CLOSEST = false stops at the first candidate (the result then says
// only that there is one: face 0, t = u = v = 0), CLOSEST = true keeps the least under (t, g).  No candidate: face -1, t = u = v = 0.
template <bool CLOSEST>
__host__ __device__ __forceinline__ Hit brute_query(const MeshRef& m, const Ray& r, int32_t exclude) {
  Hit best{-1, __builtin_huge_valf(), 0.0f, 0.0f};
  FaceHit h;
  for (long long g = 0; g < m.F; ++g)
    if (g != exclude && face_hit(m, g, r, h)) {
      if constexpr (!CLOSEST) return Hit{0, 0.0f, 0.0f, 0.0f};
      closer_of(best, (int32_t)g, h);
    }
  return best.face < 0 ? Hit{-1, 0.0f, 0.0f, 0.0f} : best;
}

// may the ray, from t = 0 on, meet the box widened by pad?  Never false for a box that holds a face the rule calls a hit.  BOUNDED: the far
// end is also bounded by tmax, the best t so far (+inf while there is none), under the far bound's slack; otherwise tmax is not read.
template <bool BOUNDED>
__host__ __device__ __forceinline__ bool box_may_hit(const BvhNode& n, const Ray& r, const float* inv, float pad, float tmax) {
  const float inf = __builtin_huge_valf();
  float tn = 0.0f, tf = inf;
  bool out = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a = n.lo[k] - pad, b = n.hi[k] + pad;
    const float t0 = (a - r.o[k]) * inv[k], t1 = (b - r.o[k]) * inv[k];
    const bool free_axis = r.d[k] == 0.0f || t0 != t0 || t1 != t1;
    out = out || (r.d[k] == 0.0f && (r.o[k] < a || r.o[k] > b));
    tn = fmaxf(tn, free_axis ? 0.0f : fminf(t0, t1));
    tf = fminf(tf, free_axis ? inf : fmaxf(t0, t1));
  }
  if constexpr (BOUNDED) tf = fminf(tf, tmax);
  return !out && tn <= tf * (1.0f + 1.0f / 1048576.0f);
}

// The stackless walk.  Every index read from the blob is checked against the header's counts and skip must move forward, so a damaged blob
// cannot send a lane out of bounds or round in circles.  The same candidates as brute_query, so the same answer to the bit.
template <bool CLOSEST>
__host__ __device__ __forceinline__ Hit bvh_query(const MeshRef& m, const BvhView& t, const Ray& r, int32_t exclude) {
  const float inv[3] = {1.0f / r.d[0], 1.0f / r.d[1], 1.0f / r.d[2]};
  const float pad = kBvhPad * fmaxf(fabsf(r.o[0]), fmaxf(fabsf(r.o[1]), fabsf(r.o[2])));
  Hit best{-1, __builtin_huge_valf(), 0.0f, 0.0f};
  FaceHit h;
  uint32_t i = 0;
  while (i < t.node_count) {
    const BvhNode n = t.nodes[i];
    uint32_t next = (uint32_t)n.skip;
    if (box_may_hit<CLOSEST>(n, r, inv, pad, best.t)) {
      const uint32_t count = n.leaf & 7u, first = n.leaf >> 3;
      if (count == 0) next = i + 1;
      for (uint32_t k = 0; k < count; ++k) {
        if (first + k >= t.order_count) break;
        const int32_t g = t.order[first + k];
        if (g >= 0 && g < m.F && g != exclude && face_hit(m, g, r, h)) {
          if constexpr (!CLOSEST) return Hit{0, 0.0f, 0.0f, 0.0f};
          closer_of(best, g, h);
        }
      }
    }
    if (next <= i) break;
    i = next;
  }
  return best.face < 0 ? Hit{-1, 0.0f, 0.0f, 0.0f} : best;
}

// the names the callers use
__host__ __device__ __forceinline__ bool brute_occluded(const MeshRef& m, const Ray& r, int32_t exclude) { return brute_query<false>(m, r, exclude).face >= 0; }
__host__ __device__ __forceinline__ Hit brute_closest(const MeshRef& m, const Ray& r, int32_t exclude) { return brute_query<true>(m, r, exclude); }
__host__ __device__ __forceinline__ bool bvh_occluded(const MeshRef& m, const BvhView& t, const Ray& r, int32_t exclude) {
  return bvh_query<false>(m, t, r, exclude).face >= 0;
}
__host__ __device__ __forceinline__ Hit bvh_closest(const MeshRef& m, const BvhView& t, const Ray& r, int32_t exclude) {
  return bvh_query<true>(m, t, r, exclude);
}

size_t mesh_bvh_bytes(long long F);
int mesh_bvh_build(const float* positions, const int32_t* faces, long long V, long long F, void* bvh, size_t bytes);
// the header of a device blob, read back through the stream (one 32-byte copy and a stream synchronise), against F and, where the caller
// knows it, the blob's length
int check_device_bvh(const void* bvh, size_t bvh_bytes, bool have_bytes, long long F, hipStream_t s, const char* who);
int launch_mesh_occluded(const float* positions, const int32_t* faces, long long V, long long F, const void* bvh, const float* origins, const float* dirs,
                         const int32_t* exclude, int32_t* out, long long N, hipStream_t s);
int launch_mesh_closest_hit(const float* positions, const int32_t* faces, long long V, long long F, const void* bvh, const float* origins,
                            const float* dirs, const int32_t* exclude, int32_t* out_face, float* out_tuv, long long N, hipStream_t s);

}  // namespace drm
