// Orthographic visibility of a triangle mesh: which face each film sample of drm_render_mesh sees, and where on it.  The shading of the hits
// (mesh_shade_kernel) lives in render.hip with the frame and lobe code it shares with the sphere.  Replaces the geometry half of
// MitsubaOrthoRenderer (utils/mitsuba3_utils.py:433-564 of the reference: orthographic sensor, smooth-shaded "obj" shape).
//
// Conventions (the same text as include/drmnet_hip.h):
//   view frame    right, up, back = the columns of the row-major Rot = view[b]; a mesh point enters it as Rot^T p.  No view, or an exact
//                 identity, multiplies nothing.
//   film samples  H x W pixels of S x S samples; sample column c = j S + sx is at x = (2 c + 1) / (W S) - 1, sample row r = i S + sy at
//                 y = (H / W) (1 - (2 r + 1) / (H S)).  The ray runs along -z: of the faces covering a sample the one with the largest
//                 view-space z is seen.
//   coverage      the three edge functions times the sign of the face's screen area are all >= 0 (edges inclusive), and the sample lies in
//                 the face's screen box (implied in exact arithmetic; tested so that the box cull below can never change a result).
//                 Ties: larger z, then the lower face index.  No back-face culling.  A face of zero screen area is skipped; so is one with a
//                 vertex index outside [0, V), which is never dereferenced.
//   hit           (face, u, v, z): u = e1 / |2 area|, v = e2 / |2 area|, z = z0 + u (z1 - z0) + v (z2 - z0).
//
// Two launches.  mesh_setup_kernel writes one 80-byte record per (row, face).  mesh_visibility_kernel gives a 16 x 16 tile of film samples
// to a workgroup, which streams all F records in chunks of 256: each thread loads one record and tests its box against the tile; the
// survivors are compacted in face order into an LDS list by a ballot and a prefix count (no atomics, no global list, nothing to overflow),
// and after a barrier every thread tests the list against its own sample.  Cost: tiles x F record reads, served by L2.
#include "common.h"

namespace drm {

namespace {

constexpr int kTile = 16;                 // film samples per tile side
constexpr int kChunk = kTile * kTile;     // threads of a workgroup = records per chunk
constexpr int kListWords = 16;            // LDS words per surviving record: record words 0-13, the face id, one pad

__device__ __forceinline__ float sample_x(int c, int WS) { return mesh_sample_x(c, WS); }
__device__ __forceinline__ float sample_y(int r, int HS, float aspect) { return mesh_sample_y(r, HS, aspect); }

// grid (ceil(F / 256), B): thread = (row b, face f)
__global__ __launch_bounds__(256) void mesh_setup_kernel(const float* __restrict__ pos, const int32_t* __restrict__ faces, const float* __restrict__ view,
                                                         float* __restrict__ rec, long long V, long long F) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (f >= F) return;
  const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  bool valid = i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
  float m[9];
  bool on = false;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float id = k % 4 == 0 ? 1.0f : 0.0f;
    m[k] = view ? view[9 * (size_t)b + k] : id;
    on = on || m[k] != id;
  }
  float x[3] = {0.0f, 0.0f, 0.0f}, y[3] = {0.0f, 0.0f, 0.0f}, z[3] = {0.0f, 0.0f, 0.0f};
  if (valid) {
    const int32_t idx[3] = {i0, i1, i2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float px = pos[3 * (size_t)idx[k]], py = pos[3 * (size_t)idx[k] + 1], pz = pos[3 * (size_t)idx[k] + 2];
      // Rot^T p
      x[k] = on ? m[0] * px + m[3] * py + m[6] * pz : px;
      y[k] = on ? m[1] * px + m[4] * py + m[7] * pz : py;
      z[k] = on ? m[2] * px + m[5] * py + m[8] * pz : pz;
    }
  }
  const float area2 = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0]);
  const float inv = 1.0f / area2;
  valid = valid && area2 != 0.0f && isfinite(inv);  // (a NaN or infinite vertex fails here)
  const float inf = __builtin_huge_valf();
  float4* out = reinterpret_cast<float4*>(rec + ((size_t)b * F + f) * kMeshRecordWords);
  out[0] = make_float4(x[0], y[0], x[1], y[1]);
  out[1] = make_float4(x[2], y[2], z[0], z[1]);
  out[2] = make_float4(z[2], valid ? inv : 0.0f, valid ? fminf(x[0], fminf(x[1], x[2])) : inf, valid ? fmaxf(x[0], fmaxf(x[1], x[2])) : -inf);
  out[3] = make_float4(valid ? fminf(y[0], fminf(y[1], y[2])) : inf, valid ? fmaxf(y[0], fmaxf(y[1], y[2])) : -inf, __int_as_float(i0), __int_as_float(i1));
  out[4] = make_float4(__int_as_float(i2), __int_as_float(valid ? 1 : 0), 0.0f, 0.0f);
}

// grid (tiles_x tiles_y, B), 256 threads: thread (tid / 16, tid % 16) of tile (ty, tx) owns film sample (ty 16 + tid / 16, tx 16 + tid % 16).
// Threads outside the film stay in every barrier and only their write is masked.
__global__ __launch_bounds__(kChunk) void mesh_visibility_kernel(const float* __restrict__ rec, float* __restrict__ hits, long long F, int HS, int WS,
                                                                 float aspect, int tiles_x) {
  __shared__ float4 list[kChunk * kListWords / 4];
  __shared__ int wave_count[kChunk / 64];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int b = blockIdx.y;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int c = tx * kTile + (tid & (kTile - 1)), r = ty * kTile + (tid >> 4);
  const bool in_film = c < WS && r < HS;
  const float px = sample_x(c, WS), py = sample_y(r, HS, aspect);
  // the tile's own sample positions bound it (sample_x rises with c, sample_y falls with r, both monotone in fp32)
  const float tile_x0 = sample_x(tx * kTile, WS), tile_x1 = sample_x(min(tx * kTile + kTile - 1, WS - 1), WS);
  const float tile_y1 = sample_y(ty * kTile, HS, aspect), tile_y0 = sample_y(min(ty * kTile + kTile - 1, HS - 1), HS, aspect);
  const float4* records = reinterpret_cast<const float4*>(rec + (size_t)b * F * kMeshRecordWords);
  int best_f = -1;
  float best_u = 0.0f, best_v = 0.0f, best_z = -__builtin_huge_valf();
  for (long long base = 0; base < F; base += kChunk) {
    const long long f = base + tid;
    bool keep = false;
    float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = q0, q2 = q0, q3 = q0;
    if (f < F) {
      const float4* p = records + (size_t)f * (kMeshRecordWords / 4);
      q0 = p[0]; q1 = p[1]; q2 = p[2]; q3 = p[3];
      // box (xmin, xmax, ymin, ymax) = (q2.z, q2.w, q3.x, q3.y); an empty box (a skipped face) or a NaN fails every comparison
      keep = q2.z <= tile_x1 && q2.w >= tile_x0 && q3.x <= tile_y1 && q3.y >= tile_y0;
    }
    const unsigned long long vote = __ballot(keep);
    if ((tid & 63) == 0) wave_count[wave] = __popcll(vote);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kChunk / 64; ++w) {
      const int n = wave_count[w];
      before += w < wave ? n : 0;
      total += n;
    }
    if (keep) {
      // survivors of the lower lanes of this wave, after those of the lower waves: face order
      const int slot = before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(vote >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)vote, 0u));
      q3.z = __int_as_float((int)f);
      list[slot * 4] = q0;
      list[slot * 4 + 1] = q1;
      list[slot * 4 + 2] = q2;
      list[slot * 4 + 3] = q3;
    }
    __syncthreads();
    for (int k = 0; k < total; ++k) {
      const float4 a = list[k * 4], bq = list[k * 4 + 1], cq = list[k * 4 + 2], d = list[k * 4 + 3];
      if (!(px >= cq.z && px <= cq.w && py >= d.x && py <= d.y)) continue;
      const float x0 = a.x, y0 = a.y, x1 = a.z, y1 = a.w, x2 = bq.x, y2 = bq.y;
      const float sg = cq.y > 0.0f ? 1.0f : -1.0f;
      const float e0 = ((x2 - x1) * (py - y1) - (y2 - y1) * (px - x1)) * sg;
      const float e1 = ((x0 - x2) * (py - y2) - (y0 - y2) * (px - x2)) * sg;
      const float e2 = ((x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)) * sg;
      if (!(e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f)) continue;
      const float ainv = fabsf(cq.y);
      const float u = e1 * ainv, v = e2 * ainv;
      const float z = bq.z + u * (bq.w - bq.z) + v * (cq.x - bq.z);
      const int fid = __float_as_int(d.z);
      if (z > best_z || (z == best_z && fid < best_f)) {
        best_z = z;
        best_u = u;
        best_v = v;
        best_f = fid;
      }
    }
    __syncthreads();  // (the list and the counts are rewritten by the next chunk)
  }
  if (in_film) {
    float4* out = reinterpret_cast<float4*>(hits) + ((size_t)b * HS + r) * WS + c;
    *out = make_float4(__int_as_float(best_f), best_u, best_v, best_f >= 0 ? best_z : 0.0f);
  }
}

bool mesh_shape_ok(long long F, int B, int H, int W, int subpixel) {
  return F >= 1 && F < (1LL << 24) && B >= 1 && B <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096 && subpixel >= 1 && subpixel <= 4;
}

}  // namespace

size_t render_mesh_workspace_bytes(long long F, int B, int H, int W, int subpixel) {
  if (!mesh_shape_ok(F, B, H, W, subpixel)) return 0;
  return (size_t)B * (size_t)F * kMeshRecordWords * 4 + (size_t)B * ((size_t)H * subpixel) * ((size_t)W * subpixel) * kMeshHitWords * 4;
}

int launch_mesh_visibility(const float* positions, const int32_t* faces, long long V, long long F, const float* view, int B, int H, int W, int subpixel,
                           float* records, float* hits, hipStream_t s) {
  DRM_REQUIRE(positions && faces && records && hits, "render_mesh: null pointer");
  DRM_REQUIRE(mesh_shape_ok(F, B, H, W, subpixel) && V >= 1 && V <= 0x7fffffffLL,
              "render_mesh: 1 <= F < 2^24 faces, V >= 1 vertices, 1 <= B <= 65535 rows, H and W in [1, 4096], subpixel in [1, 4]");
  const int HS = H * subpixel, WS = W * subpixel;
  const int tiles_x = (WS + kTile - 1) / kTile, tiles_y = (HS + kTile - 1) / kTile;
  hipLaunchKernelGGL(mesh_setup_kernel, dim3((unsigned)((F + 255) / 256), (unsigned)B), dim3(256), 0, s, positions, faces, view, records, V, F);
  hipLaunchKernelGGL(mesh_visibility_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)B), dim3(kChunk), 0, s, records, hits, F, HS, WS,
                     (float)H / (float)W, tiles_x);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

}  // namespace drm
