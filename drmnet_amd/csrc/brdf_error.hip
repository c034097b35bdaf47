// BRDF-space error sums: how far principled rows are from a target BRDF on the MERL grid (drm_brdf_error_sums; the host turns the sums into
// the figures of drmnet_amd/reflectance.py, and fit_principled searches with them).  C candidate rows are scored against one target -- a
// packed table, or one principled row -- in one pass over the 1 458 000 nodes: the target entry is read once per node, every candidate is
// evaluated there in fp64 (merl_grid.h: the value drm_brdf_to_merl would store, so a row against its own export scores exactly 0), and nothing
// per candidate goes to memory but kErrParts x 9 fp64 partial sums.
//
// Mapping.  A block is 256 threads = 16 candidate lanes x 16 node lanes and owns (part, chunk): the tiles part, part + 128, ... of 256
// consecutive nodes, scored against the candidates 16 chunk .. 16 chunk + 15.
//   stage   thread t forms node 256 tile + t once: its cosines (six fp64 sin / cos), the 16-byte target entry and the target's share of
//           every term (log10 b, log1p(b ci)), 15 doubles in LDS.  A node that does not count is staged with ci = 0 and skipped.
//   score   a thread keeps ONE candidate in registers for the whole launch (its Principled struct is 32 bytes: registers hold what LDS would)
//           and walks the nodes lane, lane + 16, ... of the tile; the 16 candidate lanes read the same LDS address (a broadcast), the four node
//           lanes of a wave four different banks (the stride is 30 words).  The nine sums stay in registers across all tiles: no shuffle and
//           no reduction inside the loop, which is what a thread-per-node mapping would pay per candidate.
//   meet    once per block: the 16 node lanes of a candidate meet in a fixed tree through LDS; partial [part][c][9] goes to the workspace.
// A finalising launch adds the 128 parts of every (candidate, sum) in order.  The order in which a candidate's nodes are added depends on
// (part, node lane) alone, never on C or on the candidate's place in the batch: a row scored alone, or as any row of any batch, gives the same
// bits; there are no atomics, so two calls are bitwise equal.
// Cost of the choice: a chunk with fewer than 16 candidates leaves lanes idle (C = 1 runs at 1 / 16), and every chunk stages the nodes again
// (about 1 / 16 of its scoring work).  The searches this serves score 104 rows and more per launch.
#include "../../include/drmnet_hip.h"
#include "common.h"
#include "merl_grid.h"

namespace drm {

namespace {

constexpr int kErrThreads = 256;
constexpr int kErrCand = 16;                         // candidate lanes of a block
constexpr int kErrLanes = kErrThreads / kErrCand;    // node lanes of a block
constexpr int kErrParts = 128;                       // DRM_BRDF_ERROR_PARTS: partial sums per (candidate, sum)
constexpr int kErrSums = 9;                          // DRM_BRDF_ERROR_SUMS
constexpr int kErrTile = kErrThreads;                // nodes staged at a time, one per thread
constexpr int kErrTiles = (int)((kTableEntries + kErrTile - 1) / kErrTile);
constexpr int kErrNode = 15;                         // doubles per staged node: cv, cl, nh, cd, lh, ci, b[3], log10 b [3], log1p(b ci) [3]
static_assert(kErrNode >= kErrSums, "the meet reuses the staging buffer");
static_assert(kErrParts == DRM_BRDF_ERROR_PARTS && kErrSums == DRM_BRDF_ERROR_SUMS, "include/drmnet_hip.h states the workspace size");

__global__ __launch_bounds__(kErrThreads) void brdf_error_partial_kernel(const float* __restrict__ z, int C, const float4* __restrict__ table,
                                                                         const float* __restrict__ z_target, double* __restrict__ ws) {
  __shared__ double sh[kErrTile * kErrNode];
  const int tid = threadIdx.x, cand = tid % kErrCand, lane = tid / kErrCand;
  const int part = blockIdx.x, c = blockIdx.y * kErrCand + cand;
  const Principled p = principled(z + 6 * (c < C ? c : C - 1));  // (an idle lane scores the last row and writes nothing)
  Principled pt = p;
  if (z_target) pt = principled(z_target);
  double acc[kErrSums];
#pragma unroll
  for (int s = 0; s < kErrSums; ++s) acc[s] = 0.0;
  for (int tile = part; tile < kErrTiles; tile += kErrParts) {
    __syncthreads();  // the last tile has been read
    {
      const int at = tile * kErrTile + tid;
      float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (table && at < (int)kTableEntries) e = table[at];  // one 16-byte load, issued ahead of the trigonometry
      double* nd_out = sh + tid * kErrNode;
      nd_out[5] = 0.0;
      if (at < (int)kTableEntries) {
        const MerlNode nd = merl_node(at);
        float b[3] = {e.x, e.y, e.z};
        bool counts = merl_node_lit(nd);
        if (counts && !table) merl_entry(pt, nd, b);
        counts = counts && b[0] >= 0.0f && b[1] >= 0.0f && b[2] >= 0.0f;
        if (counts) {
          nd_out[0] = nd.g.cv; nd_out[1] = nd.g.cl; nd_out[2] = nd.g.nh; nd_out[3] = nd.g.cd; nd_out[4] = nd.g.lh;
          nd_out[5] = nd.ci;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const double bv = (double)b[ch];
            nd_out[6 + ch] = bv;
            nd_out[9 + ch] = bv > 0.0 ? log10(bv) : 0.0;
            nd_out[12 + ch] = log1p(bv * nd.ci);
          }
        }
      }
    }
    __syncthreads();
    for (int q = lane; q < kErrTile; q += kErrLanes) {
      const double* nd_in = sh + q * kErrNode;
      const double ci = nd_in[5];
      if (!(ci > 0.0)) continue;
      MerlNode nd;
      nd.g.cv = nd_in[0]; nd.g.cl = nd_in[1]; nd.g.nh = nd_in[2]; nd.g.cd = nd_in[3]; nd.g.lh = nd_in[4];
      nd.co = nd.g.cv;
      nd.ci = ci;
      float a[3];
      merl_entry(p, nd, a);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const double av = (double)a[ch], bv = nd_in[6 + ch];
        acc[0] += 1.0;
        if (av > 0.0 && bv > 0.0) {
          const double d = log10(av) - nd_in[9 + ch];
          acc[1] += 1.0;
          acc[2] += d;
          acc[3] += d * d;
        }
        const double ac = av * ci, bc = bv * ci;
        const double l = log1p(ac) - nd_in[12 + ch];
        acc[4] += l * l;
        const double dl = (av - bv) * ci;
        acc[5] += dl * dl;
        acc[6] += ac * ac;
        acc[7] += ac * bc;
        acc[8] += bc * bc;
      }
    }
  }
  // the node lanes of a candidate meet: fixed tree over lane, through the staging buffer
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kErrSums; ++s) sh[tid * kErrSums + s] = acc[s];
  __syncthreads();
#pragma unroll
  for (int o = kErrLanes / 2; o > 0; o >>= 1) {
    if (lane < o) {
#pragma unroll
      for (int s = 0; s < kErrSums; ++s) sh[tid * kErrSums + s] += sh[(tid + o * kErrCand) * kErrSums + s];
    }
    __syncthreads();
  }
  if (lane == 0 && c < C) {
    double* out = ws + ((size_t)part * C + c) * kErrSums;
#pragma unroll
    for (int s = 0; s < kErrSums; ++s) out[s] = sh[tid * kErrSums + s];
  }
}

// one thread per (candidate, sum): the parts in order
__global__ __launch_bounds__(kErrThreads) void brdf_error_finalize_kernel(const double* __restrict__ ws, int C, double* __restrict__ sums) {
  const int at = blockIdx.x * kErrThreads + threadIdx.x;
  if (at >= C * kErrSums) return;
  double s = 0.0;
  for (int part = 0; part < kErrParts; ++part) s += ws[(size_t)part * C * kErrSums + at];
  sums[at] = s;
}

}  // namespace

int launch_brdf_error_sums(const float* z, int C, const float* table, const float* z_target, double* ws, size_t ws_bytes, double* sums, hipStream_t s) {
  DRM_REQUIRE(z && ws && sums, "brdf_error_sums: null pointer");
  DRM_REQUIRE((table != nullptr) != (z_target != nullptr), "brdf_error_sums: exactly one of table and z_target is the target");
  DRM_REQUIRE(C >= 1 && C <= 4096, "brdf_error_sums: C in [1, 4096] candidate rows");
  DRM_REQUIRE(!table || (reinterpret_cast<uintptr_t>(table) & 15) == 0, "brdf_error_sums: table must be a 16-byte aligned device pointer");
  DRM_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7) == 0, "brdf_error_sums: ws and sums must be 8-byte aligned");
  DRM_REQUIRE(ws_bytes >= sizeof(double) * kErrParts * kErrSums * (size_t)C, "brdf_error_sums: workspace smaller than DRM_BRDF_ERROR_WORKSPACE_BYTES(C)");
  hipLaunchKernelGGL(brdf_error_partial_kernel, dim3(kErrParts, (C + kErrCand - 1) / kErrCand), dim3(kErrThreads), 0, s, z, C,
                     reinterpret_cast<const float4*>(table), z_target, ws);
  DRM_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(brdf_error_finalize_kernel, dim3((C * kErrSums + kErrThreads - 1) / kErrThreads), dim3(kErrThreads), 0, s, ws, C, sums);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

}  // namespace drm
