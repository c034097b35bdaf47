// Measured BRDFs: a material given as a MERL table instead of a principled row.  Replaces, on the inference side (paths relative to the
// reference root):
//   bsdf_to_merl (a BSDF sampled on the MERL grid)                    utils/mitsuba3_utils.py:602-638
//   eval_bsdf / visualize_bsdf for a measured material               utils/mitsuba3_utils.py:641-690
//   MitsubaRefMapRenderer.rendering with a measured BSDF              utils/mitsuba3_utils.py:324-430
// A table is [90][90][180] entries over (theta_h, theta_d, phi_d) of Rusinkiewicz's half-vector parametrisation, node (i, j, k) standing for
// theta_h = (i / 90)^2 pi / 2, theta_d = j pi / 180, phi_d = k pi / 180.  On the device an entry is one float4 (r, g, b, 0), so a lookup
// corner is one 16-byte load; an entry without a measurement (below the horizon) is (-1, -1, -1, 0).  One table is 23 MB: it is read from
// memory (the Infinity Cache holds it), never staged in LDS.
//
// Stated once in brdf_table.h, for this file and for the mesh under a table (mesh_table.hip): table_coords (the coordinates of a direction
// pair, fp32 in the renders and fp64 in drm_merl_eval), table_lookup (both modes), table_lane_sum, the per-normal body of every render under
// a table with its balance heuristic over both sample sets of render_shared.h, and TableMaterial.  The renders here are the pixel kernels of
// render_shared.h instantiated with TableMaterial: one wave owns one pixel, its lanes split the grid, keep their partial sums in a fixed order
// and meet in wave_sum3: bitwise reproducible, no atomics, no LDS.  Here: the export and eval kernels, check_tables, and the launches.
#include <vector>

#include "brdf_table.h"
#include "common.h"
#include "merl_grid.h"
#include "normal_map.h"
#include "render_shared.h"

namespace drm {

namespace {

// one thread per entry of every row's table: the node's directions and the entry's value are merl_grid.h's (merl_node, merl_entry); -1 where
// n.wo < 0 or n.wi < 0, 0 where a cosine is exactly 0 (kSnap).
__global__ __launch_bounds__(256) void brdf_to_merl_kernel(const float* __restrict__ z, float4* __restrict__ out, long long total) {
  for (long long at = (long long)blockIdx.x * blockDim.x + threadIdx.x; at < total; at += (long long)gridDim.x * blockDim.x) {
    const long long row = at / kTableEntries;
    const MerlNode nd = merl_node((int)(at - row * kTableEntries));
    float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (merl_node_below(nd)) {
      e.x = e.y = e.z = -1.0f;
    } else if (merl_node_lit(nd)) {
      float f[3];
      merl_entry(principled(z + 6 * row), nd, f);
      e.x = f[0];
      e.y = f[1];
      e.z = f[2];
    }
    out[at] = e;
  }
}

// one thread per element: out[k] = f_table(n[k], v[k], l[k]) (n.l) under table table_of[k] (null: table 0), coordinates in fp64
__global__ __launch_bounds__(256) void merl_eval_kernel(const float4* __restrict__ tables, const int32_t* __restrict__ table_of, const float* __restrict__ n,
                                                        const float* __restrict__ v, const float* __restrict__ l, float* __restrict__ out, long long N,
                                                        int linear) {
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < N; k += (long long)gridDim.x * blockDim.x) {
    const double nn[3] = {n[3 * k], n[3 * k + 1], n[3 * k + 2]}, vv[3] = {v[3 * k], v[3 * k + 1], v[3 * k + 2]};
    const double ll[3] = {l[3 * k], l[3 * k + 1], l[3 * k + 2]};
    const double cv = nn[0] * vv[0] + nn[1] * vv[1] + nn[2] * vv[2], cl = nn[0] * ll[0] + nn[1] * ll[1] + nn[2] * ll[2];
    double f[3] = {0.0, 0.0, 0.0};
    if (cv > 0.0 && cl > 0.0) {
      double x[3];
      table_coords(nn, vv, ll, x);
      table_lookup(tables + (size_t)(table_of ? table_of[k] : 0) * kTableEntries, x, linear, f);
    }
    out[3 * k] = (float)(f[0] * cl);
    out[3 * k + 1] = (float)(f[1] * cl);
    out[3 * k + 2] = (float)(f[2] * cl);
  }
}

}  // namespace

// (declared in brdf_table.h)
int check_tables(const std::string& who, const void* tables, int NT, const int32_t* table_of, long long count, const float* alpha, bool renders,
                 hipStream_t s) {
  DRM_REQUIRE(tables && (reinterpret_cast<uintptr_t>(tables) & 15) == 0, who + ": tables must be a 16-byte aligned device pointer");
  DRM_REQUIRE(NT >= 1 && NT <= 4096, who + ": NT in [1, 4096] tables");
  DRM_REQUIRE(!renders || alpha, who + ": alpha is null");
  std::vector<int32_t> of(table_of ? (size_t)count : 0);
  std::vector<float> al(renders ? (size_t)NT : 0);
  if (!of.empty()) DRM_HIP_CHECK(hipMemcpyAsync(of.data(), table_of, of.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (!al.empty()) DRM_HIP_CHECK(hipMemcpyAsync(al.data(), alpha, al.size() * sizeof(float), hipMemcpyDeviceToHost, s));
  if (!of.empty() || !al.empty()) DRM_HIP_CHECK(hipStreamSynchronize(s));
  for (size_t k = 0; k < of.size(); ++k)
    DRM_REQUIRE(of[k] >= 0 && of[k] < NT, who + ": table_of[" + std::to_string(k) + "] = " + std::to_string(of[k]) + " is outside [0, NT = " +
                                              std::to_string(NT) + ")");
  for (size_t k = 0; k < al.size(); ++k)
    DRM_REQUIRE(al[k] >= 0.005f && al[k] <= 1.0f, who + ": alpha[" + std::to_string(k) + "] must be a finite value in [0.005, 1]");  // (a NaN fails both)
  return DRM_OK;
}

int launch_brdf_to_merl(const float* z, int rows, float* tables_out, hipStream_t s) {
  DRM_REQUIRE(z && tables_out, "brdf_to_merl: null pointer");
  DRM_REQUIRE((reinterpret_cast<uintptr_t>(tables_out) & 15) == 0, "brdf_to_merl: tables_out must be 16-byte aligned");
  DRM_REQUIRE(rows >= 1 && rows <= 4096, "brdf_to_merl: rows in [1, 4096]");
  const long long total = (long long)rows * kTableEntries;
  const long long blocks = std::min<long long>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(brdf_to_merl_kernel, dim3((unsigned)blocks), dim3(256), 0, s, z, reinterpret_cast<float4*>(tables_out), total);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

int launch_merl_eval(const float* tables, int NT, const int32_t* table_of, const float* n, const float* v, const float* l, float* out, long long N,
                     int linear, hipStream_t s) {
  DRM_REQUIRE(N >= 0 && N <= (1LL << 31), "merl_eval: 0 <= N <= 2^31");
  if (N == 0) return DRM_OK;
  DRM_REQUIRE(n && v && l && out, "merl_eval: null pointer");
  DRM_TRY(check_tables("merl_eval", tables, NT, table_of, N, nullptr, false, s));
  const long long blocks = std::min<long long>((N + 255) / 256, 65536);
  hipLaunchKernelGGL(merl_eval_kernel, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(tables), table_of, n, v, l, out, N,
                     linear ? 1 : 0);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

int launch_refmap_tables(const drm_shading& sh, const PixelLaunch& pl, int R, int subpixel, int flip, float* out, hipStream_t s) {
  DRM_TRY(check_tables("render_refmap", sh.tables, sh.NT, sh.table_of, sh.B, sh.table_alpha, true, s));
  const auto kernel = pl.view ? sphere_pixel_kernel<true, TableMaterial> : sphere_pixel_kernel<false, TableMaterial>;
  hipLaunchKernelGGL(kernel, dim3(pl.blocks), dim3(64 * kRenderWaves), 0, s, table_args(sh), sh.envmap, pl.view, out, sh.B, sh.B, R, pl.EH, pl.EW, sh.quad,
                     subpixel, flip ? 1 : 0);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

int launch_normals_tables(const drm_shading& sh, const PixelLaunch& pl, const float* normals, const unsigned char* mask, int Bn, int H, int W, float* image,
                          float* alpha, hipStream_t s) {
  DRM_TRY(check_tables("render_normals", sh.tables, sh.NT, sh.table_of, sh.B, sh.table_alpha, true, s));
  const auto kernel = pl.view ? normals_pixel_kernel<true, TableMaterial> : normals_pixel_kernel<false, TableMaterial>;
  hipLaunchKernelGGL(kernel, dim3(pl.blocks), dim3(64 * kRenderWaves), 0, s, table_args(sh), normals, mask, Bn, sh.envmap, pl.view, image, alpha, sh.B, H, W,
                     pl.EH, pl.EW, sh.quad);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

}  // namespace drm
