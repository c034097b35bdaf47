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
// Stated once here: table_coords (the coordinates of a direction pair, fp32 in the renders and fp64 in drm_merl_eval), table_lookup (both
// modes) and table_lane_sum, the per-normal body of both renders.  A table has no analytic lobe, so table_lane_sum cannot split the
// integrand as normal_lane_sum does: both sample sets of render_shared.h -- the Q x Q grid mapped to the GGX visible normals of the table's
// proxy roughness alpha (ggx_sample), and the same grid mapped to cosine-weighted directions (cosine_direction) -- estimate the whole
// integrand L f (n.l), combined with the balance heuristic: a sample l of either set adds L(l) f(n, v, l) (n.l) / (Q^2 (p_s(l) + p_d(l))),
// p_s = G1(v) D(h) / (4 n.v) at h = normalize(v + l), p_d = (n.l) / pi.  The weights of a direction sum to one, so the rule is consistent
// for any alpha; alpha only decides where the accuracy goes.  No direction is constructed in this file.  The renders are the pixel kernels of
// render_shared.h instantiated with TableMaterial: one wave owns one pixel, its lanes split the grid, keep their partial sums in a fixed order
// and meet in wave_sum3: bitwise reproducible, no atomics, no LDS.
#include <vector>

#include "common.h"
#include "merl_grid.h"
#include "normal_map.h"
#include "render_shared.h"

namespace drm {

namespace {

// (the grid's sizes, kPi64 and the export's node geometry and entry value: merl_grid.h)
// The continuous table coordinates x = (90 sqrt(theta_h / (pi / 2)), 90 theta_d / (pi / 2), 180 phi_d / pi) of unit n, v (toward the
// viewer) and l (toward the light): h = normalize(v + l), theta_h = atan2(|n x h|, n.h), theta_d = atan2(|l x h|, l.h) (never acos of a dot
// product near 1), and MERL's azimuth: in the half-vector frame the normal lies at azimuth pi, x_h = -normalize(n - (n.h) h), y_h = h x x_h,
// phi_d = atan2(v.y_h, v.x_h) mod pi (reciprocity gives the other half); 0 where |n - (n.h) h| < 1e-6.
template <typename T>
__device__ __forceinline__ void table_coords(const T* n, const T* v, const T* l, T x[3]) {
  const T pi = T(kPi64);
  T h[3] = {v[0] + l[0], v[1] + l[1], v[2] + l[2]};
  const T hl = sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
  h[0] = h[0] / hl; h[1] = h[1] / hl; h[2] = h[2] / hl;
  const T nh = n[0] * h[0] + n[1] * h[1] + n[2] * h[2], lh = l[0] * h[0] + l[1] * h[1] + l[2] * h[2];
  T cx = n[1] * h[2] - n[2] * h[1], cy = n[2] * h[0] - n[0] * h[2], cz = n[0] * h[1] - n[1] * h[0];
  const T th = atan2(sqrt(cx * cx + cy * cy + cz * cz), nh);
  cx = l[1] * h[2] - l[2] * h[1]; cy = l[2] * h[0] - l[0] * h[2]; cz = l[0] * h[1] - l[1] * h[0];
  const T td = atan2(sqrt(cx * cx + cy * cy + cz * cz), lh);
  const T p[3] = {n[0] - nh * h[0], n[1] - nh * h[1], n[2] - nh * h[2]};
  const T pl = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  T ph = T(0);
  if (pl >= T(1e-6)) {
    const T xh[3] = {-p[0] / pl, -p[1] / pl, -p[2] / pl};
    const T yh[3] = {h[1] * xh[2] - h[2] * xh[1], h[2] * xh[0] - h[0] * xh[2], h[0] * xh[1] - h[1] * xh[0]};
    ph = atan2(v[0] * yh[0] + v[1] * yh[1] + v[2] * yh[2], v[0] * xh[0] + v[1] * xh[1] + v[2] * xh[2]);
    if (ph < T(0)) ph = ph + pi;
    if (ph >= pi) ph = ph - pi;
  }
  x[0] = T(90) * sqrt(th / (pi / T(2)));
  x[1] = T(90) * td / (pi / T(2));
  x[2] = T(180) * ph / pi;
}

__device__ __forceinline__ int clampi(int a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : a); }
__device__ __forceinline__ size_t entry_at(int i, int j, int k) { return ((size_t)i * kND + j) * kNP + k; }

// f_table at the coordinates x.  nearest (the MERL distribution reader's rule): floor, clamp to [0, 89] x [0, 89] x [0, 179], a negative
// entry reads 0.  linear: trilinear between floor and floor + 1, clamped at 89 in theta_h and theta_d and wrapping 179 -> 0 in phi_d; a
// corner whose entry is negative is dropped and the remaining weights renormalised, 0 where all eight are.  Every index is clamped after
// the conversion, so a NaN coordinate reads inside the table too.  The eight corner loads are issued together.
template <typename T>
__device__ __forceinline__ void table_lookup(const float4* __restrict__ tab, const T x[3], int linear, T f[3]) {
  const T fh = floor(x[0]), fd = floor(x[1]), fp = floor(x[2]);
  const int ih = (int)fh, id = (int)fd, ip = (int)fp;
  if (!linear) {
    const float4 e = tab[entry_at(clampi(ih, 0, kNH - 1), clampi(id, 0, kND - 1), clampi(ip, 0, kNP - 1))];
    const bool ok = !(e.x < 0.0f);
    f[0] = ok ? T(e.x) : T(0);
    f[1] = ok ? T(e.y) : T(0);
    f[2] = ok ? T(e.z) : T(0);
    return;
  }
  const int i0 = clampi(ih, 0, kNH - 1), i1 = clampi(ih + 1, 0, kNH - 1);
  const int j0 = clampi(id, 0, kND - 1), j1 = clampi(id + 1, 0, kND - 1);
  int k0 = clampi(ip, 0, 2 * kNP - 1) % kNP;
  const int k1 = k0 + 1 == kNP ? 0 : k0 + 1;
  float4 e[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) e[c] = tab[entry_at(c & 4 ? i1 : i0, c & 2 ? j1 : j0, c & 1 ? k1 : k0)];
  const T th = x[0] - fh, td = x[1] - fd, tp = x[2] - fp;
  T num[3] = {T(0), T(0), T(0)}, den = T(0);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const T w = e[c].x < 0.0f ? T(0) : (c & 4 ? th : T(1) - th) * (c & 2 ? td : T(1) - td) * (c & 1 ? tp : T(1) - tp);
    num[0] += w * T(e[c].x);
    num[1] += w * T(e[c].y);
    num[2] += w * T(e[c].z);
    den += w;
  }
  const bool ok = den > T(0);
  f[0] = ok ? num[0] / den : T(0);
  f[1] = ok ? num[1] / den : T(0);
  f[2] = ok ? num[2] / den : T(0);
}

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

// One sample of either set: a direction l above the surface (cl = n.l > 0) with its balance weight w = (n.l) / (p_s + p_d).  The table is
// asked first -- the eight corner loads go out together, ahead of the environment's four -- then the radiance is read along to_world(rot, l).
template <bool VIEW>
__device__ __forceinline__ void table_sample(const float4* __restrict__ tab, int linear, const float* __restrict__ env, const ViewRot& rot, int EH, int EW,
                                             V3 n, V3 l, float w, float acc[3]) {
  const float nn[3] = {n.x, n.y, n.z}, vv[3] = {0.0f, 0.0f, 1.0f}, ll[3] = {l.x, l.y, l.z};
  float x[3], f[3], L[3] = {1.0f, 1.0f, 1.0f};
  table_coords(nn, vv, ll, x);
  table_lookup(tab, x, linear, f);
  if (env) env_lookup(env, EH, EW, to_world<VIEW>(rot, l), L);
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[c] += L[c] * f[c] * w;
}

// one lane's share of the radiance a surface point with unit normal n (n.z > 0) reflects toward the viewer at +z under a table: the grid
// points q = lane, lane + lanes, ... of both sample sets of render_shared.h, in that order, summed into acc (to be divided by Q^2), with
// the table's proxy roughness alpha in the place of the row's; what is stated here is the balance weight of each.
template <bool VIEW>
__device__ __forceinline__ void table_lane_sum(const float4* __restrict__ tab, float alpha, int linear, const float* __restrict__ env, const ViewRot& rot,
                                               int EH, int EW, V3 n, int Q, int lane, int lanes, float acc[3]) {
  const float invQ = 1.0f / (float)Q, a2 = alpha * alpha;
  const float cv = n.z;
  const Frame f = duff_frame(n, 1.0f);
  const VisibleFrame vf = visible_frame(n, alpha);
  const float g1v = ggx_g1(a2, n.z, n.x * n.x + n.y * n.y, 1.0f);  // G1(v): v.h > 0 wherever it is used
  for (int q = lane; q < Q * Q; q += lanes) {
    const GridPoint g = grid_point(q, Q, invQ);
    // the GGX set: p_s from the h the sample was built from
    {
      const GgxSample s = ggx_sample(vf, alpha, n, f, g);
      const float D = ggx_d(a2, s.nh, s.s2h);
      if (s.vh > 0.0f && s.cl > 0.0f && D > 0.0f) {
        const float ps = visible_density(g1v, D, cv), pd = s.cl * (1.0f / kPi);
        table_sample<VIEW>(tab, linear, env, rot, EH, EW, n, s.l, s.cl / (ps + pd), acc);
      }
    }
    // the cosine set: p_s at h = normalize(v + l)
    {
      float cl;
      const V3 l = cosine_direction(n, f, g.u1, g.sp, g.cp, cl);
      const V3 h = half_vector(l);
      const float ps = visible_density(g1v, ggx_d(a2, dot3(n, h), cross_sq(n, h)), cv), pd = cl * (1.0f / kPi);
      if (cl > 0.0f) table_sample<VIEW>(tab, linear, env, rot, EH, EW, n, l, cl / (ps + pd), acc);
    }
  }
}

// The material of the pixel kernels (render_shared.h) for a table: row b is table table_of[b] (null: table 0) with alpha[table]; nothing joins.
struct TableArgs {
  const float4* tables;
  const int32_t* table_of;
  const float* alpha;
  int linear;
};
struct TableMaterial {
  using Args = TableArgs;
  static constexpr bool kStacked = false;  // rows = B
  const float4* tab;
  float alpha;
  int linear;
  __device__ __forceinline__ TableMaterial(const Args& a, int, int b, int, int) : linear(a.linear) {
    const int t = a.table_of ? a.table_of[b] : 0;
    tab = a.tables + (size_t)t * kTableEntries;
    alpha = a.alpha[t];
  }
  template <bool VIEW>
  __device__ __forceinline__ void lane_sum(const float* __restrict__ env, const ViewRot& rot, int EH, int EW, V3 n, int Q, int lane, int lanes, float acc[3]) {
    table_lane_sum<VIEW>(tab, alpha, linear, env, rot, EH, EW, n, Q, lane, lanes, acc);
  }
  __device__ __forceinline__ void meet() {}
  __device__ __forceinline__ float joined(int, float px, float) const { return px; }
};

}  // namespace

// What every entry that reads tables checks of them before anything is launched: the pointers, NT, every table_of value (brought to the
// host: `count` of them; null stands for table 0 everywhere) and, where the entry renders, every alpha.  `who` names the entry.
static int check_tables(const std::string& who, const void* tables, int NT, const int32_t* table_of, long long count, const float* alpha, bool renders,
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
  const TableArgs margs{reinterpret_cast<const float4*>(sh.tables), sh.table_of, sh.table_alpha, sh.table_linear ? 1 : 0};
  const auto kernel = pl.view ? sphere_pixel_kernel<true, TableMaterial> : sphere_pixel_kernel<false, TableMaterial>;
  hipLaunchKernelGGL(kernel, dim3(pl.blocks), dim3(64 * kRenderWaves), 0, s, margs, sh.envmap, pl.view, out, sh.B, sh.B, R, pl.EH, pl.EW, sh.quad, subpixel,
                     flip ? 1 : 0);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

int launch_normals_tables(const drm_shading& sh, const PixelLaunch& pl, const float* normals, const unsigned char* mask, int Bn, int H, int W, float* image,
                          float* alpha, hipStream_t s) {
  DRM_TRY(check_tables("render_normals", sh.tables, sh.NT, sh.table_of, sh.B, sh.table_alpha, true, s));
  const TableArgs margs{reinterpret_cast<const float4*>(sh.tables), sh.table_of, sh.table_alpha, sh.table_linear ? 1 : 0};
  const auto kernel = pl.view ? normals_pixel_kernel<true, TableMaterial> : normals_pixel_kernel<false, TableMaterial>;
  hipLaunchKernelGGL(kernel, dim3(pl.blocks), dim3(64 * kRenderWaves), 0, s, margs, normals, mask, Bn, sh.envmap, pl.view, image, alpha, sh.B, H, W, pl.EH,
                     pl.EW, sh.quad);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

}  // namespace drm
