// A measured table as a material, for every source that shades under one (brdf_table.hip: the sphere, the normal map, drm_merl_eval;
// mesh_table.hip: the mesh): table_coords (the coordinates of a direction pair, fp32 in the renders and fp64 in drm_merl_eval), table_lookup
// (both modes), table_sample and table_lane_sum, the per-normal body of every render under a table, TableMaterial, the material of the pixel
// kernels of render_shared.h, and check_tables, what every entry that reads tables checks of them.  (Device side: unnamed namespace.)
//
// A table has no analytic lobe, so table_lane_sum cannot split the integrand as normal_lane_sum does: both sample sets of render_shared.h
// -- the Q x Q grid mapped to the GGX visible normals of the table's proxy roughness alpha (ggx_sample), and the same grid mapped to
// cosine-weighted directions (cosine_direction) -- estimate the whole integrand L f (n.l), combined with the balance heuristic: a sample l
// of either set adds L(l) f(n, v, l) (n.l) / (Q^2 (p_s(l) + p_d(l))), p_s = G1(v) D(h) / (4 n.v) at h = normalize(v + l), p_d = (n.l) / pi.
// The weights of a direction sum to one, so the rule is consistent for any alpha; alpha only decides where the accuracy goes.  No direction
// is constructed in this file.
#pragma once
#include <string>
#include <type_traits>

#include "common.h"
#include "merl_grid.h"
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

// What table_lane_sum asks about a sample with a non-zero balance weight before the table and the environment are read: is the world
// direction open?  Unoccluded answers yes for every one without a direction being formed for it: it compiles to nothing, and the kernels of
// the sphere, the normal map and the mesh without shadows are what they are without the question.  The shadowed mesh (mesh_table.hip)
// passes a callable that answers with a ray through its BVH.
struct Unoccluded {};
template <bool VIEW, typename OPEN>
__device__ __forceinline__ bool sample_open(const OPEN& open, const ViewRot& rot, V3 l) {
  if constexpr (std::is_same_v<OPEN, Unoccluded>) return true;  // (no direction is formed for the asking)
  else return open(to_world<VIEW>(rot, l));
}

// one lane's share of the radiance a surface point with unit normal n (n.z > 0) reflects toward the viewer at +z under a table: the grid
// points q = lane, lane + lanes, ... of both sample sets of render_shared.h, in that order, summed into acc (to be divided by Q^2), with
// the table's proxy roughness alpha in the place of the row's; what is stated here is the balance weight of each.  A sample that `open`
// refuses (asked along to_world(rot, l), the vector the environment lookup forms) contributes nothing; an open one is not changed by the asking.
template <bool VIEW, typename OPEN = Unoccluded>
__device__ __forceinline__ void table_lane_sum(const float4* __restrict__ tab, float alpha, int linear, const float* __restrict__ env, const ViewRot& rot,
                                               int EH, int EW, V3 n, int Q, int lane, int lanes, float acc[3], const OPEN& open = OPEN()) {
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
      if (s.vh > 0.0f && s.cl > 0.0f && D > 0.0f && sample_open<VIEW>(open, rot, s.l)) {
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
      if (cl > 0.0f && sample_open<VIEW>(open, rot, l)) table_sample<VIEW>(tab, linear, env, rot, EH, EW, n, l, cl / (ps + pd), acc);
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

// What every entry that reads tables checks of them before anything is launched (brdf_table.hip): the pointers, NT, every table_of value
// (brought to the host: `count` of them; null stands for table 0 everywhere) and, where the entry renders, every alpha.  `who` names the entry.
int check_tables(const std::string& who, const void* tables, int NT, const int32_t* table_of, long long count, const float* alpha, bool renders,
                 hipStream_t s);
// the launch arguments of a shading's tables, once check_tables has passed them
static inline TableArgs table_args(const drm_shading& sh) {
  return TableArgs{reinterpret_cast<const float4*>(sh.tables), sh.table_of, sh.table_alpha, sh.table_linear ? 1 : 0};
}

}  // namespace drm
