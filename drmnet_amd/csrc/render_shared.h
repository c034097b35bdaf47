// What the per-normal sums of render.hip (normal_lane_sum: a principled row) and brdf_table.h (table_lane_sum: a measured table) share:
// the three-vector helpers, the frame about a normal and the cosine-weighted direction, the sample sets (the grid point, the visible-normal
// frame, the GGX sample, its density, the half vector), the principled row with its GGX, Fresnel and diffuse terms and their eval, the
// environment lookup (env_taps + bilerp), the sensor's normals, the view rotation and the wave butterfly; the two pixel kernels, templates
// over the material that each source instantiates with its own; and the checks and grid of their launches.  (Device side: unnamed namespace.)
#pragma once
#include <string>

#include "common.h"
#include "normal_map.h"

namespace drm {

namespace {

constexpr float kPi = 3.14159265358979323846f;
constexpr int kRenderWaves = 4;  // pixels (one wave each) per 256-thread workgroup

// (V3, v3, dot3 and unit_or_zero: normal_map.h)
__host__ __device__ __forceinline__ V3 axpy(float s, V3 a, V3 b) { return v3(s * a.x + b.x, s * a.y + b.y, s * a.z + b.z); }
// |a x b|^2: sin^2 of the angle between unit vectors without the cancellation of 1 - cos^2 near 0
__host__ __device__ __forceinline__ float cross_sq(V3 a, V3 b) {
  const float cx = a.y * b.z - a.z * b.y, cy = a.z * b.x - a.x * b.z, cz = a.x * b.y - a.y * b.x;
  return cx * cx + cy * cy + cz * cz;
}
__host__ __device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
// the barycentric mix (1 - u - v, u, v) of three vertex normals, not normalised: the shading normal of a point of a face, in object space
__host__ __device__ __forceinline__ V3 mix_normals(const float* n0, const float* n1, const float* n2, float u, float v) {
  const float w0 = 1.0f - u - v;
  return v3(w0 * n0[0] + u * n1[0] + v * n2[0], w0 * n0[1] + u * n1[1] + v * n2[1], w0 * n0[2] + u * n1[2] + v * n2[2]);
}
// The orthonormal frame (t, bt, n) of Duff et al. 2017 about a unit n, with its sign term: sg = 1 where n.z >= 0, else -1,
// a = -1 / (sg + n.z), b = n.x n.y a, t = (1 + sg n.x^2 a, sg b, -sg n.x), bt = (b, sg + n.y^2 a, -n.y).  A caller that knows n.z > 0 passes
// the literal 1.0f: every sg is then an exact factor of 1 that the compiler folds away.
struct Frame {
  V3 t, bt;
};
__host__ __device__ __forceinline__ Frame duff_frame(V3 n, float sg) {
  const float ka = -1.0f / (sg + n.z), kb = n.x * n.y * ka;
  return Frame{v3(1.0f + sg * n.x * n.x * ka, sg * kb, -sg * n.x), v3(kb, sg + n.y * n.y * ka, -n.y)};
}
// the cosine-weighted direction of the grid point (u1, u2) about n: cl n + sqrt(u1) (cos(2 pi u2) t + sin(2 pi u2) bt), cl = n.l = sqrt(1 - u1);
// sp, cp: sin and cos of 2 pi u2
__host__ __device__ __forceinline__ V3 cosine_direction(V3 n, const Frame& f, float u1, float sp, float cp, float& cl) {
  const float rs = sqrtf(u1);
  cl = sqrtf(1.0f - u1);
  return axpy(cl, n, axpy(rs * sp, f.bt, v3(rs * cp * f.t.x, rs * cp * f.t.y, rs * cp * f.t.z)));
}

// The sample sets of a normal seen from v = +z, for normal_lane_sum and table_lane_sum; every operation and its order is part of a render's bits.
// the point of index q of a Q x Q midpoint grid, (u1, u2) = ((q / Q + 1/2) / Q, (q % Q + 1/2) / Q), as (u1, sin 2 pi u2, cos 2 pi u2); invQ = 1 / Q
struct GridPoint {
  float u1, sp, cp;
};
__host__ __device__ __forceinline__ GridPoint grid_point(int q, int Q, float invQ) {
  const float u1 = ((float)(q / Q) + 0.5f) * invQ, u2 = ((float)(q % Q) + 0.5f) * invQ;
  return GridPoint{u1, sinf(2.0f * kPi * u2), cosf(2.0f * kPi * u2)};
}
// visible-normal sampling frame about (n, alpha): V = normalize(alpha v_t, alpha v_b, v_n), T1 = normalize(z x V) (x if V = z), T2 = V x T1
struct VisibleFrame {
  float Vx, Vy, Vz, T1x, T1y, T2x, T2y, T2z, vs;
};
__host__ __device__ __forceinline__ VisibleFrame visible_frame(V3 n, float alpha) {
  float Vx = -alpha * n.x, Vy = -alpha * n.y, Vz = n.z;
  const float vinv = 1.0f / sqrtf(Vx * Vx + Vy * Vy + Vz * Vz);
  Vx *= vinv; Vy *= vinv; Vz *= vinv;
  const float lensq = Vx * Vx + Vy * Vy;
  const float tinv = lensq > 0.0f ? 1.0f / sqrtf(lensq) : 0.0f;
  const float T1x = lensq > 0.0f ? -Vy * tinv : 1.0f, T1y = lensq > 0.0f ? Vx * tinv : 0.0f;
  return VisibleFrame{Vx, Vy, Vz, T1x, T1y, -Vz * T1y, Vz * T1x, Vx * T1y - Vy * T1x, 0.5f * (1.0f + Vz)};
}
// The GGX sample of a grid point: h from the distribution of visible normals (Heitz 2018) seen from v = +z, l = reflect(v, h); nh = n.h,
// s2h = 1 - nh^2 from the components (no cancellation), vh = v.h, cl = n.l.  f = duff_frame(n, 1).  The caller keeps it where vh > 0, cl > 0, D > 0.
struct GgxSample {
  V3 l;
  float nh, s2h, vh, cl;
};
__host__ __device__ __forceinline__ GgxSample ggx_sample(const VisibleFrame& vf, float alpha, V3 n, const Frame& f, const GridPoint& g) {
  const V3 v = v3(0.0f, 0.0f, 1.0f);
  const float rs = sqrtf(g.u1), t1 = rs * g.cp;
  const float t2 = (1.0f - vf.vs) * sqrtf(1.0f - t1 * t1) + vf.vs * rs * g.sp;
  const float tz = sqrtf(fmaxf(1.0f - t1 * t1 - t2 * t2, 0.0f));
  const float hx = alpha * (t1 * vf.T1x + t2 * vf.T2x + tz * vf.Vx), hy = alpha * (t1 * vf.T1y + t2 * vf.T2y + tz * vf.Vy);
  const float hz = fmaxf(t2 * vf.T2z + tz * vf.Vz, 0.0f);
  const float hinv = 1.0f / sqrtf(hx * hx + hy * hy + hz * hz);
  const float nh = hz * hinv, s2h = (hx * hx + hy * hy) * hinv * hinv;
  const V3 h = axpy(nh, n, axpy(hy * hinv, f.bt, v3(hx * hinv * f.t.x, hx * hinv * f.t.y, hx * hinv * f.t.z)));
  const float vh = dot3(v, h);
  const V3 l = axpy(2.0f * vh, h, v3(-v.x, -v.y, -v.z));
  return GgxSample{l, nh, s2h, vh, dot3(n, l)};
}
// p_s(l) = G1(v) D(h) / (4 n.v): the density of l = reflect(v, h) under the visible-normal sampling
__host__ __device__ __forceinline__ float visible_density(float g1v, float D, float cv) { return g1v * D / (4.0f * cv); }
// normalize(v + l) for v = +z, in the form (v + l) * (1 / |v + l|)
__host__ __device__ __forceinline__ V3 half_vector(V3 l) {
  const V3 h = v3(l.x, l.y, l.z + 1.0f);
  const float hinv = 1.0f / sqrtf(dot3(h, h));
  return v3(h.x * hinv, h.y * hinv, h.z * hinv);
}

// canonical row (metallic, base colour R G B, roughness, specular), clipped to [0, 1] as get_bsdf / _render_scene clip
struct Principled {
  float m, c[3], r, alpha, a2, eta;
};
__host__ __device__ __forceinline__ Principled principled(const float* z) {
  Principled p;
  p.m = clip01(z[0]);
  p.c[0] = clip01(z[1]);
  p.c[1] = clip01(z[2]);
  p.c[2] = clip01(z[3]);
  p.r = clip01(z[4]);
  p.alpha = fmaxf(0.001f, p.r * p.r);
  p.a2 = p.alpha * p.alpha;
  p.eta = 2.0f / (1.0f - sqrtf(0.08f * clip01(z[5]))) - 1.0f;  // Mitsuba's specular -> eta; >= 1, so no total internal reflection
  return p;
}

// The BSDF terms are templates: the quadrature runs them in fp32; drm_brdf_eval runs them in fp64, since near a narrow peak (alpha down
// to 0.001) the value is ill-conditioned in the half vector: fp32 rounding of h alone would move D by more than 1e-5.
// GGX D with 1 - (n.h)^2 passed as s2 = |n x h|^2; 0 where D (n.h) <= 1e-20 (Mitsuba's cut-off)
template <typename T>
__host__ __device__ __forceinline__ T ggx_d(T a2, T nh, T s2) {
  const T t = s2 + a2 * nh * nh;
  const T d = a2 / (T(kPi) * t * t);
  return d * nh > T(1e-20) ? d : T(0);
}
// Smith G1 of GGX for a direction w: c = n.w, s2 = |n x w|^2, wh = w.h; 0 on the back of the microfacet, 1 at normal incidence
template <typename T>
__host__ __device__ __forceinline__ T ggx_g1(T a2, T c, T s2, T wh) {
  if (wh * c <= T(0)) return T(0);
  if (s2 == T(0)) return T(1);
  return T(2) / (T(1) + sqrt(T(1) + a2 * s2 / (c * c)));
}
// exact unpolarised dielectric Fresnel at cos cd, relative index eta >= 1 (0 when index-matched)
template <typename T>
__host__ __device__ __forceinline__ T fresnel_dielectric(T cd, T eta) {
  if (eta == T(1)) return T(0);
  const T ct = sqrt(fmax(T(1) - (T(1) - cd * cd) / (eta * eta), T(0)));
  const T as = (cd - eta * ct) / (cd + eta * ct);
  const T ap = (ct - eta * cd) / (ct + eta * cd);
  return T(0.5) * (as * as + ap * ap);
}
template <typename T>
__host__ __device__ __forceinline__ T schlick_weight(T c) {
  const T t = fmin(fmax(T(1) - c, T(0)), T(1));
  const T t2 = t * t;
  return t2 * t2 * t;
}
// Disney diffuse term without c / pi: (1 - F_l / 2)(1 - F_v / 2) + R_r (F_l + F_v + F_l F_v (R_r - 1)), R_r = 2 r cd^2
template <typename T>
__host__ __device__ __forceinline__ T diffuse_shape(T r, T cl, T cv, T cd) {
  const T fl = schlick_weight(cl), fv = schlick_weight(cv), rr = T(2) * r * cd * cd;
  return (T(1) - T(0.5) * fl) * (T(1) - T(0.5) * fv) + rr * (fl + fv + fl * fv * (rr - T(1)));
}

// Mitsuba's eval (f times n.l) per channel, in fp64; n, v (toward the viewer), l (toward the light) unit vectors, given as fp32
// (drm_brdf_eval) or as fp64 (drm_brdf_to_merl, whose grid directions are formed in fp64): S
// in two halves, so that a kernel that scores many rows on one direction triple (brdf_error.hip) forms the first half once: EvalGeom, the
// cosines of the triple, which no row enters, and principled_eval_at, the terms a row enters.  principled_eval is the two in sequence.
struct EvalGeom {
  double cv, cl, nh, cd, lh;  // n.v, n.l, n.h, h.v, h.l at h = normalize(v + l); nh, cd, lh are set only where cv > 0 and cl > 0
};
template <typename S>
__host__ __device__ __forceinline__ EvalGeom eval_geom(const S* n, const S* v, const S* l) {
  EvalGeom g;
  const double nx = n[0], ny = n[1], nz = n[2];
  g.cv = nx * v[0] + ny * v[1] + nz * v[2];
  g.cl = nx * l[0] + ny * l[1] + nz * l[2];
  g.nh = g.cd = g.lh = 0.0;
  if (!(g.cv > 0.0 && g.cl > 0.0)) return g;
  double hx = (double)v[0] + l[0], hy = (double)v[1] + l[1], hz = (double)v[2] + l[2];
  const double inv = 1.0 / sqrt(hx * hx + hy * hy + hz * hz);
  hx *= inv; hy *= inv; hz *= inv;
  g.nh = nx * hx + ny * hy + nz * hz;  // > 0: v and l are both above the surface
  g.cd = hx * v[0] + hy * v[1] + hz * v[2];
  g.lh = hx * l[0] + hy * l[1] + hz * l[2];
  return g;
}
__host__ __device__ __forceinline__ void principled_eval_at(const Principled& p, const EvalGeom& g, float out[3]) {
  out[0] = out[1] = out[2] = 0.0f;
  const double cv = g.cv, cl = g.cl, nh = g.nh, cd = g.cd, lh = g.lh;
  if (!(cv > 0.0 && cl > 0.0)) return;
  const double a2 = (double)p.alpha * p.alpha, m = p.m;
  // sin^2 as 1 - cos^2 (in fp64 the cancellation costs nothing, and this is the definition's form for inputs that are unit only to fp32)
  const double D = ggx_d(a2, nh, 1.0 - nh * nh);
  const double G = ggx_g1(a2, cv, 1.0 - cv * cv, cd) * ggx_g1(a2, cl, 1.0 - cl * cl, lh);
  const double k = D * G / (4.0 * cv);
  const double fd = (1.0 - m) * fresnel_dielectric(cd, (double)p.eta), sw = schlick_weight(cd);
  const double kd = (1.0 - m) * cl * diffuse_shape((double)p.r, cl, cv, cd) / kPi;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = (float)((fd + m * (p.c[ch] + (1.0 - p.c[ch]) * sw)) * k + kd * p.c[ch]);
}
template <typename S>
__host__ __device__ __forceinline__ void principled_eval(const Principled& p, const S* n, const S* v, const S* l, float out[3]) {
  principled_eval_at(p, eval_geom(n, v, l), out);
}

// principled_eval's expression in fp32 on the same terms, sin^2 passed as |n x .|^2 as the quadrature passes it: what a surface point reflects
// inside the bounce of Bounced, where a value accurate to fp32 is all the sum around it can use
__host__ __device__ __forceinline__ void principled_eval32(const Principled& p, V3 n, V3 v, V3 l, float out[3]) {
  out[0] = out[1] = out[2] = 0.0f;
  const float cv = dot3(n, v), cl = dot3(n, l);
  if (!(cv > 0.0f && cl > 0.0f)) return;
  V3 h = v3(v.x + l.x, v.y + l.y, v.z + l.z);
  const float inv = 1.0f / sqrtf(dot3(h, h));
  h = v3(h.x * inv, h.y * inv, h.z * inv);
  const float nh = dot3(n, h), cd = dot3(h, v), lh = dot3(h, l);
  const float D = ggx_d(p.a2, nh, cross_sq(n, h));
  const float G = ggx_g1(p.a2, cv, cross_sq(n, v), cd) * ggx_g1(p.a2, cl, cross_sq(n, l), lh);
  const float k = D * G / (4.0f * cv);
  const float fd = (1.0f - p.m) * fresnel_dielectric(cd, p.eta), sw = schlick_weight(cd);
  const float kd = (1.0f - p.m) * cl * diffuse_shape(p.r, cl, cv, cd) / kPi;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = (fd + p.m * (p.c[ch] + (1.0f - p.c[ch]) * sw)) * k + kd * p.c[ch];
}

// radiance toward w: bilinear in the texel grid of an EH x EW map whose texel (i, j) looks along theta = (i + 1/2) pi / EH,
// psi = (j + 1/2) 2 pi / EW, w = (sin theta sin psi, cos theta, -sin theta cos psi); wraps in psi, clamps in theta.  env [EH][EW][3].
// EnvTaps: the four texels (rows r0 / r1 = texel rows i0 / i0 + 1 clamped, columns j0 / j1) and the fractions of that lookup; pole: w lies
// in a polar half row, where theta is clamped and fy = 0.
struct EnvTaps {
  const float *r0, *r1;
  int j0, j1, i0;
  float fx, fy;
  bool pole;
};
__host__ __device__ __forceinline__ EnvTaps env_taps(const float* __restrict__ env, int EH, int EW, V3 w) {
  const float u = atan2f(w.x, -w.z) * (0.5f / kPi);
  const float t = acosf(fminf(fmaxf(w.y, -1.0f), 1.0f)) * (1.0f / kPi);
  const float x = u * (float)EW - 0.5f;
  const float yu = t * (float)EH - 0.5f;
  const float y = fminf(fmaxf(yu, 0.0f), (float)(EH - 1));
  const float xf = floorf(x), yf = floorf(y);
  int j0 = (int)xf % EW;
  if (j0 < 0) j0 += EW;
  const int j1 = j0 + 1 == EW ? 0 : j0 + 1;
  const int i0 = (int)yf, i1 = i0 + 1 < EH ? i0 + 1 : EH - 1;
  return EnvTaps{env + (size_t)i0 * EW * 3, env + (size_t)i1 * EW * 3, j0, j1, i0, x - xf, y - yf, yu < 0.0f || yu >= (float)(EH - 1)};
}
// the bilinear form over the taps' four corner values v{row}{column}
__host__ __device__ __forceinline__ float bilerp(const EnvTaps& e, float v00, float v01, float v10, float v11) {
  const float top = (1.0f - e.fx) * v00 + e.fx * v01;
  const float bot = (1.0f - e.fx) * v10 + e.fx * v11;
  return (1.0f - e.fy) * top + e.fy * bot;
}
__host__ __device__ __forceinline__ void bilerp(const EnvTaps& e, float L[3]) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) L[ch] = bilerp(e, e.r0[e.j0 * 3 + ch], e.r0[e.j1 * 3 + ch], e.r1[e.j0 * 3 + ch], e.r1[e.j1 * 3 + ch]);
}
__host__ __device__ __forceinline__ void env_lookup(const float* __restrict__ env, int EH, int EW, V3 w, float L[3]) {
  bilerp(env_taps(env, EH, EW, w), L);
}

// RefMapSensor: the normal seen at film position (px, py) in [0, 1]^2 (from the left / from the top); flip mirrors x
__host__ __device__ __forceinline__ V3 sensor_normal(float px, float py, int flip) {
  const float a = (2.0f * px - 1.0f) * (0.5f * kPi), b = (1.0f - 2.0f * py) * (0.5f * kPi);
  const float cb = cosf(b);
  const float nx = cb * sinf(a);
  return v3(flip ? -nx : nx, sinf(b), cb * cosf(a));
}

// the view rotation of one row: directions of the quadrature live in the frame whose viewer is +z; the environment is read at Rot l
// (row-major Rot).  on == false: the view from +z, l is used as it is (not multiplied by the identity: 0 * l.y + ... would turn -0 into +0
// in front of atan2f, and the +z renders must not move).  The kernel is compiled with and without the view (VIEW): a launch without view
// matrices runs the instantiation that holds no rotation at all, at the register count (and occupancy) the +z renderer always had.
struct ViewRot {
  float m[9];
  bool on;
};
__host__ __device__ __forceinline__ ViewRot view_rot(const float* view) {
  ViewRot r;
  r.on = false;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    r.m[k] = view ? view[k] : (k % 4 == 0 ? 1.0f : 0.0f);
    r.on = r.on || r.m[k] != (k % 4 == 0 ? 1.0f : 0.0f);
  }
  return r;
}
template <bool VIEW>
__host__ __device__ __forceinline__ V3 to_world(const ViewRot& r, V3 l) {
  if (!VIEW || !r.on) return l;
  return v3(r.m[0] * l.x + r.m[1] * l.y + r.m[2] * l.z, r.m[3] * l.x + r.m[4] * l.y + r.m[5] * l.z, r.m[6] * l.x + r.m[7] * l.y + r.m[8] * l.z);
}

// Rot^T w: a world direction (a light sample) in the row's frame
template <bool VIEW>
__host__ __device__ __forceinline__ V3 from_world(const ViewRot& r, V3 w) {
  if (!VIEW || !r.on) return w;
  return v3(r.m[0] * w.x + r.m[3] * w.y + r.m[6] * w.z, r.m[1] * w.x + r.m[4] * w.y + r.m[7] * w.z, r.m[2] * w.x + r.m[5] * w.y + r.m[8] * w.z);
}

// the fixed butterfly in which the 64 lanes' partial sums meet: every lane ends with the wave's sum
__device__ __forceinline__ void wave_sum3(float a[3]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] += __shfl_xor(a[c], o);
  }
}

// ------------------------------------------------------------------------------------------------ pixel kernels
// The two pixel kernels, stated once for every material.  One wave owns one pixel: its lanes split the Q x Q grid, keep their partial sums in
// a fixed order and meet in wave_sum3.  MAT is what a row is and how one lane shades one normal under it (RowMaterial in render.hip: a
// principled row with Plain or LightSampled; TableMaterial in brdf_table.hip): MAT::Args, its launch arguments, one small struct passed by
// value; MAT(args, row, b, EH, Q), the material of row `row` lit by map b; lane_sum<VIEW>(...), one lane's share of normal n summed into acc
// (unnormalised); meet(), the butterfly of what it summed beside acc, if anything; joined(c, px, inv_s2), channel c of the pixel with that
// sum joined to px = acc[c] / (S^2 Q^2).  Every difference between materials is a type: no kernel holds state or a branch of another's.

// The sphere.  grid: ceil(rows R^2 / 4) workgroups of 4 waves; wave = pixel (row, i, j), row = l B + b lit by env[b], seen through view[b];
// out [rows][3][R][R].  Every row runs the same per-lane order whatever L is: a stacked render (rows = L B) equals its rows rendered alone.
template <bool VIEW, typename MAT>
__global__ __launch_bounds__(256) void sphere_pixel_kernel(typename MAT::Args margs, const float* __restrict__ env, const float* __restrict__ view,
                                                           float* __restrict__ out, int rows, int B, int R, int EH, int EW, int Q, int S, int flip) {
  const long long pix = (long long)blockIdx.x * kRenderWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pix >= (long long)rows * R * R) return;  // (wave-uniform)
  // (a wave is one pixel: the map and the view matrix are fetched through scalar loads.  A material without stacks, rows = B, has row = b:
  // it pays for no modulo and its row is wave-uniform too, as in the kernel it had of its own)
  const int at = (int)(pix / ((long long)R * R));
  const int row = MAT::kStacked ? at : __builtin_amdgcn_readfirstlane(at);
  const int b = MAT::kStacked ? __builtin_amdgcn_readfirstlane(at % B) : row;
  const int rem = (int)(pix - (long long)row * R * R);
  const int i = rem / R, j = rem - (rem / R) * R;
  MAT mat(margs, row, b, EH, Q);
  const float* e = env ? env + (size_t)b * EH * EW * 3 : nullptr;
  const ViewRot rot = view_rot(VIEW ? view + 9 * (size_t)b : nullptr);
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (int sy = 0; sy < S; ++sy) {
    for (int sx = 0; sx < S; ++sx) {
      const V3 n = sensor_normal(((float)j + ((float)sx + 0.5f) / (float)S) / (float)R, ((float)i + ((float)sy + 0.5f) / (float)S) / (float)R, flip);
      mat.template lane_sum<VIEW>(e, rot, EH, EW, n, Q, lane, 64, acc);
    }
  }
  wave_sum3(acc);
  mat.meet();
  if (lane == 0) {
    const float scale = 1.0f / ((float)(S * S) * (float)(Q * Q));
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(((size_t)row * 3 + c) * R + i) * R + j] = mat.joined(c, acc[c] * scale, 1.0f / (float)(S * S));
  }
}

// A normal map (no mesh behind it).  grid: ceil(B H W / 4) workgroups of 4 waves; wave = pixel (row b, i, j), lit by env[b]; view[b] turns
// the environment lookups only (the normals are in the view frame).  The wave reads the normal of map (Bn == 1 ? 0 : b) through one address
// (normal_map_pixel) and, where the pixel is drawn, runs lane_sum once: the sphere's pixel with S = 1.  Not drawn: image 0, alpha 0 (wave-uniform).
template <bool VIEW, typename MAT>
__global__ __launch_bounds__(256) void normals_pixel_kernel(typename MAT::Args margs, const float* __restrict__ normals, const unsigned char* __restrict__ mask,
                                                            int Bn, const float* __restrict__ env, const float* __restrict__ view, float* __restrict__ image,
                                                            float* __restrict__ alpha, int B, int H, int W, int EH, int EW, int Q) {
  const long long pix = (long long)blockIdx.x * kRenderWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pix >= (long long)B * H * W) return;  // (wave-uniform)
  const size_t plane = (size_t)H * W;
  const int b = __builtin_amdgcn_readfirstlane((int)(pix / ((long long)H * W)));
  const size_t at = (size_t)(pix - (long long)b * H * W);
  V3 n = v3(0.0f, 0.0f, 0.0f);
  const bool drawn = normal_map_pixel(normals, mask, (Bn == 1 ? 0 : (size_t)b * plane) + at, n);  // (wave-uniform: every lane read the same pixel)
  float acc[3] = {0.0f, 0.0f, 0.0f};
  MAT mat(margs, b, b, EH, Q);  // (ahead of the drawn test: what the material reads is under way while the normal is)
  if (drawn) {
    const float* e = env ? env + (size_t)b * EH * EW * 3 : nullptr;
    const ViewRot rot = view_rot(VIEW ? view + 9 * (size_t)b : nullptr);
    mat.template lane_sum<VIEW>(e, rot, EH, EW, n, Q, lane, 64, acc);
    wave_sum3(acc);
    mat.meet();
  }
  if (lane == 0) {
    const float scale = 1.0f / (float)(Q * Q);
#pragma unroll
    for (int c = 0; c < 3; ++c) image[((size_t)b * 3 + c) * plane + at] = drawn ? mat.joined(c, acc[c] * scale, 1.0f) : 0.0f;
    if (alpha) alpha[(size_t)b * plane + at] = drawn ? 1.0f : 0.0f;
  }
}

}  // namespace

// What every render checks of its drm_shading (render.hip) before anything is launched: the struct's size, exactly one material, the
// quadrature (subpixel_max = 0: the caller bounds subpixel itself), the map sizes and light_samples.  `who` names the entry in the messages.
// *lit: light samples are in play (light_samples > 0 under a map); light_fault: what is wrong with their workspace, empty where nothing is
// -- handed back, since each surface reports it with its own code.
int check_shading(const std::string& who, const drm_shading& sh, int subpixel, int subpixel_max, bool* lit, std::string* light_fault);
// the grid of a pixel kernel: one wave per pixel, kRenderWaves to a workgroup
static inline long long pixel_blocks(long long pixels) { return (pixels + kRenderWaves - 1) / kRenderWaves; }

// What the launches of a pixel kernel share whatever the material: the grid, and the environment as the kernel sees it (a view only turns
// it, so under a white one, nominally 1 x 1, view is null and the kernel the one without it).  `size` names the pixel count in the message.
struct PixelLaunch {
  unsigned blocks;
  const float* view;
  int EH, EW;
};
static inline int plan_pixel_launch(const std::string& who, const char* size, long long pixels, const float* env, const float* view, int EH, int EW,
                                    PixelLaunch& pl) {
  const long long blocks = pixel_blocks(pixels);
  DRM_REQUIRE(blocks <= 0x7fffffffLL, who + ": " + size + " too large for one launch");
  pl = PixelLaunch{(unsigned)blocks, env ? view : nullptr, env ? EH : 1, env ? EW : 1};
  return DRM_OK;
}
// The launches under tables (brdf_table.hip, next to the material they instantiate), after the checks every material shares: check_tables,
// then sphere_pixel_kernel / normals_pixel_kernel on the planned grid.
int launch_refmap_tables(const drm_shading& sh, const PixelLaunch& pl, int R, int subpixel, int flip, float* out, hipStream_t s);
int launch_normals_tables(const drm_shading& sh, const PixelLaunch& pl, const float* normals, const unsigned char* mask, int Bn, int H, int W, float* image,
                          float* alpha, hipStream_t s);

}  // namespace drm
