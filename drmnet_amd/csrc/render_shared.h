// What the per-normal sums of render.hip (normal_lane_sum: a principled row) and brdf_table.hip (table_lane_sum: a measured table) share:
// the three-vector helpers, the frame about a normal and the cosine-weighted direction, the principled row with its GGX, Fresnel and diffuse
// terms and their eval, the environment lookup (env_taps + bilerp), the sensor's normals, the view rotation, the wave butterfly, and the
// checks and grid of a pixel kernel's launch.  Everything device-side sits in an unnamed namespace, as it did inside render.hip: every
// translation unit gets its own copy, and render.hip's kernels compile to the instructions they had.
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
template <typename S>
__host__ __device__ __forceinline__ void principled_eval(const Principled& p, const S* n, const S* v, const S* l, float out[3]) {
  out[0] = out[1] = out[2] = 0.0f;
  const double nx = n[0], ny = n[1], nz = n[2];
  const double cv = nx * v[0] + ny * v[1] + nz * v[2], cl = nx * l[0] + ny * l[1] + nz * l[2];
  if (!(cv > 0.0 && cl > 0.0)) return;
  double hx = (double)v[0] + l[0], hy = (double)v[1] + l[1], hz = (double)v[2] + l[2];
  const double inv = 1.0 / sqrt(hx * hx + hy * hy + hz * hz);
  hx *= inv; hy *= inv; hz *= inv;
  const double nh = nx * hx + ny * hy + nz * hz;  // > 0: v and l are both above the surface
  const double cd = hx * v[0] + hy * v[1] + hz * v[2], lh = hx * l[0] + hy * l[1] + hz * l[2];
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

}  // namespace

// What every launch of a pixel kernel checks of its quadrature and environment (`who` names the entry in the message; subpixel_max = 0: the
// caller bounds subpixel itself), and its grid: one wave per pixel, kRenderWaves to a workgroup.
static inline int check_quadrature(const std::string& who, int quad, int subpixel, int subpixel_max, const float* env, int EH, int EW) {
  DRM_REQUIRE(quad >= 1 && quad <= 1024 && (!subpixel_max || (subpixel >= 1 && subpixel <= subpixel_max)),
              who + ": quad in [1, 1024]" + (subpixel_max ? ", subpixel in [1, " + std::to_string(subpixel_max) + "]" : ""));
  DRM_REQUIRE(!env || (EH > 0 && EW > 0 && (long long)EH * EW <= (1LL << 28)), who + ": envmap must be EH x EW with EH, EW >= 1");
  return DRM_OK;
}
static inline long long pixel_blocks(long long pixels) { return (pixels + kRenderWaves - 1) / kRenderWaves; }

}  // namespace drm
