// The forward model DRMNet inverts: a reflectance map of one sphere lit only by a lat-long environment map, seen through the principled
// BSDF subset of the shipped configs, under a direct-lighting integral.  Replaces the reference's Mitsuba 3 renders on the inference side
// (paths relative to the reference root):
//   RefMapSensor (camera at +z, up +y, orthographic over the sphere)   utils/mitsuba3_utils.py:14-89
//   MitsubaRefMapRenderer.rendering (sphere + envmap, "direct")        utils/mitsuba3_utils.py:324-430
//   get_bsdf / eval_bsdf / visualize_bsdf ("principled")             utils/mitsuba3_utils.py:528-640
//   DRMNet.instantiate_brdf_model (basis_r0), reconstruct            models/drmnet.py:328-347, 943-953
// The BSDF is Mitsuba 3's principled with spec_tint, sheen, clearcoat, anisotropic, spec_trans and flatness at 0: a GGX specular lobe with
// Smith G and the exact dielectric / Schlick metallic Fresnel mix, plus the retro-reflective Disney diffuse.  A pixel is the box-filtered
// mean over its footprint of P(n) = integral over {l : n.l > 0} of L(l) f(v, l) (n.l) dl, with v = +z and n the sphere normal the sensor
// sees.  The integral is a deterministic stratified quadrature per lobe: a Q x Q midpoint grid of (u1, u2) mapped to the GGX visible
// normals seen from v (Heitz 2018: weight F G1(l), bounded, so the heavy GGX tail needs no extra strata) for the specular lobe and to
// cosine-weighted directions for the diffuse one, at S x S sub-pixel normals.  One wave
// owns one pixel: its lanes split the Q^2 grid, keep their partial sums in a fixed order and meet in a fixed butterfly, so a render is
// bitwise reproducible (no atomics).
//
// Light sampling (opt-in, light_samples = M > 0): the quadrature never consults the map when it places samples, so a light a few texels
// wide can fall between the strata of a rough lobe.  light_samples > 0 adds a third technique, M directions drawn from the map's own
// light density, and combines the three with lobe-separated multiple importance sampling (power heuristic, beta = 2): see "light density"
// below.
//
// Object images of meshes (drm_render_mesh): mesh.hip finds which face every film sample sees; mesh_shade_kernel here shades the hit with
// normal_lane_sum, the per-normal body of the sphere's sum, so a mesh point is shaded exactly as the sphere point with the same normal
// (direct light, no interreflection).  shadows runs mesh_shade_kernel<VIEW, true, false>, which traces every quadrature
// direction from the hit point through the mesh's BVH (bvh.h) and drops the occluded ones.  light_samples > 0 runs
// mesh_shade_kernel<VIEW, SHADOW, true>: the light samples of the sphere's lit render on the mesh, each traced like a lobe direction where
// there is a BVH.  bounces = 1 runs mesh_shade_kernel<VIEW, true, false, true>: an occluded direction reads the radiance its
// closest hit reflects back under direct light (one bounce; see Bounced).
//
// Object images of a normal map (drm_render_normals): normals_pixel_kernel (render_shared.h) with Plain, or normals_lit_kernel with
// LightSampled, runs the same per-normal body on the normals of a normal map, the input estimate's user has: no mesh, no shadows.
//
// One statement of the quadrature: normal_lane_sum builds both lobes once and accumulates each in one place; what differs between the
// renders is its technique parameter (Plain, LightSampled, Occluded, LitOccluded, Bounced: see "techniques"), which decides per lobe sample whether
// it counts, what radiance it reads and what scales its weight.  Every texel fetch is env_taps + bilerp.  Plain holds nothing: the
// instantiations without light samples and without shadows carry no code and no registers of the others.
//
// Also stated once: the traced techniques ask the mesh through one Tracer (mesh_shade.h, shared with the mesh under a table,
// mesh_table.hip, as are the shadowed kernels' launch arguments and the host's mesh checks), the only place that builds a Ray; the shading normal
// (mix_normals, unit_or_zero), the frame about a normal (duff_frame) and the cosine-weighted direction (cosine_direction) serve the film's
// hit and the bounce's; mesh_technique builds the technique of a mesh pixel; on the host every render checks its drm_shading through
// check_shading, every mesh render is launch_render_mesh, and the lit renders share launch_light_tables.
//
// Shared with the renders under a measured table (brdf_table.hip), in render_shared.h: the vector, frame, BSDF-term, environment-lookup,
// sensor, view and butterfly helpers; the sample sets (grid_point, visible_frame, ggx_sample, visible_density, half_vector), so that
// normal_lane_sum holds only the lobe weights and the technique calls; the two pixel kernels, instantiated here with RowMaterial; their checks.
#include <type_traits>

#include "bvh.h"
#include "common.h"
#include "mesh_shade.h"
#include "normal_map.h"
#include "render_shared.h"

namespace drm {

namespace {

// ------------------------------------------------------------------------------------------------ light density
// The density lives on the dual grid of the bilinear lookup, where env_lookup is exactly bilinear.  Cell (c, j), c = 0 .. EH, j = 0 .. EW - 1,
// spans theta in [lo_c, hi_c] = [(c - 1/2), (c + 1/2)] pi / EH clipped to [0, pi] (the polar rows are half cells) and psi in
// [(j + 1/2), (j + 3/2)] dpsi, dpsi = 2 pi / EW (wrapping); its corners are the texels (clamp(c - 1), clamp(c)) x (j, j + 1 mod EW), each
// valued at its Rec. 709 luminance clamped at 0.  With respect to (theta, psi) the density inside a cell is val sc_c / (tot dpsi): val the
// bilinear interpolant of the corner luminances, sc_c = sin((lo_c + hi_c) / 2), tot = sum over cells of mean4(corners) sc_c (hi_c - lo_c).
// The solid-angle pdf is p_L(w) = density / max(sin theta, 1e-6): any direction's pdf follows from the four texels its lookup loads and
// norm = 1 / (tot dpsi); there is no pdf image.
//
// Workspace of one map (light_ws_stride bytes): fp64 cdf[EH + 2] (cdf[0] = 0, cdf[EH + 1] = tot), rowsum[EH + 1] (sum over j of mean4),
// mass[EH + 1] (rowsum sc (hi - lo)); fp32 norm (0: the map has no light: black, or all non-positive) and a pad; the sample table, seven
// planes of M floats (direction x y z, radiance r g b, p_L: 28 bytes a sample, laid out so a wave's loads are contiguous).
struct LightTable {
  const float* tab;
  int M;
  float norm;
};
__host__ __device__ __forceinline__ size_t light_ws_doubles(int EH) { return 3 * (size_t)EH + 4; }
__host__ __device__ __forceinline__ size_t light_ws_stride(int EH, int M) { return light_ws_doubles(EH) * 8 + 8 + 28 * (size_t)M; }
__host__ __device__ __forceinline__ LightTable light_table(const char* ws, int b, int EH, int M) {
  const char* base = ws + (size_t)b * light_ws_stride(EH, M) + light_ws_doubles(EH) * 8;
  LightTable lt;
  lt.norm = *reinterpret_cast<const float*>(base);
  lt.tab = reinterpret_cast<const float*>(base + 8);
  lt.M = M;
  return lt;
}

// a^2 / (a^2 + b^2) for a > 0 (the lobe pdfs are positive wherever a lobe sample is kept)
__host__ __device__ __forceinline__ float power_weight(float a, float b) { return (a * a) / (a * a + b * b); }
__host__ __device__ __forceinline__ float luma(const float* t) { return fmaxf(0.2126f * t[0] + 0.7152f * t[1] + 0.0722f * t[2], 0.0f); }

// env_lookup that also returns p_L(w) from the four texels it loads.  sc_pole = sin(pi / (4 EH)).
__host__ __device__ __forceinline__ float env_lookup_pdf(const float* __restrict__ env, int EH, int EW, V3 w, float norm, float sc_pole, float L[3]) {
  const EnvTaps e = env_taps(env, EH, EW, w);
  bilerp(e, L);
  // cell row: c = floor(yu) + 1 clamped to [0, EH]; in the half cells y is clamped, fy = 0 and the value is the polar texel row's
  const float sc = e.pole ? sc_pole : sinf((float)(e.i0 + 1) * (kPi / (float)EH));
  const float val = bilerp(e, luma(e.r0 + e.j0 * 3), luma(e.r0 + e.j1 * 3), luma(e.r1 + e.j0 * 3), luma(e.r1 + e.j1 * 3));
  return val * sc * norm / fmaxf(sqrtf(w.x * w.x + w.z * w.z), 1e-6f);
}

// ------------------------------------------------------------------------------------------------ techniques
// What normal_lane_sum does with one lobe sample is the technique's: take() gets the sample's world direction wl (any length) and np, the
// lobe's sample count times its density at wl (formed only for kNeedsDensity), and returns whether the sample counts at all; if so it has
// read the radiance into L (left as it is under a white environment) and scaled the weight w.  begin() opens a normal, finish() closes it.
struct Plain {
  static constexpr bool kNeedsDensity = false;
  __host__ __device__ __forceinline__ void begin(const Principled&, V3) {}
  __host__ __device__ __forceinline__ bool take(const float* __restrict__ env, int EH, int EW, V3 wl, float, float&, float L[3]) const {
    if (env) env_lookup(env, EH, EW, wl, L);
    return true;
  }
  template <bool VIEW>
  __host__ __device__ __forceinline__ void finish(const Principled&, const ViewRot&, V3, int, int) {}
};

// (Tracer, through which the traced techniques ask the mesh: mesh_shade.h)
// The shadowed mesh: a direction the BVH finds cut off between the sample's hit point and the environment is dropped before any lookup.
struct Occluded : Plain {
  Tracer trace;
  __host__ __device__ __forceinline__ bool take(const float* __restrict__ env, int EH, int EW, V3 wl, float np, float& w, float L[3]) const {
    return !trace.occluded(wl) && Plain::take(env, EH, EW, wl, np, w, L);
  }
};

// One bounce of interreflection on the shadowed mesh: a direction wl that Occluded would drop reads, instead of the map, the radiance L_b
// its closest hit y = o + t wl on face g' reflects toward -wl under direct light.  With n_y the normalised barycentric mix of the vertex
// normals of g' in object space (zero or NaN: L_b = 0), w_o = -wl / |wl| (n_y.w_o <= 0: L_b = 0) and duff_frame(n_y, sign of n_y.z), valid
// for every unit n:
//   L_b = (pi / K) sum_k V_k L(w_k) E(n_y, w_o, w_k) / cos_k,  K = bounce_quad^2,
// w_k = cosine_direction of the midpoint grid (u1, u2) = ((k / bq + 1/2) / bq, (k % bq + 1/2) / bq), the diffuse lobe's mapping,
// cos_k = sqrt(1 - u1); E = principled_eval32 (the BSDF value times cosine);
// V_k = 0 iff the ray (y, w_k) excluding g' is occluded (any-hit); L the map's bilinear radiance along w_k, an object-space direction being
// the world direction as for lobe rays, 1 under a white environment.  A direction with E = 0 is neither traced nor looked up.  Each lane
// runs the K directions of its own bounce serially, in k order.  An open direction is Plain::take: unchanged to the bit.  The weight w is
// not touched.  One traversal serves both questions: a ray is occluded iff it has a closest hit (the same candidates).
struct Bounced : Plain {
  Tracer trace;
  const float* vnormal;  // [V][3] vertex normals, object space
  Principled p;          // the row's BSDF, which the hit reflects with as well
  int bq;                // bounce_quad
  __host__ __device__ __forceinline__ void reflected(const float* __restrict__ env, int EH, int EW, V3 wl, const Hit& h, float L[3]) const {
    L[0] = L[1] = L[2] = 0.0f;
    const int32_t* idx = trace.mesh.faces + 3 * (size_t)h.face;  // (a candidate's indices are in [0, V))
    const V3 n = unit_or_zero(mix_normals(vnormal + 3 * (size_t)idx[0], vnormal + 3 * (size_t)idx[1], vnormal + 3 * (size_t)idx[2], h.u, h.v));
    const float dinv = 1.0f / sqrtf(dot3(wl, wl));
    const V3 wo = v3(-wl.x * dinv, -wl.y * dinv, -wl.z * dinv);
    if (!(dot3(n, wo) > 0.0f)) return;  // (a zero normal leaves here as well)
    const Tracer inner{trace.mesh, trace.tree, {trace.o[0] + h.t * wl.x, trace.o[1] + h.t * wl.y, trace.o[2] + h.t * wl.z}, h.face};
    const Frame f = duff_frame(n, n.z >= 0.0f ? 1.0f : -1.0f);
    const float invq = 1.0f / (float)bq;
    for (int k = 0; k < bq * bq; ++k) {
      const GridPoint g = grid_point(k, bq, invq);
      float ck;
      const V3 l = cosine_direction(n, f, g.u1, g.sp, g.cp, ck);
      float E[3];
      principled_eval32(p, n, wo, l, E);
      if (E[0] == 0.0f && E[1] == 0.0f && E[2] == 0.0f) continue;
      if (inner.occluded(l)) continue;
      float Lk[3] = {1.0f, 1.0f, 1.0f};
      if (env) env_lookup(env, EH, EW, l, Lk);
#pragma unroll
      for (int c = 0; c < 3; ++c) L[c] += Lk[c] * E[c] / ck;
    }
    const float scale = kPi / (float)(bq * bq);
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] *= scale;
  }
  __host__ __device__ __forceinline__ bool take(const float* __restrict__ env, int EH, int EW, V3 wl, float np, float& w, float L[3]) const {
    const Hit h = trace.closest(wl);
    if (h.face < 0) {
      // (normal_lane_sum keeps one L for both lobes of a grid point and Plain::take leaves it alone under a white environment: the specular
      // lobe's bounce must not reach an open diffuse direction)
      if (!env) L[0] = L[1] = L[2] = 1.0f;
      return Plain::take(env, EH, EW, wl, np, w, L);
    }
    reflected(env, EH, EW, wl, h, L);
    return true;
  }
};

// The light technique: where the map has light (lt.norm > 0) every lobe sample is weighted by the power heuristic against the
// n_L = lt.M light samples, and finish() lets the lanes stride the light table as they strode the grid, summing into accL (to be
// normalised by 1 / S^2 only: the weights hold 1 / n).  Needs a map: env is never null here.  The table loop is table_sum, written once for
// this technique and for LitOccluded: it asks open() about a table direction after the cheap rejections (n.l > 0, p_L > 0); here
// every direction is open and the question compiles to nothing.
struct LightSampled {
  static constexpr bool kNeedsDensity = true;
  LightTable lt;
  float accL[3];
  float nlobe, nlight, sc_pole, g1v;
  bool lit;
  // G1(v): v = +z is above the surface on the whole film and v.h > 0 wherever it is used
  __host__ __device__ __forceinline__ void begin(const Principled& p, V3 n) { g1v = ggx_g1(p.a2, n.z, n.x * n.x + n.y * n.y, 1.0f); }
  __host__ __device__ __forceinline__ bool take(const float* __restrict__ env, int EH, int EW, V3 wl, float np, float& w, float L[3]) const {
    const float pl = env_lookup_pdf(env, EH, EW, wl, lt.norm, sc_pole, L);
    w = w * (lit ? power_weight(np, nlight * pl) : 1.0f);
    return true;
  }
  __host__ __device__ __forceinline__ bool open(V3) const { return true; }
  // table entry k = (direction, radiance, p_L), SoA planes of M floats; l_k = Rot^T w_k in the row's frame.  t: the technique itself
  // (accL, the table) with its own open().
  template <bool VIEW, typename T>
  __host__ __device__ static __forceinline__ void table_sum(T& t, const Principled& p, const ViewRot& rot, V3 n, int lane, int lanes) {
    if (!t.lit) return;
    const LightTable& lt = t.lt;
    const float nlight = t.nlight, nlobe = t.nlobe, g1v = t.g1v;
    float* accL = t.accL;
    const bool diffuse = p.m < 1.0f;
    const float cv = n.z;
    for (int k = lane; k < lt.M; k += lanes) {
      const V3 wd = v3(lt.tab[k], lt.tab[lt.M + k], lt.tab[2 * lt.M + k]);
      const float pl = lt.tab[6 * lt.M + k];
      const V3 l = from_world<VIEW>(rot, wd);
      const float cl = dot3(n, l);
      if (cl > 0.0f && pl > 0.0f && t.open(wd)) {
        const V3 h = half_vector(l);
        const float vh = h.z, nh = dot3(n, h);
        const float ps = visible_density(g1v, ggx_d(p.a2, nh, cross_sq(n, h)), cv);
        const float ks = ps * ggx_g1(p.a2, cl, cross_sq(n, l), dot3(l, h));  // D G / (4 n.v)
        const float kd = diffuse ? (1.0f - p.m) * cl * diffuse_shape(p.r, cl, cv, vh) * (1.0f / kPi) : 0.0f;
        const float a = nlight * pl, as = nlobe * ps, ad = diffuse ? nlobe * cl * (1.0f / kPi) : 0.0f;
        const float ws = ks * (a / (as * as + a * a)), wd2 = kd * (a / (ad * ad + a * a));
        const float fd = (1.0f - p.m) * fresnel_dielectric(vh, p.eta), sw = schlick_weight(vh);
#pragma unroll
        for (int c = 0; c < 3; ++c) accL[c] += lt.tab[(3 + c) * lt.M + k] * ((fd + p.m * (p.c[c] + (1.0f - p.c[c]) * sw)) * ws + p.c[c] * wd2);
      }
    }
  }
  template <bool VIEW>
  __host__ __device__ __forceinline__ void finish(const Principled& p, const ViewRot& rot, V3 n, int lane, int lanes) {
    table_sum<VIEW>(*this, p, rot, n, lane, lanes);
  }
};
__host__ __device__ __forceinline__ LightSampled light_sampled(const LightTable& lt, int EH, int Q) {
  return LightSampled{lt, {0.0f, 0.0f, 0.0f}, (float)(Q * Q), (float)lt.M, sinf(0.25f * kPi / (float)EH), 0.0f, lt.norm > 0.0f};
}

// The light technique on the shadowed mesh: both of its sample sets estimate L V f cos, V = 0 along an occluded ray, with the weights of
// LightSampled (p_L knows nothing of occlusion; the weights of a direction still sum to one, so the estimator stays consistent).  A lobe
// sample is traced where Occluded traces it, before any texel fetch; a table direction -- a world direction, which is the object-space ray
// direction, as to_world(rot, l) is for a lobe sample -- is traced after its cheap rejections.
struct LitOccluded : LightSampled {
  Tracer trace;
  __host__ __device__ __forceinline__ bool open(V3 w) const { return !trace.occluded(w); }
  __host__ __device__ __forceinline__ bool take(const float* __restrict__ env, int EH, int EW, V3 wl, float np, float& w, float L[3]) const {
    return open(wl) && LightSampled::take(env, EH, EW, wl, np, w, L);
  }
  template <bool VIEW>
  __host__ __device__ __forceinline__ void finish(const Principled& p, const ViewRot& rot, V3 n, int lane, int lanes) {
    table_sum<VIEW>(*this, p, rot, n, lane, lanes);
  }
};

// one lane's share of the radiance a surface point with unit normal n (n.z > -1; the callers pass n.z > 0) reflects toward the viewer at +z:
// the grid points q = lane, lane + lanes, ... of both lobes, summed in that order into acc (unnormalised).  env == nullptr: white
// environment (L = 1).  The pixel kernels (RowMaterial) and the mesh (mesh_shade_kernel) share this body; TECH (above) is asked about every
// lobe sample with a non-zero weight, along to_world(rot, l), the vector the environment lookup forms.
template <bool VIEW, typename TECH>
__host__ __device__ __forceinline__ void normal_lane_sum(const Principled& p, const float* __restrict__ env, const ViewRot& rot, int EH, int EW, V3 n,
                                                         int Q, int lane, int lanes, float acc[3], TECH& tech) {
  static_assert(std::is_same_v<TECH, Plain> || std::is_same_v<TECH, Occluded> || std::is_same_v<TECH, LightSampled> || std::is_same_v<TECH, LitOccluded> ||
                    std::is_same_v<TECH, Bounced>,
                "the techniques: {no light samples, light samples} x {not traced, traced}, and traced with one bounce (no light samples)");
  const float invQ = 1.0f / (float)Q;
  const bool diffuse = p.m < 1.0f;
  const float cv = n.z;  // n.v for v = +z
  // orthonormal frame (t, bt, n) (n.z > 0 on the whole film: the sign term is the literal 1); v = (-n.x, -n.y, n.z) in it
  const Frame f = duff_frame(n, 1.0f);
  const VisibleFrame vf = visible_frame(n, p.alpha);
  tech.begin(p, n);
  for (int q = lane; q < Q * Q; q += lanes) {
    const GridPoint g = grid_point(q, Q, invQ);
    float L[3] = {1.0f, 1.0f, 1.0f};
    // specular lobe: the GGX sample; weight F G1(l)
    {
      const GgxSample s = ggx_sample(vf, p.alpha, n, f, g);
      if (s.vh > 0.0f && s.cl > 0.0f && ggx_d(p.a2, s.nh, s.s2h) > 0.0f) {
        float w = ggx_g1(p.a2, s.cl, cross_sq(n, s.l), s.vh), np = 0.0f;
        const float fd = (1.0f - p.m) * fresnel_dielectric(s.vh, p.eta), sw = schlick_weight(s.vh);
        if constexpr (TECH::kNeedsDensity) np = tech.nlobe * visible_density(tech.g1v, ggx_d(p.a2, s.nh, s.s2h), cv);
        if (tech.take(env, EH, EW, to_world<VIEW>(rot, s.l), np, w, L)) {
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] += (fd + p.m * (p.c[c] + (1.0f - p.c[c]) * sw)) * w * L[c];
        }
      }
    }
    // diffuse lobe: cosine-weighted l; weight pi diff / (n.l) = (1 - m) c shape
    if (diffuse) {
      float cl;
      const V3 l = cosine_direction(n, f, g.u1, g.sp, g.cp, cl);
      // (not half_vector(l).z: this lobe divides h.z by |h| where half_vector multiplies by 1 / |h|, another rounding, and a render's bits stay)
      const V3 h = v3(l.x, l.y, l.z + 1.0f);
      const float cd = h.z / sqrtf(dot3(h, h));  // h.v for h = normalize(v + l)
      float w = (1.0f - p.m) * diffuse_shape(p.r, cl, cv, cd), np = 0.0f;
      if constexpr (TECH::kNeedsDensity) np = tech.nlobe * cl * (1.0f / kPi);  // p_d(l) = n.l / pi
      if (tech.take(env, EH, EW, to_world<VIEW>(rot, l), np, w, L)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += p.c[c] * w * L[c];
      }
    }
  }
  tech.template finish<VIEW>(p, rot, n, lane, lanes);
}

// The material of the pixel kernels of render_shared.h for a principled row: row `row` of z [rows][6] under Plain, or, LIGHT, under
// LightSampled with the light table of map b (lws: the light workspace of the B maps, M samples each), which every pixel of the map's rows
// reads from memory, a wave's loads contiguous: it is not staged in LDS.  (Staging would tie the four waves of a workgroup, which may
// belong to different maps and may have left at the bounds check, to barriers, and a table of M = 65536 samples, 1.8 MB, does not fit; the
// 28 KB of M = 1024 stay cache-resident.)  accL joins the pixel after the butterfly, divided by S^2 only.  Without LIGHT: the row alone.
struct RowArgs {
  const float* z;
};
struct LitRowArgs {
  const float* z;
  const char* lws;
  int M;
};
template <bool LIGHT>
struct RowMaterial {
  using Args = std::conditional_t<LIGHT, LitRowArgs, RowArgs>;
  static constexpr bool kStacked = true;  // rows = L B
  Principled p;
  std::conditional_t<LIGHT, LightSampled, Plain> tech;
  __device__ __forceinline__ RowMaterial(const Args& a, int row, int b, int EH, int Q) : p(principled(a.z + 6 * (size_t)row)) {
    if constexpr (LIGHT) tech = light_sampled(light_table(a.lws, b, EH, a.M), EH, Q);
  }
  template <bool VIEW>
  __device__ __forceinline__ void lane_sum(const float* __restrict__ env, const ViewRot& rot, int EH, int EW, V3 n, int Q, int lane, int lanes, float acc[3]) {
    normal_lane_sum<VIEW>(p, env, rot, EH, EW, n, Q, lane, lanes, acc, tech);
  }
  __device__ __forceinline__ void meet() {
    if constexpr (LIGHT) wave_sum3(tech.accL);
  }
  __device__ __forceinline__ float joined(int c, float px, float inv_s2) const {
    if constexpr (LIGHT) return px + tech.accL[c] * inv_s2;
    else return px;
  }
};

// The lit normal map keeps a kernel of its own: normals_pixel_kernel's pixel (render_shared.h: the same reading of the normal map, drawn rule
// and stores) with LightSampled, the light table's header read ahead of the drawn test and the row inside it.  As an instantiation of the
// shared kernel it measured 0.05 .. 0.17 % slower than this in every run, more than two copies of one library differ.
template <bool VIEW>
__global__ __launch_bounds__(256) void normals_lit_kernel(const float* __restrict__ normals, const unsigned char* __restrict__ mask, int Bn,
                                                          const float* __restrict__ z, const float* __restrict__ env, const float* __restrict__ view,
                                                          float* __restrict__ image, float* __restrict__ alpha, int B, int H, int W, int EH, int EW, int Q,
                                                          const char* __restrict__ lws, int M) {
  const long long pix = (long long)blockIdx.x * kRenderWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pix >= (long long)B * H * W) return;  // (wave-uniform)
  const size_t plane = (size_t)H * W;
  const int b = __builtin_amdgcn_readfirstlane((int)(pix / ((long long)H * W)));
  const size_t at = (size_t)(pix - (long long)b * H * W);
  V3 n = v3(0.0f, 0.0f, 0.0f);
  const bool drawn = normal_map_pixel(normals, mask, (Bn == 1 ? 0 : (size_t)b * plane) + at, n);  // (wave-uniform: every lane read the same pixel)
  float acc[3] = {0.0f, 0.0f, 0.0f};
  LightSampled tech = light_sampled(light_table(lws, b, EH, M), EH, Q);
  if (drawn) {
    const Principled p = principled(z + 6 * (size_t)b);
    const float* e = env ? env + (size_t)b * EH * EW * 3 : nullptr;
    const ViewRot rot = view_rot(VIEW ? view + 9 * (size_t)b : nullptr);
    normal_lane_sum<VIEW>(p, e, rot, EH, EW, n, Q, lane, 64, acc, tech);
    wave_sum3(acc);
    wave_sum3(tech.accL);
  }
  if (lane == 0) {
    const float scale = 1.0f / (float)(Q * Q);
#pragma unroll
    for (int c = 0; c < 3; ++c) image[((size_t)b * 3 + c) * plane + at] = drawn ? acc[c] * scale + tech.accL[c] : 0.0f;
    if (alpha) alpha[(size_t)b * plane + at] = drawn ? 1.0f : 0.0f;
  }
}

// Shading of the hits of mesh.hip's visibility pass.  grid: ceil(B H W / 4) workgroups of 4 waves; wave = pixel (row b, i, j) of the object image,
// lit by env[b] and seen through view[b].  For each of the pixel's S x S samples, in sample order, the wave fetches the hit (one address: a
// broadcast), forms the shading normal -- the barycentric mix of the face's vertex normals, taken into the view frame (Rot^T n) and normalised;
// a zero mix stays zero -- and, where n.z > 0, runs the sphere's normal_lane_sum: the same Q x Q grids, per-lane order and butterfly, so a
// mesh point is shaded exactly as the sphere point with that normal.  Lane 0 also writes the means of the normals, of 1.1 - z over the
// hits, and the hit fraction.  rec / hits: the workspace halves of launch_mesh_visibility.
// The technique is built in one place, mesh_technique below, for all five, and a traced one is moved to every hit sample.  A
// light-sampled one is the pixel's: its accL runs through the pixel's hit samples in sample order and meets in a second butterfly, as in
// the sphere's lit kernel.
// SHADOW: every direction of a hit sample is traced from the hit point -- the view-space (x_sample, y_sample, z_hit) taken to object
// space with Rot -- through the BVH in sh, the hit face excluded.  Without it sh is an empty struct and the kernel is the one it always was.
// LIGHT: li holds the light workspace of the B maps (M samples each; see RowMaterial on why the table is not staged in LDS).
// Without it li is an empty struct.
// BOUNCE (with SHADOW, without LIGHT): the technique is Bounced instead of Occluded; bo holds bounce_quad.  Without it bo is an empty struct.
// (NoShadowArgs, ShadowArgs: mesh_shade.h)
struct NoLightArgs {};
struct LightArgs {
  const char* lws;
  int M;
};
struct NoBounceArgs {};
struct BounceArgs {
  int quad;
};
// the technique of a mesh pixel of row b: {Plain, LightSampled} without the BVH, {Occluded, LitOccluded, Bounced} with it
template <bool SHADOW, bool LIGHT, bool BOUNCE>
using MeshTechnique = std::conditional_t<BOUNCE, Bounced, std::conditional_t<LIGHT, std::conditional_t<SHADOW, LitOccluded, LightSampled>,
                                                                             std::conditional_t<SHADOW, Occluded, Plain>>>;
template <bool SHADOW, bool LIGHT, bool BOUNCE, typename SH, typename LI, typename BO>
__device__ __forceinline__ MeshTechnique<SHADOW, LIGHT, BOUNCE> mesh_technique(const Principled& p, const float* vnormal, long long F, int b, int EH, int Q,
                                                                               const SH& sh, const LI& li, const BO& bo) {
  MeshTechnique<SHADOW, LIGHT, BOUNCE> t;
  if constexpr (LIGHT) static_cast<LightSampled&>(t) = light_sampled(light_table(li.lws, b, EH, li.M), EH, Q);
  if constexpr (SHADOW) {
    trace_mesh(t.trace, sh, F);
  }
  if constexpr (BOUNCE) {
    t.vnormal = vnormal;
    t.p = p;
    t.bq = bo.quad;
  }
  return t;
}

template <bool VIEW, bool SHADOW, bool LIGHT, bool BOUNCE = false>
__global__ __launch_bounds__(256) void mesh_shade_kernel(const float* __restrict__ z, const float* __restrict__ env, const float* __restrict__ view,
                                                         const float* __restrict__ vnormal, const float* __restrict__ rec, const float* __restrict__ hits,
                                                         float* __restrict__ image, float* __restrict__ normal, float* __restrict__ depth,
                                                         float* __restrict__ alpha, int B, long long F, int H, int W, int EH, int EW, int Q, int S,
                                                         std::conditional_t<SHADOW, ShadowArgs, NoShadowArgs> sh,
                                                         std::conditional_t<LIGHT, LightArgs, NoLightArgs> li,
                                                         std::conditional_t<BOUNCE, BounceArgs, NoBounceArgs> bo) {
  static_assert(!BOUNCE || (SHADOW && !LIGHT), "the bounce needs the BVH and is not combined with light samples");
  const long long pix = (long long)blockIdx.x * kRenderWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pix >= (long long)B * H * W) return;  // (wave-uniform)
  const int b = __builtin_amdgcn_readfirstlane((int)(pix / ((long long)H * W)));
  const int rem = (int)(pix - (long long)b * H * W);
  const int i = rem / W, j = rem - (rem / W) * W;
  const Principled p = principled(z + 6 * (size_t)b);
  const float* e = env ? env + (size_t)b * EH * EW * 3 : nullptr;
  const ViewRot rot = view_rot(VIEW ? view + 9 * (size_t)b : nullptr);
  const float4* hit = reinterpret_cast<const float4*>(hits) + (size_t)b * H * S * W * S;
  const float* records = rec + (size_t)b * F * kMeshRecordWords;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  float nsum[3] = {0.0f, 0.0f, 0.0f}, dsum = 0.0f;
  int count = 0;
  // (a technique is built where its state begins: a light-sampled one carries accL through the pixel's hit samples; the others carry nothing
  // from one hit sample to the next and are built at each.  Held across the pixel, the tree's header cost the shadowed kernel 0.9 % on a
  // mesh of 20 480 faces; rebuilt per sample, the lit + shadowed one lost 0.6 %.)
  MeshTechnique<SHADOW, LIGHT, BOUNCE> tech;
  if constexpr (LIGHT) tech = mesh_technique<SHADOW, LIGHT, BOUNCE>(p, vnormal, F, b, EH, Q, sh, li, bo);
  for (int sy = 0; sy < S; ++sy) {
    for (int sx = 0; sx < S; ++sx) {
      const float4 h = hit[((size_t)i * S + sy) * W * S + (size_t)j * S + sx];
      const int f = __float_as_int(h.x);
      if (f < 0) continue;  // (wave-uniform: every lane read the same hit)
      const float* r = records + (size_t)f * kMeshRecordWords;
      const float* n0 = vnormal + 3 * (size_t)__float_as_int(r[kMeshRecIndex]);
      const float* n1 = vnormal + 3 * (size_t)__float_as_int(r[kMeshRecIndex + 1]);
      const float* n2 = vnormal + 3 * (size_t)__float_as_int(r[kMeshRecIndex + 2]);
      const V3 n = unit_or_zero(from_world<VIEW>(rot, mix_normals(n0, n1, n2, h.y, h.z)));  // (a zero or NaN mix stays a zero normal)
      nsum[0] += n.x;
      nsum[1] += n.y;
      nsum[2] += n.z;
      dsum += 1.1f - h.w;
      ++count;
      if (n.z > 0.0f) {
        if constexpr (!LIGHT) tech = mesh_technique<SHADOW, LIGHT, BOUNCE>(p, vnormal, F, b, EH, Q, sh, li, bo);
        if constexpr (SHADOW)
          tech.trace.from(mesh_sample_origin<VIEW>(rot, j * S + sx, i * S + sy, W, H, S, h.w), f);
        normal_lane_sum<VIEW>(p, e, rot, EH, EW, n, Q, lane, 64, acc, tech);
      }
    }
  }
  wave_sum3(acc);
  if constexpr (LIGHT) wave_sum3(tech.accL);
  if (lane == 0) {
    const float inv_s2 = 1.0f / (float)(S * S), scale = 1.0f / ((float)(S * S) * (float)(Q * Q));
    const size_t at = (size_t)i * W + j, plane = (size_t)H * W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float px = acc[c] * scale;
      if constexpr (LIGHT) px = px + tech.accL[c] * inv_s2;
      image[((size_t)b * 3 + c) * plane + at] = px;
      if (normal) normal[((size_t)b * 3 + c) * plane + at] = nsum[c] * inv_s2;
    }
    if (depth) depth[(size_t)b * plane + at] = count > 0 ? dsum / (float)count : 0.0f;
    if (alpha) alpha[(size_t)b * plane + at] = (float)count * inv_s2;
  }
}

// ---- building the light workspace: three launches per render, fp64 sums in a fixed order, no atomics
constexpr double kPiD = 3.14159265358979323846;
__device__ __forceinline__ double luma64(const float* t) { return fmax(0.2126 * (double)t[0] + 0.7152 * (double)t[1] + 0.0722 * (double)t[2], 0.0); }
struct LightCell {
  double v00, v01, v10, v11;  // corner luminances, v{theta}{psi}
};
__device__ __forceinline__ LightCell light_cell(const float* __restrict__ env, int EH, int EW, int c, int j) {
  const int i0 = c > 0 ? c - 1 : 0, i1 = c < EH ? c : EH - 1, j1 = j + 1 == EW ? 0 : j + 1;
  const float* r0 = env + (size_t)i0 * EW * 3;
  const float* r1 = env + (size_t)i1 * EW * 3;
  return LightCell{luma64(r0 + 3 * j), luma64(r0 + 3 * j1), luma64(r1 + 3 * j), luma64(r1 + 3 * j1)};
}
__device__ __forceinline__ double mean4(const LightCell& v) { return 0.25 * (v.v00 + v.v01 + v.v10 + v.v11); }
__device__ __forceinline__ double cell_lo(int c, int EH) { return c > 0 ? ((double)c - 0.5) * kPiD / (double)EH : 0.0; }
__device__ __forceinline__ double cell_hi(int c, int EH) { return c < EH ? ((double)c + 0.5) * kPiD / (double)EH : kPiD; }
// inclusive prefix sum over the 64 lanes, in a fixed order
__device__ __forceinline__ double wave_scan(double x, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(x, o);
    if (lane >= o) x += t;
  }
  return x;
}
// x in [0, 1] whose cdf is u under the density proportional to (1 - x) a + x b; x = u where a + b = 0
__device__ __forceinline__ double linear_inverse(double u, double a, double b) {
  const double d = a + sqrt((1.0 - u) * a * a + u * b * b);
  return (a + b > 0.0 && d > 0.0) ? u * (a + b) / d : u;
}

// grid (EH + 1, B), 256 threads: rowsum[c] and mass[c] of cell row c of map b
__global__ __launch_bounds__(256) void light_rows_kernel(const float* __restrict__ env, char* __restrict__ ws, int EH, int EW, int M) {
  __shared__ double sh[256];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* e = env + (size_t)b * EH * EW * 3;
  double s = 0.0;
  for (int j = tid; j < EW; j += 256) s += mean4(light_cell(e, EH, EW, c, j));
  sh[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    double* d = reinterpret_cast<double*>(ws + (size_t)b * light_ws_stride(EH, M));
    const double lo = cell_lo(c, EH), hi = cell_hi(c, EH);
    d[(EH + 2) + c] = sh[0];
    d[(EH + 2) + (EH + 1) + c] = sh[0] * sin(0.5 * (lo + hi)) * (hi - lo);
  }
}

// grid B, one wave: the marginal CDF over the EH + 1 rows, tot and norm = 1 / (tot dpsi) (0 for a map without light)
__global__ __launch_bounds__(64) void light_cdf_kernel(char* __restrict__ ws, int EH, int EW, int M) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double* d = reinterpret_cast<double*>(ws + (size_t)b * light_ws_stride(EH, M));
  const double* mass = d + (EH + 2) + (EH + 1);
  double run = 0.0;
  if (lane == 0) d[0] = 0.0;
  for (int base = 0; base <= EH; base += 64) {
    const int c = base + lane;
    const double incl = wave_scan(c <= EH ? mass[c] : 0.0, lane);
    if (c <= EH) d[c + 1] = run + incl;
    run += __shfl(incl, 63);
  }
  if (lane == 0) {
    const bool ok = run > 0.0 && run < 1e300;  // (an infinite total gives a map no light technique either; a NaN texel has luminance 0)
    *reinterpret_cast<float*>(d + light_ws_doubles(EH)) = ok ? (float)(1.0 / (run * (2.0 * kPiD / (double)EW))) : 0.0f;
  }
}

// grid (M / 4, B), 4 waves: one wave per sample k, the Hammersley point U1 = (k + 1/2) / M, U2 = bitreverse32(k) 2^-32 + 1 / (2 M).  U1 picks
// the cell row through the marginal CDF; U2 picks the column through the row's conditional CDF, which is not stored: the wave scans the row
// in 64-wide chunks in a fixed order.  The remapped pair is the position inside the cell, found by inverting the bilinear density: theta from
// the linear marginal (v00 + v01, v10 + v11), then psi from the linear conditional.  The radiance is the bilinear interpolant of the cell's
// corners at that position (what env_lookup reads there) and p_L the cell's own density, both evaluated in fp64.
__global__ __launch_bounds__(256) void light_table_kernel(const float* __restrict__ env, char* __restrict__ ws, int EH, int EW, int M) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y, lane = threadIdx.x & 63;
  char* base_ws = ws + (size_t)b * light_ws_stride(EH, M);
  const double* cdf = reinterpret_cast<const double*>(base_ws);
  const double* rowsum = cdf + (EH + 2);
  const double* mass = rowsum + (EH + 1);
  const float norm = *reinterpret_cast<const float*>(base_ws + light_ws_doubles(EH) * 8);
  if (k >= M || !(norm > 0.0f)) return;  // (wave-uniform)
  float* tab = reinterpret_cast<float*>(base_ws + light_ws_doubles(EH) * 8 + 8);
  const float* e = env + (size_t)b * EH * EW * 3;
  const double tot = cdf[EH + 1];
  const double U1 = ((double)k + 0.5) / (double)M;
  const double U2 = (double)__brev((unsigned)k) * (1.0 / 4294967296.0) + 0.5 / (double)M;
  // the last row whose cdf is <= U1 tot
  const double t1 = U1 * tot;
  int c = 0, hi = EH + 1;
  while (hi - c > 1) {
    const int mid = (c + hi) >> 1;
    if (cdf[mid] <= t1) c = mid; else hi = mid;
  }
  const double u1 = mass[c] > 0.0 ? fmin(fmax((t1 - cdf[c]) / mass[c], 0.0), 1.0) : 0.5;
  // the first column whose running sum exceeds U2 rowsum
  const double t2 = U2 * rowsum[c];
  double run = 0.0, before = 0.0;
  int j = -1;
  for (int base = 0; base < EW && j < 0; base += 64) {
    const int jj = base + lane;
    const double x = jj < EW ? mean4(light_cell(e, EH, EW, c, jj)) : 0.0;
    const double incl = wave_scan(x, lane);
    const unsigned long long hit = __ballot(jj < EW && run + incl > t2);
    if (hit) {
      const int f = __ffsll((long long)hit) - 1;
      j = base + f;
      const double prev = __shfl(incl, f > 0 ? f - 1 : 0);
      before = f > 0 ? run + prev : run;
    }
    run += __shfl(incl, 63);
  }
  const bool found = j >= 0;
  if (!found) j = EW - 1;  // (U2 rowsum at or past the scanned total: rounding only)
  const LightCell v = light_cell(e, EH, EW, c, j);
  const double m4 = mean4(v);
  const double u2 = !found ? 1.0 : m4 > 0.0 ? fmin(fmax((t2 - before) / m4, 0.0), 1.0) : 0.5;
  const double s = linear_inverse(u1, v.v00 + v.v01, v.v10 + v.v11);
  const double t = linear_inverse(u2, (1.0 - s) * v.v00 + s * v.v10, (1.0 - s) * v.v01 + s * v.v11);
  const double lo = cell_lo(c, EH), hic = cell_hi(c, EH), dpsi = 2.0 * kPiD / (double)EW;
  const double theta = lo + s * (hic - lo), psi = ((double)j + 0.5 + t) * dpsi;
  const double st = sin(theta), val = (1.0 - s) * ((1.0 - t) * v.v00 + t * v.v01) + s * ((1.0 - t) * v.v10 + t * v.v11);
  const double pdf = val * sin(0.5 * (lo + hic)) / (tot * dpsi) / fmax(st, 1e-6);
  if (lane == 0) {
    tab[k] = (float)(st * sin(psi));
    tab[M + k] = (float)cos(theta);
    tab[2 * M + k] = (float)(-st * cos(psi));
    const int i0 = c > 0 ? c - 1 : 0, i1 = c < EH ? c : EH - 1, j1 = j + 1 == EW ? 0 : j + 1;
    const float* r0 = e + (size_t)i0 * EW * 3;
    const float* r1 = e + (size_t)i1 * EW * 3;
    for (int ch = 0; ch < 3; ++ch)
      tab[(3 + ch) * M + k] = (float)((1.0 - s) * ((1.0 - t) * (double)r0[3 * j + ch] + t * (double)r0[3 * j1 + ch]) +
                                      s * ((1.0 - t) * (double)r1[3 * j + ch] + t * (double)r1[3 * j1 + ch]));
    tab[6 * M + k] = (float)pdf;
  }
}

// one thread per element: out[k] = eval(z[k or 0], n[k], v[k], l[k])
__global__ __launch_bounds__(256) void brdf_eval_kernel(const float* __restrict__ z, int z_rows, const float* __restrict__ n, const float* __restrict__ v,
                                                        const float* __restrict__ l, float* __restrict__ out, long long N) {
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < N; k += (long long)gridDim.x * blockDim.x) {
    const Principled p = principled(z + (z_rows == 1 ? 0 : 6 * k));
    float f[3];
    principled_eval(p, n + 3 * k, v + 3 * k, l + 3 * k, f);
    out[3 * k] = f[0];
    out[3 * k + 1] = f[1];
    out[3 * k + 2] = f[2];
  }
}

}  // namespace

static bool light_samples_ok(int M) { return M >= 64 && M <= 65536 && (M & (M - 1)) == 0; }

size_t render_light_workspace_bytes(int B, int EH, int EW, int light_samples) {
  if (B < 1 || EH < 1 || EW < 1 || (long long)EH * EW > (1LL << 28) || !light_samples_ok(light_samples)) return 0;
  return (size_t)B * light_ws_stride(EH, light_samples);
}

// the light workspace of the B maps, M samples each: three launches (see "building the light workspace")
static void launch_light_tables(const drm_shading& sh, hipStream_t s) {
  char* ws = static_cast<char*>(sh.light_workspace);
  const int M = sh.light_samples;
  hipLaunchKernelGGL(light_rows_kernel, dim3((unsigned)(sh.EH + 1), (unsigned)sh.B), dim3(256), 0, s, sh.envmap, ws, sh.EH, sh.EW, M);
  hipLaunchKernelGGL(light_cdf_kernel, dim3((unsigned)sh.B), dim3(64), 0, s, ws, sh.EH, sh.EW, M);
  hipLaunchKernelGGL(light_table_kernel, dim3((unsigned)(M / 4), (unsigned)sh.B), dim3(256), 0, s, sh.envmap, ws, sh.EH, sh.EW, M);
}

int check_shading(const std::string& who, const drm_shading& sh, int subpixel, int subpixel_max, bool* lit, std::string* light_fault) {
  DRM_REQUIRE_SIZE(&sh, drm_shading);
  DRM_REQUIRE((sh.z != nullptr) != (sh.tables != nullptr), who + ": exactly one material, z (principled rows) or tables (measured), must be given");
  DRM_REQUIRE(sh.light_samples >= 0, who + ": light_samples >= 0");
  DRM_REQUIRE(sh.quad >= 1 && sh.quad <= 1024 && (!subpixel_max || (subpixel >= 1 && subpixel <= subpixel_max)),
              who + ": quad in [1, 1024]" + (subpixel_max ? ", subpixel in [1, " + std::to_string(subpixel_max) + "]" : ""));
  DRM_REQUIRE(!sh.envmap || (sh.EH > 0 && sh.EW > 0 && (long long)sh.EH * sh.EW <= (1LL << 28)), who + ": envmap must be EH x EW with EH, EW >= 1");
  *lit = sh.light_samples > 0 && sh.envmap;
  light_fault->clear();
  if (!*lit) return DRM_OK;
  DRM_REQUIRE(!sh.tables, who + ": light samples under tables are not built");
  DRM_REQUIRE(light_samples_ok(sh.light_samples), who + ": light_samples must be 0 or a power of two in [64, 65536]");
  const size_t need = render_light_workspace_bytes(sh.B, sh.EH, sh.EW, sh.light_samples);
  if (need == 0 || !sh.light_workspace || sh.light_workspace_bytes < need || (reinterpret_cast<uintptr_t>(sh.light_workspace) & 7) != 0)
    *light_fault = who + ": light_workspace must be 8-byte aligned and hold drm_render_light_workspace_bytes = " + std::to_string(need) + " bytes";
  return DRM_OK;
}

// every sphere render: light_samples = 0, or a white environment, is the plain one (no workspace, no light kernels)
int launch_render_refmap(const drm_shading& sh, int L, int R, int subpixel, int flip, float* out, hipStream_t s) {
  bool lit;
  std::string light_fault;
  DRM_TRY(check_shading("render_refmap", sh, subpixel, 16, &lit, &light_fault));
  DRM_REQUIRE(out, "render_refmap: out is null");
  DRM_REQUIRE(!sh.tables || L == 1, "render_refmap: tables render one set of rows (L == 1)");
  const int B = sh.B;
  DRM_REQUIRE(L > 0 && B > 0 && ((!lit && !sh.tables) || B <= 65535) && (long long)L * B <= 0x7fffffffLL && R > 0 && R <= 8192,
              lit || sh.tables ? "render_refmap: L >= 1 stacks of 1 <= B <= 65535 rows (lit, or under tables) of R x R pixels, 1 <= R <= 8192"
                               : "render_refmap: L >= 1 stacks of B >= 1 rows of R x R pixels, 1 <= R <= 8192");
  if (!light_fault.empty()) {
    set_error(light_fault);
    return DRM_ERR_WORKSPACE;
  }
  PixelLaunch pl;
  DRM_TRY(plan_pixel_launch("render_refmap", "L B R^2", (long long)L * B * R * R, sh.envmap, sh.view, sh.EH, sh.EW, pl));
  if (sh.tables) return launch_refmap_tables(sh, pl, R, subpixel, flip, out, s);
  if (lit) launch_light_tables(sh, s);
  const auto launch = [&](auto kernel, auto margs) {
    hipLaunchKernelGGL(kernel, dim3(pl.blocks), dim3(64 * kRenderWaves), 0, s, margs, sh.envmap, pl.view, out, L * B, B, R, pl.EH, pl.EW, sh.quad, subpixel,
                       flip ? 1 : 0);
  };
  if (lit)
    launch(pl.view ? sphere_pixel_kernel<true, RowMaterial<true>> : sphere_pixel_kernel<false, RowMaterial<true>>,
           LitRowArgs{sh.z, static_cast<char*>(sh.light_workspace), sh.light_samples});
  else launch(pl.view ? sphere_pixel_kernel<true, RowMaterial<false>> : sphere_pixel_kernel<false, RowMaterial<false>>, RowArgs{sh.z});
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

// Every mesh render: the same checks and visibility launches.  shadows verifies the blob (nothing is launched before that) and shades with
// it; light samples build the tables as the sphere's lit render does and shade with them; bounces = 1 (with shadows and without light
// samples) shades with one bounce.
int launch_render_mesh(const drm_shading& sh, const drm_mesh_render& m, hipStream_t s) {
  DRM_REQUIRE_SIZE(&m, drm_mesh_render);
  bool lit;
  std::string light_fault;
  DRM_TRY(check_shading("render_mesh", sh, m.subpixel, 0, &lit, &light_fault));
  DRM_REQUIRE(!sh.tables, "render_mesh: a mesh is shaded with principled rows z, not tables");
  DRM_REQUIRE(m.vertex_positions && m.vertex_normals && m.faces && m.image, "render_mesh: null pointer");
  DRM_REQUIRE(m.bounces == 0 || (m.bounces == 1 && m.shadows && !lit && m.bounce_quad >= 1 && m.bounce_quad <= 16),
              "render_mesh: bounces is 0, or 1 with shadows, without light samples and with bounce_quad in [1, 16]");
  const int B = sh.B;
  const long long V = m.V, F = m.F;
  MeshLaunch ml;
  DRM_TRY(plan_mesh_render("render_mesh", B, m, ml));
  DRM_REQUIRE(light_fault.empty(), light_fault);
  if (m.shadows) DRM_TRY(check_device_bvh(m.bvh, m.bvh_bytes, true, F, s, "render_mesh"));
  float *const records = ml.records, *const hits = ml.hits;
  DRM_TRY(launch_mesh_visibility(m.vertex_positions, m.faces, V, F, sh.view, B, m.H, m.W, m.subpixel, records, hits, s));
  if (lit) launch_light_tables(sh, s);
  // the instantiation: with or without the view, then the technique
  const auto shade = [&](auto with_view) {
    constexpr bool VIEW = decltype(with_view)::value;
    const auto launch = [&](auto kernel, auto shadow, auto li, auto bo) {
      hipLaunchKernelGGL(kernel, dim3(ml.blocks), dim3(64 * kRenderWaves), 0, s, sh.z, sh.envmap, sh.view, m.vertex_normals, records, hits, m.image,
                         m.normal, m.depth, m.alpha, B, F, m.H, m.W, sh.envmap ? sh.EH : 1, sh.envmap ? sh.EW : 1, sh.quad, m.subpixel, shadow, li, bo);
    };
    const ShadowArgs shadow{m.vertex_positions, m.faces, V, m.bvh};
    const LightArgs li{lit ? static_cast<char*>(sh.light_workspace) : nullptr, sh.light_samples};
    if (m.bounces) launch(mesh_shade_kernel<VIEW, true, false, true>, shadow, NoLightArgs{}, BounceArgs{m.bounce_quad});
    else if (lit && m.shadows) launch(mesh_shade_kernel<VIEW, true, true>, shadow, li, NoBounceArgs{});
    else if (lit) launch(mesh_shade_kernel<VIEW, false, true>, NoShadowArgs{}, li, NoBounceArgs{});
    else if (m.shadows) launch(mesh_shade_kernel<VIEW, true, false>, shadow, NoLightArgs{}, NoBounceArgs{});
    else launch(mesh_shade_kernel<VIEW, false, false>, NoShadowArgs{}, NoLightArgs{}, NoBounceArgs{});
  };
  if (sh.view) shade(std::true_type{});
  else shade(std::false_type{});
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

// A normal map shaded B ways (see drm_render_normals): light samples build the tables as the lit renders do and shade with them.
int launch_render_normals(const drm_shading& sh, const float* normals, const unsigned char* mask, int Bn, int H, int W, float* image, float* alpha,
                          hipStream_t s) {
  bool lit;
  std::string light_fault;
  DRM_TRY(check_shading("render_normals", sh, 1, 0, &lit, &light_fault));
  DRM_REQUIRE(normals && image, "render_normals: null pointer");
  const int B = sh.B;
  DRM_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096 && (Bn == 1 || Bn == B),
              "render_normals: 1 <= B <= 65535 rows, H and W in [1, 4096], Bn = 1 or B normal maps");
  PixelLaunch pl;
  DRM_TRY(plan_pixel_launch("render_normals", "B H W", (long long)B * H * W, sh.envmap, sh.view, sh.EH, sh.EW, pl));
  DRM_REQUIRE(light_fault.empty(), light_fault);
  if (sh.tables) return launch_normals_tables(sh, pl, normals, mask, Bn, H, W, image, alpha, s);
  if (lit) {
    launch_light_tables(sh, s);
    const auto kernel = pl.view ? normals_lit_kernel<true> : normals_lit_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(pl.blocks), dim3(64 * kRenderWaves), 0, s, normals, mask, Bn, sh.z, sh.envmap, pl.view, image, alpha, B, H, W, pl.EH, pl.EW,
                       sh.quad, static_cast<char*>(sh.light_workspace), sh.light_samples);
  } else {
    const auto kernel = pl.view ? normals_pixel_kernel<true, RowMaterial<false>> : normals_pixel_kernel<false, RowMaterial<false>>;
    hipLaunchKernelGGL(kernel, dim3(pl.blocks), dim3(64 * kRenderWaves), 0, s, RowArgs{sh.z}, normals, mask, Bn, sh.envmap, pl.view, image, alpha, B, H, W, pl.EH,
                       pl.EW, sh.quad);
  }
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

int launch_brdf_eval(const float* z, int z_rows, const float* n, const float* v, const float* l, float* out, long long N, hipStream_t s) {
  DRM_REQUIRE(N >= 0, "brdf_eval: N >= 0");
  if (N == 0) return DRM_OK;
  DRM_REQUIRE(z && n && v && l && out, "brdf_eval: null pointer");
  DRM_REQUIRE(z_rows == 1 || (long long)z_rows == N, "brdf_eval: z has 1 or N rows");
  const long long blocks = std::min<long long>((N + 255) / 256, 65536);
  hipLaunchKernelGGL(brdf_eval_kernel, dim3((unsigned)blocks), dim3(256), 0, s, z, z_rows, n, v, l, out, N);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

}  // namespace drm
