// The MERL grid as the export and the BRDF-space error sums see it (brdf_table.hip, brdf_error.hip): the directions a node stands for, which
// nodes lie above the horizon, and the value a principled row has at a node.  Stated once here so that drm_brdf_to_merl and
// drm_brdf_error_sums agree bit for bit: a row scored against its own exported table has the error 0, not a rounding of it.
#pragma once
#include "render_shared.h"

namespace drm {

constexpr int kNH = 90, kND = 90, kNP = 180;
constexpr long long kTableEntries = (long long)kNH * kND * kNP;  // float4 each
constexpr double kPi64 = 3.14159265358979323846;
constexpr double kSnap = 1e-12;  // a cosine of the export grid below this is the rounding of an exact zero (theta_h + theta_d = pi / 2, phi_d = 0)

// Node (i, j, k) = at / (90 * 180), (at / 180) % 90, at % 180: the half-vector frame has h = +z and n = (-sin theta_h, 0, cos theta_h); the
// viewer is wo = (sin theta_d cos phi_d, sin theta_d sin phi_d, cos theta_d), the light wi = wo (-1, -1, 1).  co = n.wo and ci = n.wi with
// the kSnap rule applied; g = the cosines principled_eval_at takes.
struct MerlNode {
  EvalGeom g;
  double co, ci;
};
__device__ __forceinline__ MerlNode merl_node(int at) {
  const int i = at / (kND * kNP), j = (at / kNP) % kND, k = at % kNP;
  const double t = (double)i / 90.0;
  const double th = t * t * (kPi64 / 2), td = (double)j * (kPi64 / 180), pd = (double)k * (kPi64 / 180);
  const double n[3] = {-sin(th), 0.0, cos(th)};
  const double wo[3] = {sin(td) * cos(pd), sin(td) * sin(pd), cos(td)};
  const double wi[3] = {-wo[0], -wo[1], wo[2]};
  MerlNode nd;
  nd.co = n[0] * wo[0] + n[1] * wo[1] + n[2] * wo[2];
  nd.ci = n[0] * wi[0] + n[1] * wi[1] + n[2] * wi[2];
  if (fabs(nd.co) < kSnap) nd.co = 0.0;
  if (fabs(nd.ci) < kSnap) nd.ci = 0.0;
  nd.g = eval_geom(n, wo, wi);
  return nd;
}
// below the horizon: the entry is -1
__device__ __forceinline__ bool merl_node_below(const MerlNode& nd) { return nd.co < 0.0 || nd.ci < 0.0; }
// both cosines strictly positive: the entry is a BRDF value (elsewhere above the horizon it is 0)
__device__ __forceinline__ bool merl_node_lit(const MerlNode& nd) { return nd.co > 0.0 && nd.ci > 0.0; }
// what drm_brdf_to_merl stores at a lit node for the row p: principled_eval in fp64 (its fp32 result), divided by n.wi, rounded to fp32
__device__ __forceinline__ void merl_entry(const Principled& p, const MerlNode& nd, float e[3]) {
  float f[3];
  principled_eval_at(p, nd.g, f);
  e[0] = (float)((double)f[0] / nd.ci);
  e[1] = (float)((double)f[1] / nd.ci);
  e[2] = (float)((double)f[2] / nd.ci);
}

}  // namespace drm
