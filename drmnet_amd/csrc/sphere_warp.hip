// The sphere / environment-map warp family around the forward model, as one gather-and-pool kernel with a map functor per warp.
//
// Reference semantics restated (paths relative to the reference root, all in utils/transform.py):
//   thetaphi2xyz / xyz2thetaphi / normalize   :17-103   (used with assume_normalized: frame vectors are taken as given)
//   refmap2refimg_torch                       :170-198  (+ gen_sphere_normals_realcentering :147-167)
//   envmap2mirmap                             :201-242  (grid_sample on an S x S grid, then adaptive_avg_pool2d: fused here)
//   mirimg2envmap                             :245-284
//   rotate_envmap                             :317-363
// Every warp is "for each output pixel, map sample positions to (u, v) of the input, fetch with grid_sample's bilinear / border /
// align_corners=False arithmetic (grid_sample.h), average".  The frames (zenith, left edge, view, top and the binormals the reference derives
// from them) arrive as a small per-item device array [B][k][3] built by the caller in fp32; nothing about them is built into a kernel.
// Python's `%` on floats is floor-mod, x - m floor(x / m).
#include "common.h"
#include "grid_sample.h"

namespace drm {

namespace {

constexpr double PI_D = 3.14159265358979323846;

struct Vec3 {
  float x, y, z;
};
__device__ __forceinline__ Vec3 load3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ float dot3(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float floor_mod(float x, float m) { return x - m * floorf(x / m); }

// thetaphi2xyz (:48-51) about the frame f = (normal, tangent, binormal): cos(theta) n, then + (sin(theta) cos(phi)) t, then + (sin(theta) sin(phi)) b
__device__ __forceinline__ Vec3 sphere_dir(float theta, float phi, const float* f) {
  const Vec3 n = load3(f), t = load3(f + 3), b = load3(f + 6);
  const float ct = cosf(theta), st = sinf(theta);
  const float a = st * cosf(phi), c = st * sinf(phi);
  return {(ct * n.x + a * t.x) + c * b.x, (ct * n.y + a * t.y) + c * b.y, (ct * n.z + a * t.z) + c * b.z};
}
// xyz2thetaphi (:87-88) about the frame f = (normal, tangent, binormal)
__device__ __forceinline__ void dir_angles(Vec3 d, const float* f, float& theta, float& phi) {
  theta = acosf(dot3(d, load3(f)));
  phi = atan2f(dot3(d, load3(f + 6)), dot3(d, load3(f + 3)));
}
// normalize (:92-103): x / max(|x|, 1e-12)
__device__ __forceinline__ Vec3 unit(Vec3 d) {
  const float len = fmaxf(sqrtf(d.x * d.x + d.y * d.y + d.z * d.z), 1e-12f);
  return {d.x / len, d.y / len, d.z / len};
}

// A map functor turns sample (sy, sx) of item b's SH x SW sample grid into the normalised input position (u, v); false = not drawn.

// envmap2mirmap (:225-233).  frames [B][6][3]: top, view_from, their binormal (negated for flip_horizontal); envmap_zenith, envmap_left_edge,
// their binormal (negated for reverse_azimuth_envmap).  Sample (sy, sx) is the mirror-ball normal at (theta, phi) about (top, view); the
// viewing ray reflects about it and the reflected direction's (theta, phi) about the envmap frame is the texel.
struct Env2MirMap {
  const float* frames;
  float dtheta, dphi, mid;  // pi / S, pi / S, (S - 1) / 2
  float two_pi, pi, two_over_pi;
  __device__ __forceinline__ bool operator()(int b, int sy, int sx, float& u, float& v) const {
    const float* f = frames + (size_t)b * 18;
    const Vec3 n = sphere_dir(((float)sy + 0.5f) * dtheta, ((float)sx - mid) * dphi, f);
    const Vec3 view = load3(f + 3);
    const float k = 2.0f * dot3(n, view);
    float theta, phi;
    dir_angles(unit({k * n.x - view.x, k * n.y - view.y, k * n.z - view.z}), f + 9, theta, phi);
    u = floor_mod(phi, two_pi) / pi - 1.0f;
    v = theta * two_over_pi - 1.0f;
    return true;
  }
};

// rotate_envmap (:343-355).  frames [B][6][3]: target zenith, left edge, binormal; source zenith, left edge, binormal (both binormals
// negated: reverse_phi=True).  theta / phi follow torch.linspace's two-ended rule (start + step i below the middle, end - step (n - 1 - i)
// from it on).
struct RotateMap {
  const float* frames;
  int OH, OW;
  float t0, t1, tstep, p0, p1, pstep;
  float half_pi, pi;
  __device__ __forceinline__ static float linspace(int i, int n, float start, float end, float step) {
    return i < n / 2 ? start + step * (float)i : end - step * (float)(n - i - 1);
  }
  __device__ __forceinline__ bool operator()(int b, int sy, int sx, float& u, float& v) const {
    const float* f = frames + (size_t)b * 18;
    const Vec3 d = sphere_dir(linspace(sy, OH, t0, t1, tstep), linspace(sx, OW, p0, p1, pstep), f);
    float theta, phi;
    dir_angles(d, f + 9, theta, phi);
    v = theta / half_pi + -1.0f;
    u = floor_mod(phi / pi, 2.0f) - 1.0f;
    return true;
  }
};

// mirimg2envmap (:267-275).  frames [B][7][3]: envmap_zenith, envmap_left_edge, binormal (negated for reverse_azimuth); then the frame the
// half vector is measured in: top, cross(view_from, top), their binormal; then view_from.  The texel's direction plus the view is the
// mirror ball's normal there; its angles, shifted by pi / 2, give the orthographic image position (u, v) = (cos t sin p, sin t).
struct MirImgMap {
  const float* frames;
  float dtheta, dphi, half_pi;
  __device__ __forceinline__ bool operator()(int b, int sy, int sx, float& u, float& v) const {
    const float* f = frames + (size_t)b * 21;
    const Vec3 d = sphere_dir(((float)sy + 0.5f) * dtheta, ((float)sx + 0.5f) * dphi, f);
    const Vec3 view = load3(f + 18);
    float theta, phi;
    dir_angles(unit({d.x + view.x, d.y + view.y, d.z + view.z}), f + 9, theta, phi);
    theta = theta - half_pi;
    phi = phi - half_pi;
    v = sinf(theta);
    u = cosf(theta) * sinf(phi);
    return true;
  }
};

// refmap2refimg_torch (:175-193): pixel (sy, sx) of the 2 radius x 2 radius ball image; inside the disc of gen_sphere_normals_realcentering
// its normal (x, y in float64 as numpy builds them, stored and normalised in fp32) is read about normal +y, tangent -x (binormal +z).
// The functor also records the disc (item 0 writes it; every item computes the same bit).
struct RefImgMap {
  int radius;
  unsigned char* mask;  // [2 radius][2 radius] or null
  float two_over_pi;
  __device__ __forceinline__ bool operator()(int b, int sy, int sx, float& u, float& v) const {
    const double x = -(double)radius + 0.5 + (double)sx, y = (double)radius - 0.5 - (double)sy;
    const double zsq = (double)radius * (double)radius - (x * x + y * y);
    const bool inside = zsq >= 0.0;
    if (mask && b == 0) mask[(size_t)sy * (2 * radius) + sx] = inside ? 1 : 0;
    if (!inside) return false;
    float nx = (float)x, ny = (float)y, nz = (float)sqrt(zsq);
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    nx /= len; ny /= len; nz /= len;
    u = atan2f(nz, -nx) * two_over_pi - 1.0f;
    v = acosf(ny) * two_over_pi - 1.0f;
    return true;
  }
};

// LANES = 1: one thread per output pixel walks its window (one sample when nothing is pooled).  LANES = 64: one wave per output pixel, the
// lanes stride the window (consecutive lanes on consecutive sample columns, so their taps fall on neighbouring texels) and combine with a
// fixed-order xor-shuffle tree.  Either way a pixel's value depends on its own item's map and frame alone: the same bits on every run and
// in every batch.  Window (oy, ox) is adaptive_avg_pool2d's: rows [floor(oy SH / OH), ceil((oy + 1) SH / OH)), columns likewise.
// in [B][C][H][W], or [B][H][W][C] with nhwc_in; out [B][C][OH][OW].  grid (pixel blocks, items), 256 threads.
template <typename Map, int LANES>
__global__ __launch_bounds__(256) void gather_pool_kernel(Map map, const float* __restrict__ in, float* __restrict__ out, int B, int C, int H, int W,
                                                          int SH, int SW, int OH, int OW, int log_interp, int nhwc_in) {
  static_assert(LANES == 1 || LANES == 64, "a thread or a whole wave per output pixel");
  const int lane = LANES == 1 ? 0 : (int)(threadIdx.x & 63);
  const int pix = LANES == 1 ? (int)(blockIdx.x * blockDim.x + threadIdx.x) : (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (pix >= OH * OW) return;  // (wave-uniform in the wave form: the shuffles below always see all 64 lanes)
  const int oy = pix / OW, ox = pix - oy * OW;
  const int y0 = (int)((long long)oy * SH / OH), y1 = (int)(((long long)(oy + 1) * SH + OH - 1) / OH);
  const int x0 = (int)((long long)ox * SW / OW), x1 = (int)(((long long)(ox + 1) * SW + OW - 1) / OW);
  const int ww = x1 - x0, n = (y1 - y0) * ww;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    for (int c0 = 0; c0 < C; c0 += 4) {  // four channels per pass over the window (C = 3 everywhere in the project: one pass)
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      bool drawn = false;
      for (int s = lane; s < n; s += LANES) {
        const int sy = y0 + s / ww, sx = x0 + s % ww;
        float u, v;
        if (!map(b, sy, sx, u, v)) continue;
        drawn = true;
        const BilinearTaps t = grid_sample_taps(u, v, H, W);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = c0 + k;
          if (c >= C) break;
          auto at = [&](int y, int x) {
            const size_t i = nhwc_in ? (((size_t)b * H + y) * W + x) * C + c : (((size_t)b * C + c) * H + y) * W + x;
            const float e = in[i];
            return log_interp ? logf(fmaxf(e, 1e-7f)) : e;
          };
          float a = at(t.y0, t.x0) * t.w00;
          if (t.has_x1) a += at(t.y0, t.x0 + 1) * t.w01;
          if (t.has_y1) a += at(t.y0 + 1, t.x0) * t.w10;
          if (t.has_x1 && t.has_y1) a += at(t.y0 + 1, t.x0 + 1) * t.w11;
          acc[k] += a;
        }
      }
      if (LANES == 64) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], o);
        }
        drawn = __any(drawn);
      }
      if (lane != 0) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = c0 + k;
        if (c >= C) break;
        float r = acc[k] / (float)n;  // the pooled mean (in the log domain under log_interp)
        if (log_interp) r = expf(r);
        out[(((size_t)b * C + c) * OH + oy) * OW + ox] = drawn ? r : 0.0f;
      }
    }
  }
}

constexpr int MAX_SIDE = 16384;  // of an input, a sample grid or an output

template <typename Map>
int launch_gather_pool(const Map& map, const float* in, float* out, int B, int C, int H, int W, int SH, int SW, int OH, int OW, int log_interp,
                       int nhwc_in, hipStream_t s) {
  // the smallest pool window decides the form: all of a warp's windows are within one row / column of each other
  const long long min_window = (long long)(SH / OH > 0 ? SH / OH : 1) * (SW / OW > 0 ? SW / OW : 1);
  const int pixels = OH * OW;
  const dim3 items((unsigned)std::min(B, 65535));
  if (min_window >= 64)
    hipLaunchKernelGGL((gather_pool_kernel<Map, 64>), dim3((pixels + 3) / 4, items.x), dim3(256), 0, s, map, in, out, B, C, H, W, SH, SW, OH, OW,
                       log_interp, nhwc_in);
  else
    hipLaunchKernelGGL((gather_pool_kernel<Map, 1>), dim3((pixels + 255) / 256, items.x), dim3(256), 0, s, map, in, out, B, C, H, W, SH, SW, OH, OW,
                       log_interp, nhwc_in);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

bool sides_ok(int a, int b) { return a > 0 && b > 0 && a <= MAX_SIDE && b <= MAX_SIDE; }

}  // namespace

int launch_envmap2mirmap(const float* env, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int mitigate_aliasing,
                         int log_interp, int nhwc_in, hipStream_t s) {
  DRM_REQUIRE(env && frames && out, "envmap2mirmap: null pointer");
  DRM_REQUIRE(B > 0 && C > 0 && sides_ok(H, W) && sides_ok(OH, OW), "envmap2mirmap: B, C > 0 and every side in [1, 16384]");
  int SH = OH, SW = OW;
  if (mitigate_aliasing) SH = SW = OH < H ? std::min(H, W) : std::max(OH, OW);  // (:221-224)
  Env2MirMap map{frames, (float)(PI_D / SH), (float)(PI_D / SW), (float)((SW - 1) / 2.0), (float)(2 * PI_D), (float)PI_D, (float)(2 / PI_D)};
  return launch_gather_pool(map, env, out, B, C, H, W, SH, SW, OH, OW, log_interp, nhwc_in, s);
}

int launch_rotate_envmap(const float* env, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int nhwc_in, hipStream_t s) {
  DRM_REQUIRE(env && frames && out, "rotate_envmap: null pointer");
  DRM_REQUIRE(B > 0 && C > 0 && sides_ok(H, W) && sides_ok(OH, OW), "rotate_envmap: B, C > 0 and every side in [1, 16384]");
  const double hs = PI_D / OH / 2, ws = PI_D / OW;  // (:343-345; torch.linspace computes its step in fp32 from the fp32 ends)
  const float t0 = (float)hs, t1 = (float)(PI_D - hs), p0 = (float)ws, p1 = (float)(PI_D * 2 - ws);
  RotateMap map{frames, OH, OW, t0, t1, OH > 1 ? (t1 - t0) / (float)(OH - 1) : 0.f, p0, p1, OW > 1 ? (p1 - p0) / (float)(OW - 1) : 0.f,
                (float)(PI_D / 2), (float)PI_D};
  return launch_gather_pool(map, env, out, B, C, H, W, OH, OW, OH, OW, 0, nhwc_in, s);
}

int launch_mirimg2envmap(const float* img, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int log_interp, int nhwc_in,
                         hipStream_t s) {
  DRM_REQUIRE(img && frames && out, "mirimg2envmap: null pointer");
  DRM_REQUIRE(B > 0 && C > 0 && sides_ok(H, W) && sides_ok(OH, OW), "mirimg2envmap: B, C > 0 and every side in [1, 16384]");
  MirImgMap map{frames, (float)(PI_D / OH), (float)(PI_D * 2 / OW), (float)(PI_D / 2)};
  return launch_gather_pool(map, img, out, B, C, H, W, OH, OW, OH, OW, log_interp, nhwc_in, s);
}

int launch_refmap2refimg(const float* refmap, float* out, unsigned char* mask, int B, int C, int H, int W, int radius, int nhwc_in, hipStream_t s) {
  DRM_REQUIRE(refmap && out, "refmap2refimg: null pointer");
  DRM_REQUIRE(B > 0 && C > 0 && sides_ok(H, W) && radius > 0 && 2 * radius <= MAX_SIDE, "refmap2refimg: B, C > 0, every side in [1, 16384], radius in [1, 8192]");
  RefImgMap map{radius, mask, (float)(2 / PI_D)};
  const int res = 2 * radius;
  return launch_gather_pool(map, refmap, out, B, C, H, W, res, res, res, res, 0, nhwc_in, s);
}

}  // namespace drm
