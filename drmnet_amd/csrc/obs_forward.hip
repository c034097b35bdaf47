// The validation pass of ObsNetDiffusion around its one network forward (reference models/obsnet.py, ldm/models/diffusion/ddpm.py):
//   obs_forward_kernel: the forward process of a batch in ONE elementwise launch -- the masked, jittered, noise-padded conditioning of
//     get_input (models/obsnet.py:375-398) and q_sample (ddpm.py:288-294):
//       cond    = mask x  [+ noisy_observe e1]  [+ (1 - mask) e2]
//       x_noisy = sqrt_alphas_cumprod[t_b] x + sqrt_one_minus_alphas_cumprod[t_b] e3,      noise = e3
//     e1, e2, e3: injected tensors, or elements [0, n), [n, 2n), [2n, 3n) of the Philox stream of `seed` (n = B C H W; the reference's draw order).
//   diffusion_loss_partial_kernel + diffusion_loss_finalize_kernel: p_losses in eval mode after the network (models/obsnet.py:469-498), built as
//     losses.hip is: fp64 partial sums on a (parts, B) grid, then one block that folds every row's partials in a fixed order, forms the per-row
//     loss L_b and the three scalars.  No atomics, no host synchronisation; two calls are bitwise equal.
// Both passes are HBM-bound (a few floats per element): the row is blockIdx.y, so t_b and its table entries are scalar loads, and a thread moves
// four consecutive floats at a time (one 16-byte access where the pointers and the plane size allow it).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "philox.h"

namespace drm {

namespace {

constexpr int kObsThreads = 256;
constexpr int kDiffLossMaxParts = 32;    // DRM_DIFFUSION_LOSS_MAX_PARTS
constexpr int kDiffLossQuadsPerThread = 2;  // a part covers up to 256 x 2 quads before the rows get more parts

struct Quad {
  float v[4];
};

// four consecutive floats at p[0..3]: one 16-byte load (VEC: p is 16-byte aligned and all four exist), else up to `n` scalar loads (rest = 0)
template <bool VEC>
__device__ __forceinline__ Quad load_quad(const float* __restrict__ p, int n) {
  Quad q;
  if (VEC) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    q.v[0] = f.x; q.v[1] = f.y; q.v[2] = f.z; q.v[3] = f.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) q.v[k] = k < n ? p[k] : 0.f;
  }
  return q;
}

template <bool VEC>
__device__ __forceinline__ void store_quad(float* __restrict__ p, const Quad& q, int n) {
  if (VEC) {
    *reinterpret_cast<float4*>(p) = make_float4(q.v[0], q.v[1], q.v[2], q.v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) p[k] = q.v[k];
  }
}

// a draw of stream `stream` (0 observe, 1 padding, 2 q-noise): the injected tensor, or elements stream * n_total + g .. + 3 of Philox(seed)
template <bool VEC>
__device__ __forceinline__ Quad draw_quad(const float* __restrict__ inj, long long g, int n, uint64_t seed, uint64_t stream_off) {
  if (inj) return load_quad<VEC>(inj + g, n);
  Quad q;
  const uint64_t e = stream_off + (uint64_t)g;
  if (VEC) {  // (n_total and g are multiples of 4 here: the four elements share one counter)
    const float4 f = philox_normal4(seed, e >> 2);
    q.v[0] = f.x; q.v[1] = f.y; q.v[2] = f.z; q.v[3] = f.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) q.v[k] = k < n ? philox_normal1(seed, e + k) : 0.f;
  }
  return q;
}

// grid (ceil(per_row / 4 / 256), B).  VEC: hw % 4 == 0 and every pointer 16-byte aligned, so a quad never leaves its channel plane.
template <bool VEC>
__global__ __launch_bounds__(kObsThreads) void obs_forward_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                                  const int32_t* __restrict__ t, const float* __restrict__ sqrt_ac,
                                                                  const float* __restrict__ sqrt_1mac, int T, float noisy_observe, int pad_noise,
                                                                  const float* __restrict__ e_obs, const float* __restrict__ e_pad,
                                                                  const float* __restrict__ e_q, uint64_t seed, float* __restrict__ cond,
                                                                  float* __restrict__ x_noisy, float* __restrict__ noise, int hw,
                                                                  long long per_row, long long n_total) {
  const int b = blockIdx.y;  // wave-uniform: t_b and its two table entries are scalar loads
  float a = 0.f, s = 0.f;
  if (x_noisy) {
    const int tb = t[b];
    const bool t_ok = tb >= 0 && tb < T;  // a step outside the tables is never looked up: its row of x_noisy is NaN
    a = t_ok ? sqrt_ac[tb] : __builtin_nanf("");
    s = t_ok ? sqrt_1mac[tb] : __builtin_nanf("");
  }
  const long long e0 = ((long long)blockIdx.x * kObsThreads + threadIdx.x) * 4;
  if (e0 >= per_row) return;
  const int n = per_row - e0 < 4 ? (int)(per_row - e0) : 4;
  const long long g = (long long)b * per_row + e0;
  const Quad xv = load_quad<VEC>(x + g, n);
  if (cond) {  // (kernel arguments: the two halves are wave-uniform branches)
    Quad mv;
    if (VEC) {
      mv = load_quad<true>(mask + (long long)b * hw + e0 % hw, 4);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) mv.v[k] = k < n ? mask[(long long)b * hw + (e0 + k) % hw] : 0.f;
    }
    const bool observe = noisy_observe > 0.f;
    Quad e1 = {}, e2 = {};
    if (observe) e1 = draw_quad<VEC>(e_obs, g, n, seed, 0);
    if (pad_noise) e2 = draw_quad<VEC>(e_pad, g, n, seed, (uint64_t)n_total);
    Quad c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float ck = mv.v[k] * xv.v[k];                        // cond = mask * LrK                            :379
      if (observe) ck = noisy_observe * e1.v[k] + ck;      // cond = noisy_observe * randn + cond          :385
      if (pad_noise) ck = ck + (1.f - mv.v[k]) * e2.v[k];  // cond += (1 - mask) * randn                   :398
      c.v[k] = ck;
    }
    store_quad<VEC>(cond + g, c, n);
  }
  if (x_noisy) {
    const Quad e3 = draw_quad<VEC>(e_q, g, n, seed, 2 * (uint64_t)n_total);
    Quad xn;
#pragma unroll
    for (int k = 0; k < 4; ++k) xn.v[k] = a * xv.v[k] + s * e3.v[k];  // q_sample                         ddpm.py:290-293
    store_quad<VEC>(x_noisy + g, xn, n);
    store_quad<VEC>(noise + g, e3, n);
  }
}

__device__ __forceinline__ double loss_term(double d, int l2) { return l2 ? d * d : fabs(d); }

// fixed tree over the 256 threads of a block; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = kObsThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// grid (parts, B): block (p, b) sums f(model_out - target) [times invmask] over the quads p, p + parts, ... of 256-quad tiles of row b, each thread
// its quads in ascending order and their four elements in order -- the same order whether a quad is one 16-byte load or four scalar ones.
// partial[(b * parts + p) * 2] = (sum f [invmask], sum invmask over the row's first channel plane).
template <bool VEC>
__global__ __launch_bounds__(kObsThreads) void diffusion_loss_partial_kernel(const float* __restrict__ model_out, const float* __restrict__ target,
                                                                             const float* __restrict__ invmask, int hw, long long per_row, int l2,
                                                                             double* __restrict__ partial) {
  __shared__ double sh[kObsThreads];
  const int b = blockIdx.y, parts = gridDim.x;
  const float* __restrict__ mo = model_out + (long long)b * per_row;
  const float* __restrict__ tg = target + (long long)b * per_row;
  const float* __restrict__ im = invmask ? invmask + (long long)b * hw : nullptr;
  double acc = 0.0, acc_m = 0.0;
  const long long quads = (per_row + 3) / 4;
  for (long long q = (long long)blockIdx.x * kObsThreads + threadIdx.x; q < quads; q += (long long)parts * kObsThreads) {
    const long long e0 = q * 4;
    const int n = per_row - e0 < 4 ? (int)(per_row - e0) : 4;
    const Quad m = load_quad<VEC>(mo + e0, n), g = load_quad<VEC>(tg + e0, n);
    Quad w = {};
    if (im) {
      if (VEC) {
        w = load_quad<true>(im + e0 % hw, 4);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w.v[k] = k < n ? im[(e0 + k) % hw] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= n) break;
      const double f = loss_term((double)m.v[k] - (double)g.v[k], l2);
      if (im) {
        acc += f * (double)w.v[k];
        if (e0 + k < hw) acc_m += (double)w.v[k];
      } else {
        acc += f;
      }
    }
  }
  const double s = block_sum(acc, sh), s_m = block_sum(acc_m, sh);
  if (threadIdx.x == 0) {
    partial[((long long)b * parts + blockIdx.x) * 2] = s;
    partial[((long long)b * parts + blockIdx.x) * 2 + 1] = s_m;
  }
}

// one block: thread i folds the partials of rows i, i + 256, ... in ascending order, forms L_b, and the three batch means go through the fixed tree
__global__ __launch_bounds__(kObsThreads) void diffusion_loss_finalize_kernel(const double* __restrict__ partial, int parts, int masked,
                                                                              const int32_t* __restrict__ t, const float* __restrict__ logvar,
                                                                              const float* __restrict__ lvlb, int T, double w_simple, double w_elbo,
                                                                              int B, long long per_row, int C, float* __restrict__ out,
                                                                              float* __restrict__ rows_out) {
  __shared__ double sh[kObsThreads];
  double a_simple = 0.0, a_vlb = 0.0, a_gamma = 0.0;
  for (int b = threadIdx.x; b < B; b += kObsThreads) {
    double s = 0.0, s_m = 0.0;
    for (int p = 0; p < parts; ++p) {
      s += partial[((long long)b * parts + p) * 2];
      s_m += partial[((long long)b * parts + p) * 2 + 1];
    }
    // masked: sum(f invmask) / (sum(invmask) C), 0 / 0 = NaN for a row without an unobserved pixel, as the reference gives      :471-473
    const double L = masked ? s / (s_m * (double)C) : s / (double)per_row;
    if (rows_out) rows_out[b] = (float)L;
    const int tb = t[b];
    const bool t_ok = tb >= 0 && tb < T;
    const double lv = t_ok ? (double)logvar[tb] : (double)__builtin_nanf(""), wv = t_ok ? (double)lvlb[tb] : (double)__builtin_nanf("");
    a_simple += L;
    a_vlb += wv * L;            // lvlb_weights[t] * loss_vlb                                                                       :493
    a_gamma += L / exp(lv) + lv;  // loss_simple / exp(logvar_t) + logvar_t                                                         :479
  }
  const double s_simple = block_sum(a_simple, sh), s_vlb = block_sum(a_vlb, sh), s_gamma = block_sum(a_gamma, sh);
  if (threadIdx.x == 0) {
    const double loss_simple = s_simple / (double)B, loss_vlb = s_vlb / (double)B;
    out[0] = (float)loss_simple;
    out[1] = (float)loss_vlb;
    out[2] = (float)(w_simple * (s_gamma / (double)B) + w_elbo * loss_vlb);
  }
}

bool aligned16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

int launch_obs_forward_process(const float* x, const float* mask, const int32_t* t, const float* sqrt_ac, const float* sqrt_1mac, int T,
                               float noisy_observe, int padding_mode, const float* e_obs, const float* e_pad, const float* e_q, uint64_t seed,
                               float* cond, float* x_noisy, float* noise, int B, int C, int H, int W, int mask_H, int mask_W, hipStream_t s) {
  DRM_REQUIRE(x && (cond || x_noisy), "obs_forward_process: null pointer (x, and at least one of cond and x_noisy)");
  DRM_REQUIRE(!cond || mask, "obs_forward_process: cond needs the mask");
  DRM_REQUIRE((x_noisy != nullptr) == (noise != nullptr), "obs_forward_process: x_noisy and noise go together");
  DRM_REQUIRE(!x_noisy || (t && sqrt_ac && sqrt_1mac && T > 0), "obs_forward_process: x_noisy needs t and the two tables of T >= 1 entries");
  DRM_REQUIRE(B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0, "obs_forward_process: 1 <= B <= 65535 rows of C x H x W >= 1 elements");
  DRM_REQUIRE(!cond || (mask_H == H && mask_W == W), "obs_forward_process: the mask must have the size of x (resize it first)");
  DRM_REQUIRE(padding_mode == 0 || padding_mode == 1, "obs_forward_process: padding_mode is DRM_PAD_ZEROS or DRM_PAD_NOISE");
  DRM_REQUIRE(noisy_observe >= 0.f, "obs_forward_process: noisy_observe >= 0");
  const int hw = H * W;
  const long long per_row = (long long)C * hw, n_total = per_row * B;
  const bool vec = hw % 4 == 0 && aligned16(x) && aligned16(mask) && aligned16(e_obs) && aligned16(e_pad) && aligned16(e_q) && aligned16(cond) &&
                   aligned16(x_noisy) && aligned16(noise);
  const long long quads = (per_row + 3) / 4;
  const dim3 grid((unsigned)((quads + kObsThreads - 1) / kObsThreads), (unsigned)B);
  if (vec)
    hipLaunchKernelGGL(obs_forward_kernel<true>, grid, dim3(kObsThreads), 0, s, x, mask, t, sqrt_ac, sqrt_1mac, T, noisy_observe, padding_mode, e_obs,
                       e_pad, e_q, seed, cond, x_noisy, noise, hw, per_row, n_total);
  else
    hipLaunchKernelGGL(obs_forward_kernel<false>, grid, dim3(kObsThreads), 0, s, x, mask, t, sqrt_ac, sqrt_1mac, T, noisy_observe, padding_mode, e_obs,
                       e_pad, e_q, seed, cond, x_noisy, noise, hw, per_row, n_total);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

int launch_diffusion_losses(const float* model_out, const float* target, const float* invmask, const int32_t* t, const float* logvar,
                            const float* lvlb, int T, int loss_type, double w_simple, double w_elbo, int B, long long per_row, int C, double* ws,
                            size_t ws_bytes, float* out, float* rows_out, hipStream_t s) {
  DRM_REQUIRE(model_out && target && t && logvar && lvlb && ws && out, "diffusion_losses: null pointer");
  DRM_REQUIRE(B > 0 && B <= 65535 && per_row > 0 && C > 0 && per_row % C == 0 && per_row / C <= 0x7fffffffLL && T > 0,
              "diffusion_losses: 1 <= B <= 65535 rows of per_row = C x HW >= 1 elements, T >= 1");
  DRM_REQUIRE(loss_type == 0 || loss_type == 1, "diffusion_losses: loss_type is DRM_LOSS_L1 or DRM_LOSS_L2");
  DRM_REQUIRE(ws_bytes >= sizeof(double) * 2 * kDiffLossMaxParts * (size_t)B, "diffusion_losses: workspace smaller than DRM_DIFFUSION_LOSS_WORKSPACE_BYTES(B)");
  const int hw = (int)(per_row / C);
  const long long quads = (per_row + 3) / 4;
  const long long per_part = (long long)kObsThreads * kDiffLossQuadsPerThread;
  const int parts = (int)std::max<long long>(1, std::min<long long>((quads + per_part - 1) / per_part, kDiffLossMaxParts));
  const bool vec = hw % 4 == 0 && aligned16(model_out) && aligned16(target) && aligned16(invmask);
  if (vec)
    hipLaunchKernelGGL(diffusion_loss_partial_kernel<true>, dim3(parts, B), dim3(kObsThreads), 0, s, model_out, target, invmask, hw, per_row, loss_type, ws);
  else
    hipLaunchKernelGGL(diffusion_loss_partial_kernel<false>, dim3(parts, B), dim3(kObsThreads), 0, s, model_out, target, invmask, hw, per_row, loss_type,
                       ws);
  DRM_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(diffusion_loss_finalize_kernel, dim3(1), dim3(kObsThreads), 0, s, ws, parts, invmask != nullptr ? 1 : 0, t, logvar, lvlb, T, w_simple,
                     w_elbo, B, per_row, C, out, rows_out);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

}  // namespace drm
