// The validation losses of DRMNet.p_losses in eval mode (reference models/drmnet.py:398-450, get_brdf_out :390-396, the power of
// get_schedule :494-496) as two launches without a host synchronisation:
//   1. refmap_loss_partial_kernel: every block sums |d| or d^2, d = model_out - (Lr_km1 - Lr_k), over its share of the rows with K != 0 (the
//      rows are selected, not weighted: a masked row is never loaded, so the NaN the dataset writes there cannot reach the sum) into one
//      fp64 partial;
//   2. loss_finalize_kernel: one block adds the partials in a fixed order, counts the selected rows, evaluates the two code losses
//      (B x P elements) and writes [loss_refmap, loss_refcode, loss] as fp32.
// Element arithmetic and every sum are fp64, each thread and each tree in a fixed order and no atomics: two calls are bitwise equal.
#include <cmath>

#include "common.h"

namespace drm {

namespace {

constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 256;  // fp64 partials the workspace holds

__device__ __forceinline__ double loss_term(double d, int l2) { return l2 ? d * d : fabs(d); }

// fixed tree over the 256 threads of a block; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = kLossThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kLossThreads) void refmap_loss_partial_kernel(const float* __restrict__ model_out, const float* __restrict__ Lr_k,
                                                                           const float* __restrict__ Lr_km1, const int32_t* __restrict__ K,
                                                                           long long per_row, long long total, int l2,
                                                                           double* __restrict__ partial) {
  __shared__ double sh[kLossThreads];
  double acc = 0.0;
  for (long long e = (long long)blockIdx.x * kLossThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kLossThreads) {
    if (K[e / per_row] == 0) continue;
    acc += loss_term((double)model_out[e] - ((double)Lr_km1[e] - (double)Lr_k[e]), l2);
  }
  const double sum = block_sum(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kLossThreads) void loss_finalize_kernel(const double* __restrict__ partial, int n_partial, const int32_t* __restrict__ K,
                                                                     const float* __restrict__ z_out, const float* __restrict__ z_k,
                                                                     const float* __restrict__ z_K, const int32_t* __restrict__ reversed_k,
                                                                     const float* __restrict__ z0, double ln_gamma, int l2, double w_refmap,
                                                                     double w_refcode, int B, long long per_row, int P, float* __restrict__ out) {
  __shared__ double sh[kLossThreads];
  double a_map = 0.0, a_rows = 0.0, a_zk = 0.0, a_zK = 0.0;
  for (int k = threadIdx.x; k < n_partial; k += kLossThreads) a_map += partial[k];
  for (int b = threadIdx.x; b < B; b += kLossThreads) a_rows += K[b] != 0 ? 1.0 : 0.0;
  for (long long e = threadIdx.x; e < (long long)B * P; e += kLossThreads) {
    const int b = (int)(e / P), p = (int)(e - (long long)b * P);
    // gamma^r as exp(r ln gamma) in fp64, cast to fp32 before the multiply, as get_schedule does
    const double pw = (double)(float)exp((double)reversed_k[b] * ln_gamma);
    const double zo = (double)z_out[e], a = (double)z0[p];
    const double zk_out = fmin(fmax(a + pw * (zo - a), 0.0), 1.0);
    const double zK_out = fmin(fmax(zo, 0.0), 1.0);
    a_zk += loss_term(zk_out - (double)z_k[e], l2);
    a_zK += loss_term(zK_out - (double)z_K[e], l2);
  }
  const double s_map = block_sum(a_map, sh), s_rows = block_sum(a_rows, sh), s_zk = block_sum(a_zk, sh), s_zK = block_sum(a_zK, sh);
  if (threadIdx.x == 0) {
    const double n_code = (double)B * (double)P;
    // no selected row: 0 / 0 = NaN, torch's mean of an empty selection
    const double loss_refmap = s_map / (s_rows * (double)per_row);
    const double loss_refcode = (s_zk / n_code + s_zK / n_code) / 2.0;
    out[0] = (float)loss_refmap;
    out[1] = (float)loss_refcode;
    out[2] = (float)(w_refmap * loss_refmap + w_refcode * loss_refcode);
  }
}

}  // namespace

int launch_validation_losses(const float* model_out, const float* Lr_k, const float* Lr_km1, const int32_t* K, const float* z_out, const float* z_k,
                             const float* z_K, const int32_t* reversed_k, const float* z0, double gamma, int loss_type, double w_refmap,
                             double w_refcode, int B, long long per_row, int P, double* ws, size_t ws_bytes, float* out, hipStream_t s) {
  DRM_REQUIRE(model_out && Lr_k && Lr_km1 && K && z_out && z_k && z_K && reversed_k && z0 && ws && out, "validation_losses: null pointer");
  DRM_REQUIRE(B > 0 && per_row > 0 && P > 0 && P <= 64, "validation_losses: B >= 1 rows of per_row >= 1 elements, 1 <= P <= 64");
  DRM_REQUIRE(loss_type == 0 || loss_type == 1, "validation_losses: loss_type is DRM_LOSS_L1 or DRM_LOSS_L2");
  DRM_REQUIRE(gamma > 0.0, "validation_losses: gamma > 0");
  DRM_REQUIRE(ws_bytes >= sizeof(double) * kLossMaxBlocks, "validation_losses: workspace smaller than DRM_LOSS_WORKSPACE_BYTES");
  const long long total = (long long)B * per_row;
  const int blocks = (int)std::min<long long>((total + 4 * kLossThreads - 1) / (4 * kLossThreads), kLossMaxBlocks);
  hipLaunchKernelGGL(refmap_loss_partial_kernel, dim3(blocks), dim3(kLossThreads), 0, s, model_out, Lr_k, Lr_km1, K, per_row, total, loss_type, ws);
  DRM_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(kLossThreads), 0, s, ws, blocks, K, z_out, z_k, z_K, reversed_k, z0, std::log(gamma), loss_type,
                     w_refmap, w_refcode, B, per_row, P, out);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

}  // namespace drm
