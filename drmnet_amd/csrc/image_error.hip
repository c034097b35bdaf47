// Image-space error sums: how far P pairs of images are apart on a mask (drm_image_error_sums; the host turns the sums into the figures of
// drmnet_amd/relight.py image_errors_batch, and drmnet_amd/samples.py ranks the draws of one image with them).  Each pair names an image of
// stack a, an image of stack b and a mask; the stacks are read through (batch, pixel, channel) strides, so channel-first renders and
// channel-last inputs go in as they lie in memory.  Nothing comes back to the host but [P][10] fp64 sums.
//
// Mapping.  A block is 256 threads and owns (part, pair): the pixels part * 256 + t, + 4096, + 8192, ... of that pair, thread t its own
// column of them.  kImgParts = 16 parts per pair whatever HW is.
//   walk    a thread reads its pixel's mask byte, and only where it is set the 2 x 3 floats; element arithmetic is fp64 (two log10 per
//           entry with a > 0 and b > 0), the sums stay in registers across all its pixels.  Nothing is staged in LDS: every input byte is
//           used by exactly one thread, once per pass.
//   meet    once per block: the 64 lanes of a wave meet in a fixed shuffle tree, the four waves through LDS in wave order; partial
//           [pair][part][10] goes to the workspace.
//   pass 2  the same walk again for the two sums that need the first eight finished: the scale s = AB / AA and the mean of d.  Every block
//           forms them itself from the pair's 16 first-pass parts, added in part order -- the finaliser's order, so they are the bits
//           of the finished sums -- and there is no host synchronisation and no fourth launch.  The one-pass identities BB - AB^2 / AA and
//           DD - D^2 / n cancel to about sqrt(n 2^-53) in the figures, the size of the differences a ranking of near-equal draws turns on.
// A finalising launch adds the 16 parts of every (pair, sum) in order.  The order in which a pair's pixels are added depends on (part, lane)
// alone, never on P or the pair's place: a pair scored alone, or anywhere in any list, gives the same bits; no atomics, so two calls are
// bitwise equal.
// Cost of the choice.  The images are small (128 x 128 x 3 fp32 = 196 KB a side, L2-resident after the first pair that names them): a
// launch is bound by launch latency and by the reduction tail, not by bandwidth.  So loads are plain dwords (channel-last lanes stride 12
// bytes and use every byte over the three channel loads), the second pass reads the pixels again instead of keeping them, and a 16 x 16
// image leaves all but one part idle (those blocks write zeros and leave).  16 parts give one 128 x 128 pair 64 waves; the N^2 = 4096
// pairs of the all-pairs launch fill the machine by themselves.
#include "../../include/drmnet_hip.h"
#include "common.h"

namespace drm {

namespace {

constexpr int kImgThreads = 256;
constexpr int kImgWaves = kImgThreads / 64;
constexpr int kImgParts = 16;   // DRM_IMAGE_ERROR_PARTS
constexpr int kImgSums = 10;    // DRM_IMAGE_ERROR_SUMS
constexpr int kImgFirst = 8;    // the sums of the first pass; the second adds DRM_IMAGE_ERROR_L2_SCALED and DRM_IMAGE_ERROR_DD_CENTRED
static_assert(kImgParts == DRM_IMAGE_ERROR_PARTS && kImgSums == DRM_IMAGE_ERROR_SUMS, "include/drmnet_hip.h states the workspace size");
static_assert(DRM_IMAGE_ERROR_L2_SCALED == kImgFirst && DRM_IMAGE_ERROR_DD_CENTRED == kImgFirst + 1, "the second pass owns the last two sums");

struct ImageStack {
  const float* data;
  long long batch, pixel, channel;  // strides in elements
  int count;
};

struct ImagePair {
  const float* a;
  const float* b;
  const uint8_t* mask;  // null: a triple out of range
};

__device__ inline ImagePair image_pair(const ImageStack& A, const ImageStack& B, const uint8_t* mask, int mask_count, long long HW,
                                       const int32_t* pairs, int pair) {
  const int ia = pairs[3 * pair], ib = pairs[3 * pair + 1], im = pairs[3 * pair + 2];
  ImagePair p = {nullptr, nullptr, nullptr};
  if (ia < 0 || ia >= A.count || ib < 0 || ib >= B.count || im < 0 || im >= mask_count) return p;
  p.a = A.data + ia * A.batch;
  p.b = B.data + ib * B.batch;
  p.mask = mask + im * HW;
  return p;
}

// the block's N sums meet: a fixed tree over the lanes of a wave, then the waves in order; thread s < N writes sum s
template <int N>
__device__ inline void image_meet(double (&acc)[N], double* out) {
  __shared__ double sh[kImgWaves * N];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int s = 0; s < N; ++s) acc[s] += __shfl_down(acc[s], o, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < N; ++s) sh[wave * N + s] = acc[s];
  }
  __syncthreads();
  if (tid < N) {
    double v = sh[tid];
    for (int w = 1; w < kImgWaves; ++w) v += sh[w * N + tid];
    out[tid] = v;
  }
}

__global__ __launch_bounds__(kImgThreads) void image_error_first_kernel(ImageStack A, ImageStack B, const uint8_t* __restrict__ mask, int mask_count,
                                                                        long long HW, const int32_t* __restrict__ pairs, double* __restrict__ ws) {
  const int tid = threadIdx.x, part = blockIdx.x, pair = blockIdx.y;
  double* out = ws + ((size_t)pair * kImgParts + part) * kImgSums;
  const ImagePair p = image_pair(A, B, mask, mask_count, HW, pairs, pair);
  if (!p.mask) {
    if (tid < kImgFirst) out[tid] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  double acc[kImgFirst];
#pragma unroll
  for (int s = 0; s < kImgFirst; ++s) acc[s] = 0.0;
  for (long long q = (long long)part * kImgThreads + tid; q < HW; q += (long long)kImgParts * kImgThreads) {
    if (!p.mask[q]) continue;
    acc[DRM_IMAGE_ERROR_N] += 1.0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double av = (double)p.a[q * A.pixel + ch * A.channel], bv = (double)p.b[q * B.pixel + ch * B.channel];
      acc[DRM_IMAGE_ERROR_AA] += av * av;
      acc[DRM_IMAGE_ERROR_BB] += bv * bv;
      acc[DRM_IMAGE_ERROR_AB] += av * bv;
      const double df = av - bv;
      acc[DRM_IMAGE_ERROR_L2] += df * df;
      if (av > 0.0 && bv > 0.0) {
        const double d = log10(av) - log10(bv);
        acc[DRM_IMAGE_ERROR_N_LOG] += 1.0;
        acc[DRM_IMAGE_ERROR_D] += d;
        acc[DRM_IMAGE_ERROR_DD] += d * d;
      }
    }
  }
  image_meet<kImgFirst>(acc, out);
}

// one finished first-pass sum of a pair: its parts in order (what image_error_finalize_kernel writes)
__device__ inline double image_finished(const double* ws, int pair, int sum) {
  const double* at = ws + (size_t)pair * kImgParts * kImgSums + sum;
  double v = 0.0;
  for (int part = 0; part < kImgParts; ++part) v += at[part * kImgSums];
  return v;
}

__global__ __launch_bounds__(kImgThreads) void image_error_second_kernel(ImageStack A, ImageStack B, const uint8_t* __restrict__ mask, int mask_count,
                                                                         long long HW, const int32_t* __restrict__ pairs, double* ws) {
  const int tid = threadIdx.x, part = blockIdx.x, pair = blockIdx.y;
  double* out = ws + ((size_t)pair * kImgParts + part) * kImgSums + kImgFirst;
  const ImagePair p = image_pair(A, B, mask, mask_count, HW, pairs, pair);
  if (!p.mask) {
    if (tid < kImgSums - kImgFirst) out[tid] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  // (block-uniform, from parts no block of this launch writes: the second pass writes only the last two sums of its own part)
  const double aa = image_finished(ws, pair, DRM_IMAGE_ERROR_AA), ab = image_finished(ws, pair, DRM_IMAGE_ERROR_AB);
  const double n_log = image_finished(ws, pair, DRM_IMAGE_ERROR_N_LOG), sd = image_finished(ws, pair, DRM_IMAGE_ERROR_D);
  const double scale = aa > 0.0 ? ab / aa : 0.0, mean = n_log > 0.0 ? sd / n_log : 0.0;
  double acc[kImgSums - kImgFirst] = {0.0, 0.0};
  for (long long q = (long long)part * kImgThreads + tid; q < HW; q += (long long)kImgParts * kImgThreads) {
    if (!p.mask[q]) continue;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double av = (double)p.a[q * A.pixel + ch * A.channel], bv = (double)p.b[q * B.pixel + ch * B.channel];
      const double r = scale * av - bv;
      acc[0] += r * r;
      if (av > 0.0 && bv > 0.0) {
        const double e = (log10(av) - log10(bv)) - mean;
        acc[1] += e * e;
      }
    }
  }
  image_meet<kImgSums - kImgFirst>(acc, out);
}

// one thread per (pair, sum): the parts in order
__global__ __launch_bounds__(kImgThreads) void image_error_finalize_kernel(const double* __restrict__ ws, int P, double* __restrict__ sums) {
  const int at = blockIdx.x * kImgThreads + threadIdx.x;
  if (at >= P * kImgSums) return;
  const int pair = at / kImgSums, sum = at - pair * kImgSums;
  const double* from = ws + (size_t)pair * kImgParts * kImgSums + sum;
  double v = 0.0;
  for (int part = 0; part < kImgParts; ++part) v += from[part * kImgSums];
  sums[at] = v;
}

}  // namespace

int launch_image_error_sums(const drm_image_error& g, hipStream_t s) {
  DRM_REQUIRE_SIZE(&g, drm_image_error);
  DRM_REQUIRE(g.a && g.b && g.mask && g.pairs && g.workspace && g.sums, "image_error_sums: null pointer (a, b, mask, pairs, workspace and sums are all required)");
  DRM_REQUIRE(g.P >= 1 && g.P <= 4096, "image_error_sums: P in [1, 4096] pairs");
  DRM_REQUIRE(g.HW >= 1, "image_error_sums: HW >= 1 pixels");
  DRM_REQUIRE(g.a_count >= 1 && g.b_count >= 1 && g.mask_count >= 1, "image_error_sums: a_count, b_count and mask_count must be >= 1");
  DRM_REQUIRE(g.workspace_bytes >= DRM_IMAGE_ERROR_WORKSPACE_BYTES(g.P), "image_error_sums: workspace smaller than DRM_IMAGE_ERROR_WORKSPACE_BYTES(P)");
  DRM_REQUIRE((reinterpret_cast<uintptr_t>(g.workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(g.sums) & 7) == 0,
              "image_error_sums: workspace and sums must be 8-byte aligned");
  const ImageStack A = {g.a, (long long)g.a_batch_stride, (long long)g.a_pixel_stride, (long long)g.a_channel_stride, g.a_count};
  const ImageStack B = {g.b, (long long)g.b_batch_stride, (long long)g.b_pixel_stride, (long long)g.b_channel_stride, g.b_count};
  double* ws = static_cast<double*>(g.workspace);
  const dim3 grid(kImgParts, g.P), block(kImgThreads);
  hipLaunchKernelGGL(image_error_first_kernel, grid, block, 0, s, A, B, g.mask, g.mask_count, (long long)g.HW, g.pairs, ws);
  DRM_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(image_error_second_kernel, grid, block, 0, s, A, B, g.mask, g.mask_count, (long long)g.HW, g.pairs, ws);
  DRM_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(image_error_finalize_kernel, dim3((g.P * kImgSums + kImgThreads - 1) / kImgThreads), block, 0, s, ws, g.P, g.sums);
  DRM_HIP_CHECK(hipGetLastError());
  return DRM_OK;
}

}  // namespace drm
