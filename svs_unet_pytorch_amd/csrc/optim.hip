// Optimiser options of the training step (gfx950): the global gradient norm with its clip coefficient, and the Adam update
// with decoupled weight decay, clipping, a skip on a non-finite gradient and an exponential moving average of the weights.
// Everything the host would otherwise read back -- the norm, the coefficient, the counts -- stays in a device double[4]
// (`stats`), so a step still reads nothing from the device.  Bound: HBM (the norm reads 4n bytes, the update moves 28n, 36n
// with the average).
//
// Step count: the bias corrections of svs_adamw_step use the HOST's step count, and a skipped step still advances it (the
// host cannot know that the step was skipped without reading back).  After k skipped steps the corrections are those of
// step t + k, not t: both tend to 1, and the moments themselves are untouched by a skipped step.
#include "common.h"

#include <math.h>

#define NORM_BLOCKS 1024     // partial sums of svs_grad_norm: one double per block, four per thread of the finalise block

// a + b + c + d of the block's four waves, in a fixed order; every thread of the block must call it
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// partial[block] = sum of g[i]^2 over the block's share, each element widened to double before it is squared.  `g` is any
// 4-byte-aligned pointer: `head` (0..3) elements in front of the first 16-byte boundary and the (n - head) % 4 behind the
// last float4 are taken by the first threads of block 0; the float4 body is walked with a grid stride.  The order of the
// additions depends on (n, head) only.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long n, int head, double* __restrict__ partial) {
  __shared__ double sh[4];
  const int t = threadIdx.x;
  const long n4 = (n - head) >> 2;
  const f32x4* __restrict__ body = (const f32x4*)(g + head);
  double acc = 0.0;
  if (blockIdx.x == 0) {
    const long tail0 = head + (n4 << 2);
    if (t < head) { const double x = (double)g[t]; acc += x * x; }
    if (tail0 + t < n && t < 4) { const double x = (double)g[tail0 + t]; acc += x * x; }
  }
#pragma unroll 4
  for (long i = (long)blockIdx.x * 256 + t; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 x = body[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double d = (double)x[k]; acc += d * d; }
  }
  acc = block_sum_f64(acc, sh);
  if (t == 0) partial[blockIdx.x] = acc;
}

// One block folds the partials in a fixed tree and writes stats: [0] the norm of grad_scale * g, [1] the clip coefficient
// min(1, max_norm / (norm + 1e-6)) of torch.nn.utils.clip_grad_norm_ (1 when max_norm <= 0, 0 when the norm is not finite),
// [2] += 1 when the coefficient is below 1, [3] += 1 when the norm is not finite.
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const double* __restrict__ partial, int nb, double gscale_abs,
                                                                 double max_norm, double* __restrict__ stats) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) acc += partial[i];
  acc = block_sum_f64(acc, sh);
  if (threadIdx.x != 0) return;
  const double norm = gscale_abs * sqrt(acc);
  double coef = 1.0;
  if (!isfinite(norm)) {
    coef = 0.0;
    stats[3] = stats[3] + 1.0;
  } else if (max_norm > 0.0) {
    coef = fmin(1.0, max_norm / (norm + 1e-6));
    if (coef < 1.0) stats[2] = stats[2] + 1.0;
  }
  stats[0] = norm;
  stats[1] = coef;
}

static int norm_blocks(long n) {
  long nb = (n + 1023) / 1024;            // one float4 per thread and pass
  if (nb > NORM_BLOCKS) nb = NORM_BLOCKS;
  if (nb < 1) nb = 1;
  return (int)nb;
}

extern "C" size_t svs_grad_norm_workspace_bytes(int64_t n) { (void)n; return NORM_BLOCKS * sizeof(double); }

extern "C" int svs_grad_norm(const float* g, int64_t n, float grad_scale, double max_norm, double* stats, void* ws,
                             size_t ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(g && stats && n > 0, "svs_grad_norm: bad arguments");
  SVS_REQUIRE((((uintptr_t)g) & 3u) == 0 && (((uintptr_t)stats) & 7u) == 0 && (((uintptr_t)ws) & 7u) == 0, "svs_grad_norm: misaligned pointer");
  if (!ws || ws_bytes < svs_grad_norm_workspace_bytes(n)) { svs_set_error("svs_grad_norm: workspace too small"); return SVS_ERR_WORKSPACE; }
  long head = (long)(((16u - (unsigned)(((uintptr_t)g) & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  const int nb = norm_blocks(n);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nb), dim3(256), 0, stream, g, (long)n, (int)head, (double*)ws);
  SVS_CHECK_LAUNCH("grad_sumsq");
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, stream, (const double*)ws, nb, fabs((double)grad_scale),
                     max_norm, stats);
  SVS_CHECK_LAUNCH("grad_norm_finalize");
  return SVS_OK;
}

// adam_kernel of elementwise.hip (the same expressions in the same order, so that with no decay the parameters and moments
// are bit for bit its own at grad_scale = gs) with: a skip when stats[1] == 0, the clip coefficient folded into the one float
// gs, p *= decay in front of the update (torch.optim.AdamW) and ema = d * ema + (1 - d) * p behind it.
template <bool DECAY, bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, float b1, float b2, float omb1, float omb2,
                                                    float eps, float step_size, float bc2_sqrt, float gscale, float decay,
                                                    const double* __restrict__ stats, float* __restrict__ ema, float ed, float omed) {
  float gs = gscale;
  if (stats) {
    const double coef = stats[1];        // one value for the whole grid: the branch is uniform
    if (coef == 0.0) return;
    gs = gscale * (float)coef;
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float gi = g[i] * gs;
    const float mi = m[i] * b1 + omb1 * gi;
    const float vi = v[i] * b2 + omb2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    float pi = p[i];
    if (DECAY) pi *= decay;
    pi -= step_size * (mi / denom);
    p[i] = pi;
    if (EMA) ema[i] = ed * ema[i] + omed * pi;
  }
}

extern "C" int svs_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                              double eps, int step, float grad_scale, double weight_decay, const double* stats, float* ema,
                              double ema_decay, hipStream_t stream) {
  SVS_REQUIRE(p && g && m && v && n > 0 && step >= 1, "svs_adamw_step: bad arguments");
  SVS_REQUIRE(weight_decay >= 0.0 && ema_decay >= 0.0 && ema_decay < 1.0, "svs_adamw_step: weight_decay %g must be >= 0, ema_decay %g in [0, 1)",
              weight_decay, ema_decay);
  SVS_REQUIRE((((uintptr_t)stats) & 7u) == 0, "svs_adamw_step: misaligned stats");
  const double bc1 = 1.0 - pow(beta1, step);
  const double bc2 = 1.0 - pow(beta2, step);
  long grid = (n + 255) / 256;
  if (grid > 4096) grid = 4096;
  const bool decay = weight_decay != 0.0;
  auto kernel = decay ? (ema ? adamw_kernel<true, true> : adamw_kernel<true, false>)
                      : (ema ? adamw_kernel<false, true> : adamw_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((int)grid), dim3(256), 0, stream, p, g, m, v, (long)n, (float)beta1, (float)beta2,
                     (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)(lr / bc1), (float)sqrt(bc2), grad_scale,
                     (float)(1.0 - lr * weight_decay), stats, ema, (float)ema_decay, (float)(1.0 - ema_decay));
  SVS_CHECK_LAUNCH("adamw");
  return SVS_OK;
}
