// Look-ahead true-peak limiter on the device (include/svs_hip.h; the float64 definition is svs_unet_pytorch_amd/limiter.py): the
// envelope of all written rows, the gain curve, and its application.  The reference has no limiter: it peak-normalises every written
// stem (data.py:162-166), so one transient sets the level of a whole file.
//
// svs_limiter_envelope: a block owns TP_BLOCK samples and walks over the rows.  Each row's tile is staged with its halo by
// true_peak.h's tp_stage, and the per-phase accumulators are tp_phase's, so max_i e[i] is bitwise svs_true_peaks' largest true peak.
// A lane keeps the running maximum of its eight samples in registers over the rows: one store per sample, no atomics.
//
// svs_limiter_curve: a block owns LC_TILE outputs and stages r over [t0 - 2h, t0 + LC_TILE + 2h) in LDS.  The sliding minimum is
// taken by doubling: after the pass with shift s, v[l] = min r[l .. l + 2s); floor(log2(2h+1)) passes give windows of P = 2^p
// samples, and one more pass m[l] = min(v[l], v[l + 2h+1 - P]) covers 2h+1 samples by two overlapping windows: ceil(log2(2h+1))
// passes of one min per element instead of 2h+1 reads per output.  Every pass reads into registers, synchronises, writes back,
// synchronises (in place without a race).  For the smoothing a lane owns LC_PER = 8 consecutive outputs and slides an 8-sample
// register window along m: one LDS read feeds eight fmaf.  Lanes are then 8 words apart, which would put 32 lanes on 4 banks; the
// array is stored with one word of padding after every 8 (LC_PAD), so the lanes are 9 words apart and a 32-lane group hits 32
// different banks.  The passes with unit stride pay a 2-way conflict on 4 of 32 banks for it.  min is order-independent and every
// output has one fixed fmaf order: the curve is bitwise reproducible.
//
// svs_limiter_apply: x[row][i] *= g[i], 16-byte loads and stores where x, ld_row and g allow, scalar otherwise.
#include <cmath>

#include "internal.h"
#include "true_peak.h"

#define LC_THREADS 256
#define LC_PER 8
#define LC_TILE (LC_THREADS * LC_PER)
#define LC_H_MAX 1024
#define LC_PAD(l) ((l) + ((l) >> 3))
#define LC_MAX_ELEMS ((LC_TILE + 4 * LC_H_MAX + LC_THREADS - 1) / LC_THREADS)      // elements of the staged array per lane
#define LA_THREADS 256
#define LIM_MAX_ROWS 64

// ------------------------------------------------------------------------------------------------
// envelope
// ------------------------------------------------------------------------------------------------
template <int F>
__global__ __launch_bounds__(TP_THREADS) void limiter_envelope_kernel(const float* __restrict__ x, int rows, int channels, long n, long ld_stem,
                                                                      long ld_ch, const float* __restrict__ taps, float* __restrict__ e) {
  __shared__ __attribute__((aligned(16))) float sx[TP_LDS];
  __shared__ float st[12 * F + 1];
  const int tid = threadIdx.x;
  const long b0 = (long)blockIdx.x * TP_BLOCK;
  if (F > 1 && tid < 12 * F + 1) st[tid] = taps[tid];
  float env[TP_PER];
#pragma unroll
  for (int j = 0; j < TP_PER; ++j) env[j] = 0.f;
  for (int row = 0; row < rows; ++row) {
    const float* xr = x + (long)(row / channels) * ld_stem + (long)(row % channels) * ld_ch;
    if (row) __syncthreads();                                     // every lane has read the tile of the row before
    tp_stage(sx, xr, b0, n, tid);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TP_PER / 4; ++q) {
      const int s0 = 4 * (tid + q * TP_THREADS);
      if (b0 + s0 >= n) break;
      float r[20];
      tp_window(sx, s0, r);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        float v = fabsf(r[TP_ORIGIN + d]);
#pragma unroll
        for (int p = 1; p < F; ++p) v = fmaxf(v, fabsf(tp_phase<F>(st, r, d, p)));
        env[4 * q + d] = fmaxf(env[4 * q + d], v);
      }
    }
  }
  const bool vec = (((uintptr_t)e) & 15u) == 0;
#pragma unroll
  for (int q = 0; q < TP_PER / 4; ++q) {
    const long i = b0 + 4 * (tid + q * TP_THREADS);
    if (i >= n) break;
    if (vec && i + 3 < n) {
      *reinterpret_cast<float4*>(e + i) = make_float4(env[4 * q], env[4 * q + 1], env[4 * q + 2], env[4 * q + 3]);
    } else {
#pragma unroll
      for (int d = 0; d < 4; ++d)
        if (i + d < n) e[i + d] = env[4 * q + d];
    }
  }
}

extern "C" int svs_limiter_envelope(const float* x, int stems, int channels, int64_t n, int64_t ld_stem, int64_t ld_ch, const float* taps,
                                    int factor, float* e, hipStream_t stream) {
  SVS_REQUIRE(stems >= 1 && stems <= 8, "svs_limiter_envelope: stems must be in 1..8, got %d", stems);
  SVS_REQUIRE(channels >= 1 && channels <= 8, "svs_limiter_envelope: channels must be in 1..8, got %d", channels);
  SVS_REQUIRE(n >= 0 && n <= (INT64_MAX / 16), "svs_limiter_envelope: n must not be negative, got %lld", (long long)n);
  SVS_REQUIRE(ld_ch >= n, "svs_limiter_envelope: ld_ch must be at least n = %lld, got %lld", (long long)n, (long long)ld_ch);
  SVS_REQUIRE(stems == 1 || ld_stem >= ld_ch * (channels - 1) + n, "svs_limiter_envelope: ld_stem must be at least a stem's %lld samples, got %lld",
              (long long)(ld_ch * (channels - 1) + n), (long long)ld_stem);
  SVS_REQUIRE(factor == 1 || factor == 2 || factor == 4, "svs_limiter_envelope: factor must be 1, 2 or 4, got %d", factor);
  const long nblk = (long)((n + TP_BLOCK - 1) / TP_BLOCK);
  SVS_REQUIRE(nblk < (1L << 31), "svs_limiter_envelope: %ld blocks do not fit a grid", nblk);
  SVS_REQUIRE(n == 0 || (x && e && (taps || factor == 1)), "svs_limiter_envelope: null pointer");
  SVS_REQUIRE((((uintptr_t)x) & 3u) == 0 && (((uintptr_t)e) & 3u) == 0, "svs_limiter_envelope: x and e must be 4-byte aligned");
  if (n == 0) return SVS_OK;
  const int rows = stems * channels;
  const dim3 grid((unsigned)nblk);
  if (factor == 1) {
    hipLaunchKernelGGL((limiter_envelope_kernel<1>), grid, dim3(TP_THREADS), 0, stream, x, rows, channels, (long)n, (long)ld_stem, (long)ld_ch, taps, e);
  } else if (factor == 2) {
    hipLaunchKernelGGL((limiter_envelope_kernel<2>), grid, dim3(TP_THREADS), 0, stream, x, rows, channels, (long)n, (long)ld_stem, (long)ld_ch, taps, e);
  } else {
    hipLaunchKernelGGL((limiter_envelope_kernel<4>), grid, dim3(TP_THREADS), 0, stream, x, rows, channels, (long)n, (long)ld_stem, (long)ld_ch, taps, e);
  }
  SVS_CHECK_LAUNCH("limiter envelope");
  return SVS_OK;
}

// ------------------------------------------------------------------------------------------------
// gain curve
// ------------------------------------------------------------------------------------------------
// r of one envelope value: 1 where G e <= C (fp64 product), else (float)(C / (G (double)e)): one fp64 division, one rounding
__device__ __forceinline__ float lc_demand(float e, double G, double C, bool on) {
  if (!on) return 1.f;
  const double d = __dmul_rn(G, (double)e);
  return d <= C ? 1.f : (float)(C / d);
}

__global__ __launch_bounds__(LC_THREADS) void limiter_curve_kernel(const float* __restrict__ e, long n, double G, const double* __restrict__ G_dev,
                                                                   double C, const float* __restrict__ window, int h, float* __restrict__ g) {
  extern __shared__ float sv[];                                   // LC_PAD(LC_TILE + 4 h) floats
  const int tid = threadIdx.x;
  const long t0 = (long)blockIdx.x * LC_TILE;
  const int W = 2 * h + 1;
  const int total = LC_TILE + 4 * h;                              // sv index l holds sample t0 - 2h + l
  if (G_dev) G = G_dev[0];
  const bool on = G > 0.0 && G < INFINITY;                        // NaN, 0, negative, +-inf: no limiting
  for (int l = tid; l < total; l += LC_THREADS) {
    const long i = t0 - 2L * h + l;
    sv[LC_PAD(l)] = (i >= 0 && i < n) ? lc_demand(e[i], G, C, on) : 1.f;
  }
  __syncthreads();
  float tmp[LC_MAX_ELEMS];
  int s = 1;
  for (; 2 * s <= W; s *= 2) {                                    // v[l] = min r[l .. l + 2s) afterwards
#pragma unroll
    for (int j = 0; j < LC_MAX_ELEMS; ++j) {
      const int l = tid + j * LC_THREADS;
      if (l < total) {
        const float a = sv[LC_PAD(l)];
        tmp[j] = l + s < total ? fminf(a, sv[LC_PAD(l + s)]) : a;  // past the end: never read into a result
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LC_MAX_ELEMS; ++j) {
      const int l = tid + j * LC_THREADS;
      if (l < total) sv[LC_PAD(l)] = tmp[j];
    }
    __syncthreads();
  }
  // s = P, the largest power of two <= W.  m of sample t0 - h + l = min r[l .. l + W) = min(v[l], v[l + W - P]) for l < LC_TILE + 2h
  const int span = LC_TILE + 2 * h;
  const int shift = W - s;
#pragma unroll
  for (int j = 0; j < LC_MAX_ELEMS; ++j) {
    const int l = tid + j * LC_THREADS;
    if (l < span) tmp[j] = fminf(sv[LC_PAD(l)], sv[LC_PAD(l + shift)]);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < LC_MAX_ELEMS; ++j) {
    const int l = tid + j * LC_THREADS;
    if (l < span) sv[LC_PAD(l)] = tmp[j];
  }
  __syncthreads();
  // a of output o = sum_kk window[kk] m[o + kk] in sv's indices; win holds m[o0 + kk .. o0 + kk + 8), rotated through 8 registers
  const int o0 = LC_PER * tid;
  if (t0 + o0 >= n) return;
  float acc[LC_PER], win[LC_PER];
#pragma unroll
  for (int j = 0; j < LC_PER; ++j) acc[j] = 0.f;
#pragma unroll
  for (int j = 0; j < LC_PER - 1; ++j) win[j] = sv[LC_PAD(o0 + j)];
  for (int kk = 0; kk < W; kk += LC_PER) {
#pragma unroll
    for (int u = 0; u < LC_PER; ++u) {
      if (kk + u < W) {                                           // uniform
        const float wk = window[kk + u];
        win[(LC_PER - 1 + u) % LC_PER] = sv[LC_PAD(o0 + kk + u + LC_PER - 1)];
#pragma unroll
        for (int j = 0; j < LC_PER; ++j) acc[j] = fmaf(wk, win[(j + u) % LC_PER], acc[j]);
      }
    }
  }
  float out[LC_PER];
#pragma unroll
  for (int j = 0; j < LC_PER; ++j) {
    const long i = t0 + o0 + j;
    out[j] = i < n ? fminf(acc[j], lc_demand(e[i], G, C, on)) : 1.f;
  }
  const long i0 = t0 + o0;
  if ((((uintptr_t)g) & 15u) == 0 && i0 + LC_PER <= n) {
    *reinterpret_cast<float4*>(g + i0) = make_float4(out[0], out[1], out[2], out[3]);
    *reinterpret_cast<float4*>(g + i0 + 4) = make_float4(out[4], out[5], out[6], out[7]);
  } else {
#pragma unroll
    for (int j = 0; j < LC_PER; ++j)
      if (i0 + j < n) g[i0 + j] = out[j];
  }
}

extern "C" int svs_limiter_curve(const float* e, int64_t n, double G, const double* G_dev, double ceiling, const float* window, int h, float* g,
                                 hipStream_t stream) {
  SVS_REQUIRE(n >= 0 && n <= (INT64_MAX / 16), "svs_limiter_curve: n must not be negative, got %lld", (long long)n);
  SVS_REQUIRE(h >= 1 && h <= LC_H_MAX, "svs_limiter_curve: h must be in 1..%d, got %d", LC_H_MAX, h);
  SVS_REQUIRE(ceiling > 0.0 && ceiling < INFINITY, "svs_limiter_curve: the ceiling must be positive and finite, got %g", ceiling);
  const long nblk = (long)((n + LC_TILE - 1) / LC_TILE);
  SVS_REQUIRE(nblk < (1L << 31), "svs_limiter_curve: %ld blocks do not fit a grid", nblk);
  SVS_REQUIRE(window && (n == 0 || (e && g)), "svs_limiter_curve: null pointer");
  SVS_REQUIRE((((uintptr_t)e) & 3u) == 0 && (((uintptr_t)g) & 3u) == 0 && (((uintptr_t)window) & 3u) == 0 && (((uintptr_t)G_dev) & 7u) == 0,
              "svs_limiter_curve: e, g and window must be 4-byte aligned, G_dev 8-byte aligned");
  if (n == 0) return SVS_OK;
  const size_t lds = (size_t)(LC_PAD(LC_TILE + 4 * h) + 1) * sizeof(float);
  hipLaunchKernelGGL(limiter_curve_kernel, dim3((unsigned)nblk), dim3(LC_THREADS), lds, stream, e, (long)n, G, G_dev, ceiling, window, h, g);
  SVS_CHECK_LAUNCH("limiter curve");
  return SVS_OK;
}

// ------------------------------------------------------------------------------------------------
// apply
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LA_THREADS) void limiter_apply_kernel(float* __restrict__ x, long n, long ld_row, const float* __restrict__ g, int vec) {
  float* xr = x + (long)blockIdx.y * ld_row;
  const long i = ((long)blockIdx.x * LA_THREADS + threadIdx.x) * 4;
  if (i >= n) return;
  if (vec && i + 3 < n) {
    float4 v = *reinterpret_cast<const float4*>(xr + i);
    const float4 q = *reinterpret_cast<const float4*>(g + i);
    v.x *= q.x; v.y *= q.y; v.z *= q.z; v.w *= q.w;
    *reinterpret_cast<float4*>(xr + i) = v;
  } else {
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (i + d < n) xr[i + d] *= g[i + d];
  }
}

extern "C" int svs_limiter_apply(float* x, int rows, int64_t n, int64_t ld_row, const float* g, hipStream_t stream) {
  SVS_REQUIRE(rows >= 1 && rows <= LIM_MAX_ROWS, "svs_limiter_apply: rows must be in 1..%d, got %d", LIM_MAX_ROWS, rows);
  SVS_REQUIRE(n >= 0 && n <= (INT64_MAX / 16), "svs_limiter_apply: n must not be negative, got %lld", (long long)n);
  SVS_REQUIRE(ld_row >= n, "svs_limiter_apply: ld_row must be at least n = %lld, got %lld", (long long)n, (long long)ld_row);
  const long nblk = (long)((n + 4L * LA_THREADS - 1) / (4L * LA_THREADS));
  SVS_REQUIRE(nblk < (1L << 31), "svs_limiter_apply: %ld blocks do not fit a grid", nblk);
  SVS_REQUIRE(n == 0 || (x && g), "svs_limiter_apply: null pointer");
  SVS_REQUIRE((((uintptr_t)x) & 3u) == 0 && (((uintptr_t)g) & 3u) == 0, "svs_limiter_apply: x and g must be 4-byte aligned");
  if (n == 0) return SVS_OK;
  const int vec = svs_aligned16(x) && svs_aligned16(g) && ld_row % 4 == 0;
  hipLaunchKernelGGL(limiter_apply_kernel, dim3((unsigned)nblk, (unsigned)rows), dim3(LA_THREADS), 0, stream, x, (long)n, (long)ld_row, g, vec);
  SVS_CHECK_LAUNCH("limiter apply");
  return SVS_OK;
}
