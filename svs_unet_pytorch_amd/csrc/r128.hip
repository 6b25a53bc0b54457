// The rest of the EBU R 128 meter on the device (include/svs_hip.h; the float64 definitions are svs_unet_pytorch_amd/loudness.py):
// the maximum momentary and short-term loudness and the loudness range (EBU Tech 3341 / 3342) from the window energies of
// svs_loudness_series, and the true peak (ITU-R BS.1770-4 Annex 2: the peak of the over-sampled signal) of planar fp32 rows.  The
// reference peak-normalises every written stem to its SAMPLE peak (data.py:162-166) and has no meter.
//
// svs_loudness_stats is one block.  The two percentiles of the loudness range are exact selections: a positive double orders as its
// 64-bit pattern, so the value of rank r among the gated windows is the largest 64-bit v with  #(keys < v) <= r,  found bit by bit
// from the top (64 counting passes over the keys, both ranks in the same pass).  The keys are the gated windows' bit patterns, all
// ones where the gates dropped a window, written to the workspace once.  Counts are integers, so their order does not matter; the
// gate's sum is one fixed tree.  No atomics, nothing returns to the host.
//
// svs_true_peaks is one launch over (blocks of TP_BLOCK samples) x rows and one reduce launch.  A block stages its samples and a
// 6-sample halo each side in LDS from 16-byte loads (scalar at the row's ends and where a vector straddles them).  A lane takes four
// consecutive samples at a time: five 16-byte LDS reads give it their 15-sample window in registers (lanes 16 bytes apart: no bank
// conflict), against 13 scalar reads per sample.  It forms the factor - 1 interpolated values that follow each of its samples,
// acc = fmaf(taps[p + f k], x[i + 6 - k], acc) in ascending k.  max is order-independent: the result is bitwise reproducible however
// the blocks are scheduled.
#include <cmath>

#include "internal.h"
#include "true_peak.h"                       // TP_*: the staging and the phase accumulator, shared with limiter.hip

#define ST_THREADS 1024
#define TP_MAX_ROWS 64

// ------------------------------------------------------------------------------------------------
// maxima and loudness range
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double st_lufs(double z) { return -0.691 + 10.0 * log10(z); }      // loud_gain_kernel's expression

// a over the block by one fixed tree (sum) or by max; every lane gets the result
template <bool MAX>
__device__ __forceinline__ double st_block_reduce(double* sh, double a) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = a;
  __syncthreads();
#pragma unroll
  for (int o = ST_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) sh[tid] = MAX ? fmax(sh[tid], sh[tid + o]) : sh[tid] + sh[tid + o];
    __syncthreads();
  }
  return sh[0];
}

__device__ __forceinline__ void st_block_count2(unsigned* sh, unsigned& a, unsigned& b) {   // two integer sums over the block
  const int tid = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  __syncthreads();
  if ((tid & 63) == 0) { sh[tid >> 6] = a; sh[16 + (tid >> 6)] = b; }
  __syncthreads();
  a = 0;
  b = 0;
#pragma unroll
  for (int i = 0; i < ST_THREADS / 64; ++i) { a += sh[i]; b += sh[16 + i]; }
}

__global__ __launch_bounds__(ST_THREADS) void loud_stats_kernel(const double* __restrict__ z_m, long n_m, const double* __restrict__ z_s, long n_s,
                                                                double* __restrict__ stats, unsigned long long* __restrict__ keys) {
  __shared__ double sh[ST_THREADS];
  __shared__ unsigned shc[32];
  const int tid = threadIdx.x;
  double mm = 0.0, ms = 0.0, sum = 0.0, cnt = 0.0;
  for (long j = tid; j < n_m; j += ST_THREADS) mm = fmax(mm, z_m[j]);
  for (long j = tid; j < n_s; j += ST_THREADS) {                 // absolute gate
    const double v = z_s[j];
    ms = fmax(ms, v);
    if (st_lufs(v) > -70.0) { sum += v; cnt += 1.0; }
  }
  mm = st_block_reduce<true>(sh, mm);
  ms = st_block_reduce<true>(sh, ms);
  sum = st_block_reduce<false>(sh, sum);
  cnt = st_block_reduce<false>(sh, cnt);
  const double gamma = cnt > 0.0 ? st_lufs(sum / cnt) - 20.0 : INFINITY;
  unsigned kept = 0, unused = 0;
  for (long j = tid; j < n_s; j += ST_THREADS) {                 // both gates; a lane reads back only the keys it wrote
    const double v = z_s[j];
    const double l = st_lufs(v);
    const bool keep = l > -70.0 && l > gamma;
    keys[j] = keep ? (unsigned long long)__double_as_longlong(v) : ~0ull;
    kept += keep ? 1u : 0u;
  }
  st_block_count2(shc, kept, unused);
  unsigned long long lo = 0, hi = 0;
  if (kept > 0) {
    const unsigned r_lo = (unsigned)floor(__dadd_rn(__dmul_rn((double)(kept - 1), 0.10), 0.5));
    const unsigned r_hi = (unsigned)floor(__dadd_rn(__dmul_rn((double)(kept - 1), 0.95), 0.5));
    for (int b = 63; b >= 0; --b) {
      const unsigned long long c_lo = lo | (1ull << b), c_hi = hi | (1ull << b);
      unsigned n_lo = 0, n_hi = 0;
      for (long j = tid; j < n_s; j += ST_THREADS) {
        const unsigned long long k = keys[j];
        n_lo += k < c_lo ? 1u : 0u;
        n_hi += k < c_hi ? 1u : 0u;
      }
      st_block_count2(shc, n_lo, n_hi);
      if (n_lo <= r_lo) lo = c_lo;                                // uniform over the block
      if (n_hi <= r_hi) hi = c_hi;
    }
  }
  if (tid != 0) return;
  const double z_lo = kept > 0 ? __longlong_as_double((long long)lo) : 0.0;
  const double z_hi = kept > 0 ? __longlong_as_double((long long)hi) : 0.0;
  const double l_lo = kept > 0 ? st_lufs(z_lo) : -INFINITY, l_hi = kept > 0 ? st_lufs(z_hi) : -INFINITY;
  stats[0] = n_m > 0 ? st_lufs(mm) : -INFINITY;
  stats[1] = n_s > 0 ? st_lufs(ms) : -INFINITY;
  stats[2] = kept > 0 ? l_hi - l_lo : 0.0;
  stats[3] = (double)kept;
  stats[4] = l_lo;
  stats[5] = l_hi;
  stats[6] = z_lo;
  stats[7] = z_hi;
}

#define ST_MAX_N (1L << 31)                  // the kept count is a 32-bit integer

extern "C" size_t svs_loudness_stats_workspace_bytes(int64_t n_s) {
  if (n_s < 0 || n_s >= ST_MAX_N) return 0;
  return n_s ? (size_t)n_s * sizeof(unsigned long long) : 64;
}

extern "C" int svs_loudness_stats(const double* z_m, int64_t n_m, const double* z_s, int64_t n_s, double* stats, void* ws, size_t ws_bytes,
                                  hipStream_t stream) {
  SVS_REQUIRE(n_m >= 0, "svs_loudness_stats: n_m must not be negative, got %lld", (long long)n_m);
  SVS_REQUIRE(n_s >= 0 && n_s < ST_MAX_N, "svs_loudness_stats: n_s must be in 0..2^31 - 1, got %lld", (long long)n_s);
  SVS_REQUIRE(stats && (z_m || n_m == 0) && (z_s || n_s == 0), "svs_loudness_stats: null pointer");
  SVS_REQUIRE((((uintptr_t)z_m) & 7u) == 0 && (((uintptr_t)z_s) & 7u) == 0 && (((uintptr_t)stats) & 7u) == 0 && (((uintptr_t)ws) & 7u) == 0,
              "svs_loudness_stats: z_m, z_s, stats and the workspace must be 8-byte aligned");
  if (!ws || ws_bytes < svs_loudness_stats_workspace_bytes(n_s)) {
    svs_set_error("svs_loudness_stats: workspace too small (%zu bytes, need %zu)", ws_bytes, svs_loudness_stats_workspace_bytes(n_s));
    return SVS_ERR_WORKSPACE;
  }
  hipLaunchKernelGGL(loud_stats_kernel, dim3(1), dim3(ST_THREADS), 0, stream, z_m, (long)n_m, z_s, (long)n_s, stats, (unsigned long long*)ws);
  SVS_CHECK_LAUNCH("loudness stats");
  return SVS_OK;
}

// ------------------------------------------------------------------------------------------------
// true peaks
// ------------------------------------------------------------------------------------------------
// partial[(row * nblk + block) * 2 + {0, 1}] = the block's largest |sample| and largest |sample or interpolated value|
template <int F>
__global__ __launch_bounds__(TP_THREADS) void true_peaks_kernel(const float* __restrict__ x, int channels, long n, long ld_stem, long ld_ch,
                                                                const float* __restrict__ taps, float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float sx[TP_LDS];
  __shared__ float st[12 * F + 1];
  __shared__ float sm[2 * (TP_THREADS / 64)];
  const int tid = threadIdx.x;
  const int row = blockIdx.y;
  const float* xr = x + (long)(row / channels) * ld_stem + (long)(row % channels) * ld_ch;
  const long b0 = (long)blockIdx.x * TP_BLOCK;
  tp_stage(sx, xr, b0, n, tid);
  if (F > 1 && tid < 12 * F + 1) st[tid] = taps[tid];
  __syncthreads();
  float sp = 0.f, tp = 0.f;
#pragma unroll
  for (int q = 0; q < TP_PER / 4; ++q) {
    const int s0 = 4 * (tid + q * TP_THREADS);                     // four consecutive samples b0 + s0 + d from five 16-byte LDS reads
    if (b0 + s0 >= n) break;
    float r[20];                                                  // r[j] = x[b0 + s0 + j - TP_ORIGIN], zero outside the row
    tp_window(sx, s0, r);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (b0 + s0 + d >= n) break;
      sp = fmaxf(sp, fabsf(r[TP_ORIGIN + d]));
#pragma unroll
      for (int p = 1; p < F; ++p) {
        tp = fmaxf(tp, fabsf(tp_phase<F>(st, r, d, p)));
      }
    }
  }
  tp = fmaxf(tp, sp);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sp = fmaxf(sp, __shfl_xor(sp, o, 64));
    tp = fmaxf(tp, __shfl_xor(tp, o, 64));
  }
  if ((tid & 63) == 0) { sm[tid >> 6] = sp; sm[TP_THREADS / 64 + (tid >> 6)] = tp; }
  __syncthreads();
  if (tid == 0) {
    float a = sm[0], b = sm[TP_THREADS / 64];
#pragma unroll
    for (int i = 1; i < TP_THREADS / 64; ++i) { a = fmaxf(a, sm[i]); b = fmaxf(b, sm[TP_THREADS / 64 + i]); }
    float* out = partial + ((long)row * gridDim.x + blockIdx.x) * 2;
    out[0] = a;
    out[1] = b;
  }
}

// one wave per row: the maxima of its blocks
__global__ __launch_bounds__(64) void true_peaks_reduce_kernel(const float* __restrict__ partial, long nblk, float* __restrict__ sample_peaks,
                                                               float* __restrict__ true_peaks) {
  const float* row = partial + (long)blockIdx.x * nblk * 2;
  float a = 0.f, b = 0.f;
  for (long i = threadIdx.x; i < nblk; i += 64) {
    a = fmaxf(a, row[2 * i]);
    b = fmaxf(b, row[2 * i + 1]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a = fmaxf(a, __shfl_xor(a, o, 64));
    b = fmaxf(b, __shfl_xor(b, o, 64));
  }
  if (threadIdx.x == 0) {
    if (sample_peaks) sample_peaks[blockIdx.x] = a;
    if (true_peaks) true_peaks[blockIdx.x] = b;
  }
}

static long tp_blocks(int64_t n) { return n > 0 ? (long)((n + TP_BLOCK - 1) / TP_BLOCK) : 1; }

extern "C" size_t svs_true_peaks_workspace_bytes(int64_t n, int rows) {
  if (n < 0 || n > (INT64_MAX / 16) || rows < 1 || rows > TP_MAX_ROWS || tp_blocks(n) >= (1L << 31)) return 0;
  return (size_t)rows * (size_t)tp_blocks(n) * 2 * sizeof(float);
}

extern "C" int svs_true_peaks(const float* x, int stems, int channels, int64_t n, int64_t ld_stem, int64_t ld_ch, const float* taps, int factor,
                              float* sample_peaks, float* true_peaks, void* ws, size_t ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(stems >= 1 && stems <= 8, "svs_true_peaks: stems must be in 1..8, got %d", stems);
  SVS_REQUIRE(channels >= 1 && channels <= 8, "svs_true_peaks: channels must be in 1..8, got %d", channels);
  SVS_REQUIRE(n >= 0 && n <= (INT64_MAX / 16), "svs_true_peaks: n must not be negative, got %lld", (long long)n);
  SVS_REQUIRE(ld_ch >= n, "svs_true_peaks: ld_ch must be at least n = %lld, got %lld", (long long)n, (long long)ld_ch);
  SVS_REQUIRE(stems == 1 || ld_stem >= ld_ch * (channels - 1) + n, "svs_true_peaks: ld_stem must be at least a stem's %lld samples, got %lld",
              (long long)(ld_ch * (channels - 1) + n), (long long)ld_stem);
  SVS_REQUIRE(factor == 1 || factor == 2 || factor == 4, "svs_true_peaks: factor must be 1, 2 or 4, got %d", factor);
  const long nblk = tp_blocks(n);
  SVS_REQUIRE(nblk < (1L << 31), "svs_true_peaks: %ld blocks do not fit a grid", nblk);
  SVS_REQUIRE((x || n == 0) && (taps || factor == 1), "svs_true_peaks: null pointer");
  SVS_REQUIRE((((uintptr_t)x) & 3u) == 0 && (((uintptr_t)ws) & 3u) == 0, "svs_true_peaks: x and the workspace must be 4-byte aligned");
  const int rows = stems * channels;
  if (!ws || ws_bytes < svs_true_peaks_workspace_bytes(n, rows)) {
    svs_set_error("svs_true_peaks: workspace too small (%zu bytes, need %zu)", ws_bytes, svs_true_peaks_workspace_bytes(n, rows));
    return SVS_ERR_WORKSPACE;
  }
  if (!sample_peaks && !true_peaks) return SVS_OK;
  const dim3 grid((unsigned)nblk, (unsigned)rows);
  float* partial = (float*)ws;
  if (factor == 1) {
    hipLaunchKernelGGL((true_peaks_kernel<1>), grid, dim3(TP_THREADS), 0, stream, x, channels, (long)n, (long)ld_stem, (long)ld_ch, taps, partial);
  } else if (factor == 2) {
    hipLaunchKernelGGL((true_peaks_kernel<2>), grid, dim3(TP_THREADS), 0, stream, x, channels, (long)n, (long)ld_stem, (long)ld_ch, taps, partial);
  } else {
    hipLaunchKernelGGL((true_peaks_kernel<4>), grid, dim3(TP_THREADS), 0, stream, x, channels, (long)n, (long)ld_stem, (long)ld_ch, taps, partial);
  }
  SVS_CHECK_LAUNCH("true peaks");
  hipLaunchKernelGGL(true_peaks_reduce_kernel, dim3((unsigned)rows), dim3(64), 0, stream, (const float*)partial, nblk, sample_peaks, true_peaks);
  SVS_CHECK_LAUNCH("true peaks reduce");
  return SVS_OK;
}
