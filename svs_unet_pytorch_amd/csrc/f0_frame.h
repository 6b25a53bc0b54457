// The per-frame device functions of the YIN tracker -- staging, d', pick -- and the launch plan and argument rules that go with them,
// shared by f0.hip (svs_f0_cmnd / svs_f0_pick / svs_f0_track) and f0_smooth.hip (svs_f0_candidates): one definition, so that what the
// two files compute per frame is the same instruction sequence and their outputs are the same bits.  f0.hip's header comment describes
// the layout (one wave per frame, L lags per lane, the padded LDS signal); both files are built with -fno-slp-vectorize (build.py).
#pragma once
#include <climits>
#include <cmath>

#include "internal.h"

#define F0_MAX_W 4096
#define F0_MAX_TAU 2048
#define F0_MAX_ROWS 64
#define F0_MAX_FRAMES 4                                             // frames, and waves, of a block
#define F0_LDS_BYTES (48 * 1024)

template <int LOG2L>
__host__ __device__ __forceinline__ int f0_pad(int i) { return i + (i >> LOG2L); }

__device__ __forceinline__ double f0_wave_scan(double v, int lane) {        // inclusive, one fixed order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// the block's samples into LDS: len of them from xr, then L zeros, one word of padding after every L
template <int LOG2L>
__device__ __forceinline__ void f0_stage(const float* __restrict__ xr, int len, int tid, int nthreads, float* xs) {
  constexpr int L = 1 << LOG2L;
  for (int i = tid; i < len + L; i += nthreads) xs[f0_pad<LOG2L>(i)] = i < len ? xr[i] : 0.f;
}

// one step of the window: x[j] against the L lags of the lane; U = j mod L places the newest sample in the rotating window
template <int LOG2L, int U>
__device__ __forceinline__ void f0_step(const float* xs, int at_j, int at_w, float* win, double* acc) {
  constexpr int L = 1 << LOG2L;
  const float xj = xs[f0_pad<LOG2L>(at_j + U)];
  win[(L - 1 + U) % L] = xs[f0_pad<LOG2L>(at_w + U + L - 1)];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const double d = (double)(xj - win[(l + U) % L]);                 // one fp32 subtraction, then exact
    acc[l] = fma(d, d, acc[l]);
  }
}

// d'(0 .. tau_max) of the frame that starts at xs index `base` into dp (the wave's LDS row), and its rms
template <int LOG2L>
__device__ __forceinline__ float f0_frame_cmnd(const float* xs, int base, int W, int tau_max, int lane, float* dp) {
  constexpr int L = 1 << LOG2L;
  if (lane == 0) dp[0] = 1.f;
  double carry = 0.0;
  for (int g0 = 0; g0 * L < tau_max; g0 += 64) {
    const int tau0 = 1 + L * (g0 + lane);
    double acc[L];
#pragma unroll
    for (int l = 0; l < L; ++l) acc[l] = 0.0;
    if (tau0 <= tau_max) {
      float win[L];
      const int wb = base + tau0;
#pragma unroll
      for (int l = 0; l < L - 1; ++l) win[l] = xs[f0_pad<LOG2L>(wb + l)];
      int j = 0;
      for (; j + L <= W; j += L) svs_static_for<L>([&](auto u) { f0_step<LOG2L, decltype(u)::value>(xs, base + j, wb + j, win, acc); });
      svs_static_for<L>([&](auto u) {
        if (j + decltype(u)::value < W) f0_step<LOG2L, decltype(u)::value>(xs, base + j, wb + j, win, acc);      // uniform
      });
    }
    double pre[L], s = 0.0;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      if (tau0 + l > tau_max) acc[l] = 0.0;                           // lags past the range read the zero padding
      s += acc[l];
      pre[l] = s;
    }
    const double inc = f0_wave_scan(s, lane);
    double exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = 0.0;
    const double before = carry + exc;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const int tau = tau0 + l;
      if (tau <= tau_max) {
        const double S = before + pre[l];
        dp[tau] = S == 0.0 ? 1.f : (float)(acc[l] * (double)tau / S);
      }
    }
    carry += __shfl(inc, 63, 64);
  }
  double e = 0.0;
  for (int j = lane; j < W; j += 64) {
    const double v = (double)xs[f0_pad<LOG2L>(base + j)];
    e = fma(v, v, e);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
  return (float)sqrt(e / (double)W);
}

// the pick on one row of d' (LDS or memory), by one wave; lane 0 writes the three outputs
__device__ __forceinline__ void f0_frame_pick(const float* dp, int tau_min, int tau_max, double threshold, double sr, int lane, bool gated,
                                              float rms, float rms_gate, float* f0, float* ap, int* voiced) {
  int first = INT_MAX;
  for (int t = tau_min + lane; t <= tau_max; t += 64)
    if ((double)dp[t] < threshold) {
      first = t;
      break;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  const bool found = first != INT_MAX;
  int tau = first;
  if (found) {
    while (tau + 1 <= tau_max && dp[tau + 1] < dp[tau]) ++tau;        // the same walk on every lane
  } else {
    float best = INFINITY;
    int at = INT_MAX;
    for (int t = tau_min + lane; t <= tau_max; t += 64) {
      const float v = dp[t];
      if (v < best) {
        best = v;
        at = t;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oa = __shfl_xor(at, o, 64);
      if (ob < best || (ob == best && oa < at)) {
        best = ob;
        at = oa;
      }
    }
    tau = at == INT_MAX ? tau_min : at;                               // a row without one ordered value
  }
  if (lane != 0) return;
  const double b = (double)dp[tau];
  double delta = 0.0;
  if (tau - 1 >= 1 && tau + 1 <= tau_max) {
    const double a = (double)dp[tau - 1], c = (double)dp[tau + 1];
    const double q = a - 2.0 * b + c;
    if (q > 0.0) delta = fmin(1.0, fmax(-1.0, 0.5 * (a - c) / q));
  }
  *f0 = (float)(sr / ((double)tau + delta));
  *ap = (float)b;
  *voiced = (found && (!gated || rms >= rms_gate)) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct F0Plan { int log2l, F, xcap; size_t lds; };

// Lags per lane: the wave walks ceil(tau_max / 64 L) passes of 64 L lags, and the lanes past tau_max in the last pass idle.  The largest
// L of 8, 4, 2 that keeps at least 85 % of the lanes busy, else the one that keeps most (the larger on a tie): 679 lags are 2 passes at
// L = 8 with 66 % of the lanes busy, 3 passes at L = 4 with 88 %.  L follows from tau_max alone, so it is the same for every launch of a geometry.
static inline int f0_lags_per_lane_log2(int tau_max) {
  int best = 3;
  double best_busy = 0.0;
  for (int log2l = 3; log2l >= 1; --log2l) {
    const int groups = (tau_max + (1 << log2l) - 1) >> log2l, passes = (groups + 63) / 64;
    const double busy = (double)groups / (64.0 * passes);
    if (busy >= 0.85) return log2l;
    if (busy > best_busy) best_busy = busy, best = log2l;
  }
  return best;
}

static inline F0Plan f0_plan(int W, int tau_max, int hop) {
  F0Plan p;
  p.log2l = f0_lags_per_lane_log2(tau_max);
  const int L = 1 << p.log2l, span = W + tau_max;
  p.F = hop >= span ? 1 : F0_MAX_FRAMES;
  for (;; --p.F) {
    const int len = span + (p.F - 1) * hop + L;
    p.xcap = (p.log2l == 1 ? f0_pad<1>(len) : p.log2l == 2 ? f0_pad<2>(len) : f0_pad<3>(len)) + 1;
    p.lds = ((size_t)p.xcap + (size_t)p.F * (tau_max + 1)) * sizeof(float);
    if (p.lds <= F0_LDS_BYTES || p.F == 1) return p;
  }
}

// the rules the kernels over the signal share; `who` starts every message
static inline int f0_check_signal(const char* who, const float* x, int rows, int64_t n, int64_t ld_row, int W, int tau_max, int hop,
                                  int64_t first_frame, int64_t n_frames) {
  SVS_REQUIRE(rows >= 1 && rows <= F0_MAX_ROWS, "%s: rows must be in 1..%d, got %d", who, F0_MAX_ROWS, rows);
  SVS_REQUIRE(W >= 1 && W <= F0_MAX_W, "%s: W must be in 1..%d, got %d", who, F0_MAX_W, W);
  SVS_REQUIRE(tau_max >= 1 && tau_max <= F0_MAX_TAU, "%s: tau_max must be in 1..%d, got %d", who, F0_MAX_TAU, tau_max);
  SVS_REQUIRE(hop >= 1, "%s: hop must be at least 1, got %d", who, hop);
  SVS_REQUIRE(first_frame >= 0 && n_frames >= 0, "%s: first_frame and n_frames must not be negative, got %lld and %lld", who,
              (long long)first_frame, (long long)n_frames);
  SVS_REQUIRE(n >= 0 && n <= (INT64_MAX / 16), "%s: n must not be negative, got %lld", who, (long long)n);
  SVS_REQUIRE(first_frame + n_frames <= (INT64_MAX / 16) / hop, "%s: the frames do not fit 64-bit sample indices", who);
  SVS_REQUIRE(n_frames == 0 || (first_frame + n_frames - 1) * hop + W + tau_max <= n,
              "%s: frames %lld..%lld need %lld samples, the signal has n = %lld (only whole frames are formed)", who, (long long)first_frame,
              (long long)(first_frame + n_frames - 1), (long long)((first_frame + n_frames - 1) * hop + W + tau_max), (long long)n);
  SVS_REQUIRE(rows == 1 || ld_row >= n, "%s: ld_row must be at least n = %lld, got %lld", who, (long long)n, (long long)ld_row);
  SVS_REQUIRE((((uintptr_t)x) & 3u) == 0, "%s: x must be 4-byte aligned", who);
  return SVS_OK;
}

static inline int f0_check_pick(const char* who, int tau_min, int tau_max, double threshold, float rms_gate, double sr) {
  SVS_REQUIRE(tau_max >= 1 && tau_max <= F0_MAX_TAU, "%s: tau_max must be in 1..%d, got %d", who, F0_MAX_TAU, tau_max);
  SVS_REQUIRE(tau_min >= 1 && tau_min < tau_max, "%s: tau_min must be in 1..tau_max - 1 = %d, got %d", who, tau_max - 1, tau_min);
  SVS_REQUIRE(threshold > 0.0 && threshold < INFINITY, "%s: the threshold must be positive and finite, got %g", who, threshold);
  SVS_REQUIRE(rms_gate >= 0.f && rms_gate < INFINITY, "%s: rms_gate must be finite and not negative, got %g", who, (double)rms_gate);
  SVS_REQUIRE(sr > 0.0 && sr < INFINITY, "%s: sr must be positive and finite, got %g", who, sr);
  return SVS_OK;
}
