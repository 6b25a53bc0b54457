// The over-sampling arithmetic of the true-peak meter, shared by svs_true_peaks (r128.hip) and svs_limiter_envelope (limiter.hip), so
// that the interpolated values of the two are the same floats: the staging of a block's samples with their halo, a lane's 20-sample
// register window, and one phase's accumulator.
#pragma once
#include "common.h"

#define TP_THREADS 256
#define TP_PER 8                             // samples per lane
#define TP_BLOCK (TP_THREADS * TP_PER)       // samples per block
#define TP_HALO 6
#define TP_ORIGIN 8                          // LDS index of a block's first sample: the halo in front, and 16-byte aligned
#define TP_LDS (TP_ORIGIN + TP_BLOCK + 8)    // a lane's last 16-byte read ends at TP_BLOCK - 4 + 20

// sx[TP_ORIGIN + j] = xr[b0 + j] for -TP_HALO <= j < TP_BLOCK + TP_HALO, zero outside [0, n), from 16-byte loads (scalar at the row's ends
// and where a vector straddles them); the two words each side that the lanes' 16-byte reads reach besides are zeroed.  The caller
// synchronises the block afterwards.
__device__ __forceinline__ void tp_stage(float* __restrict__ sx, const float* __restrict__ xr, long b0, long n, int tid) {
  // in u = i + m the row's vectors are 16-byte aligned; the window [b0 - 6, b0 + TP_BLOCK + 6) is widened to whole vectors
  const long m = (long)((((uintptr_t)xr) >> 2) & 3u);
  const long u_first = b0 - TP_HALO + m;
  const long u0 = (u_first >= 0 ? u_first / 4 : -((3 - u_first) / 4)) * 4;           // floor to a multiple of 4
  const int nvec = (int)((b0 + TP_BLOCK + TP_HALO + m - u0 + 3) / 4);                // what falls outside the window is dropped
  for (int v = tid; v < nvec; v += TP_THREADS) {
    const long i = u0 + 4L * v - m;                              // the row index of the vector's first element
    float4 q;
    if (i >= 0 && i + 3 < n) {
      q = *reinterpret_cast<const float4*>(xr + i);
    } else {
      q.x = (i >= 0 && i < n) ? xr[i] : 0.f;
      q.y = (i + 1 >= 0 && i + 1 < n) ? xr[i + 1] : 0.f;
      q.z = (i + 2 >= 0 && i + 2 < n) ? xr[i + 2] : 0.f;
      q.w = (i + 3 >= 0 && i + 3 < n) ? xr[i + 3] : 0.f;
    }
    const float e[4] = {q.x, q.y, q.z, q.w};
    const int l = (int)(i - b0) + TP_ORIGIN;                      // sample b0 sits at the 16-byte aligned LDS index TP_ORIGIN
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (l + d >= TP_ORIGIN - TP_HALO && l + d < TP_ORIGIN + TP_BLOCK + TP_HALO) sx[l + d] = e[d];
  }
  if (tid < TP_ORIGIN - TP_HALO) {                                // the lanes' 16-byte reads reach these; no result depends on them
    sx[tid] = 0.f;
    sx[TP_ORIGIN + TP_BLOCK + TP_HALO + tid] = 0.f;
  }
}

// r[j] = x[b0 + s0 + j - TP_ORIGIN], zero outside the row: the window of the four consecutive samples b0 + s0 + d, from five 16-byte
// LDS reads (lanes 16 bytes apart: no bank conflict)
__device__ __forceinline__ void tp_window(const float* __restrict__ sx, int s0, float (&r)[20]) {
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const float4 a = *reinterpret_cast<const float4*>(sx + s0 + 4 * j);
    r[4 * j] = a.x; r[4 * j + 1] = a.y; r[4 * j + 2] = a.z; r[4 * j + 3] = a.w;
  }
}

// y[F i + p] of the window's sample d: acc = fmaf(taps[p + F k], x[i + 6 - k], acc), k ascending, from 0
template <int F>
__device__ __forceinline__ float tp_phase(const float* __restrict__ st, const float (&r)[20], int d, int p) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 12; ++k) acc = fmaf(st[p + F * k], r[TP_ORIGIN + d + TP_HALO - k], acc);
  return acc;
}
