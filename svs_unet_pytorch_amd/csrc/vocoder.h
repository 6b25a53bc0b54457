// Device helpers shared by the two phase vocoders on the resident spectra, stretch.hip (time) and pitch.hip (frequency): angles as
// 32-bit fractions of a turn, the polar form of one source frame, and the prefix sum inside a wave.
#pragma once
#include "internal.h"

namespace vocoder {

constexpr double kTurnsPerRad = 4294967296.0 / 6.283185307179586476925286766559;     // 2^32 / (2 pi)
constexpr double kRadPerTurn = 6.283185307179586476925286766559 / 4294967296.0;

// an angle |phi| <= pi as a 32-bit fraction of a turn, modulo 1 (fp32 pi is a hair above half a turn: the conversion to unsigned wraps it)
__device__ __forceinline__ uint32_t to_turns(float phi) { return (uint32_t)__double2ll_rn((double)phi * kTurnsPerRad); }
// ... and back, in [-pi, pi]
__device__ __forceinline__ float to_radians(uint32_t turns) { return (float)((double)(int32_t)turns * kRadPerTurn); }

// m cis(phi) for |phi| <= pi (augment.hip's cis_scaled: the large-argument reduction of sincosf is not built)
__device__ __forceinline__ void cis_scaled(float m, float phi, float& re, float& im) {
  __builtin_assume(__builtin_fabsf(phi) < 0x1.0p+17f);
  float s, c;
  sincosf(phi, &s, &c);
  re = m * c;
  im = m * s;
}

// |S[k]| and arg S[k] (in turns) of the vocal (ACC false) or the accompaniment (ACC true) of the song row at `base` (T frames)
template <bool ACC>
__device__ __forceinline__ void source_frame(const float* __restrict__ mix_songs, const float* __restrict__ voc_songs,
                                             const float* __restrict__ mix_ang, const float* __restrict__ voc_ang, long base, int k,
                                             int T, bool live, float& mag, uint32_t& turns) {
  mag = 0.f;
  turns = 0u;
  if (!live || k < 0 || k >= T) return;                // outside the song (or the tile): magnitude 0, arg 0
  const float V = voc_songs[base + k], pv = voc_ang[base + k];
  float arg;
  if constexpr (!ACC) {
    mag = V;
    arg = pv;
  } else {
    const float M = mix_songs[base + k], pm = mix_ang[base + k];
    float mr, mi, vr, vi;
    cis_scaled(M, pm, mr, mi);
    cis_scaled(V, pv, vr, vi);
    const float re = mr - vr, im = mi - vi;
    mag = hypotf(re, im);
    arg = atan2f(im, re);
  }
  turns = mag == 0.f ? 0u : to_turns(arg);
}

// |S[k]| alone, the same value (pitch.hip's second bin: its angle is not used)
template <bool ACC>
__device__ __forceinline__ float source_magnitude(const float* __restrict__ mix_songs, const float* __restrict__ voc_songs,
                                                  const float* __restrict__ mix_ang, const float* __restrict__ voc_ang, long base,
                                                  int k, int T, bool live) {
  if (!live || k < 0 || k >= T) return 0.f;
  const float V = voc_songs[base + k];
  if constexpr (!ACC) {
    return V;
  } else {
    const float M = mix_songs[base + k];
    float mr, mi, vr, vi;
    cis_scaled(M, mix_ang[base + k], mr, mi);
    cis_scaled(V, voc_ang[base + k], vr, vi);
    return hypotf(mr - vr, mi - vi);
  }
}

// inclusive prefix sum over the 64 lanes of a wave (wrapping unsigned adds: exact)
__device__ __forceinline__ uint32_t wave_scan(uint32_t x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

}  // namespace vocoder
