// Time-stretch augmentation of the training tiles: a phase vocoder between "read the source frames" and "mix" of augment.hip, whose
// song storage, DC-row convention, tables and right zero-padding this keeps (the reference's SpectrogramDataset, train.py:86-143,
// has no augmentation).  Item b stretches the vocal of song A = song_v[b] from column s_v = start_v[b] at rate q_v / 1024 and the
// accompaniment M cis(phi_m) - V cis(phi_v) of song B = song_a[b] from s_a at q_a / 1024 (song_a[b] < 0: B = A, s_a = s_v, q_a = q_v),
// then mixes the two stretched sources.  For one source S, row f (bin = f + 1), output frame t:
//     n = t q,  k = s + (n >> 10),  alpha = (n & 1023) / 1024            index and weight exact in integers
//     mag_t = (1 - alpha) |S[k]| + alpha |S[k+1]|
//     acc_0 = arg S[s],  acc_{t+1} = acc_t + w + wrap(arg S[k+1] - arg S[k] - w)       w = 2 pi ((hop bin) mod n_fft) / n_fft
//     out_t = mag_t cis(acc_t)                                            (the classic phase vocoder, augment.stretch_reference)
//     z = g_v PV(vocal) + g_a PV(accompaniment):  mix = |z|, mix_phase = arg z, voc = g_v mag_v, voc_phase = acc_v in [-pi, pi]
// arg of an exactly zero magnitude is 0, columns outside [0, T) are zero, and a phase is written as 0 where its magnitude is 0.
//
// The accumulator: 2 pi hop bin / n_fft reaches ~2,400 rad per frame and a plain fp32 sum over 128 frames loses the phase.  Here
// every angle becomes a 32-bit fraction of a turn (rounded once, from fp64: 2^-33 turn), w is the exact fraction
// ((hop bin) mod n_fft) * 2^32 / n_fft, wrap() is the signed reading of the 32-bit difference, and the sum is unsigned 32-bit
// addition: it wraps for free, is exact and associative, so the scan gives the same bits whatever the order, the grid or the batch.
// (In this arithmetic w + wrap(delta - w) == delta identically: the size of w cannot reach the accumulator.)
//
// One wave = one (item, row); lanes run along time (a row's source reads stay contiguous), 64 frames per round, the prefix sum is a
// shuffle scan inside the wave and the carry into the next round is lane 63's total.  No LDS, no workspace, no atomics; per
// element 12 loads, 6 sincosf, 3 atan2f, 3 hypotf (the device library's accurate forms, as in augment.hip).
#include "internal.h"
#include "vocoder.h"

namespace {

using namespace vocoder;       // to_turns / to_radians, cis_scaled, source_frame, wave_scan

// one source of one row over one round of 64 output frames: mag (interpolated) and acc (turns) of frame t, `carry` updated
template <bool ACC>
__device__ __forceinline__ void vocode(const float* __restrict__ mix_songs, const float* __restrict__ voc_songs,
                                       const float* __restrict__ mix_ang, const float* __restrict__ voc_ang, long base, int T, int s,
                                       int q, uint32_t w, int t, bool live, int lane, bool first, uint32_t& carry, float& mag,
                                       uint32_t& acc) {
  const int n = t * q, k = s + (n >> 10);
  const float alpha = (float)(n & 1023) * (1.0f / 1024.0f);
  float m0, m1;
  uint32_t a0, a1;
  source_frame<ACC>(mix_songs, voc_songs, mix_ang, voc_ang, base, k, T, live, m0, a0);
  source_frame<ACC>(mix_songs, voc_songs, mix_ang, voc_ang, base, k + 1, T, live, m1, a1);
  mag = (1.0f - alpha) * m0 + alpha * m1;
  const uint32_t d = a1 - a0 - w;                      // its signed reading is the deviation wrapped to [-1/2, 1/2) turn
  const uint32_t step = live ? w + d : 0u;             // the advance from frame t to t + 1
  if (first) carry = __shfl(a0, 0, 64);                // acc_0 = arg S[s]: frame 0 reads k = s
  const uint32_t incl = wave_scan(step, lane);
  acc = carry + incl - step;                           // exclusive: the advances of frames 0 .. t-1
  carry += __shfl(incl, 63, 64);
}

// PHASE: the two phase tiles are written.
template <bool PHASE>
__global__ __launch_bounds__(256) void crop_stretch_tiles_kernel(
    const float* __restrict__ mix_songs, const float* __restrict__ voc_songs, const float* __restrict__ mix_ang,
    const float* __restrict__ voc_ang, const long long* __restrict__ offset, const int* __restrict__ frames,
    const int* __restrict__ song_v, const int* __restrict__ start_v, const int* __restrict__ song_a, const int* __restrict__ start_a,
    const float* __restrict__ gain_v, const float* __restrict__ gain_a, const int* __restrict__ rate_v, const int* __restrict__ rate_a,
    int B, int F, int seg, int n_fft, int hop, float* __restrict__ mix, float* __restrict__ voc, float* __restrict__ mix_phase,
    float* __restrict__ voc_phase) {
  const int lane = threadIdx.x & 63;
  const long rows = (long)B * F;
  const int turn_shift = 32 - (31 - __builtin_clz((unsigned)n_fft));       // 2^32 / n_fft as a shift (n_fft a power of two)
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * 4) {      // wave-uniform
    const int f = (int)(row % F), b = (int)(row / F);
    const int sv = song_v[b], Tv = frames[sv], stv = start_v[b], qv = rate_v[b];
    int sa = song_a[b], sta = start_a[b], qa = rate_a[b];
    if (sa < 0) sa = sv, sta = stv, qa = qv;           // gain item: its own accompaniment, through the same complex path
    const int Ta = frames[sa];
    const long basev = offset[sv] + (long)f * Tv, basea = offset[sa] + (long)f * Ta;
    const float gv = gain_v[b], ga = gain_a[b];
    const uint32_t w = (uint32_t)(((long)hop * (f + 1)) % n_fft) << turn_shift;       // (hop bin mod n_fft) / n_fft of a turn, exact
    uint32_t carry_v = 0u, carry_a = 0u;
    for (int t0 = 0; t0 < seg; t0 += 64) {
      const int t = t0 + lane;
      const bool live = t < seg;
      float mag_v, mag_a;
      uint32_t acc_v, acc_a;
      vocode<false>(mix_songs, voc_songs, mix_ang, voc_ang, basev, Tv, stv, qv, w, t, live, lane, t0 == 0, carry_v, mag_v, acc_v);
      vocode<true>(mix_songs, voc_songs, mix_ang, voc_ang, basea, Ta, sta, qa, w, t, live, lane, t0 == 0, carry_a, mag_a, acc_a);
      if (!live) continue;                             // (after the shuffles: every lane took part in them)
      const float v = gv * mag_v, a = ga * mag_a;
      const float phv = to_radians(acc_v);
      float vr, vi, ar, ai;
      cis_scaled(v, phv, vr, vi);
      cis_scaled(a, to_radians(acc_a), ar, ai);
      const float re = vr + ar, im = vi + ai;
      const float m = hypotf(re, im);
      const long dst = row * seg + t;
      mix[dst] = m;
      voc[dst] = v;
      if constexpr (PHASE) {
        mix_phase[dst] = m == 0.f ? 0.f : atan2f(im, re);
        voc_phase[dst] = v == 0.f ? 0.f : phv;
      }
    }
  }
}

int stretch_grid(long rows) {                          // 8 blocks of 4 waves on each of the 256 CUs; the rest by grid stride
  long g = (rows + 3) / 4;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

extern "C" int svs_crop_stretch_tiles(const float* mix_songs, const float* voc_songs, const float* mix_ang, const float* voc_ang,
                                      const int64_t* offset, const int32_t* frames, const int32_t* song_v, const int32_t* start_v,
                                      const int32_t* song_a, const int32_t* start_a, const float* gain_v, const float* gain_a,
                                      const int32_t* rate_v, const int32_t* rate_a, int B, int F, int seg, int n_fft, int hop,
                                      float* mix, float* voc, float* mix_phase, float* voc_phase, hipStream_t stream) {
  const char* who = "svs_crop_stretch_tiles";
  SVS_REQUIRE(mix_songs && voc_songs && mix_ang && voc_ang && offset && frames && mix && voc,
              "%s: null pointer (songs, angles, offset, frames, mix or voc; there is no magnitude-only stretch)", who);
  SVS_REQUIRE(song_v && start_v && song_a && start_a && gain_v && gain_a && rate_v && rate_a,
              "%s: null table (song_v, start_v, song_a, start_a, gain_v, gain_a, rate_v or rate_a)", who);
  SVS_REQUIRE((mix_phase != nullptr) == (voc_phase != nullptr), "%s: mix_phase and voc_phase must both be given or both be NULL", who);
  SVS_REQUIRE(n_fft == 512 || n_fft == 1024 || n_fft == 2048, "%s: n_fft must be 512, 1024 or 2048, got %d", who, n_fft);
  SVS_REQUIRE(hop > 0 && hop <= n_fft, "%s: hop must be in 1..n_fft, got hop=%d n_fft=%d", who, hop, n_fft);
  SVS_REQUIRE(B > 0 && seg > 0 && seg % 4 == 0, "%s: bad geometry, B and seg must be positive and seg a multiple of 4, got B=%d seg=%d", who, B, seg);
  // rows are bins 1..F of an n_fft-point spectrum: the whole of it (F == n_fft / 2, what augment.crop_stretch passes) or its lowest band
  SVS_REQUIRE(F > 0 && F <= n_fft / 2, "%s: bad geometry, F rows are bins 1..F of an n_fft spectrum: 1 <= F <= n_fft / 2, got F=%d n_fft=%d", who, F, n_fft);
  SVS_REQUIRE(svs_aligned16(mix) && svs_aligned16(voc) && svs_aligned16(mix_phase) && svs_aligned16(voc_phase),
              "%s: bad geometry, the output tiles must be 16-byte aligned", who);
  const dim3 grid(stretch_grid((long)B * F)), block(256);
#define STRETCH_LAUNCH(PHASE)                                                                                                        \
  hipLaunchKernelGGL((crop_stretch_tiles_kernel<PHASE>), grid, block, 0, stream, mix_songs, voc_songs, mix_ang, voc_ang,             \
                     (const long long*)offset, frames, song_v, start_v, song_a, start_a, gain_v, gain_a, rate_v, rate_a, B, F, seg, \
                     n_fft, hop, mix, voc, mix_phase, voc_phase)
  if (mix_phase) STRETCH_LAUNCH(true);
  else STRETCH_LAUNCH(false);
#undef STRETCH_LAUNCH
  SVS_CHECK_LAUNCH("crop_stretch_tiles");
  return SVS_OK;
}
