// Pitch-shift augmentation of the training tiles: stretch.hip's phase vocoder with the frequency axis resampled and the phase
// advance scaled (the reference's SpectrogramDataset, train.py:86-143, has no augmentation).  Items, song storage, DC-row convention,
// tables, gains, rates and right zero-padding are those of svs_crop_stretch_tiles; pitch_v / pitch_a are Q10 pitches P (p = P / 1024).
// For one source S (rows are bins 1..F, every bin outside 1..F is zero), output row f (b = f + 1), output frame t:
//     n = t q,  k = s + (n >> 10),  alpha = (n & 1023) / 1024                                   stretch.hip's time indexing
//     N = 1024 b,  j0 = N div P,  gamma = (N mod P) / P,  j = clamp((2 N + P) div 2 P, 1, F)    all integer: j is j0 or j0 + 1
//     tm(i) = (1 - alpha) |S[i, k]| + alpha |S[i, k+1]|
//     mag_t = (1 - gamma) tm(j0) + gamma tm(j0 + 1)                       the source magnitude at the fractional bin b / p
//     w  = 2 pi ((hop j) mod n_fft) / n_fft,   d = wrap(arg S[j, k+1] - arg S[j, k] - w) in [-pi, pi)
//     w' = 2 pi ((hop j P) mod (1024 n_fft)) / (1024 n_fft)               p times the unreduced centre advance of bin j, reduced exactly
//     acc_0 = arg S[j, s],  acc_{t+1} = acc_t + w' + p d,  out_t = mag_t cis(acc_t)             (augment.pitch_reference)
//     z = g_v PV(vocal) + g_a PV(accompaniment):  mix = |z|, mix_phase = arg z, voc = g_v mag_v, voc_phase = acc_v in [-pi, pi]
// arg of an exactly zero magnitude is 0, columns outside [0, T) are zero, and a phase is written as 0 where its magnitude is 0.  At
// P = 1024 this is svs_crop_stretch_tiles: gamma = 0, j0 = j = b, w' = w, p d = d.
//
// The accumulator is stretch.hip's 32-bit fraction of a turn.  w' is the exact integer ((hop j P) mod (1024 n_fft)) 2^32 /
// (1024 n_fft) (the product is formed in 64 bits: hop = 2048, j = 1024, P = 2048 would make it 2^32, rows 1..F pass 2^31); p d is
// (int64(d) P) >> 10, the only rounding in the sum (below 2^-32 turn per frame); the sum is wrapping unsigned addition, exact and
// associative: the same bits whatever the grid, the batch or the item's place in it, and at P = 1024 stretch.hip's bits.  Unlike
// there, w does not cancel: p wrap(delta - w) depends on which turn the wrap removes.
//
// One wave = one (item, row); lanes run along time, 64 frames per round, the prefix sum is vocoder.h's shuffle scan and the carry
// into the next round is lane 63's total.  j0, gamma and j are uniform in the wave.  Each source is read at two bins and two
// frames; the accompaniment is formed as a complex number at each of its four points before its magnitude is taken, and its angle
// only at the two points of the phase bin j.  Rows whose two source bins both lie above F read nothing.  No LDS, no workspace, no
// atomics; per element 20 loads, 10 sincosf, 3 atan2f, 5 hypotf.
#include "internal.h"
#include "vocoder.h"

namespace {

using namespace vocoder;

// what a row needs of one source: uniform in the wave
struct RowBins {
  long base_p, base_o;      // the song rows of the phase bin j and of the other one of {j0, j0 + 1}
  bool live_p, live_o;      // whether they lie in 1..F
  float wgt_p, wgt_o;       // their weights in the magnitude: {1 - gamma, gamma}
  uint32_t w, w_scaled;     // w and w' as fractions of a turn
};

__device__ __forceinline__ RowBins row_bins(long song_base, int T, int b, int F, int P, int n_fft, int hop, int turn_shift) {
  const int N = b << 10, j0 = N / P, rem = N - j0 * P;
  int j = j0 + (2 * rem >= P ? 1 : 0);                 // the nearest source bin, ties up: (2 N + P) div 2 P
  j = j < 1 ? 1 : (j > F ? F : j);                     // the clamp leaves {j0, j0 + 1} only where j0 > F: there both magnitudes are 0
  const bool up = j > j0;
  const int jp = up ? j0 + 1 : j0, jo = up ? j0 : j0 + 1;
  const float lo = (float)(P - rem) / (float)P, hi = (float)rem / (float)P;     // 1 - gamma and gamma: one rounding each
  RowBins r;
  r.live_p = jp >= 1 && jp <= F;
  r.live_o = jo >= 1 && jo <= F;
  r.base_p = song_base + (long)(jp - 1) * T;
  r.base_o = song_base + (long)(jo - 1) * T;
  r.wgt_p = up ? hi : lo;
  r.wgt_o = up ? lo : hi;
  r.w = (uint32_t)(((long)hop * j) % n_fft) << turn_shift;
  const uint64_t full = (uint64_t)hop * (uint64_t)j * (uint64_t)P;                       // up to 2^32
  r.w_scaled = (uint32_t)(full & (uint64_t)(1024 * n_fft - 1)) << (turn_shift - 10);     // n_fft <= 2048: the shift is >= 11
  return r;
}

// one source of one row over one round of 64 output frames: mag (interpolated in time and bin) and acc (turns) of frame t
template <bool ACC>
__device__ __forceinline__ void vocode(const float* __restrict__ mix_songs, const float* __restrict__ voc_songs,
                                       const float* __restrict__ mix_ang, const float* __restrict__ voc_ang, const RowBins& r, int T,
                                       int s, int q, int P, int t, bool live, int lane, bool first, uint32_t& carry, float& mag,
                                       uint32_t& acc) {
  const int n = t * q, k = s + (n >> 10);
  const float alpha = (float)(n & 1023) * (1.0f / 1024.0f);
  float p0, p1;
  uint32_t a0, a1;
  source_frame<ACC>(mix_songs, voc_songs, mix_ang, voc_ang, r.base_p, k, T, live && r.live_p, p0, a0);
  source_frame<ACC>(mix_songs, voc_songs, mix_ang, voc_ang, r.base_p, k + 1, T, live && r.live_p, p1, a1);
  const float o0 = source_magnitude<ACC>(mix_songs, voc_songs, mix_ang, voc_ang, r.base_o, k, T, live && r.live_o);
  const float o1 = source_magnitude<ACC>(mix_songs, voc_songs, mix_ang, voc_ang, r.base_o, k + 1, T, live && r.live_o);
  const float tm_p = (1.0f - alpha) * p0 + alpha * p1, tm_o = (1.0f - alpha) * o0 + alpha * o1;
  mag = r.wgt_p * tm_p + r.wgt_o * tm_o;
  const int32_t d = (int32_t)(a1 - a0 - r.w);          // the deviation wrapped to [-1/2, 1/2) turn
  const uint32_t scaled = (uint32_t)(((int64_t)d * P) >> 10);                            // p d, rounded down: < 2^-32 turn
  const uint32_t step = live ? r.w_scaled + scaled : 0u;                                 // the advance from frame t to t + 1
  if (first) carry = __shfl(a0, 0, 64);                // acc_0 = arg S[j, s]: frame 0 reads k = s
  const uint32_t incl = wave_scan(step, lane);
  acc = carry + incl - step;                           // exclusive: the advances of frames 0 .. t-1
  carry += __shfl(incl, 63, 64);
}

// PHASE: the two phase tiles are written.
template <bool PHASE>
__global__ __launch_bounds__(256) void crop_pitch_tiles_kernel(
    const float* __restrict__ mix_songs, const float* __restrict__ voc_songs, const float* __restrict__ mix_ang,
    const float* __restrict__ voc_ang, const long long* __restrict__ offset, const int* __restrict__ frames,
    const int* __restrict__ song_v, const int* __restrict__ start_v, const int* __restrict__ song_a, const int* __restrict__ start_a,
    const float* __restrict__ gain_v, const float* __restrict__ gain_a, const int* __restrict__ rate_v, const int* __restrict__ rate_a,
    const int* __restrict__ pitch_v, const int* __restrict__ pitch_a, int B, int F, int seg, int n_fft, int hop,
    float* __restrict__ mix, float* __restrict__ voc, float* __restrict__ mix_phase, float* __restrict__ voc_phase) {
  const int lane = threadIdx.x & 63;
  const long rows = (long)B * F;
  const int turn_shift = 32 - (31 - __builtin_clz((unsigned)n_fft));       // 2^32 / n_fft as a shift (n_fft a power of two)
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * 4) {      // wave-uniform
    const int f = (int)(row % F), b = (int)(row / F);
    const int sv = song_v[b], Tv = frames[sv], stv = start_v[b], qv = rate_v[b], Pv = pitch_v[b];
    int sa = song_a[b], sta = start_a[b], qa = rate_a[b], Pa = pitch_a[b];
    if (sa < 0) sa = sv, sta = stv, qa = qv, Pa = Pv;  // gain item: its own accompaniment, through the same complex path
    const int Ta = frames[sa];
    const RowBins rv = row_bins(offset[sv], Tv, f + 1, F, Pv, n_fft, hop, turn_shift);
    const RowBins ra = row_bins(offset[sa], Ta, f + 1, F, Pa, n_fft, hop, turn_shift);
    const float gv = gain_v[b], ga = gain_a[b];
    uint32_t carry_v = 0u, carry_a = 0u;
    for (int t0 = 0; t0 < seg; t0 += 64) {
      const int t = t0 + lane;
      const bool live = t < seg;
      float mag_v, mag_a;
      uint32_t acc_v, acc_a;
      vocode<false>(mix_songs, voc_songs, mix_ang, voc_ang, rv, Tv, stv, qv, Pv, t, live, lane, t0 == 0, carry_v, mag_v, acc_v);
      vocode<true>(mix_songs, voc_songs, mix_ang, voc_ang, ra, Ta, sta, qa, Pa, t, live, lane, t0 == 0, carry_a, mag_a, acc_a);
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

int pitch_grid(long rows) {                            // stretch.hip's: 8 blocks of 4 waves on each of the 256 CUs; the rest by grid stride
  long g = (rows + 3) / 4;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

extern "C" int svs_crop_pitch_tiles(const float* mix_songs, const float* voc_songs, const float* mix_ang, const float* voc_ang,
                                    const int64_t* offset, const int32_t* frames, const int32_t* song_v, const int32_t* start_v,
                                    const int32_t* song_a, const int32_t* start_a, const float* gain_v, const float* gain_a,
                                    const int32_t* rate_v, const int32_t* rate_a, const int32_t* pitch_v, const int32_t* pitch_a,
                                    int B, int F, int seg, int n_fft, int hop, float* mix, float* voc, float* mix_phase,
                                    float* voc_phase, hipStream_t stream) {
  const char* who = "svs_crop_pitch_tiles";
  SVS_REQUIRE(mix_songs && voc_songs && mix_ang && voc_ang && offset && frames && mix && voc,
              "%s: null pointer (songs, angles, offset, frames, mix or voc; there is no magnitude-only shift)", who);
  SVS_REQUIRE(song_v && start_v && song_a && start_a && gain_v && gain_a && rate_v && rate_a && pitch_v && pitch_a,
              "%s: null table (song_v, start_v, song_a, start_a, gain_v, gain_a, rate_v, rate_a, pitch_v or pitch_a)", who);
  SVS_REQUIRE((mix_phase != nullptr) == (voc_phase != nullptr), "%s: mix_phase and voc_phase must both be given or both be NULL", who);
  SVS_REQUIRE(n_fft == 512 || n_fft == 1024 || n_fft == 2048, "%s: n_fft must be 512, 1024 or 2048, got %d", who, n_fft);
  SVS_REQUIRE(hop > 0 && hop <= n_fft, "%s: hop must be in 1..n_fft, got hop=%d n_fft=%d", who, hop, n_fft);
  SVS_REQUIRE(B > 0 && seg > 0 && seg % 4 == 0, "%s: bad geometry, B and seg must be positive and seg a multiple of 4, got B=%d seg=%d", who, B, seg);
  // rows are bins 1..F of an n_fft-point spectrum: the whole of it (F == n_fft / 2, what augment.crop_pitch passes) or its lowest band
  SVS_REQUIRE(F > 0 && F <= n_fft / 2, "%s: bad geometry, F rows are bins 1..F of an n_fft spectrum: 1 <= F <= n_fft / 2, got F=%d n_fft=%d", who, F, n_fft);
  SVS_REQUIRE(svs_aligned16(mix) && svs_aligned16(voc) && svs_aligned16(mix_phase) && svs_aligned16(voc_phase),
              "%s: bad geometry, the output tiles must be 16-byte aligned", who);
  const dim3 grid(pitch_grid((long)B * F)), block(256);
#define PITCH_LAUNCH(PHASE)                                                                                                        \
  hipLaunchKernelGGL((crop_pitch_tiles_kernel<PHASE>), grid, block, 0, stream, mix_songs, voc_songs, mix_ang, voc_ang,             \
                     (const long long*)offset, frames, song_v, start_v, song_a, start_a, gain_v, gain_a, rate_v, rate_a, pitch_v, \
                     pitch_a, B, F, seg, n_fft, hop, mix, voc, mix_phase, voc_phase)
  if (mix_phase) PITCH_LAUNCH(true);
  else PITCH_LAUNCH(false);
#undef PITCH_LAUNCH
  SVS_CHECK_LAUNCH("crop_pitch_tiles");
  return SVS_OK;
}
