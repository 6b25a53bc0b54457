// Remix and gain augmentation of the training tiles, cut from the spectrograms resident in HBM (the option beside crop_tiles_kernel of
// elementwise.hip, whose song storage, DC-row convention and right zero-padding this keeps).  The reference's SpectrogramDataset
// (train.py:86-143) always pairs a song's mixture with its own vocal; here item b takes its vocal from song A = song_v[b] at column
// start_v[b] and, when song_a[b] >= 0, its accompaniment from song B = song_a[b] at column start_a[b].  Magnitude M and angle phi of
// mixture and vocal are resident and share one per-song norm, so M cis(phi_m) - V cis(phi_v) is the accompaniment's STFT, and frame
// for frame
//     z = g_v V_A cis(phi_vA) + g_a (M_B cis(phi_mB) - V_B cis(phi_vB))
// is the STFT of the re-mixed waveform (the transform is linear per frame):  mix = |z|, mix_phase = arg z, voc = g_v V_A,
// voc_phase = phi_vA.  song_a[b] < 0: the item keeps its own mixture, mix = g_v M_A and voc = g_v V_A (one multiply each), both
// angles copied.  Columns past a song's end read as 0, separately for A and for B.
//
// One launch writes all four tiles; one thread = 4 consecutive frames of one row, per-element loads (a source column starts at any
// frame) and one 16-byte store per tile.  sincosf / atan2f / hypotf are the device library's accurate forms.  The resident angles
// are atan2f results, |phi| <= pi: the kernel tells the compiler so in the device library's own terms, and the large-argument
// (Payne-Hanek) reduction of sincosf is not built: 54 / 60 VGPRs instead of 92 / 96, no scratch either way
// (profiles/augment_resources.txt).
#include "internal.h"

static int augment_grid(long total) {              // 8 blocks of 256 threads on each of the 256 CUs; the rest by grid stride
  long g = (total + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

// m cis(phi) for |phi| <= pi.  The assumption is written as the comparison sincosf itself makes before it reduces (its small-argument
// bound, 2^17), which is the form the optimiser can use to drop the other branch; should a later library compare otherwise, the
// branch is merely kept and the resource file shows the registers it costs.  Only values depend on phi, never an address.
__device__ __forceinline__ void cis_scaled(float m, float phi, float& re, float& im) {
  __builtin_assume(__builtin_fabsf(phi) < 0x1.0p+17f);
  float s, c;
  sincosf(phi, &s, &c);
  re = m * c;
  im = m * s;
}

// ANG: the resident angles are given (remix items possible).  PHASE: the two phase tiles are written.
template <bool ANG, bool PHASE>
__global__ __launch_bounds__(256) void crop_remix_tiles_kernel(
    const float* __restrict__ mix_songs, const float* __restrict__ voc_songs, const float* __restrict__ mix_ang,
    const float* __restrict__ voc_ang, const long long* __restrict__ offset, const int* __restrict__ frames,
    const int* __restrict__ song_v, const int* __restrict__ start_v, const int* __restrict__ song_a, const int* __restrict__ start_a,
    const float* __restrict__ gain_v, const float* __restrict__ gain_a, int B, int F, int seg, float* __restrict__ mix,
    float* __restrict__ voc, float* __restrict__ mix_phase, float* __restrict__ voc_phase) {
  static_assert(ANG || !PHASE, "phase tiles come from the resident angles");
  const int q4 = seg / 4;
  const long total = (long)B * F * q4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int t4 = (int)(i % q4);
    const long row = i / q4;
    const int f = (int)(row % F), b = (int)(row / F);
    const int sv = song_v[b], Tv = frames[sv], stv = start_v[b] + 4 * t4;
    const long srcv = offset[sv] + (long)f * Tv + stv;
    const float gv = gain_v[b];
    int sa = -1;
    if constexpr (ANG) sa = song_a[b];                // the gain-only form never reads song_a / start_a
    f32x4 m = {0.f, 0.f, 0.f, 0.f}, v = m, pm = m, pv = m;
    if (sa < 0) {                                     // gain-only item: the item's own mixture
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = stv + k < Tv;
        m[k] = in ? gv * mix_songs[srcv + k] : 0.f;
        v[k] = in ? gv * voc_songs[srcv + k] : 0.f;
        if constexpr (PHASE) {
          pm[k] = in ? mix_ang[srcv + k] : 0.f;
          pv[k] = in ? voc_ang[srcv + k] : 0.f;
        }
      }
    } else if constexpr (ANG) {                       // remix item: vocal of A over the accompaniment of B
      const int Ta = frames[sa], sta = start_a[b] + 4 * t4;
      const long srca = offset[sa] + (long)f * Ta + sta;
      const float ga = gain_a[b];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in_v = stv + k < Tv, in_a = sta + k < Ta;
        const float VA = in_v ? gv * voc_songs[srcv + k] : 0.f;
        const float phv = in_v ? voc_ang[srcv + k] : 0.f;
        const float MB = in_a ? mix_songs[srca + k] : 0.f, VB = in_a ? voc_songs[srca + k] : 0.f;
        const float phmB = in_a ? mix_ang[srca + k] : 0.f, phvB = in_a ? voc_ang[srca + k] : 0.f;
        float vr, vi, mr, mi, br, bi;
        cis_scaled(VA, phv, vr, vi);
        cis_scaled(MB, phmB, mr, mi);
        cis_scaled(VB, phvB, br, bi);
        const float re = vr + ga * (mr - br), im = vi + ga * (mi - bi);
        m[k] = hypotf(re, im);
        v[k] = VA;
        if constexpr (PHASE) {
          pm[k] = atan2f(im, re);
          pv[k] = phv;
        }
      }
    }
    const long dst = row * seg + 4 * t4;
    *(f32x4*)(mix + dst) = m;
    *(f32x4*)(voc + dst) = v;
    if constexpr (PHASE) {
      *(f32x4*)(mix_phase + dst) = pm;
      *(f32x4*)(voc_phase + dst) = pv;
    }
  }
}

extern "C" int svs_crop_remix_tiles(const float* mix_songs, const float* voc_songs, const float* mix_ang, const float* voc_ang,
                                    const int64_t* offset, const int32_t* frames, const int32_t* song_v, const int32_t* start_v,
                                    const int32_t* song_a, const int32_t* start_a, const float* gain_v, const float* gain_a, int B,
                                    int F, int seg, float* mix, float* voc, float* mix_phase, float* voc_phase, hipStream_t stream) {
  const char* who = "svs_crop_remix_tiles";
  SVS_REQUIRE(mix_songs && voc_songs && offset && frames && mix && voc, "%s: null pointer (songs, offset, frames, mix or voc)", who);
  SVS_REQUIRE(song_v && start_v && song_a && start_a && gain_v && gain_a, "%s: null table (song_v, start_v, song_a, start_a, gain_v or gain_a)", who);
  SVS_REQUIRE((mix_ang != nullptr) == (voc_ang != nullptr), "%s: mix_ang and voc_ang must both be given or both be NULL", who);
  SVS_REQUIRE((mix_phase != nullptr) == (voc_phase != nullptr), "%s: mix_phase and voc_phase must both be given or both be NULL", who);
  SVS_REQUIRE(!mix_phase || mix_ang, "%s: phase outputs need the angle sources (mix_ang, voc_ang)", who);
  SVS_REQUIRE(B > 0 && F > 0 && seg > 0 && seg % 4 == 0, "%s: bad geometry, B, F, seg must be positive and seg a multiple of 4, got B=%d F=%d seg=%d", who, B, F, seg);
  SVS_REQUIRE(svs_aligned16(mix) && svs_aligned16(voc) && svs_aligned16(mix_phase) && svs_aligned16(voc_phase),
              "%s: bad geometry, the output tiles must be 16-byte aligned", who);
  const dim3 grid(augment_grid((long)B * F * (seg / 4))), block(256);
#define AUGMENT_LAUNCH(ANG, PHASE)                                                                                                   \
  hipLaunchKernelGGL((crop_remix_tiles_kernel<ANG, PHASE>), grid, block, 0, stream, mix_songs, voc_songs, mix_ang, voc_ang,          \
                     (const long long*)offset, frames, song_v, start_v, song_a, start_a, gain_v, gain_a, B, F, seg, mix, voc, mix_phase, \
                     voc_phase)
  if (!mix_ang) AUGMENT_LAUNCH(false, false);
  else if (!mix_phase) AUGMENT_LAUNCH(true, false);
  else AUGMENT_LAUNCH(true, true);
#undef AUGMENT_LAUNCH
  SVS_CHECK_LAUNCH("crop_remix_tiles");
  return SVS_OK;
}
