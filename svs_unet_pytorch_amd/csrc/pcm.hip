// 24-bit PCM in and out, and TPDF dither for the written stems (include/svs_hip.h: svs_pcm24_widen, svs_pcm_encode_dither).
//
// Replaces nothing in the reference -- it writes 16-bit through libsndfile (data.py:166) and reads through librosa -- but two host
// passes of this project: scipy widening every 3-byte sample of a 24-bit file to int32 before the copy to the device, and the
// missing 24-bit / dithered writer.  The float64 / integer definitions are svs_unet_pytorch_amd/pcm.py.
//
// Layout.  Both kernels stream: no LDS, no atomics, 64-bit indices, a grid-stride walk over groups of four.
//   widen   a thread takes 4 samples: 12 contiguous bytes in (one 3-dword load; lane i at base + 12 i, so a wave's load is one
//           contiguous 768-byte run) and one 16-byte store out (a contiguous KiB per wave).  The 16-sample form (three 16-byte
//           loads, four 16-byte stores) puts 48 / 64 bytes between neighbouring lanes of one instruction and needs a 16-byte aligned
//           source; the 4-sample form needs 4, so any slice of a device buffer that starts at a multiple of 4 samples will do.
//   encode  a thread owns 4 consecutive frames of every channel: one 16-byte load per channel row (scalar loads where the rows
//           are not 16-byte aligned) and 3 * channels whole dwords out at 24 bits, 2 * channels at 16, as 16- or 8-byte stores
//           where that count is a multiple of 4 or 2 and `out` is 16-byte aligned.  The last frames % 4 frames (samples % 4 on the
//           way in) go by bytes, from one thread.
#include "common.h"

namespace {

constexpr int PCM_THREADS = 256;
constexpr int PCM_MAX_BLOCKS = 2048;
constexpr int PCM_MAX_CH = 8;

typedef uint32_t pcm_u32x3 __attribute__((ext_vector_type(3)));
typedef pcm_u32x3 PcmTriple __attribute__((aligned(4)));      // three dwords at a 4-byte aligned address: one global_load_dwordx3

__global__ void __launch_bounds__(PCM_THREADS) pcm24_widen_kernel(const uint8_t* __restrict__ packed, int64_t n, int32_t* __restrict__ out) {
  const int64_t groups = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * PCM_THREADS;
  for (int64_t g = (int64_t)blockIdx.x * PCM_THREADS + threadIdx.x; g <= groups; g += stride) {
    if (g < groups) {
      const pcm_u32x3 t = *reinterpret_cast<const PcmTriple*>(packed + g * 12);
      uint4 o;
      o.x = t.x << 8;
      o.y = ((t.x >> 24) << 8) | (t.y << 16);
      o.z = ((t.y >> 16) << 8) | (t.z << 24);
      o.w = t.z & 0xFFFFFF00u;
      *reinterpret_cast<uint4*>(out + g * 4) = o;
    } else {                                                  // the last n % 4 samples, by bytes
      for (int64_t e = groups * 4; e < n; ++e) {
        const uint8_t* b = packed + e * 3;
        out[e] = (int32_t)(((uint32_t)b[0] << 8) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 24));
      }
    }
  }
}

struct PcmEncArgs {
  const float* x; int64_t frames, ld_in;
  const float* gain; int dither; uint32_t seed; int64_t first_frame;
  void* out; int vec_in, vec_out;
};

__device__ __forceinline__ float pcm_uniform(uint32_t seed, uint64_t m) { return (float)(svs_u32(seed, m) >> 8) * 0x1p-24f; }

// one sample: v after the gain, d the dither in LSB -> the integer that is written
template <int BITS>
__device__ __forceinline__ int32_t pcm_quantise(float v, float d, bool dithered) {
  if (BITS == 16 && !dithered) {                              // svs_resample_encode's I16 rule, bit for bit
    const float s = rintf(v * 32767.0f);
    if (s != s) return 0;
    return (int32_t)fminf(fmaxf(s, -32768.0f), 32767.0f);
  }
  constexpr double Q = (double)((1 << (BITS - 1)) - 1);
  const double s = rint((double)v * Q + (double)d);
  if (s != s) return 0;
  return (int32_t)fmin(fmax(s, -(Q + 1.0)), Q);
}

// the dither of frame F (absolute), channel c.  carry: the high-passed form's u(F * channels + c) on entry, u((F + 1) * channels + c)
// on return, so a thread that walks consecutive frames of a channel hashes every shared uniform once
template <int NCH>
__device__ __forceinline__ float pcm_dither(const PcmEncArgs& a, uint64_t F, int c, float* carry) {
  if (a.dither == 1) {
    const uint64_t m = 2 * (F * NCH + c);
    return pcm_uniform(a.seed, m) - pcm_uniform(a.seed, m + 1);
  }
  if (a.dither == 2) {                                        // first difference of one uniform sequence per channel
    const float hi = pcm_uniform(a.seed, (F + 1) * NCH + c);
    const float d = hi - *carry;
    *carry = hi;
    return d;
  }
  return 0.0f;
}

template <int NCH, int BITS>
__global__ void __launch_bounds__(PCM_THREADS) pcm_encode_dither_kernel(const PcmEncArgs a) {
  constexpr int NS = 4 * NCH;                                 // samples of a thread's four frames, frame-major
  constexpr int ND = NS * (BITS / 8) / 4;                     // the whole dwords they fill
  constexpr int VW = ND % 4 == 0 ? 4 : ND % 2 == 0 ? 2 : 1;
  const int64_t groups = a.frames >> 2;
  const int64_t stride = (int64_t)gridDim.x * PCM_THREADS;
  const bool dithered = a.dither != 0;
  float g[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) g[c] = a.gain ? a.gain[c] : 1.0f;

  for (int64_t grp = (int64_t)blockIdx.x * PCM_THREADS + threadIdx.x; grp <= groups; grp += stride) {
    const uint64_t F0 = (uint64_t)(a.first_frame + grp * 4);
    if (grp < groups) {
      int32_t s[NS];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const float* row = a.x + (int64_t)c * a.ld_in + grp * 4;
        float v[4];
        if (a.vec_in) {
          const float4 q = *reinterpret_cast<const float4*>(row);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = row[i];
        }
        float carry = a.dither == 2 ? pcm_uniform(a.seed, F0 * NCH + c) : 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float d = pcm_dither<NCH>(a, F0 + i, c, &carry);
          s[i * NCH + c] = pcm_quantise<BITS>(a.gain ? v[i] * g[c] : v[i], d, dithered);
        }
      }
      uint32_t w[ND];
#pragma unroll
      for (int k = 0; k < ND; ++k) w[k] = 0u;
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        if (BITS == 16) {
          w[k >> 1] |= ((uint32_t)s[k] & 0xFFFFu) << (16 * (k & 1));
        } else {
          const uint32_t u = (uint32_t)s[k] & 0xFFFFFFu;
          const int word = (24 * k) >> 5, sh = (24 * k) & 31;
          w[word] |= u << sh;
          if (sh > 8) w[word + 1] |= u >> (32 - sh);
        }
      }
      uint32_t* o = (uint32_t*)a.out + grp * ND;
      if (VW == 4 && a.vec_out) {
#pragma unroll
        for (int k = 0; k < ND; k += 4) *reinterpret_cast<uint4*>(o + k) = make_uint4(w[k], w[k + 1], w[k + 2], w[k + 3]);
      } else if (VW == 2 && a.vec_out) {
#pragma unroll
        for (int k = 0; k < ND; k += 2) *reinterpret_cast<uint2*>(o + k) = make_uint2(w[k], w[k + 1]);
      } else {
#pragma unroll
        for (int k = 0; k < ND; ++k) o[k] = w[k];
      }
    } else {                                                  // the last frames % 4 frames, by bytes
      uint8_t* o = (uint8_t*)a.out + groups * 4 * NCH * (BITS / 8);
      for (int c = 0; c < NCH; ++c) {
        float carry = a.dither == 2 ? pcm_uniform(a.seed, F0 * NCH + c) : 0.0f;
        for (int64_t i = groups * 4; i < a.frames; ++i) {
          const int r = (int)(i - groups * 4);
          const float x = a.x[(int64_t)c * a.ld_in + i];
          const float d = pcm_dither<NCH>(a, F0 + r, c, &carry);
          const uint32_t u = (uint32_t)pcm_quantise<BITS>(a.gain ? x * g[c] : x, d, dithered);
          uint8_t* p = o + (r * NCH + c) * (BITS / 8);
          p[0] = (uint8_t)u; p[1] = (uint8_t)(u >> 8);
          if (BITS == 24) p[2] = (uint8_t)(u >> 16);
        }
      }
    }
  }
}

template <int BITS>
const void* pcm_encode_kernel_for(int channels) {
  switch (channels) {
    case 1: return (const void*)pcm_encode_dither_kernel<1, BITS>;
    case 2: return (const void*)pcm_encode_dither_kernel<2, BITS>;
    case 3: return (const void*)pcm_encode_dither_kernel<3, BITS>;
    case 4: return (const void*)pcm_encode_dither_kernel<4, BITS>;
    case 5: return (const void*)pcm_encode_dither_kernel<5, BITS>;
    case 6: return (const void*)pcm_encode_dither_kernel<6, BITS>;
    case 7: return (const void*)pcm_encode_dither_kernel<7, BITS>;
    case 8: return (const void*)pcm_encode_dither_kernel<8, BITS>;
  }
  return nullptr;
}

unsigned pcm_grid(int64_t items) {
  const int64_t blocks = (items + PCM_THREADS - 1) / PCM_THREADS;
  return (unsigned)(blocks < PCM_MAX_BLOCKS ? blocks : PCM_MAX_BLOCKS);
}

}  // namespace

extern "C" int svs_pcm24_widen(const void* packed, int64_t n_samples, int32_t* out, hipStream_t stream) {
  SVS_REQUIRE(packed && out, "svs_pcm24_widen: null pointer");
  SVS_REQUIRE(n_samples >= 1 && n_samples <= INT64_MAX / 4, "svs_pcm24_widen: n_samples %lld out of range", (long long)n_samples);
  SVS_REQUIRE((((uintptr_t)packed) & 3u) == 0 && svs_aligned16(out),
              "svs_pcm24_widen: packed must be 4-byte aligned and out 16-byte aligned");
  hipLaunchKernelGGL(pcm24_widen_kernel, dim3(pcm_grid(n_samples / 4 + 1)), dim3(PCM_THREADS), 0, stream, (const uint8_t*)packed, n_samples, out);
  SVS_CHECK_LAUNCH("pcm24_widen");
  return SVS_OK;
}

extern "C" int svs_pcm_encode_dither(const float* x, int channels, int64_t frames, int64_t ld_in, const float* gain, int bits, int dither,
                                     uint32_t seed, int64_t first_frame, void* out, hipStream_t stream) {
  SVS_REQUIRE(x && out, "svs_pcm_encode_dither: null pointer");
  SVS_REQUIRE(bits == 16 || bits == 24, "svs_pcm_encode_dither: bits %d (16 or 24)", bits);
  SVS_REQUIRE(dither >= 0 && dither <= 2, "svs_pcm_encode_dither: dither %d (0 none, 1 tpdf, 2 high-passed tpdf)", dither);
  SVS_REQUIRE(channels >= 1 && channels <= PCM_MAX_CH, "svs_pcm_encode_dither: channels %d (1..%d)", channels, PCM_MAX_CH);
  SVS_REQUIRE(frames >= 1 && frames <= (INT64_MAX >> 8), "svs_pcm_encode_dither: frames %lld out of range", (long long)frames);
  SVS_REQUIRE(ld_in >= frames, "svs_pcm_encode_dither: ld_in %lld is shorter than a row (%lld)", (long long)ld_in, (long long)frames);
  SVS_REQUIRE(first_frame >= 0 && first_frame <= (INT64_MAX >> 8) - frames, "svs_pcm_encode_dither: first_frame %lld out of range",
              (long long)first_frame);
  SVS_REQUIRE((((uintptr_t)out) & 3u) == 0, "svs_pcm_encode_dither: out must be 4-byte aligned");
  PcmEncArgs a{};
  a.x = x; a.frames = frames; a.ld_in = ld_in; a.gain = gain; a.dither = dither; a.seed = seed; a.first_frame = first_frame; a.out = out;
  a.vec_in = (svs_aligned16(x) && ld_in % 4 == 0) ? 1 : 0;
  a.vec_out = svs_aligned16(out) ? 1 : 0;
  const void* kernel = bits == 16 ? pcm_encode_kernel_for<16>(channels) : pcm_encode_kernel_for<24>(channels);
  void* args[] = {(void*)&a};
  SVS_HIP(hipLaunchKernel(kernel, dim3(pcm_grid(frames / 4 + 1)), dim3(PCM_THREADS), args, 0, stream));
  return SVS_OK;
}
