// Full-band stems (include/svs_hip.h: svs_fullband_*).  The network runs at 8,192 Hz, so a stem that is up-sampled to the file's
// rate is empty above 4,096 Hz.  Here the band the network never saw, hi = x - U(y) (x the file's PCM, y the signal the network was
// given, U the up-sampling FIR of svs_resample_poly), is shared out between the stems in the time domain at the file's rate:
//
//   out_s[c][i] = norm[c] * U(v_s[c])[i] + g_s[c](i) * hi[c][i],      g_vocal = g,  g_accompaniment = 1 - g,
//
// with g the network's own mask in the highest band it has (svs_fullband_gains: per frame, the magnitude-weighted mean of the mask
// over the top rows / FB_TOP_DIV rows of the tile layout), interpolated linearly between frame centres; or g = 0 (gf == NULL), which
// hands the whole band to the accompaniment.
//
// svs_fullband_mix is resample_poly_kernel's walk (resample_plan.h: the same plan, tap rows in LDS, (n0, pos % up) increments and the
// k = 0 .. T-1 fmaf chain) over up to three planar rows at once -- the stems and y of ONE channel, whose input indices are identical,
// staged side by side in LDS -- so every accumulator is bitwise the float svs_resample_poly writes for that row; the PCM sample, the
// gain and the two products follow in registers and each output is written once.  A segment's outputs start at m * up + q0, which is
// 16-byte aligned for no up that occurs (11025, 375: odd), so the stores are one dword per lane, 256 contiguous bytes per wave.
#include "resample_plan.h"

namespace {

constexpr int FB_TOP_DIV = 4;        // the top rows / 4 rows of the tiles carry the gain (3 to 4 kHz at the default geometry)
constexpr int FB_COLS = 128;         // threads of a gains block: one per frame of a 128-frame tile
constexpr int FB_MAX_CH = 8;

// gf[c][t] = sum_r mask * mag / sum_r mag over the top rows, r ascending; the plain mean of the mask where sum_r mag == 0
__global__ void __launch_bounds__(FB_COLS) fullband_gains_kernel(const float* __restrict__ tiles, const float* __restrict__ mask,
                                                                 int64_t chan_stride, int rows, int seg, int frames,
                                                                 float* __restrict__ gf) {
  const int tile = blockIdx.x, c = blockIdx.y;
  const int top = rows / FB_TOP_DIV;
  const int64_t base = (int64_t)c * chan_stride + ((int64_t)tile * rows + (rows - top)) * seg;
  for (int col = threadIdx.x; col < seg; col += FB_COLS) {
    const int64_t t = (int64_t)tile * seg + col;
    if (t >= frames) return;                                // the padded frames of the last tile (col ascends: the rest are padded too)
    const float* a = tiles + base + col;
    const float* m = mask + base + col;
    float num = 0.0f, den = 0.0f, msum = 0.0f;
    for (int r = 0; r < top; ++r) {
      const float av = a[(int64_t)r * seg], mv = m[(int64_t)r * seg];
      num = fmaf(mv, av, num);
      den += av;
      msum += mv;
    }
    gf[(int64_t)c * frames + t] = den == 0.0f ? msum / (float)top : num / den;
  }
}

struct FbArgs {
  const float* stems; int64_t ld_stem, ld_in, n_in;        // stem s, channel c at stems + s*ld_stem + c*ld_in
  const float* y; int64_t ld_y;
  const void* pcm; int fmt, channels; int64_t n_pcm;
  const float* table; int T, up, down; int64_t half;
  const float* norm; const float* gf; int frames, invert;
  int64_t den, gq, gr;                                     // up * hop; what one step adds to (frame, remainder) of i*down / den
  float* out; int64_t ld_out, ld_out_stem, n_out;
  RsPlan p;
};

template <int NS>
__global__ void __launch_bounds__(RS_THREADS) fullband_mix_kernel(const FbArgs a) {
  constexpr int NR = NS + 1;                               // rows staged: the stems, then y
  extern __shared__ __attribute__((aligned(16))) float fb_smem[];
  const RsPlan& p = a.p;
  float* taps = fb_smem;                                   // [T][Wt]
  float* xs = fb_smem + (size_t)p.Wt * a.T;                // [S][NR][span]
  const int t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * (p.nqb > 1 ? p.W : 0);
  const int lseg = p.nqb > 1 ? (int)min((int64_t)p.W, a.up - q0) : p.W;
  const int seg = t / p.W, r = t % p.W;
  const bool active = seg < p.S && r < lseg;
  const int c = blockIdx.z;
  const float* src[NR];
#pragma unroll
  for (int s = 0; s < NS; ++s) src[s] = a.stems + (int64_t)s * a.ld_stem + (int64_t)c * a.ld_in;
  src[NS] = a.y + (int64_t)c * a.ld_y;
  const float* gfc = a.gf ? a.gf + (int64_t)c * a.frames : nullptr;
  const float norm = a.norm[c];

  for (int e = t; e < p.Wt * a.T; e += RS_THREADS) {       // this block's tap rows
    const int k = e / p.Wt, q = e % p.Wt;
    taps[e] = q0 + q < a.up ? a.table[(int64_t)k * a.up + q0 + q] : 0.0f;
  }

  const int64_t it0 = (int64_t)blockIdx.y * p.ipc;
  const int64_t it1 = min(it0 + p.ipc, p.nsteps);
  int64_t i_f = ((it0 * p.S + seg) * p.stride) + q0;
  int64_t n0f, remf, n0, rem, kf, krem;
  {
    const int64_t posf = i_f * a.down + a.half;
    n0f = posf / a.up; remf = posf % a.up;
    const int64_t pos = posf + (int64_t)r * a.down;
    n0 = pos / a.up; rem = pos % a.up;
    const int64_t num = (i_f + r) * a.down;                // the frame coordinate u = i * down / (up * hop), in integers
    kf = num / a.den; krem = num % a.den;
  }
  const float* tp = taps + r % p.Wt;
  float* xseg = xs + (size_t)seg * NR * p.span;
  const int64_t di = (int64_t)p.S * p.stride;
  const float fden = (float)a.den;

  for (int64_t it = it0; it < it1; ++it) {
    const bool live = active && i_f < a.n_out;
    __syncthreads();                                       // taps complete (first step); xs free again (later steps)
    if (live) {
      const int64_t lo = n0f - (a.T - 1);
      for (int e = r; e < p.span; e += lseg) {
        const int64_t j = lo + e;
        const bool in = j >= 0 && j < a.n_in;
#pragma unroll
        for (int s = 0; s < NR; ++s) xseg[s * p.span + e] = in ? src[s][j] : 0.0f;
      }
    }
    __syncthreads();
    if (live && i_f + r < a.n_out) {
      const int64_t i = i_f + r;
      const float* xp = xseg + (int)(n0 - n0f) + a.T - 1;
      float acc[NR];
#pragma unroll
      for (int s = 0; s < NR; ++s) acc[s] = 0.0f;
#pragma unroll 4
      for (int k = 0; k < a.T; ++k) {
        const float tap = tp[(size_t)k * p.Wt];
#pragma unroll
        for (int s = 0; s < NR; ++s) acc[s] = fmaf(xp[s * p.span - k], tap, acc[s]);
      }
      const float x = i < a.n_pcm ? rs_cvt(a.pcm, a.fmt, i * a.channels + c) : 0.0f;
      const float hi = x - acc[NS];
      float g = 0.0f;
      if (gfc) {
        const int64_t last = a.frames - 1;
        const float g0 = gfc[min(kf, last)], g1 = gfc[min(kf + 1, last)];
        g = fmaf((float)krem / fden, g1 - g0, g0);
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const float gs = (s == 0 && !a.invert) ? g : 1.0f - g;
        a.out[(int64_t)s * a.ld_out_stem + (int64_t)c * a.ld_out + i] = fmaf(gs, hi, norm * acc[s]);
      }
    }
    i_f += di;
    n0f += p.dq; remf += p.dr; if (remf >= a.up) { remf -= a.up; ++n0f; }
    n0 += p.dq; rem += p.dr; if (rem >= a.up) { rem -= a.up; ++n0; }
    kf += a.gq; krem += a.gr; if (krem >= a.den) { krem -= a.den; ++kf; }
  }
}

}  // namespace

extern "C" int svs_fullband_gains(const float* tiles, const float* mask, int64_t chan_stride, int channels, int n_tiles, int rows, int seg,
                                  int frames, float* gf, hipStream_t stream) {
  SVS_REQUIRE(channels >= 1 && channels <= 65535 && n_tiles >= 1 && rows >= 1 && seg >= 1 && frames >= 1,
              "svs_fullband_gains: all sizes must be positive, got channels=%d n_tiles=%d rows=%d seg=%d frames=%d", channels, n_tiles, rows,
              seg, frames);
  SVS_REQUIRE(rows % FB_TOP_DIV == 0, "svs_fullband_gains: rows must be a multiple of %d (the top rows / %d carry the gain), got %d",
              FB_TOP_DIV, FB_TOP_DIV, rows);
  SVS_REQUIRE((int64_t)n_tiles * seg < ((int64_t)1 << 31), "svs_fullband_gains: n_tiles * seg must stay below 2^31, got %d * %d", n_tiles, seg);
  SVS_REQUIRE(frames <= (int64_t)n_tiles * seg && frames > (int64_t)(n_tiles - 1) * seg,
              "svs_fullband_gains: frames %d do not end in the last of %d tiles of %d frames", frames, n_tiles, seg);
  SVS_REQUIRE(chan_stride >= (int64_t)n_tiles * rows * seg, "svs_fullband_gains: chan_stride must be at least n_tiles * rows * seg = %lld, got %lld",
              (long long)n_tiles * rows * seg, (long long)chan_stride);
  SVS_REQUIRE(tiles && mask && gf, "svs_fullband_gains: null pointer");
  hipLaunchKernelGGL(fullband_gains_kernel, dim3((unsigned)n_tiles, (unsigned)channels), dim3(FB_COLS), 0, stream, tiles, mask, chan_stride,
                     rows, seg, frames, gf);
  SVS_CHECK_LAUNCH("fullband_gains");
  return SVS_OK;
}

extern "C" int svs_fullband_mix(const float* stems, int nstems, int64_t ld_stem, int64_t ld_in, const float* y, int64_t ld_y, int channels,
                                int64_t n_in, const void* pcm, int pcm_fmt, int64_t n_pcm, const void* table, int ntaps, int up, int down,
                                const float* norm, const float* gf, int frames, int hop, int invert, float* out, int64_t ld_out,
                                int64_t ld_out_stem, hipStream_t stream) {
  SVS_REQUIRE(nstems == 1 || nstems == 2, "svs_fullband_mix: nstems %d (1 or 2)", nstems);
  SVS_REQUIRE(channels >= 1 && channels <= FB_MAX_CH, "svs_fullband_mix: channels %d (1..%d)", channels, FB_MAX_CH);
  SVS_REQUIRE(!invert || nstems == 1, "svs_fullband_mix: invert names the accompaniment as the ONE stem; two stems are vocal, accompaniment");
  SVS_REQUIRE(pcm_fmt == RS_F32 || pcm_fmt == RS_I16 || pcm_fmt == RS_I32, "svs_fullband_mix: pcm_fmt %d (0 float32, 1 int16, 2 int32)", pcm_fmt);
  SVS_REQUIRE(rs_filter_ok(ntaps, up, down), "svs_fullband_mix: bad filter (need an odd number of taps, 1 <= up, down <= 2^24)");
  SVS_REQUIRE(frames >= 1 && hop >= 1 && hop <= (1 << 20), "svs_fullband_mix: frames %d (>= 1), hop %d (1..2^20)", frames, hop);
  const int64_t n_out = svs_resample_out_len(n_in, up, down);
  SVS_REQUIRE(n_in >= 1 && n_out >= 1, "svs_fullband_mix: n_in %lld out of range", (long long)n_in);
  SVS_REQUIRE(n_pcm >= 0 && n_pcm <= INT64_MAX / FB_MAX_CH, "svs_fullband_mix: n_pcm %lld out of range", (long long)n_pcm);
  SVS_REQUIRE(ld_in >= n_in && ld_y >= n_in, "svs_fullband_mix: ld_in %lld / ld_y %lld are shorter than a row (%lld)", (long long)ld_in,
              (long long)ld_y, (long long)n_in);
  SVS_REQUIRE(nstems == 1 || ld_stem >= ld_in * channels, "svs_fullband_mix: ld_stem %lld is shorter than a stem (%lld x %d)",
              (long long)ld_stem, (long long)ld_in, channels);
  SVS_REQUIRE(ld_out >= n_out, "svs_fullband_mix: ld_out %lld < n_out %lld", (long long)ld_out, (long long)n_out);
  SVS_REQUIRE(nstems == 1 || ld_out_stem >= ld_out * channels, "svs_fullband_mix: ld_out_stem %lld is shorter than a stem (%lld x %d)",
              (long long)ld_out_stem, (long long)ld_out, channels);
  SVS_REQUIRE(stems && y && pcm && table && norm && out, "svs_fullband_mix: null pointer");
  FbArgs a{};
  a.stems = stems; a.ld_stem = ld_stem; a.ld_in = ld_in; a.n_in = n_in; a.y = y; a.ld_y = ld_y;
  a.pcm = pcm; a.fmt = pcm_fmt; a.channels = channels; a.n_pcm = n_pcm;
  a.table = (const float*)table; a.T = rs_taps_per_phase(ntaps, up); a.up = up; a.down = down; a.half = (ntaps - 1) / 2;
  a.norm = norm; a.gf = gf; a.frames = frames; a.invert = invert ? 1 : 0;
  a.out = out; a.ld_out = ld_out; a.ld_out_stem = ld_out_stem; a.n_out = n_out;
  SVS_REQUIRE(rs_plan(n_out, a.T, up, down, channels, nstems + 1, &a.p),
              "svs_fullband_mix: %d taps per output at %d/%d with %d rows do not fit the LDS", a.T, up, down, nstems + 1);
  SVS_REQUIRE(a.p.chunks <= 65535, "svs_fullband_mix: grid too large");
  a.den = (int64_t)up * hop;
  const int64_t dnum = (int64_t)a.p.S * a.p.stride * down;
  a.gq = dnum / a.den; a.gr = dnum % a.den;
  const void* kernel = nstems == 2 ? (const void*)fullband_mix_kernel<2> : (const void*)fullband_mix_kernel<1>;
  SVS_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.p.lds));
  void* args[] = {(void*)&a};
  SVS_HIP(hipLaunchKernel(kernel, dim3((unsigned)a.p.nqb, (unsigned)a.p.chunks, (unsigned)channels), dim3(RS_THREADS), args, a.p.lds, stream));
  return SVS_OK;
}
