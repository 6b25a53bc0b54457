// Windowed STFT / inverse STFT on the GPU (gfx950) as bandwidth kernels.
// Replaces librosa.stft / librosa.magphase / librosa.istft (reference data.py:79-80,100-101,159) and torch.istft
// (train.py:51-58): periodic Hann window of n_fft samples, centred frames with zero padding,
// frames = 1 + n_samples / hop; inverse = irfft, window, overlap-add, divide by the window sum-of-squares, trim
// n_fft/2 from both ends.  Every kernel is a template on N = n_fft, instantiated for 512, 1024 (the reference's config.py:47)
// and 2048 (data.py:24 lets --win_size vary); the numbers in the comments below are those of N = 1024.
//
// Structure (both directions): a 512-thread block owns 16 consecutive frames (hops) of one channel.
//   * FFT: one N-point complex FFT per WAVE in LDS (fft_wave.h: three register-radix passes, no block barriers),
//     and TWO real frames per transform (frame t in the real part, frame t+1 in the imaginary part; the two spectra
//     separate by Hermitian symmetry) -- half the arithmetic of a complex transform per real frame.
//   * Layout: spectrograms are f-major with time fastest ((513, T) files of data.py:107-109, (tiles, 1, 512, 128)
//     network tiles of inference.py:84, (B, 1, 512, 128) training tiles of train.py:138).  A frame is a COLUMN of
//     them, so the 16 frames of a block go through an LDS transpose and every row is written / read as one 64-byte
//     run (the first version did 513 scattered 4-byte accesses per frame).  `SpecLayout` addresses all three forms,
//     DC row dropped or not, so the forward transform writes network tiles directly and the inverse reads them.
//   * Inverse: the 17 frames that touch the block's 16 hops are overlap-added in LDS (even frames, then odd frames:
//     fixed order, no atomics), divided by the window envelope and written once -- no frame buffer in HBM.
//   * Fused around them: mask application (inference.py:100-107) on the inverse's input, per-block |.|max partials
//     for the normalisations of data.py:84-85,162-164, and -- for the differentiable inverse of train.py:33-60 --
//     the transposed operator (`SINK_DMAG`) that maps d(loss)/d(waveform) back to d(loss)/d(mask logit).
// Bound: HBM.  Algorithmic bytes per frame: hop*4 in, 513*4 (+513*8 with phase) out, and the reverse.
#include "internal.h"
#include "fft_wave.h"

#define GROUP 16                  // forward: frames per block (8 waves x 2)
#define SROW (GROUP + 1)          // floats per staged angle row (odd -> conflict-free column access)
#define IGROUP 15                 // inverse: hops per step; they touch 16 frames = 8 waves x 2 (one of 16 transforms is halo)

// Address of (channel c, bin k, frame t) of an f-major spectrogram cut into `seg`-frame tiles of `rows` rows each,
// the first of which is bin `first_bin`:  (513, T) file: seg = T, rows = 513, first_bin = 0;
// network tiles (n, 1, 512, 128): seg = 128, rows = 512, first_bin = 1 (DC row dropped, inference.py:68 / train.py:109).
struct SpecLayout {
  long chan_stride; int seg, rows, first_bin, frames_alloc;      // frames_alloc: columns that exist (>= T: tile padding)
  __device__ __forceinline__ long at(int c, int k, int t) const {
    const int tile = t / seg;
    return (long)c * chan_stride + ((long)tile * rows + (k - first_bin)) * seg + (t - tile * seg);
  }
  // the same as col(c, t) + k * seg: one division per (thread, group) instead of one per element
  __device__ __forceinline__ long col(int c, int t) const {
    const int tile = t / seg;
    return (long)c * chan_stride + ((long)tile * rows - first_bin) * seg + (t - tile * seg);
  }
};

// Window of the forward transform, N = 1024: from the FFT's pass-2 twiddle table (tw2[256 + k] = exp(-2 pi i k / 1024),
// k < 256: exact sincospi entries), by symmetry: an LDS read and three selects instead of a ~40-instruction cospif
__device__ __forceinline__ float hann_tw(const float2* tw2, int m) {
  constexpr int NFFT = 1024;
  const int r = m <= NFFT / 2 ? m : NFFT - m;
  const float c = r < 256 ? tw2[256 + r].x : (r == 256 ? 0.f : -tw2[256 + (512 - r)].x);
  return 0.5f - 0.5f * c;
}
// N = 512 / 2048: the pass-2 tables of those plans hold less than a quarter circle (k < 64 of 512; an eighth of 2048), so the
// window comes from the device-wide table of svs_fft_hann (fft_tables.hip: sin^2(pi m / N) rounded from double, m <= N / 2)
template <int NFFT>
__device__ __forceinline__ float hann_tab(const float* __restrict__ tab, int m) { return tab[m <= NFFT / 2 ? m : NFFT - m]; }
// one-instruction form (v_cos_f32 takes revolutions; absolute error ~1e-6): used where the window also divides out again
// (the inverse's overlap-add / envelope), not for the forward magnitudes
template <int NFFT>
__device__ __forceinline__ float hann_fast(int m) { return 0.5f - 0.5f * __builtin_amdgcn_cosf((float)m * (1.0f / NFFT)); }

// window sum-of-squares at padded position q (= sample index + n_fft/2) for T frames of hop `hop`
template <int NFFT>
__device__ __forceinline__ float envelope_at(int q, int hop, int T) {      // (32-bit: two 64-bit divisions per sample were most of the caller)
  if (q < 0) return 0.f;
  int t1 = (int)((unsigned)q / (unsigned)hop);
  if (t1 > T - 1) t1 = T - 1;
  int t0 = q - (NFFT - 1);
  t0 = t0 <= 0 ? 0 : (int)((unsigned)(t0 + hop - 1) / (unsigned)hop);
  float env = 0.f;
  for (int t = t0; t <= t1; ++t) { const float w = hann_fast<NFFT>(q - t * hop); env += w * w; }
  return env;
}

// The transposes between "a frame = a column" (what a transform works on) and "a row = consecutive frames" (what HBM
// holds) go through the waves' own FFT buffers: wave w keeps the two values (frame 2w, frame 2w+1) of bin k as ONE
// float2 at raw element k + w of its buffer (the + w skews the waves by one bank pair, so the 16 values of a row -- two
// from each of the 8 buffers, BUF * 2 floats apart = 0 mod 32 banks -- come from 16 different banks).
// The second plane of a transposed round (phasors of the odd frames, angles) lies BUF / 2 elements higher: k + w <= N / 2 + 7
// stays below BUF / 2 = N / 2 + N / 32 for every N >= 512.
template <int NFFT>
__device__ __forceinline__ int xpose_at(int wave, int k) { return wave * FftSize<NFFT>::BUF + k + wave; }

// ------------------------------------------------------------------------------------------------
// forward: frames of a real signal -> bins
// ------------------------------------------------------------------------------------------------
// x[s] zero-padded | d_wav[s] / envelope (transpose of the inverse's tail) | stem s of two plus half of what the stems fail to add
// up to, x_s + 0.5 (mix - x_0 - x_1), formed on load (MISI's re-analysis input)
enum { SRC_SIGNAL = 0, SRC_ENVDIV = 1, SRC_MISI = 2 };
// SINK_PHASOR: only the frame-major unit phasors of phase_mode 1, [s][c][t][N / 2 + 1] (re, im), straight from registers: no
// magnitudes, no transposed LDS round, no tile padding, no |.|max (svs_stft_rephase_n)
enum { SINK_MAGPHASE = 0, SINK_DMAG = 1, SINK_PHASOR = 2 };
// SINK_DMAG: whether the angle rows are staged after the transform in the waves' own buffers (no LDS plane of their own)
__host__ __device__ constexpr bool dmag_late_angles(int n_fft) { return n_fft == 2048; }
struct StftArgs {
  const float* y; long n_samples; int channels; int hop; int T;     // T frames per channel
  float* mag; SpecLayout lay;                                       // SINK_MAGPHASE
  float* phase; int phase_mode;                                     // 0 none, 1 frame-major [c][t][513] float2, 2 f-major (513, T) float2
  float* absmax_partial;                                            // [gridDim.y * gridDim.x] or null
  // SINK_DMAG: d_logit[idx] += alpha * d|S| * mix[idx] * mask[idx] * (1 - mask[idx]), all in layout `lay`
  const float* angle; const float* mix; const float* mask; float* d_logit; float alpha;
  const float2* twiddles;                                           // svs_fft_twiddles(N): the device-wide table
  const float* hann;                                                // svs_fft_hann(N), N != 1024
  // SINK_PHASOR: y is (stems, channels, n_samples) with stem_stride floats between the stems, and stem s writes its phasors at
  // phase + s * phase_stem_stride floats; SRC_MISI: msig is the mixture (channels, n_samples)
  const float* msig; long stem_stride; long phase_stem_stride;
};

template <int NFFT, int SRC, int SINK>
__global__ __launch_bounds__(512) void stft_fwd_kernel(StftArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NBIN = NFFT / 2 + 1, NR = NFFT / 128 + 1;   // bins; bins per lane (9 = ceil(513 / 64))
  constexpr int BUF = FftSize<NFFT>::BUF, TW = FftSize<NFFT>::TW;
  float2* const fbuf = (float2*)smem;                       // [8][BUF]
  float2* const tw = fbuf + 8 * BUF;                        // [TW]
  float* const angs = (float*)(tw + TW);                    // SINK_DMAG, N <= 1024 only: [513 * 17]
  // SINK_DMAG at N = 2048: the eight buffers and the twiddles are 157,696 of the CU's 163,840 B, so the 1025 x 17 staged
  // angles (69,700 B) have no room of their own.  They are loaded AFTER the transform instead, into the second plane of the
  // transposed round (BUF / 2 above the first, as phase_mode 2 uses it), once every wave holds its spectra in registers.
  constexpr bool LATE_ANGLES = SINK == SINK_DMAG && dmag_late_angles(NFFT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int stem = SINK == SINK_PHASOR ? (int)blockIdx.y / p.channels : 0;    // SINK_PHASOR: blockIdx.y = stem * channels + channel
  const int c = (int)blockIdx.y - stem * p.channels, t0 = blockIdx.x * GROUP;
  if (SINK == SINK_DMAG && !LATE_ANGLES) {
    const int col = tid & (GROUP - 1), t = t0 + col;
    const long cbase = t < p.T ? p.lay.col(c, t) : 0;
    for (int k = tid >> 4; k < NBIN; k += 512 / GROUP)
      angs[k * SROW + col] = (k >= p.lay.first_bin && t < p.T) ? p.angle[cbase + (long)k * p.lay.seg] : 0.f;
  }
  float2* const buf = fbuf + wave * BUF;
  const int ta = t0 + 2 * wave, tb = ta + 1;
  // ---- frames ta, tb -> z = a + i b (windowed); 4 consecutive samples per lane and step.  The loads are issued first and
  // stay in flight while the twiddle table is built.
  // SRC_MISI reads three streams, stem 0 (ysig), stem 1 and the mixture, and keeps its own stem's sample plus half the residual;
  // SRC_SIGNAL under SINK_PHASOR reads stem `stem` alone
  constexpr bool misi = SRC == SRC_MISI;
  const float* ysig = p.y + (long)c * p.n_samples + (SINK == SINK_PHASOR && !misi ? (long)stem * p.stem_stride : 0);
  const float* const ysig1 = misi ? ysig + p.stem_stride : ysig;
  const float* const ymix = misi ? p.msig + (long)c * p.n_samples : ysig;
  const bool vec_ok = ((p.n_samples | p.hop) & 3) == 0 && ((uintptr_t)p.y & 15u) == 0 &&
                      (SINK != SINK_PHASOR || ((p.stem_stride & 3) == 0 && ((uintptr_t)p.msig & 15u) == 0));
  float v[NFFT / 256][2][4];
#pragma unroll
  for (int r = 0; r < NFFT / 256; ++r) {
    const int m0 = 4 * lane + 256 * r;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t = ta + h;
      const long q0 = (long)t * p.hop + m0, s0 = q0 - NFFT / 2;
      if (t < p.T && vec_ok && s0 >= 0 && s0 + 3 < p.n_samples) {
        const f32x4 x = *(const f32x4*)(ysig + s0);
        if (misi) {
          const f32x4 x1 = *(const f32x4*)(ysig1 + s0), xm = *(const f32x4*)(ymix + s0);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[r][h][j] = (stem ? x1[j] : x[j]) + 0.5f * (xm[j] - x[j] - x1[j]);
        } else {
          v[r][h][0] = x[0]; v[r][h][1] = x[1]; v[r][h][2] = x[2]; v[r][h][3] = x[3];
        }
      } else if (misi) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const long s = s0 + j;
          const bool ok = t < p.T && s >= 0 && s < p.n_samples;
          const float x0 = ok ? ysig[s] : 0.f, x1 = ok ? ysig1[s] : 0.f, xm = ok ? ymix[s] : 0.f;
          v[r][h][j] = (stem ? x1 : x0) + 0.5f * (xm - x0 - x1);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) { const long s = s0 + j; v[r][h][j] = (t < p.T && s >= 0 && s < p.n_samples) ? ysig[s] : 0.f; }
      }
      if (SRC == SRC_ENVDIV) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float env = envelope_at<NFFT>((int)(q0 + j), p.hop, p.T); if (env > 1.1754944e-38f) v[r][h][j] *= __builtin_amdgcn_rcpf(env); }   // (as the inverse itself divides)
      }
    }
  }
  fft_load_twiddles<NFFT>(tw, p.twiddles, tid, 512);
  __syncthreads();                                          // twiddles (and staged angles) are complete
  const float2* const tw2 = tw + FftSize<NFFT>::TW1;
#pragma unroll
  for (int r = 0; r < NFFT / 256; ++r) {
    const int m0 = 4 * lane + 256 * r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float w;
      if constexpr (NFFT == 1024) w = hann_tw(tw2, m0 + j); else w = hann_tab<NFFT>(p.hann, m0 + j);
      buf[fft_pad(m0 + j)] = float2{v[r][0][j] * w, v[r][1][j] * w};
    }
  }
  fft_wave<NFFT>(buf, tw, lane);
  // ---- separate the two spectra, bins k = 0 .. N / 2, into registers (every Z is read before the buffer is reused)
  float2 A[NR], B[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int k = lane + 64 * r;
    A[r] = B[r] = float2{0.f, 0.f};
    if (k > NFFT / 2) continue;
    const float2 zk = buf[fft_pad(k)], zn = buf[fft_pad((NFFT - k) & (NFFT - 1))];
    A[r] = float2{0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)};
    B[r] = float2{0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x)};
  }
  if constexpr (SINK == SINK_PHASOR) {
    // the wave's two frames straight from registers: per r, 64 lanes x 8 B contiguous.  The arithmetic is phase_mode 1's below
    // (v_sqrt_f32 / v_rcp_f32, exactly 1 + 0i where the bin is exactly zero); nothing goes back through LDS, so no barrier follows
    float2* const ph = (float2*)(p.phase + (long)stem * p.phase_stem_stride) + (long)c * p.T * NBIN;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int k = lane + 64 * r;
      if (k > NFFT / 2) continue;
      const float ma = __builtin_amdgcn_sqrtf(A[r].x * A[r].x + A[r].y * A[r].y), mb = __builtin_amdgcn_sqrtf(B[r].x * B[r].x + B[r].y * B[r].y);
      const float ia = __builtin_amdgcn_rcpf(ma), ib = __builtin_amdgcn_rcpf(mb);
      if (ta < p.T) ph[(long)ta * NBIN + k] = ma == 0.f ? float2{1.f, 0.f} : float2{A[r].x * ia, A[r].y * ia};
      if (tb < p.T) ph[(long)tb * NBIN + k] = mb == 0.f ? float2{1.f, 0.f} : float2{B[r].x * ib, B[r].y * ib};
    }
    return;
  }
  fft_wave_sync();                                          // every lane has read Z before the buffer is rewritten below
  if (LATE_ANGLES) {
    // rows in: 16 consecutive frames of a bin = one 64-byte run; thread (k, col) -> second plane of wave col >> 1, component
    // col & 1, so that a wave reads the angles of its two frames back as one float2 (the banks are those of the rows-out read)
    __syncthreads();                                        // every WAVE has read its Z: other waves' threads write into its buffer
    float* const xa = (float*)fbuf;
    const int col = tid & (GROUP - 1), t = t0 + col;
    const long cbase = t < p.T ? p.lay.col(c, t) : 0;
    for (int k = tid >> 4; k < NBIN; k += 512 / GROUP)
      xa[2 * (xpose_at<NFFT>(col >> 1, k) + BUF / 2) + (col & 1)] = (k >= p.lay.first_bin && t < p.T) ? p.angle[cbase + (long)k * p.lay.seg] : 0.f;
    __syncthreads();
  }
  float vmax = 0.f;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int k = lane + 64 * r;
    if (k > NFFT / 2) continue;
    float2 out;
    if (SINK == SINK_MAGPHASE) {
      // v_sqrt_f32 / v_rcp_f32 (1 ulp) instead of the ~12-instruction IEEE sequences: the kernel is VALU-issue-bound
      const float ma = __builtin_amdgcn_sqrtf(A[r].x * A[r].x + A[r].y * A[r].y), mb = __builtin_amdgcn_sqrtf(B[r].x * B[r].x + B[r].y * B[r].y);
      out = float2{ma, mb};
      if (ta < p.T) vmax = fmaxf(vmax, ma);
      if (tb < p.T) vmax = fmaxf(vmax, mb);
      if (p.phase_mode == 1) {                             // unit phasors, 1 + 0i where the bin is exactly zero (librosa.magphase)
        float2* ph = (float2*)p.phase;
        const float ia = __builtin_amdgcn_rcpf(ma), ib = __builtin_amdgcn_rcpf(mb);
        if (ta < p.T) ph[((long)c * p.T + ta) * NBIN + k] = ma == 0.f ? float2{1.f, 0.f} : float2{A[r].x * ia, A[r].y * ia};
        if (tb < p.T) ph[((long)c * p.T + tb) * NBIN + k] = mb == 0.f ? float2{1.f, 0.f} : float2{B[r].x * ib, B[r].y * ib};
      }
    } else {
      // transpose of irfft (1/N, bins 1..511 count twice, imaginary parts of DC / Nyquist are ignored by irfft), then
      // d|S| = Re(conj(e^{i phi}) G)
      const bool edge = (k == 0 || k == NFFT / 2);
      const float ck = edge ? 1.0f / NFFT : 2.0f / NFFT;
      // (the same one-instruction phasors as the inverse it is the transpose of)
      float aa, ab;
      if (LATE_ANGLES) { const float2 a2 = fbuf[xpose_at<NFFT>(wave, k) + BUF / 2]; aa = a2.x; ab = a2.y; }
      else { aa = angs[k * SROW + 2 * wave]; ab = angs[k * SROW + 2 * wave + 1]; }
      const float ra = aa * 0.15915494309189535f, rb = ab * 0.15915494309189535f;
      const float sa = __builtin_amdgcn_sinf(ra), ca = __builtin_amdgcn_cosf(ra), sb = __builtin_amdgcn_sinf(rb), cb = __builtin_amdgcn_cosf(rb);
      out = float2{ck * (A[r].x * ca + (edge ? 0.f : A[r].y * sa)), ck * (B[r].x * cb + (edge ? 0.f : B[r].y * sb))};
    }
    fbuf[xpose_at<NFFT>(wave, k)] = out;
  }
  __syncthreads();
  // ---- rows out: 16 consecutive frames of a bin = one 64-byte run
  const float* const xp = (const float*)fbuf;
  {
    const int col = tid & (GROUP - 1), t = t0 + col;        // a thread keeps its frame: one tile division per thread
    if (t < p.lay.frames_alloc) {
      const long cbase = p.lay.col(c, t);
      for (int k = tid >> 4; k < NBIN; k += 512 / GROUP) {
        if (k < p.lay.first_bin) continue;
        const float v = t < p.T ? xp[2 * xpose_at<NFFT>(col >> 1, k) + (col & 1)] : 0.f;   // tile padding beyond the last frame is written as zeros
        const long idx = cbase + (long)k * p.lay.seg;
        if (SINK == SINK_MAGPHASE) p.mag[idx] = v;
        else if (t < p.T) { const float m = p.mask[idx]; p.d_logit[idx] += p.alpha * v * p.mix[idx] * m * (1.f - m); }
      }
    }
  }
  if (SINK == SINK_MAGPHASE && p.phase_mode == 2) {
    // f-major phasors (the .npy layout of data.py:108-109): a second transposed round, phasor of frame 2w at raw
    // element k + w, of frame 2w+1 at BUF / 2 + k + w (544 + k + w) of the wave's buffer
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int k = lane + 64 * r;
      if (k > NFFT / 2) continue;
      const float ma = sqrtf(A[r].x * A[r].x + A[r].y * A[r].y), mb = sqrtf(B[r].x * B[r].x + B[r].y * B[r].y);
      fbuf[xpose_at<NFFT>(wave, k)] = ma == 0.f ? float2{1.f, 0.f} : float2{A[r].x / ma, A[r].y / ma};
      fbuf[xpose_at<NFFT>(wave, k) + BUF / 2] = mb == 0.f ? float2{1.f, 0.f} : float2{B[r].x / mb, B[r].y / mb};
    }
    __syncthreads();
    float2* ph = (float2*)p.phase;
    for (int e = tid; e < NBIN * GROUP; e += 512) {
      const int k = e / GROUP, col = e - k * GROUP, t = t0 + col;
      if (t < p.T) ph[((long)c * NBIN + k) * p.T + t] = fbuf[xpose_at<NFFT>(col >> 1, k) + (BUF / 2) * (col & 1)];
    }
  }
  if (p.absmax_partial) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
    __syncthreads();
    float* red = (float*)fbuf;
    if (lane == 0) red[wave] = vmax;
    __syncthreads();
    if (tid == 0) {
      float m = red[0];
      for (int w = 1; w < 8; ++w) m = fmaxf(m, red[w]);
      p.absmax_partial[(long)blockIdx.y * gridDim.x + blockIdx.x] = m;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// inverse: bins -> overlap-added signal
// ------------------------------------------------------------------------------------------------
struct IstftArgs {
  const float* mag; SpecLayout lay;
  const float* mask; int invert;                  // optional: |S| = mag * mask (or * (1 - mask)), inference.py:100-107
  const float* phase; int phase_mode;             // 1 frame-major phasors [c][t][513] float2, 3 angles in layout `lay`
  int channels, T, hop;
  float* y; long n_out;                           // (channels, hop * (T - 1))
  long stem_stride;                               // STEMS: stem 1 (mag * (1 - mask)) is written this many floats after stem 0 (mag * mask)
  float* absmax_partial;                          // [channel][group]; STEMS: [stem][channel][group]
  const float2* twiddles;                         // svs_fft_twiddles(N)
};

// A 512-thread block (8 waves) owns the padded samples [hop * t0, hop * (t0 + 15)) of one channel: exactly the 16 frames
// t0-1 .. t0+14 touch them (hop >= n_fft / 2), two per wave.  Inputs are transposed into the waves' buffers (magnitudes as
// raw floats 2(k + w) + (f & 1), angles 1088 floats higher), each wave builds the Hermitian spectrum of Sa + i Sb,
// transforms, and the output threads add the (at most two) frames that cover a sample straight from the buffers and divide
// by the window envelope of the same frames.  No integer division in any per-element loop (a thread keeps its frame /
// walks its samples incrementally); the Hann window comes from the twiddle table.  79,872 B of LDS and <= 128 VGPRs: two
// blocks per CU, so one block's loads overlap the other's transform.
// (Measured alternatives, 240 s stereo: one block per CU with per-element divisions 0.29 ms; persistent blocks with register
// prefetch of the next group, 239 VGPRs, one block per CU 0.165 ms.)
// N = 2048: 157,696 B of LDS, one block per CU (and its 256 VGPRs); N = 512: 39,424 B.
//
// STEMS (svs_istft_stems_n): both stems of a mask from ONE launch, y = istft(mag * mask * phase) and, stem_stride floats higher,
// istft(mag * (1 - mask) * phase).  The block stages magnitude, mask and phasors once and forms both spectra of its two frames;
// the spectra of the second stem wait in registers while the first stem is transformed and written, then go through the same
// buffers.  Same frames per block, same LDS, same transform count as two single-stem launches; half the loads, half the
// staging and one launch.  Each stem is transformed on its own (two frames of ONE stem per transform, as above): a transform
// of vocal + i accompaniment of one frame would leak rounding noise of either stem into the other (the imaginary part of a
// transform of a Hermitian spectrum is ~1e-7 of it, not 0), and a stem whose mask is 0 everywhere must come out as exact zeros.
// The second staged plane (BUF / 2 elements up) holds the second stem's magnitudes (PMODE 1) or the angles (PMODE 3, where the
// second stem's magnitudes follow through the first plane in a second staging step).  The waiting spectra cost 4 NR VGPRs:
// N = 1024 is held to 128 (four waves per SIMD = the two blocks per CU of the single-stem kernel; the compiler's own choice
// was 132 and one block), N = 2048 spills 9-11 of its 256 to scratch.
template <int NFFT, int PMODE, int STEMS = 0>               // phase_mode as a template argument: only its registers exist
__global__ __launch_bounds__(512, NFFT == 2048 ? 1 : (STEMS && NFFT == 1024 ? 4 : 2)) void istft_kernel(IstftArgs p, int ngroups) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NBIN = NFFT / 2 + 1, NR = NFFT / 128 + 1;
  constexpr int BUF = FftSize<NFFT>::BUF, NW = 8, NF = 2 * NW;
  constexpr int NIT = (NBIN * NF + 511) / 512;             // staged values per thread (17: 513 * 16 / 512)
  float2* const fbuf = (float2*)smem;                       // [8][BUF]
  float2* const tw = fbuf + NW * BUF;
  float* const raw = (float*)fbuf;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x, c = g / ngroups, t0 = (g - c * ngroups) * IGROUP;
  float2* const buf = fbuf + wave * BUF;
  // 32-bit byte offsets into buffer descriptors (one VGPR per address in flight; the host checks that the views stay below
  // 2 GiB); an out-of-range element is pointed past num_records and reads as zero
  constexpr unsigned OOB = 0x80000000u;
  const __amdgpu_buffer_rsrc_t rmag = __builtin_amdgcn_make_buffer_rsrc((void*)p.mag, 0, OOB, 0x00020000);
  const __amdgpu_buffer_rsrc_t rmask = __builtin_amdgcn_make_buffer_rsrc((void*)(p.mask ? p.mask : p.mag), 0, OOB, 0x00020000);
  const __amdgpu_buffer_rsrc_t rph = __builtin_amdgcn_make_buffer_rsrc((void*)p.phase, 0, OOB, 0x00020000);
  const bool has_mask = p.mask != nullptr;
  // ---- loads first (in flight while the twiddles are built): this thread's frame column, and this wave's phasors
  float sm[NIT], sa[PMODE == 3 ? NIT : 1], sm2[STEMS ? NIT : 1];
  {
    const int tf = t0 - 1 + (tid & (NF - 1));               // a thread keeps its frame: one tile division per thread
    const bool tok = tf >= 0 && tf < p.T;
    const unsigned cbase = tok ? (unsigned)p.lay.col(c, tf) : 0u;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int k = (tid >> 4) + (512 / NF) * it;
      const bool ok = tok && k < NBIN && k >= p.lay.first_bin;
      const unsigned off = ok ? (cbase + (unsigned)(k * p.lay.seg)) * 4u : OOB;
      float m = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmag, (int)off, 0, 0));
      if (STEMS) {
        const float mk = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmask, (int)off, 0, 0));
        sm2[STEMS ? it : 0] = m * (1.f - mk);
        m *= mk;
      } else if (has_mask) {
        const float mk = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmask, (int)off, 0, 0));
        m *= p.invert ? 1.f - mk : mk;
      }
      sm[it] = m;
      if (PMODE == 3) sa[PMODE == 3 ? it : 0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rph, (int)off, 0, 0));
    }
  }
  float2 pa[PMODE == 1 ? NR : 1], pb[PMODE == 1 ? NR : 1];
  const int ta = t0 - 1 + 2 * wave;
  if (PMODE == 1) {
    struct F2 { float x, y; };                              // (bit_cast: whatever 8-byte type the builtin returns)
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int k = lane + 64 * r;
      const bool oka = k <= NFFT / 2 && ta >= 0 && ta < p.T, okb = k <= NFFT / 2 && ta + 1 >= 0 && ta + 1 < p.T;
      const unsigned oa = oka ? (unsigned)(((long)c * p.T + ta) * NBIN + k) * 8u : OOB;
      const unsigned ob = okb ? (unsigned)(((long)c * p.T + ta + 1) * NBIN + k) * 8u : OOB;
      const F2 va = __builtin_bit_cast(F2, __builtin_amdgcn_raw_buffer_load_b64(rph, (int)oa, 0, 0));
      const F2 vb = __builtin_bit_cast(F2, __builtin_amdgcn_raw_buffer_load_b64(rph, (int)ob, 0, 0));
      pa[PMODE == 1 ? r : 0] = float2{va.x, va.y};
      pb[PMODE == 1 ? r : 0] = float2{vb.x, vb.y};
    }
  }
  fft_load_twiddles<NFFT>(tw, p.twiddles, tid, 512);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int k = (tid >> 4) + (512 / NF) * it, f = tid & (NF - 1);
    if (k < NBIN) {
      const int w = f >> 1, at = 2 * (w * BUF + k + w) + (f & 1);
      raw[at] = sm[it];
      if (PMODE == 3) raw[at + BUF] = sa[PMODE == 3 ? it : 0];       // BUF floats = half a buffer higher
      else if (STEMS) raw[at + BUF] = sm2[STEMS ? it : 0];
    }
  }
  __syncthreads();
  // spectra of this wave's two frames into registers (imaginary parts of DC / Nyquist dropped, as irfft does)
  float2 Sa[NR], Sb[NR];
  float2 Ua[STEMS ? NR : 1], Ub[STEMS ? NR : 1];            // STEMS: the second stem's (PMODE 3: its phasors until its magnitudes arrive)
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int k = lane + 64 * r;
    Sa[r] = Sb[r] = float2{0.f, 0.f};
    if (STEMS) Ua[STEMS ? r : 0] = Ub[STEMS ? r : 0] = float2{0.f, 0.f};
    if (k > NFFT / 2) continue;
    const float2 m = buf[k + wave];
    float2 qa = pa[PMODE == 1 ? r : 0], qb = pb[PMODE == 1 ? r : 0];
    if (PMODE == 3) {
      const float2 a = buf[k + wave + BUF / 2];
      // v_sin_f32 / v_cos_f32 (argument in revolutions; absolute error ~1e-6, the phasor multiplies a magnitude): the library
      // sincosf with its large-argument reduction was a third of this kernel's instructions
      const float ra = a.x * 0.15915494309189535f, rb = a.y * 0.15915494309189535f;
      qa = float2{__builtin_amdgcn_cosf(ra), __builtin_amdgcn_sinf(ra)};
      qb = float2{__builtin_amdgcn_cosf(rb), __builtin_amdgcn_sinf(rb)};
    }
    const bool edge = (k == 0 || k == NFFT / 2);
    Sa[r] = float2{m.x * qa.x, edge ? 0.f : m.x * qa.y};
    Sb[r] = float2{m.y * qb.x, edge ? 0.f : m.y * qb.y};
    if (STEMS && PMODE == 1) {
      const float2 m2 = buf[k + wave + BUF / 2];
      Ua[STEMS ? r : 0] = float2{m2.x * qa.x, edge ? 0.f : m2.x * qa.y};
      Ub[STEMS ? r : 0] = float2{m2.y * qb.x, edge ? 0.f : m2.y * qb.y};
    } else if (STEMS) {
      Ua[STEMS ? r : 0] = qa;
      Ub[STEMS ? r : 0] = qb;
    }
  }
  if constexpr (STEMS != 0 && PMODE == 3) {                 // the angles took the second plane: the second stem's magnitudes follow
    __syncthreads();                                        // every wave has read its staged values: other waves' threads refill its buffer
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int k = (tid >> 4) + (512 / NF) * it, f = tid & (NF - 1);
      if (k < NBIN) raw[2 * ((f >> 1) * BUF + k + (f >> 1)) + (f & 1)] = sm2[STEMS ? it : 0];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int k = lane + 64 * r;
      if (k > NFFT / 2) continue;
      const float2 m2 = buf[k + wave], qa = Ua[STEMS ? r : 0], qb = Ub[STEMS ? r : 0];
      const bool edge = (k == 0 || k == NFFT / 2);
      Ua[STEMS ? r : 0] = float2{m2.x * qa.x, edge ? 0.f : m2.x * qa.y};
      Ub[STEMS ? r : 0] = float2{m2.y * qb.x, edge ? 0.f : m2.y * qb.y};
    }
  }
  // conj(Z) with Z = Sa + i Sb (Hermitian-extended): the forward transform of conj(Z) is conj(ifft(Z)) = a - i b
  auto transform = [&](const auto& A, const auto& B) __attribute__((always_inline)) {
    fft_wave_sync();                                        // every lane has read its staged values before the buffer is refilled
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int k = lane + 64 * r;
      if (k > NFFT / 2) continue;
      buf[fft_pad(k)] = float2{A[r].x - B[r].y, -(A[r].y + B[r].x)};
      if (k > 0 && k < NFFT / 2) buf[fft_pad(NFFT - k)] = float2{A[r].x + B[r].y, -(B[r].x - A[r].y)};
    }
    fft_wave<NFFT>(buf, tw, lane);
  };
  transform(Sa, Sb);
  __syncthreads();
  // ---- output: sample rel = hop * (f - 1) + m of local frame f; at most frames f_hi (m < hop) and f_hi - 1 (m + hop < n_fft)
  float vmax = 0.f, vmax2 = 0.f;
  auto write_hops = [&](float* const yc, float& vmax) __attribute__((always_inline)) {
    // A thread keeps its position m inside the hop and walks the 15 hops: the two window values (and, away from the ends of
    // the signal, the envelope) are computed once per thread, and which frames exist is uniform across the block per hop.
    const long ilo = NFFT / 2 - (long)p.hop * t0, ihi = p.n_out + ilo;       // valid e: ilo <= e < ihi
    auto emit = [&](int m, int fh_lo, int fh_hi) __attribute__((always_inline)) {
      const bool two = m + p.hop < NFFT;                    // frame fh - 1 still covers this position
      const float w1 = hann_fast<NFFT>(m) * (1.0f / NFFT), w0 = two ? hann_fast<NFFT>(m + p.hop) * (1.0f / NFFT) : 0.f;
      const float e1 = w1 * w1 * (float)(NFFT * NFFT), e0 = w0 * w0 * (float)(NFFT * NFFT);
      const int a1 = fft_pad(m), a0 = fft_pad(two ? m + p.hop : 0);
#pragma unroll 4
      for (int fh = fh_lo; fh <= fh_hi; ++fh) {
        const int e = (fh - 1) * p.hop + m;
        if (e < ilo || e >= ihi) continue;
        const int th = t0 - 1 + fh;                         // global index of local frame fh; fh - 1 is th - 1
        const float2 z1 = fbuf[(fh >> 1) * BUF + a1], z0 = fbuf[((fh - 1) >> 1) * BUF + a0];
        const float s = ((fh & 1) ? -z1.y : z1.x) * w1 + ((fh & 1) ? z0.x : -z0.y) * w0;     // (frames outside [0, T) hold zeros)
        const float env = ((th >= 0 && th < p.T) ? e1 : 0.f) + ((th - 1 >= 0 && th - 1 < p.T) ? e0 : 0.f);
        const float v = env > 1.1754944e-38f ? s * __builtin_amdgcn_rcpf(env) : s;
        yc[e] = v;
        vmax = fmaxf(vmax, fabsf(v));
      }
    };
    // positions 0 .. 511: one per thread, all 15 hops.  The remaining hop - 512 positions (256 at hop 768) would leave half
    // the block idle for a second full pass: instead position 512 + j is shared by threads j and j + hop - 512 (if it exists),
    // which take the lower and the upper half of the hops
    if (tid < p.hop) emit(tid, 1, IGROUP);
    const int rest = p.hop - 512;
    if (rest > 0) {
      if (2 * rest <= 512) {
        if (tid < rest) emit(512 + tid, 1, (IGROUP + 1) / 2);
        else if (tid < 2 * rest) emit(512 + tid - rest, (IGROUP + 1) / 2 + 1, IGROUP);
      } else {
        for (int m = 512 + tid; m < p.hop; m += 512) emit(m, 1, IGROUP);
      }
    }
  };
  float* const yc0 = p.y + (long)c * p.n_out + ((long)p.hop * t0 - NFFT / 2);
  write_hops(yc0, vmax);
  if constexpr (STEMS != 0) {
    __syncthreads();                                        // every thread has read the first stem's frames before the buffers are refilled
    transform(Ua, Ub);
    __syncthreads();
    write_hops(yc0 + p.stem_stride, vmax2);
  }
  if (p.absmax_partial) {                                   // partial[c][group]: max |y| of this block (STEMS: [stem][c][group])
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64)); if (STEMS) vmax2 = fmaxf(vmax2, __shfl_xor(vmax2, o, 64)); }
    __syncthreads();
    if (lane == 0) { raw[wave] = vmax; if (STEMS) raw[NW + wave] = vmax2; }
    __syncthreads();
    if (tid <= STEMS) {
      float m = raw[NW * tid];
      for (int w = 1; w < NW; ++w) m = fmaxf(m, raw[NW * tid + w]);
      p.absmax_partial[(long)tid * gridDim.x + g] = m;
    }
  }
}

// General overlap-add for ANY 0 < hop <= n_fft (data.py:24-25 lets --hop_size override the config, and config.py:14-25 records
// runs at HOP_SIZE = 256: four frames per sample).  A block owns G hops = G * hop padded samples of one channel and walks the
// frames that touch them, floor((n_fft - 1) / hop) + G of them, in rounds of NF = 16 (two per wave, the same transform as above);
// after each round every thread adds the round's frames into ITS OWN positions of an LDS accumulator (windowed sample and
// squared window side by side: fixed frame order, no atomics), and after the last round divides and stores.  Slower than the
// two-frames-per-sample kernel (one block per CU, divisions per position and round); that one keeps hop >= n_fft / 2.
// NW waves per block (NF = 2 NW frames per round): 8, except N = 2048, where eight buffers and the twiddles fill 157,696 of the
// CU's 163,840 B and leave no room for the accumulator -- four waves (88,064 B) leave 75,776 B (istft_plan below).
// STEMS: both stems, as in istft_kernel -- one staging per round, the second stem's spectra wait in registers while the first
// stem's frames are transformed and accumulated, then take the same buffers.  The accumulator gains one float per position
// (sum of the second stem's windowed samples; the squared-window sum is shared): 12 B per position (istft_stems_plan).
template <int NFFT, int NW, int PMODE, int STEMS = 0>
__global__ __launch_bounds__(64 * NW) void istft_general_kernel(IstftArgs p, int ngroups, int G, int rounds) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NBIN = NFFT / 2 + 1, NR = NFFT / 128 + 1, NT = 64 * NW;
  constexpr int BUF = FftSize<NFFT>::BUF, TW = FftSize<NFFT>::TW, NF = 2 * NW;
  constexpr int NIT = (NBIN * NF + NT - 1) / NT;
  float2* const fbuf = (float2*)smem;                       // [NW][BUF]
  float2* const tw = fbuf + NW * BUF;
  float2* const acc = tw + TW;                              // [G * hop]: (sum of windowed samples, sum of squared windows)
  float* const raw = (float*)fbuf;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x, c = g / ngroups, t0 = (g - c * ngroups) * G;      // padded samples [hop * t0, hop * (t0 + G))
  const int seg_len = G * p.hop, halo = (NFFT - 1) / p.hop;
  float* const acc2 = (float*)(acc + seg_len);              // STEMS: [G * hop] sum of the second stem's windowed samples
  float2* const buf = fbuf + wave * BUF;
  constexpr unsigned OOB = 0x80000000u;
  const __amdgpu_buffer_rsrc_t rmag = __builtin_amdgcn_make_buffer_rsrc((void*)p.mag, 0, OOB, 0x00020000);
  const __amdgpu_buffer_rsrc_t rmask = __builtin_amdgcn_make_buffer_rsrc((void*)(p.mask ? p.mask : p.mag), 0, OOB, 0x00020000);
  const __amdgpu_buffer_rsrc_t rph = __builtin_amdgcn_make_buffer_rsrc((void*)p.phase, 0, OOB, 0x00020000);
  const bool has_mask = p.mask != nullptr;
  fft_load_twiddles<NFFT>(tw, p.twiddles, tid, NT);
  for (int i = tid; i < seg_len; i += NT) { acc[i] = float2{0.f, 0.f}; if (STEMS) acc2[i] = 0.f; }
  for (int r = 0; r < rounds; ++r) {
    const int tb = t0 - halo + NF * r;                      // first frame of this round
    __syncthreads();                                        // the previous round's buffers have been consumed (and, r = 0: twiddles)
    // ---- stage: this thread's frame column (NF frames x NBIN bins through the waves' buffers, as in istft_kernel)
    {
      const int tf = tb + (tid & (NF - 1));
      const bool tok = tf >= 0 && tf < p.T;
      const unsigned cbase = tok ? (unsigned)p.lay.col(c, tf) : 0u;
      for (int it = 0; it < NIT; ++it) {
        const int k = tid / NF + (NT / NF) * it;
        if (k >= NBIN) continue;
        const bool ok = tok && k >= p.lay.first_bin;
        const unsigned off = ok ? (cbase + (unsigned)(k * p.lay.seg)) * 4u : OOB;
        float m = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmag, (int)off, 0, 0));
        const int f = tid & (NF - 1), w = f >> 1, at = 2 * (w * BUF + k + w) + (f & 1);
        if (STEMS) {
          const float mk = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmask, (int)off, 0, 0));
          if (PMODE == 1) raw[at + BUF] = m * (1.f - mk);
          m *= mk;
        } else if (has_mask) {
          const float mk = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmask, (int)off, 0, 0));
          m *= p.invert ? 1.f - mk : mk;
        }
        raw[at] = m;
        if (PMODE == 3) raw[at + BUF] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rph, (int)off, 0, 0));
      }
    }
    __syncthreads();
    // ---- spectra of this wave's two frames, Hermitian-extended conj(Sa + i Sb), one transform
    const int ta = tb + 2 * wave;
    float2 Sa[NR], Sb[NR];
    float2 Ua[STEMS ? NR : 1], Ub[STEMS ? NR : 1];          // STEMS: the second stem's (PMODE 3: its phasors until its magnitudes arrive)
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      const int k = lane + 64 * q;
      Sa[q] = Sb[q] = float2{0.f, 0.f};
      if (STEMS) Ua[STEMS ? q : 0] = Ub[STEMS ? q : 0] = float2{0.f, 0.f};
      if (k > NFFT / 2) continue;
      const float2 m = buf[k + wave];
      float2 qa, qb;
      if (PMODE == 3) {
        const float2 a = buf[k + wave + BUF / 2];
        const float ra = a.x * 0.15915494309189535f, rb = a.y * 0.15915494309189535f;
        qa = float2{__builtin_amdgcn_cosf(ra), __builtin_amdgcn_sinf(ra)};
        qb = float2{__builtin_amdgcn_cosf(rb), __builtin_amdgcn_sinf(rb)};
      } else {
        struct F2 { float x, y; };
        const bool oka = ta >= 0 && ta < p.T, okb = ta + 1 >= 0 && ta + 1 < p.T;
        const unsigned oa = oka ? (unsigned)(((long)c * p.T + ta) * NBIN + k) * 8u : OOB;
        const unsigned ob = okb ? (unsigned)(((long)c * p.T + ta + 1) * NBIN + k) * 8u : OOB;
        const F2 va = __builtin_bit_cast(F2, __builtin_amdgcn_raw_buffer_load_b64(rph, (int)oa, 0, 0));
        const F2 vb = __builtin_bit_cast(F2, __builtin_amdgcn_raw_buffer_load_b64(rph, (int)ob, 0, 0));
        qa = float2{va.x, va.y};
        qb = float2{vb.x, vb.y};
      }
      const bool edge = (k == 0 || k == NFFT / 2);
      Sa[q] = float2{m.x * qa.x, edge ? 0.f : m.x * qa.y};
      Sb[q] = float2{m.y * qb.x, edge ? 0.f : m.y * qb.y};
      if (STEMS && PMODE == 1) {
        const float2 m2 = buf[k + wave + BUF / 2];
        Ua[STEMS ? q : 0] = float2{m2.x * qa.x, edge ? 0.f : m2.x * qa.y};
        Ub[STEMS ? q : 0] = float2{m2.y * qb.x, edge ? 0.f : m2.y * qb.y};
      } else if (STEMS) {
        Ua[STEMS ? q : 0] = qa;
        Ub[STEMS ? q : 0] = qb;
      }
    }
    if constexpr (STEMS != 0 && PMODE == 3) {
      // the angles took the second plane: the second stem's magnitudes follow through the first (loaded again: this kernel keeps
      // no staged value in registers, and the lines are in L2 from a moment ago)
      __syncthreads();                                      // every wave has read its staged values: other waves' threads refill its buffer
      const int tf = tb + (tid & (NF - 1));
      const bool tok = tf >= 0 && tf < p.T;
      const unsigned cbase = tok ? (unsigned)p.lay.col(c, tf) : 0u;
      for (int it = 0; it < NIT; ++it) {
        const int k = tid / NF + (NT / NF) * it;
        if (k >= NBIN) continue;
        const bool ok = tok && k >= p.lay.first_bin;
        const unsigned off = ok ? (cbase + (unsigned)(k * p.lay.seg)) * 4u : OOB;
        const float m = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmag, (int)off, 0, 0));
        const float mk = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmask, (int)off, 0, 0));
        const int f = tid & (NF - 1), w = f >> 1;
        raw[2 * (w * BUF + k + w) + (f & 1)] = m * (1.f - mk);
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        const int k = lane + 64 * q;
        if (k > NFFT / 2) continue;
        const float2 m2 = buf[k + wave], qa = Ua[STEMS ? q : 0], qb = Ub[STEMS ? q : 0];
        const bool edge = (k == 0 || k == NFFT / 2);
        Ua[STEMS ? q : 0] = float2{m2.x * qa.x, edge ? 0.f : m2.x * qa.y};
        Ub[STEMS ? q : 0] = float2{m2.y * qb.x, edge ? 0.f : m2.y * qb.y};
      }
    }
    auto transform = [&](const auto& A, const auto& B) __attribute__((always_inline)) {
      fft_wave_sync();                                      // every lane has read its staged values before the buffer is refilled
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        const int k = lane + 64 * q;
        if (k > NFFT / 2) continue;
        buf[fft_pad(k)] = float2{A[q].x - B[q].y, -(A[q].y + B[q].x)};
        if (k > 0 && k < NFFT / 2) buf[fft_pad(NFFT - k)] = float2{A[q].x + B[q].y, -(B[q].x - A[q].y)};
      }
      fft_wave<NFFT>(buf, tw, lane);
    };
    // ---- accumulate: position i (padded sample hop * t0 + i) takes every frame of this round that covers it, ascending
    auto accumulate = [&](const bool second) __attribute__((always_inline)) {
      for (int i = tid; i < seg_len; i += NT) {
        const int q = p.hop * t0 + i;
        int lo = q - (NFFT - 1);
        lo = lo <= 0 ? 0 : (int)((unsigned)(lo + p.hop - 1) / (unsigned)p.hop);
        int hi = (int)((unsigned)q / (unsigned)p.hop);
        if (hi > p.T - 1) hi = p.T - 1;
        if (lo < tb) lo = tb;
        if (hi > tb + NF - 1) hi = tb + NF - 1;
        float2 a = second ? float2{acc2[i], 0.f} : acc[i];
        for (int t = lo; t <= hi; ++t) {
          const int f = t - tb, m = q - t * p.hop;
          const float2 z = fbuf[(f >> 1) * BUF + fft_pad(m)];
          const float w = hann_fast<NFFT>(m);
          a.x += ((f & 1) ? -z.y : z.x) * (w * (1.0f / NFFT));
          if (!second) a.y += w * w;
        }
        if (second) acc2[i] = a.x; else acc[i] = a;
      }
    };
    transform(Sa, Sb);
    __syncthreads();
    accumulate(false);
    if constexpr (STEMS != 0) {
      __syncthreads();                                      // every thread has read the first stem's frames before the buffers are refilled
      transform(Ua, Ub);
      __syncthreads();
      accumulate(true);
    }
  }
  // ---- divide by the window envelope, store, |.|max
  float vmax = 0.f, vmax2 = 0.f;
  for (int i = tid; i < seg_len; i += NT) {
    const long e = (long)p.hop * t0 + i - NFFT / 2;
    if (e < 0 || e >= p.n_out) continue;
    const float2 a = acc[i];
    const bool div = a.y > 1.1754944e-38f;
    const float v = div ? a.x * __builtin_amdgcn_rcpf(a.y) : a.x;
    p.y[(long)c * p.n_out + e] = v;
    vmax = fmaxf(vmax, fabsf(v));
    if (STEMS) {
      const float b = acc2[i], v2 = div ? b * __builtin_amdgcn_rcpf(a.y) : b;
      p.y[p.stem_stride + (long)c * p.n_out + e] = v2;
      vmax2 = fmaxf(vmax2, fabsf(v2));
    }
  }
  if (p.absmax_partial) {                                   // (STEMS: [stem][c][group])
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64)); if (STEMS) vmax2 = fmaxf(vmax2, __shfl_xor(vmax2, o, 64)); }
    __syncthreads();
    if (lane == 0) { raw[wave] = vmax; if (STEMS) raw[NW + wave] = vmax2; }
    __syncthreads();
    if (tid <= STEMS) {
      float m = raw[NW * tid];
      for (int w = 1; w < NW; ++w) m = fmaxf(m, raw[NW * tid + w]);
      p.absmax_partial[(long)tid * gridDim.x + g] = m;
    }
  }
}

// (R, C) float2 matrix -> (C, R): f-major phasors of a .npy file <-> the frame-major form the kernels stream
__global__ __launch_bounds__(256) void transpose_c64_kernel(const float2* __restrict__ in, float2* __restrict__ out, int R, int C) {
  __shared__ float2 tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int i = threadIdx.x; i < 1024; i += 256) {
    const int r = r0 + (i >> 5), cc = c0 + (i & 31);
    if (r < R && cc < C) tile[i >> 5][i & 31] = in[(long)r * C + cc];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 1024; i += 256) {
    const int cc = c0 + (i >> 5), r = r0 + (i & 31);
    if (r < R && cc < C) out[(long)cc * R + r] = tile[i & 31][i >> 5];
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static bool nfft_built(int n) { return n == 512 || n == 1024 || n == 2048; }
#define SVS_REQUIRE_NFFT(who, n) SVS_REQUIRE(nfft_built(n), who ": n_fft must be 512, 1024 or 2048 (the sizes that are built), got %d", n)
static size_t fft_lds_bytes(int n_fft, int waves) {       // the waves' buffers and the twiddle table
  const size_t buf = n_fft == 512 ? FftSize<512>::BUF : n_fft == 1024 ? FftSize<1024>::BUF : FftSize<2048>::BUF;
  const size_t tw = n_fft == 512 ? FftSize<512>::TW : n_fft == 1024 ? FftSize<1024>::TW : FftSize<2048>::TW;
  return (size_t)waves * buf * 8 + tw * 8;
}
// forward and two-frames-per-sample inverse, eight waves: 39,424 B (512), 79,872 B (1024: two blocks per CU), 157,696 B (2048)
// the transposed operator adds its staged-angle plane: 56,900 B (512) and 114,756 B (1024); at 2048 the angles go through the
// buffers themselves (dmag_late_angles) and the block stays at 157,696 B
static size_t fwd_lds_bytes(int n_fft, bool dmag) {
  return fft_lds_bytes(n_fft, 8) + (dmag && !dmag_late_angles(n_fft) ? (size_t)(n_fft / 2 + 1) * SROW * 4 : 0);
}
template <class K>
static int allow_lds(K kernel, size_t bytes) {
  SVS_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return SVS_OK;
}
static int check_layout(const char* who, int n_fft, int seg, int rows, int first_bin, int frames_alloc, int T) {
  SVS_REQUIRE(seg > 0 && (first_bin == 0 || first_bin == 1) && rows == n_fft / 2 + 1 - first_bin && frames_alloc >= T,
              "%s: bad spectrogram layout (seg=%d rows=%d first_bin=%d frames_alloc=%d T=%d)", who, seg, rows, first_bin, frames_alloc, T);
  return SVS_OK;
}

extern "C" int svs_stft_frames(int64_t n_samples, int hop) { return hop > 0 && n_samples >= 0 ? (int)(1 + n_samples / hop) : -1; }

template <int N>
static int launch_stft_fwd(StftArgs& a, int frames_alloc, hipStream_t stream) {
  int rc = svs_fft_twiddles(N, stream, &a.twiddles);
  if (rc) return rc;
  if (N != 1024 && (rc = svs_fft_hann(N, stream, &a.hann))) return rc;
  const size_t lds = fwd_lds_bytes(N, false);
  if ((rc = allow_lds(stft_fwd_kernel<N, SRC_SIGNAL, SINK_MAGPHASE>, lds))) return rc;
  dim3 grid((unsigned)((frames_alloc + GROUP - 1) / GROUP), (unsigned)a.channels);
  hipLaunchKernelGGL((stft_fwd_kernel<N, SRC_SIGNAL, SINK_MAGPHASE>), grid, dim3(512), lds, stream, a);
  SVS_CHECK_LAUNCH("stft_fwd");
  return SVS_OK;
}

extern "C" int svs_stft_tiles_n(const float* y, int64_t n_samples, int channels, int n_fft, int hop, float* mag, int64_t chan_stride,
                                int seg, int rows, int first_bin, int frames_alloc, float* phase, int phase_mode,
                                float* absmax_partial, hipStream_t stream) {
  SVS_REQUIRE(y && mag && n_samples > 0 && channels > 0 && hop > 0, "svs_stft_tiles: bad arguments");
  SVS_REQUIRE_NFFT("svs_stft_tiles_n", n_fft);
  SVS_REQUIRE(phase_mode >= 0 && phase_mode <= 2 && (phase_mode == 0 || (phase && (((uintptr_t)phase) & 7u) == 0)), "svs_stft_tiles: bad phase arguments");
  const int T = (int)(1 + n_samples / hop);
  int rc = check_layout("svs_stft_tiles", n_fft, seg, rows, first_bin, frames_alloc, T);
  if (rc) return rc;
  StftArgs a{};
  a.y = y; a.n_samples = n_samples; a.channels = channels; a.hop = hop; a.T = T;
  a.mag = mag; a.lay = SpecLayout{chan_stride, seg, rows, first_bin, frames_alloc};
  a.phase = phase; a.phase_mode = phase_mode; a.absmax_partial = absmax_partial;
  return n_fft == 512 ? launch_stft_fwd<512>(a, frames_alloc, stream)
       : n_fft == 1024 ? launch_stft_fwd<1024>(a, frames_alloc, stream) : launch_stft_fwd<2048>(a, frames_alloc, stream);
}
extern "C" int svs_stft_tiles(const float* y, int64_t n_samples, int channels, int n_fft, int hop, float* mag, int64_t chan_stride,
                              int seg, int rows, int first_bin, int frames_alloc, float* phase, int phase_mode,
                              float* absmax_partial, hipStream_t stream) {
  SVS_REQUIRE(y && mag && n_samples > 0 && channels > 0 && hop > 0, "svs_stft_tiles: bad arguments");
  SVS_REQUIRE(n_fft == 1024, "svs_stft_tiles: only n_fft=1024 (reference config.py:47) is built, got %d", n_fft);
  return svs_stft_tiles_n(y, n_samples, channels, n_fft, hop, mag, chan_stride, seg, rows, first_bin, frames_alloc, phase, phase_mode,
                          absmax_partial, stream);
}
// blocks per channel of the forward = absmax partials per channel: 16 frames per block at every n_fft
extern "C" int svs_stft_groups(int frames_alloc) { return (frames_alloc + GROUP - 1) / GROUP; }
extern "C" int svs_stft_groups_n(int n_fft, int frames_alloc) {
  SVS_REQUIRE_NFFT("svs_stft_groups_n", n_fft);
  return svs_stft_groups(frames_alloc);
}

// ---- re-phasing forward transform: the analysis half of a Griffin-Lim (SRC_SIGNAL) / MISI (SRC_MISI) iteration, SINK_PHASOR
template <int N>
static int launch_stft_rephase(StftArgs& a, int stems, hipStream_t stream) {
  int rc = svs_fft_twiddles(N, stream, &a.twiddles);
  if (rc) return rc;
  if (N != 1024 && (rc = svs_fft_hann(N, stream, &a.hann))) return rc;
  const size_t lds = fft_lds_bytes(N, 8);                 // the eight wave buffers and the twiddle table: the forward kernel's own
  if ((rc = a.msig ? allow_lds(stft_fwd_kernel<N, SRC_MISI, SINK_PHASOR>, lds) : allow_lds(stft_fwd_kernel<N, SRC_SIGNAL, SINK_PHASOR>, lds))) return rc;
  dim3 grid((unsigned)((a.T + GROUP - 1) / GROUP), (unsigned)(a.channels * stems));
  if (a.msig) hipLaunchKernelGGL((stft_fwd_kernel<N, SRC_MISI, SINK_PHASOR>), grid, dim3(512), lds, stream, a);
  else hipLaunchKernelGGL((stft_fwd_kernel<N, SRC_SIGNAL, SINK_PHASOR>), grid, dim3(512), lds, stream, a);
  SVS_CHECK_LAUNCH("stft_rephase");
  return SVS_OK;
}

extern "C" int svs_stft_rephase_n(const float* x, int64_t stem_stride, int stems, const float* mix, int64_t n_samples, int channels,
                                  int n_fft, int hop, float* phase, int64_t phase_stem_stride, hipStream_t stream) {
  SVS_REQUIRE(n_samples > 0 && channels > 0, "svs_stft_rephase_n: n_samples and channels must be positive (n_samples=%lld channels=%d)",
              (long long)n_samples, channels);
  SVS_REQUIRE(stems == 1 || stems == 2, "svs_stft_rephase_n: stems must be 1 or 2, got %d", stems);
  SVS_REQUIRE(!mix || stems == 2, "svs_stft_rephase_n: a mixture needs stems == 2 (x_s + (mix - x_0 - x_1) / 2), got stems = %d", stems);
  SVS_REQUIRE_NFFT("svs_stft_rephase_n", n_fft);
  SVS_REQUIRE(hop > 0 && hop <= n_fft, "svs_stft_rephase_n: hop %d is not in 1..n_fft (a larger hop leaves samples that no frame covers)", hop);
  SVS_REQUIRE((long)channels * stems <= 65535, "svs_stft_rephase_n: channels * stems = %ld exceeds the grid's 65535", (long)channels * stems);
  const long T = 1 + n_samples / hop, nbin = n_fft / 2 + 1;
  const long x_one = (long)channels * n_samples, ph_one = (long)channels * T * nbin * 2;        // floats of one stem
  SVS_REQUIRE(stems == 1 || (stem_stride >= x_one && phase_stem_stride >= ph_one),
              "svs_stft_rephase_n: stem_stride %lld / phase_stem_stride %lld are below one stem's %lld samples / %lld phase floats",
              (long long)stem_stride, (long long)phase_stem_stride, (long long)x_one, (long long)ph_one);
  SVS_REQUIRE(stems == 1 || (phase_stem_stride & 1) == 0, "svs_stft_rephase_n: phase_stem_stride %lld must be even (whole (re, im) pairs)",
              (long long)phase_stem_stride);
  const long x_view = (stems - 1) * (long)stem_stride + x_one, ph_view = (stems - 1) * (long)phase_stem_stride + ph_one;
  SVS_REQUIRE(x_view * 4 < (1L << 31) && ph_view * 4 < (1L << 31),
              "svs_stft_rephase_n: a view of 2 GiB or more (signals %lld B, phasors %lld B); split the channels",
              (long long)(x_view * 4), (long long)(ph_view * 4));
  SVS_REQUIRE(x && phase, "svs_stft_rephase_n: null pointer (x or phase)");
  SVS_REQUIRE((((uintptr_t)phase) & 7u) == 0 && (((uintptr_t)x | (uintptr_t)mix) & 3u) == 0,
              "svs_stft_rephase_n: phase must be 8-byte aligned, x and mix 4-byte aligned");
  StftArgs a{};
  a.y = x; a.n_samples = n_samples; a.channels = channels; a.hop = hop; a.T = (int)T;
  a.msig = mix; a.stem_stride = stems == 2 ? (long)stem_stride : 0; a.phase = phase; a.phase_mode = 1;
  a.phase_stem_stride = stems == 2 ? (long)phase_stem_stride : 0;
  return n_fft == 512 ? launch_stft_rephase<512>(a, stems, stream)
       : n_fft == 1024 ? launch_stft_rephase<1024>(a, stems, stream) : launch_stft_rephase<2048>(a, stems, stream);
}

extern "C" int svs_stft_fwd(const float* y, int64_t n_samples, int n_fft, int hop, float* mag, float* phase, hipStream_t stream) {
  SVS_REQUIRE(y && mag && n_samples > 0 && hop > 0, "svs_stft_fwd: bad arguments");
  const int T = (int)(1 + n_samples / hop);
  return svs_stft_tiles(y, n_samples, 1, n_fft, hop, mag, (int64_t)513 * T, T, 513, 0, T, phase, phase ? 2 : 0, nullptr, stream);
}

// The inverse's launch plan: the one value that the launch, svs_istft_groups_n and svs_istft_plan_n read.
//   hop >= n_fft / 2: istft_kernel, eight waves, 15 hops per block (they touch 16 frames), one round.
//   hop <  n_fft / 2: istft_general_kernel.  G + halo frames touch G hops, halo = floor((n_fft - 1) / hop); they are walked in
//     rounds of NF = 2 * waves frames: one round while the halo leaves at least 4 hops of it (n_fft 1024: hop >= 86), else enough
//     rounds that at least half of every round is new hops.  waves = 8, except n_fft = 2048, where eight buffers leave 6 KB of the
//     CU's 160 KiB and the accumulator (G * hop * 8 B, up to 6 * 1023 * 8) needs 49 KB: four waves, eight frames per round.
struct IstftPlan { bool general; int waves, G, rounds; size_t lds; };
static IstftPlan istft_plan(int n_fft, int hop) {
  IstftPlan pl{};
  pl.general = hop < n_fft / 2;
  if (!pl.general) { pl.waves = 8; pl.G = IGROUP; pl.rounds = 1; pl.lds = fft_lds_bytes(n_fft, 8); return pl; }
  pl.waves = n_fft == 2048 ? 4 : 8;
  const int nf = 2 * pl.waves, halo = (n_fft - 1) / hop;
  pl.rounds = halo <= nf - 4 ? 1 : (halo + nf / 2 - 1) / (nf / 2);
  pl.G = nf * pl.rounds - halo;
  pl.lds = fft_lds_bytes(n_fft, pl.waves) + (size_t)pl.G * hop * 8;
  return pl;
}
// padded length n_fft + hop * (T - 1): the last samples belong to group floor((padded - 1) / (G hop))
static int svs_istft_groups_per_channel(int n_fft, int hop, int frames) {
  const long span = (long)istft_plan(n_fft, hop).G * hop;
  return (int)((n_fft + (long)hop * (frames - 1) + span - 1) / span);
}
// blocks per channel of svs_istft_tiles = absmax partials per channel (layout [channel][group])
extern "C" int svs_istft_groups(int hop, int frames, int channels) { (void)channels; return svs_istft_groups_per_channel(1024, hop, frames); }
extern "C" int svs_istft_groups_n(int n_fft, int hop, int frames, int channels) {
  (void)channels;
  SVS_REQUIRE_NFFT("svs_istft_groups_n", n_fft);
  SVS_REQUIRE(hop > 0 && hop <= n_fft && frames > 0, "svs_istft_groups_n: need 0 < hop <= n_fft and frames > 0 (hop=%d frames=%d)", hop, frames);
  return svs_istft_groups_per_channel(n_fft, hop, frames);
}
extern "C" int svs_istft_plan_n(int n_fft, int hop, int* hops_per_block, int* rounds, size_t* lds_bytes) {
  SVS_REQUIRE_NFFT("svs_istft_plan_n", n_fft);
  SVS_REQUIRE(hop > 0 && hop <= n_fft, "svs_istft_plan_n: hop %d is not in 1..n_fft (a larger hop leaves samples that no frame covers)", hop);
  const IstftPlan pl = istft_plan(n_fft, hop);
  if (hops_per_block) *hops_per_block = pl.G;
  if (rounds) *rounds = pl.rounds;
  if (lds_bytes) *lds_bytes = pl.lds;
  return SVS_OK;
}

template <int N, int NW>
static int launch_istft(IstftArgs& a, const IstftPlan& pl, int ngroups, hipStream_t stream) {
  int rc = svs_fft_twiddles(N, stream, &a.twiddles);
  if (rc) return rc;
  const dim3 grid((unsigned)((long)ngroups * a.channels));
  if (pl.general) {                               // more than two frames per sample: the general overlap-add
    if ((rc = a.phase_mode == 1 ? allow_lds(istft_general_kernel<N, NW, 1>, pl.lds) : allow_lds(istft_general_kernel<N, NW, 3>, pl.lds))) return rc;
    if (a.phase_mode == 1) hipLaunchKernelGGL((istft_general_kernel<N, NW, 1>), grid, dim3(64 * NW), pl.lds, stream, a, ngroups, pl.G, pl.rounds);
    else hipLaunchKernelGGL((istft_general_kernel<N, NW, 3>), grid, dim3(64 * NW), pl.lds, stream, a, ngroups, pl.G, pl.rounds);
    SVS_CHECK_LAUNCH("istft_general");
    return SVS_OK;
  }
  if ((rc = a.phase_mode == 1 ? allow_lds(istft_kernel<N, 1>, pl.lds) : allow_lds(istft_kernel<N, 3>, pl.lds))) return rc;
  if (a.phase_mode == 1) hipLaunchKernelGGL((istft_kernel<N, 1>), grid, dim3(512), pl.lds, stream, a, ngroups);
  else hipLaunchKernelGGL((istft_kernel<N, 3>), grid, dim3(512), pl.lds, stream, a, ngroups);
  SVS_CHECK_LAUNCH("istft");
  return SVS_OK;
}

extern "C" int svs_istft_tiles_n(const float* mag, int64_t chan_stride, int seg, int rows, int first_bin, const float* mask, int invert,
                                 const float* phase, int phase_mode, int channels, int n_fft, int hop, int frames, float* y,
                                 float* absmax_partial, hipStream_t stream) {
  SVS_REQUIRE(mag && phase && y && hop > 0 && frames > 1 && channels > 0, "svs_istft_tiles: bad arguments (need >= 2 frames)");
  SVS_REQUIRE_NFFT("svs_istft_tiles_n", n_fft);
  SVS_REQUIRE(hop <= n_fft, "svs_istft_tiles: hop %d > n_fft leaves samples that no frame covers", hop);
  SVS_REQUIRE(phase_mode == 1 || phase_mode == 3, "svs_istft_tiles: phase_mode must be 1 (frame-major phasors) or 3 (angles)");
  const long nbin = n_fft / 2 + 1;
  SVS_REQUIRE((long)channels * (chan_stride > (long)frames * nbin ? chan_stride : (long)frames * nbin) * 8 < (1L << 31),
              "svs_istft_tiles: a spectrogram view of more than 2 GiB needs 64-bit offsets; split the channels");
  int rc = check_layout("svs_istft_tiles", n_fft, seg, rows, first_bin, frames, frames);
  if (rc) return rc;
  IstftArgs a{};
  a.mag = mag; a.lay = SpecLayout{chan_stride, seg, rows, first_bin, frames};
  a.mask = mask; a.invert = invert; a.phase = phase; a.phase_mode = phase_mode;
  a.channels = channels; a.T = frames; a.hop = hop; a.y = y; a.n_out = (long)hop * (frames - 1);
  a.absmax_partial = absmax_partial;
  const IstftPlan pl = istft_plan(n_fft, hop);
  const int ngroups = svs_istft_groups_per_channel(n_fft, hop, frames);
  return n_fft == 512 ? launch_istft<512, 8>(a, pl, ngroups, stream)
       : n_fft == 1024 ? launch_istft<1024, 8>(a, pl, ngroups, stream) : launch_istft<2048, 4>(a, pl, ngroups, stream);
}
extern "C" int svs_istft_tiles(const float* mag, int64_t chan_stride, int seg, int rows, int first_bin, const float* mask, int invert,
                               const float* phase, int phase_mode, int channels, int n_fft, int hop, int frames, float* y,
                               float* absmax_partial, hipStream_t stream) {
  SVS_REQUIRE(mag && phase && y && hop > 0 && frames > 1 && channels > 0, "svs_istft_tiles: bad arguments (need >= 2 frames)");
  SVS_REQUIRE(n_fft == 1024, "svs_istft_tiles: only n_fft=1024 (reference config.py:47) is built, got %d", n_fft);
  return svs_istft_tiles_n(mag, chan_stride, seg, rows, first_bin, mask, invert, phase, phase_mode, channels, n_fft, hop, frames, y,
                           absmax_partial, stream);
}

// ---- both stems of a mask from one launch (STEMS kernels)
// The two-frames-per-sample kernel keeps its plan (the second stem goes through the same buffers).  The general kernel's
// accumulator is 12 B per position instead of 8: where G hops of it no longer fit beside the buffers (n_fft 1024, hop 500 .. 511:
// 14 hops x 12 B x hop > 83,968 B) the block owns as many hops as fit; the rounds still cover G + halo frames.
static constexpr size_t LDS_PER_CU = 163840;
static IstftPlan istft_stems_plan(int n_fft, int hop) {
  IstftPlan pl = istft_plan(n_fft, hop);
  if (!pl.general) return pl;
  const size_t fft = fft_lds_bytes(n_fft, pl.waves);
  const int nf = 2 * pl.waves, halo = (n_fft - 1) / hop, fit = (int)((LDS_PER_CU - fft) / ((size_t)hop * 12));
  if (pl.G > fit) { pl.G = fit; pl.rounds = (pl.G + halo + nf - 1) / nf; }
  pl.lds = fft + (size_t)pl.G * hop * 12;
  return pl;
}
static int istft_stems_groups_per_channel(int n_fft, int hop, int frames) {
  const long span = (long)istft_stems_plan(n_fft, hop).G * hop;
  return (int)((n_fft + (long)hop * (frames - 1) + span - 1) / span);
}
// blocks per channel of svs_istft_stems_n = absmax partials per channel and stem (layout [stem][channel][group])
extern "C" int svs_istft_stems_groups_n(int n_fft, int hop, int frames, int channels) {
  (void)channels;
  SVS_REQUIRE_NFFT("svs_istft_stems_groups_n", n_fft);
  SVS_REQUIRE(hop > 0 && hop <= n_fft && frames > 0, "svs_istft_stems_groups_n: need 0 < hop <= n_fft and frames > 0 (hop=%d frames=%d)", hop, frames);
  return istft_stems_groups_per_channel(n_fft, hop, frames);
}
extern "C" int svs_istft_stems_plan_n(int n_fft, int hop, int* hops_per_block, int* rounds, size_t* lds_bytes) {
  SVS_REQUIRE_NFFT("svs_istft_stems_plan_n", n_fft);
  SVS_REQUIRE(hop > 0 && hop <= n_fft, "svs_istft_stems_plan_n: hop %d is not in 1..n_fft (a larger hop leaves samples that no frame covers)", hop);
  const IstftPlan pl = istft_stems_plan(n_fft, hop);
  if (hops_per_block) *hops_per_block = pl.G;
  if (rounds) *rounds = pl.rounds;
  if (lds_bytes) *lds_bytes = pl.lds;
  return SVS_OK;
}

template <int N, int NW>
static int launch_istft_stems(IstftArgs& a, const IstftPlan& pl, int ngroups, hipStream_t stream) {
  int rc = svs_fft_twiddles(N, stream, &a.twiddles);
  if (rc) return rc;
  const dim3 grid((unsigned)((long)ngroups * a.channels));
  if (pl.general) {
    if ((rc = a.phase_mode == 1 ? allow_lds(istft_general_kernel<N, NW, 1, 1>, pl.lds) : allow_lds(istft_general_kernel<N, NW, 3, 1>, pl.lds))) return rc;
    if (a.phase_mode == 1) hipLaunchKernelGGL((istft_general_kernel<N, NW, 1, 1>), grid, dim3(64 * NW), pl.lds, stream, a, ngroups, pl.G, pl.rounds);
    else hipLaunchKernelGGL((istft_general_kernel<N, NW, 3, 1>), grid, dim3(64 * NW), pl.lds, stream, a, ngroups, pl.G, pl.rounds);
    SVS_CHECK_LAUNCH("istft_general (stems)");
    return SVS_OK;
  }
  if ((rc = a.phase_mode == 1 ? allow_lds(istft_kernel<N, 1, 1>, pl.lds) : allow_lds(istft_kernel<N, 3, 1>, pl.lds))) return rc;
  if (a.phase_mode == 1) hipLaunchKernelGGL((istft_kernel<N, 1, 1>), grid, dim3(512), pl.lds, stream, a, ngroups);
  else hipLaunchKernelGGL((istft_kernel<N, 3, 1>), grid, dim3(512), pl.lds, stream, a, ngroups);
  SVS_CHECK_LAUNCH("istft (stems)");
  return SVS_OK;
}

extern "C" int svs_istft_stems_n(const float* mag, int64_t chan_stride, int seg, int rows, int first_bin, const float* mask,
                                 const float* phase, int phase_mode, int channels, int n_fft, int hop, int frames, float* y,
                                 int64_t stem_stride, float* absmax_partial, hipStream_t stream) {
  SVS_REQUIRE(mask, "svs_istft_stems: the mask is required (stem 0 is mag * mask, stem 1 mag * (1 - mask))");
  SVS_REQUIRE(mag && phase && y && channels > 0, "svs_istft_stems: bad arguments (null pointer or channels < 1)");
  SVS_REQUIRE_NFFT("svs_istft_stems_n", n_fft);
  SVS_REQUIRE(hop > 0 && hop <= n_fft, "svs_istft_stems: hop %d is not in 1..n_fft (a larger hop leaves samples that no frame covers)", hop);
  SVS_REQUIRE(frames > 1, "svs_istft_stems: need >= 2 frames, got %d", frames);
  SVS_REQUIRE(phase_mode == 1 || phase_mode == 3, "svs_istft_stems: phase_mode must be 1 (frame-major phasors) or 3 (angles)");
  const long nbin = n_fft / 2 + 1;
  SVS_REQUIRE((long)channels * (chan_stride > (long)frames * nbin ? chan_stride : (long)frames * nbin) * 8 < (1L << 31),
              "svs_istft_stems: a spectrogram view of more than 2 GiB needs 64-bit offsets; split the channels");
  const long n_out = (long)hop * (frames - 1);
  SVS_REQUIRE(stem_stride >= n_out * channels, "svs_istft_stems: stem_stride %lld is below the %lld samples of one stem (hop * (frames - 1) * channels)",
              (long long)stem_stride, (long long)(n_out * channels));
  int rc = check_layout("svs_istft_stems", n_fft, seg, rows, first_bin, frames, frames);
  if (rc) return rc;
  IstftArgs a{};
  a.mag = mag; a.lay = SpecLayout{chan_stride, seg, rows, first_bin, frames};
  a.mask = mask; a.phase = phase; a.phase_mode = phase_mode;
  a.channels = channels; a.T = frames; a.hop = hop; a.y = y; a.n_out = n_out; a.stem_stride = stem_stride;
  a.absmax_partial = absmax_partial;
  const IstftPlan pl = istft_stems_plan(n_fft, hop);
  const int ngroups = istft_stems_groups_per_channel(n_fft, hop, frames);
  return n_fft == 512 ? launch_istft_stems<512, 8>(a, pl, ngroups, stream)
       : n_fft == 1024 ? launch_istft_stems<1024, 8>(a, pl, ngroups, stream) : launch_istft_stems<2048, 4>(a, pl, ngroups, stream);
}

extern "C" size_t svs_istft_workspace_bytes(int n_fft, int hop, int frames) {
  (void)hop;
  return (size_t)frames * (n_fft / 2 + 1) * 8 + 256;           // frame-major copy of f-major phasors
}

extern "C" int svs_transpose_c64(const float* in, float* out, int rows, int cols, hipStream_t stream) {
  SVS_REQUIRE(in && out && rows > 0 && cols > 0, "svs_transpose_c64: bad arguments");
  dim3 grid((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32));
  hipLaunchKernelGGL(transpose_c64_kernel, grid, dim3(256), 0, stream, (const float2*)in, (float2*)out, rows, cols);
  SVS_CHECK_LAUNCH("transpose_c64");
  return SVS_OK;
}

extern "C" int svs_istft(const float* mag, const float* phase, int phase_is_angle, int n_fft, int hop, int frames, float* y,
                         void* ws, size_t ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(mag && phase && y && hop > 0 && frames > 1, "svs_istft: bad arguments (need >= 2 frames)");
  SVS_REQUIRE(n_fft == 1024, "svs_istft: only n_fft=1024 (reference config.py:47) is built, got %d", n_fft);
  constexpr int NBIN = 513;
  if (phase_is_angle)
    return svs_istft_tiles(mag, (int64_t)NBIN * frames, frames, NBIN, 0, nullptr, 0, phase, 3, 1, n_fft, hop, frames, y, nullptr, stream);
  if (!ws || ws_bytes < svs_istft_workspace_bytes(n_fft, hop, frames) || !svs_aligned16(ws)) { svs_set_error("svs_istft: workspace too small"); return SVS_ERR_WORKSPACE; }
  int rc = svs_transpose_c64(phase, (float*)ws, NBIN, frames, stream);
  if (rc) return rc;
  return svs_istft_tiles(mag, (int64_t)NBIN * frames, frames, NBIN, 0, nullptr, 0, (const float*)ws, 1, 1, n_fft, hop, frames, y, nullptr, stream);
}

// Transpose of the differentiable inverse of train.py:33-60 (`specific_istft`), fused with the mask's chain rule:
//   d_logit[b, f, t] += alpha * dL/d|S|[b, f+1, t] * mix * mask * (1 - mask),   |S| = mask * mix (train.py:275,288)
// d_wav: (B, hop * (T - 1)); angle / mix / mask / d_logit: (B, 1, n_fft / 2, T) training tiles.  n_fft = 512, 1024 or 2048 and
// any 0 < hop <= n_fft (the envelope division of SRC_ENVDIV walks however many frames cover a sample).
template <int N>
static int launch_istft_bwd(StftArgs& a, hipStream_t stream) {
  const size_t lds = fwd_lds_bytes(N, true);
  int rc = allow_lds(stft_fwd_kernel<N, SRC_ENVDIV, SINK_DMAG>, lds);
  if (rc) return rc;
  if ((rc = svs_fft_twiddles(N, stream, &a.twiddles))) return rc;
  if (N != 1024 && (rc = svs_fft_hann(N, stream, &a.hann))) return rc;
  dim3 grid((unsigned)((a.T + GROUP - 1) / GROUP), (unsigned)a.channels);
  hipLaunchKernelGGL((stft_fwd_kernel<N, SRC_ENVDIV, SINK_DMAG>), grid, dim3(512), lds, stream, a);
  SVS_CHECK_LAUNCH("istft_bwd");
  return SVS_OK;
}
extern "C" int svs_istft_bwd_mask(const float* d_wav, const float* angle, const float* mix, const float* mask, float* d_logit,
                                  float alpha, int B, int n_fft, int hop, int frames, hipStream_t stream) {
  SVS_REQUIRE(d_wav && angle && mix && mask && d_logit && B > 0 && frames > 1 && hop > 0, "svs_istft_bwd_mask: bad arguments");
  SVS_REQUIRE_NFFT("svs_istft_bwd_mask", n_fft);
  SVS_REQUIRE(hop <= n_fft, "svs_istft_bwd_mask: hop %d > n_fft leaves samples that no frame covers", hop);
  SVS_REQUIRE(B <= 65535, "svs_istft_bwd_mask: B = %d exceeds the grid's 65535 channels", B);
  const int nbin = n_fft / 2 + 1;
  StftArgs a{};
  a.y = d_wav; a.n_samples = (long)hop * (frames - 1); a.channels = B; a.hop = hop; a.T = frames;
  a.lay = SpecLayout{(long)(nbin - 1) * frames, frames, nbin - 1, 1, frames};
  a.angle = angle; a.mix = mix; a.mask = mask; a.d_logit = d_logit; a.alpha = alpha;
  return n_fft == 512 ? launch_istft_bwd<512>(a, stream) : n_fft == 1024 ? launch_istft_bwd<1024>(a, stream) : launch_istft_bwd<2048>(a, stream);
}
