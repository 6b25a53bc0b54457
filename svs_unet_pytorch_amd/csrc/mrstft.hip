// Multi-resolution STFT loss on the GPU (gfx950): forward value and gradient with respect to the predicted waveform.
//
// The reference adds `alpha_MR * auraloss.freq.MultiResolutionSTFTLoss(sample_rate=SAMPLE_RATE, device=device)(pred_wav,
// target_wav)` to the L1 terms (train.py:24-26,287-296).  auraloss 0.4.0 (uv.lock:90-91) is NOT vendored and not
// installable here, so this file restates its published definition for the constructor arguments the reference passes
// (everything else at its default) -- PARITY UNPINNED against auraloss itself; pinned against oracle/mrstft_oracle.py,
// which states the same definition on torch.stft:
//   three resolutions (n_fft, hop, win_length) = (1024, 120, 600), (2048, 240, 1200), (512, 50, 240); per resolution
//   X = torch.stft(x, n_fft, hop, win_length, hann_window(win_length), center=True, pad_mode="reflect"),
//   |X| = sqrt(clamp(re^2 + im^2, min=1e-8));  loss = mean_b( ||Y_b| - |X_b||_F / ||Y_b||_F )  +  mean |log|X| - log|Y||
//   (w_sc = w_log_mag = 1; the spectral-convergence ratio is taken PER WAVEFORM of the batch and averaged, as 0.4.0's
//   SpectralConvergenceLoss does with norm(dim=[-1, -2]) -- the 0.2.x form took one ratio over the whole batch tensor);
//   result = mean over the three resolutions.
//
// Kernels (one template per n_fft, fft_wave.h transforms, 512-thread blocks = 8 independent waves):
//   mr_sums_kernel  one wave per frame position: the predicted and the target frame share ONE complex FFT (x in the
//                   real part, y in the imaginary part); per-block partial sums of (|Y|-|X|)^2, |Y|^2, |log|X|-log|Y||.
//   mr_finalize     fixed-order double-precision sums -> loss value, the log-magnitude gradient coefficient per resolution and
//                   the spectral-convergence gradient coefficient per resolution and waveform.
//   mr_pass_kernel  (when the gradient is wanted, instead of mr_sums) the same sums AND, from the same spectra, both unscaled
//                   gradient parts of the frame brought back with ONE inverse FFT (real / imaginary part);
//                   the 8 frames of a block are overlap-added in LDS (fixed order) and leave as ONE segment of
//                   7 hop + win samples -- a third of the bytes of the 8 windowed frames (hop is win / 5).
//   mr_ola_kernel   gathers, per output sample, the (at most two) segments that cover it, for the sample itself and for the
//                   two reflect-padding mirrors, in a fixed order -- no atomics, bitwise reproducible.
// Bound: HBM + VALU (FFT); algorithmic FLOPs ~ 2.5 * 5 N log2 N per frame position.
#include "internal.h"
#include "fft_wave.h"

#define MR_NRES 3
static const int MR_NFFT[MR_NRES] = {1024, 2048, 512};
static const int MR_HOP[MR_NRES] = {120, 240, 50};
static const int MR_WIN[MR_NRES] = {600, 1200, 240};
#define MR_EPS 1e-8f

// 8 waves (= independent transforms) per block at every size: 79 KB of LDS for 1024 points (two blocks per CU), 158 KB for 2048
// (one block per CU; three waves per block, which fits twice, measured 1.65x slower: 530 vs 321 us for the gradient kernel).
// No window table in LDS -- the window is one v_cos_f32 per sample.
template <int N> struct MrCfg {
  static constexpr int WAVES = 8;
  static constexpr int WIN = (N == 2048) ? 1200 : (N == 1024) ? 600 : 240;      // = MR_WIN of this n_fft (checked on the host)
  static constexpr int HOP = (N == 2048) ? 240 : (N == 1024) ? 120 : 50;          // = MR_HOP of this n_fft (checked on the host)
  static constexpr int OFF = (N - WIN) / 2, NJ = (WIN + 63) / 64;
};
static int mr_waves(int n) { (void)n; return 8; }

struct MrArgs {
  const float* x; const float* y; int B; long L;     // predicted / target waveforms (B, L)
  int hop, win, F;                                   // this resolution: hop, window length, frames = 1 + L / hop
  float* partial;                                    // [B * gridDim.x][3]
  const float* coef;                                 // [1 + B]: log-magnitude coefficient, then the SC coefficient of every waveform (device)
  float* frames;                                     // [B][ceil(F / 8)][7 hop + win] (sc, log) pairs: the blocks' overlap-added frame gradients ("segments")
  const float2* twiddles;                            // this n_fft's table (svs_fft_twiddles)
};

// periodic Hann window of `win` samples, centred inside n_fft (torch.stft pads a short window on both sides), sample j of the
// window; v_cos_f32 takes revolutions (absolute error ~1e-6, far below the loss tolerance)
__device__ __forceinline__ float mr_window_at(int j, float inv_win) { return 0.5f - 0.5f * __builtin_amdgcn_cosf((float)j * inv_win); }   // 0 <= j < win
__device__ __forceinline__ long mr_reflect(long p, long L) { return p < 0 ? -p : (p >= L ? 2 * (L - 1) - p : p); }

// frame t of x (real part) and y (imaginary part), windowed, into the wave's buffer
template <int N>
__device__ __forceinline__ void mr_fill(float2* buf, const MrArgs& p, int b, int t, int lane) {
  constexpr int WIN = MrCfg<N>::WIN, off = MrCfg<N>::OFF;   // the window covers samples off .. off + win - 1 of the frame: nothing else is read
  const float inv_win = 1.0f / (float)WIN;
#pragma unroll 4
  for (int r = 0; r < N / 64; ++r) {
    const int m = lane + 64 * r, j = m - off;
    float2 v = float2{0.f, 0.f};
    if (t < p.F && j >= 0 && j < WIN) {
      const long s = mr_reflect((long)t * p.hop + m - N / 2, p.L);
      const float w = mr_window_at(j, inv_win);
      v = float2{p.x[(long)b * p.L + s] * w, p.y[(long)b * p.L + s] * w};
    }
    buf[fft_pad(m)] = v;
  }
}
// spectra of the two real signals that shared the transform
__device__ __forceinline__ void mr_split(const float2 zk, const float2 zn, float2& X, float2& Y) {
  X = float2{0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)};
  Y = float2{0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x)};
}

template <int N>
__global__ __launch_bounds__(64 * MrCfg<N>::WAVES) void mr_sums_kernel(MrArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int BUF = FftSize<N>::BUF, TW = FftSize<N>::TW, WV = MrCfg<N>::WAVES;
  float2* const fbuf = (float2*)smem;
  float2* const tw = fbuf + WV * BUF;
  float* const red = (float*)(tw + TW);              // [WV][3]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, t = blockIdx.x * WV + wave;
  fft_load_twiddles<N>(tw, p.twiddles, tid, 64 * WV);
  float2* const buf = fbuf + wave * BUF;
  mr_fill<N>(buf, p, b, t, lane);
  __syncthreads();
  fft_wave<N>(buf, tw, lane);
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (t < p.F) {
#pragma unroll
    for (int r = 0; r < N / 128 + 1; ++r) {
      const int k = lane + 64 * r;
      if (k > N / 2) continue;
      float2 X, Y;
      mr_split(buf[fft_pad(k)], buf[fft_pad((N - k) & (N - 1))], X, Y);
      // one-instruction sqrt / log2 (v_sqrt_f32, v_log_f32: ~1 ulp): the kernel is VALU-bound, and |log|X| - log|Y|| =
      // (ln 2 / 2) |log2 |X|^2 - log2 |Y|^2| needs no square root at all
      const float x2 = fmaxf(X.x * X.x + X.y * X.y, MR_EPS), y2 = fmaxf(Y.x * Y.x + Y.y * Y.y, MR_EPS);
      const float xm = __builtin_amdgcn_sqrtf(x2), ym = __builtin_amdgcn_sqrtf(y2);
      const float d = ym - xm;
      s1 += d * d;
      s2 += y2;
      s3 += 0.34657359027997264f * fabsf(__builtin_amdgcn_logf(x2) - __builtin_amdgcn_logf(y2));
    }
  }
  s1 = svs_wave_sum(s1); s2 = svs_wave_sum(s2); s3 = svs_wave_sum(s3);
  if (lane == 0) { red[wave * 3] = s1; red[wave * 3 + 1] = s2; red[wave * 3 + 2] = s3; }
  __syncthreads();
  if (tid < 3) {
    float a = 0.f;
    for (int w = 0; w < WV; ++w) a += red[w * 3 + tid];
    p.partial[((long)b * gridDim.x + blockIdx.x) * 3 + tid] = a;
  }
}

struct MrFinalArgs {
  const float* partial[MR_NRES]; int gx[MR_NRES]; double count[MR_NRES];        // partial[r]: [B][gx[r]][3]
  int B; float grad_scale; double* terms; float* coef[MR_NRES];                 // terms: [MR_NRES] this resolution's loss; coef[r]: [1 + B]
};
// One block per resolution, one wave per waveform (16 waves walk b = wave, wave + 16, ...): the lanes sum that waveform's gx
// block partials, lane 0 forms its spectral-convergence ratio and gradient coefficient and keeps the wave's running sums;
// thread 0 adds the 16 waves' sums in a fixed order.  Everything in double, every order fixed: bitwise reproducible.  (One
// block for all three resolutions took 28 us -- twelve dependent (resolution, waveform) rounds per wave; the three terms are
// added by whoever runs next: mr_ola, or mr_total for a value-only call.)
__global__ __launch_bounds__(1024) void mr_finalize_kernel(MrFinalArgs a) {
  __shared__ double sh[2][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
  double ratio_sum = 0.0, log_sum = 0.0;
  for (int b = wave; b < a.B; b += 16) {
    double s[3] = {0.0, 0.0, 0.0};
    const float* pb = a.partial[r] + (long)b * a.gx[r] * 3;
    for (int i = lane; i < a.gx[r]; i += 64)
      for (int j = 0; j < 3; ++j) s[j] += (double)pb[(long)i * 3 + j];
    for (int j = 0; j < 3; ++j)
      for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, 64);
    if (lane == 0) {
      const double nd = sqrt(s[0]), ny = sqrt(s[1]);
      ratio_sum += ny > 0.0 ? nd / ny : 0.0;
      log_sum += s[2];
      // d/d|X_b| of  (1/B) ||Y_b|-|X_b||_F / ||Y_b||_F  is  -(|Y_b|-|X_b|) / (B ||Y_b|-|X_b||_F ||Y_b||_F)
      a.coef[r][1 + b] = (nd > 0.0 && ny > 0.0) ? (float)((double)a.grad_scale / (MR_NRES * (double)a.B * nd * ny)) : 0.f;
    }
  }
  if (lane == 0) { sh[0][wave] = ratio_sum; sh[1][wave] = log_sum; }
  __syncthreads();
  if (tid == 0) {
    double ratio = 0.0, lg = 0.0;
    for (int w = 0; w < 16; ++w) { ratio += sh[0][w]; lg += sh[1][w]; }
    a.terms[r] = ratio / (double)a.B + lg / a.count[r];
    a.coef[r][0] = (float)((double)a.grad_scale / (MR_NRES * a.count[r]));      // of the mean log distance: sign / (count |X|)
  }
}
__device__ __forceinline__ float mr_total(const double* terms) {              // mean over the resolutions, in their fixed order
  double t = 0.0;
  for (int r = 0; r < MR_NRES; ++r) t += terms[r];
  return (float)(t / MR_NRES);
}
__global__ void mr_total_kernel(const double* terms, float* loss) { loss[0] = mr_total(terms); }

// ONE pass for the loss value AND the gradient (used whenever the gradient is asked for): a wave transforms frame t once (x real,
// y imaginary), adds the frame's three partial sums, and forms BOTH gradient spectra from the same X, Y -- the
// spectral-convergence part -(|Y| - |X|) X / |X| and the log-magnitude part sign(|X| - |Y|) X / |X|^2, each WITHOUT its global
// coefficient (1 / (B ||Y_b| - |X_b|| ||Y_b||) is known only after all frames: mr_finalize) -- as the real and imaginary part of
// one inverse transform.  Everything after the spectra is linear, so the coefficients are applied at the very end, in mr_ola.
// Two transforms per frame; the two-pass form (sums, then spectra again for the gradient, two frames per inverse) needed 2.5.
// The block's 8 frames are overlap-added in LDS (fixed order) and leave as ONE segment of 7 hop + win positions x (sc, log): a
// third of the bytes of the windowed frames.
template <int N>
__global__ __launch_bounds__(64 * MrCfg<N>::WAVES) void mr_pass_kernel(MrArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int BUF = FftSize<N>::BUF, TW = FftSize<N>::TW, NR = N / 128 + 1, WV = MrCfg<N>::WAVES;
  float2* const fbuf = (float2*)smem;
  float2* const tw = fbuf + WV * BUF;
  float* const red = (float*)(tw + TW);              // [WV][3]
  float* const unbalance = red + 3 * WV;             // [WV]: what takes a frame's log part back to its scale (below)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, t = blockIdx.x * WV + wave;
  fft_load_twiddles<N>(tw, p.twiddles, tid, 64 * WV);
  float2* const buf = fbuf + wave * BUF;
  mr_fill<N>(buf, p, b, t, lane);                    // (zeros past the last frame)
  __syncthreads();
  fft_wave<N>(buf, tw, lane);
  float s1 = 0.f, s2 = 0.f, s3 = 0.f, es = 0.f, el = 0.f;     // (es, el: energy of the frame's two gradient spectra, see below)
  float2 Hs[NR], Hl[NR];                             // Hermitian-weighted, unscaled dL/dX: spectral-convergence and log-magnitude parts
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int k = lane + 64 * r;
    Hs[r] = Hl[r] = float2{0.f, 0.f};
    if (k <= N / 2 && t < p.F) {
      float2 X, Y;
      mr_split(buf[fft_pad(k)], buf[fft_pad((N - k) & (N - 1))], X, Y);
      const float x2r = X.x * X.x + X.y * X.y;
      const float x2 = fmaxf(x2r, MR_EPS), y2 = fmaxf(Y.x * Y.x + Y.y * Y.y, MR_EPS);
      const float xm = __builtin_amdgcn_sqrtf(x2), ym = __builtin_amdgcn_sqrtf(y2);
      const float d = ym - xm;
      s1 += d * d;
      s2 += y2;
      s3 += 0.34657359027997264f * fabsf(__builtin_amdgcn_logf(x2) - __builtin_amdgcn_logf(y2));
      if (x2r > MR_EPS) {                            // clamp(min=eps) passes no gradient below eps
        const float ix = __builtin_amdgcn_rcpf(xm);
        const bool edge = (k == 0 || k == N / 2);
        const float h = (edge ? 1.0f : 0.5f) * ix;
        const float gs = -d * h, gl = (x2 > y2 ? 1.f : (x2 < y2 ? -1.f : 0.f)) * ix * h;      // sign(log|X| - log|Y|) = sign(|X|^2 - |Y|^2)
        Hs[r] = float2{gs * X.x, edge ? 0.f : gs * X.y};
        Hl[r] = float2{gl * X.x, edge ? 0.f : gl * X.y};
        es += gs * gs * x2r;
        el += gl * gl * x2r;
      }
    }
  }
  // The two parts share one inverse transform, whose rounding error is relative to the LARGER part -- and unscaled they are
  // |log part| / |sc part| ~ 1 / (|X| (|Y| - |X|)) apart: 1e8 for a waveform at -90 dBFS, where the spectral-convergence part
  // came back as noise several times the whole gradient (and, the other way round, 1e-4 at full scale).  So the frame's log part
  // goes through the transform times the power of two that brings its energy to the sc part's (exact), and the overlap-add
  // below takes that factor out again.
  es = svs_wave_sum(es); el = svs_wave_sum(el);      // (the same bits in every lane)
  int bal = 0;                                       // half the difference of the two energies' binary exponents
  if (es > 0.f && el > 0.f && es < INFINITY && el < INFINITY) {
    bal = ((int)(__float_as_uint(es) >> 23) - (int)(__float_as_uint(el) >> 23)) / 2;
    bal = bal < -48 ? -48 : (bal > 48 ? 48 : bal);
  }
  const float balance = __uint_as_float((unsigned)(127 + bal) << 23);      // 2^bal
#pragma unroll
  for (int r = 0; r < NR; ++r) { Hl[r].x *= balance; Hl[r].y *= balance; }
  if (lane == 0) unbalance[wave] = __uint_as_float((unsigned)(127 - bal) << 23);
  fft_wave_sync();                                   // every lane has read the spectra before the buffer is refilled
  // conj(Z), Z = Hs + i Hl extended Hermitian; forward transform -> conj(ifft(Z)) = g_sc - i g_log
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int k = lane + 64 * r;
    if (k > N / 2) continue;
    const float2 a = Hs[r], c = Hl[r];
    buf[fft_pad(k)] = float2{a.x - c.y, -(a.y + c.x)};
    if (k > 0 && k < N / 2) buf[fft_pad(N - k)] = float2{a.x + c.y, -(c.x - a.y)};
  }
  fft_wave<N>(buf, tw, lane);
  s1 = svs_wave_sum(s1); s2 = svs_wave_sum(s2); s3 = svs_wave_sum(s3);
  if (lane == 0) { red[wave * 3] = s1; red[wave * 3 + 1] = s2; red[wave * 3 + 2] = s3; }
  __syncthreads();
  if (tid < 3) {
    float a = 0.f;
    for (int w = 0; w < WV; ++w) a += red[w * 3 + tid];
    p.partial[((long)b * gridDim.x + blockIdx.x) * 3 + tid] = a;
  }
  // ---- overlap-add of the block's WV frames (local frame f = its wave) over their common support: local position i = f hop + j,
  // j = index inside the window.  A thread owns positions tid, tid + 64 WV, ... and adds the <= ceil(win / hop) frames that
  // cover each in ascending f: a fixed order.
  constexpr int WIN = MrCfg<N>::WIN, off = MrCfg<N>::OFF, HOP = MrCfg<N>::HOP;      // (compile-time hop: the divisions below are multiplications)
  const int t0 = blockIdx.x * WV;
  constexpr int SL = (WV - 1) * HOP + WIN;
  float2* const seg = (float2*)p.frames + ((long)b * gridDim.x + blockIdx.x) * SL;
  const float inv_win = 1.0f / (float)WIN;
  for (int i = tid; i < SL; i += 64 * WV) {
    int f_hi = (int)((unsigned)i / (unsigned)HOP);
    if (f_hi > WV - 1) f_hi = WV - 1;
    if (t0 + f_hi > p.F - 1) f_hi = p.F - 1 - t0;
    int f_lo = i - (WIN - 1);
    f_lo = f_lo <= 0 ? 0 : (int)((unsigned)(f_lo + HOP - 1) / (unsigned)HOP);
    float2 s = float2{0.f, 0.f};
    for (int f = f_lo; f <= f_hi; ++f) {
      const int j = i - f * HOP;
      const float2 z = fbuf[f * BUF + fft_pad(j + off)];
      const float w = mr_window_at(j, inv_win);
      s.x += z.x * w;
      s.y -= z.y * (w * unbalance[f]);
    }
    seg[i] = s;
  }
}

struct MrOlaArgs {
  const float* frames[MR_NRES]; const float* coef[MR_NRES]; int n[MR_NRES], hop[MR_NRES], F[MR_NRES], win[MR_NRES];
  int B; long L; float* d_x; const double* terms; float* loss;
};
// contributions of padded position q (= p + N/2) of one resolution to its sample: in "frame-window" coordinates u = q - off
// (= hop t + j for a frame t and a window index j) the sample takes the block segments that cover u -- segment k spans
// [8 hop k, 8 hop k + 7 hop + win) -- at most two of them, the earlier block first: a fixed order.  (sc, log) pairs.
// (n_fft, window, hop are template arguments: the division by the segment span is then a multiplication -- with run-time values the
// three resolutions' gathers were ~45 % of this kernel's instructions in divisions)
template <int N, int win, int hop>
__device__ __forceinline__ float2 mr_gather(const float2* sg, int nseg, int q) {
  const int u = q - (N - win) / 2;                        // (32-bit throughout: L + n_fft < 2^31 is checked on the host)
  float2 s = float2{0.f, 0.f};
  if (u < 0) return s;
  constexpr int span = 8 * hop, SL = 7 * hop + win;
  const int k = (int)((unsigned)u / (unsigned)span);
  const int r = u - k * span;                             // position inside segment k
  if (k >= 1 && k - 1 < nseg && r + span < SL) { const float2 v = sg[(long)(k - 1) * SL + r + span]; s.x += v.x; s.y += v.y; }   // the previous segment's tail
  if (k < nseg && r < SL) { const float2 v = sg[(long)k * SL + r]; s.x += v.x; s.y += v.y; }
  return s;
}
__global__ __launch_bounds__(256) void mr_ola_kernel(MrOlaArgs a) {
  const int L = (int)a.L;
  // one waveform per blockIdx.y: no division by L per sample
  const int b = blockIdx.y;
  if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) a.loss[0] = mr_total(a.terms);
  for (int nidx = blockIdx.x * 256 + threadIdx.x; nidx < L; nidx += gridDim.x * 256) {
    float s = 0.f;
    auto one = [&](auto rc, auto nc, auto wc, auto hc) __attribute__((always_inline)) {
      constexpr int r = decltype(rc)::value, N = decltype(nc)::value, WIN = decltype(wc)::value, HOP = decltype(hc)::value, half = N / 2;
      const int nseg = (a.F[r] + 7) / 8;
      const float2* fr = (const float2*)a.frames[r] + (long)b * nseg * (7 * HOP + WIN);
      float2 g = mr_gather<N, WIN, HOP>(fr, nseg, nidx + half);                                                       // the sample itself
      if (nidx >= 1 && nidx <= half) { const float2 v = mr_gather<N, WIN, HOP>(fr, nseg, half - nidx); g.x += v.x; g.y += v.y; }   // left mirror: p = -n
      const int pr = 2 * (L - 1) - nidx;                                                                              // right mirror: p = 2(L-1) - n
      if (nidx <= L - 2 && pr < L + half) { const float2 v = mr_gather<N, WIN, HOP>(fr, nseg, pr + half); g.x += v.x; g.y += v.y; }
      s += a.coef[r][1 + b] * g.x + a.coef[r][0] * g.y;         // the global coefficients of mr_finalize: spectral convergence (per waveform), log magnitude
    };
    using std::integral_constant;                                // the three resolutions, in MR_NFFT / MR_WIN / MR_HOP order (checked on the host)
    one(integral_constant<int, 0>{}, integral_constant<int, 1024>{}, integral_constant<int, 600>{}, integral_constant<int, 120>{});
    one(integral_constant<int, 1>{}, integral_constant<int, 2048>{}, integral_constant<int, 1200>{}, integral_constant<int, 240>{});
    one(integral_constant<int, 2>{}, integral_constant<int, 512>{}, integral_constant<int, 240>{}, integral_constant<int, 50>{});
    a.d_x[(long)b * L + nidx] = s;
  }
}

// ---- host side -----------------------------------------------------------------------------------
// (wave buffers, twiddles, [WAVES][3] partial sums, [WAVES] log-part factors of mr_pass)
template <int N> static size_t mr_lds_bytes() { return (size_t)MrCfg<N>::WAVES * FftSize<N>::BUF * 8 + FftSize<N>::TW * 8 + MrCfg<N>::WAVES * 3 * 4 + MrCfg<N>::WAVES * 4; }
struct MrWs { float* partial[MR_NRES]; int nblk[MR_NRES]; float* frames[MR_NRES]; float* coef; double* terms; size_t total; };
static MrWs mr_layout(int B, long L, void* ws) {
  MrWs w{};
  char* base = (char*)ws;
  size_t used = 0;
  auto take = [&](size_t nfloats) { float* p = base ? (float*)(base + used) : nullptr; used += svs_align_up(nfloats * 4, 256); return p; };
  w.coef = take((size_t)MR_NRES * (1 + B));
  w.terms = (double*)take(2 * MR_NRES);
  for (int r = 0; r < MR_NRES; ++r) {
    const int F = (int)(1 + L / MR_HOP[r]);
    w.nblk[r] = B * ((F + mr_waves(MR_NFFT[r]) - 1) / mr_waves(MR_NFFT[r]));
    w.partial[r] = take((size_t)w.nblk[r] * 3);
    w.frames[r] = take((size_t)2 * B * ((F + 7) / 8) * (7 * MR_HOP[r] + MR_WIN[r]));     // one overlap-added (sc, log) segment per block of 8 frames
  }
  w.total = used;
  return w;
}
extern "C" size_t svs_mrstft_workspace_bytes(int B, int64_t L) { return B > 0 && L > 0 ? mr_layout(B, L, nullptr).total : 0; }

template <int N>
static int mr_launch(bool grad, const MrArgs& a, int B, hipStream_t stream) {      // grad: the one-pass kernel (sums + gradient segments), else the sums only
  const size_t lds = mr_lds_bytes<N>();
  constexpr int per = MrCfg<N>::WAVES;
  const dim3 grid((unsigned)((a.F + per - 1) / per), (unsigned)B), block(64 * MrCfg<N>::WAVES);
  if (grad) {
    SVS_HIP(hipFuncSetAttribute((const void*)mr_pass_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mr_pass_kernel<N>, grid, block, lds, stream, a);
  } else {
    SVS_HIP(hipFuncSetAttribute((const void*)mr_sums_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mr_sums_kernel<N>, grid, block, lds, stream, a);
  }
  SVS_CHECK_LAUNCH(grad ? "mr_pass" : "mr_sums");
  return SVS_OK;
}

// loss[0] = MultiResolutionSTFTLoss(x, y); d_x (may be NULL) = grad_scale * d loss / d x.   x, y, d_x: (B, L) fp32.
extern "C" int svs_mrstft_loss_fwd_bwd(const float* x, const float* y, int B, int64_t L, float grad_scale, float* loss, float* d_x,
                                       void* ws, size_t ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(x && y && loss && B > 0 && B <= 65535 && L > 2048 && L < (1L << 30), "svs_mrstft_loss_fwd_bwd: bad arguments (need 2048 < L < 2^30 -- reflect padding, 32-bit sample indices -- and B <= 65535)");
  const MrWs w = mr_layout(B, L, ws);
  if (!ws || ws_bytes < w.total || !svs_aligned16(ws)) { svs_set_error("svs_mrstft_loss_fwd_bwd: workspace too small (%zu < %zu)", ws_bytes, w.total); return SVS_ERR_WORKSPACE; }
  static_assert(MrCfg<1024>::WIN == 600 && MrCfg<2048>::WIN == 1200 && MrCfg<512>::WIN == 240, "MrCfg::WIN must match MR_WIN");
  SVS_REQUIRE(MR_NFFT[0] == 1024 && MR_NFFT[1] == 2048 && MR_NFFT[2] == 512 && MR_HOP[0] == 120 && MR_HOP[1] == 240 && MR_HOP[2] == 50 &&
              MR_WIN[0] == 600 && MR_WIN[1] == 1200 && MR_WIN[2] == 240, "svs_mrstft_loss_fwd_bwd: mr_ola_kernel is compiled for other resolutions");
  int rc;
  MrArgs a[MR_NRES];
  MrFinalArgs f{};
  const bool grad = d_x != nullptr;
  MrOlaArgs o{};
  for (int r = 0; r < MR_NRES; ++r) {
    const float2* twiddles = nullptr;
    if ((rc = svs_fft_twiddles(MR_NFFT[r], stream, &twiddles))) return rc;
    a[r] = MrArgs{x, y, B, (long)L, MR_HOP[r], MR_WIN[r], (int)(1 + L / MR_HOP[r]), w.partial[r], w.coef + (size_t)r * (1 + B), w.frames[r], twiddles};
    rc = MR_NFFT[r] == 1024 ? mr_launch<1024>(grad, a[r], B, stream) : MR_NFFT[r] == 2048 ? mr_launch<2048>(grad, a[r], B, stream)
                                                                                             : mr_launch<512>(grad, a[r], B, stream);
    if (rc) return rc;
    f.partial[r] = w.partial[r]; f.gx[r] = w.nblk[r] / B; f.coef[r] = w.coef + (size_t)r * (1 + B);
    f.count[r] = (double)B * a[r].F * (MR_NFFT[r] / 2 + 1);
    o.frames[r] = w.frames[r]; o.coef[r] = f.coef[r]; o.n[r] = MR_NFFT[r]; o.hop[r] = MR_HOP[r]; o.F[r] = a[r].F; o.win[r] = MR_WIN[r];
  }
  f.B = B; f.grad_scale = grad_scale; f.terms = w.terms;
  hipLaunchKernelGGL(mr_finalize_kernel, dim3(MR_NRES), dim3(1024), 0, stream, f);
  SVS_CHECK_LAUNCH("mr_finalize");
  if (!grad) {
    hipLaunchKernelGGL(mr_total_kernel, dim3(1), dim3(1), 0, stream, (const double*)w.terms, loss);
    SVS_CHECK_LAUNCH("mr_total");
    return SVS_OK;
  }
  o.B = B; o.L = L; o.d_x = d_x; o.terms = w.terms; o.loss = loss;
  long g = (L + 255) / 256;
  if (g > 1024) g = 1024;
  hipLaunchKernelGGL(mr_ola_kernel, dim3((unsigned)g, (unsigned)B), dim3(256), 0, stream, o);
  SVS_CHECK_LAUNCH("mr_ola");
  return SVS_OK;
}
