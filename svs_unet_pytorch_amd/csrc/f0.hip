// YIN fundamental-frequency tracker on the device (include/svs_hip.h; the float64 definition is svs_unet_pytorch_amd/f0.py, DESIGN.md
// section 26): steps 1 to 5 of de Cheveigne & Kawahara (JASA 2002).  The reference has no pitch estimator of any kind.
//
// One wave owns one frame; a block owns F <= 4 consecutive frames of one row (64 F threads) and stages their span + (F - 1) hop samples
// once in LDS.  Where hop >= span the frames share no sample and F = 1.  F, and the lags a lane owns, follow from (W, tau_max, hop)
// alone, and no wave reads what another wave computed, so a frame's values depend neither on the grid nor on its neighbours in the
// block: every d(tau) is ONE chain of fp64 FMAs over j = 0 .. W-1 in ascending order.
//
// Difference function.  A lane owns L consecutive lags (L = 2, 4 or 8 by tau_max, so that a short lag range still fills the wave) and
// slides an L-sample register window along x[j + tau]: per j one LDS read of x[j] (one address for the whole wave: a broadcast) and
// one of x[j + tau0 + L - 1] feed L subtractions in fp32, L conversions and L fp64 FMAs.  The lanes' window reads are L words apart,
// which would put 32 lanes on 32 / L banks; the staged signal carries one word of padding after every L (f0_pad), so the lanes are
// L + 1 words apart -- odd, hence 32 different banks.  tau_max lags take ceil(tau_max / 64 L) passes.
//
// S(tau) is a scan over the lags in fp64: within the lane in order, an inclusive Hillis-Steele scan of the lanes' totals, and a
// carry from pass to pass.  d'(tau) is rounded once to float32 and kept in the wave's LDS row, from where svs_f0_cmnd copies it out
// and svs_f0_track picks; svs_f0_pick runs the same pick on a row in memory.  The pick's two searches are wave minima over
// (value, index) that keep the smallest index on ties.  No atomics, 64-bit indices, nothing returns to the host.
// The per-frame device functions live in f0_frame.h, which f0_smooth.hip (candidates and the Viterbi decode) includes as well.
#include "f0_frame.h"

// FUSED: svs_f0_track (d' stays in LDS); otherwise svs_f0_cmnd (d' and, where asked for, rms go to memory)
template <int LOG2L, bool FUSED>
__global__ __launch_bounds__(64 * F0_MAX_FRAMES) void f0_kernel(const float* __restrict__ x, long ld_row, int W, int tau_min, int tau_max, int hop,
                                                                long first_frame, long n_frames, int F, int xcap, double threshold,
                                                                float rms_gate, double sr, float* __restrict__ dprime,
                                                                float* __restrict__ rms, float* __restrict__ f0, float* __restrict__ ap,
                                                                int* __restrict__ voiced) {
  extern __shared__ float f0_lds[];                                   // xcap floats of signal, then F rows of tau_max + 1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long fb = (long)blockIdx.x * F;                               // the block's first frame within the call
  const int nf = (int)min((long)F, n_frames - fb);
  const int len = W + tau_max + (nf - 1) * hop;
  const float* xr = x + (long)blockIdx.y * ld_row + (first_frame + fb) * (long)hop;
  f0_stage<LOG2L>(xr, len, tid, (int)blockDim.x, f0_lds);
  __syncthreads();
  float* dp = f0_lds + xcap + wave * (tau_max + 1);
  const bool active = wave < nf;
  float r = 0.f;
  if (active) r = f0_frame_cmnd<LOG2L>(f0_lds, wave * hop, W, tau_max, lane, dp);
  __syncthreads();                                                    // the row is complete before other lanes read it
  if (!active) return;
  const long o = (long)blockIdx.y * n_frames + fb + wave;
  if (FUSED) {
    f0_frame_pick(dp, tau_min, tau_max, threshold, sr, lane, true, r, rms_gate, f0 + o, ap + o, voiced + o);
    if (lane == 0) rms[o] = r;
  } else {
    float* out = dprime + o * (long)(tau_max + 1);
    for (int t = lane; t <= tau_max; t += 64) out[t] = dp[t];
    if (rms && lane == 0) rms[o] = r;
  }
}

__global__ __launch_bounds__(256) void f0_pick_kernel(const float* __restrict__ dprime, long count, int tau_min, int tau_max, double threshold,
                                                      const float* __restrict__ rms, float rms_gate, double sr, float* __restrict__ f0,
                                                      float* __restrict__ ap, int* __restrict__ voiced) {
  const int lane = threadIdx.x & 63;
  const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= count) return;
  f0_frame_pick(dprime + f * (long)(tau_max + 1), tau_min, tau_max, threshold, sr, lane, rms != nullptr, rms ? rms[f] : 0.f, rms_gate, f0 + f,
                ap + f, voiced + f);
}

// ------------------------------------------------------------------------------------------------
// host side (the plan and the argument rules are f0_frame.h's)
// ------------------------------------------------------------------------------------------------
template <bool FUSED>
static int f0_launch(const char* who, const float* x, int rows, int64_t ld_row, int W, int tau_min, int tau_max, int hop, int64_t first_frame,
                     int64_t n_frames, double threshold, float rms_gate, double sr, float* dprime, float* rms, float* f0, float* ap, int* voiced,
                     hipStream_t stream) {
  const F0Plan p = f0_plan(W, tau_max, hop);
  const long nblk = (long)((n_frames + p.F - 1) / p.F);
  SVS_REQUIRE(nblk < (1L << 31), "%s: %ld blocks do not fit a grid", who, nblk);
  const dim3 grid((unsigned)nblk, (unsigned)rows), block(64u * p.F);
#define F0_GO(LOG2L)                                                                                                                       \
  hipLaunchKernelGGL((f0_kernel<LOG2L, FUSED>), grid, block, p.lds, stream, x, (long)ld_row, W, tau_min, tau_max, hop, (long)first_frame, \
                     (long)n_frames, p.F, p.xcap, threshold, rms_gate, sr, dprime, rms, f0, ap, voiced)
  if (p.log2l == 1) F0_GO(1);
  else if (p.log2l == 2) F0_GO(2);
  else F0_GO(3);
#undef F0_GO
  SVS_CHECK_LAUNCH(who);
  return SVS_OK;
}

extern "C" int svs_f0_cmnd(const float* x, int rows, int64_t n, int64_t ld_row, int W, int tau_max, int hop, int64_t first_frame, int64_t n_frames,
                           float* dprime, float* rms, hipStream_t stream) {
  const int rc = f0_check_signal("svs_f0_cmnd", x, rows, n, ld_row, W, tau_max, hop, first_frame, n_frames);
  if (rc != SVS_OK) return rc;
  SVS_REQUIRE(n_frames == 0 || (x && dprime), "svs_f0_cmnd: null pointer");
  SVS_REQUIRE((((uintptr_t)dprime) & 3u) == 0 && (((uintptr_t)rms) & 3u) == 0, "svs_f0_cmnd: dprime and rms must be 4-byte aligned");
  if (n_frames == 0) return SVS_OK;
  return f0_launch<false>("svs_f0_cmnd", x, rows, ld_row, W, 1, tau_max, hop, first_frame, n_frames, 0.0, 0.f, 0.0, dprime, rms, nullptr, nullptr,
                          nullptr, stream);
}

extern "C" int svs_f0_pick(const float* dprime, int64_t count, int tau_min, int tau_max, double threshold, const float* rms, float rms_gate,
                           double sr, float* f0, float* ap, int32_t* voiced, hipStream_t stream) {
  const int rc = f0_check_pick("svs_f0_pick", tau_min, tau_max, threshold, rms_gate, sr);
  if (rc != SVS_OK) return rc;
  SVS_REQUIRE(count >= 0 && count <= (INT64_MAX / 16) / (F0_MAX_TAU + 1), "svs_f0_pick: the frame count must not be negative, got %lld",
              (long long)count);
  const long nblk = (long)((count + 3) / 4);
  SVS_REQUIRE(nblk < (1L << 31), "svs_f0_pick: %ld blocks do not fit a grid", nblk);
  SVS_REQUIRE(count == 0 || (dprime && f0 && ap && voiced), "svs_f0_pick: null pointer");
  SVS_REQUIRE(((((uintptr_t)dprime) | ((uintptr_t)rms) | ((uintptr_t)f0) | ((uintptr_t)ap) | ((uintptr_t)voiced)) & 3u) == 0,
              "svs_f0_pick: dprime, rms, f0, ap and voiced must be 4-byte aligned");
  if (count == 0) return SVS_OK;
  hipLaunchKernelGGL(f0_pick_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, dprime, (long)count, tau_min, tau_max, threshold, rms, rms_gate, sr,
                     f0, ap, voiced);
  SVS_CHECK_LAUNCH("svs_f0_pick");
  return SVS_OK;
}

extern "C" int svs_f0_track(const float* x, int rows, int64_t n, int64_t ld_row, int W, int tau_min, int tau_max, int hop, int64_t first_frame,
                            int64_t n_frames, double threshold, float rms_gate, double sr, float* f0, float* ap, float* rms, int32_t* voiced,
                            hipStream_t stream) {
  int rc = f0_check_signal("svs_f0_track", x, rows, n, ld_row, W, tau_max, hop, first_frame, n_frames);
  if (rc != SVS_OK) return rc;
  rc = f0_check_pick("svs_f0_track", tau_min, tau_max, threshold, rms_gate, sr);
  if (rc != SVS_OK) return rc;
  SVS_REQUIRE(n_frames == 0 || (x && f0 && ap && rms && voiced), "svs_f0_track: null pointer");
  SVS_REQUIRE(((((uintptr_t)f0) | ((uintptr_t)ap) | ((uintptr_t)rms) | ((uintptr_t)voiced)) & 3u) == 0,
              "svs_f0_track: f0, ap, rms and voiced must be 4-byte aligned");
  if (n_frames == 0) return SVS_OK;
  return f0_launch<true>("svs_f0_track", x, rows, ld_row, W, tau_min, tau_max, hop, first_frame, n_frames, threshold, rms_gate, sr, nullptr, rms,
                         f0, ap, voiced, stream);
}
