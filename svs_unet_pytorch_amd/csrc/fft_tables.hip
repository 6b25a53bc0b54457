// The twiddle tables of fft_wave.h (N = 512 / 1024 / 2048) built ONCE per device and kept in device memory, so that a transform
// block copies its table (4.6 / 10 / 18 KB, L2-resident) into LDS instead of evaluating 576 / 1280 / 2304 sincospif per block:
// with one or two transforms per wave that evaluation was 10-20 % of the VALU work of the STFT, iSTFT and MR-STFT kernels.
// The entries are the same sincospif values the blocks used to compute themselves: results are bitwise unchanged.
//
// Beside them: the periodic Hann window of the three sizes, entries m = 0 .. N / 2 (the other half by symmetry).  The forward
// STFT of N = 512 / 2048 reads it (stft.hip; the 1024 plan's pass-2 twiddles happen to hold the quarter circle that window
// needs, the other two plans' do not).  The values are computed on the host in double as sin^2(pi m / N) and rounded once --
// 0.5 - 0.5 cos(2 pi m / N) in float loses the small values near the window's ends to cancellation -- and copied to the device
// with the twiddle build; svs_hann_table returns the same array to a host caller.
#include <cmath>
#include <mutex>

#include "internal.h"
#include "fft_wave.h"

#define FFT_TAB_TOTAL (FftSize<512>::TW + FftSize<1024>::TW + FftSize<2048>::TW)
__device__ __attribute__((aligned(16))) float2 g_fft_twiddles[FFT_TAB_TOTAL];

// N / 2 + 1 entries each, every table starting on a 16-byte boundary
#define HANN_OFF_512 0
#define HANN_OFF_1024 260
#define HANN_OFF_2048 (260 + 516)
#define HANN_TAB_TOTAL (260 + 516 + 1028)
__device__ __attribute__((aligned(16))) float g_hann[HANN_TAB_TOTAL];
static int hann_offset(int n) { return n == 512 ? HANN_OFF_512 : n == 1024 ? HANN_OFF_1024 : HANN_OFF_2048; }
static void hann_fill(int n, float* out) {
  for (int m = 0; m <= n / 2; ++m) { const double s = std::sin(M_PI * (double)m / (double)n); out[m] = (float)(s * s); }
  out[n / 2] = 1.0f;
}
extern "C" int svs_hann_table(int n_fft, float* out) {
  SVS_REQUIRE(n_fft == 512 || n_fft == 1024 || n_fft == 2048, "svs_hann_table: n_fft must be 512, 1024 or 2048, got %d", n_fft);
  SVS_REQUIRE(out, "svs_hann_table: null pointer");
  hann_fill(n_fft, out);
  return SVS_OK;
}

__global__ __launch_bounds__(256) void fft_tables_kernel() {
  const int tid = blockIdx.x * 256 + threadIdx.x, n = gridDim.x * 256;
  fft_build_twiddles<512>(g_fft_twiddles, tid, n);
  fft_build_twiddles<1024>(g_fft_twiddles + FftSize<512>::TW, tid, n);
  fft_build_twiddles<2048>(g_fft_twiddles + FftSize<512>::TW + FftSize<1024>::TW, tid, n);
}

// State per device: 0 = not built, 1 = build enqueued (other streams wait for `ready`), 2 = build seen complete.
namespace {
struct TabState { int state = 0; const float2* base = nullptr; const float* hann = nullptr; hipEvent_t ready = nullptr; };
std::mutex g_mu;
TabState g_tab[64];
float g_hann_host[HANN_TAB_TOTAL];               // the source of every device's copy (filled once, under g_mu; never freed)
bool g_hann_host_ready = false;
}

int svs_fft_twiddles(int n, hipStream_t stream, const float2** out) {
  SVS_REQUIRE(n == 512 || n == 1024 || n == 2048, "svs_fft_twiddles: no table for n_fft = %d", n);
  int dev = 0;
  SVS_HIP(hipGetDevice(&dev));
  SVS_REQUIRE(dev >= 0 && dev < 64, "svs_fft_twiddles: device index %d", dev);
  std::lock_guard<std::mutex> guard(g_mu);
  TabState& t = g_tab[dev];
  if (t.state != 2) {                 // (state 2 needs no stream operation at all and is safe inside a capture)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) {
      svs_set_error("svs_fft_twiddles: the first transform of a process must run outside a stream capture (it builds the twiddle tables)");
      return SVS_ERR_INVALID;
    }
    (void)hipGetLastError();
  }
  if (t.state == 0) {
    void *p = nullptr, *ph = nullptr;
    SVS_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(g_fft_twiddles)));
    SVS_HIP(hipGetSymbolAddress(&ph, HIP_SYMBOL(g_hann)));
    if (!g_hann_host_ready) {
      for (int n = 512; n <= 2048; n *= 2) hann_fill(n, g_hann_host + hann_offset(n));
      g_hann_host_ready = true;
    }
    SVS_HIP(hipEventCreateWithFlags(&t.ready, hipEventDisableTiming));
    hipLaunchKernelGGL(fft_tables_kernel, dim3(8), dim3(256), 0, stream);
    SVS_CHECK_LAUNCH("fft_tables");
    SVS_HIP(hipMemcpyAsync(ph, g_hann_host, sizeof(g_hann_host), hipMemcpyHostToDevice, stream));
    SVS_HIP(hipEventRecord(t.ready, stream));
    t.base = (const float2*)p;
    t.hann = (const float*)ph;
    t.state = 1;
  } else if (t.state == 1) {
    // built on some stream, possibly not this one: order this stream behind the build until the host has seen it complete
    if (hipEventQuery(t.ready) == hipSuccess) t.state = 2;
    else {
      (void)hipGetLastError();                     // (hipErrorNotReady is not an error of ours)
      SVS_HIP(hipStreamWaitEvent(stream, t.ready, 0));
    }
  }
  *out = t.base + (n == 512 ? 0 : n == 1024 ? FftSize<512>::TW : FftSize<512>::TW + FftSize<1024>::TW);
  return SVS_OK;
}

int svs_fft_hann(int n, hipStream_t stream, const float** out) {
  const float2* tw = nullptr;
  const int rc = svs_fft_twiddles(n, stream, &tw);          // builds (or orders `stream` behind) both tables
  if (rc) return rc;
  int dev = 0;
  SVS_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> guard(g_mu);
  *out = g_tab[dev].hann + hann_offset(n);
  return SVS_OK;
}
