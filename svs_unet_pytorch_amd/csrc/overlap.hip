// Overlapped tiles for separation (the option beside inference.py:72-120, which cuts a spectrogram into DISJOINT seg-frame tiles):
// tile j of a channel covers frames [j * tile_hop, j * tile_hop + seg), every tile goes through the network alone, and the masks
// are cross-faded back into the disjoint-tile layout the inverse STFT reads.  Two streaming kernels, one on each side of the
// network; one thread = 4 consecutive frames of one row.  4 divides seg and tile_hop, so the four frames lie in one tile, have the
// same contributing tiles and the same offset in each of them: every access is a 16-byte load or store.  No LDS, no atomics.
//
// The cross-fade window w[i] = sin^2(pi * (i + 0.5) / seg), i = 0 .. seg - 1, is computed on the host in double, rounded once and kept
// in device memory per (device, seg) for the life of the process (seg floats; it is never rewritten, so no launch has to be ordered
// behind another one's table).
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "internal.h"

#define OVERLAP_MAX_RATIO 8

static int overlap_grid(long total) {              // 8 blocks of 256 threads on each of the 256 CUs; the rest by grid stride
  long g = (total + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

// the argument rules the two kernels share (include/svs_hip.h)
static int overlap_check(const char* who, int channels, int n_tiles, int rows, int seg, int tile_hop) {
  SVS_REQUIRE(channels > 0 && n_tiles > 0 && rows > 0 && seg > 0 && tile_hop > 0,
              "%s: all sizes must be positive, got channels=%d n_tiles=%d rows=%d seg=%d tile_hop=%d", who, channels, n_tiles, rows, seg, tile_hop);
  SVS_REQUIRE(seg % 4 == 0, "%s: seg must be a multiple of 4, got %d", who, seg);
  SVS_REQUIRE(tile_hop % 4 == 0, "%s: tile_hop must be a multiple of 4, got %d", who, tile_hop);
  SVS_REQUIRE(seg % tile_hop == 0, "%s: tile_hop must divide seg, got seg=%d tile_hop=%d", who, seg, tile_hop);
  SVS_REQUIRE(seg / tile_hop <= OVERLAP_MAX_RATIO, "%s: seg / tile_hop must be at most %d, got %d / %d", who, OVERLAP_MAX_RATIO, seg, tile_hop);
  SVS_REQUIRE((long)n_tiles * seg < (1L << 31), "%s: n_tiles * seg must stay below 2^31 (a frame index is an int), got %d * %d", who, n_tiles, seg);
  return SVS_OK;
}
static int overlap_check_stride(const char* who, const char* name, long stride, int n_tiles, int rows, int seg) {
  SVS_REQUIRE(stride >= (long)n_tiles * rows * seg, "%s: %s must be at least n_tiles * rows * seg = %ld, got %ld", who, name,
              (long)n_tiles * rows * seg, stride);
  SVS_REQUIRE(stride % 4 == 0, "%s: %s must be a multiple of 4 floats, got %ld", who, name, stride);
  return SVS_OK;
}

extern "C" int svs_overlap_count(int n_tiles, int seg, int tile_hop) {
  SVS_REQUIRE(n_tiles > 0 && seg > 0 && tile_hop > 0, "svs_overlap_count: all sizes must be positive, got n_tiles=%d seg=%d tile_hop=%d", n_tiles, seg, tile_hop);
  SVS_REQUIRE(seg % tile_hop == 0, "svs_overlap_count: tile_hop must divide seg, got seg=%d tile_hop=%d", seg, tile_hop);
  SVS_REQUIRE(((long)n_tiles - 1) * (seg / tile_hop) + 1 < (1L << 31), "svs_overlap_count: the count does not fit an int");
  return (n_tiles - 1) * (seg / tile_hop) + 1;
}

// ------------------------------------------------------------------------------------------------
// cut: overlapped tile j <- frames [j * tile_hop, j * tile_hop + seg) of the disjoint tiles
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void overlap_tiles_kernel(const float* __restrict__ tiles, long chan_stride, int n_ov, int rows, int seg,
                                                            int tile_hop, long total, float* __restrict__ out) {
  const int q4 = seg / 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int q = (int)(i % q4);
    const long row = i / q4;                         // (c * n_ov + j) * rows + r: the output is contiguous in exactly this order
    const int r = (int)(row % rows);
    const long cj = row / rows;
    const int j = (int)(cj % n_ov);
    const long c = cj / n_ov;
    const int t = j * tile_hop + 4 * q;              // < n_tiles * seg: the last overlapped tile IS the last disjoint tile
    const f32x4 v = *(const f32x4*)(tiles + c * chan_stride + ((long)(t / seg) * rows + r) * seg + t % seg);
    *(f32x4*)(out + i * 4) = v;
  }
}

extern "C" int svs_overlap_tiles(const float* tiles, int64_t chan_stride, int channels, int n_tiles, int rows, int seg, int tile_hop,
                                 float* out, hipStream_t stream) {
  int rc = overlap_check("svs_overlap_tiles", channels, n_tiles, rows, seg, tile_hop);
  if (rc) return rc;
  rc = overlap_check_stride("svs_overlap_tiles", "chan_stride", (long)chan_stride, n_tiles, rows, seg);
  if (rc) return rc;
  SVS_REQUIRE(tiles && out, "svs_overlap_tiles: null pointer");
  SVS_REQUIRE(svs_aligned16(tiles) && svs_aligned16(out), "svs_overlap_tiles: pointers must be 16-byte aligned");
  const int n_ov = (n_tiles - 1) * (seg / tile_hop) + 1;
  const long total = (long)channels * n_ov * rows * (seg / 4);
  hipLaunchKernelGGL(overlap_tiles_kernel, dim3(overlap_grid(total)), dim3(256), 0, stream, tiles, (long)chan_stride, n_ov, rows, seg,
                     tile_hop, total, out);
  SVS_CHECK_LAUNCH("overlap_tiles");
  return SVS_OK;
}

// ------------------------------------------------------------------------------------------------
// the cross-fade window, one device copy per (device, seg)
// ------------------------------------------------------------------------------------------------
namespace {
std::mutex g_mu;
std::map<std::pair<int, int>, const float*> g_window;
}

static int overlap_window(int seg, hipStream_t stream, const float** out) {
  int dev = 0;
  SVS_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> guard(g_mu);
  auto it = g_window.find({dev, seg});
  if (it == g_window.end()) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    SVS_HIP(hipStreamIsCapturing(stream, &cap));
    if (cap != hipStreamCaptureStatusNone) {
      svs_set_error("svs_overlap_blend: the first blend of a process at seg = %d must run outside a stream capture (it uploads the window)", seg);
      return SVS_ERR_INVALID;
    }
    std::vector<float> w((size_t)seg);
    for (int i = 0; i < seg; ++i) { const double s = std::sin(M_PI * ((double)i + 0.5) / (double)seg); w[i] = (float)(s * s); }
    void* p = nullptr;
    SVS_HIP(hipMalloc(&p, (size_t)seg * sizeof(float)));
    const hipError_t e = hipMemcpy(p, w.data(), (size_t)seg * sizeof(float), hipMemcpyHostToDevice);   // complete on return
    if (e != hipSuccess) {
      (void)hipFree(p);
      svs_set_error("svs_overlap_blend: uploading the window failed: %s", hipGetErrorString(e));
      return (int)e;
    }
    it = g_window.emplace(std::make_pair(dev, seg), (const float*)p).first;
  }
  *out = it->second;
  return SVS_OK;
}

// ------------------------------------------------------------------------------------------------
// blend: b(t) = sum_j w[t - j*hop] * masks[j][t - j*hop] / sum_j w[t - j*hop], written in the disjoint-tile layout
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void overlap_blend_kernel(const float* __restrict__ masks, const float* __restrict__ win, int n_tiles,
                                                            int n_ov, int rows, int seg, int tile_hop, const float* __restrict__ mix,
                                                            long mix_chan_stride, int invert, float* __restrict__ out,
                                                            long out_chan_stride, long total) {
  const int q4 = seg / 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int q = (int)(i % q4);
    const long row = i / q4;                         // (c * n_tiles + tile) * rows + r
    const int r = (int)(row % rows);
    const long ct = row / rows;
    const int tile = (int)(ct % n_tiles);
    const long c = ct / n_tiles;
    const int t = tile * seg + 4 * q;
    // the tiles j with 0 <= t - j * hop < seg, the same for t .. t + 3
    const int j_lo = t < seg ? 0 : (t - seg) / tile_hop + 1;
    const int j_hi = min(t / tile_hop, n_ov - 1);
    const float* m0 = masks + ((c * n_ov) * rows + r) * seg + t;          // + j * (rows * seg - tile_hop): tile j, frame t - j * hop
    const long step = (long)rows * seg - tile_hop;
    f32x4 b;
    if (j_lo == j_hi) {
      b = *(const f32x4*)(m0 + j_lo * step);         // one tile covers these frames: its values, untouched
    } else {
      f32x4 num = {0.f, 0.f, 0.f, 0.f}, den = {0.f, 0.f, 0.f, 0.f};
      for (int j = j_lo; j <= j_hi; ++j) {
        const f32x4 m = *(const f32x4*)(m0 + j * step);
        const f32x4 w = *(const f32x4*)(win + (t - j * tile_hop));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          num[k] = fmaf(w[k], m[k], num[k]);
          den[k] += w[k];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) b[k] = num[k] / den[k];
    }
    const long off = ((long)tile * rows + r) * seg + 4 * q;
    if (invert) {
#pragma unroll
      for (int k = 0; k < 4; ++k) b[k] = 1.f - b[k];
    }
    if (mix) {
      const f32x4 x = *(const f32x4*)(mix + c * mix_chan_stride + off);
#pragma unroll
      for (int k = 0; k < 4; ++k) b[k] = x[k] * b[k];
    }
    *(f32x4*)(out + c * out_chan_stride + off) = b;
  }
}

extern "C" int svs_overlap_blend(const float* masks, int channels, int n_tiles, int rows, int seg, int tile_hop, const float* mix,
                                 int64_t mix_chan_stride, int invert, float* out, int64_t out_chan_stride, hipStream_t stream) {
  int rc = overlap_check("svs_overlap_blend", channels, n_tiles, rows, seg, tile_hop);
  if (rc) return rc;
  rc = overlap_check_stride("svs_overlap_blend", "out_chan_stride", (long)out_chan_stride, n_tiles, rows, seg);
  if (rc) return rc;
  if (mix) {
    rc = overlap_check_stride("svs_overlap_blend", "mix_chan_stride", (long)mix_chan_stride, n_tiles, rows, seg);
    if (rc) return rc;
  }
  SVS_REQUIRE(masks && out, "svs_overlap_blend: null pointer");
  SVS_REQUIRE(svs_aligned16(masks) && svs_aligned16(out) && svs_aligned16(mix), "svs_overlap_blend: pointers must be 16-byte aligned");
  const int n_ov = (n_tiles - 1) * (seg / tile_hop) + 1;
  const float* win = nullptr;
  if (n_ov > n_tiles) {                                               // (one tile per frame, tile_hop == seg or n_tiles == 1: a copy, no window)
    rc = overlap_window(seg, stream, &win);
    if (rc) return rc;
  }
  const long total = (long)channels * n_tiles * rows * (seg / 4);
  hipLaunchKernelGGL(overlap_blend_kernel, dim3(overlap_grid(total)), dim3(256), 0, stream, masks, win, n_tiles, n_ov, rows, seg, tile_hop,
                     mix, (long)mix_chan_stride, invert, out, (long)out_chan_stride, total);
  SVS_CHECK_LAUNCH("overlap_blend");
  return SVS_OK;
}
