// Multichannel Wiener filter with EM updates of a local Gaussian model (Duong, Vincent and Gribonval; the post-filter of
// Open-Unmix / norbert.wiener), the step between the mask and the inverse transform.  The reference writes
// `mag * mask * phase of the mixture` (inference.py:100-107, data.py:159) and has no such step.
//
// J = 2 sources (0 vocal, 1 accompaniment), C = 1 or 2 channels, bins (t, f) with f over the tiles' rows (the DC bin is absent).
// With x_c = scale_c * mag_c * P_c the mixture, one update is
//     v_j[t,f] = mean_c |y_jc|^2
//     R_j[f]   = sum_t y_j y_j^H / (eps + sum_t v_j[t,f])          C x C Hermitian, real frames only
//     Cxx[t,f] = sum_j v_j R_j + reg * I
//     y_j      = v_j R_j Cxx^-1 x
// starting from y_0c = scale_c mag_c mask_c P_c, y_1c = scale_c mag_c (1 - mask_c) P_c.  No y is stored between passes: a pass
// reads (v, R) of the pass before and forms W(v, R) x on the fly.
//
// Arithmetic is fp64 throughout (for identical channels Cxx = s 11^T + reg I, whose adjugate and determinant cancel: fp32 is off by
// half the peak there); what is stored per bin (mag, mask, v, the stems' magnitudes and phasors) is fp32.
//
// Shape of both kernels: one block = 64 rows x 32 frames of one tile, 256 threads.  The time-minor tiles (mag, mask, v) are moved
// with 16-byte global accesses through an LDS tile of 33-float rows; in the compute phase lane l of every wave owns row l, wave w
// the frames 8w .. 8w + 7, so the frame-major phasors are 64 lanes x 8 B contiguous, the LDS is read transposed without bank
// conflicts (33 l + t mod 32 is a permutation of a 32-lane half) and the sums over t are per-lane fp64 registers.  The four waves'
// sums are added in wave order through LDS, the per-block partials go to the workspace, and a second kernel adds them in a fixed
// order (ascending within 16 consecutive runs of chunks, then the runs in ascending order): no atomics, bitwise reproducible.
#include "internal.h"

#define WN_ROWS 64
#define WN_FRAMES 32
#define WN_LD 33
#define WN_TILE (WN_ROWS * WN_LD)            // floats of one staged array
#define WN_THREADS 256
#define WN_PER_WAVE (WN_FRAMES / 4)

struct WnGeom {
  int seg, rows, frames, channels;
  int cpt;                                   // chunks of WN_FRAMES frames per tile (the last may be narrower)
};

struct WnChunk {
  long row0;                                 // tile * rows + first row of the block: the row index of the tile addressing
  long T0;                                   // first frame of the chunk in the signal
  int t0, w4, valid;                         // first frame within the tile, 16-byte quads per row, real (unpadded) frames
};

__device__ __forceinline__ WnChunk wn_chunk(const WnGeom& g) {
  WnChunk c;
  const int tile = (int)(blockIdx.x / g.cpt);
  c.t0 = (int)(blockIdx.x % g.cpt) * WN_FRAMES;
  const int width = min(WN_FRAMES, g.seg - c.t0);
  c.w4 = width / 4;
  c.T0 = (long)tile * g.seg + c.t0;
  const long left = (long)g.frames - c.T0;
  c.valid = left <= 0 ? 0 : (left < width ? (int)left : width);
  c.row0 = (long)tile * g.rows + (long)blockIdx.y * WN_ROWS;
  return c;
}

// 64 rows x w4 quads of one array: global (16-byte loads) -> LDS rows of WN_LD floats
__device__ __forceinline__ void wn_stage_in(float* lds, const float* src, const WnChunk& c, int seg) {
#pragma unroll
  for (int i = 0; i < WN_ROWS * (WN_FRAMES / 4) / WN_THREADS; ++i) {
    const int idx = threadIdx.x + i * WN_THREADS, row = idx >> 3, q = idx & 7;
    if (q < c.w4) {
      const f32x4 v = *(const f32x4*)(src + (c.row0 + row) * seg + c.t0 + 4 * q);
      float* d = lds + row * WN_LD + 4 * q;
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
  }
}
__device__ __forceinline__ void wn_stage_out(const float* lds, float* dst, const WnChunk& c, int seg) {
#pragma unroll
  for (int i = 0; i < WN_ROWS * (WN_FRAMES / 4) / WN_THREADS; ++i) {
    const int idx = threadIdx.x + i * WN_THREADS, row = idx >> 3, q = idx & 7;
    if (q < c.w4) {
      const float* s = lds + row * WN_LD + 4 * q;
      const f32x4 v = {s[0], s[1], s[2], s[3]};
      *(f32x4*)(dst + (c.row0 + row) * seg + c.t0 + 4 * q) = v;
    }
  }
}

// y_j = v_j R_j Cxx^-1 x for both sources.  R[j] = (R00, R11, Re R01, Im R01).  Closed-form 2 x 2 solve: with Cxx = [[A, c], [c*, B]],
// z = Cxx^-1 x by elimination, z_1 = (x_1 - c* x_0 / A) / (B - |c|^2 / A), z_0 = (x_0 - c z_1) / A, then y_j = v_j R_j z.  Elimination is
// backward stable for a Hermitian positive definite Cxx; adjugate over determinant is not (for a panned point source Cxx = s p p^H +
// reg I, and A B - |c|^2 and adj(Cxx) x both cancel to reg / s of their terms).  One channel: the power-ratio filter.
template <int C>
__device__ __forceinline__ void wn_posterior(const double (&v)[2], const double (&R)[2][4], const double (&xr)[C], const double (&xi)[C],
                                             double reg, double (&yr)[2][C], double (&yi)[2][C]) {
  if constexpr (C == 1) {
    const double inv = 1.0 / (v[0] * R[0][0] + v[1] * R[1][0] + reg);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const double g = v[j] * R[j][0] * inv;
      yr[j][0] = g * xr[0];
      yi[j][0] = g * xi[0];
    }
  } else {
    const double A = v[0] * R[0][0] + v[1] * R[1][0] + reg, B = v[0] * R[0][1] + v[1] * R[1][1] + reg;
    const double cr = v[0] * R[0][2] + v[1] * R[1][2], ci = v[0] * R[0][3] + v[1] * R[1][3];
    const double iA = 1.0 / A, id = 1.0 / (B - (cr * cr + ci * ci) * iA);
    const double ur = xr[0] * iA, ui = xi[0] * iA;
    const double z1r = (xr[1] - (cr * ur + ci * ui)) * id, z1i = (xi[1] - (cr * ui - ci * ur)) * id;
    const double z0r = (xr[0] - (cr * z1r - ci * z1i)) * iA, z0i = (xi[0] - (cr * z1i + ci * z1r)) * iA;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const double a = R[j][0], b = R[j][1], pr = R[j][2], pi = R[j][3];
      yr[j][0] = v[j] * (a * z0r + (pr * z1r - pi * z1i));
      yi[j][0] = v[j] * (a * z0i + (pr * z1i + pi * z1r));
      yr[j][1] = v[j] * ((pr * z0r + pi * z0i) + b * z1r);
      yi[j][1] = v[j] * ((pr * z0i - pi * z0r) + b * z1i);
    }
  }
}

struct WnModelArgs {
  WnGeom g;
  const float* mag; long chan_stride;
  const float* mask;
  const float* phase;                        // (C, frames, rows + 1, 2)
  const float* scale;
  const float* v_prev; long v_prev_stride;
  const double* R_prev;
  double reg;
  float* v; long v_stride;
  double* partial;                           // [chunks][NK][rows], NK = 2 (one channel) or 8
};

// LDS arrays.  PREV: [v_prev0, v_prev1, mag_0, (mag_1)], else [mag_0, (mag_1), mask_0, (mask_1)]; v_0 and v_1 replace arrays 0 and 1
// cell by cell (a cell is read and rewritten by the one lane that owns it).
template <int C, bool PREV>
__global__ __launch_bounds__(WN_THREADS) void wiener_model_kernel(WnModelArgs a) {
  constexpr int NIN = PREV ? 2 + C : 2 * C;
  constexpr int KS = C == 2 ? 4 : 1, NK = 2 * KS;
  static_assert(NIN * WN_TILE * sizeof(float) >= 4 * NK * 64 * sizeof(double), "the partial sums reuse the staged arrays");
  __shared__ double smem_d[NIN * WN_TILE / 2];
  float* lds = (float*)smem_d;
  const WnGeom g = a.g;
  const WnChunk c = wn_chunk(g);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.y * WN_ROWS + lane;

  if constexpr (PREV) {
    wn_stage_in(lds, a.v_prev, c, g.seg);
    wn_stage_in(lds + WN_TILE, a.v_prev + a.v_prev_stride, c, g.seg);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) wn_stage_in(lds + (2 + ch) * WN_TILE, a.mag + ch * a.chan_stride, c, g.seg);
  } else {
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      wn_stage_in(lds + ch * WN_TILE, a.mag + ch * a.chan_stride, c, g.seg);
      wn_stage_in(lds + (C + ch) * WN_TILE, a.mask + ch * a.chan_stride, c, g.seg);
    }
  }
  double R[2][4] = {};
  if constexpr (PREV) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) R[j][k] = a.R_prev[((long)j * g.rows + f) * 4 + k];
  }
  double sc[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) sc[ch] = (double)a.scale[ch];
  __syncthreads();

  double S[2][KS] = {};
  const long nbin = g.rows + 1;
#pragma unroll 2
  for (int i = 0; i < WN_PER_WAVE; ++i) {
    const int t = wave * WN_PER_WAVE + i;
    float* cell = lds + lane * WN_LD + t;
    if (t < c.valid) {
      double yr[2][C], yi[2][C];
      double pr[C], pi[C], m[C];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const float2 p = *(const float2*)(a.phase + (((long)ch * g.frames + c.T0 + t) * nbin + f + 1) * 2);
        pr[ch] = (double)p.x;
        pi[ch] = (double)p.y;
        m[ch] = sc[ch] * (double)cell[(PREV ? 2 + ch : ch) * WN_TILE];
      }
      if constexpr (PREV) {
        const double v[2] = {(double)cell[0], (double)cell[WN_TILE]};
        double xr[C], xi[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          xr[ch] = m[ch] * pr[ch];
          xi[ch] = m[ch] * pi[ch];
        }
        wn_posterior<C>(v, R, xr, xi, a.reg, yr, yi);
      } else {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          const double k = (double)cell[(C + ch) * WN_TILE];
          const double m0 = m[ch] * k, m1 = m[ch] * (1.0 - k);
          yr[0][ch] = m0 * pr[ch]; yi[0][ch] = m0 * pi[ch];
          yr[1][ch] = m1 * pr[ch]; yi[1][ch] = m1 * pi[ch];
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const double e0 = yr[j][0] * yr[j][0] + yi[j][0] * yi[j][0];
        S[j][0] += e0;
        if constexpr (C == 2) {
          const double e1 = yr[j][1] * yr[j][1] + yi[j][1] * yi[j][1];
          S[j][1] += e1;
          S[j][2] += yr[j][0] * yr[j][1] + yi[j][0] * yi[j][1];      // y_0 conj(y_1)
          S[j][3] += yi[j][0] * yr[j][1] - yr[j][0] * yi[j][1];
          cell[j * WN_TILE] = (float)(0.5 * (e0 + e1));
        } else {
          cell[j * WN_TILE] = (float)e0;
        }
      }
    } else if (t < 4 * c.w4) {                 // tile padding past the last real frame
      cell[0] = 0.f;
      cell[WN_TILE] = 0.f;
    }
  }
  __syncthreads();
  wn_stage_out(lds, a.v, c, g.seg);
  wn_stage_out(lds + WN_TILE, a.v + a.v_stride, c, g.seg);
  __syncthreads();
  // the four waves' sums, added in wave order
  double* red = smem_d;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int k = 0; k < KS; ++k) red[(wave * NK + j * KS + k) * 64 + lane] = S[j][k];
  __syncthreads();
  for (int idx = threadIdx.x; idx < NK * 64; idx += WN_THREADS) {
    const int k = idx >> 6, l = idx & 63;
    const double s = ((red[(0 * NK + k) * 64 + l] + red[(1 * NK + k) * 64 + l]) + red[(2 * NK + k) * 64 + l]) + red[(3 * NK + k) * 64 + l];
    a.partial[((long)blockIdx.x * NK + k) * g.rows + blockIdx.y * WN_ROWS + l] = s;
  }
}

// R_j[f] = the sum of the partial sums over the chunks / (eps + sum_t v_j);  sum_t v_j = mean_c of the diagonal sums.  One block = 64
// frequencies of one source; wave s adds run s of the chunks (WN_RED_RUNS consecutive runs of equal length) in ascending order, every
// load independent of the sum before it, and wave 0 adds the runs in ascending order: a fixed order for a given geometry.  (One thread
// walking all chunks of a frequency is the same sum but a chain of `chunks` dependent latencies: 0.35 ms at 864 chunks.)
#define WN_RED_RUNS 16
template <int C>
__global__ __launch_bounds__(64 * WN_RED_RUNS) void wiener_reduce_kernel(const double* __restrict__ partial, int chunks, int rows, double eps,
                                                                         double* __restrict__ R) {
  constexpr int KS = C == 2 ? 4 : 1, NK = 2 * KS;
  __shared__ double red[WN_RED_RUNS][KS][64];
  const int lane = threadIdx.x & 63, run = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + lane, j = blockIdx.y;
  const int per = (chunks + WN_RED_RUNS - 1) / WN_RED_RUNS;
  const int c0 = run * per, c1 = min(chunks, c0 + per);
  double S[KS] = {};
#pragma unroll 4
  for (int ch = c0; ch < c1; ++ch)
#pragma unroll
    for (int k = 0; k < KS; ++k) S[k] += partial[((long)ch * NK + j * KS + k) * rows + f];
#pragma unroll
  for (int k = 0; k < KS; ++k) red[run][k][lane] = S[k];
  __syncthreads();
  if (run != 0) return;
  double T[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    double t = red[0][k][lane];
    for (int q = 1; q < WN_RED_RUNS; ++q) t += red[q][k][lane];
    T[k] = t;
  }
  const double inv = 1.0 / (eps + (C == 2 ? 0.5 * (T[0] + T[1]) : T[0]));
#pragma unroll
  for (int k = 0; k < 4; ++k) R[((long)j * rows + f) * 4 + k] = T[k] * inv;
}

struct WnStemsArgs {
  WnGeom g;
  const float* mag; long chan_stride;
  const float* phase;
  const float* scale;
  const float* v; long v_stride;
  const double* R;
  double reg;
  int stem;                                  // 0, 1: that stem alone, written at the base pointers; 2: stem j at base + j * stem stride
  float* out_mag; long out_chan_stride, out_mag_stem_stride;
  float* out_phase; long out_phase_stem_stride;
};

// LDS arrays [v_0, v_1, mag_0, (mag_1)]; |y_jc| replaces array j * C + c cell by cell
template <int C>
__global__ __launch_bounds__(WN_THREADS) void wiener_stems_kernel(WnStemsArgs a) {
  __shared__ float lds[(2 + C) * WN_TILE];
  const WnGeom g = a.g;
  const WnChunk c = wn_chunk(g);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.y * WN_ROWS + lane;
  wn_stage_in(lds, a.v, c, g.seg);
  wn_stage_in(lds + WN_TILE, a.v + a.v_stride, c, g.seg);
#pragma unroll
  for (int ch = 0; ch < C; ++ch) wn_stage_in(lds + (2 + ch) * WN_TILE, a.mag + ch * a.chan_stride, c, g.seg);
  double R[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) R[j][k] = a.R[((long)j * g.rows + f) * 4 + k];
  double sc[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) sc[ch] = (double)a.scale[ch];
  __syncthreads();

  const long nbin = g.rows + 1;
#pragma unroll 2
  for (int i = 0; i < WN_PER_WAVE; ++i) {
    const int t = wave * WN_PER_WAVE + i;
    float* cell = lds + lane * WN_LD + t;
    if (t < c.valid) {
      const double v[2] = {(double)cell[0], (double)cell[WN_TILE]};
      double xr[C], xi[C], yr[2][C], yi[2][C];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const float2 p = *(const float2*)(a.phase + (((long)ch * g.frames + c.T0 + t) * nbin + f + 1) * 2);
        const double m = sc[ch] * (double)cell[(2 + ch) * WN_TILE];
        xr[ch] = m * (double)p.x;
        xi[ch] = m * (double)p.y;
      }
      wn_posterior<C>(v, R, xr, xi, a.reg, yr, yi);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (a.stem != 2 && a.stem != j) continue;
        float* ph = a.out_phase + (a.stem == 2 ? j * a.out_phase_stem_stride : 0);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          const double n = sqrt(yr[j][ch] * yr[j][ch] + yi[j][ch] * yi[j][ch]);
          const float nf = (float)n;
          float2 p = make_float2(1.f, 0.f);                                  // phasor(0) = 1 + 0i (phase_mode 1), also where |y| rounds to 0
          if (nf != 0.f) {
            const double inv = 1.0 / n;
            p.x = (float)(yr[j][ch] * inv);
            p.y = (float)(yi[j][ch] * inv);
          }
          cell[(j * C + ch) * WN_TILE] = nf;
          float* row = ph + (((long)ch * g.frames + c.T0 + t) * nbin) * 2;
          *(float2*)(row + (f + 1) * 2) = p;
          if (f == 0) *(float2*)row = make_float2(1.f, 0.f);             // the DC bin, absent from the tiles: zero in every stem
        }
      }
    } else if (t < 4 * c.w4) {
#pragma unroll
      for (int k = 0; k < 2 * C; ++k) cell[k * WN_TILE] = 0.f;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (a.stem != 2 && a.stem != j) continue;
    float* om = a.out_mag + (a.stem == 2 ? j * a.out_mag_stem_stride : 0);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) wn_stage_out(lds + (j * C + ch) * WN_TILE, om + ch * a.out_chan_stride, c, g.seg);
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static const long WN_2GIB = 1L << 31;

static int wn_check_geom(const char* who, int channels, int rows, int seg, int frames, WnGeom* g, long* tile_floats, long* chunks) {
  SVS_REQUIRE(channels == 1 || channels == 2, "%s: channels must be 1 or 2, got %d", who, channels);
  SVS_REQUIRE(rows > 0 && rows % WN_ROWS == 0, "%s: rows must be a positive multiple of %d, got %d", who, WN_ROWS, rows);
  SVS_REQUIRE(seg > 0 && seg % 4 == 0, "%s: seg must be a positive multiple of 4, got %d", who, seg);
  SVS_REQUIRE(frames >= 1, "%s: frames must be at least 1, got %d", who, frames);
  const long n_tiles = ((long)frames + seg - 1) / seg;
  g->seg = seg; g->rows = rows; g->frames = frames; g->channels = channels;
  g->cpt = (seg + WN_FRAMES - 1) / WN_FRAMES;
  *tile_floats = n_tiles * rows * seg;
  *chunks = n_tiles * g->cpt;
  return SVS_OK;
}
// a view of `count` pieces of `one` floats, `stride` floats apart
static int wn_check_view(const char* who, const char* name, long stride, long one, int count, const char* piece) {
  SVS_REQUIRE(stride >= one, "%s: %s must be at least one %s's size = %ld floats, got %ld", who, name, piece, one, stride);
  SVS_REQUIRE(stride % 4 == 0, "%s: %s must be a multiple of 4 floats (16-byte accesses), got %ld", who, name, stride);
  SVS_REQUIRE(((long)(count - 1) * stride + one) * 4 < WN_2GIB, "%s: the view addressed through %s must stay below 2 GiB, got %ld bytes", who,
              name, ((long)(count - 1) * stride + one) * 4);
  return SVS_OK;
}
static inline bool wn_aligned8(const void* p) { return (((uintptr_t)p) & 7u) == 0; }

extern "C" size_t svs_wiener_workspace_bytes(int channels, int rows, int seg, int frames) {
  WnGeom g;
  long tile_floats, chunks;
  if (wn_check_geom("svs_wiener_workspace_bytes", channels, rows, seg, frames, &g, &tile_floats, &chunks)) return 0;
  return (size_t)chunks * (channels == 2 ? 8 : 2) * rows * sizeof(double);
}

extern "C" int svs_wiener_model(const float* mag, int64_t chan_stride, int seg, int rows, const float* mask, const float* phase,
                                const float* scale, int channels, int frames, const float* v_prev, int64_t v_prev_stem_stride,
                                const double* R_prev, double eps, double reg, float* v, int64_t v_stem_stride, double* R, void* ws,
                                size_t ws_bytes, hipStream_t stream) {
  const char* who = "svs_wiener_model";
  WnGeom g;
  long one, chunks;
  int rc = wn_check_geom(who, channels, rows, seg, frames, &g, &one, &chunks);
  if (rc) return rc;
  if ((rc = wn_check_view(who, "chan_stride", (long)chan_stride, one, channels, "channel"))) return rc;
  if ((rc = wn_check_view(who, "v_stem_stride", (long)v_stem_stride, one, 2, "stem"))) return rc;
  SVS_REQUIRE((v_prev == nullptr) == (R_prev == nullptr), "%s: v_prev and R_prev are given together (a previous model) or not at all", who);
  if (v_prev && (rc = wn_check_view(who, "v_prev_stem_stride", (long)v_prev_stem_stride, one, 2, "stem"))) return rc;
  SVS_REQUIRE(v_prev || mask, "%s: the first update needs the mask (no previous model was given)", who);
  SVS_REQUIRE(mag && phase && scale && v && R && ws, "%s: null pointer", who);
  SVS_REQUIRE(svs_aligned16(mag) && svs_aligned16(mask) && svs_aligned16(v) && svs_aligned16(v_prev),
              "%s: mag, mask, v and v_prev must be 16-byte aligned", who);
  SVS_REQUIRE(wn_aligned8(phase) && wn_aligned8(R) && wn_aligned8(R_prev) && wn_aligned8(ws),
              "%s: phase, R, R_prev and the workspace must be 8-byte aligned", who);
  SVS_REQUIRE((long)channels * frames * (rows + 1) * 8 < WN_2GIB, "%s: the phasors must stay below 2 GiB, got %ld bytes", who,
              (long)channels * frames * (rows + 1) * 8);
  SVS_REQUIRE(eps >= 0.0 && reg > 0.0, "%s: eps must not be negative and reg must be positive, got eps=%g reg=%g", who, eps, reg);
  const size_t need = (size_t)chunks * (channels == 2 ? 8 : 2) * rows * sizeof(double);
  SVS_REQUIRE(ws_bytes >= need, "%s: the workspace needs %zu bytes (svs_wiener_workspace_bytes), got %zu", who, need, ws_bytes);

  WnModelArgs a;
  a.g = g; a.mag = mag; a.chan_stride = (long)chan_stride; a.mask = mask; a.phase = phase; a.scale = scale;
  a.v_prev = v_prev; a.v_prev_stride = (long)v_prev_stem_stride; a.R_prev = R_prev; a.reg = reg;
  a.v = v; a.v_stride = (long)v_stem_stride; a.partial = (double*)ws;
  const dim3 grid((unsigned)chunks, (unsigned)(rows / WN_ROWS));
  if (channels == 2) {
    if (v_prev) hipLaunchKernelGGL((wiener_model_kernel<2, true>), grid, dim3(WN_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((wiener_model_kernel<2, false>), grid, dim3(WN_THREADS), 0, stream, a);
  } else {
    if (v_prev) hipLaunchKernelGGL((wiener_model_kernel<1, true>), grid, dim3(WN_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((wiener_model_kernel<1, false>), grid, dim3(WN_THREADS), 0, stream, a);
  }
  SVS_CHECK_LAUNCH("wiener_model");
  const dim3 rgrid((unsigned)(rows / 64), 2), rblock(64 * WN_RED_RUNS);
  if (channels == 2) hipLaunchKernelGGL((wiener_reduce_kernel<2>), rgrid, rblock, 0, stream, (const double*)ws, (int)chunks, rows, eps, R);
  else hipLaunchKernelGGL((wiener_reduce_kernel<1>), rgrid, rblock, 0, stream, (const double*)ws, (int)chunks, rows, eps, R);
  SVS_CHECK_LAUNCH("wiener_reduce");
  return SVS_OK;
}

extern "C" int svs_wiener_stems(const float* mag, int64_t chan_stride, int seg, int rows, const float* phase, const float* scale,
                                int channels, int frames, const float* v, int64_t v_stem_stride, const double* R, double reg, int stem,
                                float* out_mag, int64_t out_chan_stride, int64_t out_mag_stem_stride, float* out_phase,
                                int64_t out_phase_stem_stride, hipStream_t stream) {
  const char* who = "svs_wiener_stems";
  WnGeom g;
  long one, chunks;
  int rc = wn_check_geom(who, channels, rows, seg, frames, &g, &one, &chunks);
  if (rc) return rc;
  SVS_REQUIRE(stem >= 0 && stem <= 2, "%s: stem must be 0 (vocal), 1 (accompaniment) or 2 (both), got %d", who, stem);
  if ((rc = wn_check_view(who, "chan_stride", (long)chan_stride, one, channels, "channel"))) return rc;
  if ((rc = wn_check_view(who, "v_stem_stride", (long)v_stem_stride, one, 2, "stem"))) return rc;
  if ((rc = wn_check_view(who, "out_chan_stride", (long)out_chan_stride, one, channels, "channel"))) return rc;
  const long phase_one = (long)channels * frames * (rows + 1) * 2;
  SVS_REQUIRE(phase_one * 4 < WN_2GIB, "%s: the phasors must stay below 2 GiB, got %ld bytes", who, phase_one * 4);
  if (stem == 2) {
    const long mag_one = (long)(channels - 1) * out_chan_stride + one;
    if ((rc = wn_check_view(who, "out_mag_stem_stride", (long)out_mag_stem_stride, mag_one, 2, "stem"))) return rc;
    SVS_REQUIRE(out_phase_stem_stride >= phase_one, "%s: out_phase_stem_stride must be at least one stem's size = %ld floats, got %ld", who,
                phase_one, (long)out_phase_stem_stride);
    SVS_REQUIRE(out_phase_stem_stride % 2 == 0, "%s: out_phase_stem_stride must be even (8-byte accesses), got %ld", who,
                (long)out_phase_stem_stride);
    SVS_REQUIRE((out_phase_stem_stride + phase_one) * 4 < WN_2GIB, "%s: the view addressed through out_phase_stem_stride must stay below 2 GiB", who);
  }
  SVS_REQUIRE(mag && phase && scale && v && R && out_mag && out_phase, "%s: null pointer", who);
  SVS_REQUIRE(svs_aligned16(mag) && svs_aligned16(v) && svs_aligned16(out_mag), "%s: mag, v and out_mag must be 16-byte aligned", who);
  SVS_REQUIRE(wn_aligned8(phase) && wn_aligned8(R) && wn_aligned8(out_phase), "%s: phase, R and out_phase must be 8-byte aligned", who);
  SVS_REQUIRE(reg > 0.0, "%s: reg must be positive, got %g", who, reg);

  WnStemsArgs a;
  a.g = g; a.mag = mag; a.chan_stride = (long)chan_stride; a.phase = phase; a.scale = scale; a.v = v; a.v_stride = (long)v_stem_stride;
  a.R = R; a.reg = reg; a.stem = stem; a.out_mag = out_mag; a.out_chan_stride = (long)out_chan_stride;
  a.out_mag_stem_stride = (long)out_mag_stem_stride; a.out_phase = out_phase; a.out_phase_stem_stride = (long)out_phase_stem_stride;
  const dim3 grid((unsigned)chunks, (unsigned)(rows / WN_ROWS));
  if (channels == 2) hipLaunchKernelGGL((wiener_stems_kernel<2>), grid, dim3(WN_THREADS), 0, stream, a);
  else hipLaunchKernelGGL((wiener_stems_kernel<1>), grid, dim3(WN_THREADS), 0, stream, a);
  SVS_CHECK_LAUNCH("wiener_stems");
  return SVS_OK;
}
