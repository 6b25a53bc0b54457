// Smoothing the YIN pitch track on the device (include/svs_hip.h; the definition is svs_unet_pytorch_amd/f0.py):
// K = 7 period candidates per frame -- the deepest dips of d' -- and an exact Viterbi decode over them plus one unvoiced state.
// The reference has no pitch estimator of any kind.
//
// Candidates.  f0_frame_dips runs on one row of d' (LDS or memory) by one wave: seven rounds of a wave minimum over (d', tau) among the
// dips that lie after the previous round's winner in that order, so round r finds the r-th smallest dip and equal depths go to the
// smaller tau.  Lane k < 7 then ranks winner k by its tau among the winners and writes slot `rank` (tau, the parabolic f0 of the pick,
// ap = d'(tau)); lanes count..6 write the empty slots.  svs_f0_dips does this on rows in memory; svs_f0_candidates is svs_f0_track's
// kernel (f0_frame.h: the same staging, d' and pick, hence the same bits) with the dips taken from the wave's LDS row before it is left.
//
// Decode.  All costs are int64 in units of 1/4096, so the (min,+) product of the frames' 8x8 matrices M_t(i,j) = A_t(i,j) + obs_t(j) is
// associative without rounding, and a row of n_frames frames is cut into chunks of `chunk` frames (A_0 = 0 and an all-zero vector in
// front of frame 0 make frame 0 a frame like any other):
//   (a) vit_product_kernel  one wave per chunk: the product of the chunk's matrices, lane 8i + j holding entry (i, j); the row operand
//                           P(i, 0..7) comes from a double-buffered 512-byte LDS copy of P, the column operand from the staged frame
//   (b) vit_scan_kernel     one wave per row: the 8-vector delta carried across the chunk products (n_frames / chunk steps, the products
//                           fetched eight ahead); writes every chunk's entry vector, the row's cost and its end state
//   (c) vit_rerun_kernel    one wave per chunk: the chunk's frames again from its entry vector, lane 8k + j holding delta(k) + A(k, j),
//                           the minimum over k (smallest k on ties) by three xor steps; psi_t as three 8-bit planes in one word;
//   (d)                     in the same launch lanes 0..7 walk the chunk's psi words from each end state to the entry state: the table
//   (e) vit_chain_kernel    one wave per row walks the chunk tables backwards, 64 tables per load
//   (f) vit_backtrace_kernel per chunk: from its known end state through its psi words, then the states go out coalesced
// A wave stages its chunk's per-frame values (obs, cents of the candidates) in LDS first, all lanes in parallel, so the serial loops of
// (a) and (c) read LDS only.  No thread walks a row frame by frame.  Plain int64 adds and mins: INF = 2^40 accumulates on the paths
// through gated or empty slots and stays below 2^62 for n_frames <= 2^20 and costs <= 2^20 (no saturation -- it would break
// associativity).  No atomics, 64-bit indices, nothing returns to the host.
#include "f0_frame.h"

#define F0_K 7                                                      // candidates per frame; state 7 is "unvoiced"
#define VIT_INF (1LL << 40)
#define VIT_MAX_CHUNK 128
#define VIT_MAX_FRAMES (1L << 20)
#define VIT_MAX_COST (1L << 20)

// ------------------------------------------------------------------------------------------------
// candidates
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void f0_frame_dips(const float* dp, int tau_min, int tau_max, double sr, int lane, int* ctau, float* cf0, float* cap,
                                              int* count) {
  float last_v = -INFINITY;
  int last_t = -1, n = 0;
  int taus[F0_K];
#pragma unroll
  for (int r = 0; r < F0_K; ++r) {
    float best = INFINITY;
    int at = INT_MAX;
    for (int t = tau_min + lane; t <= tau_max; t += 64) {
      const float v = dp[t];
      const bool dip = (t == tau_min || v < dp[t - 1]) && (t == tau_max || v <= dp[t + 1]);
      const bool after = v > last_v || (v == last_v && t > last_t);
      if (dip && after && (v < best || (v == best && t < at))) {
        best = v;
        at = t;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oa = __shfl_xor(at, o, 64);
      if (ob < best || (ob == best && oa < at)) {
        best = ob;
        at = oa;
      }
    }
    taus[r] = at;                                                     // the same on every lane
    if (at != INT_MAX) {
      ++n;
      last_v = best;
      last_t = at;
    }
  }
  if (lane == 0) *count = n;
  if (lane >= F0_K) return;
  int tau = INT_MAX, rank = 0;
#pragma unroll
  for (int r = 0; r < F0_K; ++r)
    if (r == lane) tau = taus[r];
  if (lane >= n) {                                                    // an empty slot
    ctau[lane] = 0;
    cf0[lane] = 0.f;
    cap[lane] = 0.f;
    return;
  }
#pragma unroll
  for (int r = 0; r < F0_K; ++r) rank += taus[r] < tau ? 1 : 0;      // winners past n are INT_MAX
  const double b = (double)dp[tau];
  double delta = 0.0;
  if (tau - 1 >= 1 && tau + 1 <= tau_max) {
    const double a = (double)dp[tau - 1], c = (double)dp[tau + 1];
    const double q = a - 2.0 * b + c;
    if (q > 0.0) delta = fmin(1.0, fmax(-1.0, 0.5 * (a - c) / q));
  }
  ctau[rank] = tau;
  cf0[rank] = (float)(sr / ((double)tau + delta));
  cap[rank] = (float)b;
}

__global__ __launch_bounds__(256) void f0_dips_kernel(const float* __restrict__ dprime, long count, int tau_min, int tau_max, double sr,
                                                      int* __restrict__ ctau, float* __restrict__ cf0, float* __restrict__ cap,
                                                      int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= count) return;
  f0_frame_dips(dprime + f * (long)(tau_max + 1), tau_min, tau_max, sr, lane, ctau + f * F0_K, cf0 + f * F0_K, cap + f * F0_K, cnt + f);
}

// svs_f0_track's kernel with the dips taken from the LDS row as well
template <int LOG2L>
__global__ __launch_bounds__(64 * F0_MAX_FRAMES) void f0_candidates_kernel(const float* __restrict__ x, long ld_row, int W, int tau_min, int tau_max,
                                                                           int hop, long first_frame, long n_frames, int F, int xcap,
                                                                           double threshold, float rms_gate, double sr, float* __restrict__ rms,
                                                                           float* __restrict__ f0, float* __restrict__ ap, int* __restrict__ voiced,
                                                                           int* __restrict__ ctau, float* __restrict__ cf0, float* __restrict__ cap,
                                                                           int* __restrict__ cnt) {
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
  f0_frame_dips(dp, tau_min, tau_max, sr, lane, ctau + o * F0_K, cf0 + o * F0_K, cap + o * F0_K, cnt + o);
  f0_frame_pick(dp, tau_min, tau_max, threshold, sr, lane, true, r, rms_gate, f0 + o, ap + o, voiced + o);
  if (lane == 0) rms[o] = r;
}

// ------------------------------------------------------------------------------------------------
// the decode
// ------------------------------------------------------------------------------------------------
struct VitArgs {
  const int* ctau;                                                    // [rows][T][7]
  const float* cap;                                                   // [rows][T][7]
  const int* cnt;                                                     // [rows][T]
  const float* rms;                                                   // [rows][T]
  const int* cents;                                                   // [tau_max + 1]
  long T;
  int nc, chunk, tau_min, tau_max;
  float rms_gate;
  long long pitch_cost, switch_cost, unvoiced_cost, octave_cost;
};

struct VitWorkspace {                                                 // per row: nc chunks, T frames
  long long* prod;                                                    // [rows][nc][64]  the chunk products
  long long* entry;                                                   // [rows][nc][8]   delta in front of the chunk
  unsigned* psi;                                                      // [rows][T]       three 8-bit planes per frame
  unsigned* tab;                                                      // [rows][nc]      end state -> entry state, the same packing
  int* cend;                                                          // [rows][nc]      the chunk's end state on the best path
  int* last;                                                          // [rows]          the row's end state
};

__host__ __device__ __forceinline__ size_t vit_up(size_t b) { return (b + 15) & ~(size_t)15; }

static VitWorkspace vit_carve(void* ws, int rows, long T, int nc, size_t* bytes) {
  char* p = (char*)ws;
  size_t o = 0;
  VitWorkspace w;
  w.prod = (long long*)(p + o), o += vit_up((size_t)rows * nc * 64 * sizeof(long long));
  w.entry = (long long*)(p + o), o += vit_up((size_t)rows * nc * 8 * sizeof(long long));
  w.psi = (unsigned*)(p + o), o += vit_up((size_t)rows * T * sizeof(unsigned));
  w.tab = (unsigned*)(p + o), o += vit_up((size_t)rows * nc * sizeof(unsigned));
  w.cend = (int*)(p + o), o += vit_up((size_t)rows * nc * sizeof(int));
  w.last = (int*)(p + o), o += vit_up((size_t)rows * sizeof(int));
  *bytes = o;
  return w;
}

// a wave's LDS, sized by the chunk (2.7 KB at 16 frames, 13.9 KB at 128): the more waves a CU holds the shorter the chunk
struct VitLds {
  long long* P;                                                       // [2][64]
  long long* obs;                                                     // [(chunk + 1) * 8]: frames s-1 .. e-1 of the chunk [s, e)
  int* cen;                                                           // [(chunk + 1) * 8]
  unsigned* psi;                                                      // [chunk]
};

__host__ __device__ __forceinline__ size_t vit_lds_bytes(int chunk) { return 128 * sizeof(long long) + (size_t)(chunk + 1) * 8 * 12 + (size_t)chunk * 4; }

__device__ __forceinline__ VitLds vit_lds(long long* base, int chunk) {
  VitLds l;
  l.P = base;
  l.obs = base + 128;
  l.cen = (int*)(l.obs + (chunk + 1) * 8);
  l.psi = (unsigned*)(l.cen + (chunk + 1) * 8);
  return l;
}

__device__ __forceinline__ long long vit_floordiv(long long a, long long b) {       // b > 0
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// obs and the candidates' cents of frames s-1 .. e-1 into LDS, one (frame, state) per lane and step; the frame in front of frame 0 reads 0
__device__ __forceinline__ void vit_stage(const VitArgs& a, long row, long s, long e, int lane, const VitLds& l) {
  const int items = (int)(e - s + 1) * 8;
  const int c_min = a.cents[a.tau_min];
  for (int idx = lane; idx < items; idx += 64) {
    const long f = s - 1 + (idx >> 3);
    const int j = idx & 7;
    long long o = 0;
    int c = 0;
    if (f >= 0) {
      const long at = row * a.T + f;
      if (j < F0_K) {
        const int tau = min(max(a.ctau[at * F0_K + j], 0), a.tau_max);   // the table has tau_max + 1 entries
        c = a.cents[tau];
        const bool live = j < a.cnt[at] && a.rms[at] >= a.rms_gate;
        o = live ? llrint((double)a.cap[at * F0_K + j] * 4096.0) + vit_floordiv(a.octave_cost * (long long)(c_min - c), 1200) : VIT_INF;
      } else {
        o = a.unvoiced_cost;
      }
    }
    l.obs[idx] = o;
    l.cen[idx] = c;
  }
}

__device__ __forceinline__ long long vit_trans(const VitArgs& a, int i, int j, int ci, int cj) {
  if (i < F0_K && j < F0_K) return a.pitch_cost * (long long)abs(ci - cj);
  return (i == F0_K && j == F0_K) ? 0 : a.switch_cost;
}

__device__ __forceinline__ int vit_lookup(unsigned w, int s) { return ((w >> s) & 1u) | (((w >> (8 + s)) & 1u) << 1) | (((w >> (16 + s)) & 1u) << 2); }

// the word of 8 states held by lanes 0..7 (every lane calls)
__device__ __forceinline__ unsigned vit_pack(int s) {
  const unsigned m0 = (unsigned)(__ballot(s & 1) & 0xffull), m1 = (unsigned)(__ballot(s & 2) & 0xffull), m2 = (unsigned)(__ballot(s & 4) & 0xffull);
  return m0 | (m1 << 8) | (m2 << 16);
}

// (a)
__global__ __launch_bounds__(64) void vit_product_kernel(VitArgs a, VitWorkspace w) {
  extern __shared__ long long vit_shared[];
  const VitLds l = vit_lds(vit_shared, a.chunk);
  const int lane = threadIdx.x, i = lane >> 3, j = lane & 7;
  const long row = blockIdx.y, c = blockIdx.x, s = c * a.chunk, e = min(s + (long)a.chunk, a.T);
  vit_stage(a, row, s, e, lane, l);
  __syncthreads();
  long long P = (s == 0 ? 0 : vit_trans(a, i, j, l.cen[i], l.cen[8 + j])) + l.obs[8 + j];
  for (int q = 2; q <= (int)(e - s); ++q) {                           // frame s - 1 + q
    long long* buf = l.P + 64 * (q & 1);
    buf[lane] = P;
    __syncthreads();
    const int cj = l.cen[q * 8 + j];
    long long best = LLONG_MAX;
#pragma unroll
    for (int k = 0; k < 8; ++k) best = min(best, buf[i * 8 + k] + vit_trans(a, k, j, l.cen[(q - 1) * 8 + k], cj));
    P = best + l.obs[q * 8 + j];
  }
  w.prod[(row * a.nc + c) * 64 + lane] = P;
}

// (b)
__global__ __launch_bounds__(64) void vit_scan_kernel(VitArgs a, VitWorkspace w, long long* __restrict__ cost) {
  const int lane = threadIdx.x;
  const long row = blockIdx.x;
  const long long* prod = w.prod + row * a.nc * 64;
  long long* entry = w.entry + row * a.nc * 8;
  long long dj = 0, di = 0;                                           // delta(lane & 7), delta(lane >> 3)
  for (int c0 = 0; c0 < a.nc; c0 += 8) {
    long long p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = c0 + u < a.nc ? prod[(long)(c0 + u) * 64 + lane] : 0;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (c0 + u < a.nc) {                                            // uniform
        if (lane < 8) entry[(long)(c0 + u) * 8 + lane] = dj;
        long long v = di + p[u];
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) v = min(v, __shfl_xor(v, o, 64));
        dj = v;
        di = __shfl(v, lane >> 3, 64);
      }
  }
  int at = lane & 7;
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    const long long ov = __shfl_xor(dj, o, 64);
    const int oa = __shfl_xor(at, o, 64);
    if (ov < dj || (ov == dj && oa < at)) {
      dj = ov;
      at = oa;
    }
  }
  if (lane == 0) {
    cost[row] = dj;
    w.last[row] = at;
  }
}

// (c) and (d)
__global__ __launch_bounds__(64) void vit_rerun_kernel(VitArgs a, VitWorkspace w) {
  extern __shared__ long long vit_shared[];
  const VitLds l = vit_lds(vit_shared, a.chunk);
  const int lane = threadIdx.x, k = lane >> 3, j = lane & 7;
  const long row = blockIdx.y, c = blockIdx.x, s = c * a.chunk, e = min(s + (long)a.chunk, a.T);
  const int len = (int)(e - s);
  vit_stage(a, row, s, e, lane, l);
  __syncthreads();
  long long dk = w.entry[(row * a.nc + c) * 8 + k];
  for (int q = 1; q <= len; ++q) {                                    // frame s - 1 + q
    long long v = dk + ((s == 0 && q == 1) ? 0 : vit_trans(a, k, j, l.cen[(q - 1) * 8 + k], l.cen[q * 8 + j]));
    int at = k;
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
      const long long ov = __shfl_xor(v, o, 64);
      const int oa = __shfl_xor(at, o, 64);
      if (ov < v || (ov == v && oa < at)) {
        v = ov;
        at = oa;
      }
    }
    const unsigned word = vit_pack(at);                               // lanes 0..7: psi(j), j = lane
    if (lane == 0) l.psi[q - 1] = word;
    dk = __shfl(v + l.obs[q * 8 + j], k, 64);
  }
  __syncthreads();
  for (int idx = lane; idx < len; idx += 64) w.psi[row * a.T + s + idx] = l.psi[idx];
  int st = lane & 7;                                                  // the state at frame e - 1
  for (int q = len; q >= 1; --q)
    if (s + q - 1 > 0) st = vit_lookup(l.psi[q - 1], st);            // psi of frame 0 leads nowhere
  const unsigned table = vit_pack(st);
  if (lane == 0) w.tab[row * a.nc + c] = table;
}

// (e)
__global__ __launch_bounds__(64) void vit_chain_kernel(VitArgs a, VitWorkspace w) {
  const int lane = threadIdx.x;
  const long row = blockIdx.x;
  const unsigned* tab = w.tab + row * a.nc;
  int st = w.last[row];
  for (int base = ((a.nc - 1) / 64) * 64; base >= 0; base -= 64) {
    const int c = base + lane;
    const unsigned word = c < a.nc ? tab[c] : 0u;
    int mine = 0;
    for (int u = min(63, a.nc - 1 - base); u >= 0; --u) {
      if (lane == u) mine = st;
      st = vit_lookup(__shfl(word, u, 64), st);                       // the end state of the chunk in front
    }
    if (c < a.nc) w.cend[row * a.nc + c] = mine;
  }
}

// (f)
__global__ __launch_bounds__(64) void vit_backtrace_kernel(VitArgs a, VitWorkspace w, int* __restrict__ state) {
  __shared__ unsigned psi[VIT_MAX_CHUNK];
  __shared__ int path[VIT_MAX_CHUNK];
  const int lane = threadIdx.x;
  const long row = blockIdx.y, c = blockIdx.x, s = c * a.chunk, e = min(s + (long)a.chunk, a.T);
  const int len = (int)(e - s);
  for (int idx = lane; idx < len; idx += 64) psi[idx] = w.psi[row * a.T + s + idx];
  __syncthreads();
  if (lane == 0) {
    int st = w.cend[row * a.nc + c];
    for (int q = len - 1; q >= 0; --q) {
      path[q] = st;
      st = vit_lookup(psi[q], st);
    }
  }
  __syncthreads();
  for (int idx = lane; idx < len; idx += 64) state[row * a.T + s + idx] = path[idx];
}

__global__ __launch_bounds__(256) void f0_select_kernel(const int* __restrict__ state, const float* __restrict__ cf0, const float* __restrict__ cap,
                                                        const float* __restrict__ raw_f0, const float* __restrict__ raw_ap, long count,
                                                        float* __restrict__ f0, float* __restrict__ ap, int* __restrict__ voiced) {
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  if (f >= count) return;
  const int s = state[f];
  const bool v = s >= 0 && s < F0_K;
  f0[f] = v ? cf0[f * F0_K + s] : raw_f0[f];
  ap[f] = v ? cap[f * F0_K + s] : raw_ap[f];
  voiced[f] = v ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int vit_check_shape(const char* who, int rows, int64_t n_frames, int chunk) {
  SVS_REQUIRE(rows >= 1 && rows <= F0_MAX_ROWS, "%s: rows must be in 1..%d, got %d", who, F0_MAX_ROWS, rows);
  SVS_REQUIRE(n_frames >= 0 && n_frames <= VIT_MAX_FRAMES, "%s: n_frames must be in 0..2^20 (the path sums stay below 2^62), got %lld", who,
              (long long)n_frames);
  SVS_REQUIRE(chunk == 16 || chunk == 32 || chunk == 64 || chunk == 128, "%s: chunk must be 16, 32, 64 or 128, got %d", who, chunk);
  return SVS_OK;
}

extern "C" size_t svs_f0_viterbi_workspace(int rows, int64_t n_frames, int chunk) {
  if (vit_check_shape("svs_f0_viterbi_workspace", rows, n_frames, chunk) != SVS_OK) return 0;
  size_t bytes = 0;
  vit_carve(nullptr, rows, (long)n_frames, (int)((n_frames + chunk - 1) / chunk), &bytes);
  return bytes;
}

extern "C" int svs_f0_dips(const float* dprime, int64_t count, int tau_min, int tau_max, double sr, int32_t* cand_tau, float* cand_f0,
                           float* cand_ap, int32_t* cand_count, hipStream_t stream) {
  SVS_REQUIRE(tau_max >= 1 && tau_max <= F0_MAX_TAU, "svs_f0_dips: tau_max must be in 1..%d, got %d", F0_MAX_TAU, tau_max);
  SVS_REQUIRE(tau_min >= 1 && tau_min < tau_max, "svs_f0_dips: tau_min must be in 1..tau_max - 1 = %d, got %d", tau_max - 1, tau_min);
  SVS_REQUIRE(sr > 0.0 && sr < INFINITY, "svs_f0_dips: sr must be positive and finite, got %g", sr);
  SVS_REQUIRE(count >= 0 && count <= (INT64_MAX / 16) / (F0_MAX_TAU + 1), "svs_f0_dips: the frame count must not be negative, got %lld",
              (long long)count);
  const long nblk = (long)((count + 3) / 4);
  SVS_REQUIRE(nblk < (1L << 31), "svs_f0_dips: %ld blocks do not fit a grid", nblk);
  SVS_REQUIRE(count == 0 || (dprime && cand_tau && cand_f0 && cand_ap && cand_count), "svs_f0_dips: null pointer");
  SVS_REQUIRE(((((uintptr_t)dprime) | ((uintptr_t)cand_tau) | ((uintptr_t)cand_f0) | ((uintptr_t)cand_ap) | ((uintptr_t)cand_count)) & 3u) == 0,
              "svs_f0_dips: dprime, cand_tau, cand_f0, cand_ap and count must be 4-byte aligned");
  if (count == 0) return SVS_OK;
  hipLaunchKernelGGL(f0_dips_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, dprime, (long)count, tau_min, tau_max, sr, cand_tau, cand_f0,
                     cand_ap, cand_count);
  SVS_CHECK_LAUNCH("svs_f0_dips");
  return SVS_OK;
}

extern "C" int svs_f0_candidates(const float* x, int rows, int64_t n, int64_t ld_row, int W, int tau_min, int tau_max, int hop, int64_t first_frame,
                                 int64_t n_frames, double threshold, float rms_gate, double sr, float* f0, float* ap, float* rms, int32_t* voiced,
                                 int32_t* cand_tau, float* cand_f0, float* cand_ap, int32_t* cand_count, hipStream_t stream) {
  const char* who = "svs_f0_candidates";
  int rc = f0_check_signal(who, x, rows, n, ld_row, W, tau_max, hop, first_frame, n_frames);
  if (rc != SVS_OK) return rc;
  rc = f0_check_pick(who, tau_min, tau_max, threshold, rms_gate, sr);
  if (rc != SVS_OK) return rc;
  SVS_REQUIRE(n_frames == 0 || (x && f0 && ap && rms && voiced && cand_tau && cand_f0 && cand_ap && cand_count), "%s: null pointer", who);
  SVS_REQUIRE(((((uintptr_t)f0) | ((uintptr_t)ap) | ((uintptr_t)rms) | ((uintptr_t)voiced) | ((uintptr_t)cand_tau) | ((uintptr_t)cand_f0) |
                ((uintptr_t)cand_ap) | ((uintptr_t)cand_count)) & 3u) == 0,
              "%s: f0, ap, rms, voiced, cand_tau, cand_f0, cand_ap and count must be 4-byte aligned", who);
  if (n_frames == 0) return SVS_OK;
  const F0Plan p = f0_plan(W, tau_max, hop);
  const long nblk = (long)((n_frames + p.F - 1) / p.F);
  SVS_REQUIRE(nblk < (1L << 31), "%s: %ld blocks do not fit a grid", who, nblk);
  const dim3 grid((unsigned)nblk, (unsigned)rows), block(64u * p.F);
#define F0_GO(LOG2L)                                                                                                                        \
  hipLaunchKernelGGL((f0_candidates_kernel<LOG2L>), grid, block, p.lds, stream, x, (long)ld_row, W, tau_min, tau_max, hop, (long)first_frame, \
                     (long)n_frames, p.F, p.xcap, threshold, rms_gate, sr, rms, f0, ap, voiced, cand_tau, cand_f0, cand_ap, cand_count)
  if (p.log2l == 1) F0_GO(1);
  else if (p.log2l == 2) F0_GO(2);
  else F0_GO(3);
#undef F0_GO
  SVS_CHECK_LAUNCH(who);
  return SVS_OK;
}

extern "C" int svs_f0_viterbi(const int32_t* cand_tau, const float* cand_ap, const int32_t* cand_count, const float* rms, int rows, int64_t n_frames,
                              const int32_t* cents, int tau_min, int tau_max, float rms_gate, int64_t pitch_cost, int64_t switch_cost,
                              int64_t unvoiced_cost, int64_t octave_cost, int chunk, void* workspace, int32_t* state, int64_t* cost,
                              hipStream_t stream) {
  const char* who = "svs_f0_viterbi";
  const int rc = vit_check_shape(who, rows, n_frames, chunk);
  if (rc != SVS_OK) return rc;
  SVS_REQUIRE(tau_max >= 1 && tau_max <= F0_MAX_TAU, "%s: tau_max must be in 1..%d, got %d", who, F0_MAX_TAU, tau_max);
  SVS_REQUIRE(tau_min >= 1 && tau_min < tau_max, "%s: tau_min must be in 1..tau_max - 1 = %d, got %d", who, tau_max - 1, tau_min);
  SVS_REQUIRE(rms_gate >= 0.f && rms_gate < INFINITY, "%s: rms_gate must be finite and not negative, got %g", who, (double)rms_gate);
  SVS_REQUIRE(pitch_cost >= 0 && pitch_cost <= VIT_MAX_COST, "%s: pitch_cost must be in 0..2^20, got %lld", who, (long long)pitch_cost);
  SVS_REQUIRE(switch_cost >= 0 && switch_cost <= VIT_MAX_COST, "%s: switch_cost must be in 0..2^20, got %lld", who, (long long)switch_cost);
  SVS_REQUIRE(unvoiced_cost >= 0 && unvoiced_cost <= VIT_MAX_COST, "%s: unvoiced_cost must be in 0..2^20, got %lld", who, (long long)unvoiced_cost);
  SVS_REQUIRE(octave_cost >= 0 && octave_cost <= VIT_MAX_COST, "%s: octave_cost must be in 0..2^20, got %lld", who, (long long)octave_cost);
  SVS_REQUIRE(n_frames == 0 || (cand_tau && cand_ap && cand_count && rms && cents && workspace && state && cost), "%s: null pointer", who);
  SVS_REQUIRE(((((uintptr_t)cand_tau) | ((uintptr_t)cand_ap) | ((uintptr_t)cand_count) | ((uintptr_t)rms) | ((uintptr_t)cents) | ((uintptr_t)state)) & 3u) == 0,
              "%s: cand_tau, cand_ap, count, rms, cents and state must be 4-byte aligned", who);
  SVS_REQUIRE((((uintptr_t)cost) & 7u) == 0, "%s: cost must be 8-byte aligned", who);
  SVS_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "%s: the workspace must be 16-byte aligned", who);
  if (n_frames == 0) return SVS_OK;
  VitArgs a;
  a.ctau = cand_tau, a.cap = cand_ap, a.cnt = cand_count, a.rms = rms, a.cents = cents;
  a.T = (long)n_frames, a.nc = (int)((n_frames + chunk - 1) / chunk), a.chunk = chunk, a.tau_min = tau_min, a.tau_max = tau_max;
  a.rms_gate = rms_gate, a.pitch_cost = pitch_cost, a.switch_cost = switch_cost, a.unvoiced_cost = unvoiced_cost, a.octave_cost = octave_cost;
  size_t bytes = 0;
  const VitWorkspace w = vit_carve(workspace, rows, a.T, a.nc, &bytes);
  const dim3 chunks((unsigned)a.nc, (unsigned)rows), per_row((unsigned)rows), wave(64);
  hipLaunchKernelGGL(vit_product_kernel, chunks, wave, vit_lds_bytes(chunk), stream, a, w);
  SVS_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(vit_scan_kernel, per_row, wave, 0, stream, a, w, (long long*)cost);
  SVS_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(vit_rerun_kernel, chunks, wave, vit_lds_bytes(chunk), stream, a, w);
  SVS_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(vit_chain_kernel, per_row, wave, 0, stream, a, w);
  SVS_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(vit_backtrace_kernel, chunks, wave, 0, stream, a, w, state);
  SVS_CHECK_LAUNCH(who);
  return SVS_OK;
}

extern "C" int svs_f0_smooth_select(const int32_t* state, const float* cand_f0, const float* cand_ap, const float* raw_f0, const float* raw_ap,
                                    int64_t count, float* f0, float* ap, int32_t* voiced, hipStream_t stream) {
  const char* who = "svs_f0_smooth_select";
  SVS_REQUIRE(count >= 0 && count <= (int64_t)F0_MAX_ROWS * VIT_MAX_FRAMES, "%s: the frame count must be in 0..2^26, got %lld", who, (long long)count);
  SVS_REQUIRE(count == 0 || (state && cand_f0 && cand_ap && raw_f0 && raw_ap && f0 && ap && voiced), "%s: null pointer", who);
  SVS_REQUIRE(((((uintptr_t)state) | ((uintptr_t)cand_f0) | ((uintptr_t)cand_ap) | ((uintptr_t)raw_f0) | ((uintptr_t)raw_ap) | ((uintptr_t)f0) |
                ((uintptr_t)ap) | ((uintptr_t)voiced)) & 3u) == 0,
              "%s: every pointer must be 4-byte aligned", who);
  if (count == 0) return SVS_OK;
  hipLaunchKernelGGL(f0_select_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, state, cand_f0, cand_ap, raw_f0, raw_ap,
                     (long)count, f0, ap, voiced);
  SVS_CHECK_LAUNCH(who);
  return SVS_OK;
}
