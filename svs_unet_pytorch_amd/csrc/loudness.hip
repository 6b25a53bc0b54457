// ITU-R BS.1770-4 / EBU R 128 integrated loudness on the device (include/svs_hip.h; the float64 definition is
// svs_unet_pytorch_amd/loudness.py).  The reference peak-normalises every written stem on its own (data.py:162-166) and has no meter.
//
// K-weighting is two cascaded biquads, a sequential recurrence.  In transposed direct form II the cascade is a linear system with
// a 4-value state s = (shelf z0, z1, high-pass z0, z1):  s' = A s + B x,  so a run of L samples maps its start state to
// A^L s + (the end state the same samples give from s = 0).  That makes the recurrence exact in three levels, all fp64:
//   segment   every 100 ms bin [e_k, e_k+1), e_k = floor(k fs / 10), is cut into P equal parts of at most LD_SEG samples; one block
//             stages a segment in LDS (coalesced loads, the stems summed in fp64) and cuts it into chunks of Lc samples, a lane each.
//             Lc is odd, so the lanes' LDS reads, 2 Lc dwords apart, fall on distinct banks.
//   chunk     every lane filters its chunk from s = 0; a Kogge-Stone scan over the lanes with A^(Lc 2^t), t = 0..7, turns the end
//             states into the states at every chunk boundary.  Pass A keeps the segment's end state; pass B starts lane 0 from the
//             segment's true state, scans again, and every lane refilters its chunk from its true state and sums y^2.
//   scan      between the passes one block per channel carries the state over the segments: a lane composes the affine maps of a
//             run of segments, a Kogge-Stone scan over the lanes composes the runs, every lane walks its run again from its true
//             state.  Segment lengths take two values, floor and ceil of a bin over P, so two matrices serve.
// The matrix powers are host arithmetic (repeated squaring in double) and travel as kernel arguments.  Every sum -- the block
// reduction of y^2, the parts of a bin, the bins of a window (4 of a block, 30 of a short-term window), the channels -- is taken in one fixed order: no atomics, and two
// calls on the same input give the same bits.  Indices into the signal are 64-bit.
#include <cmath>

#include "internal.h"

#define LD_SEG 4864          // samples of a segment staged in LDS as doubles (38 KiB); 44.1 and 48 kHz bins fit in one
#define LD_THREADS 256
#define LD_MAX_CH 8
#define LD_FS_MIN 4000       // the shelf's centre (1682 Hz) must lie below fs / 2
#define LD_FS_MAX 768000

// ------------------------------------------------------------------------------------------------
// host arithmetic: coefficients, block count, plan
// ------------------------------------------------------------------------------------------------
static void loud_coeffs(double fs, double* c) {                   // the expressions of loudness.k_weighting, in its order
#pragma clang fp contract(off)
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(M_PI * f0 / fs);
    const double Vh = std::pow(10.0, G / 20.0);
    const double Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    c[0] = (Vh + Vb * K / Q + K * K) / a0;
    c[1] = 2.0 * (K * K - Vh) / a0;
    c[2] = (Vh - Vb * K / Q + K * K) / a0;
    c[3] = 2.0 * (K * K - 1.0) / a0;
    c[4] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(M_PI * f0 / fs);
    const double a0 = 1.0 + K / Q + K * K;
    c[5] = 1.0;
    c[6] = -2.0;
    c[7] = 1.0;
    c[8] = 2.0 * (K * K - 1.0) / a0;
    c[9] = (1.0 - K / Q + K * K) / a0;
  }
}

static bool loud_fs_ok(int fs) { return fs >= LD_FS_MIN && fs <= LD_FS_MAX; }

extern "C" int svs_loudness_coeffs(int fs, double* c) {
  SVS_REQUIRE(c, "svs_loudness_coeffs: null pointer");
  SVS_REQUIRE(loud_fs_ok(fs), "svs_loudness_coeffs: fs must be in %d..%d, got %d", LD_FS_MIN, LD_FS_MAX, fs);
  loud_coeffs((double)fs, c);
  return SVS_OK;
}

extern "C" int64_t svs_loudness_nblocks(int64_t n, int fs) {
  if (n < 0 || !loud_fs_ok(fs) || n > (INT64_MAX / 16)) {
    svs_set_error("svs_loudness_nblocks: n must not be negative and fs must be in %d..%d, got n=%lld fs=%d", LD_FS_MIN, LD_FS_MAX, (long long)n, fs);
    return -1;
  }
  const int64_t bins = (10 * n + 9) / fs;                         // the largest k with e_k <= n; floor(10 n / fs) when 10 divides fs
  return bins > 3 ? bins - 3 : 0;
}

struct LoudTab {
  double c[10];        // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
  double K[8][16];     // A^(Lc 2^t), row-major
  double M[2][16];     // A^len0, A^(len0 + 1): the two segment lengths
};
struct LoudPlan {
  int P;               // parts per bin
  int Lc;              // samples per chunk (odd)
  int len0;            // the shorter segment length
  int64_t nbins, nblocks, nseg;
};

// Powers of A by repeated squaring, in long double.  The high-pass's poles nearly coincide (radius 0.995 at 48 kHz), so A^k has
// entries near 75 for k around 200 while its products with a real state stay near the state's size: every squaring cancels two digits,
// and in double the chain to A^(128 Lc) left z with a relative error of 3e-9 on a DC step.
typedef long double ld_real;
static void mat_mul(const ld_real* a, const ld_real* b, ld_real* out) {
  ld_real t[16];
  for (int r = 0; r < 4; ++r)
    for (int q = 0; q < 4; ++q) {
      ld_real s = 0;
      for (int k = 0; k < 4; ++k) s += a[r * 4 + k] * b[k * 4 + q];
      t[r * 4 + q] = s;
    }
  for (int i = 0; i < 16; ++i) out[i] = t[i];
}
static void mat_pow(const ld_real* a, long e, ld_real* out) {
  ld_real base[16], acc[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (int i = 0; i < 16; ++i) base[i] = a[i];
  for (; e > 0; e >>= 1) {
    if (e & 1) mat_mul(base, acc, acc);
    mat_mul(base, base, base);
  }
  for (int i = 0; i < 16; ++i) out[i] = acc[i];
}
static void mat_round(const ld_real* a, double* out) {
  for (int i = 0; i < 16; ++i) out[i] = (double)a[i];
}

static bool loud_plan(int64_t n, int fs, LoudPlan* p) {
  if (n < 0 || !loud_fs_ok(fs) || n > (INT64_MAX / 16)) return false;
  const int lb_max = fs / 10 + (fs % 10 ? 1 : 0);
  p->P = (lb_max + LD_SEG - 1) / LD_SEG;
  const int lmax = (lb_max + p->P - 1) / p->P;                    // <= LD_SEG
  p->Lc = ((lmax + LD_THREADS - 1) / LD_THREADS) | 1;             // LD_THREADS * Lc >= lmax
  p->len0 = (fs / 10) / p->P;                                     // every segment has len0 or len0 + 1 samples
  const int64_t bins = (10 * n + 9) / fs;                         // the largest k with e_k <= n; floor(10 n / fs) when 10 divides fs
  p->nblocks = bins > 3 ? bins - 3 : 0;
  p->nbins = p->nblocks ? bins : 0;
  p->nseg = p->nbins * p->P;
  return true;
}

static void loud_tab(int fs, const LoudPlan& p, LoudTab* t) {
  loud_coeffs((double)fs, t->c);
  const double *a = t->c + 3, *d = t->c + 5, *e = t->c + 8;      // shelf a1 a2; high-pass b, a1 a2
  // one sample with x = 0: y1 = s0; s0' = -a1 y1 + s1; s1' = -a2 y1; y2 = d0 y1 + s2; s2' = d1 y1 - e1 y2 + s3; s3' = d2 y1 - e2 y2
  const ld_real A[16] = {-(ld_real)a[0], 1, 0, 0,
                         -(ld_real)a[1], 0, 0, 0,
                         (ld_real)d[1] - (ld_real)e[0] * d[0], 0, -(ld_real)e[0], 1,
                         (ld_real)d[2] - (ld_real)e[1] * d[0], 0, -(ld_real)e[1], 0};
  ld_real k[16], m[16];
  mat_pow(A, p.Lc, k);
  for (int i = 0; i < 8; ++i) {
    mat_round(k, t->K[i]);
    mat_mul(k, k, k);
  }
  mat_pow(A, p.len0, m);
  mat_round(m, t->M[0]);
  mat_mul(A, m, m);
  mat_round(m, t->M[1]);
}

static size_t loud_ws_bytes(const LoudPlan& p, int channels) {
  const size_t per = (size_t)channels * (size_t)p.nseg;          // end states, start states (4 doubles each), energies
  const size_t b = per * 9 * sizeof(double);
  return b ? b : 64;
}

extern "C" size_t svs_loudness_workspace_bytes(int64_t n, int channels, int fs) {
  LoudPlan p{};
  if (channels < 1 || channels > LD_MAX_CH || !loud_plan(n, fs, &p)) return 0;
  return loud_ws_bytes(p, channels);
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
struct LoudState { double s0, s1, s2, s3; };

__device__ __forceinline__ double loud_step(const double* __restrict__ c, LoudState& s, double x) {
  const double y1 = c[0] * x + s.s0;
  s.s0 = c[1] * x - c[3] * y1 + s.s1;
  s.s1 = c[2] * x - c[4] * y1;
  const double y2 = c[5] * y1 + s.s2;
  s.s2 = c[6] * y1 - c[8] * y2 + s.s3;
  s.s3 = c[7] * y1 - c[9] * y2;
  return y2;
}

__device__ __forceinline__ LoudState loud_matvec(const double* __restrict__ m, const LoudState& v) {
  LoudState r;
  r.s0 = m[0] * v.s0 + m[1] * v.s1 + m[2] * v.s2 + m[3] * v.s3;
  r.s1 = m[4] * v.s0 + m[5] * v.s1 + m[6] * v.s2 + m[7] * v.s3;
  r.s2 = m[8] * v.s0 + m[9] * v.s1 + m[10] * v.s2 + m[11] * v.s3;
  r.s3 = m[12] * v.s0 + m[13] * v.s1 + m[14] * v.s2 + m[15] * v.s3;
  return r;
}

// segment g = part p of bin k: [e_k + floor(p Lb / P), e_k + floor((p + 1) Lb / P)), Lb = e_k+1 - e_k
__device__ __forceinline__ void loud_segment(long g, int P, long fs, long* start, int* len) {
  const long k = g / P;
  const int p = (int)(g % P);
  const long e0 = k * fs / 10, e1 = (k + 1) * fs / 10;
  const long lb = e1 - e0;
  const long a = p * lb / P, b = (p + 1) * lb / P;
  *start = e0 + a;
  *len = (int)(b - a);
}

// FINAL false (pass A): state_out[(c nseg + g) 4 ..] = the state the segment's samples leave behind when it starts from zero.
// FINAL true (pass B): the segment starts from state_in[...]; energy[c nseg + g] = sum of y^2 over the segment.
template <int STEMS, bool FINAL>
__global__ __launch_bounds__(LD_THREADS) void loud_pass_kernel(const float* __restrict__ x, long ld_stem, long ld_ch, long fs, int P, long nseg,
                                                               int Lc, const LoudTab tab, const double* __restrict__ state_in,
                                                               double* __restrict__ out) {
  __shared__ double sx[LD_SEG];
  __shared__ double sp[LD_THREADS * 4];
  const int tid = threadIdx.x;
  const long g = blockIdx.x;
  const int ch = blockIdx.y;
  long start;
  int len;
  loud_segment(g, P, fs, &start, &len);
  const float* xc = x + (long)ch * ld_ch + start;
  for (int i = tid; i < len; i += LD_THREADS) {
    double v = (double)xc[i];
    if (STEMS == 2) v += (double)xc[ld_stem + i];
    sx[i] = v;
  }
  __syncthreads();

  const int nfull = len / Lc;                                     // lanes 0 .. nfull - 1 hold Lc samples, lane nfull the rest
  const int rest = len - nfull * Lc;
  const int mine = tid < nfull ? Lc : (tid == nfull ? rest : 0);
  const double* xs = sx + tid * Lc;
  LoudState first = {0.0, 0.0, 0.0, 0.0};
  if (FINAL) {
    const double* si = state_in + ((long)ch * nseg + g) * 4;
    first = {si[0], si[1], si[2], si[3]};
  }
  LoudState s = {0.0, 0.0, 0.0, 0.0};
  if (tid == 0) s = first;
  if (tid < nfull) {
    for (int t = 0; t < Lc; ++t) (void)loud_step(tab.c, s, xs[t]);
  } else {
    s = {0.0, 0.0, 0.0, 0.0};
  }
  // inclusive scan: after step t, s of lane i = sum over the last 2^(t+1) chunks m <= i of A^(Lc (i - m)) (end state of chunk m)
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int d = 1 << t;
    if (d < nfull) {                                              // uniform over the block
      sp[tid * 4 + 0] = s.s0; sp[tid * 4 + 1] = s.s1; sp[tid * 4 + 2] = s.s2; sp[tid * 4 + 3] = s.s3;
      __syncthreads();
      if (tid >= d && tid < nfull) {
        const LoudState o = {sp[(tid - d) * 4 + 0], sp[(tid - d) * 4 + 1], sp[(tid - d) * 4 + 2], sp[(tid - d) * 4 + 3]};
        const LoudState m = loud_matvec(tab.K[t], o);
        s.s0 += m.s0; s.s1 += m.s1; s.s2 += m.s2; s.s3 += m.s3;
      }
      __syncthreads();
    }
  }
  sp[tid * 4 + 0] = s.s0; sp[tid * 4 + 1] = s.s1; sp[tid * 4 + 2] = s.s2; sp[tid * 4 + 3] = s.s3;
  __syncthreads();
  LoudState begin = first;                                        // the true state at the start of this lane's chunk
  if (tid > 0 && tid <= nfull) begin = {sp[(tid - 1) * 4 + 0], sp[(tid - 1) * 4 + 1], sp[(tid - 1) * 4 + 2], sp[(tid - 1) * 4 + 3]};

  if (!FINAL) {
    double* so = out + ((long)ch * nseg + g) * 4;
    if (rest == 0) {
      if (tid == nfull - 1) { so[0] = s.s0; so[1] = s.s1; so[2] = s.s2; so[3] = s.s3; }
    } else if (tid == nfull) {
      for (int t = 0; t < rest; ++t) (void)loud_step(tab.c, begin, xs[t]);
      so[0] = begin.s0; so[1] = begin.s1; so[2] = begin.s2; so[3] = begin.s3;
    }
    return;
  }
  double e = 0.0;
  for (int t = 0; t < mine; ++t) {
    const double y = loud_step(tab.c, begin, xs[t]);
    e += y * y;
  }
  __syncthreads();                                                // every lane has read its start state
  sp[tid] = e;
  __syncthreads();
#pragma unroll
  for (int o = LD_THREADS / 2; o > 0; o >>= 1) {                  // one fixed tree
    if (tid < o) sp[tid] += sp[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[(long)ch * nseg + g] = sp[0];
}

// the states at the segment boundaries of one channel: ends[g] (from zero) -> starts[g] (true), one block per channel.  A lane
// composes the affine maps s -> A^len s + b of its run of segments into (T, t); a Kogge-Stone scan over the lanes composes the runs,
// (T_i, t_i) o (T_o, t_o) = (T_i T_o, T_i t_o + t_i); from zero at the signal's start the state after run i is the scanned t_i.
__device__ __forceinline__ void loud_matmul(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) out[r * 4 + q] = a[r * 4 + 0] * b[q] + a[r * 4 + 1] * b[4 + q] + a[r * 4 + 2] * b[8 + q] + a[r * 4 + 3] * b[12 + q];
}

__global__ __launch_bounds__(LD_THREADS) void loud_scan_kernel(const double* __restrict__ ends, double* __restrict__ starts, long nseg, int P,
                                                               long fs, int len0, const LoudTab tab) {
  __shared__ double sT[LD_THREADS * 16];
  __shared__ double st[LD_THREADS * 4];
  const int lane = threadIdx.x;
  const long base = (long)blockIdx.x * nseg;
  const long per = (nseg + LD_THREADS - 1) / LD_THREADS;
  const long g0 = lane * per < nseg ? lane * per : nseg;
  const long g1 = g0 + per < nseg ? g0 + per : nseg;
  double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  LoudState t = {0.0, 0.0, 0.0, 0.0};
  for (long g = g0; g < g1; ++g) {                               // the run from zero, and the run's matrix
    long start;
    int len;
    loud_segment(g, P, fs, &start, &len);
    double m[16], n[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = len == len0 ? tab.M[0][i] : tab.M[1][i];
    const double* b = ends + (base + g) * 4;
    t = loud_matvec(m, t);
    t.s0 += b[0]; t.s1 += b[1]; t.s2 += b[2]; t.s3 += b[3];
    loud_matmul(m, T, n);
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = n[i];
  }
#pragma unroll
  for (int d = 1; d < LD_THREADS; d <<= 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) sT[lane * 16 + i] = T[i];
    st[lane * 4 + 0] = t.s0; st[lane * 4 + 1] = t.s1; st[lane * 4 + 2] = t.s2; st[lane * 4 + 3] = t.s3;
    __syncthreads();
    if (lane >= d) {
      const LoudState to = {st[(lane - d) * 4 + 0], st[(lane - d) * 4 + 1], st[(lane - d) * 4 + 2], st[(lane - d) * 4 + 3]};
      const LoudState add = loud_matvec(T, to);
      t.s0 += add.s0; t.s1 += add.s1; t.s2 += add.s2; t.s3 += add.s3;
      double o[16], n[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) o[i] = sT[(lane - d) * 16 + i];
      loud_matmul(T, o, n);
#pragma unroll
      for (int i = 0; i < 16; ++i) T[i] = n[i];
    }
    __syncthreads();
  }
  st[lane * 4 + 0] = t.s0; st[lane * 4 + 1] = t.s1; st[lane * 4 + 2] = t.s2; st[lane * 4 + 3] = t.s3;
  __syncthreads();
  LoudState s = {0.0, 0.0, 0.0, 0.0};
  if (lane > 0) s = {st[(lane - 1) * 4 + 0], st[(lane - 1) * 4 + 1], st[(lane - 1) * 4 + 2], st[(lane - 1) * 4 + 3]};
  for (long g = g0; g < g1; ++g) {
    long start;
    int len;
    loud_segment(g, P, fs, &start, &len);
    double* o = starts + (base + g) * 4;
    o[0] = s.s0; o[1] = s.s1; o[2] = s.s2; o[3] = s.s3;
    double m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = len == len0 ? tab.M[0][i] : tab.M[1][i];
    const double* b = ends + (base + g) * 4;
    s = loud_matvec(m, s);
    s.s0 += b[0]; s.s1 += b[1]; s.s2 += b[2]; s.s3 += b[3];
  }
}

// z[j] = sum_c (energy of bins j .. j + w - 1 of channel c) / (e_j+w - e_j): parts, bins and channels in ascending order.  w = 4 is
// the 400 ms block of the integrated and momentary loudness, w = 30 the 3 s window of the short-term loudness (EBU Tech 3341 / 3342).
__global__ __launch_bounds__(256) void loud_blocks_kernel(const double* __restrict__ energy, long nseg, int P, long fs, int channels, long nwin,
                                                          int w, double* __restrict__ z) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= nwin) return;
  const double count = (double)((j + w) * fs / 10 - j * fs / 10);
  double sum = 0.0;
  for (int c = 0; c < channels; ++c) {
    double e = 0.0;
    for (long s = j * P; s < (j + w) * P; ++s) e += energy[(long)c * nseg + s];
    sum += e / count;
  }
  z[j] = sum;
}

#define LD_BINS_M 4          // 400 ms
#define LD_BINS_S 30         // 3 s
#define LD_BINS_MAX 600

extern "C" int64_t svs_loudness_nwindows(int64_t n, int fs, int bins) {
  if (n < 0 || !loud_fs_ok(fs) || n > (INT64_MAX / 16) || bins < 1 || bins > LD_BINS_MAX) {
    svs_set_error("svs_loudness_nwindows: n must not be negative, fs must be in %d..%d and bins in 1..%d, got n=%lld fs=%d bins=%d", LD_FS_MIN,
                  LD_FS_MAX, LD_BINS_MAX, (long long)n, fs, bins);
    return -1;
  }
  const int64_t k = (10 * n + 9) / fs;                            // the largest k with e_k <= n
  return k > bins - 1 ? k - (bins - 1) : 0;
}

// The body of svs_loudness_blocks and svs_loudness_series: the argument rules under the caller's name, passes A, scan and B once, then
// the window sums that were asked for.  need_zm: svs_loudness_blocks' rule that z is given.
static int loud_run(const char* who, const float* x, int stems, int channels, int64_t n, int64_t ld_stem, int64_t ld_ch, int fs, double* z_m,
                    double* z_s, bool need_zm, void* ws, size_t ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(stems == 1 || stems == 2, "%s: stems must be 1 or 2, got %d", who, stems);
  SVS_REQUIRE(channels >= 1 && channels <= LD_MAX_CH, "%s: channels must be in 1..%d, got %d", who, LD_MAX_CH, channels);
  SVS_REQUIRE(loud_fs_ok(fs), "%s: fs must be in %d..%d, got %d", who, LD_FS_MIN, LD_FS_MAX, fs);
  LoudPlan p{};
  SVS_REQUIRE(n >= 0 && loud_plan(n, fs, &p), "%s: n must not be negative, got %lld", who, (long long)n);
  SVS_REQUIRE(ld_ch >= n, "%s: ld_ch must be at least n = %lld, got %lld", who, (long long)n, (long long)ld_ch);
  SVS_REQUIRE(p.nseg < (1L << 31), "%s: %lld segments do not fit a grid", who, (long long)p.nseg);
  if (p.nblocks == 0) return SVS_OK;                              // under 400 ms: nothing to write
  SVS_REQUIRE(x && (z_m || !need_zm), "%s: null pointer", who);
  SVS_REQUIRE((((uintptr_t)z_m) & 7u) == 0 && (((uintptr_t)z_s) & 7u) == 0 && (((uintptr_t)ws) & 7u) == 0,
              "%s: z and the workspace must be 8-byte aligned", who);
  if (!ws || ws_bytes < loud_ws_bytes(p, channels)) {
    svs_set_error("%s: workspace too small (%zu bytes, need %zu)", who, ws_bytes, loud_ws_bytes(p, channels));
    return SVS_ERR_WORKSPACE;
  }
  const long nwin_s = p.nbins > LD_BINS_S - 1 ? (long)(p.nbins - (LD_BINS_S - 1)) : 0;
  if (!z_m && (!z_s || nwin_s == 0)) return SVS_OK;               // nothing was asked for
  LoudTab tab;
  loud_tab(fs, p, &tab);
  const size_t per = (size_t)channels * (size_t)p.nseg;
  double* ends = (double*)ws;
  double* starts = ends + per * 4;
  double* energy = starts + per * 4;
  const dim3 grid((unsigned)p.nseg, (unsigned)channels);
  if (stems == 1) {
    hipLaunchKernelGGL((loud_pass_kernel<1, false>), grid, dim3(LD_THREADS), 0, stream, x, (long)ld_stem, (long)ld_ch, (long)fs, p.P, (long)p.nseg,
                       p.Lc, tab, (const double*)nullptr, ends);
  } else {
    hipLaunchKernelGGL((loud_pass_kernel<2, false>), grid, dim3(LD_THREADS), 0, stream, x, (long)ld_stem, (long)ld_ch, (long)fs, p.P, (long)p.nseg,
                       p.Lc, tab, (const double*)nullptr, ends);
  }
  SVS_CHECK_LAUNCH("loudness pass A");
  hipLaunchKernelGGL(loud_scan_kernel, dim3((unsigned)channels), dim3(LD_THREADS), 0, stream, (const double*)ends, starts, (long)p.nseg, p.P, (long)fs,
                     p.len0, tab);
  SVS_CHECK_LAUNCH("loudness scan");
  if (stems == 1) {
    hipLaunchKernelGGL((loud_pass_kernel<1, true>), grid, dim3(LD_THREADS), 0, stream, x, (long)ld_stem, (long)ld_ch, (long)fs, p.P, (long)p.nseg,
                       p.Lc, tab, (const double*)starts, energy);
  } else {
    hipLaunchKernelGGL((loud_pass_kernel<2, true>), grid, dim3(LD_THREADS), 0, stream, x, (long)ld_stem, (long)ld_ch, (long)fs, p.P, (long)p.nseg,
                       p.Lc, tab, (const double*)starts, energy);
  }
  SVS_CHECK_LAUNCH("loudness pass B");
  if (z_m) {
    hipLaunchKernelGGL(loud_blocks_kernel, dim3((unsigned)svs_cdiv(p.nblocks, 256)), dim3(256), 0, stream, (const double*)energy, (long)p.nseg, p.P,
                       (long)fs, channels, (long)p.nblocks, LD_BINS_M, z_m);
    SVS_CHECK_LAUNCH("loudness blocks");
  }
  if (z_s && nwin_s > 0) {
    hipLaunchKernelGGL(loud_blocks_kernel, dim3((unsigned)svs_cdiv(nwin_s, 256)), dim3(256), 0, stream, (const double*)energy, (long)p.nseg, p.P,
                       (long)fs, channels, nwin_s, LD_BINS_S, z_s);
    SVS_CHECK_LAUNCH("loudness short-term windows");
  }
  return SVS_OK;
}

extern "C" int svs_loudness_blocks(const float* x, int stems, int channels, int64_t n, int64_t ld_stem, int64_t ld_ch, int fs, double* z,
                                   void* ws, size_t ws_bytes, hipStream_t stream) {
  return loud_run("svs_loudness_blocks", x, stems, channels, n, ld_stem, ld_ch, fs, z, nullptr, true, ws, ws_bytes, stream);
}

extern "C" int svs_loudness_series(const float* x, int stems, int channels, int64_t n, int64_t ld_stem, int64_t ld_ch, int fs, double* z_m,
                                   double* z_s, void* ws, size_t ws_bytes, hipStream_t stream) {
  return loud_run("svs_loudness_series", x, stems, channels, n, ld_stem, ld_ch, fs, z_m, z_s, false, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// gating and the gain rule: one block
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void loud_block_sum(double* sh, double& a, double& b) {       // both sums over the block, one fixed tree
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = a;
  sh[256 + tid] = b;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { sh[tid] += sh[tid + o]; sh[256 + tid] += sh[256 + tid + o]; }
    __syncthreads();
  }
  a = sh[0];
  b = sh[256];
}

__global__ __launch_bounds__(256) void loud_gain_kernel(const double* __restrict__ z, long nblocks, const float* __restrict__ peaks, int npeaks,
                                                        double target, const double* __restrict__ target_dev, double ceiling,
                                                        float* __restrict__ gain_out, int channels, double* __restrict__ info) {
  __shared__ double sh[512];
  const int tid = threadIdx.x;
  double sum = 0.0, cnt = 0.0;
  for (long j = tid; j < nblocks; j += 256) {                     // absolute gate
    const double v = z[j];
    if (-0.691 + 10.0 * log10(v) > -70.0) { sum += v; cnt += 1.0; }
  }
  loud_block_sum(sh, sum, cnt);
  double L = -INFINITY, kept = 0.0;
  if (cnt > 0.0) {
    const double gamma = -0.691 + 10.0 * log10(sum / cnt) - 10.0;
    double sum2 = 0.0, cnt2 = 0.0;
    for (long j = tid; j < nblocks; j += 256) {                   // both gates
      const double v = z[j];
      const double l = -0.691 + 10.0 * log10(v);
      if (l > -70.0 && l > gamma) { sum2 += v; cnt2 += 1.0; }
    }
    loud_block_sum(sh, sum2, cnt2);
    kept = cnt2;
    if (cnt2 > 0.0) L = -0.691 + 10.0 * log10(sum2 / cnt2);
  }
  if (tid != 0) return;
  float peak = 0.f;
  for (int i = 0; i < npeaks; ++i) peak = fmaxf(peak, fabsf(peaks[i]));
  const double tgt = target_dev ? target_dev[0] : target;
  info[0] = L;
  info[1] = kept;
  if (tgt != tgt) {                                               // NaN: measure only
    info[2] = tgt;
    info[3] = 0.0;
    return;
  }
  const double unlimited = L == -INFINITY ? INFINITY : pow(10.0, (tgt - L) / 20.0);
  const double cap = peak > 0.f ? ceiling / (double)peak : INFINITY;
  double g = unlimited < cap ? unlimited : cap;
  if (!(g < INFINITY)) g = 1.0;                                    // silence with nothing to aim at stays as it is
  info[2] = unlimited;
  info[3] = cap < unlimited ? 1.0 : 0.0;
  for (int c = 0; c < channels; ++c) gain_out[c] = (float)g;
}

extern "C" int svs_loudness_gain(const double* z, int64_t nblocks, const float* peaks, int npeaks, double target, const double* target_dev,
                                 double ceiling, float* gain_out, int channels, double* info, hipStream_t stream) {
  SVS_REQUIRE(nblocks >= 0, "svs_loudness_gain: nblocks must not be negative, got %lld", (long long)nblocks);
  SVS_REQUIRE(npeaks >= 0, "svs_loudness_gain: npeaks must not be negative, got %d", npeaks);
  SVS_REQUIRE(channels >= 0 && channels <= LD_MAX_CH, "svs_loudness_gain: channels must be in 0..%d, got %d", LD_MAX_CH, channels);
  SVS_REQUIRE(ceiling > 0.0, "svs_loudness_gain: ceiling must be positive, got %g", ceiling);
  SVS_REQUIRE(info && (z || nblocks == 0) && (peaks || npeaks == 0) && (gain_out || channels == 0), "svs_loudness_gain: null pointer");
  SVS_REQUIRE(target_dev || target != target || channels > 0, "svs_loudness_gain: a target needs gain_out[channels], channels >= 1");
  SVS_REQUIRE((((uintptr_t)z) & 7u) == 0 && (((uintptr_t)info) & 7u) == 0 && (((uintptr_t)target_dev) & 7u) == 0,
              "svs_loudness_gain: z, info and target_dev must be 8-byte aligned");
  hipLaunchKernelGGL(loud_gain_kernel, dim3(1), dim3(256), 0, stream, z, (long)nblocks, peaks, npeaks, target, target_dev, ceiling, gain_out,
                     channels, info);
  SVS_CHECK_LAUNCH("loudness gain");
  return SVS_OK;
}
