// BSS-eval on the GPU (svs_unet_pytorch_amd/evaluate.py: _project / _criteria), fp64 throughout, gfx950:
//   bss_corr_kernel         lagged correlations C_xy[k] = sum_m x[m+k] y[m], 0 <= k < nlags, of requested signal pairs.
//                           A block stages a chunk of T samples of every signal (plus a MAX_LAG halo) in LDS; a thread
//                           owns a run of 8 consecutive lags of one pair and sweeps the chunk with the run's window in
//                           registers (8 FMAs per two LDS reads).  Blocks stride over chunks and write one partial per
//                           (block, lag) to a slab.  The framewise form runs every window of a signal in the same launch:
//                           each window has blocks and a slab of its own.
//   bss_corr_reduce_kernel  sums the slab over blocks in a fixed order: no atomics, bitwise reproducible.
//   bss_expand_kernel       block-Toeplitz Gram matrix G (order K*flen, padded to a multiple of 64 with an identity) and
//                           the right-hand sides D, stored below G as extra rows: [G; D^T].
//   bss_panel_kernel /      right-looking blocked Cholesky of G in 64-wide panels.  Because the right-hand sides are rows
//   bss_update_kernel       under G, the same triangular solves and updates that form L turn them into y^T = (L^-1 D)^T.
//   bss_norm_kernel         |y|^2 per right-hand side = D^T G^-1 D, the energy of the projection (fixed-order sums).
//   bss_back_diag_kernel /  BSS-eval v4 only (at the end of this file): the back substitution L^T c = y that leaves the filter
//   bss_back_update_kernel  coefficients c = G^-1 D; csrc/bss_v4.hip applies them to the frames.
// The solve kernels take a batch of independent systems of one shape: the system is the leading part of the flattened
// block index, so a batch costs the launches of one system.  A pivot that is not > 0 (a silent reference: G singular) is
// reported through the system's status word; the factorisation goes on with a unit pivot so that nothing faults, and the
// caller discards that system's result.  The image entry points (below) share the host side and the expand, update and
// norm kernels; their tile factorisation (the rank rule, the diagonal tile factored once per step) and their panel kernel
// stay beside the mono ones: one templated tile routine gave the same bits but cost the mono path 3 to 4 % in three forms
// (DESIGN.md section 9).
#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int BSS_T = 1024;                          // samples per chunk
constexpr int BSS_RUN = 8;                           // lags per thread
constexpr int BSS_STAGE = BSS_T + SVS_BSS_MAX_LAG;   // staged samples per signal: chunk + halo (+1 for the last window load)
constexpr int BSS_PADLEN = BSS_STAGE + BSS_STAGE / 8;
constexpr int BSS_THREADS = 256;
constexpr int BSS_MAX_BLOCKS = 1024;                 // blocks per launch (x * y); 2 blocks of 5 signals fit a CU's LDS
constexpr long BSS_MAX_GRID = 0xffffffffL / BSS_THREADS;   // blocks in one grid dimension (its work-items must fit 32 bits)
constexpr int NB = 64;                               // Cholesky panel width

// one padding double after every 8: the 8-lag runs of consecutive lanes start 9 doubles apart, so a wave's window loads
// hit distinct banks
__device__ __forceinline__ int pidx(int i) { return i + (i >> 3); }

// Window w of a launch is x[:, w*hop .. w*hop + window), zero past its end and past n; a whole signal is one window
// (window = hop = n).  chunks: per window; gx: blocks per window (the grid is nwin * gx blocks wide); rblocks: reduce blocks
// per window.  Slab [window][block][lag]; window w's correlations go to out + w * out_stride.
struct CorrArgs {
  const double* x; long ld; long n; int nsig, npairs, runs, chunks;
  int px[SVS_BSS_MAX_PAIRS], py[SVS_BSS_MAX_PAIRS], nl[SVS_BSS_MAX_PAIRS], run0[SVS_BSS_MAX_PAIRS + 1], off[SVS_BSS_MAX_PAIRS];
  double* slab; double* out;
  long hop, window, out_stride; int gx, rblocks;
};

__device__ __forceinline__ int pair_of_run(const CorrArgs& a, int run) {
  int p = 0;
  while (p + 1 < a.npairs && run >= a.run0[p + 1]) ++p;
  return p;
}

// One staged chunk of a run: acc[j] += sum_m X[m + k0 + j] Y[m], m < BSS_T, with the run's window of X in registers.
__device__ __forceinline__ void corr_sweep(const double* X, const double* Y, int k0, double (&acc)[BSS_RUN]) {
  double win[BSS_RUN];
#pragma unroll
  for (int j = 0; j < BSS_RUN; ++j) win[j] = X[pidx(k0 + j)];
  for (int m = 0; m < BSS_T; m += BSS_RUN) {
    // m, k0 multiples of 8: the next window and the 8 y samples are contiguous groups of the padded layout
    const double* xn = X + (m + k0 + BSS_RUN) / 8 * 9;
    const double* yn = Y + m / 8 * 9;
    double nx[BSS_RUN], y[BSS_RUN];
#pragma unroll
    for (int j = 0; j < BSS_RUN; ++j) { nx[j] = xn[j]; y[j] = yn[j]; }
#pragma unroll
    for (int t = 0; t < BSS_RUN; ++t)
#pragma unroll
      for (int j = 0; j < BSS_RUN; ++j) acc[j] = fma(t + j < BSS_RUN ? win[t + j] : nx[t + j - BSS_RUN], y[t], acc[j]);
#pragma unroll
    for (int j = 0; j < BSS_RUN; ++j) win[j] = nx[j];
  }
}

__global__ __launch_bounds__(BSS_THREADS) void bss_corr_kernel(CorrArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sig[];      // [nsig][BSS_PADLEN]
  const int tid = threadIdx.x;
  const int run = blockIdx.y * BSS_THREADS + tid;
  const bool active = run < a.runs;
  int p = 0, k0 = 0;
  if (active) {
    p = pair_of_run(a, run);
    k0 = (run - a.run0[p]) * BSS_RUN;
  }
  const double* X = sig + (active ? a.px[p] : 0) * BSS_PADLEN;
  const double* Y = sig + (active ? a.py[p] : 0) * BSS_PADLEN;
  const int w = blockIdx.x / a.gx, bx = blockIdx.x % a.gx;
  const long base = (long)w * a.hop;
  const long nw = a.n - base < a.window ? a.n - base : a.window;   // samples of window w that exist (<= 0: none)
  double acc[BSS_RUN];
#pragma unroll
  for (int j = 0; j < BSS_RUN; ++j) acc[j] = 0.0;
  for (int c = bx; c < a.chunks; c += a.gx) {
    const long m0 = (long)c * BSS_T;
    __syncthreads();
    for (int s = 0; s < a.nsig; ++s) {
      const double* src = a.x + (long)s * a.ld + base;
      for (int i = tid; i < BSS_STAGE; i += BSS_THREADS) {
        const long g = m0 + i;
        sig[s * BSS_PADLEN + pidx(i)] = g < nw ? src[g] : 0.0;
      }
    }
    __syncthreads();
    if (active) {
      corr_sweep(X, Y, k0, acc);
    }
  }
  if (active) {
    double* dst = a.slab + (((long)w * a.gx + bx) * a.runs + run) * BSS_RUN;
#pragma unroll
    for (int j = 0; j < BSS_RUN; ++j) dst[j] = acc[j];
  }
}

__global__ __launch_bounds__(BSS_THREADS) void bss_corr_reduce_kernel(CorrArgs a) {
  const int w = blockIdx.x / a.rblocks;
  const int l = (blockIdx.x % a.rblocks) * BSS_THREADS + threadIdx.x;
  if (l >= a.runs * BSS_RUN) return;
  const int run = l / BSS_RUN;
  const int p = pair_of_run(a, run);
  const int k = (run - a.run0[p]) * BSS_RUN + l % BSS_RUN;
  if (k >= a.nl[p]) return;
  const long stride = (long)a.runs * BSS_RUN;
  const double* slab = a.slab + (long)w * a.gx * stride;
  double s = 0.0;
  for (int b = 0; b < a.gx; ++b) s += slab[b * stride + l];
  a.out[(long)w * a.out_stride + a.off[p] + k] = s;
}

// blocks per window: one per chunk while the whole grid stays within BSS_MAX_BLOCKS
int corr_blocks(long window, int runs, long nwin) {
  const long chunks = (window + BSS_T - 1) / BSS_T;
  const long ygroups = (runs + BSS_THREADS - 1) / BSS_THREADS;
  return (int)std::min<long>(chunks, std::max<long>(1, BSS_MAX_BLOCKS / (ygroups * nwin)));
}

int count_runs(int npairs, const int* pairs) {
  int runs = 0;
  for (int q = 0; q < npairs; ++q) runs += (pairs[3 * q + 2] + BSS_RUN - 1) / BSS_RUN;
  return runs;
}

bool pairs_valid(int npairs, const int* pairs) {
  if (npairs < 1 || npairs > SVS_BSS_MAX_PAIRS || !pairs) return false;
  for (int q = 0; q < npairs; ++q)
    if (pairs[3 * q] < 0 || pairs[3 * q + 1] < 0 || pairs[3 * q + 2] < 1 || pairs[3 * q + 2] > SVS_BSS_MAX_LAG) return false;
  return true;
}

// the argument checks of both correlation entry points (`who`), which differ in their signal and pair limits
int corr_check(const char* who, int max_signals, int max_pairs, const double* x, int64_t ld, int nsig, int64_t n,
               int64_t window, int64_t hop, int64_t nwin, const int* pairs, int npairs, const double* out,
               int64_t out_stride) {
  SVS_REQUIRE(x && out && pairs && n >= 1 && ld >= n && nsig >= 1 && nsig <= max_signals && npairs >= 1 &&
              npairs <= max_pairs, "%s: bad arguments", who);
  long lags = 0;
  for (int q = 0; q < npairs; ++q) {
    const int px = pairs[3 * q], py = pairs[3 * q + 1], nl = pairs[3 * q + 2];
    SVS_REQUIRE(px >= 0 && px < nsig && py >= 0 && py < nsig && nl >= 1 && nl <= SVS_BSS_MAX_LAG,
                "%s: pair %d = (%d, %d, %d) out of range", who, q, px, py, nl);
    lags += nl;
  }
  SVS_REQUIRE(window >= 1 && hop >= 1 && nwin >= 1 && out_stride >= lags,
              "%s: window = %ld, hop = %ld, nwin = %ld, out_stride = %ld (>= %ld lags) out of range", who, (long)window,
              (long)hop, (long)nwin, (long)out_stride, lags);
  return SVS_OK;
}

int corr_launch(const CorrArgs& a, long nwin, hipStream_t stream) {
  const int gy = (a.runs + BSS_THREADS - 1) / BSS_THREADS;
  const int lds = a.nsig * BSS_PADLEN * (int)sizeof(double);
  SVS_HIP(hipFuncSetAttribute((const void*)bss_corr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL(bss_corr_kernel, dim3((unsigned)(nwin * a.gx), gy), dim3(BSS_THREADS), lds, stream, a);
  SVS_CHECK_LAUNCH("bss_corr");
  hipLaunchKernelGGL(bss_corr_reduce_kernel, dim3((unsigned)(nwin * a.rblocks)), dim3(BSS_THREADS), 0, stream, a);
  SVS_CHECK_LAUNCH("bss_corr_reduce");
  return SVS_OK;
}

// ---- Gram matrix, Cholesky, forward solve ---------------------------------------------------

// System s of a launch: its matrix at M + s * mstride, its status word status[s], its norms at ynorm2 + s * nrhs.  Its
// offsets in corr come from goff / roff (one system) or from the device table tab (per system: K*K gram offsets, then
// K*nrhs right-hand-side offsets).
struct SolveArgs {
  const double* corr; int K, flen, nrhs, np, rows;      // np: order padded to NB; rows = np + rhs rows (padded to NB)
  int goff[4], roff[2 * SVS_BSS_MAX_RHS];
  double* M; int* status; double* ynorm2;               // M: rows x np, row-major
  const int64_t* tab; long mstride;
};

__device__ __forceinline__ long gram_at(const SolveArgs& a, int s, int q) {
  return a.tab ? a.tab[(long)s * (a.K * a.K + a.K * a.nrhs) + q] : a.goff[q];
}

__device__ __forceinline__ long rhs_at(const SolveArgs& a, int s, int q) {
  return a.tab ? a.tab[(long)s * (a.K * a.K + a.K * a.nrhs) + a.K * a.K + q] : a.roff[q];
}

__global__ __launch_bounds__(BSS_THREADS) void bss_expand_kernel(SolveArgs a, int per) {
  const int s = blockIdx.x / per;
  const long e = (long)(blockIdx.x % per) * BSS_THREADS + threadIdx.x;
  double* M = a.M + s * a.mstride;
  if (e == 0) a.status[s] = 0;
  if (e >= (long)a.rows * a.np) return;
  const int r = (int)(e / a.np), c = (int)(e % a.np), kf = a.K * a.flen;
  double v = 0.0;
  if (r < a.np) {
    if (r < kf && c < kf) {                          // G[(i,p),(j,q)] = R_ij[q-p]; R_ij[-d] = R_ji[d]
      const int i = r / a.flen, pp = r % a.flen, j = c / a.flen, q = c % a.flen;
      v = q >= pp ? a.corr[gram_at(a, s, i * a.K + j) + (q - pp)] : a.corr[gram_at(a, s, j * a.K + i) + (pp - q)];
    } else {
      v = r == c ? 1.0 : 0.0;
    }
  } else if (r - a.np < a.nrhs && c < kf) {          // D[(i,p)] of right-hand side r
    v = a.corr[rhs_at(a, s, (r - a.np) * a.K + c / a.flen) + c % a.flen];
  }
  M[e] = v;
}

// The rank rule on the 64 x 64 tile in L (lower part), all threads of the block; col0 is the tile's first column and kf the
// order of G (the identity padding past it is never counted).  bad: first failing column of the tile or -1; nskip: skipped.
__device__ __forceinline__ void img_factor_tile(double (*L)[NB + 1], double thr, int col0, int kf, int& bad, int& nskip) {
  const int tid = threadIdx.x;
  bad = -1; nskip = 0;
  for (int c = 0; c < NB; ++c) {
    __syncthreads();
    const double d = L[c][c];
    const bool ok = d > thr;                           // false for NaN
    if (!ok && col0 + c < kf) {
      if (fabs(d) <= thr) ++nskip;
      else if (bad < 0) bad = c;
    }
    const double piv = ok ? sqrt(d) : 0.0;
    __syncthreads();
    if (tid == c) L[c][c] = piv;
    else if (tid > c && tid < NB) L[tid][c] = ok ? L[tid][c] / piv : 0.0;
    __syncthreads();
    for (int e = tid; e < NB * NB; e += BSS_THREADS) {
      const int r = e / NB, q = e % NB;
      if (q > c && r >= q) L[r][q] -= L[r][c] * L[q][c];
    }
  }
  __syncthreads();
}

// thr = order * 2^-52 * max diag G (LAPACK dpstrf's tolerance)
__device__ __forceinline__ double rank_threshold(const SolveArgs& a, int s) {
  double top = 0.0;
  for (int i = 0; i < a.K; ++i) top = fmax(top, a.corr[gram_at(a, s, i * a.K + i)]);
  return (double)(a.K * a.flen) * 0x1p-52 * top;
}

// Step k of the image solve, one block per system: factor tile (k,k) in place under the rank rule.
__global__ __launch_bounds__(BSS_THREADS) void bss_diag_kernel(SolveArgs a, int* skipped, int k) {
  __shared__ double L[NB][NB + 1];
  const int s = blockIdx.x, tid = threadIdx.x;
  const long ld = a.np;
  double* dk = a.M + s * a.mstride + (long)k * NB * ld + (long)k * NB;
  for (int e = tid; e < NB * NB; e += BSS_THREADS) L[e / NB][e % NB] = dk[(e / NB) * ld + e % NB];
  int bad, nskip;
  img_factor_tile(L, rank_threshold(a, s), k * NB, a.K * a.flen, bad, nskip);
  for (int e = tid; e < NB * NB; e += BSS_THREADS) dk[(e / NB) * ld + e % NB] = L[e / NB][e % NB];
  if (tid == 0) {
    if (bad >= 0 && a.status[s] == 0) a.status[s] = k * NB + bad + 1;
    skipped[s] = (k ? skipped[s] : 0) + nskip;         // one block per system and step, steps in stream order
  }
}

// Step k of the mono solve: block b factors the diagonal tile (k,k) in LDS (every block, the same bits) and either reports
// its first bad pivot (b == 0) or solves tile (k+b, k) against it: X L_kk^T = A.  The factor is never written back: the
// blocks of one launch may start at any time, and a late block must still read the unfactored tile.  Nothing later reads
// tile (k,k).  A whole track is a batch of one system, where this costs a launch less per step than factoring once
// (DESIGN.md section 9).
__global__ __launch_bounds__(BSS_THREADS) void bss_panel_kernel(SolveArgs a, int k) {
  __shared__ double L[NB][NB + 1];
  __shared__ double A[NB][NB + 1];
  const int nt = a.rows / NB - k;
  const int s = blockIdx.x / nt;
  const int tid = threadIdx.x, i = k + blockIdx.x % nt;
  const long ld = a.np;
  double* M = a.M + s * a.mstride;
  const double* dk = M + (long)k * NB * ld + (long)k * NB;
  const double* di = M + (long)i * NB * ld + (long)k * NB;
  for (int e = tid; e < NB * NB; e += BSS_THREADS) {
    L[e / NB][e % NB] = dk[(e / NB) * ld + e % NB];
    if (i != k) A[e / NB][e % NB] = di[(e / NB) * ld + e % NB];
  }
  int bad = -1;
  for (int c = 0; c < NB; ++c) {
    __syncthreads();
    const double d = L[c][c];
    const bool ok = d > 0.0;                         // false for 0, negative and NaN
    if (!ok && bad < 0) bad = c;
    const double piv = ok ? sqrt(d) : 1.0;
    __syncthreads();
    if (tid == c) L[c][c] = piv;
    else if (tid > c && tid < NB) L[tid][c] /= piv;
    __syncthreads();
    for (int e = tid; e < NB * NB; e += BSS_THREADS) {
      const int r = e / NB, q = e % NB;
      if (q > c && r >= q) L[r][q] -= L[r][c] * L[q][c];
    }
  }
  __syncthreads();
  if (i == k) {
    if (tid == 0 && bad >= 0 && a.status[s] == 0) a.status[s] = k * NB + bad + 1;
    return;
  }
  for (int c = 0; c < NB; ++c) {
    if (tid < NB) A[tid][c] /= L[c][c];
    __syncthreads();
    for (int e = tid; e < NB * NB; e += BSS_THREADS) {
      const int r = e / NB, q = e % NB;
      if (q > c) A[r][q] -= A[r][c] * L[q][c];
    }
    __syncthreads();
  }
  double* dst = M + (long)i * NB * ld + (long)k * NB;
  for (int e = tid; e < NB * NB; e += BSS_THREADS) dst[(e / NB) * ld + e % NB] = A[e / NB][e % NB];
}

// Step k of the image solve: tile (i, k), i > k, becomes X with X L_kk^T = A against the factor bss_diag_kernel left in
// tile (k,k); a skipped column (L_kk[c][c] == 0) of X is zero.  Block index: system, then tile row.
__global__ __launch_bounds__(BSS_THREADS) void bss_img_panel_kernel(SolveArgs a, int k) {
  __shared__ double L[NB][NB + 1];
  __shared__ double A[NB][NB + 1];
  const int nt = a.rows / NB - k - 1;
  const int s = blockIdx.x / nt;
  const int tid = threadIdx.x, i = k + 1 + blockIdx.x % nt;
  const long ld = a.np;
  double* M = a.M + s * a.mstride;
  const double* dk = M + (long)k * NB * ld + (long)k * NB;
  double* di = M + (long)i * NB * ld + (long)k * NB;
  for (int e = tid; e < NB * NB; e += BSS_THREADS) {
    L[e / NB][e % NB] = dk[(e / NB) * ld + e % NB];
    A[e / NB][e % NB] = di[(e / NB) * ld + e % NB];
  }
  __syncthreads();
  for (int c = 0; c < NB; ++c) {
    const double piv = L[c][c];
    if (tid < NB) A[tid][c] = piv != 0.0 ? A[tid][c] / piv : 0.0;
    __syncthreads();
    for (int e = tid; e < NB * NB; e += BSS_THREADS) {
      const int r = e / NB, q = e % NB;
      if (q > c) A[r][q] -= A[r][c] * L[q][c];
    }
    __syncthreads();
  }
  for (int e = tid; e < NB * NB; e += BSS_THREADS) di[(e / NB) * ld + e % NB] = A[e / NB][e % NB];
}

// Step k: tile (i, j), k < j <= i, j a column tile of G: A_ij -= L_ik L_jk^T.  Thread (tr, tc) owns rows tr + 16 a and
// columns tc + 16 b.  Block index: system, then tile row, then tile column.
__global__ __launch_bounds__(BSS_THREADS) void bss_update_kernel(SolveArgs a, int k) {
  const int nj = a.np / NB - k - 1, ni = a.rows / NB - k - 1;
  const int s = blockIdx.x / (ni * nj), t = blockIdx.x % (ni * nj);
  const int j = k + 1 + t % nj, i = k + 1 + t / nj;
  if (i < j) return;
  __shared__ double Li[NB][NB + 1];                  // [kk][r]
  __shared__ double Lj[NB][NB + 1];
  const int tid = threadIdx.x, tr = tid / 16, tc = tid % 16;
  const long ld = a.np;
  double* M = a.M + s * a.mstride;
  const double* si = M + (long)i * NB * ld + (long)k * NB;
  const double* sj = M + (long)j * NB * ld + (long)k * NB;
  for (int e = tid; e < NB * NB; e += BSS_THREADS) {
    const int r = e / NB, kk = e % NB;
    Li[kk][r] = si[r * ld + kk];
    Lj[kk][r] = sj[r * ld + kk];
  }
  __syncthreads();
  double acc[4][4] = {};
  for (int kk = 0; kk < NB; ++kk) {
    double u[4], v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { u[q] = Li[kk][tr + 16 * q]; v[q] = Lj[kk][tc + 16 * q]; }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[p][q] = fma(u[p], v[q], acc[p][q]);
  }
  double* dst = M + (long)i * NB * ld + (long)j * NB;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[(tr + 16 * p) * ld + tc + 16 * q] -= acc[p][q];
}

__global__ __launch_bounds__(BSS_THREADS) void bss_norm_kernel(SolveArgs a) {
  __shared__ double red[BSS_THREADS];
  const int tid = threadIdx.x;
  const int s = blockIdx.x / a.nrhs, r = blockIdx.x % a.nrhs;
  const double* y = a.M + s * a.mstride + (long)(a.np + r) * a.np;
  double acc = 0.0;
  for (int c = tid; c < a.np; c += BSS_THREADS) acc = fma(y[c], y[c], acc);
  red[tid] = acc;
  for (int h = BSS_THREADS / 2; h > 0; h >>= 1) {
    __syncthreads();
    if (tid < h) red[tid] += red[tid + h];
  }
  if (tid == 0) a.ynorm2[(long)s * a.nrhs + r] = red[0];
}

void solve_dims(int K, int flen, int nrhs, int& np, int& rows) {
  np = (K * flen + NB - 1) / NB * NB;
  rows = np + (nrhs + NB - 1) / NB * NB;
}

bool solve_shape_valid(int max_refs, int K, int flen, int nrhs) {
  return K >= 1 && K <= max_refs && flen >= 1 && flen <= SVS_BSS_MAX_LAG && nrhs >= 1 && nrhs <= SVS_BSS_MAX_RHS;
}

// systems that fit one batch: the widest launch of one system (the expand launch, or the first update launch of a small
// order) times the batch must stay within BSS_MAX_GRID blocks
long solve_max_systems(int K, int flen, int nrhs) {
  int np, rows;
  solve_dims(K, flen, nrhs, np, rows);
  const long tc = np / NB, tr = rows / NB;
  const long widest = std::max<long>({(long)svs_cdiv((long)rows * np, BSS_THREADS), tr, (tc - 1) * (tr - 1), (long)nrhs});
  return BSS_MAX_GRID / widest;
}

size_t solve_table_bytes(long nbatch, int K, int nrhs) {
  return svs_align_up((size_t)nbatch * (K * K + K * nrhs) * sizeof(int64_t), 256);
}

// the offset table, then nbatch matrices; 0: the shape is invalid or the batch too large for one launch
size_t solve_batched_ws_bytes(int max_refs, long nbatch, int K, int flen, int nrhs) {
  if (!solve_shape_valid(max_refs, K, flen, nrhs) || nbatch < 1 || nbatch > solve_max_systems(K, flen, nrhs)) return 0;
  int np, rows;
  solve_dims(K, flen, nrhs, np, rows);
  return solve_table_bytes(nbatch, K, nrhs) + (size_t)nbatch * rows * np * sizeof(double);
}

// expand; per step the panel launch (images: after the diagonal launch) and the update launch; the norms -- each over all
// nsys systems at once
int solve_launch(const SolveArgs& a, int* skipped, long nsys, bool rank, hipStream_t stream) {
  const int tc = a.np / NB, tr = a.rows / NB;
  const int per = svs_cdiv((long)a.rows * a.np, BSS_THREADS);
  hipLaunchKernelGGL(bss_expand_kernel, dim3((unsigned)(nsys * per)), dim3(BSS_THREADS), 0, stream, a, per);
  SVS_CHECK_LAUNCH("bss_expand");
  for (int k = 0; k < tc; ++k) {
    if (rank) {
      hipLaunchKernelGGL(bss_diag_kernel, dim3((unsigned)nsys), dim3(BSS_THREADS), 0, stream, a, skipped, k);
      SVS_CHECK_LAUNCH("bss_diag");
      hipLaunchKernelGGL(bss_img_panel_kernel, dim3((unsigned)(nsys * (tr - k - 1))), dim3(BSS_THREADS), 0, stream, a, k);
      SVS_CHECK_LAUNCH("bss_img_panel");
    } else {
      hipLaunchKernelGGL(bss_panel_kernel, dim3((unsigned)(nsys * (tr - k))), dim3(BSS_THREADS), 0, stream, a, k);
      SVS_CHECK_LAUNCH("bss_panel");
    }
    if (k + 1 < tc) {
      hipLaunchKernelGGL(bss_update_kernel, dim3((unsigned)(nsys * (tc - k - 1) * (tr - k - 1))), dim3(BSS_THREADS), 0,
                         stream, a, k);
      SVS_CHECK_LAUNCH("bss_update");
    }
  }
  hipLaunchKernelGGL(bss_norm_kernel, dim3((unsigned)(nsys * a.nrhs)), dim3(BSS_THREADS), 0, stream, a);
  SVS_CHECK_LAUNCH("bss_norm");
  return SVS_OK;
}

// the body of the batched-solve entry points (`who`): K <= max_refs; rank: the image pivot rule, which fills skipped;
// made: where the launches' arguments go for a caller that has more to launch on the factored systems
int solve_batched(const char* who, int max_refs, bool rank, const double* corr, int64_t nbatch, int K, int flen,
                  const int64_t* gram_off, const int64_t* rhs_off, int nrhs, double* ynorm2, int* status, int* skipped,
                  void* ws, size_t ws_bytes, hipStream_t stream, SolveArgs* made = nullptr) {
  SVS_REQUIRE(corr && gram_off && rhs_off && ynorm2 && status && (skipped || !rank) && nbatch >= 1 &&
              solve_shape_valid(max_refs, K, flen, nrhs), "%s: bad arguments", who);
  SVS_REQUIRE(nbatch <= solve_max_systems(K, flen, nrhs), "%s: nbatch = %ld too large for one launch", who, (long)nbatch);
  const int ng = K * K, nr = K * nrhs;
  std::vector<int64_t> tab((size_t)nbatch * (ng + nr));
  for (long s = 0; s < nbatch; ++s) {
    for (int q = 0; q < ng; ++q) {
      SVS_REQUIRE(gram_off[s * ng + q] >= 0, "%s: negative offset (system %ld)", who, s);
      tab[s * (ng + nr) + q] = gram_off[s * ng + q];
    }
    for (int q = 0; q < nr; ++q) {
      SVS_REQUIRE(rhs_off[s * nr + q] >= 0, "%s: negative offset (system %ld)", who, s);
      tab[s * (ng + nr) + ng + q] = rhs_off[s * nr + q];
    }
  }
  if (!ws || ws_bytes < solve_batched_ws_bytes(max_refs, nbatch, K, flen, nrhs)) {
    svs_set_error("%s: workspace too small", who);
    return SVS_ERR_WORKSPACE;
  }
  SolveArgs a{};
  a.corr = corr; a.K = K; a.flen = flen; a.nrhs = nrhs; a.status = status; a.ynorm2 = ynorm2;
  solve_dims(K, flen, nrhs, a.np, a.rows);
  a.tab = (const int64_t*)ws;
  a.M = (double*)((char*)ws + solve_table_bytes(nbatch, K, nrhs));
  a.mstride = (long)a.rows * a.np;
  // from pageable memory: the runtime has staged `tab` by the time the copy call returns
  SVS_HIP(hipMemcpyAsync((void*)a.tab, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
  if (made) *made = a;
  return solve_launch(a, skipped, nbatch, rank, stream);
}

}  // namespace

extern "C" size_t svs_bss_corr_windows_workspace_bytes(int64_t window, int64_t nwin, int npairs, const int* pairs) {
  if (window < 1 || nwin < 1 || !pairs_valid(npairs, pairs) || (window + BSS_T - 1) / BSS_T >= (1L << 31)) return 0;
  const int runs = count_runs(npairs, pairs);
  const long gx = corr_blocks(window, runs, nwin), rblocks = svs_cdiv((long)runs * BSS_RUN, BSS_THREADS);
  if (nwin > BSS_MAX_GRID / gx || nwin > BSS_MAX_GRID / rblocks) return 0;
  return (size_t)nwin * gx * runs * BSS_RUN * sizeof(double);
}

extern "C" int svs_bss_corr_windows(const double* x, int64_t ld, int nsig, int64_t n, int64_t window, int64_t hop,
                                    int64_t nwin, const int* pairs, int npairs, double* out, int64_t out_stride, void* ws,
                                    size_t ws_bytes, hipStream_t stream) {
  const int rc = corr_check("svs_bss_corr_windows", SVS_BSS_MAX_SIGNALS, SVS_BSS_MAX_PAIRS, x, ld, nsig, n, window, hop, nwin,
                            pairs, npairs, out, out_stride);
  if (rc != SVS_OK) return rc;
  const size_t need = svs_bss_corr_windows_workspace_bytes(window, nwin, npairs, pairs);
  SVS_REQUIRE(need > 0, "svs_bss_corr_windows: %ld windows of %ld samples do not fit one launch", (long)nwin, (long)window);
  if (!ws || ws_bytes < need) {
    svs_set_error("svs_bss_corr_windows: workspace too small");
    return SVS_ERR_WORKSPACE;
  }
  CorrArgs a{};
  a.x = x; a.ld = ld; a.n = n; a.nsig = nsig; a.npairs = npairs; a.out = out; a.slab = (double*)ws;
  for (int q = 0, off = 0; q < npairs; ++q) {
    a.px[q] = pairs[3 * q]; a.py[q] = pairs[3 * q + 1]; a.nl[q] = pairs[3 * q + 2]; a.off[q] = off; a.run0[q] = a.runs;
    off += a.nl[q];
    a.runs += (a.nl[q] + BSS_RUN - 1) / BSS_RUN;
  }
  a.run0[npairs] = a.runs;
  a.hop = hop; a.window = window; a.out_stride = out_stride;
  a.chunks = (int)((window + BSS_T - 1) / BSS_T);
  a.gx = corr_blocks(window, a.runs, nwin);
  a.rblocks = svs_cdiv((long)a.runs * BSS_RUN, BSS_THREADS);
  return corr_launch(a, nwin, stream);
}

// The whole-signal correlation is the one-window call: the same launch geometry (corr_blocks(n, runs, 1), window base 0),
// the same bits.
extern "C" size_t svs_bss_corr_workspace_bytes(int64_t n, int npairs, const int* pairs) {
  return svs_bss_corr_windows_workspace_bytes(n, 1, npairs, pairs);
}

extern "C" int svs_bss_corr(const double* x, int64_t ld, int nsig, int64_t n, const int* pairs, int npairs, double* out,
                            void* ws, size_t ws_bytes, hipStream_t stream) {
  int64_t lags = 0;
  if (pairs && npairs >= 1 && npairs <= SVS_BSS_MAX_PAIRS)
    for (int q = 0; q < npairs; ++q) lags += pairs[3 * q + 2];
  return svs_bss_corr_windows(x, ld, nsig, n, n, n, 1, pairs, npairs, out, lags, ws, ws_bytes, stream);
}

// the bytes of one system's matrix [G; D^T] (K <= 2)
extern "C" size_t svs_bss_solve_workspace_bytes(int K, int flen, int nrhs) {
  if (!solve_shape_valid(2, K, flen, nrhs)) return 0;
  int np, rows;
  solve_dims(K, flen, nrhs, np, rows);
  return (size_t)rows * np * sizeof(double);
}

// one system with its offsets in the kernel arguments: no table, no host-to-device copy
extern "C" int svs_bss_solve(const double* corr, int K, int flen, const int* gram_off, const int* rhs_off, int nrhs,
                             double* ynorm2, int* status, void* ws, size_t ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(corr && gram_off && rhs_off && ynorm2 && status && solve_shape_valid(2, K, flen, nrhs),
              "svs_bss_solve: bad arguments");
  SolveArgs a{};
  a.corr = corr; a.K = K; a.flen = flen; a.nrhs = nrhs; a.M = (double*)ws; a.status = status; a.ynorm2 = ynorm2;
  for (int q = 0; q < K * K; ++q) {
    SVS_REQUIRE(gram_off[q] >= 0, "svs_bss_solve: negative offset");
    a.goff[q] = gram_off[q];
  }
  for (int q = 0; q < K * nrhs; ++q) {
    SVS_REQUIRE(rhs_off[q] >= 0, "svs_bss_solve: negative offset");
    a.roff[q] = rhs_off[q];
  }
  solve_dims(K, flen, nrhs, a.np, a.rows);
  if (!ws || ws_bytes < svs_bss_solve_workspace_bytes(K, flen, nrhs)) {
    svs_set_error("svs_bss_solve: workspace too small");
    return SVS_ERR_WORKSPACE;
  }
  return solve_launch(a, nullptr, 1, false, stream);
}

extern "C" size_t svs_bss_solve_batched_workspace_bytes(int64_t nbatch, int K, int flen, int nrhs) {
  return solve_batched_ws_bytes(2, nbatch, K, flen, nrhs);
}

extern "C" int svs_bss_solve_batched(const double* corr, int64_t nbatch, int K, int flen, const int64_t* gram_off,
                                     const int64_t* rhs_off, int nrhs, double* ynorm2, int* status, void* ws,
                                     size_t ws_bytes, hipStream_t stream) {
  return solve_batched("svs_bss_solve_batched", 2, false, corr, nbatch, K, flen, gram_off, rhs_off, nrhs, ynorm2, status,
                       nullptr, ws, ws_bytes, stream);
}

// ---- BSS-eval images: stereo stems (evaluate.py: bss_eval_images) ------------------------------
// The correlation at the sizes a stereo two-source problem needs -- 10 signals, about 50 pairs -- with an entry point and
// kernels of its own, and the solve above for up to 4 reference channels (order 2048) under the rank rule:
//   bss_diag_kernel         factors the diagonal tile (k,k) ONCE per system and step and writes the factor back;
//   bss_img_panel_kernel    the panel blocks then only solve X L_kk^T = A against it (bss_panel_kernel's scheme, every block
//                           factoring the tile for itself, measured 9 % slower at order 2048: DESIGN.md section 9).
//   bss_img_corr_kernel     the sweep of bss_corr_kernel.  The pair table no longer fits the kernel arguments, so it lives in
//                           device memory at the head of the workspace, one int4 per thread slot.  The host packs whole
//                           pairs into groups of 256 slots (blockIdx.y) that touch at most SVS_BSS_MAX_SIGNALS signals, and a
//                           block stages only its group's signals: the LDS stays at the 83 KB of the kernel above and two
//                           blocks share a CU, whatever the number of signals.
//   bss_img_reduce_kernel   the fixed-order sum over blocks, one thread per (slot, lag of its run).
// Rank rule (img_factor_tile): stereo images make G singular as a rule (L == R, a silent channel).  With
// thr = order * 2^-52 * max diag G (LAPACK dpstrf's tolerance), a pivot d <= thr with |d| <= thr marks a delayed channel that
// depends on the earlier columns: its column of L and its y component are zero, so |y|^2 is the energy of the projection on
// the span of the remaining columns -- the same span.  A pivot below -thr (or NaN) is a failure: status = 1 + its index; the
// column is zeroed as well, so nothing faults.  skipped[s] counts the skipped columns of system s.

namespace {

struct ImgCorrArgs {
  const double* x; long ld; long n;
  const int4* slots;      // [ngroups * 256]: {x slot | y slot << 8 in the group's staging, k0, offset of lag k0 in a window's
                          //                   output, lags of the run that exist (0: idle slot)}
  const int* gsig;        // [ngroups * 8]: number of staged signals, then their rows
  double* slab; double* out;
  long hop, window, out_stride; int chunks, gx, ngroups;
};

__global__ __launch_bounds__(BSS_THREADS) void bss_img_corr_kernel(ImgCorrArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sig[];      // [<= SVS_BSS_MAX_SIGNALS][BSS_PADLEN]
  const int tid = threadIdx.x, g = blockIdx.y;
  const int4 slot = a.slots[g * BSS_THREADS + tid];
  const bool active = slot.w > 0;
  const int k0 = slot.y;
  const double* X = sig + (slot.x & 0xff) * BSS_PADLEN;
  const double* Y = sig + (slot.x >> 8) * BSS_PADLEN;
  const int nstage = a.gsig[g * 8];
  const int w = blockIdx.x / a.gx, bx = blockIdx.x % a.gx;
  const long base = (long)w * a.hop;
  const long nw = a.n - base < a.window ? a.n - base : a.window;
  double acc[BSS_RUN];
#pragma unroll
  for (int j = 0; j < BSS_RUN; ++j) acc[j] = 0.0;
  for (int c = bx; c < a.chunks; c += a.gx) {
    const long m0 = (long)c * BSS_T;
    __syncthreads();
    for (int s = 0; s < nstage; ++s) {
      const double* src = a.x + (long)a.gsig[g * 8 + 1 + s] * a.ld + base;
      for (int i = tid; i < BSS_STAGE; i += BSS_THREADS) {
        const long gi = m0 + i;
        sig[s * BSS_PADLEN + pidx(i)] = gi < nw ? src[gi] : 0.0;
      }
    }
    __syncthreads();
    if (active) {
      corr_sweep(X, Y, k0, acc);
    }
  }
  if (active) {
    double* dst = a.slab + ((((long)w * a.gx + bx) * a.ngroups + g) * BSS_THREADS + tid) * BSS_RUN;
#pragma unroll
    for (int j = 0; j < BSS_RUN; ++j) dst[j] = acc[j];
  }
}

// grid: nwin * ngroups * BSS_RUN blocks; thread l of a window is lag l % 8 of slot l / 8
__global__ __launch_bounds__(BSS_THREADS) void bss_img_reduce_kernel(ImgCorrArgs a) {
  const int per = a.ngroups * BSS_RUN;
  const int w = blockIdx.x / per;
  const int l = (blockIdx.x % per) * BSS_THREADS + threadIdx.x;
  const int4 slot = a.slots[l / BSS_RUN];
  const int j = l % BSS_RUN;
  if (j >= slot.w) return;
  const long stride = (long)a.ngroups * BSS_THREADS * BSS_RUN;
  const double* slab = a.slab + (long)w * a.gx * stride;
  double s = 0.0;
  for (int b = 0; b < a.gx; ++b) s += slab[b * stride + l];
  a.out[(long)w * a.out_stride + slot.z + j] = s;
}

struct ImgCorrPlan {
  int ngroups = 0;
  std::vector<int> slots, gsig;      // the device table: slots (4 ints per slot), then gsig
};

bool img_pairs_valid(int npairs, const int* pairs) {
  if (npairs < 1 || npairs > SVS_BSS_IMG_MAX_PAIRS || !pairs) return false;
  for (int q = 0; q < npairs; ++q)
    if (pairs[3 * q] < 0 || pairs[3 * q] >= SVS_BSS_IMG_MAX_SIGNALS || pairs[3 * q + 1] < 0 ||
        pairs[3 * q + 1] >= SVS_BSS_IMG_MAX_SIGNALS || pairs[3 * q + 2] < 1 || pairs[3 * q + 2] > SVS_BSS_MAX_LAG)
      return false;
  return true;
}

// Packs whole pairs into groups of at most 256 runs and SVS_BSS_MAX_SIGNALS distinct signals: a group takes the first
// pair that is left, then, while one fits, the pair that adds the fewest new signals (the first of those).  pairs valid.
ImgCorrPlan img_corr_plan(int npairs, const int* pairs) {
  ImgCorrPlan p;
  std::vector<int> off(npairs);
  for (int q = 0, lags = 0; q < npairs; ++q) { off[q] = lags; lags += pairs[3 * q + 2]; }
  std::vector<bool> done(npairs, false);
  for (int left = npairs; left > 0;) {
    int staged[SVS_BSS_MAX_SIGNALS], nstaged = 0, used = 0;
    auto slot_of = [&](int s) { for (int i = 0; i < nstaged; ++i) if (staged[i] == s) return i; return -1; };
    p.slots.resize((size_t)(p.ngroups + 1) * BSS_THREADS * 4, 0);
    for (;;) {
      int best = -1, best_new = 3;
      for (int q = 0; q < npairs; ++q) {
        if (done[q] || used + (pairs[3 * q + 2] + BSS_RUN - 1) / BSS_RUN > BSS_THREADS) continue;
        const int a = pairs[3 * q], b = pairs[3 * q + 1];
        const int add = (slot_of(a) < 0) + (b != a && slot_of(b) < 0);
        if (nstaged + add <= SVS_BSS_MAX_SIGNALS && add < best_new) { best = q; best_new = add; }
      }
      if (best < 0) break;
      const int a = pairs[3 * best], b = pairs[3 * best + 1], nl = pairs[3 * best + 2];
      if (slot_of(a) < 0) staged[nstaged++] = a;
      if (slot_of(b) < 0) staged[nstaged++] = b;
      for (int k0 = 0; k0 < nl; k0 += BSS_RUN, ++used) {
        int* s = &p.slots[((size_t)p.ngroups * BSS_THREADS + used) * 4];
        s[0] = slot_of(a) | slot_of(b) << 8; s[1] = k0; s[2] = off[best] + k0; s[3] = std::min(BSS_RUN, nl - k0);
      }
      done[best] = true;
      --left;
    }
    p.gsig.push_back(nstaged);
    for (int i = 0; i < 7; ++i) p.gsig.push_back(i < nstaged ? staged[i] : 0);
    ++p.ngroups;
  }
  return p;
}

size_t img_corr_table_bytes(int ngroups) {
  return svs_align_up((size_t)ngroups * (BSS_THREADS * 4 + 8) * sizeof(int), 256);
}

long img_corr_blocks(long window, int ngroups, long nwin) {
  const long chunks = (window + BSS_T - 1) / BSS_T;
  return std::min<long>(chunks, std::max<long>(1, BSS_MAX_BLOCKS / (ngroups * nwin)));
}

// 0: the arguments are invalid or the grid is too wide for one launch
size_t img_corr_ws_bytes(long window, long nwin, const ImgCorrPlan& p) {
  if (window < 1 || nwin < 1 || (window + BSS_T - 1) / BSS_T >= (1L << 31)) return 0;
  const long gx = img_corr_blocks(window, p.ngroups, nwin);
  if (nwin > BSS_MAX_GRID / gx || nwin > BSS_MAX_GRID / (p.ngroups * BSS_RUN)) return 0;
  return img_corr_table_bytes(p.ngroups) + (size_t)nwin * gx * p.ngroups * BSS_THREADS * BSS_RUN * sizeof(double);
}

}  // namespace

extern "C" size_t svs_bss_img_corr_windows_workspace_bytes(int64_t window, int64_t nwin, int npairs, const int* pairs) {
  if (!img_pairs_valid(npairs, pairs)) return 0;
  return img_corr_ws_bytes(window, nwin, img_corr_plan(npairs, pairs));
}

extern "C" int svs_bss_img_corr_windows(const double* x, int64_t ld, int nsig, int64_t n, int64_t window, int64_t hop,
                                        int64_t nwin, const int* pairs, int npairs, double* out, int64_t out_stride,
                                        void* ws, size_t ws_bytes, hipStream_t stream) {
  const int rc = corr_check("svs_bss_img_corr_windows", SVS_BSS_IMG_MAX_SIGNALS, SVS_BSS_IMG_MAX_PAIRS, x, ld, nsig, n, window,
                            hop, nwin, pairs, npairs, out, out_stride);
  if (rc != SVS_OK) return rc;
  const ImgCorrPlan p = img_corr_plan(npairs, pairs);
  const size_t need = img_corr_ws_bytes(window, nwin, p);
  SVS_REQUIRE(need > 0, "svs_bss_img_corr_windows: %ld windows of %ld samples do not fit one launch", (long)nwin,
              (long)window);
  if (!ws || ws_bytes < need) {
    svs_set_error("svs_bss_img_corr_windows: workspace too small");
    return SVS_ERR_WORKSPACE;
  }
  ImgCorrArgs a{};
  a.x = x; a.ld = ld; a.n = n; a.out = out; a.hop = hop; a.window = window; a.out_stride = out_stride;
  a.ngroups = p.ngroups;
  a.chunks = (int)((window + BSS_T - 1) / BSS_T);
  a.gx = (int)img_corr_blocks(window, p.ngroups, nwin);
  a.slots = (const int4*)ws;
  a.gsig = (const int*)ws + (size_t)p.ngroups * BSS_THREADS * 4;
  a.slab = (double*)((char*)ws + img_corr_table_bytes(p.ngroups));
  // from pageable memory: the runtime has staged the tables by the time the copy calls return
  SVS_HIP(hipMemcpyAsync((void*)a.slots, p.slots.data(), p.slots.size() * sizeof(int), hipMemcpyHostToDevice, stream));
  SVS_HIP(hipMemcpyAsync((void*)a.gsig, p.gsig.data(), p.gsig.size() * sizeof(int), hipMemcpyHostToDevice, stream));
  const int lds = SVS_BSS_MAX_SIGNALS * BSS_PADLEN * (int)sizeof(double);
  SVS_HIP(hipFuncSetAttribute((const void*)bss_img_corr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL(bss_img_corr_kernel, dim3((unsigned)(nwin * a.gx), p.ngroups), dim3(BSS_THREADS), lds, stream, a);
  SVS_CHECK_LAUNCH("bss_img_corr");
  hipLaunchKernelGGL(bss_img_reduce_kernel, dim3((unsigned)(nwin * p.ngroups * BSS_RUN)), dim3(BSS_THREADS), 0, stream, a);
  SVS_CHECK_LAUNCH("bss_img_reduce");
  return SVS_OK;
}

extern "C" size_t svs_bss_img_solve_batched_workspace_bytes(int64_t nbatch, int K, int flen, int nrhs) {
  return solve_batched_ws_bytes(SVS_BSS_IMG_MAX_REFS, nbatch, K, flen, nrhs);
}

extern "C" int svs_bss_img_solve_batched(const double* corr, int64_t nbatch, int K, int flen, const int64_t* gram_off,
                                         const int64_t* rhs_off, int nrhs, double* ynorm2, int* status, int* skipped,
                                         void* ws, size_t ws_bytes, hipStream_t stream) {
  return solve_batched("svs_bss_img_solve_batched", SVS_BSS_IMG_MAX_REFS, true, corr, nbatch, K, flen, gram_off, rhs_off, nrhs,
                       ynorm2, status, skipped, ws, ws_bytes, stream);
}

// ---- BSS-eval v4: the filter coefficients (evaluate.py: bss_eval_v4) ---------------------------
// v4 applies filters estimated once per track to every frame (csrc/bss_v4.hip), so it needs the coefficients c = G^-1 D
// themselves, not only |y|^2.  After the launches of the image solve the workspace holds L (tile (k,k) factored in place by
// bss_diag_kernel, the tiles below it by bss_img_panel_kernel) and, in the rows under it, y^T.  The back substitution
// L^T c = y mirrors the forward direction in 64-column steps, from the last step to the first:
//   bss_back_diag_kernel    one block per system: c_k = L_kk^-T y_k for every right-hand side, in place and into coef;
//   bss_back_update_kernel  one block per (system, tile j < k): y_j -= L_kj^T c_k.
// A column that the rank rule skipped has the pivot 0, a zero column of L and y = 0: its coefficient is 0 (no division),
// which is the solution on the span of the remaining columns.  The identity padding has y = 0 and gives c = 0.

namespace {

__global__ __launch_bounds__(BSS_THREADS) void bss_back_diag_kernel(SolveArgs a, double* coef, int k) {
  __shared__ double L[NB][NB + 1];
  __shared__ double Y[SVS_BSS_MAX_RHS][NB + 1];
  const int s = blockIdx.x, tid = threadIdx.x, kf = a.K * a.flen;
  const long ld = a.np;
  double* M = a.M + s * a.mstride;
  const double* dk = M + (long)k * NB * ld + (long)k * NB;
  double* yk = M + (long)a.np * ld + (long)k * NB;
  for (int e = tid; e < NB * NB; e += BSS_THREADS) L[e / NB][e % NB] = dk[(e / NB) * ld + e % NB];
  for (int e = tid; e < a.nrhs * NB; e += BSS_THREADS) Y[e / NB][e % NB] = yk[(e / NB) * ld + e % NB];
  __syncthreads();
  for (int c = NB - 1; c >= 0; --c) {
    const double piv = L[c][c];
    if (tid < a.nrhs) Y[tid][c] = piv != 0.0 ? Y[tid][c] / piv : 0.0;
    __syncthreads();
    for (int e = tid; e < a.nrhs * NB; e += BSS_THREADS) {
      const int r = e / NB, q = e % NB;
      if (q < c) Y[r][q] -= L[c][q] * Y[r][c];
    }
    __syncthreads();
  }
  for (int e = tid; e < a.nrhs * NB; e += BSS_THREADS) {
    const int r = e / NB, q = e % NB, col = k * NB + q;
    yk[r * ld + q] = Y[r][q];
    if (col < kf) coef[((long)s * a.nrhs + r) * kf + col] = Y[r][q];
  }
}

__global__ __launch_bounds__(BSS_THREADS) void bss_back_update_kernel(SolveArgs a, int k) {
  __shared__ double L[NB][NB + 1];                   // tile (k, j): [p][q]
  __shared__ double Ck[SVS_BSS_MAX_RHS][NB];
  const int s = blockIdx.x / k, j = blockIdx.x % k, tid = threadIdx.x;
  const long ld = a.np;
  double* M = a.M + s * a.mstride;
  const double* lkj = M + (long)k * NB * ld + (long)j * NB;
  const double* ck = M + (long)a.np * ld + (long)k * NB;
  double* yj = M + (long)a.np * ld + (long)j * NB;
  for (int e = tid; e < NB * NB; e += BSS_THREADS) L[e / NB][e % NB] = lkj[(e / NB) * ld + e % NB];
  for (int e = tid; e < a.nrhs * NB; e += BSS_THREADS) Ck[e / NB][e % NB] = ck[(e / NB) * ld + e % NB];
  __syncthreads();
  for (int e = tid; e < a.nrhs * NB; e += BSS_THREADS) {
    const int r = e / NB, q = e % NB;
    double acc = 0.0;
    for (int p = 0; p < NB; ++p) acc = fma(L[p][q], Ck[r][p], acc);
    yj[r * ld + q] -= acc;
  }
}

}  // namespace

extern "C" size_t svs_bss_img_filters_batched_workspace_bytes(int64_t nbatch, int K, int flen, int nrhs) {
  return solve_batched_ws_bytes(SVS_BSS_IMG_MAX_REFS, nbatch, K, flen, nrhs);
}

extern "C" int svs_bss_img_filters_batched(const double* corr, int64_t nbatch, int K, int flen, const int64_t* gram_off,
                                           const int64_t* rhs_off, int nrhs, double* ynorm2, int* status, int* skipped,
                                           double* coef, void* ws, size_t ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(coef, "svs_bss_img_filters_batched: bad arguments");
  SolveArgs a{};
  const int rc = solve_batched("svs_bss_img_filters_batched", SVS_BSS_IMG_MAX_REFS, true, corr, nbatch, K, flen, gram_off,
                               rhs_off, nrhs, ynorm2, status, skipped, ws, ws_bytes, stream, &a);
  if (rc != SVS_OK) return rc;
  for (int k = a.np / NB - 1; k >= 0; --k) {
    hipLaunchKernelGGL(bss_back_diag_kernel, dim3((unsigned)nbatch), dim3(BSS_THREADS), 0, stream, a, coef, k);
    SVS_CHECK_LAUNCH("bss_back_diag");
    if (k > 0) {
      hipLaunchKernelGGL(bss_back_update_kernel, dim3((unsigned)(nbatch * k)), dim3(BSS_THREADS), 0, stream, a, k);
      SVS_CHECK_LAUNCH("bss_back_update");
    }
  }
  return SVS_OK;
}
