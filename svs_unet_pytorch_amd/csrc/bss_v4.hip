// BSS-eval v4 on the GPU (svs_unet_pytorch_amd/evaluate.py: bss_eval_v4), fp64 throughout, gfx950: the distortion filters come
// from the whole track (svs_bss_img_filters_batched, csrc/bss.hip) and are applied to every frame's references.  The Gram form
// of bss.hip does not reach this: the figures need energies of DIFFERENCES of projected signals inside a frame, where the
// spans are no longer nested, so the projected signals themselves are formed -- and never stored:
//   bss_project_kernel         block = (frame w, source j, tile of PRJ_T outputs m).  It stages the tile's samples of every
//                              reference row, with a lead of flen - 1 (rounded up to a whole chunk of taps) before it, in LDS as
//                              doubles: zero before the frame's start, past its end and past n.  The rows of source j come
//                              first.  A lane owns PRJ_R consecutive outputs of every estimate channel c and slides a
//                              register window of each staged row over the taps:
//                                p1_c[m] += C_j[c][i, tau] r_i[m - tau]   (rows of source j)
//                                pa_c[m] += C_all[c][i, tau] r_i[m - tau] (all rows)
//                              so one 8-byte LDS read feeds 4 PRJ_R FMAs (two channels, p1 and pa) on a row of source j and
//                              2 PRJ_R on another row.  PRJ_R is odd: the lanes' reads, PRJ_R doubles apart, fall on distinct
//                              banks within a half-wave.  The coefficients depend on (j, c, i, tau) only: wave-uniform, read
//                              through the scalar cache.  After the last tap the lane forms the seven sums of its outputs
//                                S0 s^2, S1 (e-s)^2, S2 (p1-s)^2, S3 p1^2, S4 (pa-p1)^2, S5 pa^2, S6 (e-pa)^2
//                              over m < L + flen - 1 (L: the frame's length; the flen - 1 tail is part of the frame) and both
//                              channels; the block adds them in a fixed tree and writes one partial per (block, sum).
//   bss_project_reduce_kernel  sums the partials of a (frame, source) over its tiles in ascending order: no atomics, bitwise
//                              reproducible.
#include <algorithm>

#include "common.h"

namespace {

constexpr int PRJ_THREADS = 256;
constexpr int PRJ_R = 5;                             // outputs per lane (odd: see above)
constexpr int PRJ_T = PRJ_THREADS * PRJ_R;           // outputs per block
constexpr int PRJ_SUMS = 7;
constexpr long PRJ_MAX_GRID = 0xffffffffL / PRJ_THREADS;   // blocks in one grid dimension (its work-items must fit 32 bits)

struct ProjArgs {
  const double* x; long ld, n, window, hop;
  int flen, chunks, ntiles;                          // chunks = ceil(flen / PRJ_R); tiles per (frame, source)
  int ref_rows[SVS_BSS_IMG_MAX_REFS], est_rows[SVS_BSS_IMG_MAX_REFS];
  const double* coef_one; const double* coef_all;
  double* part; double* sums; long groups;           // groups = nwin * nsrc
};

// PRJ_R taps tau0 .. tau0 + PRJ_R - 1 of every staged row.  hi[k][q] = S_k[o + lead - tau0 + q] on entry; on exit the same for
// tau0 + PRJ_R.  GUARD: taps >= flen (the last chunk of a flen that PRJ_R does not divide) have the coefficient 0.
template <int NCH, int NR, bool GUARD>
__device__ __forceinline__ void project_chunk(const double* stage, int slen, int at, int tau0, int flen, const double* c1,
                                              const double* ca, const int (&pos)[NR], double (&hi)[NR][PRJ_R],
                                              double (&p1)[NCH][PRJ_R], double (&pa)[NCH][PRJ_R]) {
  double lo[NR][PRJ_R];                              // S_k[at - PRJ_R + q]: the samples the window slides onto
#pragma unroll
  for (int k = 0; k < NR; ++k)
#pragma unroll
    for (int q = 0; q < PRJ_R; ++q) lo[k][q] = stage[k * slen + at - PRJ_R + q];
#pragma unroll
  for (int u = 0; u < PRJ_R; ++u) {
    const int tau = tau0 + u;
    if (GUARD && tau >= flen) break;                 // uniform
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      double wa[NCH], w1[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        wa[c] = ca[((long)c * NR + pos[k]) * flen + tau];
        w1[c] = k < NCH ? c1[((long)c * NCH + k) * flen + tau] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < PRJ_R; ++q) {
        const double v = q >= u ? hi[k][q - u] : lo[k][PRJ_R + q - u];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          pa[c][q] = fma(wa[c], v, pa[c][q]);
          if (k < NCH) p1[c][q] = fma(w1[c], v, p1[c][q]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NR; ++k)
#pragma unroll
    for (int q = 0; q < PRJ_R; ++q) hi[k][q] = lo[k][q];
}

template <int NCH, int NSRC>
__global__ __launch_bounds__(PRJ_THREADS) void bss_project_kernel(ProjArgs a) {
  constexpr int NR = NCH * NSRC;
  extern __shared__ __attribute__((aligned(16))) double stage[];    // [NR][slen]
  __shared__ double red[PRJ_THREADS / 64][PRJ_SUMS];
  const int tid = threadIdx.x;
  const int lead = a.chunks * PRJ_R, slen = PRJ_T + lead;
  const int t = (int)(blockIdx.x % a.ntiles);
  const long wj = blockIdx.x / a.ntiles;
  const int j = (int)(wj % NSRC);
  const long base = (wj / NSRC) * a.hop;
  const long L = a.n - base < a.window ? a.n - base : a.window;     // samples of the frame that exist
  const long m0 = (long)t * PRJ_T;
  int pos[NR];                                       // staged row k is reference pos[k] of the NR: source j's first
#pragma unroll
  for (int k = 0; k < NR; ++k) pos[k] = k < NCH ? j * NCH + k : (1 - j) * NCH + (k - NCH);
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const double* src = a.x + (long)a.ref_rows[pos[k]] * a.ld + base;
    for (int i = tid; i < slen; i += PRJ_THREADS) {
      const long g = m0 - lead + i;
      stage[k * slen + i] = g >= 0 && g < L ? src[g] : 0.0;
    }
  }
  __syncthreads();
  const double* c1 = a.coef_one + (long)j * NCH * NCH * a.flen;     // [c][i][tau], i over the channels of source j
  const double* ca = a.coef_all + (long)j * NCH * NR * a.flen;      // [c][i][tau], i over all NR reference channels
  const int o = tid * PRJ_R;
  double p1[NCH][PRJ_R] = {}, pa[NCH][PRJ_R] = {}, hi[NR][PRJ_R];
#pragma unroll
  for (int k = 0; k < NR; ++k)
#pragma unroll
    for (int q = 0; q < PRJ_R; ++q) hi[k][q] = stage[k * slen + o + lead + q];
  const int whole = a.flen / PRJ_R;
  for (int ch = 0; ch < whole; ++ch)
    project_chunk<NCH, NR, false>(stage, slen, o + lead - ch * PRJ_R, ch * PRJ_R, a.flen, c1, ca, pos, hi, p1, pa);
  if (whole < a.chunks)
    project_chunk<NCH, NR, true>(stage, slen, o + lead - whole * PRJ_R, whole * PRJ_R, a.flen, c1, ca, pos, hi, p1, pa);
  double S[PRJ_SUMS] = {};
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const double* sr = a.x + (long)a.ref_rows[j * NCH + c] * a.ld + base;
    const double* er = a.x + (long)a.est_rows[j * NCH + c] * a.ld + base;
#pragma unroll
    for (int q = 0; q < PRJ_R; ++q) {
      const long m = m0 + o + q;
      if (m >= L + a.flen - 1) continue;
      const double s = m < L ? sr[m] : 0.0, e = m < L ? er[m] : 0.0, d1 = p1[c][q], da = pa[c][q];
      S[0] = fma(s, s, S[0]);
      S[1] = fma(e - s, e - s, S[1]);
      S[2] = fma(d1 - s, d1 - s, S[2]);
      S[3] = fma(d1, d1, S[3]);
      S[4] = fma(da - d1, da - d1, S[4]);
      S[5] = fma(da, da, S[5]);
      S[6] = fma(e - da, e - da, S[6]);
    }
  }
#pragma unroll
  for (int i = 0; i < PRJ_SUMS; ++i) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) S[i] += __shfl_down(S[i], d, 64);
  }
  if (tid % 64 == 0)
#pragma unroll
    for (int i = 0; i < PRJ_SUMS; ++i) red[tid / 64][i] = S[i];
  __syncthreads();
  if (tid < PRJ_SUMS) {
    double v = red[0][tid];
    for (int wv = 1; wv < PRJ_THREADS / 64; ++wv) v += red[wv][tid];
    a.part[(long)blockIdx.x * PRJ_SUMS + tid] = v;
  }
}

__global__ __launch_bounds__(PRJ_THREADS) void bss_project_reduce_kernel(ProjArgs a) {
  const long g = (long)blockIdx.x * PRJ_THREADS + threadIdx.x;
  if (g >= a.groups * PRJ_SUMS) return;
  const double* p = a.part + g / PRJ_SUMS * a.ntiles * PRJ_SUMS + g % PRJ_SUMS;
  double s = 0.0;
  for (int t = 0; t < a.ntiles; ++t) s += p[(long)t * PRJ_SUMS];
  a.sums[g] = s;
}

bool project_shape_valid(int64_t window, int64_t nwin, int nsrc, int flen) {
  return window >= 1 && nwin >= 1 && (nsrc == 1 || nsrc == 2) && flen >= 1 && flen <= SVS_BSS_MAX_LAG &&
         window <= (1L << 40);
}

long project_tiles(int64_t window, int flen) { return (window + flen - 1 + PRJ_T - 1) / PRJ_T; }

template <int NCH, int NSRC>
int project_launch(const ProjArgs& a, hipStream_t stream) {
  const int lds = NCH * NSRC * (PRJ_T + a.chunks * PRJ_R) * (int)sizeof(double);
  SVS_HIP(hipFuncSetAttribute((const void*)bss_project_kernel<NCH, NSRC>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL((bss_project_kernel<NCH, NSRC>), dim3((unsigned)(a.groups * a.ntiles)), dim3(PRJ_THREADS), lds, stream,
                     a);
  SVS_CHECK_LAUNCH("bss_project");
  hipLaunchKernelGGL(bss_project_reduce_kernel, dim3((unsigned)svs_cdiv(a.groups * PRJ_SUMS, PRJ_THREADS)),
                     dim3(PRJ_THREADS), 0, stream, a);
  SVS_CHECK_LAUNCH("bss_project_reduce");
  return SVS_OK;
}

}  // namespace

// one partial per (frame, source, tile, sum); 0: the arguments are invalid or the grid is too wide for one launch
extern "C" size_t svs_bss_project_frames_workspace_bytes(int64_t window, int64_t nwin, int nsrc, int flen) {
  if (!project_shape_valid(window, nwin, nsrc, flen)) return 0;
  const long ntiles = project_tiles(window, flen);
  if (nwin > PRJ_MAX_GRID / (ntiles * nsrc)) return 0;
  return (size_t)nwin * nsrc * ntiles * PRJ_SUMS * sizeof(double);
}

extern "C" int svs_bss_project_frames(const double* x, int64_t ld, int nsig, int64_t n, int64_t window, int64_t hop,
                                      int64_t nwin, int flen, int nsrc, int nchan, const int* ref_rows, const int* est_rows,
                                      const double* coef_one, const double* coef_all, double* sums, void* ws,
                                      size_t ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(x && ref_rows && est_rows && coef_one && coef_all && sums && n >= 1 && ld >= n && nsig >= 1 &&
              (nchan == 1 || nchan == 2) && project_shape_valid(window, nwin, nsrc, flen), "svs_bss_project_frames: bad arguments");
  SVS_REQUIRE(hop >= 1 && (nwin - 1) <= (n - 1) / hop,
              "svs_bss_project_frames: hop = %ld, nwin = %ld: a frame starts past the %ld samples", (long)hop, (long)nwin,
              (long)n);
  ProjArgs a{};
  for (int q = 0; q < nsrc * nchan; ++q) {
    SVS_REQUIRE(ref_rows[q] >= 0 && ref_rows[q] < nsig && est_rows[q] >= 0 && est_rows[q] < nsig,
                "svs_bss_project_frames: row %d = (%d, %d) out of range", q, ref_rows[q], est_rows[q]);
    a.ref_rows[q] = ref_rows[q];
    a.est_rows[q] = est_rows[q];
  }
  const size_t need = svs_bss_project_frames_workspace_bytes(window, nwin, nsrc, flen);
  SVS_REQUIRE(need > 0, "svs_bss_project_frames: %ld frames of %ld samples do not fit one launch", (long)nwin, (long)window);
  if (!ws || ws_bytes < need) {
    svs_set_error("svs_bss_project_frames: workspace too small");
    return SVS_ERR_WORKSPACE;
  }
  a.x = x; a.ld = ld; a.n = n; a.window = window; a.hop = hop; a.flen = flen;
  a.chunks = (flen + PRJ_R - 1) / PRJ_R;
  a.ntiles = (int)project_tiles(window, flen);
  a.coef_one = coef_one; a.coef_all = coef_all; a.part = (double*)ws; a.sums = sums; a.groups = nwin * nsrc;
  if (nchan == 1) return nsrc == 1 ? project_launch<1, 1>(a, stream) : project_launch<1, 2>(a, stream);
  return nsrc == 1 ? project_launch<2, 1>(a, stream) : project_launch<2, 2>(a, stream);
}
