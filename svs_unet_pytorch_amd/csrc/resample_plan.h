// What the polyphase kernels share (csrc/resample.hip, csrc/fullband.hip): the sample formats and their conversion, the filter rule
// and the block plan -- one definition, so that a kernel built on them walks the outputs, stages the inputs and sums the taps in the
// order svs_resample_poly does.
#pragma once
#include "common.h"

namespace {

enum { RS_F32 = 0, RS_I16 = 1, RS_I32 = 2 };
constexpr int RS_THREADS = 256;
constexpr size_t RS_LDS_FOUR_BLOCKS = 40 * 1024;     // four blocks (16 waves) per CU: measured 1.4x faster than two blocks of twice the rows
constexpr size_t RS_LDS_MAX = 160 * 1024;

struct RsPlan {
  int W;            // outputs per segment (= tap rows a block owns when up > 256)
  int Wt;           // tap rows in LDS
  int S;            // segments per step
  int nqb;          // blocks along q
  int span;         // input samples staged per segment
  int64_t stride;   // distance in outputs between the starts of consecutive segments
  int64_t nsteps;   // steps that cover n_out
  int ipc;          // steps per block
  int chunks;       // blocks along the steps
  int64_t dq, dr;   // (S * stride * down) / up and % up: what one step adds to (n0, pos % up)
  size_t lds;
};

static inline int rs_taps_per_phase(int ntaps, int up) { return (ntaps + up - 1) / up; }

// nch: input rows a block stages per segment (1: resample_poly_kernel; the channel count: resample_encode_kernel; the stems and y:
// fullband_mix_kernel)
static size_t rs_lds_bytes(int Wt, int W, int S, int T, int up, int down, int nch, int* span) {
  *span = (int)(((int64_t)(W - 1) * down) / up) + T + 2;
  return ((size_t)Wt * T + (size_t)S * nch * *span) * sizeof(float);
}

// false: no block shape fits the LDS (the filter is too long for this kernel: about down / up > 90)
static bool rs_plan(int64_t n_out, int T, int up, int down, int rows, int nch, RsPlan* p) {
  bool ok = false;
  if (up <= RS_THREADS) {
    p->W = RS_THREADS / up * up; p->Wt = up; p->S = 1; p->nqb = 1; p->stride = p->W;
    // a long filter over few phases: shorter segments (still whole periods) leave room for the taps
    for (; p->W >= up; p->W = (p->W / up / 2) * up) {
      p->stride = p->W;
      p->lds = rs_lds_bytes(p->Wt, p->W, 1, T, up, down, nch, &p->span);
      if (p->lds <= RS_LDS_MAX) { ok = true; break; }
      if (p->W == up) break;
    }
  } else {
    for (int pass = 0; pass < 2 && !ok; ++pass)
      for (int W = RS_THREADS; W >= 16 && !ok; W >>= 1) {
        p->W = p->Wt = W; p->S = RS_THREADS / W;
        p->lds = rs_lds_bytes(W, W, p->S, T, up, down, nch, &p->span);
        ok = p->lds <= (pass ? RS_LDS_MAX : RS_LDS_FOUR_BLOCKS);
      }
    p->nqb = (up + p->W - 1) / p->W; p->stride = up;
  }
  if (!ok) return false;
  const int64_t per_step = p->S * p->stride;                         // outputs (of all q) one step advances
  p->nsteps = (n_out + per_step - 1) / per_step;
  int64_t chunks = 1024 / ((int64_t)p->nqb * rows);                  // about four blocks per CU in all
  if (chunks < 1) chunks = 1;
  if (chunks > p->nsteps) chunks = p->nsteps;
  p->ipc = (int)((p->nsteps + chunks - 1) / chunks);
  p->chunks = (int)((p->nsteps + p->ipc - 1) / p->ipc);
  const int64_t dpos = per_step * down;
  p->dq = dpos / up; p->dr = dpos % up;
  return true;
}

// one stored sample as fp32: int16 / 32768, int32 / 2^31 (the int -> float conversion rounds to nearest even), float32 as it is
__device__ __forceinline__ float rs_cvt(const void* x, int fmt, int64_t e) {
  if (fmt == RS_I16) return (float)((const int16_t*)x)[e] * (1.0f / 32768.0f);
  if (fmt == RS_I32) return (float)((const int32_t*)x)[e] * (1.0f / 2147483648.0f);
  return ((const float*)x)[e];
}

static inline bool rs_filter_ok(int ntaps, int up, int down) {
  return up >= 1 && down >= 1 && ntaps >= 1 && (ntaps & 1) && up <= (1 << 24) && down <= (1 << 24);
}

}  // namespace
