// Index arithmetic of the 5x5 / stride-2 / pad-2 layers as an implicit GEMM, once, for the kernels and for the host planner.
//
//   MODE = SVS_MODE_GATHER: GEMM row (b, hq, wq) is output pixel (hq, wq); tap (th, tw) of 5 x 5 reads input pixel
//                           (2 hq - 2 + th, 2 wq - 2 + tw).
//   MODE = SVS_MODE_PARITY: class par = 2 ph + pw has (3 - ph) x (3 - pw) taps; row (b, hq, wq) of its Ha x Wa grid is output pixel
//                           (2 hq + ph, 2 wq + pw); tap (th, tw) reads input pixel (hq + 1 - th, wq + 1 - tw).
// A row's "anchor" (h0, w0) is (2 hq, 2 wq) resp. (hq, wq).  MODE is a template argument: nothing here is a run-time branch.
#pragma once
#include "internal.h"

// first tap of parity class 0 .. 3 in the parity packing [class][n][th][tw][c] (9 + 6 + 6 + 4 taps), and their total
constexpr int SVS_CLASS_TAP0[5] = {0, 9, 15, 21, 25};
// class of step s of the 25 taps taken in class order (the window kernels' compile-time walk)
constexpr int svs_step_class(int s) { return s < SVS_CLASS_TAP0[1] ? 0 : s < SVS_CLASS_TAP0[2] ? 1 : s < SVS_CLASS_TAP0[3] ? 2 : 3; }

struct SvsConvClass { int ph, pw, nth, ntw, Ha, Wa, tap0; };      // Ha x Wa: the class's grid of GEMM rows per image
template <int MODE>
__host__ __device__ __forceinline__ SvsConvClass svs_conv_class(int par, int Ho, int Wo) {
  if (MODE != SVS_MODE_PARITY) return {0, 0, 5, 5, Ho, Wo, 0};
  const int ph = par >> 1, pw = par & 1;
  const int tap0 = (par == 0) ? SVS_CLASS_TAP0[0] : (par == 1) ? SVS_CLASS_TAP0[1] : (par == 2) ? SVS_CLASS_TAP0[2] : SVS_CLASS_TAP0[3];
  return {ph, pw, 3 - ph, 3 - pw, (Ho - ph + 1) >> 1, (Wo - pw + 1) >> 1, tap0};
}

// GEMM row m -> (b, hq, wq).  BATCH_INNER = false: rows ordered (b, h, w); true: (w, h, b), the tap-skipping kernels' order.
// 32-bit: M < 2^31 follows from the hosts' 2 GiB view checks (64-bit divisions cost ~100 instructions each).
struct SvsConvRow { int b, hq, wq; };
template <bool BATCH_INNER>
__host__ __device__ __forceinline__ SvsConvRow svs_conv_row(unsigned m, unsigned B, unsigned Ha, unsigned Wa) {
  if (BATCH_INNER) {
    const unsigned pos = m / B, wq = pos / Ha;
    return {(int)(m - pos * B), (int)(pos - wq * Ha), (int)wq};
  }
  const unsigned t = m / Wa, b = t / Ha;
  return {(int)b, (int)(t - b * Ha), (int)(m - t * Wa)};
}

template <int MODE> __host__ __device__ __forceinline__ int svs_conv_anchor(int q) { return MODE == SVS_MODE_GATHER ? 2 * q : q; }
// input coordinate that tap t reads from anchor coordinate x0 (either axis)
template <int MODE> __host__ __device__ __forceinline__ int svs_tap_coord(int x0, int t) { return MODE == SVS_MODE_GATHER ? x0 - 2 + t : x0 + 1 - t; }

// bit th * ntw + tw: tap (th, tw) of the row anchored at (h0, w0) reads inside the H x W image
template <int MODE>
__host__ __device__ __forceinline__ unsigned svs_tap_mask(int h0, int w0, int nth, int ntw, int H, int W) {
  unsigned wbits = 0, mask = 0;                   // taps tw inside the image's columns, then one copy per tap th inside its rows
  for (int tw = 0; tw < ntw; ++tw)
    if ((unsigned)svs_tap_coord<MODE>(w0, tw) < (unsigned)W) wbits |= 1u << tw;
  for (int th = 0; th < nth; ++th)
    if ((unsigned)svs_tap_coord<MODE>(h0, th) < (unsigned)H) mask |= wbits << (th * ntw);
  return mask;
}
__host__ __device__ __forceinline__ int svs_tap_row(int tap, int ntw) { return (ntw == 5) ? tap / 5 : (ntw == 3) ? tap / 3 : tap >> 1; }

// The operand base is moved back by svs_tap_base_shift pixels' worth of elements so that every tap's offset from an anchor,
// svs_tap_pix, is >= 0 (it becomes a scalar buffer offset): GATHER tap (th, tw) reads anchor + (th - 2, tw - 2) =
// [anchor - (2, 2)] + (th, tw); PARITY reads anchor + (1 - th, 1 - tw) = [anchor - (1, 1)] + (2 - th, 2 - tw).
template <int MODE> __host__ __device__ __forceinline__ long svs_tap_base_shift(int W, long ld) { return (MODE == SVS_MODE_GATHER ? 2L * W + 2 : 1L * W + 1) * ld; }
template <int MODE> __host__ __device__ __forceinline__ int svs_tap_pix(int th, int tw, int W) { return MODE == SVS_MODE_GATHER ? th * W + tw : (2 - th) * W + (2 - tw); }

// output pixel index (in an image batch of Ho x Wo) of row (b, hq, wq) of class (ph, pw)
template <int MODE>
__host__ __device__ __forceinline__ long svs_out_pixel(long b, int hq, int wq, int ph, int pw, int Ho, int Wo) {
  return MODE == SVS_MODE_GATHER ? (b * Ho + hq) * Wo + wq : (b * Ho + 2 * hq + ph) * Wo + 2 * wq + pw;
}
