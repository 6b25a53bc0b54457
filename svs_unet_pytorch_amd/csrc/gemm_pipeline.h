// The software pipeline of the LDS-staged fp32 GEMM kernels (conv_gemm_kernel, wgrad_gemm_kernel), once.  (conv_gemm_bf16_kernel
// keeps the PF = 2 schedule written out by hand: gemm_bf16.hip says why.)
//
// Operands go global -> registers -> LDS -> MFMA, through two LDS buffers with one barrier per K position.  The kernel supplies
//   next(k)          the K position to compute after k (anything >= k_end: none; tap-skipping kernels jump over positions here);
//   fetch(k, set)    global memory -> register set `set` (a std::integral_constant<int, 0 | 1>: a compile-time choice);
//   store(buf, set)  register set `set` -> LDS buffer `buf`;
//   multiply(buf)    the MFMAs of the position held in LDS buffer `buf`.
// k is the first position to compute (k >= k_end: the block computes nothing, and fetches nothing).  Positions are visited in
// next() order, each exactly once; every store is followed by a barrier before its buffer is multiplied or its set refilled.
#pragma once
#include <type_traits>

#include "common.h"

// PF = 1: one position requested ahead -- one register set, filled while the previous position is multiplied.
//
// PF = 2: two positions in flight: the request for position n + 2 goes out when position n starts, so an operand has two
// position times to arrive before it is written to LDS.  For the fp32 kernels one K-tile time -- 512 MFMA cycles on the 64x64 tile
// -- is less than an L2 / Infinity-Cache round trip under load (per layer at batch 64, one against two tiles ahead: deconv3
// forward 130.7 -> 115.2 us, conv4 backward-data 70.1 -> 63.3, the deep layers -1 ... -5 %).  Written out as two phases so that
// register set and LDS buffer are compile-time choices.  THREE tiles ahead (six phases) and a generic ring of PF sets with
// computed indices both measured ~5 % SLOWER on the whole train step (3.60 / 3.63 against 3.43 / 3.445 ms, same device): the loop
// body triples.
template <int PF, class Next, class Fetch, class Store, class Mul>
__device__ __forceinline__ void svs_k_loop(int k, int k_end, Next&& next, Fetch&& fetch, Store&& store, Mul&& multiply) {
  static_assert(PF == 1 || PF == 2, "one or two positions ahead");
  constexpr std::integral_constant<int, 0> set0{};
  constexpr std::integral_constant<int, 1> set1{};
  if constexpr (PF == 2) {
    int k1 = next(k);
    if (k < k_end) fetch(k, set0);
    if (k1 < k_end) fetch(k1, set1);
    if (k < k_end) store(0, set0);
    __syncthreads();
    while (k < k_end) {
      int k2 = next(k1);                                      // position in LDS buffer 0; set 1 holds k1; set 0 is free
      if (k2 < k_end) fetch(k2, set0);
      multiply(0);
      if (k1 < k_end) store(1, set1);
      __syncthreads();
      k = k1; k1 = k2;
      if (k >= k_end) break;
      k2 = next(k1);                                          // position in LDS buffer 1; set 0 holds k1; set 1 is free
      if (k2 < k_end) fetch(k2, set1);
      multiply(1);
      if (k1 < k_end) store(0, set0);
      __syncthreads();
      k = k1; k1 = k2;
    }
  } else {
    if (k < k_end) {
      fetch(k, set0);
      store(0, set0);
    }
    __syncthreads();
    for (int it = 0; k < k_end; ++it) {
      const int buf = it & 1;
      const int kn = next(k);
      const bool more = kn < k_end;
      if (more) fetch(kn, set0);
      k = kn;
      multiply(buf);
      if (more) store(buf ^ 1, set0);
      __syncthreads();
    }
  }
}
