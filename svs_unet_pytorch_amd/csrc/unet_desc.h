// The one description of the twelve-block U-Net that the fp32 eval, training and bf16 eval paths share (host code only):
// channels, layers, tile geometry, the workspace allocator, the concat addressing rule and the prepared-blob layout.
#pragma once
#include "internal.h"

// Level k (k = 0..6) has spatial size (h[k], w[k]) = repeated ceil-halving of the input and CH[k] channels.
static constexpr int CH[7] = {1, 16, 32, 64, 128, 256, 512};                 // model.py:47-76

// The layers in state_dict order: conv1..conv6 (0..5), deconv1..deconv6 (6..11).  A decoder reads the whole concat
// buffer of its input level (C = 2 * CH[lin]; c6 for deconv1) and writes the decoder half of its output level.
struct Layer { bool up; int C, N, lin, lout, bn; };      // up: ConvTranspose2d; C -> N channels, level lin -> lout; bn: BatchNorm index, -1 = none
static constexpr Layer LAYERS[12] = {
    {false, 1, 16, 0, 1, 0},    {false, 16, 32, 1, 2, 1},   {false, 32, 64, 2, 3, 2},  {false, 64, 128, 3, 4, 3},
    {false, 128, 256, 4, 5, 4}, {false, 256, 512, 5, 6, 5},                                       // model.py:47-76
    {true, 512, 256, 6, 5, 6},  {true, 512, 128, 5, 4, 7},  {true, 256, 64, 4, 3, 8},  {true, 128, 32, 3, 2, 9},
    {true, 64, 16, 2, 1, 10},   {true, 32, 1, 1, 0, -1}};                                         // model.py:79-109
// parameter tensor index: 4 * layer + {0 w, 1 b, 2 gamma, 3 beta}
static constexpr long param_numel(int idx) { return idx % 4 ? LAYERS[idx / 4].N : (long)LAYERS[idx / 4].C * LAYERS[idx / 4].N * 25; }
static constexpr int bn_channels(int bn) { return LAYERS[bn].N; }            // BatchNorm bn follows layer bn,
static constexpr int bn_level(int bn) { return LAYERS[bn].lout; }            // at that layer's output level
// channels that Dropout2d masks per tile: the outputs of deconv1..deconv5
static constexpr int DROPOUT_CHANNELS = LAYERS[6].N + LAYERS[7].N + LAYERS[8].N + LAYERS[9].N + LAYERS[10].N;

struct Geo { int B; int h[7], w[7]; long P[7]; };
static int make_geo(int B, int H, int W, Geo& g) {
  SVS_REQUIRE(B > 0 && H > 0 && W > 0, "bad tile geometry B=%d H=%d W=%d", B, H, W);
  g.B = B; g.h[0] = H; g.w[0] = W;
  for (int k = 1; k <= 6; ++k) { g.h[k] = svs_conv_out(g.h[k - 1]); g.w[k] = svs_conv_out(g.w[k - 1]); }
  for (int k = 0; k <= 6; ++k) g.P[k] = (long)B * g.h[k] * g.w[k];
  return SVS_OK;
}

// bf16 eval workspace (gemm_bf16.hip: bf16_ws_layout): byte offset of "cat1" .. "cat5" / "c6", -1 for any other name
long svs_unet_bf16_ws_offset(const char* name, const Geo& g);

// bump allocator of every workspace and prepared blob (each block 256-byte aligned); a null base only measures
struct Arena {
  char* base; size_t used;
  size_t skip(size_t bytes) { const size_t o = used; used += svs_align_up(bytes, 256); return o; }      // offset of the block
  template <class T> T* take(size_t n) { const size_t o = skip(n * sizeof(T)); return base ? (T*)(base + o) : nullptr; }
};

// One channel half of the level-k concat buffer (which: 0 = decoder output, 1 = encoder/skip output).
// Levels 2..5 interleave the halves inside a pixel (ld = 2*ch, a half is >= 128 B in fp32 so accesses are whole lines).
// Level 1 has 16-channel halves (64 B in fp32, 32 B in bf16): interleaved, every access of a half would touch half a
// line and drag the other half through the caches, so level 1 is PLANAR -- two dense (P, 16) planes back to back; the
// kernels that need all 32 channels of a pixel (deconv6 forward / weight gradient / data gradient) take the plane
// distance level1_plane() as `half` (special.hip: chan_off).
template <class T> struct HalfView { T* p; long ld; };
static long level1_plane(const Geo& g) { return g.P[1] * CH[1]; }
template <class T> static HalfView<T> cat_half(T* const* cat, const Geo& g, int k, int which) {
  if (k == 1) return {cat[1] + which * level1_plane(g), CH[1]};
  return {cat[k] + (long)which * CH[k], 2L * CH[k]};
}

// largest bytes(LAYERS[l]) over the layers first..last
template <class F> static size_t max_layer_bytes(int first, int last, F bytes) {
  size_t m = 0;
  for (int l = first; l <= last; ++l) { const size_t s = bytes(LAYERS[l]); if (s > m) m = s; }
  return m;
}

// the fp32 eval blob of svs_unet_prepare_eval: packed weights, folded BatchNorm scale / shift (offsets in floats)
struct Prepared { long wp[12], scale[11], shift[11], bias6, total; };
static Prepared prepared_layout() {
  Prepared p{};
  Arena a{};
  auto take = [&](long n) { return (long)(a.skip(n * sizeof(float)) / sizeof(float)); };
  for (int l = 0; l < 12; ++l) p.wp[l] = take(param_numel(4 * l));
  for (int l = 0; l < 11; ++l) { p.scale[l] = take(bn_channels(l)); p.shift[l] = take(bn_channels(l)); }
  p.bias6 = take(1);
  p.total = (long)(a.used / sizeof(float));
  return p;
}
