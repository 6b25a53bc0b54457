// Host-side orchestration of the U-Net on one GPU: the per-block C-ABI wrappers and the whole-network
// eval forward / training forward+backward (one C call per step; every kernel goes to the caller's
// stream, nothing synchronises, so the calls are hipGraph-capturable).
//
// HBM layout (fp32, NHWC).  Level k (k = 0..6) has spatial size (h[k], w[k]) = repeated ceil-halving
// of the input and ch[k] = {1,16,32,64,128,256,512} channels (reference model.py:47-76).
//   cat[k], k=1..5 : (B, h[k], w[k], 2*ch[k])   first half  = output of decoder 6-k  (model.py:183-196)
//                                                second half = output of encoder k    (model.py:176-180)
//                    -> torch.cat([deconv_out, conv_out], 1) of model.py:186-198 is never materialised:
//                       producers write their half with ld = 2*ch[k], consumers read the full width.
//   c6             : (B, h[6], w[6], 512)
// Training additionally keeps the pre-BatchNorm ("raw") output of every block, the batch statistics,
// both weight packings, and gradient images dcat[k] / dc6 of the same shapes.
#include <math.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "unet_desc.h"

// ---------------------------------------------------------------------------------------------
// error string
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void svs_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* svs_last_error_string(void) { return g_err; }

// ---------------------------------------------------------------------------------------------
// tuning table (common.h: SvsTune)
// ---------------------------------------------------------------------------------------------
static const char* const TUNE_NAMES[SVS_TUNE_COUNT] = {
    "CONV_CFG", "CONV_KSPLIT", "CONV_WINDOW", "CONV_SKIP", "SKIP_REDUCE", "WGRAD_CFG", "WGRAD_KSPLIT", "WGRAD_SKIP",
    "WGRAD_WINDOW", "TRAIN_UNFUSED", "TRAIN_ONE_STREAM", "MFMA_SPLIT", "CONV_C1_TILED", "BF16_CFG", "BF16_KSPLIT", "BN_INLINE",
    "CONV_GWINDOW"};
static std::atomic<long> g_tune[SVS_TUNE_COUNT];      // written by svs_tuning_set while compute threads read: relaxed atomics
static std::once_flag g_tune_once;
static void tune_load_env() {
  for (int k = 0; k < SVS_TUNE_COUNT; ++k) {
    char name[64];
    snprintf(name, sizeof(name), "SVS_%s", TUNE_NAMES[k]);
    const char* e = getenv(name);
    g_tune[k].store(e ? (*e ? atol(e) : 1) : -1, std::memory_order_relaxed);
  }
}
long svs_tune(int key) {
  std::call_once(g_tune_once, tune_load_env);
  return (key >= 0 && key < SVS_TUNE_COUNT) ? g_tune[key].load(std::memory_order_relaxed) : -1;
}
extern "C" int svs_tuning_set(const char* name, long value) {
  std::call_once(g_tune_once, tune_load_env);
  SVS_REQUIRE(name, "svs_tuning_set: null name");
  if (!strcmp(name, "*")) {                 // every switch: value -1 = back to the process defaults (the SVS_<NAME> environment)
    if (value == -1) tune_load_env();
    else for (int k = 0; k < SVS_TUNE_COUNT; ++k) g_tune[k].store(value, std::memory_order_relaxed);
    return SVS_OK;
  }
  for (int k = 0; k < SVS_TUNE_COUNT; ++k)
    if (!strcmp(name, TUNE_NAMES[k])) { g_tune[k].store(value, std::memory_order_relaxed); return SVS_OK; }
  svs_set_error("svs_tuning_set: unknown switch '%s'", name);
  return SVS_ERR_INVALID;
}
extern "C" int svs_version(void) { return SVS_ABI_VERSION; }

// ---------------------------------------------------------------------------------------------
// per-block wrappers
// ---------------------------------------------------------------------------------------------
extern "C" size_t svs_enc_block_workspace_bytes(int B, int H, int W, int C, int N) {
  return svs_conv_gemm_workspace(SVS_MODE_GATHER, B, H, W, C, svs_conv_out(H), svs_conv_out(W), N);
}
extern "C" int svs_enc_block_fwd(const float* x, int64_t ldx, int B, int H, int W, int C, const float* wp,
                                 const float* bias, const float* scale, const float* shift, float slope, float* y,
                                 int64_t ldy, int N, int accumulate, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (C == 1) {
    SVS_REQUIRE(ldx == 1, "svs_enc_block_fwd: single-channel input must be dense (ldx=1)");
    return svs_conv_c1_run(x, B, H, W, wp, bias, scale, shift, slope, y, ldy, N, accumulate, stream, "svs_enc_block_fwd");
  }
  return svs_conv_gemm_run(SVS_MODE_GATHER, x, ldx, B, H, W, C, wp, bias, scale, shift, slope, y, ldy, svs_conv_out(H),
                           svs_conv_out(W), N, accumulate, ws, ws_bytes, stream, "svs_enc_block_fwd");
}
extern "C" size_t svs_dec_block_workspace_bytes(int B, int H, int W, int C, int Ho, int Wo, int N) {
  return svs_conv_gemm_workspace(SVS_MODE_PARITY, B, H, W, C, Ho, Wo, N);
}
extern "C" int svs_dec_block_fwd(const float* x, int64_t ldx, int B, int H, int W, int C, const float* wp,
                                 const float* bias, const float* scale, const float* shift, float slope, float* y,
                                 int64_t ldy, int Ho, int Wo, int N, int accumulate, void* ws, size_t ws_bytes,
                                 hipStream_t stream) {
  return svs_conv_gemm_run(SVS_MODE_PARITY, x, ldx, B, H, W, C, wp, bias, scale, shift, slope, y, ldy, Ho, Wo, N,
                           accumulate, ws, ws_bytes, stream, "svs_dec_block_fwd");
}
extern "C" int svs_out_block_fwd(const float* x, int64_t ldx, int B, int H, int W, int C, const float* w,
                                 const float* bias, float* y, int Ho, int Wo, int apply_sigmoid, hipStream_t stream) {
  return svs_deconv_to1_run(x, ldx, B, H, W, C, w, bias, y, Ho, Wo, apply_sigmoid, stream, "svs_out_block_fwd");
}
extern "C" int svs_enc_block_bwd_data(const float* dy, int64_t lddy, int B, int Ho, int Wo, int N, const float* wpar,
                                      float* dx, int64_t lddx, int H, int W, int C, int accumulate, void* ws,
                                      size_t ws_bytes, hipStream_t stream) {
  // transposed conv of dy: "input" is (Ho,Wo,N), "output" is (H,W,C)
  return svs_conv_gemm_run(SVS_MODE_PARITY, dy, lddy, B, Ho, Wo, N, wpar, nullptr, nullptr, nullptr, 0.f, dx, lddx, H, W,
                           C, accumulate, ws, ws_bytes, stream, "svs_enc_block_bwd_data");
}
extern "C" int svs_dec_block_bwd_data(const float* dy, int64_t lddy, int B, int Ho, int Wo, int N, const float* wgat,
                                      float* dx, int64_t lddx, int H, int W, int C, int accumulate, void* ws,
                                      size_t ws_bytes, hipStream_t stream) {
  // strided conv of dy: "input" is (Ho,Wo,N), "output" is (H,W,C) with H = ceil(Ho/2)
  if (N == 1) {
    SVS_REQUIRE(lddy == 1, "svs_dec_block_bwd_data: single-channel gradient must be dense");
    SVS_REQUIRE(H == svs_conv_out(Ho) && W == svs_conv_out(Wo), "svs_dec_block_bwd_data: geometry mismatch");
    return svs_conv_c1_run(dy, B, Ho, Wo, wgat, nullptr, nullptr, nullptr, 0.f, dx, lddx, C, accumulate, stream,
                           "svs_dec_block_bwd_data");
  }
  return svs_conv_gemm_run(SVS_MODE_GATHER, dy, lddy, B, Ho, Wo, N, wgat, nullptr, nullptr, nullptr, 0.f, dx, lddx, H, W,
                           C, accumulate, ws, ws_bytes, stream, "svs_dec_block_bwd_data");
}
extern "C" size_t svs_block_bwd_weight_workspace_bytes(int B, int Hs, int Ws, int Cs, int Cl) {
  size_t a = (Cl == 1) ? svs_wgrad_c1_workspace(B, Hs, Ws, Cs) : svs_wgrad_gemm_workspace(B, Hs, Ws, Cs, Cl);
  size_t b = svs_bn_workspace_bytes((int64_t)B * Hs * Ws * 4, Cs > Cl ? Cs : Cl);   // bias-gradient partials
  return a > b ? a : b;
}
extern "C" int svs_enc_block_bwd_weight(const float* dy, int64_t lddy, int B, int Ho, int Wo, int N, const float* x,
                                        int64_t ldx, int H, int W, int C, float* dw, float* db, void* ws,
                                        size_t ws_bytes, hipStream_t stream) {
  int rc;
  if (C == 1) rc = svs_wgrad_c1_run(dy, lddy, B, Ho, Wo, N, x, H, W, dw, ws, ws_bytes, stream, "svs_enc_block_bwd_weight");
  else rc = svs_wgrad_gemm_run(dy, lddy, B, Ho, Wo, N, x, ldx, H, W, C, dw, ws, ws_bytes, stream, "svs_enc_block_bwd_weight");
  if (rc || !db) return rc;
  return svs_channel_sum_run(dy, lddy, (long)B * Ho * Wo, N, db, ws, ws_bytes, stream);
}
extern "C" int svs_dec_block_bwd_weight(const float* x, int64_t ldx, int B, int H, int W, int C, const float* dy,
                                        int64_t lddy, int Ho, int Wo, int N, float* dw, float* db, void* ws,
                                        size_t ws_bytes, hipStream_t stream) {
  int rc;
  if (N == 1) {
    rc = svs_wgrad_c1_run(x, ldx, B, H, W, C, dy, Ho, Wo, dw, ws, ws_bytes, stream, "svs_dec_block_bwd_weight");
    if (rc || !db) return rc;
    return svs_sum_run(dy, (long)B * Ho * Wo, db, ws, ws_bytes, stream);
  }
  rc = svs_wgrad_gemm_run(x, ldx, B, H, W, C, dy, lddy, Ho, Wo, N, dw, ws, ws_bytes, stream, "svs_dec_block_bwd_weight");
  if (rc || !db) return rc;
  return svs_channel_sum_run(dy, lddy, (long)B * Ho * Wo, N, db, ws, ws_bytes, stream);
}

// kind 0: gather GEMM (enc fwd / dec bwd_data), 1: parity GEMM (dec fwd / enc bwd_data), 2: weight-gradient GEMM
// (then H,W,C = the strided image S and N = channels of the windowed image), 3 / 4: gather / parity layer of the bf16 eval
// network, 5 / 6: the gather / parity GEMM call with the folded-BatchNorm epilogue (the fp32 eval forward's form of kinds 0 / 1:
// plan_gemm_tile's `inference` rules).  Returns the K-split.
extern "C" int svs_describe_plan(int kind, int B, int H, int W, int C, int Ho, int Wo, int N, char* buf, size_t buflen) {
  if (!buf || !buflen) return SVS_ERR_INVALID;
  if (kind == 2) return svs_wgrad_gemm_describe(B, H, W, C, N, buf, buflen);
  if (kind == 3 || kind == 4) return svs_conv_bf16_describe(kind == 4 ? SVS_MODE_PARITY : SVS_MODE_GATHER, B, H, W, C, Ho, Wo, N, buf, buflen);
  SVS_REQUIRE(kind == 0 || kind == 1 || kind == 5 || kind == 6, "svs_describe_plan: unknown kind %d", kind);
  return svs_conv_gemm_describe(kind == 1 || kind == 6 ? SVS_MODE_PARITY : SVS_MODE_GATHER, B, H, W, C, Ho, Wo, N, C, kind >= 5, buf, buflen);
}

// ---------------------------------------------------------------------------------------------
// network description (unet_desc.h) as the C ABI shows it
// ---------------------------------------------------------------------------------------------
#define BN_EPS 1e-5f
#define BN_MOMENTUM 0.1f
#define LEAKY 0.2f

extern "C" int64_t svs_unet_param_offset(int tensor_index) {
  if (tensor_index < 0 || tensor_index > SVS_UNET_NUM_PARAMS) return -1;
  long off = 0;
  for (int i = 0; i < tensor_index; ++i) off += param_numel(i);
  return off;
}
extern "C" int64_t svs_unet_buffer_offset(int bn_index, int which) {
  if (bn_index < 0 || bn_index > SVS_UNET_NUM_BN) return -1;
  long off = 0;
  for (int i = 0; i < bn_index; ++i) off += 2 * bn_channels(i);
  if (bn_index < SVS_UNET_NUM_BN && which) off += bn_channels(bn_index);
  return off;
}

struct ParamView {
  const float* w[12]; const float* b[12]; const float* gamma[11]; const float* beta[11];   // 0..5 enc, 6..11 dec
};
static ParamView view_params(const float* params) {
  ParamView v{};
  for (int l = 0; l < 12; ++l) {
    const int base = 4 * l;
    v.w[l] = params + svs_unet_param_offset(base);
    v.b[l] = params + svs_unet_param_offset(base + 1);
    if (l < 11) {
      v.gamma[l] = params + svs_unet_param_offset(base + 2);
      v.beta[l] = params + svs_unet_param_offset(base + 3);
    }
  }
  return v;
}

typedef HalfView<float> View;

// workspace of the forward GEMM of a layer, and of the GEMMs that carry gradients back through it
static size_t fwd_ws(const Geo& g, const Layer& L) {
  return svs_conv_gemm_workspace(L.up ? SVS_MODE_PARITY : SVS_MODE_GATHER, g.B, g.h[L.lin], g.w[L.lin], L.C, g.h[L.lout], g.w[L.lout], L.N);
}
static size_t bwd_data_ws(const Geo& g, const Layer& L) {
  return svs_conv_gemm_workspace(L.up ? SVS_MODE_GATHER : SVS_MODE_PARITY, g.B, g.h[L.lout], g.w[L.lout], L.N, g.h[L.lin], g.w[L.lin], L.C);
}
static size_t bwd_weight_ws(const Geo& g, const Layer& L) {      // (strided image and its channels, channels of the windowed image)
  return L.up ? svs_block_bwd_weight_workspace_bytes(g.B, g.h[L.lin], g.w[L.lin], L.C, L.N)
              : svs_block_bwd_weight_workspace_bytes(g.B, g.h[L.lout], g.w[L.lout], L.N, L.C);
}

// ---------------------------------------------------------------------------------------------
// eval
// ---------------------------------------------------------------------------------------------
extern "C" size_t svs_unet_prepared_bytes(void) { return (size_t)prepared_layout().total * sizeof(float); }

extern "C" int svs_unet_prepare_eval(const float* params, const float* bn_buffers, void* prepared, hipStream_t stream) {
  SVS_REQUIRE(params && bn_buffers && prepared && svs_aligned16(params) && svs_aligned16(prepared), "svs_unet_prepare_eval: bad pointers");
  const Prepared L = prepared_layout();
  const ParamView v = view_params(params);
  float* blob = (float*)prepared;
  int rc;
  // conv1: C == 1, the gather packing is torch's layout; deconv6: N == 1, kernel reads torch's layout
  SVS_HIP(hipMemcpyAsync(blob + L.wp[0], v.w[0], param_numel(0) * sizeof(float), hipMemcpyDeviceToDevice, stream));
  {
    SvsPackJobs jobs{};
    for (int l = 1; l <= 10; ++l) jobs.j[jobs.n++] = SvsPackJob{v.w[l], blob + L.wp[l], LAYERS[l].N, LAYERS[l].C, LAYERS[l].up, 0};
    if ((rc = svs_pack_all_run(jobs, stream))) return rc;
  }
  SVS_HIP(hipMemcpyAsync(blob + L.wp[11], v.w[11], param_numel(44) * sizeof(float), hipMemcpyDeviceToDevice, stream));
  SVS_HIP(hipMemcpyAsync(blob + L.bias6, v.b[11], sizeof(float), hipMemcpyDeviceToDevice, stream));
  for (int l = 0; l < 11; ++l) {
    const float* rm = bn_buffers + svs_unet_buffer_offset(l, 0);
    const float* rv = bn_buffers + svs_unet_buffer_offset(l, 1);
    if ((rc = svs_bn_fold(v.gamma[l], v.beta[l], rm, rv, v.b[l], BN_EPS, blob + L.scale[l], blob + L.shift[l], bn_channels(l), stream))) return rc;
  }
  return SVS_OK;
}

struct EvalWs { float* cat[6]; float* c6; float* scratch; size_t scratch_bytes; size_t total; };
static EvalWs eval_layout(const Geo& g, void* ws) {
  EvalWs e{};
  Arena a{(char*)ws, 0};
  for (int k = 1; k <= 5; ++k) e.cat[k] = a.take<float>((size_t)g.P[k] * 2 * CH[k]);
  e.c6 = a.take<float>((size_t)g.P[6] * CH[6]);
  const size_t sb = max_layer_bytes(1, 10, [&](const Layer& L) { return fwd_ws(g, L); });
  e.scratch_bytes = sb;
  e.scratch = a.take<float>(sb / sizeof(float) + 64);
  e.total = a.used;
  return e;
}
extern "C" size_t svs_unet_eval_workspace_bytes(int B, int H, int W) {
  Geo g;
  if (make_geo(B, H, W, g)) return 0;
  return eval_layout(g, nullptr).total;
}

extern "C" int svs_unet_forward_eval(const void* prepared, const float* mix, float* mask, int B, int H, int W, void* ws,
                                     size_t ws_bytes, hipStream_t stream) {
  Geo g;
  int rc = make_geo(B, H, W, g);
  if (rc) return rc;
  SVS_REQUIRE(prepared && mix && mask && svs_aligned16(mix) && svs_aligned16(mask), "svs_unet_forward_eval: bad pointers");
  const EvalWs e = eval_layout(g, ws);
  if (!ws || ws_bytes < e.total || !svs_aligned16(ws)) { svs_set_error("svs_unet_forward_eval: workspace too small (%zu < %zu)", ws_bytes, e.total); return SVS_ERR_WORKSPACE; }
  const Prepared L = prepared_layout();
  const float* blob = (const float*)prepared;
  // encoder (model.py:176-181): BN folded, LeakyReLU(0.2) in the epilogue
  for (int k = 1; k <= 6; ++k) {
    const View xi = (k == 1) ? View{const_cast<float*>(mix), 1} : cat_half(e.cat, g, k - 1, 1);
    const View yo = (k == 6) ? View{e.c6, CH[6]} : cat_half(e.cat, g, k, 1);
    rc = svs_enc_block_fwd(xi.p, xi.ld, B, g.h[k - 1], g.w[k - 1], CH[k - 1], blob + L.wp[k - 1], nullptr,
                           blob + L.scale[k - 1], blob + L.shift[k - 1], LEAKY, yo.p, yo.ld, CH[k], 0, e.scratch, e.scratch_bytes, stream);
    if (rc) return rc;
  }
  // decoder (model.py:183-196): BN folded, ReLU; Dropout2d is the identity in eval
  for (int l = 6; l <= 10; ++l) {
    const Layer& D = LAYERS[l];
    const float* x = (l == 6) ? e.c6 : e.cat[D.lin];
    const View yo = cat_half(e.cat, g, D.lout, 0);
    rc = svs_dec_block_fwd(x, D.C, B, g.h[D.lin], g.w[D.lin], D.C, blob + L.wp[l], nullptr, blob + L.scale[l], blob + L.shift[l], 0.f,
                           yo.p, yo.ld, g.h[D.lout], g.w[D.lout], D.N, 0, e.scratch, e.scratch_bytes, stream);
    if (rc) return rc;
  }
  // deconv6 + sigmoid (model.py:198-200)
  return svs_deconv_to1_run(e.cat[1], CH[1], B, g.h[1], g.w[1], LAYERS[11].C, blob + L.wp[11], blob + L.bias6, mask, H, W, 1, stream,
                            "svs_unet_forward_eval", level1_plane(g));
}

// The reference's eval-mode objective (train.py:317-363, the loss of train.py:329-346) with no gradient: one eval forward, the
// value-only L1 kernel and -- when the phase tiles are given -- the two inverse STFTs and the MR-STFT loss exactly as
// svs_unet_train_fwd_loss_mr issues them, minus d_x.  Everything on the caller's stream; parameters and BatchNorm buffers are
// never seen (only the prepared blob is).  hop == 0 in the workspace query: the L1 part alone.
struct EvalLossWs { void* eval; size_t eval_bytes; float* mask; float* partial; float* wav_pred; float* wav_tgt; void* mr; size_t mr_bytes; size_t total; };
static EvalLossWs eval_loss_layout(const Geo& g, int W, int hop, void* ws) {
  EvalLossWs m{};
  Arena a{(char*)ws, 0};
  m.eval_bytes = eval_layout(g, nullptr).total;
  m.eval = a.take<char>(m.eval_bytes);
  m.mask = a.take<float>((size_t)g.P[0]);
  m.partial = a.take<float>(svs_l1_mask_loss_workspace_bytes(g.P[0]) / sizeof(float));
  if (hop > 0) {
    const size_t L = (size_t)hop * (W - 1);
    m.wav_pred = a.take<float>((size_t)g.B * L);
    m.wav_tgt = a.take<float>((size_t)g.B * L);
    m.mr_bytes = svs_mrstft_workspace_bytes(g.B, (int64_t)L);
    m.mr = a.take<float>(m.mr_bytes / sizeof(float) + 64);
  }
  m.total = a.used;
  return m;
}
extern "C" size_t svs_unet_eval_loss_workspace_bytes(int B, int H, int W, int hop) {
  Geo g;
  if (hop < 0 || (hop > 0 && W < 2) || make_geo(B, H, W, g)) return 0;
  return eval_loss_layout(g, W, hop, nullptr).total;
}
extern "C" int svs_unet_eval_loss(const void* prepared, const float* mix, const float* voc, const float* mix_phase,
                                  const float* voc_phase, int B, int H, int W, int hop, double alpha_l1, double alpha_mr, float* mask,
                                  float* losses, double* acc, void* ws, size_t ws_bytes, hipStream_t stream) {
  Geo g;
  int rc = make_geo(B, H, W, g);
  if (rc) return rc;
  SVS_REQUIRE(prepared && mix && voc && losses && svs_aligned16(mix) && svs_aligned16(voc) && (!mask || svs_aligned16(mask)),
              "svs_unet_eval_loss: bad pointers");
  SVS_REQUIRE(!mix_phase == !voc_phase, "svs_unet_eval_loss: give both phase tiles (full objective) or neither (L1 part only)");
  const bool full = mix_phase != nullptr;
  if (full) {                                // the early errors of svs_unet_train_fwd_loss_mr
    SVS_REQUIRE(H == 256 || H == 512 || H == 1024, "svs_unet_eval_loss: with phases needs H = n_fft / 2 = 256, 512 or 1024 (n_fft 512, 1024 or "
                "2048: the sizes the inverse STFT is built for), got H = %d", H);
    SVS_REQUIRE(W >= 2 && hop > 0 && hop <= 2 * H, "svs_unet_eval_loss: needs W >= 2 and 0 < hop <= n_fft = %d (W = %d, hop = %d)", 2 * H, W, hop);
    SVS_REQUIRE((long)hop * (W - 1) > 2048, "svs_unet_eval_loss: W = %d frames at hop = %d give waveforms of hop * (W - 1) = %ld samples; the "
                "multi-resolution STFT loss needs more than 2048", W, hop, (long)hop * (W - 1));
    SVS_REQUIRE(svs_aligned16(mix_phase) && svs_aligned16(voc_phase), "svs_unet_eval_loss: bad pointers");
  }
  const EvalLossWs m = eval_loss_layout(g, W, full ? hop : 0, ws);
  if (!ws || ws_bytes < m.total || !svs_aligned16(ws)) { svs_set_error("svs_unet_eval_loss: workspace too small (%zu < %zu)", ws_bytes, m.total); return SVS_ERR_WORKSPACE; }
  float* mk = mask ? mask : m.mask;
  if ((rc = svs_unet_forward_eval(prepared, mix, mk, B, H, W, m.eval, m.eval_bytes, stream))) return rc;
  if ((rc = svs_l1_mask_loss_fwd(mk, mix, voc, g.P[0], losses, m.partial, svs_l1_mask_loss_workspace_bytes(g.P[0]), stream))) return rc;   // train.py:329-338
  if (full) {
    const int64_t cs = (int64_t)H * W;
    const long L = (long)hop * (W - 1);
    if ((rc = svs_istft_tiles_n(mix, cs, W, H, 1, mk, 0, mix_phase, 3, B, 2 * H, hop, W, m.wav_pred, nullptr, stream))) return rc;      // train.py:341
    if ((rc = svs_istft_tiles_n(voc, cs, W, H, 1, nullptr, 0, voc_phase, 3, B, 2 * H, hop, W, m.wav_tgt, nullptr, stream))) return rc;  // train.py:342
    if ((rc = svs_mrstft_loss_fwd_bwd(m.wav_pred, m.wav_tgt, B, L, 0.f, losses + 1, nullptr, m.mr, m.mr_bytes, stream))) return rc;      // train.py:343
  } else {
    SVS_HIP(hipMemsetAsync(losses + 1, 0, sizeof(float), stream));
  }
  return acc ? svs_eval_loss_acc_run(losses, alpha_l1, alpha_mr, acc, stream) : SVS_OK;
}

// ---------------------------------------------------------------------------------------------
// training
// ---------------------------------------------------------------------------------------------
struct TrainWs {
  float* cat[6]; float* c6;
  float* raw[11];                         // pre-BatchNorm output of layer l (conv1..conv6, deconv1..deconv5)
  float* mean[11]; float* invstd[11];
  float* wfwd[12]; float* wbwd[12];       // packed weights (null where torch's layout is read directly)
  float* dcat[6]; float* dc6;
  float* d_raw; float* d_logit; float* mask;
  float* d_raw_l[11];                     // one d_raw per BatchNorm layer: the side stream's weight gradients trail freely
  float* bnws; size_t bnws_bytes;
  float* dbias_part[11];                  // per-layer partial sums of d_raw (bias gradients), reduced in one batched pass
  float* scratch; size_t scratch_bytes;
  float* scratch2; size_t scratch2_bytes;
  size_t total;
};
#define SVS_FUSED_STATS_ROWS 512          // rows of BatchNorm partials the split-K epilogue may write into bnws
static TrainWs train_layout(const Geo& g, void* ws) {
  TrainWs t{};
  Arena a{(char*)ws, 0};
  auto take = [&](size_t nfloats) { return a.take<float>(nfloats); };
  for (int k = 1; k <= 5; ++k) t.cat[k] = take((size_t)g.P[k] * 2 * CH[k]);
  t.c6 = take((size_t)g.P[6] * CH[6]);
  for (int l = 0; l < 11; ++l) t.raw[l] = take((size_t)g.P[bn_level(l)] * bn_channels(l));
  for (int l = 0; l < 11; ++l) { t.mean[l] = take(bn_channels(l)); t.invstd[l] = take(bn_channels(l)); }
  for (int l = 1; l <= 10; ++l) { t.wfwd[l] = take(param_numel(4 * l)); t.wbwd[l] = take(param_numel(4 * l)); }
  for (int k = 1; k <= 5; ++k) t.dcat[k] = take((size_t)g.P[k] * 2 * CH[k]);
  t.dc6 = take((size_t)g.P[6] * CH[6]);
  size_t dmax = 0;
  for (int k = 1; k <= 6; ++k) if ((size_t)g.P[k] * CH[k] > dmax) dmax = (size_t)g.P[k] * CH[k];
  t.d_raw = take(dmax);
  for (int l = 0; l < 11; ++l) t.d_raw_l[l] = take((size_t)g.P[bn_level(l)] * bn_channels(l));
  t.d_logit = take((size_t)g.P[0]);
  t.mask = take((size_t)g.P[0]);
  size_t bb = 0;
  for (int k = 1; k <= 6; ++k) { size_t s = svs_bn_workspace_bytes(g.P[k], CH[k]); if (s > bb) bb = s; }
  if (bb < (size_t)SVS_FUSED_STATS_ROWS * 2 * CH[6] * sizeof(float)) bb = (size_t)SVS_FUSED_STATS_ROWS * 2 * CH[6] * sizeof(float);
  t.bnws_bytes = bb + 4096;
  t.bnws = take(t.bnws_bytes / sizeof(float));
  for (int l = 0; l < 11; ++l) t.dbias_part[l] = take(svs_bn_partial_floats(g.P[bn_level(l)], bn_channels(l)));
  // scratch2: the weight-gradient GEMMs of all twelve layers (side stream); scratch: the forward and backward-data GEMMs of
  // conv2..deconv5, and the weight gradients when there is no side stream
  t.scratch2_bytes = max_layer_bytes(0, 11, [&](const Layer& L) { return bwd_weight_ws(g, L); });
  t.scratch_bytes = std::max({(size_t)4096, t.scratch2_bytes,
                              max_layer_bytes(1, 10, [&](const Layer& L) { return std::max(fwd_ws(g, L), bwd_data_ws(g, L)); })});
  t.scratch = take(t.scratch_bytes / sizeof(float) + 64);
  t.scratch2 = take(t.scratch2_bytes / sizeof(float) + 64);
  t.total = a.used;
  return t;
}

// ---- side stream ---------------------------------------------------------------------------------
// In the backward pass the weight gradient of a layer (MFMA GEMM + slab reductions) depends only on that layer's
// d_raw, while the chain that the next layer waits for is d_raw -> backward-data GEMM -> next BatchNorm backward
// (bandwidth-bound passes).  The weight-gradient work therefore runs on a second HIP stream: its GEMMs fill the
// machine while the main stream is in the bandwidth-bound BatchNorm passes and launch gaps, and its small reduction
// kernels hide under the main stream's GEMMs.  Fork / join are events; d_raw is double-buffered so that the side
// stream may trail the main one by a layer.  Results do not depend on the interleaving (no atomics anywhere).
struct SideStream { hipStream_t s; hipEvent_t fork[4], done[4], sync; int nfork; std::mutex mu; };   // nfork: forks of the current backward pass; mu: held while a training entry point enqueues
static SideStream* g_side[64] = {};
static std::mutex g_side_mutex;
static SideStream* side_stream(hipStream_t of) {       // the side stream of the device `of` belongs to (legacy / null stream: the current device)
  int dev = 0;
  hipDevice_t sdev;
  if (of && hipStreamGetDevice(of, &sdev) == hipSuccess) dev = (int)sdev;
  else if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  if (dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lock(g_side_mutex);
  if (!g_side[dev]) {
    SideStream* sd = new SideStream();
    // HIGHEST priority (measured: 3.75 ms per step against 3.77 at normal and 3.83 at low priority): the weight-gradient
    // GEMMs then start as soon as their d_raw exists and are out of the way when the main stream reaches its next GEMM
    int least = 0, greatest = 0;
    bool ok = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
    ok = ok && hipStreamCreateWithPriority(&sd->s, hipStreamNonBlocking, greatest) == hipSuccess;
    // No system-scope fence at these events: both streams are on this device, where the kernel-boundary release / acquire already
    // orders them, and no host code reads through a fork, done or sync event (the host waits on the caller's stream).  With the
    // fence every fork's marker also flushed to system scope in front of the next GEMM of the main stream: -20 us per step at
    // batch 64
    const unsigned flags = hipEventDisableTiming | hipEventDisableSystemFence;
    ok = ok && hipEventCreateWithFlags(&sd->sync, flags) == hipSuccess;
    for (int i = 0; i < 4 && ok; ++i)
      ok = hipEventCreateWithFlags(&sd->fork[i], flags) == hipSuccess &&
           hipEventCreateWithFlags(&sd->done[i], flags) == hipSuccess;
    if (!ok) { delete sd; return nullptr; }
    g_side[dev] = sd;
  }
  return g_side[dev];
}

extern "C" size_t svs_unet_train_workspace_bytes(int B, int H, int W) {
  Geo g;
  if (make_geo(B, H, W, g)) return 0;
  return train_layout(g, nullptr).total;
}

// names of svs_unet_ws_offset: stem<first> .. stem<first + count - 1> are p[0 .. count - 1]; count 0 is the bare stem, *p
struct WsName { const char* stem; int first, count; float* const* p; };
static int64_t ws_find(const WsName* tab, size_t n, const char* name, const char* base) {
  for (size_t i = 0; i < n; ++i) {
    const size_t len = strlen(tab[i].stem);
    if (strncmp(name, tab[i].stem, len)) continue;
    if (!tab[i].count) {
      if (!name[len]) return (const char*)*tab[i].p - base;
      continue;
    }
    char* end;
    const long idx = strtol(name + len, &end, 10) - tab[i].first;
    if (end != name + len && !*end && idx >= 0 && idx < tab[i].count) return (const char*)tab[i].p[idx] - base;
  }
  return -1;
}
extern "C" int64_t svs_unet_ws_offset(const char* name, int B, int H, int W, int training) {
  Geo g;
  if (!name || make_geo(B, H, W, g)) return -1;
  if (training == 2) return svs_unet_bf16_ws_offset(name, g);      // the bf16 eval workspace
  char* const base = (char*)256;   // non-null dummy so the arena hands out addresses
  if (training) {
    const TrainWs t = train_layout(g, base);
    const WsName tab[] = {{"cat", 1, 5, t.cat + 1}, {"c6", 0, 0, &t.c6},         {"raw_e", 1, 6, t.raw},  {"raw_d", 1, 5, t.raw + 6},
                          {"dcat", 1, 5, t.dcat + 1}, {"dc6", 0, 0, &t.dc6},     {"d_logit", 0, 0, &t.d_logit}, {"mask", 0, 0, &t.mask},
                          {"mean", 0, 11, t.mean},  {"invstd", 0, 11, t.invstd}};
    return ws_find(tab, sizeof(tab) / sizeof(tab[0]), name, base);
  }
  const EvalWs e = eval_layout(g, base);
  const WsName tab[] = {{"cat", 1, 5, e.cat + 1}, {"c6", 0, 0, &e.c6}};
  return ws_find(tab, sizeof(tab) / sizeof(tab[0]), name, base);
}

// everything a training entry point derives from its arguments
struct TrainCall { Geo g; TrainWs t; ParamView v; };
static int train_prologue(const char* who, const float* params, int B, int H, int W, void* ws, size_t ws_bytes, TrainCall& c) {
  const int rc = make_geo(B, H, W, c.g);
  if (rc) return rc;
  c.t = train_layout(c.g, ws);
  if (!ws || ws_bytes < c.t.total || !svs_aligned16(ws)) {
    svs_set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, c.t.total);
    return SVS_ERR_WORKSPACE;
  }
  c.v = view_params(params);
  return SVS_OK;
}

// The tail of a training block: batch statistics of raw[l] unless the GEMM's epilogue left them in bnws (stat_rows > 0),
// then finalise (running statistics included) + BatchNorm + activation (+ Dropout2d) -> y
static int train_bn_act(const TrainCall& c, int l, int stat_rows, float* bn_buffers, int64_t* nbt, float slope, const float* drop,
                        View y, hipStream_t stream) {
  const TrainWs& t = c.t;
  const int N = bn_channels(l), lvl = bn_level(l);
  const long P = c.g.P[lvl];
  if (!stat_rows) {
    const int rc = svs_bn_stats(t.raw[l], N, P, N, t.bnws, t.bnws_bytes, stream);
    if (rc) return rc;
    stat_rows = svs_bn_partial_rows(P, N);
  }
  return svs_bn_fin_act_apply_run(t.bnws, stat_rows, t.raw[l], N, P, N, (long)c.g.h[lvl] * c.g.w[lvl], c.v.gamma[l], c.v.beta[l], BN_EPS,
                                  BN_MOMENTUM, bn_buffers ? bn_buffers + svs_unet_buffer_offset(l, 0) : nullptr,
                                  bn_buffers ? bn_buffers + svs_unet_buffer_offset(l, 1) : nullptr,
                                  nbt ? (long long*)(nbt + l) : nullptr, t.mean[l], t.invstd[l], slope, drop, y.p, y.ld, stream);
}

static int train_forward_impl(const TrainCall& c, float* bn_buffers, int64_t* nbt, const float* mix, const float* drop, float* mask,
                              hipStream_t stream) {
  const Geo& g = c.g; const TrainWs& t = c.t; const ParamView& v = c.v;
  const int B = g.B;
  int rc;
  const int fused_rows = svs_tune_flag(SVS_TUNE_TRAIN_UNFUSED) ? 0 : (int)(t.bnws_bytes / sizeof(float));     // capacity (floats) for fused BatchNorm partials; A/B switch
  SideStream* sd = svs_tune_flag(SVS_TUNE_TRAIN_ONE_STREAM) ? nullptr : side_stream(stream);          // A/B switch
  std::unique_lock<std::mutex> guard;
  if (sd) guard = std::unique_lock<std::mutex>(sd->mu);
  // weight packings for this step (weights change every optimiser step)
  {
    SvsPackJobs jobs{};
    for (int l = 1; l <= 10; ++l) {
      const Layer& L = LAYERS[l];
      // forward: gather packing for a conv, parity packing (one row per output channel) for a convT; backward-data: the
      // other packing of the same tensor with the channel roles swapped ((N,C,..) read as (in=N,out=C) and the reverse)
      jobs.j[jobs.n++] = SvsPackJob{v.w[l], t.wfwd[l], L.N, L.C, L.up, 0};
      jobs.j[jobs.n++] = SvsPackJob{v.w[l], t.wbwd[l], L.C, L.N, !L.up, 0};
    }
    // conv1 reads torch's layout directly, so the packing runs beside it on the side stream (joined before conv2)
    if (sd) {
      SVS_HIP(hipEventRecord(sd->fork[0], stream));
      SVS_HIP(hipStreamWaitEvent(sd->s, sd->fork[0], 0));
    }
    if ((rc = svs_pack_all_run(jobs, sd ? sd->s : stream))) return rc;
    if (sd) SVS_HIP(hipEventRecord(sd->done[0], sd->s));
  }
  // encoder: conv (+bias) -> raw; batch stats; BN + LeakyReLU -> second half of cat[k]
  for (int k = 1; k <= 6; ++k) {
    if (k == 2 && sd) SVS_HIP(hipStreamWaitEvent(stream, sd->done[0], 0));
    const int l = k - 1;
    const View xi = (k == 1) ? View{const_cast<float*>(mix), 1} : cat_half(t.cat, g, k - 1, 1);
    int stat_rows = 0;                       // > 0: the split-K epilogue already left the BatchNorm partials in bnws
    if (k == 1) rc = svs_enc_block_fwd(xi.p, xi.ld, B, g.h[0], g.w[0], 1, v.w[0], v.b[0], nullptr, nullptr, 0.f, t.raw[0], CH[1], CH[1], 0,
                                       t.scratch, t.scratch_bytes, stream);
    else rc = svs_conv_gemm_run(SVS_MODE_GATHER, xi.p, xi.ld, B, g.h[k - 1], g.w[k - 1], CH[k - 1], t.wfwd[l], v.b[l], nullptr, nullptr, 0.f,
                                t.raw[l], CH[k], g.h[k], g.w[k], CH[k], 0, t.scratch, t.scratch_bytes, stream, "conv forward",
                                t.bnws, fused_rows, &stat_rows);
    if (rc) return rc;
    const View yo = (k == 6) ? View{t.c6, CH[6]} : cat_half(t.cat, g, k, 1);
    if ((rc = train_bn_act(c, l, stat_rows, bn_buffers, nbt, LEAKY, nullptr, yo, stream))) return rc;
  }
  // decoder: convT (+bias) -> raw; batch stats; BN + ReLU + Dropout2d -> first half of cat[lout]
  const float* dp = drop;
  for (int l = 6; l <= 10; ++l) {
    const Layer& D = LAYERS[l];
    const float* x = (l == 6) ? t.c6 : t.cat[D.lin];
    int stat_rows = 0;
    rc = svs_conv_gemm_run(SVS_MODE_PARITY, x, D.C, B, g.h[D.lin], g.w[D.lin], D.C, t.wfwd[l], v.b[l], nullptr, nullptr, 0.f,
                           t.raw[l], D.N, g.h[D.lout], g.w[D.lout], D.N, 0, t.scratch, t.scratch_bytes, stream,
                           "deconv forward", t.bnws, fused_rows, &stat_rows);
    if (rc) return rc;
    if ((rc = train_bn_act(c, l, stat_rows, bn_buffers, nbt, 0.f, dp, cat_half(t.cat, g, D.lout, 0), stream))) return rc;
    if (dp) dp += (long)B * D.N;
  }
  return svs_deconv_to1_run(t.cat[1], CH[1], B, g.h[1], g.w[1], LAYERS[11].C, v.w[11], v.b[11], mask, g.h[0], g.w[0], 1, stream,
                            "svs_unet_train_forward", level1_plane(g));
}

// parts: bit 0 = decoder half (deconv6..deconv1: gradients of parameter tensors 24..45, produced FIRST),
//        bit 1 = encoder half (conv6..conv1: tensors 0..23).  A data-parallel caller runs them as two calls and
//        all-reduces the decoder half of the flat gradient buffer while the encoder half is still being computed.
static int train_backward_impl(const TrainCall& c, float* grads, const float* mix, const float* drop, hipStream_t stream, int parts = 15) {
  const Geo& g = c.g; const TrainWs& t = c.t; const ParamView& v = c.v;
  const int B = g.B;
  int rc;
  auto G = [&](int idx) { return grads + svs_unet_param_offset(idx); };
  SvsSumJobs sums{};                         // bias-gradient reductions, run as one batched launch per half
  const bool unfused = svs_tune_flag(SVS_TUNE_TRAIN_UNFUSED);     // A/B switch: one launch per reduction, as before
  SideStream* sd = svs_tune_flag(SVS_TUNE_TRAIN_ONE_STREAM) ? nullptr : side_stream(stream);   // A/B switch: everything on `stream`
  std::unique_lock<std::mutex> guard;
  if (sd) guard = std::unique_lock<std::mutex>(sd->mu);
  const hipStream_t wstream = sd ? sd->s : stream;                  // where the weight gradients run
  float* const wscratch = sd ? t.scratch2 : t.scratch;
  const size_t wscratch_bytes = sd ? t.scratch2_bytes : t.scratch_bytes;
  // forks so far in this backward pass (kept in the SideStream across the calls of a split pass, which must come in
  // order on one host thread); fork n uses event slot n & 3.  Every layer has a d_raw buffer of its own, so the main
  // stream never waits for a weight gradient before the end of the pass (an event pair per layer measured dearer than
  // the 0.2 GB of workspace).
  int nfork_local = 0;
  int& nfork = sd ? sd->nfork : nfork_local;
  if (parts & 1) nfork = 0;
  auto layer_draw = [&](int l) -> float* { return sd ? t.d_raw_l[l] : t.d_raw; };
  auto fork = [&]() -> int {                 // the side stream may start once everything queued on `stream` so far is done
    if (!sd) return SVS_OK;
    SVS_HIP(hipEventRecord(sd->fork[nfork & 3], stream));
    SVS_HIP(hipStreamWaitEvent(sd->s, sd->fork[nfork & 3], 0));
    return SVS_OK;
  };
  auto forked = [&]() -> int { ++nfork; return SVS_OK; };
  auto join = [&]() -> int {                 // `stream` waits for all side work enqueued so far
    if (sd && nfork > 0) {
      SVS_HIP(hipEventRecord(sd->done[0], sd->s));
      SVS_HIP(hipStreamWaitEvent(stream, sd->done[0], 0));
    }
    return SVS_OK;
  };
  if (parts & 1) {
  // deconv6 (model.py:109,198): dw, db, dx -> dcat[1]
  const long half1 = level1_plane(g);
  if ((rc = fork())) return rc;
  if ((rc = svs_wgrad_c1_run(t.cat[1], CH[1], B, g.h[1], g.w[1], LAYERS[11].C, t.d_logit, g.h[0], g.w[0], G(44), wscratch, wscratch_bytes, wstream,
                             "deconv6 bwd_weight", half1))) return rc;
  if ((rc = svs_sum_run(t.d_logit, g.P[0], G(45), wscratch, wscratch_bytes, wstream))) return rc;      // deconv6 bias gradient
  if ((rc = forked())) return rc;
  if ((rc = svs_conv_c1_run(t.d_logit, B, g.h[0], g.w[0], v.w[11], nullptr, nullptr, nullptr, 0.f, t.dcat[1], CH[1], LAYERS[11].C, 0, stream,
                            "deconv6 bwd_data", half1))) return rc;
  // decoders 5..1
  long drop_off[11];                         // start of layer l's Dropout2d mask in `drop`
  { long o = 0; for (int l = 6; l <= 10; ++l) { drop_off[l] = o; o += (long)B * LAYERS[l].N; } }
  for (int l = 10; l >= 6; --l) {
    const int lin = LAYERS[l].lin, lout = LAYERS[l].lout, N = LAYERS[l].N, C = LAYERS[l].C;
    const float* x = (l == 6) ? t.c6 : t.cat[lin];
    const View dyv = cat_half(t.dcat, g, lout, 0);
    float* const d_raw = layer_draw(l);
    rc = svs_bn_bwd_run(dyv.p, dyv.ld, t.raw[l], N, g.P[lout], N, (long)g.h[lout] * g.w[lout], v.gamma[l], v.beta[l],
                        t.mean[l], t.invstd[l], 0.f, drop ? drop + drop_off[l] : nullptr, d_raw, G(4 * l + 2), G(4 * l + 3),
                        G(4 * l + 1), t.bnws, t.bnws_bytes, stream, unfused ? nullptr : t.dbias_part[l], &sums);   // + bias gradient (sum of d_raw)
    if (rc) return rc;
    if ((rc = fork())) return rc;
    if ((rc = svs_dec_block_bwd_weight(x, C, B, g.h[lin], g.w[lin], C, d_raw, N, g.h[lout], g.w[lout], N, G(4 * l), nullptr,
                                       wscratch, wscratch_bytes, wstream))) return rc;
    if ((rc = forked())) return rc;
    float* dx = (l == 6) ? t.dc6 : t.dcat[lin];
    if ((rc = svs_dec_block_bwd_data(d_raw, N, B, g.h[lout], g.w[lout], N, t.wbwd[l], dx, C, g.h[lin], g.w[lin], C, 0,
                                     t.scratch, t.scratch_bytes, stream))) return rc;
  }
  if ((rc = svs_channel_sum_finalize_multi_run(sums, stream))) return rc;    // the five decoder bias gradients
  sums.njobs = 0;
  }
  if (!(parts & 14)) return SVS_OK;
  // encoders 6..1 (bit 2: block 6, whose 13 MB of gradients are most of the encoder's; bit 4: blocks 5 and 4 (4.1 MB);
  // bit 8: blocks 3..1 (0.26 MB: the only piece a data-parallel step exchanges after the backward has ended))
  for (int k = 6; k >= 1; --k) {
    if (!(parts & (k == 6 ? 2 : k >= 4 ? 4 : 8))) continue;
    const int l = k - 1, N = CH[k], C = CH[k - 1];
    const View dyv = (k == 6) ? View{t.dc6, CH[6]} : cat_half(t.dcat, g, k, 1);
    float* const d_raw = layer_draw(l);
    rc = svs_bn_bwd_run(dyv.p, dyv.ld, t.raw[l], N, g.P[k], N, (long)g.h[k] * g.w[k], v.gamma[l], v.beta[l], t.mean[l], t.invstd[l],
                        LEAKY, nullptr, d_raw, G(4 * l + 2), G(4 * l + 3), G(4 * l + 1), t.bnws, t.bnws_bytes, stream,
                        unfused ? nullptr : t.dbias_part[l], &sums);
    if (rc) return rc;
    const View xi = (k == 1) ? View{const_cast<float*>(mix), 1} : cat_half(t.cat, g, k - 1, 1);
    const float* x = xi.p; const long ldx = xi.ld;
    if (k == 1) {
      // conv1 is the end of the pass: nothing is left for the main stream to run beside this weight gradient, so it runs there
      // itself (a fork + join for it left the main stream idle for 44 us before Adam: the fork's start latency and the join)
      if ((rc = svs_enc_block_bwd_weight(d_raw, N, B, g.h[k], g.w[k], N, x, ldx, g.h[k - 1], g.w[k - 1], C, G(4 * l), nullptr,
                                         t.scratch, t.scratch_bytes, stream))) return rc;
      continue;
    }
    if ((rc = fork())) return rc;
    if ((rc = svs_enc_block_bwd_weight(d_raw, N, B, g.h[k], g.w[k], N, x, ldx, g.h[k - 1], g.w[k - 1], C, G(4 * l), nullptr,
                                       wscratch, wscratch_bytes, wstream))) return rc;
    if ((rc = forked())) return rc;
    if (k >= 2) {
      // gradient of the skip half of cat[k-1]: add to what decoder (7-k)'s bwd_data left there
      const View dxs = cat_half(t.dcat, g, k - 1, 1);
      if ((rc = svs_enc_block_bwd_data(d_raw, N, B, g.h[k], g.w[k], N, t.wbwd[l], dxs.p, dxs.ld, g.h[k - 1], g.w[k - 1], C, 1,
                                       t.scratch, t.scratch_bytes, stream))) return rc;
    }
  }
  if ((rc = svs_channel_sum_finalize_multi_run(sums, stream))) return rc;    // the encoder bias gradients of this call
  // `stream` is joined with the side stream only by the call that ends the pass (block 1 included); after an earlier
  // part of a split pass the caller uses svs_unet_train_bwd_sync() on the stream that consumes that part's gradients
  return (parts & 8) ? join() : SVS_OK;
}

extern "C" int svs_unet_train_bwd_sync(hipStream_t consumer) {
  SideStream* sd = svs_tune_flag(SVS_TUNE_TRAIN_ONE_STREAM) ? nullptr : side_stream(consumer);
  if (!sd) return SVS_OK;
  std::lock_guard<std::mutex> guard(sd->mu);
  SVS_HIP(hipEventRecord(sd->sync, sd->s));
  SVS_HIP(hipStreamWaitEvent(consumer, sd->sync, 0));
  return SVS_OK;
}

extern "C" int svs_unet_train_forward(const float* params, float* bn_buffers, int64_t* num_batches_tracked, const float* mix,
                                      const float* drop, int B, int H, int W, float* mask, void* ws, size_t ws_bytes,
                                      hipStream_t stream) {
  SVS_REQUIRE(params && mix && mask && svs_aligned16(params) && svs_aligned16(mix) && svs_aligned16(mask), "svs_unet_train_forward: bad pointers");
  TrainCall c;
  const int rc = train_prologue("svs_unet_train_forward", params, B, H, W, ws, ws_bytes, c);
  if (rc) return rc;
  return train_forward_impl(c, bn_buffers, num_batches_tracked, mix, drop, mask, stream);
}

extern "C" int svs_unet_train_backward(const float* params, float* grads, const float* mix, const float* mask,
                                       const float* d_mask, const float* drop, int B, int H, int W, void* ws,
                                       size_t ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(params && grads && mix && mask && d_mask && svs_aligned16(grads), "svs_unet_train_backward: bad pointers");
  TrainCall c;
  int rc = train_prologue("svs_unet_train_backward", params, B, H, W, ws, ws_bytes, c);
  if (rc) return rc;
  if ((rc = svs_sigmoid_bwd_run(mask, d_mask, c.g.P[0], c.t.d_logit, stream))) return rc;
  return train_backward_impl(c, grads, mix, drop, stream);
}

// forward + L1 mask loss (scaled by loss_scale) + d(loss)/d(logit) -> d_logit; the mask goes to the workspace when the caller keeps none
static int train_fwd_loss_impl(const TrainCall& c, float* bn_buffers, int64_t* nbt, const float* mix, const float* voc, const float* drop,
                               float loss_scale, float* mask, float* loss, hipStream_t stream) {
  float* m = mask ? mask : c.t.mask;
  const int rc = train_forward_impl(c, bn_buffers, nbt, mix, drop, m, stream);
  if (rc) return rc;
  return svs_l1_mask_loss_fwd_bwd(m, mix, voc, c.g.P[0], loss_scale, c.t.d_logit, loss, c.t.bnws, c.t.bnws_bytes, stream);
}

extern "C" int svs_unet_train_fwd_bwd(const float* params, float* grads, float* bn_buffers, int64_t* num_batches_tracked,
                                      const float* mix, const float* voc, const float* drop, int B, int H, int W,
                                      float loss_scale, float* mask, float* loss, void* ws, size_t ws_bytes,
                                      hipStream_t stream) {
  SVS_REQUIRE(params && grads && mix && voc && loss && svs_aligned16(params) && svs_aligned16(grads) && svs_aligned16(mix),
              "svs_unet_train_fwd_bwd: bad pointers");
  TrainCall c;
  int rc = train_prologue("svs_unet_train_fwd_bwd", params, B, H, W, ws, ws_bytes, c);
  if (rc) return rc;
  if ((rc = train_fwd_loss_impl(c, bn_buffers, num_batches_tracked, mix, voc, drop, loss_scale, mask, loss, stream))) return rc;
  return train_backward_impl(c, grads, mix, drop, stream);
}

// Split form of svs_unet_train_fwd_bwd for gradient-exchange overlap: forward + loss, then the backward in
// two parts (see train_backward_impl).
extern "C" int svs_unet_train_fwd_loss(const float* params, float* bn_buffers, int64_t* num_batches_tracked, const float* mix,
                                       const float* voc, const float* drop, int B, int H, int W, float loss_scale, float* mask,
                                       float* loss, void* ws, size_t ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(params && mix && voc && loss && svs_aligned16(params) && svs_aligned16(mix), "svs_unet_train_fwd_loss: bad pointers");
  TrainCall c;
  const int rc = train_prologue("svs_unet_train_fwd_loss", params, B, H, W, ws, ws_bytes, c);
  if (rc) return rc;
  return train_fwd_loss_impl(c, bn_buffers, num_batches_tracked, mix, voc, drop, loss_scale, mask, loss, stream);
}

// The reference's full objective (train.py:274-296): alpha_L1 * (L1 vocal + L1 accompaniment) + alpha_MR * MR-STFT(
// specific_istft(mask * mix, mix_phase), specific_istft(voc, voc_phase)).  Forward + both losses + d(total)/d(logit); the
// backward follows with svs_unet_train_bwd_part (part 4 = the whole pass, or the split forms).  H = n_fft / 2 = 256, 512 or 1024
// (the window the tiles were made with), any 0 < hop <= n_fft, hop * (W - 1) > 2048 (the loss's own resolutions do not follow the window).
//   losses[0] = L1 part (unscaled), losses[1] = MR part (unscaled); total = alpha_l1 * losses[0] + alpha_mr * losses[1]
//   mr_ws: svs_unet_train_mr_workspace_bytes(B, W, hop) bytes (waveforms, their gradient, the loss's frame buffers)
struct MrTrainWs { float* wav_pred; float* wav_tgt; float* d_wav; void* mr; size_t mr_bytes; size_t total; };
static MrTrainWs mr_train_layout(int B, int W, int hop, void* ws) {
  MrTrainWs m{};
  Arena a{(char*)ws, 0};
  const size_t L = (size_t)hop * (W - 1);
  m.wav_pred = a.take<float>((size_t)B * L);
  m.wav_tgt = a.take<float>((size_t)B * L);
  m.d_wav = a.take<float>((size_t)B * L);
  m.mr_bytes = svs_mrstft_workspace_bytes(B, (int64_t)L);
  m.mr = a.take<float>(m.mr_bytes / sizeof(float) + 64);
  m.total = a.used;
  return m;
}
extern "C" size_t svs_unet_train_mr_workspace_bytes(int B, int W, int hop) {
  if (B <= 0 || W < 2 || hop <= 0) return 0;
  return mr_train_layout(B, W, hop, nullptr).total;
}
// where the waveforms and their gradient live inside mr_ws (tests read them): "wav_pred", "wav_tgt", "d_wav"
extern "C" int64_t svs_unet_mr_ws_offset(const char* name, int B, int W, int hop) {
  if (!name || B <= 0 || W < 2 || hop <= 0) return -1;
  char* const base = (char*)256;   // non-null dummy so the arena hands out addresses
  const MrTrainWs m = mr_train_layout(B, W, hop, base);
  const WsName tab[] = {{"wav_pred", 0, 0, &m.wav_pred}, {"wav_tgt", 0, 0, &m.wav_tgt}, {"d_wav", 0, 0, &m.d_wav}};
  return ws_find(tab, sizeof(tab) / sizeof(tab[0]), name, base);
}
extern "C" int svs_unet_train_fwd_loss_mr(const float* params, float* bn_buffers, int64_t* num_batches_tracked, const float* mix,
                                          const float* voc, const float* mix_phase, const float* voc_phase, const float* drop,
                                          int B, int H, int W, int hop, float alpha_l1, float alpha_mr, float* mask, float* losses,
                                          void* ws, size_t ws_bytes, void* mr_ws, size_t mr_ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(params && mix && voc && mix_phase && voc_phase && losses && svs_aligned16(params) && svs_aligned16(mix),
              "svs_unet_train_fwd_loss_mr: bad pointers");
  SVS_REQUIRE(H == 256 || H == 512 || H == 1024, "svs_unet_train_fwd_loss_mr: needs H = n_fft / 2 = 256, 512 or 1024 (n_fft 512, 1024 or 2048: the "
              "sizes the inverse STFT and its transpose are built for), got H = %d", H);
  SVS_REQUIRE(W >= 2 && hop > 0 && hop <= 2 * H, "svs_unet_train_fwd_loss_mr: needs W >= 2 and 0 < hop <= n_fft = %d (W = %d, hop = %d)", 2 * H, W, hop);
  // the MR-STFT loss reflect-pads by half of its widest window (2048): the waveform must be longer than that
  SVS_REQUIRE((long)hop * (W - 1) > 2048, "svs_unet_train_fwd_loss_mr: W = %d frames at hop = %d give waveforms of hop * (W - 1) = %ld samples; the "
              "multi-resolution STFT loss needs more than 2048", W, hop, (long)hop * (W - 1));
  TrainCall c;
  int rc = train_prologue("svs_unet_train_fwd_loss_mr", params, B, H, W, ws, ws_bytes, c);
  if (rc) return rc;
  const MrTrainWs m = mr_train_layout(B, W, hop, mr_ws);
  if (!mr_ws || mr_ws_bytes < m.total || !svs_aligned16(mr_ws)) { svs_set_error("svs_unet_train_fwd_loss_mr: MR workspace too small (%zu < %zu)", mr_ws_bytes, m.total); return SVS_ERR_WORKSPACE; }
  // d_logit = alpha_l1 * d(L1)/d(logit)                                                   (train.py:281-283,296)
  if ((rc = train_fwd_loss_impl(c, bn_buffers, num_batches_tracked, mix, voc, drop, alpha_l1, mask, losses, stream))) return rc;
  const float* mk = mask ? mask : c.t.mask;
  // waveforms: predicted magnitude (mask * mix, fused into the inverse's load) with the MIXTURE phase, target with its own
  const int64_t cs = (int64_t)H * W;
  const long L = (long)hop * (W - 1);
  if ((rc = svs_istft_tiles_n(mix, cs, W, H, 1, mk, 0, mix_phase, 3, B, 2 * H, hop, W, m.wav_pred, nullptr, stream))) return rc;   // train.py:288
  if ((rc = svs_istft_tiles_n(voc, cs, W, H, 1, nullptr, 0, voc_phase, 3, B, 2 * H, hop, W, m.wav_tgt, nullptr, stream))) return rc; // train.py:291
  if ((rc = svs_mrstft_loss_fwd_bwd(m.wav_pred, m.wav_tgt, B, L, alpha_mr, losses + 1, m.d_wav, m.mr, m.mr_bytes, stream))) return rc;  // train.py:293
  // d_logit += d(alpha_mr * MR)/d(wav) through the inverse STFT and |S| = mask * mix
  return svs_istft_bwd_mask(m.d_wav, mix_phase, mix, mk, c.t.d_logit, 1.0f, B, 2 * H, hop, W, stream);
}

extern "C" int svs_unet_train_bwd_part(const float* params, float* grads, const float* mix, const float* drop, int B, int H, int W,
                                       int part, void* ws, size_t ws_bytes, hipStream_t stream) {
  SVS_REQUIRE(params && grads && mix && part >= 0 && part <= 6, "svs_unet_train_bwd_part: bad arguments");
  TrainCall c;
  const int rc = train_prologue("svs_unet_train_bwd_part", params, B, H, W, ws, ws_bytes, c);
  if (rc) return rc;
  // decoder | whole encoder | conv6 block | conv5..conv1 blocks | everything | conv5 + conv4 blocks | conv3..conv1 blocks
  static const int bits[7] = {1, 2 | 4 | 8, 2, 4 | 8, 15, 4, 8};
  return train_backward_impl(c, grads, mix, drop, stream, bits[part]);
}
