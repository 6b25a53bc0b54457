/* libsvs_hip.so -- C ABI of the MI355X (gfx950) singing-voice-separation hot path.
 *
 * The reference (zouyuoz/SVS-UNet-PyTorch, cited below as <file>:<line>) has no FFI: its hot path
 * is a chain of torch / librosa library calls made from Python.  Each entry point here replaces one
 * of those calls (or a run of them) and is what a maintainer would bind with ctypes -- see
 * INTEGRATION.md for the stub.  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (torch); the library never allocates
 *     caller-visible memory and never synchronises the stream.  Library-owned state, all of it: (1) per device, ONE
 *     high-priority side stream and a handful of events, created on first use by the svs_unet_train_* entry points
 *     (the weight gradients of a backward pass run there, see svs_unet_train_bwd_sync); (2) the table of tuning
 *     switches behind svs_tuning_set (filled from the environment once).  Everything else is stateless;
 *   - scratch space is passed in (void* ws, size_t ws_bytes); the matching *_workspace_bytes query
 *     says how much is needed; 16-byte alignment is required of every tensor pointer;
 *   - activations are fp32 NHWC "views": pointer to channel 0 of pixel 0 plus `ld`, the distance in
 *     floats between consecutive pixels (so a channel slice of a wider buffer -- the decoder's
 *     skip-concat halves, model.py:186-198 -- is addressed without a copy).  With one channel NHWC
 *     and the reference's NCHW coincide, so the network input/output are the reference's tensors;
 *   - return value: 0 = OK, <0 = invalid argument / workspace too small, >0 = hipError_t;
 *     svs_last_error_string() returns a thread-local description of the last failure;
 *   - callable from any host thread and on any stream (torch's autograd engine calls from its own thread): the
 *     per-block and whole-network eval entry points are fully re-entrant; the svs_unet_train_* entry points of one
 *     DEVICE are serialised by a library mutex while they enqueue (they share that device's side stream), and a split
 *     pass (svs_unet_train_fwd_loss, then svs_unet_train_bwd_part 0, 2, 5, 6 / 0, 2, 3 / 0, 1 / 4) must be issued in order by one
 *     caller at a time;
 *   - the device is the one the `stream` argument belongs to; the caller makes it current (hipSetDevice /
 *     torch.cuda.device) around the call.
 */
#ifndef SVS_HIP_H
#define SVS_HIP_H

#include <stddef.h>
#include <stdint.h>

/* identical to the typedef in <hip/hip_runtime_api.h>; repeating it keeps this header free of HIP includes */
typedef struct ihipStream_t* hipStream_t;

#ifdef __cplusplus
extern "C" {
#endif

#define SVS_OK 0
#define SVS_ERR_INVALID (-1)
#define SVS_ERR_WORKSPACE (-2)
#define SVS_ABI_VERSION 1

int svs_version(void);
const char* svs_last_error_string(void);
/* Planner overrides for sweeps, A/B runs and tests -- never needed in production.  `name` is one of
 *   CONV_CFG / CONV_KSPLIT (tile / K-split of the fp32 conv GEMM), CONV_WINDOW (0: the GEMM form of the layers that have an
 *   LDS-window kernel, in the fp32 and the bf16 network; 2 / 3: the fp32 parity window kernel whenever the layer is eligible),
 *   CONV_SKIP (tap skipping of the fp32 conv GEMM, 0: never, 2: wherever the tile allows), SKIP_REDUCE (the split-K reduction
 *   is left out, so that bench.py can time a GEMM kernel alone), WGRAD_CFG / WGRAD_KSPLIT / WGRAD_SKIP / WGRAD_WINDOW (the
 *   same for the weight-gradient GEMM and its window kernel), TRAIN_UNFUSED (one launch per BatchNorm reduction),
 *   TRAIN_ONE_STREAM (weight gradients on the caller's stream), MFMA_SPLIT (1: the fp32 GEMM kernels form their products on
 *   the bf16 MFMA from exact three-limb splits of the fp32 operands -- fp32-accurate, see csrc/mfma_split.h; default off),
 *   CONV_C1_TILED (0: the thread-per-pixel form of the single-channel convolution, 2: the tiled form always),
 *   BF16_CFG / BF16_KSPLIT (tile -- 0: 128x128, 1: 128x64, 4: 64x128 -- and K-split of the bf16 GEMM), BN_INLINE (most partial
 *   rows a BatchNorm apply kernel folds itself instead of waiting for a finalise launch; 0: never; default 128),
 *   CONV_GWINDOW (0: conv2 forward on the GEMM kernel instead of the LDS-window kernel; 2: the window kernel whenever the
 *   layer is eligible; >= 16: that many blocks),
 * or "*" for all; value -1 = planner default ("*", -1: every switch back to what the environment gave at load).  Any other
 * name is refused.  The boolean switches (SKIP_REDUCE, TRAIN_UNFUSED, TRAIN_ONE_STREAM, MFMA_SPLIT) are ON for values > 0
 * only -- 0 and -1 both mean off; the others are valued (0 is a value).  The table is initialised from the environment
 * (SVS_<NAME>) at first use; no compute path reads the environment; entries are atomics (a setter may run beside compute
 * threads). */
int svs_tuning_set(const char* name, long value);

/* ---------------------------------------------------------------------------------------------
 * Synthetic data (bench / tests): the counter-based generator of svs_unet_pytorch_amd/synth.py.
 * out[i] = uniform(seed, offset + i) * scale + shift.                       (SURVEY.md 8d inputs) */
int svs_fill_uniform(float* out, int64_t n, uint32_t seed, uint64_t offset, float scale, float shift,
                     hipStream_t stream);
/* mix = u(seed 0), voc = mix * u(seed 1); counter = flat offset + 2^32 * (first_tile + b).
 * Stands in for SpectrogramDataset.__getitem__ (train.py:86-143) in every synthetic config. */
int svs_fill_tiles(float* mix, float* voc, int B, int H, int W, int64_t first_tile, hipStream_t stream);
/* Dropout2d(0.5) keep-masks (model.py:83,89,95,101,107): out[b*C+c] in {0, 2}. */
/* Training tiles from spectrograms kept in HBM -- SpectrogramDataset.__getitem__, train.py:86-143 (L1 path: magnitudes
 * only).  mix_songs / voc_songs: flat buffers, song s = rows 1..F of its (F+1, T_s) file (DC row dropped, train.py:109-112)
 * at float offset[s], (F, T_s) row-major.  Sample b = song[b], columns [start[b], start[b]+seg) of both tracks (shared
 * start, train.py:121), right zero-padded where the song ends (train.py:129-135).  mix / voc: (B, 1, F, seg). */
int svs_crop_tiles(const float* mix_songs, const float* voc_songs, const int64_t* offset, const int32_t* frames,
                   const int32_t* song, const int32_t* start, int B, int F, int seg, float* mix, float* voc,
                   hipStream_t stream);
/* The phase half of the same items (train.py:103-112): angle = np.angle(unit phasor) = atan2(im, re) as float32; the
 * resident angle buffers are then cropped with svs_crop_tiles exactly like the magnitudes (same shared start). */
int svs_phase_angle(const float* phasor /* n complex64 */, float* angle, int64_t n, hipStream_t stream);
/* Remix and gain augmentation of the same items (csrc/augment.hip; Uhlich et al. 2017, Open-Unmix, Demucs -- the reference's
 * SpectrogramDataset, train.py:86-143, always pairs a song's mixture with its own vocal).  Song storage, DC-row convention,
 * seg % 4 == 0, 16-byte-aligned outputs and right zero-padding are those of svs_crop_tiles; mix_ang / voc_ang are the resident
 * angles of svs_phase_angle, |angle| <= pi.  Item b, element (f, t); A = song_v[b] at column start_v[b] + t, B = song_a[b] at
 * column start_a[b] + t, every value past a song's end 0 (independently for A and B):
 *   song_a[b] >= 0 (remix):  z = g_v V_A cis(phi_vA) + g_a (M_B cis(phi_mB) - V_B cis(phi_vB))       g_v = gain_v[b], g_a = gain_a[b]
 *                            mix = |z|, mix_phase = atan2(Im z, Re z), voc = g_v V_A, voc_phase = phi_vA (0 where padded)
 *   song_a[b] <  0 (gain):   mix = g_v M_A, voc = g_v V_A (one fp32 multiply each), both angles copied; gain_a[b] is not used.
 * Mixture and vocal of a song share one norm (data.py:84-85,105), so M cis(phi_m) - V cis(phi_v) is the accompaniment's STFT and
 * z is, frame for frame, the STFT of the re-mixed waveform.  fp32 throughout, the device library's accurate sincosf / hypotf /
 * atan2f.  mix_ang == voc_ang == NULL is the gain-only form: every item is a gain item, song_a / start_a are never read (they must
 * still be non-null) and the phase outputs must be NULL.  mix_phase == voc_phase == NULL: the phase tiles are not written and no
 * atan2f is computed; mix and voc are bit for bit those of the call with phase outputs.  One angle source or one phase output
 * alone, phase outputs without angle sources, a null table and bad geometry are SVS_ERR_INVALID before any launch.  The kernel
 * trusts its tables as svs_crop_tiles does: song indices in range, 0 <= start <= max(T - seg, 0) (augment.crop_remix checks
 * them on the host).  One launch writes all the tiles.  mix, voc, mix_phase, voc_phase: (B, 1, F, seg). */
int svs_crop_remix_tiles(const float* mix_songs, const float* voc_songs, const float* mix_ang, const float* voc_ang,
                         const int64_t* offset, const int32_t* frames, const int32_t* song_v, const int32_t* start_v,
                         const int32_t* song_a, const int32_t* start_a, const float* gain_v, const float* gain_a, int B, int F,
                         int seg, float* mix, float* voc, float* mix_phase, float* voc_phase, hipStream_t stream);
/* Time-stretch augmentation of the same items (csrc/stretch.hip; Cohen-Hadria, Roebel and Peeters 2019 -- the reference's
 * SpectrogramDataset, train.py:86-143, has no augmentation): a phase vocoder on each source before the mix.  Storage, tables, gains
 * and padding are those of svs_crop_remix_tiles; rate_v / rate_a are Q10 rates q (r = q / 1024; augment.check_stretch_table keeps
 * 512 <= q <= 2048).  The sources are the vocal of A = song_v[b] from column s_v = start_v[b] at q_v, and the accompaniment
 * M cis(phi_m) - V cis(phi_v) of B = song_a[b] from s_a at q_a (song_a[b] < 0: B = A, s_a = s_v, q_a = q_v, the same complex path).
 * For a source S, row f (bin = f + 1) and output frame t:  n = t q, k = s + (n >> 10), alpha = (n & 1023) / 1024,
 *   mag_t = (1 - alpha) |S[k]| + alpha |S[k+1]|,   out_t = mag_t cis(acc_t),   acc_0 = arg S[s],
 *   acc_{t+1} = acc_t + w + wrap(arg S[k+1] - arg S[k] - w),   w = 2 pi ((hop bin) mod n_fft) / n_fft,   wrap to [-pi, pi)
 * (arg of an exactly zero magnitude is 0; columns outside [0, T) are zero), and the item is
 *   z = g_v PV(vocal) + g_a PV(accompaniment):  mix = |z|, mix_phase = arg z, voc = g_v mag_v, voc_phase = acc_v in [-pi, pi],
 * a phase being 0 wherever its magnitude is exactly 0.  The mixture is the sum of the stretched sources, never a stretched mixture.
 * acc is carried as a 32-bit fraction of a turn (exact wrapping integer sums: no error that grows with hop * bin, and the same bits
 * whatever the grid, the batch size or an item's place in the batch); magnitudes, sincosf / atan2f / hypotf are fp32.  The angle
 * sources are required (there is no magnitude-only stretch).  mix_phase == voc_phase == NULL: only mix and voc are written, bit for
 * bit those of the four-output call.  Refused with SVS_ERR_INVALID before any launch: a null pointer or table, one phase output
 * alone, seg % 4 != 0, an output that is not 16-byte aligned, n_fft other than 512 / 1024 / 2048, hop outside 1..n_fft, F outside
 * 1..n_fft / 2 (rows are bins 1..F; augment.crop_stretch passes F == n_fft / 2).  The kernel trusts its tables: song indices in
 * range, 0 <= start, 512 <= q <= 2048 (checked on the host).  One launch, no workspace, no atomics.  Outputs: (B, 1, F, seg). */
int svs_crop_stretch_tiles(const float* mix_songs, const float* voc_songs, const float* mix_ang, const float* voc_ang,
                           const int64_t* offset, const int32_t* frames, const int32_t* song_v, const int32_t* start_v,
                           const int32_t* song_a, const int32_t* start_a, const float* gain_v, const float* gain_a,
                           const int32_t* rate_v, const int32_t* rate_a, int B, int F, int seg, int n_fft, int hop, float* mix,
                           float* voc, float* mix_phase, float* voc_phase, hipStream_t stream);
/* Pitch-shift augmentation of the same items (csrc/pitch.hip; Cohen-Hadria, Roebel and Peeters 2019 -- the reference's
 * SpectrogramDataset, train.py:86-143, has no augmentation): svs_crop_stretch_tiles' phase vocoder with the frequency axis resampled
 * and the phase advance scaled.  Everything is as there; pitch_v / pitch_a are Q10 pitches P (p = P / 1024; augment.check_pitch_table
 * keeps 512 <= P <= 2048; a gain item, song_a[b] < 0, also takes P_a = P_v).  Rows of a source S are bins 1..F and every bin
 * outside 1..F is zero.  For output row f (b = f + 1) and output frame t:  n = t q, k = s + (n >> 10), alpha = (n & 1023) / 1024,
 *   N = 1024 b,  j0 = N div P,  gamma = (N mod P) / P,  j = clamp((2 N + P) div 2 P, 1, F)       (integers; j is j0 or j0 + 1)
 *   tm(i) = (1 - alpha) |S[i, k]| + alpha |S[i, k+1]|,   mag_t = (1 - gamma) tm(j0) + gamma tm(j0 + 1),   out_t = mag_t cis(acc_t)
 *   w = 2 pi ((hop j) mod n_fft) / n_fft,   d = wrap(arg S[j, k+1] - arg S[j, k] - w) to [-pi, pi)
 *   w' = 2 pi ((hop j P) mod (1024 n_fft)) / (1024 n_fft),   acc_0 = arg S[j, s],   acc_{t+1} = acc_t + w' + p d
 * (arg of an exactly zero magnitude is 0; columns outside [0, T) are zero), and the item is
 *   z = g_v PV(vocal) + g_a PV(accompaniment):  mix = |z|, mix_phase = arg z, voc = g_v mag_v, voc_phase = acc_v in [-pi, pi],
 * a phase being 0 wherever its magnitude is exactly 0.  The magnitude is the source's at the fractional bin b / p, the phase follows
 * the nearest source bin (ties up) with its true advance per hop multiplied by p.  At P = 1024 this is svs_crop_stretch_tiles, and
 * voc_phase is bit for bit its voc_phase.  acc is a 32-bit fraction of a turn: w' is an exact integer (hop j P formed in 64 bits),
 * p d is (int64(d) P) >> 10 (the only rounding, below 2^-32 turn per frame), the sums wrap: the same bits whatever the grid, the
 * batch size or an item's place in the batch.  The angle sources are required (there is no magnitude-only shift).
 * mix_phase == voc_phase == NULL: only mix and voc are written, bit for bit those of the four-output call.  Refused with
 * SVS_ERR_INVALID before any launch: a null pointer or table (pitch_v and pitch_a included), one phase output alone, seg % 4 != 0,
 * an output that is not 16-byte aligned, n_fft other than 512 / 1024 / 2048, hop outside 1..n_fft, F outside 1..n_fft / 2 (rows are
 * bins 1..F; augment.crop_pitch passes F == n_fft / 2).  The kernel trusts its tables: song indices in range, 0 <= start,
 * 512 <= q <= 2048, 512 <= P <= 2048 (checked on the host).  One launch, no workspace, no atomics.  Outputs: (B, 1, F, seg). */
int svs_crop_pitch_tiles(const float* mix_songs, const float* voc_songs, const float* mix_ang, const float* voc_ang,
                         const int64_t* offset, const int32_t* frames, const int32_t* song_v, const int32_t* start_v,
                         const int32_t* song_a, const int32_t* start_a, const float* gain_v, const float* gain_a,
                         const int32_t* rate_v, const int32_t* rate_a, const int32_t* pitch_v, const int32_t* pitch_a, int B, int F,
                         int seg, int n_fft, int hop, float* mix, float* voc, float* mix_phase, float* voc_phase, hipStream_t stream);
int svs_dropout_mask(float* out, int B, int C, int layer, uint32_t seed, int step, int rank, hipStream_t stream);
/* The five decoder masks of one step in one launch: out = [B*256 | B*128 | B*64 | B*32 | B*16] floats, each block
 * bit-identical to svs_dropout_mask(layer = 0..4) -- the layout svs_unet_train_* take as `drop`. */
int svs_dropout_masks_all(float* out, int B, uint32_t seed, int step, int rank, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Weight layouts.  Checkpoints keep torch's layouts (Conv2d (N,C,5,5), model.py:48; ConvTranspose2d
 * (C,N,5,5), model.py:79); the MFMA kernels read K-contiguous packings made by these two.
 *   gather packing  wp[n][kh][kw][c]                       = w[n][c][kh][kw]
 *   parity packing  wp[p][n][th][tw][c], p = 2*ph+pw       = w[c][n][ph+2*th][pw+2*tw]
 *                   (the four output-parity sub-convolutions of a stride-2 transposed conv:
 *                    9/6/6/4 taps; block p starts at {0,9,15,21}*N*C floats) */
int svs_pack_weight_gather(const float* w, float* wp, int N, int C, hipStream_t stream);
int svs_pack_weight_parity(const float* w, float* wp, int C, int N, hipStream_t stream);

/* Eval-mode BatchNorm folded into the producing conv's epilogue (model.py:49,81 in .eval()):
 * scale = gamma / sqrt(running_var + eps), shift = beta + (conv_bias - running_mean) * scale. */
int svs_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                const float* conv_bias, float eps, float* scale, float* shift, int C, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Encoder block: Conv2d(k5,s2,p2) (+ folded BN + LeakyReLU) -- replaces self.convK(x), model.py:176-181.
 *   y[b,oh,ow,n] = epi(bias[n] + sum_{kh,kw,c} x[b,2oh-2+kh,2ow-2+kw,c] * wp[n][kh][kw][c])
 *   epi(v) = v                                  if scale == NULL   (training: raw output for BN stats)
 *          = leaky(v*scale[n]+shift[n], slope)  otherwise          (eval: BN folded)
 * Output is (B, (H+1)/2, (W+1)/2, N).  C == 1 (conv1) takes w as wp[25][N] (tap-major).
 * accumulate != 0 adds into y instead of overwriting it. */
size_t svs_enc_block_workspace_bytes(int B, int H, int W, int C, int N);
int svs_enc_block_fwd(const float* x, int64_t ldx, int B, int H, int W, int C,
                      const float* wp, const float* bias, const float* scale, const float* shift, float slope,
                      float* y, int64_t ldy, int N, int accumulate,
                      void* ws, size_t ws_bytes, hipStream_t stream);

/* Decoder block: ConvTranspose2d(k5,s2,p2, output_size=(Ho,Wo)) (+ folded BN + ReLU) -- replaces
 * self.deconvK(cat, output_size=...), model.py:183-196.  x is the (virtually concatenated) input with
 * C channels; wp is the parity packing.  Ho in {2H-1, 2H}, Wo in {2W-1, 2W}. */
size_t svs_dec_block_workspace_bytes(int B, int H, int W, int C, int Ho, int Wo, int N);
int svs_dec_block_fwd(const float* x, int64_t ldx, int B, int H, int W, int C,
                      const float* wp, const float* bias, const float* scale, const float* shift, float slope,
                      float* y, int64_t ldy, int Ho, int Wo, int N, int accumulate,
                      void* ws, size_t ws_bytes, hipStream_t stream);

/* Output block: deconv6 (C -> 1 channel) + sigmoid -- model.py:198-200.  w is torch's (C,1,5,5)
 * layout as-is; bias is a device scalar.  y is (B,1,Ho,Wo). */
int svs_out_block_fwd(const float* x, int64_t ldx, int B, int H, int W, int C,
                      const float* w, const float* bias, float* y, int Ho, int Wo, int apply_sigmoid,
                      hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Backward (autograd of the above; the reference gets these from torch at train.py:299).
 * bwd_data of a conv is a transposed conv with the same weights and vice versa, so:
 *   svs_enc_block_bwd_data  dx (B,H,W,C) = ConvT(dy (B,Ho,Wo,N));  wpar = parity packing of the Conv2d weight
 *   svs_dec_block_bwd_data  dx (B,H,W,C) = Conv (dy (B,Ho,Wo,N));  wgat = gather packing of the ConvT weight
 * N == 1 in svs_dec_block_bwd_data (deconv6) takes w as wp[25][C]. */
int svs_enc_block_bwd_data(const float* dy, int64_t lddy, int B, int Ho, int Wo, int N, const float* wpar,
                           float* dx, int64_t lddx, int H, int W, int C, int accumulate,
                           void* ws, size_t ws_bytes, hipStream_t stream);
int svs_dec_block_bwd_data(const float* dy, int64_t lddy, int B, int Ho, int Wo, int N, const float* wgat,
                           float* dx, int64_t lddx, int H, int W, int C, int accumulate,
                           void* ws, size_t ws_bytes, hipStream_t stream);
/* Weight gradients, written in torch's layout:
 *   enc: dw[n][c][kh][kw] = sum_{b,oh,ow} dy[b,oh,ow,n] * x[b,2oh-2+kh,2ow-2+kw,c]      (N,C,5,5)
 *   dec: dw[c][n][kh][kw] = sum_{b,ih,iw} x[b,ih,iw,c] * dy[b,2ih-2+kh,2iw-2+kw,n]      (C,N,5,5)
 * and bias gradients db[n] = sum dy[...,n] when db != NULL. */
size_t svs_block_bwd_weight_workspace_bytes(int B, int Hs, int Ws, int Cs, int Cl);
int svs_enc_block_bwd_weight(const float* dy, int64_t lddy, int B, int Ho, int Wo, int N,
                             const float* x, int64_t ldx, int H, int W, int C,
                             float* dw, float* db, void* ws, size_t ws_bytes, hipStream_t stream);
int svs_dec_block_bwd_weight(const float* x, int64_t ldx, int B, int H, int W, int C,
                             const float* dy, int64_t lddy, int Ho, int Wo, int N,
                             float* dw, float* db, void* ws, size_t ws_bytes, hipStream_t stream);

/* Which kernel (name as rocprofv3 prints it) and K-split the planner uses for a block call of the given geometry:
 * kind 0 = gather GEMM (svs_enc_block_fwd / svs_dec_block_bwd_data), 1 = parity GEMM (svs_dec_block_fwd /
 * svs_enc_block_bwd_data), 2 = weight gradient (H,W,C: the strided image, N: channels of the windowed image), 3 / 4 = a gather
 * (conv4..conv6) / parity (deconv1..deconv5) layer of the bf16 eval network (svs_unet_forward_eval_bf16): conv_gemm_bf16_kernel
 * with its tile, or the parity_window_bf16_kernel instantiation; <0 for channel counts no bf16 layer has.  5 / 6 = kinds 0 / 1
 * for the call with the folded-BatchNorm epilogue (scale != NULL), the form svs_unet_forward_eval issues for conv2..conv6 /
 * deconv1..deconv5: the planner has rules of its own for those calls (tile, K-split), so the name and the split may differ
 * from kinds 0 / 1 at the same geometry; same name format.  Any other kind is SVS_ERR_INVALID.  Host arithmetic only: no GPU
 * is touched.  Lets bench.py attribute its live HIP-event timings to the kernels of the rocprofv3 summary (kinds 0..2), and
 * the per-layer gates say which kernel a layer of an eval forward launched (kinds 3..6). */
int svs_describe_plan(int kind, int B, int H, int W, int C, int Ho, int Wo, int N, char* buf, size_t buflen);

/* ---------------------------------------------------------------------------------------------
 * Training-mode BatchNorm2d + activation (+ Dropout2d) -- model.py:49-50, 81-83 in .train().
 * raw is the (P = B*H*W, C) conv output.  svs_bn_stats writes per-workgroup partial sums,
 * svs_bn_finalize turns them into batch mean / 1/sqrt(biased var + eps), updates the running
 * statistics (momentum, UNBIASED variance) and num_batches_tracked, and svs_bn_act_apply writes
 * y = leaky((raw-mean)*invstd*gamma+beta, slope) * drop[b][c]   (drop == NULL: no dropout). */
size_t svs_bn_workspace_bytes(int64_t P, int C);
int svs_bn_stats(const float* raw, int64_t ldr, int64_t P, int C, void* ws, size_t ws_bytes, hipStream_t stream);
int svs_bn_finalize(const void* ws, int64_t P, int C, float eps, float momentum,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                    float* save_mean, float* save_invstd, hipStream_t stream);
int svs_bn_act_apply(const float* raw, int64_t ldr, int64_t P, int C, int64_t pixels_per_sample,
                     const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                     float slope, const float* drop, float* y, int64_t ldy, hipStream_t stream);
/* Backward of (BN -> activation -> dropout): d_raw (P,C contiguous), dgamma, dbeta from dy (grad of y). */
int svs_bn_bwd(const float* dy, int64_t lddy, const float* raw, int64_t ldr, int64_t P, int C,
               int64_t pixels_per_sample, const float* gamma, const float* beta,
               const float* save_mean, const float* save_invstd, float slope, const float* drop,
               float* d_raw, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Loss of the training step, train.py:274-283 with model.crit = nn.L1Loss() (config.py:33,44):
 *   loss = mean|mask*mix - voc| + mean|(1-mask)*mix - max(mix-voc,0)|
 * Writes the UNSCALED loss to *loss (device scalar) and d_logit = loss_scale * dloss/dmask * mask*(1-mask)
 * (the gradient w.r.t. deconv6's pre-sigmoid output; loss_scale = alpha_L1, train.py:24,296). */
size_t svs_l1_mask_loss_workspace_bytes(int64_t n);
int svs_l1_mask_loss_fwd_bwd(const float* mask, const float* mix, const float* voc, int64_t n, float loss_scale,
                             float* d_logit, float* loss, void* ws, size_t ws_bytes, hipStream_t stream);
/* The same loss with no gradient -- the eval-mode value of train.py:329-338: three read streams, no d_logit store.  Same
 * blocks, summation order and workspace (svs_l1_mask_loss_workspace_bytes), so *loss is bit for bit what
 * svs_l1_mask_loss_fwd_bwd writes for the same inputs. */
int svs_l1_mask_loss_fwd(const float* mask, const float* mix, const float* voc, int64_t n, float* loss, void* ws,
                         size_t ws_bytes, hipStream_t stream);

/* torch.optim.Adam(lr, betas, eps), no weight decay / amsgrad (model.py:116), over flat buffers.
 * g is multiplied by grad_scale first (1/world for data-parallel mean). step is 1-based.  The hyper-parameters
 * are doubles because torch derives 1-beta and the bias corrections in double before rounding to fp32. */
int svs_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                  double eps, int step, float grad_scale, hipStream_t stream);

/* Optimiser options the reference does not have (it clips nothing and runs plain Adam, model.py:116, train.py:298-300:
 * `optim.zero_grad(); loss.backward(); optim.step()`); csrc/optim.hip.  Both work on device-resident scalars: `stats` is a
 * caller-owned device double[4], zeroed by the caller once, never read by the host inside a step.
 *
 * svs_grad_norm: the L2 norm of grad_scale * g over the flat gradient -- every element widened to double before it is squared,
 * double partial sums in a fixed order (per-thread stride, wave, block, then one finalise block folding the block partials in
 * a fixed tree), no atomics: the same (g, n, alignment of g modulo 16 bytes) gives the same bits.  g may be any 4-byte-aligned
 * pointer.  It writes
 *   stats[0] = the norm,
 *   stats[1] = the clip coefficient of torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6)); 1 when
 *              max_norm <= 0 (clipping off); 0 when the norm is not finite,
 *   stats[2] += 1 when the coefficient is below 1,   stats[3] += 1 when the norm is not finite.
 * ws: svs_grad_norm_workspace_bytes(n) bytes, 8-byte aligned.  Two launches. */
size_t svs_grad_norm_workspace_bytes(int64_t n);
int svs_grad_norm(const float* g, int64_t n, float grad_scale, double max_norm, double* stats, void* ws, size_t ws_bytes,
                  hipStream_t stream);
/* svs_adam_step with decoupled weight decay, clipping, a skip and an average of the weights, in one launch and one pass:
 *   skip:  stats != NULL and stats[1] == 0: nothing is touched -- no NaN reaches p, m, v or ema;
 *   clip:  the gradient is g[i] * gs with the one float product gs = grad_scale * (float)stats[1] (gs = grad_scale when stats
 *          is NULL); with weight_decay == 0, p, m and v are bit for bit those of svs_adam_step at grad_scale = gs;
 *   decay: p *= (float)(1 - lr * weight_decay) before the Adam update, on every element (torch.optim.AdamW's default);
 *   ema:   ema != NULL: ema[i] = d * ema[i] + (1 - d) * p[i] after the update, d = ema_decay in [0, 1), 1 - d derived in double.
 * The bias corrections use the caller's `step`; a skipped step still advances the caller's count. */
int svs_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                   double eps, int step, float grad_scale, double weight_decay, const double* stats, float* ema,
                   double ema_decay, hipStream_t stream);

/* inference.py:100-107: out = mix * mask, or mix * (1 - mask) when invert != 0. */
int svs_apply_mask(const float* mix, const float* mask, float* out, int64_t n, int invert, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Whole-network entry points (host-side orchestration in C++; one call per forward / train step).
 * `params` is the flat fp32 buffer of the 46 trainable tensors in state_dict order (each tensor in
 * torch's layout; offsets from svs_unet_param_offset), `bn_buffers` the flat running_mean/var of the
 * 11 BatchNorms in state_dict order (mean then var per layer; offsets from svs_unet_buffer_offset). */
#define SVS_UNET_NUM_PARAMS 46
#define SVS_UNET_NUM_BN 11
int64_t svs_unet_param_offset(int tensor_index);      /* index == SVS_UNET_NUM_PARAMS -> total floats */
int64_t svs_unet_buffer_offset(int bn_index, int which /*0 mean, 1 var*/);  /* bn_index == 11 -> total */

/* Eval: pack weights + fold BN once per checkpoint, then run forwards. */
size_t svs_unet_prepared_bytes(void);
int svs_unet_prepare_eval(const float* params, const float* bn_buffers, void* prepared, hipStream_t stream);
size_t svs_unet_eval_workspace_bytes(int B, int H, int W);
/* mask = UNet.forward(mix) in eval mode -- model.py:169-201; mix, mask are (B,1,H,W). */
int svs_unet_forward_eval(const void* prepared, const float* mix, float* mask, int B, int H, int W,
                          void* ws, size_t ws_bytes, hipStream_t stream);

/* Train: forward (batch statistics, dropout) + L1 loss + backward, gradients into `grads` (flat,
 * same layout as params; overwritten).  Running stats in bn_buffers and num_batches_tracked (11
 * int64) are updated like torch does.  drop: 5 pointers' worth of masks laid out back to back
 * (B*256, B*128, B*64, B*32, B*16 floats) or NULL for no dropout.  The optimiser step is separate
 * (svs_adam_step) so that a data-parallel caller can all-reduce `grads` in between.
 * svs_unet_ws_offset reports where an intermediate lives inside ws (tests read them). */
size_t svs_unet_train_workspace_bytes(int B, int H, int W);
int svs_unet_train_fwd_bwd(const float* params, float* grads, float* bn_buffers, int64_t* num_batches_tracked,
                           const float* mix, const float* voc, const float* drop, int B, int H, int W,
                           float loss_scale, float* mask /*nullable*/, float* loss,
                           void* ws, size_t ws_bytes, hipStream_t stream);
/* Split form used by the autograd Function (train.py calls model(mix), builds the loss in torch and
 * calls .backward()): forward keeps its intermediates in ws; backward consumes d_mask. */
int svs_unet_train_forward(const float* params, float* bn_buffers, int64_t* num_batches_tracked,
                           const float* mix, const float* drop, int B, int H, int W, float* mask,
                           void* ws, size_t ws_bytes, hipStream_t stream);
int svs_unet_train_backward(const float* params, float* grads, const float* mix, const float* mask,
                            const float* d_mask, const float* drop, int B, int H, int W,
                            void* ws, size_t ws_bytes, hipStream_t stream);
/* Split form for overlapping the data-parallel gradient exchange with the backward pass: forward + loss, then
 * backward part 0 (decoder half: gradients of parameter tensors 24..45, i.e. grads[svs_unet_param_offset(24)..))
 * and part 1 (encoder half: tensors 0..23), or the encoder in two pieces: part 2 (the conv6 block, tensors 20..23 --
 * 13 of the encoder's 17.5 MB) then part 3 (tensors 0..19) -- or part 3 itself as part 5 (conv5 + conv4 blocks, tensors
 * 12..19, 4.1 MB) then part 6 (conv3..conv1, tensors 0..11, 0.26 MB: all that is left to exchange once the backward has
 * ended).  Part 4 is the whole backward in one call.  The caller starts the all-reduce of a piece on a second
 * stream as soon as the part is enqueued.  Same results as svs_unet_train_fwd_bwd.
 * Weight gradients are computed on a library-owned side stream.  The call that ends the pass (part 1, 3, 4 or 6) makes
 * `stream` wait for all of them; after an earlier part, svs_unet_train_bwd_sync(s) makes stream `s` (the one the
 * exchange is issued from) wait for the side-stream work enqueued so far WITHOUT stalling the backward's own stream
 * (`s` must also wait for `stream` itself, e.g. with an event).  The parts of one pass must be issued in order from one
 * host thread; one training pass per device at a time. */
int svs_unet_train_fwd_loss(const float* params, float* bn_buffers, int64_t* num_batches_tracked, const float* mix,
                            const float* voc, const float* drop, int B, int H, int W, float loss_scale,
                            float* mask /*nullable*/, float* loss, void* ws, size_t ws_bytes, hipStream_t stream);
int svs_unet_train_bwd_part(const float* params, float* grads, const float* mix, const float* drop, int B, int H, int W,
                            int part, void* ws, size_t ws_bytes, hipStream_t stream);
int svs_unet_train_bwd_sync(hipStream_t consumer);
/* The reference's FULL objective (train.py:274-296): alpha_l1 * L1 terms + alpha_mr * MultiResolutionSTFTLoss(
 * specific_istft(mask * mix, mix_phase), specific_istft(voc, voc_phase)) -- forward, both losses, d(total)/d(logit).
 * mix_phase / voc_phase: angles (B,1,H,W) (train.py:103-112).  H = n_fft / 2 = 256, 512 or 1024 (the window the tiles were
 * made with, data.py:24), any 0 < hop <= n_fft, W >= 2 and hop * (W - 1) > 2048 (the loss's widest window, whatever the
 * tiles' own: its resolutions are auraloss's 1024 / 2048 / 512); anything else is an error before the first launch.
 * losses[0] = L1 part, losses[1] = MR part, both unscaled.  Follow with svs_unet_train_bwd_part (part 4 = whole backward;
 * or the split forms). */
size_t svs_unet_train_mr_workspace_bytes(int B, int W, int hop);
int svs_unet_train_fwd_loss_mr(const float* params, float* bn_buffers, int64_t* num_batches_tracked, const float* mix,
                               const float* voc, const float* mix_phase, const float* voc_phase, const float* drop, int B, int H,
                               int W, int hop, float alpha_l1, float alpha_mr, float* mask, float* losses, void* ws, size_t ws_bytes,
                               void* mr_ws, size_t mr_ws_bytes, hipStream_t stream);
/* One batch of the validation loop, train.py:317-363 -- the reference's eval-mode objective (train.py:329-346) with no
 * gradient, from the blob of svs_unet_prepare_eval (the fp32 network): svs_unet_forward_eval, svs_l1_mask_loss_fwd into
 * losses[0] and, when BOTH phase pointers are given, the two svs_istft_tiles_n calls of svs_unet_train_fwd_loss_mr (mix with
 * the mask fused on load and mix_phase; voc with voc_phase) and svs_mrstft_loss_fwd_bwd(d_x = NULL) into losses[1]; both
 * unscaled.  Both phase pointers NULL: the L1 part only, losses[1] = 0, any H and W the eval forward takes (hop is ignored;
 * hop = 0 in the workspace query sizes that form).  With phases the early errors of svs_unet_train_fwd_loss_mr apply before
 * the first launch: H = 256 / 512 / 1024, 0 < hop <= 2 H, W >= 2, hop * (W - 1) > 2048.  One phase pointer alone is an error.
 *   mask (nullable): receives the mask, bit for bit svs_unet_forward_eval's.
 *   acc (nullable, 3 doubles on the device): one last one-thread kernel adds, in double, each product rounded before its sum,
 *     acc[0] += alpha_l1 * losses[0]; acc[0] += alpha_mr * losses[1]; acc[1] += losses[0]; acc[2] += losses[1]
 *     -- the host loop `val_sum += ALPHA_L1 * float(l1); val_sum += alpha_mr * float(mr)` bit for bit, with no host sync per
 *     batch (the alphas are doubles for that reason).  The caller zeroes acc before a pass and reads it once after it.
 * Parameters, BatchNorm buffers and num_batches_tracked are not arguments and are never touched; every launch is on `stream`
 * (no side stream); re-entrant like the eval forward.  The workspace holds the eval forward's, the mask, the loss partials and,
 * for hop > 0, two waveforms of B * hop * (W - 1) floats and the MR-STFT workspace -- no gradient buffers. */
size_t svs_unet_eval_loss_workspace_bytes(int B, int H, int W, int hop);
int svs_unet_eval_loss(const void* prepared, const float* mix, const float* voc, const float* mix_phase, const float* voc_phase,
                       int B, int H, int W, int hop, double alpha_l1, double alpha_mr, float* mask /*nullable*/,
                       float* losses /*[2]*/, double* acc /*[3], nullable*/, void* ws, size_t ws_bytes, hipStream_t stream);
/* training = 0: the workspace of svs_unet_forward_eval, 1: of the svs_unet_train_* calls, 2: of svs_unet_forward_eval_bf16
 * (names "cat1" .. "cat5" and "c6" only; see below what they hold). */
int64_t svs_unet_ws_offset(const char* name, int B, int H, int W, int training);  /* bytes, <0 unknown */
/* Inside mr_ws of svs_unet_train_fwd_loss_mr, after the call: "wav_pred", "wav_tgt" (the two re-synthesised waveforms) and
 * "d_wav" (alpha_mr * d(MR part)/d(wav_pred)), each B rows of hop * (W - 1) floats. */
int64_t svs_unet_mr_ws_offset(const char* name, int B, int W, int hop);  /* bytes, <0 unknown */

/* bf16 eval forward (BASELINE configs[4]: "bf16 convs on MFMA"): the same network with bf16 NHWC activations and bf16
 * weights on v_mfma_f32_16x16x32_bf16, fp32 accumulation, BatchNorm folded, mix and mask still fp32.  Not bit-comparable with
 * the fp32 path (activations are rounded to 8 significant bits per layer); tests report its mask L1 against the fp32 forward.
 * prepared_f32 is the blob of svs_unet_prepare_eval.
 * After a forward every layer's output is still in ws, at svs_unet_ws_offset(name, B, H, W, 2) bytes: elements are uint16
 * bf16, NHWC, level k = the input ceil-halved k times, ch[k] = {16, 32, 64, 128, 256, 512}[k - 1] channels per half.
 *   "cat2" .. "cat5": (B, h[k], w[k], 2 ch[k]) -- a pixel is [decoder half | skip half] (pixel pitch 2 ch[k]): the output of
 *                     deconv(6-k) then the output of conv k;
 *   "cat1":           two dense planes of (P1 = B h[1] w[1], 16): the output of deconv5, then the output of conv1;
 *   "c6":             (B, h[6], w[6], 512), the output of conv6.
 * Each buffer starts 256-byte aligned; no kernel writes the padding between one buffer's end and the next one's start. */
size_t svs_unet_prepared_bf16_bytes(void);
int svs_unet_prepare_eval_bf16(const void* prepared_f32, void* prepared_bf16, hipStream_t stream);
size_t svs_unet_eval_bf16_workspace_bytes(int B, int H, int W);
int svs_unet_forward_eval_bf16(const void* prepared_bf16, const float* mix, float* mask, int B, int H, int W, void* ws,
                               size_t ws_bytes, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Signal front/back end (replaces librosa.stft / magphase / istft at data.py:79-80,100-101,159 and
 * torch.istft at train.py:51-58).  n_fft-point periodic-Hann STFT, centred with zero padding,
 * frames = 1 + n_samples / hop.  mag is (n_fft/2+1, frames) float32 row-major; phase (optional)
 * is the unit phasor as interleaved (re, im) float32 pairs, 1+0j where the bin is exactly 0. */
int svs_stft_frames(int64_t n_samples, int hop);
int svs_stft_fwd(const float* y, int64_t n_samples, int n_fft, int hop, float* mag, float* phase,
                 hipStream_t stream);
/* y (hop*(frames-1) samples) = istft(mag * phase), window-sum-square normalised, both n_fft/2 edges
 * trimmed.  phase_is_angle != 0: phase holds angles in radians (train.py:45 torch.polar), else
 * interleaved unit phasors (data.py:159). */
size_t svs_istft_workspace_bytes(int n_fft, int hop, int frames);
int svs_istft(const float* mag, const float* phase, int phase_is_angle, int n_fft, int hop, int frames,
              float* y, void* ws, size_t ws_bytes, hipStream_t stream);
/* Batched / tiled forms (what the streaming path and the training loss use; the two calls above are the 1-channel,
 * (513, frames)-file special case).  A spectrogram is addressed as f-major tiles of `seg` frames and `rows` rows whose
 * first row is bin `first_bin` (0 or 1; rows == 513 - first_bin):
 *     element (channel c, bin k, frame t) = base[c * chan_stride + ((t / seg) * rows + (k - first_bin)) * seg + t % seg]
 * -> a (513, T) file is seg = T, rows = 513, first_bin = 0 (data.py:107); the network's input tiles (n, 1, 512, 128)
 * with the DC row dropped (inference.py:68,84; train.py:109-127) are seg = 128, rows = 512, first_bin = 1, so the
 * forward transform writes network tiles and the inverse reads them with no repacking pass.
 * svs_stft_tiles: y (channels, n_samples) -> mag; frames t >= 1 + n_samples / hop up to frames_alloc are written as
 *   zeros (tile padding, inference.py:90-92).  phase_mode 0: none; 1: frame-major unit phasors [c][t][513] (re, im) --
 *   the streaming form, read back by svs_istft_tiles; 2: f-major (513, T) phasors per channel (the .npy form).
 *   absmax_partial (optional): channels * svs_stft_groups(frames_alloc) per-block maxima of mag (reduce with svs_max). */
int svs_stft_tiles(const float* y, int64_t n_samples, int channels, int n_fft, int hop, float* mag, int64_t chan_stride,
                   int seg, int rows, int first_bin, int frames_alloc, float* phase, int phase_mode,
                   float* absmax_partial, hipStream_t stream);
int svs_stft_groups(int frames_alloc);
/* svs_istft_tiles: y (channels, hop * (frames - 1)) = istft(mag [* mask or * (1 - mask)] * phase).  mask (optional, same
 *   layout as mag) fuses inference.py:100-107.  phase_mode 1: frame-major phasors; 3: angles in the layout of mag
 *   (train.py:33-60, `specific_istft`: the DC row that train.py:41-42 pads back is the absent first_bin row).
 *   0 < hop <= n_fft.  absmax_partial (optional): [channels][svs_istft_groups(hop, frames, channels)] maxima of |y|. */
int svs_istft_tiles(const float* mag, int64_t chan_stride, int seg, int rows, int first_bin, const float* mask, int invert,
                    const float* phase, int phase_mode, int channels, int n_fft, int hop, int frames, float* y,
                    float* absmax_partial, hipStream_t stream);
int svs_istft_groups(int hop, int frames, int channels);
/* The same two transforms for n_fft = 512, 1024 or 2048 -- data.py:24 (`--win_size`, handed to librosa.stft / librosa.istft at
 *   data.py:79,100,159) and the 2048-sample windows of config.py:18-44.  Arguments, layouts and results as svs_stft_tiles /
 *   svs_istft_tiles with 513 -> n_fft / 2 + 1 and 512 -> n_fft / 2 (rows == n_fft / 2 + 1 - first_bin); any other n_fft is an
 *   error that names the three sizes, and so is hop > n_fft.  At n_fft = 1024 they ARE the two functions above (which
 *   require 1024 and forward here), so results are bitwise the same through either name; the 1024-only entry points
 *   (svs_stft_fwd, svs_istft) keep rejecting any other n_fft; svs_istft_bwd_mask and svs_unet_train_fwd_loss_mr take all three. */
int svs_stft_tiles_n(const float* y, int64_t n_samples, int channels, int n_fft, int hop, float* mag, int64_t chan_stride,
                     int seg, int rows, int first_bin, int frames_alloc, float* phase, int phase_mode,
                     float* absmax_partial, hipStream_t stream);
int svs_istft_tiles_n(const float* mag, int64_t chan_stride, int seg, int rows, int first_bin, const float* mask, int invert,
                      const float* phase, int phase_mode, int channels, int n_fft, int hop, int frames, float* y,
                      float* absmax_partial, hipStream_t stream);
/* absmax partials per channel of the two calls above (data.py:84-85,162-164 reduce them); -1 and an error for an n_fft that
 * is not built or a hop outside 1..n_fft */
int svs_stft_groups_n(int n_fft, int frames_alloc);
int svs_istft_groups_n(int n_fft, int hop, int frames, int channels);
/* Host-only query of the inverse's launch plan for (n_fft, hop), read by the launch and by svs_istft_groups_n alike
 * (librosa.istft's overlap-add, data.py:159, for any --hop_size of data.py:25): hops of output that one block owns, rounds of
 * frames it walks for them (16 frames per round; 8 for n_fft = 2048 with hop < 1024, whose blocks have four waves) and the
 * dynamic LDS of a block in bytes.  hop >= n_fft / 2 is the two-frames-per-sample kernel (15 hops, one round). */
int svs_istft_plan_n(int n_fft, int hop, int* hops_per_block, int* rounds, size_t* lds_bytes);
/* Both stems of a mask from ONE launch (inference.py:100-107 computes either `mag * mask` or `mag * (1 - mask)`; the scorer
 * forms the other stem as mix - vocal_est, evaluate.py:50-51): arguments as svs_istft_tiles_n without `invert`, the mask required.
 *   y[0 .. ) (channels, hop * (frames - 1)) = istft(mag * mask * phase), and the same shape stem_stride floats higher
 *   = istft(mag * (1 - mask) * phase); stem_stride >= channels * hop * (frames - 1).  phase_mode 1 or 3.  Magnitude, mask and
 *   phase are read once; each stem goes through transforms of its own, so a mask of all ones leaves stem 1 exactly zero.
 *   absmax_partial (optional): [2][channels][svs_istft_stems_groups_n(...)] maxima of |y|, stem-major.
 * svs_istft_stems_groups_n / svs_istft_stems_plan_n: blocks per channel and the launch plan, as the two queries above (the
 *   overlap-add accumulator of hop < n_fft / 2 holds 12 B per position here, so a block may own fewer hops). */
int svs_istft_stems_n(const float* mag, int64_t chan_stride, int seg, int rows, int first_bin, const float* mask,
                      const float* phase, int phase_mode, int channels, int n_fft, int hop, int frames, float* y,
                      int64_t stem_stride, float* absmax_partial, hipStream_t stream);
int svs_istft_stems_groups_n(int n_fft, int hop, int frames, int channels);
int svs_istft_stems_plan_n(int n_fft, int hop, int* hops_per_block, int* rounds, size_t* lds_bytes);
/* The analysis half of a phase-refinement iteration (Griffin-Lim; MISI of Gunawan and Sen for two stems that must add up to a
 * mixture): the forward transform of svs_stft_tiles_n that writes ONLY the frame-major unit phasors of phase_mode 1 -- no
 * magnitudes, no tile padding, no maxima -- which svs_istft_tiles_n reads back as its `phase`.  The reference writes
 * `mag * mask * phase of the mixture` through librosa.istft (inference.py:100-107, data.py:159) and has no such step.
 *   x (stems, channels, n_samples), stem s at x + s * stem_stride; stems 1 or 2.
 *   mix (channels, n_samples) or NULL.  Given (stems == 2 only), stem s is transformed as x_s + 0.5 * (mix - x_0 - x_1), formed
 *   on load from the three streams; NULL: every stem is transformed as it is.
 *   phase (stems, channels, T, n_fft / 2 + 1, 2) (re, im), T = svs_stft_frames(n_samples, hop), stem s at
 *   phase + s * phase_stem_stride floats (even, at least one stem's size); exactly 1 + 0i where a bin is exactly zero.
 * n_fft = 512, 1024 or 2048, 0 < hop <= n_fft, every view below 2 GiB: anything else is SVS_ERR_INVALID with its own message,
 * before any launch.  16-byte loads when n_samples, hop and stem_stride are multiples of 4 and x and mix are 16-byte aligned. */
int svs_stft_rephase_n(const float* x, int64_t stem_stride, int stems, const float* mix, int64_t n_samples, int channels,
                       int n_fft, int hop, float* phase, int64_t phase_stem_stride, hipStream_t stream);
/* Host-only: the periodic Hann window the forward transform multiplies by (librosa.stft's default window, data.py:79,100):
 * out[m] = sin^2(pi m / n_fft) for m = 0 .. n_fft / 2 (n_fft / 2 + 1 floats; w[n_fft - m] = w[m]), rounded from double. */
int svs_hann_table(int n_fft, float* out);
/* (rows, cols) complex64 -> (cols, rows): f-major phasor files <-> the frame-major form */
int svs_transpose_c64(const float* in, float* out, int rows, int cols, hipStream_t stream);
/* Backward of `specific_istft` (train.py:33-60) fused with the chain rule of |S| = mask * mix (train.py:275,288):
 *   d_logit[b,f,t] += alpha * dL/d|S|[b,f,t] * mix * mask * (1 - mask);   d_wav (B, hop*(frames-1)); the rest
 *   (B,1,n_fft/2,frames).  n_fft = 512, 1024 or 2048 (any other is an error that names them), 0 < hop <= n_fft, frames >= 2. */
int svs_istft_bwd_mask(const float* d_wav, const float* angle, const float* mix, const float* mask, float* d_logit,
                       float alpha, int B, int n_fft, int hop, int frames, hipStream_t stream);
/* Multi-resolution STFT loss of train.py:24-26,287-296 (auraloss.freq.MultiResolutionSTFTLoss with the reference's
 * arguments; restated from its published definition -- csrc/mrstft.hip).  x = predicted, y = target waveform, (B, L):
 *   loss[0] = MR-STFT(x, y);  d_x (optional) = grad_scale * d loss / d x. */
size_t svs_mrstft_workspace_bytes(int B, int64_t L);
int svs_mrstft_loss_fwd_bwd(const float* x, const float* y, int B, int64_t L, float grad_scale, float* loss, float* d_x,
                            void* ws, size_t ws_bytes, hipStream_t stream);
/* data.py:84-85,105 (divide by the mixture's maximum) and data.py:162-164 (peak-normalise to 0.9). */
int svs_absmax(const float* x, int64_t n, float* out /*device scalar*/, void* ws, size_t ws_bytes, hipStream_t stream);
/* out[0] = max(x[0..n)) for x >= 0 (the per-block partials of svs_stft_tiles / svs_istft_tiles) */
int svs_max(const float* x, int64_t n, float* out, hipStream_t stream);
int svs_scale_by_inv(float* x, int64_t n, const float* denom /*device scalar; 0 -> 1*/, float numer, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * BSS-eval in fp64 (csrc/bss.hip): the Gram matrix and projection energies behind svs_unet_pytorch_amd/evaluate.py's
 * _project and _criteria, without forming the projected signals (the formulation is written down in evaluate.py). */
#define SVS_BSS_MAX_SIGNALS 6
#define SVS_BSS_MAX_PAIRS 16
#define SVS_BSS_MAX_LAG 512
#define SVS_BSS_MAX_RHS 16
/* Lagged correlations of signals x[s*ld + m], 0 <= s < nsig, 0 <= m < n, for every window w < nwin of
 * x[:, w*hop .. w*hop + window), each window zero past its end (the halo included) and past n; a whole signal is the one
 * window with window = hop = n.  pairs (HOST array of 3*npairs ints): pair q = (a, b, nlags), 1 <= nlags <=
 * SVS_BSS_MAX_LAG, asks for
 *   out[w*out_stride + off_q + k] = sum_m x_a[m+k] x_b[m],   0 <= k < nlags,   off_q = sum of the nlags of the pairs before q,
 * out_stride >= the sum of the nlags; window, hop, nwin >= 1.  One correlation launch and one reduce launch whatever nwin is.
 * _project's toeplitz(...) block of G is R_ij[q-p] with R_ij[k] = pair (i, j) for k >= 0 and pair (j, i) at -k; its ssef
 * vector D is pair (estimate, reference); a signal's energy is pair (s, s, 1).  Fixed-order sums, no atomics: bitwise
 * reproducible.  The query is 0 for invalid arguments and for a grid too wide for one launch. */
size_t svs_bss_corr_windows_workspace_bytes(int64_t window, int64_t nwin, int npairs, const int* pairs);
int svs_bss_corr_windows(const double* x, int64_t ld, int nsig, int64_t n, int64_t window, int64_t hop, int64_t nwin,
                         const int* pairs, int npairs, double* out, int64_t out_stride, void* ws, size_t ws_bytes,
                         hipStream_t stream);
/* Projection energies |P_S e|^2 = D^T G^-1 D = |y|^2 (G = L L^T, L y = D) of _project, K <= 2 references, filter length
 * flen (order K*flen of G), for nbatch independent systems of one shape (K, flen, nrhs), from correlations `corr` laid out
 * as svs_bss_corr_windows writes them.  System s takes its offsets, absolute in corr, from HOST int64 arrays read before
 * the call returns: gram_off[s*K*K + i*K + j] = offset of R_ij[0 .. flen); rhs_off[s*K*nrhs + r*K + i] = offset of the D
 * block of reference i for right-hand side r.  It writes ynorm2[s*nrhs + r] = |y_r|^2 and status[s] (device) = 0, or
 * 1 + the index of the first pivot of the Cholesky factorisation that was not > 0 (a singular G, e.g. a silent
 * reference: ynorm2 is then meaningless; _project solves by least squares instead).  The launches (expand, one panel and
 * one update launch per 64-column step, norms) do not depend on nbatch; a bad pivot in one system changes no other
 * system's result.  svs_bss_solve_workspace_bytes is the size of
 * one system's matrix; the batched query is 0 for invalid arguments and for a batch too wide for one launch. */
size_t svs_bss_solve_workspace_bytes(int K, int flen, int nrhs);
/* The one-window and one-system forms, kept as the reference the GPU tests hold the windowed and batched forms against.
 * svs_bss_corr is svs_bss_corr_windows with window = hop = n, nwin = 1 and out_stride = the sum of the nlags.
 * svs_bss_solve is one system of svs_bss_solve_batched with its offsets (HOST ints, relative to corr) in the kernel
 * arguments: no table, and a workspace of svs_bss_solve_workspace_bytes.  The same kernels, the same bits. */
size_t svs_bss_corr_workspace_bytes(int64_t n, int npairs, const int* pairs);
int svs_bss_corr(const double* x, int64_t ld, int nsig, int64_t n, const int* pairs, int npairs, double* out,
                 void* ws, size_t ws_bytes, hipStream_t stream);
int svs_bss_solve(const double* corr, int K, int flen, const int* gram_off, const int* rhs_off, int nrhs, double* ynorm2,
                  int* status, void* ws, size_t ws_bytes, hipStream_t stream);
size_t svs_bss_solve_batched_workspace_bytes(int64_t nbatch, int K, int flen, int nrhs);
int svs_bss_solve_batched(const double* corr, int64_t nbatch, int K, int flen, const int64_t* gram_off,
                          const int64_t* rhs_off, int nrhs, double* ynorm2, int* status, void* ws, size_t ws_bytes,
                          hipStream_t stream);
/* BSS-eval images (evaluate.py: bss_eval_images -- stereo stems): the two stages above at the sizes of a stereo two-source
 * problem, through entry points of their own; the limits of the entry points above do not change.  The correlation has
 * kernels of its own; the solve shares the host side and the expand, update and norm kernels of svs_bss_solve_batched,
 * under another pivot rule. */
#define SVS_BSS_IMG_MAX_SIGNALS 12
#define SVS_BSS_IMG_MAX_PAIRS 64
#define SVS_BSS_IMG_MAX_REFS 4
/* svs_bss_corr_windows for up to SVS_BSS_IMG_MAX_SIGNALS signals and SVS_BSS_IMG_MAX_PAIRS pairs: the same windows, the same
 * out[w*out_stride + off_q + k], fixed-order sums, no atomics, bitwise reproducible.  The pair table is copied to the head of
 * the workspace (pairs: HOST array, read before the call returns).  The query is 0 for invalid arguments (a signal index
 * >= SVS_BSS_IMG_MAX_SIGNALS included) and for a grid too wide for one launch. */
size_t svs_bss_img_corr_windows_workspace_bytes(int64_t window, int64_t nwin, int npairs, const int* pairs);
int svs_bss_img_corr_windows(const double* x, int64_t ld, int nsig, int64_t n, int64_t window, int64_t hop, int64_t nwin,
                             const int* pairs, int npairs, double* out, int64_t out_stride, void* ws, size_t ws_bytes,
                             hipStream_t stream);
/* svs_bss_solve_batched for K <= SVS_BSS_IMG_MAX_REFS reference channels (order up to 2048), the same arguments and layout,
 * with the diagonal tile of each step factored once per system, and with rank deficiency handled on the device: with
 * thr = K*flen * 2^-52 * (largest diagonal entry of G), a pivot d with |d| <= thr marks a column that depends on the earlier
 * ones (identical channels, a silent channel); it is skipped, and ynorm2 is the energy of the projection on the span of the
 * remaining columns -- the same span.  skipped[s] (device int) = number of skipped columns of system s.  A pivot below -thr
 * (or NaN) is a failure: status[s] = 1 + the index of the first one (ynorm2 of that system is then meaningless); the
 * factorisation goes on without faulting and no other system's result changes. */
size_t svs_bss_img_solve_batched_workspace_bytes(int64_t nbatch, int K, int flen, int nrhs);
int svs_bss_img_solve_batched(const double* corr, int64_t nbatch, int K, int flen, const int64_t* gram_off,
                              const int64_t* rhs_off, int nrhs, double* ynorm2, int* status, int* skipped, void* ws,
                              size_t ws_bytes, hipStream_t stream);
/* BSS-eval v4 (evaluate.py: bss_eval_v4 -- museval's default mode: distortion filters from the whole track, figures per
 * frame).  It needs what the entry points above never form: the filter coefficients and the projected signals.
 * svs_bss_img_filters_batched is svs_bss_img_solve_batched -- the same arguments, layout, launches, workspace size, ynorm2,
 * status and skipped, bit for bit -- followed by a back substitution L^T c = y in 64-column steps, which leaves the
 * least-squares coefficients C = G^-1 D of _project_images in
 *   coef[(s*nrhs + r)*K*flen + i*flen + tau]   (device, fp64): right-hand side r of system s, reference i, delay tau.
 * A column that the rank rule skipped has the coefficient 0 exactly (no division by its pivot, no NaN): the projection it
 * gives is the projection on the span of the remaining columns.  Coefficients of a system whose status is not 0 are
 * meaningless. */
size_t svs_bss_img_filters_batched_workspace_bytes(int64_t nbatch, int K, int flen, int nrhs);
int svs_bss_img_filters_batched(const double* corr, int64_t nbatch, int K, int flen, const int64_t* gram_off,
                                const int64_t* rhs_off, int nrhs, double* ynorm2, int* status, int* skipped, double* coef,
                                void* ws, size_t ws_bytes, hipStream_t stream);
/* The frames of BSS-eval v4 (csrc/bss_v4.hip): filters applied and the seven energies accumulated in one pass, no projected
 * signal stored.  x[s*ld + m] as svs_bss_corr_windows takes it; frame w < nwin is x[:, w*hop .. w*hop + window), zero before
 * its start, past its end and past n (L = its samples that exist; every frame must start inside the signal).  nsrc, nchan in
 * {1, 2}, R = nsrc*nchan; ref_rows / est_rows (HOST, R ints each): the row of channel c of reference / estimate source j at
 * [j*nchan + c].  coef_one[((j*nchan + c)*nchan + i)*flen + tau]: the filter from channel i of reference j to channel c of
 * estimate j (svs_bss_img_filters_batched of the nsrc systems with K = nrhs = nchan); coef_all[((j*nchan + c)*R + i)*flen + tau]:
 * the same from reference channel i of all R (one system with K = nrhs = R; for nsrc = 1 pass coef_one).  With
 *   p1_c[m] = sum_i sum_tau coef_one[j,c,i,tau] r_{j,i}[m - tau],   pa_c[m] = the same over all R channels with coef_all,
 *   s_c = channel c of reference j,   e_c = channel c of estimate j,   0 <= m < L + flen - 1   (the filters' tail included),
 * it writes sums[(w*nsrc + j)*7 + k] (device, fp64), summed over m and c:
 *   k = 0: s^2   1: (e - s)^2   2: (p1 - s)^2   3: p1^2   4: (pa - p1)^2   5: pa^2   6: (e - pa)^2
 * i.e. SDR = S0/S1, ISR = S0/S2, SIR = S3/S4, SAR = S5/S6 of bss_eval_v4.  Plain fp64 FMAs; per-block partials are added by
 * a second launch in ascending order: no atomics, bitwise reproducible.  Indices are 64-bit.  The query is 0 for invalid
 * arguments and for a grid too wide for one launch. */
size_t svs_bss_project_frames_workspace_bytes(int64_t window, int64_t nwin, int nsrc, int flen);
int svs_bss_project_frames(const double* x, int64_t ld, int nsig, int64_t n, int64_t window, int64_t hop, int64_t nwin,
                           int flen, int nsrc, int nchan, const int* ref_rows, const int* est_rows, const double* coef_one,
                           const double* coef_all, double* sums, void* ws, size_t ws_bytes, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Resampling to the network rate (csrc/resample.hip): the arithmetic half of librosa.load(path, sr=8192, mono=True),
 * data.py:78,94 -- downmix and polyphase FIR resampling; decoding the file stays host code.  The filter is the caller's
 * (svs_unet_pytorch_amd/resample.py designs scipy.signal.resample_poly's Kaiser low-pass, the project's host path; the
 * reference's librosa resamples with soxr, whose filter this does not reproduce).  With half = (ntaps - 1) / 2:
 *   y[i] = sum_j x[j] * taps[i*down - j*up + half],   0 <= j < n_in,   0 <= i < svs_resample_out_len = ceil(n_in*up/down).
 * ntaps is odd; 1 <= up, down <= 2^24 (pass them divided by their gcd: the table has `up` rows).  fp32 taps and fp32
 * accumulation; each output is summed in one fixed order that depends only on i % up (no atomics), so results are bitwise
 * reproducible and do not depend on the batch, on n_in or on where a sample lies in the signal.  Indices are 64-bit.
 * svs_resample_out_len is host arithmetic (-1 for invalid arguments). */
#define SVS_PCM_F32 0 /* float32 samples as they are */
#define SVS_PCM_I16 1 /* int16 / 32768 */
#define SVS_PCM_I32 2 /* int32 / 2^31 (24-bit files arrive left-justified in int32) */
int64_t svs_resample_out_len(int64_t n_in, int up, int down);
/* Packed tap table for svs_resample_poly: ceil(ntaps / up) x up floats, [k][q] = taps[(q*down + half) % up + k*up] (0 past
 * ntaps) -- row q serves every output i with i % up == q, and consecutive outputs read consecutive floats.  `taps` is a
 * device array of ntaps floats.  The query is 0 for invalid arguments. */
size_t svs_resample_table_bytes(int up, int down, int ntaps);
int svs_resample_pack_taps(const float* taps, int ntaps, int up, int down, void* table, hipStream_t stream);
/* x: `batch` signals of n_in sample frames, signal b at element b*ld_in, frame j of it at j*channels (interleaved as a wav
 * file stores them; channels = 1: planar), elements of format fmt (SVS_PCM_*).  downmix != 0: every frame becomes one fp32
 * sample as data.py's load_wav_mono forms it (each channel converted to fp32, added in channel order in fp32, divided
 * by `channels`) and y has `batch` rows; downmix == 0: channel c of signal b is resampled on its own into row
 * b*channels + c.  y row r at y + r*ld_out, n_out floats each.  Needs no workspace.  channels <= 64, at most 65535 rows;
 * filters too long for the LDS (down / up above about 90) are refused. */
int svs_resample_poly(const void* x, int fmt, int channels, int downmix, int64_t n_in, int64_t ld_in, int batch,
                      const void* table, int ntaps, int up, int down, float* y, int64_t ld_out, hipStream_t stream);
/* The launch svs_resample_poly makes for `rows` output rows (host arithmetic, for benchmarks and DESIGN.md section 10):
 * plan[0..8) = outputs per segment W, segments per step S, blocks along i % up, blocks along the signal, steps per block,
 * input samples staged per segment, LDS bytes per block, tap bytes all blocks together read from the packed table. */
int svs_resample_plan(int64_t n_in, int up, int down, int ntaps, int rows, int64_t* plan);

/* The way out (csrc/resample.hip): planar fp32 rows (channel c at x + c*ld_in, n_in samples each; 1 <= channels <= 8) are
 * resampled with the same table, plan and summation order as svs_resample_poly -- acc_c below is bitwise the float that
 * svs_resample_poly writes for that row -- and leave as the interleaved frames a wav file stores: frame i is `channels`
 * consecutive elements at out + i*channels,
 *   v_c = acc_c * gain[c]                       one fp32 multiply; gain (device, `channels` floats) NULL: no multiply
 *   SVS_PCM_F32: v    SVS_PCM_I16: clamp(rintf(v * 32767.0f), -32768, 32767), fp32 multiply, ties to even
 *   SVS_PCM_I32: clamp(rint((double)v * 2147483647.0), -2^31, 2^31 - 1);   NaN -> 0 and +-inf clamp in both integer formats
 * (the I16 rule is libsndfile's float -> short conversion as recalled; parity with the reference's writer, data.py:166, is
 * unpinned).  svs_resample_peaks writes peaks[c] = max_i |acc_c| -- the reference normalises at the rate it writes,
 * data.py:162-166 -- from per-block partials in ws and one reduce launch (no atomics).  1/1 with the one-tap table is a
 * pure encode.  The workspace query is 0 for invalid arguments. */
size_t svs_resample_peaks_workspace_bytes(int64_t n_in, int channels, int up, int down, int ntaps);
int svs_resample_peaks(const float* x, int channels, int64_t n_in, int64_t ld_in, const void* table, int ntaps, int up, int down,
                       float* peaks /* [channels], device */, void* ws, size_t ws_bytes, hipStream_t stream);
int svs_resample_encode(const float* x, int channels, int64_t n_in, int64_t ld_in, const void* table, int ntaps, int up, int down,
                        const float* gain /* [channels] device, nullable */, int out_fmt /* SVS_PCM_* */,
                        void* out /* svs_resample_out_len(n_in, up, down) x channels, interleaved */, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Overlapped tiles with cross-faded masks (csrc/overlap.hip).  inference.py:72-120 cuts a spectrogram into disjoint seg-frame
 * tiles, so the frames at a tile's edges see zero padding in place of their neighbours; here overlapped tile j of a channel
 * covers frames [j * tile_hop, j * tile_hop + seg), each goes through the network alone, and the masks are cross-faded back.
 * Rules, checked before any launch: all sizes positive; seg % 4 == 0, tile_hop % 4 == 0, seg % tile_hop == 0 and
 * seg / tile_hop <= 8; n_tiles * seg < 2^31 (a frame index is an int; every other index is 64-bit); channel strides at least
 * n_tiles * rows * seg and multiples of 4 floats; pointers non-null (except mix) and 16-byte aligned.  tile_hop == seg is legal: both kernels are then copies, bit for bit.
 * svs_overlap_count is host-only (inference.py:72-120's n_tiles disjoint tiles -> overlapped tiles that cover them):
 *   (n_tiles - 1) * (seg / tile_hop) + 1, the last overlapped tile being the last disjoint tile; -1 + error on bad arguments. */
int svs_overlap_count(int n_tiles, int seg, int tile_hop);
/* inference.py:72-120 with overlap, the way in.  tiles: the standard tile addressing of svs_stft_tiles,
 *   (channel c, row r, frame t) = tiles[c*chan_stride + ((t/seg)*rows + r)*seg + t%seg],   t < n_tiles*seg.
 * out: (channels * n_ov, rows, seg) contiguous, n_ov = svs_overlap_count; overlapped tile j of a channel = frames
 * [j*tile_hop, j*tile_hop + seg).  A streaming copy: one thread moves 4 frames of one row as one 16-byte load and store. */
int svs_overlap_tiles(const float* tiles, int64_t chan_stride, int channels, int n_tiles, int rows, int seg, int tile_hop,
                      float* out, hipStream_t stream);
/* inference.py:72-120 with overlap, the way out.  masks: (channels * n_ov, rows, seg), the network's output for
 * svs_overlap_tiles' tiles.  For every frame t of every channel and row
 *   b(t) = sum_j w[t - j*tile_hop] * masks[j][t - j*tile_hop] / sum_j w[t - j*tile_hop]   over the j with 0 <= t - j*tile_hop < seg,
 *   w[i] = sin^2(pi * (i + 0.5) / seg)  (strictly positive; for tile_hop = seg/2 the interior weights sum to 1),
 * summed in ascending j in fp32 (num = fmaf(w, m, num); den += w; one division).  w is computed in double and rounded once.
 * A frame that exactly one tile covers takes that tile's mask value unchanged (no multiply, no divide).
 * mix == NULL: out = b (invert != 0: 1 - b).  mix given (same addressing as out, with mix_chan_stride): out = mix * b or
 * mix * (1 - b), with svs_apply_mask's expressions (inference.py:100-107).
 * out: standard tile addressing with out_chan_stride, so it can be handed to svs_istft_tiles_n / svs_istft_stems_n as `mask`
 * unchanged.  No atomics; bitwise reproducible.  The first call of a process for a seg that cross-fades (tile_hop < seg
 * and n_tiles > 1) uploads w (seg floats, kept per device) and must run outside a stream capture. */
int svs_overlap_blend(const float* masks, int channels, int n_tiles, int rows, int seg, int tile_hop, const float* mix,
                      int64_t mix_chan_stride, int invert, float* out, int64_t out_chan_stride, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Multichannel Wiener filter with EM updates of a local Gaussian model (csrc/wiener.hip; Duong, Vincent and Gribonval; the
 * post-filter of Open-Unmix).  The reference writes `mag * mask * phase of the mixture` (inference.py:100-107, data.py:159) and
 * has no such step.  Two sources (0 vocal, 1 accompaniment), `channels` 1 or 2, bins (t, f) with f over the tiles' rows (the
 * DC bin is absent from the tiles and stays zero in every stem).  With x_c = scale[c] * mag_c * P_c the mixture, one update is
 *     v_j[t,f] = mean_c |y_jc|^2                                   R_j[f] = sum_t y_j y_j^H / (eps + sum_t v_j[t,f])
 *     Cxx[t,f] = sum_j v_j R_j + reg * I                           y_j = v_j R_j Cxx^-1 x
 * from y_0c = scale[c] mag_c mask_c P_c and y_1c = scale[c] mag_c (1 - mask_c) P_c.  All arithmetic is fp64 (identical channels make
 * Cxx = s 11^T + reg I, whose inverse cancels in fp32); loads and stores per bin are fp32.  Open-Unmix's constants are
 * eps = 1e-10 and, for a mixture whose maximum is 1, reg = 1e-7.
 *   mag, mask: the standard tile addressing of svs_stft_tiles with first_bin = 1,
 *     (channel c, row r, frame t) = base[c * chan_stride + ((t / seg) * rows + r) * seg + t % seg],  t < ceil(frames / seg) * seg.
 *   phase: frame-major unit phasors (channels, frames, rows + 1, 2) (re, im), phase_mode 1 of svs_stft_tiles.
 *   scale: [channels] floats on the device (norm_c / max_c' norm_c': both channels on one scale, |x| <= 1).
 *   v: (2, ...) float32, stem j at v + j * v_stem_stride in the tile addressing of ONE channel; zero in the padded frames.
 *   R: (2, rows, 4) doubles (R00, R11, Re R01, Im R01); one channel: R00, the rest zero.
 * Rules, each checked before any launch with its own message: channels 1 or 2; rows a positive multiple of 64; seg a positive
 * multiple of 4; frames >= 1; strides at least one channel's / stem's size and multiples of 4 floats; pointers non-null, 16-byte
 * aligned for mag, mask, v and the stems' magnitudes, 8-byte aligned for phasors, R and the workspace; every view below 2 GiB;
 * reg > 0, eps >= 0; the workspace size.
 * svs_wiener_workspace_bytes: bytes of svs_wiener_model's workspace (0 for invalid arguments).
 * svs_wiener_model: ONE update of the model.  v_prev == R_prev == NULL: the posterior is the masked magnitudes with the
 *   mixture's phase (the first update; mask required).  Given: the posterior is W(v_prev, R_prev) x, formed on the fly (mask is
 *   not read; no y is ever stored between passes).  v may be v_prev and R may be R_prev: a block reads its bins before it writes
 *   them, and R is written by a second launch.  The sums over t run over the real frames only, in fp64, per block of 32 frames
 *   into the workspace and from there in a fixed order (ascending within 16 consecutive runs of blocks, then the runs in
 *   ascending order): no atomics, bitwise reproducible. */
size_t svs_wiener_workspace_bytes(int channels, int rows, int seg, int frames);
int svs_wiener_model(const float* mag, int64_t chan_stride, int seg, int rows, const float* mask, const float* phase,
                     const float* scale, int channels, int frames, const float* v_prev, int64_t v_prev_stem_stride,
                     const double* R_prev, double eps, double reg, float* v, int64_t v_stem_stride, double* R, void* ws,
                     size_t ws_bytes, hipStream_t stream);
/* svs_wiener_stems: y_j = W_j(v, R) x as magnitude tiles (addressing of mag with out_chan_stride) and frame-major unit phasors
 *   (channels, frames, rows + 1, 2), which svs_istft_tiles_n(mask = NULL, phase_mode 1) reads unchanged.  stem 0 or 1: that stem
 *   alone, written at out_mag / out_phase (the stem strides are not read; nothing of the other stem is stored); stem 2: stem j
 *   at out_mag + j * out_mag_stem_stride and out_phase + j * out_phase_stem_stride (even).  The phasor is exactly 1 + 0i where y
 *   is exactly zero (or its magnitude rounds to a float32 zero) and in the DC bin; the magnitude is exactly zero in the padded frames of the last tile.  The stems are on the
 *   common scale of x, so the stereo balance of the mixture is kept. */
int svs_wiener_stems(const float* mag, int64_t chan_stride, int seg, int rows, const float* phase, const float* scale,
                     int channels, int frames, const float* v, int64_t v_stem_stride, const double* R, double reg, int stem,
                     float* out_mag, int64_t out_chan_stride, int64_t out_mag_stem_stride, float* out_phase,
                     int64_t out_phase_stem_stride, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Integrated loudness, ITU-R BS.1770-4 / EBU R 128 (csrc/loudness.hip; the float64 definition is
 * svs_unet_pytorch_amd/loudness.py).  The reference peak-normalises every written stem on its own (data.py:162-166) and has no
 * meter; this is the measurement behind one loudness gain for all stems of a file.
 *   K-weighting: two biquads from the analog prototypes by the bilinear transform, at any rate 4000 <= fs <= 768000.
 *   svs_loudness_coeffs writes c[10] = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (a0 = 1), bit for bit loudness.k_weighting.
 *   Blocks: e_k = floor(k*fs/10); block j covers samples [e_j, e_j+4) (400 ms, 75 % overlap);
 *   svs_loudness_nblocks = the blocks that are complete, e_j+4 <= n: max(0, floor((10*n + 9)/fs) - 3), which is
 *   max(0, floor(10*n/fs) - 3) whenever 10 divides fs; host arithmetic (-1 + error for invalid arguments).
 * svs_loudness_blocks: x holds planar fp32 rows, (stem s, channel c) at x + s*ld_stem + c*ld_ch, n samples each (ld_ch >= n).
 *   stems 1 or 2: the stems are added per sample in fp64 before the filter; channels 1..8, each with weight 1.
 *   z[j] = sum_c mean(y_c[e_j : e_j+4]^2), y the K-weighted signal, for j < svs_loudness_nblocks (nothing is written for
 *   n under 400 ms).  Recurrence and energies are fp64 and the recurrence is exact from the first sample (no warm-up): the
 *   filter state is carried over the whole signal by a scan of per-chunk end states.  Every sum has one fixed order, no
 *   atomics: two calls on the same input give the same bits.  Indices are 64-bit.  z and ws 8-byte aligned.
 * svs_loudness_workspace_bytes: bytes of its workspace (0 for invalid arguments).
 * svs_loudness_gain: one block gates z (absolute gate l_j > -70 with l_j = -0.691 + 10 log10 z_j, then the relative gate 10 LU
 *   under the loudness of what the first kept) and applies the gain rule, all on the device:
 *     info[0] = L = -0.691 + 10 log10(mean z of the kept blocks), -inf when none is kept;   info[1] = kept blocks
 *     peak = max |peaks[i]|, i < npeaks (fp32, device; as svs_resample_peaks leaves them)
 *     target: target_dev[0] when target_dev is given (a device double, e.g. another call's info[0]), else `target`
 *     target NaN: measurement only, info[2] = NaN, info[3] = 0, gain_out untouched (may be NULL with channels = 0)
 *     info[2] = unlimited gain 10^((target - L)/20) (+inf for L = -inf);   cap = ceiling / peak (+inf for peak = 0)
 *     gain_out[c] = (float)min(unlimited, cap) for c < channels, all equal (1 when both are infinite);
 *     info[3] = 1 when the cap was the smaller.
 *   gain_out is what svs_resample_encode takes as `gain`.  No host synchronisation. */
int svs_loudness_coeffs(int fs, double* c /* [10], host */);
int64_t svs_loudness_nblocks(int64_t n, int fs);
size_t svs_loudness_workspace_bytes(int64_t n, int channels, int fs);
int svs_loudness_blocks(const float* x, int stems, int channels, int64_t n, int64_t ld_stem, int64_t ld_ch, int fs,
                        double* z /* [svs_loudness_nblocks], device */, void* ws, size_t ws_bytes, hipStream_t stream);
int svs_loudness_gain(const double* z, int64_t nblocks, const float* peaks, int npeaks, double target,
                      const double* target_dev /* nullable */, double ceiling, float* gain_out /* [channels], device */,
                      int channels, double* info /* [4], device */, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The rest of the EBU R 128 meter: momentary and short-term series, their maxima, the loudness range (EBU Tech 3341 / 3342) and
 * the true peak (ITU-R BS.1770-4 Annex 2) (csrc/loudness.hip, csrc/r128.hip; the float64 definitions are
 * svs_unet_pytorch_amd/loudness.py).  The reference normalises every written stem to its sample peak (data.py:162-166): it has
 * no meter, and a sample peak lies under the peak of the signal the samples stand for (3.01 dB for a sine at fs/4 sampled at
 * 45 degrees).
 *   Windows: a window of `bins` 100 ms bins starting at bin j covers [e_j, e_j+bins); svs_loudness_nwindows = the complete ones,
 *   max(0, floor((10*n + 9)/fs) - (bins - 1)), bins in 1..600; host arithmetic (-1 + error for invalid arguments).  bins = 4 is
 *   svs_loudness_nblocks; bins = 30 is the short-term window, 3 s at a hop of 100 ms.
 * svs_loudness_series: the arguments, rules and workspace of svs_loudness_blocks; the K-weighting passes run ONCE and both series
 *   are summed from the same 100 ms energies, in the order of svs_loudness_blocks (parts, bins, channels ascending):
 *     z_m[j], j < svs_loudness_nwindows(n, fs, 4), bit for bit svs_loudness_blocks' z;   z_s[j], j < svs_loudness_nwindows(n, fs, 30).
 *   Either pointer may be NULL (that series is not written); 8-byte aligned.
 * svs_loudness_stats: one block, all on the device.  With l(v) = -0.691 + 10 log10 v, evaluated as svs_loudness_gain evaluates it:
 *     stats[0] = max_j l(z_m[j]),  stats[1] = max_j l(z_s[j])   (-inf for an empty series)
 *     loudness range after Tech 3342: keep l(z_s[j]) > -70; Gamma = l(mean z of those) - 20; keep those above Gamma as well,
 *     k[0..kept) ascending;  z_lo = k[floor((kept-1)*0.10 + 0.5)],  z_hi = k[floor((kept-1)*0.95 + 0.5)]  (nearest rank)
 *     stats[2] = LRA = l(z_hi) - l(z_lo),  stats[3] = kept,  stats[4] = l(z_lo),  stats[5] = l(z_hi),  stats[6] = z_lo,  stats[7] = z_hi
 *     kept = 0: LRA 0, both loudnesses -inf, both z 0.
 *   The two order statistics are exact selections over the 64-bit patterns of the kept energies (positive doubles order as their
 *   patterns): 64 counting passes, no sort, no atomics; equal values give the same result whichever is picked.  z_m may be NULL
 *   with n_m = 0, z_s with n_s = 0; n_s < 2^31; every pointer 8-byte aligned.
 * svs_loudness_stats_workspace_bytes: bytes of its workspace (0 for invalid n_s).
 * svs_true_peaks: x holds planar fp32 rows addressed as in svs_loudness_blocks, row s*channels + c at x + s*ld_stem + c*ld_ch, n
 *   samples each; the stems are NOT added: every row gets its own pair of peaks.  stems and channels in 1..8.  factor: the
 *   over-sampling factor, 1, 2 or 4; taps: 12*factor + 1 floats on the device, h (loudness.true_peak_taps: a Kaiser-windowed sinc
 *   whose phase 0 is the sample itself).  With x zero outside [0, n), for p = 1 .. factor-1 and 0 <= i < n
 *     y[factor*i + p] = sum_{k=0..11} h[p + factor*k] * x[i + 6 - k]     (acc = fmaf(h, x, acc), k ascending, from 0)
 *     sample_peaks[row] = max_i |x[i]|,    true_peaks[row] = max(sample_peaks[row], max_{i,p} |y[factor*i + p]|)
 *   Either output may be NULL; factor 1 reads no taps (NULL allowed) and gives true peak = sample peak.  One launch over all rows
 *   (a block stages 2048 samples and a 6-sample halo each side in LDS from 16-byte loads) and one reduce launch; max is
 *   order-independent, so the result is bitwise reproducible.  64-bit indices, no atomics, nothing returns to the host.
 * svs_true_peaks_workspace_bytes: bytes of its workspace for rows = stems * channels (0 for invalid arguments). */
int64_t svs_loudness_nwindows(int64_t n, int fs, int bins);
int svs_loudness_series(const float* x, int stems, int channels, int64_t n, int64_t ld_stem, int64_t ld_ch, int fs,
                        double* z_m /* [nwindows(4)], device, nullable */, double* z_s /* [nwindows(30)], device, nullable */,
                        void* ws, size_t ws_bytes, hipStream_t stream);
size_t svs_loudness_stats_workspace_bytes(int64_t n_s);
int svs_loudness_stats(const double* z_m, int64_t n_m, const double* z_s, int64_t n_s, double* stats /* [8], device */, void* ws,
                       size_t ws_bytes, hipStream_t stream);
size_t svs_true_peaks_workspace_bytes(int64_t n, int rows);
int svs_true_peaks(const float* x, int stems, int channels, int64_t n, int64_t ld_stem, int64_t ld_ch,
                   const float* taps /* device, 12*factor + 1 */, int factor, float* sample_peaks, float* true_peaks /* [stems*channels] each, nullable */,
                   void* ws, size_t ws_bytes, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Full-band stems (csrc/fullband.hip; the float64 definition is svs_unet_pytorch_amd/fullband.py).  The network runs at 8,192 Hz,
 * so a stem up-sampled to the file's rate is empty above 4,096 Hz; the reference never leaves the network rate (data.py:151-166
 * writes at --sr).  With x the file's PCM, y the signal the network was given and U the up-sampling FIR of svs_resample_poly,
 *   hi_c[i] = x_c[i] - U(y_c)[i],     out_s,c[i] = norm[c] * U(v_s,c)[i] + g_s,c(i) * hi_c[i],     g_vocal = g, g_accompaniment = 1 - g.
 * svs_fullband_gains: tiles and mask in the standard tile addressing of svs_stft_tiles with first_bin = 1,
 *     (channel c, row r, frame t) = base[c * chan_stride + ((t / seg) * rows + r) * seg + t % seg];
 *   gf[c * frames + t] = sum_r mask * mag / sum_r mag over the top rows / 4 rows (r ascending, num = fmaf(mask, mag, num),
 *   den += mag, one division), for t < frames; where sum_r mag is exactly 0 it is the plain mean of the mask over those rows.
 *   The padded frames of the last tile are neither read into a result nor written.  Rules, checked before any launch: all sizes
 *   positive, rows a multiple of 4, n_tiles * seg < 2^31, frames ending in the last tile, chan_stride at least a channel, pointers
 *   non-null.
 * svs_fullband_mix: stems: planar fp32, (stem s, channel c) at stems + s*ld_stem + c*ld_in, n_in samples each; nstems 1 or 2 (vocal,
 *   accompaniment; invert != 0 with nstems 1: the one stem is the accompaniment).  y: channel c at y + c*ld_y, its first n_in
 *   samples are read.  pcm: the file's frames as it stores them (interleaved, `channels` per frame, SVS_PCM_*, svs_resample_poly's
 *   conversions), n_pcm frames; x is 0 past them.  table, ntaps, up, down: svs_resample_pack_taps' table of U.  The accumulators of
 *   every stem row and of y are bitwise the floats svs_resample_poly writes for those rows.  norm: [channels], device.
 *   gf: svs_fullband_gains' (channels, frames), or NULL for g = 0.  The frame coordinate of output i is i * down / (up * hop):
 *   quotient k and remainder in 64-bit integers, frac = (float)remainder / (float)(up * hop), k and k + 1 clamped to frames - 1,
 *   g = fmaf(frac, gf[k+1] - gf[k], gf[k]);  out = fmaf(g_s, x - acc_y, norm * acc_s) with g_accompaniment = 1.0f - g.
 *   out: planar fp32, (s, c) at out + s*ld_out_stem + c*ld_out, svs_resample_out_len(n_in, up, down) samples each.
 *   1 <= channels <= 8; 1 <= hop <= 2^20; every leading dimension at least what it strides over.  No atomics, bitwise
 *   reproducible, 64-bit indices, nothing returns to the host. */
int svs_fullband_gains(const float* tiles, const float* mask, int64_t chan_stride, int channels, int n_tiles, int rows, int seg,
                       int frames, float* gf /* (channels, frames) */, hipStream_t stream);
int svs_fullband_mix(const float* stems, int nstems, int64_t ld_stem, int64_t ld_in, const float* y, int64_t ld_y, int channels,
                     int64_t n_in, const void* pcm, int pcm_fmt, int64_t n_pcm, const void* table, int ntaps, int up, int down,
                     const float* norm, const float* gf /* nullable */, int frames, int hop, int invert, float* out, int64_t ld_out,
                     int64_t ld_out_stem, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * 24-bit PCM in and out, and TPDF dither for the written stems (csrc/pcm.hip; the float64 / integer definitions are
 * svs_unet_pytorch_amd/pcm.py).  replaces: nothing in the reference -- it writes 16-bit through libsndfile, data.py:166.
 * SVS_PCM_* gets no code for 24 bits: the way in widens to SVS_PCM_I32, the way out is an encoder of its own.
 * svs_pcm24_widen: packed: n_samples little-endian two's-complement 3-byte samples as a wav data chunk stores them (interleaved or
 *   not); out[e] = (int32)(b0 << 8 | b1 << 16 | b2 << 24), the left-justified word with a zero low byte: what SVS_PCM_I32 takes for
 *   a 24-bit file, so svs_resample_poly and svs_fullband_mix read it unchanged.  Rules, checked before any launch: pointers
 *   non-null, n_samples >= 1, packed 4-byte aligned, out 16-byte aligned.  A thread takes 4 samples (3 dwords in, one 16-byte
 *   store out), the last n_samples % 4 go by bytes.
 * svs_pcm_encode_dither: x: planar fp32 rows at the written rate, channel c at x + c*ld_in, `frames` samples each, 1 <= channels
 *   <= 8.  out: interleaved frames as a wav file stores them, int16 for bits = 16, packed 3-byte little-endian for bits = 24.
 *     v = x * gain[c], one fp32 multiply (none when gain is NULL: svs_resample_encode's rule)
 *     u(m) = (svs_u32(seed, m) >> 8) * 2^-24, the counter generator of svs_fill_uniform (synth.uniform); F = first_frame + i
 *     dither 1 (TPDF):             d = u(2*(F*channels + c)) - u(2*(F*channels + c) + 1)
 *     dither 2 (high-passed TPDF): d = u((F + 1)*channels + c) - u(F*channels + c), the first difference of one uniform sequence
 *                                  per channel: the same triangular density per sample, a spectrum that rises 6 dB / octave
 *     dither 0:                    d = 0.  Both differences are exact in fp32.
 *     Q = 2^(bits-1) - 1.  dither 0 at 16 bits: s = rintf(v * 32767.0f), SVS_PCM_I16's rule bit for bit.  Every other case:
 *     s = rint((double)v * Q + (double)d).  Then clamp to [-2^(bits-1), 2^(bits-1) - 1]; NaN -> 0, +-inf clamp.
 *   The counters depend on the absolute frame alone: rows [a, b) encoded with first_frame = a give the bytes of the whole-signal
 *   call, whatever the grid.  Rules, checked before any launch: bits 16 or 24, dither 0..2, channels 1..8, frames >= 1, ld_in >=
 *   frames, first_frame >= 0, out 4-byte aligned, x and out non-null.  A thread owns 4 consecutive frames: a 16-byte load per
 *   channel where x is 16-byte aligned and ld_in % 4 == 0 (scalar loads with the same results otherwise), and 3*channels (24 bits)
 *   or 2*channels (16 bits) whole dwords out, as 16- or 8-byte stores where out is 16-byte aligned; the last frames % 4 frames go
 *   by bytes.  No LDS, no atomics, 64-bit indices, bitwise reproducible, nothing returns to the host. */
int svs_pcm24_widen(const void* packed, int64_t n_samples, int32_t* out, hipStream_t stream);
int svs_pcm_encode_dither(const float* x, int channels, int64_t frames, int64_t ld_in, const float* gain /* [channels] device, nullable */,
                          int bits /* 16 | 24 */, int dither /* 0 none, 1 tpdf, 2 high-passed tpdf */, uint32_t seed,
                          int64_t first_frame, void* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Look-ahead true-peak limiter for loud targets (csrc/limiter.hip; the float64 definition is svs_unet_pytorch_amd/limiter.py,
 * DESIGN.md section 25).  replaces: nothing in the reference -- it peak-normalises every written stem (data.py:162-166), so one
 * transient sets the level of the whole file; svs_loudness_gain's ceiling term does the same to a loudness target.  Three stages on
 * the planar rows at the written rate, one gain curve for ALL rows (stems and channels), so the stems still add up and a stereo
 * file keeps its balance.  All: gfx950, 64-bit indices, no atomics, bitwise reproducible, nothing returns to the host, arguments
 * checked before any launch.
 * svs_limiter_envelope: rows addressed as in svs_true_peaks (row s*channels + c at x + s*ld_stem + c*ld_ch, n samples, zero outside
 *   [0, n)), the same taps and factor (1, 2 or 4; 1 reads no taps, NULL allowed).  With y svs_true_peaks' over-sampled signal,
 *     e[i] = max_row max(|x[i]|, max_{p=1..factor-1} |y_row[factor*i + p]|),   0 <= i < n
 *   The accumulators are bitwise svs_true_peaks' (one shared device helper), so max_i e[i] is its largest true peak.  A block stages
 *   2048 samples of every row in turn with the 6-sample halo from 16-byte loads and keeps the running maxima in registers.
 * svs_limiter_curve: G = G_dev[0] when G_dev is given (a device double: info[2] of svs_loudness_gain), else `G`; ceiling C > 0;
 *   window: 2h + 1 floats on the device (limiter.window(h)), 1 <= h <= 1024.  r = 1 outside [0, n).
 *     r[i] = 1 where G*(double)e[i] <= C, else (float)(C / (G*(double)e[i]))    (one fp64 product, one fp64 division, one rounding)
 *     m[j] = min_{|k|<=h} r[j+k]                                                (exact)
 *     a[i] = sum_{k=-h..h} window[k+h] * m[i+k]                                 (acc = fmaf(w, m, acc), k ascending, from 0)
 *     g[i] = min(a[i], r[i])
 *   G NaN, infinite, zero or negative: g = min(sum of the window, 1) everywhere, which is 1 for limiter.window's tables.
 *   One kernel: a block owns 2048 outputs and stages 2048 + 4h values of r in LDS (one word of padding after every 8: 27 KB at
 *   h = 1024); the minimum is taken by doubling, ceil(log2(2h+1)) passes of one min per element; for the smoothing a lane owns 8
 *   consecutive outputs and slides a register window, one LDS read per 8 fmaf.
 * svs_limiter_apply: x[row][i] *= g[i] in place, row r at x + r*ld_row, 1 <= rows <= 64, one fp32 multiply; 16-byte loads and stores
 *   where x and g are 16-byte aligned and ld_row % 4 == 0, scalar accesses with the same results otherwise. */
int svs_limiter_envelope(const float* x, int stems, int channels, int64_t n, int64_t ld_stem, int64_t ld_ch,
                         const float* taps /* device, 12*factor + 1, nullable for factor 1 */, int factor, float* e /* [n], device */,
                         hipStream_t stream);
int svs_limiter_curve(const float* e, int64_t n, double G, const double* G_dev /* nullable */, double ceiling,
                      const float* window /* [2h + 1], device */, int h, float* g /* [n], device */, hipStream_t stream);
int svs_limiter_apply(float* x, int rows, int64_t n, int64_t ld_row, const float* g, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * YIN fundamental-frequency tracker (csrc/f0.hip; the float64 definition is svs_unet_pytorch_amd/f0.py):
 * steps 1 to 5 of de Cheveigne & Kawahara, JASA 2002.  replaces: nothing in the reference -- it has no pitch estimator.
 * Rows: planar fp32, row r at x + r*ld_row, n samples each.  Frame i of a call is frame F = first_frame + i of the signal and starts
 * at sample t = F*hop; it reads the span = W + tau_max samples from t on.  Only whole frames exist, nothing is zero-padded.  Outputs
 * are indexed [row][i], i < n_frames.  Per frame:
 *     d(tau)  = sum_{j=0..W-1} ((double)(x[t+j] - x[t+j+tau]))^2,  0 <= tau <= tau_max   (one fp32 subtraction; the square and the
 *               sum in fp64: acc = fma(v, v, acc), j ascending, one chain per lag)
 *     S(tau)  = sum_{k=1..tau} d(k)                                                      (fp64 scan over the lags)
 *     d'(0)   = 1;  d'(tau) = (float)(d(tau) * tau / S(tau)),  1 where S(tau) == 0       (rounded once to fp32)
 *     rms     = (float)sqrt(sum_{j=0..W-1} (double)x[t+j]^2 / W)
 *   pick, on the fp32 d':  tau = the smallest tau in [tau_min, tau_max] with (double)d'(tau) < threshold, then stepped to tau + 1
 *     while tau + 1 <= tau_max and d'(tau+1) < d'(tau); found = 1.  No such tau: the smallest tau in the range that attains the
 *     minimum of d', found = 0.  With a, b, c = d'(tau-1), d'(tau), d'(tau+1) in fp64: where tau - 1 >= 1, tau + 1 <= tau_max and
 *     q = a - 2b + c > 0, delta = clamp(0.5 (a - c) / q, -1, 1), else delta = 0.
 *     f0 = (float)(sr / (tau + delta));  ap = b;  voiced = found && rms >= rms_gate  (found alone where svs_f0_pick gets no rms)
 * Rules, checked before any launch, each with its own message: 1 <= rows <= 64; 1 <= W <= 4096; 1 <= tau_max <= 2048; hop >= 1;
 * first_frame, n_frames >= 0 (n_frames = 0 launches nothing); (first_frame + n_frames - 1)*hop + W + tau_max <= n; ld_row >= n for
 * more than one row; 1 <= tau_min < tau_max; threshold and sr positive and finite; rms_gate finite, >= 0; pointers non-null (rms of
 * svs_f0_cmnd and of svs_f0_pick may be NULL) and 4-byte aligned.
 * svs_f0_cmnd: d' [rows][n_frames][tau_max + 1] and, where rms is given, rms [rows][n_frames].  One wave per frame, a block of 64 F
 *   threads owns F <= 4 consecutive frames of one row and stages their span + (F - 1)*hop samples once in LDS (at most 48 KB with the
 *   F rows of d'; F = 1 where hop >= span).  A lane owns 2, 4 or 8 consecutive lags (by tau_max) and slides a register window: two
 *   LDS reads, one of them a broadcast, per 2 / 4 / 8 fp64 FMAs; one word of padding after every 2 / 4 / 8 keeps the lanes on
 *   different banks.  F and the lags of a lane follow from (W, tau_max, hop) alone and no frame reads another's results: a frame's
 *   values depend neither on the grid, nor on first_frame, nor on the frames that share its block.
 * svs_f0_pick: the pick on `count` rows of d' in memory, one wave per row; the two searches are wave minima that keep the smallest
 *   index on ties.
 * svs_f0_track: both in one launch, d' never leaves LDS; the same device functions, so f0, ap, rms and voiced are bitwise those of
 *   svs_f0_cmnd followed by svs_f0_pick, and frames [a, b) with first_frame = a are bitwise those of the whole-signal call.
 * All: gfx950, 64-bit indices, no atomics, bitwise reproducible, nothing returns to the host. */
int svs_f0_cmnd(const float* x, int rows, int64_t n, int64_t ld_row, int W, int tau_max, int hop, int64_t first_frame, int64_t n_frames,
                float* dprime /* [rows][n_frames][tau_max+1] */, float* rms /* [rows][n_frames], nullable */, hipStream_t stream);
int svs_f0_pick(const float* dprime, int64_t count /* rows*n_frames */, int tau_min, int tau_max, double threshold,
                const float* rms /* [count], nullable */, float rms_gate, double sr, float* f0, float* ap, int32_t* voiced, hipStream_t stream);
int svs_f0_track(const float* x, int rows, int64_t n, int64_t ld_row, int W, int tau_min, int tau_max, int hop, int64_t first_frame,
                 int64_t n_frames, double threshold, float rms_gate, double sr, float* f0, float* ap, float* rms, int32_t* voiced,
                 hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Smoothing the pitch track (csrc/f0_smooth.hip; the definition is svs_unet_pytorch_amd/f0.py): K = 7 period
 * candidates per frame from the difference function above, and an exact Viterbi decode over them and one unvoiced state.
 * replaces: nothing in the reference.  All integer arithmetic is int64.
 *   dip:        tau in [tau_min, tau_max] with (tau == tau_min || d'(tau) < d'(tau-1)) && (tau == tau_max || d'(tau) <= d'(tau+1))
 *   candidates: the 7 dips with the smallest d' (equal d': the smaller tau) in ascending tau; count = min(7, dips) >= 1; per kept dip
 *               ap = d'(tau), delta by the pick's parabolic rule, f0 = (float)(sr / (tau + delta)); slots >= count hold 0, 0.f, 0.f
 *   cents:      int32 [tau_max + 1] on the device, built by the host: cents[0] = 0, cents[tau] = rint(1200 log2(sr / tau))
 *   states:     0..6 the frame's candidates, 7 unvoiced; INF = 2^40
 *   obs_t(k):   k < count and rms >= rms_gate: llrint((double)ap_k * 4096) + floor(octave_cost * (cents[tau_min] - cents[tau_k]) / 1200);
 *               k = 7: unvoiced_cost; every other slot: INF
 *   A_t(i, j):  i, j < 7: pitch_cost * |cents[tau_i] - cents[tau_j]| (the stored tau of either frame; an empty slot's 0 reads
 *               cents[0] = 0); one of them 7: switch_cost; both 7: 0
 *   recursion:  delta_0 = obs_0;  delta_t(j) = min_i(delta_{t-1}(i) + A_t(i, j)) + obs_t(j), psi_t(j) the smallest such i;
 *               cost = min_j delta_{T-1}(j), the end state the smallest such j; state[t-1] = psi_t(state[t])
 * svs_f0_dips: the candidate rule on `count` rows of d' in memory, one wave per row: seven rounds of a wave minimum over (d', tau).
 *   Rules: 1 <= tau_min < tau_max <= 2048; sr positive and finite; count >= 0 (0 launches nothing); pointers non-null, 4-byte aligned.
 * svs_f0_candidates: svs_f0_track's arguments and rules, plus cand_tau, cand_f0, cand_ap [rows][n_frames][7] and count [rows][n_frames].
 *   One launch; d' never leaves LDS.  f0, ap, rms and voiced are bitwise svs_f0_track's (the same device functions, csrc/f0_frame.h);
 *   the candidates are bitwise svs_f0_cmnd followed by svs_f0_dips; frames [a, b) with first_frame = a are those of the whole call.
 * svs_f0_viterbi: the decode of every row over ALL n_frames of the call (pieces do not concatenate: the path is the call's best one).
 *   A row is cut into chunks of `chunk` frames: (a) one wave per chunk forms the (min,+) product of its frames' 8x8 matrices
 *   A_t(i,j) + obs_t(j), one entry per lane; (b) one wave per row carries delta across the chunk products; (c) one wave per chunk
 *   reruns its frames from its entry vector and writes psi, 3 bits x 8 per frame; (d) the same launch composes them into an end-state ->
 *   entry-state table; (e) one wave per row walks the tables backwards; (f) each chunk backtraces from its end state and writes
 *   state.  Five launches.  Integer (min,+) products are associative without rounding, so state and cost are bit for bit those of the
 *   sequential recursion for every chunk.  Plain adds and mins, no saturation: every path sum stays below 2^62.
 *   Rules, each with its own message: 1 <= rows <= 64; 0 <= n_frames <= 2^20 (0 launches nothing); chunk in {16, 32, 64, 128};
 *   1 <= tau_min < tau_max <= 2048; rms_gate finite, >= 0; each of the four costs in 0..2^20; pointers non-null, 4-byte aligned, cost
 *   8-byte and the workspace (svs_f0_viterbi_workspace bytes; 0 for arguments it refuses) 16-byte aligned.  A cand_tau outside
 *   0..tau_max is read as the nearer bound.
 * svs_f0_smooth_select: per frame f < count, s = state[f]: s in 0..6: f0 = cand_f0[f][s], ap = cand_ap[f][s], voiced = 1; else the
 *   raw pick's f0 and ap, voiced = 0.
 * All: gfx950, 64-bit indices, no atomics, bitwise reproducible, nothing returns to the host. */
int svs_f0_dips(const float* dprime, int64_t count /* rows*n_frames */, int tau_min, int tau_max, double sr, int32_t* cand_tau /* [count][7] */,
                float* cand_f0 /* [count][7] */, float* cand_ap /* [count][7] */, int32_t* cand_count /* [count] */, hipStream_t stream);
int svs_f0_candidates(const float* x, int rows, int64_t n, int64_t ld_row, int W, int tau_min, int tau_max, int hop, int64_t first_frame,
                      int64_t n_frames, double threshold, float rms_gate, double sr, float* f0, float* ap, float* rms, int32_t* voiced,
                      int32_t* cand_tau, float* cand_f0, float* cand_ap, int32_t* cand_count, hipStream_t stream);
size_t svs_f0_viterbi_workspace(int rows, int64_t n_frames, int chunk);
int svs_f0_viterbi(const int32_t* cand_tau, const float* cand_ap, const int32_t* cand_count, const float* rms, int rows, int64_t n_frames,
                   const int32_t* cents /* [tau_max+1], device */, int tau_min, int tau_max, float rms_gate, int64_t pitch_cost,
                   int64_t switch_cost, int64_t unvoiced_cost, int64_t octave_cost, int chunk, void* workspace,
                   int32_t* state /* [rows][n_frames] */, int64_t* cost /* [rows] */, hipStream_t stream);
int svs_f0_smooth_select(const int32_t* state, const float* cand_f0, const float* cand_ap, const float* raw_f0, const float* raw_ap,
                         int64_t count /* rows*n_frames */, float* f0, float* ap, int32_t* voiced, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVS_HIP_H */
