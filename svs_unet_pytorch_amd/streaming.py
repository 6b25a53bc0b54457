"""End-to-end on-GPU separation of a waveform: STFT -> normalise -> 128-frame tiles -> U-Net mask -> masked
magnitude x mixture phase -> inverse STFT -> peak-normalise, with every intermediate resident in HBM
(BASELINE.json configs[4]).

This is the composition of the reference's three CLI stages without the .npy round trips:
  data.py to_spec   (data.py:78-109)     svs_stft_fwd + svs_absmax + svs_scale_by_inv
  inference.py      (inference.py:65-127) inference.separate's bookkeeping, kept on the device
  data.py to_wave   (data.py:151-166)     svs_istft + peak normalisation
Channels of a stereo signal are separated independently (the reference itself downmixes to mono with
librosa.load(mono=True), data.py:78; a stereo caller gets per-channel masks).  wiener_iters > 0 puts the multichannel Wiener filter
(wiener.py) between the mask and the inverse transform: the channels' masked magnitudes then start one model of both channels, and
the stems are re-filtered from the complex stereo mixture.
"""
from __future__ import annotations

import torch

from . import _lib
from .config import HOP_SIZE, INPUT_LEN, SAMPLE_RATE, WINDOW_SIZE
from .data import istft_from_tiles, istft_stems_from_tiles, stft_to_tiles
from .overlap import blend_masks, check_tile_hop, overlap_tiles
from .rephase import check_phase_iters, refine_phase
from .wiener import check_wiener_iters, wiener_filter


@torch.no_grad()
def separate_spectrogram_device(model, mag: torch.Tensor, seg_len: int = INPUT_LEN, vocal_solo: bool = True, max_batch: int = 256,
                                tile_hop: int | None = None):
    """(F+1, T) magnitude on the GPU -> (F+1, T) separated magnitude on the GPU (inference.py:65-127 semantics).
    tile_hop: None (the default) or seg_len = disjoint seg_len-frame tiles, whatever seg_len is; below seg_len: overlapped tiles every
    tile_hop frames with cross-faded masks (overlap.py)."""
    if tile_hop is None:
        tile_hop = seg_len
    if tile_hop != seg_len:
        check_tile_hop(tile_hop, seg_len)
    crop = mag[1:, :]
    F_, T = crop.shape
    n = T // seg_len + 1
    if T % seg_len == 0:
        n -= 1                                     # the empty last segment is skipped (inference.py:88)
    if n == 0:
        return torch.zeros_like(mag)
    padded = torch.zeros((F_, n * seg_len), dtype=torch.float32, device=mag.device)
    padded[:, :T] = crop
    tiles = padded.view(F_, n, seg_len).permute(1, 0, 2).contiguous().unsqueeze(1)
    out = torch.empty_like(tiles)
    was_training = model.training
    model.eval()
    if tile_hop != seg_len:                        # overlapped tiles -> masks -> out = mix * cross-faded mask, one launch
        ov = overlap_tiles(tiles.view(1, n, 1, F_, seg_len), tile_hop)
        masks = torch.empty_like(ov)
        for s in range(0, ov.shape[0], max_batch):
            masks[s:s + max_batch] = model(ov[s:s + max_batch])
        blend_masks(masks, n, tile_hop, mix=tiles.view(1, n, 1, F_, seg_len), invert=not vocal_solo, out=out.view(1, n, 1, F_, seg_len))
    else:
        for s in range(0, n, max_batch):
            t = tiles[s:s + max_batch]
            mask = model(t)
            _lib.check(_lib.lib().svs_apply_mask(t.data_ptr(), mask.data_ptr(), out[s:s + max_batch].data_ptr(), t.numel(),
                                                 0 if vocal_solo else 1, _lib.stream_ptr()), "svs_apply_mask")
    model.train(was_training)
    full = out[:, 0].permute(1, 0, 2).reshape(F_, n * seg_len)[:, :T]
    return torch.cat([torch.zeros((1, T), dtype=torch.float32, device=mag.device), full], dim=0)


@torch.no_grad()
def separate_waveform(model, y: torch.Tensor, vocal_solo: bool = True, n_fft: int = WINDOW_SIZE, hop: int = HOP_SIZE,
                      peak: float | None = 0.9, max_batch: int = 256, precision: str | None = None, sr_in: int | None = None,
                      sr_out: int | None = None, both_stems: bool = False, tile_hop: int = INPUT_LEN, phase_iters: int = 0,
                      wiener_iters: int = 0):
    """float32 samples (n,) or (channels, n) on the GPU -> separated samples (hop*(T-1),) or (channels, hop*(T-1)).
    both_stems: return (2, ...) stacked [vocal, accompaniment] -- what vocal_solo=True and vocal_solo=False return -- from ONE
    forward transform, one set of network forwards and one inverse launch (data.istft_stems_from_tiles); vocal_solo is
    ignored then.  sr_out and peak apply to every stem and channel on its own, as below.
    sr_in: the rate of y if it is not config.SAMPLE_RATE yet (a file's 44,100 Hz): every channel is first resampled to
    SAMPLE_RATE on the device (resample.resample_poly_gpu, no downmix); None: y is at the network rate already.
    sr_out: the rate to return (a file's 44,100 Hz): the separated channels are resampled from SAMPLE_RATE on the device and
    peak-normalised per channel at THAT rate -> (channels, ceil(hop*(T-1) * sr_out / SAMPLE_RATE)) float32; None: the
    network rate, as always.
    All channels go through ONE forward transform (which writes network tiles and frame-major phasors directly), one
    batched network forward per `max_batch` tiles and ONE inverse transform (which applies the mask on load and
    overlap-adds in LDS); the only other passes are the two per-channel normalisations.
    tile_hop: INPUT_LEN (the default) separates disjoint tiles as the reference does (inference.py:72-120).  A smaller hop (64,
    32: a multiple of 4 that divides INPUT_LEN, at least INPUT_LEN / 8) cuts overlapped tiles out of the transform's tiles
    (overlap.overlap_tiles), runs the network over all of them, and cross-fades their masks into the one mask the inverse
    transform reads (overlap.blend_masks): two more launches, INPUT_LEN / tile_hop times the network forwards.
    phase_iters: 0 (the default) writes the masked magnitude with the mixture's phase, as the reference does.  N > 0 refines the phase
    between the mask and the last inverse (rephase.refine_phase): N Griffin-Lim updates on the requested stem, or, with both_stems,
    N MISI updates that also hand each stem half of what the two fail to add up to; the stems then come from two single-stem
    inverse launches, each with its own phase.
    wiener_iters: 0 (the default) makes exactly the calls above.  N in 1..8 runs the multichannel Wiener filter after the mask (the
    cross-faded one of tile_hop included; wiener.wiener_filter): N updates of a local Gaussian model of the two sources -- a power
    per bin and a spatial covariance per frequency, over one or two channels -- then the stems re-filtered from the complex
    mixture, each with magnitudes and phases of its own, and one inverse launch per requested stem (both_stems: two; else the one
    vocal_solo names).  The stems are on ONE scale for both channels (each channel's maximum relative to the larger), so the
    stereo balance of the mixture is kept and the two stems add up to the mixture but for the regulariser; peak and sr_out apply
    afterwards as before.  One channel is the power-ratio Wiener filter.  More than two channels, and phase_iters > 0 beside
    it (MISI on top of Wiener stems is not built), raise ValueError before any device work."""
    if tile_hop != INPUT_LEN:
        check_tile_hop(tile_hop, INPUT_LEN)
    phase_iters = check_phase_iters(phase_iters)
    wiener_iters = check_wiener_iters(wiener_iters)
    squeeze = y.dim() == 1
    if squeeze:
        y = y[None]
    if wiener_iters:
        if phase_iters:
            raise ValueError(f"wiener_iters {wiener_iters} with phase_iters {phase_iters}: phase refinement (Griffin-Lim / MISI) on top of Wiener-"
                             "filtered stems is out of scope; use one of the two")
        if y.shape[0] > 2:
            raise ValueError(f"wiener_iters {wiener_iters} with {y.shape[0]} channels: the multichannel Wiener filter is built for 1 or 2 channels")
    if sr_in is not None and sr_in != SAMPLE_RATE:
        from .resample import resample_poly_gpu
        y = resample_poly_gpu(y.contiguous().float(), SAMPLE_RATE, sr_in)
    tiles, phase, norm, T = stft_to_tiles(y, n_fft, hop, INPUT_LEN)
    L = _lib.lib()
    C, n_tiles = tiles.shape[:2]
    for c in range(C):                                           # divide by the channel's maximum magnitude (data.py:84-85,105)
        _lib.check(L.svs_scale_by_inv(tiles[c].data_ptr(), tiles[c].numel(), norm[c:].data_ptr(), 1.0, _lib.stream_ptr()), "svs_scale_by_inv")
    flat = tiles.view(C * n_tiles, 1, tiles.shape[3], tiles.shape[4])
    if tile_hop != INPUT_LEN:
        flat = overlap_tiles(tiles, tile_hop)                    # (C * n_ov, 1, rows, INPUT_LEN)
    mask = torch.empty_like(flat)
    was_training, was_precision = model.training, model.eval_precision
    try:
        model.eval()
        if precision is not None:                                # "bf16": the convolutions run on the bf16 MFMA (configs[4])
            model.eval_precision = precision
        for s in range(0, flat.shape[0], max_batch):
            mask[s:s + max_batch] = model(flat[s:s + max_batch])
    finally:                                                     # a failing forward must not leave the model in another mode
        model.eval_precision = was_precision
        model.train(was_training)
    if tile_hop != INPUT_LEN:
        mask = blend_masks(mask, n_tiles, tile_hop)              # back to one mask value per frame, in the layout of `tiles`
    if wiener_iters:                                             # stems with magnitudes and phases of their own: one inverse per stem
        want = (0, 1) if both_stems else ((0,) if vocal_solo else (1,))
        smag, sphase = wiener_filter(tiles, mask.view(tiles.shape), phase, norm, T, wiener_iters, stems=want)
        out = torch.stack([istft_from_tiles(smag[s], None, sphase[s], T, n_fft=n_fft, hop=hop, peak=None if sr_out is not None else peak)
                           for s in range(len(want))])
        out = out.view(len(want) * C, out.shape[2])
    elif phase_iters and both_stems:                             # MISI: each stem ends with its own phase, so two single-stem inverses
        ymix = y[:, :hop * (T - 1)].float().clone(memory_format=torch.contiguous_format)
        for c in range(C):                                       # the mixture at the scale of the tiles: one pass per call, not per iteration
            _lib.check(L.svs_scale_by_inv(ymix[c].data_ptr(), ymix.shape[1], norm[c:].data_ptr(), 1.0, _lib.stream_ptr()), "svs_scale_by_inv")
        refined = refine_phase(tiles, mask, phase, T, phase_iters, stems=2, mix=ymix, n_fft=n_fft, hop=hop)
        out = torch.stack([istft_from_tiles(tiles, mask, refined[s], T, invert=bool(s), n_fft=n_fft, hop=hop,
                                            peak=None if sr_out is not None else peak) for s in range(2)])
        out = out.view(2 * C, out.shape[2])
    elif both_stems:                                             # (2 * C, n): the stems are further channels to everything below
        out = istft_stems_from_tiles(tiles, mask, phase, T, n_fft=n_fft, hop=hop, peak=None if sr_out is not None else peak)
        out = out.view(2 * C, out.shape[2])
    else:
        if phase_iters:                                          # Griffin-Lim on the requested stem
            phase = refine_phase(tiles, mask, phase, T, phase_iters, stems=1, invert=not vocal_solo, n_fft=n_fft, hop=hop)[0]
        out = istft_from_tiles(tiles, mask, phase, T, invert=not vocal_solo, n_fft=n_fft, hop=hop, peak=None if sr_out is not None else peak)
    if sr_out is not None:
        from .resample import resample_poly_gpu
        out = resample_poly_gpu(out, int(sr_out), SAMPLE_RATE)
        if peak is not None:                                     # data.py:162-164 at the rate that is returned
            ws = torch.empty(4096, dtype=torch.uint8, device=out.device)
            pk = torch.empty(out.shape[0], dtype=torch.float32, device=out.device)
            for c in range(out.shape[0]):
                _lib.check(L.svs_absmax(out[c].data_ptr(), out.shape[1], pk[c:].data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "svs_absmax")
                _lib.check(L.svs_scale_by_inv(out[c].data_ptr(), out.shape[1], pk[c:].data_ptr(), float(peak), _lib.stream_ptr()), "svs_scale_by_inv")
    if both_stems:
        out = out.view(2, C, out.shape[1])
        return out[:, 0] if squeeze else out
    return out[0] if squeeze else out


def kept_length(n_encoded: int, n_source: int):
    """(frames to keep, zero frames to append) that turn n_encoded written frames into exactly n_source: a separated signal
    is short of its source by less than one hop at the network rate (the inverse STFT returns hop * (T - 1) samples; STFT ->
    iSTFT and the zero-phase FIR add no delay), and rounding up twice in the two rate changes can leave it a frame long."""
    n_encoded, n_source = int(n_encoded), int(n_source)
    if n_encoded < 0 or n_source < 0:
        raise ValueError(f"frame counts must not be negative, got {n_encoded}, {n_source}")
    keep = min(n_encoded, n_source)
    return keep, n_source - keep


def separated_frames(n_source: int, sr: int, hop: int = HOP_SIZE):
    """Frames separate_to_wav encodes for a file of n_source frames at rate sr, before keep_length: to the network rate
    (ceil), whole hops of it (the centred STFT has 1 + n // hop frames, the inverse returns hop * (T - 1) samples), and back
    (ceil)."""
    n8 = -((-int(n_source) * SAMPLE_RATE) // int(sr))
    return -((-(hop * (n8 // hop)) * int(sr)) // SAMPLE_RATE)


@torch.no_grad()
def separate_to_wav(model, src_path: str, dst_path: str, *, vocal_solo: bool = True, precision: str | None = None,
                    subtype: str = "PCM_16", keep_length: bool = True, n_fft: int = WINDOW_SIZE, hop: int = HOP_SIZE,
                    dst_accomp_path: str | None = None, tile_hop: int = INPUT_LEN, phase_iters: int = 0, wiener_iters: int = 0):
    """wav file -> separated wav file at the same rate and channel count, everything between the two files on the device:
    the PCM is copied as the file stores it, resample.resample_poly_gpu (no downmix) brings every channel to SAMPLE_RATE,
    separate_waveform(peak=None) separates them, and resample.resample_encode_gpu resamples back to the file's rate,
    peak-normalises to 0.9 with one gain for all channels (data.py:162-164), converts to `subtype` ("PCM_16", "PCM_32",
    "FLOAT") and interleaves; only those samples return to the host.  keep_length: the frames are cut or zero-padded to the
    source's frame count (kept_length), so the file lines up sample for sample with the source's stems.  n_fft / hop: the
    window and hop of the two transforms (data.WINDOW_SIZES; the network is fully convolutional, so a checkpoint trained at
    another geometry runs on the n_fft / 2 rows of that window).  dst_accomp_path: also write the accompaniment there, from the
    same pass (separate_waveform(both_stems=True)): dst_path then holds the vocal whatever vocal_solo says, and each file is
    encoded with its own common gain at peak 0.9.  tile_hop: separate_waveform's (overlapped tiles with cross-faded masks when it
    is below INPUT_LEN).  phase_iters: separate_waveform's (Griffin-Lim updates of the written stem's phase, MISI updates with
    dst_accomp_path).  wiener_iters: separate_waveform's (the multichannel Wiener filter after the mask, for files of one or two
    channels; the written stems keep the mixture's stereo balance, one gain per file).  Returns the (frames, channels) written
    (per file)."""
    if check_wiener_iters(wiener_iters) and phase_iters:
        raise ValueError(f"wiener_iters {wiener_iters} with phase_iters {phase_iters}: phase refinement (Griffin-Lim / MISI) on top of Wiener-filtered "
                         "stems is out of scope; use one of the two")
    from fractions import Fraction

    import numpy as np
    from scipy.io import wavfile

    from .resample import resample_encode_gpu, resample_poly_gpu
    rate, data = wavfile.read(src_path)
    if data.dtype.kind == "u":                                   # 8-bit files: offset binary, converted on the host
        data = (data.astype(np.float32) - 128.0) / 128.0
    elif data.dtype not in (np.int16, np.int32):
        data = data.astype(np.float32)
    n_source = data.shape[0]
    channels = data.shape[1] if data.ndim == 2 else 1
    dev = model._flat.device
    if separated_frames(n_source, rate, hop) == 0:
        raise ValueError(f"{src_path}: {n_source} frames at {rate} Hz are shorter than one hop ({hop} samples at {SAMPLE_RATE} Hz)")
    pcm = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    fr = Fraction(SAMPLE_RATE, int(rate))
    y = resample_poly_gpu(pcm, fr.numerator, fr.denominator, channels=channels, downmix=False)
    y = y[None] if y.dim() == 1 else y                            # (channels, n) at the network rate
    sep = separate_waveform(model, y, vocal_solo=vocal_solo, n_fft=n_fft, hop=hop, peak=None, precision=precision,
                            both_stems=dst_accomp_path is not None, tile_hop=tile_hop, phase_iters=phase_iters, wiener_iters=wiener_iters)
    for stem, path in ((sep, dst_path),) if dst_accomp_path is None else ((sep[0], dst_path), (sep[1], dst_accomp_path)):
        enc = resample_encode_gpu(stem, fr.denominator, fr.numerator, fmt=subtype, peak=0.9, common_gain=True)
        if keep_length:
            keep, pad = kept_length(enc.shape[0], n_source)
            enc = torch.nn.functional.pad(enc[:keep], (0, 0, 0, pad))
        out = enc.cpu().numpy()
        wavfile.write(path, int(rate), out[:, 0] if channels == 1 else out)
    return out.shape
