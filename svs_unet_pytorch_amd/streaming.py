"""End-to-end on-GPU separation, every intermediate resident in HBM (BASELINE.json configs[4]): the composition of the reference's
three CLI stages without the .npy round trips (data.py:78-109 to_spec, inference.py:65-127, data.py:151-166 to_wave).

The stages of separate_waveform, in order, each written once:

    resample        sr_in -> SAMPLE_RATE per channel (resample.resample_poly_gpu), if the caller's rate differs
    tiles           data.stft_to_tiles: ONE forward transform writes network tiles and frame-major phasors; then each channel is
                    divided by its maximum magnitude (data.py:84-85,105)
    overlap         tile_hop < INPUT_LEN only: overlap.overlap_tiles cuts overlapped tiles out of the disjoint ones
    network         _network_masks: the model over max_batch tiles at a time, the only such loop of the inference path
    blend           tile_hop < INPUT_LEN only: overlap.blend_masks cross-fades the masks back to one value per frame
    stems           per requested stem (magnitude tiles, mask, phasors, invert): the shared tiles and mask with the mixture's
                    phasors; or with rephase.refine_phase's (phase_iters: Griffin-Lim for one stem, MISI for two); or
                    wiener.wiener_filter's own tiles and phasors with no mask (wiener_iters)
    inverse         data.istft_from_tiles per stem, which applies the mask on load; the plain two-stem case is ONE launch
                    (data.istft_stems_from_tiles)
    f0              f0= only: the vocal stem's pitch track at the network rate (f0.track_gpu), one launch
    peak            every stem and channel scaled to `peak` on its own (data.py:162-164), after the resampling to sr_out if any

separate_spectrogram_device is the tiles / overlap / network / blend part for a magnitude that exists already (inference.py:65-127;
inference.separate is its host wrapper), and separate_to_wav puts the file's PCM in front of separate_waveform and the fused
resample + encode (resample.resample_encode_gpu) behind it -- or, with fullband=, fullband.fullband_mix_gpu, which also shares the
file's band above the network's out between the stems.  Channels of a stereo signal are separated independently (the reference
itself downmixes to mono with librosa.load(mono=True), data.py:78); only the Wiener filter models both channels together.
"""
from __future__ import annotations

import torch

from . import _lib
from .config import HOP_SIZE, INPUT_LEN, SAMPLE_RATE, WINDOW_SIZE
from .data import _scale_rows, istft_from_tiles, istft_stems_from_tiles, stft_to_tiles
from .fullband import check_fullband
from .overlap import blend_masks, check_tile_hop, overlap_tiles
from .rephase import check_phase_iters, refine_phase
from .wiener import check_wiener_iters, wiener_filter


def check_refinement(phase_iters: int, wiener_iters: int, channels: int | None = None):
    """(phase_iters, wiener_iters) as checked ints.  Raises ValueError for a count out of range, for the two together (MISI on top
    of Wiener stems is not built) and, if `channels` is given, for the Wiener filter on more than two channels."""
    phase_iters, wiener_iters = check_phase_iters(phase_iters), check_wiener_iters(wiener_iters)
    if wiener_iters and phase_iters:
        raise ValueError(f"wiener_iters {wiener_iters} with phase_iters {phase_iters}: phase refinement (Griffin-Lim / MISI) on top of Wiener-"
                         "filtered stems is out of scope; use one of the two")
    if wiener_iters and channels is not None and channels > 2:
        raise ValueError(f"wiener_iters {wiener_iters} with {channels} channels: the multichannel Wiener filter is built for 1 or 2 channels")
    return phase_iters, wiener_iters


def _network_masks(model, tiles: torch.Tensor, max_batch: int, precision: str | None = None):
    """(N, 1, rows, seg) tiles -> (N, 1, rows, seg) masks: the model in eval mode (and at `precision`, if given: "bf16" runs the
    convolutions on the bf16 MFMA, configs[4]) over max_batch tiles at a time.  A failing forward included, the model is left in
    the mode and at the precision it came with."""
    masks = torch.empty_like(tiles)
    was_training, was_precision = model.training, getattr(model, "eval_precision", None)
    try:
        model.eval()
        if precision is not None:
            model.eval_precision = precision
        for s in range(0, tiles.shape[0], max_batch):
            masks[s:s + max_batch] = model(tiles[s:s + max_batch])
    finally:
        if was_precision is not None:
            model.eval_precision = was_precision
        model.train(was_training)
    return masks


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
    tiles = padded.view(F_, n, seg_len).permute(1, 0, 2).contiguous().view(1, n, 1, F_, seg_len)
    out = torch.empty_like(tiles)
    if tile_hop != seg_len:                        # out = mix * cross-faded mask, one launch
        masks = _network_masks(model, overlap_tiles(tiles, tile_hop), max_batch)
        blend_masks(masks, n, tile_hop, mix=tiles, invert=not vocal_solo, out=out)
    else:
        masks = _network_masks(model, tiles[0], max_batch)
        _lib.check(_lib.lib().svs_apply_mask(tiles.data_ptr(), masks.data_ptr(), out.data_ptr(), tiles.numel(), 0 if vocal_solo else 1,
                                             _lib.stream_ptr()), "svs_apply_mask")
    full = out[0, :, 0].permute(1, 0, 2).reshape(F_, n * seg_len)[:, :T]
    return torch.cat([torch.zeros((1, T), dtype=torch.float32, device=mag.device), full], dim=0)


@torch.no_grad()
def separate_waveform(model, y: torch.Tensor, vocal_solo: bool = True, n_fft: int = WINDOW_SIZE, hop: int = HOP_SIZE,
                      peak: float | None = 0.9, max_batch: int = 256, precision: str | None = None, sr_in: int | None = None,
                      sr_out: int | None = None, both_stems: bool = False, tile_hop: int = INPUT_LEN, phase_iters: int = 0,
                      wiener_iters: int = 0, aux: dict | None = None, f0=None):
    """float32 samples (n,) or (channels, n) on the GPU -> separated samples (hop*(T-1),) or (channels, hop*(T-1)), through the
    stages the module docstring lists.  With the defaults that is ONE forward transform, one network forward per `max_batch` tiles,
    ONE inverse transform and the two per-channel normalisations, as the reference computes it.
    vocal_solo: the stem to return, the vocal (tiles * mask) or the accompaniment (tiles * (1 - mask)).
    both_stems: return (2, ...) stacked [vocal, accompaniment] -- what vocal_solo=True and vocal_solo=False return -- from the same
    transform and forwards; vocal_solo is ignored then.
    peak: every stem and channel is scaled to this maximum on its own, at the rate that is returned; None leaves the amplitude.
    sr_in: the rate of y if it is not config.SAMPLE_RATE (a file's 44,100 Hz); every channel is resampled first, with no downmix.
    sr_out: the rate to return -> (channels, ceil(hop*(T-1) * sr_out / SAMPLE_RATE)); None: the network rate.
    tile_hop: INPUT_LEN (the default) separates disjoint tiles (inference.py:72-120).  64 or 32 (overlap.check_tile_hop) runs the
    network over overlapped tiles and cross-fades their masks: two more launches, INPUT_LEN / tile_hop times the forwards.
    phase_iters: N > 0 refines the phase between the mask and the last inverse (rephase.refine_phase): N Griffin-Lim updates of the
    requested stem or, with both_stems, N MISI updates; each stem then has phasors of its own and an inverse launch of its own.
    wiener_iters: N in 1..8 runs the multichannel Wiener filter after the (blended) mask (wiener.wiener_filter), for one or two
    channels: the requested stems are re-filtered from the complex mixture, on ONE scale for both channels, so the stereo balance
    is kept and the two stems add up to the mixture but for the regulariser; one inverse launch per stem.
    check_refinement's rules are a ValueError before any device work.
    aux: a dict that receives what a post-filter at another rate needs (fullband.py): "y" (the (channels, n) signal at the network rate
    that was transformed), "tiles", "mask" (the one the stems were made from, in the layout of the tiles), "norm" and "frames".
    f0: True, or a dict of f0.track_gpu's keywords (fmin, fmax, W, hop, threshold, rms_gate, smooth -- True or the four costs: the decoded
    track of csrc/f0_smooth.hip, three entry points more): the call returns (stems, f0.Track) -- the
    pitch track of the VOCAL stem (f0.py, csrc/f0.hip), from the mean of its channels at SAMPLE_RATE as the inverse transform leaves it
    (scaled to `peak` where that rate is the one returned), after the Wiener or phase stages and before the resampling to sr_out: ONE
    svs_f0_track launch, nothing waits for the host.  The stems are those of the call without it.  vocal_solo=False without
    both_stems has no vocal stem to track: a ValueError before any device work."""
    f0_options = None
    if f0 is not None and f0 is not False:
        from .f0 import check_options
        f0_options = check_options(f0)
        if not (vocal_solo or both_stems):
            raise ValueError("f0= tracks the vocal stem, and vocal_solo=False without both_stems returns none")
    if tile_hop != INPUT_LEN:
        check_tile_hop(tile_hop, INPUT_LEN)
    phase_iters, wiener_iters = check_refinement(phase_iters, wiener_iters)       # before the waveform or the model is looked at
    squeeze = y.dim() == 1
    if squeeze:
        y = y[None]
    check_refinement(phase_iters, wiener_iters, channels=y.shape[0])
    if sr_in is not None and sr_in != SAMPLE_RATE:
        from .resample import resample_poly_gpu
        y = resample_poly_gpu(y.contiguous().float(), SAMPLE_RATE, sr_in)
    tiles, phase, norm, T = stft_to_tiles(y, n_fft, hop, INPUT_LEN)
    C, n_tiles = tiles.shape[:2]
    _scale_rows(tiles.view(C, -1), 1.0, maxima=norm)             # divide by the channel's maximum magnitude (data.py:84-85,105)
    if tile_hop != INPUT_LEN:                                    # (C * n_ov, 1, rows, INPUT_LEN) and back to the layout of `tiles`
        mask = blend_masks(_network_masks(model, overlap_tiles(tiles, tile_hop), max_batch, precision), n_tiles, tile_hop)
    else:
        mask = _network_masks(model, tiles.view(C * n_tiles, 1, tiles.shape[3], tiles.shape[4]), max_batch, precision)
    if aux is not None:
        aux.update(y=y, tiles=tiles, mask=mask, norm=norm, frames=T)

    # the stems: per requested stem what a single-stem inverse takes -- (magnitude tiles, mask, phasors, invert)
    inverts = (False, True) if both_stems else (not vocal_solo,)
    if wiener_iters:                                             # magnitudes and phasors of the stems' own, no mask
        smag, sphase = wiener_filter(tiles, mask.view(tiles.shape), phase, norm, T, wiener_iters, stems=tuple(int(i) for i in inverts))
        stems = [(smag[s], None, sphase[s], False) for s in range(len(inverts))]
    elif phase_iters:                                            # Griffin-Lim on the one stem, MISI on the two
        mix = None
        if both_stems:                                           # the mixture at the scale of the tiles: one pass per call, not per iteration
            mix = y[:, :hop * (T - 1)].float().clone(memory_format=torch.contiguous_format)
            _scale_rows(mix, 1.0, maxima=norm)
        refined = refine_phase(tiles, mask, phase, T, phase_iters, stems=len(inverts), invert=inverts[0], mix=mix, n_fft=n_fft, hop=hop)
        stems = [(tiles, mask, refined[s], invert) for s, invert in enumerate(inverts)]
    else:
        stems = [(tiles, mask, phase, invert) for invert in inverts]

    # the inverse: (stems * C, n), the stems being further channels to everything below
    peak_here = None if sr_out is not None else peak            # with sr_out the peak is taken at the rate that is returned
    if both_stems and not (wiener_iters or phase_iters):         # one mask and one set of phasors: both stems from ONE launch
        out = istft_stems_from_tiles(tiles, mask, phase, T, n_fft=n_fft, hop=hop, peak=peak_here).flatten(0, 1)
    else:
        outs = [istft_from_tiles(t, m, p, T, invert=invert, n_fft=n_fft, hop=hop, peak=peak_here) for t, m, p, invert in stems]
        out = outs[0] if len(outs) == 1 else torch.cat(outs)
    track = None
    if f0_options is not None:                                   # the vocal's rows come first
        from .f0 import channel_mean, track_gpu
        track = track_gpu(channel_mean(out[:C]), SAMPLE_RATE, **f0_options)
    if sr_out is not None:
        from .resample import resample_poly_gpu
        out = resample_poly_gpu(out, int(sr_out), SAMPLE_RATE)
        if peak is not None:                                     # data.py:162-164 at the rate that is returned
            _scale_rows(out, peak, ws=torch.empty(4096, dtype=torch.uint8, device=out.device))
    if both_stems:
        out = out.view(2, C, out.shape[1])
        out = out[:, 0] if squeeze else out
    else:
        out = out[0] if squeeze else out
    return out if f0_options is None else (out, track)


def _report_peaks(report, measured):
    """report["sample_peaks"], report["true_peaks"]: per written file and channel in dBFS, from encode_planar_gpu's peaks_out (the
    rows before the gain, and the gains); one read-back, after the PCM."""
    if report is None or "true_peaks" not in measured:
        return
    gains = torch.stack(measured["gains"])                             # (files, channels)
    both = torch.stack([measured["sample_peaks"].view_as(gains), measured["true_peaks"].view_as(gains)]) * gains
    db = (20.0 * torch.log10(both.double())).cpu().tolist()            # a silent channel reads -inf
    report["sample_peaks"], report["true_peaks"] = db


def _report_limiter(report, limited, gain):
    """report["limiter"]: {"reduction_db": 20 log10 of the smallest value of the gain curve, "loudness": the integrated loudness of the
    written rows -- of the limited rows (encode_planar_gpu's limiter_out) plus the written gain}; one read-back, after the PCM."""
    if report is None or "curve" not in limited:
        return
    import math
    low, L = torch.stack([limited["curve"].min().double(), limited["limited_info"][0]]).cpu().tolist()
    written = L + 20.0 * math.log10(gain) if gain > 0 and math.isfinite(L) else -math.inf
    report["limiter"] = {"reduction_db": 20.0 * math.log10(low) if low > 0 else -math.inf, "loudness": written}


def _encoding(subtype, dither, dither_seed):
    """(sample format for resample.pcm_format, the subtype_bits / dither / dither_seed keywords of the planar encoders -- empty when the
    existing encoder writes `subtype`) for a subtype of pcm.SUBTYPES.  ValueError for dither beside PCM_32 / FLOAT."""
    from .pcm import encoder_bits
    bits = encoder_bits(subtype, dither)
    if bits is None:
        return subtype, {}
    return "PCM_16", dict(subtype_bits=bits, dither=dither, dither_seed=int(dither_seed))


def _write_pcm(path, rate, enc, channels, bits):
    """One encoded device tensor -> its wav file (pcm.write_wav24 for packed 24-bit frames); returns the (frames, channels) written."""
    out = enc.cpu().numpy()
    if bits == 24:
        from .pcm import write_wav24
        write_wav24(path, int(rate), out)
        return out.shape[0], channels
    from scipy.io import wavfile
    wavfile.write(path, int(rate), out[:, 0] if channels == 1 else out)
    return out.shape


def _write_fullband(mode, sep, aux, pcm, y, rate, channels, fr, hop, dst_path, dst_accomp_path, vocal_solo, subtype, keep_length, loudness,
                    ceiling, report, true_peak=False, dither="none", dither_seed=0, limiter_ms=None):
    """separate_to_wav(fullband=mode) from the separated stems on: frame gains, the mix at the file's rate, then frames, gain and
    encoding on the kernels the default path uses at 1/1."""
    from .fullband import frame_gains_gpu, fullband_mix_gpu
    from .resample import encode_planar_gpu, pcm_format, resample_poly_gpu
    fmt, how = _encoding(subtype, dither, dither_seed)
    both = dst_accomp_path is not None
    stems = (sep if both else sep[None]).contiguous()                 # (S, channels, hop * (T - 1)) at the scale of the tiles
    T = aux["frames"]
    gf = frame_gains_gpu(aux["tiles"], aux["mask"], T) if mode == "mask" else None
    n_source = pcm.shape[0]
    n_out = int(_lib.lib().svs_resample_out_len(stems.shape[2], fr.denominator, fr.numerator))
    frames = n_source if keep_length else n_out
    buf = fullband_mix_gpu(stems, y, pcm, aux["norm"], gf, T, hop, fr.denominator, fr.numerator, invert=not both and not vocal_solo,
                           width=max(n_out, frames))
    target = loudness
    if loudness == "source":
        from . import loudness as ld
        target = ld.loudness_gain_gpu(resample_poly_gpu(pcm, 1, 1, channels=channels, downmix=False), int(rate))[1]
    measured, limited = {}, {}
    encs, gains, info = encode_planar_gpu(buf, frames, *pcm_format(fmt), loudness=target, ceiling=ceiling, rate=int(rate), true_peak=true_peak,
                                          peaks_out=measured if true_peak and report is not None else None, limiter_ms=limiter_ms,
                                          limiter_out=limited if limiter_ms is not None and report is not None else None, **how)
    for enc, path in zip(encs, (dst_path, dst_accomp_path)):
        shape = _write_pcm(path, rate, enc, channels, how.get("subtype_bits"))
    if report is not None:
        report["gains"] = [float(g[0].item()) for g in gains]
        if info is not None:
            report["info"], report["gain"] = info.cpu().tolist(), report["gains"][0]
            _report_limiter(report, limited, report["gain"])
        _report_peaks(report, measured)
    return shape


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
                    dst_accomp_path: str | None = None, tile_hop: int = INPUT_LEN, phase_iters: int = 0, wiener_iters: int = 0,
                    loudness=None, ceiling: float = 0.9, report: dict | None = None, fullband: str | None = None, true_peak: bool = False,
                    dither: str = "none", dither_seed: int = 0, limiter_ms: float | None = None, f0=None, f0_csv_path: str | None = None):
    """wav file -> separated wav file at the same rate and channel count, everything between the two files on the device:
    the PCM is copied as the file stores it (pcm.read_pcm_device), resample.resample_poly_gpu (no downmix) brings every channel to
    SAMPLE_RATE, separate_waveform(peak=None) separates them, and resample.resample_encode_gpu resamples back to the file's rate,
    peak-normalises to 0.9 with one gain for all channels (data.py:162-164), converts to `subtype` ("PCM_16", "PCM_32",
    "FLOAT") and interleaves; only those samples return to the host.  keep_length: the frames are cut or zero-padded to the
    source's frame count (kept_length), so the file lines up sample for sample with the source's stems.  n_fft / hop: the
    window and hop of the two transforms (data.WINDOW_SIZES; the network is fully convolutional, so a checkpoint trained at
    another geometry runs on the n_fft / 2 rows of that window).  dst_accomp_path: also write the accompaniment there, from the
    same pass (separate_waveform(both_stems=True)): dst_path then holds the vocal whatever vocal_solo says, and each file is
    encoded with its own common gain at peak 0.9.  vocal_solo, precision, tile_hop, phase_iters and wiener_iters are
    separate_waveform's.

    loudness (None: the peak rule above, byte for byte): a number of LUFS, or "source" (only with dst_accomp_path): the written
    audio is brought to that integrated loudness (ITU-R BS.1770-4, loudness.py) instead of to peak 0.9 -- one stem to the target, or,
    with dst_accomp_path, vocal + accompaniment to the target with ONE gain for both files, so that their balance is kept and
    they still add up.  "source": the target is the source file's own loudness, measured on the device at the file's rate.  The
    gain never lifts a sample of any written file above `ceiling`.  The frames are cut or padded (keep_length) before the
    measurement, so what is measured is what is written.  report: a dict that receives "info" (L before the gain, kept blocks,
    unlimited gain, ceiling-limited) and "gain", read back after the PCM.  Returns the (frames, channels) written (per file).

    fullband (None: all of the above, byte for byte): "mask" or "accomp" (fullband.py): the band of the file above the network's
    4,096 Hz, which the written stems otherwise lack, is shared out between them -- by the network's mask in its highest band, or all of
    it to the accompaniment -- and every channel is multiplied by its `norm` again, so a stereo file keeps its balance.  One kernel
    (svs_fullband_mix) up-samples the stems, takes the file's PCM and writes float32 at the file's rate; the frames are then cut or
    padded, measured and encoded 1/1 (resample.encode_planar_gpu): the peak rule with one common gain per file, or `loudness` with one
    gain for both files.  With dst_accomp_path the two files, each divided by its gain (report["gains"]), add up to the source.  It
    composes with tile_hop, precision and phase_iters; wiener_iters beside it is a ValueError before any device work; a file at or
    below SAMPLE_RATE has no such band, and the flag then changes nothing and says so in a warning.

    true_peak (False: all of the above, byte for byte): `ceiling`, or without loudness the 0.9 of the peak rule, bounds the TRUE peak
    of every written file -- the peak of the 4x (2x from 96 kHz) over-sampled signal, loudness.py -- instead of its largest sample; the
    up-sampling on the way out produces inter-sample peaks that a sample-peak bound lets through.  One launch (svs_true_peaks)
    measures all written rows in place of the sample-peak launches; without loudness the frames are cut or padded before the
    measurement as well.  report then also receives "true_peaks" and "sample_peaks", per file and channel in dBFS of what was written.

    subtype "PCM_24" writes 24-bit files (pcm.write_wav24), "source" the subtype of the source file (pcm.subtype_of).  dither ("none":
    all of the above, byte for byte; "tpdf"; "hp", its high-passed form; PCM_16 and PCM_24 only, anything else is a ValueError before
    any device work) adds TPDF dither of 2 LSB peak to peak under the quantiser, from the counter generator with dither_seed for the
    vocal and dither_seed + 1 for the accompaniment (pcm.py).  With 24 bits or dither the stems go by the planar buffer, as with
    true_peak: the frames are cut or padded first, the peak rule is held against what is written, the gain is applied and
    svs_pcm_encode_dither quantises.  A 24-bit source crosses to the device as its 3 bytes per sample (pcm.read_pcm_device).

    limiter_ms (None: all of the above, byte for byte; only with loudness, anything else is a ValueError before any device work): a
    look-ahead limiter of that half-width in milliseconds (limiter.py) bends the gain around the peaks that would otherwise cap the
    loudness gain for the whole file: ONE gain curve for every channel of both files, against the true peaks with true_peak, then the
    rule above on the limited signal, so the bound on every written sample (or true peak) is unchanged.  L is measured before the
    limiter, so the written files read under the target by what the limiter removed; report then also receives "limiter":
    {"reduction_db": the deepest gain reduction, "loudness": the integrated loudness of what was written}.

    f0 / f0_csv_path (None: all of the above, byte for byte, and the written wav files are the same bytes with them): the pitch track of
    the vocal stem (separate_waveform(f0=); f0: True or a dict of f0.track_gpu's keywords, True when only the path is given), written to
    f0_csv_path as time,f0,voiced,aperiodicity,rms per frame (f0.write_csv) ahead of the way out; report receives "f0", the f0.Track of
    device tensors.  vocal_solo=False without dst_accomp_path writes no vocal: a ValueError before any device work."""
    if f0_csv_path is not None and (f0 is None or f0 is False):
        f0 = True
    tracking = f0 is not None and f0 is not False
    if tracking:
        from .f0 import check_options
        f0 = check_options(f0)
        if not vocal_solo and dst_accomp_path is None:
            raise ValueError("f0= tracks the vocal stem, and vocal_solo=False without dst_accomp_path writes none")
    if limiter_ms is not None and loudness is None:
        raise ValueError("limiter_ms= belongs to loudness=: the peak rule never exceeds its peak, so there is nothing to limit")
    check_refinement(phase_iters, wiener_iters)
    fullband = check_fullband(fullband, wiener_iters)
    if subtype == "source":
        from .pcm import subtype_of
        subtype = subtype_of(src_path)
    fmt, how = _encoding(subtype, dither, dither_seed)
    if isinstance(loudness, str) and (loudness != "source" or dst_accomp_path is None):
        raise ValueError(f"loudness={loudness!r}: a number of LUFS, or \"source\" together with dst_accomp_path")
    from fractions import Fraction

    from .pcm import read_pcm_device
    from .resample import resample_encode_gpu, resample_poly_gpu
    dev = model._flat.device
    if limiter_ms is not None:                                     # the half-width at the file's rate, from its header
        from .limiter import half_width
        from .pcm import wav_info
        head = wav_info(src_path)
        if head is not None:
            half_width(head["rate"], limiter_ms)
    rate, pcm, channels = read_pcm_device(src_path, dev)
    n_source = pcm.shape[0]
    if separated_frames(n_source, rate, hop) == 0:
        raise ValueError(f"{src_path}: {n_source} frames at {rate} Hz are shorter than one hop ({hop} samples at {SAMPLE_RATE} Hz)")
    if fullband is not None and int(rate) <= SAMPLE_RATE:
        import warnings
        warnings.warn(f"fullband={fullband}: a file at {rate} Hz has no band above the network's {SAMPLE_RATE // 2} Hz; the flag changes nothing")
        fullband = None
    fr = Fraction(SAMPLE_RATE, int(rate))
    y = resample_poly_gpu(pcm, fr.numerator, fr.denominator, channels=channels, downmix=False)
    y = y[None] if y.dim() == 1 else y                            # (channels, n) at the network rate
    aux = None if fullband is None else {}
    sep = separate_waveform(model, y, vocal_solo=vocal_solo, n_fft=n_fft, hop=hop, peak=None, precision=precision,
                            both_stems=dst_accomp_path is not None, tile_hop=tile_hop, phase_iters=phase_iters, wiener_iters=wiener_iters,
                            aux=aux, f0=f0 if tracking else None)
    if tracking:                                                   # the track is complete before the way out begins
        sep, track = sep
        if report is not None:
            report["f0"] = track
        if f0_csv_path is not None:
            from .f0 import write_csv
            write_csv(f0_csv_path, track)
    if fullband is not None:
        return _write_fullband(fullband, sep, aux, pcm, y, rate, channels, fr, hop, dst_path, dst_accomp_path, vocal_solo, subtype,
                               keep_length, loudness, ceiling, report, true_peak, dither, dither_seed, limiter_ms)
    jobs = ((sep, dst_path),) if dst_accomp_path is None else ((sep[0], dst_path), (sep[1], dst_accomp_path))
    if loudness is not None or true_peak or how:                   # (limiter_ms comes with loudness)
        from . import loudness as ld
        from .resample import encode_loudness_gpu, pcm_format
        target = loudness
        if loudness == "source":                                   # info[0] of a measurement of the file itself; it stays on the device
            target = ld.loudness_gain_gpu(resample_poly_gpu(pcm, 1, 1, channels=channels, downmix=False), int(rate))[1]
        frames = n_source if keep_length else None
        measured, limited = {}, {}
        encs, gain, info = encode_loudness_gpu([stem.contiguous() for stem, _ in jobs], fr.denominator, fr.numerator, *pcm_format(fmt),
                                               target, ceiling, int(rate), frames, true_peak,
                                               measured if true_peak and report is not None else None, limiter_ms=limiter_ms,
                                               limiter_out=limited if limiter_ms is not None and report is not None else None, **how)
        for enc, (_, path) in zip(encs, jobs):
            shape = _write_pcm(path, rate, enc, channels, how.get("subtype_bits"))
        if report is not None and info is not None:
            report["info"], report["gain"] = info.cpu().tolist(), float(gain[0].item())
            _report_limiter(report, limited, report["gain"])
        _report_peaks(report, measured)
        return shape
    for stem, path in jobs:
        enc = resample_encode_gpu(stem, fr.denominator, fr.numerator, fmt=subtype, peak=0.9, common_gain=True)
        if keep_length:
            keep, pad = kept_length(enc.shape[0], n_source)
            enc = torch.nn.functional.pad(enc[:keep], (0, 0, 0, pad))
        shape = _write_pcm(path, rate, enc, channels, None)
    return shape
