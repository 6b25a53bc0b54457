"""wav <-> spectrogram conversion -- same command line, folder layout and file names as the reference's
data.py (/root/reference/data.py:20-28, 46-169), with the STFT / magnitude-phase split / inverse STFT /
normalisations running in the gfx950 kernels of csrc/stft.hip instead of librosa.

    python -m svs_unet_pytorch_amd.data --src MUSDB/train --tar spec/train --direction to_spec
    python -m svs_unet_pytorch_amd.data --src spec/pred --phase spec/test/mixture --tar wav --direction to_wave

to_spec (data.py:46-112): per song folder, mixture.wav fixes the normalisation (its maximum magnitude,
data.py:84-85); mixture.wav and vocals.wav are STFT'd (n_fft=--win_size, hop=--hop_size, periodic Hann,
centred), divided by that maximum (data.py:105) and saved as NNNN_<song>_spec.npy (float32 (win_size/2+1,T)) and
NNNN_<song>_phase.npy (complex64 unit phasors) under <tar>/mixture and <tar>/vocal (data.py:107-109).
to_wave (data.py:117-169): <name>_spec.npy times its phase -> inverse STFT -> peak-normalise to 0.9 ->
<name>.wav at --sr, float32 samples.  With --sr_out RATE and / or --subtype PCM_16 | PCM_32 the waveform is instead
up-sampled to RATE, peak-normalised at that rate and converted to the subtype's samples by one gfx950 kernel
(csrc/resample.hip: svs_resample_encode, save_wav_device below), and only the bytes the file stores cross to the
host.  --subtype PCM_16 is the reference's format: its sf.write(path, y, sr) (data.py:166) picks 16-bit PCM for a
.wav name; FLOAT, the default here, is what this project has always written.  --subtype PCM_24 writes 24-bit files and
--dither tpdf | hp adds TPDF dither under the 16- or 24-bit quantiser (pcm.py, csrc/pcm.hip: svs_pcm_encode_dither).

Out of the accelerated path: wav decoding (scipy.io.wavfile) and the wav
container write (soundfile there, scipy.io.wavfile here).  Downmix + resampling to --sr (the reference uses
librosa.load / soxr) is scipy.signal.resample_poly on the CPU by default; with --resample gpu (or
load_wav_mono(..., device=...)) the file's PCM is copied to the device as it is stored and one gfx950
kernel (csrc/resample.hip, svs_unet_pytorch_amd/resample.py) converts, downmixes and resamples it with
resample_poly's own filter, so the signal never visits the host between the file and the spectrogram.
Either way resampled audio matches the reference only up to the resampler's filter (soxr is not
reproduced); everything after the resampler follows the reference's arithmetic.
"""
from __future__ import annotations

import argparse
import os
import sys
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from .config import HOP_SIZE, SAMPLE_RATE, WINDOW_SIZE, num2str

TRACK_MAP = {"mixture.wav": "mixture", "vocals.wav": "vocal"}      # data.py:40-43
WINDOW_SIZES = (512, 1024, 2048)                                    # the n_fft the transforms of csrc/stft.hip are built for


def _check_window(n_fft: int, hop: int):
    if n_fft not in WINDOW_SIZES:
        raise ValueError(f"n_fft = {n_fft}: the STFT / iSTFT kernels are built for n_fft in {WINDOW_SIZES}")
    if not 0 < hop <= n_fft:
        raise ValueError(f"hop = {hop}: must be in 1..{n_fft} (a larger hop leaves samples that no frame covers)")


# ------------------------------------------------------------------------------------------------
# GPU signal path
# ------------------------------------------------------------------------------------------------
def phase_floats(phase: torch.Tensor) -> torch.Tensor:
    """complex64 phasors -> the contiguous float32 (..., 2) tensor of the same values that the kernels read (a view if it can be)."""
    return torch.view_as_real(phase.contiguous()).contiguous()


def _scale_rows(rows, numer, *, partials=None, ws=None, maxima=None):
    """Scale every row of the 2-D view `rows` (contiguous rows) by numer / its maximum, in place and row by row (data.py:84-85,
    105, 162-164) -> the (n_rows,) float32 maxima on the device.  Row r's maximum is svs_max over partials[r], the per-block
    partials a transform wrote; or svs_absmax over the row itself, with the workspace `ws`; or maxima[r], which the caller
    holds already.  numer None only reduces (`rows` may then be None beside partials)."""
    L = _lib.lib()
    n_rows = (partials if rows is None else rows).shape[0]
    if maxima is None:
        maxima = torch.empty(n_rows, dtype=torch.float32, device=(partials if rows is None else rows).device)
    for r in range(n_rows):
        if partials is not None:
            _lib.check(L.svs_max(partials[r].data_ptr(), partials.shape[1], maxima[r:].data_ptr(), _lib.stream_ptr()), "svs_max")
        elif ws is not None:
            _lib.check(L.svs_absmax(rows[r].data_ptr(), rows.shape[1], maxima[r:].data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "svs_absmax")
        if numer is not None:
            _lib.check(L.svs_scale_by_inv(rows[r].data_ptr(), rows.shape[1], maxima[r:].data_ptr(), float(numer), _lib.stream_ptr()), "svs_scale_by_inv")
    return maxima


def stft_magphase(y: torch.Tensor, n_fft: int = WINDOW_SIZE, hop: int = HOP_SIZE):
    """float32 (n,) on the GPU -> (mag float32 (n_fft/2+1,T), phase complex64 (n_fft/2+1,T)), both on the GPU."""
    _check_window(n_fft, hop)                  # (the buffers below are sized by n_fft before the library sees it)
    L = _lib.lib()
    y = y.contiguous().float()
    T = int(L.svs_stft_frames(y.numel(), hop))
    nbin = n_fft // 2 + 1
    mag = torch.empty((nbin, T), dtype=torch.float32, device=y.device)
    ph = torch.empty((nbin, T, 2), dtype=torch.float32, device=y.device)
    _lib.check(L.svs_stft_tiles_n(y.data_ptr(), y.numel(), 1, n_fft, hop, mag.data_ptr(), nbin * T, T, nbin, 0, T, ph.data_ptr(), 2, None,
                                  _lib.stream_ptr()), "svs_stft_tiles_n")
    return mag, torch.view_as_complex(ph)


def istft(mag: torch.Tensor, phase: torch.Tensor, n_fft: int = WINDOW_SIZE, hop: int = HOP_SIZE, peak: float | None = None):
    """mag float32 (n_fft/2+1,T) and phase (complex64 unit phasors, or float32 angles) -> float32 (hop*(T-1),).
    `peak`: scale so that max|y| == peak (data.py:162-164); None leaves the amplitude alone."""
    _check_window(n_fft, hop)
    L = _lib.lib()
    mag = mag.contiguous().float()
    nbin, T = mag.shape
    if nbin != n_fft // 2 + 1 or tuple(phase.shape) != (nbin, T):
        raise ValueError(f"istft: magnitude {tuple(mag.shape)} / phase {tuple(phase.shape)} are not ({n_fft // 2 + 1}, T) for n_fft = {n_fft}")
    is_angle = not torch.is_complex(phase)
    ph = phase.contiguous().float() if is_angle else phase_floats(phase.to(torch.complex64))
    y = torch.empty(hop * max(T - 1, 0), dtype=torch.float32, device=mag.device)
    ws = torch.empty(int(L.svs_istft_workspace_bytes(n_fft, hop, T)) + 4096, dtype=torch.uint8, device=mag.device)
    if is_angle:
        src, mode = ph, 3
    else:                                      # f-major phasors of a .npy file -> the frame-major form the kernels stream
        _lib.check(L.svs_transpose_c64(ph.data_ptr(), ws.data_ptr(), nbin, T, _lib.stream_ptr()), "svs_transpose_c64")
        src, mode = ws, 1
    _lib.check(L.svs_istft_tiles_n(mag.data_ptr(), nbin * T, T, nbin, 0, None, 0, src.data_ptr(), mode, 1, n_fft, hop, T, y.data_ptr(), None,
                                   _lib.stream_ptr()), "svs_istft_tiles_n")
    if peak is not None:
        _scale_rows(y[None], peak, ws=ws)
    return y


def specific_istft(magnitude: torch.Tensor, phase: torch.Tensor, n_fft: int = WINDOW_SIZE, hop: int = HOP_SIZE):
    """train.py:33-60: (B,1,n_fft/2,T) magnitude and angle (DC row dropped) -> (B,1,hop*(T-1)) waveforms, ONE launch for the
    whole batch (the DC row that train.py:41-42 pads back is the absent first row of the tile layout)."""
    _check_window(n_fft, hop)
    B, _, F_, T = magnitude.shape
    m = magnitude.contiguous().float()
    a = phase.contiguous().float()
    out = torch.empty((B, 1, hop * (T - 1)), dtype=torch.float32, device=m.device)
    _lib.check(_lib.lib().svs_istft_tiles_n(m.data_ptr(), F_ * T, T, F_, 1, None, 0, a.data_ptr(), 3, B, n_fft, hop, T, out.data_ptr(), None,
                                            _lib.stream_ptr()), "svs_istft_tiles_n")
    return out


def stft_to_tiles(y: torch.Tensor, n_fft: int = WINDOW_SIZE, hop: int = HOP_SIZE, seg: int = 128):
    """float32 (channels, n) on the GPU -> (tiles (channels, n_tiles, 1, n_fft/2, seg) magnitude with the DC row dropped and the
    last tile zero-padded (inference.py:68,84-92), frame-major unit phasors (channels, T, n_fft/2+1) complex64, the maximum
    magnitude per channel (channels,) incl. the DC row (data.py:84), T).  One launch; nothing is repacked afterwards."""
    _check_window(n_fft, hop)
    L = _lib.lib()
    y = y.contiguous().float()
    C, n = y.shape
    T = int(L.svs_stft_frames(n, hop))
    n_tiles = T // seg + (1 if T % seg else 0)                      # the empty last segment is skipped (inference.py:88)
    rows = n_fft // 2
    tiles = torch.empty((C, n_tiles, 1, rows, seg), dtype=torch.float32, device=y.device)
    phase = torch.empty((C, T, rows + 1, 2), dtype=torch.float32, device=y.device)
    groups = int(L.svs_stft_groups_n(n_fft, n_tiles * seg))
    part = torch.empty((C, groups), dtype=torch.float32, device=y.device)
    _lib.check(L.svs_stft_tiles_n(y.data_ptr(), n, C, n_fft, hop, tiles.data_ptr(), n_tiles * rows * seg, seg, rows, 1, n_tiles * seg,
                                  phase.data_ptr(), 1, part.data_ptr(), _lib.stream_ptr()), "svs_stft_tiles_n")
    return tiles, torch.view_as_complex(phase), _scale_rows(None, None, partials=part), T


def istft_from_tiles(tiles: torch.Tensor, mask, phase_fm: torch.Tensor, frames: int, invert: bool = False,
                     n_fft: int = WINDOW_SIZE, hop: int = HOP_SIZE, peak: float | None = None):
    """(channels, n_tiles, 1, n_fft/2, seg) magnitude tiles [times mask or 1 - mask, fused: inference.py:100-107] and frame-major
    phasors (channels, T, n_fft/2+1) -> (channels, hop*(T-1)) samples, optionally peak-normalised per channel (data.py:162-164)."""
    _check_window(n_fft, hop)
    L = _lib.lib()
    C, n_tiles, _, rows, seg = tiles.shape
    ph = phase_floats(phase_fm)
    y = torch.empty((C, hop * max(frames - 1, 0)), dtype=torch.float32, device=tiles.device)
    groups = int(L.svs_istft_groups_n(n_fft, hop, max(frames, 1), C))
    part = torch.empty((C, groups), dtype=torch.float32, device=tiles.device) if peak is not None else None
    _lib.check(L.svs_istft_tiles_n(tiles.data_ptr(), n_tiles * rows * seg, seg, rows, 1, None if mask is None else mask.data_ptr(),
                                   1 if invert else 0, ph.data_ptr(), 1, C, n_fft, hop, frames, y.data_ptr(),
                                   None if part is None else part.data_ptr(), _lib.stream_ptr()), "svs_istft_tiles_n")
    if peak is not None:
        _scale_rows(y, peak, partials=part)
    return y


def istft_stems_from_tiles(tiles: torch.Tensor, mask: torch.Tensor, phase_fm: torch.Tensor, frames: int, n_fft: int = WINDOW_SIZE,
                           hop: int = HOP_SIZE, peak: float | None = None):
    """Both stems of a mask from ONE launch (svs_istft_stems_n): tiles, mask and phasors as istft_from_tiles ->
    (2, channels, hop*(T-1)) samples, [0] from tiles * mask (the vocal, inference.py:100-103) and [1] from tiles * (1 - mask) (the
    accompaniment, inference.py:104-107).  peak: every stem and channel is normalised on its own (data.py:162-164)."""
    _check_window(n_fft, hop)
    if mask is None:
        raise ValueError("istft_stems_from_tiles: the mask is required (both stems come from it)")
    L = _lib.lib()
    C, n_tiles, _, rows, seg = tiles.shape
    ph = phase_floats(phase_fm)
    n_out = hop * max(frames - 1, 0)
    y = torch.empty((2, C, n_out), dtype=torch.float32, device=tiles.device)
    groups = int(L.svs_istft_stems_groups_n(n_fft, hop, max(frames, 1), C))
    part = torch.empty((2, C, groups), dtype=torch.float32, device=tiles.device) if peak is not None else None
    _lib.check(L.svs_istft_stems_n(tiles.data_ptr(), n_tiles * rows * seg, seg, rows, 1, mask.data_ptr(), ph.data_ptr(), 1, C, n_fft, hop,
                                   frames, y.data_ptr(), C * n_out, None if part is None else part.data_ptr(), _lib.stream_ptr()),
               "svs_istft_stems_n")
    if peak is not None:
        _scale_rows(y.view(2 * C, n_out), peak, partials=part.view(2 * C, groups))
    return y


# ------------------------------------------------------------------------------------------------
# host-side file glue (not on the accelerated path)
# ------------------------------------------------------------------------------------------------
def load_wav_mono(path: str, sr: int, device=None):
    """Mono float32 samples of a wav file at rate `sr`.  device=None: numpy array, decoded, downmixed and resampled on the
    host.  With a device: the PCM goes to the device as the file stores it (one copy) and svs_resample_poly converts,
    downmixes and resamples it there; returns a device tensor."""
    from scipy.io import wavfile
    if device is not None:
        return _load_wav_mono_device(path, sr, device)
    from scipy.signal import resample_poly
    rate, data = wavfile.read(path)
    if data.dtype.kind == "i":
        data = data.astype(np.float32) / float(np.iinfo(data.dtype).max + 1)
    elif data.dtype.kind == "u":
        data = (data.astype(np.float32) - 128.0) / 128.0
    else:
        data = data.astype(np.float32)
    if data.ndim == 2:
        data = data.mean(axis=1)
    if rate != sr:
        fr = Fraction(sr, rate)
        data = resample_poly(data, fr.numerator, fr.denominator).astype(np.float32)
    return np.ascontiguousarray(data, dtype=np.float32)


def read_pcm(path: str):
    """wav file -> (rate, samples, channels) for the device kernels, which convert 16- and 32-bit PCM themselves: those stay as the
    file stores them, everything else becomes float32 on the host.  samples: (frames,) or (frames, channels)."""
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    if data.dtype.kind == "u":                                 # 8-bit files: offset binary, converted on the host
        data = (data.astype(np.float32) - 128.0) / 128.0
    elif data.dtype not in (np.int16, np.int32):               # float files (and int64, which wavfile never returns)
        data = data.astype(np.float32)
    return rate, np.ascontiguousarray(data), data.shape[1] if data.ndim == 2 else 1


def _load_wav_mono_device(path: str, sr: int, device) -> torch.Tensor:
    from .pcm import read_pcm_device
    from .resample import resample_poly_gpu
    rate, pcm, channels = read_pcm_device(path, device)        # a 24-bit file crosses as its 3 bytes per sample (pcm.py)
    fr = Fraction(sr, rate)                                    # 1/1 (rate == sr): the call only converts and downmixes
    return resample_poly_gpu(pcm, fr.numerator, fr.denominator, channels=channels, downmix=True)


def write_wav(path: str, y: np.ndarray, sr: int):
    from scipy.io import wavfile
    wavfile.write(path, sr, np.asarray(y, dtype=np.float32))


def save_wav_device(path: str, y_dev: torch.Tensor, sr: int, sr_out: int | None = None, subtype: str = "PCM_16", peak: float | None = 0.9,
                    loudness: float | None = None, ceiling: float = 0.9, true_peak: bool = False, dither: str = "none", dither_seed: int = 0,
                    limiter_ms: float | None = None):
    """float32 device samples (n,) or (channels, n) at rate `sr` -> a wav file at `sr_out` (default: sr) with the samples of
    `subtype` ("PCM_16", the reference's sf.write format for a .wav name, "PCM_24", "PCM_32" or "FLOAT"), peak-normalised to `peak` at
    the rate that is written (data.py:162-166; None: not normalised; one gain for all channels).  Resampling, gain, sample
    conversion and interleaving are resample.resample_encode_gpu; one device -> host copy of the encoded samples follows.
    loudness (LUFS) replaces the peak rule: the file is brought to that integrated loudness (loudness.py), no sample above
    `ceiling`; the four numbers of the measurement are returned (None without loudness).  true_peak: `ceiling` (or `peak`, which
    must then be given) bounds the file's true peak, the over-sampled signal's (loudness.py), instead of its largest sample.
    dither ("none", "tpdf", "hp") with dither_seed: TPDF dither under the 16- or 24-bit quantiser (pcm.py); PCM_24 and dither go by
    svs_pcm_encode_dither (peak must then be given), and a 24-bit file is written by pcm.write_wav24.
    limiter_ms (only with loudness, a ValueError before any device work otherwise): resample_encode_gpu's look-ahead limiter of that
    half-width in milliseconds (limiter.py), so that a few peaks do not cap the loudness gain of the whole file."""
    from scipy.io import wavfile
    from . import pcm as pcm24
    from .resample import resample_encode_gpu
    sr_out = int(sr if sr_out is None else sr_out)
    if limiter_ms is not None:
        from .resample import _check_limiter
        _check_limiter(limiter_ms, loudness, sr_out)
    fr = Fraction(sr_out, int(sr))
    bits = pcm24.encoder_bits(subtype, dither)                 # ValueError for dither beside PCM_32 / FLOAT, before any device work
    how = {} if bits is None else dict(subtype_bits=bits, dither=dither, dither_seed=dither_seed)
    fmt = "PCM_16" if bits is not None else subtype

    def write(pcm):
        if bits == 24:
            pcm24.write_wav24(path, sr_out, pcm.cpu().numpy())
        else:
            wavfile.write(path, sr_out, pcm.cpu().numpy())

    if loudness is not None:
        pcm, info = resample_encode_gpu(y_dev.contiguous().float(), fr.numerator, fr.denominator, fmt=fmt, loudness=loudness,
                                        ceiling=ceiling, rate=sr_out, true_peak=true_peak, limiter_ms=limiter_ms, **how)
        write(pcm)
        return info.cpu().tolist()
    if true_peak:
        pcm = resample_encode_gpu(y_dev.contiguous().float(), fr.numerator, fr.denominator, fmt=fmt, peak=peak, common_gain=True,
                                  rate=sr_out, true_peak=True, **how)
        write(pcm)
        return None
    pcm = resample_encode_gpu(y_dev.contiguous().float(), fr.numerator, fr.denominator, fmt=fmt, peak=peak, common_gain=True, **how)
    write(pcm)


def to_spec(args, device):
    os.makedirs(args.tar, exist_ok=True)
    for folder in TRACK_MAP.values():
        os.makedirs(os.path.join(args.tar, folder), exist_ok=True)
    print(f"Scanning source folder: {args.src}")
    songs = sorted(d for d in os.listdir(args.src) if os.path.isdir(os.path.join(args.src, d)))
    print(f"Found {len(songs)} song folders.")
    if not songs:
        print("Error: no song folders found, check --src.")
        sys.exit(1)                                                     # data.py:61-63
    ws = torch.empty(4096, dtype=torch.uint8, device=device)
    for audio_idx, song in enumerate(songs):
        song_path = os.path.join(args.src, song)
        mix_path = os.path.join(song_path, "mixture.wav")
        if not os.path.exists(mix_path):
            continue
        try:
            on_gpu = getattr(args, "resample", "cpu") == "gpu"
            y_mix = load_wav_mono(mix_path, args.sr, device if on_gpu else None)
            spec_mix, _ = stft_magphase(y_mix if on_gpu else torch.from_numpy(y_mix).to(device), args.win_size, args.hop_size)
            norm = _scale_rows(spec_mix.view(1, -1), None, ws=ws)          # max magnitude, 0 -> 1 (data.py:84-85)
            for wav_file, folder in TRACK_MAP.items():
                track = os.path.join(song_path, wav_file)
                if not os.path.exists(track):
                    continue
                if on_gpu:
                    y = load_wav_mono(track, args.sr, device)
                    y = y[: len(y_mix)] if len(y) > len(y_mix) else torch.nn.functional.pad(y, (0, len(y_mix) - len(y)))
                else:
                    y = load_wav_mono(track, args.sr)
                    y = y[: len(y_mix)] if len(y) > len(y_mix) else np.pad(y, (0, len(y_mix) - len(y)))   # data.py:97-98
                    y = torch.from_numpy(y).to(device)
                spec, phase = stft_magphase(y, args.win_size, args.hop_size)
                _scale_rows(spec.view(1, -1), 1.0, maxima=norm)
                base = f"{num2str(audio_idx)}_{song}"
                np.save(os.path.join(args.tar, folder, f"{base}_spec.npy"), spec.cpu().numpy())
                np.save(os.path.join(args.tar, folder, f"{base}_phase.npy"), phase.cpu().numpy())
        except Exception as e:                                          # data.py:111-112
            print(f"Error processing {song}: {e}")


def to_wave(args, device):
    if args.phase == "-1":
        raise Exception("--phase is required for to_wave")            # data.py:118
    os.makedirs(args.tar, exist_ok=True)
    files = sorted(f for f in os.listdir(args.src) if f.endswith("_spec.npy"))
    print(f"Restoring {len(files)} files...")
    for spec_name in files:
        try:
            mag = np.load(os.path.join(args.src, spec_name))
            phase_name = spec_name.replace("_spec.npy", "_phase.npy")
            phase = None
            for p in (os.path.join(args.phase, phase_name), os.path.join(args.phase, "mixture", phase_name)):   # data.py:135-143
                if os.path.exists(p):
                    phase = np.load(p)
                    break
            if phase is None:
                phase = np.exp(2j * np.pi * np.random.rand(*mag.shape))                                        # data.py:148
            m = min(mag.shape[1], phase.shape[1])                                                              # data.py:151-153
            sr_out = getattr(args, "sr_out", None) or args.sr
            subtype = getattr(args, "subtype", "FLOAT")
            loudness = getattr(args, "loudness", None)
            true_peak = bool(getattr(args, "true_peak", False))
            dither = getattr(args, "dither", "none")
            encode = sr_out != args.sr or subtype != "FLOAT" or loudness is not None or true_peak   # else: float32 at --sr, written as it always was
            y = istft(torch.from_numpy(np.ascontiguousarray(mag[:, :m])).to(device),
                      torch.from_numpy(np.ascontiguousarray(phase[:, :m]).astype(np.complex64)).to(device),
                      args.win_size, args.hop_size, peak=None if encode else 0.9)
            wav_path = os.path.join(args.tar, spec_name.replace("_spec.npy", ".wav"))
            if encode:
                save_wav_device(wav_path, y, args.sr, sr_out, subtype, peak=0.9, loudness=loudness, ceiling=getattr(args, "peak_ceiling", 0.9),
                                true_peak=true_peak, dither=dither, dither_seed=getattr(args, "dither_seed", 0),
                                limiter_ms=getattr(args, "limiter", None))
            else:
                write_wav(wav_path, y.cpu().numpy(), args.sr)
        except Exception as e:                                          # data.py:168-169
            print(f"Restore failed {spec_name}: {e}")


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--src", type=str, required=True, help="source folder (song folders, or *_spec.npy for to_wave)")
    parser.add_argument("--tar", type=str, required=True, help="target folder")
    parser.add_argument("--phase", type=str, default="-1", help="phase folder (to_wave only)")
    parser.add_argument("--win_size", type=int, default=WINDOW_SIZE)
    parser.add_argument("--hop_size", type=int, default=HOP_SIZE)
    parser.add_argument("--sr", type=int, default=SAMPLE_RATE)
    parser.add_argument("--direction", default="to_spec", choices=["to_spec", "to_wave"])
    parser.add_argument("--resample", default="cpu", choices=["cpu", "gpu"],
                        help="to_spec: downmix + resample on the host (scipy, default) or on the device from the file's PCM")
    parser.add_argument("--sr_out", type=int, default=None, help="to_wave: rate of the written files (default: --sr)")
    parser.add_argument("--subtype", default="FLOAT", choices=["FLOAT", "PCM_16", "PCM_24", "PCM_32"],
                        help="to_wave: sample format of the written files (PCM_16 is the reference's)")
    parser.add_argument("--dither", default="none", choices=["none", "tpdf", "hp"],
                        help="to_wave with --subtype PCM_16 | PCM_24: TPDF dither under the quantiser, white (tpdf) or high-passed (hp)")
    parser.add_argument("--dither_seed", type=int, default=0, help="seed of the dither's counter generator (files are reproducible)")
    parser.add_argument("--loudness", type=float, default=None,
                        help="to_wave: integrated loudness of the written files in LUFS (ITU-R BS.1770-4) instead of peak 0.9")
    parser.add_argument("--peak_ceiling", type=float, default=0.9, help="to_wave with --loudness: no written sample exceeds this")
    parser.add_argument("--true_peak", action="store_true",
                        help="to_wave: bound the written files' true peak (the over-sampled signal's) instead of their largest sample")
    parser.add_argument("--limiter", type=float, nargs="?", const=2.0, default=None, metavar="MS",
                        help="to_wave with --loudness: look-ahead limiter of this half-width in milliseconds (2.0 when given without a value), "
                             "so that a few peaks do not hold the whole file under the target (limiter.py)")
    args = parser.parse_args(argv)
    if args.sr_out is not None and args.sr_out < 1:
        parser.error(f"--sr_out {args.sr_out}: must be positive")
    if args.limiter is not None:
        if args.loudness is None:
            parser.error("--limiter belongs to --loudness: the peak rule never exceeds its peak, so there is nothing to limit")
        from .limiter import half_width
        try:
            half_width(args.sr_out or args.sr, args.limiter)
        except ValueError as e:
            parser.error(f"--limiter {args.limiter:g}: {e}")
    if args.dither != "none" and args.subtype not in ("PCM_16", "PCM_24"):
        parser.error(f"--dither {args.dither} belongs to --subtype PCM_16 or PCM_24: {args.subtype} samples have nothing below the 24th bit to linearise")
    if args.win_size not in WINDOW_SIZES:        # data.py:24 lets it vary; the gfx950 transforms are built for these three
        parser.error(f"--win_size {args.win_size}: the STFT / iSTFT kernels are built for n_fft = {', '.join(map(str, WINDOW_SIZES))} "
                     f"(default {WINDOW_SIZE}, config.WINDOW_SIZE); --hop_size may be anything in 1..win_size")
    if not 0 < args.hop_size <= args.win_size:
        parser.error(f"--hop_size {args.hop_size}: must be in 1..{args.win_size} (a larger hop leaves samples that no frame covers)")
    if not torch.cuda.is_available():
        print("data.py needs a ROCm device (the STFT/iSTFT are gfx950 kernels, no CPU path).")
        sys.exit(1)
    device = torch.device("cuda")
    if args.direction == "to_spec":
        to_spec(args, device)
    else:
        to_wave(args, device)


if __name__ == "__main__":
    main()
