"""Full-band stems: the band of a file above the network's 4,096 Hz, shared out between the stems (csrc/fullband.hip).

The network runs at SAMPLE_RATE = 8,192 Hz.  separate_to_wav resamples the file down, separates, and up-samples the stems again, so
what it writes at 44.1 or 48 kHz is empty above 4,096 Hz.  The reference never leaves the network rate (data.py:151-166 writes at
--sr); Spleeter, whose networks stop at 11 or 16 kHz, fills the rest by `mask_extension = average | zeros`.  This is that step in
the time domain at the file's rate, with no second STFT grid.  With

    x_c(n)      channel c of the file's PCM as float (0 at and past the file's end)
    y_c         the signal at the network rate (resample.resample_poly_gpu of x_c)
    v_{s,c}     stem s (0 vocal, 1 accompaniment) as the inverse STFT returns it, hop * (T - 1) samples at the scale of the tiles
    norm_c      the channel's maximum magnitude (data.stft_to_tiles), which the tiles were divided by
    U(.)        the up-sampling FIR from 8,192 Hz to the file's rate: resample's filter, index rule and summation order; its
                inputs past hop * (T - 1) are zero, for v and for y alike

the output is, for n < out_len(hop * (T - 1), up, down),

    hi_c(n)      = x_c(n) - U(y_c)(n)                       what the network never saw: x = U(y) + hi by construction
    out_{s,c}(n) = norm_c * U(v_{s,c})(n) + g_{s,c}(n) * hi_c(n),           g_vocal = g,   g_accompaniment = 1 - g.

mode "mask": the high band follows the network's mask in the highest band it has.  For frame k of channel c, over the top
rows / TOP_DIV rows of the tile layout (3 to 4 kHz at the default geometry),

    gf[c, k] = sum_r mask * mag / sum_r mag                 (the plain mean of the mask where sum_r mag is exactly 0)

with `mask` the mask the stems were made from (the blended one under tile_hop), and g(n) interpolates gf linearly between frame
centres (frame k is centred at network sample k * hop): the frame coordinate is u = n * down / (up * hop) with up / down the reduced
file rate / 8,192 ratio, its integer part and remainder formed in integers (frame_coordinate), k and k + 1 clamped to T - 1.
mode "accomp": g = 0; the vocal stays band-limited and the accompaniment receives the whole high band (the karaoke case).

Either way out_vocal + out_accomp = x - U(y - norm * (v_vocal + v_accomp)): the file itself, minus what the two stems fail to add
up to below 4 kHz (the DC bin that the tile layout drops).  As a by-product the channels leave at the file's own balance: the
default path never multiplies norm back.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .resample import _FMT, design_lowpass, out_len, reduced, resample_reference, tap_table

MODES = ("mask", "accomp")
TOP_DIV = 4                                    # csrc/fullband.hip: FB_TOP_DIV


def check_fullband(fullband, wiener_iters: int = 0):
    """None or one of MODES, as given.  Raises ValueError for anything else and for the Wiener filter beside it: its stems live on a
    scale of their own (both channels on one) and its high band wants a spatial rule of its own."""
    if fullband is None:
        return None
    if fullband not in MODES:
        raise ValueError(f"fullband {fullband!r}: one of {', '.join(MODES)} (or None: band-limited stems, as ever)")
    if wiener_iters:
        raise ValueError(f"fullband {fullband} with wiener_iters {wiener_iters}: the Wiener filter's stems are on another scale and its high "
                         "band is out of scope; use one of the two")
    return fullband


def frame_coordinate(n, up: int, down: int, hop: int):
    """(k, rem, den) with n * down / (up * hop) = k + rem / den exactly, in integers (numpy int64 or Python ints): the frame output
    sample n of the file's rate falls in, and how far it is towards the next."""
    den = int(up) * int(hop)
    num = n * int(down)
    return num // den, num % den, den


def pcm_to_float(pcm) -> np.ndarray:
    """A wav file's samples as the kernels convert them: float32(int16) / 32768, float32(int32) / 2^31, float32 as it is."""
    pcm = np.asarray(pcm)
    if pcm.dtype == np.int16:
        return pcm.astype(np.float32) * np.float32(1.0 / 32768.0)
    if pcm.dtype == np.int32:
        return pcm.astype(np.float32) * np.float32(1.0 / 2147483648.0)
    if pcm.dtype != np.float32:
        raise TypeError(f"pcm dtype {pcm.dtype} (float32, int16 or int32)")
    return pcm


def frame_gains_reference(tiles, mask, frames: int, return_abs: bool = False):
    """gf (channels, frames) in float64.  tiles, mask: (channels, n_tiles, [1,] rows, seg).  return_abs: also (sum_r |mask * mag|,
    sum_r mag, sum_r |mask|) per frame, the scales of the rounding-error bound."""
    a = np.asarray(tiles, dtype=np.float64)
    m = np.asarray(mask, dtype=np.float64).reshape(a.shape)
    C, n_tiles, rows, seg = a.shape[0], a.shape[1], a.shape[-2], a.shape[-1]
    top = rows // TOP_DIV
    a = a.reshape(C, n_tiles, rows, seg)[:, :, rows - top:].transpose(0, 2, 1, 3).reshape(C, top, n_tiles * seg)[:, :, :frames]
    m = m.reshape(C, n_tiles, rows, seg)[:, :, rows - top:].transpose(0, 2, 1, 3).reshape(C, top, n_tiles * seg)[:, :, :frames]
    num, den = (m * a).sum(1), a.sum(1)
    gf = np.where(den == 0, m.mean(1), num / np.where(den == 0, 1.0, den))
    return (gf, np.abs(m * a).sum(1), den, np.abs(m).sum(1)) if return_abs else gf


def fullband_reference(stems, y, x, norm, gf, frames: int, hop: int, up: int, down: int, invert: bool = False, return_parts: bool = False):
    """The definition above in float64 numpy.  stems: (S, channels, n_in) with n_in = hop * (frames - 1); y: (channels, >= n_in); x:
    (channels, any length) float samples of the file; norm: (channels,); gf: (channels, frames) or None (mode "accomp"); up / down:
    file rate / network rate.  S = 2: vocal, accompaniment; S = 1: the vocal, or with invert the accompaniment.
    -> (S, channels, n_out); return_parts: also a dict of U(stems), U(y), their |.| sums (resample_reference(return_abs=True)), hi,
    g and the gain per stem."""
    up, down = reduced(up, down)
    stems = np.asarray(stems, dtype=np.float64)
    S, C, n_in = stems.shape
    y = np.asarray(y, dtype=np.float64)[:, :n_in]
    h = design_lowpass(up, down)
    us, us_abs = resample_reference(stems, up, down, h, return_abs=True)
    uy, uy_abs = resample_reference(y, up, down, h, return_abs=True)
    n_out = out_len(n_in, up, down)
    x = np.asarray(x, dtype=np.float64)
    xs = np.zeros((C, n_out))
    xs[:, :min(n_out, x.shape[1])] = x[:, :n_out]
    hi = xs - uy
    g = np.zeros((C, n_out))
    if gf is not None:
        gf = np.asarray(gf, dtype=np.float64)
        k, rem, den = frame_coordinate(np.arange(n_out, dtype=np.int64), up, down, hop)
        k0, k1 = np.minimum(k, frames - 1), np.minimum(k + 1, frames - 1)
        g = gf[:, k0] + (rem / den) * (gf[:, k1] - gf[:, k0])
    gs = np.stack([g, 1.0 - g])[1:] if (S == 1 and invert) else np.stack([g, 1.0 - g])[:S]
    out = np.asarray(norm, dtype=np.float64)[None, :, None] * us + gs * hi[None]
    if return_parts:
        return out, {"us": us, "us_abs": us_abs, "uy": uy, "uy_abs": uy_abs, "hi": hi, "g": g, "gs": gs, "x": xs}
    return out


def frame_gains_gpu(tiles, mask, frames: int, out=None):
    """svs_fullband_gains: magnitude tiles (channels, n_tiles, 1, rows, seg) and the mask of the same layout, float32 on the device ->
    gf (channels, frames) on the device."""
    import torch
    if not tiles.is_cuda or tiles.dtype != torch.float32 or mask.dtype != torch.float32 or mask.device != tiles.device:
        raise ValueError("frame_gains_gpu needs float32 device tensors (there is no CPU path)")
    if tiles.dim() != 5 or mask.numel() != tiles.numel():
        raise ValueError(f"tiles must be (channels, n_tiles, 1, rows, seg) and the mask of that size, got {tuple(tiles.shape)}, {tuple(mask.shape)}")
    tiles, mask = tiles.contiguous(), mask.contiguous()
    C, n_tiles, _, rows, seg = tiles.shape
    gf = torch.empty((C, int(frames)), dtype=torch.float32, device=tiles.device) if out is None else out
    with torch.cuda.device(tiles.device):
        _lib.check(_lib.lib().svs_fullband_gains(tiles.data_ptr(), mask.data_ptr(), n_tiles * rows * seg, C, n_tiles, rows, seg, int(frames),
                                                 gf.data_ptr(), _lib.stream_ptr(tiles.device)), "svs_fullband_gains")
    return gf


def fullband_mix_gpu(stems, y, pcm, norm, gf, frames: int, hop: int, up: int, down: int, *, invert: bool = False, width: int | None = None,
                     out=None):
    """svs_fullband_mix.  stems: (S, channels, n_in) float32 on the device, S = 1 or 2; y: (channels, >= n_in) at the network rate; pcm:
    the file's frames (n,) or (n, channels), float32 / int16 / int32 as the file stores them; norm: (channels,) device; gf:
    frame_gains_gpu's, or None (mode "accomp"); up / down: file rate / network rate.  -> (S, channels, width) float32, the first
    out_len(n_in, up, down) samples of every row written; width (default: that length) beyond it is zero, for a caller that pads.
    out: a contiguous float32 device tensor (S, channels, >= that length) to write into instead; what lies beyond is left as it is."""
    import torch
    if not stems.is_cuda or stems.dtype != torch.float32 or stems.dim() != 3:
        raise ValueError("fullband_mix_gpu needs the stems as a float32 device tensor (S, channels, n_in) (there is no CPU path)")
    fmt = _FMT.get(str(pcm.dtype))
    if fmt is None:
        raise TypeError(f"fullband_mix_gpu: pcm dtype {pcm.dtype} (float32, int16 or int32)")
    up, down = reduced(up, down)
    dev = stems.device
    S, C, n_in = stems.shape
    stems, y, pcm, norm = stems.contiguous(), y.contiguous().float(), pcm.contiguous(), norm.contiguous().float()
    if y.shape[0] != C or y.shape[1] < n_in or norm.numel() != C or pcm.dim() not in (1, 2) or (pcm.shape[1] if pcm.dim() == 2 else 1) != C:
        raise ValueError(f"fullband_mix_gpu: stems {tuple(stems.shape)}, y {tuple(y.shape)}, pcm {tuple(pcm.shape)}, norm {tuple(norm.shape)} "
                         "do not belong together")
    if gf is not None:
        gf = gf.contiguous()
        if gf.dtype != torch.float32 or tuple(gf.shape) != (C, int(frames)):
            raise ValueError(f"fullband_mix_gpu: gf must be float32 ({C}, {int(frames)}), got {tuple(gf.shape)}")
    L = _lib.lib()
    n_out = int(L.svs_resample_out_len(n_in, up, down))
    if out is not None:
        if not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 3 or tuple(out.shape[:2]) != (S, C):
            raise ValueError(f"fullband_mix_gpu: out must be a contiguous float32 device tensor ({S}, {C}, width), got {tuple(out.shape)}")
        width = out.shape[2]
    width = n_out if width is None else int(width)
    if n_out < 1 or width < n_out:
        raise ValueError(f"fullband_mix_gpu: n_in {n_in} gives {n_out} outputs, width {width}")
    table, ntaps = tap_table(up, down, dev)
    if out is None:
        out = (torch.zeros if width > n_out else torch.empty)((S, C, width), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.svs_fullband_mix(stems.data_ptr(), S, C * n_in, n_in, y.data_ptr(), y.shape[1], C, n_in, pcm.data_ptr(), fmt,
                                      pcm.shape[0], table.data_ptr(), ntaps, up, down, norm.data_ptr(), _lib.ptr(gf), int(frames), int(hop),
                                      1 if invert else 0, out.data_ptr(), width, C * width, _lib.stream_ptr(dev)), "svs_fullband_mix")
    return out
