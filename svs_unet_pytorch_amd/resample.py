"""Resampling to the network rate on the GPU: the arithmetic half of the reference's librosa.load(path, sr=8192, mono=True)
(data.py:78,94) -- downmix and polyphase FIR resampling -- as one gfx950 kernel (csrc/resample.hip) that reads the wav
file's PCM as it is stored.

The filter and the index rule are those of scipy.signal.resample_poly with its defaults (window=("kaiser", 5.0),
padtype="constant"), which is what data.load_wav_mono runs on the host.  The reference's librosa resamples with soxr; neither
is importable here, so parity with the reference's resampler stays unpinned (as data.py states): this module matches the
project's scipy path.  With up, down divided by their gcd:

    half = 10 * max(up, down),  N = 2 * half + 1,  h = up * lowpass(N, cutoff 1 / max(up, down), Kaiser beta 5)
    n_out = ceil(n_in * up / down)
    y[i] = sum_j x[j] * h[i * down - j * up + half]        over 0 <= j < n_in with the tap index inside [0, 2 * half]

Per output that is T = ceil(N / up) taps: with pos = i * down + half, n0 = pos // up and p = pos % up,
y[i] = sum_k x[n0 - k] * h[p + k * up].  p depends on i % up only, which is what the packed table is indexed by.
"""
from __future__ import annotations

from math import gcd

import numpy as np

from . import _lib

PCM_F32, PCM_I16, PCM_I32 = 0, 1, 2            # include/svs_hip.h: SVS_PCM_*


def reduced(up: int, down: int):
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError(f"up, down must be positive, got {up}, {down}")
    g = gcd(up, down)
    return up // g, down // g


def design_lowpass(up: int, down: int) -> np.ndarray:
    """float64 taps of resample_poly's default filter: firwin(N, 1 / max(up, down), window=("kaiser", 5.0)) * up, numpy only."""
    up, down = reduced(up, down)
    m = max(up, down)
    half = 10 * m
    n = 2 * half + 1
    fc = 1.0 / m
    k = np.arange(n, dtype=np.float64) - half
    h0 = fc * np.sinc(fc * k) * np.kaiser(n, 5.0)
    return up * h0 / h0.sum()


def out_len(n_in: int, up: int, down: int) -> int:
    up, down = reduced(up, down)
    return -((-int(n_in) * up) // down)


def taps_per_output(ntaps: int, up: int) -> int:
    return -(-int(ntaps) // int(up))


def resample_reference(x, up: int, down: int, h=None, return_abs: bool = False, chunk: int = 1 << 15):
    """The closed-form sum above in float64 numpy, along the last axis of x.  h: taps (default design_lowpass).
    return_abs: also S[i] = sum_j |x[j]| * |h[...]|, the scale of the rounding-error bound of a dot product."""
    up, down = reduced(up, down)
    h = design_lowpass(up, down) if h is None else np.asarray(h, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    n_in = x.shape[-1]
    ntaps = len(h)
    half = (ntaps - 1) // 2
    T = taps_per_output(ntaps, up)
    n_out = out_len(n_in, up, down)
    y = np.zeros(x.shape[:-1] + (n_out,), dtype=np.float64)
    s = np.zeros_like(y) if return_abs else None
    hp = np.concatenate([h, np.zeros(T * up - ntaps)])
    k = np.arange(T, dtype=np.int64)
    for a in range(0, n_out, chunk):
        i = np.arange(a, min(a + chunk, n_out), dtype=np.int64)
        pos = i * down + half
        j = (pos // up)[:, None] - k                                   # (outputs, T) input indices
        taps = hp[(pos % up)[:, None] + k * up]
        ok = (j >= 0) & (j < n_in)
        xv = np.where(ok, x[..., np.clip(j, 0, n_in - 1)], 0.0)
        y[..., i] = (xv * taps).sum(-1)
        if return_abs:
            s[..., i] = (np.abs(xv) * np.abs(taps)).sum(-1)
    return (y, s) if return_abs else y


def pack_taps(h, up: int, down: int) -> np.ndarray:
    """Host mirror of svs_resample_pack_taps: table[k, q] = h[(q * down + half) % up + k * up] (0 past the last tap), so that
    row q = i % up holds the taps of output i in the order they are summed."""
    h = np.asarray(h)
    ntaps = len(h)
    if ntaps % 2 == 0:
        raise ValueError("the filter needs an odd number of taps")
    half = (ntaps - 1) // 2
    T = taps_per_output(ntaps, up)
    hp = np.concatenate([h, np.zeros(T * up - ntaps, dtype=h.dtype)])
    q = np.arange(up, dtype=np.int64)
    return hp[((q * down + half) % up)[None, :] + (np.arange(T, dtype=np.int64) * up)[:, None]]


def unpack_row(table: np.ndarray, i: int) -> np.ndarray:
    """The T taps output i is summed with: h[(i * down + half) % up + k * up], k = 0 .. T-1."""
    return table[:, int(i) % table.shape[1]]


_TABLES: dict = {}


def tap_table(up: int, down: int, device):
    """(packed device table, ntaps) of the default filter for reduced (up, down), built once per device."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (up, down, str(device))
    if key not in _TABLES:
        L = _lib.lib()
        # 1/1 (a file already at the target rate): the one-tap identity, so the call only converts and downmixes
        h = np.ones(1, dtype=np.float32) if up == down == 1 else design_lowpass(up, down).astype(np.float32)
        nbytes = int(L.svs_resample_table_bytes(up, down, len(h)))
        if nbytes == 0:
            raise _lib.SvsError(f"svs_resample_table_bytes({up}, {down}, {len(h)}): invalid filter")
        with torch.cuda.device(device):
            taps = torch.from_numpy(h).to(device)
            table = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
            _lib.check(L.svs_resample_pack_taps(taps.data_ptr(), len(h), up, down, table.data_ptr(), _lib.stream_ptr(device)),
                       "svs_resample_pack_taps")
            torch.cuda.current_stream(device).synchronize()             # `taps` may be freed once the table is built
        _TABLES[key] = (table, len(h))
    return _TABLES[key]


_FMT = {"torch.float32": PCM_F32, "torch.int16": PCM_I16, "torch.int32": PCM_I32}


def resample_poly_gpu(x, up: int, down: int, *, channels: int = 1, downmix: bool = False):
    """Device tensor of PCM (float32, or int16 / int32 scaled by 1/32768 / 2^-31) -> float32 device tensor at rate * up / down.

    channels == 1: x is (n,) or (batch, n), planar; the result has the same leading shape.
    channels > 1: x is (n, channels) or (batch, n, channels), interleaved as a wav file stores it.  downmix=True averages the
    channels of every frame on load (as data.load_wav_mono does) -> (n_out,) / (batch, n_out); downmix=False resamples every
    channel on its own -> (channels, n_out) / (batch, channels, n_out)."""
    import torch
    if not x.is_cuda:
        raise ValueError("resample_poly_gpu needs a device tensor (there is no CPU path)")
    fmt = _FMT.get(str(x.dtype))
    if fmt is None:
        raise TypeError(f"resample_poly_gpu: dtype {x.dtype} (float32, int16 or int32)")
    up, down = reduced(up, down)
    x = x.contiguous()
    if channels == 1:
        if x.dim() not in (1, 2):
            raise ValueError(f"planar input must be (n,) or (batch, n), got {tuple(x.shape)}")
        batched = x.dim() == 2
        batch, n_in = (x.shape[0], x.shape[1]) if batched else (1, x.shape[0])
    else:
        if x.dim() not in (2, 3) or x.shape[-1] != channels:
            raise ValueError(f"interleaved input must be (n, {channels}) or (batch, n, {channels}), got {tuple(x.shape)}")
        batched = x.dim() == 3
        batch, n_in = (x.shape[0], x.shape[1]) if batched else (1, x.shape[0])
    if n_in < 1 or batch < 1:
        raise ValueError("resample_poly_gpu: empty input")
    L = _lib.lib()
    n_out = int(L.svs_resample_out_len(n_in, up, down))
    table, ntaps = tap_table(up, down, x.device)
    rps = 1 if (downmix or channels == 1) else channels
    y = torch.empty((batch * rps, n_out), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.svs_resample_poly(x.data_ptr(), fmt, channels, 1 if downmix else 0, n_in, n_in * channels, batch,
                                       table.data_ptr(), ntaps, up, down, y.data_ptr(), n_out, _lib.stream_ptr(x.device)),
                   "svs_resample_poly")
    if rps > 1:
        return y.view(batch, rps, n_out) if batched else y
    return y if batched else y[0]


# ------------------------------------------------------------------------------------------------
# the way out: planar fp32 at the network rate -> the interleaved PCM a wav file stores, at the file's rate
# ------------------------------------------------------------------------------------------------
_PCM = {"float32": (PCM_F32, np.float32), "int16": (PCM_I16, np.int16), "int32": (PCM_I32, np.int32)}
_SUBTYPE = {"FLOAT": "float32", "PCM_16": "int16", "PCM_32": "int32"}       # soundfile's names for the wav subtypes


def pcm_format(fmt):
    """(SVS_PCM_* code, numpy dtype) of "float32" / "int16" / "int32", of a wav subtype name ("FLOAT", "PCM_16", "PCM_32")
    or of a code."""
    if isinstance(fmt, str):
        fmt = _SUBTYPE.get(fmt, fmt)
        if fmt in _PCM:
            return _PCM[fmt]
    else:
        for code, dtype in _PCM.values():
            if code == fmt:
                return code, dtype
    raise ValueError(f"sample format {fmt!r}: one of {sorted(_PCM)} or {sorted(_SUBTYPE)}")


def encode_pcm_reference(y, gain, fmt):
    """numpy restatement of what svs_resample_encode does after the FIR (include/svs_hip.h).  y: (n, channels) or (n,)
    float32; gain: None, a scalar or `channels` float32 values.  v = y * gain is one float32 multiply, then
        float32: v        int16: clip(rint(v * float32(32767)), -32768, 32767), the multiply in float32
        int32: clip(rint(float64(v) * 2147483647), -2^31, 2^31 - 1)
    with rint rounding ties to even, NaN -> 0 and +-inf clipped in the integer formats."""
    code, dtype = pcm_format(fmt)
    v = np.asarray(y, dtype=np.float32)
    if gain is not None:
        v = v * np.asarray(gain, dtype=np.float32)
    if code == PCM_F32:
        return np.ascontiguousarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if code == PCM_I16:
            s = np.rint(v * np.float32(32767.0))
            lo, hi = -32768.0, 32767.0
        else:
            s = np.rint(v.astype(np.float64) * 2147483647.0)
            lo, hi = -2147483648.0, 2147483647.0
        s = np.where(np.isnan(s), 0.0, np.clip(s, lo, hi))
    return np.ascontiguousarray(s.astype(dtype))


def resample_peaks_gpu(y, up: int, down: int):
    """max |resample_poly_gpu(y, up, down)| per row of a planar float32 device tensor (channels, n), as a device tensor
    (channels,), without writing the resampled signal (svs_resample_peaks)."""
    import torch
    up, down = reduced(up, down)
    channels, n_in = y.shape
    L = _lib.lib()
    table, ntaps = tap_table(up, down, y.device)
    nbytes = int(L.svs_resample_peaks_workspace_bytes(n_in, channels, up, down, ntaps))
    if nbytes == 0:
        raise _lib.SvsError(f"svs_resample_peaks_workspace_bytes({n_in}, {channels}, {up}, {down}, {ntaps}): invalid arguments")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=y.device)
    peaks = torch.empty(channels, dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        _lib.check(L.svs_resample_peaks(y.data_ptr(), channels, n_in, n_in, table.data_ptr(), ntaps, up, down, peaks.data_ptr(),
                                        ws.data_ptr(), nbytes, _lib.stream_ptr(y.device)), "svs_resample_peaks")
    return peaks


def encode_loudness_gpu(stems, up, down, code, dtype, loudness, ceiling, rate, frames, true_peak: bool = False, peaks_out=None,
                        peak: float = 0.9, *, subtype_bits=None, dither: str = "none", dither_seed: int = 0, limiter_ms=None, limiter_out=None):
    """resample_encode_gpu(loudness=): the stems (each (channels, n_in), float32, contiguous) are resampled into one float32 buffer
    by svs_resample_poly -- bit for bit the float the fused encoder forms -- cut or zero-padded to `frames`, measured there
    (svs_loudness_blocks on their sum, svs_resample_peaks per stem, svs_loudness_gain) and encoded 1/1 with the device gain.
    loudness None: the peak rule of encode_planar_gpu with `peak`.  true_peak, peaks_out, subtype_bits, dither, dither_seed, limiter_ms,
    limiter_out: as encode_planar_gpu takes them (limiter_ms without loudness is a ValueError before any device work).
    Returns (list of PCM tensors, gain, info), all on the device."""
    import torch
    from . import loudness as ld
    _check_limiter(limiter_ms, loudness, rate)
    y = stems[0]
    dev = y.device
    channels, n_in = y.shape
    L = _lib.lib()
    n_out = int(L.svs_resample_out_len(n_in, up, down))
    frames = n_out if frames is None else int(frames)
    if frames < 1:
        raise ValueError(f"frames must be positive, got {frames}")
    width = max(n_out, frames)
    table, ntaps = tap_table(up, down, dev)
    nst = len(stems)
    alloc = torch.zeros if frames > n_out else torch.empty                # the padded frames are silence
    buf = alloc((nst, channels, width), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for k, stem in enumerate(stems):
            _lib.check(L.svs_resample_poly(stem.data_ptr(), PCM_F32, 1, 0, n_in, n_in, channels, table.data_ptr(), ntaps, up, down,
                                           buf[k].data_ptr(), width, _lib.stream_ptr(dev)), "svs_resample_poly")
    outs, gains, info = encode_planar_gpu(buf, frames, code, dtype, loudness=loudness, ceiling=ceiling, rate=rate, true_peak=true_peak,
                                          peaks_out=peaks_out, peak=peak, subtype_bits=subtype_bits, dither=dither, dither_seed=dither_seed,
                                          limiter_ms=limiter_ms, limiter_out=limiter_out)
    return outs, gains[0], info


def _check_limiter(limiter_ms, loudness, rate):
    """The limiter's argument rules, before any device work: it belongs to a loudness target (the peak rule never exceeds its peak),
    and its half-width at the written rate stays in 1..1024 samples.  Returns the half-width, or None without a limiter."""
    if limiter_ms is None:
        return None
    if loudness is None:
        raise ValueError("limiter_ms= belongs to loudness=: the peak rule never exceeds its peak, so there is nothing to limit")
    if rate is None:
        raise ValueError("limiter_ms= needs rate=, the sample rate that is written")
    from . import limiter as lim
    return lim.half_width(rate, limiter_ms)


def encode_planar_gpu(buf, frames, code, dtype, *, loudness=None, ceiling: float = 0.9, rate=None, peak: float = 0.9, true_peak: bool = False,
                      peaks_out=None, subtype_bits=None, dither: str = "none", dither_seed: int = 0, limiter_ms=None, limiter_out=None):
    """Stems that are at the written rate already -- buf: (stems, channels, width) float32, contiguous, the first `frames` of every row
    being what is written -- measured and encoded 1/1 on existing kernels: svs_resample_peaks per stem, then either the loudness rule
    (svs_loudness_blocks on the stems' sum, svs_loudness_gain: ONE gain for all stems) or the peak rule (per stem, one common gain
    peak / its loudest channel's maximum), and svs_resample_encode with the one-tap table and the device gain.
    true_peak (needs rate): the maxima that the ceiling, or the peak rule, is held against are the TRUE peaks of the rows at `rate`
    (loudness.py; svs_true_peaks, one launch over all rows in place of the svs_resample_peaks launches), so that no inter-sample
    peak of a written file exceeds `ceiling` (or `peak`); the gain rules themselves are unchanged.  peaks_out: a dict that receives
    "sample_peaks" and "true_peaks", float32 device tensors (stems * channels,) of the rows before the gain, and "gains".
    subtype_bits (None: `code` decides, as above; 16: int16 whatever `code` says; 24: packed 24-bit frames, uint8 (frames, channels * 3))
    and dither ("none", "tpdf", "hp"; pcm.py): with 24 bits or a dither the last launches are svs_pcm_encode_dither in place of
    svs_resample_encode -- after the same gain, stem k with seed dither_seed + k, so the dither of two written files is uncorrelated.
    Dither belongs to 16 and 24 bits: beside int32 or float32 it is a ValueError.  Peaks, loudness and the gain rules do not change.
    limiter_ms (None: exactly the launches above; needs loudness and rate, a ValueError before any device work otherwise): a look-ahead
    limiter of that half-width in milliseconds (limiter.py).  L and the unlimited gain G are measured first (svs_loudness_blocks,
    svs_loudness_gain without peaks); then buf[:, :, :frames] is LIMITED IN PLACE -- the caller's buffer changes -- by one gain curve for
    all stems and channels (envelope against the true peaks with true_peak, svs_limiter_envelope / _curve / _apply); then the peaks
    of the limited rows are taken as above and svs_loudness_gain runs again with the block energies from BEFORE the limiter, the same
    target and ceiling: the written gain is min(G, ceiling / peak of the limited rows), so the bound on every written file is the
    one above.  limiter_out: a dict that receives "curve" (the gain curve, float32 device (frames,)) and "limited_info"
    (svs_loudness_gain's 4 doubles measured on the limited rows, before the gain: one more svs_loudness_blocks).
    Returns (list of PCM tensors (frames, channels), list of gain tensors, info or None), all on the device."""
    import torch
    from . import loudness as ld
    from . import pcm
    dither_kind = pcm.dither_code(dither)
    if subtype_bits not in (None, 16, 24):
        raise ValueError(f"subtype_bits {subtype_bits}: None, 16 or 24")
    if subtype_bits == 16:
        code, dtype = _PCM["int16"]
    if dither_kind and subtype_bits != 24 and code != PCM_I16:
        raise ValueError(f"dither {dither!r} belongs to 16- and 24-bit output, not to {np.dtype(dtype).name}")
    bits = 24 if subtype_bits == 24 else 16 if dither_kind else None     # None: svs_resample_encode writes `code`
    _check_limiter(limiter_ms, loudness, rate)
    dev = buf.device
    nst, channels, width = buf.shape
    frames = int(frames)
    L = _lib.lib()
    one, _ = tap_table(1, 1, dev)
    if true_peak and rate is None:
        raise ValueError("true_peak= needs rate=, the sample rate that is written")
    z_before = None
    if limiter_ms is not None:
        from . import limiter as lim
        view = buf[:, :, :frames]
        z_before = ld.block_energies_gpu(view if nst == 2 else view[0], rate, nst)
        first = ld.gain_from_blocks_gpu(z_before, loudness, ceiling=ceiling, channels=channels)[1]
        curve = lim.limit_rows_gpu(buf, frames, first[2:], ceiling, rate, limiter_ms, true_peak)
        if limiter_out is not None:
            limiter_out["curve"] = curve
            limiter_out["limited_info"] = ld.loudness_gain_gpu(view if nst == 2 else view[0], rate, None, stems=nst)[1]
    if true_peak:
        sample_peaks, peaks = ld.true_peaks_rows_gpu(buf.data_ptr(), nst, channels, frames, channels * width, width, ld.true_peak_factor(rate),
                                                     dev, sample=peaks_out is not None)
        if peaks_out is not None:
            peaks_out["sample_peaks"], peaks_out["true_peaks"] = sample_peaks, peaks
    else:
        peaks = torch.empty(nst * channels, dtype=torch.float32, device=dev)
        nbytes = int(L.svs_resample_peaks_workspace_bytes(frames, channels, 1, 1, 1))
        if nbytes == 0:
            raise _lib.SvsError(f"svs_resample_peaks_workspace_bytes({frames}, {channels}, 1, 1, 1): invalid arguments")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if bits == 24:
        outs = [torch.empty((frames, channels * 3), dtype=torch.uint8, device=dev) for _ in range(nst)]
    else:
        outs = [torch.empty((frames, channels), dtype=getattr(torch, np.dtype(dtype).name), device=dev) for _ in range(nst)]
    with torch.cuda.device(dev):
        s = _lib.stream_ptr(dev)
        for k in range(0 if true_peak else nst):
            _lib.check(L.svs_resample_peaks(buf[k].data_ptr(), channels, frames, width, one.data_ptr(), 1, 1, 1,
                                            peaks[k * channels:].data_ptr(), ws.data_ptr(), nbytes, s), "svs_resample_peaks")
        info = None
        if loudness is not None:
            view = buf[:, :, :frames]
            if z_before is not None:
                gain, info = ld.gain_from_blocks_gpu(z_before, loudness, ceiling=ceiling, peaks=peaks, channels=channels)
            else:
                gain, info = ld.loudness_gain_gpu(view if nst == 2 else view[0], rate, loudness, ceiling=ceiling, stems=nst, peaks=peaks,
                                                  channels=channels)
            gains = [gain] * nst
        else:                                                              # data.py:162-164 per written file, one gain for its channels
            gains = [torch.full((channels,), float(peak), dtype=torch.float32, device=dev) for _ in range(nst)]
            top = torch.empty(nst, dtype=torch.float32, device=dev)
            for k, gain in enumerate(gains):
                _lib.check(L.svs_max(peaks[k * channels:].data_ptr(), channels, top[k:].data_ptr(), s), "svs_max")
                _lib.check(L.svs_scale_by_inv(gain.data_ptr(), channels, top[k:].data_ptr(), 1.0, s), "svs_scale_by_inv")
        for k, out in enumerate(outs):
            if bits is not None:
                pcm.encode_dither_gpu(buf[k], frames, gains[k], bits, dither_kind, int(dither_seed) + k, out=out)
                continue
            _lib.check(L.svs_resample_encode(buf[k].data_ptr(), channels, frames, width, one.data_ptr(), 1, 1, 1, gains[k].data_ptr(), code,
                                             out.data_ptr(), s), "svs_resample_encode")
    if true_peak and peaks_out is not None:
        peaks_out["gains"] = gains
    return outs, gains, info


def resample_encode_gpu(y, up: int, down: int, *, fmt="int16", peak: float | None = 0.9, common_gain: bool = True,
                        loudness=None, ceiling: float = 0.9, together=None, rate: int | None = None, frames: int | None = None,
                        true_peak: bool = False, subtype_bits=None, dither: str = "none", dither_seed: int = 0, limiter_ms=None):
    """float32 device tensor (n,) or (channels, n), planar -> device tensor (n_out,) or (n_out, channels) of int16 / int32 /
    float32 at rate * up / down, interleaved as a wav file stores it (svs_resample_encode; the rules: encode_pcm_reference).
    peak=None: the samples are encoded as they are.  Otherwise they are scaled by peak / max |resampled signal| on the way
    (data.py:162-164, at the rate that is written): the maximum comes from a first run of the FIR that stores nothing
    (svs_resample_peaks; measured against materialising the float32 signal once: DESIGN.md section 10b) and the gain is formed
    on the device, so nothing waits for the host.  common_gain=True: one gain
    for all channels, from the loudest (a stereo file keeps its balance; mono is the reference's rule); False: every channel
    is normalised on its own, as istft_from_tiles(peak=) does.  A silent signal (maximum 0) is divided by 1, the rule of
    svs_scale_by_inv, and stays silent.

    loudness (LUFS: a number, or a float64 device tensor whose first element holds it) replaces the peak rule by a loudness
    target (loudness.py): the samples at `rate` (required: the rate that is written, which K-weighting depends on) are brought to
    that integrated loudness by one gain for all channels, min(10^((loudness - L) / 20), ceiling / peak).  together: a second
    stem of y's shape that is written with it; L is then the loudness of the two stems' sum, peak the larger of theirs, and both
    get the same gain, so their balance is kept.  frames: cut or zero-pad to this many frames before measuring, so that what is
    measured is what is written.  Returns (pcm, info) or, with together, (pcm, pcm of together, info); info: 4 device doubles
    (L before the gain, kept blocks, unlimited gain, 1 when the ceiling limited it).  peak and common_gain are not read.

    true_peak (needs rate): the ceiling of the loudness rule is held against the true peaks at `rate` (loudness.py: the 4x / 2x
    over-sampled signal) instead of the sample peaks.  Without loudness the signal goes by the planar buffer (svs_resample_poly to
    float32, then encode_planar_gpu's peak rule with one common gain against the true peaks): peak must be given and common_gain
    True; the return value is the PCM alone.

    subtype_bits=24 (packed 24-bit frames, uint8 (n_out, channels * 3); fmt is then not read) and dither= "tpdf" / "hp" with dither_seed
    (pcm.py; 16 and 24 bits only) are encode_planar_gpu's: the signal goes by the planar buffer as with true_peak, so without
    loudness it is the peak rule with one common gain as well (peak given, common_gain True).  With together, y is encoded with
    dither_seed and the second stem with dither_seed + 1.

    limiter_ms (only with loudness; a ValueError before any device work otherwise): encode_planar_gpu's look-ahead limiter of that
    half-width in milliseconds, one gain curve for y and together; info is then that of the limited signal's gain."""
    import torch
    _check_limiter(limiter_ms, loudness, rate)
    planar = subtype_bits is not None or dither != "none"
    if planar and loudness is None and (peak is None or not common_gain):
        raise ValueError("subtype_bits= / dither= without loudness= is the peak rule with one common gain: peak= must be given and common_gain True")
    if loudness is None and (together is not None or frames is not None):
        raise ValueError("together= and frames= belong to loudness=")
    if true_peak and rate is None:
        raise ValueError("true_peak= needs rate=, the sample rate that is written")
    if true_peak and loudness is None and (peak is None or not common_gain):
        raise ValueError("true_peak= without loudness= is the peak rule with one common gain: peak= must be given and common_gain True")
    if not y.is_cuda:
        raise ValueError("resample_encode_gpu needs a device tensor (there is no CPU path)")
    if y.dtype != torch.float32:
        raise TypeError(f"resample_encode_gpu: dtype {y.dtype} (float32)")
    if y.dim() not in (1, 2) or y.shape[-1] < 1:
        raise ValueError(f"input must be (n,) or (channels, n), got {tuple(y.shape)}")
    code, dtype = pcm_format("int16" if subtype_bits is not None else fmt)
    up, down = reduced(up, down)
    squeeze = y.dim() == 1
    y = (y[None] if squeeze else y).contiguous()
    channels, n_in = y.shape
    how = dict(subtype_bits=subtype_bits, dither=dither, dither_seed=dither_seed)
    if loudness is not None:
        if rate is None:
            raise ValueError("loudness= needs rate=, the sample rate that is written")
        stems = [y]
        if together is not None:
            t = (together[None] if together.dim() == 1 else together).contiguous()
            if not t.is_cuda or t.dtype != torch.float32 or t.shape != y.shape:
                raise ValueError(f"together must be a float32 device tensor of the same shape, got {tuple(together.shape)}")
            stems.append(t)
        outs, _, info = encode_loudness_gpu(stems, up, down, code, dtype, loudness, ceiling, int(rate), frames, true_peak, limiter_ms=limiter_ms, **how)
        outs = [o[:, 0] if squeeze and o.dtype != torch.uint8 else o for o in outs]
        return (*outs, info)
    if true_peak or planar:
        outs, _, _ = encode_loudness_gpu([y], up, down, code, dtype, None, ceiling, None if rate is None else int(rate), None, true_peak,
                                         peak=float(peak), **how)
        return outs[0][:, 0] if squeeze and outs[0].dtype != torch.uint8 else outs[0]
    L = _lib.lib()
    n_out = int(L.svs_resample_out_len(n_in, up, down))
    table, ntaps = tap_table(up, down, y.device)
    out = torch.empty((n_out, channels), dtype=getattr(torch, np.dtype(dtype).name), device=y.device)
    with torch.cuda.device(y.device):
        s = _lib.stream_ptr(y.device)
        gain = None
        if peak is not None:
            peaks = resample_peaks_gpu(y, up, down)
            gain = torch.full((channels,), float(peak), dtype=torch.float32, device=y.device)
            if common_gain:
                top = torch.empty(1, dtype=torch.float32, device=y.device)
                _lib.check(L.svs_max(peaks.data_ptr(), channels, top.data_ptr(), s), "svs_max")
                _lib.check(L.svs_scale_by_inv(gain.data_ptr(), channels, top.data_ptr(), 1.0, s), "svs_scale_by_inv")
            else:
                for c in range(channels):
                    _lib.check(L.svs_scale_by_inv(gain[c:].data_ptr(), 1, peaks[c:].data_ptr(), 1.0, s), "svs_scale_by_inv")
        _lib.check(L.svs_resample_encode(y.data_ptr(), channels, n_in, n_in, table.data_ptr(), ntaps, up, down, _lib.ptr(gain), code,
                                         out.data_ptr(), s), "svs_resample_encode")
    return out[:, 0] if squeeze else out
