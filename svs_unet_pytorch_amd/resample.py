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
