"""24-bit PCM in and out, and TPDF dither for the written stems (csrc/pcm.hip: svs_pcm24_widen, svs_pcm_encode_dither).

The way in: a 24-bit wav file stores 3 bytes per sample.  read_pcm_device copies exactly those bytes to the device and widens them
there to the left-justified int32 that scipy.io.wavfile.read returns for such a file and that SVS_PCM_I32 takes, so everything
downstream (resample.resample_poly_gpu, fullband.fullband_mix_gpu) is unchanged, bit for bit.

The way out: svs_pcm_encode_dither encodes planar float32 rows that are at the written rate already (the buffer
resample.encode_planar_gpu holds) to int16 or packed 24-bit frames, with no dither, TPDF dither or high-passed TPDF dither from the
project's counter generator (synth.u32).  The definitions here restate its arithmetic in numpy, bit for bit:

    v = y * gain                                   one float32 multiply (none without a gain)
    u(m) = (u32(seed, m) >> 8) * 2^-24             synth.uniform
    tpdf   d = u(2 (F channels + c)) - u(2 (F channels + c) + 1)
    hp     d = u((F + 1) channels + c) - u(F channels + c)           F = first_frame + i, the absolute frame
    Q = 2^(bits - 1) - 1
    16 bits without dither: clip(rint(v * float32(32767)), -32768, 32767), resample.encode_pcm_reference's int16 rule
    otherwise:              clip(rint(float64(v) * Q + float64(d)), -2^(bits-1), 2^(bits-1) - 1);  NaN -> 0

The total error of a quantiser with TPDF dither of 2 LSB peak to peak has mean 0 and variance 1/4 LSB^2 whatever the input is: no
harmonic distortion, no noise modulation on a fade.  The high-passed form has the same density per sample and a lag-1 correlation of
-1/2, which moves the dither's power towards the Nyquist rate.  The reference writes 16-bit through libsndfile without dither
(data.py:166) and has no 24-bit path.
"""
from __future__ import annotations

import struct

import numpy as np

from . import _lib
from .synth import u32

DITHERS = {"none": 0, "tpdf": 1, "hp": 2}                  # include/svs_hip.h: svs_pcm_encode_dither's `dither`
SUBTYPES = ("PCM_16", "PCM_24", "PCM_32", "FLOAT")          # what can be written; "source" resolves to one of them

_PCM_GUID_TAIL = b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
_TAG_PCM, _TAG_FLOAT, _TAG_EXTENSIBLE = 1, 3, 0xFFFE


def dither_code(kind) -> int:
    if kind not in DITHERS:
        raise ValueError(f"dither {kind!r}: one of {sorted(DITHERS)}")
    return DITHERS[kind]


def encoder_bits(subtype: str, dither: str = "none"):
    """The word length svs_pcm_encode_dither is asked for when `subtype` is written with `dither`, or None when the existing encoder
    (svs_resample_encode) writes it.  Dither beside PCM_32 or FLOAT is a ValueError: a float32 stem has nothing below the 24th bit
    to linearise."""
    dither_code(dither)
    if subtype not in SUBTYPES:
        raise ValueError(f"subtype {subtype!r}: one of {SUBTYPES}")
    if subtype == "PCM_24":
        return 24
    if dither == "none":
        return None
    if subtype != "PCM_16":
        raise ValueError(f"dither {dither!r} with subtype {subtype}: dither belongs to PCM_16 and PCM_24")
    return 16


def _uniform(seed: int, idx) -> np.ndarray:
    return (u32(seed, idx) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def dither_reference(kind: str, seed: int, first_frame: int, frames: int, channels: int) -> np.ndarray:
    """float32 (frames, channels): the dither, in LSB, of frames first_frame .. first_frame + frames - 1."""
    code = dither_code(kind)
    if first_frame < 0 or frames < 0 or channels < 1:
        raise ValueError(f"first_frame {first_frame}, frames {frames}, channels {channels}")
    F = (np.arange(frames, dtype=np.uint64) + np.uint64(first_frame))[:, None]
    c = np.arange(channels, dtype=np.uint64)[None, :]
    ch = np.uint64(channels)
    if code == 1:
        m = np.uint64(2) * (F * ch + c)
        return _uniform(seed, m) - _uniform(seed, m + np.uint64(1))
    if code == 2:
        return _uniform(seed, (F + np.uint64(1)) * ch + c) - _uniform(seed, F * ch + c)
    return np.zeros((frames, channels), dtype=np.float32)


def encode_dither_reference(y, gain, bits: int, kind: str, seed: int, first_frame: int = 0) -> np.ndarray:
    """numpy restatement of svs_pcm_encode_dither.  y: (n, channels) or (n,) float32; gain: None, a scalar or `channels` float32
    values.  Returns the integers that are written, in y's shape: int16 for 16 bits, int32 in [-2^23, 2^23) for 24 (pack24 makes the
    bytes of them)."""
    if bits not in (16, 24):
        raise ValueError(f"bits {bits}: 16 or 24")
    code = dither_code(kind)
    v = np.asarray(y, dtype=np.float32)
    if gain is not None:
        v = v * np.asarray(gain, dtype=np.float32)
    q = float(2 ** (bits - 1) - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        if bits == 16 and code == 0:
            s = np.rint(v * np.float32(32767.0)).astype(np.float64)
        else:
            v2 = v.reshape(v.shape[0], -1)
            d = dither_reference(kind, seed, first_frame, v2.shape[0], v2.shape[1]).reshape(v.shape)
            s = np.rint(v.astype(np.float64) * q + d.astype(np.float64))
        s = np.where(np.isnan(s), 0.0, np.clip(s, -(q + 1.0), q))
    return np.ascontiguousarray(s.astype(np.int16 if bits == 16 else np.int32))


def pack24(values) -> np.ndarray:
    """int32 values in [-2^23, 2^23) -> uint8 (..., 3): the little-endian two's-complement bytes a 24-bit wav file stores."""
    u = np.asarray(values).astype(np.int32).view(np.uint32)
    return np.stack([(u & 0xFF), (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)


def unpack24(packed) -> np.ndarray:
    """uint8 bytes whose last axis (or, for a flat array, every run of 3) holds one sample -> the left-justified int32
    (b0 << 8 | b1 << 16 | b2 << 24) that scipy.io.wavfile.read returns for a 24-bit file."""
    b = np.asarray(packed, dtype=np.uint8)
    if b.ndim == 1 or b.shape[-1] != 3:
        if b.shape[-1] % 3:
            raise ValueError(f"unpack24: {b.shape[-1]} bytes are no whole number of 3-byte samples")
        b = b.reshape(b.shape[:-1] + (b.shape[-1] // 3, 3))
    w = b.astype(np.uint32)
    return ((w[..., 0] << 8) | (w[..., 1] << 16) | (w[..., 2] << 24)).view(np.int32)


# ------------------------------------------------------------------------------------------------
# the wav container: a RIFF chunk walk for the way in, a 24-bit writer for the way out
# ------------------------------------------------------------------------------------------------
def wav_info(path: str):
    """The `fmt ` and `data` chunks of a little-endian RIFF / WAVE file: a dict with tag (1 PCM, 3 float, the sub-format's for
    WAVE_FORMAT_EXTENSIBLE), channels, rate, block_align, bits, data_offset and data_bytes; None for anything else (RIFX, RF64, a
    missing chunk, a data chunk that runs past the file)."""
    try:
        with open(path, "rb") as f:
            head = f.read(12)
            if len(head) < 12 or head[:4] != b"RIFF" or head[8:] != b"WAVE":
                return None
            f.seek(0, 2)
            size = f.tell()
            pos, fmt = 12, None
            while pos + 8 <= size:
                f.seek(pos)
                cid, n = struct.unpack("<4sI", f.read(8))
                if cid == b"fmt ":
                    body = f.read(min(n, 40))
                    if len(body) < 16:
                        return None
                    tag, channels, rate, _, align, bits = struct.unpack("<HHIIHH", body[:16])
                    if tag == _TAG_EXTENSIBLE:
                        if len(body) < 40 or body[26:40] != _PCM_GUID_TAIL:
                            return None
                        tag = struct.unpack("<H", body[24:26])[0]
                    fmt = dict(tag=tag, channels=channels, rate=rate, block_align=align, bits=bits)
                elif cid == b"data":
                    if fmt is None or pos + 8 + n > size:
                        return None
                    return dict(fmt, data_offset=pos + 8, data_bytes=n)
                pos += 8 + n + (n & 1)
    except OSError:
        return None
    return None


def subtype_of(path: str) -> str:
    """The subtype name of a wav file ("PCM_16", "PCM_24", "PCM_32", "FLOAT"), for --subtype source.  An 8-bit source maps to PCM_16
    (8-bit output is not written), a 64-bit float one to FLOAT."""
    info = wav_info(path)
    if info is None:
        raise ValueError(f"{path}: not a little-endian RIFF / WAVE file with a fmt and a data chunk")
    if info["tag"] == _TAG_FLOAT:
        return "FLOAT"
    if info["tag"] == _TAG_PCM and info["bits"] in (8, 16, 24, 32):
        return {8: "PCM_16", 16: "PCM_16", 24: "PCM_24", 32: "PCM_32"}[info["bits"]]
    raise ValueError(f"{path}: format tag {info['tag']} with {info['bits']} bits has no subtype this project writes")


def write_wav24(path: str, rate: int, packed):
    """uint8 (frames, channels * 3) (encode_dither_gpu's, or pack24's (frames, channels, 3) / (frames, 3)) -> a 24-bit PCM wav file:
    the plain 44-byte header for one or two channels, WAVE_FORMAT_EXTENSIBLE with the PCM sub-format above (as the format's
    specification asks)."""
    b = np.ascontiguousarray(packed, dtype=np.uint8)
    if b.ndim == 3:
        b = b.reshape(b.shape[0], -1)
    if b.ndim != 2 or b.shape[1] < 3 or b.shape[1] % 3:
        raise ValueError(f"write_wav24: packed {b.shape} is not (frames, channels * 3)")
    channels, nbytes = b.shape[1] // 3, b.size
    if nbytes + 68 > 0xFFFFFFFF:
        raise ValueError("write_wav24: more than 4 GiB do not fit a RIFF file")
    rate = int(rate)
    fmt = struct.pack("<HHIIHH", _TAG_PCM if channels <= 2 else _TAG_EXTENSIBLE, channels, rate, rate * channels * 3, channels * 3, 24)
    if channels > 2:
        fmt += struct.pack("<HHIH", 22, 24, 0, _TAG_PCM) + _PCM_GUID_TAIL
    pad = nbytes & 1
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + nbytes + pad) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        f.write(b"data" + struct.pack("<I", nbytes))
        f.write(b.tobytes())
        if pad:
            f.write(b"\x00")


# ------------------------------------------------------------------------------------------------
# device wrappers
# ------------------------------------------------------------------------------------------------
def widen24_gpu(packed):
    """uint8 device tensor of 3-byte samples (any shape whose element count is a multiple of 3; a last axis of 3 is dropped) ->
    int32 device tensor of the left-justified words (svs_pcm24_widen)."""
    import torch
    if not packed.is_cuda:
        raise ValueError("widen24_gpu needs a device tensor (there is no CPU path)")
    if packed.dtype != torch.uint8:
        raise TypeError(f"widen24_gpu: dtype {packed.dtype} (uint8)")
    packed = packed.contiguous()
    n3 = packed.numel()
    if n3 < 3 or n3 % 3:
        raise ValueError(f"widen24_gpu: {n3} bytes are no whole, positive number of 3-byte samples")
    shape = packed.shape[:-1] if packed.dim() > 1 and packed.shape[-1] == 3 else (n3 // 3,)
    out = torch.empty(n3 // 3, dtype=torch.int32, device=packed.device)
    with torch.cuda.device(packed.device):
        _lib.check(_lib.lib().svs_pcm24_widen(packed.data_ptr(), n3 // 3, out.data_ptr(), _lib.stream_ptr(packed.device)), "svs_pcm24_widen")
    return out.view(shape)


def encode_dither_gpu(buf, frames: int, gain, bits: int, dither, seed: int = 0, first_frame: int = 0, out=None):
    """buf: float32 device tensor (channels, width) (or (width,)), rows contiguous, at the written rate; the first `frames` samples of
    every row -> int16 (frames, channels), or uint8 (frames, channels * 3) for 24 bits, interleaved as a wav file stores them
    (svs_pcm_encode_dither).  gain: None or a float32 device tensor (channels,).  dither: "none" / "tpdf" / "hp" or the code."""
    import torch
    if not buf.is_cuda:
        raise ValueError("encode_dither_gpu needs a device tensor (there is no CPU path)")
    if buf.dtype != torch.float32:
        raise TypeError(f"encode_dither_gpu: dtype {buf.dtype} (float32)")
    if buf.dim() == 1:
        buf = buf[None]
    if buf.dim() != 2 or buf.stride(1) != 1:
        raise ValueError(f"encode_dither_gpu: buf must be (channels, width) with contiguous rows, got {tuple(buf.shape)}")
    channels, width = buf.shape
    frames = int(frames)
    if not 1 <= frames <= width:
        raise ValueError(f"encode_dither_gpu: frames {frames} outside 1..{width}")
    if bits not in (16, 24):
        raise ValueError(f"encode_dither_gpu: bits {bits} (16 or 24)")
    code = dither if isinstance(dither, int) else dither_code(dither)
    ld_in = buf.stride(0) if channels > 1 else width
    if out is None:
        out = torch.empty((frames, channels) if bits == 16 else (frames, channels * 3), dtype=torch.int16 if bits == 16 else torch.uint8,
                          device=buf.device)
    with torch.cuda.device(buf.device):
        _lib.check(_lib.lib().svs_pcm_encode_dither(buf.data_ptr(), channels, frames, ld_in, _lib.ptr(gain), bits, code,
                                                    int(seed) & 0xFFFFFFFF, int(first_frame), out.data_ptr(),
                                                    _lib.stream_ptr(buf.device)), "svs_pcm_encode_dither")
    return out


def read_pcm_device(path: str, device):
    """wav file -> (rate, device tensor (frames,) or (frames, channels), channels), the samples as the device kernels take them.
    A 24-bit PCM file (plain WAVE_FORMAT_PCM, or WAVE_FORMAT_EXTENSIBLE with the PCM sub-format, block_align == 3 * channels,
    little-endian RIFF): the bytes of its data chunk go to the device as the file stores them, 3 per sample, and svs_pcm24_widen
    makes the left-justified int32 of them there (8.0 ms against 70.7 ms by the host route for 240 s of stereo: DESIGN.md section
    24).  Everything else, and whatever the chunk walk does not recognise: data.read_pcm and .to(device), as before."""
    import torch
    info = wav_info(path)
    if (info is not None and info["tag"] == _TAG_PCM and info["bits"] == 24 and 1 <= info["channels"] <= 64
            and info["block_align"] == 3 * info["channels"] and info["data_bytes"] >= info["block_align"]):
        channels = info["channels"]
        frames = info["data_bytes"] // info["block_align"]
        raw = np.fromfile(path, dtype=np.uint8, count=frames * channels * 3, offset=info["data_offset"])
        if raw.size == frames * channels * 3:
            wide = widen24_gpu(torch.from_numpy(raw).to(device))
            return info["rate"], (wide if channels == 1 else wide.view(frames, channels)), channels
    from .data import read_pcm
    rate, data, channels = read_pcm(path)
    return rate, torch.from_numpy(data).to(device), channels
