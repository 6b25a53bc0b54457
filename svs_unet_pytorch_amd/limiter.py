"""Look-ahead true-peak limiter for loud targets: the float64 definition (numpy) and the device path on csrc/limiter.hip
(include/svs_hip.h).  The reference has no limiter: it peak-normalises every written stem (data.py:162-166).

The loudness rule applies gain = min(G, ceiling / peak) with G = 10^((target - L) / 20): one transient of a separated vocal decides the
level of the whole file, which then comes out several LU under the target.  The limiter bends the gain around such peaks so that the
cap lands within a hair of G.  On the planar rows x[row][i] at the written rate, row = stem * channels + c, 0 <= i < n:

1. Envelope, linked over ALL rows (stems and channels: one gain curve per call, so the written files still add up to
   g(t) * (their sum) and a stereo file keeps its balance):
       e[i] = max_row max(|x[i]|, max_{p=1..f-1} |y_row[f i + p]|)
   y the over-sampled signal of loudness.true_peak_reference (the same taps, zeros outside [0, n)); f = loudness.true_peak_factor(rate)
   with true_peak, else f = 1 and e[i] = max_row |x[i]|.  e is rounded to float32.
2. Gain curve from G (the unlimited static gain), the ceiling C and a half-width h in samples, 1 <= h <= 1024:
       r[i] = 1 where G e[i] <= C, else float32(C / (G float64(e[i])));  r = 1 outside [0, n)                  (demand)
       m[j] = min_{|k| <= h} r[j + k]                                                                            (exact)
       a[i] = sum_{k=-h..h} w[k] m[i + k],  w = window(h)     (float32 fmaf from 0, k ascending, on the device; float64 here)
       g[i] = min(a[i], r[i])
   Every m that enters a[i] comes from a window that contains i, so a[i] <= r[i] sum(w), and the final min makes g <= r exact.
   window(h) is scaled so that its sum, in float64 and in the device's float32 order, is not below 1: where no e within 2h of i is
   over the ceiling every m is 1, a[i] >= 1 and g[i] = 1 exactly.  A peak bends the gain over +-2h samples, attack and release alike.
   G that is not finite and positive (the silent file, L = -inf) gives g = 1 everywhere.
3. Apply: z[row][i] = x[row][i] g[i], one float32 multiply, in place.

After that the EXISTING gain rule runs on the limited rows (resample.encode_planar_gpu(limiter_ms=)): peaks of z, then
svs_loudness_gain with the block energies of the signal BEFORE the limiter; the written gain is min(G, C / peak(z)), so the hard
bound of every written file is today's, whatever the gain modulation did between the samples.  On that way the limiter itself aims
at inner_ceiling(C) = C (1 - 2^-21), which keeps the float32 roundings of its own products from crossing C.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from . import loudness as ld

H_MIN, H_MAX = 1, 1024                          # csrc/limiter.hip: LC_H_MAX
DEFAULT_MS = 2.0
MARGIN = 2.0 ** -21


def inner_ceiling(ceiling) -> float:
    """The ceiling the limiter of the way out aims at, ceiling (1 - 2^-21).  Between r and a written sample lie four float32 roundings
    (r itself, x g, the gain's, and the product with the gain), together under 2^-22 relative: aimed at the ceiling itself, every
    limited peak would land within an ulp of it on either side, and the gain rule's cap C / peak would undercut G at random.  With the
    margin (4e-6 dB) the limited peaks stay strictly under the ceiling and the cap stays above G."""
    return float(ceiling) * (1.0 - MARGIN)


def check_h(h) -> int:
    if int(h) != h or not H_MIN <= int(h) <= H_MAX:
        raise ValueError(f"the limiter's half-width must be a whole number of samples in {H_MIN}..{H_MAX}, got {h}")
    return int(h)


def half_width(rate, ms) -> int:
    """max(1, round(rate * ms / 1000)) samples; ValueError when that leaves 1..1024 (or ms is not a positive number)."""
    ms = float(ms)
    if not (math.isfinite(ms) and ms > 0.0):
        raise ValueError(f"the limiter's time must be a positive number of milliseconds, got {ms}")
    h = max(1, int(round(float(rate) * ms / 1000.0)))
    if h > H_MAX:
        raise ValueError(f"a limiter time of {ms:g} ms is {h} samples at {rate} Hz; the half-width must stay in {H_MIN}..{H_MAX} "
                         f"(at most {1000.0 * H_MAX / float(rate):.2f} ms at this rate)")
    return h


def fp32_sum(w) -> np.float32:
    """The sum of float32 weights in the kernel's order: acc = fmaf(w[k], 1, acc) = float32(acc + w[k]), k ascending, from 0."""
    acc = np.float32(0.0)
    for v in np.asarray(w, dtype=np.float32):
        acc = np.float32(acc + v)
    return acc


def window(h: int) -> np.ndarray:
    """The 2h + 1 float32 smoothing weights: w[k] ~ 1 - cos(2 pi (k + h + 1) / (2h + 2)), k = -h..h (a Hann window without its zero
    ends: strictly positive, symmetric), normalised in float64 and rounded to float32.  The centre weight is then raised by the few
    float32 steps it takes for the sum to be at least 1 both in float64 and in the kernel's float32 order (fp32_sum), so that a
    stretch of m = 1 gives a >= 1 and g = min(a, 1) = 1 exactly; the sum stays within (2h + 2) 2^-24 of 1."""
    h = check_h(h)
    k = np.arange(-h, h + 1, dtype=np.float64)
    w = 1.0 - np.cos(2.0 * np.pi * (k + h + 1) / (2 * h + 2))
    w = (w / w.sum()).astype(np.float32)
    while True:
        short = max(1.0 - float(fp32_sum(w)), 1.0 - float(w.astype(np.float64).sum()))
        if short <= 0.0:
            return w
        w[h] = max(np.float32(float(w[h]) + short), np.nextafter(w[h], np.float32(2.0)))


_WINDOWS: dict = {}


def window_gpu(h: int, device):
    """window(h) on `device`, uploaded once per (h, device)."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (check_h(h), str(device))
    if key not in _WINDOWS:
        _WINDOWS[key] = torch.from_numpy(window(h)).to(device)
    return _WINDOWS[key]


# ------------------------------------------------------------------------------------------------
# the float64 definition
# ------------------------------------------------------------------------------------------------
def envelope_reference(x, factor: int = 1, taps=None) -> np.ndarray:
    """e of stage 1 in float64 (not yet rounded).  x: (rows, n) or (n,).  taps: the 12 factor + 1 taps (default
    loudness.true_peak_taps(factor); a test hands over the float32-rounded taps of the device)."""
    x = np.asarray(x, dtype=np.float64)
    x = x[None] if x.ndim == 1 else x.reshape(-1, x.shape[-1])
    f = int(factor)
    h = ld.true_peak_taps(f) if taps is None else np.asarray(taps, dtype=np.float64)
    if h.shape != (12 * f + 1,):
        raise ValueError(f"factor {f} takes {12 * f + 1} taps, got {h.shape}")
    n = x.shape[1]
    e = np.abs(x).max(axis=0) if n else np.zeros(0)
    if n and f > 1:
        xp = np.pad(x, ((0, 0), (6, 6)))                           # xp[i + 6] = x[i]
        for p in range(1, f):
            y = np.zeros_like(x)
            for k in range(12):
                y += h[p + f * k] * xp[:, 12 - k:12 - k + n]
            e = np.maximum(e, np.abs(y).max(axis=0))
    return e


def demand(e, G, ceiling) -> np.ndarray:
    """r of stage 2 as float32, bit for bit the device's: e is taken as float32."""
    e = np.asarray(e, dtype=np.float32).astype(np.float64)
    G, C = float(G), float(ceiling)
    r = np.ones(e.shape, dtype=np.float32)
    if not (math.isfinite(G) and G > 0.0):
        return r
    d = G * e
    over = ~(d <= C)
    with np.errstate(divide="ignore", invalid="ignore"):
        r[over] = (C / d[over]).astype(np.float32)
    return r


def sliding_min(r, h: int) -> np.ndarray:
    """m[j] = min_{|k| <= h} r[j + k] for -h <= j < n + h (index j + h), r = 1 outside [0, n)."""
    r = np.asarray(r)
    n = r.shape[0]
    rp = np.concatenate([np.ones(2 * h, r.dtype), r, np.ones(2 * h, r.dtype)])      # rp[i + 2h] = r[i]
    m = rp[:n + 2 * h].copy()
    for k in range(1, 2 * h + 1):
        np.minimum(m, rp[k:k + n + 2 * h], out=m)
    return m


def curve_reference(e, G, ceiling, h: int, w=None):
    """(g, r) of stage 2: g float64 (the sum in float64 with the float32 weights), r float32 (exact)."""
    h = check_h(h)
    if not float(ceiling) > 0.0:
        raise ValueError(f"the ceiling must be positive, got {ceiling}")
    w = (window(h) if w is None else np.asarray(w)).astype(np.float64)
    r = demand(e, G, ceiling)
    n = r.shape[0]
    m = sliding_min(r, h).astype(np.float64)                       # m[j + h]
    a = np.zeros(n)
    for k in range(2 * h + 1):
        a += w[k] * m[k:k + n]
    return np.minimum(a, r.astype(np.float64)), r


def limiter_reference(x, G, ceiling, h: int, *, factor: int = 1, taps=None):
    """The three stages on x: (stems, channels, n), (rows, n) or (n,).  Returns (z, g, r, e): z float32 of x's shape, the float32
    multiply x * float32(g); g float64 (n,); r float32 (n,); e float32 (n,).  factor, taps: envelope_reference's."""
    x32 = np.asarray(x, dtype=np.float32)
    e = envelope_reference(x32, factor, taps).astype(np.float32)
    g, r = curve_reference(e, G, ceiling, h)
    return x32 * g.astype(np.float32), g, r, e


# ------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------
def envelope_rows_gpu(x_ptr, stems, channels, n, ld_stem, ld_ch, factor, device):
    """svs_limiter_envelope on rows given by address: float32 device tensor (n,)."""
    import torch
    if factor not in (1, 2, 4):
        raise ValueError(f"the over-sampling factor must be 1, 2 or 4, got {factor}")
    e = torch.empty(int(n), dtype=torch.float32, device=device)
    taps = ld.true_peak_taps_gpu(factor, device) if factor > 1 else None
    with torch.cuda.device(device):
        _lib.check(_lib.lib().svs_limiter_envelope(x_ptr, stems, channels, int(n), ld_stem, ld_ch, _lib.ptr(taps), factor, e.data_ptr(),
                                                   _lib.stream_ptr(device)), "svs_limiter_envelope")
    return e


def envelope_gpu(x, factor: int = 1, stems: int = 1):
    """e of a float32 device signal (n,), (channels, n) or, with stems = 2, (2, channels, n): float32 device tensor (n,), the
    maximum over all rows of |x| and of the factor - 1 interpolated values after each sample."""
    x, channels, n, ld_stem, ld_ch = ld._planar(x, stems)
    return envelope_rows_gpu(x.data_ptr(), stems, channels, n, ld_stem if stems > 1 else channels * ld_ch, ld_ch, int(factor), x.device)


def curve_gpu(e, G, ceiling, h: int):
    """g of svs_limiter_curve: float32 device tensor (n,).  e: float32 device tensor (n,); G: a number, or a float64 device tensor
    whose first element holds it (info[2:] of loudness_gain_gpu).  h and the ceiling are checked before any device work."""
    import torch
    h = check_h(h)
    if not (math.isfinite(float(ceiling)) and float(ceiling) > 0.0):
        raise ValueError(f"the ceiling must be positive and finite, got {ceiling}")
    if not e.is_cuda or e.dtype != torch.float32 or e.dim() != 1:
        raise TypeError("the envelope must be a float32 device tensor (n,)")
    on_device = torch.is_tensor(G)
    if on_device and (G.dtype != torch.float64 or G.device != e.device):
        raise TypeError("a device G must be a float64 tensor on the envelope's device")
    e = e.contiguous()
    g = torch.empty_like(e)
    w = window_gpu(h, e.device)
    with torch.cuda.device(e.device):
        _lib.check(_lib.lib().svs_limiter_curve(e.data_ptr(), e.numel(), math.nan if on_device else float(G), G.data_ptr() if on_device else None,
                                                float(ceiling), w.data_ptr(), h, g.data_ptr(), _lib.stream_ptr(e.device)), "svs_limiter_curve")
    return g


def apply_gpu(x, g):
    """x[..., i] *= g[i] in place (svs_limiter_apply).  x: float32 device tensor (n,) or (rows, n) with unit stride along n and one
    stride between its rows; returns x."""
    import torch
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() not in (1, 2):
        raise TypeError("x must be a float32 device tensor (n,) or (rows, n)")
    n = x.shape[-1]
    if g.dtype != torch.float32 or g.device != x.device or g.shape != (n,) or (n > 1 and (g.stride(0) != 1 or x.stride(-1) != 1)):
        raise ValueError(f"g must be a contiguous float32 tensor ({n},) on x's device, and x contiguous along its last axis")
    rows = x.shape[0] if x.dim() == 2 else 1
    ld_row = x.stride(0) if x.dim() == 2 and rows > 1 else max(n, 1)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().svs_limiter_apply(x.data_ptr(), rows, n, ld_row, g.data_ptr(), _lib.stream_ptr(x.device)), "svs_limiter_apply")
    return x


def limit_rows_gpu(buf, frames, G_dev, ceiling, rate, ms, true_peak: bool = False):
    """The three stages on buf[:, :, :frames] IN PLACE.  buf: (stems, channels, width) float32, contiguous; G_dev: the unlimited gain,
    a number or a float64 device tensor whose first element holds it; ms: the half-width in milliseconds at `rate`.  true_peak: the
    envelope follows the over-sampled signal.  The curve aims at inner_ceiling(ceiling).  Returns the gain curve, a float32 device tensor (frames,); nothing waits for the host."""
    import torch
    h = half_width(rate, ms)
    if buf.dim() != 3 or buf.dtype != torch.float32 or not buf.is_contiguous():
        raise ValueError("buf must be a contiguous float32 device tensor (stems, channels, width)")
    nst, channels, width = buf.shape
    frames = int(frames)
    if not 1 <= frames <= width:
        raise ValueError(f"frames must be in 1..{width}, got {frames}")
    factor = ld.true_peak_factor(rate) if true_peak else 1
    e = envelope_rows_gpu(buf.data_ptr(), nst, channels, frames, channels * width, width, factor, buf.device)
    g = curve_gpu(e, G_dev, inner_ceiling(ceiling), h)
    apply_gpu(buf.view(nst * channels, width)[:, :frames], g)
    return g


def describe(reduction_db: float, loudness: float) -> str:
    """The limiter's part of a command's loudness line, from the two numbers of separate_to_wav's report["limiter"]."""
    return f"limiter: deepest reduction {reduction_db:.2f} dB, written {loudness:.2f} LUFS"
