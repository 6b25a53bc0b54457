"""Integrated loudness after ITU-R BS.1770-4 / EBU R 128, in LUFS: the float64 definition (numpy, scipy.signal.lfilter) and the
device path on csrc/loudness.hip (include/svs_hip.h).  The reference has no meter: it peak-normalises every written stem to 0.9 on
its own (data.py:162-166), which loses the balance between a vocal and an accompaniment file.  With a loudness target, one gain
serves every stem of a file.

    python -m svs_unet_pytorch_amd.loudness --src FILE|FOLDER [--device gpu|cpu]

prints the integrated loudness of every wav file, at the file's own rate; with --r128 the five numbers of an EBU R 128 meter:
integrated loudness I, loudness range LRA (EBU Tech 3342), maximum momentary (400 ms) and short-term (3 s) loudness (Tech 3341) and
maximum true peak in dBTP (window_energies_reference, loudness_range, true_peak_reference; csrc/r128.hip on the device), and with
--series_csv FILE the momentary and short-term loudness of every window.

K-weighting at rate fs: two biquads from their analog prototypes by the bilinear transform, with the constants that reproduce the
standard's 48 kHz table (k_weighting).  Blocks are 400 ms at 75 % overlap in integer arithmetic: e_k = floor(k fs / 10), block j
covers [e_j, e_j+4), and the blocks that are complete count: nblocks = max(0, floor((10 n + 9) / fs) - 3), the largest k with
e_k <= n less 3, which is max(0, floor(10 n / fs) - 3) whenever 10 divides fs; z_j = sum_c mean(y_c[e_j:e_j+4]^2) with every channel's weight 1 and
l_j = -0.691 + 10 log10 z_j.  Gating: keep l_j > -70; Gamma = -0.691 + 10 log10(mean z of those) - 10; keep those above both;
L = -0.691 + 10 log10(mean z of the kept), -inf when nothing is kept.

Gain rule: g = min(10^((target - L) / 20), ceiling / peak), peak the largest |sample| of everything that receives g.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib

ABSOLUTE_GATE = -70.0
RELATIVE_GATE = -10.0
OFFSET = -0.691
FS_MIN, FS_MAX = 4000, 768000                  # csrc/loudness.hip: LD_FS_MIN, LD_FS_MAX


def _check_fs(fs):
    if int(fs) != fs or not FS_MIN <= int(fs) <= FS_MAX:
        raise ValueError(f"fs must be a whole number in {FS_MIN}..{FS_MAX}, got {fs}")
    return int(fs)


def k_weighting(fs):
    """((b, a) of the shelf, (b, a) of the high-pass), a[0] = 1, as float64 lists.  math.tan / math.pow and this order of
    operations are what svs_loudness_coeffs evaluates, bit for bit."""
    fs = float(_check_fs(fs))
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    shelf = ([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0],
             [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    highpass = ([1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return shelf, highpass


def coeffs(fs):
    """The ten numbers of svs_loudness_coeffs: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2."""
    (b1, a1), (b2, a2) = k_weighting(fs)
    return b1 + a1[1:] + b2 + a2[1:]


def edge(k: int, fs: int) -> int:
    return int(k) * int(fs) // 10


def nblocks(n: int, fs: int) -> int:
    """Blocks with e_j+4 <= n (an incomplete last block is dropped)."""
    return max(0, (10 * int(n) + 9) // int(fs) - 3)


def _lufs(z):
    """-0.691 + 10 log10 z, -inf at z = 0, without warnings."""
    z = np.asarray(z, dtype=np.float64)
    out = np.full(z.shape, -np.inf)
    np.log10(z, out=out, where=z > 0)
    return np.where(z > 0, OFFSET + 10.0 * out, -np.inf)


def gate(z):
    """(L, keep-mask of the absolute gate, keep-mask of both gates) of block energies z."""
    z = np.asarray(z, dtype=np.float64)
    l = _lufs(z)
    first = l > ABSOLUTE_GATE
    if not first.any():
        return -math.inf, first, first.copy()
    gamma = float(_lufs(z[first].mean())) + RELATIVE_GATE
    kept = first & (l > gamma)
    if not kept.any():
        return -math.inf, first, kept
    return float(_lufs(z[kept].mean())), first, kept


def loudness_reference(x, fs, stems=None):
    """(L, z, keep-mask of the absolute gate, keep-mask of both gates) in float64.  x: (n,) or (channels, n); with stems = k,
    (k, n) or (k, channels, n), measured as the sample-wise sum of the k stems."""
    z = window_energies_reference(x, fs, BINS_M, stems)
    L, first, kept = gate(z)
    return L, z, first, kept


# ------------------------------------------------------------------------------------------------
# the rest of the R 128 meter: momentary and short-term series, loudness range, true peak (float64)
# ------------------------------------------------------------------------------------------------
BINS_M, BINS_S = 4, 30                         # 400 ms and 3 s in 100 ms bins (EBU Tech 3341); csrc/loudness.hip: LD_BINS_M, LD_BINS_S
BINS_MAX = 600
LRA_RELATIVE_GATE = -20.0                      # EBU Tech 3342
LRA_LOW, LRA_HIGH = 0.10, 0.95


def nwindows(n: int, fs: int, w: int) -> int:
    """Windows of w bins with e_j+w <= n; nwindows(n, fs, 4) is nblocks(n, fs)."""
    return max(0, (10 * int(n) + 9) // int(fs) - (int(w) - 1))


def window_energies_reference(x, fs, w, stems=None):
    """z_j = sum_c mean(y_c[e_j:e_j+w]^2) in float64 for every complete window of w 100 ms bins, y the K-weighted signal; x and
    stems as loudness_reference takes them.  w = 4 gives loudness_reference's z, w = 30 the short-term series."""
    from scipy.signal import lfilter
    fs = _check_fs(fs)
    if int(w) != w or not 1 <= int(w) <= BINS_MAX:
        raise ValueError(f"w must be a whole number of bins in 1..{BINS_MAX}, got {w}")
    w = int(w)
    x = np.asarray(x, dtype=np.float64)
    if stems is not None:
        if x.shape[0] != stems:
            raise ValueError(f"stems={stems}: the first axis must have that length, got {x.shape}")
        x = x.sum(axis=0)
    x = x[None] if x.ndim == 1 else x
    if x.ndim != 2:
        raise ValueError(f"the signal must be (n,) or (channels, n), got {x.shape}")
    nw = nwindows(x.shape[1], fs, w)
    z = np.zeros(nw)
    if nw:
        (b1, a1), (b2, a2) = k_weighting(fs)
        y = lfilter(b2, a2, lfilter(b1, a1, x, axis=1), axis=1)
        y2 = y * y
        for j in range(nw):
            z[j] = y2[:, edge(j, fs):edge(j + w, fs)].mean(axis=1).sum()
    return z


def max_loudness(z) -> float:
    """max_j l_j of a series of window energies, -inf for an empty one."""
    z = np.asarray(z, dtype=np.float64)
    return float(_lufs(z).max()) if z.size else -math.inf


def loudness_range(z_s):
    """(LRA, l_lo, l_hi, kept, z_lo, z_hi) of short-term energies after EBU Tech 3342's reference code: keep l_j > -70; Gamma =
    l(mean z of those) - 20; keep those above Gamma as well, sorted ascending k[0..n); z_lo = k[floor((n-1) 0.10 + 0.5)], z_hi =
    k[floor((n-1) 0.95 + 0.5)] (nearest rank, no interpolation); LRA = l(z_hi) - l(z_lo).  n = 0: (0, -inf, -inf, 0, 0, 0)."""
    z = np.asarray(z_s, dtype=np.float64)
    l = _lufs(z)
    first = l > ABSOLUTE_GATE
    if first.any():
        gamma = float(_lufs(z[first].mean())) + LRA_RELATIVE_GATE
        k = np.sort(z[first & (l > gamma)])
    else:
        k = z[:0]
    n = int(k.size)
    if n == 0:
        return 0.0, -math.inf, -math.inf, 0, 0.0, 0.0
    z_lo = float(k[int(math.floor((n - 1) * LRA_LOW + 0.5))])
    z_hi = float(k[int(math.floor((n - 1) * LRA_HIGH + 0.5))])
    l_lo, l_hi = float(_lufs(z_lo)), float(_lufs(z_hi))
    return l_hi - l_lo, l_lo, l_hi, n, z_lo, z_hi


def true_peak_factor(fs) -> int:
    """Over-sampling factor of the true-peak meter: 4 below 96 kHz, 2 below 192 kHz, 1 from there."""
    fs = _check_fs(fs)
    return 4 if fs < 96000 else (2 if fs < 192000 else 1)


def true_peak_taps(f: int) -> np.ndarray:
    """The 12 f + 1 float64 taps of the interpolator, h[t] = sinc((t - 6 f) / f) kaiser(12 f + 1, 5)[t], with the taps at the
    multiples of f exactly 0 and the centre exactly 1: phase 0 is the sample itself.  (BS.1770-4 Annex 2's table is an example,
    not a requirement; this is the project's own filter, the window of resample.design_lowpass.)"""
    if f not in (1, 2, 4):
        raise ValueError(f"the over-sampling factor must be 1, 2 or 4, got {f}")
    n = 12 * f + 1
    t = np.arange(n, dtype=np.float64)
    h = np.sinc((t - 6 * f) / f) * np.kaiser(n, 5.0)
    h[::f] = 0.0
    h[6 * f] = 1.0
    return h


def true_peak_reference(x, fs=None, *, taps=None, factor=None):
    """(sample peaks, true peaks) per row in float64.  x: (n,) or (rows, n); zero outside [0, n).  For p = 1 .. f-1 and 0 <= i < n,
    y[f i + p] = sum_{k=0..11} h[p + f k] x[i + 6 - k]; true peak = max(max |x|, max |y|).  f and h come from fs
    (true_peak_factor, true_peak_taps) unless factor / taps are given (a test hands over the float32-rounded taps of the device)."""
    f = true_peak_factor(fs) if factor is None else int(factor)
    h = true_peak_taps(f) if taps is None else np.asarray(taps, dtype=np.float64)
    if h.shape != (12 * f + 1,):
        raise ValueError(f"factor {f} takes {12 * f + 1} taps, got {h.shape}")
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    x = x[None] if one else x
    if x.ndim != 2:
        raise ValueError(f"the signal must be (n,) or (rows, n), got {x.shape}")
    n = x.shape[1]
    sample = np.abs(x).max(axis=1) if n else np.zeros(x.shape[0])
    true = sample.copy()
    if n:
        xp = np.pad(x, ((0, 0), (6, 6)))                           # xp[i + 6] = x[i]
        for p in range(1, f):
            y = np.zeros_like(x)
            for k in range(12):
                y += h[p + f * k] * xp[:, 12 - k:12 - k + n]
            true = np.maximum(true, np.abs(y).max(axis=1))
    return (sample[0], true[0]) if one else (sample, true)


def _dbfs(v) -> float:
    return 20.0 * math.log10(v) if v > 0 else -math.inf


def meter_reference(x, fs, stems=None):
    """The five numbers of EBU R 128 in float64: {"I", "LRA", "max_M", "max_S", "max_dBTP"} (the largest true peak over the
    channels), with the series "z_m" and "z_s" they were read from."""
    z_m = window_energies_reference(x, fs, BINS_M, stems)
    z_s = window_energies_reference(x, fs, BINS_S, stems)
    x = np.asarray(x, dtype=np.float64)
    if stems is not None:
        x = x.sum(axis=0)
    _, true = true_peak_reference(x[None] if x.ndim == 1 else x, fs)
    return {"I": gate(z_m)[0], "LRA": loudness_range(z_s)[0], "max_M": max_loudness(z_m), "max_S": max_loudness(z_s),
            "max_dBTP": _dbfs(float(true.max())), "z_m": z_m, "z_s": z_s}


def gain_rule(L, peak, target, ceiling=0.9):
    """(gain, unlimited gain, limited) of the rule above in float64; L = -inf leaves the peak rule alone, and silence with nothing
    to aim at keeps gain 1."""
    unlimited = math.inf if L == -math.inf else 10.0 ** ((float(target) - float(L)) / 20.0)
    cap = float(ceiling) / float(peak) if peak > 0 else math.inf
    g = min(unlimited, cap)
    return (g if g < math.inf else 1.0), unlimited, cap < unlimited


# ------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------
def _planar(x, stems: int):
    """(stems, channels, n, ld_stem, ld_ch) of a float32 device tensor (n,), (channels, n) or, for stems = 2, (2, channels, n),
    whose samples are contiguous along the last axis."""
    import torch
    if not x.is_cuda:
        raise ValueError("the device path needs a device tensor (loudness_reference is the host path)")
    if x.dtype != torch.float32:
        raise TypeError(f"dtype {x.dtype} (float32)")
    if stems not in (1, 2):
        raise ValueError(f"stems must be 1 or 2, got {stems}")
    want = 3 if stems == 2 else 2
    if x.dim() == want - 1:
        x = x.unsqueeze(-2)
    if x.dim() != want or (stems == 2 and x.shape[0] != 2):
        raise ValueError(f"stems={stems}: the signal must be {'(2, channels, n)' if stems == 2 else '(n,) or (channels, n)'}, got {tuple(x.shape)}")
    if x.shape[-1] > 1 and x.stride(-1) != 1:
        x = x.contiguous()
    channels, n = x.shape[-2], x.shape[-1]
    ld_ch = x.stride(-2) if channels > 1 else max(n, 1)
    ld_stem = x.stride(0) if stems == 2 else 0
    return x, channels, n, ld_stem, ld_ch


def block_energies_gpu(x, fs, stems: int = 1):
    """z_j of svs_loudness_blocks as a float64 device tensor (nblocks,)."""
    import torch
    fs = _check_fs(fs)
    x, channels, n, ld_stem, ld_ch = _planar(x, stems)
    L = _lib.lib()
    nb = int(L.svs_loudness_nblocks(n, fs))
    nbytes = int(L.svs_loudness_workspace_bytes(n, channels, fs))
    if nb < 0 or nbytes == 0:
        raise _lib.SvsError(f"svs_loudness_workspace_bytes({n}, {channels}, {fs}): invalid arguments")
    z = torch.empty(nb, dtype=torch.float64, device=x.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.svs_loudness_blocks(x.data_ptr(), stems, channels, n, ld_stem, ld_ch, fs, z.data_ptr(), ws.data_ptr(), nbytes,
                                         _lib.stream_ptr(x.device)), "svs_loudness_blocks")
    return z


def loudness_gain_gpu(x, fs, target=None, *, ceiling: float = 0.9, stems: int = 1, peaks=None, channels: int | None = None):
    """(gain, info) on the device, nothing waits for the host.  info: 4 doubles, L, kept blocks, unlimited gain, 1 when the ceiling
    limited it.  target: LUFS as a number, a device float64 tensor whose first element holds it (another call's info), or None
    to measure only (gain is then None).  peaks: float32 device tensor of the maxima the ceiling is held against (None: no
    ceiling).  gain: float32 (channels,), all equal, as svs_resample_encode takes it."""
    z = block_energies_gpu(x, fs, stems)
    if channels is None:
        channels = x.shape[-2] if x.dim() > 1 else 1
    return gain_from_blocks_gpu(z, target, ceiling=ceiling, peaks=peaks, channels=channels)


def gain_from_blocks_gpu(z, target=None, *, ceiling: float = 0.9, peaks=None, channels: int = 1):
    """loudness_gain_gpu's (gain, info) from block energies that are there already (block_energies_gpu's z): svs_loudness_gain alone.
    The limiter's way out calls it twice on one z, without peaks for the unlimited gain and with the limited rows' peaks for the
    written one."""
    import torch
    dev = z.device
    info = torch.empty(4, dtype=torch.float64, device=dev)
    on_device = torch.is_tensor(target)
    if on_device and (target.dtype != torch.float64 or target.device != dev):
        raise TypeError("a device target must be a float64 tensor on the signal's device")
    gain = None if target is None else torch.empty(channels, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().svs_loudness_gain(z.data_ptr(), z.numel(), _lib.ptr(peaks), 0 if peaks is None else peaks.numel(),
                                                math.nan if (target is None or on_device) else float(target),
                                                target.data_ptr() if on_device else None, float(ceiling), _lib.ptr(gain),
                                                0 if gain is None else channels, info.data_ptr(), _lib.stream_ptr(dev)),
                   "svs_loudness_gain")
    return gain, info


def integrated_loudness_gpu(x, fs, stems: int = 1) -> float:
    """Integrated loudness in LUFS of a float32 device signal (n,), (channels, n) or, with stems = 2, the sum of (2, channels, n)."""
    return float(loudness_gain_gpu(x, fs, None, stems=stems)[1][0].item())


def series_gpu(x, fs, stems: int = 1):
    """(z_m, z_s) of svs_loudness_series as float64 device tensors: the 400 ms and the 3 s window energies from one run of the
    K-weighting passes; z_m is bit for bit block_energies_gpu's z."""
    import torch
    fs = _check_fs(fs)
    x, channels, n, ld_stem, ld_ch = _planar(x, stems)
    L = _lib.lib()
    n_m, n_s = int(L.svs_loudness_nwindows(n, fs, BINS_M)), int(L.svs_loudness_nwindows(n, fs, BINS_S))
    nbytes = int(L.svs_loudness_workspace_bytes(n, channels, fs))
    if n_m < 0 or n_s < 0 or nbytes == 0:
        raise _lib.SvsError(f"svs_loudness_workspace_bytes({n}, {channels}, {fs}): invalid arguments")
    z_m = torch.empty(n_m, dtype=torch.float64, device=x.device)
    z_s = torch.empty(n_s, dtype=torch.float64, device=x.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.svs_loudness_series(x.data_ptr(), stems, channels, n, ld_stem, ld_ch, fs, z_m.data_ptr(), z_s.data_ptr(), ws.data_ptr(),
                                         nbytes, _lib.stream_ptr(x.device)), "svs_loudness_series")
    return z_m, z_s


def stats_gpu(z_m, z_s):
    """svs_loudness_stats of two float64 device series: 8 device doubles, max M, max S, LRA, kept windows, l_lo, l_hi, z_lo, z_hi."""
    import torch
    dev = z_s.device
    L = _lib.lib()
    nbytes = int(L.svs_loudness_stats_workspace_bytes(z_s.numel()))
    if nbytes == 0:
        raise _lib.SvsError(f"svs_loudness_stats_workspace_bytes({z_s.numel()}): invalid arguments")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stats = torch.empty(8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.svs_loudness_stats(z_m.data_ptr() if z_m.numel() else None, z_m.numel(), z_s.data_ptr() if z_s.numel() else None,
                                        z_s.numel(), stats.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr(dev)), "svs_loudness_stats")
    return stats


_TP_TAPS: dict = {}


def true_peak_taps_gpu(f: int, device):
    """true_peak_taps(f) rounded to float32 on `device`, built once per device."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(f), str(device))
    if key not in _TP_TAPS:
        _TP_TAPS[key] = torch.from_numpy(true_peak_taps(f).astype(np.float32)).to(device)
    return _TP_TAPS[key]


def true_peaks_rows_gpu(x_ptr, stems, channels, n, ld_stem, ld_ch, factor, device, *, sample=True):
    """svs_true_peaks on rows given by address: (sample peaks or None, true peaks), float32 device tensors (stems * channels,)."""
    import torch
    L = _lib.lib()
    rows = stems * channels
    nbytes = int(L.svs_true_peaks_workspace_bytes(n, rows))
    if nbytes == 0:
        raise _lib.SvsError(f"svs_true_peaks_workspace_bytes({n}, {rows}): invalid arguments")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    sp = torch.empty(rows, dtype=torch.float32, device=device) if sample else None
    tp = torch.empty(rows, dtype=torch.float32, device=device)
    taps = true_peak_taps_gpu(factor, device)
    with torch.cuda.device(device):
        _lib.check(L.svs_true_peaks(x_ptr, stems, channels, n, ld_stem, ld_ch, taps.data_ptr(), factor, _lib.ptr(sp), tp.data_ptr(),
                                    ws.data_ptr(), nbytes, _lib.stream_ptr(device)), "svs_true_peaks")
    return sp, tp


def true_peaks_gpu(x, fs, stems: int = 1, *, factor: int | None = None):
    """(sample peaks, true peaks) of a float32 device signal (n,), (channels, n) or, with stems = 2, (2, channels, n): two float32
    device tensors with one value per row (the stems are not added).  factor: true_peak_factor(fs) unless given."""
    factor = true_peak_factor(fs) if factor is None else int(factor)
    x, channels, n, ld_stem, ld_ch = _planar(x, stems)
    return true_peaks_rows_gpu(x.data_ptr(), stems, channels, n, ld_stem if stems > 1 else channels * ld_ch, ld_ch, factor, x.device)


def meter_gpu(x, fs, stems: int = 1, *, return_series: bool = False):
    """The R 128 meter on the device, nothing waits for the host: (info, stats, true peaks).  info: loudness_gain_gpu's 4 doubles (I
    first); stats: stats_gpu's 8 doubles; true peaks: float32, one per row.  meter_values reads them back at once.  return_series:
    also (z_m, z_s), the device series they were read from, as a fourth value."""
    import torch
    z_m, z_s = series_gpu(x, fs, stems)
    dev = z_m.device
    info = torch.empty(4, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().svs_loudness_gain(z_m.data_ptr() if z_m.numel() else None, z_m.numel(), None, 0, math.nan, None, 0.9, None, 0,
                                                info.data_ptr(), _lib.stream_ptr(dev)), "svs_loudness_gain")
    out = (info, stats_gpu(z_m, z_s), true_peaks_gpu(x, fs, stems)[1])
    return (*out, (z_m, z_s)) if return_series else out


def meter_values(info, stats, true_peaks) -> dict:
    """meter_gpu's device results as meter_reference's five numbers, with ONE read-back."""
    import torch
    v = torch.cat([info[:1], stats[:3], true_peaks.max().to(torch.float64)[None]]).cpu().tolist()
    return {"I": v[0], "max_M": v[1], "max_S": v[2], "LRA": v[3], "max_dBTP": _dbfs(v[4])}


def describe(info, gain=None, true_peak: bool = False) -> str:
    """One line for a command's output from the four numbers of info and the applied gain (already on the host).  true_peak: the
    ceiling was held against the true peaks."""
    L, _, _, limited = (float(v) for v in info)
    text = f"{L:.2f} LUFS"
    if gain is not None and gain > 0:
        which = "true-peak" if true_peak else "peak"
        text += f", gain {20.0 * math.log10(float(gain)):+.2f} dB" + (f" (limited by the {which} ceiling)" if limited else "")
    return text


def parse_target(value: str):
    """--loudness: a number of LUFS, or "source"."""
    if value == "source":
        return value
    try:
        v = float(value)
    except ValueError:
        v = math.nan
    if not math.isfinite(v):
        raise ValueError(f"{value!r}: a number of LUFS (for instance -23) or `source`")
    return v


def file_loudness(path: str, device=None) -> float:
    """Integrated loudness of a wav file at its own rate; device None: the float64 reference on the host."""
    from .data import read_pcm
    rate, data, channels = read_pcm(path)
    if device is None:
        if data.dtype.kind == "i":
            data = data.astype(np.float64) / float(np.iinfo(data.dtype).max + 1)
        return loudness_reference(data.T if data.ndim == 2 else data, rate)[0]
    import torch
    from .resample import resample_poly_gpu
    pcm = torch.from_numpy(data).to(device)
    return integrated_loudness_gpu(resample_poly_gpu(pcm, 1, 1, channels=channels, downmix=False), rate)


def file_meter(path: str, device=None, series: bool = False) -> dict:
    """The five numbers of EBU R 128 of a wav file at its own rate: {"I", "LRA", "max_M", "max_S", "max_dBTP"}; device None: the
    float64 reference on the host.  series: also "l_m" and "l_s", the momentary and short-term loudness of every window (numpy)."""
    from .data import read_pcm
    rate, data, channels = read_pcm(path)
    if device is None:
        if data.dtype.kind == "i":
            data = data.astype(np.float64) / float(np.iinfo(data.dtype).max + 1)
        out = meter_reference(data.T if data.ndim == 2 else data, rate)
        z_m, z_s = out.pop("z_m"), out.pop("z_s")
    else:
        import torch
        from .resample import resample_poly_gpu
        x = resample_poly_gpu(torch.from_numpy(data).to(device), 1, 1, channels=channels, downmix=False)
        *measured, (z_m, z_s) = meter_gpu(x, rate, return_series=True)
        out = meter_values(*measured)
        if series:
            z_m, z_s = z_m.cpu().numpy(), z_s.cpu().numpy()
    if series:
        out["l_m"], out["l_s"] = _lufs(z_m), _lufs(z_s)
    return out


def write_series_csv(handle, path: str, l_m, l_s):
    """One row per 400 ms window: the file, the time at which the window ends in seconds, M, and S once 3 s have passed."""
    for j, m in enumerate(l_m):
        k = j - (BINS_S - BINS_M)                                  # the short-term window that ends with momentary window j
        s = f"{l_s[k]:.3f}" if 0 <= k < len(l_s) else ""
        handle.write(f"{path},{(j + BINS_M) / 10.0:.1f},{m:.3f},{s}\n")


def main(argv=None):
    import argparse
    import os
    import sys
    parser = argparse.ArgumentParser(description="integrated loudness (ITU-R BS.1770-4) of wav files, in LUFS; --r128: the EBU R 128 meter")
    parser.add_argument("--src", type=str, required=True, help="a wav file, or a folder of *.wav files")
    parser.add_argument("--device", default="gpu", choices=["gpu", "cpu"], help="gpu: csrc/loudness.hip, csrc/r128.hip; cpu: the float64 definition")
    parser.add_argument("--r128", action="store_true",
                        help="print integrated loudness, loudness range, maximum momentary and short-term loudness and maximum true peak")
    parser.add_argument("--series_csv", type=str, default=None, help="with --r128: write file, time, M and S of every window to this csv file")
    args = parser.parse_args(argv)
    if args.series_csv is not None and not args.r128:
        parser.error("--series_csv belongs to --r128")
    device = None
    if args.device == "gpu":
        import torch
        if not torch.cuda.is_available():
            print("--device gpu needs a ROCm device (hand-written gfx950 kernels); --device cpu runs the float64 definition.")
            sys.exit(1)
        device = torch.device("cuda")
    paths = [os.path.join(args.src, f) for f in sorted(os.listdir(args.src)) if f.endswith(".wav")] if os.path.isdir(args.src) else [args.src]
    if not args.r128:
        for path in paths:
            print(f"{path}: {file_loudness(path, device):.2f} LUFS")
        return
    csv = open(args.series_csv, "w") if args.series_csv is not None else None
    try:
        if csv is not None:
            csv.write("file,time_s,momentary_lufs,short_term_lufs\n")
        for path in paths:
            m = file_meter(path, device, series=csv is not None)
            print(f"{path}: I {m['I']:.2f} LUFS, LRA {m['LRA']:.2f} LU, max M {m['max_M']:.2f} LUFS, max S {m['max_S']:.2f} LUFS, "
                  f"max TP {m['max_dBTP']:.2f} dBTP")
            if csv is not None:
                write_series_csv(csv, path, m["l_m"], m["l_s"])
    finally:
        if csv is not None:
            csv.close()


if __name__ == "__main__":
    main()
