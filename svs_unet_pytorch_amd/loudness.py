"""Integrated loudness after ITU-R BS.1770-4 / EBU R 128, in LUFS: the float64 definition (numpy, scipy.signal.lfilter) and the
device path on csrc/loudness.hip (include/svs_hip.h).  The reference has no meter: it peak-normalises every written stem to 0.9 on
its own (data.py:162-166), which loses the balance between a vocal and an accompaniment file.  With a loudness target, one gain
serves every stem of a file.

    python -m svs_unet_pytorch_amd.loudness --src FILE|FOLDER [--device gpu|cpu]

prints the integrated loudness of every wav file, at the file's own rate.

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
    from scipy.signal import lfilter
    fs = _check_fs(fs)
    x = np.asarray(x, dtype=np.float64)
    if stems is not None:
        if x.shape[0] != stems:
            raise ValueError(f"stems={stems}: the first axis must have that length, got {x.shape}")
        x = x.sum(axis=0)
    x = x[None] if x.ndim == 1 else x
    if x.ndim != 2:
        raise ValueError(f"the signal must be (n,) or (channels, n), got {x.shape}")
    n = x.shape[1]
    nb = nblocks(n, fs)
    z = np.zeros(nb)
    if nb:
        (b1, a1), (b2, a2) = k_weighting(fs)
        y = lfilter(b2, a2, lfilter(b1, a1, x, axis=1), axis=1)
        y2 = y * y
        for j in range(nb):
            z[j] = y2[:, edge(j, fs):edge(j + 4, fs)].mean(axis=1).sum()
    L, first, kept = gate(z)
    return L, z, first, kept


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
    import torch
    z = block_energies_gpu(x, fs, stems)
    if channels is None:
        channels = x.shape[-2] if x.dim() > 1 else 1
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


def describe(info, gain=None) -> str:
    """One line for a command's output from the four numbers of info and the applied gain (already on the host)."""
    L, _, _, limited = (float(v) for v in info)
    text = f"{L:.2f} LUFS"
    if gain is not None and gain > 0:
        text += f", gain {20.0 * math.log10(float(gain)):+.2f} dB" + (" (limited by the peak ceiling)" if limited else "")
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


def main(argv=None):
    import argparse
    import os
    import sys
    parser = argparse.ArgumentParser(description="integrated loudness (ITU-R BS.1770-4) of wav files, in LUFS")
    parser.add_argument("--src", type=str, required=True, help="a wav file, or a folder of *.wav files")
    parser.add_argument("--device", default="gpu", choices=["gpu", "cpu"], help="gpu: csrc/loudness.hip; cpu: the float64 definition")
    args = parser.parse_args(argv)
    device = None
    if args.device == "gpu":
        import torch
        if not torch.cuda.is_available():
            print("--device gpu needs a ROCm device (hand-written gfx950 kernels); --device cpu runs the float64 definition.")
            sys.exit(1)
        device = torch.device("cuda")
    paths = [os.path.join(args.src, f) for f in sorted(os.listdir(args.src)) if f.endswith(".wav")] if os.path.isdir(args.src) else [args.src]
    for path in paths:
        print(f"{path}: {file_loudness(path, device):.2f} LUFS")


if __name__ == "__main__":
    main()
