"""Fundamental frequency of a (separated) voice: the YIN tracker, steps 1 to 5 of de Cheveigne & Kawahara (JASA 2002) -- the float64
definition (numpy), the device path on csrc/f0.hip (include/svs_hip.h), the frame-level melody measures of the
MIREX melody task, and a command line.  The reference has no pitch estimator; pitch.py / csrc/pitch.hip SHIFT pitch for training.

    python -m svs_unet_pytorch_amd.f0 --src song.wav|folder --csv out.csv|folder [--fmin 65] [--fmax 1000] [--window W] [--hop H] \
        [--threshold 0.15] [--rms_gate_db DB] [--device gpu|cpu]

Geometry, from sr, fmin, fmax, W (the integration window in samples, default 2 tau_max), hop (default round(sr / 100), at least 1):
    tau_min = max(2, floor(sr / fmax)),  tau_max = ceil(sr / fmin),  span = W + tau_max,  frames = 1 + (n - span) // hop
Only whole frames are formed, nothing is zero-padded, and n < span is an error.  Limits (the kernel's, checked before any launch):
1 <= W <= 4096, tau_min < tau_max <= 2048, hop >= 1, 1 <= rows <= 64.

Frame i of a row starts at sample t = i hop:
    d(tau)  = sum_{j=0..W-1} (float64(float32(x[t+j] - x[t+j+tau])))^2,  tau = 0..tau_max     (the difference is ONE float32 subtraction)
    S(tau)  = sum_{k=1..tau} d(k)
    d'(0)   = 1;  d'(tau) = d(tau) tau / S(tau), 1 where S(tau) == 0; stored as float32
    pick (on the float32 d'): the smallest tau in [tau_min, tau_max] with float64(d'(tau)) < threshold, then tau + 1 while that is in
            range and d'(tau+1) < d'(tau); none under the threshold: the smallest tau that attains the minimum of d', found = 0
    delta   = clamp(0.5 (a - c) / (a - 2b + c), -1, 1) with a, b, c = d'(tau-1), d'(tau), d'(tau+1) in float64, where tau - 1 >= 1,
              tau + 1 <= tau_max and a - 2b + c > 0; else 0
    f0 = float32(sr / (tau + delta));  ap = b;  rms = float32(sqrt(mean of the frame's first W samples squared, in float64))
    voiced = found and rms >= rms_gate;  the frame's time is (t + span / 2) / sr
There is no step 6 of the paper (the best local estimate), no smoothing over frames and no octave-error correction.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from . import _lib

FMIN, FMAX, THRESHOLD = 65.0, 1000.0, 0.15
W_MAX, TAU_MAX, ROWS_MAX = 4096, 2048, 64                            # csrc/f0.hip: F0_MAX_W, F0_MAX_TAU, F0_MAX_ROWS
MELODY_GATE_DB = -50.0                                               # evaluate.py --melody: silent reference passages count as unvoiced
CENTS = 50.0
MELODY = ("VR", "VFA", "RPA", "RCA", "OA")


class Geometry(NamedTuple):
    sr: float
    tau_min: int
    tau_max: int
    W: int
    hop: int
    span: int
    threshold: float
    rms_gate: float


class Track(NamedTuple):
    """Per frame (numpy arrays from yin_reference, device tensors from track_gpu), (frames,) or (rows, frames): the frame's time in
    seconds (always (frames,)), f0 in Hz (float32), voiced (int32), the aperiodicity d'(tau) (float32) and the frame's rms (float32)."""
    time: object
    f0: object
    voiced: object
    ap: object
    rms: object


def geometry(sr, fmin=FMIN, fmax=FMAX, W=None, hop=None, threshold=THRESHOLD, rms_gate=0.0) -> Geometry:
    """The derived values above; every rule is a ValueError with a message of its own, before any device work."""
    sr, fmin, fmax = float(sr), float(fmin), float(fmax)
    if not (math.isfinite(sr) and sr > 0.0):
        raise ValueError(f"sr must be a positive rate in Hz, got {sr}")
    if not (math.isfinite(fmin) and fmin > 0.0 and math.isfinite(fmax) and fmax > 0.0):
        raise ValueError(f"fmin and fmax must be positive frequencies in Hz, got {fmin} and {fmax}")
    tau_min, tau_max = max(2, int(math.floor(sr / fmax))), int(math.ceil(sr / fmin))
    if tau_max > TAU_MAX:
        raise ValueError(f"fmin {fmin:g} Hz at {sr:g} Hz is a longest lag tau_max of {tau_max} samples; at most {TAU_MAX} "
                         f"(fmin >= {sr / TAU_MAX:.2f} Hz at this rate)")
    if not tau_min < tau_max:
        raise ValueError(f"fmin {fmin:g} Hz and fmax {fmax:g} Hz at {sr:g} Hz leave no lag range: tau_min {tau_min} must be below tau_max {tau_max}")
    W = 2 * tau_max if W is None else W
    if int(W) != W or not 1 <= int(W) <= W_MAX:
        raise ValueError(f"the window W must be a whole number of samples in 1..{W_MAX}, got {W}")
    hop = max(1, int(round(sr / 100.0))) if hop is None else hop
    if int(hop) != hop or int(hop) < 1:
        raise ValueError(f"hop must be a whole number of samples, at least 1, got {hop}")
    threshold, rms_gate = float(threshold), float(rms_gate)
    if not (math.isfinite(threshold) and threshold > 0.0):
        raise ValueError(f"the threshold must be positive and finite, got {threshold}")
    if not (math.isfinite(rms_gate) and rms_gate >= 0.0):
        raise ValueError(f"rms_gate is a linear level, finite and not negative, got {rms_gate}")
    return Geometry(sr, tau_min, tau_max, int(W), int(hop), int(W) + tau_max, threshold, rms_gate)


def check_rows(rows) -> int:
    if not 1 <= int(rows) <= ROWS_MAX:
        raise ValueError(f"rows must be in 1..{ROWS_MAX}, got {rows}")
    return int(rows)


def frame_count(n: int, span: int, hop: int) -> int:
    """1 + (n - span) // hop; n < span is a ValueError (nothing is zero-padded)."""
    if int(n) < int(span):
        raise ValueError(f"the signal has {int(n)} samples, one frame needs span = W + tau_max = {int(span)}")
    return 1 + (int(n) - int(span)) // int(hop)


def frame_range(n: int, g: Geometry, first_frame: int = 0, n_frames=None):
    """(first_frame, n_frames) checked against the signal's frame count; n_frames None: every frame from first_frame on."""
    total = frame_count(n, g.span, g.hop)
    first_frame = int(first_frame)
    n_frames = total - first_frame if n_frames is None else int(n_frames)
    if first_frame < 0 or n_frames < 0 or first_frame + n_frames > total:
        raise ValueError(f"frames {first_frame}..{first_frame + n_frames - 1} lie outside the signal's {total} frames")
    return first_frame, n_frames


def frame_times(g: Geometry, n_frames: int, first_frame: int = 0) -> np.ndarray:
    """(t + span / 2) / sr of frames first_frame .. first_frame + n_frames - 1, float64."""
    return ((first_frame + np.arange(int(n_frames), dtype=np.float64)) * g.hop + 0.5 * g.span) / g.sr


def gate_from_db(db) -> float:
    """A gate in dB re full scale as the linear rms_gate; None: off (0)."""
    return 0.0 if db is None else 10.0 ** (float(db) / 20.0)


def harmonic_tone(freq, sr, top: float = 3500.0, level: float = 0.25) -> np.ndarray:
    """A float32 test voice whose instantaneous fundamental at sample i is freq[i] Hz: level * sum_k sin(k phase) / k over the
    harmonics with k freq[i] <= top, phase the running integral of 2 pi freq / sr (trapezoids, float64)."""
    f = np.asarray(freq, dtype=np.float64)
    phase = np.concatenate([[0.0], np.cumsum(np.pi * (f[1:] + f[:-1]) / float(sr))])
    x = np.zeros(f.shape)
    for k in range(1, int(top // f.min()) + 1):
        x += np.where(k * f <= top, np.sin(k * phase) / k, 0.0)
    return (level * x).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# the float64 definition
# ------------------------------------------------------------------------------------------------
def cmnd_reference(x, W: int, tau_max: int, hop: int, first_frame: int = 0, n_frames=None):
    """(d' float32 (rows, frames, tau_max + 1), rms float32 (rows, frames)) of x: (n,) or (rows, n), taken as float32."""
    x = np.asarray(x, dtype=np.float32)
    x = x[None] if x.ndim == 1 else x.reshape(-1, x.shape[-1])
    n, span = x.shape[1], W + tau_max
    total = frame_count(n, span, hop)
    n_frames = total - first_frame if n_frames is None else n_frames
    starts = (first_frame + np.arange(n_frames)) * hop
    view = np.lib.stride_tricks.sliding_window_view
    d = np.zeros((x.shape[0], n_frames, tau_max + 1))
    rms = np.zeros((x.shape[0], n_frames), np.float32)
    for r, row in enumerate(x):
        sq = row.astype(np.float64) ** 2
        rms[r] = np.sqrt(view(sq, W)[starts].sum(axis=1) / W).astype(np.float32) if n_frames else 0
        for tau in range(1, tau_max + 1):
            diff = (row[:n - tau] - row[tau:]).astype(np.float64)    # the float32 subtraction, then exact
            d[r, :, tau] = view(diff * diff, W)[starts].sum(axis=1) if n_frames else 0
    S = np.cumsum(d[..., 1:], axis=-1)
    dp = np.ones_like(d)
    tau = np.arange(1, tau_max + 1, dtype=np.float64)
    np.divide(d[..., 1:] * tau, S, out=dp[..., 1:], where=S != 0.0)
    return dp.astype(np.float32), rms


def pick_reference(dprime, sr, tau_min: int, tau_max: int, threshold=THRESHOLD, rms=None, rms_gate=0.0):
    """The pick and the interpolation on any float32 d' buffer (..., tau_max + 1): (f0 float32, ap float32, voiced int32, tau int64),
    each of shape (...).  rms (...): voiced = found and rms >= rms_gate; None: voiced = found."""
    dp32 = np.asarray(dprime, dtype=np.float32)
    if dp32.shape[-1] != tau_max + 1:
        raise ValueError(f"d' must have tau_max + 1 = {tau_max + 1} values per frame, got {dp32.shape[-1]}")
    lead = dp32.shape[:-1]
    rows = dp32.reshape(-1, tau_max + 1)
    f0 = np.zeros(rows.shape[0], np.float32)
    ap = np.zeros(rows.shape[0], np.float32)
    found = np.zeros(rows.shape[0], bool)
    taus = np.zeros(rows.shape[0], np.int64)
    threshold = float(threshold)
    for i, dp in enumerate(rows):
        under = np.flatnonzero(dp[tau_min:tau_max + 1].astype(np.float64) < threshold)
        if under.size:
            tau = tau_min + int(under[0])
            while tau + 1 <= tau_max and dp[tau + 1] < dp[tau]:
                tau += 1
            found[i] = True
        else:
            tau = tau_min + int(np.argmin(dp[tau_min:tau_max + 1]))   # the first index that attains the minimum
        b, delta = float(dp[tau]), 0.0
        if tau - 1 >= 1 and tau + 1 <= tau_max:
            a, c = float(dp[tau - 1]), float(dp[tau + 1])
            q = a - 2.0 * b + c
            if q > 0.0:
                delta = min(1.0, max(-1.0, 0.5 * (a - c) / q))
        f0[i], ap[i], taus[i] = float(sr) / (tau + delta), dp[tau], tau
    voiced = found if rms is None else found & (np.asarray(rms, dtype=np.float32).reshape(-1) >= np.float32(rms_gate))
    return f0.reshape(lead), ap.reshape(lead), voiced.astype(np.int32).reshape(lead), taus.reshape(lead)


def yin_reference(x, sr, fmin=FMIN, fmax=FMAX, W=None, hop=None, threshold=THRESHOLD, rms_gate=0.0, first_frame: int = 0, n_frames=None):
    """The definition on x: (n,) or (rows, n).  Returns (Track, d') -- d' float32 (frames, tau_max + 1) or (rows, frames, tau_max + 1)."""
    g = geometry(sr, fmin, fmax, W, hop, threshold, rms_gate)
    x = np.asarray(x, dtype=np.float32)
    one = x.ndim == 1
    x = x[None] if one else x.reshape(-1, x.shape[-1])
    check_rows(x.shape[0])
    first_frame, n_frames = frame_range(x.shape[1], g, first_frame, n_frames)
    dp, rms = cmnd_reference(x, g.W, g.tau_max, g.hop, first_frame, n_frames)
    f0, ap, voiced, _ = pick_reference(dp, g.sr, g.tau_min, g.tau_max, g.threshold, rms, g.rms_gate)
    t = frame_times(g, n_frames, first_frame)
    if one:
        f0, ap, voiced, rms, dp = f0[0], ap[0], voiced[0], rms[0], dp[0]
    return Track(t, f0, voiced, ap, rms), dp


# ------------------------------------------------------------------------------------------------
# melody measures
# ------------------------------------------------------------------------------------------------
def melody_metrics(ref_f0, ref_voiced, est_f0, est_voiced) -> dict:
    """The five frame-level measures of the MIREX audio melody extraction task, as fractions in [0, 1], of two tracks on the same frames:
        VR   voicing recall:       the reference's voiced frames that the estimate calls voiced
        VFA  voicing false alarm:  the reference's unvoiced frames that the estimate calls voiced
        RPA  raw pitch accuracy:   the reference's voiced frames whose estimated f0 lies within 50 cents -- the larger of the two
                                   frequencies over the smaller is at most the double 2^(50/1200), the bound included -- whatever voicing
                                   the estimate reports there (the tracker gives a pitch on every frame)
        RCA  raw chroma accuracy:  the same with the difference folded into one octave (octave errors forgiven)
        OA   overall accuracy:     frames that are right altogether -- voiced in both with the pitch within 50 cents, or unvoiced in both --
                                   over all frames
    A measure over an empty set of frames (no voiced reference frame, no unvoiced one, no frame at all) is 0."""
    ref_f0, est_f0 = np.asarray(ref_f0, dtype=np.float64).reshape(-1), np.asarray(est_f0, dtype=np.float64).reshape(-1)
    rv, ev = np.asarray(ref_voiced).reshape(-1) != 0, np.asarray(est_voiced).reshape(-1) != 0
    if not ref_f0.shape == est_f0.shape == rv.shape == ev.shape:
        raise ValueError(f"the four arrays must have one value per frame, got {ref_f0.shape}, {rv.shape}, {est_f0.shape}, {ev.shape}")
    ok = rv & (ref_f0 > 0.0) & (est_f0 > 0.0) & np.isfinite(ref_f0) & np.isfinite(est_f0)
    ref, est = np.where(ok, ref_f0, 1.0), np.where(ok, est_f0, 1.0)
    octaves = np.round(np.log2(est / ref)).astype(np.int64)
    folded = np.ldexp(est, -octaves)                                  # exact: the estimate brought into the reference's octave

    def within(a, b):                                                 # larger over smaller at most 2^(50/1200), the bound included
        return ok & (np.maximum(a, b) / np.minimum(a, b) <= 2.0 ** (CENTS / 1200.0))
    pitch, fold = within(est, ref), within(folded, ref)

    def ratio(hits, among):
        return float(hits) / float(among) if among else 0.0
    n_v, n_u = int(rv.sum()), int((~rv).sum())
    return {"VR": ratio((rv & ev).sum(), n_v), "VFA": ratio((~rv & ev).sum(), n_u), "RPA": ratio((rv & pitch).sum(), n_v),
            "RCA": ratio((rv & fold).sum(), n_v), "OA": ratio((rv & ev & pitch).sum() + (~rv & ~ev).sum(), n_v + n_u)}


# ------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------
def _rows_gpu(x):
    """(x as (rows, n) with unit stride along n, rows, n, ld_row, whether a row axis was added)."""
    import torch
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError("the device path needs a device tensor (yin_reference is the host path)")
    if x.dtype != torch.float32:
        raise TypeError(f"dtype {x.dtype} (float32)")
    if x.dim() not in (1, 2):
        raise ValueError(f"the signal must be (n,) or (rows, n), got {tuple(x.shape)}")
    one = x.dim() == 1
    x = x[None] if one else x
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    rows, n = check_rows(x.shape[0]), x.shape[1]
    return x, rows, n, (x.stride(0) if rows > 1 else max(n, 1)), one


def cmnd_gpu(x, W: int, tau_max: int, hop: int, first_frame: int = 0, n_frames=None, rms: bool = True):
    """svs_f0_cmnd: (d' float32 (rows, frames, tau_max + 1), rms float32 (rows, frames) or None) of a float32 device signal (n,) or
    (rows, n); a 1-D signal gives (frames, tau_max + 1) and (frames,)."""
    import torch
    x, rows, n, ld_row, one = _rows_gpu(x)
    total = frame_count(n, W + tau_max, hop)
    n_frames = total - int(first_frame) if n_frames is None else int(n_frames)
    dp = torch.empty(rows, n_frames, tau_max + 1, dtype=torch.float32, device=x.device)
    r = torch.empty(rows, n_frames, dtype=torch.float32, device=x.device) if rms else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().svs_f0_cmnd(x.data_ptr(), rows, n, ld_row, int(W), int(tau_max), int(hop), int(first_frame), n_frames, dp.data_ptr(),
                                          _lib.ptr(r), _lib.stream_ptr(x.device)), "svs_f0_cmnd")
    return (dp[0], None if r is None else r[0]) if one else (dp, r)


def pick_gpu(dprime, sr, tau_min: int, threshold=THRESHOLD, rms=None, rms_gate=0.0):
    """svs_f0_pick on a float32 device buffer (..., tau_max + 1): (f0 float32, ap float32, voiced int32), each (...)."""
    import torch
    if not torch.is_tensor(dprime) or not dprime.is_cuda or dprime.dtype != torch.float32 or dprime.dim() < 1:
        raise TypeError("d' must be a float32 device tensor (..., tau_max + 1)")
    dprime = dprime.contiguous()
    lead, tau_max = dprime.shape[:-1], dprime.shape[-1] - 1
    count = int(np.prod(lead, dtype=np.int64))
    if rms is not None:
        if rms.dtype != torch.float32 or rms.device != dprime.device or rms.shape != lead:
            raise ValueError(f"rms must be a float32 tensor {tuple(lead)} on d's device")
        rms = rms.contiguous()
    f0 = torch.empty(lead, dtype=torch.float32, device=dprime.device)
    ap = torch.empty_like(f0)
    voiced = torch.empty(lead, dtype=torch.int32, device=dprime.device)
    with torch.cuda.device(dprime.device):
        _lib.check(_lib.lib().svs_f0_pick(dprime.data_ptr(), count, int(tau_min), tau_max, float(threshold), _lib.ptr(rms), float(rms_gate),
                                          float(sr), f0.data_ptr(), ap.data_ptr(), voiced.data_ptr(), _lib.stream_ptr(dprime.device)), "svs_f0_pick")
    return f0, ap, voiced


def track_gpu(x, sr, fmin=FMIN, fmax=FMAX, W=None, hop=None, threshold=THRESHOLD, rms_gate=0.0, first_frame: int = 0, n_frames=None) -> Track:
    """svs_f0_track, ONE launch: the Track of a float32 device signal (n,) or (rows, n) as device tensors (time: float64 (frames,)).
    The geometry's rules and the frame range are checked before any device work; nothing waits for the host."""
    import torch
    g = geometry(sr, fmin, fmax, W, hop, threshold, rms_gate)
    x, rows, n, ld_row, one = _rows_gpu(x)
    first_frame, n_frames = frame_range(n, g, first_frame, n_frames)
    f0, ap, rms = (torch.empty(rows, n_frames, dtype=torch.float32, device=x.device) for _ in range(3))
    voiced = torch.empty(rows, n_frames, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().svs_f0_track(x.data_ptr(), rows, n, ld_row, g.W, g.tau_min, g.tau_max, g.hop, first_frame, n_frames, g.threshold,
                                           g.rms_gate, g.sr, f0.data_ptr(), ap.data_ptr(), rms.data_ptr(), voiced.data_ptr(),
                                           _lib.stream_ptr(x.device)), "svs_f0_track")
    t = torch.from_numpy(frame_times(g, n_frames, first_frame)).to(x.device)
    return Track(t, f0[0], voiced[0], ap[0], rms[0]) if one else Track(t, f0, voiced, ap, rms)


def channel_mean(x):
    """(channels, n) or (n,) device samples -> the (n,) float32 mean of the channels that the tracker reads."""
    return x if x.dim() == 1 else x.float().mean(dim=0)


def check_options(options) -> dict:
    """The keywords of track_gpu that f0= of the separation calls takes (True or None-like: the defaults): a ValueError for anything else."""
    options = {} if options is True else dict(options)
    unknown = set(options) - {"fmin", "fmax", "W", "hop", "threshold", "rms_gate"}
    if unknown:
        raise ValueError(f"f0= takes fmin, fmax, W, hop, threshold and rms_gate, not {sorted(unknown)}")
    return options


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------
CSV_HEADER = "time,f0,voiced,aperiodicity,rms"


def write_csv(path: str, track: Track):
    """One row per frame of a one-row Track: time,f0,voiced,aperiodicity,rms."""
    cols = [np.asarray(c.cpu() if hasattr(c, "cpu") else c) for c in track]
    if cols[1].ndim != 1:
        raise ValueError(f"a csv file holds one track, got f0 of shape {cols[1].shape}")
    with open(path, "w", encoding="utf-8") as f:
        f.write(CSV_HEADER + "\n")
        for t, hz, v, a, r in zip(*cols):
            f.write(f"{t:.6f},{hz:.4f},{int(v)},{a:.6f},{r:.6e}\n")
    return len(cols[1])


def file_track(path: str, device=None, **options) -> Track:
    """The track of a wav file at its own rate, from the mean of its channels; device None: yin_reference on the host."""
    if device is None:
        from .data import read_pcm
        rate, data, channels = read_pcm(path)
        if data.dtype.kind == "i":
            data = data.astype(np.float64) / float(np.iinfo(data.dtype).max + 1)
        mono = data.mean(axis=1) if data.ndim == 2 else data
        return yin_reference(mono.astype(np.float32), rate, **options)[0]
    from .pcm import read_pcm_device
    from .resample import resample_poly_gpu
    rate, pcm, channels = read_pcm_device(path, device)             # a 24-bit file crosses as its 3 bytes per sample (pcm.py)
    return track_gpu(channel_mean(resample_poly_gpu(pcm, 1, 1, channels=channels, downmix=False)), rate, **options)


def main(argv=None):
    import argparse
    import os
    import sys
    parser = argparse.ArgumentParser(description="fundamental frequency of wav files (YIN, steps 1 to 5): time,f0,voiced,aperiodicity,rms per frame")
    parser.add_argument("--src", type=str, required=True, help="a wav file, or a folder of *.wav files")
    parser.add_argument("--csv", type=str, required=True, help="the csv file to write, or the target folder when --src is a folder")
    parser.add_argument("--fmin", type=float, default=FMIN, help=f"lowest f0 in Hz (default {FMIN:g})")
    parser.add_argument("--fmax", type=float, default=FMAX, help=f"highest f0 in Hz (default {FMAX:g})")
    parser.add_argument("--window", type=int, default=None, help="integration window W in samples (default: twice the longest lag)")
    parser.add_argument("--hop", type=int, default=None, help="samples between frames (default: 10 ms)")
    parser.add_argument("--threshold", type=float, default=THRESHOLD, help=f"absolute threshold on d' (default {THRESHOLD})")
    parser.add_argument("--rms_gate_db", type=float, default=None, help="frames whose rms lies below this level (dB re full scale) are unvoiced (default: off)")
    parser.add_argument("--device", default="gpu", choices=["gpu", "cpu"], help="gpu: csrc/f0.hip; cpu: the float64 definition")
    args = parser.parse_args(argv)
    device = None
    if args.device == "gpu":
        import torch
        if not torch.cuda.is_available():
            print("--device gpu needs a ROCm device (hand-written gfx950 kernels); --device cpu runs the float64 definition.")
            sys.exit(1)
        device = torch.device("cuda")
    options = dict(fmin=args.fmin, fmax=args.fmax, W=args.window, hop=args.hop, threshold=args.threshold, rms_gate=gate_from_db(args.rms_gate_db))
    if os.path.isdir(args.src):
        os.makedirs(args.csv, exist_ok=True)
        jobs = [(os.path.join(args.src, f), os.path.join(args.csv, f[:-4] + ".csv")) for f in sorted(os.listdir(args.src)) if f.endswith(".wav")]
    else:
        jobs = [(args.src, args.csv)]
    for src, dst in jobs:
        try:
            track = file_track(src, device, **options)
        except ValueError as e:
            parser.error(f"{src}: {e}")
        frames = write_csv(dst, track)
        voiced = int(np.asarray(track.voiced.cpu() if hasattr(track.voiced, "cpu") else track.voiced).sum())
        print(f"{dst}: {frames} frames, {voiced} voiced")


if __name__ == "__main__":
    main()
