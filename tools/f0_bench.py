#!/usr/bin/env python3
"""The f0 tracker's fused kernel on 240 s of mono, and separation with and without the pitch track, by tools/limiter_bench.py's
method: one process, warm-up, HIP events, medians of --reps with min - max, the two sides of a comparison alternating inside every
repetition.

    timeout -k 10 600 python tools/f0_bench.py [--seconds 240] [--reps 30] [--out profiles/f0_240s.jsonl]

Kernel rows: svs_f0_track with the defaults (65 .. 1000 Hz, W = 2 tau_max, 10 ms hop, threshold 0.15) on a vibrato voice plus noise at
8,192 Hz (the network's rate, where separate.py tracks) and at 44,100 Hz (a file's rate, where the f0 command line does), each beside a
torch device copy that reads the bytes the kernel reads.  The kernel's work is counted from the shapes: frames * tau_max * W terms of
the difference function plus frames * W of the rms, one fp64 FMA (2 FLOP) each; the achieved rate is that over the kernel's time, and
its share of the device's fp64 vector peak (78.6 TFLOP/s, the published figure for the MI355X) is reported, not gated.  The fp32
subtraction and the conversion that feed every FMA are not counted.
End-to-end rows, closed-form checkpoint, fp32, 240 s of stereo at the network rate: separate_waveform(both_stems) and the default way
out to --rate for both stems, without and with f0=True.  One JSON object per line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import f0 as f0m  # noqa: E402
from svs_unet_pytorch_amd import resample as rs  # noqa: E402
from svs_unet_pytorch_amd import synth  # noqa: E402
from svs_unet_pytorch_amd.config import SAMPLE_RATE  # noqa: E402
from tools._benchlib import closed_form_model, copy_of, timed_pair  # noqa: E402

FP64_VECTOR_PEAK_TFLOPS = 78.6


def ratio(a, b):
    return round(a["median_ms"] / b["median_ms"], 4)


def voice(seconds, rate):
    """A 5 Hz, +-50 cent vibrato around 220 Hz with 1 / k harmonics, plus white noise 20 dB under it."""
    n = int(seconds * rate)
    t = np.arange(n) / rate
    x = f0m.harmonic_tone(220.0 * 2.0 ** ((50.0 / 1200.0) * np.sin(2.0 * np.pi * 5.0 * t)), rate)
    return x + (0.1 * float(np.sqrt(np.mean(x.astype(np.float64) ** 2))) * np.random.default_rng(0).standard_normal(n)).astype(np.float32)


def kernel_rows(seconds, reps):
    for rate in (SAMPLE_RATE, 44100):
        x = torch.from_numpy(voice(seconds, rate)).to("cuda")
        g = f0m.geometry(rate)
        frames = f0m.frame_count(x.numel(), g.span, g.hop)
        fma = frames * (g.tau_max + 1) * g.W
        k, c = timed_pair(lambda: f0m.track_gpu(x, rate), copy_of(2 * x.numel() * 4), reps)
        track = f0m.track_gpu(x, rate)
        tflops = 2.0 * fma / (k["median_ms"] * 1e-3) / 1e12
        yield dict(kind="kernel", kernel="svs_f0_track", seconds=seconds, rate=rate, samples=x.numel(), W=g.W, tau_min=g.tau_min, tau_max=g.tau_max,
                   hop=g.hop, frames=frames, voiced_share=round(float(track.voiced.float().mean()), 4), bytes_read=x.numel() * 4,
                   bytes_written=frames * 16, fp64_fma=fma, reps=reps, kernel_time=k, torch_copy_reading_the_same_bytes=c,
                   ratio_kernel_over_copy=ratio(k, c), achieved_fp64_tflops=round(tflops, 3), fp64_vector_peak_tflops=FP64_VECTOR_PEAK_TFLOPS,
                   share_of_fp64_vector_peak=round(tflops / FP64_VECTOR_PEAK_TFLOPS, 4),
                   bound="fp64 vector rate: the bytes alone would take the copy's time")


def end_to_end_rows(seconds, rate, reps):
    from fractions import Fraction

    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = closed_form_model()
    n = int(seconds * SAMPLE_RATE)
    y = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    fr = Fraction(SAMPLE_RATE, rate)

    def run(f0):
        sep = separate_waveform(model, y, peak=None, both_stems=True, f0=f0)
        sep = sep[0] if f0 else sep
        return [rs.resample_encode_gpu(stem, fr.denominator, fr.numerator, fmt="PCM_16", peak=0.9, common_gain=True) for stem in sep]

    a, b = timed_pair(lambda: run(None), lambda: run(True), max(3, reps // 3), warmup=2)
    yield dict(kind="end_to_end", precision="fp32", seconds=seconds, rate=rate, channels=2, samples_per_channel_at_network_rate=n, subtype="PCM_16",
               reps=max(3, reps // 3), without_f0=a, with_f0=b, ratio_with_over_without=ratio(b, a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rate", type=int, default=44100, help="the rate of the written files in the end-to-end rows")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("f0_bench.py needs a ROCm device: nothing here is measured on a CPU")
    import datetime
    import itertools
    rows = []
    for row in itertools.chain(kernel_rows(a.seconds, a.reps), end_to_end_rows(a.seconds, a.rate, a.reps)):
        row["device"] = torch.cuda.get_device_name(0)
        row["date"] = datetime.date.today().isoformat()
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
