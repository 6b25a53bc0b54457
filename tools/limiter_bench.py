#!/usr/bin/env python3
"""The look-ahead limiter's three kernels and the way out with --limiter on tools/r128_bench.py's case (240 s of stereo, two stems,
files at 44.1 kHz), by that tool's method: one process, warm-up, HIP events, medians of --reps with min - max, the two sides of a
comparison alternating inside every repetition.

    timeout -k 10 600 python tools/limiter_bench.py [--seconds 240] [--reps 30] [--out profiles/limiter_240s.jsonl]

Kernel rows, h = 88 (2 ms at 44.1 kHz), each beside a torch device copy that moves the bytes the kernel touches:
  svs_limiter_envelope on both stems (2 x 2 rows, factor 4 and factor 1): reads the rows, writes e;
  svs_limiter_curve: reads e, writes g;
  svs_limiter_apply: reads the rows and g, writes the rows.
End-to-end rows, closed-form checkpoint, fp32, --loudness -14 --true_peak: the way out to --rate for both stems
(resample.encode_loudness_gpu) without and with limiter_ms = 2.0, and separation (separate_waveform(both_stems)) followed by that way
out, without and with.  One JSON object per line; ratios are reported, nothing is gated."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import limiter as lim  # noqa: E402
from svs_unet_pytorch_amd import loudness as ld  # noqa: E402
from svs_unet_pytorch_amd import resample as rs  # noqa: E402
from svs_unet_pytorch_amd import synth  # noqa: E402
from svs_unet_pytorch_amd.config import SAMPLE_RATE  # noqa: E402
from tools._benchlib import closed_form_model, copy_of, timed_pair  # noqa: E402

TARGET, MS = -14.0, 2.0


def ratio(a, b):
    return round(a["median_ms"] / b["median_ms"], 4)


def kernel_rows(seconds, rate, reps):
    n = int(seconds * rate)
    stems = torch.from_numpy(np.stack([np.stack([synth.audio(n, 20), synth.audio(n, 21)]),
                                       np.stack([synth.audio(n, 22), synth.audio(n, 23)])])).to("cuda")        # (2, 2, n)
    h = lim.half_width(rate, MS)
    common = dict(seconds=seconds, rate=rate, stems=2, channels=2, samples_per_row=n, h=h, reps=reps)
    rows_bytes, row_bytes = stems.numel() * 4, n * 4
    G = 0.9 / float(stems.abs().max()) * 10.0 ** (6.0 / 20.0)          # 6 dB over what the plain rule allows: the limiter has work
    for factor in (ld.true_peak_factor(rate), 1):
        k, c = timed_pair(lambda: lim.envelope_gpu(stems, factor, 2), copy_of(rows_bytes + row_bytes), reps)
        yield dict(kind="kernel", kernel="svs_limiter_envelope", factor=factor, **common, bytes_touched=rows_bytes + row_bytes, kernel_time=k,
                   torch_copy_moving_the_same_bytes=c, ratio_kernel_over_copy=ratio(k, c))
    e = lim.envelope_gpu(stems, ld.true_peak_factor(rate), 2)
    k, c = timed_pair(lambda: lim.curve_gpu(e, G, 0.9, h), copy_of(2 * row_bytes), reps)
    g = lim.curve_gpu(e, G, 0.9, h)
    yield dict(kind="kernel", kernel="svs_limiter_curve", **common, bytes_touched=2 * row_bytes, share_of_samples_reduced=round(float((g < 1).float().mean()), 5),
               deepest_reduction_db=round(20.0 * float(torch.log10(g.min())), 3), kernel_time=k, torch_copy_moving_the_same_bytes=c,
               ratio_kernel_over_copy=ratio(k, c))
    ones = torch.ones_like(g)                                          # x * 1 leaves the rows as they are, whatever --reps
    flat = stems.view(4, n)
    k, c = timed_pair(lambda: lim.apply_gpu(flat, ones), copy_of(2 * rows_bytes + row_bytes), reps)
    yield dict(kind="kernel", kernel="svs_limiter_apply", **common, bytes_touched=2 * rows_bytes + row_bytes, kernel_time=k,
               torch_copy_moving_the_same_bytes=c, ratio_kernel_over_copy=ratio(k, c))


def end_to_end_rows(seconds, rate, reps):
    from fractions import Fraction

    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = closed_form_model()
    n = int(seconds * SAMPLE_RATE)
    y = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    fr = Fraction(SAMPLE_RATE, rate)
    up, down = fr.denominator, fr.numerator
    code, dtype = rs.pcm_format("int16")

    def out(sep, limiter_ms, extra=None):
        return rs.encode_loudness_gpu([sep[0].contiguous(), sep[1].contiguous()], up, down, code, dtype, TARGET, 0.9, rate, None, True,
                                      limiter_ms=limiter_ms, limiter_out=extra)

    sep = separate_waveform(model, y, peak=None, both_stems=True)
    extra = {}
    _, gain_on, info_on = out(sep, MS, extra)
    _, gain_off, info_off = out(sep, None)
    L_in, unlimited = (float(v) for v in info_on[[0, 2]].cpu())
    written_on = float(extra["limited_info"][0]) + 20.0 * float(torch.log10(gain_on[0]))
    written_off = L_in + 20.0 * float(torch.log10(gain_off[0]))
    common = dict(seconds=seconds, rate=rate, channels=2, samples_per_channel_at_network_rate=n, subtype="PCM_16", loudness=TARGET, true_peak=True,
                  limiter_ms=MS, reps=reps)
    yield dict(kind="levels", **common, loudness_in=round(L_in, 3), unlimited_gain_db=round(20.0 * np.log10(unlimited), 3),
               written_lufs_without=round(written_off, 3), written_lufs_with=round(written_on, 3),
               deepest_reduction_db=round(20.0 * float(torch.log10(extra["curve"].min())), 3))
    a, b = timed_pair(lambda: out(sep, None), lambda: out(sep, MS), reps)
    yield dict(kind="way_out", **common, without_limiter=a, with_limiter=b, ratio_with_over_without=ratio(b, a))
    a, b = timed_pair(lambda: out(separate_waveform(model, y, peak=None, both_stems=True), None),
                      lambda: out(separate_waveform(model, y, peak=None, both_stems=True), MS), max(3, reps // 3), warmup=2)
    yield dict(kind="end_to_end", precision="fp32", **common, without_limiter=a, with_limiter=b, ratio_with_over_without=ratio(b, a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("limiter_bench.py needs a ROCm device: nothing here is measured on a CPU")
    import datetime
    import itertools
    rows = []
    for row in itertools.chain(kernel_rows(a.seconds, a.rate, a.reps), end_to_end_rows(a.seconds, a.rate, a.reps)):
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
