#!/usr/bin/env python3
"""The R 128 meter's kernels and the true-peak way out on tools/loudness_bench.py's case (240 s of stereo, files at 44.1 kHz), by that
tool's method: one process, warm-up, HIP events, medians of --reps with min - max, the two sides of a comparison alternating inside
every repetition.

    timeout -k 10 600 python tools/r128_bench.py [--seconds 240] [--reps 30] [--out profiles/r128_240s.jsonl]

Kernel rows:
  svs_true_peaks on both stems (2 x 2 rows, factor 4, one launch and one reduce) beside a torch device copy that reads the same bytes,
    and beside the two svs_resample_peaks launches at 1/1 that it replaces in the loudness way out;
  svs_loudness_series (both series) beside svs_loudness_blocks on the same stereo signal;
  svs_loudness_stats on that signal's series, and on 36,000 short-term windows (an hour of audio).
End-to-end rows, closed-form checkpoint, fp32: the way out to --rate for both stems with a loudness target
(resample.encode_loudness_gpu) with true_peak off and on, and separation (separate_waveform(both_stems)) followed by that way out, off
and on.  One JSON object per line; ratios are reported, nothing is gated."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import loudness as ld  # noqa: E402
from svs_unet_pytorch_amd import resample as rs  # noqa: E402
from svs_unet_pytorch_amd import synth  # noqa: E402
from svs_unet_pytorch_amd.config import SAMPLE_RATE  # noqa: E402
from tools._benchlib import closed_form_model, copy_of, timed, timed_pair  # noqa: E402


def ratio(a, b):
    return round(a["median_ms"] / b["median_ms"], 4)


def kernel_rows(seconds, rate, reps):
    n = int(seconds * rate)
    stems = torch.from_numpy(np.stack([np.stack([synth.audio(n, 20), synth.audio(n, 21)]),
                                       np.stack([synth.audio(n, 22), synth.audio(n, 23)])])).to("cuda")        # (2, 2, n)
    x = stems[0]
    common = dict(seconds=seconds, rate=rate, channels=2, samples_per_channel=n, reps=reps)
    read_bytes = stems.numel() * 4

    def true_peaks():
        return ld.true_peaks_gpu(stems, rate, 2)

    def sample_peaks():
        return [rs.resample_peaks_gpu(stems[k], 1, 1) for k in range(2)]

    k, c = timed_pair(true_peaks, copy_of(2 * read_bytes), reps)      # the copy reads read_bytes and writes as many
    yield dict(kind="kernel", kernel="svs_true_peaks", stems=2, factor=ld.true_peak_factor(rate), **common, bytes_read=read_bytes,
               kernel_time=k, torch_copy_reading_the_same_bytes=c, ratio_kernel_over_copy=ratio(k, c))
    k, p = timed_pair(true_peaks, sample_peaks, reps)
    yield dict(kind="kernel", kernel="svs_true_peaks vs 2 x svs_resample_peaks 1/1", stems=2, **common, true_peaks=k, sample_peaks=p,
               ratio_true_over_sample=ratio(k, p))
    s, b = timed_pair(lambda: ld.series_gpu(x, rate), lambda: ld.block_energies_gpu(x, rate), reps)
    yield dict(kind="kernel", kernel="svs_loudness_series vs svs_loudness_blocks", **common, windows_m=ld.nblocks(n, rate),
               windows_s=ld.nwindows(n, rate, ld.BINS_S), series=s, blocks=b, ratio_series_over_blocks=ratio(s, b))
    z_m, z_s = ld.series_gpu(x, rate)
    yield dict(kind="kernel", kernel="svs_loudness_stats", **common, n_m=z_m.numel(), n_s=z_s.numel(),
               kernel_time=timed(lambda: ld.stats_gpu(z_m, z_s), reps))
    hour = torch.from_numpy(10.0 ** np.random.default_rng(0).uniform(-6.0, -1.0, 36000)).to("cuda")
    yield dict(kind="kernel", kernel="svs_loudness_stats", n_m=hour.numel(), n_s=hour.numel(), reps=reps, note="an hour of short-term windows",
               kernel_time=timed(lambda: ld.stats_gpu(hour, hour), reps))


def end_to_end_rows(seconds, rate, reps):
    from fractions import Fraction

    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = closed_form_model()
    n = int(seconds * SAMPLE_RATE)
    y = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    fr = Fraction(SAMPLE_RATE, rate)
    up, down = fr.denominator, fr.numerator
    code, dtype = rs.pcm_format("int16")

    def out(sep, true_peak):
        return rs.encode_loudness_gpu([sep[0].contiguous(), sep[1].contiguous()], up, down, code, dtype, -23.0, 0.9, rate, None, true_peak)

    sep = separate_waveform(model, y, peak=None, both_stems=True)
    common = dict(seconds=seconds, rate=rate, channels=2, samples_per_channel_at_network_rate=n, subtype="PCM_16", loudness=-23.0, reps=reps)
    a, b = timed_pair(lambda: out(sep, False), lambda: out(sep, True), reps)
    yield dict(kind="way_out", **common, sample_peak_ceiling=a, true_peak_ceiling=b, ratio_true_over_sample=ratio(b, a))
    a, b = timed_pair(lambda: out(separate_waveform(model, y, peak=None, both_stems=True), False),
                      lambda: out(separate_waveform(model, y, peak=None, both_stems=True), True), max(3, reps // 3), warmup=2)
    yield dict(kind="end_to_end", precision="fp32", **common, sample_peak_ceiling=a, true_peak_ceiling=b, ratio_true_over_sample=ratio(b, a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("r128_bench.py needs a ROCm device: nothing here is measured on a CPU")
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
