#!/usr/bin/env python3
"""The loudness meter and the loudness-normalised way out on tools/stream_bench.py's case (240 s of stereo, files at 44.1 kHz): one
process, warm-up, HIP events, median of --reps.

    python tools/loudness_bench.py [--seconds 240] [--reps 30] [--out profiles/loudness_240s.jsonl]

Kernel row: svs_loudness_blocks on --seconds of stereo float32 at --rate beside a torch device copy of the same bytes (the signal
read once and written once; the meter reads it twice and writes next to nothing), the two alternating inside every repetition.  The
ratio is reported, not gated.  A second row adds svs_loudness_gain (measure only).
End-to-end rows, closed-form checkpoint, fp32: separate_waveform(both_stems) at the network rate followed by the way out to --rate
for both stems, once by the peak rule (resample_encode_gpu(peak=0.9) per stem: the default, unchanged) and once with a loudness target
(resample.encode_loudness_gpu: svs_resample_poly into a float32 buffer, the meter on the sum, peaks, one gain, 1/1 encode); and the
way out alone, both ways.  One JSON object per line."""
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


def kernel_rows(seconds, rate, reps):
    n = int(seconds * rate)
    x = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    nbytes = 2 * x.numel() * 4                                       # the copy's traffic: every sample read once, written once
    common = dict(seconds=seconds, rate=rate, channels=2, samples_per_channel=n, blocks=ld.nblocks(n, rate), reps=reps)
    for name, fn in (("svs_loudness_blocks", lambda: ld.block_energies_gpu(x, rate)),
                     ("svs_loudness_blocks + svs_loudness_gain", lambda: ld.loudness_gain_gpu(x, rate))):
        k, c = timed_pair(fn, copy_of(nbytes), reps)
        yield dict(kind="kernel", kernel=name, **common, copy_bytes=nbytes, kernel_time=k, torch_copy_same_bytes=c,
                   ratio_kernel_over_copy=round(k["median_ms"] / c["median_ms"], 4))


def end_to_end_rows(seconds, rate, reps):
    from fractions import Fraction

    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = closed_form_model()
    n = int(seconds * SAMPLE_RATE)
    y = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    fr = Fraction(SAMPLE_RATE, rate)
    up, down = fr.denominator, fr.numerator
    code, dtype = rs.pcm_format("int16")

    def out_peak(sep):
        return [rs.resample_encode_gpu(stem, up, down, fmt="int16", peak=0.9, common_gain=True) for stem in sep]

    def out_loudness(sep):
        return rs.encode_loudness_gpu([sep[0].contiguous(), sep[1].contiguous()], up, down, code, dtype, -23.0, 0.9, rate, None)

    sep = separate_waveform(model, y, peak=None, both_stems=True)
    common = dict(seconds=seconds, rate=rate, channels=2, samples_per_channel_at_network_rate=n, subtype="PCM_16", reps=reps)
    a, b = timed_pair(lambda: out_peak(sep), lambda: out_loudness(sep), reps)
    yield dict(kind="way_out", **common, peak_rule=a, loudness_target=b, ratio_loudness_over_peak=round(b["median_ms"] / a["median_ms"], 4))
    a, b = timed_pair(lambda: out_peak(separate_waveform(model, y, peak=None, both_stems=True)),
                      lambda: out_loudness(separate_waveform(model, y, peak=None, both_stems=True)), max(3, reps // 3), warmup=2)
    yield dict(kind="end_to_end", precision="fp32", **common, peak_rule=a, loudness_target=b,
               ratio_loudness_over_peak=round(b["median_ms"] / a["median_ms"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loudness_bench.py needs a ROCm device: nothing here is measured on a CPU")
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
