#!/usr/bin/env python3
"""The smoothed pitch track's kernels on 240 s of mono, and separation with the raw and with the smoothed track, by tools/f0_bench.py's
method: one process, warm-up, HIP events, medians of --reps with min - max, the two sides of a comparison alternating inside every
repetition.

    timeout -k 10 900 python tools/f0_smooth_bench.py [--seconds 240] [--reps 30] [--out profiles/f0_smooth_240s.jsonl]

Kernel rows, on tools/f0_bench.py's vibrato voice plus noise at 8,192 Hz and at 44,100 Hz with the default geometry:
  svs_f0_candidates beside svs_f0_track (the same difference function; the candidates add seven wave minima per frame and 88 bytes of
  output per frame to its 16);
  svs_f0_viterbi at each chunk on those candidates, beside a torch device copy that reads the bytes the decode reads (64 per frame:
  7 lags, 7 aperiodicities, the count and the rms) -- five launches against one, so at 24 k frames the comparison is one of launch
  counts more than of bytes; the row also holds the workspace size;
  the whole smoothed track (candidates, decode, select: seven launches) beside the raw one.
End-to-end rows, closed-form checkpoint, fp32, 240 s of stereo at the network rate: separate_waveform(both_stems) and the default way
out to --rate for both stems, with f0=True against f0={"smooth": True}, and without a track against the smoothed one.
One JSON object per line.  Nothing here is gated: they are first figures."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import _lib  # noqa: E402
from svs_unet_pytorch_amd import f0 as f0m  # noqa: E402
from svs_unet_pytorch_amd import resample as rs  # noqa: E402
from svs_unet_pytorch_amd import synth  # noqa: E402
from svs_unet_pytorch_amd.config import SAMPLE_RATE  # noqa: E402
from tools._benchlib import closed_form_model, copy_of, timed_pair  # noqa: E402
from tools.f0_bench import ratio, voice  # noqa: E402


def kernel_rows(seconds, reps):
    for rate in (SAMPLE_RATE, 44100):
        x = torch.from_numpy(voice(seconds, rate)).to("cuda")
        g = f0m.geometry(rate)
        frames = f0m.frame_count(x.numel(), g.span, g.hop)
        shape = dict(seconds=seconds, rate=rate, samples=x.numel(), W=g.W, tau_min=g.tau_min, tau_max=g.tau_max, hop=g.hop, frames=frames, reps=reps)
        c, t = timed_pair(lambda: f0m.candidates_gpu(x, rate), lambda: f0m.track_gpu(x, rate), reps)
        raw, (c_tau, c_f0, c_ap, count) = f0m.candidates_gpu(x, rate)
        yield dict(kind="kernel", kernel="svs_f0_candidates", **shape, mean_count=round(float(count.float().mean()), 3),
                   bytes_written=frames * (16 + 88), kernel_time=c, svs_f0_track_time=t, ratio_candidates_over_track=ratio(c, t))
        cents = f0m.cents_gpu(g.sr, g.tau_max, x.device)
        for chunk in f0m.CHUNKS:
            v, cp = timed_pair(lambda: f0m.viterbi_gpu(c_tau, c_ap, count, raw.rms, cents, g.tau_min, g.rms_gate, chunk=chunk),
                               copy_of(2 * frames * 64), reps)
            state, cost = f0m.viterbi_gpu(c_tau, c_ap, count, raw.rms, cents, g.tau_min, g.rms_gate, chunk=chunk)
            yield dict(kind="kernel", kernel="svs_f0_viterbi", chunk=chunk, chunks=-(-frames // chunk), **shape, bytes_read=frames * 64,
                       bytes_written=frames * 4 + 8, workspace_bytes=int(_lib.lib().svs_f0_viterbi_workspace(1, frames, chunk)),
                       voiced_share=round(float((state < f0m.K).float().mean()), 4), cost=int(cost), kernel_time=v,
                       torch_copy_reading_the_same_bytes=cp, ratio_kernel_over_copy=ratio(v, cp), ratio_viterbi_over_track=ratio(v, t),
                       launches=5)
        s, t2 = timed_pair(lambda: f0m.track_gpu(x, rate, smooth=True), lambda: f0m.track_gpu(x, rate), reps)
        smooth = f0m.track_gpu(x, rate, smooth=True)
        yield dict(kind="track", what="track_gpu(smooth=True) beside track_gpu()", chunk=f0m.CHUNK, **shape, launches=7,
                   raw_voiced_share=round(float(raw.voiced.float().mean()), 4), smoothed_voiced_share=round(float(smooth.voiced.float().mean()), 4),
                   smoothed_time=s, raw_time=t2, ratio_smoothed_over_raw=ratio(s, t2))


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

    reps = max(3, reps // 3)
    shape = dict(kind="end_to_end", precision="fp32", seconds=seconds, rate=rate, channels=2, samples_per_channel_at_network_rate=n,
                 subtype="PCM_16", reps=reps)
    a, b = timed_pair(lambda: run(True), lambda: run({"smooth": True}), reps, warmup=2)
    yield dict(**shape, with_raw_f0=a, with_smoothed_f0=b, ratio_smoothed_over_raw=ratio(b, a))
    a, b = timed_pair(lambda: run(None), lambda: run({"smooth": True}), reps, warmup=2)
    yield dict(**shape, without_f0=a, with_smoothed_f0=b, ratio_smoothed_over_without=ratio(b, a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rate", type=int, default=44100, help="the rate of the written files in the end-to-end rows")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("f0_smooth_bench.py needs a ROCm device: nothing here is measured on a CPU")
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
