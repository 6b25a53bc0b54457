#!/usr/bin/env python3
"""csrc/pcm.hip's two kernels and the 24-bit / dithered ways in and out on tools/loudness_bench.py's case (240 s of stereo, files at
44.1 kHz), by that tool's method: one process, warm-up, HIP events, medians of --reps with min - max, the two sides of a comparison
alternating inside every repetition.  The way in crosses the host, so it is timed with the wall clock around a device synchronise.

    timeout -k 10 600 python tools/pcm_bench.py [--seconds 240] [--reps 30] [--out profiles/pcm24_240s.jsonl]

Kernel rows:
  svs_pcm_encode_dither at 16 / 24 bits x none / tpdf / hp on a planar stereo buffer at the written rate, beside a torch device copy
    that moves the same bytes; the 16-bit undithered case also beside svs_resample_encode 1/1 int16 on the same buffer;
  svs_pcm24_widen on that many samples beside a torch device copy that moves the same bytes.
Way in: a 24-bit file of that length -> device int32 through pcm.read_pcm_device (3 bytes per sample cross, widened on the device)
against data.read_pcm + .to(device) (scipy widens on the host, 4 bytes per sample cross); the file is in the page cache for both.
Way out, both stems, closed-form checkpoint, fp32: PCM_16 / none (the fused svs_resample_encode path, the default) timed against
itself -- the spread of the method --, against PCM_16 / tpdf and against PCM_24 / none (the planar buffer and svs_pcm_encode_dither);
then separation (separate_waveform(both_stems)) followed by each of them.  One JSON object per line; ratios are reported, nothing is
gated."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import _lib, pcm  # noqa: E402
from svs_unet_pytorch_amd import resample as rs  # noqa: E402
from svs_unet_pytorch_amd import synth  # noqa: E402
from svs_unet_pytorch_amd.config import SAMPLE_RATE  # noqa: E402
from tools._benchlib import closed_form_model, copy_of, stats, timed_pair  # noqa: E402


def ratio(a, b):
    return round(a["median_ms"] / b["median_ms"], 4)


def kernel_rows(seconds, rate, reps):
    n = int(seconds * rate)
    buf = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")          # (2, n), planar
    gain = torch.full((2,), 0.9, dtype=torch.float32, device="cuda")
    common = dict(seconds=seconds, rate=rate, channels=2, frames=n, reps=reps)
    for bits in (16, 24):
        for kind in ("none", "tpdf", "hp"):
            out = torch.empty((n, 2 * bits // 8), dtype=torch.uint8, device="cuda")
            moved = buf.numel() * 4 + out.numel()
            k, c = timed_pair(lambda: pcm.encode_dither_gpu(buf, n, gain, bits, kind, 0, out=out), copy_of(moved), reps)
            yield dict(kind="kernel", kernel="svs_pcm_encode_dither", bits=bits, dither=kind, **common, bytes_moved=moved, kernel_time=k,
                       torch_copy_moving_the_same_bytes=c, ratio_kernel_over_copy=ratio(k, c))
    L = _lib.lib()
    one, _ = rs.tap_table(1, 1, buf.device)
    out16 = torch.empty((n, 2), dtype=torch.int16, device="cuda")

    def fused():
        _lib.check(L.svs_resample_encode(buf.data_ptr(), 2, n, n, one.data_ptr(), 1, 1, 1, gain.data_ptr(), rs.PCM_I16, out16.data_ptr(),
                                         _lib.stream_ptr()), "svs_resample_encode")

    k, f = timed_pair(lambda: pcm.encode_dither_gpu(buf, n, gain, 16, "none", 0, out=out16), fused, reps)
    yield dict(kind="kernel", kernel="svs_pcm_encode_dither 16 / none vs svs_resample_encode 1/1 int16", **common, pcm_encode_dither=k,
               resample_encode=f, ratio_new_over_existing=ratio(k, f))
    packed = torch.randint(0, 256, (2 * n * 3,), dtype=torch.uint8, device="cuda")
    moved = packed.numel() + 2 * n * 4
    wide = torch.empty(2 * n, dtype=torch.int32, device="cuda")

    def widen():
        _lib.check(L.svs_pcm24_widen(packed.data_ptr(), 2 * n, wide.data_ptr(), _lib.stream_ptr()), "svs_pcm24_widen")

    k, c = timed_pair(widen, copy_of(moved), reps)
    yield dict(kind="kernel", kernel="svs_pcm24_widen", **common, samples=2 * n, bytes_moved=moved, kernel_time=k,
               torch_copy_moving_the_same_bytes=c, ratio_kernel_over_copy=ratio(k, c))


def wall_pair(fa, fb, reps, warmup=2):
    """timed_pair with the wall clock: for paths whose host half is what is compared."""
    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(warmup):
        once(fa), once(fb)
    ta, tb = [], []
    for i in range(reps):
        if i % 2 == 0:
            ta.append(once(fa)), tb.append(once(fb))
        else:
            tb.append(once(fb)), ta.append(once(fa))
    return stats(ta), stats(tb)


def way_in_rows(seconds, rate, reps):
    from svs_unet_pytorch_amd import data
    n = int(seconds * rate)
    vals = np.random.default_rng(24).integers(-0x800000, 0x800000, (n, 2)).astype(np.int32)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in24.wav")
        pcm.write_wav24(path, rate, pcm.pack24(vals))
        del vals

        def host():
            _, samples, _ = data.read_pcm(path)
            return torch.from_numpy(samples).to("cuda")

        def device():
            return pcm.read_pcm_device(path, "cuda")[1]

        assert torch.equal(host(), device())
        d, h = wall_pair(device, host, reps)
    yield dict(kind="way_in", seconds=seconds, rate=rate, channels=2, frames=n, reps=reps, clock="wall, device synchronised",
               read_pcm_device=d, read_pcm_then_to_device=h, ratio_device_over_host=ratio(d, h))


def end_to_end_rows(seconds, rate, reps):
    from fractions import Fraction

    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = closed_form_model()
    n = int(seconds * SAMPLE_RATE)
    y = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    fr = Fraction(SAMPLE_RATE, rate)
    up, down = fr.denominator, fr.numerator
    code, dtype = rs.pcm_format("int16")

    def fused(sep):                                   # streaming.separate_to_wav's default: per stem, peaks then the fused encoder
        return [rs.resample_encode_gpu(sep[k], up, down, fmt="int16", peak=0.9, common_gain=True) for k in range(2)]

    def planar(sep, **how):
        return rs.encode_loudness_gpu([sep[0].contiguous(), sep[1].contiguous()], up, down, code, dtype, None, 0.9, rate, None, False, **how)

    def tpdf(sep):
        return planar(sep, subtype_bits=16, dither="tpdf", dither_seed=0)

    def p24(sep):
        return planar(sep, subtype_bits=24)

    def separated():
        return separate_waveform(model, y, peak=None, both_stems=True)

    sep = separated()
    common = dict(seconds=seconds, rate=rate, channels=2, stems=2, samples_per_channel_at_network_rate=n, reps=reps)
    a, b = timed_pair(lambda: fused(sep), lambda: fused(sep), reps)
    yield dict(kind="way_out", **common, config="PCM_16 / none twice (the method's spread)", first=a, second=b, ratio_second_over_first=ratio(b, a))
    for name, fn in (("PCM_16 / tpdf", tpdf), ("PCM_24 / none", p24)):
        a, b = timed_pair(lambda: fused(sep), lambda: fn(sep), reps)
        yield dict(kind="way_out", **common, config=f"{name} vs PCM_16 / none", pcm16_none=a, other=b, ratio_other_over_pcm16_none=ratio(b, a))
    r3 = max(3, reps // 3)
    a, b = timed_pair(lambda: fused(separated()), lambda: fused(separated()), r3, warmup=2)
    yield dict(kind="end_to_end", precision="fp32", **common, config="PCM_16 / none twice (the method's spread)", first=a, second=b,
               ratio_second_over_first=ratio(b, a))
    for name, fn in (("PCM_16 / tpdf", tpdf), ("PCM_24 / none", p24)):
        a, b = timed_pair(lambda: fused(separated()), lambda: fn(separated()), r3, warmup=2)
        yield dict(kind="end_to_end", precision="fp32", **common, config=f"{name} vs PCM_16 / none", pcm16_none=a, other=b,
                   ratio_other_over_pcm16_none=ratio(b, a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pcm_bench.py needs a ROCm device: nothing here is measured on a CPU")
    import datetime
    import itertools
    rows = []
    for row in itertools.chain(kernel_rows(a.seconds, a.rate, a.reps), way_in_rows(a.seconds, a.rate, max(5, a.reps // 3)),
                               end_to_end_rows(a.seconds, a.rate, a.reps)):
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
