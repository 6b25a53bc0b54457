#!/usr/bin/env python3
"""Full-band stems (csrc/fullband.hip) on tools/stream_bench.py's case (240 s of stereo int16 at 44.1 kHz): one process, warm-up, HIP
events, median of --reps.

    python tools/fullband_bench.py [--seconds 240] [--reps 30] [--out profiles/fullband_240s.jsonl]

Kernel rows: svs_fullband_gains on the separation's own tiles and mask, and svs_fullband_mix for one and for two stems, each beside
a torch device copy of the bytes it touches (gains: the top quarter of the rows of tiles and mask read; mix: the stems, y and the PCM
read, the float32 rows at the file's rate written), alternating inside every repetition; the mix also beside the way the stems reach
the file's rate without it (svs_resample_poly of the same stems into float32: the same bytes written, the PCM and y not read).
Way-out rows: stems -> int16 files' samples, by the default path (resample_encode_gpu(peak=0.9) per stem, the fused encoder) and with
the flag (gains, mix, encode_planar_gpu).  End-to-end rows: PCM on the device -> resampled, separated (closed-form checkpoint, fp32),
written out, flag on and off.  Ratios are reported, not gated.  One JSON object per line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import fullband as fb  # noqa: E402
from svs_unet_pytorch_amd import resample as rs  # noqa: E402
from svs_unet_pytorch_amd import synth  # noqa: E402
from svs_unet_pytorch_amd.config import HOP_SIZE, SAMPLE_RATE  # noqa: E402
from tools._benchlib import closed_form_model, copy_of, timed_pair  # noqa: E402


def rows_of(seconds, rate, reps):
    from fractions import Fraction

    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = closed_form_model()
    n = int(seconds * rate)
    mix = 0.5 * np.stack([synth.audio(n, 20), 0.7 * synth.audio(n, 21)], axis=1)
    pcm = torch.from_numpy(np.round(mix / np.abs(mix).max() * 30000).astype(np.int16)).to("cuda")
    fr = Fraction(SAMPLE_RATE, rate)
    up, down = fr.denominator, fr.numerator                         # the way up: file rate / network rate
    code, dtype = rs.pcm_format("int16")

    def separated(both=True):
        y = rs.resample_poly_gpu(pcm, down, up, channels=2, downmix=False)
        aux = {}
        return separate_waveform(model, y, peak=None, both_stems=both, aux=aux), aux

    def out_default(sep):
        return [rs.resample_encode_gpu(stem, up, down, fmt="int16", peak=0.9, common_gain=True) for stem in sep]

    def out_fullband(sep, aux, mode="mask"):
        gf = fb.frame_gains_gpu(aux["tiles"], aux["mask"], aux["frames"]) if mode == "mask" else None
        buf = fb.fullband_mix_gpu(sep, aux["y"], pcm, aux["norm"], gf, aux["frames"], HOP_SIZE, up, down)
        return rs.encode_planar_gpu(buf, buf.shape[2], code, dtype)

    sep, aux = separated()
    T, tiles, mask = aux["frames"], aux["tiles"], aux["mask"]
    C, n_in = sep.shape[1], sep.shape[2]
    n_out = rs.out_len(n_in, up, down)
    common = dict(seconds=seconds, rate=rate, channels=C, frames=T, samples_per_channel_at_network_rate=n_in,
                  samples_per_channel_at_file_rate=n_out, reps=reps)

    nbytes = 2 * tiles.numel() // fb.TOP_DIV * 4 + C * T * 4
    k, c = timed_pair(lambda: fb.frame_gains_gpu(tiles, mask, T), copy_of(nbytes), reps)
    yield dict(kind="kernel", kernel="svs_fullband_gains", **common, bytes_touched=nbytes, kernel_time=k, torch_copy_same_bytes=c,
               ratio_kernel_over_copy=round(k["median_ms"] / c["median_ms"], 4))

    gf = fb.frame_gains_gpu(tiles, mask, T)
    for S in (1, 2):
        st = sep[:S].contiguous()
        flat = st.view(S * C, n_in)
        nbytes = (S + 1) * C * n_in * 4 + C * n_out * 2 + S * C * n_out * 4
        k, c = timed_pair(lambda: fb.fullband_mix_gpu(st, aux["y"], pcm, aux["norm"], gf, T, HOP_SIZE, up, down), copy_of(nbytes), reps)
        k2, p = timed_pair(lambda: fb.fullband_mix_gpu(st, aux["y"], pcm, aux["norm"], gf, T, HOP_SIZE, up, down),
                           lambda: rs.resample_poly_gpu(flat, up, down), reps)
        yield dict(kind="kernel", kernel="svs_fullband_mix", stems=S, **common, bytes_touched=nbytes, kernel_time=k,
                   torch_copy_same_bytes=c, ratio_kernel_over_copy=round(k["median_ms"] / c["median_ms"], 4), kernel_time_beside_poly=k2,
                   svs_resample_poly_same_stems=p, ratio_kernel_over_poly=round(k2["median_ms"] / p["median_ms"], 4))

    a, b = timed_pair(lambda: out_default(sep), lambda: out_fullband(sep, aux), reps)
    yield dict(kind="way_out", subtype="PCM_16", stems=2, **common, default_fused_encode=a, fullband_mask=b,
               ratio_fullband_over_default=round(b["median_ms"] / a["median_ms"], 4))
    a, b = timed_pair(lambda: out_default(separated()[0]), lambda: out_fullband(*separated()), max(3, reps // 3), warmup=2)
    yield dict(kind="end_to_end", precision="fp32", subtype="PCM_16", stems=2, **common, flag_off=a, flag_on_mask=b,
               ratio_on_over_off=round(b["median_ms"] / a["median_ms"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fullband_bench.py needs a ROCm device: nothing here is measured on a CPU")
    import datetime
    rows = []
    for row in rows_of(a.seconds, a.rate, a.reps):
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
