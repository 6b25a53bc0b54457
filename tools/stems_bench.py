#!/usr/bin/env python3
"""Two-stem inverse STFT against two single-stem launches, and separate_waveform(both_stems=True) against the two single-stem
calls: one process, warm-up, HIP events, the two sides alternating inside every repetition, median of --reps.

    python tools/stems_bench.py [--seconds 240] [--reps 30] [--out profiles/istft_stems_240s.jsonl]

Kernel rows: stereo signal at the network rate (8,192 Hz), windows 512 / 1024 / 2048 at hops 3n/4 (two frames per sample) and n/4
(general overlap-add), 128-frame network tiles, a uniform random mask, frame-major phasors, peak partials written by both sides.
End-to-end rows: the config's 1024 / 768 with the closed-form checkpoint at fp32 and bf16.  One JSON object per line."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import _lib, synth  # noqa: E402
from svs_unet_pytorch_amd import data as svs_data  # noqa: E402
from svs_unet_pytorch_amd.config import SAMPLE_RATE  # noqa: E402
from tools._benchlib import closed_form_model, timed_pair  # noqa: E402


def kernel_rows(n, reps):
    L, S = _lib.lib(), _lib.stream_ptr
    y = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    for n_fft in (512, 1024, 2048):
        for hop in (3 * n_fft // 4, n_fft // 4):
            tiles, phase, _, T = svs_data.stft_to_tiles(y, n_fft, hop, 128)
            C, n_tiles, _, rows, seg = tiles.shape
            mask = torch.rand_like(tiles)
            ph = svs_data.phase_floats(phase)
            n_out = hop * (T - 1)
            out2 = torch.empty((2, C, n_out), device="cuda")
            out1 = torch.empty((2, C, n_out), device="cuda")
            g2 = L.svs_istft_stems_groups_n(n_fft, hop, T, C)
            g1 = L.svs_istft_groups_n(n_fft, hop, T, C)
            p2 = torch.empty((2, C, g2), device="cuda")
            p1 = torch.empty((2, C, g1), device="cuda")

            def stems():
                _lib.check(L.svs_istft_stems_n(tiles.data_ptr(), n_tiles * rows * seg, seg, rows, 1, mask.data_ptr(), ph.data_ptr(), 1, C, n_fft, hop,
                                               T, out2.data_ptr(), C * n_out, p2.data_ptr(), S()), "svs_istft_stems_n")

            def two_launches():
                for s in range(2):
                    _lib.check(L.svs_istft_tiles_n(tiles.data_ptr(), n_tiles * rows * seg, seg, rows, 1, mask.data_ptr(), s, ph.data_ptr(), 1, C, n_fft,
                                                   hop, T, out1[s].data_ptr(), p1[s].data_ptr(), S()), "svs_istft_tiles_n")

            a, b = timed_pair(stems, two_launches, reps)
            err = ((out2 - out1).abs().amax() / out1.abs().amax()).item()
            hops, rounds, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
            _lib.check(L.svs_istft_stems_plan_n(n_fft, hop, ctypes.byref(hops), ctypes.byref(rounds), ctypes.byref(lds)), "svs_istft_stems_plan_n")
            yield dict(kind="kernel", n_fft=n_fft, hop=hop, frames=T, channels=C, samples_per_channel=n, hops_per_block=hops.value,
                       rounds=rounds.value, lds_bytes=lds.value, blocks=g2 * C, svs_istft_stems_n=a, two_svs_istft_tiles_n=b,
                       ratio=round(a["median_ms"] / b["median_ms"], 4), max_rel_diff=err, reps=reps)


def end_to_end_rows(n, reps):
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = closed_form_model()
    y = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    for precision in ("fp32", "bf16"):
        res = {}

        def both():
            res["both"] = separate_waveform(model, y, precision=precision, both_stems=True)

        def two_calls():
            res["two"] = [separate_waveform(model, y, vocal_solo=v, precision=precision) for v in (True, False)]

        a, b = timed_pair(both, two_calls, reps, warmup=3)
        err = max(((res["both"][s] - res["two"][s]).abs().amax() / res["two"][s].abs().amax()).item() for s in range(2))
        yield dict(kind="end_to_end", precision=precision, n_fft=1024, hop=768, channels=2, samples_per_channel=n,
                   separate_waveform_both_stems=a, two_separate_waveform_calls=b, ratio=round(a["median_ms"] / b["median_ms"], 4),
                   max_rel_diff=err, reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stems_bench.py needs a ROCm device: nothing here is measured on a CPU")
    n = int(a.seconds * SAMPLE_RATE)
    rows = []
    import itertools
    for row in itertools.chain(kernel_rows(n, a.reps), end_to_end_rows(n, a.reps)):
        row["seconds"] = a.seconds
        row["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
