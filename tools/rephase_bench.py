#!/usr/bin/env python3
"""Phase refinement on tools/stream_bench.py's case (240 s of stereo), at the three windows with hop = 3 N / 4 and N / 4: one process,
warm-up, HIP events, medians of --reps.

    python tools/rephase_bench.py [--seconds 240] [--reps 20] [--e2e_reps 5] [--out profiles/rephase_240s.jsonl]

Kernel rows, per (n_fft, hop), the two alternating inside every repetition:
  (a) svs_stft_rephase_n for two stems with the mixture: three streams combined on load, only phasors written;
  (b) the composition the library offered before it: torch elementwise ops form x_s + (mix - x_0 - x_1) / 2 for both stems (four
      launches into preallocated buffers), then svs_stft_tiles_n(phase_mode=1) writes phasors AND magnitudes, into scratch tiles.
The ratio is reported, not gated.
End-to-end rows: separate_waveform at phase_iters 0 / 2 / 4 with the closed-form checkpoint, fp32 and bf16, one stem and both.
One JSON object per line."""
import argparse
import datetime
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import _lib, synth  # noqa: E402
from svs_unet_pytorch_amd.config import INPUT_LEN  # noqa: E402
from tools._benchlib import closed_form_model, timed, timed_pair  # noqa: E402

WINDOWS = (512, 1024, 2048)


def geometries():
    return [(n_fft, hop) for n_fft in WINDOWS for hop in (3 * n_fft // 4, n_fft // 4)]


def kernel_rows(y, reps):
    L, S = _lib.lib(), _lib.stream_ptr
    C, n_in = y.shape
    for n_fft, hop in geometries():
        n = hop * (n_in // hop)                                   # the length the inverse returns: hop * (T - 1)
        T, nbin, rows = 1 + n // hop, n_fft // 2 + 1, n_fft // 2
        x = torch.stack([0.6 * y[:, :n], 0.3 * y[:, :n].flip(0)]).contiguous()       # two stems that do not add up to the mixture
        mix = y[:, :n].contiguous()
        ph_a = torch.empty((2, C, T, nbin, 2), device="cuda")
        ph_b = torch.empty_like(ph_a)
        e, z = torch.empty_like(mix), torch.empty_like(x)
        n_tiles = -(-T // INPUT_LEN)
        scratch = torch.empty((2 * C, n_tiles, 1, rows, INPUT_LEN), device="cuda")

        def run_a():
            _lib.check(L.svs_stft_rephase_n(x.data_ptr(), C * n, 2, mix.data_ptr(), n, C, n_fft, hop, ph_a.data_ptr(), C * T * nbin * 2, S()),
                       "svs_stft_rephase_n")

        def run_b():
            torch.sub(mix, x[0], out=e)
            e.sub_(x[1])
            e.mul_(0.5)
            torch.add(x, e, out=z)
            _lib.check(L.svs_stft_tiles_n(z.data_ptr(), n, 2 * C, n_fft, hop, scratch.data_ptr(), n_tiles * rows * INPUT_LEN, INPUT_LEN, rows, 1,
                                          n_tiles * INPUT_LEN, ph_b.data_ptr(), 1, None, S()), "svs_stft_tiles_n")

        a, b = timed_pair(run_a, run_b, reps)
        worst = (torch.view_as_complex(ph_a) - torch.view_as_complex(ph_b)).abs().max().item()     # same transform, same phasors
        read_a, written_a = (x.numel() + mix.numel()) * 4, ph_a.numel() * 4
        yield dict(kind="kernel", n_fft=n_fft, hop=hop, frames=T, channels=C, stems=2, samples_per_channel=n, reps=reps,
                   rephase=a, composition=b, ratio_rephase_over_composition=round(a["median_ms"] / b["median_ms"], 4),
                   rephase_bytes=read_a + written_a, rephase_tb_per_s=round((read_a + written_a) / a["median_ms"] / 1e9, 3),
                   composition_bytes_written=(z.numel() + e.numel() * 3 + ph_b.numel() + scratch.numel()) * 4,
                   max_abs_phasor_difference=worst)


def end_to_end_rows(y, reps):
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = closed_form_model()
    for (n_fft, hop), precision, both in itertools.product(geometries(), ("fp32", "bf16"), (False, True)):
        base = None
        for iters in (0, 2, 4):
            kw = dict(n_fft=n_fft, hop=hop, precision=precision, both_stems=both, phase_iters=iters)
            s = timed(lambda: separate_waveform(model, y, **kw), reps)
            base = s["median_ms"] if base is None else base
            yield dict(kind="end_to_end", n_fft=n_fft, hop=hop, precision=precision, both_stems=both, phase_iters=iters, channels=y.shape[0],
                       samples_per_channel=y.shape[1], frames=1 + y.shape[1] // hop, separate_waveform=s,
                       ms_per_iteration=None if iters == 0 else round((s["median_ms"] - base) / iters, 5),
                       over_phase_iters_0=round(s["median_ms"] / base, 4), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e_reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rephase_bench.py needs a ROCm device: nothing here is measured on a CPU")
    n = int(a.seconds * a.rate)
    y = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    rows = []
    for row in itertools.chain(kernel_rows(y, a.reps), end_to_end_rows(y, a.e2e_reps)):
        row["seconds"] = a.seconds
        row["device"] = torch.cuda.get_device_name(0)
        row["date"] = datetime.date.today().isoformat()
        print(json.dumps(row), flush=True)
        rows.append(row)
        if a.out:                                                 # rewritten after every row: a run that is cut short keeps its rows
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
