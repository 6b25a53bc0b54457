#!/usr/bin/env python3
"""The multichannel Wiener filter on tools/stream_bench.py's case (240 s of stereo) at the three windows: one process, warm-up, HIP
events, median of --reps.

    python tools/wiener_bench.py [--seconds 240] [--reps 30] [--out profiles/wiener_240s.jsonl]

Kernel rows, per window (512 / 384, 1024 / 768, 2048 / 1536): one model pass without a previous model (svs_wiener_model: the model
kernel and its reduction), one with, and one stems pass for both stems (svs_wiener_stems), on the tiles and phasors of that signal
with a uniform random mask; each beside a torch device copy that moves as many bytes as the pass reads plus writes, the two
alternating inside every repetition.  The ratio is reported, not gated.
End-to-end rows: separate_waveform at wiener_iters 0 / 1 / 2 with the closed-form checkpoint in bf16, for one stem and for both.
One JSON object per line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import _lib, synth  # noqa: E402
from svs_unet_pytorch_amd import data as svs_data  # noqa: E402
from svs_unet_pytorch_amd import wiener as wn  # noqa: E402
from svs_unet_pytorch_amd.config import INPUT_LEN  # noqa: E402
from tools._benchlib import closed_form_model, copy_of, timed, timed_pair  # noqa: E402

WINDOWS = ((512, 384), (1024, 768), (2048, 1536))


def kernel_rows(y, reps):
    L, S = _lib.lib(), _lib.stream_ptr
    for n_fft, hop in WINDOWS:
        tiles, phase, norm, T = svs_data.stft_to_tiles(y, n_fft, hop, INPUT_LEN)
        C, n_tiles, _, rows, seg = tiles.shape
        for c in range(C):
            _lib.check(L.svs_scale_by_inv(tiles[c].data_ptr(), tiles[c].numel(), norm[c:].data_ptr(), 1.0, S()), "svs_scale_by_inv")
        mask = torch.rand_like(tiles)
        scale = wn.common_scale(norm)
        ph = svs_data.phase_floats(phase)
        one = n_tiles * rows * seg
        first = wn.wiener_model(tiles, mask, phase, scale, T)
        v, R = torch.empty_like(first[0]), torch.empty_like(first[1])
        ws = torch.empty(int(L.svs_wiener_workspace_bytes(C, rows, seg, T)), dtype=torch.uint8, device="cuda")
        smag = torch.empty((2, C) + tuple(tiles.shape[1:]), device="cuda")
        sph = torch.empty((2,) + tuple(ph.shape), device="cuda")

        def model(prev):
            vp, Rp = (None, None) if prev is None else prev
            _lib.check(L.svs_wiener_model(tiles.data_ptr(), one, seg, rows, mask.data_ptr(), ph.data_ptr(), scale.data_ptr(), C, T,
                                          _lib.ptr(vp), one, _lib.ptr(Rp), wn.EPS, wn.REG, v.data_ptr(), one, R.data_ptr(), ws.data_ptr(),
                                          ws.numel(), S()), "svs_wiener_model")

        def stems():
            _lib.check(L.svs_wiener_stems(tiles.data_ptr(), one, seg, rows, ph.data_ptr(), scale.data_ptr(), C, T, first[0].data_ptr(), one,
                                          first[1].data_ptr(), wn.REG, 2, smag.data_ptr(), one, C * one, sph.data_ptr(), ph.numel(), S()),
                       "svs_wiener_stems")

        # bytes: tiles are read whole (padding included), phasors without the DC bin; partial sums and R are noise beside them
        tile_b, ph_b = C * one * 4, C * T * rows * 8
        passes = (("svs_wiener_model, first update", lambda: model(None), 2 * tile_b + ph_b + 2 * one * 4),
                  ("svs_wiener_model, later update", lambda: model(first), tile_b + 2 * one * 4 + ph_b + 2 * one * 4),
                  ("svs_wiener_stems, both stems", stems, tile_b + 2 * one * 4 + ph_b + 2 * tile_b + 2 * sph[0].numel() * 4))
        for name, fn, nbytes in passes:
            k, c = timed_pair(fn, copy_of(nbytes), reps)
            yield dict(kind="kernel", kernel=name, n_fft=n_fft, hop=hop, frames=T, channels=C, n_tiles=n_tiles, rows=rows, seg=seg, reps=reps,
                       bytes_moved=nbytes, kernel_time=k, torch_copy_same_bytes=c, kernel_tb_per_s=round(nbytes / k["median_ms"] / 1e9, 3),
                       copy_tb_per_s=round(nbytes / c["median_ms"] / 1e9, 3), ratio_kernel_over_copy=round(k["median_ms"] / c["median_ms"], 4))


def end_to_end_rows(y, reps):
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = closed_form_model()
    for n_fft, hop in WINDOWS if reps > 0 else ():
        for both in (False, True):
            base = None
            for iters in (0, 1, 2):
                kw = dict(n_fft=n_fft, hop=hop, precision="bf16", both_stems=both, wiener_iters=iters)
                s = timed(lambda: separate_waveform(model, y, **kw), reps)
                base = s["median_ms"] if base is None else base
                yield dict(kind="end_to_end", precision="bf16", n_fft=n_fft, hop=hop, both_stems=both, wiener_iters=iters, channels=y.shape[0],
                           samples_per_channel=y.shape[1], frames=1 + y.shape[1] // hop, separate_waveform=s,
                           over_wiener_iters_0=round(s["median_ms"] / base, 4), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--e2e_reps", type=int, default=5, help="repetitions of the end-to-end rows; 0 leaves them out (a kernel trace of the passes alone)")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wiener_bench.py needs a ROCm device: nothing here is measured on a CPU")
    n = int(a.seconds * a.rate)
    y = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    rows = []
    import datetime
    import itertools
    for row in itertools.chain(kernel_rows(y, a.reps), end_to_end_rows(y, a.e2e_reps)):
        row["seconds"] = a.seconds
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
