#!/usr/bin/env python3
"""Overlapped tiles with cross-faded masks on tools/stream_bench.py's case (240 s of stereo at the config's 1024 / 768): one process,
warm-up, HIP events, median of --reps.

    python tools/overlap_bench.py [--seconds 240] [--reps 30] [--out profiles/overlap_240s.jsonl]

Kernel rows, tile_hop 64 and 32: svs_overlap_tiles and svs_overlap_blend on the tiles of that signal (the blend on uniform random
masks), each beside a torch device copy that reads and writes as many bytes as the kernel does (the yardstick: a copy of
(read + written) / 2 bytes), the two alternating inside every repetition.  The ratio is reported, not gated.
End-to-end rows: separate_waveform at tile_hop 128 / 64 / 32 with the closed-form checkpoint, fp32 and bf16.  One JSON object per
line."""
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
from svs_unet_pytorch_amd import overlap as ov  # noqa: E402
from svs_unet_pytorch_amd.config import INPUT_LEN  # noqa: E402
from tools._benchlib import closed_form_model, copy_of, timed, timed_pair  # noqa: E402


def kernel_rows(y, reps):
    L, S = _lib.lib(), _lib.stream_ptr
    tiles, _, _, T = svs_data.stft_to_tiles(y, seg=INPUT_LEN)
    C, n_tiles, _, rows, seg = tiles.shape
    stride = n_tiles * rows * seg
    for tile_hop in (64, 32):
        n_ov = ov.overlap_count(n_tiles, seg, tile_hop)
        cut = torch.empty((C * n_ov, 1, rows, seg), device="cuda")
        masks = torch.rand((C * n_ov, 1, rows, seg), device="cuda")
        blended = torch.empty_like(tiles)
        common = dict(tile_hop=tile_hop, frames=T, channels=C, n_tiles=n_tiles, n_ov=n_ov, rows=rows, seg=seg, reps=reps)

        def run_cut():
            _lib.check(L.svs_overlap_tiles(tiles.data_ptr(), stride, C, n_tiles, rows, seg, tile_hop, cut.data_ptr(), S()), "svs_overlap_tiles")

        def run_blend():
            _lib.check(L.svs_overlap_blend(masks.data_ptr(), C, n_tiles, rows, seg, tile_hop, None, 0, 0, blended.data_ptr(), stride, S()),
                       "svs_overlap_blend")

        # the cut reads every overlapped tile's frames (seg / tile_hop times the disjoint tiles, less the ends) and writes them once
        for name, fn, nbytes in (("svs_overlap_tiles", run_cut, 2 * cut.numel() * 4),
                                 ("svs_overlap_blend", run_blend, (masks.numel() + blended.numel()) * 4)):
            k, c = timed_pair(fn, copy_of(nbytes), reps)
            yield dict(kind="kernel", kernel=name, **common, bytes_moved=nbytes, kernel_time=k, torch_copy_same_bytes=c,
                       kernel_tb_per_s=round(nbytes / k["median_ms"] / 1e9, 3), copy_tb_per_s=round(nbytes / c["median_ms"] / 1e9, 3),
                       ratio_kernel_over_copy=round(k["median_ms"] / c["median_ms"], 4))


def end_to_end_rows(y, reps):
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = closed_form_model()
    frames = 1 + y.shape[1] // 768
    n_tiles = -(-frames // INPUT_LEN)
    for precision in ("fp32", "bf16"):
        base = None
        for tile_hop in (128, 64, 32):
            s = timed(lambda: separate_waveform(model, y, precision=precision, tile_hop=tile_hop), reps)
            base = s["median_ms"] if base is None else base
            n_net = y.shape[0] * ov.overlap_count(n_tiles, INPUT_LEN, tile_hop)
            yield dict(kind="end_to_end", precision=precision, tile_hop=tile_hop, n_fft=1024, hop=768, channels=y.shape[0],
                       samples_per_channel=y.shape[1], network_tiles=n_net, separate_waveform=s,
                       over_tile_hop_128=round(s["median_ms"] / base, 4), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("overlap_bench.py needs a ROCm device: nothing here is measured on a CPU")
    n = int(a.seconds * a.rate)
    y = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    rows = []
    import datetime
    import itertools
    for row in itertools.chain(kernel_rows(y, a.reps), end_to_end_rows(y, a.reps)):
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
