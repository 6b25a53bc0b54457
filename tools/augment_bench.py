#!/usr/bin/env python3
"""Remix and gain augmentation at the training shape (B = 64, F = 512, seg = 128) on a synthetic resident set of a few songs: one
process, warm-up, HIP events, median of --reps, the two sides of every comparison alternating inside each repetition.

    python tools/augment_bench.py [--reps 30] [--out profiles/augment_b64.jsonl]

Kernel rows: svs_crop_remix_tiles with an all-remix table (with the phase tiles and without) and with an all-gain table, and the two
svs_crop_tiles launches it replaces, each beside a torch device copy that moves as many bytes as the remix reads and writes (10 tiles:
6 read, 4 written).  Each timed call is --burst back-to-back launches divided by their number, so these are call times with the
launch gaps of a stream that is kept busy, not profiler kernel times.
Step rows: UNet.train_step with the L1 terms and with the full objective, fed by ResidentSpectrograms.batches and by
augmented_batches (remix) in alternation: the host side of each feed (the draws, the table's upload) is inside the time.
One JSON object per line; ratios are reported, not gated."""
import argparse
import datetime
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import augment as au  # noqa: E402
from svs_unet_pytorch_amd import train as svs_train  # noqa: E402
from svs_unet_pytorch_amd.config import HOP_SIZE, INPUT_LEN  # noqa: E402
from svs_unet_pytorch_amd.model import ALPHA_L1, ALPHA_MR, UNet  # noqa: E402
from tools._benchlib import copy_of, timed_pair  # noqa: E402

FRAMES = (700, 431, 1024, 90, 555)                   # one song shorter than a tile


def synthetic_set(root, per_song):
    """A folder of len(FRAMES) songs at the config's window (513-row files, unit-phasor phase files) and its resident set."""
    rng = np.random.default_rng(0)
    for d in ("mixture", "vocal"):
        os.makedirs(os.path.join(root, d))
    for i, T in enumerate(FRAMES):
        mix = rng.random((513, T), dtype=np.float32)
        for d, mag in (("mixture", mix), ("vocal", mix * rng.random((513, T), dtype=np.float32))):
            np.save(os.path.join(root, d, f"{i:04d}_song_spec.npy"), mag)
            np.save(os.path.join(root, d, f"{i:04d}_song_phase.npy"), np.exp(1j * rng.uniform(-np.pi, np.pi, (513, T))).astype(np.complex64))
    return svs_train.ResidentSpectrograms(svs_train.SpectrogramDataset(root, samples_per_song=per_song), torch.device("cuda"))


def per_call(stats, burst):
    return {k: round(v / burst, 5) for k, v in stats.items()}


def kernel_rows(res, B, reps, burst):
    tile_bytes = B * res.rows * INPUT_LEN * 4
    copy = copy_of(10 * tile_bytes)
    remix = au.draw_epoch(B, res.frames_host, INPUT_LEN, 0, 0, au.GAIN_RANGE, 1.0)
    gain = au.draw_epoch(B, res.frames_host, INPUT_LEN, 0, 0, au.GAIN_RANGE, 0.0)
    t_remix, t_gain = au.upload_table(res, remix), au.upload_table(res, gain)
    t_plain = res.upload_table(remix.song_v.tolist(), remix.start_v.tolist())
    cases = [("svs_crop_remix_tiles all-remix, phase tiles", lambda: au.crop_remix(res, t_remix, 0, B, True), 10),
             ("svs_crop_remix_tiles all-remix, no phase tiles", lambda: au.crop_remix(res, t_remix, 0, B, False), 8),
             ("svs_crop_remix_tiles all-gain, phase tiles", lambda: au.crop_remix(res, t_gain, 0, B, True), 8),
             ("svs_crop_tiles x 2 (the plain path)", lambda: res.crop_table(t_plain, 0, B, True), 8)]
    burst_of = lambda f: (lambda: [f() for _ in range(burst)])
    for name, fn, tiles_moved in cases:
        k, c = timed_pair(burst_of(fn), burst_of(copy), reps)
        k, c = per_call(k, burst), per_call(c, burst)
        yield dict(kind="kernel", call=name, batch=B, rows=res.rows, seg=INPUT_LEN, tiles_moved=tiles_moved, bytes_moved=tiles_moved * tile_bytes,
                   call_time=k, torch_copy_of_10_tiles=c, tb_per_s=round(tiles_moved * tile_bytes / k["median_ms"] / 1e9, 3),
                   copy_tb_per_s=round(10 * tile_bytes / c["median_ms"] / 1e9, 3), ratio_over_copy=round(k["median_ms"] / c["median_ms"], 4),
                   reps=reps, burst=burst)


def step_rows(res, B, reps):
    aug = au.Augment("remix", au.GAIN_RANGE, au.REMIX_PROB, 0)

    def feed(make):
        epoch = 0
        while True:
            yield from make(epoch)
            epoch += 1
    for objective in ("l1", "full"):
        full = objective == "full"
        model = UNet().to("cuda").train()
        plain = feed(lambda ep: res.batches(B, True, 0, 1, ep, with_phase=full))
        remixed = feed(lambda ep: res.augmented_batches(B, 0, 1, ep, with_phase=full, aug=aug))

        def step(source):
            t = next(source)
            while t[0].shape[0] != B:                 # (a short last batch would be another shape: not what is timed)
                t = next(source)
            if full:
                model.train_step(t[0], t[1], loss_scale=ALPHA_L1, mix_phase=t[2], voc_phase=t[3], alpha_mr=ALPHA_MR, hop=HOP_SIZE)
            else:
                model.train_step(t[0], t[1], loss_scale=ALPHA_L1)
        p, a = timed_pair(lambda: step(plain), lambda: step(remixed), reps)
        yield dict(kind="train_step", objective=objective, batch=B, rows=res.rows, seg=INPUT_LEN, fed_by_batches=p, fed_by_augmented_batches=a,
                   augmented_over_plain=round(a["median_ms"] / p["median_ms"], 4), reps=reps,
                   finite=bool(torch.isfinite(model._flat).all().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=10, help="back-to-back launches per timed kernel call")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_bench.py needs a ROCm device: nothing here is measured on a CPU")
    rows = []
    with tempfile.TemporaryDirectory() as root:
        res = synthetic_set(root, per_song=a.batch)
    import itertools
    for row in itertools.chain(kernel_rows(res, a.batch, a.reps, a.burst), step_rows(res, a.batch, a.reps)):
        row["songs"] = list(FRAMES)
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
