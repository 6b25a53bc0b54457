#!/usr/bin/env python3
"""Pitch-shift augmentation at the training shape (B = 64, F = 512, seg = 128) on a synthetic resident set of a few songs: one
process, warm-up, HIP events, median of --reps, the two sides of every comparison alternating inside each repetition.

    python tools/pitch_bench.py [--reps 30] [--out profiles/pitch_b64.jsonl]

Kernel rows: one svs_crop_pitch_tiles launch (all-remix table, pitches in -2 .. 2 semitones with rates in 0.8 .. 1.25, with the
phase tiles and without; the same pitches at rate 1; the ends of the range, -12 .. 12 semitones; and every pitch at 1024) beside one
svs_crop_stretch_tiles launch on the same items (the same table without its two pitch rows) and beside a torch device copy that
moves as many bytes as the remix reads and writes (10 tiles: 6 read, 4 written; the pitch shift reads its six source planes at two
bins each).  Each timed call is --burst back-to-back launches divided by their number: call times with the launch gaps of a stream
that is kept busy, not profiler kernel times.
Step rows: UNet.train_step with the L1 terms and with the full objective, fed by augmented_batches with a pitch range and a stretch
range beside augmented_batches with the stretch range alone, and the stretch feed beside a second stretch feed -- the spread the
first ratio is read against.  The host side of each feed (the draws, the table's upload) is inside the time.
One JSON object per line; nothing is gated."""
import argparse
import datetime
import itertools
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import augment as au  # noqa: E402
from svs_unet_pytorch_amd.config import HOP_SIZE, INPUT_LEN, WINDOW_SIZE  # noqa: E402
from svs_unet_pytorch_amd.model import ALPHA_L1, ALPHA_MR, UNet  # noqa: E402
from tools._benchlib import copy_of, timed_pair  # noqa: E402
from tools.augment_bench import FRAMES, per_call, synthetic_set  # noqa: E402


def kernel_rows(res, B, reps, burst):
    tile_bytes = B * res.rows * INPUT_LEN * 4
    copy = copy_of(10 * tile_bytes)
    draw = lambda pitch, stretch: au.draw_epoch_pitch(B, res.frames_host, INPUT_LEN, 0, 0, au.GAIN_RANGE, 1.0, pitch, stretch)
    burst_of = lambda f: (lambda: [f() for _ in range(burst)])
    cases = [("svs_crop_pitch_tiles all-remix, -2 .. 2 semitones, rates 0.8 .. 1.25, phase tiles", draw(au.PITCH_RANGE, au.STRETCH_RANGE), True),
             ("svs_crop_pitch_tiles all-remix, -2 .. 2 semitones, rates 0.8 .. 1.25, no phase tiles", draw(au.PITCH_RANGE, au.STRETCH_RANGE), False),
             ("svs_crop_pitch_tiles all-remix, -2 .. 2 semitones, rate 1, phase tiles", draw(au.PITCH_RANGE, None), True),
             ("svs_crop_pitch_tiles all-remix, -12 .. 12 semitones, rates 0.8 .. 1.25, phase tiles", draw((-12.0, 12.0), au.STRETCH_RANGE), True),
             ("svs_crop_pitch_tiles all-remix, pitch 1, rates 0.8 .. 1.25, phase tiles", draw((0.0, 0.0), au.STRETCH_RANGE), True)]
    for name, drawn, phase in cases:
        t_pitch = au.upload_pitch_table(res, drawn)
        t_stretch = au.upload_stretch_table(res, au.StretchTable(*drawn[:8]))                      # the same items, unshifted
        fn = lambda: au.crop_pitch(res, t_pitch, 0, B, WINDOW_SIZE, HOP_SIZE, phase)
        stretch = lambda: au.crop_stretch(res, t_stretch, 0, B, WINDOW_SIZE, HOP_SIZE, phase)
        k, s = timed_pair(burst_of(fn), burst_of(stretch), reps)
        _, c = timed_pair(burst_of(fn), burst_of(copy), reps)
        k, s, c = per_call(k, burst), per_call(s, burst), per_call(c, burst)
        yield dict(kind="kernel", call=name, batch=B, rows=res.rows, seg=INPUT_LEN, n_fft=WINDOW_SIZE, hop=HOP_SIZE, call_time=k,
                   svs_crop_stretch_tiles_same_items=s, torch_copy_of_10_tiles=c, ratio_over_stretch=round(k["median_ms"] / s["median_ms"], 4),
                   ratio_over_copy=round(k["median_ms"] / c["median_ms"], 4), elements_per_us=round(B * res.rows * INPUT_LEN / k["median_ms"] / 1e3, 1),
                   reps=reps, burst=burst)


def step_rows(res, B, reps):
    stretch_aug = au.Augment("remix", au.GAIN_RANGE, au.REMIX_PROB, 0, au.STRETCH_RANGE)
    pitch_aug = au.Augment("remix", au.GAIN_RANGE, au.REMIX_PROB, 0, au.STRETCH_RANGE, au.PITCH_RANGE)

    def feed(aug, full):
        epoch = 0
        while True:
            yield from res.augmented_batches(B, 0, 1, epoch, with_phase=full, aug=aug, hop=HOP_SIZE)
            epoch += 1
    for objective in ("l1", "full"):
        full = objective == "full"
        model = UNet().to("cuda").train()
        stretched, stretched_again, shifted = feed(stretch_aug, full), feed(stretch_aug, full), feed(pitch_aug, full)

        def step(source):
            t = next(source)
            while t[0].shape[0] != B:                 # (a short last batch would be another shape: not what is timed)
                t = next(source)
            if full:
                model.train_step(t[0], t[1], loss_scale=ALPHA_L1, mix_phase=t[2], voc_phase=t[3], alpha_mr=ALPHA_MR, hop=HOP_SIZE)
            else:
                model.train_step(t[0], t[1], loss_scale=ALPHA_L1)
        s, p = timed_pair(lambda: step(stretched), lambda: step(shifted), reps)
        s1, s2 = timed_pair(lambda: step(stretched), lambda: step(stretched_again), reps)
        yield dict(kind="train_step", objective=objective, batch=B, rows=res.rows, seg=INPUT_LEN, fed_by_stretch=s, fed_by_pitch_and_stretch=p,
                   pitch_over_stretch=round(p["median_ms"] / s["median_ms"], 4), stretch_run_1=s1, stretch_run_2=s2,
                   stretch_over_stretch=round(s2["median_ms"] / s1["median_ms"], 4), reps=reps,
                   finite=bool(torch.isfinite(model._flat).all().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=10, help="back-to-back launches per timed kernel call")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pitch_bench.py needs a ROCm device: nothing here is measured on a CPU")
    rows = []
    with tempfile.TemporaryDirectory() as root:
        res = synthetic_set(root, per_song=a.batch)
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
