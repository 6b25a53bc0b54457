#!/usr/bin/env python3
"""A validation pass, the host loop against the on-device pass, on one synthetic folder in one process.

    python tools/valid_bench.py [--songs 14] [--frames 2560] [--samples_per_song 64] [--batch 64] [--passes 5]
                                [--out profiles/valid_pass.jsonl]

Writes a validation folder from `synth.song` (magnitudes and unit-phasor files, as data.py writes them, at 1024 / 768) into a
temporary directory, then alternates whole passes of
  * the host loop that stays in train.py for SVS_DATA_LOADER != resident: SpectrogramDataset + DataLoader(num_workers=2,
    shuffle=False, pin_memory=True) + l1_terms / mr_term with their two float() reads per batch, and
  * train.validation_pass on a ResidentSpectrograms of the same folder (one svs_crop_tiles per tile pair and one
    svs_unet_eval_loss per batch, one read-back per pass),
each warmed once and timed with a host clock around work that ends in a device synchronise; median and best of --passes
(at least 5) passes each.  Also the device time of one UNet.eval_losses call at B = 64 (HIP events over back-to-back calls:
launch gaps included) and the one-off cost of making the folder resident.  Appends one JSON line to --out.  The two paths draw
different random starts (the loader's workers draw their own); both see every item once per pass.
"""
import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.utils.data as Data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import synth  # noqa: E402
from svs_unet_pytorch_amd import train as svs_train  # noqa: E402
from svs_unet_pytorch_amd.config import HOP_SIZE, INPUT_LEN, WINDOW_SIZE  # noqa: E402
from svs_unet_pytorch_amd.model import ALPHA_L1, ALPHA_MR  # noqa: E402
from tools._benchlib import closed_form_model  # noqa: E402


def write_folder(root, songs, frames):
    os.makedirs(os.path.join(root, "mixture")), os.makedirs(os.path.join(root, "vocal"))
    for n in range(songs):
        mix, voc, pm, pv = synth.song(n, frames)
        base = f"{n:04d}_synth"
        for track, mag, ph in (("mixture", mix, pm), ("vocal", voc, pv)):
            np.save(os.path.join(root, track, f"{base}_spec.npy"), mag)
            np.save(os.path.join(root, track, f"{base}_phase.npy"), ph)


def host_pass(model, loader, device):
    """The validation loop of train.py's main() for SVS_DATA_LOADER != resident, as it stands there."""
    val_sum = 0.0
    with torch.no_grad():
        for mix, voc, mph, vph in loader:
            mix, voc = mix.to(device), voc.to(device)
            val_sum += ALPHA_L1 * float(svs_train.l1_terms(model, mix, voc))
            val_sum += ALPHA_MR * float(svs_train.mr_term(model, mix, voc, mph.to(device), vph.to(device), WINDOW_SIZE, HOP_SIZE))
    torch.cuda.synchronize()
    return val_sum / len(loader)


def device_pass(model, resident, batch, rng):
    with torch.no_grad():
        acc, n = svs_train.validation_pass(model, resident, batch, True, WINDOW_SIZE, HOP_SIZE, rng)
    value = float(acc.cpu()[0]) / n            # the pass's one read-back
    torch.cuda.synchronize()
    return value


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    value = fn()
    return (time.perf_counter() - t0) * 1e3, value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=14)
    ap.add_argument("--frames", type=int, default=2560)
    ap.add_argument("--samples_per_song", type=int, default=svs_train.SAMPLES_PER_SONG)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "valid_pass.jsonl"))
    a = ap.parse_args()
    if a.passes < 5:
        ap.error("--passes: at least 5 (median and best are reported)")
    if not torch.cuda.is_available():
        raise SystemExit("valid_bench.py needs a ROCm device: nothing is timed without one.")
    device = torch.device("cuda")
    root = tempfile.mkdtemp(prefix="svs_valid_bench_")
    try:
        write_folder(root, a.songs, a.frames)
        dataset = svs_train.SpectrogramDataset(root, samples_per_song=a.samples_per_song)
        loader = Data.DataLoader(dataset, batch_size=a.batch, num_workers=2, shuffle=False, pin_memory=True)
        model = closed_form_model(device)
        upload_ms, resident = clocked(lambda: svs_train.ResidentSpectrograms(dataset, device))
        torch.cuda.synchronize()
        rng = random.Random(0)
        host_pass(model, loader, device), device_pass(model, resident, a.batch, rng)            # warm each once
        host_ms, dev_ms, host_val, dev_val = [], [], [], []
        for _ in range(a.passes):                                                               # alternating
            ms, v = clocked(lambda: host_pass(model, loader, device))
            host_ms.append(ms), host_val.append(v)
            ms, v = clocked(lambda: device_pass(model, resident, a.batch, rng))
            dev_ms.append(ms), dev_val.append(v)
        # one eval_losses call at B = 64 on the device
        songs, starts = resident.draw(range(64), rng)
        tiles = resident.crop(songs, starts, with_phase=True)
        acc = torch.zeros(3, dtype=torch.float64, device=device)
        call = lambda: model.eval_losses(*tiles, hop=HOP_SIZE, acc=acc)
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            call()
        e1.record()
        torch.cuda.synchronize()
        call_ms = e0.elapsed_time(e1) / 20
    finally:
        shutil.rmtree(root, ignore_errors=True)
    rec = {"songs": a.songs, "frames": a.frames, "items": len(dataset), "batch": a.batch, "batches": len(loader), "passes": a.passes,
           "tile": [WINDOW_SIZE // 2, INPUT_LEN], "hop": HOP_SIZE,
           "host_loop_ms": {"median": round(statistics.median(host_ms), 2), "best": round(min(host_ms), 2), "all": [round(x, 2) for x in host_ms]},
           "device_pass_ms": {"median": round(statistics.median(dev_ms), 2), "best": round(min(dev_ms), 2), "all": [round(x, 2) for x in dev_ms]},
           "speedup_median": round(statistics.median(host_ms) / statistics.median(dev_ms), 2),
           "eval_losses_b64_ms": round(call_ms, 4), "make_resident_ms": round(upload_ms, 1),
           "host_loop_val": host_val[-1], "device_pass_val": dev_val[-1],
           "cpus": len(os.sched_getaffinity(0)), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    if rec["device_pass_ms"]["median"] >= rec["host_loop_ms"]["median"]:
        raise SystemExit("the on-device pass was not faster than the host loop")


if __name__ == "__main__":
    main()
