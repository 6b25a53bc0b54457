#!/usr/bin/env python3
"""The optimiser options at the network's parameter count (one flat buffer of UNet()._n_params floats) and in the batch-64 train
step: one process, warm-up, HIP events, median of --reps, the two sides of every comparison alternating inside each repetition.

    python tools/optim_bench.py [--reps 30] [--out profiles/optim_b64.jsonl]

Kernel rows: svs_adam_step (the plain update, 28n bytes: p, m, v read and written, g read), svs_grad_norm (4n read; two launches),
svs_adamw_step with each option alone -- decay, clip (a coefficient below 1 in `stats`), the EMA (36n) -- and with all three, each
beside a torch device copy that moves as many bytes as the kernel has to.  Each timed call is --burst back-to-back launches divided
by their number, so these are call times with the launch gaps of a stream that is kept busy, not profiler kernel times; the buffers
(39 MB each) stay in the last-level cache between launches, for the kernels and for the copies alike.
Step rows: UNet.train_step (L1 terms, synthetic tiles) with the options off against itself -- two models, the same calls: the
run-to-run spread -- and with the options off against all three on.
One JSON object per line; ratios are reported, not gated."""
import argparse
import datetime
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import _lib, synth  # noqa: E402
from svs_unet_pytorch_amd.model import ALPHA_L1, UNet  # noqa: E402
from tools._benchlib import copy_of, timed_pair  # noqa: E402

LR, WD, D = 1e-3, 1e-2, 0.999


def per_call(stats, burst):
    return {k: round(v / burst, 5) for k, v in stats.items()}


def kernel_rows(n, reps, burst):
    L, S = _lib.lib(), _lib.stream_ptr
    dev = "cuda"
    p, m = torch.rand(n, device=dev) - 0.5, torch.zeros(n, device=dev)
    v, ema = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    g = (torch.rand(n, device=dev) - 0.5) * 0.02
    ws = torch.empty(int(L.svs_grad_norm_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    norm = float(g.double().norm())

    def adam():
        _lib.check(L.svs_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, 0.9, 0.999, 1e-8, 10, 1.0, S()), "svs_adam_step")

    def grad_norm(max_norm=0.5 * norm):
        _lib.check(L.svs_grad_norm(g.data_ptr(), n, 1.0, max_norm, stats.data_ptr(), ws.data_ptr(), ws.numel(), S()), "svs_grad_norm")

    def adamw(wd, clip, with_ema):
        def call():
            _lib.check(L.svs_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, 0.9, 0.999, 1e-8, 10, 1.0, wd,
                                        stats.data_ptr() if clip else None, ema.data_ptr() if with_ema else None, D if with_ema else 0.0, S()),
                       "svs_adamw_step")
        return call
    grad_norm()                                                  # stats[1] = 0.5: what the clip rows read
    torch.cuda.synchronize()
    assert 0.49 < stats[1].item() < 0.51
    cases = [("svs_adam_step", adam, 28), ("svs_grad_norm", grad_norm, 4), ("svs_adamw_step decay", adamw(WD, False, False), 28),
             ("svs_adamw_step clip", adamw(0.0, True, False), 28), ("svs_adamw_step ema", adamw(0.0, False, True), 36),
             ("svs_adamw_step decay + clip + ema", adamw(WD, True, True), 36),
             ("svs_grad_norm + svs_adamw_step decay + clip + ema", lambda: (grad_norm(), adamw(WD, True, True)()), 40)]
    burst_of = lambda f: (lambda: [f() for _ in range(burst)])
    adam_ms = None
    for name, fn, bytes_per_elem in cases:
        nbytes = bytes_per_elem * n
        k, c = timed_pair(burst_of(fn), burst_of(copy_of(nbytes)), reps)
        k, c = per_call(k, burst), per_call(c, burst)
        if adam_ms is None:
            adam_ms = k["median_ms"]
        yield dict(kind="kernel", call=name, n=n, bytes_per_element=bytes_per_elem, bytes_moved=nbytes, call_time=k, torch_copy_of_same_bytes=c,
                   tb_per_s=round(nbytes / k["median_ms"] / 1e9, 3), copy_tb_per_s=round(nbytes / c["median_ms"] / 1e9, 3),
                   ratio_over_copy=round(k["median_ms"] / c["median_ms"], 4), ratio_over_svs_adam_step=round(k["median_ms"] / adam_ms, 4),
                   reps=reps, burst=burst)


def step_rows(B, reps):
    mix_np, voc_np = synth.tiles(B)
    mix, voc = torch.from_numpy(mix_np).to("cuda"), torch.from_numpy(voc_np).to("cuda")

    def model_with(**options):
        model = UNet().to("cuda").train()
        for k, val in options.items():
            setattr(model.optim, k, val)
        return model
    off_a, off_b = model_with(), model_with()
    step = lambda model: (lambda: model.train_step(mix, voc, loss_scale=ALPHA_L1))
    a, b = timed_pair(step(off_a), step(off_b), reps)
    yield dict(kind="train_step", compare="options off against itself (run-to-run spread)", batch=B, first=a, second=b,
               second_over_first=round(b["median_ms"] / a["median_ms"], 4), reps=reps)
    on = model_with(weight_decay=WD, max_grad_norm=1.0, ema_decay=D)
    a, b = timed_pair(step(off_a), step(on), reps)
    stats = on.optim_stats.cpu().tolist()
    yield dict(kind="train_step", compare="options off against weight_decay + max_grad_norm + ema_decay", batch=B, options_off=a, options_on=b,
               on_over_off=round(b["median_ms"] / a["median_ms"], 4), added_ms=round(b["median_ms"] - a["median_ms"], 5), reps=reps,
               clipped_steps=int(stats[2]), skipped_steps=int(stats[3]), finite=bool(torch.isfinite(on._flat).all().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=10, help="back-to-back launches per timed kernel call")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_bench.py needs a ROCm device: nothing here is measured on a CPU")
    import itertools
    rows = []
    for row in itertools.chain(kernel_rows(UNet()._n_params, a.reps, a.burst), step_rows(a.batch, a.reps)):
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
