#!/usr/bin/env python3
"""Training at the three STFT windows (512 / 1024 / 2048): one JSON line per window at B = 64, W = 128, hop = 3 n_fft / 4,
timed with HIP events over back-to-back calls (the manner of tools/signal_bench.py: `timed`).

    python tools/train_windows_bench.py [--batch 64] [--out profiles/train_windows_b64.jsonl]

Per window: svs_istft_bwd_mask (the transpose of specific_istft fused with the mask's chain rule) with its algorithmic bytes
and GB/s, specific_istft (one waveform batch), the MR-STFT loss with its gradient, and the whole train_step (forward, losses,
backward, Adam) with the full objective and with the L1 terms only.  Algorithmic bytes of the adjoint: d_wav read; angle / mix /
mask read; d_logit read and written.  The numbers are call times (launch gaps included), not profiler kernel times.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import _lib, synth  # noqa: E402
from svs_unet_pytorch_amd.model import ALPHA_L1, ALPHA_MR, UNet  # noqa: E402


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def adjoint_bytes(B, n_fft, hop, W):
    tile = B * (n_fft // 2) * W * 4
    return B * hop * (W - 1) * 4 + 3 * tile + 2 * tile


def window_record(n_fft, B=64, W=128):
    H, hop, dev = n_fft // 2, 3 * n_fft // 4, "cuda"
    L, S = _lib.lib(), _lib.stream_ptr
    Ls = hop * (W - 1)
    rnd = lambda seed, lo, hi: torch.from_numpy((synth.uniform(seed, B * H * W) * (hi - lo) + lo).astype(np.float32).reshape(B, 1, H, W)).to(dev)
    mix_np, voc_np = synth.tiles(B, H, W, first_tile=800)
    mix, voc = torch.from_numpy(mix_np).to(dev), torch.from_numpy(voc_np).to(dev)
    mph, vph, mask = rnd(30, -np.pi, np.pi), rnd(31, -np.pi, np.pi), rnd(11, 0.1, 0.9)
    d_wav = torch.from_numpy((synth.uniform(8, B * Ls) - 0.5).reshape(B, Ls)).to(dev)
    d_logit = torch.zeros((B, 1, H, W), device=dev)
    wav_a, wav_b = torch.empty((B, Ls), device=dev), torch.empty((B, Ls), device=dev)
    loss = torch.empty(1, device=dev)
    mr_ws = torch.empty(int(L.svs_mrstft_workspace_bytes(B, Ls)) + 4096, dtype=torch.uint8, device=dev)

    def adjoint():
        _lib.check(L.svs_istft_bwd_mask(d_wav.data_ptr(), mph.data_ptr(), mix.data_ptr(), mask.data_ptr(), d_logit.data_ptr(), 1.0, B, n_fft,
                                        hop, W, S()), "svs_istft_bwd_mask")

    def inverse(src=mix, ang=mph, out=wav_a):
        _lib.check(L.svs_istft_tiles_n(src.data_ptr(), H * W, W, H, 1, None, 0, ang.data_ptr(), 3, B, n_fft, hop, W, out.data_ptr(), None, S()),
                   "svs_istft_tiles_n")

    def mr_loss():
        _lib.check(L.svs_mrstft_loss_fwd_bwd(wav_a.data_ptr(), wav_b.data_ptr(), B, Ls, 1.0, loss.data_ptr(), d_wav.data_ptr(), mr_ws.data_ptr(),
                                             mr_ws.numel(), S()), "svs_mrstft_loss_fwd_bwd")

    inverse()
    inverse(voc, vph, wav_b)
    rec = {"n_fft": n_fft, "hop": hop, "batch": B, "tile": [H, W], "wave_samples": Ls}
    ms = timed(adjoint)
    nbytes = adjoint_bytes(B, n_fft, hop, W)
    rec["istft_bwd_mask_ms"], rec["istft_bwd_mask_bytes"] = round(ms, 4), nbytes
    rec["istft_bwd_mask_GBps"] = round(nbytes / ms / 1e6, 1)
    rec["specific_istft_ms"] = round(timed(inverse), 4)
    rec["mrstft_loss_ms"] = round(timed(mr_loss), 4)         # (after the adjoint: it overwrites d_wav with its gradient)
    model = UNet().to(dev).train()
    full = lambda: model.train_step(mix, voc, loss_scale=ALPHA_L1, mix_phase=mph, voc_phase=vph, alpha_mr=ALPHA_MR, hop=hop)
    l1 = lambda: model.train_step(mix, voc, loss_scale=ALPHA_L1)
    rec["train_step_full_ms"] = round(timed(full, reps=10), 3)
    rec["train_step_l1_ms"] = round(timed(l1, reps=10), 3)
    rec["finite"] = bool(torch.isfinite(model._flat).all().item() and torch.isfinite(model.last_mr_loss if model.last_mr_loss is not None else loss).all().item())
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_windows_bench.py needs a ROCm device: nothing is timed without one.")
    lines = []
    for n_fft in (512, 1024, 2048):
        lines.append(json.dumps(window_record(n_fft, a.batch)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
