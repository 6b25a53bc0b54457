"""Inference driver -- same command line and file conventions as the reference's inference.py
(/root/reference/inference.py:29-34, 56-127), with the per-tile loop replaced by ONE batched forward.

    python -m svs_unet_pytorch_amd.inference --model_path CKPT/svs_x.pth --mixture_folder spec/mixture \
        --tar spec/pred [--vocal_solo 0|1] [--tile_hop 128|64|32]

Per file: load (513, T) -> drop the DC row (inference.py:68) -> cut into T//INPUT_LEN + 1 segments of
INPUT_LEN frames, skipping an empty last one and right-zero-padding a short one (inference.py:75-92)
-> mask = UNet(tile) (inference.py:100) -> optionally 1-mask (inference.py:102) -> mix*mask
(inference.py:107) -> crop the padding (inference.py:113-114) -> concatenate (inference.py:120) ->
put a zero float32 row back on top (inference.py:123) -> save under the same name (inference.py:126-127).
Tiles are independent in eval mode, so all segments of a file go through the network as one batch and
stay on the GPU until the finished spectrogram is copied back once (the reference copies every tile).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from .config import INPUT_LEN
from .model import UNet
from .overlap import check_tile_hop


def segment_plan(n_frames: int, seg_len: int = INPUT_LEN):
    """[(start, end, pad)] of the non-empty segments, in order (inference.py:75-92)."""
    plan = []
    for i in range(n_frames // seg_len + 1):
        start = i * seg_len
        end = min(start + seg_len, n_frames)
        if end > start:
            plan.append((start, end, seg_len - (end - start)))
    return plan


@torch.no_grad()
def separate(model: UNet, mix_spec, seg_len: int = INPUT_LEN, vocal_solo: bool = True, max_batch: int = 256,
             tile_hop: int | None = None):
    """(F+1, T) mixture magnitude (numpy or tensor) -> (F+1, T) float32 numpy array, or None for a spectrogram with no frames:
    the host wrapper of streaming.separate_spectrogram_device, whose arguments these are."""
    from .streaming import separate_spectrogram_device
    spec = torch.as_tensor(np.asarray(mix_spec)).to(torch.float32)
    if spec.shape[1] == 0:
        return None
    return separate_spectrogram_device(model, spec.to(model._flat.device), seg_len, vocal_solo, max_batch, tile_hop).cpu().numpy()


def no_ema_message(tool: str, path: str) -> str:
    return (f"{tool}: --ema: {path} has no ema_state_dict (only the resume checkpoint of a `train.py --ema_decay` run has one; the "
            "best-validation checkpoint of such a run already carries the EMA weights as its model_state_dict: load it without --ema)")


def load_checkpoint_model(path: str, device, ema: bool = False, tool: str = "inference.py"):
    """A UNet on `device` in eval mode with the checkpoint's model_state_dict -- with `ema`, its ema_state_dict (the resume
    checkpoint of `train.py --ema_decay`), and the process ends with a message when it has none; a checkpoint that does not load
    is reported and ends the process with status 1 (inference.py:49-51)."""
    model = UNet().to(device)
    try:
        checkpoint = torch.load(path, map_location=device)
        if ema and not (isinstance(checkpoint, dict) and "ema_state_dict" in checkpoint):
            raise SystemExit(no_ema_message(tool, path))
        if ema:
            model.load_state_dict(checkpoint["ema_state_dict"])
        elif isinstance(checkpoint, dict) and "model_state_dict" in checkpoint:
            model.load_state_dict(checkpoint["model_state_dict"])
    except Exception as e:
        print(f"Failed to load the model: {e}")
        sys.exit(1)
    return model.eval()


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--model_path", type=str, required=True)
    parser.add_argument("--tar", type=str, required=True)
    parser.add_argument("--mixture_folder", type=str, required=True)
    parser.add_argument("--vocal_solo", type=int, default=1, help="1: keep the vocal, 0: remove it")
    parser.add_argument("--tile_hop", type=int, default=INPUT_LEN,
                        help=f"frames between tiles: {INPUT_LEN} = disjoint tiles as the reference cuts them; 64 or 32 = overlapped tiles with cross-faded masks")
    parser.add_argument("--ema", action="store_true", help="load the checkpoint's ema_state_dict (train.py --ema_decay) instead of its live weights")
    args = parser.parse_args(argv)
    try:
        check_tile_hop(args.tile_hop, INPUT_LEN)
    except ValueError as e:
        parser.error(f"--tile_hop: {e}")

    os.makedirs(args.tar, exist_ok=True)
    if not torch.cuda.is_available():
        print("Inference needs a ROCm device (hand-written gfx950 kernels, no CPU path).")
        sys.exit(1)
    device = torch.device("cuda")
    print(f"Inference using device: {device}")

    model = load_checkpoint_model(args.model_path, device, ema=args.ema)

    files = sorted(f for f in os.listdir(args.mixture_folder) if f.endswith("_spec.npy"))[:20]   # inference.py:58-59
    print(f"Found {len(files)} files, separating...")
    for name in files:
        mix = np.load(os.path.join(args.mixture_folder, name))
        pred = separate(model, mix, INPUT_LEN, bool(args.vocal_solo), tile_hop=args.tile_hop)
        if pred is not None:
            np.save(os.path.join(args.tar, name), pred)
    print("Separation finished!")


if __name__ == "__main__":
    main()
