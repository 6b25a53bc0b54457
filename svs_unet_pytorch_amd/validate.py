"""Validation loss of a checkpoint without training: the validation loop of train.py (the reference's train.py:317-363) on its
own, from the HBM-resident set -- `train.validation_pass`: one `svs_crop_tiles` and one `svs_unet_eval_loss` per batch, one
read-back per pass.  This is how two checkpoints are compared on the same folder.

    python -m svs_unet_pytorch_amd.validate --model_path CKPT/svs_x.pth --valid_folder spec/valid \
        [--batch_size 64] [--win_size 512|1024|2048] [--hop_size N] [--seed N] [--passes K] [--ema]

The STFT geometry defaults to the one the checkpoint records (`win_size` / `hop_size`, written by train.py; the config's
1024 / 768 for a checkpoint from before those keys); a flag that contradicts the checkpoint is an error, and so are a
geometry that is not built, a missing or empty folder and a folder written at another window -- all of them before any
device is touched.  A pass draws its crops from `random.Random(seed)`, one generator for the K passes: the same seed gives
the same items, starts and values.  Per pass it prints the objective ALPHA_L1 * L1 + ALPHA_MR * MR-STFT (the `Val` value
train.py logs: the mean of per-batch totals) and its two parts, then their means over the passes; `main()` returns them.  A
folder without *_phase.npy files is scored on the L1 part only, with a warning (MR = 0).  The fp32 network always.
--ema scores the checkpoint's `ema_state_dict` (the resume checkpoint of `train.py --ema_decay`) and exits with a message when
it has none.
"""
from __future__ import annotations

import argparse
import random
import sys

import torch

from .model import ALPHA_L1, ALPHA_MR, UNet
from .train import ResidentSpectrograms, SpectrogramDataset, check_geometry, checkpoint_geometry, validation_pass


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--model_path", type=str, required=True)
    parser.add_argument("--valid_folder", type=str, required=True)
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("--win_size", type=int, default=None, help="STFT window the folder was written with (default: the checkpoint's)")
    parser.add_argument("--hop_size", type=int, default=None, help="hop the folder was written with (default: the checkpoint's)")
    parser.add_argument("--seed", type=int, default=0, help="seed of the crops' random starts")
    parser.add_argument("--passes", type=int, default=1, help="validation passes to average over")
    parser.add_argument("--ema", action="store_true", help="score the checkpoint's ema_state_dict (train.py --ema_decay) instead of its live weights")
    args = parser.parse_args(argv)
    if args.batch_size < 1 or args.passes < 1:
        parser.error("--batch_size and --passes must be at least 1")
    if args.win_size is not None:                                # what can be refused without the checkpoint is refused first
        bad = check_geometry(args.win_size, args.hop_size if args.hop_size is not None else 1)
        if bad:
            parser.error(bad)
    try:
        checkpoint = torch.load(args.model_path, map_location="cpu")
    except Exception as e:
        raise SystemExit(f"validate.py: cannot load {args.model_path}: {e}")
    if not isinstance(checkpoint, dict) or "model_state_dict" not in checkpoint:
        raise SystemExit(f"validate.py: {args.model_path} has no model_state_dict (not a checkpoint of train.py)")
    if args.ema and "ema_state_dict" not in checkpoint:
        from .inference import no_ema_message
        raise SystemExit(no_ema_message("validate.py", args.model_path))
    ck_win, ck_hop = checkpoint_geometry(checkpoint)
    win_size = ck_win if args.win_size is None else args.win_size
    hop_size = ck_hop if args.hop_size is None else args.hop_size
    if (win_size, hop_size) != (ck_win, ck_hop):
        raise SystemExit(f"validate.py: {args.model_path} was trained at --win_size {ck_win} --hop_size {ck_hop}, not at "
                         f"--win_size {win_size} --hop_size {hop_size}: validate it at its own geometry")
    bad = check_geometry(win_size, hop_size)
    if bad:
        parser.error(bad)
    try:
        dataset = SpectrogramDataset(args.valid_folder, win_size=win_size)
    except (ValueError, FileNotFoundError) as e:
        raise SystemExit(f"validate.py: {e}")
    if len(dataset) == 0:
        raise SystemExit(f"validate.py: no *_spec.npy pairs under {args.valid_folder}")
    with_phase = dataset.has_phase_files()
    if not with_phase:
        print("Warning: the validation set has no *_phase.npy files -- its loss is the L1 part only.")

    if not torch.cuda.is_available():
        print("validate.py needs a ROCm device (hand-written gfx950 kernels, no CPU path).")
        sys.exit(1)
    device = torch.device("cuda")
    model = UNet().to(device)
    model.load_state_dict(checkpoint["ema_state_dict" if args.ema else "model_state_dict"])
    model.eval()
    resident = ResidentSpectrograms(dataset, device, with_phase=with_phase)
    with_phase = with_phase and resident.has_phase
    rng = random.Random(args.seed)
    out = {"total": [], "l1": [], "mr": [], "with_phase": with_phase, "win_size": win_size, "hop_size": hop_size}
    for k in range(args.passes):
        with torch.no_grad():
            acc, n_batches = validation_pass(model, resident, args.batch_size, with_phase, win_size, hop_size, rng)
        total, l1, mr = (float(v) / n_batches for v in acc.cpu())          # the pass's one read-back
        out["total"].append(total), out["l1"].append(l1), out["mr"].append(mr)
        print(f"pass {k + 1}: Val {total}  (L1 part {l1}, MR-STFT part {mr}; {ALPHA_L1} * L1 + {ALPHA_MR} * MR over {n_batches} batches)")
    out["n_batches"] = n_batches
    for key in ("total", "l1", "mr"):
        out[f"mean_{key}"] = sum(out[key]) / len(out[key])
    print(f"mean of {args.passes} passes: Val {out['mean_total']}  (L1 part {out['mean_l1']}, MR-STFT part {out['mean_mr']})")
    return out


if __name__ == "__main__":
    main()
