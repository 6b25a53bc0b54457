"""The optimiser flags through the command lines: train.py --clip_grad_norm / --weight_decay / --ema_decay / --warmup_steps on a
synthetic folder (two short songs at win 512, no phase files: the L1 objective), the keys of both checkpoints, the resume, and
--ema of validate.py with and without an EMA in the checkpoint."""
import os

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import train as svs_train
from svs_unet_pytorch_amd import validate as svs_validate

pytestmark = pytest.mark.gpu
FRAMES = [150, 200]
OPTIONS = ["--clip_grad_norm", "1", "--weight_decay", "1e-5", "--ema_decay", "0.9", "--warmup_steps", "3"]


def write_folder(root):
    rng = np.random.default_rng(23)
    for d in ("mixture", "vocal"):
        os.makedirs(root / d)
    for i, T in enumerate(FRAMES):
        mix = rng.random((257, T)).astype(np.float32)
        np.save(root / "mixture" / f"{i:04d}_song_spec.npy", mix)
        np.save(root / "vocal" / f"{i:04d}_song_spec.npy", (mix * rng.random((257, T))).astype(np.float32))
    return str(root)


def test_train_validate_with_optimiser_flags(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    folder = write_folder(tmp_path / "spec")
    common = ["--train_folder", folder, "--valid_folder", folder, "--batch_size", "32", "--val_interval", "1", "--win_size", "512",
              "--hop_size", "384"]
    saves = []
    real_save = torch.save

    def recording_save(obj, path, *a, **k):
        ema = obj.get("ema_state_dict") if isinstance(obj, dict) else None          # (a copy: state dicts alias live buffers)
        saves.append((os.path.basename(str(path)), None if ema is None else {k: v.detach().cpu().clone() for k, v in ema.items()}))
        return real_save(obj, path, *a, **k)
    monkeypatch.setattr(torch, "save", recording_save)

    svs_train.main(common + ["--label", "o", "--epoch", "2", "--load_path", "none.pth"] + OPTIONS)
    out = capsys.readouterr().out
    assert out.count("last grad norm") == 2 and "clipped" in out and "skipped (non-finite) 0" in out
    resume = torch.load(tmp_path / "CKPT" / "svs_o.pth", map_location="cpu")
    best = torch.load(tmp_path / "CKPT" / "svs_best_o.pth", map_location="cpu")
    assert resume["epoch"] == 2 and resume["ema_decay"] == 0.9 and len(resume["ema_state_dict"]) == len(resume["model_state_dict"]) == 79
    assert list(resume["ema_state_dict"]) == list(resume["model_state_dict"])
    assert len(best["model_state_dict"]) == 79 and "optim" in best and "ema_state_dict" not in best
    assert resume["optim"]["param_groups"][0]["lr"] == 1e-3            # 8 steps: the 3-step warm-up is over
    assert any(not torch.equal(resume["ema_state_dict"][k], resume["model_state_dict"][k]) for k in resume["model_state_dict"])
    # the best checkpoint's weights are the EMA of the resume checkpoint written in the same epoch (the next save after it)
    names = [n for n, _ in saves]
    last_best = max(i for i, n in enumerate(names) if n == "svs_best_o.pth")
    assert names[last_best + 1] == "svs_o.pth"
    same_epoch = saves[last_best + 1][1]
    for k, v in best["model_state_dict"].items():
        assert torch.equal(v.cpu(), same_epoch[k]), k

    # resume to epoch 3: the EMA comes from the checkpoint
    svs_train.main(common + ["--label", "o", "--epoch", "3", "--load_path", "CKPT/svs_o.pth"] + OPTIONS)
    out = capsys.readouterr().out
    assert "has no ema_state_dict" not in out and out.count("last grad norm") == 1
    resumed = torch.load(tmp_path / "CKPT" / "svs_o.pth", map_location="cpu")
    assert resumed["epoch"] == 3 and "ema_state_dict" in resumed
    steps = int(float(resumed["optim"]["state"][0]["step"]))
    assert steps == 12                                                   # 2 songs x 64 crops / 32 per batch x 3 epochs

    res = svs_validate.main(["--model_path", "CKPT/svs_o.pth", "--valid_folder", folder, "--batch_size", "32", "--ema"])
    live = svs_validate.main(["--model_path", "CKPT/svs_o.pth", "--valid_folder", folder, "--batch_size", "32"])
    assert np.isfinite(res["mean_total"]) and res["mean_total"] != live["mean_total"]

    # a run without the flags: no EMA in its checkpoint; --ema says so, and a resume under --ema_decay starts one
    svs_train.main(common + ["--label", "p", "--epoch", "1", "--load_path", "none.pth"])
    out = capsys.readouterr().out
    assert "last grad norm" not in out
    plain = torch.load(tmp_path / "CKPT" / "svs_p.pth", map_location="cpu")
    assert "ema_state_dict" not in plain and "ema_decay" not in plain
    with pytest.raises(SystemExit) as e:
        svs_validate.main(["--model_path", "CKPT/svs_p.pth", "--valid_folder", folder, "--batch_size", "32", "--ema"])
    assert "has no ema_state_dict" in str(e.value)
    svs_train.main(common + ["--label", "p", "--epoch", "2", "--load_path", "CKPT/svs_p.pth", "--ema_decay", "0.5"])
    out = capsys.readouterr().out
    assert "has no ema_state_dict: the EMA starts from the loaded weights" in out
    assert "ema_state_dict" in torch.load(tmp_path / "CKPT" / "svs_p.pth", map_location="cpu")
