"""Validation on the device, host half (-m "not gpu"): the three new entry points are declared and bound, the `validate`
command line refuses bad geometries, a contradicted checkpoint and a folder written at another window before it touches a
device, and a pass sees the items DataLoader(shuffle=False) would hand out, in batches with a short last one."""
import os
import random

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd import train as svs_train
from svs_unet_pytorch_amd import validate as svs_validate

NEW = ("svs_l1_mask_loss_fwd", "svs_unet_eval_loss_workspace_bytes", "svs_unet_eval_loss")


@pytest.fixture(scope="module")
def lib():
    from svs_unet_pytorch_amd import build
    build.build_lib(verbose=False)
    return _lib.lib()


def test_new_symbols_declared_and_bound(lib):
    syms = _lib.header_symbols()
    for name in NEW:
        assert name in syms and name in _lib._SIGS and hasattr(lib, name), name
    # double alphas (the pass total must equal the host's double loop), size_t workspace, and the stream last
    res, args = _lib._SIGS["svs_unet_eval_loss"]
    assert res is _lib.I and len(args) == 17 and args[9] is _lib.D and args[10] is _lib.D and args[15] is _lib.Z
    assert _lib._SIGS["svs_l1_mask_loss_fwd"] == (_lib.I, [_lib.P, _lib.P, _lib.P, _lib.L, _lib.P, _lib.P, _lib.Z, _lib.P])


def test_eval_loss_workspace_query(lib):
    """Host arithmetic: the L1-only form holds the eval workspace, the mask and the partials; the full form adds two waveforms
    and the MR-STFT workspace; nothing for an invalid geometry."""
    B, H, W, hop = 4, 512, 128, 768
    ev = lib.svs_unet_eval_workspace_bytes(B, H, W)
    l1_only = lib.svs_unet_eval_loss_workspace_bytes(B, H, W, 0)
    full = lib.svs_unet_eval_loss_workspace_bytes(B, H, W, hop)
    part = lib.svs_l1_mask_loss_workspace_bytes(B * H * W)
    assert ev + 4 * B * H * W + part <= l1_only <= ev + 4 * B * H * W + part + 3 * 256
    wav = 4 * B * hop * (W - 1)
    mr = lib.svs_mrstft_workspace_bytes(B, hop * (W - 1))
    assert l1_only + 2 * wav + mr <= full <= l1_only + 2 * wav + mr + 3 * 256 + 256
    assert full < lib.svs_unet_train_workspace_bytes(B, H, W)             # no gradient buffers
    assert lib.svs_unet_eval_loss_workspace_bytes(0, H, W, hop) == 0 and lib.svs_unet_eval_loss_workspace_bytes(B, H, W, -1) == 0
    assert lib.svs_unet_eval_loss_workspace_bytes(B, H, 1, hop) == 0 and lib.svs_unet_eval_loss_workspace_bytes(B, 64, 16, 0) > 0


# ------------------------------------------------------------------------------------------------
# validate.py: everything it refuses, it refuses on the host
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach a device fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(svs_validate, "UNet", boom)
    monkeypatch.setattr(svs_validate, "ResidentSpectrograms", boom)


def _checkpoint(path, **geometry):
    state = {k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state().items()}
    torch.save({"model_state_dict": state, "epoch": 1, **geometry}, path)
    return str(path)


def _folder(root, frames, rows=513, phase=False):
    os.makedirs(root / "mixture"), os.makedirs(root / "vocal")
    for n, T in enumerate(frames):
        mix, voc, pm, pv = synth.song(n, T)
        assert mix.shape == (513, T)
        base = f"{n:04d}_len{T}"
        np.save(root / "mixture" / f"{base}_spec.npy", mix[:rows]), np.save(root / "vocal" / f"{base}_spec.npy", voc[:rows])
        if phase:
            np.save(root / "mixture" / f"{base}_phase.npy", pm[:rows]), np.save(root / "vocal" / f"{base}_phase.npy", pv[:rows])
    return str(root)


def test_validate_refuses_bad_geometry(tmp_path, no_device, capsys):
    ck = _checkpoint(tmp_path / "ck.pth", win_size=1024, hop_size=768)
    folder = _folder(tmp_path / "spec", [40])
    with pytest.raises(SystemExit):
        svs_validate.main(["--model_path", str(tmp_path / "absent.pth"), "--valid_folder", folder, "--win_size", "1000"])   # before the checkpoint
    assert "--win_size 1000" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        svs_validate.main(["--model_path", ck, "--valid_folder", folder, "--win_size", "1024", "--hop_size", "1025"])
    assert "--hop_size 1025" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        svs_validate.main(["--model_path", ck, "--valid_folder", folder, "--hop_size", "0"])
    with pytest.raises(SystemExit):
        svs_validate.main(["--model_path", ck, "--valid_folder", folder, "--passes", "0"])


def test_validate_refuses_contradicted_checkpoint(tmp_path, no_device):
    folder = _folder(tmp_path / "spec", [40])
    ck512 = _checkpoint(tmp_path / "ck512.pth", win_size=512, hop_size=384)
    with pytest.raises(SystemExit) as ei:
        svs_validate.main(["--model_path", ck512, "--valid_folder", folder, "--win_size", "1024"])
    assert "trained at --win_size 512 --hop_size 384" in str(ei.value) and "--win_size 1024" in str(ei.value)
    with pytest.raises(SystemExit) as ei:
        svs_validate.main(["--model_path", ck512, "--valid_folder", folder, "--hop_size", "128"])
    assert "trained at --win_size 512 --hop_size 384" in str(ei.value)
    old = _checkpoint(tmp_path / "old.pth")                       # no keys: trained at the config's 1024 / 768
    with pytest.raises(SystemExit) as ei:
        svs_validate.main(["--model_path", old, "--valid_folder", folder, "--win_size", "2048", "--hop_size", "768"])
    assert "trained at --win_size 1024 --hop_size 768" in str(ei.value)
    with pytest.raises(SystemExit) as ei:
        svs_validate.main(["--model_path", str(tmp_path / "absent.pth"), "--valid_folder", folder])
    assert "cannot load" in str(ei.value)


def test_validate_refuses_folder_of_another_window(tmp_path, no_device):
    """The checkpoint's own geometry is the default: a 513-row folder under a 512 checkpoint is refused by the row check, a
    missing and an empty folder by name."""
    folder = _folder(tmp_path / "spec", [40, 200])
    ck512 = _checkpoint(tmp_path / "ck512.pth", win_size=512, hop_size=384)
    with pytest.raises(SystemExit) as ei:
        svs_validate.main(["--model_path", ck512, "--valid_folder", folder])
    msg = str(ei.value)
    assert "513 rows" in msg and "--win_size 1024 would match" in msg and "0000_len40_spec.npy" in msg, msg
    ck = _checkpoint(tmp_path / "ck.pth", win_size=1024, hop_size=768)
    with pytest.raises(SystemExit) as ei:
        svs_validate.main(["--model_path", ck, "--valid_folder", str(tmp_path / "nowhere")])
    assert "not found" in str(ei.value)
    os.makedirs(tmp_path / "empty" / "mixture")
    with pytest.raises(SystemExit) as ei:
        svs_validate.main(["--model_path", ck, "--valid_folder", str(tmp_path / "empty")])
    assert "no *_spec.npy" in str(ei.value)


# ------------------------------------------------------------------------------------------------
# the pass's items
# ------------------------------------------------------------------------------------------------
def test_validation_plan_order_and_batches(tmp_path):
    """9 items at batch 4: batches of 4, 4 and 1; item idx is song idx % n_songs; songs of <= 128 frames start at 0; long ones
    anywhere up to the last whole tile; a seeded generator reproduces the starts, which are `draw`'s."""
    frames = [300, 128, 90]
    ds = svs_train.SpectrogramDataset(_folder(tmp_path / "spec", frames), samples_per_song=3)
    res = svs_train.ResidentSpectrograms(ds, torch.device("cpu"), with_phase=False)      # host tensors: no kernel runs
    assert len(res) == 9 and not res.has_phase and res.rows == 512
    songs, starts, bounds = svs_train.validation_plan(res, 4, random.Random(7))
    assert bounds == [(0, 4), (4, 8), (8, 9)]
    assert songs == [i % 3 for i in range(9)]
    assert all(st == 0 for s, st in zip(songs, starts) if frames[s] <= 128)
    assert all(0 <= st <= 300 - 128 for s, st in zip(songs, starts) if s == 0)
    assert len({st for s, st in zip(songs, starts) if s == 0}) > 1                       # three independent draws
    assert (songs, starts, bounds) == svs_train.validation_plan(res, 4, random.Random(7))
    assert (songs, starts) == res.draw(range(9), random.Random(7))
    assert svs_train.validation_plan(res, 4, random.Random(8))[1] != starts
    assert svs_train.validation_plan(res, 9, random.Random(7))[2] == [(0, 9)]
    assert svs_train.validation_plan(res, 64, random.Random(7))[2] == [(0, 9)]
    assert len(svs_train.validation_plan(res, 1, random.Random(7))[2]) == 9
    # the module-level generator is the default, as in SpectrogramDataset.__getitem__
    random.seed(3)
    a = svs_train.validation_plan(res, 4)
    random.seed(3)
    assert a == svs_train.validation_plan(res, 4)


def test_upload_table_is_one_tensor(tmp_path):
    ds = svs_train.SpectrogramDataset(_folder(tmp_path / "spec", [300, 128, 90]), samples_per_song=3)
    res = svs_train.ResidentSpectrograms(ds, torch.device("cpu"), with_phase=False)
    songs, starts, _ = svs_train.validation_plan(res, 4, random.Random(7))
    pin = torch.Tensor.pin_memory
    try:
        torch.Tensor.pin_memory = lambda self, *a, **k: self                # (no device here to pin for)
        table = res.upload_table(songs, starts)
    finally:
        torch.Tensor.pin_memory = pin
    assert table.dtype == torch.int32 and table.shape == (2, 9) and table.is_contiguous()
    assert table[0].tolist() == songs and table[1].tolist() == starts
    with pytest.raises(ValueError):
        res.crop_table(table, 4, 4)
    with pytest.raises(ValueError):
        res.crop_table(table, 8, 10)
    with pytest.raises(ValueError, match="phase"):
        res.crop_table(table, 0, 4, with_phase=True)
