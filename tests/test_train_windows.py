"""Host side of training at 512- and 2048-sample STFT windows (no GPU): the dataset's row count follows --win_size, files of
another window are refused by name, train.py's geometry flags are validated before any device is touched, and a checkpoint
without geometry keys is read as the config's 1024 / 768."""
import os
import random

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import train as svs_train
from svs_unet_pytorch_amd.config import HOP_SIZE, INPUT_LEN, WINDOW_SIZE


@pytest.fixture
def folder_512(tmp_path):
    """Two songs as `data.py --win_size 512` writes them: (257, T) magnitudes and unit phasors, one longer than a tile (the
    crop branch) and one shorter (the right-pad branch)."""
    rng = np.random.default_rng(5)
    root = tmp_path / "spec"
    os.makedirs(root / "mixture"), os.makedirs(root / "vocal")
    songs = {}
    for i, T in enumerate((200, 70)):
        for track in ("mixture", "vocal"):
            mag = rng.random((257, T), dtype=np.float32)
            ph = np.exp(1j * rng.uniform(-np.pi, np.pi, (257, T))).astype(np.complex64)
            np.save(root / track / f"{i:04d}_s{i}_spec.npy", mag), np.save(root / track / f"{i:04d}_s{i}_phase.npy", ph)
            songs[(i, track)] = (mag, ph)
    return str(root), songs


def test_dataset_rows_follow_the_window(folder_512):
    root, songs = folder_512
    ds = svs_train.SpectrogramDataset(root, samples_per_song=2, win_size=512)
    assert len(ds) == 4 and ds.has_phase_files()
    random.seed(3)
    for idx in range(len(ds)):
        item = ds[idx]
        assert len(item) == 4
        for t in item:
            assert t.dtype == torch.float32 and tuple(t.shape) == (1, 256, INPUT_LEN)
        song = idx % 2
        mag = songs[(song, "mixture")][0][1:]
        mix = item[0][0].numpy()
        if song == 1:                                         # short song: the frames, then zeros (train.py:129-135)
            assert np.array_equal(mix[:, :70], mag) and not mix[:, 70:].any() and not item[2][0].numpy()[:, 70:].any()
            assert np.allclose(item[2][0].numpy()[:, :70], np.angle(songs[(song, "mixture")][1])[1:], atol=1e-6)
        else:                                                 # long song: one 128-frame window of it, the same for all four
            starts = [s for s in range(200 - INPUT_LEN + 1) if np.array_equal(mag[:, s:s + INPUT_LEN], mix)]
            assert len(starts) == 1
            s = starts[0]
            assert np.array_equal(item[1][0].numpy(), songs[(song, "vocal")][0][1:, s:s + INPUT_LEN])
            assert np.allclose(item[3][0].numpy(), np.angle(songs[(song, "vocal")][1])[1:, s:s + INPUT_LEN], atol=1e-6)


def test_dataset_refuses_files_of_another_window(folder_512):
    root, _ = folder_512
    with pytest.raises(ValueError) as ei:
        svs_train.SpectrogramDataset(root, samples_per_song=2)                  # the default window: 1024
    msg = str(ei.value)
    assert "0000_s0_spec.npy" in msg and "257 rows" in msg and "--win_size 1024" in msg and "--win_size 512 would match" in msg, msg
    with pytest.raises(ValueError, match="--win_size 512 would match"):
        svs_train.SpectrogramDataset(root, samples_per_song=2, win_size=2048)
    # a row count that no built window writes
    np.save(os.path.join(root, "mixture", "0000_s0_spec.npy"), np.zeros((300, 10), np.float32))
    with pytest.raises(ValueError, match="300 rows.*no built window"):
        svs_train.SpectrogramDataset(root, samples_per_song=2, win_size=512)


@pytest.mark.parametrize("flags,text", [(["--win_size", "768"], "512, 1024, 2048"),
                                        (["--hop_size", "0"], "--hop_size 0"),
                                        (["--win_size", "512", "--hop_size", "513"], "1..512"),
                                        (["--hop_size", "1025"], "1..1024")])
def test_train_flags_are_checked_before_any_device(flags, text, monkeypatch, capsys, tmp_path):
    monkeypatch.chdir(tmp_path)

    def no_device():
        raise AssertionError("the device was asked for before the flags were checked")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    with pytest.raises(SystemExit) as ei:
        svs_train.main(["--label", "x", "--train_folder", "nowhere"] + flags)
    assert ei.value.code == 2                                 # argparse's own error exit
    assert text in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "CKPT") and not os.path.exists(tmp_path / "LOG")


def test_geometry_rules():
    assert svs_train.check_geometry(512, 384) is None and svs_train.check_geometry(2048, 2048) is None
    assert svs_train.check_geometry(1024, 768) is None and svs_train.check_geometry(2048, 1) is None
    for win in (0, 256, 1000, 4096):
        assert "512, 1024, 2048" in svs_train.check_geometry(win, 1)
    assert "1..512" in svs_train.check_geometry(512, 513) and "--hop_size -3" in svs_train.check_geometry(512, -3)


def test_checkpoint_geometry_default():
    assert (WINDOW_SIZE, HOP_SIZE) == (1024, 768)
    assert svs_train.checkpoint_geometry({"epoch": 3, "model_state_dict": {}}) == (1024, 768)       # written before the keys existed
    assert svs_train.checkpoint_geometry({"win_size": 512, "hop_size": 384}) == (512, 384)
    assert svs_train.checkpoint_geometry({"win_size": 2048}) == (2048, 768)
    assert svs_train.checkpoint_geometry({"win_size": np.int64(2048), "hop_size": np.int64(1536)}) == (2048, 1536)
