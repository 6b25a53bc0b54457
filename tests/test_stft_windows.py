"""CPU suite (-m "not gpu"): host side of the STFT / inverse STFT at n_fft = 512, 1024 and 2048 (data.py:24 `--win_size`) --
the group and workspace queries of the `_n` family against the 1024-only functions they generalise, the inverse's launch
plan for every hop, the Hann table the forward transform multiplies by, and data.main's argument checks."""
import ctypes

import numpy as np
import pytest

from oracle import stft_oracle as so
from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import data as svs_data

SIZES = (512, 1024, 2048)
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    from svs_unet_pytorch_amd import build
    build.build_lib(verbose=False)
    return _lib.lib()


def plan(lib, n_fft, hop):
    g, r, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0)
    rc = lib.svs_istft_plan_n(n_fft, hop, ctypes.byref(g), ctypes.byref(r), ctypes.byref(lds))
    return rc, g.value, r.value, lds.value


def frames_per_round(n_fft, hop):
    """Two frames per wave: eight waves, except the general kernel (hop < n_fft / 2) at 2048, whose blocks have four."""
    return 8 if n_fft == 2048 and hop < n_fft // 2 else 16


def test_window_sizes_constant():
    assert svs_data.WINDOW_SIZES == SIZES


def test_groups_and_workspace_match_the_1024_functions(lib):
    for frames in (2, 17, 131):
        assert lib.svs_stft_groups_n(1024, frames) == lib.svs_stft_groups(frames)
        for n_fft in (512, 2048):                        # 16 frames per block at every window
            assert lib.svs_stft_groups_n(n_fft, frames) == (frames + 15) // 16
        for hop in (1, 50, 100, 256, 511, 512, 768, 1024):
            assert lib.svs_istft_groups_n(1024, hop, frames, 2) == lib.svs_istft_groups(hop, frames, 2), (hop, frames)
            assert lib.svs_istft_workspace_bytes(1024, hop, frames) == frames * 513 * 8 + 256
            assert lib.svs_istft_workspace_bytes(512, hop, frames) == frames * 257 * 8 + 256
            assert lib.svs_istft_workspace_bytes(2048, hop, frames) == frames * 1025 * 8 + 256
    for bad in (256, 768, 4096):
        assert lib.svs_stft_groups_n(bad, 16) == -1 and b"512, 1024 or 2048" in lib.svs_last_error_string()
        assert lib.svs_istft_groups_n(bad, 100, 16, 1) == -1 and b"512, 1024 or 2048" in lib.svs_last_error_string()
    assert lib.svs_istft_groups_n(512, 513, 16, 1) == -1 and b"hop" in lib.svs_last_error_string()


@pytest.mark.parametrize("n_fft", SIZES)
def test_inverse_launch_plan_for_every_hop(lib, n_fft):
    for hop in range(1, n_fft + 1):
        rc, G, rounds, lds = plan(lib, n_fft, hop)
        assert rc == 0, (hop, lib.svs_last_error_string())
        assert lds <= LDS_PER_CU, (hop, lds)
        assert G >= 1 and rounds >= 1, (hop, G, rounds)
        # every frame that touches the block's G hops is walked
        assert frames_per_round(n_fft, hop) * rounds >= G + (n_fft - 1) // hop, (hop, G, rounds)
        for T in (2, 100):                               # the blocks of a channel cover its padded length
            groups = lib.svs_istft_groups_n(n_fft, hop, T, 2)
            assert groups >= 1 and groups * G * hop >= n_fft + hop * (T - 1), (hop, T, groups, G)
            assert (groups - 1) * G * hop < n_fft + hop * (T - 1), (hop, T, groups, G)      # and none is idle
    # the 1024 geometry is the one the kernels have always had
    if n_fft == 1024:
        assert plan(lib, 1024, 768) == (0, 15, 1, 79872) and plan(lib, 1024, 512) == (0, 15, 1, 79872)
        assert plan(lib, 1024, 256) == (0, 13, 1, 79872 + 13 * 256 * 8)
        assert plan(lib, 1024, 50) == (0, 28, 3, 79872 + 28 * 50 * 8)


def test_inverse_launch_plan_rejections(lib):
    for bad in (768, 256, 4096):
        assert plan(lib, bad, 100)[0] != 0 and b"512, 1024 or 2048" in lib.svs_last_error_string()
    for n_fft in SIZES:
        assert plan(lib, n_fft, n_fft + 1)[0] != 0 and b"hop" in lib.svs_last_error_string()
        assert plan(lib, n_fft, 0)[0] != 0 and b"hop" in lib.svs_last_error_string()


@pytest.mark.parametrize("n_fft", SIZES)
def test_hann_table_is_exact_to_float32(lib, n_fft):
    """The table the forward transform reads at 512 / 2048 (built on the host, copied to the device as it is): within one
    float32 ulp of the float64 periodic Hann window at EVERY entry, the small ones near the window's ends included."""
    out = (ctypes.c_float * (n_fft // 2 + 1))()
    assert lib.svs_hann_table(n_fft, out) == 0
    got = np.frombuffer(out, dtype=np.float32)
    # (the oracle's 0.5 - 0.5 cos form cancels near m = 0 in float64 too, to ~1e-16 absolute: far below an ulp of those entries)
    want = so.hann_periodic(n_fft)[: n_fft // 2 + 1]
    assert got[0] == 0.0 and got[n_fft // 2] == 1.0
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - want) <= ulp), np.abs(got - want).max()
    assert lib.svs_hann_table(768, out) != 0 and b"n_fft" in lib.svs_last_error_string()


def test_data_main_checks_the_window_before_the_device(tmp_path, capsys):
    base = ["--src", str(tmp_path), "--tar", str(tmp_path / "out")]
    with pytest.raises(SystemExit) as e:
        svs_data.main(base + ["--win_size", "768"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert all(str(n) in err for n in SIZES), err
    with pytest.raises(SystemExit) as e:
        svs_data.main(base + ["--win_size", "2048", "--hop_size", "2049"])
    assert e.value.code == 2 and "--hop_size" in capsys.readouterr().err
    import torch
    if not torch.cuda.is_available():                    # past the parser: the next stop is the device check
        with pytest.raises(SystemExit) as e:
            svs_data.main(base + ["--win_size", "2048", "--hop_size", "1536"])
        assert e.value.code == 1 and "ROCm device" in capsys.readouterr().out
