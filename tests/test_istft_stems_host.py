"""CPU suite: the host side of the two-stem inverse STFT (svs_istft_stems_n and its two queries) -- every rejection is reported
before any launch, the launch plan fits a CU's LDS and covers the padded signal at every (n_fft, hop), and the separate CLI
refuses --tar_accomp with --vocal_solo 0 before it looks for a device."""
import ctypes

import pytest

from svs_unet_pytorch_amd import _lib

LDS_PER_CU = 163840
FAKE = ctypes.c_void_p(4096)                    # a non-null pointer that nothing may dereference: no call here launches


@pytest.fixture(scope="module")
def lib():
    from svs_unet_pytorch_amd import build
    build.build_lib(verbose=False)
    return _lib.lib()


def _stems(lib, mag=FAKE, mask=FAKE, phase=FAKE, y=FAKE, n_fft=1024, hop=768, frames=9, channels=2, chan_stride=None, stem_stride=None,
           phase_mode=1, seg=None, rows=None, first_bin=1):
    rows = n_fft // 2 + 1 - first_bin if rows is None else rows
    seg = frames if seg is None else seg
    chan_stride = rows * seg if chan_stride is None else chan_stride
    stem_stride = hop * (frames - 1) * channels if stem_stride is None else stem_stride
    return lib.svs_istft_stems_n(mag, chan_stride, seg, rows, first_bin, mask, phase, phase_mode, channels, n_fft, hop, frames, y, stem_stride,
                                 None, None)


def test_rejections_are_reported_without_touching_the_gpu(lib):
    err = lib.svs_last_error_string
    assert _stems(lib, mask=None) == -1 and b"mask is required" in err()
    for bad in (256, 768, 4096):
        assert _stems(lib, n_fft=bad, hop=128, rows=bad // 2) == -1 and b"512, 1024 or 2048" in err()
    for n_fft in (512, 1024, 2048):
        for hop in (0, -3, n_fft + 1):
            assert _stems(lib, n_fft=n_fft, hop=hop, stem_stride=1 << 20) == -1 and b"hop" in err(), (n_fft, hop)
        for frames in (1, 0):
            assert _stems(lib, n_fft=n_fft, hop=n_fft // 2, frames=frames, seg=4, stem_stride=1 << 20) == -1 and b"frames" in err()
        n_out = (n_fft // 4) * 8
        assert _stems(lib, n_fft=n_fft, hop=n_fft // 4, stem_stride=2 * n_out - 1) == -1 and b"stem_stride" in err()
        assert _stems(lib, n_fft=n_fft, hop=n_fft // 4, channels=1, stem_stride=n_out - 1) == -1 and b"stem_stride" in err()
    # 2 channels x 2^27 elements x 8 B (the phasors of as many bins) = 2 GiB: 32-bit buffer offsets no longer reach it
    assert _stems(lib, chan_stride=1 << 27) == -1 and b"2 GiB" in err()
    assert _stems(lib, n_fft=512, hop=384, frames=600000, channels=2, seg=128, stem_stride=1 << 40) == -1 and b"2 GiB" in err()
    assert _stems(lib, phase_mode=2) == -1 and b"phase_mode" in err()
    assert _stems(lib, mag=None) == -1 and _stems(lib, phase=None) == -1 and _stems(lib, y=None) == -1
    assert _stems(lib, rows=513) == -1 and b"layout" in err()
    assert lib.svs_istft_stems_groups_n(768, 100, 16, 1) == -1 and b"512, 1024 or 2048" in err()
    assert lib.svs_istft_stems_groups_n(512, 513, 16, 1) == -1 and b"hop" in err()
    assert lib.svs_istft_stems_plan_n(1000, 100, None, None, None) == -1 and b"512, 1024 or 2048" in err()
    assert lib.svs_istft_stems_plan_n(1024, 1025, None, None, None) == -1 and b"hop" in err()


def _plan(lib, n_fft, hop, stems=True):
    g, r, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    fn = lib.svs_istft_stems_plan_n if stems else lib.svs_istft_plan_n
    assert fn(n_fft, hop, ctypes.byref(g), ctypes.byref(r), ctypes.byref(lds)) == 0
    return g.value, r.value, lds.value


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_plan_fits_and_covers_at_every_hop(lib, n_fft):
    """For every hop: the block's LDS fits the CU, a block owns at least one hop, its rounds walk every frame that touches its
    hops, and the blocks of a channel cover the padded signal n_fft + hop * (frames - 1)."""
    waves = 4 if n_fft == 2048 else 8
    capped = []
    for hop in range(1, n_fft + 1):
        G, rounds, lds = _plan(lib, n_fft, hop)
        assert lds <= LDS_PER_CU, (hop, lds)
        assert G >= 1 and rounds >= 1, (hop, G, rounds)
        G1, rounds1, lds1 = _plan(lib, n_fft, hop, stems=False)
        if hop >= n_fft // 2:                                    # two frames per sample: the single-stem plan, buffers reused
            assert (G, rounds, lds) == (G1, rounds1, lds1) == (15, 1, lds1)
        else:                                                    # 12 B per accumulated position instead of 8
            halo = (n_fft - 1) // hop
            assert G + halo <= 2 * waves * rounds, (hop, G, halo, rounds)
            assert lds == lds1 - 8 * G1 * hop + 12 * G * hop and G <= G1 and rounds <= rounds1
            if G < G1:
                capped.append(hop)
                assert lds + 12 * hop > LDS_PER_CU               # one more hop would not have fitted
        for frames in (2, 9, 130):
            groups = lib.svs_istft_stems_groups_n(n_fft, hop, frames, 2)
            padded = n_fft + hop * (frames - 1)
            assert groups * G * hop >= padded > (groups - 1) * G * hop, (hop, frames, groups)
    # only the 1024 window with two frames of halo has an accumulator that outgrows the CU: 14 hops x 12 B x hop > 83,968 B
    assert capped == ([h for h in range(342, 512) if 14 * 12 * h > LDS_PER_CU - 79872] if n_fft == 1024 else []), capped


def test_cli_rejects_accompaniment_with_vocal_solo_0(capsys, monkeypatch):
    """--tar_accomp with --vocal_solo 0 is a parser error, raised before the device check (no device is needed to see it)."""
    import torch

    from svs_unet_pytorch_amd import separate
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was looked for before the arguments were checked"))
    with pytest.raises(SystemExit) as e:
        separate.main(["--model_path", "none.pth", "--src", "a.wav", "--tar", "v.wav", "--tar_accomp", "x", "--vocal_solo", "0"])
    assert e.value.code == 2
    assert "--tar_accomp" in capsys.readouterr().err
