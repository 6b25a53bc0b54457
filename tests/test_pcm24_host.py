"""24-bit PCM and TPDF dither, the host half (no GPU): the two entry points of csrc/pcm.hip are declared, bound and exported and refuse
bad arguments before any launch; the 3-byte packing, the 24-bit wav writer and the chunk walk against scipy; the float64 definition of
the dithered quantiser against the existing int16 rule and against the textbook properties of TPDF dither; the command lines."""
import ctypes

import numpy as np
import pytest
from scipy.io import wavfile

from svs_unet_pytorch_amd import _lib, pcm
from svs_unet_pytorch_amd import resample as rs


@pytest.fixture(scope="module")
def lib():
    from svs_unet_pytorch_amd import build
    build.build_lib(verbose=False)
    return _lib.lib()


def test_symbols_are_declared_bound_and_exported(lib):
    for name in ("svs_pcm24_widen", "svs_pcm_encode_dither"):
        assert name in _lib.header_symbols() and name in _lib._SIGS
        assert getattr(lib, name).argtypes == _lib._SIGS[name][1]
    assert len(_lib._SIGS["svs_pcm24_widen"][1]) == 4 and len(_lib._SIGS["svs_pcm_encode_dither"][1]) == 11


def test_invalid_arguments_are_reported_without_touching_the_gpu(lib):
    p = ctypes.c_void_p(256)                          # a non-null, 16-byte aligned address that nothing dereferences
    err = lib.svs_last_error_string
    enc = lambda **k: lib.svs_pcm_encode_dither(*[k.get(n, d) for n, d in (                                    # noqa: E731
        ("x", p), ("channels", 2), ("frames", 100), ("ld_in", 100), ("gain", None), ("bits", 16), ("dither", 0), ("seed", 0),
        ("first_frame", 0), ("out", p), ("stream", None))])
    for bad, word in (({"x": None}, b"null pointer"), ({"out": None}, b"null pointer"), ({"bits": 32}, b"bits"), ({"bits": 8}, b"bits"),
                      ({"dither": 3}, b"dither"), ({"dither": -1}, b"dither"), ({"channels": 9}, b"channels"), ({"channels": 0}, b"channels"),
                      ({"frames": 0}, b"frames"), ({"ld_in": 99}, b"ld_in"), ({"first_frame": -1}, b"first_frame"),
                      ({"out": ctypes.c_void_p(258)}, b"aligned")):
        assert enc(**bad) == -1, bad
        assert b"svs_pcm_encode_dither" in err() and word in err(), (bad, err())
    wid = lambda **k: lib.svs_pcm24_widen(*[k.get(n, d) for n, d in (("packed", p), ("n", 100), ("out", p), ("stream", None))])   # noqa: E731
    for bad, word in (({"packed": None}, b"null pointer"), ({"out": None}, b"null pointer"), ({"n": 0}, b"n_samples"), ({"n": -5}, b"n_samples"),
                      ({"packed": ctypes.c_void_p(258)}, b"aligned"), ({"out": ctypes.c_void_p(264)}, b"aligned")):
        assert wid(**bad) == -1, bad
        assert b"svs_pcm24_widen" in err() and word in err(), (bad, err())


def test_pack24_unpack24_round_trip():
    edge = np.array([0, 1, -1, 0x7FFFFF, -0x800000], dtype=np.int32)
    assert pcm.pack24(edge).tolist() == [[0, 0, 0], [1, 0, 0], [255, 255, 255], [255, 255, 127], [0, 0, 128]]
    vals = np.concatenate([edge, np.random.default_rng(24).integers(-0x800000, 0x800000, 5000).astype(np.int32)])
    b = pcm.pack24(vals)
    assert b.dtype == np.uint8 and b.shape == (5005, 3)
    wide = pcm.unpack24(b)
    assert wide.dtype == np.int32 and np.array_equal(wide, vals * 256) and not (wide & 0xFF).any()
    assert np.array_equal(pcm.unpack24(b.reshape(-1)), wide)                       # a flat run of bytes
    two = pcm.pack24(vals[:5000].reshape(2500, 2))
    assert two.shape == (2500, 2, 3) and np.array_equal(pcm.unpack24(two.reshape(2500, 6)), vals[:5000].reshape(2500, 2) * 256)
    with pytest.raises(ValueError):
        pcm.unpack24(np.zeros(4, dtype=np.uint8))


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_write_wav24_reads_back_through_scipy(tmp_path, channels):
    """The plain header (1, 2 channels) and the extensible one (3) both read back as the left-justified int32; odd byte counts are padded."""
    vals = np.random.default_rng(channels).integers(-0x800000, 0x800000, (333, channels)).astype(np.int32)
    vals[0, 0], vals[1, 0] = 0x7FFFFF, -0x800000
    packed = pcm.pack24(vals).reshape(333, channels * 3)
    path = str(tmp_path / "a.wav")
    pcm.write_wav24(path, 48000, packed)
    head = open(path, "rb").read(44)
    assert (head[20:22] == b"\x01\x00") == (channels <= 2) and (len(open(path, "rb").read()) == 44 + packed.size + packed.size % 2) == (channels <= 2)
    rate, back = wavfile.read(path)
    assert rate == 48000 and back.dtype == np.int32 and back.shape == ((333,) if channels == 1 else (333, channels))
    assert np.array_equal(back.reshape(333, channels), pcm.unpack24(packed).reshape(333, channels))
    info = pcm.wav_info(path)
    assert info["tag"] == 1 and info["bits"] == 24 and info["channels"] == channels and info["block_align"] == 3 * channels
    assert info["rate"] == 48000 and info["data_bytes"] == packed.size
    raw = np.fromfile(path, dtype=np.uint8, count=info["data_bytes"], offset=info["data_offset"])
    assert np.array_equal(raw, packed.reshape(-1))
    assert pcm.subtype_of(path) == "PCM_24"
    pcm.write_wav24(path, 8000, pcm.pack24(vals))                                   # pack24's own (frames, channels, 3)
    assert np.array_equal(wavfile.read(path)[1].reshape(333, channels), vals * 256)
    with pytest.raises(ValueError):
        pcm.write_wav24(path, 8000, np.zeros((10, 4), dtype=np.uint8))


def test_subtype_of_scipy_files(tmp_path):
    path = str(tmp_path / "s.wav")
    for arr, want in ((np.zeros((50, 2), np.int16), "PCM_16"), (np.zeros(50, np.int32), "PCM_32"), (np.zeros((50, 2), np.float32), "FLOAT"),
                      (np.zeros(50, np.uint8), "PCM_16"), (np.zeros(50, np.float64), "FLOAT")):
        wavfile.write(path, 22050, arr)
        assert pcm.subtype_of(path) == want
        assert pcm.wav_info(path)["rate"] == 22050
    open(path, "wb").write(b"RIFX" + bytes(40))
    assert pcm.wav_info(path) is None
    with pytest.raises(ValueError):
        pcm.subtype_of(path)
    assert pcm.wav_info(str(tmp_path / "absent.wav")) is None


def awkward(n=6000, channels=2, seed=5):
    """Random float32 rows with NaN, +-inf, +-1.0 and exact ties of the int16 rule planted."""
    y = (0.7 * np.random.default_rng(seed).standard_normal((n, channels))).astype(np.float32)
    j = np.arange(-100, 100)
    y[:200, 0] = ((2 * j + 1) / 65534).astype(np.float32)                           # v * 32767 = j + 0.5 in float32
    y[200:207, -1] = [np.nan, np.inf, -np.inf, 1.0, -1.0, 0.0, -0.0]
    return y


def test_undithered_16_bit_is_the_existing_int16_rule():
    y = awkward()
    for gain in (None, np.float32(0.9), np.array([1.5, 0.25], dtype=np.float32)):
        got = pcm.encode_dither_reference(y, gain, 16, "none", 0)
        assert got.dtype == np.int16 and np.array_equal(got, rs.encode_pcm_reference(y, gain, "int16"))
    assert np.array_equal(pcm.encode_dither_reference(y, None, 16, "none", 99, first_frame=1234), rs.encode_pcm_reference(y, None, "int16"))
    # 24 bits without dither: the float64 rule, full scale 2^23 - 1, -2^23 reachable
    x = np.array([1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 0.5, 0.0], dtype=np.float32)
    assert pcm.encode_dither_reference(x, None, 24, "none", 0).tolist() == [8388607, -8388607, 8388607, -8388608, 0, 8388607, -8388608, 4194304, 0]
    assert pcm.encode_dither_reference(x, None, 24, "none", 0).dtype == np.int32
    for bad in (dict(bits=32, kind="none"), dict(bits=16, kind="rpdf")):
        with pytest.raises(ValueError):
            pcm.encode_dither_reference(x, None, bad["bits"], bad["kind"], 0)


N = 65536


def test_dither_is_triangular_exact_and_differs_between_seeds_and_channels():
    for kind in ("tpdf", "hp"):
        d = pcm.dither_reference(kind, 0, 0, N, 2)
        assert d.dtype == np.float32 and d.shape == (N, 2) and np.abs(d).max() < 1.0
        assert np.array_equal(d * 2.0 ** 24, np.rint(d * 2.0 ** 24))               # multiples of 2^-24: the difference is exact
        assert abs(d.mean()) < 5 * np.sqrt(1 / 6 / (2 * N)) and d.var() == pytest.approx(1 / 6, rel=0.03)   # a triangle on (-1, 1)
        assert abs(np.corrcoef(d[:, 0], d[:, 1])[0, 1]) < 0.02
        assert abs(np.corrcoef(d[:, 0], pcm.dither_reference(kind, 1, 0, N, 2)[:, 0])[0, 1]) < 0.02
    assert not pcm.dither_reference("none", 0, 0, 10, 3).any()
    from svs_unet_pytorch_amd import synth
    u = synth.uniform(0, 8)                                                        # the project's counter generator, counters 0 .. 7
    assert np.array_equal(pcm.dither_reference("tpdf", 0, 0, 4, 1)[:, 0], u[0::2] - u[1::2])
    assert np.array_equal(pcm.dither_reference("hp", 0, 1, 2, 2), u[4:8].reshape(2, 2) - u[2:6].reshape(2, 2))


def test_dithered_quantiser_has_no_bias_and_no_noise_modulation():
    """Seed 0, 65,536 frames, 16 bits, a constant of 0.3 LSB: without dither every sample rounds to 0 (the error is the signal);
    with TPDF dither the mean is the input and the error variance is 1/4 LSB^2 whatever the input."""
    lsb = 1.0 / 32767.0
    x = np.full((N, 1), 0.3 * lsb, dtype=np.float32)
    assert not pcm.encode_dither_reference(x, None, 16, "none", 0).any()
    for kind in ("tpdf", "hp"):
        q = pcm.encode_dither_reference(x, None, 16, kind, 0).astype(np.float64)
        print(f"{kind}: mean {q.mean():.5f} LSB (input 0.3)")
        assert abs(q.mean() - 0.3) <= 5 * 0.5 / np.sqrt(N)
    for level in (0.0, 0.3, 0.5):
        x = np.full((N, 1), level * lsb, dtype=np.float32)
        q = pcm.encode_dither_reference(x, None, 16, "tpdf", 0).astype(np.float64)
        var = ((q - np.float64(x[0, 0]) * 32767.0) ** 2).mean()
        print(f"tpdf at {level} LSB: error variance {var:.5f} LSB^2 (1/4)")
        assert abs(var - 0.25) <= 0.05 * 0.25


def test_lag_one_correlation():
    for kind, want in (("hp", -0.5), ("tpdf", 0.0)):
        d = pcm.dither_reference(kind, 0, 0, N, 1)[:, 0].astype(np.float64)
        r = float(np.corrcoef(d[:-1], d[1:])[0, 1])
        print(f"{kind}: lag-1 correlation {r:.4f}")
        assert abs(r - want) <= 0.02


@pytest.mark.parametrize("kind", ["tpdf", "hp"])
@pytest.mark.parametrize("bits", [16, 24])
def test_first_frame_gives_the_slice_of_the_whole(kind, bits):
    y = awkward(4099, 3, seed=8)
    gain = np.array([0.5, 1.0, 2.0], dtype=np.float32)
    whole = pcm.encode_dither_reference(y, gain, bits, kind, 12345)
    for a, b in ((0, 1000), (1000, 4099), (4098, 4099)):
        assert np.array_equal(pcm.encode_dither_reference(y[a:b], gain, bits, kind, 12345, first_frame=a), whole[a:b])
    assert not np.array_equal(pcm.encode_dither_reference(y[1000:], gain, bits, kind, 12345), whole[1000:])
    assert not np.array_equal(pcm.encode_dither_reference(y, gain, bits, kind, 12346), whole)


def test_encoder_bits_and_host_refusals():
    assert [pcm.encoder_bits(s) for s in pcm.SUBTYPES] == [None, 24, None, None]
    assert pcm.encoder_bits("PCM_16", "tpdf") == 16 and pcm.encoder_bits("PCM_24", "hp") == 24
    for subtype in ("PCM_32", "FLOAT"):
        with pytest.raises(ValueError, match="dither"):
            pcm.encoder_bits(subtype, "tpdf")
    with pytest.raises(ValueError):
        pcm.encoder_bits("PCM_16", "noise")
    with pytest.raises(ValueError):
        pcm.encoder_bits("PCM_8")
    with pytest.raises(ValueError):
        rs.pcm_format("PCM_24")                                                    # SVS_PCM_* has no 24-bit code
    import torch
    with pytest.raises(ValueError):
        pcm.widen24_gpu(torch.zeros(6, dtype=torch.uint8))
    with pytest.raises(ValueError):
        pcm.encode_dither_gpu(torch.zeros(2, 8), 8, None, 24, "none")


@pytest.mark.parametrize("mod", ["data", "separate"])
def test_cli_flags(mod, capsys):
    import importlib
    m = importlib.import_module(f"svs_unet_pytorch_amd.{mod}")
    with pytest.raises(SystemExit) as e:
        m.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for f in ("PCM_24", "--dither", "--dither_seed", "tpdf", "hp") + (("source",) if mod == "separate" else ()):
        assert f in text, f


def test_dither_beside_float_is_refused_before_anything_is_opened(tmp_path, capsys):
    from svs_unet_pytorch_amd import data, separate
    absent = str(tmp_path / "absent")
    for subtype in ("FLOAT", "PCM_32"):
        with pytest.raises(SystemExit) as e:
            separate.main(["--model_path", absent + ".pth", "--src", absent + ".wav", "--tar", absent + "_out.wav", "--subtype", subtype,
                           "--dither", "tpdf"])
        assert e.value.code not in (0, None) and "--dither" in capsys.readouterr().err
        with pytest.raises(SystemExit) as e:
            data.main(["--src", absent, "--tar", absent + "_out", "--direction", "to_wave", "--subtype", subtype, "--dither", "hp"])
        assert e.value.code not in (0, None) and "--dither" in capsys.readouterr().err
