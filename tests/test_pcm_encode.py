"""CPU suite for the way out of the pipeline (csrc/resample.hip: svs_resample_peaks / svs_resample_encode and their Python
callers): the numpy oracle of the sample-format rules, the peak-normalisation identity the GPU tests rest on, the host
writer, argument checks that must not reach a GPU, and the CLI surfaces."""
import ctypes

import numpy as np
import pytest
from scipy.io import wavfile

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import resample as rs
from svs_unet_pytorch_amd.streaming import kept_length, separated_frames


@pytest.fixture(scope="module")
def lib():
    from svs_unet_pytorch_amd import build
    build.build_lib(verbose=False)
    return _lib.lib()


def tie_input():
    """6,000 float32 samples whose product with float32(32767) is exactly j + 0.5, j = -3000 .. 2999."""
    j = np.arange(-3000, 3000)
    return j, ((2 * j + 1) / 65534).astype(np.float32)


def test_int16_ties_round_to_even():
    j, x = tie_input()
    prod = x * np.float32(32767.0)
    assert prod.dtype == np.float32 and int((prod == (j + 0.5)).sum()) == 6000          # every sample is a tie in fp32
    got = rs.encode_pcm_reference(x, None, "int16")
    assert got.dtype == np.int16 and got.shape == x.shape
    assert np.array_equal(got, np.where(j % 2 == 0, j, j + 1))                            # the even neighbour of j + 0.5
    assert np.array_equal(rs.encode_pcm_reference(x, None, "PCM_16"), got)                # the wav subtype's name, and the code
    assert np.array_equal(rs.encode_pcm_reference(x, None, rs.PCM_I16), got)


def test_limits_of_the_three_formats():
    f = np.float32
    x = np.array([1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 0.0, -0.0, 32767.5 / 32767, -32767.6 / 32767], dtype=f)
    i16 = rs.encode_pcm_reference(x, None, "int16")
    assert i16.tolist() == [32767, -32767, 32767, -32768, 0, 32767, -32768, 0, 0, 32767, -32768]   # -32768 is reachable
    i32 = rs.encode_pcm_reference(x[:9], None, "int32")
    assert i32.dtype == np.int32
    assert i32.tolist() == [2 ** 31 - 1, -(2 ** 31 - 1), 2 ** 31 - 1, -2 ** 31, 0, 2 ** 31 - 1, -2 ** 31, 0, 0]
    assert rs.encode_pcm_reference(np.array([0.5, -0.25], f), None, "int32").tolist() == [1073741824, -536870912]   # rint(.5 * (2^31 - 1)) is even
    f32 = rs.encode_pcm_reference(x, None, "float32")
    assert f32.dtype == np.float32 and np.array_equal(f32.view(np.uint32), x.view(np.uint32))    # bit for bit, NaN and -0 included
    # the gain is one float32 multiply per channel, before the format's own arithmetic
    y = np.array([[0.25, -0.5], [0.75, 0.1]], dtype=f)
    g = np.array([2.0, 3.0], dtype=f)
    assert np.array_equal(rs.encode_pcm_reference(y, g, "float32"), y * g)
    assert rs.encode_pcm_reference(y, g, "int16").tolist() == [[16384, -32768], [32767, int(np.rint(f(0.1) * f(3.0) * f(32767.0)))]]
    assert rs.encode_pcm_reference(y[:, 0], f(4.0), "int16").tolist() == [32767, 32767]
    with pytest.raises(ValueError):
        rs.encode_pcm_reference(y, None, "int8")


def test_peak_normalisation_lands_on_29490():
    """gain = float32(0.9) / p, v = float32(p * gain): whatever p > 0 is, v * 32767 rounds to 29490 -- v is within 1.5 ulp
    (1e-7) of 0.9 and 0.9 * 32767 = 29490.3 is 0.2 from the nearest tie."""
    p = (10.0 ** np.random.default_rng(29490).uniform(-4.0, 2.0, 2000)).astype(np.float32)
    gain = np.float32(0.9) / p
    assert gain.dtype == np.float32
    for sign in (1.0, -1.0):
        got = rs.encode_pcm_reference(np.float32(sign) * p, gain, "int16")
        assert np.array_equal(got, np.full(2000, int(sign) * 29490, dtype=np.int16))
    assert np.array_equal(np.rint((p * gain).astype(np.float32) * np.float32(32767.0)), np.full(2000, 29490.0, dtype=np.float32))


@pytest.mark.parametrize("subtype,dtype", [("PCM_16", np.int16), ("PCM_32", np.int32), ("FLOAT", np.float32)])
@pytest.mark.parametrize("channels", [1, 2])
def test_host_writer_round_trip(tmp_path, subtype, dtype, channels):
    """What save_wav_device hands to scipy.io.wavfile.write -- encode_pcm_reference's array, (n, channels) or (n,) -- comes
    back from wavfile.read with the rate, dtype, shape and samples it had."""
    y = (0.5 * np.random.default_rng(channels).standard_normal((500, channels))).astype(np.float32)
    pcm = rs.encode_pcm_reference(y, np.float32(0.9), subtype)
    assert pcm.dtype == dtype and pcm.shape == (500, channels) and rs.pcm_format(subtype)[1] == dtype
    path = str(tmp_path / "a.wav")
    wavfile.write(path, 44100, pcm[:, 0] if channels == 1 else pcm)
    rate, back = wavfile.read(path)
    assert rate == 44100 and back.dtype == dtype and back.shape == ((500,) if channels == 1 else (500, 2))
    assert np.array_equal(back.reshape(500, channels), pcm)


def test_invalid_arguments_are_reported_without_touching_the_gpu(lib):
    p = ctypes.c_void_p(256)                          # a non-null, 16-byte aligned address that nothing dereferences
    err = lib.svs_last_error_string
    enc = lambda **k: lib.svs_resample_encode(*[k.get(n, d) for n, d in (                                      # noqa: E731
        ("x", p), ("channels", 2), ("n_in", 100), ("ld_in", 100), ("table", p), ("ntaps", 41), ("up", 2), ("down", 1), ("gain", None),
        ("fmt", 1), ("out", p), ("stream", None))])
    pk = lambda **k: lib.svs_resample_peaks(*[k.get(n, d) for n, d in (                                        # noqa: E731
        ("x", p), ("channels", 2), ("n_in", 100), ("ld_in", 100), ("table", p), ("ntaps", 41), ("up", 2), ("down", 1), ("peaks", p),
        ("ws", p), ("ws_bytes", 1 << 20), ("stream", None))])
    for call, name in ((enc, b"svs_resample_encode"), (pk, b"svs_resample_peaks")):
        for bad, word in (({"x": None}, b"null pointer"), ({"table": None}, b"null pointer"), ({"channels": 0}, b"channels"),
                          ({"channels": 9}, b"channels"), ({"n_in": 0}, b"n_in"), ({"ld_in": 99}, b"ld_in"), ({"ntaps": 40}, b"filter"),
                          ({"up": 0}, b"filter"), ({"down": 0}, b"filter"), ({"ntaps": 20 * 4000 + 1, "up": 1, "down": 4000}, b"LDS")):
            assert call(**bad) == -1, (name, bad)
            assert name in err() and word in err(), (bad, err())
    assert enc(out=None) == -1 and b"null pointer" in err()
    assert enc(out=ctypes.c_void_p(260)) == -1 and b"aligned" in err()
    assert enc(fmt=3) == -1 and b"out_fmt" in err()
    assert enc(fmt=-1) == -1
    assert pk(peaks=None) == -1 and b"null pointer" in err()
    assert pk(ws=None) < 0 and b"workspace" in err()
    need = lib.svs_resample_peaks_workspace_bytes(100, 2, 2, 1, 41)
    assert need > 0 and need % 8 == 0                                              # a float per channel per block
    assert pk(ws_bytes=need - 1) < 0 and b"workspace" in err()
    q = lib.svs_resample_peaks_workspace_bytes
    assert q(0, 2, 2, 1, 41) == 0 and q(100, 0, 2, 1, 41) == 0 and q(100, 9, 2, 1, 41) == 0 and q(100, 2, 2, 1, 40) == 0
    assert q(100, 2, 0, 1, 41) == 0 and q(100, 1, 1, 4000, 20 * 4000 + 1) == 0
    # 240 s of stereo, 8,192 -> 44,100 Hz: 44 blocks along i % up (the last with 17 rows) times 23 along the signal
    assert q(240 * 8192, 2, 11025, 2048, 20 * 11025 + 1) == 2 * 44 * 23 * 4
    # the plan svs_resample_plan reports for svs_resample_poly is what it was before the channel count entered the LDS budget
    plan = (ctypes.c_int64 * 8)()
    assert lib.svs_resample_plan(2646000, 2048, 11025, 20 * 11025 + 1, 1, plan) == 0
    assert plan[0] * plan[1] == 256 and plan[2] == (2048 + plan[0] - 1) // plan[0] and plan[6] <= 40 * 1024


def test_device_wrappers_refuse_host_tensors():
    import torch
    with pytest.raises(ValueError):
        rs.resample_encode_gpu(torch.zeros(10), 2, 1)
    with pytest.raises(ValueError):
        rs.pcm_format("PCM_24")


@pytest.mark.parametrize("mod,flags", [("data", ["--sr_out", "--subtype", "PCM_16", "PCM_32", "FLOAT", "--sr", "--direction"]),
                                       ("separate", ["--model_path", "--src", "--tar", "--vocal_solo", "--precision", "--subtype", "PCM_16",
                                                     "--no_keep_length"])])
def test_cli_flags(mod, flags, capsys):
    import importlib
    m = importlib.import_module(f"svs_unet_pytorch_amd.{mod}")
    with pytest.raises(SystemExit) as e:
        m.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for f in flags:
        assert f in text, f


def test_kept_length_arithmetic():
    """A 44.1 kHz file of n frames: ceil(n * 8192 / 44100) samples at the network rate, whole hops of 768 of them survive
    STFT -> iSTFT, and ceil(. * 44100 / 8192) frames are encoded; keep_length cuts or zero-pads those to n."""
    assert [separated_frames(n, 44100) for n in (1, 767, 768, 40000)] == [0, 0, 0, 37210]     # 40000 -> 7431 -> 6912 -> 37210
    assert [separated_frames(n, 8192) for n in (1, 767, 768, 40000)] == [0, 0, 768, 39936]
    for n in (1, 767, 768, 40000):
        for sr in (44100, 48000, 8192):
            enc = separated_frames(n, sr)
            keep, pad = kept_length(enc, n)
            assert keep == min(enc, n) and keep + pad == n and pad >= 0
            assert n - enc < 768 * sr / 8192 + 1                                           # the shortfall is under one hop
    assert kept_length(37210, 40000) == (37210, 2790)
    assert kept_length(768, 768) == (768, 0)
    assert kept_length(0, 1) == (0, 1)
    assert kept_length(4135, 4134) == (4134, 0)             # 768 samples at 8,192 Hz are 4,135 frames at 44,100 Hz: cut, not padded
    assert separated_frames(4134, 44100) == 4135
    with pytest.raises(ValueError):
        kept_length(-1, 5)
