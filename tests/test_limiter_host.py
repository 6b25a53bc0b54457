"""The look-ahead limiter, the host half (no GPU): the three entry points' declarations, the argument rules that hold before any
device work, the smoothing window, and the properties of the float64 definition limiter.limiter_reference."""
import math

import numpy as np
import pytest

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import limiter as lim
from svs_unet_pytorch_amd import loudness as ld

NAMES = ("svs_limiter_envelope", "svs_limiter_curve", "svs_limiter_apply")


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def err(lib):
    return lib.svs_last_error_string().decode()


def test_symbols_are_declared_bound_and_exported(lib):
    syms = _lib.header_symbols()
    for name in NAMES:
        assert name in syms and name in _lib._SIGS and hasattr(lib, name), name


# ------------------------------------------------------------------------------------------------
# argument rules, before any launch
# ------------------------------------------------------------------------------------------------
# (stems, channels, n, ld_stem, ld_ch, taps, factor, e)
@pytest.mark.parametrize("args,msg", [
    ((0, 2, 100, 200, 100, 64, 4, 64), "stems must be in 1..8"),
    ((1, 9, 100, 200, 100, 64, 4, 64), "channels must be in 1..8"),
    ((1, 2, -1, 200, 100, 64, 4, 64), "n must not be negative"),
    ((1, 2, 100, 200, 99, 64, 4, 64), "ld_ch must be at least n"),
    ((2, 2, 100, 199, 100, 64, 4, 64), "ld_stem must be at least"),
    ((1, 2, 100, 200, 100, 64, 3, 64), "factor must be 1, 2 or 4"),
    ((1, 2, 100, 200, 100, None, 4, 64), "null pointer"),
    ((1, 2, 100, 200, 100, 64, 4, None), "null pointer"),
    ((1, 2, 100, 200, 100, 64, 4, 66), "4-byte aligned"),
])
def test_envelope_refuses_before_any_launch(lib, args, msg):
    stems, channels, n, ld_stem, ld_ch, taps, factor, e = args
    assert lib.svs_limiter_envelope(64, stems, channels, n, ld_stem, ld_ch, taps, factor, e, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_limiter_envelope:")


# (e, n, G_dev, ceiling, window, h, g)
@pytest.mark.parametrize("args,msg", [
    ((64, 100, None, 0.9, 64, 0, 64), "h must be in 1..1024"),
    ((64, 100, None, 0.9, 64, 1025, 64), "h must be in 1..1024"),
    ((64, -1, None, 0.9, 64, 8, 64), "n must not be negative"),
    ((64, 100, None, 0.0, 64, 8, 64), "ceiling must be positive"),
    ((64, 100, None, math.inf, 64, 8, 64), "ceiling must be positive"),
    ((64, 100, None, math.nan, 64, 8, 64), "ceiling must be positive"),
    ((64, 100, None, 0.9, None, 8, 64), "null pointer"),
    ((None, 100, None, 0.9, 64, 8, 64), "null pointer"),
    ((64, 100, None, 0.9, 64, 8, None), "null pointer"),
    ((64, 100, 68, 0.9, 64, 8, 64), "G_dev 8-byte aligned"),
    ((66, 100, None, 0.9, 64, 8, 64), "4-byte aligned"),
])
def test_curve_refuses_before_any_launch(lib, args, msg):
    e, n, G_dev, ceiling, window, h, g = args
    assert lib.svs_limiter_curve(e, n, 2.0, G_dev, ceiling, window, h, g, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_limiter_curve:")


# (x, rows, n, ld_row, g)
@pytest.mark.parametrize("args,msg", [
    ((64, 0, 100, 100, 64), "rows must be in 1..64"),
    ((64, 65, 100, 100, 64), "rows must be in 1..64"),
    ((64, 2, -1, 100, 64), "n must not be negative"),
    ((64, 2, 100, 99, 64), "ld_row must be at least n"),
    ((None, 2, 100, 100, 64), "null pointer"),
    ((64, 2, 100, 100, None), "null pointer"),
    ((64, 2, 100, 100, 66), "4-byte aligned"),
])
def test_apply_refuses_before_any_launch(lib, args, msg):
    x, rows, n, ld_row, g = args
    assert lib.svs_limiter_apply(x, rows, n, ld_row, g, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_limiter_apply:")


def test_empty_signals_launch_nothing(lib):
    assert lib.svs_limiter_envelope(None, 1, 2, 0, 0, 0, None, 1, None, None) == 0
    assert lib.svs_limiter_curve(None, 0, 2.0, None, 0.9, 64, 8, None, None) == 0
    assert lib.svs_limiter_apply(None, 2, 0, 0, None, None) == 0


def test_python_entry_points_check_their_arguments():
    import torch
    from svs_unet_pytorch_amd import data, resample, streaming
    for h in (0, 1025, 1.5, -3):
        with pytest.raises(ValueError, match="half-width"):
            lim.check_h(h)
        with pytest.raises(ValueError, match="half-width"):
            lim.window(h)
        with pytest.raises(ValueError, match="half-width"):
            lim.curve_gpu(torch.zeros(8), 2.0, 0.9, h)               # before the tensor is looked at
        with pytest.raises(ValueError, match="half-width"):
            lim.curve_reference(np.zeros(8), 2.0, 0.9, h)
    with pytest.raises(ValueError, match="ceiling"):
        lim.curve_gpu(torch.zeros(8), 2.0, 0.0, 8)
    with pytest.raises(TypeError, match="device tensor"):
        lim.curve_gpu(torch.zeros(8), 2.0, 0.9, 8)
    assert lim.half_width(44100, 2.0) == 88 and lim.half_width(8192, 2.0) == 16 and lim.half_width(8192, 0.01) == 1
    assert lim.half_width(44100, 1024 / 44.1) == 1024
    for rate, ms in ((44100, 24.0), (192000, 6.0), (44100, 0.0), (44100, -1.0), (44100, math.nan)):
        with pytest.raises(ValueError):
            lim.half_width(rate, ms)
    # limiter_ms without loudness: a ValueError before any device work (host tensors, no device here)
    buf = torch.zeros(2, 2, 64)
    with pytest.raises(ValueError, match="belongs to loudness"):
        resample.encode_planar_gpu(buf, 64, *resample.pcm_format("FLOAT"), rate=44100, limiter_ms=2.0)
    with pytest.raises(ValueError, match="belongs to loudness"):
        resample.encode_loudness_gpu([buf[0]], 1, 1, *resample.pcm_format("FLOAT"), None, 0.9, 44100, None, limiter_ms=2.0)
    with pytest.raises(ValueError, match="belongs to loudness"):
        resample.resample_encode_gpu(torch.zeros(4), 1, 1, limiter_ms=2.0)
    with pytest.raises(ValueError, match="belongs to loudness"):
        data.save_wav_device("unused.wav", torch.zeros(4), 8192, limiter_ms=2.0)
    with pytest.raises(ValueError, match="belongs to loudness"):
        streaming.separate_to_wav(None, "unused.wav", "unused_out.wav", limiter_ms=2.0)
    with pytest.raises(ValueError, match="rate="):
        resample.encode_planar_gpu(buf, 64, *resample.pcm_format("FLOAT"), loudness=-14.0, limiter_ms=2.0)
    with pytest.raises(ValueError, match="half-width"):
        resample.encode_planar_gpu(buf, 64, *resample.pcm_format("FLOAT"), loudness=-14.0, rate=44100, limiter_ms=30.0)
    assert lim.describe(-3.456, -14.2) == "limiter: deepest reduction -3.46 dB, written -14.20 LUFS"


def test_parser_errors(tmp_path, capsys):
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import data, separate
    src = str(tmp_path / "a.wav")
    wavfile.write(src, 44100, np.zeros((4410, 2), np.float32))
    base = ["--model_path", "none.pth", "--src", src, "--tar", str(tmp_path / "o.wav")]
    for tool, argv, msg in ((separate, base + ["--limiter"], "--limiter belongs to --loudness"),
                            (separate, base + ["--loudness", "-14", "--limiter", "30"], "--limiter 30"),
                            (separate, base + ["--loudness", "-14", "--limiter", "0"], "--limiter 0"),
                            (data, ["--src", "s", "--tar", "t", "--direction", "to_wave", "--limiter"], "--limiter belongs to --loudness"),
                            (data, ["--src", "s", "--tar", "t", "--direction", "to_wave", "--loudness", "-14", "--sr_out", "44100", "--limiter", "30"],
                             "--limiter 30")):
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, (argv, msg)
    for tool in (separate, data):
        with pytest.raises(SystemExit) as e:
            tool.main(["--help"])
        assert e.value.code == 0 and "--limiter" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------
# the window
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1, 2, 3, 16, 63, 64, 88, 500, 1024])
def test_window(h):
    w = lim.window(h)
    assert w.dtype == np.float32 and w.shape == (2 * h + 1,)
    assert (w > 0).all() and np.array_equal(w, w[::-1])
    s = float(lim.fp32_sum(w))
    print(f"window h={h}: fp32 sum - 1 = {s - 1.0:.3e}, fp64 sum - 1 = {float(w.astype(np.float64).sum()) - 1.0:.3e}")
    assert abs(s - 1.0) <= (2 * h + 2) * 2.0 ** -24
    assert s >= 1.0 and float(w.astype(np.float64).sum()) >= 1.0        # a stretch of m = 1 clamps at exactly 1
    ideal = 1.0 - np.cos(2.0 * np.pi * (np.arange(2 * h + 1) + 1) / (2 * h + 2))
    assert np.abs(w - ideal / ideal.sum()).max() <= (2 * h + 2) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------
def noise(shape, seed, scale=0.1):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


@pytest.mark.parametrize("h", [1, 7, 88])
@pytest.mark.parametrize("factor", [1, 4])
def test_reference_bounds(h, factor):
    G, C = 2.5, 0.9
    x = noise((2, 2, 3000), seed=h + factor)
    x[0, 1, 0], x[1, 0, 2999], x[0, 0, 1500], x[1, 1, 1503] = 1.0, -1.0, 0.8, 0.9
    z, g, r, e = lim.limiter_reference(x, G, C, h, factor=factor)
    assert z.dtype == np.float32 and z.shape == x.shape and g.shape == r.shape == e.shape == (3000,)
    assert (g <= r).all() and (g > 0).all() and (r < 1).any()                       # g <= r everywhere, exactly
    assert np.array_equal(r, lim.demand(e, G, C))
    assert np.array_equal(e, lim.envelope_reference(x, factor).astype(np.float32))
    if factor == 1:
        assert np.array_equal(e, np.abs(x).reshape(4, -1).max(axis=0))
    # g = 1 exactly farther than 2h from every over-ceiling sample, and only r pulls it under 1
    over = np.flatnonzero(r < 1)
    far = np.abs(np.arange(3000)[:, None] - over[None, :]).min(axis=1) > 2 * h
    assert (g[far] == 1.0).all()
    # |G g x| <= C (1 + 2^-22): r's rounding to float32, g's, and the float32 product
    assert np.abs(G * z.astype(np.float64)).max() <= C * (1.0 + 2.0 ** -22)
    # two stems limited together add up to g (their sum), within 2^-23 of the peak: two float32 products
    total = x.astype(np.float64).sum(axis=0) * g
    assert np.abs(z.astype(np.float64).sum(axis=0) - total).max() <= 2.0 ** -23 * float(np.abs(x).max())


def test_reference_is_one_when_nothing_is_over_the_ceiling():
    x = noise((2, 2000), seed=3)
    peak = float(np.abs(x).max())
    for G in (0.9 / peak, 0.5, math.inf, 0.0, -1.0, math.nan):
        z, g, r, e = lim.limiter_reference(x, G, 0.9, 32)
        assert (g == 1.0).all() and (r == 1.0).all() and np.array_equal(z, x), G
    z, g, r, e = lim.limiter_reference(x, np.nextafter(0.9 / peak, 2.0) * (1.0 + 1e-6), 0.9, 32)
    assert (g < 1.0).any()


@pytest.mark.parametrize("h", [1, 5, 64])
def test_curve_is_monotone_around_one_spike(h):
    n, s = 8 * h + 40, 4 * h + 17
    e = np.full(n, 0.01, np.float32)
    e[s] = 1.0
    g, r = lim.curve_reference(e, 3.0, 0.9, h)
    assert r[s] == np.float32(0.9 / 3.0) and (np.delete(r, s) == 1.0).all()
    slack = (2 * h + 1) * 2.0 ** -53                                 # the float64 sums of the definition
    d = np.diff(g)
    assert (d[:s] <= slack).all() and (d[s:] >= -slack).all()        # down into the spike, up out of it
    assert g[s] == r[s]                                              # the clamp holds the demand exactly
    assert (g[:s - 2 * h] == 1.0).all() and (g[s + 2 * h + 1:] == 1.0).all()
    assert (g[s - 2 * h + 1:s + 2 * h] < 1.0).all()                  # the +-2h samples the spike bends
    # the whole plateau of the minimum sits under the spike: g stays at the demand's level within the window's rounding there
    assert abs(g[s - 1] - g[s + 1]) <= slack and g[s - 1] < 1.0


def test_sliding_minimum_against_brute_force():
    r = np.random.default_rng(5).uniform(0.2, 1.0, 300).astype(np.float32)
    for h in (1, 4, 50):
        m = lim.sliding_min(r, h)
        rp = np.concatenate([np.ones(2 * h, np.float32), r, np.ones(2 * h, np.float32)])
        want = np.array([rp[j:j + 2 * h + 1].min() for j in range(300 + 2 * h)])
        assert np.array_equal(m, want)


def test_demand_is_one_division_and_one_rounding():
    e = np.array([0.0, 0.2, 0.3, 0.30000001, 0.5, 1.0, 7.0], np.float32)
    r = lim.demand(e, 3.0, 0.9)
    want = [1.0 if 3.0 * float(v) <= 0.9 else np.float32(0.9 / (3.0 * float(v))) for v in e]
    assert r.dtype == np.float32 and r.tolist() == [float(v) for v in want]


def test_way_out_input_is_ceiling_limited_under_the_plain_rule():
    """The input of tests/test_gpu_limiter.py's way-out cases, checked on the CPU reference alone: the plain rule's cap lies more than
    6 dB under the unlimited gain."""
    for fs in (8192, 44100):
        x = way_out_stems(fs)
        L = ld.loudness_reference(x, fs, stems=2)[0]
        for tp in (False, True):
            peak = (ld.true_peak_reference(x.reshape(4, -1), fs)[1] if tp else np.abs(x).reshape(4, -1).max(axis=1)).max()
            gain, unlimited, limited = ld.gain_rule(L, peak, -14.0, 0.9)
            print(f"fs={fs} true_peak={tp}: L {L:.2f} LUFS, unlimited {20 * math.log10(unlimited):.2f} dB, cap {20 * math.log10(0.9 / peak):.2f} dB")
            assert limited and 20.0 * math.log10(unlimited / (0.9 / peak)) > 6.0


def way_out_stems(fs, seconds=1.5):
    """Two stereo stems of noise at -30 dBFS RMS with one full-scale sample every 100 ms (alternating stem, channel and sign)."""
    n = int(seconds * fs)
    x = noise((2, 2, n), seed=fs, scale=10.0 ** (-30.0 / 20.0))
    for k, i in enumerate(range(fs // 20, n, fs // 10)):
        x[k % 2, (k // 2) % 2, i] = 1.0 if k % 3 else -1.0
    return x
