"""The GPU resampler (csrc/resample.hip: svs_resample_pack_taps / svs_resample_poly, resample.resample_poly_gpu) and its callers
(data.load_wav_mono(device=...), data.py --resample gpu, streaming.separate_waveform(sr_in=...)) against float64
scipy.signal.resample_poly, the project's host resampler.

Accuracy bound (no measured tolerance): a length-T dot product in fp32 with taps rounded to fp32 satisfies, for any summation
order and with or without FMA,
    |y_gpu[i] - y_ref64[i]| <= (T + 2) * 2^-24 * S[i] + T * 2^-126,     S[i] = sum_j |x[j]| * |h[i*down - j*up + half]|,
(T + 1 roundings of (1 + 2^-24) on the worst product -- tap rounding, T - 1 additions at most and the product, fused or
not -- is (1 + 2^-24)^(T+1) - 1 <= (T + 2) * 2^-24 for T < 2^10; T * 2^-126 covers products that underflow).  It is applied
to every output, edges included.
"""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy.io import wavfile
from scipy.signal import resample_poly

from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd import data as svs_data
from svs_unet_pytorch_amd import resample as rs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RATE_PAIRS = [(44100, 8192), (48000, 8192), (22050, 8192), (16000, 8192), (8192, 44100), (8192, 16384), (16384, 8192)]


def updown(rate_in, rate_out):
    fr = Fraction(rate_out, rate_in)
    return fr.numerator, fr.denominator


def gpu(x, up, down, **kw):
    out = rs.resample_poly_gpu(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), up, down, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bound_of(x32, up, down):
    """(y_ref64 from scipy, per-output bound) for float32 samples x32."""
    ntaps = 20 * max(up, down) + 1
    T = rs.taps_per_output(ntaps, up)
    _, S = rs.resample_reference(x32, up, down, return_abs=True)
    return resample_poly(x32.astype(np.float64), up, down), (T + 2) * 2.0 ** -24 * S + T * 2.0 ** -126


def check_bound(name, got, want, bound, report, times=1.0):
    assert got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bound).max())                       # bound > 0 everywhere (T * 2^-126 at least)
    print(f"{name}: max err {err.max():.3e} rms err {np.sqrt((err ** 2).mean()):.3e} worst err/bound {worst:.3f}")
    report(f"{name} max |d|", float(err.max()), float(bound.max()) * times)
    report(f"{name} rms d", float(np.sqrt((err ** 2).mean())), float(bound.max()) * times)
    assert report(f"{name} worst err / bound", worst, times)


@pytest.mark.parametrize("rates", RATE_PAIRS, ids=lambda r: f"{r[0]}to{r[1]}")
@pytest.mark.parametrize("n_in", [1, 700, 30001, "3s"])
def test_accuracy_within_the_dot_product_bound(rates, n_in, report):
    up, down = updown(*rates)
    n = 3 * rates[0] if n_in == "3s" else n_in
    x = np.random.default_rng(n + rates[0]).standard_normal(n).astype(np.float32)
    want, bound = bound_of(x, up, down)
    got = gpu(x, up, down)
    assert len(got) == rs.out_len(n, up, down) == len(want)
    check_bound(f"resample {rates[0]}->{rates[1]} n_in={n}", got, want, bound, report)


def test_index_arithmetic_past_2_to_31(report):
    """i * down passes 2^31 after output 194,783 at down = 11025 (24 s of audio): 60 s of 44.1 kHz input."""
    up, down = updown(44100, 8192)
    n = 60 * 44100
    x = np.random.default_rng(60).standard_normal(n).astype(np.float32)
    want, bound = bound_of(x, up, down)
    got = gpu(x, up, down)
    assert len(got) == 491520 and (194783 + 1) * down > 2 ** 31 >= 194783 * down
    check_bound("resample 44100->8192 60 s, all outputs", got, want, bound, report)
    check_bound("resample 44100->8192 60 s, outputs past i*down = 2^31", got[194784:], want[194784:], bound[194784:], report)


@pytest.mark.parametrize("rates", [(44100, 8192), (48000, 8192), (8192, 44100), (16384, 8192)], ids=lambda r: f"{r[0]}to{r[1]}")
def test_bitwise_properties(rates):
    up, down = updown(*rates)
    half = 10 * max(up, down)
    n = 2 * rates[0] + 17
    rng = np.random.default_rng(7)
    x = rng.standard_normal(n).astype(np.float32)
    y = gpu(x, up, down)
    assert np.array_equal(y, gpu(x, up, down))                                   # run to run
    batch = np.stack([x, rng.standard_normal(n).astype(np.float32), x[::-1].copy()])
    yb = gpu(batch, up, down)
    assert yb.shape == (3, len(y))
    for b in range(3):                                                           # batch independence
        assert np.array_equal(yb[b], gpu(batch[b], up, down)), b
    assert np.array_equal(yb[0], y)
    for m in (1, 1000, n // 2 + 3, n - 1):                                       # prefix consistency
        yp = gpu(x[:m], up, down)
        i = np.arange(len(yp), dtype=np.int64)
        assert len(yp) == -((-m * up) // down)
        inside = (i * down + half) // up <= m - 1          # the last input sample output i reads lies inside the prefix
        assert np.array_equal(yp[inside], y[: len(yp)][inside]), m
    yd = gpu(np.concatenate([np.zeros(down, np.float32), x]), up, down)          # a delay of `down` in is `up` out
    assert len(yd) == len(y) + up and np.array_equal(yd[up:], y)


@pytest.mark.parametrize("fmt", ["int16", "int32"])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_fused_front_end_is_bitwise_the_host_conversion(fmt, channels):
    up, down = updown(44100, 8192)
    n = 50001
    rng = np.random.default_rng(channels)
    if fmt == "int16":
        pcm = rng.integers(-32768, 32768, size=(n, channels), dtype=np.int16)
        scale = np.float32(32768.0)
    else:
        pcm = rng.integers(-2 ** 31, 2 ** 31, size=(n, channels), dtype=np.int64).astype(np.int32)
        scale = np.float32(2.0 ** 31)
    chans = [pcm[:, c].astype(np.float32) / scale for c in range(channels)]       # as load_wav_mono converts
    mono = chans[0]
    for c in chans[1:]:
        mono = mono + c
    mono = (mono / np.float32(channels)).astype(np.float32)
    src = pcm if channels > 1 else pcm[:, 0]
    fused = gpu(src, up, down, channels=channels, downmix=True)
    assert fused.shape == (rs.out_len(n, up, down),)
    assert np.array_equal(fused, gpu(mono, up, down))
    each = gpu(src, up, down, channels=channels, downmix=False)
    each = each[None] if channels == 1 else each
    assert each.shape == (channels, len(fused))
    for c in range(channels):
        assert np.array_equal(each[c], gpu(chans[c], up, down)), c
    f32 = np.stack(chans, axis=1)                                                 # float32 interleaved takes the same path
    if channels > 1:
        assert np.array_equal(gpu(f32, up, down, channels=channels, downmix=True), fused)
    two = gpu(np.stack([src, src[::-1].copy()]), up, down, channels=channels, downmix=True)   # a batch of files
    assert np.array_equal(two[0], fused)


def test_stereo_downmix_matches_numpy_mean():
    """load_wav_mono's data.mean(axis=1) on a stereo file is (l + r) / 2 in fp32: the fused downmix reproduces it."""
    pcm = np.random.default_rng(3).integers(-32768, 32768, size=(4096, 2), dtype=np.int16)
    host = (pcm.astype(np.float32) / 32768.0).mean(axis=1)
    got = gpu(pcm, 1, 1, channels=2, downmix=True)                               # 1/1: the identity filter
    assert np.array_equal(got, host)


def test_invalid_arguments_are_errors():
    L = _lib.lib()
    x = torch.zeros(100, device=DEV)
    table, ntaps = rs.tap_table(2, 1, DEV)
    y = torch.zeros(200, device=DEV)
    s = _lib.stream_ptr()
    assert L.svs_resample_poly(x.data_ptr(), 7, 1, 0, 100, 100, 1, table.data_ptr(), ntaps, 2, 1, y.data_ptr(), 200, s) < 0
    assert b"fmt" in L.svs_last_error_string()
    assert L.svs_resample_poly(x.data_ptr(), 0, 1, 0, 0, 100, 1, table.data_ptr(), ntaps, 2, 1, y.data_ptr(), 200, s) < 0
    assert L.svs_resample_poly(x.data_ptr(), 0, 1, 0, 100, 100, 1, table.data_ptr(), ntaps - 1, 2, 1, y.data_ptr(), 200, s) < 0
    assert L.svs_resample_poly(x.data_ptr(), 0, 1, 0, 100, 100, 1, table.data_ptr(), 20 * 4000 + 1, 1, 4000, y.data_ptr(), 200, s) < 0
    assert b"LDS" in L.svs_last_error_string()                                   # down / up = 4000: refused, not mis-computed
    assert L.svs_resample_table_bytes(2, 1, 40) == 0 and L.svs_resample_out_len(-1, 2, 1) == -1
    assert L.svs_resample_out_len(2646000, 2048, 11025) == 491520
    with pytest.raises(ValueError):
        rs.resample_poly_gpu(torch.zeros(10), 2, 1)                              # host tensor: no CPU path
    with pytest.raises(TypeError):
        rs.resample_poly_gpu(torch.zeros(10, dtype=torch.float64, device=DEV), 2, 1)


# ------------------------------------------------------------------------------------------------
# callers
# ------------------------------------------------------------------------------------------------
def _bound_for_file(path, sr):
    """Test-5 bound for load_wav_mono(path, sr): inputs are the host-converted, host-downmixed fp32 samples."""
    rate, data = wavfile.read(path)
    data = data.astype(np.float32) / float(np.iinfo(data.dtype).max + 1) if data.dtype.kind == "i" else data.astype(np.float32)
    if data.ndim == 2:
        data = data.mean(axis=1)
    up, down = updown(rate, sr)
    return bound_of(np.ascontiguousarray(data, dtype=np.float32), up, down)


def test_load_wav_mono_on_the_device(tmp_path, report):
    rng = np.random.default_rng(21)
    stereo = str(tmp_path / "stereo16.wav")
    wavfile.write(stereo, 44100, (rng.standard_normal((3 * 44100, 2)) * 5000).astype(np.int16))
    mono = str(tmp_path / "mono32f.wav")
    svs_data.write_wav(mono, 0.3 * rng.standard_normal(2 * 48000), 48000)
    for name, path in (("int16 stereo 44100", stereo), ("float32 mono 48000", mono)):
        host = svs_data.load_wav_mono(path, 8192)
        dev = svs_data.load_wav_mono(path, 8192, DEV)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float32 and dev.shape == host.shape
        want, bound = _bound_for_file(path, 8192)
        check_bound(f"load_wav_mono device vs float64, {name}", dev.cpu().numpy(), want, bound, report)
        # the host result is itself an fp32 computation within the same bound: against it, the bound twice
        check_bound(f"load_wav_mono device vs host, {name}", dev.cpu().numpy(), host.astype(np.float64), bound, report, times=2.0)
    same_rate = svs_data.load_wav_mono(mono, 48000, DEV)                          # no resampling: conversion only
    assert np.array_equal(same_rate.cpu().numpy(), svs_data.load_wav_mono(mono, 48000))


def _model():
    from svs_unet_pytorch_amd.model import UNet
    m = UNet()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state().items()})
    return m.to(DEV).eval()


def test_separate_waveform_from_the_file_rate():
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = _model()
    n = 44100 * 12
    y44 = torch.from_numpy(np.stack([synth.audio(n, 70), synth.audio(n, 71)]).astype(np.float32)).to(DEV)
    a = separate_waveform(model, y44, sr_in=44100)
    b = separate_waveform(model, rs.resample_poly_gpu(y44, 2048, 11025))
    n8 = rs.out_len(n, 8192, 44100)
    assert a.shape == b.shape == (2, 768 * (n8 // 768)) and torch.equal(a, b)
    mono = separate_waveform(model, y44[0], sr_in=44100)                          # (n,) in, (n',) out
    assert mono.shape == (768 * (n8 // 768),)
    y8 = rs.resample_poly_gpu(y44, 2048, 11025)
    assert torch.equal(separate_waveform(model, y8, sr_in=8192), separate_waveform(model, y8))   # already at the network rate


def _write_song44(folder, idx, n):
    os.makedirs(folder, exist_ok=True)
    voc = synth.audio(n - 3000, 2 * idx + 80) * 0.3
    acc = synth.audio(n, 2 * idx + 81) * 0.5
    mix = acc.copy()
    mix[: voc.size] += voc
    to16 = lambda a: np.clip(np.round(a * 20000), -32768, 32767).astype(np.int16)       # noqa: E731
    stereo = np.stack([to16(mix), to16(0.9 * mix)], axis=1)
    wavfile.write(os.path.join(folder, "mixture.wav"), 44100, stereo)                   # int16 stereo
    wavfile.write(os.path.join(folder, "vocals.wav"), 44100, voc.astype(np.float32))    # float32 mono, shorter (data.py:97-98)


def test_to_spec_with_resample_gpu(tmp_path, report):
    """data.py --direction to_spec --resample gpu against --resample cpu: same files, shapes and dtypes; values gated at 4 x the
    deviation that fp32 (against fp64) scipy resampling of the same files causes through the same STFT (two fp32 paths
    against each other, times 2 for headroom)."""
    src = tmp_path / "wav"
    for i, (name, n) in enumerate((("songA", 44100 * 6), ("songB", 44100 * 5 + 777))):
        _write_song44(str(src / name), i, n)
    out = {}
    for mode in ("cpu", "gpu"):
        out[mode] = tmp_path / f"spec_{mode}"
        svs_data.main(["--src", str(src), "--tar", str(out[mode]), "--direction", "to_spec", "--resample", mode])
    dflt = tmp_path / "spec_default"
    svs_data.main(["--src", str(src), "--tar", str(dflt), "--direction", "to_spec"])
    up, down = updown(44100, 8192)
    d_gpu = {"spec": 0.0, "phase": 0.0}
    d_ref = {"spec": 0.0, "phase": 0.0}
    for track in ("mixture", "vocal"):
        names = sorted(os.listdir(out["cpu"] / track))
        assert names == sorted(os.listdir(out["gpu"] / track)) and len(names) == 4
        for f in names:
            a, b = np.load(out["cpu"] / track / f), np.load(out["gpu"] / track / f)
            assert a.shape == b.shape and a.dtype == b.dtype
            assert np.array_equal(a, np.load(dflt / track / f))                         # the default is the cpu path
    for i, song in enumerate(("songA", "songB")):
        # the reference's own fp32 noise: the same files resampled by scipy in fp32 and in fp64, through the same STFT
        specs = {}
        for prec in (np.float32, np.float64):
            ys = {}
            for wav, track in svs_data.TRACK_MAP.items():
                rate, data = wavfile.read(str(src / song / wav))
                data = data.astype(np.float32) / 32768.0 if data.dtype.kind == "i" else data.astype(np.float32)
                data = data.mean(axis=1) if data.ndim == 2 else data
                ys[track] = resample_poly(data.astype(prec), up, down).astype(np.float32)
            n_mix = len(ys["mixture"])
            ys["vocal"] = np.pad(ys["vocal"], (0, n_mix - len(ys["vocal"])))
            mags = {t: svs_data.stft_magphase(torch.from_numpy(y).to(DEV)) for t, y in ys.items()}
            norm = mags["mixture"][0].max()
            specs[prec] = {t: ((m / norm).cpu().numpy(), p.cpu().numpy()) for t, (m, p) in mags.items()}
        for track in ("mixture", "vocal"):
            base = f"{i:04d}_{song}"
            strong = specs[np.float64][track][0] > 1e-3               # the phase of a near-zero bin is noise in any fp32 FFT
            cpu_s, gpu_s = (np.load(out[m] / track / f"{base}_spec.npy") for m in ("cpu", "gpu"))
            cpu_p, gpu_p = (np.load(out[m] / track / f"{base}_phase.npy") for m in ("cpu", "gpu"))
            d_ref["spec"] = max(d_ref["spec"], float(np.abs(specs[np.float32][track][0] - specs[np.float64][track][0]).max()))
            d_ref["phase"] = max(d_ref["phase"], float(np.abs(specs[np.float32][track][1] - specs[np.float64][track][1])[strong].max()))
            d_gpu["spec"] = max(d_gpu["spec"], float(np.abs(gpu_s - cpu_s).max()))
            d_gpu["phase"] = max(d_gpu["phase"], float(np.abs(gpu_p - cpu_p)[strong].max()))
    print("to_spec --resample gpu vs cpu:", d_gpu, "fp32 vs fp64 scipy:", d_ref)
    report("to_spec magnitude, fp32 vs fp64 scipy resampling (the yardstick)", d_ref["spec"], d_ref["spec"])
    report("to_spec phase (|S| > 1e-3), fp32 vs fp64 scipy resampling (the yardstick)", d_ref["phase"], d_ref["phase"])
    ok_s = report("to_spec magnitude, --resample gpu vs cpu", d_gpu["spec"], 4 * d_ref["spec"])
    ok_p = report("to_spec phase (|S| > 1e-3), --resample gpu vs cpu", d_gpu["phase"], 4 * d_ref["phase"])
    assert ok_s and ok_p
