"""CPU suite for svs_unet_pytorch_amd/resample.py: the filter design, the closed-form index rule and the packed tap table
against scipy.signal.resample_poly (the project's host resampler), and load_wav_mono's untouched host path."""
from fractions import Fraction

import numpy as np
import pytest
from scipy.io import wavfile
from scipy.signal import firwin, resample_poly

from svs_unet_pytorch_amd import data as D
from svs_unet_pytorch_amd import resample as rs

# (rate in, rate out) of the cases the index rule was checked for: the file rates down to the network's 8,192 Hz, and up
RATE_PAIRS = [(44100, 8192), (48000, 8192), (22050, 8192), (16000, 8192), (8192, 44100), (8192, 16384), (16384, 8192)]


def updown(rate_in, rate_out):
    fr = Fraction(rate_out, rate_in)
    return fr.numerator, fr.denominator


@pytest.mark.parametrize("up,down", [(2048, 11025), (64, 375), (4096, 11025), (1, 2), (2, 1), (11025, 2048)])
def test_design_lowpass_equals_firwin(up, down):
    m = max(up, down)
    want = firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up
    got = rs.design_lowpass(up, down)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-15


def test_design_lowpass_reduces_by_the_gcd():
    assert np.array_equal(rs.design_lowpass(8192, 44100), rs.design_lowpass(2048, 11025))
    assert rs.reduced(8192, 48000) == (64, 375)


@pytest.mark.parametrize("rates", RATE_PAIRS, ids=lambda r: f"{r[0]}to{r[1]}")
@pytest.mark.parametrize("n_in", [1, 2, 700, 30001, 132317])
def test_reference_sum_equals_resample_poly(rates, n_in):
    up, down = updown(*rates)
    x = np.random.default_rng(n_in).standard_normal(n_in)
    want = resample_poly(x, up, down)
    got = rs.resample_reference(x, up, down)
    assert got.shape == want.shape and len(got) == rs.out_len(n_in, up, down)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_reference_abs_sum_is_resample_poly_of_magnitudes():
    up, down = 2048, 11025
    x = np.random.default_rng(5).standard_normal(5000)
    h = rs.design_lowpass(up, down)
    y, s = rs.resample_reference(x, up, down, return_abs=True)
    want = resample_poly(np.abs(x), up, down, window=np.abs(h) / up)
    assert np.abs(s - want).max() <= 1e-13 * want.max()
    assert np.all(np.abs(y) <= s * (1 + 1e-12))
    rows = rs.resample_reference(np.stack([x, -2 * x]), up, down)                 # leading axes are batch axes
    tol = 1e-13 * np.abs(y).max()                        # numpy may sum the (rows, outputs, T) product in another order
    assert np.abs(rows[0] - y).max() <= tol and np.abs(rows[1] + 2 * y).max() <= 2 * tol


@pytest.mark.parametrize("up,down", [(2048, 11025), (64, 375), (11025, 2048), (2, 1), (1, 2), (3, 7)])
def test_packed_table_round_trips(up, down):
    h = rs.design_lowpass(up, down)
    half = (len(h) - 1) // 2
    T = rs.taps_per_output(len(h), up)
    table = rs.pack_taps(h, up, down)
    assert table.shape == (T, up)
    hp = np.concatenate([h, np.zeros(T * up - len(h))])
    for i in [0, 1, 2, up - 1, up, up + 1, 194783, 194784, 2 ** 33 + 12345]:
        p = (i * down + half) % up
        assert np.array_equal(rs.unpack_row(table, i), hp[p + np.arange(T) * up]), i
    assert np.array_equal(np.sort(table.ravel()), np.sort(hp))          # every tap is there exactly once


def _parent_load_wav_mono(path, sr):
    """load_wav_mono as it was before the device path existed, written out."""
    rate, data = wavfile.read(path)
    if data.dtype.kind == "i":
        data = data.astype(np.float32) / float(np.iinfo(data.dtype).max + 1)
    elif data.dtype.kind == "u":
        data = (data.astype(np.float32) - 128.0) / 128.0
    else:
        data = data.astype(np.float32)
    if data.ndim == 2:
        data = data.mean(axis=1)
    if rate != sr:
        fr = Fraction(sr, rate)
        data = resample_poly(data, fr.numerator, fr.denominator).astype(np.float32)
    return np.ascontiguousarray(data, dtype=np.float32)


def test_load_wav_mono_host_path_is_unchanged(tmp_path):
    rng = np.random.default_rng(11)
    stereo = str(tmp_path / "stereo16.wav")
    wavfile.write(stereo, 44100, (rng.standard_normal((20000, 2)) * 6000).astype(np.int16))
    mono = str(tmp_path / "mono32f.wav")
    D.write_wav(mono, 0.3 * rng.standard_normal(15000), 22050)
    for path in (stereo, mono):
        for sr in (8192, 44100 if path == stereo else 22050):
            got = D.load_wav_mono(path, sr)
            want = _parent_load_wav_mono(path, sr)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.flags.c_contiguous
            assert np.array_equal(got, want)
            assert np.array_equal(D.load_wav_mono(path, sr, device=None), want)
