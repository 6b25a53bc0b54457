"""The multichannel Wiener filter's float64 definition (wiener.wiener_reference) and the argument rules of the public interface:
no GPU.

Signals: two band-limited, time-gated noise sources from synth.audio, hop * 40 + 5 samples, panned (0.9, 0.3) and (0.3, 0.9);
the mask is 0.6 * the ideal ratio mask + 0.4 * uniform noise; the mixture is scaled to a maximum magnitude of 1, the scale
reg = 1e-7 is stated for.  Tolerances are 1e-12 of the peak.  The condition number of Cxx reaches |x|^2 / reg = 1e7 for a panned
point source (Cxx = s p p^H + reg I), so 1e-12 holds only between backward-stable solves, whose errors lie along the small
eigenvector that R_j then annihilates: the reference's elimination form and an LU solve here (see `restated`)."""
import functools

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import rephase as rp
from svs_unet_pytorch_amd import synth
from svs_unet_pytorch_amd import wiener as wn

GEOMETRIES = [(512, 384), (1024, 768)]
PAN = np.array([[0.9, 0.3], [0.3, 0.9]])           # [source][channel]
BANDS = ((0.02, 0.30), (0.18, 0.70))               # pass bands of the sources, in cycles per sample / 0.5
GATES = ((0.00, 0.65), (0.30, 1.00))               # on / off of the sources, as fractions of the signal


@functools.lru_cache(maxsize=None)
def scene(n_fft, hop):
    """-> (x (2, F, T) complex mixture, images (2 sources, 2 channels, F, T) complex true source images, mask (2, F, T)), DC bin
    dropped, everything divided by the mixture's maximum magnitude."""
    n = hop * 40 + 5
    src = []
    for j in range(2):
        spec = np.fft.rfft(synth.audio(n, 40 + j).astype(np.float64))
        k = np.arange(spec.size) / (spec.size - 1)
        spec[(k < BANDS[j][0]) | (k > BANDS[j][1])] = 0
        t = np.arange(n) / n
        src.append(np.fft.irfft(spec, n) * ((t >= GATES[j][0]) & (t < GATES[j][1])))
    images = np.stack([rp.reference_stft(PAN[j][:, None] * src[j][None], n_fft, hop)[:, 1:] for j in range(2)])
    x = images.sum(axis=0)
    top = np.abs(x).max()
    x, images = x / top, images / top
    a0, a1 = np.abs(images[0]), np.abs(images[1])
    ideal = a0 / np.where(a0 + a1 > 0, a0 + a1, 1.0)
    noise = synth.uniform(44, ideal.size).astype(np.float64).reshape(ideal.shape)
    assert x.shape == (2, n_fft // 2, 41)
    return x, images, 0.6 * ideal + 0.4 * noise


def start(x, mask):
    return np.stack([np.abs(x) * mask, np.abs(x) * (1.0 - mask)])


def restated(x, mags, iters, eps=1e-10, reg=1e-7):
    """The definition once more, for any C: generic einsum and a generic LU solve of Cxx z = x.  Not np.linalg.inv: for a panned
    point source Cxx = s p p^H + reg I, the entries of its inverse are of size 1 / reg and R_j Cxx^-1 cancels them, so a product
    with the explicit inverse is off by up to 9e-11 of the peak from an 80-bit evaluation of these very signals, where this form
    and wiener_reference are within 4e-13."""
    C = x.shape[0]
    a = np.abs(x)
    y = mags * np.where(a == 0, 0, x / np.where(a == 0, 1, a))[None]
    for _ in range(iters):
        v = (np.abs(y) ** 2).mean(axis=1)                                         # (J, F, T)
        R = np.einsum("jaft,jbft->jfab", y, y.conj()) / (eps + v.sum(axis=2))[:, :, None, None]
        Cxx = np.einsum("jft,jfab->ftab", v, R) + reg * np.eye(C)
        z = np.linalg.solve(Cxx, np.moveaxis(x, 0, -1)[..., None])[..., 0]          # (F, T, C)
        y = np.einsum("jft,jfab,ftb->jaft", v, R, z)
    return y


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_reference_agrees_with_a_generic_restatement(n_fft, hop, C, iters):
    x, _, mask = scene(n_fft, hop)
    x, mask = x[:C], mask[:C]
    y, v, R = wn.wiener_reference(x, start(x, mask), iters)
    want = restated(x, start(x, mask), iters)
    assert y.shape == want.shape == (2, C, n_fft // 2, 41) and v.shape == (2, n_fft // 2, 41) and R.shape == (2, n_fft // 2, C, C)
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()


def test_zero_updates_return_the_start():
    x, _, mask = scene(512, 384)
    y, v, R = wn.wiener_reference(x, start(x, mask), 0)
    assert v is None and R is None
    assert np.abs(y[0] + y[1] - x).max() <= 1e-15
    assert np.abs(np.abs(y) - start(x, mask)).max() <= 1e-15


@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_one_channel_is_the_power_ratio_filter(n_fft, hop):
    x, _, mask = scene(n_fft, hop)
    x, mask = x[:1], mask[:1]
    mags = start(x, mask)
    v = mags[:, 0] ** 2
    r = v.sum(axis=-1) / (1e-10 + v.sum(axis=-1))
    g = v * r[:, :, None]
    want = x[None] * (g / (g.sum(axis=0) + 1e-7))[:, None]
    y, _, _ = wn.wiener_reference(x, mags, 1)
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_stems_add_up_to_the_mixture_but_for_the_regulariser(n_fft, hop, C):
    x, _, mask = scene(n_fft, hop)
    x, mask = x[:C], mask[:C]
    reg = 1e-7
    for iters in (1, 2, 3):
        y, v, R = wn.wiener_reference(x, start(x, mask), iters, reg=reg)
        Cxx = np.einsum("jft,jfab->ftab", v, R) + reg * np.eye(C)
        lost = reg * np.einsum("ftab,bft->aft", np.linalg.inv(Cxx), x)
        assert np.abs(y.sum(axis=0) + lost - x).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_identical_channels_in_identical_channels_out(n_fft, hop):
    x, _, mask = scene(n_fft, hop)
    x, mask = np.stack([x[0], x[0]]), np.stack([mask[0], mask[0]])
    for iters in (1, 2, 3):
        y, _, _ = wn.wiener_reference(x, start(x, mask), iters)
        assert np.isfinite(y.real).all() and np.isfinite(y.imag).all()
        assert np.abs(y[:, 0] - y[:, 1]).max() <= 1e-12 * np.abs(y).max()
        assert np.abs(y).max() > 0.1


@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_silent_second_channel_stays_exactly_silent(n_fft, hop):
    x, _, mask = scene(n_fft, hop)
    x = np.stack([x[0], np.zeros_like(x[0])])
    for iters in (1, 2, 3):
        y, v, R = wn.wiener_reference(x, start(x, mask), iters)
        assert not np.isnan(y).any() and not np.isnan(v).any() and not np.isnan(R).any()
        assert np.all(y[:, 1] == 0)
        assert np.abs(y[:, 0]).max() > 0.1


@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_every_update_brings_the_stems_closer_to_the_sources(n_fft, hop):
    """Relative squared error of each stem against the true source image, after 0..3 updates: it falls strictly at every update
    (DESIGN.md section 15 records the figures)."""
    x, images, mask = scene(n_fft, hop)
    err = np.array([[(np.abs(wn.wiener_reference(x, start(x, mask), it)[0][j] - images[j]) ** 2).sum() / (np.abs(images[j]) ** 2).sum()
                     for j in range(2)] for it in range(4)])
    print(f"N={n_fft} hop={hop} relative squared error (vocal, accompaniment) after 0..3 updates:", np.array2string(err, precision=4))
    assert np.all(np.diff(err, axis=0) < 0), err


def test_check_wiener_iters():
    for ok in (0, 1, 8, np.int64(3)):
        assert wn.check_wiener_iters(ok) == int(ok)
    for bad in (-1, 9, 1.0, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="wiener_iters"):
            wn.check_wiener_iters(bad)


def test_reference_rejects_bad_shapes():
    x, _, mask = scene(512, 384)
    with pytest.raises(ValueError, match="wiener_reference"):
        wn.wiener_reference(np.concatenate([x, x[:1]]), start(np.concatenate([x, x[:1]]), np.concatenate([mask, mask[:1]])), 1)
    with pytest.raises(ValueError, match="wiener_reference"):
        wn.wiener_reference(x, start(x, mask)[:, :1], 1)


def test_separate_waveform_checks_its_arguments_before_any_device_work():
    """A CPU tensor and no model: a rejected call has touched neither."""
    from svs_unet_pytorch_amd.streaming import separate_to_wav, separate_waveform
    with pytest.raises(ValueError, match="3 channels.*1 or 2 channels"):
        separate_waveform(None, torch.zeros(3, 4096), wiener_iters=1)
    with pytest.raises(ValueError, match="phase_iters 2.*out of scope"):
        separate_waveform(None, torch.zeros(2, 4096), wiener_iters=1, phase_iters=2)
    with pytest.raises(ValueError, match="wiener_iters"):
        separate_waveform(None, torch.zeros(2, 4096), wiener_iters=9)
    with pytest.raises(ValueError, match="wiener_iters"):
        separate_waveform(None, torch.zeros(2, 4096), wiener_iters=-1)
    with pytest.raises(ValueError, match="phase_iters 1.*out of scope"):
        separate_to_wav(None, "no_such_source.wav", "no_such_target.wav", wiener_iters=2, phase_iters=1)


def test_cli_rejects_the_flag_combinations():
    from svs_unet_pytorch_amd import separate
    for extra in (["--wiener_iters", "9"], ["--wiener_iters", "-1"], ["--wiener_iters", "1", "--phase_iters", "1"]):
        with pytest.raises(SystemExit):
            separate.main(["--model_path", "x.pth", "--src", "a.wav", "--tar", "b.wav"] + extra)
