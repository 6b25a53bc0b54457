"""Integrated loudness on the device (-m gpu; csrc/loudness.hip) against the float64 definition loudness.loudness_reference: the
block energies z_j over rates, channel counts, stem counts and lengths around the block edges, a long-memory input, a row stride,
bitwise reproducibility, both gating outcomes, the gain rule with and without the ceiling, the loudness path of
resample_encode_gpu, and separate.py --loudness.  No case runs more than 3 s of audio.

Z_BOUND: the worst relative |dz_j| seen on an MI355X over every z case here is 6.1e-11, on the long-memory input (noise inputs:
2.5e-15 at most); DESIGN.md section 20 says where it comes from.  The gate is 8x that, and in any case below 1e-7 (above fp32's
6e-8 a difference is no fp64 round-off but an fp32 accumulation or a lost state)."""
import math
import os

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import loudness as ld
from svs_unet_pytorch_amd import resample as rs

pytestmark = pytest.mark.gpu
DEV = "cuda"
Z_BOUND = 4.9e-10            # 8 x 6.1e-11, the worst case measured
assert Z_BOUND < 1e-7


def noise(shape, seed, scale=0.1):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def z_error(x, fs, stems):
    """(worst relative |dz|, z of the device) of x: (channels, n) or (stems, channels, n) float32 on the host."""
    want = ld.loudness_reference(x, fs, stems=stems if stems == 2 else None)[1]
    got = ld.block_energies_gpu(torch.from_numpy(x).to(DEV), fs, stems).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64
    if want.size == 0:
        return 0.0, got
    assert np.all(want > 0)
    return float((np.abs(got - want) / want).max()), got


@pytest.mark.parametrize("stems", [1, 2])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("fs", [8192, 44100, 48000])
def test_block_energies_match_the_definition(fs, channels, stems, report):
    """n = e_4 - 1: no block; n = e_4: exactly one; n = e_9 + 37: a ragged tail (8192 Hz: bins of 819 and 820 samples)."""
    for n, blocks in ((ld.edge(4, fs) - 1, 0), (ld.edge(4, fs), 1), (ld.edge(9, fs) + 37, 6)):
        x = noise((stems, channels, n) if stems == 2 else (channels, n), seed=fs + 10 * channels + stems)
        e, got = z_error(x, fs, stems)
        print(f"loudness z fs={fs} channels={channels} stems={stems} n={n}: blocks {got.size}, worst relative error {e:.3e}")
        assert got.size == blocks == ld.nblocks(n, fs)
        assert report(f"loudness z fs={fs} ch={channels} stems={stems} n={n}", e, Z_BOUND)


def test_long_memory_input_carries_its_state(report):
    """A DC step of 0.5 under a 10 Hz sine, 3 s at 48 kHz: the high-pass pole (radius 0.995) remembers the step for thousands of
    samples, so every chunk's output depends on state carried in from all chunks before it."""
    fs, n = 48000, 3 * 48000
    t = np.arange(n) / fs
    x = (0.5 + 0.25 * np.sin(2 * np.pi * 10.0 * t)).astype(np.float32)[None]
    e, got = z_error(x, fs, 1)
    print(f"loudness z long memory: blocks {got.size}, worst relative error {e:.3e}")
    assert got.size == 27
    assert report("loudness z DC step + 10 Hz sine, 48 kHz, 3 s", e, Z_BOUND)


def test_row_stride_and_reproducibility(report):
    fs, n = 44100, ld.edge(9, 44100) + 37
    wide = torch.from_numpy(noise((2, n + 13), seed=5)).to(DEV)
    view = wide[:, :n]
    assert view.stride(0) == n + 13
    z1 = ld.block_energies_gpu(view, fs)
    z2 = ld.block_energies_gpu(view, fs)
    assert torch.equal(z1, z2)                                     # bit for bit
    want = ld.loudness_reference(view.cpu().numpy(), fs)[1]
    e = float((np.abs(z1.cpu().numpy() - want) / want).max())
    print(f"loudness z ld_ch > n: worst relative error {e:.3e}")
    assert report("loudness z with a row stride", e, Z_BOUND)
    assert torch.equal(ld.block_energies_gpu(view.contiguous(), fs), z1)


def peaks_of(x):
    return x.abs().reshape(-1, x.shape[-1]).amax(dim=1)


def test_gating_loud_then_quiet(report):
    """1.2 s of noise, then the same 30 dB lower: the relative gate drops the quiet blocks."""
    fs = 48000
    loud = noise((2, int(1.2 * fs)), seed=11)
    x = np.concatenate([loud, noise((2, int(1.8 * fs)), seed=11) * np.float32(10 ** (-30 / 20))], axis=1)
    L, z, first, kept = ld.loudness_reference(x, fs)
    l = -0.691 + 10 * np.log10(z)
    gamma = -0.691 + 10 * np.log10(z[first].mean()) - 10.0
    assert np.abs(l + 70.0).min() > 0.01 and np.abs(l - gamma).min() > 0.01      # a condition on the input, not a tolerance
    assert 0 < kept.sum() < z.size
    _, info = ld.loudness_gain_gpu(torch.from_numpy(x).to(DEV), fs)
    info = info.cpu().numpy()
    print(f"loudness gating: reference L {L:.9f} kept {kept.sum()} of {z.size}; device L {info[0]:.9f} kept {info[1]}")
    assert info[1] == kept.sum()
    assert report("loudness gated L vs reference (LU)", abs(info[0] - L), 1e-6)
    assert math.isnan(info[2]) and info[3] == 0                    # measured only


@pytest.mark.parametrize("case", ["short", "below the absolute gate"])
def test_nothing_kept_leaves_the_peak_rule(case):
    fs = 44100
    x = noise((2, ld.edge(4, fs) - 1), seed=3) if case == "short" else noise((2, fs), seed=4, scale=1e-6)
    xd = torch.from_numpy(x).to(DEV)
    gain, info = ld.loudness_gain_gpu(xd, fs, -23.0, ceiling=0.9, peaks=peaks_of(xd))
    info, gain = info.cpu().numpy(), gain.cpu().numpy()
    assert info[0] == -np.inf and info[1] == 0 and info[3] == 1
    want = np.float32(0.9 / float(np.abs(x).max()))
    assert gain.shape == (2,) and gain[0] == gain[1] and abs(gain[0] - want) <= np.spacing(want)


@pytest.mark.parametrize("target,limited", [(-20.0, False), (10.0, True)])
def test_gain_rule(target, limited):
    fs = 48000
    xd = torch.from_numpy(noise((2, fs), seed=8)).to(DEV)
    peaks = peaks_of(xd)
    gain, info = ld.loudness_gain_gpu(xd, fs, target, ceiling=0.9, peaks=peaks)
    info, gain = info.cpu().numpy(), gain.cpu().numpy()
    g, unlimited, lim = ld.gain_rule(info[0], float(peaks.max().item()), target, 0.9)
    want = np.float32(g)
    print(f"loudness gain target {target}: device {gain[0]!r}, rule {g!r}, L {info[0]:.6f}, limited {info[3]}")
    assert lim == limited and info[3] == (1.0 if limited else 0.0)
    assert gain[0] == gain[1] and abs(gain[0] - want) <= np.spacing(want)
    assert abs(info[2] - unlimited) <= 1e-12 * unlimited
    # a device target: the same number read from another call's info
    tdev = torch.tensor([target, 0.0, 0.0, 0.0], dtype=torch.float64, device=DEV)
    gain2, _ = ld.loudness_gain_gpu(xd, fs, tdev, ceiling=0.9, peaks=peaks)
    assert np.array_equal(gain2.cpu().numpy(), gain)


def tones(n, fs, seed, channels=2):
    t = np.arange(n) / fs
    rng = np.random.default_rng(seed)
    rows = [sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.2, 0.1, 0.05), rng.uniform(200, 2500, 3), rng.uniform(0, 6, 3)))
            for _ in range(channels)]
    return (np.stack(rows) + 0.01 * rng.standard_normal((channels, n))).astype(np.float32)


def test_encode_float_reads_the_target(report):
    y = torch.from_numpy(tones(8192, 8192, seed=1)).to(DEV)
    pcm, info = rs.resample_encode_gpu(y, 44100, 8192, fmt="FLOAT", loudness=-20.0, rate=44100)
    pcm, info = pcm.cpu().numpy(), info.cpu().numpy()
    assert pcm.dtype == np.float32 and pcm.shape == (44100, 2) and info[3] == 0 and np.abs(pcm).max() <= 0.9
    L = ld.loudness_reference(pcm.T, 44100)[0]
    print(f"loudness encode FLOAT: written {L:.6f} LUFS for target -20; measured before the gain {info[0]:.6f}")
    assert report("loudness encode FLOAT vs target (LU)", abs(L + 20.0), 1e-3)


def test_encode_int16_is_the_fused_encoders_arithmetic():
    y = torch.from_numpy(tones(8192, 8192, seed=2)).to(DEV)
    fr = rs.reduced(44100, 8192)
    poly = rs.resample_poly_gpu(y, *fr)                            # (channels, n_out): the float the fused encoder forms
    gain, _ = ld.loudness_gain_gpu(poly, 44100, -20.0, ceiling=0.9, peaks=peaks_of(poly))
    want = rs.encode_pcm_reference(poly.cpu().numpy().T, gain.cpu().numpy(), "int16")
    got, _ = rs.resample_encode_gpu(y, 44100, 8192, fmt="int16", loudness=-20.0, rate=44100)
    assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), want)


def test_encode_together_shares_one_gain(report):
    v = torch.from_numpy(tones(8192, 8192, seed=3)).to(DEV)
    a = torch.from_numpy(2 * tones(8192, 8192, seed=4)).to(DEV)
    pv, pa, info = rs.resample_encode_gpu(v, 44100, 8192, fmt="FLOAT", loudness=-20.0, rate=44100, together=a)
    fr = rs.reduced(44100, 8192)
    both = torch.stack([rs.resample_poly_gpu(v, *fr), rs.resample_poly_gpu(a, *fr)])
    gain, info2 = ld.loudness_gain_gpu(both, 44100, -20.0, ceiling=0.9, stems=2, peaks=peaks_of(both))
    assert torch.equal(info, info2) and info[3].item() == 0
    g = gain.cpu().numpy()
    assert g[0] == g[1]
    for got, stem in ((pv, both[0]), (pa, both[1])):               # the same gain on both files, bit for bit
        assert np.array_equal(got.cpu().numpy(), rs.encode_pcm_reference(stem.cpu().numpy().T, g, "FLOAT"))
    total = pv.cpu().numpy().astype(np.float64) + pa.cpu().numpy().astype(np.float64)
    L = ld.loudness_reference(total.T, 44100)[0]
    print(f"loudness encode together: the sum reads {L:.6f} LUFS for target -20")
    assert report("loudness encode together, sum vs target (LU)", abs(L + 20.0), 1e-3)


def test_separate_cli_loudness_source(tmp_path, report, capsys):
    """separate.py --tar_accomp --loudness source: vocal + accompaniment read the source's loudness; without --loudness the files are
    byte for byte those of the default path (separate_waveform, resample_encode_gpu(peak=0.9), kept_length), rebuilt here from
    its pieces."""
    from fractions import Fraction

    from scipy.io import wavfile

    from svs_unet_pytorch_amd import data, separate, streaming, synth
    from svs_unet_pytorch_amd.model import UNet
    torch.manual_seed(1234)
    model = UNet().to(DEV).eval()
    ck = str(tmp_path / "svs_random.pth")
    torch.save({"model_state_dict": model.state_dict()}, ck)
    n, rate = 2 * 44100, 44100
    mix = (0.5 * np.stack([synth.audio(n, 50), 0.7 * synth.audio(n, 51)], axis=1)).astype(np.float32)
    mix *= np.float32(0.5 / np.abs(mix).max())
    src = str(tmp_path / "mixture.wav")
    wavfile.write(src, rate, mix)
    common = ["--model_path", ck, "--src", src, "--subtype", "FLOAT"]
    voc, acc = str(tmp_path / "vocal.wav"), str(tmp_path / "accomp.wav")
    separate.main(common + ["--tar", voc, "--tar_accomp", acc, "--loudness", "source"])
    line = [l for l in capsys.readouterr().out.splitlines() if "LUFS" in l]
    assert len(line) == 1 and "gain" in line[0]
    (r0, v), (r1, a) = wavfile.read(voc), wavfile.read(acc)
    assert r0 == r1 == rate and v.dtype == a.dtype == np.float32 and v.shape == a.shape == (n, 2)
    want = ld.loudness_reference(mix.T, rate)[0]
    got = ld.loudness_reference((v.astype(np.float64) + a.astype(np.float64)).T, rate)[0]
    print(f"separate --loudness source: source {want:.4f} LUFS, vocal + accompaniment {got:.4f} LUFS; {line[0]}")
    assert report("separate --loudness source, sum vs source (LU)", abs(got - want), 0.01)
    assert max(np.abs(v).max(), np.abs(a).max()) <= 0.9

    # without --loudness: the default path's bytes
    v0, a0 = str(tmp_path / "v0.wav"), str(tmp_path / "a0.wav")
    separate.main(common + ["--tar", v0, "--tar_accomp", a0])
    _, pcm, channels = data.read_pcm(src)
    fr = Fraction(8192, rate)
    y = rs.resample_poly_gpu(torch.from_numpy(pcm).to(DEV), fr.numerator, fr.denominator, channels=channels, downmix=False)
    sep = streaming.separate_waveform(model, y, peak=None, both_stems=True)
    for stem, path in ((sep[0], v0), (sep[1], a0)):
        enc = rs.resample_encode_gpu(stem, fr.denominator, fr.numerator, fmt="FLOAT", peak=0.9, common_gain=True)
        keep, pad = streaming.kept_length(enc.shape[0], n)
        enc = torch.nn.functional.pad(enc[:keep], (0, 0, 0, pad))
        ref = str(tmp_path / ("ref_" + os.path.basename(path)))
        wavfile.write(ref, rate, enc.cpu().numpy())
        assert open(ref, "rb").read() == open(path, "rb").read()
