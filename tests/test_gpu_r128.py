"""The EBU R 128 meter on the device (-m gpu; csrc/loudness.hip, csrc/r128.hip) against the float64 definitions of loudness.py: the
momentary and short-term series of svs_loudness_series, the maxima and the loudness range of svs_loudness_stats with its exact
selections, svs_true_peaks, the way out under true_peak=True, and the command lines.  No case runs more than 12 s of audio.

Bounds.  z_s: DESIGN.md section 20's gate on z, 4.9e-10 relative (the arithmetic per bin is that of z; the sum is longer).  True peaks:
14 * 2^-24 * S * max|x| with S = max_p sum_k |h[p + f k]| (about 1.92): twelve fused multiply-adds, the rounding of the product and the
compare.  Selections, counts, sample peaks and z_m: equality."""
import math
import os

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import loudness as ld
from svs_unet_pytorch_amd import resample as rs

pytestmark = pytest.mark.gpu
DEV = "cuda"
Z_BOUND = 4.9e-10            # tests/test_gpu_loudness.py, DESIGN.md section 20
U24 = 2.0 ** -24


def noise(shape, seed, scale=0.1):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------
# series
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stems", [1, 2])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("fs", [8192, 44100, 48000])
def test_series_match_the_definition(fs, channels, stems, report):
    """n = e_30 - 1: momentary windows and no short-term window; n = e_30: exactly one; n = e_33 + 37: four and a ragged tail."""
    for n, n_s in ((ld.edge(30, fs) - 1, 0), (ld.edge(30, fs), 1), (ld.edge(33, fs) + 37, 4)):
        x = noise((stems, channels, n) if stems == 2 else (channels, n), seed=fs + 10 * channels + stems)
        xd = dev(x)
        z_m, z_s = ld.series_gpu(xd, fs, stems)
        assert z_m.dtype == z_s.dtype == torch.float64 and z_s.numel() == n_s == ld.nwindows(n, fs, 30) and z_m.numel() == ld.nblocks(n, fs)
        assert torch.equal(z_m, ld.block_energies_gpu(xd, fs, stems))                   # bit for bit
        again = ld.series_gpu(xd, fs, stems)
        assert torch.equal(again[0], z_m) and torch.equal(again[1], z_s)
        want = ld.window_energies_reference(x, fs, 30, stems=stems if stems == 2 else None)
        e = float((np.abs(z_s.cpu().numpy() - want) / want).max()) if n_s else 0.0
        print(f"series fs={fs} channels={channels} stems={stems} n={n}: {z_m.numel()} momentary, {n_s} short-term, worst relative error of z_s {e:.3e}")
        assert report(f"r128 z_s fs={fs} ch={channels} stems={stems} n={n}", e, Z_BOUND)


def test_series_with_a_row_stride_and_one_series_alone(report):
    fs, n = 44100, ld.edge(33, 44100) + 37
    wide = dev(noise((2, n + 13), seed=5))
    view = wide[:, :n]
    assert view.stride(0) == n + 13
    z_m, z_s = ld.series_gpu(view, fs)
    assert torch.equal(z_m, ld.block_energies_gpu(view, fs))
    c_m, c_s = ld.series_gpu(view.contiguous(), fs)
    assert torch.equal(c_m, z_m) and torch.equal(c_s, z_s)
    want = ld.window_energies_reference(view.cpu().numpy(), fs, 30)
    e = float((np.abs(z_s.cpu().numpy() - want) / want).max())
    assert report("r128 z_s with a row stride", e, Z_BOUND)
    # z_s alone (z_m NULL): the same bits
    L = _lib.lib()
    nbytes = int(L.svs_loudness_workspace_bytes(n, 2, fs))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    only = torch.zeros_like(z_s)
    _lib.check(L.svs_loudness_series(view.data_ptr(), 1, 2, n, 0, n + 13, fs, None, only.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()),
               "svs_loudness_series")
    assert torch.equal(only, z_s)


# ------------------------------------------------------------------------------------------------
# stats
# ------------------------------------------------------------------------------------------------
def synthetic_series(n, seed):
    """Log-uniform energies over 60 dB with duplicated values, zeros and entries under the absolute gate."""
    rng = np.random.default_rng(seed)
    z = 10.0 ** rng.uniform(-6.5, -0.5, n)
    if n >= 10:
        idx = rng.permutation(n)
        k = max(1, n // 10)
        z[idx[:k]] = z[idx[k:2 * k]]                                # duplicates
        z[idx[2 * k:2 * k + max(1, k // 2)]] = 0.0                   # zeros
        z[idx[3 * k:3 * k + max(1, k // 2)]] = 10.0 ** rng.uniform(-9.0, -7.5, max(1, k // 2))      # under -70
    return z


def clear_of_the_gates(z):
    """No reference l_j within 1e-9 LU of either gate: a condition on the input, checked on the reference alone, so that a gate
    decision can never hide a selection error."""
    l = ld._lufs(z)
    first = l > ld.ABSOLUTE_GATE
    ok = not np.any(np.abs(l[np.isfinite(l)] - ld.ABSOLUTE_GATE) <= 1e-9)
    if first.any():
        gamma = float(ld._lufs(z[first].mean())) + ld.LRA_RELATIVE_GATE
        ok = ok and not np.any(np.abs(l[np.isfinite(l)] - gamma) <= 1e-9)
    return ok


@pytest.mark.parametrize("n_s", [0, 1, 2, 10, 11, 255, 256, 257, 4097, 36000])
def test_stats_select_exactly(n_s, report):
    z_s = synthetic_series(n_s, seed=100 + n_s)
    z_m = synthetic_series(n_s + 26 if n_s else 0, seed=200 + n_s)
    assert clear_of_the_gates(z_s)
    lra, l_lo, l_hi, kept, z_lo, z_hi = ld.loudness_range(z_s)
    got = ld.stats_gpu(dev(z_m), dev(z_s)).cpu().numpy()
    again = ld.stats_gpu(dev(z_m), dev(z_s)).cpu().numpy()
    assert np.array_equal(got, again, equal_nan=True)
    print(f"stats n_s={n_s}: reference LRA {lra!r} kept {kept} z_lo {z_lo!r} z_hi {z_hi!r}; device {got.tolist()}")
    assert got[3] == kept
    assert got[6] == z_lo and got[7] == z_hi                        # exact selections
    if kept:
        assert abs(got[4] - l_lo) <= 1e-12 and abs(got[5] - l_hi) <= 1e-12
        assert report(f"r128 LRA n_s={n_s} (LU)", abs(got[2] - lra), 1e-12)
    else:
        assert got[2] == 0.0 and got[4] == -np.inf and got[5] == -np.inf
    for i, z in ((0, z_m), (1, z_s)):
        want = ld.max_loudness(z)
        assert got[i] == want if want == -math.inf else abs(got[i] - want) <= 1e-12


def test_stats_with_equal_values_and_nothing_kept():
    same = np.full(300, 1e-3)
    got = ld.stats_gpu(dev(same), dev(same)).cpu().numpy()
    assert got[2] == 0.0 and got[3] == 300 and got[6] == got[7] == 1e-3
    quiet = np.full(50, 1e-9)
    got = ld.stats_gpu(dev(quiet[:0]), dev(quiet)).cpu().numpy()
    assert got[0] == -np.inf and got[2] == 0.0 and got[3] == 0 and got[4] == got[5] == -np.inf and got[6] == got[7] == 0.0
    assert abs(got[1] - float(ld._lufs(1e-9))) <= 1e-12


def test_loud_then_quiet_end_to_end(report):
    """6 s of noise, then 6 s of it 12 dB lower, at 8,192 Hz: series and stats against the reference."""
    fs = 8192
    a = noise((2, 6 * fs), seed=21)
    x = np.concatenate([a, noise((2, 6 * fs), seed=22) * np.float32(10 ** (-12 / 20))], axis=1)
    want = ld.meter_reference(x, fs)
    lra, l_lo, l_hi, kept, z_lo, z_hi = ld.loudness_range(want["z_s"])
    l = ld._lufs(want["z_s"])
    gamma = float(ld._lufs(want["z_s"].mean())) - 20.0
    assert np.abs(l + 70.0).min() > 0.01 and np.abs(l - gamma).min() > 0.01 and lra > 6.0      # conditions on the input
    info, stats, tp = ld.meter_gpu(dev(x), fs)
    got = ld.meter_values(info, stats, tp)
    stats = stats.cpu().numpy()
    print(f"loud then quiet: reference {[want[k] for k in ('I', 'LRA', 'max_M', 'max_S', 'max_dBTP')]} kept {kept}; device {got} kept {stats[3]}")
    assert stats[3] == kept
    tol = 2.0 * 10.0 * math.log10(1.0 + Z_BOUND)                    # two energies, each within Z_BOUND
    assert report("r128 end to end LRA (LU)", abs(got["LRA"] - lra), tol)
    for key in ("I", "max_M", "max_S"):
        assert abs(got[key] - want[key]) <= 1e-6, key
    assert abs(got["max_dBTP"] - want["max_dBTP"]) <= 1e-4


# ------------------------------------------------------------------------------------------------
# true peaks
# ------------------------------------------------------------------------------------------------
def taps32(f):
    return ld.true_peak_taps(f).astype(np.float32)


def tap_sum(f):
    h = np.abs(taps32(f).astype(np.float64))
    return max(h[p::f][:12].sum() for p in range(1, f)) if f > 1 else 0.0


@pytest.mark.parametrize("n", [1, 5, 6, 7, 1023, 1024, 1025, 70001])
@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("f", [1, 2, 4])
def test_true_peaks_within_the_derived_bound(f, rows, n, report):
    """Shorter than the halo, at the halo, across a vector's and a block's edge (a block is 2048 samples); odd n leaves the rows at every
    alignment.  Noise, and a unit impulse at sample 0 and at sample n - 1."""
    shape = (2, 2, n) if rows == 4 else (n,)
    first, last = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    first[..., 0], last[..., n - 1] = 1.0, -1.0
    for name, x in (("noise", noise(shape, seed=7 * n + rows + f, scale=0.3)), ("impulse at 0", first), ("impulse at n-1", last)):
        xd = dev(x)
        sp, tp = ld.true_peaks_gpu(xd, 48000, 2 if rows == 4 else 1, factor=f)
        assert sp.shape == tp.shape == (rows,) and sp.dtype == tp.dtype == torch.float32
        assert torch.equal(sp, xd.abs().reshape(rows, n).amax(dim=1))                    # bit for bit
        assert bool((tp >= sp).all())
        want_s, want_t = ld.true_peak_reference(x.reshape(rows, n).astype(np.float64), taps=taps32(f).astype(np.float64), factor=f)
        bound = 14.0 * U24 * tap_sum(f) * float(np.abs(x).max())
        e = float(np.abs(tp.cpu().numpy().astype(np.float64) - want_t).max())
        assert report(f"true peaks f={f} rows={rows} n={n} {name}", e, bound)
        if f == 1:
            assert torch.equal(tp, sp)


def test_true_peak_of_the_quarter_rate_sine():
    i = np.arange(4800)
    w = np.ones(4800)
    w[:480] = 0.5 - 0.5 * np.cos(np.pi * np.arange(480) / 480)
    w[-480:] = w[:480][::-1]
    x = (0.5 * np.sin(2.0 * np.pi * 0.25 * i + math.radians(45.0)) * w).astype(np.float32)
    sp, tp = ld.true_peaks_gpu(dev(x), 48000)
    print(f"fs/4 at 45 degrees, amplitude 0.5: sample peak {sp.item():.6f}, true peak {tp.item():.6f}")
    assert abs(sp.item() - 0.3536) <= 1e-4 and abs(tp.item() - 0.5) <= 1e-3


# ------------------------------------------------------------------------------------------------
# the way out
# ------------------------------------------------------------------------------------------------
def peaky(fs=44100, seconds=2):
    """Quiet noise with a 12 ms burst of a sine at fs/4 sampled at 45 degrees (sample peak 0.3536, true peak 0.5)."""
    n = seconds * fs
    x = noise((2, n), seed=31, scale=1e-3).astype(np.float64)
    m = 529
    w = np.ones(m)
    w[:220] = 0.5 - 0.5 * np.cos(np.pi * np.arange(220) / 220)
    w[-220:] = w[:220][::-1]
    x[:, fs:fs + m] += 0.5 * np.sin(2.0 * np.pi * 0.25 * np.arange(m) + math.radians(45.0)) * w
    return x.astype(np.float32)


def test_true_peak_ceiling_on_the_way_out(report):
    fs, ceiling = 44100, 0.9
    x = peaky(fs)
    L = ld.loudness_reference(x, fs)[0]
    sample, true = ld.true_peak_reference(x.astype(np.float64), fs)
    unlimited = 10.0 ** ((-10.0 - L) / 20.0)
    # conditions on the input, float64 on the host: the ceiling binds under the true peak, and a sample-peak rule leaves the true peak above it
    assert unlimited > 1.05 * ceiling / true.max() and min(unlimited, ceiling / sample.max()) * true.max() > 1.2 * ceiling
    S = tap_sum(4)
    out, info = rs.resample_encode_gpu(dev(x), 1, 1, fmt="float32", loudness=-10.0, rate=fs, ceiling=ceiling, true_peak=True)
    out, info = out.cpu().numpy(), info.cpu().numpy()
    written = ld.true_peak_reference(out.T.astype(np.float64), fs)[1].max()
    bound = ceiling * (1.0 + 2.0 ** -23) + 14.0 * U24 * S * float(np.abs(out).max())
    print(f"way out, true_peak=True: written true peak {written!r} (bound {bound!r}), info {info.tolist()}")
    assert info[3] == 1
    assert report("way out true peak under the ceiling (excess)", max(0.0, written - bound), 0.0)
    assert written > 0.99 * ceiling                                 # the ceiling is what limited it
    off, info0 = rs.resample_encode_gpu(dev(x), 1, 1, fmt="float32", loudness=-10.0, rate=fs, ceiling=ceiling, true_peak=False)
    above = ld.true_peak_reference(off.cpu().numpy().T.astype(np.float64), fs)[1].max()
    print(f"way out, true_peak=False: written true peak {above!r}, sample peak {float(off.abs().max())!r}")
    assert above > ceiling and float(off.abs().max()) <= ceiling
    # without a target: the peak rule against the true peaks
    pk = rs.resample_encode_gpu(dev(x), 1, 1, fmt="float32", peak=0.9, rate=fs, true_peak=True).cpu().numpy()
    got = ld.true_peak_reference(pk.T.astype(np.float64), fs)[1].max()
    assert 0.99 * 0.9 < got <= 0.9 * (1.0 + 2.0 ** -22) + 14.0 * U24 * S * float(np.abs(pk).max())


@pytest.fixture(scope="module")
def model():
    from svs_unet_pytorch_amd import synth
    from svs_unet_pytorch_amd.model import UNet
    m = UNet()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state().items()})
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def song(tmp_path_factory, model):
    """(checkpoint, 2 s stereo float32 file at 44.1 kHz, its frames)."""
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import synth
    d = tmp_path_factory.mktemp("r128")
    ck = str(d / "svs_closed_form.pth")
    torch.save({"model_state_dict": model.state_dict()}, ck)
    n, rate = 2 * 44100, 44100
    mix = (0.5 * np.stack([synth.audio(n, 50), 0.7 * synth.audio(n, 51)], axis=1)).astype(np.float32)
    mix *= np.float32(0.5 / np.abs(mix).max())
    src = str(d / "mixture.wav")
    wavfile.write(src, rate, mix)
    return ck, src, mix


def test_separate_cli_true_peak(song, tmp_path, report, capsys):
    """separate.py --tar_accomp --loudness source --true_peak: one gain for both files, and where the ceiling does not bind their sum
    reads what the same command writes without the flag."""
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import separate
    ck, src, mix = song
    files = {}
    for tag, extra in (("off", []), ("on", ["--true_peak"])):
        v, a = str(tmp_path / f"{tag}_v.wav"), str(tmp_path / f"{tag}_a.wav")
        separate.main(["--model_path", ck, "--src", src, "--subtype", "FLOAT", "--tar", v, "--tar_accomp", a, "--loudness", "source"] + extra)
        line = [l for l in capsys.readouterr().out.splitlines() if "LUFS" in l]
        assert len(line) == 1 and ("dBTP" in line[0]) == (tag == "on")
        files[tag] = (wavfile.read(v)[1].astype(np.float64), wavfile.read(a)[1].astype(np.float64), line[0])
    (v0, a0, line0), (v1, a1, line1) = files["off"], files["on"]
    cv, ca = float((v1 * v0).sum() / (v0 * v0).sum()), float((a1 * a0).sum() / (a0 * a0).sum())
    print(f"separate --true_peak: gain ratio on / off vocal {cv!r} accompaniment {ca!r}; {line1}")
    assert abs(cv - ca) <= 1e-6 * abs(cv)                           # both files carry one gain
    assert np.abs(v1 - cv * v0).max() <= 1e-6 and np.abs(a1 - ca * a0).max() <= 1e-6
    if "limited" not in line1 and "limited" not in line0:
        got, want = ld.loudness_reference((v1 + a1).T, 44100)[0], ld.loudness_reference((v0 + a0).T, 44100)[0]
        assert report("separate --true_peak, sum vs the same without the flag (LU)", abs(got - want), 0.01)
    assert "true-peak ceiling" in line1 or "limited" not in line1
    tp = ld.true_peak_reference(np.concatenate([v1.T, a1.T]), 44100)[1].max()
    assert tp <= 0.9 * (1.0 + 2.0 ** -22) + 14.0 * U24 * tap_sum(4) * max(np.abs(v1).max(), np.abs(a1).max())


def test_report_carries_the_written_peaks(song, model, tmp_path):
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import streaming
    ck, src, mix = song
    for kw in ({"loudness": -16.0}, {}):
        report = {}
        v, a = str(tmp_path / "v.wav"), str(tmp_path / "a.wav")
        streaming.separate_to_wav(model, src, v, subtype="FLOAT", dst_accomp_path=a, report=report, true_peak=True, **kw)
        assert ("info" in report) == bool(kw)
        written = np.stack([wavfile.read(v)[1].T, wavfile.read(a)[1].T]).astype(np.float64)          # (files, channels, n)
        sample, true = ld.true_peak_reference(written.reshape(4, -1), 44100)
        got_s, got_t = np.array(report["sample_peaks"]), np.array(report["true_peaks"])
        assert got_s.shape == got_t.shape == (2, 2)
        assert np.abs(got_s.ravel() - 20 * np.log10(sample)).max() <= 1e-3 and np.abs(got_t.ravel() - 20 * np.log10(true)).max() <= 1e-3
        if not kw:                                                  # the peak rule: each file's loudest channel at true peak 0.9
            assert np.abs(got_t.max(axis=1) - 20 * math.log10(0.9)).max() <= 1e-3


def parent_encode_planar(buf, frames, fmt, loudness=None, ceiling=0.9, rate=None, peak=0.9):
    """encode_planar_gpu as it stood before true_peak=, restated on the library's entry points: svs_resample_peaks per stem, the
    loudness rule or the peak rule, svs_resample_encode 1/1."""
    code, dtype = rs.pcm_format(fmt)
    nst, channels, width = buf.shape
    L = _lib.lib()
    one, _ = rs.tap_table(1, 1, buf.device)
    peaks = torch.empty(nst * channels, dtype=torch.float32, device=DEV)
    nbytes = int(L.svs_resample_peaks_workspace_bytes(frames, channels, 1, 1, 1))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    outs = [torch.empty((frames, channels), dtype=getattr(torch, np.dtype(dtype).name), device=DEV) for _ in range(nst)]
    s = _lib.stream_ptr()
    for k in range(nst):
        _lib.check(L.svs_resample_peaks(buf[k].data_ptr(), channels, frames, width, one.data_ptr(), 1, 1, 1, peaks[k * channels:].data_ptr(),
                                        ws.data_ptr(), nbytes, s), "svs_resample_peaks")
    if loudness is not None:
        view = buf[:, :, :frames]
        gain, _ = ld.loudness_gain_gpu(view if nst == 2 else view[0], rate, loudness, ceiling=ceiling, stems=nst, peaks=peaks, channels=channels)
        gains = [gain] * nst
    else:
        gains = [torch.full((channels,), float(peak), dtype=torch.float32, device=DEV) for _ in range(nst)]
        top = torch.empty(nst, dtype=torch.float32, device=DEV)
        for k, gain in enumerate(gains):
            _lib.check(L.svs_max(peaks[k * channels:].data_ptr(), channels, top[k:].data_ptr(), s), "svs_max")
            _lib.check(L.svs_scale_by_inv(gain.data_ptr(), channels, top[k:].data_ptr(), 1.0, s), "svs_scale_by_inv")
    for k, out in enumerate(outs):
        _lib.check(L.svs_resample_encode(buf[k].data_ptr(), channels, frames, width, one.data_ptr(), 1, 1, 1, gains[k].data_ptr(), code,
                                         out.data_ptr(), s), "svs_resample_encode")
    return [o.cpu().numpy() for o in outs]


def test_flag_absent_writes_the_bytes_of_the_path_before(song, model, tmp_path):
    """Without true_peak the files are byte for byte those of the path as it stood: the peak rule, a loudness target, and fullband."""
    from fractions import Fraction

    from scipy.io import wavfile

    from svs_unet_pytorch_amd import data, fullband as fb, streaming
    ck, src, mix = song
    rate, pcm, channels = data.read_pcm(src)
    n = pcm.shape[0]
    fr = Fraction(8192, rate)
    pcm_d = dev(pcm)
    y = rs.resample_poly_gpu(pcm_d, fr.numerator, fr.denominator, channels=channels, downmix=False)

    def same(paths, encs):
        for path, enc in zip(paths, encs):
            ref = path + ".ref.wav"
            wavfile.write(ref, rate, enc)
            assert open(ref, "rb").read() == open(path, "rb").read(), path

    def run(tag, **kw):
        paths = [str(tmp_path / f"{tag}_{s}.wav") for s in "va"]
        streaming.separate_to_wav(model, src, paths[0], subtype="FLOAT", dst_accomp_path=paths[1], **kw)
        return paths

    sep = streaming.separate_waveform(model, y, peak=None, both_stems=True)
    # the peak rule
    encs = []
    for stem in sep:
        enc = rs.resample_encode_gpu(stem, fr.denominator, fr.numerator, fmt="FLOAT", peak=0.9, common_gain=True)
        keep, pad = streaming.kept_length(enc.shape[0], n)
        encs.append(torch.nn.functional.pad(enc[:keep], (0, 0, 0, pad)).cpu().numpy())
    same(run("plain"), encs)
    # a loudness target: the stems resampled into one buffer, cut or padded to the source's frames
    up = [rs.resample_poly_gpu(stem.contiguous(), fr.denominator, fr.numerator) for stem in sep]
    n_out = up[0].shape[-1]
    buf = torch.zeros((2, channels, max(n_out, n)), dtype=torch.float32, device=DEV)
    for k, u in enumerate(up):
        buf[k, :, :n_out] = u
    same(run("lufs", loudness=-20.0), parent_encode_planar(buf, n, "FLOAT", loudness=-20.0, rate=rate))
    # fullband mask, with the peak rule and with a target
    aux = {}
    sep = streaming.separate_waveform(model, y, peak=None, both_stems=True, aux=aux)
    T = aux["frames"]
    gf = fb.frame_gains_gpu(aux["tiles"], aux["mask"], T)
    n_out = int(_lib.lib().svs_resample_out_len(sep.shape[2], fr.denominator, fr.numerator))
    buf = fb.fullband_mix_gpu(sep.contiguous(), y, pcm_d, aux["norm"], gf, T, streaming.HOP_SIZE, fr.denominator, fr.numerator, invert=False, width=max(n_out, n))
    same(run("fb", fullband="mask"), parent_encode_planar(buf, n, "FLOAT"))
    same(run("fb_lufs", fullband="mask", loudness=-20.0), parent_encode_planar(buf, n, "FLOAT", loudness=-20.0, rate=rate))


def test_meter_cli_agrees_with_the_host(song, tmp_path, capsys):
    ck, src, mix = song
    csv = [str(tmp_path / "host.csv"), str(tmp_path / "device.csv")]
    ld.main(["--src", src, "--r128", "--device", "cpu", "--series_csv", csv[0]])
    host = capsys.readouterr().out.splitlines()
    ld.main(["--src", src, "--r128", "--device", "gpu", "--series_csv", csv[1]])
    device = capsys.readouterr().out.splitlines()
    print(host, device)
    assert len(host) == 1 and host == device and "dBTP" in host[0]
    rows = [open(p).read().splitlines() for p in csv]
    assert rows[0] == rows[1] and len(rows[0]) == 1 + ld.nblocks(mix.shape[0], 44100)
