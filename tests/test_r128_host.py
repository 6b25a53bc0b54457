"""The EBU R 128 meter, the host half (no GPU): the float64 definitions of loudness.py -- window counts and energies, loudness range
on EBU Tech 3342's four signals, true peak on faded sines -- the interpolator's taps, the over-sampling factor by rate, the new
entry points' declarations and their argument rules before any launch, and the command lines."""
import ctypes as C
import math

import numpy as np
import pytest

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import loudness as ld

NAMES = ("svs_loudness_nwindows", "svs_loudness_series", "svs_loudness_stats_workspace_bytes", "svs_loudness_stats",
         "svs_true_peaks_workspace_bytes", "svs_true_peaks")


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def err(lib):
    return lib.svs_last_error_string().decode()


def test_symbols_are_declared_and_bound(lib):
    syms = _lib.header_symbols()
    for name in NAMES:
        assert name in syms and name in _lib._SIGS and hasattr(lib, name), name


# ------------------------------------------------------------------------------------------------
# windows and loudness range
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [8192, 44100, 48000])
def test_window_count_against_brute_force(lib, fs):
    for w in (1, 4, 30):
        for n in list(range(ld.edge(30, fs) - 3, ld.edge(30, fs) + 4)) + [0, 1, ld.edge(w, fs) - 1, ld.edge(w, fs), ld.edge(33, fs) + 37]:
            want = sum(1 for j in range(60) if ld.edge(j + w, fs) <= n)
            assert ld.nwindows(n, fs, w) == want, (n, fs, w)
            assert lib.svs_loudness_nwindows(n, fs, w) == want
            if w == 4:
                assert want == ld.nblocks(n, fs) == lib.svs_loudness_nblocks(n, fs)
    assert ld.nwindows(ld.edge(30, fs) - 1, fs, 30) == 0 and ld.nwindows(ld.edge(30, fs), fs, 30) == 1


def test_window_count_refuses_invalid_arguments(lib):
    for n, fs, bins in ((-1, 48000, 4), (48000, 100, 4), (48000, 48000, 0), (48000, 48000, 601)):
        assert lib.svs_loudness_nwindows(n, fs, bins) == -1 and err(lib).startswith("svs_loudness_nwindows:"), (n, fs, bins)
    assert lib.svs_loudness_nwindows(48000 * 70, 48000, 600) == 101


def test_four_bin_windows_are_the_blocks_exactly():
    rng = np.random.default_rng(3)
    x = 0.1 * rng.standard_normal((2, 2, 30011))
    assert np.array_equal(ld.window_energies_reference(x[0], 44100, 4), ld.loudness_reference(x[0], 44100)[1])
    assert np.array_equal(ld.window_energies_reference(x, 44100, 4, stems=2), ld.loudness_reference(x, 44100, stems=2)[1])
    assert ld.window_energies_reference(x[0], 8192, 30).shape == (ld.nwindows(30011, 8192, 30),)


def segments(levels, seconds=20, fs=48000):
    t = np.arange(seconds * fs) / fs
    s = np.concatenate([10.0 ** (db / 20.0) * np.sin(2.0 * np.pi * 1000.0 * t) for db in levels])
    return np.stack([s, s])


@pytest.mark.parametrize("levels,want", [((-20, -30), 10.0), ((-20, -15), 5.0), ((-40, -20), 20.0), ((-50, -35, -20, -35, -50), 15.0)])
def test_tech_3342_cases(levels, want):
    """EBU Tech 3342's four signals, 1 kHz stereo sines at 48 kHz in 20 s segments: within the document's +-1 LU, and within 1e-9 LU of
    the whole number, which the definition gives on these signals."""
    z = ld.window_energies_reference(segments(levels), 48000, ld.BINS_S)
    lra, l_lo, l_hi, kept, z_lo, z_hi = ld.loudness_range(z)
    print("Tech 3342", levels, "LRA", lra, "kept", kept, "of", z.size)
    assert abs(lra - want) <= 1.0
    assert abs(lra - want) <= 1e-9
    assert 0 < kept <= z.size and z_lo <= z_hi and abs((l_hi - l_lo) - lra) == 0.0


def test_loudness_range_is_zero_at_a_constant_level_and_without_a_window():
    t = np.arange(10 * 48000) / 48000.0
    s = 0.1 * np.sin(2.0 * np.pi * 1000.0 * t)
    m = ld.meter_reference(np.stack([s, s]), 48000)
    assert abs(m["LRA"]) <= 1e-9 and m["z_s"].size == 71
    short = ld.meter_reference(s[: 3 * 48000 - 1], 48000)
    assert short["z_s"].size == 0 and short["LRA"] == 0.0 and short["max_S"] == -math.inf and short["max_M"] > -30.0
    assert ld.loudness_range(np.zeros(5)) == (0.0, -math.inf, -math.inf, 0, 0.0, 0.0)
    assert ld.max_loudness(np.zeros(0)) == -math.inf


def test_loudness_range_picks_nearest_ranks():
    z = 10.0 ** (np.arange(21.0) / 10.0 - 3.0)                      # 21 levels 1 dB apart, all above both gates
    lra, l_lo, l_hi, kept, z_lo, z_hi = ld.loudness_range(z[::-1])
    assert kept == 21 and z_lo == z[2] and z_hi == z[19] and abs(lra - 17.0) <= 1e-12


# ------------------------------------------------------------------------------------------------
# true peak
# ------------------------------------------------------------------------------------------------
def faded_sine(amp, cycles_per_sample, phase_deg, n=4800, ramp=480):
    i = np.arange(n)
    s = amp * np.sin(2.0 * np.pi * cycles_per_sample * i + math.radians(phase_deg))
    w = np.ones(n)
    w[:ramp] = 0.5 - 0.5 * np.cos(np.pi * np.arange(ramp) / ramp)
    w[n - ramp:] = w[:ramp][::-1]
    return s * w


@pytest.mark.parametrize("amp,freq,phase", [(0.5, 1 / 4, 0.0), (0.5, 1 / 4, 45.0), (0.5, 1 / 6, 60.0), (0.5, 1 / 8, 67.5), (1.41, 1 / 4, 45.0)])
def test_true_peak_of_faded_sines(amp, freq, phase):
    """Sines with 10 ms raised-cosine fades (an abrupt onset has real inter-sample content and over-reads): the true peak reads the
    sine's amplitude within +0.2 / -0.4 dB.  That tolerance is the one EBU Tech 3341 gives its true-peak cases, quoted from memory of
    that document."""
    sample, true = ld.true_peak_reference(faded_sine(amp, freq, phase), 48000)
    d = 20.0 * math.log10(true / amp)
    print(f"amplitude {amp} at fs*{freq:.4f}, {phase} deg: true peak {20 * math.log10(true):+.3f} dBTP ({d:+.4f} dB), sample peak {20 * math.log10(sample):+.3f} dBFS")
    assert -0.4 <= d <= 0.2
    assert true >= sample
    if amp == 1.41:
        assert abs(20.0 * math.log10(true / sample) - 3.0) <= 0.1     # the sample peak reads 3 dB low


def test_true_peak_shapes_and_edges():
    x = np.zeros((3, 40))
    x[0, 0], x[1, 39], x[2, 20] = 1.0, -1.0, 0.5
    sample, true = ld.true_peak_reference(x, 44100)
    assert sample.tolist() == [1.0, 1.0, 0.5] and (true >= sample).all()
    assert ld.true_peak_reference(x[2], 44100) == (sample[2], true[2])
    s1, t1 = ld.true_peak_reference(x, 192000)
    assert np.array_equal(s1, t1)                                   # factor 1: the sample peak
    assert ld.true_peak_reference(np.zeros(0), 48000) == (0.0, 0.0)
    m = ld.meter_reference(np.zeros((2, 1000)), 48000)
    assert m["max_dBTP"] == -math.inf and m["I"] == -math.inf


@pytest.mark.parametrize("f", [1, 2, 4])
def test_taps(f):
    h = ld.true_peak_taps(f)
    assert h.shape == (12 * f + 1,) and h.dtype == np.float64
    assert h[6 * f] == 1.0
    assert all(h[t] == 0.0 for t in range(0, 12 * f + 1, f) if t != 6 * f)
    assert np.array_equal(h, h[::-1])
    if f > 1:
        S = max(np.abs(h[p::f][:12]).sum() for p in range(1, f))
        print("factor", f, "S = max_p sum_k |h[p + f k]| =", S)
        assert 1.5 < S < 2.0
    with pytest.raises(ValueError):
        ld.true_peak_taps(3)


def test_factor_by_rate():
    assert [ld.true_peak_factor(fs) for fs in (8192, 44100, 48000, 95999, 96000, 191999, 192000, 384000)] == [4, 4, 4, 4, 2, 2, 1, 1]


# ------------------------------------------------------------------------------------------------
# argument rules, every pointer NULL: a launch would come back differently
# ------------------------------------------------------------------------------------------------
SERIES_RULES = [
    ((0, 2, 48000, 48000, 48000), "stems must be 1 or 2"),
    ((3, 2, 48000, 48000, 48000), "stems must be 1 or 2"),
    ((1, 0, 48000, 48000, 48000), "channels must be in 1..8"),
    ((1, 9, 48000, 48000, 48000), "channels must be in 1..8"),
    ((1, 2, 48000, 48000, 3999), "fs must be in"),
    ((1, 2, -5, 48000, 48000), "n must not be negative"),
    ((1, 2, 48000, 47999, 48000), "ld_ch must be at least n"),
    ((1, 2, 48000, 48000, 48000), "null pointer"),
]


@pytest.mark.parametrize("args,msg", SERIES_RULES)
def test_series_refuses_before_any_launch(lib, args, msg):
    stems, channels, n, ld_ch, fs = args
    assert lib.svs_loudness_series(None, stems, channels, n, channels * ld_ch, ld_ch, fs, None, None, None, 0, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_loudness_series:")


def test_series_short_input_workspace_and_alignment(lib):
    assert lib.svs_loudness_series(None, 1, 2, 19199, 0, 19199, 48000, None, None, None, 0, None) == 0       # under 400 ms
    assert lib.svs_loudness_series(64, 1, 2, 48000, 0, 48000, 48000, 64, 64, 64, 8, None) == -2 and "workspace too small" in err(lib)
    assert lib.svs_loudness_series(64, 1, 2, 48000, 0, 48000, 48000, 64, 68, 64, 1 << 20, None) == -1 and "8-byte aligned" in err(lib)
    assert lib.svs_loudness_series(64, 1, 2, 48000, 0, 48000, 48000, None, None, 64, 1 << 20, None) == 0     # neither series asked for


@pytest.mark.parametrize("args,msg", [
    ((None, -1, None, 0, 64, 64, 64), "n_m must not be negative"),
    ((None, 0, None, -1, 64, 64, 64), "n_s must be in"),
    ((None, 0, None, 1 << 31, 64, 64, 64), "n_s must be in"),
    ((None, 0, None, 0, None, 64, 64), "null pointer"),
    ((None, 3, None, 0, 64, 64, 64), "null pointer"),
    ((None, 0, None, 3, 64, 64, 64), "null pointer"),
    ((None, 0, None, 0, 68, 64, 64), "8-byte aligned"),
    ((None, 0, 64, 100, 64, 64, 64), "workspace too small"),
    ((None, 0, None, 0, 64, None, 64), "workspace too small"),
])
def test_stats_refuses_before_any_launch(lib, args, msg):
    assert lib.svs_loudness_stats(*args, None) in (-1, -2)
    assert msg in err(lib) and err(lib).startswith("svs_loudness_stats:")


def test_stats_workspace_query(lib):
    assert lib.svs_loudness_stats_workspace_bytes(36000) == 36000 * 8
    assert lib.svs_loudness_stats_workspace_bytes(0) > 0
    assert lib.svs_loudness_stats_workspace_bytes(-1) == 0 and lib.svs_loudness_stats_workspace_bytes(1 << 31) == 0


# (stems, channels, n, ld_stem, ld_ch, taps, factor, ws, ws_bytes)
@pytest.mark.parametrize("args,msg", [
    ((0, 2, 100, 200, 100, 64, 4, 64, 64), "stems must be in 1..8"),
    ((9, 2, 100, 200, 100, 64, 4, 64, 64), "stems must be in 1..8"),
    ((1, 0, 100, 200, 100, 64, 4, 64, 64), "channels must be in 1..8"),
    ((1, 9, 100, 200, 100, 64, 4, 64, 64), "channels must be in 1..8"),
    ((1, 2, -1, 200, 100, 64, 4, 64, 64), "n must not be negative"),
    ((1, 2, 100, 200, 99, 64, 4, 64, 64), "ld_ch must be at least n"),
    ((2, 2, 100, 199, 100, 64, 4, 64, 64), "ld_stem must be at least"),
    ((1, 2, 100, 200, 100, 64, 3, 64, 64), "factor must be 1, 2 or 4"),
    ((1, 2, 100, 200, 100, 64, 8, 64, 64), "factor must be 1, 2 or 4"),
    ((1, 2, 100, 200, 100, 64, 4, 64, 64), "null pointer"),
])
def test_true_peaks_refuses_before_any_launch(lib, args, msg):
    stems, channels, n, ld_stem, ld_ch, taps, factor, ws, ws_bytes = args
    assert lib.svs_true_peaks(None, stems, channels, n, ld_stem, ld_ch, taps, factor, None, None, ws, ws_bytes, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_true_peaks:")


def test_true_peaks_taps_workspace_and_alignment(lib):
    assert lib.svs_true_peaks(64, 1, 2, 100, 200, 100, None, 4, None, None, 64, 64, None) == -1 and "null pointer" in err(lib)
    assert lib.svs_true_peaks(64, 1, 2, 100, 200, 100, 64, 4, None, None, 64, 8, None) == -2 and "workspace too small" in err(lib)
    assert lib.svs_true_peaks(66, 1, 2, 100, 200, 100, 64, 4, None, None, 64, 64, None) == -1 and "4-byte aligned" in err(lib)
    assert lib.svs_true_peaks(64, 1, 2, 100, 200, 100, None, 1, None, None, 64, 64, None) == 0          # factor 1 reads no taps; no output asked for
    assert lib.svs_true_peaks_workspace_bytes(100, 2) == 16 and lib.svs_true_peaks_workspace_bytes(2049, 4) == 64
    assert lib.svs_true_peaks_workspace_bytes(0, 1) == 8
    for n, rows in ((-1, 2), (100, 0), (100, 65)):
        assert lib.svs_true_peaks_workspace_bytes(n, rows) == 0, (n, rows)


def test_python_entry_points_check_their_arguments():
    import torch
    with pytest.raises(ValueError, match="device tensor"):
        ld.true_peaks_gpu(torch.zeros(2, 100), 48000)
    with pytest.raises(ValueError, match="device tensor"):
        ld.series_gpu(torch.zeros(2, 100), 48000)
    with pytest.raises(ValueError, match="w must be"):
        ld.window_energies_reference(np.zeros(100), 48000, 0)
    with pytest.raises(ValueError, match="taps"):
        ld.true_peak_reference(np.zeros(100), taps=np.zeros(5), factor=4)
    assert "true-peak ceiling" in ld.describe([-23.0, 10.0, 2.0, 1.0], 1.5, True)
    assert ld.describe([-23.0, 10.0, 2.0, 1.0], 1.5) == "-23.00 LUFS, gain +3.52 dB (limited by the peak ceiling)"
    assert "ceiling" not in ld.describe([-23.0, 10.0, 2.0, 0.0], 1.5, True)


# ------------------------------------------------------------------------------------------------
# command lines
# ------------------------------------------------------------------------------------------------
def write_case(tmp_path):
    from scipy.io import wavfile
    t = np.arange(8 * 44100) / 44100.0
    s = np.concatenate([10.0 ** (-23.0 / 20.0) * np.sin(2.0 * np.pi * 1000.0 * t[: 4 * 44100]), 10.0 ** (-33.0 / 20.0) * np.sin(2.0 * np.pi * 1000.0 * t[: 4 * 44100])])
    path = str(tmp_path / "a.wav")
    wavfile.write(path, 44100, np.stack([s, s], axis=1).astype(np.float32))
    return path, np.stack([s, s]).astype(np.float32)


def test_meter_cli_on_the_host(tmp_path, capsys):
    path, x = write_case(tmp_path)
    csv = str(tmp_path / "series.csv")
    ld.main(["--src", path, "--device", "cpu", "--r128", "--series_csv", csv])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 1 and "a.wav" in lines[0]
    want = ld.meter_reference(x.astype(np.float64), 44100)
    for name, key, unit in (("I", "I", "LUFS"), ("LRA", "LRA", "LU"), ("max M", "max_M", "LUFS"), ("max S", "max_S", "LUFS"), ("max TP", "max_dBTP", "dBTP")):
        assert f"{name} {want[key]:.2f} {unit}" in lines[0], (name, lines[0])
    assert abs(want["max_M"] + 23.0) <= 0.1 and abs(want["max_dBTP"] + 23.0) <= 0.1 and want["LRA"] > 1.0
    rows = open(csv).read().splitlines()
    assert rows[0] == "file,time_s,momentary_lufs,short_term_lufs" and len(rows) == 1 + want["z_m"].size
    first, last = rows[1].split(","), rows[-1].split(",")
    assert first[1] == "0.4" and first[3] == "" and abs(float(first[2]) + 23.0) <= 0.1
    assert last[1] == "8.0" and abs(float(last[3]) - float(ld._lufs(want["z_s"][-1]))) <= 1e-3
    assert sum(1 for r in rows[1:] if r.split(",")[3]) == want["z_s"].size


def test_loudness_cli_without_the_flag_prints_the_old_line(tmp_path, capsys):
    path, x = write_case(tmp_path)
    ld.main(["--src", path, "--device", "cpu"])
    lines = capsys.readouterr().out.splitlines()
    assert lines == [f"{path}: {ld.loudness_reference(x.astype(np.float64), 44100)[0]:.2f} LUFS"]
    with pytest.raises(SystemExit):
        ld.main(["--src", path, "--device", "cpu", "--series_csv", str(tmp_path / "s.csv")])


def test_cli_help_names_the_flag(capsys):
    from svs_unet_pytorch_amd import data, separate
    for tool in (separate, data):
        with pytest.raises(SystemExit) as e:
            tool.main(["--help"])
        assert e.value.code == 0
        assert "--true_peak" in capsys.readouterr().out


def test_true_peak_needs_the_written_rate():
    import torch
    from svs_unet_pytorch_amd import resample
    with pytest.raises(ValueError, match="rate="):
        resample.resample_encode_gpu(torch.zeros(4), 1, 1, true_peak=True)
    with pytest.raises(ValueError, match="common gain"):
        resample.resample_encode_gpu(torch.zeros(4), 1, 1, true_peak=True, rate=48000, peak=None)
