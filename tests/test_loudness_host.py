"""Integrated loudness (ITU-R BS.1770-4 / EBU R 128), the host half (no GPU): the K-weighting coefficients against the standard's
48 kHz table, svs_loudness_coeffs and svs_loudness_nblocks against the Python bit for bit, the float64 definition
(loudness.loudness_reference) on the standard's and EBU Tech 3341's signals, inputs that keep no block, the argument rules of the
new entry points before any launch, and the command line's refusal of `--loudness source` without --tar_accomp."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import loudness as ld

NAMES = ("svs_loudness_coeffs", "svs_loudness_nblocks", "svs_loudness_workspace_bytes", "svs_loudness_blocks", "svs_loudness_gain")
RATES = (8192, 22050, 44100, 48000)


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def err(lib):
    return lib.svs_last_error_string().decode()


def test_symbols_are_declared_and_bound(lib):
    syms = _lib.header_symbols()
    for name in NAMES:
        assert name in syms and name in _lib._SIGS and hasattr(lib, name), name
    assert lib.svs_version() == 1


def test_coefficients_reproduce_the_standards_table():
    (b1, a1), (b2, a2) = ld.k_weighting(48000)
    table = [(b1, [1.53512485958697, -2.69169618940638, 1.19839281085285]), (a1, [1.0, -1.69065929318241, 0.73248077421585]),
             (b2, [1.0, -2.0, 1.0]), (a2, [1.0, -1.99004745483398, 0.99007225036621])]
    worst = max(abs(g - w) for got, want in table for g, w in zip(got, want))
    print("K-weighting at 48 kHz vs the BS.1770 table:", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("fs", RATES)
def test_library_coefficients_are_the_pythons(lib, fs):
    c = (C.c_double * 10)()
    assert lib.svs_loudness_coeffs(fs, c) == 0
    assert list(c) == ld.coeffs(fs)                                # bit for bit


@pytest.mark.parametrize("fs", RATES)
def test_library_block_count_is_the_pythons(lib, fs):
    for k in range(0, 14):
        for d in (-2, -1, 0, 1, 2):
            n = ld.edge(k, fs) + d
            if n < 0:
                continue
            want = ld.nblocks(n, fs)
            assert lib.svs_loudness_nblocks(n, fs) == want
            assert want == sum(1 for j in range(20) if ld.edge(j + 4, fs) <= n)      # the complete blocks, counted
            if fs % 10 == 0:
                assert want == max(0, 10 * n // fs - 3)
    assert ld.nblocks(ld.edge(4, fs) - 1, fs) == 0 and ld.nblocks(ld.edge(4, fs), fs) == 1


def sine(freq, dbfs, seconds, fs):
    t = np.arange(int(seconds * fs)) / fs
    return 10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * freq * t)


def test_full_scale_997_hz_sine_reads_minus_3_01():
    L = ld.loudness_reference(sine(997.0, 0.0, 5, 48000), 48000)[0]
    print("0 dBFS 997 Hz mono sine:", L)
    assert abs(L + 3.01) <= 0.01


def test_ebu_3341_case_1():
    s = sine(1000.0, -23.0, 20, 48000)
    L = ld.loudness_reference(np.stack([s, s]), 48000)[0]
    print("EBU Tech 3341 case 1:", L)
    assert abs(L + 23.0) <= 0.1


def test_ebu_3341_gating_case():
    s = np.concatenate([sine(1000.0, -36.0, 10, 48000), sine(1000.0, -23.0, 60, 48000), sine(1000.0, -36.0, 10, 48000)])
    L, z, first, kept = ld.loudness_reference(np.stack([s, s]), 48000)
    print("EBU Tech 3341 gating case:", L, "kept", int(kept.sum()), "of", z.size)
    assert abs(L + 23.0) <= 0.1
    assert first.all() and 0 < kept.sum() < z.size               # the -36 dBFS parts pass the absolute gate and fall to the relative one


def test_two_stems_are_measured_as_their_sum():
    rng = np.random.default_rng(0)
    x = 0.1 * rng.standard_normal((2, 2, 30000))
    a = ld.loudness_reference(x, 44100, stems=2)
    b = ld.loudness_reference(x[0] + x[1], 44100)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("x", [np.zeros(100), np.zeros((2, 19199)), np.zeros(48000), 1e-6 * np.random.default_rng(1).standard_normal(48000)],
                         ids=["100 samples", "under 400 ms", "digital silence", "all below -70"])
def test_nothing_kept_reads_minus_infinity_without_warnings(x):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        L, z, first, kept = ld.loudness_reference(x, 48000)
    assert L == -math.inf and not kept.any() and z.size == ld.nblocks(x.shape[-1], 48000)


def test_gain_rule():
    g, unlimited, limited = ld.gain_rule(-30.0, 0.05, -20.0, 0.9)
    assert abs(g - 10 ** 0.5) < 1e-15 and g == unlimited and not limited
    g, unlimited, limited = ld.gain_rule(-30.0, 0.5, -20.0, 0.9)
    assert g == 0.9 / 0.5 and limited and unlimited > g
    assert ld.gain_rule(-math.inf, 0.25, -20.0, 0.9) == (0.9 / 0.25, math.inf, True)            # the peak rule alone
    assert ld.gain_rule(-math.inf, 0.0, -20.0, 0.9) == (1.0, math.inf, False)                   # silence stays as it is


def test_workspace_query_is_zero_for_invalid_arguments(lib):
    assert lib.svs_loudness_workspace_bytes(48000, 2, 48000) > 0
    assert lib.svs_loudness_workspace_bytes(100, 1, 48000) > 0                                   # valid, no block: a token size
    for n, channels, fs in ((-1, 2, 48000), (48000, 0, 48000), (48000, 9, 48000), (48000, 2, 0), (48000, 2, 3999), (48000, 2, 768001)):
        assert lib.svs_loudness_workspace_bytes(n, channels, fs) == 0, (n, channels, fs)
    assert lib.svs_loudness_nblocks(-1, 48000) == -1 and "svs_loudness_nblocks" in err(lib)
    assert lib.svs_loudness_nblocks(48000, 100) == -1
    assert lib.svs_loudness_coeffs(100, (C.c_double * 10)()) == -1 and "fs must be in" in err(lib)


# (stems, channels, n, ld_ch, fs) -> the words of the rule's message; every pointer NULL, so a launch would come back differently
BLOCK_RULES = [
    ((0, 2, 48000, 48000, 48000), "stems must be 1 or 2"),
    ((3, 2, 48000, 48000, 48000), "stems must be 1 or 2"),
    ((1, 0, 48000, 48000, 48000), "channels must be in 1..8"),
    ((1, 9, 48000, 48000, 48000), "channels must be in 1..8"),
    ((1, 2, 48000, 48000, 3999), "fs must be in"),
    ((1, 2, -5, 48000, 48000), "n must not be negative"),
    ((1, 2, 48000, 47999, 48000), "ld_ch must be at least n"),
    ((1, 2, 48000, 48000, 48000), "null pointer"),
]


@pytest.mark.parametrize("args,msg", BLOCK_RULES)
def test_blocks_refuses_before_any_launch(lib, args, msg):
    stems, channels, n, ld_ch, fs = args
    assert lib.svs_loudness_blocks(None, stems, channels, n, channels * ld_ch, ld_ch, fs, None, None, 0, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_loudness_blocks:")


def test_blocks_under_400_ms_is_a_no_op_and_the_workspace_is_checked(lib):
    assert lib.svs_loudness_blocks(None, 1, 2, 19199, 0, 19199, 48000, None, None, 0, None) == 0     # nothing to write, nothing read
    assert lib.svs_loudness_blocks(64, 1, 2, 48000, 0, 48000, 48000, 64, 64, 8, None) == -2 and "workspace too small" in err(lib)
    assert lib.svs_loudness_blocks(64, 1, 2, 48000, 0, 48000, 48000, 68, 64, 1 << 20, None) == -1 and "8-byte aligned" in err(lib)


@pytest.mark.parametrize("args,msg", [
    ((None, -1, None, 0, math.nan, None, 0.9, None, 0, 64), "nblocks must not be negative"),
    ((None, 0, None, -1, math.nan, None, 0.9, None, 0, 64), "npeaks must not be negative"),
    ((None, 0, None, 0, math.nan, None, 0.9, None, 9, 64), "channels must be in 0..8"),
    ((None, 0, None, 0, math.nan, None, 0.0, None, 0, 64), "ceiling must be positive"),
    ((None, 0, None, 0, math.nan, None, 0.9, None, 0, None), "null pointer"),
    ((None, 5, None, 0, math.nan, None, 0.9, None, 0, 64), "null pointer"),
    ((None, 0, None, 2, math.nan, None, 0.9, None, 0, 64), "null pointer"),
    ((None, 0, None, 0, -23.0, None, 0.9, None, 2, 64), "null pointer"),
    ((None, 0, None, 0, -23.0, None, 0.9, None, 0, 64), "a target needs gain_out"),
    ((None, 0, None, 0, math.nan, None, 0.9, None, 0, 68), "8-byte aligned"),
])
def test_gain_refuses_before_any_launch(lib, args, msg):
    assert lib.svs_loudness_gain(*args, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_loudness_gain:")


def test_python_entry_points_check_their_arguments():
    import torch
    with pytest.raises(ValueError, match="fs must be"):
        ld.k_weighting(100)
    with pytest.raises(ValueError, match="device tensor"):
        ld.block_energies_gpu(torch.zeros(2, 100), 48000)
    with pytest.raises(ValueError, match="first axis"):
        ld.loudness_reference(np.zeros((3, 100)), 48000, stems=2)
    from svs_unet_pytorch_amd import streaming
    with pytest.raises(ValueError, match="source"):
        streaming.separate_to_wav(None, "a.wav", "b.wav", loudness="source")
    assert ld.parse_target("-23") == -23.0 and ld.parse_target("source") == "source"
    for bad in ("loud", "nan", "inf"):
        with pytest.raises(ValueError, match="LUFS"):
            ld.parse_target(bad)


@pytest.mark.parametrize("extra,msg", [(["--loudness", "source"], "--tar_accomp"), (["--loudness", "loud"], "LUFS"),
                                       (["--loudness", "-23", "--peak_ceiling", "0"], "--peak_ceiling")])
def test_cli_refuses_before_the_checkpoint(extra, msg, tmp_path, capsys):
    from svs_unet_pytorch_amd import separate
    missing = str(tmp_path / "no_such_checkpoint.pth")             # loading it would fail with another message
    with pytest.raises(SystemExit) as e:
        separate.main(["--model_path", missing, "--src", str(tmp_path / "in.wav"), "--tar", str(tmp_path / "out.wav")] + extra)
    assert e.value.code not in (0, None)
    text = capsys.readouterr().err
    assert "--loudness" in text and msg in text


def test_cli_help_names_the_flags(capsys):
    from svs_unet_pytorch_amd import separate
    with pytest.raises(SystemExit) as e:
        separate.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--loudness" in text and "--peak_ceiling" in text and "source" in text


def test_loudness_cli_on_the_host(tmp_path, capsys):
    """python -m svs_unet_pytorch_amd.loudness --device cpu: a file and a folder, at the files' own rates."""
    from scipy.io import wavfile
    s = sine(1000.0, -23.0, 3, 44100)
    wavfile.write(str(tmp_path / "a.wav"), 44100, np.stack([s, s], axis=1).astype(np.float32))
    wavfile.write(str(tmp_path / "b.wav"), 48000, np.round(sine(997.0, 0.0, 3, 48000) * 32767).astype(np.int16))
    ld.main(["--src", str(tmp_path), "--device", "cpu"])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0].endswith("LUFS") and "a.wav" in lines[0] and "b.wav" in lines[1]
    got = [float(l.split(": ")[1].split()[0]) for l in lines]
    assert abs(got[0] + 23.0) <= 0.1 and abs(got[1] + 3.01) <= 0.02
