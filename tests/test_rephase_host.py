"""Phase refinement (Griffin-Lim / MISI), the host half (no GPU): svs_stft_rephase_n is declared, bound and refuses bad arguments
with its own message before any launch (all device pointers are NULL); the float64 definition rephase.rephase_reference agrees
with the same loop written with torch.stft / torch.istft, and has the property the feature exists for -- the inconsistency
|| |STFT(x)| - M ||^2 / || M ||^2 falls at every iteration; argument errors of the Python layer, the defaults of the public
signatures, and the command line's refusal of a negative --phase_iters before a checkpoint is read."""
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd import rephase as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(512, 384), (1024, 768), (1024, 256), (2048, 1536), (1024, 100)]
ITERS = 4


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def err(lib):
    return lib.svs_last_error_string().decode()


def test_symbol_is_declared_and_bound(lib, tmp_path):
    assert "svs_stft_rephase_n" in _lib.header_symbols() and "svs_stft_rephase_n" in _lib._SIGS and hasattr(lib, "svs_stft_rephase_n")
    res, args = _lib._SIGS["svs_stft_rephase_n"]
    assert res is _lib.I and args == [_lib.P, _lib.L, _lib.I, _lib.P, _lib.L, _lib.I, _lib.I, _lib.I, _lib.P, _lib.L, _lib.P]
    src = tmp_path / "t.c"                                       # the header still compiles as C, and the declaration has this type
    src.write_text('#include "svs_hip.h"\n'
                   "int (*probe)(const float*, int64_t, int, const float*, int64_t, int, int, int, float*, int64_t, hipStream_t) = svs_stft_rephase_n;\n"
                   "int main(void){return probe != svs_stft_rephase_n;}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# (stem_stride, stems, mix, n_samples, channels, n_fft, hop, phase_stem_stride) -> words of the rule's message
N1 = 30725
RULES = [
    ((0, 0, None, N1, 2, 1024, 768, 0), "stems must be 1 or 2"),
    ((0, 3, None, N1, 2, 1024, 768, 0), "stems must be 1 or 2"),
    ((0, 1, 64, N1, 2, 1024, 768, 0), "a mixture needs stems == 2"),
    ((0, 1, None, N1, 2, 768, 256, 0), "n_fft must be 512, 1024 or 2048"),
    ((0, 1, None, N1, 2, 4096, 256, 0), "n_fft must be 512, 1024 or 2048"),
    ((0, 1, None, N1, 2, 1024, 0, 0), "hop 0 is not in 1..n_fft"),
    ((0, 1, None, N1, 2, 1024, 1025, 0), "hop 1025 is not in 1..n_fft"),
    ((0, 1, None, 0, 2, 1024, 768, 0), "must be positive"),
    ((0, 1, None, N1, 0, 1024, 768, 0), "must be positive"),
    ((2 * N1 - 1, 2, None, N1, 2, 1024, 768, 2 * 41 * 513 * 2), "are below one stem's"),
    ((2 * N1, 2, None, N1, 2, 1024, 768, 2 * 41 * 513 * 2 - 2), "are below one stem's"),
    ((2 * N1, 2, None, N1, 2, 1024, 768, 2 * 41 * 513 * 2 + 1), "must be even"),
    ((0, 1, None, 1 << 28, 2, 1024, 768, 0), "2 GiB"),                      # the signals: 2 x 2^28 x 4 B = 2 GiB
    ((0, 1, None, 100 * 300000, 2, 1024, 100, 0), "2 GiB"),                 # the phasors: 2 x 300001 x 513 x 8 B
    ((1 << 29, 2, None, N1, 2, 1024, 768, 2 * 41 * 513 * 2), "2 GiB"),      # the stride between the stems
    ((0, 1, None, N1, 2, 1024, 768, 0), "null pointer"),
    ((2 * N1, 2, None, N1, 2, 512, 384, 2 * 81 * 257 * 2), "null pointer"),
]


@pytest.mark.parametrize("a,msg", RULES)
def test_rephase_refuses_before_any_launch(lib, a, msg):
    stem_stride, stems, mix, n, C, n_fft, hop, pstride = a
    assert lib.svs_stft_rephase_n(None, stem_stride, stems, mix, n, C, n_fft, hop, None, pstride, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_stft_rephase_n:"), err(lib)


def test_misaligned_phase_is_refused(lib):
    assert lib.svs_stft_rephase_n(16, 0, 1, None, N1, 2, 1024, 768, 20, 0, None) == -1 and "8-byte aligned" in err(lib)


# ---- the float64 definition ------------------------------------------------------------------------------------------------

def case(n_fft, hop, stems):
    """synth.audio, two channels of hop * 40 + 5 samples, a uniform random mask, the DC row zeroed."""
    n = hop * 40 + 5
    y = np.stack([synth.audio(n, 0), synth.audio(n, 1)]).astype(np.float64)
    spec = rp.reference_stft(y, n_fft, hop)
    assert spec.shape == (2, n_fft // 2 + 1, 41)
    mask = np.random.default_rng(n_fft + hop).random(spec.shape)
    mag = np.abs(spec)
    mag[:, 0] = 0.0
    mags = np.stack([mag * mask, mag * (1.0 - mask)])[:stems]
    mix = y[:, :hop * 40] if stems == 2 else None
    return mags, rp.reference_phasor(spec), mix


def torch_loop(mags, phase, iters, mix, n_fft, hop):
    """The same loop with torch.stft / torch.istft in float64."""
    win = torch.hann_window(n_fft, dtype=torch.float64)
    M = torch.from_numpy(mags)
    S, C, nbin, T = M.shape
    P = torch.from_numpy(np.broadcast_to(phase, mags.shape).copy())
    mx = None if mix is None else torch.from_numpy(mix)

    def inverse(P):
        return torch.istft((M * P).reshape(S * C, nbin, T), n_fft=n_fft, hop_length=hop, win_length=n_fft, window=win, center=True,
                           return_complex=False).reshape(S, C, -1)

    x = inverse(P)
    for _ in range(iters):
        z = x if mx is None else x + 0.5 * (mx - x[0] - x[1])[None]
        Z = torch.stft(z.reshape(S * C, -1), n_fft, hop, n_fft, win, center=True, pad_mode="constant", return_complex=True).reshape(S, C, nbin, T)
        a = Z.abs()
        P = torch.where(a == 0, torch.ones_like(Z), Z / torch.where(a == 0, torch.ones_like(a), a))
        x = inverse(P)
    return P.numpy(), x.numpy()


@pytest.mark.parametrize("stems", [1, 2])
@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_reference_agrees_with_torch_and_lowers_the_inconsistency(n_fft, hop, stems):
    mags, phase, mix = case(n_fft, hop, stems)
    phases, waves, measure = rp.rephase_reference(mags, phase, ITERS, mix, n_fft=n_fft, hop=hop)
    assert phases.shape == mags.shape and waves.shape == (stems, 2, hop * 40) and measure.shape == (ITERS + 1,)
    _, want = torch_loop(mags, phase, ITERS, mix, n_fft, hop)
    e = np.abs(waves - want).max() / np.abs(want).max()
    print(f"N={n_fft} hop={hop} stems={stems}: vs torch {e:.2e}, inconsistency {measure}")
    assert e <= 1e-9
    assert np.abs(np.abs(phases) - 1).max() <= 1e-12
    # the property, as a statement about the definition: the measure falls at each of the iterations.  One stem:
    # || |STFT(x)| - M ||^2 / || M ||^2; two stems: the sum over both, taken on x_k + (mix - x_0 - x_1) / 2
    assert np.all(np.diff(measure) < 0), measure
    # the measure is what inconsistency() computes from the returned waveforms
    z = waves if mix is None else waves + 0.5 * (mix - waves[0] - waves[1])[None]
    assert abs(rp.inconsistency(z, mags, n_fft, hop).sum() - measure[-1]) <= 1e-12 * measure[-1]
    # and every shorter run is a prefix of the longer one
    _, w2, m2 = rp.rephase_reference(mags, phase, 2, mix, n_fft=n_fft, hop=hop)
    assert np.array_equal(m2[:2], measure[:2]) and abs(m2[2] - measure[2]) <= 1e-12 * measure[2]


def test_reference_zero_iterations_and_zero_bins():
    mags, phase, _ = case(512, 384, 1)
    phases, waves, measure = rp.rephase_reference(mags, phase, 0, n_fft=512, hop=384)
    assert np.array_equal(phases[0], phase) and measure.shape == (1,)
    assert np.array_equal(waves, rp.reference_istft(mags * phase, 512, 384))
    assert np.array_equal(rp.reference_phasor(np.array([0.0 + 0.0j, 0.0 - 4.0j, -0.5 + 0.0j])), np.array([1.0 + 0.0j, 0.0 - 1.0j, -1.0 + 0.0j]))
    # a silent channel: every bin is exactly zero, so every phasor is exactly 1 + 0i and the waveform stays zero
    silent = np.zeros_like(mags)
    p0, w0, _ = rp.rephase_reference(silent[:, :1], phase[:1], 2, n_fft=512, hop=384)
    assert np.all(p0 == 1.0 + 0.0j) and np.all(w0 == 0)


# ---- argument errors ---------------------------------------------------------------------------------------------------------

def test_python_argument_errors():
    from svs_unet_pytorch_amd import streaming
    mags, phase, mix = case(512, 384, 2)
    for bad in (-1, -4, 1.5):
        with pytest.raises(ValueError, match="phase_iters"):
            rp.check_phase_iters(bad)
    assert rp.check_phase_iters(0) == 0 and rp.check_phase_iters(3) == 3
    with pytest.raises(ValueError, match="phase_iters"):                     # refused before the waveform or the model is looked at
        streaming.separate_waveform(None, None, phase_iters=-1)
    with pytest.raises(ValueError, match="phase_iters"):
        rp.refine_phase(None, None, None, 41, -1, stems=1, n_fft=512, hop=384)
    with pytest.raises(ValueError, match="phase_iters"):
        rp.rephase_reference(mags, phase, -1, mix, n_fft=512, hop=384)
    with pytest.raises(ValueError, match="mix"):                             # stems=2 without mix
        rp.refine_phase(None, None, None, 41, 2, stems=2, n_fft=512, hop=384)
    with pytest.raises(ValueError, match="mix"):
        rp.rephase_reference(mags, phase, 2, None, n_fft=512, hop=384)
    with pytest.raises(ValueError, match="stems=1"):                         # mix with stems=1
        rp.refine_phase(None, None, None, 41, 2, stems=1, mix=mix, n_fft=512, hop=384)
    with pytest.raises(ValueError, match="stems=1"):
        rp.rephase_reference(mags[:1], phase, 2, mix, n_fft=512, hop=384)
    with pytest.raises(ValueError, match="stems"):
        rp.refine_phase(None, None, None, 41, 2, stems=3, mix=mix, n_fft=512, hop=384)
    for n_fft in (768, 4096):                                                # an n_fft that is not built
        with pytest.raises(ValueError, match="n_fft"):
            rp.refine_phase(None, None, None, 41, 2, stems=1, n_fft=n_fft, hop=256)
        with pytest.raises(ValueError, match="n_fft"):
            rp.rephase(torch.zeros((1, 2, 1000)), None, n_fft, 256)
    with pytest.raises(ValueError, match="n_fft"):
        rp.rephase_reference(np.zeros((1, 2, 385, 41)), np.ones((2, 385, 41)), 1, n_fft=768, hop=256)
    with pytest.raises(ValueError, match="hop"):
        rp.rephase(torch.zeros((1, 2, 1000)), None, 512, 513)


# ---- signatures and the command line -----------------------------------------------------------------------------------------

def test_phase_iters_defaults_to_zero():
    from svs_unet_pytorch_amd import streaming
    for fn in (streaming.separate_waveform, streaming.separate_to_wav):
        assert inspect.signature(fn).parameters["phase_iters"].default == 0, fn.__name__
    sig = inspect.signature(rp.refine_phase)
    for name in ("stems", "invert", "mix", "n_fft", "hop"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name


@pytest.mark.parametrize("value", ["-1", "-3"])
def test_cli_refuses_negative_phase_iters_before_the_checkpoint(value, tmp_path, capsys):
    from svs_unet_pytorch_amd import separate
    missing = str(tmp_path / "no_such_checkpoint.pth")             # loading it would fail with another message
    with pytest.raises(SystemExit) as e:
        separate.main(["--model_path", missing, "--src", str(tmp_path / "in.wav"), "--tar", str(tmp_path / "out"), "--phase_iters", value])
    assert e.value.code == 2                                       # argparse's usage error
    text = capsys.readouterr().err
    assert "usage:" in text and "--phase_iters" in text and "must be 0" in text
    assert not (tmp_path / "out").exists()


def test_cli_help_names_phase_iters(capsys):
    from svs_unet_pytorch_amd import separate
    with pytest.raises(SystemExit) as e:
        separate.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--phase_iters" in text and "Griffin-Lim" in text and "MISI" in text
