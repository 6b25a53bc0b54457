"""The way out of the pipeline on the GPU (csrc/resample.hip: svs_resample_peaks / svs_resample_encode) and its callers
(resample.resample_encode_gpu, data.save_wav_device, data.py to_wave --sr_out / --subtype, streaming.separate_waveform(sr_out=),
streaming.separate_to_wav, the separate CLI).

The kernel tests are bitwise: the encode kernel's value before the gain is, by construction, the float svs_resample_poly writes
(same table, same plan, same k = 0 .. T-1 fmaf chain), and everything after it is restated in numpy by
resample.encode_pcm_reference, so torch.equal is the bound.  Shapes: n_in = 1, 7 (fewer inputs than taps), 300 and 4099 (several
steps of the up <= 256 plans); 375/64 runs two blocks along i % up, 11025/2048 forty-four, the last with 17 rows.
"""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd import data as svs_data
from svs_unet_pytorch_amd import resample as rs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RATIOS = [(1, 1), (2, 1), (3, 2), (375, 64), (11025, 2048)]
N_IN = [1, 7, 300, 4099]
FMTS = [("int16", rs.PCM_I16, torch.int16), ("int32", rs.PCM_I32, torch.int32), ("float32", rs.PCM_F32, torch.float32)]
GAIN = np.array([3.0, 5.5, 4.25], dtype=np.float32)          # on 0.3 * N(0, 1) input: samples past full scale on both sides


def signal(channels, n, seed=0):
    return (0.3 * np.random.default_rng(1000 * channels + n + seed).standard_normal((channels, n))).astype(np.float32)


def encode(x, up, down, gain, code, dtype):
    """svs_resample_encode itself: x (channels, n) float32 on the device -> (n_out, channels) of dtype."""
    L = _lib.lib()
    channels, n = x.shape
    table, ntaps = rs.tap_table(up, down, DEV)
    out = torch.empty((rs.out_len(n, up, down), channels), dtype=dtype, device=DEV)
    _lib.check(L.svs_resample_encode(x.data_ptr(), channels, n, n, table.data_ptr(), ntaps, up, down, _lib.ptr(gain), code, out.data_ptr(),
                                     _lib.stream_ptr()), "svs_resample_encode")
    return out


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("up,down", RATIOS, ids=lambda v: str(v))
def test_encode_is_bitwise_the_reference_of_the_resampled_signal(up, down, channels):
    gain = torch.from_numpy(GAIN[:channels]).to(DEV)
    for n in N_IN:
        x = torch.from_numpy(signal(channels, n)).to(DEV)
        y = rs.resample_poly_gpu(x, up, down).cpu().numpy().T                            # (n_out, channels), computed once per shape
        assert y.shape == (rs.out_len(n, up, down), channels)
        for name, code, dtype in FMTS:
            for g_dev, g_np in ((None, None), (gain, GAIN[:channels])):
                got = encode(x, up, down, g_dev, code, dtype)
                want = torch.from_numpy(rs.encode_pcm_reference(y, g_np, name))
                assert got.dtype == want.dtype and torch.equal(got.cpu(), want), (n, name, g_np is not None)
        if n == 4099:                                                                     # the gain does push samples past both ends
            clipped = rs.encode_pcm_reference(y, GAIN[:channels], "int16")
            assert (clipped == 32767).any() and (clipped == -32768).any() and (np.abs(y * GAIN[:channels]) < 1).any()


def test_encode_rounds_ties_to_even():
    j = np.arange(-3000, 3000)
    x = ((2 * j + 1) / 65534).astype(np.float32)                                          # x * 32767 = j + 0.5 exactly, all 6,000
    xd = torch.from_numpy(x[None]).to(DEV)
    got = encode(xd, 1, 1, None, rs.PCM_I16, torch.int16).cpu().numpy()[:, 0]
    assert np.array_equal(got, np.where(j % 2 == 0, j, j + 1))
    y = rs.resample_poly_gpu(xd, 1, 1).cpu().numpy().T
    assert np.array_equal(y[:, 0], x) and np.array_equal(got, rs.encode_pcm_reference(y, None, "int16")[:, 0])


def test_encode_non_finite_samples():
    x = torch.tensor([[float("nan"), float("inf"), -float("inf"), 1.0, -1.0, 2.0, -2.0, 0.25]], device=DEV)
    y = x.cpu().numpy().T
    for name, code, dtype in FMTS:
        got = encode(x, 1, 1, None, code, dtype).cpu().numpy()
        want = rs.encode_pcm_reference(y, None, name)
        assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=(name == "float32")), name
    assert encode(x, 1, 1, None, rs.PCM_I16, torch.int16).cpu().numpy()[:3, 0].tolist() == [0, 32767, -32768]


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("up,down", RATIOS, ids=lambda v: str(v))
def test_peaks_equal_the_maximum_of_the_resampled_signal(up, down, channels):
    for n in N_IN:
        x = torch.from_numpy(signal(channels, n, seed=5)).to(DEV)
        want = rs.resample_poly_gpu(x, up, down).abs().amax(-1)
        got = rs.resample_peaks_gpu(x, up, down)
        assert got.shape == (channels,) and torch.equal(got, want), (n, got, want)


def test_resample_encode_gpu_normalises_to_the_peak():
    x = signal(3, 4099, seed=9) * np.array([[1.0], [0.5], [0.1]], dtype=np.float32)
    xd = torch.from_numpy(x).to(DEV)
    for up, down in ((11025, 2048), (1, 1)):
        pcm = rs.resample_encode_gpu(xd, up, down, fmt="int16", peak=0.9)
        assert pcm.dtype == torch.int16 and pcm.shape == (rs.out_len(4099, up, down), 3)
        top = pcm.to(torch.int32).abs().amax(0).tolist()
        loudest = int(rs.resample_poly_gpu(xd, up, down).abs().amax(-1).argmax())
        assert top[loudest] == 29490 == max(top) and min(top) < 29490 // 2                # one gain: the balance is kept
        each = rs.resample_encode_gpu(xd, up, down, fmt="int16", peak=0.9, common_gain=False)
        assert each.to(torch.int32).abs().amax(0).tolist() == [29490, 29490, 29490]
        raw = rs.resample_encode_gpu(xd, up, down, fmt="float32", peak=None)
        assert torch.equal(raw, rs.resample_poly_gpu(xd, up, down).T)
    mono = rs.resample_encode_gpu(xd[0], 375, 64, fmt="int32", peak=0.9)                  # (n,) in, (n_out,) out
    assert mono.dtype == torch.int32 and mono.shape == (rs.out_len(4099, 375, 64),)
    # float32(p * (float32(0.9) / p)) is within 1.5 ulp (2^-24 each) of 0.9
    assert abs(int(mono.to(torch.int64).abs().max()) - 0.9 * 2147483647) <= 2.0 ** -23 * 2147483647
    zeros = rs.resample_encode_gpu(torch.zeros((2, 300), device=DEV), 11025, 2048, fmt="int16", peak=0.9)
    assert zeros.shape == (rs.out_len(300, 11025, 2048), 2) and not zeros.any()
    with pytest.raises(TypeError):
        rs.resample_encode_gpu(xd.double(), 2, 1)


def test_save_wav_device(tmp_path):
    y = torch.from_numpy(signal(2, 3000, seed=3)).to(DEV)
    path = str(tmp_path / "a.wav")
    svs_data.save_wav_device(path, y, 8192, 44100, "PCM_16")
    rate, pcm = wavfile.read(path)
    assert rate == 44100 and pcm.dtype == np.int16 and pcm.shape == (-(-3000 * 11025 // 2048), 2)
    assert int(np.abs(pcm.astype(np.int32)).max()) == 29490
    svs_data.save_wav_device(path, y[0], 8192, subtype="FLOAT", peak=None)                # same rate, nothing but the copy
    rate, f = wavfile.read(path)
    assert rate == 8192 and f.dtype == np.float32 and np.array_equal(f, y[0].cpu().numpy())


def _model():
    from svs_unet_pytorch_amd.model import UNet
    m = UNet()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state().items()})
    return m.to(DEV).eval()


def test_separate_waveform_at_the_file_rate():
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = _model()
    n = 8192 * 2 + 100
    y = torch.from_numpy(np.stack([synth.audio(n, 30), 0.5 * synth.audio(n, 31)]).astype(np.float32)).to(DEV)
    base = separate_waveform(model, y)
    assert torch.equal(separate_waveform(model, y, sr_out=None), base)
    got = separate_waveform(model, y, sr_out=44100)
    n8 = 768 * (n // 768)
    assert base.shape == (2, n8) and got.shape == (2, rs.out_len(n8, 44100, 8192)) and got.dtype == torch.float32
    r = rs.resample_poly_gpu(separate_waveform(model, y, peak=None), 44100, 8192).cpu().numpy().astype(np.float64)
    want = r / np.abs(r).max(axis=1, keepdims=True) * float(np.float32(0.9))
    # x / d * numer in fp32: two roundings of 2^-24 relative each, on values of at most the peak
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print(f"separate_waveform(sr_out=44100) vs float64 normalisation: max err {err:.3e}")
    assert err <= 2.0 * 2.0 ** -24 * 0.9 * (1 + 2.0 ** -20)
    assert np.abs(np.abs(got.cpu().numpy()).max(axis=1) - 0.9).max() <= 2.0 ** -23
    mono = separate_waveform(model, y[0], sr_out=44100)
    assert mono.shape == (got.shape[1],)                                                  # (n,) in, (n',) out


def test_separate_cli_writes_a_file_evaluate_accepts(tmp_path):
    from svs_unet_pytorch_amd import evaluate, separate
    ck = str(tmp_path / "svs_synth.pth")
    torch.save({"model_state_dict": {k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state().items()}}, ck)
    n = 40000
    mix = np.stack([synth.audio(n, 40), 0.7 * synth.audio(n, 41)], axis=1)
    src = str(tmp_path / "mixture.wav")
    wavfile.write(src, 44100, np.clip(np.round(mix * 20000), -32768, 32767).astype(np.int16))
    dst = str(tmp_path / "vocals_est.wav")
    separate.main(["--model_path", ck, "--src", src, "--tar", dst])
    rate, pcm = wavfile.read(dst)
    assert rate == 44100 and pcm.dtype == np.int16 and pcm.shape == (n, 2)
    assert int(np.abs(pcm.astype(np.int32)).max()) == 29490
    assert not pcm[37210:].any() and pcm[:37210].any()                                    # 7431 -> 6912 samples -> 37,210 frames, then zeros
    est, sr = evaluate.load_mono_audio(dst)
    ref, sr_ref = evaluate.load_mono_audio(src)
    assert sr == sr_ref == 44100 and est.shape == ref.shape
    out_dir = tmp_path / "out"                                                            # a folder: every *.wav under its own name
    separate.main(["--model_path", ck, "--src", str(tmp_path), "--tar", str(out_dir), "--subtype", "FLOAT", "--no_keep_length"])
    assert sorted(os.listdir(out_dir)) == ["mixture.wav", "vocals_est.wav"]
    rate, f = wavfile.read(str(out_dir / "mixture.wav"))
    assert rate == 44100 and f.dtype == np.float32 and f.shape == (37210, 2) and abs(float(np.abs(f).max()) - 0.9) <= 2.0 ** -23


def test_to_wave_flags(tmp_path):
    y = torch.from_numpy(synth.audio(768 * 20, 50).astype(np.float32)).to(DEV)
    mag, phase = svs_data.stft_magphase(y)
    spec_dir, phase_dir = tmp_path / "pred", tmp_path / "phase"
    os.makedirs(spec_dir), os.makedirs(phase_dir)
    np.save(spec_dir / "0000_a_spec.npy", mag.cpu().numpy())
    np.save(phase_dir / "0000_a_phase.npy", phase.cpu().numpy())
    common = ["--src", str(spec_dir), "--phase", str(phase_dir), "--direction", "to_wave"]
    svs_data.main(common + ["--tar", str(tmp_path / "w16"), "--sr_out", "44100", "--subtype", "PCM_16"])
    rate, pcm = wavfile.read(str(tmp_path / "w16" / "0000_a.wav"))
    assert rate == 44100 and pcm.dtype == np.int16 and pcm.shape == (rs.out_len(768 * 20, 44100, 8192),)
    assert int(np.abs(pcm.astype(np.int32)).max()) == 29490
    svs_data.main(common + ["--tar", str(tmp_path / "w32"), "--subtype", "PCM_32"])       # the rate stays: a pure encode
    rate, pcm = wavfile.read(str(tmp_path / "w32" / "0000_a.wav"))
    assert rate == 8192 and pcm.dtype == np.int32 and pcm.shape == (768 * 20,)
    svs_data.main(common + ["--tar", str(tmp_path / "wdef")])                             # neither flag: today's file, byte for byte
    want = svs_data.istft(mag, phase, peak=0.9)
    svs_data.write_wav(str(tmp_path / "want.wav"), want.cpu().numpy(), 8192)
    assert open(tmp_path / "wdef" / "0000_a.wav", "rb").read() == open(tmp_path / "want.wav", "rb").read()
