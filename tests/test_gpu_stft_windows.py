"""STFT / inverse STFT at n_fft = 512 and 2048 (-m gpu): data.py:24 `--win_size`, handed to librosa.stft / librosa.istft by the
reference.  Gates are the 1024 path's own (tests/test_gpu_ops.py): torch.stft / torch.istft in float32 err by 1.3e-7 .. 1.8e-7
(forward) and 3.0e-7 .. 1.1e-6 (inverse) against float64 at all three window sizes, so 2e-6 / 2e-5 / 1e-4 leave more than 10x
over a correct fp32 implementation whatever N is.  torch.istft refuses hop = N (NOLA), so no inverse case uses it."""
import os

import numpy as np
import pytest
import torch

from oracle import stft_oracle as so
from oracle import tiling_oracle as to
from oracle import unet_oracle as uo
from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd import data as svs_data

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = (512, 2048)


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr()


def torch_stft(y, n_fft, hop):
    return torch.stft(torch.from_numpy(y).double(), n_fft, hop, n_fft, torch.hann_window(n_fft, dtype=torch.float64), center=True,
                      pad_mode="constant", return_complex=True)


def c128(t):
    """complex64 device tensor -> complex128 on the host"""
    return torch.view_as_complex(torch.view_as_real(t).cpu().double())


@pytest.mark.parametrize("n_fft", SIZES)
def test_forward_vs_torch_and_oracle(n_fft, report):
    """n = 700 is shorter than one 2048 window, 40003 is no multiple of 4 (scalar loads), T is never a multiple of 16."""
    for hop in (3 * n_fft // 4, 100):
        for n in (700, 20000, 40003):
            y = synth.audio(n)
            T = 1 + n // hop
            assert T % 16 != 0
            mag, ph = svs_data.stft_magphase(torch.from_numpy(y).to(DEV), n_fft, hop)
            assert mag.shape == ph.shape == (n_fft // 2 + 1, T) and mag.dtype == torch.float32 and ph.dtype == torch.complex64
            d = torch_stft(y, n_fft, hop)
            assert d.shape == (n_fft // 2 + 1, T)
            scale = d.abs().max().item()
            name = f"stft N={n_fft} hop={hop} n={n}"
            e_mag = (mag.cpu().double() - d.abs()).abs().max().item() / scale
            e_cpx = (c128(ph) * mag.cpu().double() - d).abs().max().item() / scale
            m_o, p_o = so.magphase(so.stft(y, n_fft, hop))
            e_orc = np.abs(mag.cpu().numpy() - m_o).max() / scale
            e_orc_c = np.abs(ph.cpu().numpy().astype(np.complex128) * mag.cpu().numpy() - m_o.astype(np.float64) * p_o).max() / scale
            print(name, e_mag, e_cpx, e_orc, e_orc_c)
            assert report(f"{name} mag vs torch.stft", e_mag, 2e-6)
            assert report(f"{name} mag x phasor vs torch.stft", e_cpx, 2e-6)
            assert report(f"{name} mag vs oracle", e_orc, 2e-6)
            assert report(f"{name} mag x phasor vs oracle", e_orc_c, 2e-6)
            norm = ph.abs()
            assert torch.all((norm - 1).abs() <= 2e-6)


@pytest.mark.parametrize("n_fft", SIZES)
def test_forward_into_tiles(n_fft, report):
    """Two channels into 32-frame network tiles with the DC row dropped: T = 69 -> three tiles, 27 padded columns."""
    hop, seg, rows = 3 * n_fft // 4, 32, n_fft // 2
    n = hop * 68 + 5
    y_np = np.stack([synth.audio(n, 0), synth.audio(n, 1) * 0.5])
    tiles, phase, peak, T = svs_data.stft_to_tiles(torch.from_numpy(y_np).to(DEV), n_fft, hop, seg)
    assert T == 69 and tiles.shape == (2, 3, 1, rows, seg) and phase.shape == (2, T, rows + 1)
    tiles_h, phase_h = tiles.cpu().numpy(), phase.cpu().numpy()
    for c in range(2):
        mag_o, ph_o = so.magphase(so.stft(y_np[c], n_fft, hop))
        scale = mag_o.max()
        full = tiles_h[c, :, 0].transpose(1, 0, 2).reshape(rows, 3 * seg)
        assert report(f"stft_tiles N={n_fft} ch{c} magnitude", np.abs(full[:, :T] - mag_o[1:]).max() / scale, 2e-6)
        assert full[:, T:].shape == (rows, 27) and np.all(full[:, T:] == 0)         # tile padding (inference.py:90-92)
        assert report(f"stft_tiles N={n_fft} ch{c} peak", abs(peak[c].item() - scale) / scale, 2e-6)
        big = mag_o.T > 1e-3 * scale
        assert report(f"stft_tiles N={n_fft} ch{c} phasors", np.abs(phase_h[c] - ph_o.T)[big].max(), 2e-4)


def _inverse_cases():
    return [(n_fft, hop) for n_fft in SIZES for hop in (n_fft // 4, n_fft // 2, 5 * n_fft // 8, 3 * n_fft // 4, 100, 50)]


@pytest.mark.parametrize("n_fft,hop", _inverse_cases())
def test_inverse_vs_torch_istft(n_fft, hop, report):
    """Both kernels (hop >= N / 2: two frames per sample; below: the general overlap-add in one round or several -- hop 50 at
    N = 2048 has a 40-frame halo), both phase forms, then two channels from tiles with a mask, invert and peak."""
    win = torch.hann_window(n_fft, dtype=torch.float64)
    nbin, rows = n_fft // 2 + 1, n_fft // 2
    n = 40000 if hop >= 100 else 12000
    y = synth.audio(n)
    T = 1 + n // hop
    tol = 2e-5 if n_fft % hop == 0 else 1e-4
    # envelope troughs of hops above N / 4 amplify fp32 noise, and the envelope falls to zero at both ends: interior only there
    interior = slice(None) if hop <= n_fft // 4 else slice(n_fft, -n_fft)
    tag = f"N={n_fft} hop={hop}"
    # ---- phasor form from the file layout (data.py:159)
    mag, ph = svs_data.stft_magphase(torch.from_numpy(y).to(DEV), n_fft, hop)
    d = torch_stft(y, n_fft, hop)
    got = svs_data.istft(mag, ph, n_fft, hop).cpu().double()
    want = torch.istft(d, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=win, return_complex=False)
    assert got.shape == want.shape == (hop * (T - 1),)
    e = (got - want).abs()[interior].max().item() / want.abs().max().item()
    e_rt = (got[interior] - torch.from_numpy(y).double()[:hop * (T - 1)][interior]).abs().max().item()
    print(tag, "phasor", e, "round trip", e_rt)
    assert report(f"istft {tag} phasor form vs torch.istft", e, tol)
    assert report(f"stft->istft round trip {tag}", e_rt, 5 * tol)
    # ---- angle form: three (N / 2) x 40 tiles with the DC row dropped (train.py:33-60)
    B, Tt = 3, 40
    m = synth.uniform(3, B * rows * Tt).reshape(B, 1, rows, Tt)
    a = (synth.uniform(4, B * rows * Tt) * 2 * np.pi - np.pi).astype(np.float32).reshape(B, 1, rows, Tt)
    got = svs_data.specific_istft(torch.from_numpy(m).to(DEV), torch.from_numpy(a).to(DEV), n_fft, hop).cpu().double()
    m64 = torch.nn.functional.pad(torch.from_numpy(m).double(), (0, 0, 1, 0))
    a64 = torch.nn.functional.pad(torch.from_numpy(a).double(), (0, 0, 1, 0))
    want = torch.istft(torch.polar(m64, a64).squeeze(1), n_fft=n_fft, hop_length=hop, win_length=n_fft, window=win, return_complex=False)
    assert got.shape == (B, 1, hop * (Tt - 1))
    e = (got[:, 0] - want).abs()[:, interior].max().item() / want.abs().max().item()
    print(tag, "angle", e)
    assert report(f"specific_istft {tag} vs torch.istft", e, tol)
    # ---- two channels from tiles, uniform mask, invert, peak 0.9 (inference.py:100-107, data.py:162-164)
    y2 = np.stack([y, synth.audio(n, 1) * 0.5])
    tiles, phase, _, T2 = svs_data.stft_to_tiles(torch.from_numpy(y2).to(DEV), n_fft, hop, 128)
    assert T2 == T
    n_tiles = tiles.shape[1]
    mask = torch.from_numpy(synth.uniform(9, tiles.numel()).reshape(tiles.shape)).to(DEV)
    got_m = svs_data.istft_from_tiles(tiles, mask, phase, T, invert=True, n_fft=n_fft, hop=hop, peak=0.9).cpu().numpy()
    assert got_m.shape == (2, hop * (T - 1))
    tiles_h, mask_h = tiles.cpu().numpy(), mask.cpu().numpy()
    for c in range(2):
        _, ph_o = so.magphase(so.stft(y2[c], n_fft, hop))
        full = tiles_h[c, :, 0].transpose(1, 0, 2).reshape(rows, n_tiles * 128)[:, :T]
        mfull = 1.0 - mask_h[c, :, 0].transpose(1, 0, 2).reshape(rows, n_tiles * 128)[:, :T]
        want_m = so.istft(np.concatenate([np.zeros((1, T), np.float32), full * mfull], axis=0) * ph_o, n_fft, hop)
        e = np.abs(got_m[c] / 0.9 * np.abs(want_m).max() - want_m)[interior].max() / np.abs(want_m).max()
        print(tag, "masked ch", c, e)
        assert report(f"istft_tiles {tag} ch{c} masked + peak-normalised", e, 5e-5)
        assert report(f"istft_tiles {tag} ch{c} peak 0.9", abs(np.abs(got_m[c]).max() - 0.9), 1e-5)


def test_1024_through_the_n_names_is_bitwise_the_old_path():
    n, hop, seg = 768 * 70 + 3, 768, 128
    y = torch.from_numpy(np.stack([synth.audio(n, 0), synth.audio(n, 1) * 0.5])).to(DEV)
    T = 1 + n // hop
    groups = L().svs_stft_groups(seg)
    assert groups == L().svs_stft_groups_n(1024, seg)
    outs = []
    for fn in (L().svs_stft_tiles, L().svs_stft_tiles_n):
        tiles = torch.full((2, 1, 1, 512, seg), -1.0, device=DEV)
        ph = torch.full((2, T, 513, 2), -1.0, device=DEV)
        part = torch.full((2, groups), -1.0, device=DEV)
        _lib.check(fn(y.data_ptr(), n, 2, 1024, hop, tiles.data_ptr(), 512 * seg, seg, 512, 1, seg, ph.data_ptr(), 1, part.data_ptr(), S()))
        outs.append((tiles, ph, part))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    tiles, _, _ = outs[0]
    mask = torch.from_numpy(synth.uniform(9, tiles.numel()).reshape(tiles.shape)).to(DEV)
    for hop_i in (768, 256):                             # the two-frames-per-sample kernel and the general one
        ph = torch.view_as_real(torch.polar(torch.ones((2, T, 513), device=DEV), torch.rand((2, T, 513), device=DEV) * 6.0 - 3.0)).contiguous()
        g = L().svs_istft_groups(hop_i, T, 2)
        assert g == L().svs_istft_groups_n(1024, hop_i, T, 2)
        res = []
        for fn in (L().svs_istft_tiles, L().svs_istft_tiles_n):
            out = torch.full((2, hop_i * (T - 1)), -1.0, device=DEV)
            part = torch.full((2, g), -1.0, device=DEV)
            _lib.check(fn(tiles.data_ptr(), 512 * seg, seg, 512, 1, mask.data_ptr(), 1, ph.data_ptr(), 1, 2, 1024, hop_i, T, out.data_ptr(),
                          part.data_ptr(), S()))
            res.append((out, part))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert torch.all(res[0][1] >= 0) and res[0][0].abs().max().item() == res[0][1].max().item()


def test_rejections():
    n, T = 8192, 5                                       # buffers large enough for any accepted size: nothing here may launch
    y = torch.zeros((1, n), device=DEV)
    mag = torch.zeros((1025, 128), device=DEV)
    ph = torch.zeros((128, 1025, 2), device=DEV)
    out = torch.zeros(4 * n, device=DEV)
    for bad in (768, 256, 4096):
        with pytest.raises(RuntimeError, match="n_fft"):
            _lib.check(L().svs_stft_tiles_n(y.data_ptr(), n, 1, bad, 128, mag.data_ptr(), (bad // 2 + 1) * 128, 128, bad // 2 + 1, 0, 128, None, 0,
                                            None, S()))
        with pytest.raises(RuntimeError, match="n_fft"):
            _lib.check(L().svs_istft_tiles_n(mag.data_ptr(), (bad // 2 + 1) * T, T, bad // 2 + 1, 0, None, 0, ph.data_ptr(), 1, 1, bad, 128, T,
                                             out.data_ptr(), None, S()))
        with pytest.raises(ValueError, match="n_fft"):
            svs_data.stft_magphase(y[0], bad, 128)
    for n_fft in SIZES:
        nbin = n_fft // 2 + 1
        with pytest.raises(RuntimeError, match="hop"):
            _lib.check(L().svs_istft_tiles_n(mag.data_ptr(), nbin * T, T, nbin, 0, None, 0, ph.data_ptr(), 1, 1, n_fft, n_fft + 1, T, out.data_ptr(),
                                             None, S()))
        with pytest.raises(RuntimeError, match="frames"):
            _lib.check(L().svs_istft_tiles_n(mag.data_ptr(), nbin, 1, nbin, 0, None, 0, ph.data_ptr(), 1, 1, n_fft, n_fft // 2, 1, out.data_ptr(),
                                             None, S()))
        with pytest.raises(RuntimeError, match="layout"):                          # the 1024 path's rows at another window
            _lib.check(L().svs_stft_tiles_n(y.data_ptr(), n, 1, n_fft, 128, mag.data_ptr(), 513 * 128, 128, 513, 0, 128, None, 0, None, S()))


def _end_to_end(n_fft, hop, n, report):
    from svs_unet_pytorch_amd.model import UNet
    from svs_unet_pytorch_amd.streaming import separate_waveform
    state = synth.closed_form_state()
    model = UNet()
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.to(DEV).eval()
    y = np.stack([synth.audio(n, 10), synth.audio(n, 11)])
    got = separate_waveform(model, torch.from_numpy(y).to(DEV), n_fft=n_fft, hop=hop).cpu().numpy()
    T = 1 + n // hop
    assert got.shape == (2, hop * (T - 1))
    st = uo.to_torch_state(state)
    for ch in range(2):
        spec, phase = so.to_spec(y[ch], y[ch], n_fft, hop)
        assert spec.shape == (n_fft // 2 + 1, T)
        with torch.no_grad():
            pred = to.separate(spec, lambda t: uo.forward(st, torch.from_numpy(t)).numpy())
        want = so.to_wave(pred, phase, n_fft, hop)
        e = np.abs(got[ch] - want)[n_fft:-n_fft].max()
        print(f"end to end N={n_fft} ch{ch}", e, np.abs(got[ch]).max())
        assert abs(np.abs(got[ch]).max() - 0.9) <= 1e-5
        assert report(f"streaming separation N={n_fft} channel {ch} (interior)", e, 1e-4)


def test_end_to_end_512(report):
    """separate_waveform at n_fft = 512, hop 384: T = 141, two 256 x 128 tiles per channel, against the three oracles."""
    _end_to_end(512, 384, 384 * 140, report)


def test_end_to_end_2048(report):
    """The same at n_fft = 2048, hop 1536: T = 131, two 1024 x 128 tiles per channel -- the first run of the network at
    H = 1024 on the device, in a test of its own: a failure here with the transform tests green lies in the network."""
    _end_to_end(2048, 1536, 1536 * 130, report)


def test_command_line_at_512(tmp_path, report, monkeypatch):
    """data.main to_spec / to_wave with --win_size 512 --hop_size 128 on two short songs (data.py:20-28,46-169)."""
    from scipy.io import wavfile
    monkeypatch.chdir(tmp_path)
    sr, songs = 8192, {}
    for i, (name, n) in enumerate((("songA", 9000), ("songB", 7001))):
        os.makedirs(tmp_path / "wav" / name)
        voc = (synth.audio(n - 500, 2 * i) * 0.3).astype(np.float32)
        mix = (synth.audio(n, 2 * i + 1) * 0.5).astype(np.float32)
        mix[: voc.size] += voc
        wavfile.write(tmp_path / "wav" / name / "mixture.wav", sr, mix)
        wavfile.write(tmp_path / "wav" / name / "vocals.wav", sr, voc)
        songs[name] = (mix, voc)
    spec_dir, wav_dir = tmp_path / "spec", tmp_path / "out"
    geometry = ["--win_size", "512", "--hop_size", "128"]
    svs_data.main(["--src", str(tmp_path / "wav"), "--tar", str(spec_dir), "--direction", "to_spec"] + geometry)
    for i, (name, (mix, voc)) in enumerate(songs.items()):
        T = 1 + mix.size // 128
        for track, y in (("mixture", mix), ("vocal", voc)):
            spec = np.load(spec_dir / track / f"{i:04d}_{name}_spec.npy")
            phase = np.load(spec_dir / track / f"{i:04d}_{name}_phase.npy")
            want_s, want_p = so.to_spec(mix, y, 512, 128)
            assert spec.dtype == np.float32 and phase.dtype == np.complex64 and spec.shape == phase.shape == want_s.shape == (257, T)
            assert report(f"cli to_spec 512/128 {name}/{track} magnitude", np.abs(spec - want_s).max(), 2e-6)
            assert report(f"cli to_spec 512/128 {name}/{track} mag x phasor",
                          np.abs(spec * phase.astype(np.complex128) - want_s * want_p.astype(np.complex128)).max(), 2e-6)
    svs_data.main(["--src", str(spec_dir / "mixture"), "--phase", str(spec_dir / "mixture"), "--tar", str(wav_dir), "--direction", "to_wave"] + geometry)
    for i, (name, (mix, _)) in enumerate(songs.items()):
        rate, wav = wavfile.read(wav_dir / f"{i:04d}_{name}.wav")
        T = 1 + mix.size // 128
        assert rate == sr and wav.dtype == np.float32 and wav.shape == (128 * (T - 1),)
        assert abs(np.abs(wav).max() - 0.9) <= 1e-5
        want = so.to_wave(np.load(spec_dir / "mixture" / f"{i:04d}_{name}_spec.npy"), np.load(spec_dir / "mixture" / f"{i:04d}_{name}_phase.npy"), 512, 128)
        # hop divides the window and four frames cover every sample: the whole signal, at the peak-normalised inverse's gate
        assert report(f"cli to_wave 512/128 {name}", np.abs(wav - want).max() / 0.9, 5e-5)
