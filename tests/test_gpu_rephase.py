"""Phase refinement (-m gpu): the re-phasing forward transform svs_stft_rephase_n against the float64 transform of the float64
source, the device loop rephase.refine_phase against the float64 definition rephase.rephase_reference (final waveforms and the
inconsistency the iterations lower), and phase_iters through separate_waveform / separate_to_wav.

Kernel gates: 2e-6 on |S_ref| * |p_gpu - p_ref| / max |S_ref| and on | |p| - 1 |, what tests/test_gpu_stft_windows.py holds the same
transform's mag x phasor and phasor norms to.  Loop gates: LOOP_GATE / MEASURE_GATE below, 4x the maxima measured on an MI355X over
iters 1..4 and the three modes (DESIGN.md section 14 has the figures per iteration)."""
import functools
import os

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd import data as svs_data
from svs_unet_pytorch_amd import overlap as ov
from svs_unet_pytorch_amd import rephase as rp
from svs_unet_pytorch_amd.config import INPUT_LEN, SAMPLE_RATE

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -777.0
GUARD = 64                # floats before and after the phase buffer
GAP = 32                  # floats between the stems, beyond one stem's phasors
ITERS = 4


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr()


def c128(t):
    """complex64 device tensor -> complex128 numpy array"""
    return torch.view_as_complex(torch.view_as_real(t).cpu().double()).numpy()


# ---- the kernel --------------------------------------------------------------------------------------------------------------

def signals(stems, n, zero_channel=False):
    """(x (stems, 2, n), mix (2, n) or None) float32: mix is an arbitrary third signal, so the residual mix - x_0 - x_1 is as large
    as the stems."""
    x = np.stack([np.stack([synth.audio(n, 60 + 2 * s), 0.5 * synth.audio(n, 61 + 2 * s)]) for s in range(stems)]).astype(np.float32)
    mix = np.stack([synth.audio(n, 70), 0.7 * synth.audio(n, 71)]).astype(np.float32) if stems == 2 else None
    if zero_channel:
        x[:, 1] = 0
        if mix is not None:
            mix[1] = 0
    return x, mix


def run_rephase(x, mix, n_fft, hop):
    """svs_stft_rephase_n into a guarded buffer whose stems lie GAP floats apart -> (phasors (stems, 2, T, nbin) complex128, the raw
    buffer, the float offsets of the stems)."""
    stems, C, n = x.shape
    T, nbin = 1 + n // hop, n_fft // 2 + 1
    one = C * T * nbin * 2
    stride = one + GAP
    buf = torch.full((GUARD + (stems - 1) * stride + one + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    xd = torch.from_numpy(x).to(DEV)
    md = None if mix is None else torch.from_numpy(mix).to(DEV)
    _lib.check(L().svs_stft_rephase_n(xd.data_ptr(), C * n, stems, _lib.ptr(md), n, C, n_fft, hop, buf.data_ptr() + 4 * GUARD, stride, S()),
               "svs_stft_rephase_n")
    host = buf.cpu().numpy()
    offs = [GUARD + s * stride for s in range(stems)]
    ph = np.stack([host[o:o + one].astype(np.float64).reshape(C, T, nbin, 2) for o in offs])
    return ph[..., 0] + 1j * ph[..., 1], host, offs, one


@pytest.mark.parametrize("stems", [1, 2])
@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_rephase_kernel_vs_float64(n_fft, stems, report):
    """n = 700 is shorter than one 2048 window, 40003 is no multiple of 4 (so it takes the scalar loads, the other two lengths the
    16-byte ones), T is never a multiple of 16.  Two channels; one stem without a mixture, two stems with one."""
    for hop in (3 * n_fft // 4, n_fft // 4, 100):
        for n in (700, 20000, 40003):
            T = 1 + n // hop
            assert T % 16 != 0
            x, mix = signals(stems, n)
            got, host, offs, one = run_rephase(x, mix, n_fft, hop)
            z = x.astype(np.float64)
            if mix is not None:
                z = z + 0.5 * (mix.astype(np.float64) - z[0] - z[1])[None]
            ref = np.moveaxis(rp.reference_stft(z, n_fft, hop), -1, -2)                     # (stems, 2, T, nbin)
            assert got.shape == ref.shape == (stems, 2, T, n_fft // 2 + 1)
            e = (np.abs(ref) * np.abs(got - rp.reference_phasor(ref))).max() / np.abs(ref).max()
            e_norm = np.abs(np.abs(got) - 1).max()
            name = f"rephase N={n_fft} hop={hop} n={n} stems={stems}"
            print(name, e, e_norm)
            assert report(f"{name} |S| x |p - p_ref|", e, 2e-6)
            assert report(f"{name} | |p| - 1 |", e_norm, 2e-6)
            # nothing outside the phasors is written: before, after, and between the stems
            assert np.all(host[:GUARD] == SENTINEL) and np.all(host[offs[-1] + one:] == SENTINEL)
            if stems == 2:
                assert np.all(host[offs[0] + one:offs[1]] == SENTINEL)


@pytest.mark.parametrize("stems", [1, 2])
@pytest.mark.parametrize("n_fft,hop,n", [(512, 384, 20000), (1024, 256, 40003), (2048, 1536, 20000)])
def test_rephase_zero_channel_is_exactly_one(n_fft, hop, n, stems):
    """A channel of exact zeros (in both stems and the mixture) comes back as exactly 1 + 0i everywhere (librosa.magphase)."""
    x, mix = signals(stems, n, zero_channel=True)
    got, _, _, _ = run_rephase(x, mix, n_fft, hop)
    assert np.all(got[:, 1] == 1.0 + 0.0j)
    assert not np.all(got[:, 0] == 1.0 + 0.0j)


def test_rephase_binding_and_rejections():
    x, mix = signals(2, 20000)
    xd, md = torch.from_numpy(x).to(DEV), torch.from_numpy(mix).to(DEV)
    ph = rp.rephase(xd, md, 1024, 768)
    assert ph.shape == (2, 2, 27, 513) and ph.dtype == torch.complex64
    want, _, _, _ = run_rephase(x, mix, 1024, 768)
    assert np.array_equal(c128(ph), want)
    alone = rp.rephase(xd, None, 1024, 768)                      # two independent signals: stem 0 is what one stem gives
    assert torch.equal(alone[:1], rp.rephase(xd[:1].contiguous(), None, 1024, 768))
    with pytest.raises(ValueError, match="mix"):
        rp.rephase(xd[:1].contiguous(), md, 1024, 768)
    with pytest.raises(_lib.SvsError, match="a mixture needs stems == 2"):
        _lib.check(L().svs_stft_rephase_n(xd.data_ptr(), 0, 1, md.data_ptr(), 20000, 2, 1024, 768, ph.data_ptr(), 0, S()))
    with pytest.raises(_lib.SvsError, match="n_fft"):
        _lib.check(L().svs_stft_rephase_n(xd.data_ptr(), 0, 1, None, 20000, 2, 768, 256, ph.data_ptr(), 0, S()))


# ---- the loop ----------------------------------------------------------------------------------------------------------------

LOOP_GEOMETRIES = [(512, 384), (1024, 768), (2048, 1536), (1024, 256)]
MODES = ("plain", "inverted", "misi")
# 4x the maxima measured on an MI355X over the three modes and iters 1..4: the final waveforms against
# float64 relative to their peak, and the inconsistency against the reference's, relative
LOOP_GATE = {(512, 384): 3.8e-6, (1024, 768): 3.1e-6, (2048, 1536): 6.8e-6, (1024, 256): 2.0e-6}        # measured: 9.5e-7, 7.7e-7, 1.7e-6, 4.9e-7
MEASURE_GATE = {(512, 384): 4.6e-7, (1024, 768): 4.5e-7, (2048, 1536): 3.7e-7, (1024, 256): 2.8e-8}     # measured: 1.14e-7, 1.11e-7, 9.2e-8, 7.0e-9


def untile(t, T):
    """(C, n_tiles, 1, rows, seg) device tiles -> float64 (C, rows, T)"""
    a = t[:, :, 0].cpu().numpy().astype(np.float64)
    C, n_tiles, rows, seg = a.shape
    return a.transpose(0, 2, 1, 3).reshape(C, rows, n_tiles * seg)[:, :, :T]


@functools.lru_cache(maxsize=None)
def loop_case(n_fft, hop, mode):
    """Synthetic tiles (seg = 32, T = 41: the last tile is padded, rows = n_fft / 2), a uniform random mask, the phasors of the GPU's
    own forward transform, two channels; no network.  Returns the GPU's final waveforms and the reference's (float64, per iters
    0..4), the inconsistency of both per iters, and the interior slice the waveforms are compared on."""
    seg, n = 32, hop * 40 + 5
    y = torch.from_numpy(np.stack([synth.audio(n, 80), 0.5 * synth.audio(n, 81)])).to(DEV)
    tiles, phase, _, T = svs_data.stft_to_tiles(y, n_fft, hop, seg)
    assert T == 41 and tiles.shape == (2, 2, 1, n_fft // 2, seg)
    mask = torch.from_numpy(synth.uniform(82, tiles.numel()).reshape(tiles.shape)).to(DEV)
    stems = 2 if mode == "misi" else 1
    inverts = [False, True] if stems == 2 else [mode == "inverted"]
    mix = y[:, :hop * 40].contiguous() if stems == 2 else None
    mag, m = untile(tiles, T), untile(mask, T)
    dc = np.zeros((2, 1, T))
    mags = np.stack([np.concatenate([dc, mag * (1.0 - m if inv else m)], axis=1) for inv in inverts])
    phase0 = np.moveaxis(c128(phase), -1, -2)                                     # (C, nbin, T)
    mix64 = None if mix is None else mix.cpu().numpy().astype(np.float64)

    def analysed(w):
        return w if mix64 is None else w + 0.5 * (mix64 - w[0] - w[1])[None]

    got, want, m_got, m_want = [], [], [], []
    for iters in range(ITERS + 1):
        ph = rp.refine_phase(tiles, mask, phase, T, iters, stems=stems, invert=inverts[0], mix=mix, n_fft=n_fft, hop=hop)
        assert ph.shape == (stems, 2, T, n_fft // 2 + 1)
        w = np.stack([svs_data.istft_from_tiles(tiles, mask, ph[s], T, invert=inverts[s], n_fft=n_fft, hop=hop).cpu().numpy().astype(np.float64)
                      for s in range(stems)])
        _, w_ref, measure = rp.rephase_reference(mags, phase0, iters, mix64, n_fft=n_fft, hop=hop)
        got.append(w)
        want.append(w_ref)
        m_got.append(rp.inconsistency(analysed(w), mags, n_fft, hop).sum())
        m_want.append(measure[-1])
    # envelope troughs of hops above N / 4 amplify fp32 noise, and the envelope falls to zero at both ends: interior only there
    interior = slice(None) if hop <= n_fft // 4 else slice(n_fft, -n_fft)
    return got, want, np.array(m_got), np.array(m_want), interior


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_fft,hop", LOOP_GEOMETRIES)
def test_loop_vs_float64_definition(n_fft, hop, mode, report):
    got, want, _, _, interior = loop_case(n_fft, hop, mode)
    for iters in range(1, ITERS + 1):
        assert got[iters].shape == want[iters].shape == (2 if mode == "misi" else 1, 2, hop * 40)
        e = np.abs(got[iters] - want[iters])[..., interior].max() / np.abs(want[iters]).max()
        name = f"refine_phase N={n_fft} hop={hop} {mode} iters={iters} final waveform vs float64"
        print(name, e)
        assert report(name, e, LOOP_GATE[(n_fft, hop)])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_fft,hop", LOOP_GEOMETRIES)
def test_loop_lowers_the_inconsistency_on_the_device(n_fft, hop, mode, report):
    """|| |STFT(x)| - M ||^2 / || M ||^2 (two stems: summed, on x_k + (mix - x_0 - x_1) / 2), computed on the host in float64 from
    the GPU's waveforms: the reference's value at each of iters 0..4, and lower after four updates than before."""
    _, _, m_got, m_want, _ = loop_case(n_fft, hop, mode)
    for iters in range(ITERS + 1):
        e = abs(m_got[iters] - m_want[iters]) / m_want[iters]
        name = f"refine_phase N={n_fft} hop={hop} {mode} iters={iters} inconsistency {m_got[iters]:.6f} vs {m_want[iters]:.6f}"
        print(name, e)
        assert report(f"refine_phase N={n_fft} hop={hop} {mode} iters={iters} inconsistency vs float64", e, MEASURE_GATE[(n_fft, hop)])
    assert m_got[ITERS] < m_got[0]
    assert np.all(np.diff(m_want) < 0)


def test_zero_iterations_launch_nothing():
    seg, hop, n_fft = 32, 384, 512
    y = torch.from_numpy(np.stack([synth.audio(hop * 40 + 5, 80), 0.5 * synth.audio(hop * 40 + 5, 81)])).to(DEV)
    tiles, phase, _, T = svs_data.stft_to_tiles(y, n_fft, hop, seg)
    for stems, mix in ((1, None), (2, y[:, :hop * 40].contiguous())):
        ph = rp.refine_phase(tiles, None, phase, T, 0, stems=stems, mix=mix, n_fft=n_fft, hop=hop)
        assert ph.shape == (stems, 2, T, 257) and ph.data_ptr() == phase.data_ptr()      # the input, broadcast
        assert all(torch.equal(ph[s], phase) for s in range(stems))


# ---- the public path ---------------------------------------------------------------------------------------------------------

N_FFT, HOP = 512, 128


@functools.lru_cache(maxsize=None)
def random_model():
    from svs_unet_pytorch_amd.model import UNet
    torch.manual_seed(4321)
    return UNet().to(DEV).eval()


@functools.lru_cache(maxsize=None)
def stereo():
    """2 channels of hop * 130 + 5 samples: 131 frames, two 256 x 128 tiles per channel."""
    n = HOP * 130 + 5
    return torch.from_numpy(np.stack([synth.audio(n, 90), 0.5 * synth.audio(n, 91)])).to(DEV)


def by_hand(tile_hop, phase_iters):
    """separate_waveform(both_stems=True, peak=None, phase_iters=...) through the public pieces -> (2, C, hop * 130)."""
    model, y = random_model(), stereo()
    tiles, phase, norm, T = svs_data.stft_to_tiles(y, N_FFT, HOP, INPUT_LEN)
    assert T == 131 and tiles.shape == (2, 2, 1, N_FFT // 2, INPUT_LEN)
    for c in range(2):
        _lib.check(L().svs_scale_by_inv(tiles[c].data_ptr(), tiles[c].numel(), norm[c:].data_ptr(), 1.0, S()), "svs_scale_by_inv")
    flat = tiles.view(4, 1, N_FFT // 2, INPUT_LEN) if tile_hop == INPUT_LEN else ov.overlap_tiles(tiles, tile_hop)
    mask = torch.empty_like(flat)
    with torch.no_grad():
        mask[:] = model(flat)
    mask = mask.view(tiles.shape) if tile_hop == INPUT_LEN else ov.blend_masks(mask, 2, tile_hop)
    mix = y[:, :HOP * 130].clone(memory_format=torch.contiguous_format)
    for c in range(2):
        _lib.check(L().svs_scale_by_inv(mix[c].data_ptr(), mix.shape[1], norm[c:].data_ptr(), 1.0, S()), "svs_scale_by_inv")
    ph = rp.refine_phase(tiles, mask, phase, T, phase_iters, stems=2, mix=mix, n_fft=N_FFT, hop=HOP)
    return torch.stack([svs_data.istft_from_tiles(tiles, mask, ph[s], T, invert=bool(s), n_fft=N_FFT, hop=HOP) for s in range(2)])


def test_phase_iters_zero_is_the_default_path():
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    for kw in ({}, {"vocal_solo": False}, {"both_stems": True}, {"both_stems": True, "tile_hop": 64}, {"sr_out": 44100}):
        a = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, **kw)
        assert torch.equal(separate_waveform(model, y, n_fft=N_FFT, hop=HOP, phase_iters=0, **kw), a), kw


@pytest.mark.parametrize("tile_hop", [INPUT_LEN, 64])
def test_both_stems_is_its_composition(tile_hop):
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    want = by_hand(tile_hop, 2)
    got = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=None, both_stems=True, tile_hop=tile_hop, phase_iters=2)
    assert got.shape == (2, 2, HOP * 130) and torch.equal(got, want)
    plain = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=None, both_stems=True, tile_hop=tile_hop)
    assert not torch.equal(got, plain)                           # the option does something
    assert model.eval_precision == "fp32" and not model.training


def test_single_stem_is_griffin_lim_on_that_stem():
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    tiles, phase, norm, T = svs_data.stft_to_tiles(y, N_FFT, HOP, INPUT_LEN)
    for c in range(2):
        _lib.check(L().svs_scale_by_inv(tiles[c].data_ptr(), tiles[c].numel(), norm[c:].data_ptr(), 1.0, S()), "svs_scale_by_inv")
    mask = torch.empty_like(tiles)
    with torch.no_grad():
        mask.view(4, 1, N_FFT // 2, INPUT_LEN)[:] = model(tiles.view(4, 1, N_FFT // 2, INPUT_LEN))
    for solo in (True, False):
        ph = rp.refine_phase(tiles, mask, phase, T, 2, stems=1, invert=not solo, n_fft=N_FFT, hop=HOP)
        want = svs_data.istft_from_tiles(tiles, mask, ph[0], T, invert=not solo, n_fft=N_FFT, hop=HOP, peak=0.9)
        got = separate_waveform(model, y, vocal_solo=solo, n_fft=N_FFT, hop=HOP, phase_iters=2)
        assert torch.equal(got, want)
        assert abs(got.abs().max().item() - 0.9) <= 1e-5


def test_both_stems_at_the_output_rate():
    """sr_out = 44100: the refined stems are resampled, and `peak` is applied per stem and channel at THAT rate, as it is today."""
    from svs_unet_pytorch_amd.resample import resample_poly_gpu
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    want = resample_poly_gpu(by_hand(INPUT_LEN, 2).view(4, HOP * 130), 44100, SAMPLE_RATE)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
    pk = torch.empty(4, dtype=torch.float32, device=DEV)
    for c in range(4):
        _lib.check(L().svs_absmax(want[c].data_ptr(), want.shape[1], pk[c:].data_ptr(), ws.data_ptr(), ws.numel(), S()), "svs_absmax")
        _lib.check(L().svs_scale_by_inv(want[c].data_ptr(), want.shape[1], pk[c:].data_ptr(), 0.9, S()), "svs_scale_by_inv")
    got = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=0.9, sr_out=44100, both_stems=True, phase_iters=2)
    assert got.shape == (2, 2, want.shape[1]) and torch.equal(got.view(4, -1), want)
    assert torch.all((got.abs().amax(dim=2) - 0.9).abs() <= 1e-5)


def test_separate_to_wav_writes_both_files(tmp_path):
    from scipy.io import wavfile

    from svs_unet_pytorch_amd.streaming import separate_to_wav
    n = 90000                                                     # ~2 s of 44.1 kHz stereo: 131 frames at 512 / 128, two tiles
    mix = np.stack([synth.audio(n, 50), 0.5 * synth.audio(n, 51)], axis=1)
    src, voc, acc = (str(tmp_path / f) for f in ("mixture.wav", "vocal.wav", "accomp.wav"))
    wavfile.write(src, 44100, np.clip(np.round(mix * 20000), -32768, 32767).astype(np.int16))
    shape = separate_to_wav(random_model(), src, voc, n_fft=N_FFT, hop=HOP, subtype="FLOAT", dst_accomp_path=acc, phase_iters=2)
    assert tuple(shape) == (n, 2)
    files = []
    for path in (voc, acc):
        assert os.path.exists(path)
        rate, pcm = wavfile.read(path)
        assert rate == 44100 and pcm.dtype == np.float32 and pcm.shape == (n, 2) and np.isfinite(pcm).all()
        files.append(pcm)
    separate_to_wav(random_model(), src, voc, n_fft=N_FFT, hop=HOP, subtype="FLOAT", dst_accomp_path=acc)
    assert not np.array_equal(wavfile.read(voc)[1], files[0])    # the option reaches the files
