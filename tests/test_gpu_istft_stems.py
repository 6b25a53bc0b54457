"""Two-stem inverse STFT (-m gpu): svs_istft_stems_n writes istft(mag * mask * phase) and istft(mag * (1 - mask) * phase) from one
launch (inference.py:100-107 computes one of the two per run; the scorer forms the other as mix - vocal_est, evaluate.py:50-51).
Checked per stem against the float64 oracle at the masked single-stem path's own gate (tests/test_gpu_stft_windows.py: 5e-5 of the
stem's maximum), against the single-stem kernel (twice that, by the triangle inequality), for its peaks, its footprint, degenerate
masks and sizes, and through separate_waveform(both_stems=True) and the separate CLI's --tar_accomp."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import stft_oracle as so
from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd import data as svs_data

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEG = 32
GUARD = 4096
# (n_fft, hop): no tail positions | . | . | shared tail positions | . | . | . | tail loop | . | . | many rounds
CASES = [(512, 384), (512, 256), (512, 128), (1024, 768), (1024, 512), (1024, 256), (1024, 100),
         (2048, 1536), (2048, 1024), (2048, 512), (2048, 50)]


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr()


def plan(n_fft, hop):
    g, r, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    assert L().svs_istft_stems_plan_n(n_fft, hop, ctypes.byref(g), ctypes.byref(r), ctypes.byref(lds)) == 0
    return g.value, r.value, lds.value


def untile(x, rows, T):
    """(n_tiles, 1, rows, SEG) -> (rows, T)"""
    return x[:, 0].transpose(1, 0, 2).reshape(rows, -1)[:, :T]


def interior_of(n_fft, hop):
    # envelope troughs of hops above N / 4 amplify fp32 noise, and the envelope falls to zero at both ends (as test_gpu_stft_windows.py)
    return slice(None) if hop <= n_fft // 4 else slice(n_fft, -n_fft)


@functools.lru_cache(maxsize=None)
def case(n_fft, hop, n=None, frames=None):
    """Inputs on the device and the float64 expectation of both stems, computed once per (n_fft, hop) and never modified.
    frames: use only the first `frames` frames of the transform (the tiles keep their size)."""
    n = (12000 if hop < 100 else 40000) if n is None else n
    rows = n_fft // 2
    y2 = np.stack([synth.audio(n, 0), synth.audio(n, 1) * 0.5])
    tiles, phase, _, T = svs_data.stft_to_tiles(torch.from_numpy(y2).to(DEV), n_fft, hop, SEG)
    if frames is not None:
        assert 2 <= frames <= T
        T = frames
        phase = phase[:, :T].contiguous()
    mask = torch.from_numpy(synth.uniform(9, tiles.numel()).reshape(tiles.shape)).to(DEV)
    ph = torch.view_as_real(phase.contiguous()).contiguous()
    angle = torch.zeros_like(tiles)                              # phase mode 3: angles in the layout of the tiles
    ang_full = torch.angle(phase).permute(0, 2, 1)[:, 1:, :]     # (C, rows, T)
    n_tiles = tiles.shape[1]
    pad = torch.zeros((2, rows, n_tiles * SEG), device=DEV)
    pad[:, :, :T] = ang_full
    angle.copy_(pad.view(2, rows, n_tiles, SEG).permute(0, 2, 1, 3).unsqueeze(2))
    tiles_h, mask_h = tiles.cpu().numpy(), mask.cpu().numpy()
    want = np.empty((2, 2, hop * (T - 1)), np.float32)
    for c in range(2):
        full, mfull = untile(tiles_h[c], rows, T), untile(mask_h[c], rows, T)
        ph_o = so.magphase(so.stft(y2[c], n_fft, hop))[1][:, :T]  # the oracle's phasors, as test_inverse_vs_torch_istft's masked part
        for s, m in enumerate((mfull, 1.0 - mfull)):
            want[s, c] = so.istft(np.concatenate([np.zeros((1, T), np.float32), full * m], axis=0) * ph_o, n_fft, hop)
    return dict(n_fft=n_fft, hop=hop, T=T, rows=rows, tiles=tiles, mask=mask, ph=ph, angle=angle, want=want, n_tiles=n_tiles)


def run_stems(cs, mask=None, mode=1, partials=True, extra=0):
    """One launch into sentinel-filled, guarded buffers -> (y (2, C, n_out), partials (2, C, groups) or None).  extra: floats
    between the end of stem 0 and the start of stem 1."""
    n_fft, hop, T, rows = cs["n_fft"], cs["hop"], cs["T"], cs["rows"]
    tiles, mask = cs["tiles"], cs["mask"] if mask is None else mask
    C, n_out = 2, hop * (T - 1)
    stride = C * n_out + extra
    groups = L().svs_istft_stems_groups_n(n_fft, hop, T, C)
    ybuf = torch.full((GUARD + 2 * stride + GUARD,), -1.0, device=DEV)
    pbuf = torch.full((GUARD + 2 * C * groups + GUARD,), -1.0, device=DEV)
    y = ybuf[GUARD:GUARD + 2 * stride]
    src = cs["ph"] if mode == 1 else cs["angle"]
    _lib.check(L().svs_istft_stems_n(tiles.data_ptr(), cs["n_tiles"] * rows * SEG, SEG, rows, 1, mask.data_ptr(), src.data_ptr(), mode, C, n_fft,
                                     hop, T, y.data_ptr(), stride, pbuf[GUARD:].data_ptr() if partials else None, S()), "svs_istft_stems_n")
    # nothing outside [y, y + 2 * stem_stride) and the partials changed; inside, every element of both was overwritten
    assert torch.all(ybuf[:GUARD] == -1) and torch.all(ybuf[GUARD + 2 * stride:] == -1)
    assert torch.all(pbuf[:GUARD] == -1) and torch.all(pbuf[GUARD + 2 * C * groups:] == -1)
    out = y.view(2, stride)[:, :C * n_out].reshape(2, C, n_out)
    assert torch.all(y.view(2, stride)[:, C * n_out:] == -1)     # the gap between the stems is not written either
    assert not torch.any(out == -1.0)
    part = pbuf[GUARD:GUARD + 2 * C * groups].view(2, C, groups)
    if partials:
        assert torch.all(part >= 0)
        assert torch.equal(part.max(dim=2).values, out.abs().max(dim=2).values)     # exact: the maximum of the same floats
    else:
        assert torch.all(part == -1)
    return out, (part if partials else None)


def single(cs, mask, invert, mode=1):
    n_fft, hop, T, rows = cs["n_fft"], cs["hop"], cs["T"], cs["rows"]
    out = torch.empty((2, hop * (T - 1)), device=DEV)
    src = cs["ph"] if mode == 1 else cs["angle"]
    _lib.check(L().svs_istft_tiles_n(cs["tiles"].data_ptr(), cs["n_tiles"] * rows * SEG, SEG, rows, 1, None if mask is None else mask.data_ptr(),
                                     invert, src.data_ptr(), mode, 2, n_fft, hop, T, out.data_ptr(), None, S()), "svs_istft_tiles_n")
    return out


def gate_vs_float64(cs, got, report, tag, tol=5e-5):
    sl = interior_of(cs["n_fft"], cs["hop"])
    ok = True
    for s in range(2):
        for c in range(2):
            want = cs["want"][s, c]
            if want[sl].size == 0:
                continue
            e = np.abs(got[s, c].astype(np.float64) - want)[sl].max() / np.abs(want).max()
            print(tag, "stem", s, "ch", c, e)
            ok &= report(f"istft_stems {tag} stem{s} ch{c} vs float64", e, tol)
    return ok


@pytest.mark.parametrize("n_fft,hop", CASES)
def test_each_stem_vs_float64(n_fft, hop, report):
    """(1) both phase modes; (3) sentinels, guards and exact peaks are checked by run_stems on every launch."""
    cs = case(n_fft, hop)
    for mode in (1, 3):
        got, _ = run_stems(cs, mode=mode)
        # phase mode 3 goes through v_sin_f32 / v_cos_f32 of an angle that is itself atan2 in fp32: the masked single-stem gate holds
        assert gate_vs_float64(cs, got.cpu().numpy(), report, f"N={n_fft} hop={hop} mode={mode}")


@pytest.mark.parametrize("n_fft,hop", CASES)
def test_vs_single_stem_kernel(n_fft, hop, report):
    """(2) stem 0 against invert = 0, stem 1 against invert = 1, and their sum against the unmasked call."""
    cs = case(n_fft, hop)
    sl = interior_of(n_fft, hop)
    for mode in (1, 3):
        got, _ = run_stems(cs, mode=mode, extra=24)
        tag = f"N={n_fft} hop={hop} mode={mode}"
        for s in range(2):
            ref = single(cs, cs["mask"], s, mode)
            e = ((got[s] - ref).abs()[:, sl].max() / ref.abs().max()).item()
            print(tag, "stem", s, "vs single-stem kernel", e)
            assert report(f"istft_stems {tag} stem{s} vs svs_istft_tiles_n(invert={s})", e, 1e-4)
        whole = single(cs, None, 0, mode)
        e = ((got[0] + got[1] - whole).abs()[:, sl].max() / whole.abs().max()).item()
        print(tag, "stem0 + stem1 vs unmasked", e)
        assert report(f"istft_stems {tag} stem0 + stem1 vs unmasked", e, 1e-4)


@pytest.mark.parametrize("n_fft,hop", CASES)
def test_degenerate_masks_and_repeatability(n_fft, hop):
    """(4) a mask of all ones leaves stem 1 exactly zero (values and partials), all zeros the mirror image; two identical
    launches are bitwise equal; without a partials pointer nothing is written there."""
    cs = case(n_fft, hop)
    for value, empty in ((1.0, 1), (0.0, 0)):
        m = torch.full_like(cs["mask"], value)
        a, pa = run_stems(cs, mask=m)
        b, pb = run_stems(cs, mask=m)
        assert torch.all(a[empty] == 0.0) and torch.all(pa[empty] == 0.0)
        assert torch.equal(a[1 - empty], b[1 - empty]) and torch.equal(pa, pb) and a[1 - empty].abs().max() > 0
    for mode in (1, 3):
        a, pa = run_stems(cs, mode=mode)
        b, pb = run_stems(cs, mode=mode)
        assert torch.equal(a, b) and torch.equal(pa, pb)
        c, none = run_stems(cs, mode=mode, partials=False)
        assert none is None and torch.equal(c, a)


@pytest.mark.parametrize("n_fft,hop", CASES)
def test_minimum_and_one_hop_last_group(n_fft, hop, report):
    """(4) frames = 2, the minimum, and frames = hops_per_block + 1 (hops_per_block hops of output: with the n_fft padding the
    last group holds the rest), both at the gate of (1).  At two frames and hop > n_fft / 4 the interior slice is empty whenever
    hop <= 2 n_fft, which is always; the comparison is then made wherever the window envelope is at least 1e-2: the kernel's
    one-instruction window (hann_fast) is documented at ~1e-6 absolute, i.e. 1e-6 / w relative where a single frame of window
    value w covers a sample, and w^2 >= 1e-2 keeps that at 1e-5, a fifth of the gate.  For these hops that is every sample."""
    G, _, _ = plan(n_fft, hop)
    for frames in (2, G + 1):
        cs = case(n_fft, hop, None, frames)
        got, _ = run_stems(cs)
        got = got.cpu().numpy()
        n_out = hop * (frames - 1)
        assert got.shape == (2, 2, n_out)
        tag = f"N={n_fft} hop={hop} frames={frames}"
        sl = interior_of(n_fft, hop)
        if cs["want"][0, 0][sl].size:
            assert gate_vs_float64(cs, got, report, tag)
        else:
            env = so.window_sumsquare(frames, n_fft, hop)[n_fft // 2: n_fft // 2 + n_out]
            keep = env >= 1e-2
            assert keep.all()
            for s in range(2):
                for c in range(2):
                    want = cs["want"][s, c]
                    e = np.abs(got[s, c].astype(np.float64) - want)[keep].max() / np.abs(want).max()
                    print(tag, "stem", s, "ch", c, e)
                    assert report(f"istft_stems {tag} stem{s} ch{c} vs float64 (envelope >= 1e-2)", e, 5e-5)


def test_python_wrapper_and_peak():
    """data.istft_stems_from_tiles: the launch above, and with peak every stem and channel normalised on its own."""
    cs = case(1024, 768)
    from torch import view_as_complex
    phase = view_as_complex(cs["ph"])
    raw = svs_data.istft_stems_from_tiles(cs["tiles"], cs["mask"], phase, cs["T"], 1024, 768)
    assert raw.shape == (2, 2, 768 * (cs["T"] - 1)) and torch.equal(raw, run_stems(cs)[0])
    got = svs_data.istft_stems_from_tiles(cs["tiles"], cs["mask"], phase, cs["T"], 1024, 768, peak=0.9)
    assert torch.all((got.abs().amax(dim=2) - 0.9).abs() <= 1e-6)
    for s in range(2):
        ref = svs_data.istft_from_tiles(cs["tiles"], cs["mask"], phase, cs["T"], invert=bool(s), n_fft=1024, hop=768, peak=0.9)
        assert (got[s] - ref).abs().max().item() <= 1e-4 * 0.9
    with pytest.raises(ValueError, match="mask"):
        svs_data.istft_stems_from_tiles(cs["tiles"], None, phase, cs["T"], 1024, 768)


@functools.lru_cache(maxsize=None)
def random_model():
    from svs_unet_pytorch_amd.model import UNet
    torch.manual_seed(1234)
    return UNet().to(DEV).eval()


@pytest.mark.parametrize("n_fft,hop", [(1024, 768), (512, 128)])
def test_separate_waveform_both_stems(n_fft, hop, report):
    """(5) one STFT, one set of forwards, one inverse launch against the two single-stem calls."""
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model = random_model()
    n = hop * 140 + 17
    y = torch.from_numpy(np.stack([synth.audio(n, 20), 0.5 * synth.audio(n, 21)])).to(DEV)
    both = separate_waveform(model, y, n_fft=n_fft, hop=hop, peak=None, both_stems=True)
    assert both.shape == (2, 2, hop * (n // hop))
    for s, solo in enumerate((True, False)):
        ref = separate_waveform(model, y, vocal_solo=solo, n_fft=n_fft, hop=hop, peak=None)
        e = ((both[s] - ref).abs().max() / ref.abs().max()).item()
        print(f"separate_waveform both_stems N={n_fft} hop={hop} stem {s}", e)
        assert report(f"separate_waveform(both_stems) N={n_fft} hop={hop} stem{s} vs vocal_solo={solo}", e, 1e-4)
    assert torch.equal(separate_waveform(model, y, vocal_solo=False, n_fft=n_fft, hop=hop, peak=None, both_stems=True), both)   # vocal_solo is ignored
    mono = separate_waveform(model, y[0], n_fft=n_fft, hop=hop, both_stems=True)
    assert mono.shape == (2, hop * (n // hop)) and torch.all((mono.abs().amax(dim=1) - 0.9).abs() <= 1e-6)
    up = separate_waveform(model, y, n_fft=n_fft, hop=hop, both_stems=True, sr_out=44100)
    assert up.shape[:2] == (2, 2) and torch.all((up.abs().amax(dim=2) - 0.9).abs() <= 1e-6)


def test_separate_cli_writes_both_stems(tmp_path, report):
    """(5) --tar_accomp: the two files against the files of two single-stem runs (FLOAT), then PCM_16 form and peak, then a
    folder."""
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import separate
    ck = str(tmp_path / "svs_random.pth")
    torch.save({"model_state_dict": random_model().state_dict()}, ck)
    n = 66150                                                    # 1.5 s at 44,100 Hz
    mix = np.stack([synth.audio(n, 40), 0.5 * synth.audio(n, 41)], axis=1)
    os.makedirs(tmp_path / "in")
    src = str(tmp_path / "in" / "mixture.wav")
    wavfile.write(src, 44100, np.clip(np.round(mix * 20000), -32768, 32767).astype(np.int16))
    common = ["--model_path", ck, "--src", src]
    voc, acc = str(tmp_path / "vocal.wav"), str(tmp_path / "accomp.wav")
    separate.main(common + ["--tar", voc, "--tar_accomp", acc, "--subtype", "FLOAT"])
    for solo, got_path in ((1, voc), (0, acc)):
        ref_path = str(tmp_path / f"single{solo}.wav")
        separate.main(common + ["--tar", ref_path, "--vocal_solo", str(solo), "--subtype", "FLOAT"])
        (r0, got), (r1, ref) = wavfile.read(got_path), wavfile.read(ref_path)
        assert r0 == r1 == 44100 and got.dtype == ref.dtype == np.float32 and got.shape == ref.shape == (n, 2)
        e = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("separate --tar_accomp vs --vocal_solo", solo, e)
        assert report(f"separate CLI --tar_accomp vs --vocal_solo {solo}", e, 2e-4)
    separate.main(common + ["--tar", voc, "--tar_accomp", acc, "--subtype", "PCM_16"])
    for path in (voc, acc):
        rate, pcm = wavfile.read(path)
        assert rate == 44100 and pcm.dtype == np.int16 and pcm.shape == (n, 2)
        assert abs(int(np.abs(pcm.astype(np.int32)).max()) - round(0.9 * 32767)) <= 1
    separate.main(["--model_path", ck, "--src", str(tmp_path / "in"), "--tar", str(tmp_path / "v"), "--tar_accomp", str(tmp_path / "a")])
    assert os.listdir(tmp_path / "v") == os.listdir(tmp_path / "a") == ["mixture.wav"]
    assert np.array_equal(wavfile.read(str(tmp_path / "a" / "mixture.wav"))[1], wavfile.read(acc)[1])
