"""Overlapped tiles with cross-faded masks (-m gpu): svs_overlap_tiles bit for bit against numpy slicing, svs_overlap_blend against the
float64 definition (overlap.blend_reference), and the option through separate_waveform, separate_spectrogram_device,
inference.separate and the separate command line.  The network runs on 256 x 128 tiles (n_fft 512, hop 128).

The blend's tolerance is 2e-6 absolute on masks in [0, 1]: all terms are positive and at most 8 tiles cover a frame, so there are at
most 9 roundings in the numerator, 8 in the denominator and a division of at most 2.5 ulp, under 20 * 2^-24 = 1.2e-6."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd import data as svs_data
from svs_unet_pytorch_amd import overlap as ov
from svs_unet_pytorch_amd.config import INPUT_LEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
PAD = 8                   # floats between channels, beyond the data
SENTINEL = -777.0
TOL = 2e-6
N_FFT, HOP = 512, 128
SHAPES = [(rows, seg) for rows in (5, 512) for seg in (16, 128)]


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr()


def untile(x):
    """(C, n_tiles, rows, seg) -> (C, rows, n_tiles * seg)"""
    C, n_tiles, rows, seg = x.shape
    return x.transpose(0, 2, 1, 3).reshape(C, rows, n_tiles * seg)


def padded(values, C):
    """values (C, per) -> a device buffer of C channels `per + PAD` floats apart, the padding holding SENTINEL"""
    per = values.shape[1]
    buf = torch.full((C, per + PAD), SENTINEL, dtype=torch.float32, device=DEV)
    buf[:, :per] = torch.from_numpy(values).to(DEV)
    return buf


def geometries(seg):
    """tile_hop in {seg, seg/2, seg/4, seg/8} x 1..3 tiles x 1 and 2 channels; seg/8 of seg = 16 is 2, no multiple of 4 (test_refused_hop)"""
    for ratio in (1, 2, 4, 8):
        if (seg // ratio) % 4:
            continue
        for n_tiles in (1, 2, 3):
            for C in (1, 2):
                yield seg // ratio, n_tiles, C


def test_refused_hop():
    """seg 16 at tile_hop 16 / 8 = 2: four frames of a thread would straddle two sets of tiles, and the call is refused, not run."""
    x = torch.zeros(2 * 3 * 5 * 16, dtype=torch.float32, device=DEV)
    out = torch.full((2 * 17 * 5 * 16,), SENTINEL, dtype=torch.float32, device=DEV)
    assert L().svs_overlap_tiles(x.data_ptr(), 240, 2, 3, 5, 16, 2, out.data_ptr(), S()) == -1
    assert b"tile_hop must be a multiple of 4" in L().svs_last_error_string()
    assert L().svs_overlap_blend(out.data_ptr(), 2, 3, 5, 16, 2, None, 0, 0, x.data_ptr(), 240, S()) == -1
    assert b"tile_hop must be a multiple of 4" in L().svs_last_error_string()
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL) and torch.all(x == 0)


@pytest.mark.parametrize("rows,seg", SHAPES)
def test_overlap_tiles_is_numpy_slicing(rows, seg):
    """(1) every tile_hop in {seg, seg/2, seg/4, seg/8}, 1..3 tiles, 1 and 2 channels, bit for bit; the padding between the channels
    of the input and a guard behind the output keep their sentinel."""
    for hop, n_tiles, C in geometries(seg):
        per = n_tiles * rows * seg
        src = synth.uniform(11, C * per, offset=rows * seg + hop).reshape(C, per)
        buf = padded(src, C)
        n_ov = ov.overlap_count(n_tiles, seg, hop)
        out = torch.full((C * n_ov * rows * seg + PAD,), SENTINEL, dtype=torch.float32, device=DEV)
        _lib.check(L().svs_overlap_tiles(buf.data_ptr(), per + PAD, C, n_tiles, rows, seg, hop, out.data_ptr(), S()), "svs_overlap_tiles")
        full = untile(src.reshape(C, n_tiles, rows, seg))
        want = np.stack([full[c, :, j * hop:j * hop + seg] for c in range(C) for j in range(n_ov)])
        got = out.cpu().numpy()
        tag = f"rows={rows} seg={seg} hop={hop} n_tiles={n_tiles} C={C}"
        assert np.array_equal(got[:-PAD].reshape(C * n_ov, rows, seg), want), tag
        assert np.all(got[-PAD:] == SENTINEL), tag
        back = buf.cpu().numpy()
        assert np.array_equal(back[:, :per], src) and np.all(back[:, per:] == SENTINEL), tag


def run_blend(masks, C, n_tiles, rows, seg, hop, mix=None, invert=0):
    """The kernel on (C * n_ov, rows, seg) device masks -> ((C, per) result, the whole padded output buffer)."""
    per = n_tiles * rows * seg
    out = torch.full((C, per + PAD), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.check(L().svs_overlap_blend(masks.data_ptr(), C, n_tiles, rows, seg, hop, None if mix is None else mix.data_ptr(), per + PAD, invert,
                                     out.data_ptr(), per + PAD, S()), "svs_overlap_blend")
    return out[:, :per], out


@pytest.mark.parametrize("rows,seg", SHAPES)
def test_overlap_blend_vs_float64_definition(rows, seg, report):
    """(2) against blend_reference at 2e-6; frames one tile covers (everything at n_tiles = 1 or tile_hop = seg, and the first and
    last tile_hop frames of a song otherwise) are == the input; the invert and mix forms are == svs_apply_mask on the kernel's own
    b; two runs are bit-identical; the padding of the output keeps its sentinel."""
    worst = 0.0
    for hop, n_tiles, C in geometries(seg):
        per = n_tiles * rows * seg
        n_ov = ov.overlap_count(n_tiles, seg, hop)
        m_np = synth.uniform(12, C * n_ov * rows * seg, offset=7 * hop + n_tiles).reshape(C * n_ov, rows, seg)
        masks = torch.from_numpy(m_np).to(DEV)
        b, whole = run_blend(masks, C, n_tiles, rows, seg, hop)
        tag = f"rows={rows} seg={seg} hop={hop} n_tiles={n_tiles} C={C}"
        assert torch.all(whole[:, per:] == SENTINEL), tag
        got = untile(b.cpu().numpy().reshape(C, n_tiles, rows, seg))
        e = float(np.abs(got.astype(np.float64) - ov.blend_reference(m_np, n_tiles, hop)).max())
        worst = max(worst, e)
        print("svs_overlap_blend", tag, "max |b - float64|", e)
        assert e <= TOL, (tag, e)
        per_ch = m_np.reshape(C, n_ov, rows, seg)
        if n_ov == 1 or hop == seg:                                # one tile everywhere: a copy
            assert np.array_equal(got, untile(per_ch)), tag
        else:                                                      # both ends of the song
            assert np.array_equal(got[:, :, :hop], per_ch[:, 0, :, :hop]), tag
            assert np.array_equal(got[:, :, -hop:], per_ch[:, -1, :, -hop:]), tag
        assert torch.equal(run_blend(masks, C, n_tiles, rows, seg, hop)[0], b), tag
        # the other three forms against svs_apply_mask (inference.py:100-107) on b, channel by channel
        mix = padded(synth.uniform(13, C * per, offset=hop).reshape(C, per) * np.float32(3.0), C)
        bc = b.contiguous()
        ones = torch.ones(per, dtype=torch.float32, device=DEV)
        for invert, with_mix in ((1, False), (0, True), (1, True)):
            form, whole = run_blend(masks, C, n_tiles, rows, seg, hop, mix if with_mix else None, invert)
            assert torch.all(whole[:, per:] == SENTINEL), tag
            want = torch.empty(per, dtype=torch.float32, device=DEV)
            for c in range(C):
                x = mix[c, :per].contiguous() if with_mix else ones
                _lib.check(L().svs_apply_mask(x.data_ptr(), bc[c].data_ptr(), want.data_ptr(), per, invert, S()), "svs_apply_mask")
                assert torch.equal(form[c], want), (tag, invert, with_mix, c)
        assert torch.all(mix[:, per:] == SENTINEL), tag
    assert report(f"svs_overlap_blend rows={rows} seg={seg} vs blend_reference (max over hops, tiles, channels)", worst, TOL)


# ---- through the network ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_model():
    from svs_unet_pytorch_amd.model import UNet
    torch.manual_seed(4321)
    return UNet().to(DEV).eval()


@functools.lru_cache(maxsize=None)
def stereo():
    """2 channels, 301 frames at n_fft 512 / hop 128: 3 disjoint tiles, 5 overlapped ones at tile_hop 64."""
    n = HOP * 300 + 17
    return torch.from_numpy(np.stack([synth.audio(n, 30), 0.5 * synth.audio(n, 31)])).to(DEV)


def compose(tile_hop, precision=None, max_batch=256):
    """separate_waveform's steps through the public pieces, up to the blended mask: (tiles, phase, T, overlapped masks, mask)."""
    model, y = random_model(), stereo()
    tiles, phase, norm, T = svs_data.stft_to_tiles(y, N_FFT, HOP, INPUT_LEN)
    for c in range(tiles.shape[0]):
        _lib.check(L().svs_scale_by_inv(tiles[c].data_ptr(), tiles[c].numel(), norm[c:].data_ptr(), 1.0, S()), "svs_scale_by_inv")
    n_tiles = tiles.shape[1]
    assert tiles.shape == (2, 3, 1, N_FFT // 2, INPUT_LEN) and T == 301
    tiled = ov.overlap_tiles(tiles, tile_hop)
    masks = torch.empty_like(tiled)
    was = model.eval_precision
    try:
        if precision is not None:
            model.eval_precision = precision
        with torch.no_grad():
            for s in range(0, tiled.shape[0], max_batch):
                masks[s:s + max_batch] = model(tiled[s:s + max_batch])
    finally:
        model.eval_precision = was
    return tiles, phase, T, masks, ov.blend_masks(masks, n_tiles, tile_hop)


def mask_gate(masks, mask, n_tiles, tile_hop, report, name):
    got = untile(mask[:, :, 0].cpu().numpy())
    e = float(np.abs(got.astype(np.float64) - ov.blend_reference(masks.cpu().numpy(), n_tiles, tile_hop)).max())
    print(name, "max |mask - float64|", e)
    assert report(name, e, TOL)


@pytest.mark.parametrize("precision", [None, "bf16"])
def test_separate_waveform_is_its_composition(precision, report):
    """(3) tile_hop = 64, bit-equal to stft_to_tiles, scale, overlap_tiles, model, blend_masks, istft_from_tiles; the blended mask within
    2e-6 of the definition on the model's own overlapped masks; the same for both stems, whose sum is the mixture's reconstruction
    at the gate tests/test_gpu_istft_stems.py has for that identity (1e-4 of its maximum; hop = n_fft / 4: every sample)."""
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    tiles, phase, T, masks, mask = compose(64, precision)
    assert masks.shape == (10, 1, 256, 128) and mask.shape == tiles.shape
    want = svs_data.istft_from_tiles(tiles, mask, phase, T, n_fft=N_FFT, hop=HOP)
    got = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=None, precision=precision, tile_hop=64)
    assert got.shape == (2, HOP * 300) and torch.equal(got, want)
    assert model.eval_precision == "fp32" and not model.training
    mask_gate(masks, mask, 3, 64, report, f"separate_waveform tile_hop=64 precision={precision}: blended mask vs blend_reference")
    if precision is None:
        inv = separate_waveform(model, y, vocal_solo=False, n_fft=N_FFT, hop=HOP, peak=None, tile_hop=64)
        assert torch.equal(inv, svs_data.istft_from_tiles(tiles, mask, phase, T, invert=True, n_fft=N_FFT, hop=HOP))
        both = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=None, both_stems=True, tile_hop=64)
        assert both.shape == (2, 2, HOP * 300)
        assert torch.equal(both, svs_data.istft_stems_from_tiles(tiles, mask, phase, T, n_fft=N_FFT, hop=HOP))
        whole = svs_data.istft_from_tiles(tiles, None, phase, T, n_fft=N_FFT, hop=HOP)
        e = ((both[0] + both[1] - whole).abs().max() / whole.abs().max()).item()
        print("tile_hop=64 stem0 + stem1 vs unmasked", e)
        assert report("separate_waveform(both_stems, tile_hop=64) stem0 + stem1 vs unmasked", e, 1e-4)


def test_tile_hop_128_is_the_default_path():
    """(4) passing the default explicitly changes nothing, in all three functions."""
    from svs_unet_pytorch_amd import inference
    from svs_unet_pytorch_amd.streaming import separate_spectrogram_device, separate_waveform
    model, y = random_model(), stereo()
    for kw in ({}, {"both_stems": True}, {"vocal_solo": False, "precision": "bf16"}):
        a = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, **kw)
        assert torch.equal(separate_waveform(model, y, n_fft=N_FFT, hop=HOP, tile_hop=INPUT_LEN, **kw), a)
    mag = torch.from_numpy(synth.uniform(14, 257 * 300).reshape(257, 300)).to(DEV)
    for solo in (True, False):
        a = separate_spectrogram_device(model, mag, vocal_solo=solo)
        assert torch.equal(separate_spectrogram_device(model, mag, vocal_solo=solo, tile_hop=INPUT_LEN), a)
        b = inference.separate(model, mag.cpu().numpy(), vocal_solo=solo)
        assert np.array_equal(inference.separate(model, mag.cpu().numpy(), vocal_solo=solo, tile_hop=INPUT_LEN), b)


@pytest.mark.parametrize("seg_len", [256, 64])
def test_default_is_disjoint_tiles_at_any_seg_len(seg_len):
    """(4) at a tile length other than 128: omitting tile_hop separates disjoint seg_len-frame tiles -- bit-equal to the masks of the
    disjoint tiles applied with svs_apply_mask, which is all these two functions did before the option -- and so does tile_hop =
    seg_len; half of it takes the overlapped route there too.  128 rows, 300 frames: 2 tiles of 256, 5 of 64, the last one padded."""
    from svs_unet_pytorch_amd import inference
    from svs_unet_pytorch_amd.streaming import separate_spectrogram_device
    model = random_model()
    rows, T = 128, 300
    mag_np = synth.uniform(16, (rows + 1) * T, offset=seg_len).reshape(rows + 1, T)
    mag = torch.from_numpy(mag_np).to(DEV)
    n = -(-T // seg_len)
    pad = np.zeros((rows, n * seg_len), np.float32)
    pad[:, :T] = mag_np[1:]
    tiles = torch.from_numpy(np.ascontiguousarray(pad.reshape(rows, n, seg_len).transpose(1, 0, 2))).to(DEV).unsqueeze(1)
    with torch.no_grad():
        masks = model(tiles)
    for solo in (True, False):
        want = torch.empty_like(tiles)
        _lib.check(L().svs_apply_mask(tiles.data_ptr(), masks.data_ptr(), want.data_ptr(), tiles.numel(), 0 if solo else 1, S()), "svs_apply_mask")
        want = want[:, 0].permute(1, 0, 2).reshape(rows, n * seg_len)[:, :T]
        got = separate_spectrogram_device(model, mag, seg_len=seg_len, vocal_solo=solo)
        assert got.shape == (rows + 1, T) and torch.all(got[0] == 0) and torch.equal(got[1:], want)
        assert torch.equal(separate_spectrogram_device(model, mag, seg_len=seg_len, vocal_solo=solo, tile_hop=seg_len), got)
        host = inference.separate(model, mag_np, seg_len=seg_len, vocal_solo=solo)
        assert np.array_equal(host, got.cpu().numpy())
        assert np.array_equal(inference.separate(model, mag_np, seg_len=seg_len, vocal_solo=solo, tile_hop=seg_len), host)
    half = separate_spectrogram_device(model, mag, seg_len=seg_len, tile_hop=seg_len // 2)
    assert half.shape == got.shape and not torch.equal(half, separate_spectrogram_device(model, mag, seg_len=seg_len))
    assert np.array_equal(inference.separate(model, mag_np, seg_len=seg_len, tile_hop=seg_len // 2), half.cpu().numpy())


def test_remainder_batches_through_the_spectrogram_path():
    """max_batch that does not divide the tiles: 128 rows, 300 frames at seg_len 64 are 5 tiles, batches of 2, 2 and 1.  Bit-equal
    to the model on those three slices and ONE svs_apply_mask over all five, on the device and through the host wrapper.  (Nothing
    is compared across max_batch values: the layers' plans, and with them the bits of the masks, depend on the batch size.)"""
    from svs_unet_pytorch_amd import inference
    from svs_unet_pytorch_amd.streaming import separate_spectrogram_device
    model = random_model()
    rows, T, seg_len, max_batch = 128, 300, 64, 2
    mag_np = synth.uniform(17, (rows + 1) * T, offset=seg_len).reshape(rows + 1, T)
    mag = torch.from_numpy(mag_np).to(DEV)
    n = -(-T // seg_len)
    assert n == 5
    pad = np.zeros((rows, n * seg_len), np.float32)
    pad[:, :T] = mag_np[1:]
    tiles = torch.from_numpy(np.ascontiguousarray(pad.reshape(rows, n, seg_len).transpose(1, 0, 2))).to(DEV).unsqueeze(1)
    with torch.no_grad():
        batches = [model(tiles[s:s + max_batch]) for s in range(0, n, max_batch)]
    assert [b.shape[0] for b in batches] == [2, 2, 1]
    masks = torch.cat(batches)
    for solo in (True, False):
        want = torch.empty_like(tiles)
        _lib.check(L().svs_apply_mask(tiles.data_ptr(), masks.data_ptr(), want.data_ptr(), tiles.numel(), 0 if solo else 1, S()), "svs_apply_mask")
        want = want[:, 0].permute(1, 0, 2).reshape(rows, n * seg_len)[:, :T]
        got = separate_spectrogram_device(model, mag, seg_len=seg_len, vocal_solo=solo, max_batch=max_batch)
        assert got.shape == (rows + 1, T) and torch.all(got[0] == 0) and torch.equal(got[1:], want)
        host = inference.separate(model, mag_np, seg_len=seg_len, vocal_solo=solo, max_batch=max_batch)
        assert host.dtype == np.float32 and np.array_equal(host, got.cpu().numpy())
    assert not model.training and model.eval_precision == "fp32"


def test_remainder_batches_through_the_waveform_path():
    """The same through separate_waveform: 10 overlapped tiles at tile_hop 64 in batches of 4, 4 and 2, bit-equal to the composition
    with those batches, for one stem and for both."""
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    tiles, phase, T, masks, mask = compose(64, max_batch=4)
    assert masks.shape[0] == 10
    one = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=None, tile_hop=64, max_batch=4)
    assert one.shape == (2, HOP * 300) and torch.equal(one, svs_data.istft_from_tiles(tiles, mask, phase, T, n_fft=N_FFT, hop=HOP))
    both = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=None, both_stems=True, tile_hop=64, max_batch=4)
    assert both.shape == (2, 2, HOP * 300) and torch.equal(both, svs_data.istft_stems_from_tiles(tiles, mask, phase, T, n_fft=N_FFT, hop=HOP))
    assert not model.training and model.eval_precision == "fp32"


def test_the_option_does_something():
    """(5) tile_hop = 64 changes the output, and leaves the mask of the song's first and last 64 frames bit for bit what disjoint
    tiles give: overlapped tile 0 is disjoint tile 0 and the last overlapped tile is the last disjoint one, and one tile covers
    those frames.  The forwards run one tile at a time (max_batch = 1) so that both runs hand the network the same batch for those
    tiles: the layers' plans, and with them the order of their sums, depend on the batch size."""
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    a = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=None)
    b = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=None, tile_hop=64)
    assert a.shape == b.shape and not torch.equal(a, b)
    _, _, _, _, disjoint = compose(INPUT_LEN, max_batch=1)
    _, _, _, _, crossfaded = compose(64, max_batch=1)
    d, x = disjoint[:, :, 0], crossfaded[:, :, 0]                  # (2, 3, 256, 128)
    assert torch.equal(d[:, 0, :, :64], x[:, 0, :, :64]) and torch.equal(d[:, -1, :, -64:], x[:, -1, :, -64:])
    assert not torch.equal(d[:, 0, :, 64:], x[:, 0, :, 64:]) and not torch.equal(d[:, 1], x[:, 1])


@pytest.mark.parametrize("T", [300, 128])
def test_separate_spectrogram_device_tile_hop_32(T, report):
    """(6) 300 frames (3 tiles, the last one zero-padded, 9 overlapped tiles) and exactly one tile: mix * b and mix * (1 - b) against
    the float64 definition on the model's own masks; 1 - b and the product add two roundings of values below 1, 2^-25 each, to the
    blend's 2e-6."""
    from svs_unet_pytorch_amd import inference
    from svs_unet_pytorch_amd.streaming import separate_spectrogram_device
    model = random_model()
    mag_np = synth.uniform(15, 257 * T, offset=T).reshape(257, T)
    mag = torch.from_numpy(mag_np).to(DEV)
    n = -(-T // INPUT_LEN)
    pad = np.zeros((256, n * INPUT_LEN), np.float32)
    pad[:, :T] = mag_np[1:]
    tiles = torch.from_numpy(np.ascontiguousarray(pad.reshape(256, n, INPUT_LEN).transpose(1, 0, 2))).to(DEV).view(1, n, 1, 256, INPUT_LEN)
    with torch.no_grad():
        masks = model(ov.overlap_tiles(tiles, 32))
    assert masks.shape[0] == (n - 1) * 4 + 1
    b = ov.blend_reference(masks.cpu().numpy(), n, 32)[0][:, :T]
    tol = TOL + 2.0 ** -24
    for solo in (True, False):
        got = separate_spectrogram_device(model, mag, vocal_solo=solo, tile_hop=32)
        assert got.shape == (257, T) and got.dtype == torch.float32 and torch.all(got[0] == 0)
        want = mag_np[1:].astype(np.float64) * (b if solo else 1.0 - b)
        e = float(np.abs(got[1:].cpu().numpy() - want).max())
        print(f"separate_spectrogram_device tile_hop=32 T={T} vocal_solo={solo}", e)
        assert report(f"separate_spectrogram_device(tile_hop=32) T={T} vocal_solo={solo} vs float64", e, tol)
        assert np.array_equal(inference.separate(model, mag_np, vocal_solo=solo, tile_hop=32), got.cpu().numpy())
    with pytest.raises(ValueError, match="divides the tile length"):
        separate_spectrogram_device(model, mag, tile_hop=48)


def test_separate_cli_tile_hop(tmp_path):
    """(7) --tile_hop 64 --tar_accomp on 3 s of 44.1 kHz stereo (two tiles at --win_size 512 --hop_size 128): two files of the
    source's frame and channel count, different from the default run's.  The --tile_hop run is `python -m
    svs_unet_pytorch_amd.separate` as a process; the default run calls the same main() here."""
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import separate
    ck = str(tmp_path / "svs_random.pth")
    torch.save({"model_state_dict": random_model().state_dict()}, ck)
    n = 132300
    mix = np.stack([synth.audio(n, 50), 0.5 * synth.audio(n, 51)], axis=1)
    src = str(tmp_path / "mixture.wav")
    wavfile.write(src, 44100, np.clip(np.round(mix * 20000), -32768, 32767).astype(np.int16))
    files = {}
    for name, extra in (("default", []), ("hop64", ["--tile_hop", "64"])):
        voc, acc = str(tmp_path / f"{name}_vocal.wav"), str(tmp_path / f"{name}_accomp.wav")
        args = ["--model_path", ck, "--src", src, "--tar", voc, "--tar_accomp", acc, "--win_size", "512", "--hop_size", "128",
                "--subtype", "FLOAT"] + extra
        if extra:                                                  # the option as a user types it: the module's own entry, one process
            r = subprocess.run([sys.executable, "-m", "svs_unet_pytorch_amd.separate"] + args, cwd=ROOT, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        else:
            separate.main(args)
        for path in (voc, acc):
            assert os.path.exists(path)
            rate, pcm = wavfile.read(path)
            assert rate == 44100 and pcm.dtype == np.float32 and pcm.shape == (n, 2)
        files[name] = (wavfile.read(voc)[1], wavfile.read(acc)[1])
    for k in range(2):
        assert not np.array_equal(files["default"][k], files["hop64"][k])
