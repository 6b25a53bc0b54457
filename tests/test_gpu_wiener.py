"""The multichannel Wiener filter on the device (-m gpu): svs_wiener_model and svs_wiener_stems against the float64 definition
wiener.wiener_reference, fed the same float32 tiles, mask and phasors converted to float64, after every model pass and at the
end; the layout promises of the stems (guards, padding, exact phasors); the argument rules; and wiener_iters through
separate_waveform / separate_to_wav.

32-frame tiles with T = 41 frames, so the last tile is padded; tiles and phasors are the GPU's own forward transform's.

Gates.  All arithmetic on the device is fp64; what differs from the reference is that v is stored as float32 between passes and
the stems as float32 magnitudes and phasors.  A CPU emulation of the float32 v alone gives at most 7.5e-8 of the peak, identical
channels included; rounding the stems' magnitudes and phasors to float32 adds up to one ulp of each.  V_GATE / R_GATE / Y_GATE are
4x the maxima measured on an MI355X over all cases below (DESIGN.md section 15 has the figures); a measured maximum above 2e-6,
the gate tests/test_gpu_stft_windows.py holds mag x phasor products to, would be a bug (SANITY)."""
import functools
import os

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd import data as svs_data
from svs_unet_pytorch_amd import overlap as ov
from svs_unet_pytorch_amd import rephase as rp
from svs_unet_pytorch_amd import wiener as wn
from svs_unet_pytorch_amd.config import INPUT_LEN, SAMPLE_RATE

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -777.0
GUARD = 64                # floats before and after a buffer
GAP = 32                  # floats between the stems, beyond one stem's size
SEG, T = 32, 41
MAX_ITERS = 4
GEOMETRY = {256: (512, 384), 512: (1024, 768)}          # rows -> (n_fft, hop)
KINDS = ("panned", "identical", "silent", "mono")
# 4x the maxima measured on an MI355X over every case below (DESIGN.md section 15 has them per case)
V_GATE = 2.0e-7           # |v - v_ref| / max v_ref after every model pass                      measured: 4.9e-8
R_GATE = 6.4e-7           # |R - R_ref| / the largest |entry| of R_ref at that frequency         measured: 1.6e-7 (1e-15 after the first pass)
Y_GATE = 6.4e-7           # |mag x phasor - y_ref| / max |y_ref|                                 measured: 1.6e-7 (6.3e-8 after one update)
SANITY = 2e-6


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr()


def c128(t):
    return torch.view_as_complex(torch.view_as_real(t).cpu().double()).numpy()


def untile(t, frames=T):
    """(..., n_tiles, 1, rows, seg) device tiles -> float64 (..., rows, frames)"""
    a = t.cpu().numpy().astype(np.float64)
    a = a.reshape((-1,) + a.shape[-4:])[:, :, 0]
    n, n_tiles, rows, seg = a.shape
    return a.transpose(0, 2, 1, 3).reshape(n, rows, n_tiles * seg)[:, :, :frames].reshape(t.shape[:-4] + (rows, frames))


def sources(n):
    """Two band-limited, time-gated noise sources, float64 (2, n)."""
    out = []
    for j, (band, gate) in enumerate((((0.02, 0.30), (0.00, 0.65)), ((0.18, 0.70), (0.30, 1.00)))):
        spec = np.fft.rfft(synth.audio(n, 40 + j).astype(np.float64))
        k = np.arange(spec.size) / (spec.size - 1)
        spec[(k < band[0]) | (k > band[1])] = 0
        t = np.arange(n) / n
        out.append(np.fft.irfft(spec, n) * ((t >= gate[0]) & (t < gate[1])))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def case(rows, kind):
    """The device inputs of one case, the model after each of MAX_ITERS passes on the device, and the float64 reference of each."""
    n_fft, hop = GEOMETRY[rows]
    n = hop * 40 + 5
    src = sources(n)
    pan = np.array([[0.9, 0.3], [0.3, 0.9]])
    images = pan[:, :, None] * src[:, None, :]                                       # (source, channel, n)
    if kind == "identical":
        images = np.stack([images[:, 0], images[:, 0]], axis=1)
    elif kind == "silent":
        images[:, 1] = 0
    elif kind == "mono":
        images = images[:, :1]
    C = images.shape[1]
    y = torch.from_numpy(images.sum(axis=0).astype(np.float32)).to(DEV)
    tiles, phase, norm, frames = svs_data.stft_to_tiles(y, n_fft, hop, SEG)
    assert frames == T and tiles.shape == (C, 2, 1, rows, SEG)
    for c in range(C):
        _lib.check(L().svs_scale_by_inv(tiles[c].data_ptr(), tiles[c].numel(), norm[c:].data_ptr(), 1.0, S()), "svs_scale_by_inv")
    # 0.6 x the ideal ratio mask + 0.4 x uniform noise, the padded frames of the last tile included (they must not be read)
    a = np.abs(rp.reference_stft(images, n_fft, hop)[:, :, 1:])                       # (source, channel, rows, T)
    ideal = np.zeros((C, rows, 2 * SEG))
    ideal[:, :, :T] = a[0] / np.where(a[0] + a[1] > 0, a[0] + a[1], 1.0)
    noise = synth.uniform(44, ideal.size).astype(np.float64).reshape(ideal.shape)
    if kind == "identical":
        noise[1] = noise[0]
    m = (0.6 * ideal + 0.4 * noise).astype(np.float32)
    mask = torch.from_numpy(np.ascontiguousarray(m.reshape(C, rows, 2, SEG).transpose(0, 2, 1, 3))[:, :, None]).to(DEV).contiguous()
    scale = wn.common_scale(norm)
    if kind == "silent":
        assert scale[1].item() == 0.0 and not tiles[1].any()

    models = []
    for _ in range(MAX_ITERS):
        models.append(wn.wiener_model(tiles, mask if not models else None, phase, scale, T, models[-1] if models else None))

    sc = scale.cpu().numpy().astype(np.float64)[:, None, None]
    P = np.moveaxis(c128(phase), -1, -2)[:, 1:]                                       # (C, rows, T): float32 phasors, |P| = 1 +- 6e-8
    mag, m64 = untile(tiles), untile(mask)
    x = sc * mag * P
    start = np.stack([sc * mag * m64 * np.abs(P), sc * mag * (1.0 - m64) * np.abs(P)])
    refs = [wn.wiener_reference(x, start, it) for it in range(1, MAX_ITERS + 1)]
    return dict(C=C, tiles=tiles, mask=mask, phase=phase, scale=scale, norm=norm, models=models, refs=refs, x=x)


def R_matrix(R, C):
    """(2, rows, 4) device doubles -> complex128 (2, rows, C, C)"""
    r = R.cpu().numpy()
    out = np.zeros(r.shape[:2] + (2, 2), dtype=np.complex128)
    out[..., 0, 0], out[..., 1, 1] = r[..., 0], r[..., 1]
    out[..., 0, 1] = r[..., 2] + 1j * r[..., 3]
    out[..., 1, 0] = r[..., 2] - 1j * r[..., 3]
    return out[..., :C, :C]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", [256, 512])
def test_model_passes_vs_float64(rows, kind, report):
    k = case(rows, kind)
    for it in range(MAX_ITERS):
        v, R = k["models"][it]
        _, v_ref, R_ref = k["refs"][it]
        full = v[:, :, 0].cpu().numpy()                                              # (2, n_tiles, rows, seg)
        assert np.all(full[:, 1, :, T - SEG:] == 0)                                  # the padded frames hold exact zeros
        e_v = np.abs(untile(v) - v_ref).max() / v_ref.max()
        top = np.abs(R_ref).max(axis=(2, 3))
        e_R = (np.abs(R_matrix(R, k["C"]) - R_ref).max(axis=(2, 3)) / np.where(top > 0, top, 1.0)).max()
        name = f"wiener model rows={rows} {kind} pass {it + 1}"
        print(name, "v", e_v, "R", e_R)
        assert e_v < SANITY and e_R < SANITY
        assert report(f"{name} v", e_v, V_GATE)
        assert report(f"{name} R", e_R, R_GATE)
        if k["C"] == 1:
            assert not R[:, :, 1:].any()


def run_stems(k, rows, iters, stem):
    """svs_wiener_stems into guarded buffers whose stems lie GAP floats apart -> (host magnitudes, host phasors, one stem's sizes)."""
    C, tiles = k["C"], k["tiles"]
    one = 2 * rows * SEG
    mag_one, ph_one = C * one, C * T * (rows + 1) * 2
    mags = torch.full((GUARD + 2 * mag_one + GAP + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    ph = torch.full((GUARD + 2 * ph_one + GAP + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    v, R = k["models"][iters - 1]
    phase = torch.view_as_real(k["phase"].contiguous()).contiguous()
    _lib.check(L().svs_wiener_stems(tiles.data_ptr(), one, SEG, rows, phase.data_ptr(), k["scale"].data_ptr(), C, T, v.data_ptr(), one,
                                    R.data_ptr(), wn.REG, stem, mags.data_ptr() + 4 * GUARD, one, mag_one + GAP, ph.data_ptr() + 4 * GUARD,
                                    ph_one + GAP, S()), "svs_wiener_stems")
    return mags.cpu().numpy(), ph.cpu().numpy(), mag_one, ph_one


@pytest.mark.parametrize("stem", [0, 1, 2])
@pytest.mark.parametrize("iters", [1, 2, 4])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", [256, 512])
def test_stems_vs_float64(rows, kind, iters, stem, report):
    k = case(rows, kind)
    C = k["C"]
    mags, ph, mag_one, ph_one = run_stems(k, rows, iters, stem)
    y_ref = k["refs"][iters - 1][0]                                                  # (2, C, rows, T)
    written = (0, 1) if stem == 2 else (stem,)
    for slot, j in enumerate(written):
        mo, po = GUARD + slot * (mag_one + GAP), GUARD + slot * (ph_one + GAP)
        m = mags[mo:mo + mag_one].reshape(C, 2, rows, SEG)
        p = ph[po:po + ph_one].astype(np.float64).reshape(C, T, rows + 1, 2)
        p = np.moveaxis(p[..., 0] + 1j * p[..., 1], -1, -2)                          # (C, rows + 1, T)
        assert np.all(m[:, 1, :, T - SEG:] == 0)                                     # exactly zero in the padded frames
        mag = m.astype(np.float64).transpose(0, 2, 1, 3).reshape(C, rows, 2 * SEG)[:, :, :T]
        assert np.all(p[:, 0] == 1.0 + 0.0j)                                         # the DC bin
        assert np.all(p[:, 1:][mag == 0] == 1.0 + 0.0j)                              # phasor(0) = 1 + 0i
        assert np.abs(np.abs(p) - 1).max() <= 4 * 2e-7
        e = np.abs(mag * p[:, 1:] - y_ref[j]).max() / np.abs(y_ref[j]).max()
        name = f"wiener stems rows={rows} {kind} iters={iters} stem {j}" + (" of both" if stem == 2 else " alone")
        print(name, e)
        assert e < SANITY
        assert report(name, e, Y_GATE)
        if kind == "silent":
            assert not mag[1].any() and np.all(p[1] == 1.0 + 0.0j) and mag[0].max() > 0.1
            assert np.all(y_ref[j][1] == 0)
    # nothing outside the stems is written: before, after, between -- and, for one stem, where the other would lie
    end_m = GUARD + (len(written) - 1) * (mag_one + GAP) + mag_one
    end_p = GUARD + (len(written) - 1) * (ph_one + GAP) + ph_one
    assert np.all(mags[:GUARD] == SENTINEL) and np.all(mags[end_m:] == SENTINEL)
    assert np.all(ph[:GUARD] == SENTINEL) and np.all(ph[end_p:] == SENTINEL)
    if stem == 2:
        assert np.all(mags[GUARD + mag_one:GUARD + mag_one + GAP] == SENTINEL)
        assert np.all(ph[GUARD + ph_one:GUARD + ph_one + GAP] == SENTINEL)


@pytest.mark.parametrize("kind", ["panned", "mono"])
def test_two_runs_are_bitwise_equal_and_the_filter_is_its_passes(kind):
    k = case(256, kind)
    for iters in (1, 3):
        a = wn.wiener_filter(k["tiles"], k["mask"], k["phase"], k["norm"], T, iters)
        b = wn.wiener_filter(k["tiles"], k["mask"], k["phase"], k["norm"], T, iters)
        assert torch.equal(a[0], b[0]) and torch.equal(torch.view_as_real(a[1]), torch.view_as_real(b[1]))
        # the in-place updates of wiener_filter are the out-of-place passes of case()
        c = wn.wiener_stems(k["tiles"], k["phase"], k["scale"], T, k["models"][iters - 1])
        assert torch.equal(a[0], c[0]) and torch.equal(torch.view_as_real(a[1]), torch.view_as_real(c[1]))
        for j in (0, 1):
            one = wn.wiener_filter(k["tiles"], k["mask"], k["phase"], k["norm"], T, iters, stems=(j,))
            assert one[0].shape[0] == 1 and torch.equal(one[0][0], a[0][j]) and torch.equal(torch.view_as_real(one[1][0]), torch.view_as_real(a[1][j]))
    again = wn.wiener_model(k["tiles"], k["mask"], k["phase"], k["scale"], T)
    assert torch.equal(again[0], k["models"][0][0]) and torch.equal(again[1], k["models"][0][1])


def test_every_rule_is_checked_before_any_launch():
    k = case(256, "panned")
    rows, one = 256, 2 * 256 * SEG
    tiles, mask, scale = k["tiles"], k["mask"], k["scale"]
    phase = torch.view_as_real(k["phase"].contiguous()).contiguous()
    v0, R0 = k["models"][0]
    v = torch.full((2 * one + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    R = torch.full((2 * rows * 4 + 2,), SENTINEL, dtype=torch.float64, device=DEV)
    ws_bytes = int(L().svs_wiener_workspace_bytes(2, rows, SEG, T))
    assert ws_bytes == 2 * 8 * rows * 8                                              # 2 chunks (one per 32-frame tile) x 8 sums x rows doubles
    ws = torch.empty(ws_bytes + 16, dtype=torch.uint8, device=DEV)
    om = torch.full((4 * one + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    op = torch.full((2 * phase.numel() + 4,), SENTINEL, dtype=torch.float32, device=DEV)

    def model(**kw):
        a = dict(mag=tiles.data_ptr(), chan_stride=one, seg=SEG, rows=rows, mask=mask.data_ptr(), phase=phase.data_ptr(),
                 scale=scale.data_ptr(), channels=2, frames=T, v_prev=None, v_prev_stride=one, R_prev=None, eps=wn.EPS, reg=wn.REG,
                 v=v.data_ptr(), v_stride=one, R=R.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws_bytes)
        a.update(kw)
        return L().svs_wiener_model(*a.values(), S())

    def stems(**kw):
        a = dict(mag=tiles.data_ptr(), chan_stride=one, seg=SEG, rows=rows, phase=phase.data_ptr(), scale=scale.data_ptr(), channels=2,
                 frames=T, v=v0.data_ptr(), v_stride=one, R=R0.data_ptr(), reg=wn.REG, stem=2, out_mag=om.data_ptr(), out_chan_stride=one,
                 out_mag_stem_stride=2 * one, out_phase=op.data_ptr(), out_phase_stem_stride=phase.numel())
        a.update(kw)
        return L().svs_wiener_stems(*a.values(), S())

    INVALID = -1                                                                     # SVS_ERR_INVALID
    rules = [
        (model, dict(channels=3), "channels must be 1 or 2"),
        (model, dict(channels=0), "channels must be 1 or 2"),
        (model, dict(rows=96), "rows must be a positive multiple of 64"),
        (model, dict(rows=0), "rows must be a positive multiple of 64"),
        (model, dict(seg=30), "seg must be a positive multiple of 4"),
        (model, dict(seg=0), "seg must be a positive multiple of 4"),
        (model, dict(frames=0), "frames must be at least 1"),
        (model, dict(chan_stride=one - 4), "chan_stride must be at least one channel's size"),
        (model, dict(chan_stride=one + 2), "chan_stride must be a multiple of 4 floats"),
        (model, dict(v_stride=one - 4), "v_stem_stride must be at least one stem's size"),
        (model, dict(v_prev=v0.data_ptr(), R_prev=R0.data_ptr(), v_prev_stride=one - 4), "v_prev_stem_stride must be at least one stem's size"),
        (model, dict(v_prev=v0.data_ptr()), "v_prev and R_prev are given together"),
        (model, dict(mask=None), "the first update needs the mask"),
        (model, dict(mag=None), "null pointer"),
        (model, dict(phase=None), "null pointer"),
        (model, dict(scale=None), "null pointer"),
        (model, dict(R=None), "null pointer"),
        (model, dict(ws=None), "null pointer"),
        (model, dict(mag=tiles.data_ptr() + 4), "must be 16-byte aligned"),
        (model, dict(mask=mask.data_ptr() + 8), "must be 16-byte aligned"),
        (model, dict(v=v.data_ptr() + 4), "must be 16-byte aligned"),
        (model, dict(phase=phase.data_ptr() + 4), "must be 8-byte aligned"),
        (model, dict(R=R.data_ptr() + 4), "must be 8-byte aligned"),
        (model, dict(chan_stride=1 << 29), "must stay below 2 GiB"),
        (model, dict(v_stride=1 << 29), "must stay below 2 GiB"),
        (model, dict(frames=600000, chan_stride=153600000, v_stride=153600000), "the phasors must stay below 2 GiB"),  # 18750 tiles: 1.2 GB of tiles, 2.5 GB of phasors
        (model, dict(reg=0.0), "reg must be positive"),
        (model, dict(eps=-1.0), "eps must not be negative"),
        (model, dict(ws_bytes=ws_bytes - 8), "the workspace needs"),
        (stems, dict(channels=3), "channels must be 1 or 2"),
        (stems, dict(rows=96), "rows must be a positive multiple of 64"),
        (stems, dict(seg=30), "seg must be a positive multiple of 4"),
        (stems, dict(frames=0), "frames must be at least 1"),
        (stems, dict(stem=3), "stem must be 0"),
        (stems, dict(chan_stride=one - 4), "chan_stride must be at least one channel's size"),
        (stems, dict(v_stride=one - 4), "v_stem_stride must be at least one stem's size"),
        (stems, dict(out_chan_stride=one - 4), "out_chan_stride must be at least one channel's size"),
        (stems, dict(out_mag_stem_stride=2 * one - 4), "out_mag_stem_stride must be at least one stem's size"),
        (stems, dict(out_phase_stem_stride=phase.numel() - 2), "out_phase_stem_stride must be at least one stem's size"),
        (stems, dict(out_phase_stem_stride=phase.numel() + 1), "out_phase_stem_stride must be even"),
        (stems, dict(out_mag_stem_stride=1 << 29), "must stay below 2 GiB"),
        (stems, dict(out_phase_stem_stride=1 << 29), "must stay below 2 GiB"),
        (stems, dict(v=None), "null pointer"),
        (stems, dict(out_mag=None), "null pointer"),
        (stems, dict(out_phase=None), "null pointer"),
        (stems, dict(out_mag=om.data_ptr() + 4), "must be 16-byte aligned"),
        (stems, dict(v=v0.data_ptr() + 8), "must be 16-byte aligned"),
        (stems, dict(out_phase=op.data_ptr() + 4), "must be 8-byte aligned"),
        (stems, dict(reg=-1.0), "reg must be positive"),
    ]
    for fn, kw, message in rules:
        rc = fn(**kw)
        text = L().svs_last_error_string().decode()
        assert rc == INVALID and message in text, (fn.__name__, kw, rc, text)
    assert int(L().svs_wiener_workspace_bytes(3, rows, SEG, T)) == 0
    torch.cuda.synchronize()
    for buf in (v, om, op):                                                          # none of the rejected calls launched anything
        assert torch.all(buf == SENTINEL)
    assert torch.all(R == SENTINEL)
    with pytest.raises(ValueError, match="at least 1"):
        wn.wiener_filter(tiles, mask, k["phase"], k["norm"], T, 0)
    with pytest.raises(ValueError, match="stems"):
        wn.wiener_stems(tiles, k["phase"], scale, T, k["models"][0], stems=(1, 0))
    # and the same buffers take a valid call of each kind
    assert model() == 0 and stems() == 0
    torch.cuda.synchronize()
    assert torch.equal(v[:2 * one].view(v0.shape), v0) and torch.equal(R[:2 * rows * 4].view(R0.shape), R0)


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


def by_hand(tile_hop, iters, stems, y=None):
    """separate_waveform(peak=None, wiener_iters=iters) through the public pieces -> (len(stems), C, hop * 130), and the inverse of
    the mixture on the common scale."""
    model, y = random_model(), stereo() if y is None else y
    C = y.shape[0]
    tiles, phase, norm, frames = svs_data.stft_to_tiles(y, N_FFT, HOP, INPUT_LEN)
    assert frames == 131 and tiles.shape == (C, 2, 1, N_FFT // 2, INPUT_LEN)
    for c in range(C):
        _lib.check(L().svs_scale_by_inv(tiles[c].data_ptr(), tiles[c].numel(), norm[c:].data_ptr(), 1.0, S()), "svs_scale_by_inv")
    flat = tiles.view(2 * C, 1, N_FFT // 2, INPUT_LEN) if tile_hop == INPUT_LEN else ov.overlap_tiles(tiles, tile_hop)
    mask = torch.empty_like(flat)
    with torch.no_grad():
        mask[:] = model(flat)
    mask = mask.view(tiles.shape) if tile_hop == INPUT_LEN else ov.blend_masks(mask, 2, tile_hop)
    smag, sphase = wn.wiener_filter(tiles, mask, phase, norm, frames, iters, stems=stems)
    out = torch.stack([svs_data.istft_from_tiles(smag[s], None, sphase[s], frames, n_fft=N_FFT, hop=HOP) for s in range(len(stems))])
    mix = svs_data.istft_from_tiles(tiles, None, phase, frames, n_fft=N_FFT, hop=HOP) * wn.common_scale(norm)[:, None]
    return out, mix


def test_wiener_iters_zero_is_the_default_path():
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    for kw in ({}, {"vocal_solo": False}, {"both_stems": True}, {"both_stems": True, "tile_hop": 64}, {"sr_out": 44100}):
        a = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, **kw)
        assert torch.equal(separate_waveform(model, y, n_fft=N_FFT, hop=HOP, wiener_iters=0, **kw), a), kw


@pytest.mark.parametrize("tile_hop", [INPUT_LEN, 64])
def test_wiener_iters_is_its_composition(tile_hop):
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    want, _ = by_hand(tile_hop, 2, (0, 1))
    got = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=None, both_stems=True, tile_hop=tile_hop, wiener_iters=2)
    assert got.shape == (2, 2, HOP * 130) and torch.equal(got, want)
    plain = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=None, both_stems=True, tile_hop=tile_hop)
    assert not torch.equal(got, plain)                           # the option does something
    assert model.eval_precision == "fp32" and not model.training
    if tile_hop == INPUT_LEN:
        for solo in (True, False):                               # one stem, and the inverted one
            one = separate_waveform(model, y, vocal_solo=solo, n_fft=N_FFT, hop=HOP, peak=None, wiener_iters=2)
            assert one.shape == (2, HOP * 130) and torch.equal(one, by_hand(tile_hop, 2, (0,) if solo else (1,))[0][0])
            assert torch.equal(one, want[0 if solo else 1])


def test_mono_and_peak():
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    got = separate_waveform(model, y[0], n_fft=N_FFT, hop=HOP, wiener_iters=2)
    assert got.shape == (HOP * 130,) and abs(got.abs().max().item() - 0.9) <= 1e-5
    want, _ = by_hand(INPUT_LEN, 2, (0,), y=y[:1].contiguous())
    raw = separate_waveform(model, y[0], n_fft=N_FFT, hop=HOP, peak=None, wiener_iters=2)
    assert torch.equal(raw, want[0, 0])


def test_both_stems_at_the_output_rate():
    """sr_out = 44100: the filtered stems are resampled, and `peak` is applied per stem and channel at THAT rate, as it is today."""
    from svs_unet_pytorch_amd.resample import resample_poly_gpu
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    want = resample_poly_gpu(by_hand(INPUT_LEN, 2, (0, 1))[0].view(4, HOP * 130), 44100, SAMPLE_RATE)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
    pk = torch.empty(4, dtype=torch.float32, device=DEV)
    for c in range(4):
        _lib.check(L().svs_absmax(want[c].data_ptr(), want.shape[1], pk[c:].data_ptr(), ws.data_ptr(), ws.numel(), S()), "svs_absmax")
        _lib.check(L().svs_scale_by_inv(want[c].data_ptr(), want.shape[1], pk[c:].data_ptr(), 0.9, S()), "svs_scale_by_inv")
    got = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=0.9, sr_out=44100, both_stems=True, wiener_iters=2)
    assert got.shape == (2, 2, want.shape[1]) and torch.equal(got.view(4, -1), want)


def test_stems_add_up_to_the_mixture(report):
    """At the network rate and before any peak normalisation the two stems add up to the inverse transform of the mixture (on the
    common scale) but for reg * Cxx^-1 x and float32 rounding.  Bound: in a bin the model explains, the loss is reg |x| / (|x|^2 +
    reg) <= sqrt(reg) / 2 of the peak, so sqrt(reg) = 3.2e-4 bounds the relative l2 loss of a signal whose every bin were the
    worst one.  Measured on an MI355X: 7.1e-6 (l2) and 1.9e-5 of the peak after one update, 6.9e-6 and 1.9e-5 after two."""
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), stereo()
    for iters in (1, 2):
        got = separate_waveform(model, y, n_fft=N_FFT, hop=HOP, peak=None, both_stems=True, wiener_iters=iters).double()
        _, mix = by_hand(INPUT_LEN, iters, (0, 1))
        mix = mix.double()
        e2 = ((got[0] + got[1] - mix).norm() / mix.norm()).item()
        e_peak = ((got[0] + got[1] - mix).abs().max() / mix.abs().max()).item()
        print(f"wiener_iters={iters}: stems + ... vs the mixture's inverse, relative l2 {e2:.3e}, of the peak {e_peak:.3e}")
        assert report(f"wiener_iters={iters} vocal + accompaniment vs mixture, relative l2", e2, wn.REG ** 0.5)
        assert report(f"wiener_iters={iters} vocal + accompaniment vs mixture, of the peak", e_peak, wn.REG ** 0.5)


def test_separate_to_wav_writes_both_files(tmp_path):
    from scipy.io import wavfile

    from svs_unet_pytorch_amd.streaming import separate_to_wav
    n = 90000                                                     # ~2 s of 44.1 kHz stereo: 131 frames at 512 / 128, two tiles
    mix = np.stack([synth.audio(n, 50), 0.5 * synth.audio(n, 51)], axis=1)
    src, voc, acc = (str(tmp_path / f) for f in ("mixture.wav", "vocal.wav", "accomp.wav"))
    wavfile.write(src, 44100, np.clip(np.round(mix * 20000), -32768, 32767).astype(np.int16))
    shape = separate_to_wav(random_model(), src, voc, n_fft=N_FFT, hop=HOP, subtype="FLOAT", dst_accomp_path=acc, wiener_iters=1)
    assert tuple(shape) == (n, 2)
    files = []
    for path in (voc, acc):
        assert os.path.exists(path)
        rate, pcm = wavfile.read(path)
        assert rate == 44100 and pcm.dtype == np.float32 and pcm.shape == (n, 2) and np.isfinite(pcm).all()
        files.append(pcm)
    separate_to_wav(random_model(), src, voc, n_fft=N_FFT, hop=HOP, subtype="FLOAT", dst_accomp_path=acc)
    assert not np.array_equal(wavfile.read(voc)[1], files[0])    # the option reaches the files


def test_separate_cli_writes_two_stereo_files(tmp_path):
    """python -m svs_unet_pytorch_amd.separate ... --wiener_iters 1 --tar_accomp ...: two stereo files of the source's rate and frame
    count (what evaluate.py takes beside the stems), equal to separate_to_wav's, and different from the files without the flag."""
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import separate
    from svs_unet_pytorch_amd.streaming import separate_to_wav
    ck = str(tmp_path / "svs_random.pth")
    torch.save({"model_state_dict": random_model().state_dict()}, ck)
    n = 66150                                                    # 1.5 s at 44,100 Hz
    mix = np.stack([synth.audio(n, 40), 0.5 * synth.audio(n, 41)], axis=1)
    src, voc, acc = (str(tmp_path / f) for f in ("mixture.wav", "vocal.wav", "accomp.wav"))
    wavfile.write(src, 44100, np.clip(np.round(mix * 20000), -32768, 32767).astype(np.int16))
    separate.main(["--model_path", ck, "--src", src, "--tar", voc, "--tar_accomp", acc, "--wiener_iters", "1", "--subtype", "FLOAT"])
    got = [wavfile.read(p) for p in (voc, acc)]
    for rate, pcm in got:
        assert rate == 44100 and pcm.dtype == np.float32 and pcm.shape == (n, 2) and np.isfinite(pcm).all()
        assert abs(np.abs(pcm).max() - 0.9) <= 1e-5              # one gain per file: the louder channel peaks at 0.9
    v2, a2 = str(tmp_path / "v2.wav"), str(tmp_path / "a2.wav")
    separate_to_wav(random_model(), src, v2, subtype="FLOAT", dst_accomp_path=a2, wiener_iters=1)
    assert np.array_equal(wavfile.read(v2)[1], got[0][1]) and np.array_equal(wavfile.read(a2)[1], got[1][1])
    separate.main(["--model_path", ck, "--src", src, "--tar", v2, "--tar_accomp", a2, "--subtype", "FLOAT"])
    assert not np.array_equal(wavfile.read(v2)[1], got[0][1])
