"""24-bit PCM and TPDF dither on the device (csrc/pcm.hip), every comparison bitwise: svs_pcm24_widen against pcm.unpack24 and against
scipy's reading of the same file; svs_pcm_encode_dither against pcm.encode_dither_reference over channel counts, frame counts around
the four-frame group, both word lengths, the three dithers, both load paths and both store paths, against svs_resample_encode for the
undithered int16 rule, and in pieces against the whole (first_frame); the plumbing through resample.py; and separate.py end to end."""
import functools
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from svs_unet_pytorch_amd import _lib, pcm, synth
from svs_unet_pytorch_amd import resample as rs

pytestmark = pytest.mark.gpu
DEV = "cuda"
EDGE = np.array([0, 1, -1, 0x7FFFFF, -0x800000], dtype=np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the way in ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 4099, 3 * 2 ** 16 + 1])
def test_widen_matches_unpack24(n):
    vals = np.random.default_rng(n).integers(-0x800000, 0x800000, n).astype(np.int32)
    vals[:min(n, 5)] = EDGE[:min(n, 5)]
    vals[-1] = -0x800000 if n > 1 else 0x7FFFFF
    packed = pcm.pack24(vals)
    got = pcm.widen24_gpu(dev(packed.reshape(-1)))
    assert got.dtype == torch.int32 and got.shape == (n,)
    assert np.array_equal(got.cpu().numpy(), pcm.unpack24(packed)) and np.array_equal(got.cpu().numpy(), vals * 256)
    assert pcm.widen24_gpu(dev(packed)).shape == (n,)                              # a last axis of 3 is one sample


def test_read_pcm_device_is_scipys_int32_and_resamples_the_same(tmp_path):
    vals = np.random.default_rng(7).integers(-0x800000, 0x800000, (4099, 2)).astype(np.int32)
    vals[:5, 0], vals[-5:, 1] = EDGE, EDGE
    path = str(tmp_path / "s24.wav")
    pcm.write_wav24(path, 44100, pcm.pack24(vals))
    rate, host = wavfile.read(path)
    r2, wide, channels = pcm.read_pcm_device(path, DEV)
    assert (r2, channels) == (rate, 2) == (44100, 2) and wide.dtype == torch.int32 and wide.shape == (4099, 2)
    assert np.array_equal(wide.cpu().numpy(), host)
    a = rs.resample_poly_gpu(wide, 2048, 11025, channels=2, downmix=False)
    b = rs.resample_poly_gpu(dev(host), 2048, 11025, channels=2, downmix=False)
    assert torch.equal(a, b)
    mono = str(tmp_path / "m24.wav")
    pcm.write_wav24(mono, 8192, pcm.pack24(vals[:, 0]))
    assert np.array_equal(pcm.read_pcm_device(mono, DEV)[1].cpu().numpy(), wavfile.read(mono)[1])
    other = str(tmp_path / "s16.wav")                                              # everything else: data.read_pcm, unchanged
    wavfile.write(other, 22050, (vals >> 8).astype(np.int16))
    r3, t16, c3 = pcm.read_pcm_device(other, DEV)
    assert (r3, c3) == (22050, 2) and t16.dtype == torch.int16 and np.array_equal(t16.cpu().numpy(), (vals >> 8).astype(np.int16))


# ---- the way out --------------------------------------------------------------------------------------------------------------

def rows(channels, frames, pad, seed=3):
    """(channels, frames + pad) float32 rows; from 7 frames on with NaN, +-inf and +-1.0 planted in the first and the last channel
    (the gains below push +-1.0 past full scale in the last)."""
    x = (0.6 * np.random.default_rng(seed + 16 * channels + frames).standard_normal((channels, frames + pad))).astype(np.float32)
    if frames >= 7:
        x[0, :7] = [np.nan, np.inf, -np.inf, 1.0, -1.0, 0.0, -0.0]
        x[-1, frames - 7:frames] = [1.0, -1.0, np.inf, np.nan, -np.inf, 1.0, -1.0]
    return x


def as_written(ref, bits):
    """encode_dither_reference's integers (frames, channels) in the form the device writes."""
    return ref if bits == 16 else pcm.pack24(ref).reshape(ref.shape[0], -1)


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 8])
def test_encode_matches_the_reference(channels):
    gain = np.linspace(0.5, 1.5, channels).astype(np.float32)                      # the last channel: 1.5 (1 channel: 0.5)
    gain[-1] = 1.5
    g_dev = dev(gain)
    checked = 0
    for frames in (1, 3, 4, 7, 4099):
        for pad in (0, 5):                                                         # pad 5: ld_in % 4 != 0, the scalar loads
            x = rows(channels, frames, pad)
            buf = dev(x)
            for bits in (16, 24):
                for kind in ("none", "tpdf", "hp"):
                    for g, gd in ((None, None), (gain, g_dev)):
                        for seed in (0, 12345):
                            got = pcm.encode_dither_gpu(buf, frames, gd, bits, kind, seed)
                            want = as_written(pcm.encode_dither_reference(x[:, :frames].T, g, bits, kind, seed), bits)
                            assert got.shape == want.shape and got.dtype == (torch.int16 if bits == 16 else torch.uint8)
                            assert np.array_equal(got.cpu().numpy(), want), (channels, frames, pad, bits, kind, g is not None, seed)
                            checked += 1
    assert checked == 5 * 2 * 2 * 3 * 2 * 2


@pytest.mark.parametrize("bits", [16, 24])
def test_encode_unaligned_rows_and_output(bits):
    """Rows that start 4 bytes past a 16-byte boundary (scalar loads although ld_in % 4 == 0) and an output that is 4- but not
    16-byte aligned (dword stores): the same bytes."""
    channels, frames = 2, 4099
    x = rows(channels, frames, 5)                                                  # width 4104
    big = dev(x)
    view = big[:, 1:]                                                              # (2, 4103), stride 4104, data_ptr + 4
    assert view.data_ptr() % 16 == 4 and view.stride(0) % 4 == 0
    want = as_written(pcm.encode_dither_reference(x[:, 1:1 + frames].T, None, bits, "tpdf", 3), bits)
    assert np.array_equal(pcm.encode_dither_gpu(view, frames, None, bits, "tpdf", 3).cpu().numpy(), want)
    per = 2 if bits == 16 else 1                                                   # bytes per element of the output tensor
    flat = torch.zeros(want.size + 16, dtype=torch.int16 if bits == 16 else torch.uint8, device=DEV)
    out = flat[4 // per:4 // per + want.size].view(want.shape)
    assert out.data_ptr() % 16 == 4
    pcm.encode_dither_gpu(big, frames, None, bits, "tpdf", 3, out=out)
    want0 = as_written(pcm.encode_dither_reference(x[:, :frames].T, None, bits, "tpdf", 3), bits)
    assert np.array_equal(out.cpu().numpy(), want0)
    assert not flat[:4 // per].any() and not flat[4 // per + want.size:].any()     # nothing outside the frames is written


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
def test_undithered_int16_is_svs_resample_encode(channels):
    frames = 4099
    x = rows(channels, frames, 0)
    j = np.arange(-500, 500)
    x[0, 100:1100] = ((2 * j + 1) / 65534).astype(np.float32)                      # exact ties of the int16 rule
    buf, L = dev(x), _lib.lib()
    one, _ = rs.tap_table(1, 1, buf.device)
    for gain in (None, dev(np.linspace(0.7, 1.4, channels).astype(np.float32))):
        old = torch.empty((frames, channels), dtype=torch.int16, device=DEV)
        _lib.check(L.svs_resample_encode(buf.data_ptr(), channels, frames, frames, one.data_ptr(), 1, 1, 1, _lib.ptr(gain), rs.PCM_I16,
                                         old.data_ptr(), _lib.stream_ptr()), "svs_resample_encode")
        assert torch.equal(pcm.encode_dither_gpu(buf, frames, gain, 16, "none", 0), old)


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("kind", ["none", "tpdf", "hp"])
def test_first_frame_pieces_concatenate_to_the_whole(bits, kind):
    channels, frames = 3, 4099
    buf = dev(rows(channels, frames, 0))
    gain = dev(np.array([0.5, 1.0, 1.5], dtype=np.float32))
    whole = pcm.encode_dither_gpu(buf, frames, gain, bits, kind, 12345)
    assert torch.equal(pcm.encode_dither_gpu(buf, frames, gain, bits, kind, 12345), whole)        # the same call, the same bytes
    head = pcm.encode_dither_gpu(buf[:, :1000].contiguous(), 1000, gain, bits, kind, 12345)
    tail = pcm.encode_dither_gpu(buf[:, 1000:].contiguous(), frames - 1000, gain, bits, kind, 12345, first_frame=1000)
    assert torch.equal(torch.cat([head, tail]), whole)
    if kind != "none":
        assert not torch.equal(pcm.encode_dither_gpu(buf[:, 1000:].contiguous(), frames - 1000, gain, bits, kind, 12345), whole[1000:])


# ---- the plumbing -------------------------------------------------------------------------------------------------------------

def stems(n=3001):
    return dev(np.stack([0.8 * synth.audio(n, 60), 0.4 * synth.audio(n, 61)]))


@pytest.mark.parametrize("fmt", ["int16", "int32", "float32"])
def test_default_keywords_change_nothing(fmt):
    y = stems()
    assert torch.equal(rs.resample_encode_gpu(y, 5, 4, fmt=fmt, subtype_bits=None, dither="none"), rs.resample_encode_gpu(y, 5, 4, fmt=fmt))
    buf = torch.stack([y, 0.5 * y]).contiguous()
    a, ga, _ = rs.encode_planar_gpu(buf, 2999, *rs.pcm_format(fmt))
    b, gb, _ = rs.encode_planar_gpu(buf, 2999, *rs.pcm_format(fmt), subtype_bits=None, dither="none", dither_seed=5)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and all(torch.equal(p, q) for p, q in zip(ga, gb))


def test_24_bits_and_dither_through_the_peak_rule():
    y = stems()
    v = rs.resample_encode_gpu(y, 5, 4, fmt="float32").cpu().numpy()                # the fused path's samples after the gain
    assert abs(float(np.abs(v).max()) - 0.9) <= 1e-6
    out = rs.resample_encode_gpu(y, 5, 4, subtype_bits=24)
    assert out.dtype == torch.uint8 and out.shape == (v.shape[0], 6)
    want = np.clip(np.rint(v.astype(np.float64) * 8388607.0), -8388608.0, 8388607.0).astype(np.int32)
    assert np.array_equal(pcm.unpack24(out.cpu().numpy()), want * 256)
    d16 = rs.resample_encode_gpu(y, 5, 4, fmt="int16", dither="hp", dither_seed=9)
    assert np.array_equal(d16.cpu().numpy(), pcm.encode_dither_reference(v, None, 16, "hp", 9))
    # two stems through encode_planar_gpu: stem k is dithered with seed + k
    buf = torch.stack([y, 0.5 * y.flip(0)]).contiguous()
    f, _, _ = rs.encode_planar_gpu(buf, 3001, *rs.pcm_format("float32"))
    e, _, _ = rs.encode_planar_gpu(buf, 3001, *rs.pcm_format("float32"), subtype_bits=24, dither="tpdf", dither_seed=7)
    for k in range(2):
        want = pcm.pack24(pcm.encode_dither_reference(f[k].cpu().numpy(), None, 24, "tpdf", 7 + k)).reshape(3001, 6)
        assert np.array_equal(e[k].cpu().numpy(), want)
    for bad in (dict(fmt="int32", dither="tpdf"), dict(fmt="float32", dither="hp"), dict(subtype_bits=24, peak=None), dict(subtype_bits=20)):
        with pytest.raises(ValueError):
            rs.resample_encode_gpu(y, 5, 4, **bad)


def test_save_wav_device_writes_24_bit_files(tmp_path):
    """data.save_wav_device (behind data.py to_wave): a mono signal, 8,000 -> 10,000 Hz, by the peak rule and by a loudness target."""
    from svs_unet_pytorch_amd import data
    y = stems(12001)[0]                                                            # 1.5 s: whole loudness blocks
    f, p = str(tmp_path / "f.wav"), str(tmp_path / "p.wav")
    for kw in ({}, {"loudness": -20.0}):
        data.save_wav_device(f, y, 8000, 10000, "FLOAT", **kw)
        data.save_wav_device(p, y, 8000, 10000, "PCM_24", dither="hp", dither_seed=3, **kw)
        (rf, v), (rp, got) = wavfile.read(f), wavfile.read(p)
        assert rf == rp == 10000 and v.dtype == np.float32 and got.dtype == np.int32 and got.shape == v.shape == (15002,)
        assert pcm.subtype_of(p) == "PCM_24"
        assert np.array_equal(got, pcm.encode_dither_reference(v, None, 24, "hp", 3) * 256)
    with pytest.raises(ValueError, match="dither"):
        data.save_wav_device(p, y, 8000, 10000, "FLOAT", dither="tpdf")


# ---- end to end ---------------------------------------------------------------------------------------------------------------

N_SRC, WIN = 66000, ["--win_size", "512", "--hop_size", "128"]      # 65,462 separated frames: the last 538 written frames are padding


@functools.lru_cache(maxsize=None)
def random_model():
    from svs_unet_pytorch_amd.model import UNet
    torch.manual_seed(1234)
    return UNet().to(DEV).eval()


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    """A checkpoint, 1.5 s of stereo noise at 44.1 kHz as a 24-bit file and as the 32-bit file of the same left-justified words, and a
    runner of separate.main that returns the two written paths."""
    from svs_unet_pytorch_amd import separate
    root = tmp_path_factory.mktemp("pcm24")
    ck = str(root / "svs_random.pth")
    torch.save({"model_state_dict": random_model().state_dict()}, ck)
    mix = np.stack([synth.audio(N_SRC, 40), 0.5 * synth.audio(N_SRC, 41)], axis=1)
    vals = np.clip(np.round(mix.astype(np.float64) * 5000000), -0x800000, 0x7FFFFF).astype(np.int32)
    src24, src32 = str(root / "src24.wav"), str(root / "src32.wav")
    pcm.write_wav24(src24, 44100, pcm.pack24(vals))
    wavfile.write(src32, 44100, vals * 256)

    def run(tag, src, *flags):
        v, a = str(root / f"{tag}_v.wav"), str(root / f"{tag}_a.wav")
        separate.main(["--model_path", ck, "--src", src, "--tar", v, "--tar_accomp", a, *WIN, *flags])
        return v, a
    return dict(run=run, src24=src24, src32=src32, cache={})


def float_run(e2e, *flags):
    """The FLOAT files of a configuration (vocal, accompaniment), separated once per module."""
    if flags not in e2e["cache"]:
        paths = e2e["run"]("float" + "".join(flags).replace("-", ""), e2e["src24"], "--subtype", "FLOAT", *flags)
        e2e["cache"][flags] = [wavfile.read(p)[1] for p in paths]
        assert all(f.dtype == np.float32 and f.shape == (N_SRC, 2) for f in e2e["cache"][flags])
    return e2e["cache"][flags]


def check_24(paths, floats):
    for path, f in zip(paths, floats):
        rate, got = wavfile.read(path)
        assert rate == 44100 and got.dtype == np.int32 and got.shape == (N_SRC, 2) and not (got & 0xFF).any()
        assert pcm.subtype_of(path) == "PCM_24" and os.path.getsize(path) == 44 + N_SRC * 6
        assert np.array_equal(got, pcm.encode_dither_reference(f, None, 24, "none", 0) * 256)


def test_separate_pcm24_is_the_float_run_quantised(e2e):
    floats = float_run(e2e)
    assert abs(float(np.abs(floats[0]).max()) - 0.9) <= 1e-6
    check_24(e2e["run"]("p24", e2e["src24"], "--subtype", "PCM_24"), floats)
    check_24(e2e["run"]("psrc", e2e["src24"], "--subtype", "source"), floats)        # the source is a 24-bit file


def test_separate_dither_seeds(e2e):
    floats = float_run(e2e)
    paths = e2e["run"]("tpdf", e2e["src24"], "--dither", "tpdf", "--dither_seed", "7")
    for k, (path, f) in enumerate(zip(paths, floats)):
        rate, got = wavfile.read(path)
        assert rate == 44100 and got.dtype == np.int16
        assert np.array_equal(got, pcm.encode_dither_reference(f, None, 16, "tpdf", 7 + k))
        assert not np.array_equal(got, pcm.encode_dither_reference(f, None, 16, "none", 0))
        assert not f[-100:].any() and got[-100:].any() and np.abs(got[-100:]).max() == 1   # the padded frames are dithered silence


def test_24_bit_source_is_the_32_bit_source(e2e):
    floats = float_run(e2e)
    for path, f in zip(e2e["run"]("from32", e2e["src32"], "--subtype", "FLOAT"), floats):
        assert np.array_equal(wavfile.read(path)[1].view(np.uint32), f.view(np.uint32))


@pytest.mark.parametrize("flags", [("--fullband", "mask"), ("--loudness", "-23")])
def test_separate_pcm24_through_both_planar_callers(e2e, flags):
    check_24(e2e["run"]("p24" + flags[0].strip("-"), e2e["src24"], "--subtype", "PCM_24", *flags), float_run(e2e, *flags))
