"""Full-band stems, the host half (no GPU): the two entry points are declared and bound and refuse bad arguments before any launch
(all device pointers are NULL, so a call that got as far as a launch would come back with another code and message); the float64
definition's own properties (fullband.fullband_reference): the sum identity, the accomp mode, the integer frame coordinate, the
zero-magnitude fallback; the refusals of a bad mode and of the Wiener filter before a file or a checkpoint is opened; and the order
of the three ways out by SNR against the true full-band sources on a pinned synthetic pair."""
from fractions import Fraction

import numpy as np
import pytest

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import fullband as fb
from svs_unet_pytorch_amd import resample as rs

NAMES = ("svs_fullband_gains", "svs_fullband_mix")
RATES = (44100, 48000, 22050, 16000)


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def err(lib):
    return lib.svs_last_error_string().decode()


def updown(rate):
    fr = Fraction(rate, 8192)
    return fr.numerator, fr.denominator


def test_symbols_are_declared_and_bound(lib):
    syms = _lib.header_symbols()
    for name in NAMES:
        assert name in syms and name in _lib._SIGS and hasattr(lib, name), name
    assert fb.TOP_DIV == 4 and fb.MODES == ("mask", "accomp")


# (channels, n_tiles, rows, seg, frames, stride) -> the rule's words; stride None = the minimum
GAIN_RULES = [
    ((0, 2, 256, 128, 200, None), "all sizes must be positive"),
    ((2, 0, 256, 128, 200, None), "all sizes must be positive"),
    ((2, 2, 0, 128, 200, None), "all sizes must be positive"),
    ((2, 2, 256, 0, 200, None), "all sizes must be positive"),
    ((2, 2, 256, 128, 0, None), "all sizes must be positive"),
    ((2, 2, 254, 128, 200, None), "rows must be a multiple of 4"),
    ((2, 2, 256, 128, 257, None), "do not end in the last"),
    ((2, 2, 256, 128, 128, None), "do not end in the last"),
    ((2, 2, 256, 128, 200, 2 * 256 * 128 - 1), "chan_stride must be at least"),
    ((2, 2, 256, 128, 200, None), "null pointer"),
]


@pytest.mark.parametrize("geom,msg", GAIN_RULES)
def test_gains_refuses_before_any_launch(lib, geom, msg):
    C, n_tiles, rows, seg, frames, stride = geom
    stride = n_tiles * rows * seg if stride is None else stride
    assert lib.svs_fullband_gains(None, None, stride, C, n_tiles, rows, seg, frames, None, None) < 0
    assert msg in err(lib) and err(lib).startswith("svs_fullband_gains:")


def mix_args(**kw):
    a = dict(stems=None, nstems=2, ld_stem=2 * 768, ld_in=768, y=None, ld_y=768, channels=2, n_in=768, pcm=None, fmt=1, n_pcm=4000,
             table=None, ntaps=20 * 11025 + 1, up=11025, down=2048, norm=None, gf=None, frames=2, hop=768, invert=0, out=None, ld_out=4135,
             ld_out_stem=2 * 4135, stream=None)
    a.update(kw)
    return list(a.values())


MIX_RULES = [
    (dict(nstems=0), "nstems"), (dict(nstems=3), "nstems"), (dict(channels=0), "channels"), (dict(channels=9), "channels"),
    (dict(invert=1), "invert"), (dict(fmt=3), "pcm_fmt"), (dict(ntaps=20 * 11025), "bad filter"), (dict(up=0), "bad filter"),
    (dict(frames=0), "frames"), (dict(hop=0), "hop"), (dict(n_in=0), "n_in"), (dict(n_pcm=-1), "n_pcm"), (dict(ld_in=767), "ld_in"),
    (dict(ld_y=700), "ld_y"), (dict(ld_stem=768), "ld_stem"), (dict(ld_out=4134), "ld_out"), (dict(ld_out_stem=4135), "ld_out_stem"),
    (dict(), "null pointer"), (dict(nstems=1, invert=1), "null pointer"),
]


@pytest.mark.parametrize("kw,msg", MIX_RULES)
def test_mix_refuses_before_any_launch(lib, kw, msg):
    assert rs.out_len(768, 11025, 2048) == 4135
    assert lib.svs_fullband_mix(*mix_args(**kw)) < 0
    assert msg in err(lib) and err(lib).startswith("svs_fullband_mix:")


# ---- the float64 definition ------------------------------------------------------------------------------------------------

def random_case(rate, frames=5, hop=96, C=2, seed=0, rows=256, seg=128):
    rng = np.random.default_rng(seed)
    up, down = updown(rate)
    n_in = hop * (frames - 1)
    n_out = rs.out_len(n_in, up, down)
    stems = rng.standard_normal((2, C, n_in))
    y = rng.standard_normal((C, n_in + 13))
    x = rng.standard_normal((C, n_out + 5))
    norm = rng.uniform(0.5, 3.0, C)
    gf = rng.random((C, frames))
    return stems, y, x, norm, gf, frames, hop, up, down


@pytest.mark.parametrize("rate", RATES)
def test_the_two_stems_add_up_to_the_file(rate):
    """out_vocal + out_accomp = x - U(y - norm * (v_vocal + v_accomp)), to 1e-12 of the peak, in both modes."""
    stems, y, x, norm, gf, frames, hop, up, down = random_case(rate)
    n_in = stems.shape[2]
    n_out = rs.out_len(n_in, up, down)
    want = x[:, :n_out] - rs.resample_reference(y[:, :n_in] - norm[:, None] * (stems[0] + stems[1]), up, down)
    for g in (gf, None):
        out = fb.fullband_reference(stems, y, x, norm, g, frames, hop, up, down)
        assert out.shape == (2, 2, n_out)
        d = np.abs(out[0] + out[1] - want).max() / np.abs(want).max()
        print(f"identity at {rate} Hz, {'mask' if g is not None else 'accomp'}: {d:.2e} of the peak")
        assert d <= 1e-12


def test_accomp_mode_leaves_the_vocal_band_limited():
    stems, y, x, norm, gf, frames, hop, up, down = random_case(44100, seed=1)
    out, parts = fb.fullband_reference(stems, y, x, norm, None, frames, hop, up, down, return_parts=True)
    assert np.array_equal(out[0], norm[:, None] * rs.resample_reference(stems[0], up, down))
    assert np.array_equal(out[1], norm[:, None] * parts["us"][1] + parts["hi"])
    assert not parts["g"].any() and np.array_equal(parts["gs"][1], np.ones_like(parts["g"]))
    # one stem: the vocal, or with invert the accompaniment -- the rows of the two-stem call
    assert np.array_equal(fb.fullband_reference(stems[:1], y, x, norm, gf, frames, hop, up, down)[0],
                          fb.fullband_reference(stems, y, x, norm, gf, frames, hop, up, down)[0])
    assert np.array_equal(fb.fullband_reference(stems[1:], y, x, norm, gf, frames, hop, up, down, invert=True)[0],
                          fb.fullband_reference(stems, y, x, norm, gf, frames, hop, up, down)[1])
    # a short file: x is zero past its end
    short = fb.fullband_reference(stems, y, x[:, :100], norm, gf, frames, hop, up, down, return_parts=True)[1]["x"]
    assert np.array_equal(short[:, :100], x[:, :100]) and not short[:, 100:].any()


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("hop,frames", [(768, 9), (96, 2), (768, 2561)])
def test_frame_coordinate_is_the_rational_exactly(rate, hop, frames):
    up, down = updown(rate)
    n_out = rs.out_len(hop * (frames - 1), up, down)
    # first and last output, the outputs around every frame centre of the first and the last frames, and the clamped tail
    centres = [Fraction(k * hop * up, down) for k in (0, 1, 2, frames - 2, frames - 1)]
    picks = {0, 1, n_out - 1, n_out - 2} | {int(c) + d for c in centres for d in (-1, 0, 1)}
    picks = sorted(n for n in picks if 0 <= n < n_out)
    vec = fb.frame_coordinate(np.array(picks, dtype=np.int64), up, down, hop)
    for j, n in enumerate(picks):
        k, rem, den = fb.frame_coordinate(n, up, down, hop)
        assert den == up * hop and 0 <= rem < den
        assert k + Fraction(rem, den) == Fraction(n * down, up * hop)
        assert (int(vec[0][j]), int(vec[1][j]), vec[2]) == (k, rem, den)
    assert fb.frame_coordinate(0, up, down, hop)[:2] == (0, 0)
    k_last = fb.frame_coordinate(n_out - 1, up, down, hop)[0]
    assert k_last in (frames - 2, frames - 1)                     # the last output lies in the last interval or past the last centre


def test_clamped_frames_take_the_last_gain():
    stems, y, x, norm, gf, frames, hop, up, down = random_case(16000, frames=2, hop=96, seed=3)
    g = fb.fullband_reference(stems, y, x, norm, gf, frames, hop, up, down, return_parts=True)[1]["g"]
    assert np.array_equal(g[:, 0], gf[:, 0])
    k, rem, den = fb.frame_coordinate(np.arange(g.shape[1], dtype=np.int64), up, down, hop)
    assert k.max() == 0                                           # n_in = hop: every output before the last frame's centre
    assert np.allclose(g, gf[:, :1] + (rem / den) * (gf[:, 1:] - gf[:, :1]), rtol=0, atol=1e-15)
    # T = 1 would clamp both ends to frame 0
    one = fb.fullband_reference(stems, y, x, norm, gf[:, :1], 1, hop, up, down, return_parts=True)[1]["g"]
    assert np.array_equal(one, np.broadcast_to(gf[:, :1], one.shape))


@pytest.mark.parametrize("rows", [256, 512])
def test_frame_gains_and_the_zero_magnitude_fallback(rows):
    rng = np.random.default_rng(rows)
    C, n_tiles, seg, frames = 2, 2, 128, 200
    tiles = rng.random((C, n_tiles, 1, rows, seg))
    mask = rng.random((C * n_tiles, 1, rows, seg))                # the network's layout of the same elements
    top = rows // fb.TOP_DIV
    tiles[1, 0, 0, rows - top:, 7] = 0.0                          # a frame whose top rows are silent
    tiles[0, 1, 0, :rows - top, 3] = 0.0                          # silence BELOW the top rows changes nothing
    gf, a, den, msum = fb.frame_gains_reference(tiles, mask, frames, return_abs=True)
    assert gf.shape == (C, frames) and den[1, 7] == 0 and a[1, 7] == 0
    m = mask.reshape(C, n_tiles, rows, seg)
    assert abs(gf[1, 7] - m[1, 0, rows - top:, 7].mean()) <= 1e-15      # the plain mean of the mask (another summation order)
    for c, t in ((0, 0), (0, 131), (1, 199), (0, 128 + 3)):
        mm, aa = m[c, t // seg, rows - top:, t % seg], tiles[c, t // seg, 0, rows - top:, t % seg]
        assert abs(gf[c, t] - (mm * aa).sum() / aa.sum()) <= 1e-15
    assert gf.min() >= 0 and gf.max() <= 1                        # a weighted mean of a mask in [0, 1]


# ---- refusals before a file or a checkpoint is opened ------------------------------------------------------------------------

def test_check_fullband_names_the_rule():
    assert fb.check_fullband(None) is None and fb.check_fullband(None, 3) is None
    for mode in fb.MODES:
        assert fb.check_fullband(mode) == mode
    for bad in ("average", "zeros", "", True, 1):
        with pytest.raises(ValueError, match="one of mask, accomp"):
            fb.check_fullband(bad)
    with pytest.raises(ValueError, match="wiener_iters 2"):
        fb.check_fullband("mask", 2)


def test_separate_to_wav_refuses_before_any_file_is_read(tmp_path):
    import inspect

    from svs_unet_pytorch_amd import streaming
    assert inspect.signature(streaming.separate_to_wav).parameters["fullband"].default is None
    assert inspect.signature(streaming.separate_waveform).parameters["aux"].default is None
    missing = str(tmp_path / "no_such.wav")
    with pytest.raises(ValueError, match="wiener_iters 1"):
        streaming.separate_to_wav(None, missing, str(tmp_path / "out.wav"), fullband="mask", wiener_iters=1)
    with pytest.raises(ValueError, match="one of mask, accomp"):
        streaming.separate_to_wav(None, missing, str(tmp_path / "out.wav"), fullband="average")
    assert not (tmp_path / "out.wav").exists()


@pytest.mark.parametrize("flags,msg", [(["--fullband", "mask", "--wiener_iters", "2"], "wiener_iters 2"),
                                       (["--fullband", "average"], "invalid choice")])
def test_cli_refuses_before_a_checkpoint_is_read(tmp_path, capsys, flags, msg):
    from svs_unet_pytorch_amd import separate
    with pytest.raises(SystemExit) as e:
        separate.main(["--model_path", str(tmp_path / "no_such_checkpoint.pth"), "--src", str(tmp_path / "in.wav"),
                       "--tar", str(tmp_path / "out.wav")] + flags)
    assert e.value.code == 2
    text = capsys.readouterr().err
    assert "--fullband" in text and msg in text
    assert not (tmp_path / "out.wav").exists()


def test_cli_help_names_the_modes(capsys):
    from svs_unet_pytorch_amd import separate
    with pytest.raises(SystemExit) as e:
        separate.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--fullband" in text and "mask" in text and "accomp" in text


# ---- quality: which way out is closest to the true full-band sources ---------------------------------------------------------

def snr(est, true):
    return 10 * np.log10((true ** 2).sum() / ((true - est) ** 2).sum())


def test_quality_ordering_on_a_pinned_pair():
    """44.1 kHz, 3 s.  Vocal: 49 harmonics of 220 Hz with 1/k amplitudes (up to 10,780 Hz), gated on and off at 1.7 Hz.  Accompaniment:
    smoothed noise plus a 110 Hz tone.  The mask is the ideal ratio mask at the network rate.  Against the true full-band sources
    the SNR must come out as  vocal: mask > band-limited;  accompaniment: mask > accomp > band-limited.  The order is asserted, not
    the figures (printed)."""
    from oracle import stft_oracle as so
    rate, n_fft, hop, seg = 44100, 1024, 768, 128
    n = 3 * rate
    t = np.arange(n) / rate
    gate = 0.5 * (1 + np.tanh(6 * np.sin(2 * np.pi * 1.7 * t)))
    voc = 0.2 * gate * sum(np.sin(2 * np.pi * 220 * k * t) / k for k in range(1, 50))
    noise = np.random.default_rng(2024).standard_normal(n + 3)
    acc = 0.15 * np.convolve(noise, np.ones(4) / 4, mode="valid") + 0.2 * np.sin(2 * np.pi * 110 * t)
    x = voc + acc
    up, down = updown(rate)
    y, yv, ya = (rs.resample_reference(s, down, up) for s in (x, voc, acc))
    Y, V, A = (so.stft(s, n_fft, hop).astype(np.complex128) for s in (y, yv, ya))
    frames = Y.shape[1]
    n_in = hop * (frames - 1)
    mask = np.abs(V) / (np.abs(V) + np.abs(A) + 1e-12)
    Y[0] = 0                                                     # the tile layout drops the DC bin
    stems = np.stack([so.istft(mask * Y, n_fft, hop), so.istft((1 - mask) * Y, n_fft, hop)])[:, None, :].astype(np.float64)
    assert stems.shape == (2, 1, n_in)
    rows = n_fft // 2
    tiles, mtiles = np.zeros((1, 1, 1, rows, seg)), np.zeros((1, 1, 1, rows, seg))
    tiles[0, 0, 0, :, :frames], mtiles[0, 0, 0, :, :frames] = np.abs(Y)[1:], mask[1:]
    gf = fb.frame_gains_reference(tiles, mtiles, frames)
    args = (stems, y[None], x[None], np.ones(1), gf, frames, hop, up, down)
    by_mask, parts = fb.fullband_reference(*args, return_parts=True)
    by_accomp = fb.fullband_reference(*args[:4], None, *args[5:])
    limited = parts["us"]
    n_out = by_mask.shape[2]
    true = np.stack([voc[:n_out], acc[:n_out]])
    res = {name: [snr(out[s, 0], true[s]) for s in (0, 1)] for name, out in (("mask", by_mask), ("accomp", by_accomp), ("limited", limited))}
    print("SNR (vocal, accompaniment) dB:", {k: [round(v, 2) for v in r] for k, r in res.items()})
    assert res["mask"][0] > res["limited"][0]
    assert res["accomp"][0] == res["limited"][0]
    assert res["mask"][1] > res["accomp"][1] > res["limited"][1]
