"""The look-ahead limiter on the device (-m gpu; csrc/limiter.hip) against the float64 definition of limiter.py: the envelope, the
gain curve, the apply stage, the way out under limiter_ms=, and the command line.  No case runs more than a few thousand samples per
row, except the way out at 44.1 kHz (1.5 s).

Bounds.  Envelope: tests/test_gpu_r128.py's true-peak bound, 14 * 2^-24 * S * max|x| with S = max_p sum_k |h[p + f k]|; factor 1:
equality.  Curve: g <= r exactly (r recomputed in numpy); |g - definition| <= (2h + 3) 2^-24, from 2h + 1 fmaf of terms in (0, 1] with
weights that sum to 1, plus the window's rounding; 1.0f exactly farther than 2h from all demand.  Apply: equality.  Way out: the
FLOAT samples within (2h + 8) 2^-24 of the ceiling, integers within 1 LSB."""
import math

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import limiter as lim
from svs_unet_pytorch_amd import loudness as ld
from svs_unet_pytorch_amd import pcm
from svs_unet_pytorch_amd import resample as rs

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24
TILE = 2048


def noise(shape, seed, scale=0.1):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def taps32(f):
    return ld.true_peak_taps(f).astype(np.float32)


def tap_sum(f):
    h = np.abs(taps32(f).astype(np.float64))
    return max(h[p::f][:12].sum() for p in range(1, f)) if f > 1 else 0.0


def strided(x, pad=13, off=1):
    """A device view of x's values whose rows are `pad` floats further apart than their length and start `off` floats past a 16-byte
    boundary."""
    rows, n = int(np.prod(x.shape[:-1])), x.shape[-1]
    base = torch.zeros(off + rows * (n + pad) + 3, dtype=torch.float32, device=DEV)
    view = base[off:off + rows * (n + pad)].view(*x.shape[:-1], n + pad)[..., :n]
    view.copy_(dev(x))
    assert view.data_ptr() % 16 == 4 * off and view.stride(-1) == 1
    return view


# ------------------------------------------------------------------------------------------------
# envelope
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [1, 2, 4])
@pytest.mark.parametrize("stems,channels", [(1, 1), (1, 2), (2, 2), (2, 3)])
def test_envelope(stems, channels, f, report):
    """Shorter than the halo, across a block's edge (a block is 2048 samples) and two blocks on; every row carries an impulse at one
    of its ends on top of noise."""
    for n in (1, 5, 2047, 2048, 2049, 4099):
        shape = (2, channels, n) if stems == 2 else (channels, n)
        x = noise(shape, seed=n + 7 * channels + f, scale=0.3)
        flat = x.reshape(-1, n)
        flat[0, 0], flat[-1, n - 1] = 1.0, -1.0
        want = lim.envelope_reference(x, f, taps32(f).astype(np.float64))
        bound = 14.0 * U24 * tap_sum(f) * float(np.abs(x).max())
        xd = dev(x)
        tp = ld.true_peaks_gpu(xd, 48000, stems, factor=f)[1]
        for name, view in (("contiguous", xd), ("rows 13 apart, 4 bytes off", strided(x))):
            e = lim.envelope_gpu(view, f, stems)
            assert e.shape == (n,) and e.dtype == torch.float32
            assert torch.equal(e, lim.envelope_gpu(view, f, stems))                      # the same bits again
            got = e.cpu().numpy()
            err = float(np.abs(got.astype(np.float64) - want).max())
            assert report(f"limiter envelope f={f} rows={stems}x{channels} n={n} {name}", err, bound)
            if f == 1:
                assert np.array_equal(got, np.abs(x).reshape(-1, n).max(axis=0))         # bit for bit
            assert float(e.max()) == float(tp.max())                                     # svs_true_peaks' largest, bit for bit


# ------------------------------------------------------------------------------------------------
# curve
# ------------------------------------------------------------------------------------------------
def spiky_envelope(n, h, seed):
    """Uniform noise up to 0.1 with spikes of 1.0 at 0, n - 1 and both sides of every tile edge, and a plateau longer than 2h + 1."""
    e = (0.1 * np.random.default_rng(seed).uniform(0.0, 1.0, n)).astype(np.float32)
    e[0] = e[n - 1] = 1.0
    for t in range(TILE, n, TILE):
        e[t - 1] = 1.0
        e[t] = 0.9
    a = n // 3
    e[a:min(n, a + 2 * h + 5)] = 0.7
    return e


def far_from_demand(r, h):
    over = np.flatnonzero(r < 1)
    i = np.arange(r.size)
    if over.size == 0:
        return np.ones(r.size, bool)
    pos = np.searchsorted(over, i)
    left = np.where(pos > 0, i - over[np.clip(pos - 1, 0, over.size - 1)], 1 << 30)
    right = np.where(pos < over.size, over[np.clip(pos, 0, over.size - 1)] - i, 1 << 30)
    return np.minimum(left, right) > 2 * h


@pytest.mark.parametrize("h", [1, 2, 63, 64, 88, 1024])
def test_curve(h, report):
    G, C = 3.0, 0.9
    bound = (2 * h + 3) * U24
    for n in (1, 2 * h, 2 * h + 1, 2047, 2049, 3 * TILE + 5):
        e = spiky_envelope(n, h, seed=h + n)
        ed = dev(e)
        g = lim.curve_gpu(ed, G, C, h)
        assert g.shape == (n,) and g.dtype == torch.float32
        assert torch.equal(g, lim.curve_gpu(ed, G, C, h))                                # the same bits again
        on_device = lim.curve_gpu(ed, torch.tensor([math.nan, 7.0, G, 0.0], dtype=torch.float64, device=DEV)[2:], C, h)
        assert torch.equal(g, on_device)                                                 # G as a device double
        got = g.cpu().numpy()
        want, r = lim.curve_reference(e, G, C, h)
        assert (r < 1).any() and (got <= r).all()                                        # r bounds g from above EXACTLY
        err = float(np.abs(got.astype(np.float64) - want).max())
        assert report(f"limiter curve h={h} n={n}", err, bound)
        far = far_from_demand(r, h)
        assert (got[far] == 1.0).all()
        print(f"curve h={h} n={n}: err {err:.3e} (bound {bound:.3e}), min g {got.min():.6f}, {int(far.sum())} samples far from all demand")
        # nothing over the ceiling, and the gains that switch the limiter off: exactly 1 everywhere
        quiet = dev(np.minimum(e, np.float32(0.1)))
        for case in (lim.curve_gpu(quiet, G, C, h), lim.curve_gpu(ed, math.inf, C, h), lim.curve_gpu(ed, 0.0, C, h),
                     lim.curve_gpu(ed, math.nan, C, h), lim.curve_gpu(ed, -2.0, C, h)):
            assert bool((case == 1.0).all())


# ------------------------------------------------------------------------------------------------
# apply
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 7, 4099])
def test_apply_is_one_multiply(n):
    x = noise((3, n), seed=n, scale=0.5)
    g = np.random.default_rng(n).uniform(0.2, 1.0, n).astype(np.float32)
    want = x * g[None, :]
    for view in (dev(x), strided(x)):
        assert torch.equal(lim.apply_gpu(view, dev(g)), dev(want)) and torch.equal(view, dev(want))        # in place, bit for bit
    one = dev(x[0])
    assert torch.equal(lim.apply_gpu(one, dev(g)), dev(want[0]))
    off = torch.zeros(n + 1, dtype=torch.float32, device=DEV)                            # g 4 bytes off a 16-byte boundary
    off[1:] = dev(g)
    assert torch.equal(lim.apply_gpu(dev(x), off[1:]), dev(want))


# ------------------------------------------------------------------------------------------------
# the way out
# ------------------------------------------------------------------------------------------------
TARGET, CEILING, MS = -14.0, 0.9, 2.0


def way_out_stems(fs, seconds=1.5):
    """Two stereo stems of noise at -30 dBFS RMS with one full-scale sample every 100 ms (alternating stem, channel and sign);
    tests/test_limiter_host.py shows on the CPU reference alone that the plain rule is ceiling-limited on it by more than 6 dB."""
    n = int(seconds * fs)
    x = noise((2, 2, n), seed=fs, scale=10.0 ** (-30.0 / 20.0))
    for k, i in enumerate(range(fs // 20, n, fs // 10)):
        x[k % 2, (k // 2) % 2, i] = 1.0 if k % 3 else -1.0
    return x


@pytest.fixture(scope="module")
def float64_pipeline():
    """(x, L, per true_peak: z, g, gain, the float32 samples that are written) of the definition followed by the float64 gain rule;
    computed once per rate."""
    out = {}
    for fs in (8192, 44100):
        x = way_out_stems(fs)
        h = lim.half_width(fs, MS)
        L = ld.loudness_reference(x, fs, stems=2)[0]
        G = 10.0 ** ((TARGET - L) / 20.0)
        plain = ld.gain_rule(L, float(np.abs(x).max()), TARGET, CEILING)
        assert plain[2] and 20.0 * math.log10(plain[1] / plain[0]) > 6.0                 # the plain rule is ceiling-limited by > 6 dB
        for tp in (False, True):
            f = ld.true_peak_factor(fs) if tp else 1
            t = taps32(f).astype(np.float64)
            z, g, r, e = lim.limiter_reference(x, G, lim.inner_ceiling(CEILING), h, factor=f, taps=t)   # what limit_rows_gpu aims at
            rows = z.reshape(4, -1).astype(np.float64)
            peak = float(ld.true_peak_reference(rows, taps=t, factor=f)[1].max()) if tp else float(np.abs(rows).max())
            gain = ld.gain_rule(L, peak, TARGET, CEILING)[0]
            out[fs, tp] = (x, L, h, z, g, gain, z * np.float32(gain))
    return out


@pytest.mark.parametrize("tp", [False, True])
@pytest.mark.parametrize("fs", [8192, 44100])
def test_way_out(fs, tp, float64_pipeline, report):
    x, L, h, z, g_want, gain_want, want = float64_pipeline[fs, tp]
    n = x.shape[-1]
    S = tap_sum(ld.true_peak_factor(fs))

    def run(fmt="FLOAT", **kw):
        buf = dev(x)
        outs, gains, info = rs.encode_planar_gpu(buf, n, *rs.pcm_format(fmt), loudness=TARGET, ceiling=CEILING, rate=fs, true_peak=tp, **kw)
        return [o.cpu().numpy() for o in outs], float(gains[0][0].item()), info.cpu().numpy(), buf

    extra = {}
    outs, gain, info, buf = run(limiter_ms=MS, limiter_out=extra)
    assert torch.equal(buf, dev(x) * extra["curve"])                                     # the caller's buffer is limited in place
    curve = extra["curve"].cpu().numpy().astype(np.float64)
    print(f"way out fs={fs} true_peak={tp}: h {h}, L {info[0]:.3f} (float64 {L:.3f}), gain {gain!r} (float64 {gain_want!r}), "
          f"unlimited {info[2]!r}, min g {curve.min():.4f} (float64 {g_want.min():.4f})")
    assert abs(info[0] - L) <= 1e-6 and abs(info[2] - 10.0 ** ((TARGET - L) / 20.0)) <= 1e-6 * info[2]
    err = max(float(np.abs(o.T.astype(np.float64) - w.astype(np.float64)).max()) for o, w in zip(outs, want))
    assert report(f"limiter way out FLOAT fs={fs} true_peak={tp}", err, (2 * h + 8) * U24 * CEILING)
    top = max(float(np.abs(o).max()) for o in outs)
    assert top <= CEILING                                                                # no written sample exceeds the ceiling
    assert top > 0.98 * CEILING or not info[3]
    if tp:
        rows = np.concatenate([o.T for o in outs]).astype(np.float64)
        written = float(ld.true_peak_reference(rows, fs)[1].max())
        assert report(f"limiter way out true peak fs={fs}", written, CEILING * (1.0 + 14.0 * U24 * S))
    # the two stems still add up: gain * g * (their sum), two float32 products per stem
    total = gain * curve * x.astype(np.float64).sum(axis=0)
    assert np.abs((outs[0].astype(np.float64) + outs[1]).T - total).max() <= 2.0 ** -22 * CEILING
    # integers: at most 1 LSB from the encoding of the float64 pipeline's samples
    i16 = run("PCM_16", limiter_ms=MS)[0]
    i24 = run("PCM_16", limiter_ms=MS, subtype_bits=24)[0]
    for k in range(2):
        w16 = rs.encode_pcm_reference(want[k].T, None, "int16")
        w24 = pcm.encode_dither_reference(want[k].T, None, 24, "none", 0)
        assert i16[k].dtype == np.int16 and np.abs(i16[k].astype(np.int64) - w16).max() <= 1
        got24 = (pcm.unpack24(i24[k].reshape(n, 2, 3)) >> 8).astype(np.int64)
        assert report(f"limiter way out 24-bit fs={fs} true_peak={tp} stem {k} (LSB)", float(np.abs(got24 - w24).max()), 1.0)
        assert np.abs(i16[k]).max() <= round(CEILING * 32767) and np.abs(got24).max() <= round(CEILING * (2 ** 23 - 1))
    # loudness of the written sum: nearer the target than without the limiter, and what the float64 pipeline gives
    plain, plain_gain, plain_info, untouched = run()
    assert torch.equal(untouched, dev(x)) and plain_info[3] == 1
    l_on = ld.loudness_reference(np.stack([o.T for o in outs]).astype(np.float64), fs, stems=2)[0]
    l_off = ld.loudness_reference(np.stack([o.T for o in plain]).astype(np.float64), fs, stems=2)[0]
    l_want = ld.loudness_reference(want.astype(np.float64), fs, stems=2)[0]
    l_limited = float(extra["limited_info"][0].item()) + 20.0 * math.log10(gain)
    print(f"    written {l_on:.3f} LUFS (float64 pipeline {l_want:.3f}, device meter {l_limited:.3f}); without the limiter {l_off:.3f}; target {TARGET}")
    assert abs(l_on - TARGET) < abs(l_off - TARGET) and gain > plain_gain
    assert report(f"limiter way out loudness fs={fs} true_peak={tp} (LU)", abs(l_on - l_want), 0.01)
    assert abs(l_limited - l_on) <= 1e-3
    # limiter_ms=None: the bytes of the call without the keyword
    none = run(limiter_ms=None)
    assert all(np.array_equal(a, b) for a, b in zip(none[0], plain)) and none[1] == plain_gain


def test_resample_encode_passes_the_limiter_on():
    fs = 8192
    x = way_out_stems(fs)
    a, b, info = rs.resample_encode_gpu(dev(x[0]), 1, 1, fmt="float32", loudness=TARGET, rate=fs, together=dev(x[1]), limiter_ms=MS)
    a0, b0, info0 = rs.resample_encode_gpu(dev(x[0]), 1, 1, fmt="float32", loudness=TARGET, rate=fs, together=dev(x[1]))
    assert float(a.abs().max()) <= 0.9 and float(b.abs().max()) <= 0.9
    assert info0[3].item() == 1 and float((a * a).sum()) > 2.0 * float((a0 * a0).sum())  # the limited file is more than 3 dB louder


# ------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def song(tmp_path_factory):
    """(checkpoint of the closed-form weights, 2 s stereo float32 file at 44.1 kHz with a click every 250 ms)."""
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import synth
    from svs_unet_pytorch_amd.model import UNet
    d = tmp_path_factory.mktemp("limiter")
    m = UNet()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state().items()})
    ck = str(d / "svs_closed_form.pth")
    torch.save({"model_state_dict": m.state_dict()}, ck)
    n, rate = 2 * 44100, 44100
    mix = np.stack([synth.audio(n, 50), 0.7 * synth.audio(n, 51)], axis=1).astype(np.float32)
    mix *= np.float32(0.05 / np.abs(mix).max())
    mix[rate // 8::rate // 4, :] = 0.9
    src = str(d / "mixture.wav")
    wavfile.write(src, rate, mix)
    return ck, src


def test_separate_cli_with_the_limiter(song, tmp_path, capsys):
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import separate
    ck, src = song
    v, a = str(tmp_path / "v.wav"), str(tmp_path / "a.wav")
    base = ["--model_path", ck, "--src", src, "--tar", v, "--tar_accomp", a]
    separate.main(base + ["--loudness", "-14", "--limiter", "--peak_ceiling", "0.8"])
    lines = [l for l in capsys.readouterr().out.splitlines() if "LUFS" in l]
    assert len(lines) == 1 and "limiter: deepest reduction" in lines[0] and "dB, written" in lines[0]
    for path in (v, a):
        rate, data = wavfile.read(path)
        assert rate == 44100 and data.dtype == np.int16 and data.shape == (2 * 44100, 2)
        assert np.abs(data.astype(np.int64)).max() <= round(0.8 * 32767)
    separate.main(base + ["--loudness", "-14", "--peak_ceiling", "0.8"])
    plain = [l for l in capsys.readouterr().out.splitlines() if "LUFS" in l]
    assert len(plain) == 1 and "limiter" not in plain[0]
    separate.main(base + ["--loudness", "-14", "--limiter", "3", "--true_peak", "--subtype", "PCM_24", "--dither", "tpdf"])
    line = [l for l in capsys.readouterr().out.splitlines() if "LUFS" in l]
    assert len(line) == 1 and "limiter: deepest reduction" in line[0] and "dBTP" in line[0]
    assert pcm.subtype_of(v) == "PCM_24" and pcm.subtype_of(a) == "PCM_24"
    with pytest.raises(SystemExit) as e:
        separate.main(base + ["--limiter"])
    assert e.value.code == 2 and "--limiter belongs to --loudness" in capsys.readouterr().err
    print(lines[0], plain[0], line[0], sep="\n")
