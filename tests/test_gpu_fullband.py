"""Full-band stems on the GPU (csrc/fullband.hip: svs_fullband_gains / svs_fullband_mix; fullband.py; separate_to_wav(fullband=))
against fullband.fullband_reference, the float64 definition, fed the device's own buffers.

Bounds (derived, no measured tolerance; u = 2^-24).  As tests/test_gpu_resample.py derives it, a T-term fp32 dot product with taps
rounded to fp32 is within  B = (T + 2) u S + T 2^-126  of the float64 sum, S = sum |in| |tap| (resample_reference(return_abs=True)).

  gains   num = sum_r mask mag by R fmaf, den = sum_r mag by R additions, q = num / den:
            |num' - num| <= (R + 2) u A with A = sum_r |mask mag|;   den' = den (1 + d), |d| <= R u;   one rounding of the quotient
            |q' - q| <= ((R + 2) A / den + (R + 1) |q|) u (1 + 2 R u)             [the factor 1.001 below covers 2 R u, R <= 128]
          den == 0 (every magnitude exactly zero, in fp32 as in fp64): the mean of the mask, |err| <= (R + 1) u sum_r |mask| / R.
  mix     g' = fmaf(frac', g1 - g0, g0) with frac' = (float)rem / (float)den: the conversions are exact below 2^24 (up * hop <= 11025 * 768
          here) and round once each above, the division rounds once, g1 - g0 once, the fmaf once:
            E_g = (4 |g1 - g0| + |g|) u,      E_gs = E_g (vocal),  E_g + u |1 - g| (accompaniment: one subtraction more)
          hi' = fl(x - acc_y'), p' = fl(norm acc_s'), out' = fl(g_s' hi' + p'):
            |out' - out| <= |norm| B_s + |g_s| B_y + E_gs (|hi| + B_y) + u (|norm U(v_s)| + |g_s hi| + |out|)   [times 1.001 for the
          second-order terms], the last bracket being the few ulps of the two products and of the result.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd import fullband as fb
from svs_unet_pytorch_amd import resample as rs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
CANARY = 777.0


def updown(rate):
    fr = Fraction(rate, 8192)
    return fr.numerator, fr.denominator


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def worst(name, got, want, bound, report):
    err = np.abs(got.astype(np.float64) - want)
    w = float((err / bound).max())
    print(f"{name}: max err {err.max():.3e}, worst err / bound {w:.3f}")
    return report(f"{name} worst err / bound", w, 1.0)


# ---- gains -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [256, 512])
@pytest.mark.parametrize("C", [1, 2])
def test_gains_within_the_quotient_bound(rows, C, report):
    seg, R = 128, rows // fb.TOP_DIV
    ok = True
    for T in (1, 2, 127, 128, 129, 200):
        rng = np.random.default_rng(1000 * rows + 10 * T + C)
        n_tiles = -(-T // seg)
        tiles = rng.random((C, n_tiles, 1, rows, seg), dtype=np.float32)
        mask = rng.random((C * n_tiles, 1, rows, seg), dtype=np.float32)
        silent = T - 1                                              # a frame whose top rows are all zero: the mean of the mask
        tiles[C - 1, silent // seg, 0, rows - R:, silent % seg] = 0.0
        if T % seg:                                                 # the padded frames of the last tile must not reach a result
            tiles[:, -1, 0, :, T % seg:] = np.nan
            mask.reshape(tiles.shape)[:, -1, 0, :, T % seg:] = np.nan
        buf = torch.full((C * T + 64,), CANARY, dtype=torch.float32, device=DEV)
        got = fb.frame_gains_gpu(dev(tiles), dev(mask), T, out=buf[:C * T].view(C, T))
        torch.cuda.synchronize()
        assert got.data_ptr() == buf.data_ptr()
        host = buf.cpu().numpy()
        assert (host[C * T:] == CANARY).all(), "svs_fullband_gains wrote behind gf"
        got = host[:C * T].reshape(C, T)
        assert np.isfinite(got).all()
        want, A, den, msum = fb.frame_gains_reference(tiles, mask, T, return_abs=True)
        zero = den == 0
        assert zero[C - 1, silent] and zero.sum() == 1
        safe = np.where(zero, 1.0, den)
        bound = np.where(zero, (R + 1) * U * msum / R, ((R + 2) * A / safe + (R + 1) * np.abs(want)) * U * 1.001)
        ok &= worst(f"fullband gains rows={rows} C={C} T={T}", got, want, bound, report)
        again = fb.frame_gains_gpu(dev(tiles), dev(mask), T)
        assert np.array_equal(again.cpu().numpy(), got)             # run to run
    assert ok


# ---- mix -------------------------------------------------------------------------------------------------------------------

def make_pcm(rng, fmt, n, C):
    if fmt == "int16":
        return rng.integers(-32768, 32768, size=(n, C), dtype=np.int16)
    if fmt == "int32":
        return rng.integers(-2 ** 31, 2 ** 31, size=(n, C), dtype=np.int64).astype(np.int32)
    return (0.5 * rng.standard_normal((n, C))).astype(np.float32)


def mix_case(rate, hop, T, S, C, fmt, dlen, seed):
    """Random device-ready inputs: stems (S, C, n_in), y (C, n_in + 5), pcm of n_out + dlen frames, norm, gf."""
    rng = np.random.default_rng(seed)
    up, down = updown(rate)
    n_in = hop * (T - 1)
    n_out = rs.out_len(n_in, up, down)
    stems = rng.standard_normal((S, C, n_in)).astype(np.float32)
    y = rng.standard_normal((C, n_in + 5)).astype(np.float32)
    pcm = make_pcm(rng, fmt, n_out + dlen, C)
    norm = rng.uniform(0.5, 3.0, C).astype(np.float32)
    gf = rng.random((C, T), dtype=np.float32)
    return up, down, n_in, n_out, stems, y, pcm, norm, gf


def mix_bound(parts, out, norm, gf, frames, hop, up, down, S, invert):
    T = rs.taps_per_output(20 * max(up, down) + 1, up)
    Bs = (T + 2) * U * parts["us_abs"] + T * 2.0 ** -126
    By = (T + 2) * U * parts["uy_abs"] + T * 2.0 ** -126
    g, gs, hi = parts["g"], parts["gs"], parts["hi"]
    Eg = np.zeros_like(g)
    if gf is not None:
        k = fb.frame_coordinate(np.arange(g.shape[1], dtype=np.int64), up, down, hop)[0]
        g64 = gf.astype(np.float64)
        d = g64[:, np.minimum(k + 1, frames - 1)] - g64[:, np.minimum(k, frames - 1)]
        Eg = (4 * np.abs(d) + np.abs(g)) * U
    Egs = np.stack([Eg, Eg + U * np.abs(1 - g)])
    Egs = Egs[1:] if (S == 1 and invert) else Egs[:S]
    nu = np.abs(norm.astype(np.float64))[None, :, None]
    return (nu * Bs + np.abs(gs) * By + Egs * (np.abs(hi) + By) + U * (nu * np.abs(parts["us"]) + np.abs(gs * hi) + np.abs(out))) * 1.001


# (frames, stems, channels, pcm format, file length - n_out, mode, invert): every value of every column, and every pair of the
# frames / stems / channels columns, occurs
COMBOS = [(2, 1, 1, "int16", -1, "mask", False), (2, 2, 2, "int32", 1, "accomp", False), (9, 1, 2, "float32", 1, "mask", False),
          (9, 2, 1, "int16", -1, "accomp", False), (9, 2, 2, "float32", -1, "mask", False), (2, 1, 2, "int32", -1, "accomp", True),
          (9, 1, 1, "int32", 1, "mask", True), (2, 2, 1, "float32", 1, "mask", False)]


@pytest.mark.parametrize("rate", [44100, 48000, 22050, 16000])
@pytest.mark.parametrize("hop", [768, 96])
def test_mix_within_the_derived_bound(rate, hop, report):
    ok = True
    for j, (T, S, C, fmt, dlen, mode, invert) in enumerate(COMBOS):
        up, down, n_in, n_out, stems, y, pcm, norm, gf = mix_case(rate, hop, T, S, C, fmt, dlen, seed=rate + hop + j)
        gf = gf if mode == "mask" else None
        out = torch.full((S, C, n_out + 32), CANARY, dtype=torch.float32, device=DEV)
        got = fb.fullband_mix_gpu(dev(stems), dev(y), dev(pcm if C > 1 else pcm[:, 0]), dev(norm), None if gf is None else dev(gf), T, hop,
                                  up, down, invert=invert, out=out)
        torch.cuda.synchronize()
        host = got.cpu().numpy()
        assert (host[:, :, n_out:] == CANARY).all(), "svs_fullband_mix wrote behind a row"
        x = fb.pcm_to_float(pcm).T                                  # (C, frames): one frame short of, or past, n_out
        want, parts = fb.fullband_reference(stems, y, x, norm, gf, T, hop, up, down, invert=invert, return_parts=True)
        assert want.shape == (S, C, n_out)
        if dlen < 0:
            assert not parts["x"][:, -1].any()                      # x is zero past the file's end
        bound = mix_bound(parts, want, norm, gf, T, hop, up, down, S, invert)
        ok &= worst(f"fullband mix {rate} Hz hop={hop} T={T} S={S} C={C} {fmt} {mode}{' inverted' if invert else ''}", host[:, :, :n_out], want,
                    bound, report)
    assert ok


@pytest.mark.parametrize("rate", [44100, 16000])
def test_mix_bitwise_properties(rate):
    """The accumulators are svs_resample_poly's floats: with gf = 0 and norm = 1 the vocal IS the up-sampled stem, with zero stems
    and gf = 1 it is x - svs_resample_poly(y); the accompaniment of gf = 0 takes the same high band; two runs agree."""
    T, hop, C = 9, 768, 2
    up, down, n_in, n_out, stems, y, pcm, norm, gf = mix_case(rate, hop, T, 2, C, "int16", 1, seed=rate)
    st, yd, pd = dev(stems), dev(y), dev(pcm)
    one, zero_gf, one_gf = torch.ones(C, device=DEV), torch.zeros((C, T), device=DEV), torch.ones((C, T), device=DEV)
    up_stems = rs.resample_poly_gpu(st.view(2 * C, n_in), up, down).view(2, C, n_out)
    up_y = rs.resample_poly_gpu(yd[:, :n_in].contiguous(), up, down)
    x = dev(fb.pcm_to_float(pcm).T[:, :n_out])
    hi = x - up_y
    for g in (zero_gf, None):                                       # gf = 0 and mode "accomp" are the same arithmetic
        a = fb.fullband_mix_gpu(st, yd, pd, one, g, T, hop, up, down)
        assert torch.equal(a[0], up_stems[0])
        assert torch.equal(fb.fullband_mix_gpu(st[:1], yd, pd, one, g, T, hop, up, down)[0], up_stems[0])
    b = fb.fullband_mix_gpu(torch.zeros_like(st), yd, pd, dev(norm), one_gf, T, hop, up, down)
    assert torch.equal(b[0], hi)
    c = fb.fullband_mix_gpu(torch.zeros_like(st), yd, pd, dev(norm), None, T, hop, up, down)
    assert torch.equal(c[1], hi) and not c[0].any()
    full = [fb.fullband_mix_gpu(st, yd, pd, dev(norm), dev(gf), T, hop, up, down) for _ in range(2)]
    assert torch.equal(full[0], full[1])
    solo = fb.fullband_mix_gpu(st[1:], yd, pd, dev(norm), dev(gf), T, hop, up, down, invert=True)
    assert torch.equal(solo[0], full[0][1])                         # one stem or two: the same floats


def test_argument_errors_launch_nothing():
    L = _lib.lib()
    T, hop, C = 2, 768, 2
    up, down, n_in, n_out, stems, y, pcm, norm, gf = mix_case(44100, hop, T, 2, C, "int16", 0, seed=5)
    st, yd, pd, nd, gd = dev(stems), dev(y), dev(pcm), dev(norm), dev(gf)
    table, ntaps = rs.tap_table(up, down, DEV)
    out = torch.full((2, C, n_out), CANARY, dtype=torch.float32, device=DEV)
    s = _lib.stream_ptr()

    def call(**kw):
        a = dict(stems=st.data_ptr(), nstems=2, ld_stem=C * n_in, ld_in=n_in, y=yd.data_ptr(), ld_y=y.shape[1], channels=C, n_in=n_in,
                 pcm=pd.data_ptr(), fmt=1, n_pcm=n_out, table=table.data_ptr(), ntaps=ntaps, up=up, down=down, norm=nd.data_ptr(),
                 gf=gd.data_ptr(), frames=T, hop=hop, invert=0, out=out.data_ptr(), ld_out=n_out, ld_out_stem=C * n_out, stream=s)
        a.update(kw)
        return L.svs_fullband_mix(*a.values())

    for kw, msg in ((dict(nstems=3), b"nstems"), (dict(channels=9), b"channels"), (dict(invert=1), b"invert"), (dict(fmt=5), b"pcm_fmt"),
                    (dict(ntaps=ntaps - 1), b"bad filter"), (dict(frames=0), b"frames"), (dict(hop=0), b"hop"), (dict(n_in=0), b"n_in"),
                    (dict(ld_y=n_in - 1), b"ld_y"), (dict(ld_out=n_out - 1), b"ld_out"), (dict(ld_out_stem=n_out), b"ld_out_stem"),
                    (dict(norm=None), b"null pointer"), (dict(out=None), b"null pointer")):
        assert call(**kw) < 0, kw
        assert msg in L.svs_last_error_string(), (kw, L.svs_last_error_string())
    tiles = torch.zeros((C, 1, 1, 256, 128), device=DEV)
    gout = torch.full((C, T), CANARY, device=DEV)
    for geom, msg in (((C, 1, 254, 128, T), b"multiple of 4"), ((C, 1, 256, 128, 129), b"do not end"), ((C, 2, 256, 128, T), b"do not end"),
                      ((0, 1, 256, 128, T), b"positive")):
        c, n_tiles, rows, seg, frames = geom
        assert L.svs_fullband_gains(tiles.data_ptr(), tiles.data_ptr(), 256 * 128, c, n_tiles, rows, seg, frames, gout.data_ptr(), s) < 0
        assert msg in L.svs_last_error_string()
    torch.cuda.synchronize()
    assert (out == CANARY).all() and (gout == CANARY).all()         # nothing was launched
    assert call() == 0                                              # the unchanged call is legal
    torch.cuda.synchronize()
    assert not (out == CANARY).any()
    with pytest.raises(ValueError):
        fb.fullband_mix_gpu(torch.zeros(2, 2, 768), yd, pd, nd, gd, T, hop, up, down)       # host tensor: no CPU path
    with pytest.raises(TypeError):
        fb.fullband_mix_gpu(st, yd, pd.double(), nd, gd, T, hop, up, down)


# ---- end to end --------------------------------------------------------------------------------------------------------------

RATE, HOP = 44100, 768


@pytest.fixture(scope="module")
def model():
    from svs_unet_pytorch_amd.model import UNet
    m = UNet()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state().items()})
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def noise_file(tmp_path_factory):
    """1 s of stereo int16 white noise at 44.1 kHz, the right channel 6 dB under the left, faded in over 0.1 s and out to silence by
    frame 40,000.  The separated signal ends at frame 41,344 (hop * (T - 1) samples of the network rate) and the file is padded
    with zeros from there: noise that is still running at that frame would put a step there, whose click has 4.7e-6 of the
    source's energy above 5 kHz by itself (numpy, float64) and would be all that a measurement of that band sees."""
    n, fade = RATE, RATE // 10
    rng = np.random.default_rng(44)
    env = np.ones(n)
    env[:fade] = 0.5 - 0.5 * np.cos(np.pi * np.arange(fade) / fade)
    env[40000 - fade:40000] = 0.5 + 0.5 * np.cos(np.pi * np.arange(fade) / fade)
    env[40000:] = 0.0
    x = rng.uniform(-1.0, 1.0, (n, 2)) * env[:, None] * np.array([1.0, 0.5])
    path = str(tmp_path_factory.mktemp("fullband") / "noise.wav")
    wavfile.write(path, RATE, np.round(x * 32767).astype(np.int16))
    return path


def energy_above(sig, hz=5000.0):
    """Energy above `hz` per channel summed, of (frames, channels) samples at RATE."""
    spec = np.fft.rfft(np.asarray(sig, dtype=np.float64), axis=0)
    return float((np.abs(spec[np.fft.rfftfreq(sig.shape[0], 1.0 / RATE) > hz]) ** 2).sum())


def separate(model, src, tmp_path, tag, **kw):
    from svs_unet_pytorch_amd import streaming
    v, a = str(tmp_path / f"{tag}_v.wav"), str(tmp_path / f"{tag}_a.wav")
    report = {}
    streaming.separate_to_wav(model, src, v, subtype="FLOAT", dst_accomp_path=a, report=report, **kw)
    return wavfile.read(v)[1], wavfile.read(a)[1], report


def expected(model, src, mode="mask", both=True, vocal_solo=True, **kw):
    """What separate_to_wav(fullband=mode) must write before the gain, from its pieces: the float64 definition fed the device's own
    y, stems, tiles, mask and norm (and the device's gf), its bound, and the identity's right-hand side."""
    from svs_unet_pytorch_amd import data, streaming
    rate, pcm, channels = data.read_pcm(src)
    up, down = updown(rate)
    y = rs.resample_poly_gpu(dev(pcm), down, up, channels=channels, downmix=False)
    aux = {}
    stems = streaming.separate_waveform(model, y, peak=None, both_stems=both, vocal_solo=vocal_solo, aux=aux, **kw)
    stems = stems if both else stems[None]
    invert = not both and not vocal_solo
    T = aux["frames"]
    gf = fb.frame_gains_gpu(aux["tiles"], aux["mask"], T).cpu().numpy() if mode == "mask" else None
    st, yh, norm = stems.cpu().numpy(), aux["y"].cpu().numpy(), aux["norm"].cpu().numpy()
    want, parts = fb.fullband_reference(st, yh, fb.pcm_to_float(pcm).T, norm, gf, T, HOP, up, down, invert=invert, return_parts=True)
    bound = mix_bound(parts, want, norm, gf, T, HOP, up, down, len(st), invert)
    n_in = st.shape[2]
    both_sum = st.astype(np.float64).sum(0)                         # (with one stem the identity has no second term: rhs is not used)
    rhs = parts["x"] - rs.resample_reference(yh[:, :n_in].astype(np.float64) - norm[:, None].astype(np.float64) * both_sum, up, down)
    return want, bound, rhs, pcm


def check_files(name, v, a, gains, want, bound, rhs, n_source, report):
    """The two FLOAT files, each divided by its gain, are the definition's stems (within the mix bound and the encoder's one
    multiply) and add up to the identity's right-hand side; past the separated frames they are silent."""
    n_out = want.shape[2]
    assert v.shape == a.shape == (n_source, 2) and v.dtype == a.dtype == np.float32 and n_out <= n_source
    assert not v[n_out:].any() and not a[n_out:].any()
    got = np.stack([v[:n_out].T.astype(np.float64) / gains[0], a[:n_out].T.astype(np.float64) / gains[1]])
    enc = 1.001 * U * np.abs(got)                                   # the encoder's fp32 multiply by the gain
    ok = worst(f"{name}: files / gain vs the definition", got, want, bound + enc, report)
    total = (bound + enc).sum(0) + 1e-15 * np.abs(rhs)              # (the identity holds to 5e-16 in float64)
    ok &= worst(f"{name}: vocal + accompaniment vs x - U(y - norm (v0 + v1))", got.sum(0), rhs, total, report)
    return ok


def test_flag_absent_writes_the_same_bytes(model, noise_file, tmp_path):
    from svs_unet_pytorch_amd import streaming
    for both in (False, True):
        paths = {}
        for tag, kw in (("plain", {}), ("none", {"fullband": None})):
            paths[tag] = [str(tmp_path / f"{tag}{both}_{s}.wav") for s in "va"]
            streaming.separate_to_wav(model, noise_file, paths[tag][0], dst_accomp_path=paths[tag][1] if both else None, **kw)
        for p, q in zip(paths["plain"][:1 + both], paths["none"]):
            assert open(p, "rb").read() == open(q, "rb").read()


def test_separate_to_wav_mask_adds_up_and_fills_the_band(model, noise_file, tmp_path, report):
    src = wavfile.read(noise_file)[1].astype(np.float64) / 32768.0
    e_src = energy_above(src)
    v, a, rep = separate(model, noise_file, tmp_path, "mask", fullband="mask")
    want, bound, rhs, pcm = expected(model, noise_file)
    assert set(rep) == {"gains"} and len(rep["gains"]) == 2
    assert np.abs(v).max() == pytest.approx(0.9, abs=1e-6) and np.abs(a).max() == pytest.approx(0.9, abs=1e-6)   # the peak rule, per file
    assert check_files("separate_to_wav mask", v, a, rep["gains"], want, bound, rhs, len(src), report)
    full = v.astype(np.float64) / rep["gains"][0] + a.astype(np.float64) / rep["gains"][1]
    ratio_on = energy_above(full) / e_src
    # the stereo balance is the file's again: the right channel lies 6 dB under the left
    lr = np.sqrt((full[:, 1] ** 2).sum() / (full[:, 0] ** 2).sum())
    v0, a0, _ = separate(model, noise_file, tmp_path, "off")
    ratios_off = [energy_above(s) / e_src for s in (v0, a0)]
    print(f"energy above 5 kHz / the source's: flag on (stems summed) {ratio_on:.6f}; flag off, vocal {ratios_off[0]:.3e}, "
          f"accompaniment {ratios_off[1]:.3e}; right / left of the sum {lr:.4f}")
    assert report("fullband mask: |energy above 5 kHz / source - 1|", abs(ratio_on - 1.0), 0.01)
    assert report("fullband off: energy above 5 kHz / source, worse stem", max(ratios_off), 1e-6)
    assert abs(lr - 0.5) < 0.01


def test_separate_to_wav_accomp_and_one_stem(model, noise_file, tmp_path, report):
    from svs_unet_pytorch_amd import streaming
    v, a, rep = separate(model, noise_file, tmp_path, "accomp", fullband="accomp")
    want, bound, rhs, pcm = expected(model, noise_file, mode="accomp")
    assert check_files("separate_to_wav accomp", v, a, rep["gains"], want, bound, rhs, len(pcm), report)
    e_src = energy_above(pcm.astype(np.float64) / 32768.0)
    assert energy_above(v) / e_src < 1e-6                           # the vocal stays band-limited
    # without dst_accomp_path one stem is written (S = 1), the vocal or the accompaniment, by the peak rule
    ok = True
    for tag, solo in (("solo_v", True), ("solo_a", False)):
        path, rep1 = str(tmp_path / f"{tag}.wav"), {}
        streaming.separate_to_wav(model, noise_file, path, subtype="FLOAT", vocal_solo=solo, fullband="mask", report=rep1)
        one = wavfile.read(path)[1]
        want1, bound1, _, _ = expected(model, noise_file, both=False, vocal_solo=solo)
        n_out = want1.shape[2]
        assert one.shape == (len(pcm), 2) and not one[n_out:].any() and np.abs(one).max() == pytest.approx(0.9, abs=1e-6)
        got = one[:n_out].T.astype(np.float64) / rep1["gains"][0]
        ok &= worst(f"separate_to_wav mask, one stem ({tag})", got[None], want1, bound1 + 1.001 * U * np.abs(got), report)
    assert ok


@pytest.mark.parametrize("kw", [{"tile_hop": 64}, {"phase_iters": 1}], ids=["tile_hop64", "phase_iters1"])
def test_composes_with_the_other_post_filters(model, noise_file, tmp_path, report, kw):
    v, a, rep = separate(model, noise_file, tmp_path, "compose", fullband="mask", **kw)
    want, bound, rhs, pcm = expected(model, noise_file, **kw)
    assert check_files(f"separate_to_wav mask {kw}", v, a, rep["gains"], want, bound, rhs, len(pcm), report)


def test_tile_hop_on_two_tiles(model, tmp_path, report):
    """The 1 s file above has 11 frames, one tile, where tile_hop = 64 cuts nothing.  13 s have 139 frames, two disjoint tiles and
    three overlapped ones: the gains must come from the BLENDED mask, the one the stems were made from."""
    from svs_unet_pytorch_amd import data, streaming
    n = 13 * RATE
    mix = 0.4 * np.stack([synth.audio(n, 30), 0.8 * synth.audio(n, 31)], axis=1)
    src = str(tmp_path / "long.wav")
    wavfile.write(src, RATE, np.round(mix / np.abs(mix).max() * 30000).astype(np.int16))
    v, a, rep = separate(model, src, tmp_path, "hop64", fullband="mask", tile_hop=64)
    want, bound, rhs, pcm = expected(model, src, tile_hop=64)
    assert check_files("separate_to_wav mask tile_hop=64, 139 frames", v, a, rep["gains"], want, bound, rhs, n, report)
    y = rs.resample_poly_gpu(dev(data.read_pcm(src)[1]), 2048, 11025, channels=2, downmix=False)
    gfs = []
    for hop in (128, 64):
        aux = {}
        streaming.separate_waveform(model, y, peak=None, both_stems=True, tile_hop=hop, aux=aux)
        assert aux["frames"] == 139 and aux["tiles"].shape[1] == 2 and aux["mask"].numel() == aux["tiles"].numel()
        gfs.append(fb.frame_gains_gpu(aux["tiles"], aux["mask"], aux["frames"]))
    assert not torch.equal(gfs[0], gfs[1])                          # the cross-fade changed the mask the gains are read from


def test_loudness_gives_both_files_one_gain(model, noise_file, tmp_path, report):
    from svs_unet_pytorch_amd import loudness as ld
    v, a, rep = separate(model, noise_file, tmp_path, "lufs", fullband="mask", loudness=-23.0)
    want, bound, rhs, pcm = expected(model, noise_file)
    assert rep["gains"][0] == rep["gains"][1] == rep["gain"] and len(rep["info"]) == 4
    assert check_files("separate_to_wav mask loudness=-23", v, a, rep["gains"], want, bound, rhs, len(pcm), report)
    L = ld.loudness_reference((v.astype(np.float64) + a.astype(np.float64)).T, RATE)[0]
    print(f"fullband + loudness: the sum reads {L:.4f} LUFS for target -23 (limited: {rep['info'][3]})")
    if not rep["info"][3]:
        assert report("fullband + loudness, sum vs target (LU)", abs(L + 23.0), 0.01)
    assert max(np.abs(v).max(), np.abs(a).max()) <= 0.9


def test_cli_and_a_file_at_the_network_rate(model, tmp_path, capsys):
    """separate.py --fullband through the command line; a file at 8,192 Hz has no high band: a warning, and the default path's bytes."""
    from svs_unet_pytorch_amd import separate as cli
    from svs_unet_pytorch_amd import streaming
    ck = str(tmp_path / "svs.pth")
    torch.save({"model_state_dict": model.state_dict()}, ck)
    n = 22050 // 2
    pcm = np.random.default_rng(3).integers(-9000, 9000, size=(n, 2), dtype=np.int16)
    src = str(tmp_path / "in22.wav")
    wavfile.write(src, 22050, pcm)
    voc, acc = str(tmp_path / "v.wav"), str(tmp_path / "a.wav")
    cli.main(["--model_path", ck, "--src", src, "--tar", voc, "--tar_accomp", acc, "--fullband", "mask"])
    assert "Separation finished" in capsys.readouterr().out
    (r0, v), (r1, a) = wavfile.read(voc), wavfile.read(acc)
    assert r0 == r1 == 22050 and v.dtype == a.dtype == np.int16 and v.shape == a.shape == (n, 2)
    assert max(np.abs(v.astype(np.int32)).max(), np.abs(a.astype(np.int32)).max()) == 29490       # rint(0.9 * 32767), one file at least
    low = str(tmp_path / "in8.wav")
    wavfile.write(low, 8192, pcm)
    with pytest.warns(UserWarning, match="no band above"):
        streaming.separate_to_wav(model, low, voc, fullband="mask")
    streaming.separate_to_wav(model, low, acc)
    assert open(voc, "rb").read() == open(acc, "rb").read()
