"""The YIN f0 tracker on the device (-m gpu; csrc/f0.hip) against the float64 definition of f0.py: d' and the rms, the pick as a stage
gate on the device's own d', the fused launch against the staged pair, independence of the launch, the pitch on known tones, and the
three interfaces (separate_waveform(f0=), separate.py --f0_csv, evaluate.py --melody --device gpu).

Shapes: the smallest at which each path of the kernel is taken -- 2, 4 and 8 lags per lane (tau_max 127, 160, 882 / 2048), a lag
range that needs one, two and four passes of the wave, an odd W, hop 1, frames that share no sample (one frame per block), W < tau_max,
and both limits at once (W 4096, tau_max 2048: one frame per block by the LDS bound).  No signal is longer than 18,432 samples.

Bounds.  d' and rms: one float32 ulp, |delta| <= 2^-23 |value| -- the fp64 sum of at most 4,096 non-negative terms and the 2,048-term
scan err by at most about 6,144 * 2^-53 relative in any order, far below half an ulp of float32, so only a flip at a rounding boundary
remains.  The pick, on the device's own d': voiced and ap bitwise, f0 to 2^-22 relative (one fp64 division chain rounded once to
float32, with one ulp of slack for the division's contraction).  The kernel has no tau output: tau is pinned through ap = d'(tau)
bitwise together with f0 = sr / (tau + delta).  Everything else is equality of bits."""
import functools

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import f0 as f0m

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -23
GATE = 1e-3                                                          # between the rms of the rows at level 1e-3 and at level 1

# (sr, fmin, fmax, W, tau_max, hop, tone Hz, frames)
SHAPES = {
    "defaults": (8192, 65, 1000, 252, 127, 82, 220.0, 11),
    "odd W, hop 1": (8192, 65, 1000, 257, 127, 1, 220.0, 13),
    "file rate": (44100, 50, 1000, 1358, 882, 441, 220.0, 6),
    "W < tau_max, disjoint frames": (16000, 100, 4000, 64, 160, 300, 440.0, 6),
    "limits": (100000, 48.83, 50000, 4096, 2048, 4096, 200.0, 4),
}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # a copy: the cached cases are read-only


def strided(x):
    """A device view of x's rows whose row stride is no multiple of 4 and whose first sample lies one float past a 16-byte boundary."""
    rows, n = x.shape
    ld = n + 5 + (1 if (n + 5) % 4 == 0 else 0)
    base = torch.zeros(1 + rows * ld + 3, dtype=torch.float32, device=DEV)
    view = base[1:1 + rows * ld].view(rows, ld)[:, :n]
    view.copy_(dev(x))
    assert view.data_ptr() % 16 == 4 and view.stride(0) % 4 != 0 and view.stride(1) == 1
    return view


@functools.lru_cache(maxsize=None)
def case(name):
    """(geometry, x (4, n) float32: a harmonic tone plus noise 20 dB under it at levels 1, 1e-3 and 30, and a row of noise alone;
    the definition's d' and rms).  Computed once per shape and left unchanged."""
    sr, fmin, fmax, W, tau_max, hop, hz, frames = SHAPES[name]
    g = f0m.geometry(sr, fmin, fmax, W, hop, rms_gate=GATE)
    assert g.tau_max == tau_max and g.W == W and g.hop == hop
    n = g.span + (frames - 1) * hop + min(hop - 1, 37)               # a tail that forms no further frame
    assert f0m.frame_count(n, g.span, hop) == frames
    rng = np.random.default_rng(len(name))
    tone = f0m.harmonic_tone(np.full(n, hz), sr).astype(np.float64)
    noisy = tone + 0.1 * np.sqrt(np.mean(tone ** 2)) * rng.standard_normal(n)
    x = np.stack([noisy, 1e-3 * noisy, 30.0 * noisy, 0.1 * rng.standard_normal(n)]).astype(np.float32)
    x.setflags(write=False)
    dp, rms = f0m.cmnd_reference(x, W, tau_max, hop)
    return g, x, dp, rms


def track(x, name, **kw):
    sr, fmin, fmax, W, tau_max, hop, hz, frames = SHAPES[name]
    return f0m.track_gpu(x, sr, fmin, fmax, W, hop, rms_gate=GATE, **kw)


def same(a: f0m.Track, b: f0m.Track):
    return all(torch.equal(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------------------------------------
# d' and rms against the definition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_cmnd_against_the_definition(name, report):
    g, x, want, want_rms = case(name)
    for what, view in (("contiguous", dev(x)), ("odd row stride, 4 bytes off", strided(x))):
        dp, rms = f0m.cmnd_gpu(view, g.W, g.tau_max, g.hop)
        assert dp.shape == want.shape and dp.dtype == torch.float32 and rms.shape == want_rms.shape
        again = f0m.cmnd_gpu(view, g.W, g.tau_max, g.hop)
        assert torch.equal(dp, again[0]) and torch.equal(rms, again[1])                  # the same bits again
        got, got_rms = dp.cpu().numpy().astype(np.float64), rms.cpu().numpy().astype(np.float64)
        assert (got[..., 0] == 1.0).all() and np.isfinite(got).all()
        err = float((np.abs(got - want) / np.abs(want)).max())
        err_rms = float((np.abs(got_rms - want_rms) / want_rms).max())
        flips = int((got != want).sum())
        print(f"f0 cmnd {name} {what}: d' err {err:.3e} of its value ({flips} of {got.size} values differ), rms err {err_rms:.3e}; bound {ULP:.3e}")
        assert report(f"f0 d' {name} {what}", err, ULP)
        assert report(f"f0 rms {name} {what}", err_rms, ULP)
        assert f0m.cmnd_gpu(view, g.W, g.tau_max, g.hop, rms=False)[1] is None


@pytest.mark.parametrize("name", ["defaults", "W < tau_max, disjoint frames"])
def test_one_and_two_frame_signals(name, report):
    g, x, _, _ = case(name)
    for n, frames in ((g.span, 1), (g.span + g.hop - 1, 1), (g.span + g.hop, 2)):
        piece = np.ascontiguousarray(x[:, :n])
        want, want_rms = f0m.cmnd_reference(piece, g.W, g.tau_max, g.hop)
        dp, rms = f0m.cmnd_gpu(strided(piece), g.W, g.tau_max, g.hop)
        assert dp.shape == (4, frames, g.tau_max + 1)
        err = float((np.abs(dp.cpu().numpy().astype(np.float64) - want) / want).max())
        assert report(f"f0 d' {name} n={n} ({frames} frames)", err, ULP)
        assert report(f"f0 rms {name} n={n}", float((np.abs(rms.cpu().numpy().astype(np.float64) - want_rms) / want_rms).max()), ULP)
        fused = track(dev(piece), name)
        assert fused.f0.shape == (4, frames) and torch.equal(fused.rms, rms)
        assert torch.equal(fused.f0[:, :1], track(dev(x), name, n_frames=1).f0)          # the first frame of the longer signal
    with pytest.raises(ValueError, match="one frame needs span"):
        track(dev(x[:, :g.span - 1]), name)


# ------------------------------------------------------------------------------------------------
# the pick: a stage gate on the device's own d'
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_pick_on_the_devices_own_dprime(name, report):
    g, x, _, _ = case(name)
    dp, rms = f0m.cmnd_gpu(dev(x), g.W, g.tau_max, g.hop)
    f0, ap, voiced = f0m.pick_gpu(dp, g.sr, g.tau_min, g.threshold, rms, GATE)
    w_f0, w_ap, w_voiced, w_tau = f0m.pick_reference(dp.cpu().numpy(), g.sr, g.tau_min, g.tau_max, g.threshold, rms.cpu().numpy(), GATE)
    found = f0m.pick_reference(dp.cpu().numpy(), g.sr, g.tau_min, g.tau_max, g.threshold)[2].astype(bool)
    assert found[0].all() and found[1].all() and found[2].all() and not found[3].any()  # both branches are taken: the tones, the noise
    assert np.array_equal(voiced.cpu().numpy(), w_voiced) and voiced.dtype == torch.int32
    assert w_voiced[0].all() and not w_voiced[1].any() and w_voiced[2].all()            # the gate takes the quiet row, whatever its d'
    assert np.array_equal(ap.cpu().numpy(), w_ap)                                        # d'(tau), bit for bit
    got = f0.cpu().numpy().astype(np.float64)
    err = float((np.abs(got - w_f0.astype(np.float64)) / w_f0).max())
    print(f"f0 pick {name}: f0 err {err:.3e} relative (bound {2.0 ** -22:.3e}); tau {w_tau.min()}..{w_tau.max()} of {g.tau_min}..{g.tau_max}")
    assert report(f"f0 pick {name}", err, 2.0 ** -22)
    assert (np.abs(g.sr / got - w_tau) <= 1.0 + 1e-6).all()                              # tau + delta, |delta| <= 1
    ungated = f0m.pick_gpu(dp, g.sr, g.tau_min, g.threshold)                              # no rms: voiced = found
    assert np.array_equal(ungated[2].cpu().numpy().astype(bool), found) and torch.equal(ungated[0], f0)


def test_pick_keeps_the_smallest_index_on_ties():
    """Hand-made rows wider than one pass of the wave: equal minima 64 and 128 lags apart, and two lags under the threshold."""
    tau_max = 300
    rows = np.ones((4, tau_max + 1), np.float32)
    rows[0, [70, 134, 198]] = 0.5                # no lag under the threshold: the first of three equal minima
    rows[1, [262, 6]] = 0.4                      # the same with the smaller index on a later lane
    rows[2, [200, 90]] = 0.1                     # two under the threshold: the first; no walk (its neighbours are 1)
    rows[3, 40:44] = [0.14, 0.12, 0.12, 0.13]    # walks down from 40 to 41 and stops on equality
    f0, ap, voiced = f0m.pick_gpu(dev(rows), 8192.0, 5, 0.15)
    w_f0, w_ap, w_voiced, w_tau = f0m.pick_reference(rows, 8192.0, 5, tau_max, 0.15)
    assert w_tau.tolist() == [70, 6, 90, 41] and w_voiced.tolist() == [0, 0, 1, 1]
    assert np.array_equal(voiced.cpu().numpy(), w_voiced) and np.array_equal(ap.cpu().numpy(), w_ap)
    assert np.allclose(f0.cpu().numpy(), w_f0, rtol=2.0 ** -22, atol=0)


# ------------------------------------------------------------------------------------------------
# fused against staged, independence of the launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_is_staged_and_no_frame_depends_on_the_launch(name):
    g, x, _, _ = case(name)
    frames = SHAPES[name][7]
    xd = strided(x)
    dp, rms = f0m.cmnd_gpu(xd, g.W, g.tau_max, g.hop)
    f0, ap, voiced = f0m.pick_gpu(dp, g.sr, g.tau_min, g.threshold, rms, GATE)
    whole = track(xd, name)
    assert whole.f0.shape == (4, frames) and np.array_equal(whole.time.cpu().numpy(), f0m.frame_times(g, frames))
    assert same(whole, f0m.Track(whole.time, f0, voiced, ap, rms))                        # bit for bit the staged pair
    assert same(whole, track(dev(x), name))                                               # whatever the alignment
    for cut in (1, frames // 2, frames - 1):                                              # 1 is no multiple of the frames a block owns
        head, tail = track(xd, name, first_frame=0, n_frames=cut), track(xd, name, first_frame=cut)
        assert tail.f0.shape == (4, frames - cut)
        assert same(whole, f0m.Track(*(torch.cat([a, b], dim=-1) for a, b in zip(head, tail))))
        dp_tail = f0m.cmnd_gpu(xd, g.W, g.tau_max, g.hop, first_frame=cut)[0]
        assert torch.equal(dp_tail, dp[:, cut:])
    for r in range(4):                                                                    # a row alone is the row among the others
        alone = track(dev(x[r]), name)
        assert alone.f0.shape == (frames,) and same(alone, f0m.Track(whole.time, *(c[r] for c in whole[1:])))


# ------------------------------------------------------------------------------------------------
# the pitch on the host file's tones
# ------------------------------------------------------------------------------------------------
def test_device_pitch_on_known_tones(report):
    from test_f0_host import MEASURED, SR, cents_off, tones
    for name, (freq, n) in tones().items():
        x = f0m.harmonic_tone(freq(np.arange(n) / SR), SR)
        t = f0m.track_gpu(dev(x), SR)
        got = f0m.Track(*(c.cpu().numpy() for c in t))
        worst = float(cents_off(got, freq).max())
        print(f"device {name}: {got.f0.size} frames, largest error {worst:.6f} cents (CPU measured {MEASURED[name]})")
        assert (got.voiced == 1).all()
        assert report(f"f0 device pitch {name} (cents)", worst, 1.5 * MEASURED[name] + 0.01)


# ------------------------------------------------------------------------------------------------
# the interfaces
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_model():
    from svs_unet_pytorch_amd.model import UNet
    torch.manual_seed(1234)
    return UNet().to(DEV).eval()


def mixture(seconds=3.0, rate=44100):
    """Stereo noise plus a 220 Hz harmonic tone."""
    n = int(seconds * rate)
    tone = f0m.harmonic_tone(np.full(n, 220.0), rate)
    noise = (0.05 * np.random.default_rng(7).standard_normal((2, n))).astype(np.float32)
    return np.stack([tone + noise[0], 0.6 * tone + noise[1]]).astype(np.float32)


def test_separate_waveform_returns_the_track_beside_the_stems():
    from svs_unet_pytorch_amd.streaming import separate_waveform
    model, y = random_model(), dev(mixture())
    frames = f0m.frame_count(24576, 381, 82)                         # 3 s at 8,192 Hz are 32 whole hops of the transform
    for kw in (dict(), dict(both_stems=True), dict(both_stems=True, sr_out=44100, peak=None), dict(wiener_iters=1)):
        plain = separate_waveform(model, y, sr_in=44100, **kw)
        stems, t = separate_waveform(model, y, sr_in=44100, f0=True, **kw)
        assert torch.equal(stems, plain)                                                  # the stems of the call without it
        assert t.f0.shape == (frames,)
        if "sr_out" not in kw:                                                            # the returned vocal IS at the network rate
            vocal = stems[0] if kw.get("both_stems") else stems
            assert vocal.shape == (2, 24576) and same(t, f0m.track_gpu(f0m.channel_mean(vocal), 8192))
    stems, t = separate_waveform(model, y, sr_in=44100, f0=dict(fmin=100.0, hop=41, rms_gate=1e-3))
    assert same(t, f0m.track_gpu(f0m.channel_mean(stems), 8192, fmin=100.0, hop=41, rms_gate=1e-3))
    mono, t = separate_waveform(model, y[0], sr_in=44100, f0=True)
    assert mono.dim() == 1 and same(t, f0m.track_gpu(mono, 8192))
    with pytest.raises(ValueError, match="tracks the vocal stem"):
        separate_waveform(model, y, sr_in=44100, vocal_solo=False, f0=True)


def test_separate_cli_writes_the_track(tmp_path, capsys):
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import separate
    ck = str(tmp_path / "svs_random.pth")
    torch.save({"model_state_dict": random_model().state_dict()}, ck)
    (tmp_path / "in").mkdir()
    src = str(tmp_path / "in" / "mixture.wav")
    mix = mixture(1.5)
    wavfile.write(src, 44100, np.clip(np.round(mix.T * 20000), -32768, 32767).astype(np.int16))
    n8 = -((-mix.shape[1] * 8192) // 44100)
    frames = f0m.frame_count(768 * (n8 // 768), 381, 82)             # the stem at the network rate: whole hops of the transform
    for extra in ([], ["--tar_accomp", str(tmp_path / "a.wav")], ["--fullband", "mask", "--loudness", "-20"]):
        plain, with_csv, track = str(tmp_path / "plain.wav"), str(tmp_path / "with.wav"), str(tmp_path / "track.csv")
        separate.main(["--model_path", ck, "--src", src, "--tar", plain] + extra)
        capsys.readouterr()
        separate.main(["--model_path", ck, "--src", src, "--tar", with_csv, "--f0_csv", track] + extra)
        assert f"{track}: {frames} pitch frames" in capsys.readouterr().out
        assert open(plain, "rb").read() == open(with_csv, "rb").read()                    # the wav bytes of the run without the flag
        lines = open(track).read().splitlines()
        assert lines[0] == f0m.CSV_HEADER and len(lines) == 1 + frames
        cols = np.array([[float(v) for v in line.split(",")] for line in lines[1:]])
        assert np.allclose(cols[:, 0], f0m.frame_times(f0m.geometry(8192), frames), atol=1e-6) and np.isfinite(cols).all()
    separate.main(["--model_path", ck, "--src", str(tmp_path / "in"), "--tar", str(tmp_path / "v"), "--f0_csv", str(tmp_path / "f")])
    assert open(tmp_path / "f" / "mixture.csv").read() == open(track).read()              # a folder: NAME.csv, the same track
    with pytest.raises(SystemExit) as e:
        separate.main(["--model_path", ck, "--src", src, "--tar", plain, "--vocal_solo", "0", "--f0_csv", track])
    assert e.value.code == 2 and "--f0_csv tracks the vocal stem, and --vocal_solo 0 writes none" in capsys.readouterr().err


def test_f0_cli_on_the_device(tmp_path, capsys):
    """16- and 24-bit files: the device track of the mean of the channels, and the numbers of --device cpu within the tone's bound."""
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import pcm
    x = f0m.harmonic_tone(np.full(8192, 220.0), 8192)
    stereo = np.stack([x, 0.5 * x], axis=1)
    p16, p24 = str(tmp_path / "t16.wav"), str(tmp_path / "t24.wav")
    wavfile.write(p16, 8192, np.round(stereo * 32767.0).astype(np.int16))
    pcm.write_wav24(p24, 8192, pcm.pack24(np.round(stereo.astype(np.float64) * (2 ** 23 - 1)).astype(np.int32)))
    for path in (p16, p24):
        out_gpu, out_cpu = path[:-4] + "_gpu.csv", path[:-4] + "_cpu.csv"
        f0m.main(["--src", path, "--csv", out_gpu])
        f0m.main(["--src", path, "--csv", out_cpu, "--device", "cpu"])
        assert capsys.readouterr().out.count("96 frames, 96 voiced") == 2
        a, b = (np.array([[float(v) for v in line.split(",")] for line in open(p).read().splitlines()[1:]]) for p in (out_gpu, out_cpu))
        assert a.shape == b.shape == (96, 5) and np.array_equal(a[:, [0, 2]], b[:, [0, 2]])
        assert np.abs(1200.0 * np.log2(a[:, 1] / b[:, 1])).max() <= 0.01 and np.allclose(a[:, 4], b[:, 4], rtol=1e-5)


def test_evaluate_melody_on_the_device(tmp_path, capsys):
    """The reference tone and the same tone with an octave jump in the middle: the five columns are melody_metrics of the two device
    tracks, and RPA < RCA = 1."""
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import evaluate
    sr, n = 8192, 12288
    t = np.arange(n) / sr
    ref = f0m.harmonic_tone(np.full(n, 220.0), sr)
    est = f0m.harmonic_tone(np.where((t >= 0.5) & (t < 1.0), 440.0, 220.0), sr)
    accomp = (0.02 * np.random.default_rng(3).standard_normal(n)).astype(np.float32)
    for folder, x in (("ref", ref), ("est", est), ("mix", ref + accomp)):
        (tmp_path / folder).mkdir()
        wavfile.write(str(tmp_path / folder / "song.wav"), sr, x)
    results = evaluate.main(["--est", str(tmp_path / "est"), "--mix", str(tmp_path / "mix"), "--ref", str(tmp_path / "ref"), "--melody",
                             "--device", "gpu"])
    said = capsys.readouterr().out
    gate = f0m.gate_from_db(f0m.MELODY_GATE_DB)
    tr, te = (f0m.track_gpu(dev(x), sr, rms_gate=gate) for x in (ref, est))
    want = f0m.melody_metrics(tr.f0.cpu().numpy(), tr.voiced.cpu().numpy(), te.f0.cpu().numpy(), te.voiced.cpu().numpy())
    print(want)
    assert {k: results[0][k] for k in f0m.MELODY} == want
    assert want["RPA"] < want["RCA"] == 1.0 and want["VR"] == 1.0
    assert all(f"{k}={want[k]:.3f}" in said and f"Mean {k:4s}: {want[k]:.3f}" in said for k in f0m.MELODY)
