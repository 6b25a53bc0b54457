"""The YIN f0 tracker, the host half (no GPU): the three entry points' declarations, the argument rules that hold before any device
work, the float64 definition f0.yin_reference on known tones, silence and noise, the pick on hand-made d' rows, the melody measures
on hand-made tracks, and the command lines.

Pitch bounds.  The error of YIN on a clean tone is a property of the method -- the parabola through three samples of d' at a short
period, the window's average over a moving pitch -- not of the arithmetic, so only a measurement can set it: MEASURED below holds the
largest error in cents over the frames of each signal, measured with yin_reference on the CPU against the signal's own instantaneous
frequency at the frame's time (2026-10-21; DESIGN.md section 26 records them), and the bound is 1.5 times that.
tests/test_gpu_f0.py holds the device to the same bounds plus 0.01 cent."""
import math

import numpy as np
import pytest

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import f0 as f0m

NAMES = ("svs_f0_cmnd", "svs_f0_pick", "svs_f0_track")
SR = 8192


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def err(lib):
    return lib.svs_last_error_string().decode()


def test_symbols_are_declared_bound_and_exported(lib):
    syms = _lib.header_symbols()
    for name in NAMES:
        assert name in syms and name in _lib._SIGS and hasattr(lib, name), name


# ------------------------------------------------------------------------------------------------
# argument rules, before any launch
# ------------------------------------------------------------------------------------------------
# svs_f0_track(x, rows, n, ld_row, W, tau_min, tau_max, hop, first_frame, n_frames, threshold, rms_gate, sr, f0, ap, rms, voiced)
GOOD = dict(x=64, rows=2, n=1000, ld_row=1000, W=252, tau_min=8, tau_max=127, hop=82, first_frame=0, n_frames=8, threshold=0.15, rms_gate=0.0,
            sr=8192.0, f0=64, ap=64, rms=64, voiced=64)                # frames 0..7 need 7 * 82 + 379 = 953 samples


def track_call(lib, **change):
    a = {**GOOD, **change}
    return lib.svs_f0_track(a["x"], a["rows"], a["n"], a["ld_row"], a["W"], a["tau_min"], a["tau_max"], a["hop"], a["first_frame"], a["n_frames"],
                            a["threshold"], a["rms_gate"], a["sr"], a["f0"], a["ap"], a["rms"], a["voiced"], None)


@pytest.mark.parametrize("change,msg", [
    (dict(rows=0), "rows must be in 1..64"),
    (dict(rows=65), "rows must be in 1..64"),
    (dict(W=0), "W must be in 1..4096"),
    (dict(W=4097, n=10000, ld_row=10000), "W must be in 1..4096"),
    (dict(tau_max=2049, n=10000, ld_row=10000), "tau_max must be in 1..2048"),
    (dict(tau_max=0), "tau_max must be in 1..2048"),
    (dict(tau_min=127), "tau_min must be in 1..tau_max - 1"),
    (dict(tau_min=0), "tau_min must be in 1..tau_max - 1"),
    (dict(hop=0), "hop must be at least 1"),
    (dict(first_frame=-1), "must not be negative"),
    (dict(n_frames=-1), "must not be negative"),
    (dict(n=-1), "n must not be negative"),
    (dict(n_frames=9), "only whole frames are formed"),
    (dict(first_frame=1), "only whole frames are formed"),
    (dict(n=952, ld_row=952), "only whole frames are formed"),
    (dict(ld_row=999), "ld_row must be at least n"),
    (dict(threshold=0.0), "threshold must be positive and finite"),
    (dict(threshold=math.nan), "threshold must be positive and finite"),
    (dict(rms_gate=-1.0), "rms_gate must be finite and not negative"),
    (dict(sr=0.0), "sr must be positive and finite"),
    (dict(sr=math.inf), "sr must be positive and finite"),
    (dict(x=None), "null pointer"),
    (dict(f0=None), "null pointer"),
    (dict(rms=None), "null pointer"),
    (dict(voiced=None), "null pointer"),
    (dict(x=66), "x must be 4-byte aligned"),
    (dict(ap=66), "4-byte aligned"),
])
def test_track_refuses_before_any_launch(lib, change, msg):
    assert track_call(lib, **change) == -1
    assert msg in err(lib) and err(lib).startswith("svs_f0_track:"), err(lib)


# svs_f0_cmnd(x, rows, n, ld_row, W, tau_max, hop, first_frame, n_frames, dprime, rms)
@pytest.mark.parametrize("args,msg", [
    ((64, 65, 1000, 1000, 252, 127, 82, 0, 8, 64, 64), "rows must be in 1..64"),
    ((64, 2, 1000, 1000, 4097, 127, 82, 0, 0, 64, 64), "W must be in 1..4096"),
    ((64, 2, 1000, 1000, 252, 2049, 82, 0, 0, 64, 64), "tau_max must be in 1..2048"),
    ((64, 2, 1000, 1000, 252, 127, 0, 0, 8, 64, 64), "hop must be at least 1"),
    ((64, 2, 1000, 1000, 252, 127, 82, 0, 9, 64, 64), "only whole frames are formed"),
    ((64, 2, 1000, 999, 252, 127, 82, 0, 8, 64, 64), "ld_row must be at least n"),
    ((64, 2, 1000, 1000, 252, 127, 82, 0, 8, None, 64), "null pointer"),
    ((None, 2, 1000, 1000, 252, 127, 82, 0, 8, 64, 64), "null pointer"),
    ((64, 2, 1000, 1000, 252, 127, 82, 0, 8, 66, 64), "4-byte aligned"),
])
def test_cmnd_refuses_before_any_launch(lib, args, msg):
    assert lib.svs_f0_cmnd(*args, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_f0_cmnd:"), err(lib)


# svs_f0_pick(dprime, count, tau_min, tau_max, threshold, rms, rms_gate, sr, f0, ap, voiced)
@pytest.mark.parametrize("args,msg", [
    ((64, 10, 8, 2049, 0.15, 64, 0.0, 8192.0, 64, 64, 64), "tau_max must be in 1..2048"),
    ((64, 10, 127, 127, 0.15, 64, 0.0, 8192.0, 64, 64, 64), "tau_min must be in 1..tau_max - 1"),
    ((64, 10, 8, 127, -0.1, 64, 0.0, 8192.0, 64, 64, 64), "threshold must be positive and finite"),
    ((64, 10, 8, 127, 0.15, 64, math.inf, 8192.0, 64, 64, 64), "rms_gate must be finite and not negative"),
    ((64, 10, 8, 127, 0.15, 64, 0.0, -1.0, 64, 64, 64), "sr must be positive and finite"),
    ((64, -1, 8, 127, 0.15, 64, 0.0, 8192.0, 64, 64, 64), "frame count must not be negative"),
    ((None, 10, 8, 127, 0.15, 64, 0.0, 8192.0, 64, 64, 64), "null pointer"),
    ((64, 10, 8, 127, 0.15, 64, 0.0, 8192.0, 64, 64, None), "null pointer"),
    ((64, 10, 8, 127, 0.15, 66, 0.0, 8192.0, 64, 64, 64), "4-byte aligned"),
])
def test_pick_refuses_before_any_launch(lib, args, msg):
    assert lib.svs_f0_pick(*args, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_f0_pick:"), err(lib)


def test_no_frames_launch_nothing(lib):
    assert track_call(lib, n_frames=0, x=None, f0=None, ap=None, rms=None, voiced=None) == 0
    assert lib.svs_f0_cmnd(None, 2, 1000, 1000, 252, 127, 82, 0, 0, None, None, None) == 0
    assert lib.svs_f0_pick(None, 0, 8, 127, 0.15, None, 0.0, 8192.0, None, None, None, None) == 0


def test_geometry_and_its_rules():
    g = f0m.geometry(8192)
    assert (g.tau_min, g.tau_max, g.W, g.hop, g.span) == (8, 127, 254, 82, 381) and g.threshold == 0.15 and g.rms_gate == 0.0
    g = f0m.geometry(44100, fmin=50, W=1358)
    assert (g.tau_min, g.tau_max, g.W, g.hop, g.span) == (44, 882, 1358, 441, 2240)
    g = f0m.geometry(100000, fmin=48.83, fmax=50000, W=4096, hop=4096)
    assert (g.tau_min, g.tau_max) == (2, 2048)                       # sr / fmin rounds up to the limit, tau_min clamps to 2
    assert f0m.geometry(50, fmin=1, fmax=40).hop == 1                # round(sr / 100) = 0 -> at least 1
    assert f0m.frame_count(381, 381, 82) == 1 and f0m.frame_count(381 + 81, 381, 82) == 1 and f0m.frame_count(381 + 82, 381, 82) == 2
    assert np.array_equal(f0m.frame_times(f0m.geometry(8192), 2, first_frame=3), (np.array([3, 4]) * 82 + 190.5) / 8192)
    for kw, msg in ((dict(sr=44100, fmin=20), "longest lag tau_max of 2205"), (dict(sr=8192, fmin=3000), "no lag range"),
                    (dict(sr=8192, W=4097), "window W"), (dict(sr=8192, W=0), "window W"), (dict(sr=8192, W=12.5), "window W"),
                    (dict(sr=8192, hop=0), "hop must be"), (dict(sr=8192, threshold=0), "threshold"), (dict(sr=8192, rms_gate=-1), "rms_gate"),
                    (dict(sr=0), "sr must be"), (dict(sr=8192, fmin=0), "fmin and fmax")):
        with pytest.raises(ValueError, match=msg):
            f0m.geometry(**kw)
    with pytest.raises(ValueError, match="one frame needs span"):
        f0m.yin_reference(np.zeros(380, np.float32), 8192)
    with pytest.raises(ValueError, match="rows must be in 1..64"):
        f0m.yin_reference(np.zeros((65, 400), np.float32), 8192)
    with pytest.raises(ValueError, match="outside the signal's 1 frames"):
        f0m.yin_reference(np.zeros(400, np.float32), 8192, first_frame=1, n_frames=1)


def test_python_entry_points_check_before_any_device_work(tmp_path, capsys):
    import torch
    from svs_unet_pytorch_amd import evaluate, separate, streaming
    with pytest.raises(ValueError, match="window W"):
        f0m.track_gpu(torch.zeros(8), 8192, W=5000)                  # before the tensor is looked at
    with pytest.raises(ValueError, match="device tensor"):
        f0m.track_gpu(torch.zeros(800), 8192)
    with pytest.raises(ValueError, match="device tensor"):
        f0m.cmnd_gpu(torch.zeros(800), 252, 127, 82)
    with pytest.raises(TypeError, match="float32 device tensor"):
        f0m.pick_gpu(torch.zeros(4, 128), 8192, 8)
    with pytest.raises(ValueError, match="not \\['window'\\]"):
        f0m.check_options({"window": 3})
    assert f0m.check_options(True) == {} and f0m.check_options({"fmin": 80}) == {"fmin": 80}
    with pytest.raises(ValueError, match="tracks the vocal stem"):
        streaming.separate_waveform(None, torch.zeros(4), vocal_solo=False, f0=True)
    with pytest.raises(ValueError, match="tracks the vocal stem"):
        streaming.separate_to_wav(None, "unused.wav", "unused_out.wav", vocal_solo=False, f0_csv_path="unused.csv")
    with pytest.raises(ValueError, match="f0= takes"):
        streaming.separate_to_wav(None, "unused.wav", "unused_out.wav", f0={"rate": 3})
    with pytest.raises(SystemExit) as e:
        separate.main(["--model_path", "none.pth", "--src", "a.wav", "--tar", "o.wav", "--vocal_solo", "0", "--f0_csv", str(tmp_path / "t.csv")])
    assert e.value.code == 2 and "--f0_csv tracks the vocal stem, and --vocal_solo 0 writes none" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--est", "e", "--mix", "m", "--ref", "r", "--rms_gate_db", "-40"])
    assert e.value.code == 2 and "--rms_gate_db belongs to --melody" in capsys.readouterr().err
    for tool, flag in ((separate, "--f0_csv"), (evaluate, "--melody")):
        with pytest.raises(SystemExit) as e:
            tool.main(["--help"])
        assert e.value.code == 0 and flag in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------
# the definition on known signals
# ------------------------------------------------------------------------------------------------
def tones():
    """name -> (instantaneous frequency in Hz as a function of the time in seconds, samples at 8,192 Hz): harmonic tones with 1 / k
    amplitudes up to 3.5 kHz (f0.harmonic_tone)."""
    out = {f"tone {hz:g} Hz": ((lambda t, hz=hz: np.full_like(t, hz)), SR // 2) for hz in (82.41, 220.0, 440.0, 987.77)}
    out["vibrato 330 Hz"] = ((lambda t: 330.0 * 2.0 ** ((50.0 / 1200.0) * np.sin(2.0 * np.pi * 5.0 * t))), SR)      # 5 Hz, +-50 cents
    out["glide 200-400 Hz"] = ((lambda t: 200.0 + 100.0 * t), 2 * SR)                                               # over 2 s
    return out


# the largest error in cents over the frames, measured with yin_reference (module docstring)
MEASURED = {"tone 82.41 Hz": 1.450760, "tone 220 Hz": 3.264645, "tone 440 Hz": 2.328862, "tone 987.77 Hz": 20.378494,
            "vibrato 330 Hz": 13.511067, "glide 200-400 Hz": 6.192380}


def cents_off(track, freq):
    return 1200.0 * np.abs(np.log2(np.asarray(track.f0, dtype=np.float64) / freq(np.asarray(track.time))))


@pytest.mark.parametrize("name", list(MEASURED))
def test_reference_pitch_on_known_tones(name):
    freq, n = tones()[name]
    x = f0m.harmonic_tone(freq(np.arange(n) / SR), SR)
    track, dp = f0m.yin_reference(x, SR)
    frames = 1 + (n - 381) // 82
    assert track.f0.shape == track.voiced.shape == track.ap.shape == track.rms.shape == track.time.shape == (frames,)
    assert track.f0.dtype == track.ap.dtype == track.rms.dtype == dp.dtype == np.float32 and track.voiced.dtype == np.int32
    assert dp.shape == (frames, 128) and (dp[:, 0] == 1).all()
    worst = float(cents_off(track, freq).max())
    print(f"{name}: {frames} frames, {int(track.voiced.sum())} voiced, largest error {worst:.6f} cents (measured {MEASURED[name]}, "
          f"bound {1.5 * MEASURED[name]:.6f})")
    assert (track.voiced == 1).all()                                 # every frame of these signals is voiced
    assert worst <= 1.5 * MEASURED[name]
    assert (track.ap < 0.15).all() and np.allclose(track.rms, np.sqrt(np.mean(x[:254].astype(np.float64) ** 2)), rtol=0.2)


def test_white_noise_is_unvoiced():
    """At threshold 0.15 white noise has no lag whose d' comes near the threshold: seed 0 gives 0 voiced frames of 96 (at most 2 % are
    allowed), and every frame goes through the argmin branch."""
    x = (0.1 * np.random.default_rng(0).standard_normal(SR)).astype(np.float32)
    track, dp = f0m.yin_reference(x, SR)
    assert track.voiced.shape == (96,) and int(track.voiced.sum()) == 0 <= 0.02 * 96
    assert (track.ap >= 0.15).all() and np.array_equal(track.ap, dp[:, 8:].min(axis=1))
    assert np.isfinite(track.f0).all() and (track.f0 >= SR / 128.0).all() and (track.f0 <= SR / 7.0).all()


def test_silence():
    track, dp = f0m.yin_reference(np.zeros(1000, np.float32), SR)
    assert (dp == 1.0).all() and (track.voiced == 0).all() and (track.ap == 1.0).all() and (track.rms == 0.0).all()
    assert (track.f0 == np.float32(SR / 8)).all()                    # tau = tau_min, delta = 0: finite
    gated, _ = f0m.yin_reference(f0m.harmonic_tone(np.full(1000, 220.0), SR, level=1e-4), SR, rms_gate=f0m.gate_from_db(-50.0))
    loud, _ = f0m.yin_reference(f0m.harmonic_tone(np.full(1000, 220.0), SR), SR, rms_gate=f0m.gate_from_db(-50.0))
    assert (gated.voiced == 0).all() and (loud.voiced == 1).all()    # the gate alone silences a clean quiet tone


def test_rows_and_pieces_of_the_reference():
    x = np.stack([f0m.harmonic_tone(np.full(900, hz), SR, level=lv) for hz, lv in ((220.0, 0.25), (330.0, 0.01))])
    both, dp = f0m.yin_reference(x, SR)
    for r in range(2):
        one, dp1 = f0m.yin_reference(x[r], SR)
        assert all(np.array_equal(a[r], b) for a, b in zip(both[1:], one[1:])) and np.array_equal(dp[r], dp1)
    piece, dpp = f0m.yin_reference(x, SR, first_frame=2, n_frames=3)
    assert all(np.array_equal(a[..., 2:5], b) for a, b in zip(both, piece)) and np.array_equal(dp[:, 2:5], dpp)


# ------------------------------------------------------------------------------------------------
# the pick
# ------------------------------------------------------------------------------------------------
def test_pick_on_hand_made_rows():
    tau_min, tau_max = 2, 9
    rows = np.ones((5, 10), np.float32)
    rows[0, 3:7] = [0.14, 0.10, 0.05, 0.30]      # first under the threshold at 3, walks down to 5; a = .10, b = .05, c = .30
    rows[1, 4], rows[1, 7] = 0.5, 0.5            # nothing under the threshold: the FIRST index of the minimum, found = 0
    rows[2, 9] = 0.01                            # at tau_max: no tau + 1, delta = 0
    rows[3, 1], rows[3, 2], rows[3, 3] = 0.0, 0.1, 0.2   # at tau_min = 2: tau - 1 = 1 is allowed, but q = 0 - 0.2 + 0.2 = 0: delta = 0
    rows[4, 5:8] = 0.12                          # a flat run under the threshold: no step on equality, a = 1, b = c = .12
    f0, ap, voiced, tau = f0m.pick_reference(rows, 1000.0, tau_min, tau_max, 0.15)
    assert tau.tolist() == [5, 4, 9, 2, 5] and voiced.tolist() == [1, 0, 1, 1, 1]
    assert np.array_equal(ap, rows[np.arange(5), tau])
    a, b, c = (float(np.float32(v)) for v in (0.10, 0.05, 0.30))
    d0 = 0.5 * (a - c) / (a - 2 * b + c)
    a4, b4 = 1.0, float(np.float32(0.12))
    d4 = 0.5 * (a4 - b4) / (a4 - 2 * b4 + b4)    # 0.5: the parabola through (1, .12, .12) has its vertex half a sample on
    want = [1000.0 / (5 + d0), 1000.0 / 4, 1000.0 / 9, 1000.0 / 2, 1000.0 / (5 + d4)]
    assert -1 < d0 < 0 and d4 == 0.5 and np.array_equal(f0, np.array(want, np.float32))
    gated = f0m.pick_reference(rows, 1000.0, tau_min, tau_max, 0.15, rms=np.array([0.5, 0.5, 0.01, 0.02, 0.0], np.float32), rms_gate=0.02)[2]
    assert gated.tolist() == [1, 0, 0, 1, 0]     # found and rms >= rms_gate, the gate's own level included
    with pytest.raises(ValueError, match="tau_max \\+ 1"):
        f0m.pick_reference(rows, 1000.0, 2, 10)


# ------------------------------------------------------------------------------------------------
# melody measures
# ------------------------------------------------------------------------------------------------
def test_melody_metrics_on_hand_made_tracks():
    # 2^(1/24) is irrational: "exactly 50 cents" is the pair whose ratio IS the double 2^(50/1200) that melody_metrics compares with,
    # which a reference that is a power of two makes exact (128 r / 128 = r)
    r50 = 2.0 ** (50.0 / 1200.0)
    ref_f0 = np.array([100.0, 100.0, 128.0, 100.0, 100.0, 0.0, 0.0, 55.0])
    ref_v = np.array([1, 1, 1, 1, 1, 0, 0, 0])
    est_f0 = np.array([100.0, 200.0, 128.0 * r50, 100.0 * 2.0 ** (51.0 / 1200.0), 100.0, 300.0, 0.0, 55.0])
    est_v = np.array([1, 1, 1, 1, 0, 1, 0, 0])
    assert est_f0[2] / ref_f0[2] == r50          # frame 2 at EXACTLY 50 cents
    # frame: 0 right; 1 an octave up (chroma only); 2 at 50 cents (counts: the bound is included); 3 at 51 cents (does not); 4 the right
    # pitch on a frame the estimate calls unvoiced (RPA and RCA count it, VR and OA do not); 5 a false alarm; 6, 7 unvoiced in both
    #   VR  = {0, 1, 2, 3} of the 5 voiced                      = 4 / 5
    #   VFA = {5} of the 3 unvoiced                             = 1 / 3
    #   RPA = {0, 2, 4} of the 5 voiced                         = 3 / 5
    #   RCA = {0, 1, 2, 4} of the 5 voiced                      = 4 / 5
    #   OA  = ({0, 2} voiced in both and in tune + {6, 7}) / 8  = 4 / 8
    m = f0m.melody_metrics(ref_f0, ref_v, est_f0, est_v)
    assert m == {"VR": 4 / 5, "VFA": 1 / 3, "RPA": 3 / 5, "RCA": 4 / 5, "OA": 4 / 8} and tuple(m) == f0m.MELODY
    est_f0[2] = np.nextafter(est_f0[2], np.inf)  # one step past 50 cents: out
    m = f0m.melody_metrics(ref_f0, ref_v, est_f0, est_v)
    assert m == {"VR": 4 / 5, "VFA": 1 / 3, "RPA": 2 / 5, "RCA": 3 / 5, "OA": 3 / 8}
    est_f0[2] = 128.0 / r50 / 2.0                # 50 cents flat and an octave down: chroma only (128 / (128 / r50) rounds to r50)
    assert ref_f0[2] / (2.0 * est_f0[2]) == r50
    m = f0m.melody_metrics(ref_f0, ref_v, est_f0, est_v)
    assert m == {"VR": 4 / 5, "VFA": 1 / 3, "RPA": 2 / 5, "RCA": 4 / 5, "OA": 3 / 8}
    # an octave DOWN and two octaves up fold as well
    m = f0m.melody_metrics([200.0, 200.0], [1, 1], [100.0, 800.0], [1, 1])
    assert m == {"VR": 1.0, "VFA": 0.0, "RPA": 0.0, "RCA": 1.0, "OA": 0.0}
    # no voiced reference frame: VR, RPA and RCA are over an empty set, 0; VFA = 1 of 3; OA = the 2 frames unvoiced in both, of 3
    m = f0m.melody_metrics([0.0, 0.0, 0.0], [0, 0, 0], [100.0, 100.0, 100.0], [0, 1, 0])
    assert m == {"VR": 0.0, "VFA": 1 / 3, "RPA": 0.0, "RCA": 0.0, "OA": 2 / 3}
    # no unvoiced reference frame: VFA over an empty set, 0; and no frame at all: everything 0
    assert f0m.melody_metrics([100.0], [1], [100.0], [1]) == {"VR": 1.0, "VFA": 0.0, "RPA": 1.0, "RCA": 1.0, "OA": 1.0}
    assert f0m.melody_metrics([], [], [], []) == dict.fromkeys(f0m.MELODY, 0.0)
    with pytest.raises(ValueError, match="one value per frame"):
        f0m.melody_metrics([1.0, 2.0], [1, 1], [1.0], [1])


# ------------------------------------------------------------------------------------------------
# the command lines on the CPU
# ------------------------------------------------------------------------------------------------
def test_cli_on_the_cpu(tmp_path, capsys):
    from scipy.io import wavfile
    x = f0m.harmonic_tone(np.full(SR, 220.0), SR)
    src, dst = str(tmp_path / "tone.wav"), str(tmp_path / "tone.csv")
    wavfile.write(src, SR, np.stack([np.round(x * 32767.0), np.round(0.5 * x * 32767.0)], axis=1).astype(np.int16))     # 1 s of stereo
    f0m.main(["--src", src, "--csv", dst, "--device", "cpu"])
    assert f"{dst}: 96 frames, 96 voiced" in capsys.readouterr().out
    lines = open(dst).read().splitlines()
    assert lines[0] == "time,f0,voiced,aperiodicity,rms" == f0m.CSV_HEADER and len(lines) == 1 + 96
    cols = np.array([[float(v) for v in line.split(",")] for line in lines[1:]])
    assert np.allclose(cols[:, 0], (np.arange(96) * 82 + 190.5) / SR, atol=1e-6)
    assert (1200.0 * np.abs(np.log2(cols[:, 1] / 220.0)) <= 1.5 * MEASURED["tone 220 Hz"]).all()
    assert (cols[:, 2] == 1).all() and (cols[:, 3] < 0.15).all() and (cols[:, 4] > 0.05).all()
    # the same numbers as the definition on the mean of the channels as the file stores them
    data = wavfile.read(src)[1].astype(np.float64) / 32768.0
    want = f0m.yin_reference(data.mean(axis=1).astype(np.float32), SR)[0]
    assert np.allclose(cols[:, 1], want.f0, rtol=0, atol=1e-4) and np.allclose(cols[:, 4], want.rms, rtol=1e-6)
    # a folder, other parameters, the gate
    folder = tmp_path / "in"
    folder.mkdir()
    wavfile.write(str(folder / "a.wav"), SR, x)
    wavfile.write(str(folder / "b.wav"), SR, (1e-4 * x).astype(np.float32))
    out = tmp_path / "out"
    f0m.main(["--src", str(folder), "--csv", str(out), "--device", "cpu", "--fmin", "100", "--fmax", "500", "--window", "200", "--hop", "100",
              "--threshold", "0.1", "--rms_gate_db", "-50"])
    said = capsys.readouterr().out
    frames = 1 + (SR - (200 + 82)) // 100
    assert f"a.csv: {frames} frames, {frames} voiced" in said and f"b.csv: {frames} frames, 0 voiced" in said
    assert len(open(out / "a.csv").read().splitlines()) == 1 + frames
    with pytest.raises(SystemExit) as e:
        f0m.main(["--src", src, "--csv", dst, "--device", "cpu", "--fmin", "1"])
    assert e.value.code == 2 and "longest lag" in capsys.readouterr().err


def test_evaluate_melody_on_the_cpu(tmp_path, capsys):
    """--melody adds the five columns to the line, the means and the csv; without it none of them appears."""
    import csv

    from scipy.io import wavfile

    from svs_unet_pytorch_amd import evaluate
    n = SR
    t = np.arange(n) / SR
    ref = f0m.harmonic_tone(np.where(t < 0.75, 220.0, 330.0), SR)
    ref[int(0.5 * n):int(0.75 * n)] = 0.0                            # a silent passage: unvoiced under the gate
    est = f0m.harmonic_tone(np.where(t < 0.25, 220.0, np.where(t < 0.75, 440.0, 330.0)), SR)      # an octave up from 0.25 s to 0.75 s
    accomp = (0.05 * np.random.default_rng(2).standard_normal(n)).astype(np.float32)
    for folder, x in (("ref", ref), ("est", est), ("mix", ref + accomp)):
        (tmp_path / folder).mkdir()
        wavfile.write(str(tmp_path / folder / "song.wav"), SR, x)
    base = ["--est", str(tmp_path / "est"), "--mix", str(tmp_path / "mix"), "--ref", str(tmp_path / "ref")]
    evaluate.main(base)
    plain = capsys.readouterr().out
    assert "SDR=" in plain and not any(k + "=" in plain or f"Mean {k:4s}" in plain for k in f0m.MELODY)
    out_csv = str(tmp_path / "r.csv")
    results = evaluate.main(base + ["--melody", "--out_csv", out_csv])
    said = capsys.readouterr().out
    gate = f0m.gate_from_db(-50.0)
    tr, te = (f0m.yin_reference(x, SR, rms_gate=gate)[0] for x in (ref, est))
    want = f0m.melody_metrics(tr.f0, tr.voiced, te.f0, te.voiced)
    print(want)
    assert {k: results[0][k] for k in f0m.MELODY} == want
    assert 0 < want["RPA"] < want["RCA"] <= 1 and 0 < want["VFA"] and int(tr.voiced.sum()) < tr.voiced.size
    line = [l for l in said.splitlines() if l.startswith("song")][0]
    assert line.startswith([l for l in plain.splitlines() if l.startswith("song")][0])         # the BSS-eval part is unchanged
    assert all(f",\t{k}={want[k]:.3f}" in line for k in f0m.MELODY) and all(f"Mean {k:4s}: {want[k]:.3f}" in said for k in f0m.MELODY)
    rows = list(csv.DictReader(open(out_csv)))
    assert list(rows[0])[-5:] == list(f0m.MELODY) and all(float(rows[0][k]) == want[k] for k in f0m.MELODY)
    evaluate.main(base + ["--melody", "--rms_gate_db", "-200"])      # the gate off: the silent passage is no longer unvoiced as a whole
    assert "VR=" in capsys.readouterr().out
