"""Smoothing the pitch track on the device (-m gpu; csrc/f0_smooth.hip) against the definition of f0.py: the candidate rule on hand-made
rows and on the device's own d', the fused candidates launch against the staged pair and against svs_f0_track, the Viterbi decode
against the sequential recursion for every chunk, the smoothed track end to end on the 6 dB tone of tests/test_f0_smooth_host.py, and
the command lines.

Everything here is equality of bits: the candidates are selections and one fp64 division chain rounded once (the pick's), the decode is
integer arithmetic.  The metric bounds are the host file's.  Shapes: about 1 s of signal at one geometry per lags-per-lane class of
the kernel (2, 4 and 8: tau_max 127, 160, 882), frame counts around every chunk boundary, 1,000 frames, and 2^16 gated frames for the
sums of INF."""
import functools

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import f0 as f0m
from test_f0_smooth_host import (HAND_TAU_MAX, HAND_TAU_MIN, SR, VALUE_GEOMETRY, hand_made_rows, noisy_tone, synthetic_candidates,
                                 value_bounds)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def same(got, want):
    return all(np.array_equal(g.cpu().numpy(), w) and g.cpu().numpy().dtype == w.dtype for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------
# svs_f0_dips
# ------------------------------------------------------------------------------------------------
def test_dips_on_hand_made_rows():
    rows, want_tau = hand_made_rows()
    got = f0m.dips_gpu(dev(rows), 8192.0, HAND_TAU_MIN)
    want = f0m.candidates_reference(rows, 8192.0, HAND_TAU_MIN, HAND_TAU_MAX)
    assert got[0].shape == (7, 7) and got[3].shape == (7,)
    assert got[3].cpu().tolist() == [len(w) for w in want_tau]
    assert all(got[0][r, :len(w)].cpu().tolist() == w for r, w in enumerate(want_tau))
    assert same(got, want)                                           # tau, f0, ap and count, bit for bit; zeros in the empty slots
    again = f0m.dips_gpu(dev(rows), 8192.0, HAND_TAU_MIN)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    lead = f0m.dips_gpu(dev(rows).reshape(7, 1, -1), 8192.0, HAND_TAU_MIN)          # any leading shape
    assert lead[0].shape == (7, 1, 7) and torch.equal(lead[1].reshape(7, 7), got[1])


def test_dips_on_the_devices_own_dprime():
    x, _, _ = noisy_tone(0)
    g = f0m.geometry(SR, **VALUE_GEOMETRY)
    dp, _ = f0m.cmnd_gpu(dev(x), g.W, g.tau_max, g.hop)
    got = f0m.dips_gpu(dp, g.sr, g.tau_min)
    want = f0m.candidates_reference(dp.cpu().numpy(), g.sr, g.tau_min, g.tau_max)
    assert want[3].min() >= 1 and want[3].max() == 7 and (want[3] < 7).any()         # full and partly empty frames
    assert same(got, want)


# ------------------------------------------------------------------------------------------------
# svs_f0_candidates
# ------------------------------------------------------------------------------------------------
# one geometry per lags-per-lane class: (sr, fmin, fmax, W, tau_max, hop, samples of about 1 s)
CLASSES = {
    "2 lags per lane": (8192, 65, 1000, 252, 127, 82, 8192),
    "4 lags per lane, disjoint frames": (16000, 100, 4000, 64, 160, 300, 16000),
    "8 lags per lane": (44100, 50, 1000, 1358, 882, 441, 44100),
}


@pytest.mark.parametrize("name", list(CLASSES))
def test_candidates_is_the_staged_pair_and_the_raw_track(name):
    sr, fmin, fmax, W, tau_max, hop, n = CLASSES[name]
    g = f0m.geometry(sr, fmin, fmax, W, hop, rms_gate=1e-3)
    assert g.tau_max == tau_max
    rng = np.random.default_rng(len(name))
    freq = np.linspace(180.0, 300.0, n)
    tone = f0m.harmonic_tone(freq, sr).astype(np.float64)
    level = np.sqrt(np.mean(tone ** 2))
    x = np.stack([tone + 0.5 * level * rng.standard_normal(n), 1e-4 * tone, 0.1 * rng.standard_normal(n)]).astype(np.float32)
    for rows, first in ((3, 3), (1, 5)):
        xd = dev(x[:rows] if rows > 1 else x[0])
        kw = dict(fmin=fmin, fmax=fmax, W=W, hop=hop, rms_gate=1e-3, first_frame=first)
        track, cand = f0m.candidates_gpu(xd, sr, **kw)
        raw = f0m.track_gpu(xd, sr, **kw)
        assert all(torch.equal(a, b) for a, b in zip(track, raw))                         # f0, voiced, ap, rms: svs_f0_track's bits
        dp, _ = f0m.cmnd_gpu(xd, g.W, g.tau_max, g.hop, first_frame=first)
        staged = f0m.dips_gpu(dp, g.sr, g.tau_min)
        assert cand[0].shape == dp.shape[:-1] + (7,) and cand[3].shape == dp.shape[:-1] and cand[0].dtype == cand[3].dtype == torch.int32
        assert all(torch.equal(a, b) for a, b in zip(cand, staged))                       # svs_f0_cmnd then svs_f0_dips
        whole = f0m.candidates_gpu(xd, sr, **{**kw, "first_frame": 0})[1]                 # a piece is the whole call's frames
        assert all(torch.equal(a, b[..., first:, :] if i < 3 else b[..., first:]) for i, (a, b) in enumerate(zip(cand, whole)))


# ------------------------------------------------------------------------------------------------
# svs_f0_viterbi
# ------------------------------------------------------------------------------------------------
GATE = 0.5


@functools.lru_cache(maxsize=None)
def buffers(T, zero=False):
    """64 rows of synthetic candidates and the reference decode of every row (computed once per T)."""
    tau, ap, count, rms = synthetic_candidates(64, T, 1000 + T, ap_zero=zero)
    costs = dict.fromkeys(f0m.COSTS, 0) if zero else {}
    state, cost = f0m.viterbi_reference(tau, ap, count, rms, f0m.cents_table(SR, 127), 8, GATE, **costs)
    return (tau, ap, count, rms), state, cost, costs


def decode(T, rows, chunk, zero=False):
    (tau, ap, count, rms), want, want_cost, costs = buffers(T, zero)
    cents = f0m.cents_gpu(SR, 127, DEV)
    state, cost = f0m.viterbi_gpu(dev(tau[:rows]), dev(ap[:rows]), dev(count[:rows]), dev(rms[:rows]), cents, 8, GATE, chunk=chunk, **costs)
    assert state.dtype == torch.int32 and cost.dtype == torch.int64 and state.shape == (rows, T) and cost.shape == (rows,)
    return state.cpu().numpy(), cost.cpu().numpy(), want[:rows], want_cost[:rows]


@pytest.mark.parametrize("chunk", f0m.CHUNKS)
def test_viterbi_is_the_sequential_recursion(chunk):
    for T in (1, 2, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 1000):
        for rows in (1, 3, 64):
            state, cost, want, want_cost = decode(T, rows, chunk)
            assert np.array_equal(cost, want_cost), (chunk, T, rows)
            assert np.array_equal(state, want), (chunk, T, rows, int((state != want).sum()))
    want = buffers(1000)[1]
    assert (want == 7).any() and (want < 7).any() and len(np.unique(want)) == 8         # every state is on some path


def test_viterbi_is_the_same_for_every_chunk_and_keeps_the_tie_rules():
    for T, zero in ((1000, False), (389, False), (200, True)):
        got = [decode(T, 64, chunk, zero) for chunk in f0m.CHUNKS]
        for state, cost, want, want_cost in got:
            assert np.array_equal(state, got[0][0]) and np.array_equal(cost, got[0][1])
            assert np.array_equal(state, want) and np.array_equal(cost, want_cost)
    state, cost, _, _ = decode(200, 64, 64, True)
    rms = buffers(200, True)[0][3]
    assert (cost == 0).all() and (state[rms >= GATE] == 0).all() and (state[rms < GATE] == 7).all()     # every cost zero: the smallest index
    one = f0m.viterbi_gpu(*(dev(b[0]) for b in buffers(53)[0]), f0m.cents_gpu(SR, 127, DEV), 8, GATE, chunk=16)       # without the row axis
    assert one[0].shape == (53,) and one[1].shape == () and np.array_equal(one[0].cpu().numpy(), buffers(53)[1][0])


@pytest.mark.parametrize("chunk", [16, 128])
def test_viterbi_carries_inf_over_65536_gated_frames(chunk):
    T = 1 << 16
    tau, ap, count, _ = synthetic_candidates(1, T, 7)
    rms = np.zeros((1, T), np.float32)                               # every frame under the gate: INF on all voiced states, every frame
    state, cost = f0m.viterbi_gpu(dev(tau), dev(ap), dev(count), dev(rms), f0m.cents_gpu(SR, 127, DEV), 8, GATE, chunk=chunk)
    assert int(cost[0]) == T * f0m.COSTS["unvoiced_cost"] and bool((state == 7).all())


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_smoothed_track_end_to_end(seed):
    x, ref_f0, ref_voiced = noisy_tone(seed)
    g = f0m.geometry(SR, **VALUE_GEOMETRY)
    xd = dev(x)
    raw = f0m.track_gpu(xd, SR, **VALUE_GEOMETRY)
    got = f0m.track_gpu(xd, SR, smooth=True, **VALUE_GEOMETRY)
    dp, rms = f0m.cmnd_gpu(xd, g.W, g.tau_max, g.hop)
    f0, ap, voiced, state, cost = f0m.smooth_reference(dp.cpu().numpy(), rms.cpu().numpy(), g.sr, g.tau_min, g.tau_max, g.threshold, g.rms_gate)
    assert got.f0.shape == (297,) and got.voiced.dtype == torch.int32
    assert same((got.f0, got.ap, got.voiced), (f0, ap, voiced))      # the definition on the device's own d', bit for bit
    assert torch.equal(got.rms, raw.rms) and torch.equal(got.time, raw.time) and torch.equal(got.rms, rms)
    assert all(torch.equal(a, b) for a, b in zip(got, f0m.track_gpu(xd, SR, smooth=dict(f0m.COSTS), **VALUE_GEOMETRY)))
    assert all(torch.equal(a, b) for a, b in zip(raw, f0m.track_gpu(xd, SR, smooth=None, **VALUE_GEOMETRY)))
    value_bounds(ref_f0, ref_voiced, (raw.f0.cpu().numpy(), raw.voiced.cpu().numpy()), (got.f0.cpu().numpy(), got.voiced.cpu().numpy()),
                 f"device, 6 dB, seed {seed}")
    if seed == 0:                                                    # rows decode independently, with other costs too
        both = f0m.track_gpu(dev(np.stack([x, noisy_tone(1)[0]])), SR, smooth={"octave_cost": 0}, **VALUE_GEOMETRY)
        alone = f0m.track_gpu(xd, SR, smooth={"octave_cost": 0}, **VALUE_GEOMETRY)
        assert both.f0.shape == (2, 297) and torch.equal(both.f0[0], alone.f0) and torch.equal(both.voiced[0], alone.voiced)
        want = f0m.smooth_reference(dp.cpu().numpy(), rms.cpu().numpy(), g.sr, g.tau_min, g.tau_max, smooth={"octave_cost": 0})
        assert same((alone.f0, alone.ap, alone.voiced), want[:3])


# ------------------------------------------------------------------------------------------------
# the command lines
# ------------------------------------------------------------------------------------------------
def test_separate_cli_writes_the_smoothed_track(tmp_path, capsys):
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import separate, streaming
    from svs_unet_pytorch_amd.model import UNet
    torch.manual_seed(1234)
    model = UNet().to(DEV).eval()
    ck = str(tmp_path / "svs_random.pth")
    torch.save({"model_state_dict": model.state_dict()}, ck)
    n = int(1.5 * 44100)
    tone = f0m.harmonic_tone(np.linspace(200.0, 260.0, n), 44100)
    noise = (0.05 * np.random.default_rng(7).standard_normal((2, n))).astype(np.float32)
    src = str(tmp_path / "mixture.wav")
    wavfile.write(src, 44100, np.clip(np.round(np.stack([tone + noise[0], 0.6 * tone + noise[1]]).T * 20000), -32768, 32767).astype(np.int16))
    plain, with_raw, with_smooth = (str(tmp_path / f) for f in ("plain.wav", "raw.wav", "smooth.wav"))
    raw_csv, smooth_csv = str(tmp_path / "raw.csv"), str(tmp_path / "smooth.csv")
    base = ["--model_path", ck, "--src", src]
    separate.main(base + ["--tar", plain])
    separate.main(base + ["--tar", with_raw, "--f0_csv", raw_csv])
    separate.main(base + ["--tar", with_smooth, "--f0_csv", smooth_csv, "--f0_smooth"])
    assert "pitch frames" in capsys.readouterr().out
    assert open(plain, "rb").read() == open(with_raw, "rb").read() == open(with_smooth, "rb").read()     # the wav bytes do not change
    # without the flag the csv is byte for byte track_gpu's raw track of the vocal stem (f0=True), with it the smoothed one
    for f0_option, path in ((True, raw_csv), ({"smooth": True}, smooth_csv)):
        report = {}
        streaming.separate_to_wav(model, src, str(tmp_path / "again.wav"), f0=f0_option, report=report)
        want = str(tmp_path / "want.csv")
        f0m.write_csv(want, report["f0"])
        assert open(path).read() == open(want).read()
    lines_raw, lines_smooth = open(raw_csv).read().splitlines(), open(smooth_csv).read().splitlines()
    assert lines_raw[0] == lines_smooth[0] == f0m.CSV_HEADER and len(lines_raw) == len(lines_smooth) > 50
    a, b = (np.array([[float(v) for v in line.split(",")] for line in lines[1:]]) for lines in (lines_raw, lines_smooth))
    assert np.array_equal(a[:, [0, 4]], b[:, [0, 4]]) and np.isfinite(b).all()            # time and rms are the raw track's


def test_evaluate_melody_smoothed_on_the_device(tmp_path, capsys):
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import evaluate
    x, _, _ = noisy_tone(0)
    clean, _, _ = noisy_tone(0, 40.0)
    for folder, y in (("ref", clean), ("est", x), ("mix", x)):
        (tmp_path / folder).mkdir()
        wavfile.write(str(tmp_path / folder / "song.wav"), SR, np.array(y))
    results = evaluate.main(["--est", str(tmp_path / "est"), "--mix", str(tmp_path / "mix"), "--ref", str(tmp_path / "ref"), "--melody",
                             "--f0_smooth", "--device", "gpu"])
    said = capsys.readouterr().out
    gate = f0m.gate_from_db(f0m.MELODY_GATE_DB)
    t = f0m.track_gpu(dev(np.stack([clean, x])), SR, rms_gate=gate, smooth=True)
    f0, voiced = t.f0.cpu().numpy(), t.voiced.cpu().numpy()
    want = f0m.melody_metrics(f0[0], voiced[0], f0[1], voiced[1])
    print(want)
    assert {k: results[0][k] for k in f0m.MELODY} == want
    assert all(f"{k}={want[k]:.3f}" in said and f"Mean {k:4s}: {want[k]:.3f}" in said for k in f0m.MELODY)       # the five measures
