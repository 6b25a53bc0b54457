"""Framewise BSS-eval on the host (evaluate.bss_eval_sources_framewise, metrics_from_waveforms_framewise, the
--frame_window / --frame_hop / --frames_csv options) against the whole-signal bss_eval_sources on each window's slices,
the argument checks of the framewise C entry points, and the window rules of the device="gpu" entry points (silent window,
bad pivot, which solves an output needs) with the one library-calling function replaced by numpy.  No GPU needed."""
import csv
import ctypes
import warnings

import numpy as np
import pytest
import torch
from scipy.linalg import LinAlgError, cholesky, solve_triangular

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import evaluate as ev
from test_bss_gram import assert_bss_close, corr
from test_gpu_bss_framewise import assert_frames_close, track_with_silence, two_sources

FLEN = 16                                            # the window rules do not depend on flen; short filters keep numpy fast


def sources(n, seed, K=2):
    rng = np.random.default_rng(seed)
    refs = rng.standard_normal((K, n))
    ests = refs + 0.3 * rng.standard_normal((K, n))
    ests[-1] += 0.2 * refs[0]
    return refs, ests


@pytest.mark.parametrize("n,window,hop,nwin", [(100, 10, 10, 10), (100, 30, 15, 5), (100, 50, 50, 2), (100, 20, 30, 3),
                                               (100, 10, 45, 3), (110, 100, 10, 2), (100, 100, 10, 1), (99, 100, 10, 0),
                                               (10, 11, 1, 0), (5, 20, 3, -4)])
def test_frame_count(n, window, hop, nwin):
    assert ev.frame_count(n, window, hop) == nwin == int(np.floor((n - window + hop) / hop))


@pytest.mark.parametrize("window,hop,perm", [(300, 200, False), (300, 200, True), (200, 300, False), (250, 250, False)])
def test_each_window_is_bss_eval_of_its_slices(window, hop, perm):
    refs, ests = sources(900, 1)
    got = ev.bss_eval_sources_framewise(refs, ests, window, hop, perm, FLEN)
    nwin = ev.frame_count(900, window, hop)
    assert nwin >= 2
    for k in range(nwin):
        want = ev.bss_eval_sources(refs[:, k * hop:k * hop + window], ests[:, k * hop:k * hop + window], perm, FLEN)
        for g, w in zip(got, want):
            assert g.shape == (2, nwin)
            np.testing.assert_array_equal(g[:, k], w)


@pytest.mark.parametrize("window,hop", [(900, 100), (1000, 50), (600, 400)])
def test_fewer_than_two_windows_is_the_whole_signal(window, hop):
    refs, ests = sources(900, 2)
    got = ev.bss_eval_sources_framewise(refs, ests, window, hop, flen=FLEN)
    want = ev.bss_eval_sources(refs, ests, False, FLEN)
    for g, w in zip(got, want):
        assert g.shape == (2, 1)
        np.testing.assert_array_equal(g[:, 0], w)


def test_silent_windows_are_nan_and_partly_silent_ones_are_not():
    refs, ests = sources(1000, 3)
    refs[1, 200:400] = 0.0                           # window 1: a silent reference
    ests[0, 600:800] = 0.0                           # window 3: a silent estimate
    refs[0, 850:1000] = 0.0                          # window 4: partly silent
    got = ev.bss_eval_sources_framewise(refs, ests, 200, 200, flen=FLEN)
    for g in got:
        assert np.isnan(g[:, [1, 3]]).all() and not np.isnan(g[:, [0, 2, 4]]).any()
    want = ev.bss_eval_sources(refs[:, 800:], ests[:, 800:], False, FLEN)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g[:, 4], w)


def test_one_dimensional_inputs():
    refs, ests = sources(800, 4, K=1)
    got = ev.bss_eval_sources_framewise(refs[0], ests[0], 200, 100, flen=FLEN)
    want = ev.bss_eval_sources_framewise(refs, ests, 200, 100, flen=FLEN)
    for g, w in zip(got, want):
        assert g.shape == (1, 7)
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("kwargs", [dict(window=0), dict(hop=0), dict(window=-5), dict(hop=2.5), dict(window=True),
                                    dict(hop=None)])
def test_bad_window_or_hop_raises(kwargs):
    refs, ests = sources(400, 5)
    args = {"window": 100, "hop": 100, **kwargs}
    with pytest.raises(ValueError):
        ev.bss_eval_sources_framewise(refs, ests, args["window"], args["hop"], flen=FLEN)


@pytest.mark.parametrize("ref_shape,est_shape", [((2, 400), (2, 399)), ((2, 400), (1, 400)), ((2, 2, 100), (2, 2, 100))])
def test_bad_shapes_raise(ref_shape, est_shape):
    with pytest.raises(ValueError):
        ev.bss_eval_sources_framewise(np.ones(ref_shape), np.ones(est_shape), 100, 100, flen=FLEN)


def vocal_track(n, seed):
    rng = np.random.default_rng(seed)
    vocal = np.convolve(rng.standard_normal(n), [1.0, 0.5])[:n]
    acc = 0.5 * rng.standard_normal(n)
    est = vocal + 0.1 * acc + 0.05 * rng.standard_normal(n)
    return vocal + acc, vocal, est


def test_metrics_framewise_nsdr_is_sdr_minus_mixture_sdr():
    mix, vocal, est = vocal_track(4 * 1500, 6)
    vocal[1500:3000] = 0.0                           # window 1: silent vocal -> all NaN
    mix[4500:] = 0.0                                 # window 3: silent mixture -> NSDR NaN
    fr = ev.metrics_from_waveforms_framewise(mix, vocal, est, 1500, 1500)
    assert set(fr) == {"SDR", "SIR", "SAR", "NSDR", "start"}
    assert list(fr["start"]) == [0, 1500, 3000, 4500]
    sdr, sir, sar, _ = ev.bss_eval_sources_framewise(np.stack([vocal, mix - vocal]), np.stack([est, mix - est]), 1500, 1500)
    sdr_mix = ev.bss_eval_sources_framewise(vocal[None], mix[None], 1500, 1500)[0][0]
    for k, want in (("SDR", sdr[0]), ("SIR", sir[0]), ("SAR", sar[0]), ("NSDR", sdr[0] - sdr_mix)):
        np.testing.assert_array_equal(fr[k], want)
    assert np.isnan(fr["SDR"][1]) and not np.isnan(fr["SDR"][[0, 2]]).any()
    assert list(np.isnan(fr["NSDR"])) == [False, True, False, True]


def test_metrics_framewise_one_window_is_the_whole_track():
    mix, vocal, est = vocal_track(3000, 7)
    fr = ev.metrics_from_waveforms_framewise(mix, vocal, est, 2000, 2000)
    sdr, sir, sar, _ = ev.bss_eval_sources(np.stack([vocal, mix - vocal]), np.stack([est, mix - est]), False)
    assert fr["SDR"].shape == (1,) and fr["SDR"][0] == sdr[0] and list(fr["start"]) == [0]


def test_frame_summary_ignores_nan():
    frames = {"SDR": np.array([1.0, np.nan, 3.0, 5.0]), "SIR": np.array([2.0, np.nan, 4.0, 6.0]),
              "SAR": np.array([0.0, np.nan, 0.0, 1.0]), "NSDR": np.array([np.nan, np.nan, np.nan, 2.0])}
    s = ev.frame_summary(frames)
    assert s == {"SDR": 3.0, "SIR": 4.0, "SAR": 0.0, "NSDR": 2.0, "frames": 3}


def test_seconds_to_samples():
    assert ev.frame_samples(1, 8192) == 8192
    assert ev.frame_samples(0.5, 44100) == 22050
    assert ev.frame_samples(0.1, 44100) == 4410
    assert ev.frame_samples(0.25, 10) == 2                 # int(round(2.5)): round half to even
    assert ev.frame_samples(1.5, 8191) == 12286            # round(12286.5)
    with pytest.raises(ValueError):
        ev.frame_samples(1e-5, 8192)


def test_cli_frame_options_parse(capsys, tmp_path):
    with pytest.raises(SystemExit):
        ev.main(["--help"])
    out = capsys.readouterr().out
    assert "--frame_window" in out and "--frame_hop" in out and "--frames_csv" in out
    base = ["--est", str(tmp_path), "--mix", str(tmp_path), "--ref", str(tmp_path)]
    for bad in (["--frame_window", "0"], ["--frame_window", "-1"], ["--frame_hop", "1"], ["--frames_csv", "f.csv"],
                ["--frame_window", "1", "--frame_hop", "0"]):
        with pytest.raises(SystemExit) as ex:
            ev.main(base + bad)
        assert ex.value.code == 2


def write_tracks(tmp_path, seconds=3, sr=8192):
    """a.wav, b.wav (vocal silent in its middle second) and c.wav (estimate all zeros): 3 s at 8192 Hz."""
    from scipy.io import wavfile
    for d in ("est", "mix", "ref"):
        (tmp_path / d).mkdir()
    for i, name in enumerate(("a.wav", "b.wav", "c.wav")):
        mix, vocal, est = vocal_track(seconds * sr, 40 + i)
        if name == "b.wav":
            vocal[sr:2 * sr] = 0.0
            est[sr:2 * sr] = 0.0
        if name == "c.wav":
            est[:] = 0.0
        for d, x in (("mix", mix), ("ref", vocal), ("est", est)):
            wavfile.write(tmp_path / d / name, sr, (0.3 * x).astype(np.float32))
    return ["--est", str(tmp_path / "est"), "--mix", str(tmp_path / "mix"), "--ref", str(tmp_path / "ref")]


def test_cli_framewise_medians_frames_and_csv(tmp_path, capsys):
    argv = write_tracks(tmp_path)
    out, frames = tmp_path / "r.csv", tmp_path / "f.csv"
    res = ev.main(argv + ["--out_csv", str(out), "--frame_window", "1", "--frames_csv", str(frames)])
    printed = capsys.readouterr().out
    assert [r["track"] for r in res] == ["a", "b"]
    assert "[Error] No valid frame in c.wav" in printed and "frames=2/3" in printed
    with open(out) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == ["track", "SDR", "SIR", "SAR", "NSDR", "frames"]
    assert [r["frames"] for r in rows] == ["3", "2"]
    for r in rows:
        fr = ev.compute_frame_metrics_for_track(*(str(tmp_path / d / f"{r['track']}.wav") for d in ("mix", "ref", "est")), 1.0)
        for k in ev.METRICS:
            assert float(r[k]) == float(np.nanmedian(fr[k])), (r["track"], k)
    with open(frames) as f:
        frows = list(csv.DictReader(f))
    assert list(frows[0]) == ["track", "frame", "start_s", "SDR", "SIR", "SAR", "NSDR"]
    assert [(r["track"], r["frame"], float(r["start_s"])) for r in frows] == \
        [(t, str(i), float(i)) for t in ("a", "b") for i in range(3)]
    assert frows[4]["SDR"] == "nan"


def test_cli_without_frame_window_is_unchanged(tmp_path, capsys):
    argv = write_tracks(tmp_path, seconds=1)
    out = tmp_path / "r.csv"
    res = ev.main(argv + ["--out_csv", str(out)])
    printed = capsys.readouterr().out
    with open(out) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == ["track", "SDR", "SIR", "SAR", "NSDR"]
    lines = []
    for r, row in zip(res, rows):
        want = ev.compute_metrics_for_track(*(str(tmp_path / d / f"{r['track']}.wav") for d in ("mix", "ref", "est")))
        assert r == {"track": row["track"], **want} and all(float(row[k]) == want[k] for k in ev.METRICS)
        lines.append(f"{r['track'][:20]}:\tSDR={want['SDR']:.3f} dB,\tSIR={want['SIR']:.3f} dB,\tSAR={want['SAR']:.3f} dB,"
                     f"\tNSDR={want['NSDR']:.3f} dB")
    assert "frames" not in printed and "Frame results" not in printed
    for line in lines:
        assert line + "\n" in printed


@pytest.fixture(scope="module")
def lib():
    from svs_unet_pytorch_amd import build
    build.build_lib(verbose=False)
    return _lib.lib()


def ints(v, t=ctypes.c_int):
    return (t * len(v))(*v)


def test_framewise_workspace_queries_are_zero_for_invalid_arguments(lib):
    pairs = ints([0, 1, 512, 1, 1, 1])
    assert lib.svs_bss_corr_windows_workspace_bytes(8192, 10, 2, pairs) > 0
    for args in [(0, 10, 2, pairs), (8192, 0, 2, pairs), (8192, 10, 0, pairs), (8192, 10, 17, pairs), (8192, 10, 2, None),
                 (8192, 10, 1, ints([0, 0, 513])), (8192, 10, 1, ints([0, 0, 0])), (8192, 10, 1, ints([-1, 0, 5])),
                 (8192, 1 << 40, 2, pairs)]:
        assert lib.svs_bss_corr_windows_workspace_bytes(*args) == 0, args
    one = lib.svs_bss_solve_workspace_bytes(2, 512, 2)
    assert lib.svs_bss_solve_batched_workspace_bytes(250, 2, 512, 2) >= 250 * one > 1 << 31    # 64-bit batch bases
    for args in [(0, 2, 512, 2), (4, 3, 512, 2), (4, 0, 512, 2), (4, 2, 513, 2), (4, 2, 0, 2), (4, 2, 512, 0),
                 (4, 2, 512, 17), (1 << 40, 2, 512, 2)]:
        assert lib.svs_bss_solve_batched_workspace_bytes(*args) == 0, args


def test_framewise_entry_points_reject_invalid_calls_without_touching_the_gpu(lib):
    fake = ctypes.c_void_p(16)
    pairs = ints([0, 1, 512, 1, 1, 1])
    err = lib.svs_last_error_string
    # x, ld, nsig, n, window, hop, nwin, pairs, npairs, out, out_stride, ws, ws_bytes, stream
    assert lib.svs_bss_corr_windows(None, 1000, 2, 1000, 100, 100, 10, pairs, 2, fake, 513, fake, 1 << 30, None) == -1
    assert b"bad arguments" in err()
    assert lib.svs_bss_corr_windows(fake, 1000, 2, 1000, 100, 0, 10, pairs, 2, fake, 513, fake, 1 << 30, None) == -1
    assert b"hop = 0" in err()
    assert lib.svs_bss_corr_windows(fake, 1000, 2, 1000, 100, 100, 10, pairs, 2, fake, 512, fake, 1 << 30, None) == -1
    assert b"out_stride" in err()
    assert lib.svs_bss_corr_windows(fake, 1000, 1, 1000, 100, 100, 10, pairs, 2, fake, 513, fake, 1 << 30, None) == -1
    assert b"out of range" in err()
    assert lib.svs_bss_corr_windows(fake, 1000, 2, 1000, 100, 100, 10, pairs, 2, fake, 513, None, 0, None) == -2
    assert b"workspace too small" in err()
    g, r = ints([0, 0], ctypes.c_int64), ints([0, 0, 0, 0], ctypes.c_int64)
    # corr, nbatch, K, flen, gram_off, rhs_off, nrhs, ynorm2, status, ws, ws_bytes, stream
    assert lib.svs_bss_solve_batched(None, 2, 1, 512, g, r, 2, fake, fake, fake, 1 << 30, None) == -1
    assert lib.svs_bss_solve_batched(fake, 0, 1, 512, g, r, 2, fake, fake, fake, 1 << 30, None) == -1
    assert lib.svs_bss_solve_batched(fake, 2, 3, 512, g, r, 2, fake, fake, fake, 1 << 30, None) == -1
    assert lib.svs_bss_solve_batched(fake, 2, 1, 512, ints([0, -8], ctypes.c_int64), r, 2, fake, fake, fake, 1 << 30,
                                     None) == -1
    assert b"negative offset (system 1)" in err()
    assert lib.svs_bss_solve_batched(fake, 2, 1, 512, g, r, 2, fake, fake, fake, 1000, None) == -2
    assert b"workspace too small" in err()


# ---- the window rules of the GPU path, with numpy in place of the library ---------------------

class NumpyProjections:
    """float64 numpy stand-in for evaluate._gpu_window_projections: per window and solve the block-Toeplitz Gram matrix from
    lagged correlations, scipy's Cholesky and a forward solve, |y|^2.  A matrix that scipy cannot factor, or a (window,
    solve) in force_bad, has status 1."""

    def __init__(self, force_bad=()):
        self.force_bad = set(force_bad)

    def __call__(self, sig, window, hop, nwin, solves, energies, flen, ws_budget):
        x = sig.numpy()
        d = np.arange(flen)[None, :] - np.arange(flen)[:, None]
        energy = np.empty((nwin, len(energies)))
        ys = [np.zeros((nwin, len(ests))) for _, ests in solves]
        status = [np.zeros(nwin, dtype=np.int32) for _ in solves]
        for w in range(nwin):
            s = x[:, w * hop:w * hop + window]
            energy[w] = [corr(s[e], s[e], 1)[0] for e in energies]
            for q, (refs, ests) in enumerate(solves):
                c = {(i, j): corr(s[i], s[j], flen) for i in refs for j in refs}
                G = np.block([[np.where(d >= 0, c[i, j][np.abs(d)], c[j, i][np.abs(d)]) for j in refs] for i in refs])
                D = np.stack([np.concatenate([corr(s[e], s[i], flen) for i in refs]) for e in ests], axis=1)
                try:
                    if (w, q) in self.force_bad:
                        raise LinAlgError("forced")
                    Y = solve_triangular(cholesky(G, lower=True), D, lower=True)
                    ys[q][w] = (Y * Y).sum(axis=0)
                except LinAlgError:
                    status[q][w] = 1
        return energy, ys, status


def host_f64(x):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(dtype=torch.float64)


def use_numpy_projections(mp, force_bad=()):
    mp.setattr(ev, "_gpu_window_projections", NumpyProjections(force_bad))
    mp.setattr(ev, "_device_f64", host_f64)


def fallback_warnings(rec):
    """The RuntimeWarnings of a recorded call, all of which must be the fallback warning."""
    got = [str(r.message) for r in rec if issubclass(r.category, RuntimeWarning)]
    assert all("falls back to the numpy path" in m for m in got), got
    return got


SR = 8192


def test_gpu_window_rules_silent_windows_are_nan(monkeypatch):
    mix, vocal, est = track_with_silence(7, seed=50)
    want = ev.metrics_from_waveforms_framewise(mix, vocal, est, SR, SR)
    assert list(np.isnan(want["SDR"])) == [False, True, False, False, False, False, True]      # silent vocal; all silent
    use_numpy_projections(monkeypatch)
    monkeypatch.setattr(ev, "bss_eval_sources", None)                        # no fallback: not called at all
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = ev.metrics_from_waveforms_framewise(mix, vocal, est, SR, SR, device="gpu")
    assert_frames_close(got, want)


@pytest.mark.parametrize("perm", [False, True])
def test_gpu_window_rules_sources_framewise(perm, monkeypatch):
    refs, ests = two_sources(24000, 53)
    want = ev.bss_eval_sources_framewise(refs, ests, 4000, 2000, perm, 64)
    assert np.isnan(want[0][:, 4]).all() and not np.isnan(want[0][:, 3]).any()
    use_numpy_projections(monkeypatch)
    monkeypatch.setattr(ev, "bss_eval_sources", None)
    got = ev.bss_eval_sources_framewise_gpu(refs, ests, 4000, 2000, perm, 64)
    for g, w in zip(got, want):
        assert g.shape == w.shape == (2, 11) and g.dtype == np.float64
        assert np.array_equal(np.isnan(g), np.isnan(w))
    for k in np.flatnonzero(~np.isnan(want[0][0])):
        assert_bss_close(tuple(v[:, k] for v in got), tuple(v[:, k] for v in want))


@pytest.mark.parametrize("solve,numpy_calls", [(2, 1), (1, 1), (0, 2)])
def test_gpu_window_rules_bad_pivot_rescores_that_window_with_numpy(solve, numpy_calls, monkeypatch):
    """SDR / SIR / SAR need all three solves of a window, the mixture's SDR only solve 0 (the vocal alone)."""
    mix, vocal, est = track_with_silence(7, seed=50)
    want = ev.metrics_from_waveforms_framewise(mix, vocal, est, SR, SR)
    use_numpy_projections(monkeypatch)
    clean = ev.metrics_from_waveforms_framewise(mix, vocal, est, SR, SR, device="gpu")
    use_numpy_projections(monkeypatch, force_bad=[(3, solve)])
    calls, numpy_bss = [], ev.bss_eval_sources

    def spy(refs, ests, *args, **kwargs):
        calls.append((np.array(refs), np.array(ests)))
        return numpy_bss(refs, ests, *args, **kwargs)

    monkeypatch.setattr(ev, "bss_eval_sources", spy)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = ev.metrics_from_waveforms_framewise(mix, vocal, est, SR, SR, device="gpu")
    assert len(fallback_warnings(rec)) == 1
    others = np.arange(7) != 3
    for k in ev.METRICS:
        assert np.array_equal(got[k][others], clean[k][others], equal_nan=True), k
    for k in ("SDR", "SIR", "SAR"):
        assert got[k][3] == want[k][3], k                                      # bitwise the numpy result
    sl = slice(3 * SR, 4 * SR)
    sdr_mix = want["SDR"][3] - want["NSDR"][3] if solve == 0 else clean["SDR"][3] - clean["NSDR"][3]
    assert abs(got["NSDR"][3] - (want["SDR"][3] - sdr_mix)) <= 1e-9
    assert len(calls) == numpy_calls
    assert np.array_equal(calls[0][0], np.stack([vocal[sl], (mix - vocal)[sl]]))
    assert np.array_equal(calls[0][1], np.stack([est[sl], (mix - est)[sl]]))
    if numpy_calls == 2:
        assert got["NSDR"][3] == want["NSDR"][3]
        assert np.array_equal(calls[1][0], vocal[None, sl]) and np.array_equal(calls[1][1], mix[None, sl])


def test_gpu_window_rules_one_window_is_the_whole_track(monkeypatch):
    mix, vocal, est = track_with_silence(7, seed=50)
    n = mix.size
    assert list(ev.bss_eval_sources(np.stack([vocal, mix - vocal]), np.stack([est, mix - est]))[3]) == [0, 1]
    want = ev.metrics_from_waveforms(mix, vocal, est)
    use_numpy_projections(monkeypatch)
    monkeypatch.setattr(ev, "bss_eval_sources", None)
    whole = ev.metrics_from_waveforms(mix, vocal, est, device="gpu")
    for window, hop in [(n, n), (n + 5, 100), (2 * n, SR)]:
        fr = ev.metrics_from_waveforms_framewise(mix, vocal, est, window, hop, device="gpu")
        assert list(fr["start"]) == [0]
        for k in ev.METRICS:
            assert fr[k].shape == (1,) and fr[k][0] == whole[k], (k, window, hop)
    assert whole.keys() == want.keys() and all(isinstance(v, float) for v in whole.values())
    for k in want:
        assert abs(whole[k] - want[k]) <= 1e-3, (k, whole[k], want[k])


def test_gpu_window_rules_silent_reference_falls_back_to_numpy(monkeypatch):
    rng = np.random.default_rng(4)
    refs = np.stack([np.zeros(8000), rng.standard_normal(8000)])
    ests = np.stack([0.01 * rng.standard_normal(8000), refs[1] + 0.1 * rng.standard_normal(8000)])
    use_numpy_projections(monkeypatch)
    with np.errstate(all="ignore"):
        with pytest.warns(RuntimeWarning, match="falls back to the numpy path"):
            got = ev.bss_eval_sources_gpu(refs, ests)
        want = ev.bss_eval_sources(refs, ests)
    for g, w in zip(got, want):
        assert g.shape == (2,)
        np.testing.assert_array_equal(g, w)
    assert np.issubdtype(got[3].dtype, np.integer)
