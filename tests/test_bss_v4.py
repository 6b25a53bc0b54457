"""BSS-eval v4 on the host (evaluate.bss_eval_v4, image_metrics_from_waveforms_v4, --mode v4): the float64 definition against
bss_eval_images on one frame and against an independent least-squares restatement on several, the frame rules, the
device="gpu" driver with its one library-calling function replaced by numpy, the declarations and argument checks of the
svs_bss_img_filters_batched / svs_bss_project_frames entry points, and the command line.  No GPU needed."""
import csv
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import evaluate as ev
from test_bss_images import host_f64, stereo_track, write_stereo_tracks

# (flen, window, hop, n, nchan): the full filter length; a flen and a window that no tile size divides, overlapping frames
# and ignored trailing samples; one channel; the degenerate filter
SHAPES = [(512, 3001, 3001, 12781, 2), (37, 1000, 600, 5000, 2), (64, 900, 900, 3700, 1), (1, 257, 100, 1000, 2)]


def v4_case(n, nchan, seed=0):
    """(references, estimates), each (2, n, nchan): references of white noise through [1, .6, .3, .1]; channel c of estimate
    j = 0.8 of its reference channel 5 samples late + 0.1 of the source's other channel + 0.15 of the other source's channel
    c + 0.05 noise, so every one of the seven sums of a frame is a sizeable share of the frame's energy and the delay puts
    energy into the filters' tail."""
    rng = np.random.default_rng(seed)
    white = rng.standard_normal((2, n + 3, nchan))
    ref = sum(g * white[:, 3 - k:n + 3 - k] for k, g in enumerate((1.0, 0.6, 0.3, 0.1)))
    noise = rng.standard_normal((2, n, nchan))
    est = np.empty_like(ref)
    for j in range(2):
        for c in range(nchan):
            late = np.concatenate([np.zeros(5), ref[j, :-5, c]])
            est[j, :, c] = 0.8 * late + 0.1 * ref[j, :, (c + 1) % nchan] + 0.15 * ref[1 - j, :, c] + 0.05 * noise[j, :, c]
    return ref, est


def delayed(rows, flen, length):
    """(length, R * flen): column i * flen + tau is row i delayed by tau samples, zero outside the row."""
    out = np.zeros((length, rows.shape[0] * flen))
    for i, r in enumerate(rows):
        for tau in range(flen):
            m = min(len(r), length - tau)
            out[tau:tau + m, i * flen + tau] = r[:m]
    return out


def lstsq_v4_sums(rc, ec, window, hop, nwin, flen):
    """The seven sums (nwin, nsrc, 7) restated without evaluate.py: filters by least squares on the matrix of delayed whole
    references, frames by a product with the matrix of the frame's delayed references."""
    nsrc, nchan, n = rc.shape
    allc = rc.reshape(nsrc * nchan, n)
    pad = lambda x, k: np.concatenate([x, np.zeros(x.shape[:-1] + (k,))], axis=-1)
    sums = np.zeros((nwin, nsrc, 7))
    for j in range(nsrc):
        target = pad(ec[j], flen - 1).T
        c_one = np.linalg.lstsq(delayed(rc[j], flen, n + flen - 1), target, rcond=None)[0]
        c_all = np.linalg.lstsq(delayed(allc, flen, n + flen - 1), target, rcond=None)[0]
        for w in range(nwin):
            sl = slice(w * hop, w * hop + window)
            length = rc[j, :, sl].shape[1] + flen - 1
            p1 = (delayed(rc[j, :, sl], flen, length) @ c_one).T
            pa = (delayed(allc[:, sl], flen, length) @ c_all).T
            s, e = pad(rc[j, :, sl], flen - 1), pad(ec[j, :, sl], flen - 1)
            sums[w, j] = [np.sum(v ** 2) for v in (s, e - s, p1 - s, p1, pa - p1, pa, e - pa)]
    return sums


def assert_v4_close(got, want, tol):
    assert len(got) == len(want) == 4
    for name, g, w in zip(("sdr", "isr", "sir", "sar"), got, want):
        assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), (name, g, w)
        inf = np.isinf(w)                                    # one source: no interference, SIR is +inf in both
        assert np.array_equal(g[inf], w[inf]), (name, g, w)
        ok = ~np.isnan(w) & ~inf
        assert np.all(np.abs(w[ok]) < 60.0) and np.all(np.abs(g[ok] - w[ok]) <= tol), (name, g, w)


# ---- the definition -------------------------------------------------------------------------

@pytest.mark.parametrize("nchan", [1, 2])
def test_one_frame_is_bss_eval_images_without_permutation(nchan):
    ref, est = v4_case(4000, nchan, seed=1)
    want = ev.bss_eval_images(ref, est, compute_permutation=False, flen=32)[:4]
    for window, hop in [(4000, 4000), (3999, 3), (9000, 100)]:                    # frame_count 1, 1 and < 1
        got = ev.bss_eval_v4(ref, est, window, hop, flen=32)
        assert all(g.shape == (2, 1) for g in got)
        assert_v4_close(tuple(g[:, 0] for g in got), want, 1e-9)


def test_one_source_has_no_interference():
    ref, est = v4_case(3000, 2, seed=2)
    sdr, isr, sir, sar = ev.bss_eval_v4(ref[:1], est[:1], 1000, 1000, flen=16)
    assert sdr.shape == (1, 3) and np.all(sir == np.inf) and np.all(np.isfinite(sar)) and np.all(np.isfinite(isr))


@pytest.mark.parametrize("flen,window,hop,n,nchan", SHAPES[1:])
def test_definition_matches_a_least_squares_restatement(flen, window, hop, n, nchan):
    ref, est = v4_case(n, nchan, seed=flen)
    nwin = ev.frame_count(n, window, hop)
    got = ev.bss_eval_v4(ref, est, window, hop, flen=flen)
    sums = lstsq_v4_sums(ref.transpose(0, 2, 1), est.transpose(0, 2, 1), window, hop, nwin, flen)
    want = tuple(np.array([[ev._v4_figures(sums[w, j])[k] for w in range(nwin)] for j in range(2)]) for k in range(4))
    assert got[0].shape == (2, nwin)
    assert_v4_close(got, want, 1e-8)


def test_filters_are_track_wide_sdr_is_the_framewise_sdr_and_sir_is_not():
    flen, window, hop, n, nchan = SHAPES[1]
    ref, est = v4_case(n, nchan, seed=flen)
    sdr, isr, sir, sar = ev.bss_eval_v4(ref, est, window, hop, flen=flen)
    fw = ev.bss_eval_images_framewise(ref, est, window, hop, flen=flen)
    assert np.all(np.abs(sdr - fw[0]) <= 1e-9)                                   # no filter enters the SDR
    assert np.all(np.abs(sir - fw[2]) > 0.05)                                    # per-frame filters fit each frame better:
    assert np.all(fw[3] > sar)                                                   # less is left over as artifacts


def test_a_silent_frame_is_nan_and_only_that_frame():
    ref, est = v4_case(4000, 2, seed=3)
    ref[1, 1000:2000] = 0.0
    got = ev.bss_eval_v4(ref, est, 1000, 1000, flen=16)
    for g in got:
        assert g.shape == (2, 4) and np.isnan(g[:, 1]).all() and not np.isnan(g[:, [0, 2, 3]]).any()
    est[0, 3000:, :] = 0.0                                                       # a silent estimate as well
    got = ev.bss_eval_v4(ref, est, 1000, 1000, flen=16)
    assert list(np.isnan(got[0][0])) == [False, True, False, True]
    ref[1, 1000:2000, 0] = 1e-3                                                  # one channel sounding: not silent
    assert list(np.isnan(ev.bss_eval_v4(ref, est, 1000, 1000, flen=16)[0][0])) == [False, False, False, True]


def test_two_d_input_is_a_one_channel_image():
    ref, est = v4_case(3000, 1, seed=4)
    a = ev.bss_eval_v4(ref[:, :, 0], est[:, :, 0], 1000, 500, flen=16)
    b = ev.bss_eval_v4(ref, est, 1000, 500, flen=16)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_bad_arguments_raise():
    ref, est = v4_case(1000, 2, seed=5)
    with pytest.raises(ValueError, match="no permutation search"):
        ev.bss_eval_v4(ref, est, 500, 500, flen=8, compute_permutation=True)
    with pytest.raises(ValueError, match="same shape"):
        ev.bss_eval_v4(ref, est[:, :, :1], 500, 500, flen=8)
    with pytest.raises(ValueError, match="window"):
        ev.bss_eval_v4(ref, est, 0, 500, flen=8)
    with pytest.raises(ValueError):
        ev.bss_eval_v4(np.ones(100), np.ones(100), 50, 50, flen=8)


def test_project_images_is_the_two_factored_halves():
    ref, est = v4_case(2000, 2, seed=6)
    rows = ref.transpose(0, 2, 1).reshape(4, -1)
    C = ev._projection_filters(rows, est[0].T, 16)
    assert C.shape == (16, 4, 2)
    np.testing.assert_array_equal(ev._apply_filters(C, rows), ev._project_images(rows, est[0].T, 16))


# ---- the GPU driver, with numpy in place of the library ----------------------------------------

class NumpyV4Sums:
    """float64 numpy stand-in for evaluate._gpu_v4_sums, from lstsq_v4_sums.  force_bad: the status it reports."""

    def __init__(self, force_bad=0):
        self.force_bad = force_bad
        self.calls = 0

    def __call__(self, sig, window, hop, nwin, nsrc, nchan, flen, energies, crosses):
        self.calls += 1
        x = sig.numpy()
        R, n = nsrc * nchan, x.shape[1]
        sums = lstsq_v4_sums(x[:R].reshape(nsrc, nchan, n), x[R:2 * R].reshape(nsrc, nchan, n), window, hop, nwin, flen)
        fr = [x[:, w * hop:w * hop + window] for w in range(nwin)]
        energy = np.array([[np.sum(s[e] * s[e]) for e in energies] for s in fr]).reshape(nwin, len(energies))
        cross = np.array([[np.sum(s[a] * s[b]) for a, b in crosses] for s in fr]).reshape(nwin, len(crosses))
        status = np.zeros(nsrc + (nsrc == 2), dtype=np.int32)
        status[-1] = self.force_bad
        return sums, energy, cross, status


def use_numpy_sums(mp, force_bad=0):
    stand_in = NumpyV4Sums(force_bad)
    mp.setattr(ev, "_gpu_v4_sums", stand_in)
    mp.setattr(ev, "_device_f64", host_f64)
    return stand_in


@pytest.mark.parametrize("nsrc", [1, 2])
@pytest.mark.parametrize("flen,window,hop,n,nchan", SHAPES[1:])
def test_gpu_driver_reproduces_the_definition(flen, window, hop, n, nchan, nsrc, monkeypatch):
    ref, est = v4_case(n, nchan, seed=flen)
    ref, est = ref[:nsrc], est[:nsrc]
    ref[0, hop:hop + window] = 0.0                                               # frame 1 is silent
    want = ev.bss_eval_v4(ref, est, window, hop, flen=flen)
    assert np.isnan(want[0][:, 1]).all() and np.count_nonzero(np.isnan(want[0][0])) < want[0].shape[1]
    stand_in = use_numpy_sums(monkeypatch)
    monkeypatch.setattr(ev, "bss_eval_v4", None)                                 # no fallback: not called at all
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = ev.bss_eval_v4_gpu(ref, est, window, hop, flen=flen)
    assert stand_in.calls == 1
    assert_v4_close(got, want, 1e-8)


def test_gpu_driver_fewer_than_two_frames_is_the_whole_track(monkeypatch):
    ref, est = v4_case(3000, 2, seed=7)
    want = ev.bss_eval_images(ref, est, compute_permutation=False, flen=16)[:4]
    use_numpy_sums(monkeypatch)
    for window, hop in [(3000, 3000), (5000, 10)]:
        got = ev.bss_eval_v4_gpu(ref, est, window, hop, flen=16)
        assert_v4_close(tuple(g[:, 0] for g in got), want, 1e-8)


def test_gpu_driver_bad_status_scores_the_track_with_numpy(monkeypatch):
    ref, est = v4_case(3000, 2, seed=8)
    want = ev.bss_eval_v4(ref, est, 1000, 1000, flen=16)
    use_numpy_sums(monkeypatch, force_bad=3)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = ev.bss_eval_v4_gpu(ref, est, 1000, 1000, flen=16)
    msgs = [str(r.message) for r in rec if issubclass(r.category, RuntimeWarning)]
    assert len(msgs) == 1 and "falls back to the numpy path" in msgs[0]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_gpu_driver_rejects_what_the_kernels_do_not_take(monkeypatch):
    use_numpy_sums(monkeypatch)
    with pytest.raises(ValueError, match="1 or 2 sources"):
        ev.bss_eval_v4_gpu(np.ones((3, 100, 2)), np.ones((3, 100, 2)), 50, 50)
    with pytest.raises(ValueError, match="1 or 2 channels"):
        ev.bss_eval_v4_gpu(np.ones((2, 100, 3)), np.ones((2, 100, 3)), 50, 50)
    with pytest.raises(ValueError, match="no permutation search"):
        ev.bss_eval_v4_gpu(np.ones((2, 100, 2)), np.ones((2, 100, 2)), 50, 50, compute_permutation=True)
    with pytest.raises(ValueError, match="filter lengths"):
        ev.bss_eval_v4_gpu(np.ones((2, 100, 2)), np.ones((2, 100, 2)), 50, 50, flen=513)
    with pytest.raises(ValueError, match="device"):
        ev.image_metrics_from_waveforms_v4(np.ones((100, 2)), np.ones((100, 2)), np.ones((100, 2)), 50, 50, device="tpu")


@pytest.mark.parametrize("stereo", [False, True])
def test_vocal_frames_gpu_driver_matches_cpu(stereo, monkeypatch):
    monkeypatch.setattr(ev, "FILTER_LEN", 16)
    mix, vocal, est = stereo_track(4, 1200, seed=41, silent_second=2)
    if not stereo:
        mix, vocal, est = mix.mean(axis=1), vocal.mean(axis=1), est.mean(axis=1)
    want = ev.image_metrics_from_waveforms_v4(mix, vocal, est, 1200, 1200)
    assert list(np.isnan(want["SDR"])) == [False, False, True, False] == list(np.isnan(want["NSDR"]))
    direct = ev._image_sdr_direct(vocal[:1200], est[:1200])
    assert abs(want["SDR"][0] - direct) <= 1e-9
    use_numpy_sums(monkeypatch)
    got = ev.image_metrics_from_waveforms_v4(mix, vocal, est, 1200, 1200, device="gpu")
    assert set(got) == set(want) == {"SDR", "ISR", "SIR", "SAR", "NSDR", "start"}
    assert np.array_equal(got["start"], want["start"]) and list(want["start"]) == [0, 1200, 2400, 3600]
    for k in ev.IMAGE_METRICS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        ok = ~np.isnan(want[k])
        assert np.all(np.abs(got[k][ok] - want[k][ok]) <= 1e-8), (k, got[k], want[k])
    summary = ev.frame_summary(want, ev.IMAGE_METRICS)
    assert summary["frames"] == 3 and summary["SDR"] == float(np.median(want["SDR"][[0, 1, 3]]))


# ---- the C ABI -------------------------------------------------------------------------------

NEW_SYMBOLS = ("svs_bss_img_filters_batched_workspace_bytes", "svs_bss_img_filters_batched",
               "svs_bss_project_frames_workspace_bytes", "svs_bss_project_frames")


@pytest.fixture(scope="module")
def lib():
    from svs_unet_pytorch_amd import build
    build.build_lib(verbose=False)
    return _lib.lib()


def ints(v, t=ctypes.c_int):
    return (t * len(v))(*v)


def test_new_symbols_are_declared_bound_and_exported(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svs_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f" {name}(" in header and name in _lib.header_symbols() and name in _lib._SIGS, name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("bss_eval_v4", "bss_eval_v4_gpu", "image_metrics_from_waveforms_v4", "compute_v4_frame_metrics_for_track"):
        assert callable(getattr(ev, name)), name


def test_workspace_queries(lib):
    q = lib.svs_bss_img_filters_batched_workspace_bytes
    for args in [(1, 4, 512, 4), (2, 2, 512, 2), (3, 1, 37, 16)]:
        assert q(*args) == lib.svs_bss_img_solve_batched_workspace_bytes(*args) > 0
    for args in [(0, 2, 512, 2), (4, 5, 512, 2), (4, 2, 513, 2), (4, 2, 512, 17)]:
        assert q(*args) == 0, args
    q = lib.svs_bss_project_frames_workspace_bytes
    one = q(44100, 1, 1, 512)
    assert one > 0 and one % 56 == 0 and q(44100, 240, 2, 512) == 480 * one
    assert q(1, 1, 1, 1) == 56                                                  # one tile, seven sums
    assert q(240 * 44100, 1, 2, 512) > 0                                        # a whole track as one frame
    for args in [(0, 1, 1, 512), (44100, 0, 1, 512), (44100, 1, 0, 512), (44100, 1, 3, 512), (44100, 1, 2, 0),
                 (44100, 1, 2, 513), (44100, 1 << 40, 2, 512), (1 << 50, 1, 2, 512)]:
        assert q(*args) == 0, args


def test_entry_points_reject_invalid_calls_without_touching_the_gpu(lib):
    fake = ctypes.c_void_p(16)
    err = lib.svs_last_error_string
    g, r = ints([0, 0], ctypes.c_int64), ints([0, 0, 0, 0], ctypes.c_int64)
    # corr, nbatch, K, flen, gram_off, rhs_off, nrhs, ynorm2, status, skipped, coef, ws, ws_bytes, stream
    call = lib.svs_bss_img_filters_batched
    ok = [fake, 2, 1, 512, g, r, 2, fake, fake, fake, fake, fake, 1 << 30, None]
    for at in (0, 4, 5, 7, 8, 9, 10):                                           # each null pointer
        args = list(ok)
        args[at] = None
        assert call(*args) == -1, at
        assert b"bad arguments" in err()
    for at, bad in [(1, 0), (2, 0), (2, 5), (3, 0), (3, 513), (6, 0), (6, 17)]:
        args = list(ok)
        args[at] = bad
        assert call(*args) == -1, (at, bad)
    args = list(ok)
    args[12] = 1000
    assert call(*args) == -2
    assert b"svs_bss_img_filters_batched: workspace too small" in err()
    rows = ints([0, 1, 2, 3])
    # x, ld, nsig, n, window, hop, nwin, flen, nsrc, nchan, ref_rows, est_rows, coef_one, coef_all, sums, ws, ws_bytes, stream
    call = lib.svs_bss_project_frames
    ok = [fake, 5000, 8, 5000, 1000, 600, 7, 37, 2, 2, rows, ints([4, 5, 6, 7]), fake, fake, fake, fake, 1 << 30, None]
    for at in (0, 10, 11, 12, 13, 14):
        args = list(ok)
        args[at] = None
        assert call(*args) == -1, at
        assert b"bad arguments" in err()
    for at, bad in [(1, 4999), (2, 0), (3, 0), (4, 0), (6, 0), (7, 0), (7, 513), (8, 0), (8, 3), (9, 0), (9, 3)]:
        args = list(ok)
        args[at] = bad
        assert call(*args) == -1, (at, bad)
        assert b"bad arguments" in err()
    for at, bad in [(5, 0), (6, 10)]:                                           # frame 9 would start at sample 5400
        args = list(ok)
        args[at] = bad
        assert call(*args) == -1, (at, bad)
        assert b"a frame starts past" in err()
    args = list(ok)
    args[11] = ints([4, 5, 6, 8])
    assert call(*args) == -1
    assert b"out of range" in err()
    args = list(ok)
    args[15], args[16] = None, 0
    assert call(*args) == -2
    args = list(ok)
    args[16] = 100
    assert call(*args) == -2
    assert b"workspace too small" in err()


# ---- the command line ------------------------------------------------------------------------

@pytest.mark.parametrize("stereo", [False, True])
def test_cli_mode_v4_writes_five_figures_and_every_frame(stereo, tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(ev, "FILTER_LEN", 64)                                   # the plumbing, not 512 taps again
    argv = write_stereo_tracks(tmp_path) + (["--stereo"] if stereo else [])
    out, frames = tmp_path / "r.csv", tmp_path / "f.csv"
    res = ev.main(argv + ["--mode", "v4", "--out_csv", str(out), "--frames_csv", str(frames)])
    printed = capsys.readouterr().out
    tracks = ["a"] if stereo else ["a", "b"]                                    # b's estimate is mono: scored only downmixed
    assert [r["track"] for r in res] == tracks and "frames=2/2" in printed and "Mean ISR : " in printed
    with open(out) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == ["track", "SDR", "ISR", "SIR", "SAR", "NSDR", "frames"] and len(rows) == len(tracks)
    with open(frames) as f:
        frows = list(csv.DictReader(f))
    assert list(frows[0]) == ["track", "frame", "start_s", "SDR", "ISR", "SIR", "SAR", "NSDR"]
    assert len(frows) == 2 * len(tracks) and [r["start_s"] for r in frows[:2]] == ["0.0", "1.0"]    # 1 s frames by default
    paths = [str(tmp_path / d / "a.wav") for d in ("mix", "ref", "est")]
    want = ev.compute_v4_frame_metrics_for_track(*paths, stereo=stereo)
    assert want["SDR"].shape == (2,)
    for k in ev.IMAGE_METRICS:
        assert [float(r[k]) for r in frows[:2]] == list(want[k]), k
        assert float(rows[0][k]) == float(np.median(want[k])), k
    res = ev.main(argv + ["--mode", "v4", "--frame_window", "0.5", "--frame_hop", "0.25", "--frames_csv", str(frames)])
    assert "frames=7/7" in capsys.readouterr().out and len(res) == len(tracks)


def test_cli_without_the_flag_is_unchanged(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(ev, "FILTER_LEN", 64)
    argv = write_stereo_tracks(tmp_path)
    outputs = {}
    for name, extra in (("default", []), ("v3", ["--mode", "v3"])):
        out = tmp_path / f"{name}.csv"
        res = ev.main(argv + ["--out_csv", str(out)] + extra)
        outputs[name] = (capsys.readouterr().out.replace(str(out), ""), open(out, "rb").read(), res)
    assert outputs["default"][:2] == outputs["v3"][:2]
    printed, written, res = outputs["default"]
    assert "ISR" not in printed and "frames=" not in printed and written.startswith(b"track,SDR,SIR,SAR,NSDR\r\n")
    paths = [str(tmp_path / d / "a.wav") for d in ("mix", "ref", "est")]
    want = ev.compute_metrics_for_track(*paths)                                 # the whole-track v3 figures, as before
    assert {k: res[0][k] for k in ev.METRICS} == want
    assert f"a:\tSDR={want['SDR']:.3f} dB,\tSIR={want['SIR']:.3f} dB,\tSAR={want['SAR']:.3f} dB,\tNSDR={want['NSDR']:.3f} dB\n" in printed
    with pytest.raises(SystemExit):
        ev.main(argv + ["--frames_csv", str(tmp_path / "f.csv")])               # still needs --frame_window without v4
