"""Framewise BSS-eval on the GPU (svs_bss_corr_windows, svs_bss_solve_batched, evaluate.bss_eval_sources_framewise_gpu,
metrics_from_waveforms_framewise(device="gpu"), --frame_window with --device gpu) against the whole-signal entry points
and the numpy framewise functions."""
import csv
import ctypes

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import evaluate as ev
from test_bss_gram import assert_bss_close, corr
from test_gpu_bss_eval import gpu_corr, gpu_only, gpu_solve, ints, music_like_track, solve_problem

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAIRS = [(0, 0, 512), (0, 1, 512), (1, 0, 512), (2, 4, 100), (4, 3, 7), (3, 3, 1), (1, 2, 1), (4, 4, 512), (2, 0, 505)]


def i64(v):
    return (ctypes.c_int64 * len(v))(*v)


def gpu_corr_windows(sig, pairs, window, hop, nwin, ld, out_stride):
    S, n = sig.shape
    buf = torch.zeros(S, ld, dtype=torch.float64, device=DEV)
    buf[:, :n] = torch.from_numpy(sig)
    L = _lib.lib()
    flat = ints([v for p in pairs for v in p])
    out = torch.zeros(nwin, out_stride, dtype=torch.float64, device=DEV)
    ws = torch.empty(int(L.svs_bss_corr_windows_workspace_bytes(window, nwin, len(pairs), flat)), dtype=torch.uint8,
                     device=DEV)
    _lib.check(L.svs_bss_corr_windows(buf.data_ptr(), ld, S, n, window, hop, nwin, flat, len(pairs), out.data_ptr(),
                                      out_stride, ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "svs_bss_corr_windows")
    return out


@pytest.mark.parametrize("window,hop", [(8192, 8192), (8192, 4096), (3000, 1000), (513, 700)])
def test_corr_windows_matches_corr_per_slice(window, hop, report):
    n = 40000
    rng = np.random.default_rng(window + hop)
    sig = rng.standard_normal((5, n)) * np.array([1.0, 0.01, 3.0, 1.0, 1e3])[:, None]
    nwin = ev.frame_count(n, window, hop)
    lags = sum(p[2] for p in PAIRS)
    out = gpu_corr_windows(sig, PAIRS, window, hop, nwin, ld=n + 3, out_stride=lags + 5)
    got = out.cpu().numpy()
    worst = 0.0
    for w in range(nwin):
        sl = np.ascontiguousarray(sig[:, w * hop:w * hop + window])
        single = gpu_corr(sl, PAIRS).cpu().numpy()
        off = 0
        for a, b, nl in PAIRS:
            scale = corr(np.abs(sl[a]), np.abs(sl[b]), nl)
            for want in (single[off:off + nl], corr(sl[a], sl[b], nl)):
                err = np.abs(got[w, off:off + nl] - want) / np.maximum(scale, 1e-300)
                worst = max(worst, float(err.max()))
            off += nl
    assert report(f"bss_corr_windows window={window} hop={hop} rel. to sum|products|", worst, 1e-12)
    assert not got[:, lags:].any()                                          # the stride padding is not written
    assert torch.equal(out, gpu_corr_windows(sig, PAIRS, window, hop, nwin, ld=n + 3, out_stride=lags + 5))


def batched_problem(K, flen, nrhs, seeds, zero_ref_at=None):
    """The systems of solve_problem(seed) for each seed, their correlations concatenated into one buffer; the offsets of
    system s are absolute in it."""
    chunks, goffs, roffs, base = [], [], [], 0
    for s, seed in enumerate(seeds):
        c, g, r, _, _ = solve_problem(K, flen, nrhs, seed, zero_ref=0 if s == zero_ref_at else None)
        chunks.append(c)
        goffs += [base + v for v in g]
        roffs += [base + v for v in r]
        base += c.numel()
    return torch.cat(chunks), goffs, roffs


def gpu_solve_batched(corr_dev, nbatch, K, flen, goffs, roffs, nrhs):
    L = _lib.lib()
    ws = torch.empty(int(L.svs_bss_solve_batched_workspace_bytes(nbatch, K, flen, nrhs)), dtype=torch.uint8, device=DEV)
    y = torch.empty(nbatch, nrhs, dtype=torch.float64, device=DEV)
    status = torch.full((nbatch,), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.svs_bss_solve_batched(corr_dev.data_ptr(), nbatch, K, flen, i64(goffs), i64(roffs), nrhs, y.data_ptr(),
                                       status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "svs_bss_solve_batched")
    return y.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("K,flen,nrhs", [(1, 512, 3), (2, 512, 2), (2, 100, 5), (1, 37, 16)])
def test_solve_batched_matches_single_solves(K, flen, nrhs, report):
    seeds = [K * 1000 + flen + s for s in range(5)]
    corr_dev, goffs, roffs = batched_problem(K, flen, nrhs, seeds)
    y, status = gpu_solve_batched(corr_dev, len(seeds), K, flen, goffs, roffs, nrhs)
    assert not status.any()
    worst = 0.0
    for s, seed in enumerate(seeds):
        c, g, r, _, _ = solve_problem(K, flen, nrhs, seed)
        want, st = gpu_solve(c, K, flen, g, r, nrhs)
        assert st == 0
        worst = max(worst, float(np.max(np.abs(y[s] - want) / want)))
    assert report(f"bss_solve_batched K={K} flen={flen} nrhs={nrhs} rel. to single", worst, 1e-12)
    assert np.array_equal(y, gpu_solve_batched(corr_dev, len(seeds), K, flen, goffs, roffs, nrhs)[0])


def test_solve_batched_isolates_a_singular_system():
    seeds = [7, 8, 9, 10]
    corr_dev, goffs, roffs = batched_problem(2, 512, 2, seeds, zero_ref_at=2)
    y, status = gpu_solve_batched(corr_dev, 4, 2, 512, goffs, roffs, 2)
    assert list(status) == [0, 0, 1, 0]                 # the silent reference's first pivot, in its own system only
    keep = [0, 1, 3]
    g3 = [goffs[s * 4 + q] for s in keep for q in range(4)]
    r3 = [roffs[s * 4 + q] for s in keep for q in range(4)]
    y3, status3 = gpu_solve_batched(corr_dev, 3, 2, 512, g3, r3, 2)
    assert not status3.any()
    assert np.array_equal(y[keep], y3)


def track_with_silence(seconds, seed, sr=8192):
    """music_like_track with a silent vocal in [1 s, 2 s), a silent estimate in [2.3 s, 2.6 s) and everything silent
    from 6 s on: whole silent windows and partly silent ones at 1 s / 1 s and at 3 s / 1.5 s."""
    mix, vocal, est = music_like_track(seconds, sr=sr, seed=seed)
    vocal[sr:2 * sr] = 0.0
    est[int(2.3 * sr):int(2.6 * sr)] = 0.0
    for x in (mix, vocal, est):
        x[6 * sr:] = 0.0
    return mix, vocal, est


def assert_frames_close(got, want):
    for k in ev.METRICS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (k, got[k], want[k])
    assert np.array_equal(got["start"], want["start"])
    for w in np.flatnonzero(~np.isnan(want["SDR"])):
        assert_bss_close(([got["SDR"][w]], [got["SIR"][w]], [got["SAR"][w]], [0]),
                         ([want["SDR"][w]], [want["SIR"][w]], [want["SAR"][w]], [0]))
    ok = ~np.isnan(want["NSDR"])
    assert np.all(np.abs(got["NSDR"][ok] - want["NSDR"][ok]) <= 1e-3), (got["NSDR"], want["NSDR"])


@pytest.mark.parametrize("window_s,hop_s", [(1.0, 1.0), (3.0, 1.5)])
def test_metrics_framewise_gpu_matches_numpy(window_s, hop_s):
    mix, vocal, est = track_with_silence(10, seed=50)
    window, hop = int(window_s * 8192), int(hop_s * 8192)
    want = ev.metrics_from_waveforms_framewise(mix, vocal, est, window, hop)
    assert np.isnan(want["SDR"]).any() and not np.isnan(want["SDR"]).all()
    got = gpu_only(ev.metrics_from_waveforms_framewise, mix, vocal, est, window, hop, device="gpu")
    assert_frames_close(got, want)


def test_metrics_framewise_gpu_one_window():
    mix, vocal, est = music_like_track(2, seed=51)
    want = ev.metrics_from_waveforms_framewise(mix, vocal, est, 10000, 10000)
    got = gpu_only(ev.metrics_from_waveforms_framewise, mix, vocal, est, 10000, 10000, device="gpu")
    assert got["SDR"].shape == (1,)
    assert_frames_close(got, want)


def test_metrics_framewise_gpu_independent_of_workspace_budget():
    mix, vocal, est = track_with_silence(8, seed=52)
    a = gpu_only(ev.metrics_from_waveforms_framewise, mix, vocal, est, 8192, 4096, device="gpu")
    b = gpu_only(ev.metrics_from_waveforms_framewise, mix, vocal, est, 8192, 4096, device="gpu", ws_budget=1)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def two_sources(n, seed):
    rng = np.random.default_rng(seed)
    refs = np.stack([np.convolve(rng.standard_normal(n), [1.0, 0.6])[:n], rng.standard_normal(n)])
    ests = np.stack([refs[0] + 0.1 * refs[1], refs[1] - 0.2 * refs[0]]) + 0.05 * rng.standard_normal((2, n))
    refs[0, 8000:12000] = 0.0                            # window [8000, 12000) silent, its neighbours partly silent
    return refs, ests


@pytest.mark.parametrize("perm", [False, True])
def test_bss_eval_sources_framewise_gpu_matches_numpy(perm):
    refs, ests = two_sources(24000, 53)
    want = ev.bss_eval_sources_framewise(refs, ests, 4000, 2000, perm, 64)
    got = gpu_only(ev.bss_eval_sources_framewise_gpu, refs, ests, 4000, 2000, perm, 64)
    for g, w in zip(got, want):
        assert g.shape == w.shape == (2, 11)
        assert np.array_equal(np.isnan(g), np.isnan(w))
    assert np.isnan(want[0][:, 4]).all() and not np.isnan(want[0][:, 3]).any()
    for k in np.flatnonzero(~np.isnan(want[0][0])):
        assert_bss_close(tuple(v[:, k] for v in got), tuple(v[:, k] for v in want))
    one = gpu_only(ev.bss_eval_sources_framewise_gpu, refs[:1], ests[:1], 4000, 2000, perm, 64)
    want_one = ev.bss_eval_sources_framewise(refs[:1], ests[:1], 4000, 2000, perm, 64)
    for k in np.flatnonzero(~np.isnan(want_one[0][0])):
        assert_bss_close(tuple(v[:, k] for v in one), tuple(v[:, k] for v in want_one))
    whole = gpu_only(ev.bss_eval_sources_framewise_gpu, refs, ests, 24000, 2000, perm, 64)
    want_whole = ev.bss_eval_sources_framewise(refs, ests, 24000, 2000, perm, 64)
    assert whole[0].shape == (2, 1)
    assert_bss_close(tuple(v[:, 0] for v in whole), tuple(v[:, 0] for v in want_whole))


def test_cli_frame_window_gpu_matches_cpu(tmp_path, capsys):
    from scipy.io import wavfile
    for d in ("est", "mix", "ref"):
        (tmp_path / d).mkdir()
    for i, name in enumerate(("a.wav", "b.wav")):
        mix, vocal, est = music_like_track(3, seed=60 + i)
        if i == 1:
            vocal[8192:16384] = 0.0
        for d, x in (("mix", mix), ("ref", vocal), ("est", est)):
            wavfile.write(tmp_path / d / name, 8192, (0.5 * x).astype(np.float32))
    rows, frames, printed = {}, {}, {}
    for device in ("cpu", "gpu"):
        out, fout = tmp_path / f"{device}.csv", tmp_path / f"{device}_frames.csv"
        argv = ["--est", str(tmp_path / "est"), "--mix", str(tmp_path / "mix"), "--ref", str(tmp_path / "ref"),
                "--out_csv", str(out), "--device", device, "--frame_window", "1", "--frames_csv", str(fout)]
        res = gpu_only(ev.main, argv) if device == "gpu" else ev.main(argv)
        assert len(res) == 2
        printed[device] = capsys.readouterr().out.replace(str(out), "").replace(str(fout), "")
        with open(out) as f:
            rows[device] = [[r[0]] + [f"{float(v):.3f}" for v in r[1:]] for r in list(csv.reader(f))[1:]]
        with open(fout) as f:
            frames[device] = [r[:3] + [f"{float(v):.3f}" for v in r[3:]] for r in list(csv.reader(f))[1:]]
    assert rows["gpu"] == rows["cpu"]
    assert frames["gpu"] == frames["cpu"] and len(frames["cpu"]) == 6
    assert printed["gpu"] == printed["cpu"]
