"""BSS-eval images on the GPU (svs_bss_img_corr_windows, svs_bss_img_solve_batched, evaluate.bss_eval_images_gpu / _framewise_gpu,
image_metrics_from_waveforms(device="gpu"), --stereo --device gpu) against numpy: the lagged correlations, scipy's Cholesky
and least squares, and the numpy bss_eval_images."""
import csv
import ctypes

import numpy as np
import pytest
import torch
from scipy.linalg import cholesky, solve_triangular

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import evaluate as ev
from test_bss_gram import corr
from test_bss_images import (assert_image_frames_close, assert_images_close, degenerate_case, image_cases, stereo_track)
from test_gpu_bss_framewise import batched_problem, gpu_solve_batched

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = -12345.0


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def i64(v):
    return (ctypes.c_int64 * len(v))(*v)


# 10 signals, 40 pairs: the Gram and right-hand-side pairs of a stereo problem in both orders, signal 0 in 12 of them, and
# the lag counts 512, 505, 100, 7 and 1
PAIRS = ([(i, j, 512) for i in range(4) for j in range(4)] + [(4 + e, 0, 512) for e in range(6)] +
         [(9, 1, 505), (1, 9, 505), (8, 2, 505), (5, 6, 100), (6, 5, 100), (7, 3, 100), (3, 8, 100), (0, 9, 7), (9, 0, 7),
          (4, 4, 7), (2, 7, 7)] + [(s, s, 1) for s in (0, 3, 4, 9)] + [(4, 0, 1), (0, 4, 1), (9, 2, 1)])


def gpu_img_corr_windows(sig, pairs, window, hop, nwin, ld, out_stride):
    S, n = sig.shape
    buf = torch.zeros(S, ld, dtype=torch.float64, device=DEV)
    buf[:, :n] = torch.from_numpy(sig)
    L = _lib.lib()
    flat = ints([v for p in pairs for v in p])
    out = torch.full((nwin * out_stride + 64,), GUARD, dtype=torch.float64, device=DEV)
    ws = torch.empty(int(L.svs_bss_img_corr_windows_workspace_bytes(window, nwin, len(pairs), flat)), dtype=torch.uint8,
                     device=DEV)
    assert ws.numel() > 0
    _lib.check(L.svs_bss_img_corr_windows(buf.data_ptr(), ld, S, n, window, hop, nwin, flat, len(pairs), out.data_ptr(),
                                          out_stride, ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "svs_bss_img_corr_windows")
    return out


@pytest.mark.parametrize("framed", [False, True])
@pytest.mark.parametrize("n", [1000, 1535, 1536, 5000])
def test_img_corr_windows_matches_numpy(n, framed, report):
    assert len(PAIRS) == 40 and len({s for p in PAIRS for s in p[:2]}) == 10
    rng = np.random.default_rng(n)
    sig = rng.standard_normal((10, n)) * np.array([1.0, 0.01, 3.0, 1.0, 1e3, 1.0, 0.5, 2.0, 1e-2, 10.0])[:, None]
    window, hop, nwin = (3000, 1700, 3) if framed else (n, n, 1)           # framed: the last window runs past n
    lags = sum(p[2] for p in PAIRS)
    stride = lags + 5
    out = gpu_img_corr_windows(sig, PAIRS, window, hop, nwin, ld=n + 3, out_stride=stride)
    got = out.cpu().numpy()
    worst = 0.0
    for w in range(nwin):
        sl = sig[:, w * hop:w * hop + window]
        off = 0
        for a, b, nl in PAIRS:
            if sl.shape[1]:
                want, scale = corr(sl[a], sl[b], nl), corr(np.abs(sl[a]), np.abs(sl[b]), nl)
            else:
                want, scale = np.zeros(nl), np.zeros(nl)
            err = np.abs(got[w * stride + off:w * stride + off + nl] - want) / np.maximum(scale, 1e-300)
            worst = max(worst, float(err.max()))
            off += nl
        assert np.all(got[w * stride + lags:(w + 1) * stride] == GUARD)        # the stride padding is not written
    assert report(f"bss_img_corr_windows n={n} framed={framed} rel. to sum|products|", worst, 1e-12)
    assert np.all(got[nwin * stride:] == GUARD)                                # the guard words after out
    assert torch.equal(out, gpu_img_corr_windows(sig, PAIRS, window, hop, nwin, ld=n + 3, out_stride=stride))


def img_problem(K, flen, nrhs, seed, zero=None, same=None, negative=None):
    """K white reference channels (one of them filtered) and nrhs estimates of 4096 samples: the correlation buffer and the
    offsets svs_bss_img_solve_batched takes, and G and D as numpy matrices.  zero: a silent channel; same = (a, b): channel
    b is channel a; negative: the lag-0 autocorrelation of that channel with its sign flipped (G indefinite)."""
    rng = np.random.default_rng(seed)
    n = 4096
    refs = rng.standard_normal((K, n))
    refs[1 % K] = np.convolve(refs[1 % K], [1.0, 0.7, 0.2])[:n]
    if zero is not None:
        refs[zero] = 0.0
    if same is not None:
        refs[same[1]] = refs[same[0]]
    ests = rng.standard_normal((nrhs, n)) + refs.sum(axis=0)
    chunks = [corr(refs[i], refs[j], flen) for i in range(K) for j in range(K)]
    if negative is not None:
        chunks[negative * K + negative][0] *= -1.0
    chunks += [corr(e, refs[i], flen) for e in ests for i in range(K)]
    offs = [q * flen for q in range(len(chunks))]
    d = np.arange(flen)[None, :] - np.arange(flen)[:, None]
    G = np.block([[np.where(d >= 0, chunks[i * K + j][np.abs(d)], chunks[j * K + i][np.abs(d)]) for j in range(K)]
                  for i in range(K)])
    D = np.stack([np.concatenate(chunks[K * K + r * K:K * K + (r + 1) * K]) for r in range(nrhs)], axis=1)
    return np.concatenate(chunks), offs[:K * K], offs[K * K:], G, D


def gpu_img_solve_batched(corr_dev, nbatch, K, flen, goffs, roffs, nrhs):
    L = _lib.lib()
    ws = torch.empty(int(L.svs_bss_img_solve_batched_workspace_bytes(nbatch, K, flen, nrhs)), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0
    y = torch.empty(nbatch, nrhs, dtype=torch.float64, device=DEV)
    status = torch.full((nbatch,), -7, dtype=torch.int32, device=DEV)
    skipped = torch.full((nbatch,), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.svs_bss_img_solve_batched(corr_dev.data_ptr(), nbatch, K, flen, i64(goffs), i64(roffs), nrhs, y.data_ptr(),
                                           status.data_ptr(), skipped.data_ptr(), ws.data_ptr(), ws.numel(),
                                           _lib.stream_ptr()), "svs_bss_img_solve_batched")
    return y.cpu().numpy(), status.cpu().numpy(), skipped.cpu().numpy()


def gpu_img_solve(problems, K, flen, nrhs):
    """One batched call over problems [(corr, gram_off, rhs_off, ...)]: (ynorm2 (nbatch, nrhs), status, skipped)."""
    base, goffs, roffs = 0, [], []
    for c, g, r, *_ in problems:
        goffs += [base + v for v in g]
        roffs += [base + v for v in r]
        base += c.size
    corr_dev = torch.from_numpy(np.concatenate([p[0] for p in problems])).to(DEV)
    return gpu_img_solve_batched(corr_dev, len(problems), K, flen, goffs, roffs, nrhs)


@pytest.mark.parametrize("K,flen,nrhs", [(4, 512, 4), (4, 100, 3), (3, 37, 16), (2, 512, 5), (1, 64, 1)])
def test_img_solve_matches_scipy_cholesky(K, flen, nrhs, report):
    prob = img_problem(K, flen, nrhs, seed=K * 1000 + flen)
    y, status, skipped = gpu_img_solve([prob], K, flen, nrhs)
    assert not status.any() and not skipped.any()
    assert np.array_equal(y, gpu_img_solve([prob], K, flen, nrhs)[0])          # bitwise run to run
    Y = solve_triangular(cholesky(prob[3], lower=True), prob[4], lower=True)
    want = (Y * Y).sum(axis=0)
    err = float(np.max(np.abs(y[0] - want) / want))
    assert report(f"bss_img_solve K={K} flen={flen} nrhs={nrhs} rel", err, 1e-10)


def test_img_solve_skips_dependent_columns_in_their_own_system(report):
    """A batch of a silent channel, a healthy system and two identical channels."""
    K, flen, nrhs = 4, 100, 3
    probs = [img_problem(K, flen, nrhs, 1, zero=2), img_problem(K, flen, nrhs, 2), img_problem(K, flen, nrhs, 3, same=(0, 3))]
    y, status, skipped = gpu_img_solve(probs, K, flen, nrhs)
    assert not status.any() and list(skipped) == [flen, 0, flen]
    alone, _, _ = gpu_img_solve(probs[1:2], K, flen, nrhs)
    assert np.array_equal(y[1], alone[0])
    worst = 0.0
    for s in (0, 2):
        G, D = probs[s][3:]
        want = (D * np.linalg.lstsq(G, D, rcond=None)[0]).sum(axis=0)          # D^T G^+ D: the energy of the projection
        worst = max(worst, float(np.max(np.abs(y[s] - want) / want)))
    assert report("bss_img_solve rank-deficient rel. to lstsq", worst, 1e-8)


def test_img_solve_reports_an_indefinite_system():
    K, flen, nrhs = 2, 100, 2
    probs = [img_problem(K, flen, nrhs, 4), img_problem(K, flen, nrhs, 5, negative=1)]
    y, status, skipped = gpu_img_solve(probs, K, flen, nrhs)
    assert list(status) == [0, flen + 1] and skipped[0] == 0                    # the first pivot of channel 1
    alone, status, _ = gpu_img_solve(probs[:1], K, flen, nrhs)                  # the stream is still usable
    assert status[0] == 0 and np.array_equal(alone[0], y[0])


@pytest.mark.parametrize("K,flen,nrhs", [(1, 64, 1), (2, 37, 16), (2, 100, 3), (2, 512, 2)])
def test_mono_and_image_solves_agree_bitwise_on_regular_systems(K, flen, nrhs):
    """svs_bss_solve_batched and svs_bss_img_solve_batched factor a tile with the same operations in the same order and
    differ in the pivot rule and in who factors the diagonal tile (every panel block, or one block once), so on systems
    where every pivot passes both rules they give the same bits: one tile with no update launch (order 64), two
    tiles with identity padding (74), a full-width right-hand-side block (16), the largest mono order (1024).  The seeds
    are ones for which the numpy skip_cholesky of test_bss_images skips nothing and reports status 0."""
    seeds = [K * 1000 + flen + s for s in range(3)]
    corr_dev, goffs, roffs = batched_problem(K, flen, nrhs, seeds)
    mono, mono_status = gpu_solve_batched(corr_dev, len(seeds), K, flen, goffs, roffs, nrhs)
    img, img_status, skipped = gpu_img_solve_batched(corr_dev, len(seeds), K, flen, goffs, roffs, nrhs)
    assert not mono_status.any() and not img_status.any()
    assert list(skipped) == [0, 0, 0]
    assert np.array_equal(mono, img)


# ---- the scorers ------------------------------------------------------------------------------

def _numpy_fallback_taken(*args, **kwargs):
    raise AssertionError("the GPU path fell back to the numpy bss_eval_images")


def gpu_only(fn, *args, **kwargs):
    """fn(*args, **kwargs) with the numpy bss_eval_images (the fallback on a failed factorisation) made to fail."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ev, "bss_eval_images", _numpy_fallback_taken)
        return fn(*args, **kwargs)


@pytest.mark.parametrize("nsrc", [1, 2])
@pytest.mark.parametrize("nchan", [1, 2])
@pytest.mark.parametrize("case", ["interference", "noise", "permuted", "spatial"])
def test_bss_eval_images_gpu_property_cases(case, nchan, nsrc):
    refs, ests = image_cases(n=6000, nchan=nchan)[case]
    refs, ests = refs[:nsrc], ests[:nsrc]
    for perm in (True, False):
        want = ev.bss_eval_images(refs, ests, perm)
        got = gpu_only(ev.bss_eval_images_gpu, refs, ests, perm)
        assert_images_close(got, want, 1e-3)
        assert np.issubdtype(got[4].dtype, np.integer)


def test_bss_eval_images_gpu_degenerate_images():
    refs, ests = degenerate_case(6000)
    assert_images_close(gpu_only(ev.bss_eval_images_gpu, refs, ests), ev.bss_eval_images(refs, ests), 1e-3)


def test_bss_eval_images_gpu_rejects_three_sources():
    x = np.ones((3, 2000, 2))
    with pytest.raises(ValueError, match="1 or 2 sources"):
        ev.bss_eval_images_gpu(x, x)


@pytest.fixture(scope="module")
def framed_track():
    sr = 8192
    mix, vocal, est = stereo_track(6, sr, seed=31, silent_second=3)
    return mix, vocal, est, ev.image_metrics_from_waveforms_framewise(mix, vocal, est, sr, sr)


@pytest.mark.parametrize("ws_budget", [ev.WS_BUDGET, 64 << 20])
def test_image_metrics_framewise_gpu_matches_numpy(framed_track, ws_budget):
    mix, vocal, est, want = framed_track
    assert list(np.isnan(want["SDR"])) == [False, False, False, True, False, False]
    got = gpu_only(ev.image_metrics_from_waveforms_framewise, mix, vocal, est, 8192, 8192, device="gpu", ws_budget=ws_budget)
    assert_image_frames_close(got, want)


def test_image_metrics_from_waveforms_gpu_matches_numpy():
    mix, vocal, est = stereo_track(2, 8192, seed=32)
    want = ev.image_metrics_from_waveforms(mix, vocal, est)
    got = gpu_only(ev.image_metrics_from_waveforms, mix, vocal, est, device="gpu")
    assert got.keys() == want.keys()
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-3, (k, got[k], want[k])


def test_cli_stereo_frame_window_gpu_matches_cpu(tmp_path, capsys):
    from scipy.io import wavfile
    for d in ("est", "mix", "ref"):
        (tmp_path / d).mkdir()
    mix, vocal, est = stereo_track(3, 8192, seed=33, silent_second=1)
    for d, x in (("mix", mix), ("ref", vocal), ("est", est)):
        wavfile.write(tmp_path / d / "a.wav", 8192, (0.3 * x).astype(np.float32))
    rows, frames, printed = {}, {}, {}
    for device in ("cpu", "gpu"):
        out, fout = tmp_path / f"{device}.csv", tmp_path / f"{device}_frames.csv"
        argv = ["--est", str(tmp_path / "est"), "--mix", str(tmp_path / "mix"), "--ref", str(tmp_path / "ref"), "--stereo",
                "--out_csv", str(out), "--device", device, "--frame_window", "1", "--frames_csv", str(fout)]
        res = gpu_only(ev.main, argv) if device == "gpu" else ev.main(argv)
        assert len(res) == 1
        printed[device] = capsys.readouterr().out.replace(str(out), "").replace(str(fout), "")
        with open(out) as f:
            rows[device] = [[r[0]] + [f"{float(v):.3f}" for v in r[1:]] for r in list(csv.reader(f))[1:]]
        with open(fout) as f:
            frames[device] = [r[:3] + [f"{float(v):.3f}" for v in r[3:]] for r in list(csv.reader(f))[1:]]
    assert "ISR=" in printed["cpu"] and "frames=2/3" in printed["cpu"]
    assert rows["gpu"] == rows["cpu"] and len(rows["cpu"][0]) == 7
    assert frames["gpu"] == frames["cpu"] and len(frames["cpu"]) == 3 and len(frames["cpu"][0]) == 8
    assert printed["gpu"] == printed["cpu"]
