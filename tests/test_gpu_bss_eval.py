"""BSS-eval on the GPU (csrc/bss.hip, evaluate.bss_eval_sources_gpu / metrics_from_waveforms(device="gpu") / --device gpu)
against float64 numpy: the correlation kernel, the Cholesky + forward solve, and the metrics against bss_eval_sources."""
import csv
import ctypes

import numpy as np
import pytest
import torch
from scipy.linalg import cholesky, solve_triangular

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import evaluate as ev
from test_bss_gram import assert_bss_close, band_limited_case, corr, property_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def gpu_corr(sig, pairs, ld=None):
    """svs_bss_corr on the rows of sig (numpy (S, n)), optionally stored with row stride ld > n."""
    S, n = sig.shape
    ld = ld or n
    buf = torch.zeros(S, ld, dtype=torch.float64, device=DEV)
    buf[:, :n] = torch.from_numpy(sig)
    L = _lib.lib()
    flat = ints([v for p in pairs for v in p])
    out = torch.empty(sum(p[2] for p in pairs), dtype=torch.float64, device=DEV)
    ws = torch.empty(int(L.svs_bss_corr_workspace_bytes(n, len(pairs), flat)), dtype=torch.uint8, device=DEV)
    _lib.check(L.svs_bss_corr(buf.data_ptr(), ld, S, n, flat, len(pairs), out.data_ptr(), ws.data_ptr(), ws.numel(),
                              _lib.stream_ptr()), "svs_bss_corr")
    return out


@pytest.mark.parametrize("n", [1, 7, 511, 512, 513, 4097, 300001])
def test_corr_kernel_matches_numpy(n, report):
    rng = np.random.default_rng(n)
    sig = rng.standard_normal((5, n)) * np.array([1.0, 0.01, 3.0, 1.0, 1e3])[:, None]
    pairs = [(0, 0, 512), (0, 1, 512), (1, 0, 512), (2, 4, 100), (4, 3, 7), (3, 3, 1), (1, 2, 1), (4, 4, 512), (2, 0, 505)]
    out = gpu_corr(sig, pairs, ld=n + 3)
    got = out.cpu().numpy()
    off = 0
    worst = 0.0
    for a, b, nl in pairs:
        want = corr(sig[a], sig[b], nl)
        scale = corr(np.abs(sig[a]), np.abs(sig[b]), nl)
        err = np.abs(got[off:off + nl] - want) / np.maximum(scale, 1e-300)
        worst = max(worst, float(err.max()))
        off += nl
    assert report(f"bss_corr n={n} rel. to sum|products|", worst, 1e-12)
    assert torch.equal(out, gpu_corr(sig, pairs, ld=n + 3))       # bitwise run to run


def gpu_solve(corr_dev, K, flen, gram_off, rhs_off, nrhs):
    L = _lib.lib()
    ws = torch.empty(int(L.svs_bss_solve_workspace_bytes(K, flen, nrhs)), dtype=torch.uint8, device=DEV)
    y = torch.empty(nrhs, dtype=torch.float64, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.svs_bss_solve(corr_dev.data_ptr(), K, flen, ints(gram_off), ints(rhs_off), nrhs, y.data_ptr(),
                               status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "svs_bss_solve")
    return y.cpu().numpy(), int(status.item())


def solve_problem(K, flen, nrhs, seed, zero_ref=None):
    """K references and nrhs estimates of 4096 samples; the block-Toeplitz G of the references and the D of each estimate
    as numpy matrices, and the correlation buffer + offsets svs_bss_solve takes."""
    rng = np.random.default_rng(seed)
    n = 4096
    refs = rng.standard_normal((K, n))
    refs[1 % K] = np.convolve(refs[1 % K], [1.0, 0.7, 0.2])[:n]
    if zero_ref is not None:
        refs[zero_ref] = 0.0
    ests = rng.standard_normal((nrhs, n)) + refs.sum(axis=0)
    chunks, off = [], 0
    gram_off, rhs_off = [], []
    for i in range(K):
        for j in range(K):
            chunks.append(corr(refs[i], refs[j], flen))
            gram_off.append(off)
            off += flen
    for e in ests:
        for i in range(K):
            chunks.append(corr(e, refs[i], flen))
            rhs_off.append(off)
            off += flen
    p = np.arange(flen)
    d = p[None, :] - p[:, None]
    G = np.empty((K * flen, K * flen))
    for i in range(K):
        for j in range(K):
            G[i * flen:(i + 1) * flen, j * flen:(j + 1) * flen] = np.where(d >= 0, chunks[i * K + j][np.abs(d)],
                                                                           chunks[j * K + i][np.abs(d)])
    D = np.stack([np.concatenate(chunks[K * K + r * K:K * K + (r + 1) * K]) for r in range(nrhs)], axis=1)
    return torch.from_numpy(np.concatenate(chunks)).to(DEV), gram_off, rhs_off, G, D


@pytest.mark.parametrize("K,flen,nrhs", [(1, 512, 3), (2, 512, 5), (2, 100, 2), (1, 37, 16)])
def test_solve_matches_numpy_cholesky(K, flen, nrhs, report):
    corr_dev, gram_off, rhs_off, G, D = solve_problem(K, flen, nrhs, seed=K * 1000 + flen)
    y, status = gpu_solve(corr_dev, K, flen, gram_off, rhs_off, nrhs)
    assert status == 0
    assert np.array_equal(y, gpu_solve(corr_dev, K, flen, gram_off, rhs_off, nrhs)[0])      # bitwise run to run
    Y = solve_triangular(cholesky(G, lower=True), D, lower=True)
    want = (Y * Y).sum(axis=0)
    err = float(np.max(np.abs(y - want) / want))
    assert report(f"bss_solve K={K} flen={flen} nrhs={nrhs} rel", err, 1e-10)


@pytest.mark.parametrize("zero_ref,first_bad", [(0, 1), (1, 513)])
def test_solve_reports_singular_gram(zero_ref, first_bad):
    """A silent reference makes its block of G zero: the status names the first non-positive pivot; nothing faults."""
    corr_dev, gram_off, rhs_off, _, _ = solve_problem(2, 512, 2, seed=9, zero_ref=zero_ref)
    _, status = gpu_solve(corr_dev, 2, 512, gram_off, rhs_off, 2)
    assert status == first_bad
    corr_dev, gram_off, rhs_off, _, _ = solve_problem(2, 512, 2, seed=9)          # the stream is still usable
    assert gpu_solve(corr_dev, 2, 512, gram_off, rhs_off, 2)[1] == 0


def _numpy_fallback_taken(*args, **kwargs):
    raise AssertionError("the GPU path fell back to the numpy bss_eval_sources")


def gpu_only(fn, *args, **kwargs):
    """fn(*args, **kwargs) with the numpy bss_eval_sources (the fallback on a singular G) made to fail: the result must
    come from the GPU path."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ev, "bss_eval_sources", _numpy_fallback_taken)
        return fn(*args, **kwargs)


@pytest.mark.parametrize("case", ["filtered", "interference", "noise", "permuted"])
def test_bss_eval_gpu_property_cases(case):
    refs, ests = property_cases()[case]
    want = ev.bss_eval_sources(refs, ests)
    assert_bss_close(gpu_only(ev.bss_eval_sources_gpu, refs, ests), want)


def test_bss_eval_gpu_band_limited_and_forced_permutation():
    refs, ests = band_limited_case(200_000)
    want = ev.bss_eval_sources(refs, ests)
    refs_dev, ests_dev = torch.from_numpy(refs).to(DEV), torch.from_numpy(ests).to(DEV)
    assert_bss_close(gpu_only(ev.bss_eval_sources_gpu, refs_dev, ests_dev), want)
    swapped = ests[::-1].copy()
    want, want_fixed = ev.bss_eval_sources(refs, swapped), ev.bss_eval_sources(refs, swapped, compute_permutation=False)
    got = gpu_only(ev.bss_eval_sources_gpu, refs, swapped)
    assert list(got[3]) == [1, 0]
    assert_bss_close(got, want)
    assert_bss_close(gpu_only(ev.bss_eval_sources_gpu, refs, swapped, compute_permutation=False), want_fixed)


def test_bss_eval_gpu_one_source():
    rng = np.random.default_rng(21)
    s = rng.standard_normal(30000)
    e = np.convolve(s, [0.6, 0.3])[:30000] + 0.1 * rng.standard_normal(30000)
    want = ev.bss_eval_sources(s, e)
    assert_bss_close(gpu_only(ev.bss_eval_sources_gpu, s, e), want)


def test_bss_eval_gpu_silent_reference_falls_back_to_numpy():
    rng = np.random.default_rng(4)
    refs = np.stack([np.zeros(8000), rng.standard_normal(8000)])
    ests = np.stack([0.01 * rng.standard_normal(8000), refs[1] + 0.1 * rng.standard_normal(8000)])
    with np.errstate(all="ignore"):
        with pytest.warns(RuntimeWarning, match="falls back to the numpy path"):
            got = ev.bss_eval_sources_gpu(refs, ests)
        want = ev.bss_eval_sources(refs, ests)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_bss_eval_gpu_rejects_three_sources():
    x = np.ones((3, 1000))
    with pytest.raises(ValueError, match="1 or 2 sources"):
        ev.bss_eval_sources_gpu(x, x)


def music_like_track(seconds, sr=8192, seed=30):
    rng = np.random.default_rng(seed)
    n = seconds * sr
    t = np.arange(n) / sr
    vocal = np.sin(2 * np.pi * 220 * t * (1 + 0.01 * np.sin(2 * np.pi * 0.5 * t))) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.3 * t))
    vocal += 0.05 * np.convolve(rng.standard_normal(n), np.ones(8) / 8)[:n]
    acc = 0.3 * np.convolve(rng.standard_normal(n), [1.0, -0.5, 0.25])[:n]
    mix = vocal + acc
    est = vocal + 0.08 * acc + 0.02 * rng.standard_normal(n)
    return mix, vocal, est


def test_metrics_from_waveforms_gpu_matches_cpu():
    mix, vocal, est = music_like_track(30)
    want = ev.metrics_from_waveforms(mix, vocal, est)
    got = gpu_only(ev.metrics_from_waveforms, mix, vocal, est, device="gpu")
    assert got.keys() == want.keys()
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-3, (k, got[k], want[k])


def test_cli_device_gpu_matches_cpu(tmp_path, capsys):
    from scipy.io import wavfile
    for d in ("est", "mix", "ref"):
        (tmp_path / d).mkdir()
    for i, name in enumerate(("a.wav", "b.wav")):
        mix, vocal, est = music_like_track(3, seed=40 + i)
        for d, x in (("mix", mix), ("ref", vocal), ("est", est)):
            wavfile.write(tmp_path / d / name, 8192, (0.5 * x).astype(np.float32))
    rows, printed = {}, {}
    for device in ("cpu", "gpu"):
        out = tmp_path / f"{device}.csv"
        argv = ["--est", str(tmp_path / "est"), "--mix", str(tmp_path / "mix"), "--ref", str(tmp_path / "ref"),
                "--out_csv", str(out), "--device", device]
        res = gpu_only(ev.main, argv) if device == "gpu" else ev.main(argv)
        assert len(res) == 2
        printed[device] = capsys.readouterr().out.replace(str(out), "")
        with open(out) as f:
            rows[device] = [[r[0]] + [f"{float(v):.3f}" for v in r[1:]] for r in list(csv.reader(f))[1:]]
    assert rows["gpu"] == rows["cpu"]
    assert printed["gpu"] == printed["cpu"]
