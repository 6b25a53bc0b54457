"""BSS-eval images on the host (evaluate.bss_eval_images / _framewise, _image_metrics_from_gram, image_metrics_from_waveforms,
--stereo): the defining properties of the image decomposition, the Gram form against the definition, the rank rule of the
device solve restated in numpy (skip_cholesky) on degenerate stereo images, the window rules of the device="gpu" entry
points with the one library-calling function replaced by numpy, the argument checks of the svs_bss_img_* entry points and
the command line.  No GPU needed."""
import csv
import ctypes
import warnings

import numpy as np
import pytest
import torch
from scipy.linalg import cholesky, solve_triangular

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import evaluate as ev
from test_bss_gram import corr

FLEN = 32
NAMES = ("sdr", "isr", "sir", "sar")


def db(num, den):
    return 10.0 * np.log10(num / den)


def image_cases(n=4000, seed=3, nchan=2):
    """Two white sources whose channels are correlated, and estimates with interference and noise in every channel, so
    that every figure stays below 60 dB."""
    rng = np.random.default_rng(seed)
    refs = rng.standard_normal((2, n, nchan))
    if nchan == 2:
        refs[0, :, 1] = 0.6 * refs[0, :, 0] + 0.8 * refs[0, :, 1]
        refs[1, :, 0] = 0.5 * refs[1, :, 1] - 0.7 * refs[1, :, 0]
    s1, s2 = refs
    noise = 0.05 * rng.standard_normal((2, n, nchan))
    return {"interference": (refs, np.stack([s1 + 0.1 * s2, s2 + 0.1 * s1]) + 0.1 * noise),
            "noise": (refs, np.stack([s1, s2]) + 2.0 * noise),
            "permuted": (refs, np.stack([s2 + 0.05 * s1, s1 + 0.05 * s2]) + noise),
            "spatial": (refs, np.stack([s1 * [0.8, 1.1][:nchan] + 0.02 * s2, 0.9 * s2 + 0.1 * s1]) + noise)}


def degenerate_case(n=4000, seed=11):
    """Vocal with L == R exactly, accompaniment with a silent right channel: both images and their union are rank
    deficient."""
    rng = np.random.default_rng(seed)
    x, y = rng.standard_normal((2, n))
    vocal = np.stack([x, x], axis=1)
    acc = np.stack([y, np.zeros(n)], axis=1)
    noise = 0.05 * rng.standard_normal((2, n, 2))
    refs = np.stack([vocal, acc])
    return refs, np.stack([vocal * [0.9, 1.0] + 0.1 * acc, acc + 0.1 * vocal]) + noise


def assert_images_close(got, want, tol):
    for name, g, w in zip(NAMES, got[:4], want[:4]):
        g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
        assert g.shape == w.shape and not np.isnan(g).any(), (name, g, w)
        fin = np.isfinite(w)                                 # one source: no interference, SIR is +inf in both
        assert np.array_equal(g[~fin], w[~fin]) and np.all(w[fin] < 60.0), (name, g, w)
        assert np.all(np.abs(g[fin] - w[fin]) <= tol), (name, g, w)
    assert list(got[4]) == list(want[4])


# ---- the definition -------------------------------------------------------------------------

def test_one_channel_is_the_source_decomposition():
    refs, ests = image_cases(nchan=1)["interference"]
    sdr, isr, sir, sar, perm = ev.bss_eval_images(refs, ests, flen=FLEN)
    _, sir1, sar1, perm1 = ev.bss_eval_sources(refs[:, :, 0], ests[:, :, 0], flen=FLEN)
    assert np.all(np.abs(sir - sir1) <= 1e-9) and np.all(np.abs(sar - sar1) <= 1e-9) and list(perm) == list(perm1)
    for j in range(2):
        assert abs(sdr[j] - db(np.sum(refs[j] ** 2), np.sum((ests[j] - refs[j]) ** 2))) <= 1e-9
    two_d = ev.bss_eval_images(refs[:, :, 0], ests[:, :, 0], flen=FLEN)          # (nsrc, nsampl) is nchan 1
    for a, b in zip(two_d, (sdr, isr, sir, sar, perm)):
        np.testing.assert_array_equal(a, b)


def test_spatial_distortion_only():
    """An estimate that is the source's own image with channel gains and cross-channel leakage is all target and spatial
    distortion: SIR and SAR > 100 dB, ISR = SDR = the direct ratio.  The source ends in 5 silent samples, so the delayed
    leakage is not cut at the end of the estimate (a cut tail is an artifact: 40 dB at this length), and a second source
    stands beside it, since SIR is +inf by definition with one source, in the mono scoring too."""
    rng = np.random.default_rng(5)
    n = 4000
    s, other = rng.standard_normal((2, n, 2))
    s[-5:] = 0.0                                                               # the delayed copy is not cut at the end
    e = s * [0.8, 1.1]
    e[5:, 0] += 0.3 * s[:-5, 1]                                                # the other channel, 5 samples late
    e[5:, 1] += 0.3 * s[:-5, 0]
    refs, ests = np.stack([s, other]), np.stack([e, other])
    sdr, isr, sir, sar, _ = ev.bss_eval_images(refs, ests, flen=FLEN)
    direct = db(np.sum(s ** 2), np.sum((e - s) ** 2))
    assert sir[0] > 100.0 and sar[0] > 100.0
    assert abs(isr[0] - direct) <= 1e-6 and abs(sdr[0] - direct) <= 1e-9
    for c in range(2):                                                         # per channel as a mono problem the leakage
        mono = ev.bss_eval_sources(refs[:, :, c], ests[:, :, c], flen=FLEN)    # is outside the span: not a filtered copy
        assert mono[1][0] < 100.0 and mono[2][0] < 100.0


def test_known_interference_noise_and_permutation():
    cases = image_cases()
    refs, ests = cases["interference"]
    sdr, isr, sir, sar, perm = ev.bss_eval_images(refs, ests, flen=FLEN)
    ratio = db(np.sum(refs[0] ** 2), np.sum(refs[1] ** 2))                     # s_j + 0.1 s_other: 20 dB at equal energies
    assert list(perm) == [0, 1] and np.all(np.abs(sir - [20.0 + ratio, 20.0 - ratio]) < 0.5) and np.all(sar > 40.0)
    refs, ests = cases["noise"]
    sdr, isr, sir, sar, perm = ev.bss_eval_images(refs, ests, flen=FLEN)
    snr = [db(np.sum(refs[j] ** 2), np.sum((ests[j] - refs[j]) ** 2)) for j in range(2)]
    assert np.all(np.abs(sar - snr) < 0.5) and np.all(np.abs(sdr - snr) <= 1e-9) and np.all(sir > 25.0)
    refs, ests = cases["permuted"]
    found = ev.bss_eval_images(refs, ests, flen=FLEN)
    assert list(found[4]) == [1, 0] and np.all(found[2] > 20.0)
    swapped = ev.bss_eval_images(refs, ests[::-1], flen=FLEN)
    for a, b in zip(found[:4], swapped[:4]):
        np.testing.assert_array_equal(a, b)
    kept = ev.bss_eval_images(refs, ests, compute_permutation=False, flen=FLEN)
    assert list(kept[4]) == [0, 1] and np.all(kept[2] < 0.0)


def test_bad_shapes_raise():
    with pytest.raises(ValueError):
        ev.bss_eval_images(np.ones((2, 100, 2)), np.ones((2, 100, 1)), flen=FLEN)
    with pytest.raises(ValueError):
        ev.bss_eval_images(np.ones(100), np.ones(100), flen=FLEN)
    with pytest.raises(ValueError):
        ev.bss_eval_images_framewise(np.ones((2, 100, 2)), np.ones((2, 100, 2)), 0, 10, flen=FLEN)


# ---- the Gram form --------------------------------------------------------------------------

def gram_system(chans, ests, flen):
    """Block-Toeplitz G of the rows of chans and D (one column per row of ests) from lagged correlations."""
    d = np.arange(flen)[None, :] - np.arange(flen)[:, None]
    c = {(i, j): corr(chans[i], chans[j], flen) for i in range(len(chans)) for j in range(len(chans))}
    G = np.block([[np.where(d >= 0, c[i, j][np.abs(d)], c[j, i][np.abs(d)]) for j in range(len(chans))]
                  for i in range(len(chans))])
    D = np.stack([np.concatenate([corr(e, s, flen) for s in chans]) for e in ests], axis=1)
    return G, D


def gram_terms(refs, ests, flen, energy_of):
    """The five channel-summed inputs of _image_metrics_from_gram; energy_of(G, D) -> |P e|^2 per column of D."""
    nsrc, n, nchan = refs.shape
    rc, ec = refs.transpose(0, 2, 1), ests.transpose(0, 2, 1)
    e_ref, e_est = (rc ** 2).sum(axis=(1, 2)), (ec ** 2).sum(axis=(1, 2))
    cross = np.array([[np.sum(rc[j] * ec[a]) for j in range(nsrc)] for a in range(nsrc)])
    flat = ec.reshape(nsrc * nchan, n)
    proj_one = np.stack([energy_of(*gram_system(rc[j], flat, flen)).reshape(nsrc, nchan).sum(axis=1)
                         for j in range(nsrc)], axis=1)
    proj_all = energy_of(*gram_system(rc.reshape(nsrc * nchan, n), flat, flen)).reshape(nsrc, nchan).sum(axis=1)
    return e_ref, e_est, cross, proj_one, proj_all


def cholesky_energy(G, D):
    Y = solve_triangular(cholesky(G, lower=True), D, lower=True)
    return (Y * Y).sum(axis=0)


@pytest.mark.parametrize("perm", [True, False])
@pytest.mark.parametrize("case", ["interference", "noise", "permuted", "spatial"])
def test_gram_form_matches_the_definition(case, perm):
    refs, ests = image_cases()[case]
    got = ev._image_metrics_from_gram(*gram_terms(refs, ests, FLEN, cholesky_energy), perm)
    assert_images_close(got, ev.bss_eval_images(refs, ests, perm, FLEN), 1e-8)


def test_gram_form_denominators_follow_db():
    got = ev._image_metrics_from_gram([1.0], [1.0], [[1.0]], [[1.0]], [1.0])
    assert all(v[0] == np.inf for v in got[:4])


# ---- the rank rule of the device solve, in numpy --------------------------------------------

def skip_cholesky(G, D):
    """The factorisation of svs_bss_img_solve_batched: right-looking Cholesky of G with the right-hand sides carried along;
    a pivot with |d| <= order * 2^-52 * max diag(G) skips its column (dependent on the earlier ones), a pivot below minus
    that is a failure (status 1 + index) and is skipped too.  Returns (|y|^2 per column of D, status, skipped)."""
    A, B = G.copy(), D.copy()
    n = len(A)
    thr = n * 2.0 ** -52 * A.diagonal().max()
    energy, status, skipped = np.zeros(D.shape[1]), 0, 0
    for c in range(n):
        d = A[c, c]
        if d > thr:
            col, y = A[c + 1:, c] / np.sqrt(d), B[c] / np.sqrt(d)
            A[c + 1:, c + 1:] -= np.outer(col, col)
            B[c + 1:] -= np.outer(col, y)
            energy += y * y
        elif abs(d) <= thr:
            skipped += 1
        elif status == 0:
            status = c + 1
    return energy, status, skipped


def test_skip_cholesky_is_cholesky_on_a_regular_system():
    refs, ests = image_cases()["interference"]
    G, D = gram_system(refs.transpose(0, 2, 1).reshape(4, -1), ests[0].T, FLEN)
    energy, status, skipped = skip_cholesky(G, D)
    assert status == 0 and skipped == 0
    np.testing.assert_allclose(energy, cholesky_energy(G, D), rtol=1e-12)


def test_skip_cholesky_reports_an_indefinite_system():
    refs, ests = image_cases()["interference"]
    G, D = gram_system(refs[0].T, ests[0].T, FLEN)
    G[FLEN + 3, FLEN + 3] = -1.0
    assert skip_cholesky(G, D)[1:] == (FLEN + 4, 0)


@pytest.mark.parametrize("flen,n", [(32, 4000), (128, 3000)])
def test_skip_rule_reproduces_the_definition_on_degenerate_images(flen, n):
    refs, ests = degenerate_case(n)
    counts = []

    def energy_of(G, D):
        energy, status, skipped = skip_cholesky(G, D)
        assert status == 0
        counts.append(skipped)
        return energy

    got = ev._image_metrics_from_gram(*gram_terms(refs, ests, flen, energy_of))
    assert counts == [flen, flen, 2 * flen]                                    # L == R; a silent channel; both
    assert_images_close(got, ev.bss_eval_images(refs, ests, flen=flen), 1e-3)


# ---- the window rules of the GPU path, with numpy in place of the library --------------------

class NumpyImageProjections:
    """float64 numpy stand-in for evaluate._gpu_image_projections: per window and solve the Gram system from lagged
    correlations and skip_cholesky.  A (window, solve) in force_bad has status 1."""

    def __init__(self, force_bad=()):
        self.force_bad = set(force_bad)
        self.skipped = []

    def __call__(self, sig, window, hop, nwin, solves, energies, crosses, flen, ws_budget):
        x = sig.numpy()
        energy = np.empty((nwin, len(energies)))
        cross = np.empty((nwin, len(crosses)))
        ys = [np.zeros((nwin, len(ests))) for _, ests in solves]
        status = [np.zeros(nwin, dtype=np.int32) for _ in solves]
        for w in range(nwin):
            s = x[:, w * hop:w * hop + window]
            energy[w] = [np.sum(s[e] * s[e]) for e in energies]
            cross[w] = [np.sum(s[a] * s[b]) for a, b in crosses]
            for q, (refs, ests) in enumerate(solves):
                ys[q][w], status[q][w], skipped = skip_cholesky(*gram_system(s[list(refs)], s[list(ests)], flen))
                self.skipped.append(skipped)
                if (w, q) in self.force_bad:
                    status[q][w] = 1
        return energy, cross, ys, status


def host_f64(x):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(dtype=torch.float64)


def use_numpy_projections(mp, force_bad=()):
    stand_in = NumpyImageProjections(force_bad)
    mp.setattr(ev, "_gpu_image_projections", stand_in)
    mp.setattr(ev, "_device_f64", host_f64)
    return stand_in


def stereo_track(seconds, sr, seed, silent_second=None):
    """(mix, vocal, estimate), each (n, 2): a centre-heavy coloured vocal, a wide accompaniment, an estimate with leakage,
    a wrong balance and noise."""
    rng = np.random.default_rng(seed)
    n = seconds * sr
    v = np.convolve(rng.standard_normal(n), [1.0, 0.5])[:n]
    vocal = np.stack([v + 0.2 * rng.standard_normal(n), 0.9 * v + 0.2 * rng.standard_normal(n)], axis=1)
    acc = 0.5 * rng.standard_normal((n, 2))
    est = vocal * [1.0, 0.8] + 0.1 * acc + 0.05 * rng.standard_normal((n, 2))
    if silent_second is not None:
        vocal[silent_second * sr:(silent_second + 1) * sr] = 0.0
    return vocal + acc, vocal, est


def assert_image_frames_close(got, want, tol=1e-3):
    assert set(got) == set(want) == {"SDR", "ISR", "SIR", "SAR", "NSDR", "start"}
    assert np.array_equal(got["start"], want["start"])
    for k in ev.IMAGE_METRICS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (k, got[k], want[k])
        ok = ~np.isnan(want[k])
        assert np.all(want[k][ok] < 60.0) and np.all(np.abs(got[k][ok] - want[k][ok]) <= tol), (k, got[k], want[k])


W = 1200                                                # window of the window-rule tests; flen stays FILTER_LEN there


def test_gpu_window_rules_silent_window_is_nan_and_budget_does_not_matter(monkeypatch):
    monkeypatch.setattr(ev, "FILTER_LEN", FLEN)
    mix, vocal, est = stereo_track(4, W, seed=21, silent_second=2)
    want = ev.image_metrics_from_waveforms_framewise(mix, vocal, est, W, W)
    assert list(np.isnan(want["SDR"])) == [False, False, True, False] == list(np.isnan(want["NSDR"]))
    use_numpy_projections(monkeypatch)
    monkeypatch.setattr(ev, "bss_eval_images", None)                          # no fallback: not called at all
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = ev.image_metrics_from_waveforms_framewise(mix, vocal, est, W, W, device="gpu")
        small = ev.image_metrics_from_waveforms_framewise(mix, vocal, est, W, W, device="gpu", ws_budget=1)
    assert_image_frames_close(got, want)
    for k in got:
        np.testing.assert_array_equal(got[k], small[k])


@pytest.mark.parametrize("perm", [False, True])
def test_gpu_window_rules_images_framewise_and_degenerate_windows(perm, monkeypatch):
    refs, ests = degenerate_case(3600)
    refs[0, 1200:2400] = 0.0
    want = ev.bss_eval_images_framewise(refs, ests, 1200, 600, perm, FLEN)
    assert np.isnan(want[0][:, 2]).all() and not np.isnan(want[0][:, [0, 1, 3, 4]]).any()
    stand_in = use_numpy_projections(monkeypatch)
    monkeypatch.setattr(ev, "bss_eval_images", None)
    got = ev.bss_eval_images_framewise_gpu(refs, ests, 1200, 600, perm, FLEN)
    assert 2 * FLEN in stand_in.skipped                                        # handled by the rank rule, no fallback
    for g, w in zip(got, want):
        assert g.shape == w.shape == (2, 5) and g.dtype == np.float64
        assert np.array_equal(np.isnan(g), np.isnan(w))
    for k in (0, 1, 3, 4):
        assert_images_close(tuple(v[:, k] for v in got), tuple(v[:, k] for v in want), 1e-3)


def test_gpu_window_rules_fewer_than_two_windows_is_the_whole_track(monkeypatch):
    monkeypatch.setattr(ev, "FILTER_LEN", FLEN)
    mix, vocal, est = stereo_track(2, W, seed=22)
    want = ev.image_metrics_from_waveforms(mix, vocal, est)
    use_numpy_projections(monkeypatch)
    monkeypatch.setattr(ev, "bss_eval_images", None)
    whole = ev.image_metrics_from_waveforms(mix, vocal, est, device="gpu")
    assert whole.keys() == want.keys() == set(ev.IMAGE_METRICS) and all(isinstance(v, float) for v in whole.values())
    for k in want:
        assert abs(whole[k] - want[k]) <= 1e-3, (k, whole[k], want[k])
    for window, hop in [(2 * W, 2 * W), (2 * W + 5, 100), (4 * W, W)]:
        fr = ev.image_metrics_from_waveforms_framewise(mix, vocal, est, window, hop, device="gpu")
        assert list(fr["start"]) == [0]
        for k in ev.IMAGE_METRICS:
            assert fr[k].shape == (1,) and fr[k][0] == whole[k], (k, window, hop)


def test_gpu_window_rules_bad_status_rescores_that_window_with_numpy(monkeypatch):
    monkeypatch.setattr(ev, "FILTER_LEN", FLEN)
    mix, vocal, est = stereo_track(4, W, seed=23)
    want = ev.image_metrics_from_waveforms_framewise(mix, vocal, est, W, W)
    use_numpy_projections(monkeypatch)
    clean = ev.image_metrics_from_waveforms_framewise(mix, vocal, est, W, W, device="gpu")
    use_numpy_projections(monkeypatch, force_bad=[(1, 2), (1, 0)])
    calls, numpy_images = [], ev.bss_eval_images

    def spy(refs, ests, *args, **kwargs):
        calls.append((np.array(refs), np.array(ests)))
        return numpy_images(refs, ests, *args, **kwargs)

    monkeypatch.setattr(ev, "bss_eval_images", spy)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = ev.image_metrics_from_waveforms_framewise(mix, vocal, est, W, W, device="gpu")
    msgs = [str(r.message) for r in rec if issubclass(r.category, RuntimeWarning)]
    assert len(msgs) == 1 and "falls back to the numpy path" in msgs[0]
    others = np.arange(4) != 1
    for k in ev.IMAGE_METRICS:
        assert np.array_equal(got[k][others], clean[k][others]), k
    for k in ("SDR", "ISR", "SIR", "SAR"):
        assert got[k][1] == want[k][1], k                                       # bitwise the numpy result
    assert abs(got["NSDR"][1] - want["NSDR"][1]) <= 1e-9                       # the mixture's SDR needs no solve
    assert len(calls) == 1
    sl = slice(W, 2 * W)
    assert np.array_equal(calls[0][0], np.stack([vocal[sl], (mix - vocal)[sl]]))
    assert np.array_equal(calls[0][1], np.stack([est[sl], (mix - est)[sl]]))


def test_gpu_scorers_reject_more_than_two_sources_or_channels(monkeypatch):
    use_numpy_projections(monkeypatch)
    with pytest.raises(ValueError, match="1 or 2 sources"):
        ev.bss_eval_images_gpu(np.ones((3, 100, 2)), np.ones((3, 100, 2)))
    with pytest.raises(ValueError, match="1 or 2 channels"):
        ev.bss_eval_images_framewise_gpu(np.ones((2, 100, 3)), np.ones((2, 100, 3)), 50, 50)
    with pytest.raises(ValueError, match="device"):
        ev.image_metrics_from_waveforms(np.ones((100, 2)), np.ones((100, 2)), np.ones((100, 2)), device="tpu")


# ---- the C ABI -------------------------------------------------------------------------------

NEW_SYMBOLS = ("svs_bss_img_corr_windows_workspace_bytes", "svs_bss_img_corr_windows",
               "svs_bss_img_solve_batched_workspace_bytes", "svs_bss_img_solve_batched")


@pytest.fixture(scope="module")
def lib():
    from svs_unet_pytorch_amd import build
    build.build_lib(verbose=False)
    return _lib.lib()


def ints(v, t=ctypes.c_int):
    return (t * len(v))(*v)


def test_new_symbols_are_declared_and_bound(lib):
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svs_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f" {name}(" in header, name
        assert getattr(lib, name).argtypes is not None, name
    for macro, least in (("SVS_BSS_IMG_MAX_SIGNALS", 10), ("SVS_BSS_IMG_MAX_PAIRS", 48), ("SVS_BSS_IMG_MAX_REFS", 4)):
        value = int(header.split(f"#define {macro} ")[1].split()[0])
        assert value >= least, macro


def test_image_workspace_queries_are_zero_for_invalid_arguments(lib):
    many = [v for q in range(48) for v in (q % 10, (q + 3) % 10, 512)]
    assert lib.svs_bss_img_corr_windows_workspace_bytes(8192, 10, 48, ints(many)) > 0
    pairs = ints([0, 1, 512, 1, 1, 1])
    assert lib.svs_bss_img_corr_windows_workspace_bytes(8192, 10, 2, pairs) > 0
    too_many = ints([0, 0, 1] * 65)
    for args in [(0, 10, 2, pairs), (8192, 0, 2, pairs), (8192, 10, 0, pairs), (8192, 10, 65, too_many),
                 (8192, 10, 2, None), (8192, 10, 1, ints([0, 0, 513])), (8192, 10, 1, ints([0, 0, 0])),
                 (8192, 10, 1, ints([-1, 0, 5])), (8192, 10, 1, ints([0, 12, 5])), (8192, 1 << 40, 2, pairs)]:
        assert lib.svs_bss_img_corr_windows_workspace_bytes(*args) == 0, args
    one = lib.svs_bss_img_solve_batched_workspace_bytes(1, 4, 512, 4)
    assert one >= (2048 + 64) * 2048 * 8
    assert lib.svs_bss_img_solve_batched_workspace_bytes(70, 4, 512, 4) >= 70 * (one - 4096) > 1 << 31   # 64-bit bases
    for K in (1, 2, 3, 4):
        assert lib.svs_bss_img_solve_batched_workspace_bytes(3, K, 512, 16) > 0
    for args in [(0, 2, 512, 2), (4, 0, 512, 2), (4, 5, 512, 2), (4, 2, 0, 2), (4, 2, 513, 2), (4, 2, 512, 0),
                 (4, 2, 512, 17), (1 << 40, 2, 512, 2)]:
        assert lib.svs_bss_img_solve_batched_workspace_bytes(*args) == 0, args


def test_image_entry_points_reject_invalid_calls_without_touching_the_gpu(lib):
    fake = ctypes.c_void_p(16)
    pairs = ints([0, 1, 512, 1, 1, 1])
    err = lib.svs_last_error_string
    # x, ld, nsig, n, window, hop, nwin, pairs, npairs, out, out_stride, ws, ws_bytes, stream
    call = lib.svs_bss_img_corr_windows
    assert call(None, 1000, 2, 1000, 100, 100, 10, pairs, 2, fake, 513, fake, 1 << 30, None) == -1
    assert b"bad arguments" in err()
    assert call(fake, 1000, 2, 1000, 100, 100, 10, pairs, 2, None, 513, fake, 1 << 30, None) == -1
    assert call(fake, 1000, 2, 1000, 100, 100, 10, None, 2, fake, 513, fake, 1 << 30, None) == -1
    assert call(fake, 1000, 13, 1000, 100, 100, 10, pairs, 2, fake, 513, fake, 1 << 30, None) == -1
    assert call(fake, 1000, 2, 1000, 100, 100, 10, ints([0, 0, 1] * 65), 65, fake, 513, fake, 1 << 30, None) == -1
    assert b"bad arguments" in err()
    assert call(fake, 1000, 2, 1000, 100, 0, 10, pairs, 2, fake, 513, fake, 1 << 30, None) == -1
    assert b"hop = 0" in err()
    assert call(fake, 1000, 2, 1000, 100, 100, 10, pairs, 2, fake, 512, fake, 1 << 30, None) == -1
    assert b"out_stride" in err()
    assert call(fake, 1000, 1, 1000, 100, 100, 10, pairs, 2, fake, 513, fake, 1 << 30, None) == -1
    assert b"out of range" in err()
    assert call(fake, 1000, 2, 1000, 100, 100, 10, pairs, 2, fake, 513, None, 0, None) == -2
    assert b"workspace too small" in err()
    assert call(fake, 1000, 2, 1000, 100, 100, 10, pairs, 2, fake, 513, fake, 100, None) == -2
    g, r = ints([0, 0], ctypes.c_int64), ints([0, 0, 0, 0], ctypes.c_int64)
    # corr, nbatch, K, flen, gram_off, rhs_off, nrhs, ynorm2, status, skipped, ws, ws_bytes, stream
    call = lib.svs_bss_img_solve_batched
    ok = [fake, 2, 1, 512, g, r, 2, fake, fake, fake, fake, 1 << 30, None]
    for at in (0, 4, 5, 7, 8, 9):                                              # each null pointer
        args = list(ok)
        args[at] = None
        assert call(*args) == -1, at
        assert b"bad arguments" in err()
    for at, bad in [(1, 0), (2, 0), (2, 5), (3, 0), (3, 513), (6, 0), (6, 17)]:
        args = list(ok)
        args[at] = bad
        assert call(*args) == -1, (at, bad)
    args = list(ok)
    args[4] = ints([0, -8], ctypes.c_int64)
    assert call(*args) == -1
    assert b"negative offset (system 1)" in err()
    args = list(ok)
    args[10], args[11] = None, 0
    assert call(*args) == -2
    args = list(ok)
    args[11] = 1000
    assert call(*args) == -2
    assert b"workspace too small" in err()


# ---- the command line ------------------------------------------------------------------------

def write_stereo_tracks(tmp_path, sr=8192):
    """a.wav: 2 s stereo in all three folders; b.wav: a mono estimate against stereo mixture and reference."""
    from scipy.io import wavfile
    for d in ("est", "mix", "ref"):
        (tmp_path / d).mkdir()
    for i, name in enumerate(("a.wav", "b.wav")):
        mix, vocal, est = stereo_track(2, sr, seed=70 + i)
        for d, x in (("mix", mix), ("ref", vocal), ("est", est)):
            wavfile.write(tmp_path / d / name, sr, (0.3 * (x[:, 0] if (d, name) == ("est", "b.wav") else x)).astype(np.float32))
    return ["--est", str(tmp_path / "est"), "--mix", str(tmp_path / "mix"), "--ref", str(tmp_path / "ref")]


def test_cli_stereo_writes_five_figures_and_reports_a_channel_mismatch(tmp_path, capsys):
    argv = write_stereo_tracks(tmp_path)
    out = tmp_path / "r.csv"
    res = ev.main(argv + ["--stereo", "--out_csv", str(out)])
    printed = capsys.readouterr().out
    assert [r["track"] for r in res] == ["a"]
    assert "[Error] Failed on b.wav: Channel count mismatch: mix=2, ref=2, est=1" in printed
    with open(out) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == ["track", "SDR", "ISR", "SIR", "SAR", "NSDR"] and len(rows) == 1
    want = ev.compute_image_metrics_for_track(*(str(tmp_path / d / "a.wav") for d in ("mix", "ref", "est")))
    assert all(float(rows[0][k]) == want[k] for k in ev.IMAGE_METRICS)
    assert want["ISR"] < 30.0 and want["SIR"] > want["ISR"]                   # the wrong balance shows in ISR
    assert "a:\t" + ",\t".join(f"{k}={want[k]:.3f} dB" for k in ev.IMAGE_METRICS) + "\n" in printed
    assert "Mean ISR : " in printed
    mix, sr = ev.load_audio_channels(str(tmp_path / "mix" / "a.wav"))
    assert mix.shape == (2 * 8192, 2) and sr == 8192
    np.testing.assert_array_equal(ev.load_mono_audio(str(tmp_path / "mix" / "a.wav"))[0], mix.mean(axis=1))
    assert ev.load_audio_channels(str(tmp_path / "est" / "b.wav"))[0].shape == (2 * 8192, 1)


def test_cli_stereo_framewise_csv(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(ev, "FILTER_LEN", 64)                                  # the frame plumbing, not 512 taps again
    argv = write_stereo_tracks(tmp_path)
    out, frames = tmp_path / "r.csv", tmp_path / "f.csv"
    res = ev.main(argv + ["--stereo", "--frame_window", "1", "--out_csv", str(out), "--frames_csv", str(frames)])
    assert len(res) == 1 and "frames=2/2" in capsys.readouterr().out
    with open(out) as f:
        assert list(csv.DictReader(f).fieldnames) == ["track", "SDR", "ISR", "SIR", "SAR", "NSDR", "frames"]
    with open(frames) as f:
        frows = list(csv.DictReader(f))
    assert list(frows[0]) == ["track", "frame", "start_s", "SDR", "ISR", "SIR", "SAR", "NSDR"] and len(frows) == 2


def test_cli_without_stereo_keeps_the_four_figure_header(tmp_path, capsys):
    argv = write_stereo_tracks(tmp_path)
    out = tmp_path / "r.csv"
    res = ev.main(argv + ["--out_csv", str(out)])
    printed = capsys.readouterr().out
    assert [r["track"] for r in res] == ["a", "b"] and "ISR" not in printed      # the downmix scores both tracks
    with open(out) as f:
        assert list(csv.DictReader(f).fieldnames) == ["track", "SDR", "SIR", "SAR", "NSDR"]
    r = res[0]
    assert f"a:\tSDR={r['SDR']:.3f} dB,\tSIR={r['SIR']:.3f} dB,\tSAR={r['SAR']:.3f} dB,\tNSDR={r['NSDR']:.3f} dB\n" in printed
