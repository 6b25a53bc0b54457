"""The Gram-matrix form of BSS-eval that the GPU path implements (svs_unet_pytorch_amd/evaluate.py, module docstring):
lagged correlations -> block-Toeplitz G -> Cholesky -> |L^-1 D|^2 -> _metrics_from_gram, restated here in float64
numpy and pinned against the numpy bss_eval_sources.  No GPU needed."""
import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular
from scipy.signal import resample_poly

from svs_unet_pytorch_amd import evaluate as ev

F = ev.FILTER_LEN


def corr(x, y, nlags):
    """C_xy[k] = sum_m x[m+k] y[m], 0 <= k < nlags (x zero past its end)."""
    return np.correlate(np.concatenate([x, np.zeros(nlags - 1)]), y, mode="valid")


def projection_energy(refs, e, flen=F):
    """|P e|^2 onto the span of refs delayed by 0 .. flen-1: D^T G^-1 D through a Cholesky factor and a forward solve."""
    K = len(refs)
    p = np.arange(flen)
    d = p[None, :] - p[:, None]                      # q - p
    G = np.empty((K * flen, K * flen))
    for i in range(K):
        for j in range(K):
            cij, cji = corr(refs[i], refs[j], flen), corr(refs[j], refs[i], flen)
            G[i * flen:(i + 1) * flen, j * flen:(j + 1) * flen] = np.where(d >= 0, cij[np.abs(d)], cji[np.abs(d)])
    D = np.concatenate([corr(e, r, flen) for r in refs])
    y = solve_triangular(cholesky(G, lower=True), D, lower=True)
    return float(y @ y)


def gram_bss_eval(refs, ests, compute_permutation=True):
    refs, ests = np.atleast_2d(refs), np.atleast_2d(ests)
    K = refs.shape[0]
    energy = [corr(e, e, 1)[0] for e in ests]
    proj_one = np.array([[projection_energy(refs[i:i + 1], e) for i in range(K)] for e in ests])
    proj_all = [projection_energy(refs, e) for e in ests] if K == 2 else proj_one[:, 0]
    return ev._metrics_from_gram(energy, proj_one, proj_all, compute_permutation)


def assert_bss_close(got, want):
    """|delta| <= 1e-3 dB where numpy reports <= 80 dB; above that, both > 80 dB; the same permutation."""
    for name, g, w in zip(("sdr", "sir", "sar"), got[:3], want[:3]):
        g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
        assert not np.isnan(g).any(), (name, g)
        low = w <= 80.0
        assert np.all(np.abs(g[low] - w[low]) <= 1e-3), (name, g, w)
        assert np.all(g[~low] > 80.0), (name, g, w)
    assert list(got[3]) == list(want[3])


def property_cases():
    """The four cases of tests/test_host.py::test_bss_eval_defining_properties."""
    rng = np.random.default_rng(3)
    n = 16000
    s1, s2 = rng.standard_normal(n), rng.standard_normal(n)
    refs = np.stack([s1, s2])
    filt = np.convolve(s1, [0.5, 0.3, -0.2])[:n]
    noise = rng.standard_normal(n) * 0.1
    return {"filtered": (refs, np.stack([filt, s2])),
            "interference": (refs, np.stack([s1 + 0.1 * s2, s2 + 0.1 * s1])),
            "noise": (refs, np.stack([s1 + noise, s2])),
            "permuted": (refs, np.stack([s2 + 0.05 * s1, s1 + 0.05 * s2]))}


def band_limited_case(n, seed=5):
    """Both sources low-passed to a quarter of the band: G is ill-conditioned the way 8192 Hz music makes it."""
    rng = np.random.default_rng(seed)
    b1, b2 = (resample_poly(resample_poly(rng.standard_normal(n), 1, 4), 4, 1)[:n] for _ in range(2))
    noise = rng.standard_normal((2, n)) * 0.01
    return np.stack([b1, b2]), np.stack([b1 + 0.1 * b2 + noise[0], b2 - 0.2 * b1 + np.convolve(b1, [0.0, 0.05])[:n] + noise[1]])


@pytest.mark.parametrize("case", ["filtered", "interference", "noise", "permuted"])
def test_gram_form_matches_bss_eval_on_property_cases(case):
    refs, ests = property_cases()[case]
    got, want = gram_bss_eval(refs, ests), ev.bss_eval_sources(refs, ests)
    assert_bss_close(got, want)
    if case == "permuted":
        assert list(got[3]) == [1, 0]


def test_gram_form_matches_bss_eval_band_limited():
    refs, ests = band_limited_case(20000)
    assert_bss_close(gram_bss_eval(refs, ests), ev.bss_eval_sources(refs, ests))
    assert_bss_close(gram_bss_eval(refs, ests, False), ev.bss_eval_sources(refs, ests, compute_permutation=False))


def test_gram_form_matches_bss_eval_one_source():
    rng = np.random.default_rng(11)
    s = rng.standard_normal(12000)
    e = np.convolve(s, [0.8, -0.1])[:12000] + 0.05 * rng.standard_normal(12000)
    got, want = gram_bss_eval(s[None], e[None]), ev.bss_eval_sources(s[None], e[None])
    assert_bss_close(got, want)
    assert np.isinf(got[1][0])                       # one source: no interference at all


def test_metrics_from_gram_never_nan():
    """Denominators that round to <= 0 give +inf (as _safe_db does for 0); a zero projection gives -inf."""
    sdr, sir, sar, perm = ev._metrics_from_gram([1.0, 2.0], [[1.0 + 1e-16, 0.0], [0.0, 2.0]], [1.0, 2.0])
    for v in (sdr, sir, sar):
        assert not np.isnan(v).any()
    assert list(perm) == [0, 1] and np.isinf(sdr[0]) and sdr[0] > 0 and np.isinf(sir[1])
    sdr, sir, sar, _ = ev._metrics_from_gram([1.0], [[0.0]], [0.0])
    assert sdr[0] == -np.inf and sir[0] == np.inf and sar[0] == -np.inf


def test_cli_has_device_flag(capsys):
    with pytest.raises(SystemExit):
        ev.main(["--help"])
    out = capsys.readouterr().out
    assert "--device" in out and "{cpu,gpu}" in out


def test_cli_gpu_without_device_exits_with_message(tmp_path, monkeypatch, capsys):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as ex:
        ev.main(["--est", str(tmp_path), "--mix", str(tmp_path), "--ref", str(tmp_path), "--device", "gpu"])
    assert ex.value.code == 1 and "needs a ROCm device" in capsys.readouterr().out
