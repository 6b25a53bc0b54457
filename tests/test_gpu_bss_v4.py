"""BSS-eval v4 on the GPU (svs_bss_img_filters_batched, svs_bss_project_frames, evaluate.bss_eval_v4_gpu,
image_metrics_from_waveforms_v4(device="gpu"), --mode v4 --device gpu) against the float64 definition evaluate.bss_eval_v4 and
its parts, on the four shapes of test_bss_v4.SHAPES.

Bounds: 8 times the worst deviation from the float64 definition measured on an MI355X (2026-10-21), the margin of
test_gpu_loudness.py; a different summation order has room in it, an fp32 value anywhere in the path would show at about 6e-8.
    projection alone   seven sums per frame, |gpu - numpy| / (S0 + sum e^2) of the frame: 2.5e-16, 2.0e-16, 1.9e-16, 1.9e-16 on
                       the four shapes, 1.5e-16 with one source (PROJ_SEEN 2.6e-16, gate 2.1e-15)
    filters            |gpu - np.linalg.solve| / max |C|: 2.1e-15, 1.9e-15, 1.1e-15, 4.0e-16 (COEF_SEEN 2.1e-15, gate 1.7e-14)
    rank-deficient     the scaled sums with the device's own coefficients (identical channels, a silent channel) against the
                       least-squares projection: 3.9e-16 (RANK_SEEN 4.0e-16, gate 3.2e-15)
    end to end         |gpu - numpy| in dB per frame and figure: 1.4e-14, 7.1e-15, 1.1e-14, 7.3e-15, with a zeroed frame
                       1.1e-14, one frame 8.9e-16 (DB_SEEN 1.5e-14, gate 1.2e-13)
The projection error is nine orders of magnitude under the 6e-8 of an fp32 value.
"""
import csv
import ctypes

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import evaluate as ev
from test_bss_gram import corr
from test_bss_v4 import SHAPES, lstsq_v4_sums, v4_case
from test_gpu_bss_images import gpu_img_solve_batched, i64, ints

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = -12345.0

PROJ_SEEN, COEF_SEEN, RANK_SEEN, DB_SEEN = 2.6e-16, 2.1e-15, 4.0e-16, 1.5e-14
PROJ_TOL, COEF_TOL, RANK_TOL, DB_TOL = 8 * PROJ_SEEN, 8 * COEF_SEEN, 8 * RANK_SEEN, 8 * DB_SEEN

_cases = {}


def case(shape):
    """The inputs of a shape and everything numpy says about them, computed once: references and estimates (2, n, nchan),
    time-last copies, the track's filters per source, the seven sums per frame and source, and bss_eval_v4's figures."""
    if shape not in _cases:
        flen, window, hop, n, nchan = shape
        ref, est = v4_case(n, nchan, seed=flen)
        rc, ec = ref.transpose(0, 2, 1), est.transpose(0, 2, 1)
        c_one = [ev._projection_filters(rc[j], ec[j], flen) for j in range(2)]
        c_all = [ev._projection_filters(rc.reshape(2 * nchan, n), ec[j], flen) for j in range(2)]
        nwin = ev.frame_count(n, window, hop)
        sums = np.array([[ev._v4_frame_sums(rc[:, :, w * hop:w * hop + window], ec[j, :, w * hop:w * hop + window], j,
                                            c_one[j], c_all[j]) for j in range(2)] for w in range(nwin)])
        scale = sums[:, :, 0] + np.array([[np.sum(ec[j, :, w * hop:w * hop + window] ** 2) for j in range(2)]
                                          for w in range(nwin)])
        _cases[shape] = dict(ref=ref, est=est, rc=rc, ec=ec, c_one=c_one, c_all=c_all, nwin=nwin, sums=sums, scale=scale,
                             figures=ev.bss_eval_v4(ref, est, window, hop, flen=flen))
    return _cases[shape]


def device_layout(filters):
    """[C (flen, K, nchan) per source] -> the coef array of svs_bss_project_frames: [j][c][i][tau]."""
    return np.ascontiguousarray(np.stack([C.transpose(2, 1, 0) for C in filters]))


def gpu_project(rc, ec, window, hop, nwin, flen, coef_one, coef_all, pad=3):
    """svs_bss_project_frames on reference rows rc and estimate rows ec ((nsrc, nchan, n) each) with device coefficient
    tensors: sums (nwin, nsrc, 7).  The rows have a stride of n + pad, and the words after the sums are checked."""
    nsrc, nchan, n = rc.shape
    R = nsrc * nchan
    sig = torch.zeros(2 * R, n + pad, dtype=torch.float64, device=DEV)
    sig[:R, :n] = torch.from_numpy(np.ascontiguousarray(rc.reshape(R, n)))
    sig[R:, :n] = torch.from_numpy(np.ascontiguousarray(ec.reshape(R, n)))
    sig[:, n:] = 1e6                                                            # what lies past n must never be read
    L = _lib.lib()
    ws = torch.empty(int(L.svs_bss_project_frames_workspace_bytes(window, nwin, nsrc, flen)), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0
    out = torch.full((nwin * nsrc * 7 + 16,), GUARD, dtype=torch.float64, device=DEV)
    _lib.check(L.svs_bss_project_frames(sig.data_ptr(), n + pad, 2 * R, n, window, hop, nwin, flen, nsrc, nchan,
                                        ints(list(range(R))), ints(list(range(R, 2 * R))), coef_one.data_ptr(),
                                        coef_all.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "svs_bss_project_frames")
    got = out.cpu().numpy()
    assert np.all(got[nwin * nsrc * 7:] == GUARD)
    return got[:nwin * nsrc * 7].reshape(nwin, nsrc, 7)


# ---- 1. the projection alone ------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_project_frames_matches_numpy_with_numpy_filters(shape, report):
    flen, window, hop, n, nchan = shape
    c = case(shape)
    assert np.isfinite(c["sums"]).all() and np.all(c["sums"] >= 1e-4 * c["scale"][:, :, None])   # a scaled error means something
    coef_one = torch.from_numpy(device_layout(c["c_one"])).to(DEV)
    coef_all = torch.from_numpy(device_layout(c["c_all"])).to(DEV)
    got = gpu_project(c["rc"], c["ec"], window, hop, c["nwin"], flen, coef_one, coef_all)
    err = float(np.max(np.abs(got - c["sums"]) / c["scale"][:, :, None]))
    ok = report(f"bss_project_frames {shape} rel. to S0 + |e|^2", err, PROJ_TOL)
    again = gpu_project(c["rc"], c["ec"], window, hop, c["nwin"], flen, coef_one, coef_all)
    assert np.array_equal(got, again)                                           # fixed-order sums: the same bits
    assert ok, err


def test_project_frames_one_source_and_the_whole_signal_as_one_frame(report):
    """nsrc = 1 (coef_all is coef_one: pa is p1 bit for bit, S4 is 0) and a frame longer than the signal (window > n)."""
    flen, window, hop, n, nchan = SHAPES[1]
    c = case(SHAPES[1])
    coef = torch.from_numpy(device_layout(c["c_one"][:1])).to(DEV)
    got = gpu_project(c["rc"][:1], c["ec"][:1], n + 77, n + 77, 1, flen, coef, coef)
    want = ev._v4_frame_sums(c["rc"][:1], c["ec"][0], 0, c["c_one"][0], c["c_one"][0])
    assert got[0, 0, 4] == 0.0 and want[4] == 0.0 and got[0, 0, 3] == got[0, 0, 5]
    err = float(np.max(np.abs(got[0, 0] - want)) / (want[0] + np.sum(c["ec"][0] ** 2)))
    assert report("bss_project_frames one source, one frame past n", err, PROJ_TOL), err


# ---- 2. the filters ---------------------------------------------------------------------------

def track_correlations(rc, ec, flen):
    """The whole-track correlation buffer of R reference and R estimate rows and the offsets of the Gram and right-hand-side
    blocks in it, as evaluate._gpu_v4_sums lays them out."""
    R = rc.shape[0]
    chunks = [corr(rc[i], rc[j], flen) for i in range(R) for j in range(R)]
    chunks += [corr(ec[e], rc[i], flen) for e in range(R) for i in range(R)]
    gram = lambda i, j: (i * R + j) * flen
    rhs = lambda e, i: (R * R + e * R + i) * flen
    return torch.from_numpy(np.concatenate(chunks)).to(DEV), gram, rhs


def gpu_filters(corr_dev, nbatch, K, flen, goffs, roffs, nrhs):
    L = _lib.lib()
    ws = torch.empty(int(L.svs_bss_img_filters_batched_workspace_bytes(nbatch, K, flen, nrhs)), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0
    y = torch.empty(nbatch, nrhs, dtype=torch.float64, device=DEV)
    status = torch.full((nbatch,), -7, dtype=torch.int32, device=DEV)
    skipped = torch.full((nbatch,), -7, dtype=torch.int32, device=DEV)
    coef = torch.full((nbatch * nrhs * K * flen + 16,), GUARD, dtype=torch.float64, device=DEV)
    _lib.check(L.svs_bss_img_filters_batched(corr_dev.data_ptr(), nbatch, K, flen, i64(goffs), i64(roffs), nrhs, y.data_ptr(),
                                             status.data_ptr(), skipped.data_ptr(), coef.data_ptr(), ws.data_ptr(),
                                             ws.numel(), _lib.stream_ptr()), "svs_bss_img_filters_batched")
    assert torch.all(coef[nbatch * nrhs * K * flen:] == GUARD)
    return coef[:nbatch * nrhs * K * flen].view(nbatch, nrhs, K * flen), y.cpu().numpy(), status.cpu().numpy(), \
        skipped.cpu().numpy()


def both_filter_calls(rc, ec, flen):
    """The two calls of the driver on (nsrc, nchan, n) rows: (coef_one (nsrc, nchan, nchan*flen), coef_all (1, R, R*flen),
    the calls' other outputs, and the same calls' outputs from svs_bss_img_solve_batched)."""
    nsrc, nchan, n = rc.shape
    R = nsrc * nchan
    corr_dev, gram, rhs = track_correlations(rc.reshape(R, n), ec.reshape(R, n), flen)
    src = [range(j * nchan, (j + 1) * nchan) for j in range(nsrc)]
    one = (nsrc, nchan, flen, [gram(a, b) for s in src for a in s for b in s], [rhs(c, i) for s in src for c in s for i in s],
           nchan)
    all_ = (1, R, flen, [gram(a, b) for a in range(R) for b in range(R)], [rhs(c, i) for c in range(R) for i in range(R)], R)
    got = [gpu_filters(corr_dev, *args) for args in (one, all_)]
    old = [gpu_img_solve_batched(corr_dev, *args) for args in (one, all_)]
    return got[0][0], got[1][0], [g[1:] for g in got], old


@pytest.mark.parametrize("shape", SHAPES)
def test_filters_match_numpy_solve_and_leave_the_solve_as_it_is(shape, report):
    flen, window, hop, n, nchan = shape
    c = case(shape)
    coef_one, coef_all, rest, old = both_filter_calls(c["rc"], c["ec"], flen)
    for (y, status, skipped), (y_old, status_old, skipped_old) in zip(rest, old):
        assert not status.any() and not skipped.any() and not status_old.any() and not skipped_old.any()
        assert np.array_equal(y, y_old)                                         # ynorm2: bit for bit the existing entry's
    want_one, want_all = device_layout(c["c_one"]), device_layout(c["c_all"]).reshape(2 * nchan, -1)
    err = max(float(np.max(np.abs(coef_one.cpu().numpy().reshape(want_one.shape) - want_one)) / np.max(np.abs(want_one))),
              float(np.max(np.abs(coef_all.cpu().numpy()[0] - want_all)) / np.max(np.abs(want_all))))
    assert report(f"bss_img_filters {shape} rel. to max |C|", err, COEF_TOL), err
    again = both_filter_calls(c["rc"], c["ec"], flen)
    assert torch.equal(coef_one, again[0]) and torch.equal(coef_all, again[1])


def test_filters_of_rank_deficient_images_are_zero_where_skipped_and_project_the_same(report):
    """Source 0 with L == R, source 1 with a silent right channel: the rank rule skips flen columns of each own-channel
    system and 2 * flen of the four-channel one; their coefficients are exactly 0, and the projection with the device's
    coefficients is the least-squares projection (lstsq_v4_sums: numpy's minimum-norm solution, another point of the same
    span)."""
    flen, window, hop, n, nchan = SHAPES[1]
    ref, est = v4_case(n, nchan, seed=5)
    ref[0, :, 1] = ref[0, :, 0]
    ref[1, :, 1] = 0.0
    rc, ec = ref.transpose(0, 2, 1), est.transpose(0, 2, 1)
    coef_one, coef_all, rest, old = both_filter_calls(rc, ec, flen)
    for (y, status, skipped), (y_old, status_old, skipped_old) in zip(rest, old):
        assert not status.any() and np.array_equal(skipped, skipped_old) and np.array_equal(y, y_old)
    assert list(rest[0][2]) == [flen, flen] and list(rest[1][2]) == [2 * flen]
    one, all_ = coef_one.cpu().numpy(), coef_all.cpu().numpy()[0]
    assert np.isfinite(one).all() and np.isfinite(all_).all()
    assert np.all(one[:, :, flen:] == 0.0) and np.any(one[:, :, :flen] != 0.0)   # the second channel depends on the first
    assert np.all(all_[:, flen:2 * flen] == 0.0) and np.all(all_[:, 3 * flen:] == 0.0)
    nwin = ev.frame_count(n, window, hop)
    got = gpu_project(rc, ec, window, hop, nwin, flen, coef_one.contiguous(), coef_all.contiguous())
    want = lstsq_v4_sums(rc, ec, window, hop, nwin, flen)
    scale = want[:, :, 0] + np.array([[np.sum(ec[j, :, w * hop:w * hop + window] ** 2) for j in range(2)] for w in range(nwin)])
    err = float(np.max(np.abs(got - want) / scale[:, :, None]))
    assert report("bss_project_frames with the device's rank-deficient filters", err, RANK_TOL), err


# ---- 3. end to end ----------------------------------------------------------------------------

def _numpy_fallback_taken(*args, **kwargs):
    raise AssertionError("the GPU path fell back to the numpy bss_eval_v4")


def gpu_only(fn, *args, **kwargs):
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ev, "bss_eval_v4", _numpy_fallback_taken)
        return fn(*args, **kwargs)


def worst_db(got, want):
    worst = 0.0
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), (g, w)
        ok = ~np.isnan(w)
        assert np.all(np.abs(w[ok]) < 60.0)
        worst = max(worst, float(np.max(np.abs(g[ok] - w[ok]), initial=0.0)))
    return worst


@pytest.mark.parametrize("shape", SHAPES)
def test_bss_eval_v4_gpu_matches_the_definition(shape, report):
    flen, window, hop, n, nchan = shape
    c = case(shape)
    assert not any(np.isnan(v).any() for v in c["figures"])
    got = gpu_only(ev.bss_eval_v4_gpu, c["ref"], c["est"], window, hop, flen=flen)
    err = worst_db(got, c["figures"])
    assert report(f"bss_eval_v4_gpu {shape} dB", err, DB_TOL), err


def test_bss_eval_v4_gpu_zeroed_frame_is_nan_in_both(report):
    flen, window, hop, n, nchan = SHAPES[2]
    ref, est = v4_case(n, nchan, seed=9)
    est[1, 2 * hop:2 * hop + window] = 0.0
    want = ev.bss_eval_v4(ref, est, window, hop, flen=flen)
    assert list(np.isnan(want[0][0])) == [False, False, True, False]
    got = gpu_only(ev.bss_eval_v4_gpu, torch.from_numpy(ref).to(DEV), torch.from_numpy(est), window, hop, flen=flen)
    err = worst_db(got, want)
    assert report("bss_eval_v4_gpu zeroed frame dB", err, DB_TOL), err


@pytest.mark.parametrize("nsrc", [1, 2])
def test_fewer_than_two_frames_is_bss_eval_images_gpu(nsrc, report):
    """One frame: the same figures as the Gram-form path gives, which test_gpu_bss_images.py holds to 1e-3 dB of numpy."""
    flen, _, _, n, nchan = SHAPES[1]
    c = case(SHAPES[1])
    ref, est = c["ref"][:nsrc], c["est"][:nsrc]
    old = ev.bss_eval_images_gpu(ref, est, compute_permutation=False, flen=flen)[:4]
    want = ev.bss_eval_images(ref, est, compute_permutation=False, flen=flen)[:4]
    for window, hop in [(n, n), (n + 5, 7)]:
        got = gpu_only(ev.bss_eval_v4_gpu, ref, est, window, hop, flen=flen)
        assert all(g.shape == (nsrc, 1) for g in got)
        got = tuple(g[:, 0] for g in got)
        for g, o, w in zip(got, old, want):
            fin = np.isfinite(w)                                                # one source: SIR is +inf in all three
            assert np.array_equal(g[~fin], w[~fin]) and np.array_equal(o[~fin], w[~fin])
            assert np.all(np.abs(g[fin] - o[fin]) <= 1e-3 + DB_TOL), (g, o)
            assert report(f"bss_eval_v4_gpu one frame nsrc={nsrc} dB", float(np.max(np.abs(g[fin] - w[fin]), initial=0.0)),
                          DB_TOL), (g, w)


def test_cli_mode_v4_gpu_matches_cpu(tmp_path, capsys):
    from scipy.io import wavfile
    from test_bss_images import stereo_track
    for d in ("est", "mix", "ref"):
        (tmp_path / d).mkdir()
    mix, vocal, est = stereo_track(3, 8192, seed=35, silent_second=1)
    for d, x in (("mix", mix), ("ref", vocal), ("est", est)):
        wavfile.write(tmp_path / d / "a.wav", 8192, (0.3 * x).astype(np.float32))
    for stereo in ([], ["--stereo"]):
        rows, frames, printed = {}, {}, {}
        for device in ("cpu", "gpu"):
            out, fout = tmp_path / f"{device}.csv", tmp_path / f"{device}_frames.csv"
            argv = ["--est", str(tmp_path / "est"), "--mix", str(tmp_path / "mix"), "--ref", str(tmp_path / "ref"), "--mode",
                    "v4", "--out_csv", str(out), "--device", device, "--frames_csv", str(fout)] + stereo
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
