"""Separation-quality evaluation -- same command line and CSV as the reference's evaluate.py
(/root/reference/evaluate.py:87-182): vocal SDR / SIR / SAR from BSS-eval on the 2-source problem
(vocal, mixture - vocal) and NSDR = SDR(estimate) - SDR(mixture taken as the estimate) (evaluate.py:26-84).

    python -m svs_unet_pytorch_amd.evaluate --est out_wav --mix test/mixture_wav --ref test/vocal_wav [--out_csv r.csv]

This is host code outside the accelerated path: the metric runs once per song on the CPU in the
reference too.  The reference delegates to `mir_eval.separation.bss_eval_sources` (mir_eval 0.8.2, uv.lock:925-926) and
`librosa.load`, neither of which is installable here -- PARITY UNPINNED.  `bss_eval_sources` below restates the
published BSS-eval v3 algorithm that function implements (Vincent, Gribonval, Fevotte 2006; 512-tap time-invariant
distortion filters): the estimate is projected by least squares onto the span of the reference source(s) delayed by
0..511 samples (Gram matrix from FFT cross-correlations, block-Toeplitz), which splits it into target + spatial
distortion, interference and artifacts; SDR / SIR / SAR are the energy ratios of those parts; the source permutation
is the one with the best mean SIR.  tests/test_host.py checks the defining properties (a filtered copy of the
reference scores > 100 dB, a known interference mix scores its mixing ratio, additive noise scores its SNR).
wav files are read with scipy.io.wavfile (mono downmix, native sample rate: evaluate.py:15-23 passes sr=None).

`bss_eval_sources_framewise` / `metrics_from_waveforms_framewise` (CLI `--frame_window`) score windows of a track the way
mir_eval.separation.bss_eval_sources_framewise does.  `bss_eval_sources_gpu`, `bss_eval_sources_framewise_gpu` and
`device="gpu"` of the two metrics functions (CLI `--device gpu`) compute the same metrics with fp64 gfx950 kernels
(csrc/bss.hip) from the Gram-matrix form below; the numpy functions stay the reference they are tested against.  The GPU
path is one path over windows (_gpu_projections, the only caller of the library, for mono sources and stereo images
alike): one windowed correlation pass, then the Gram matrices of all windows factored in batches; a whole signal is its
one-window case.  Per window, an output that needs a factorisation with a pivot that is not > 0 comes from the numpy
bss_eval_sources on that window's slice, with one RuntimeWarning per call.

The Gram-matrix form of _project / _criteria.  References s_0 .. s_{K-1} and an estimate e of length n, zero outside
[0, n); filter length F; x(.-p) is x delayed by p samples.  _project builds
    G[(i,p),(j,q)] = <s_i(.-p), s_j(.-q)> = R_ij[q-p],  R_ij[k] = sum_m s_i[m+k] s_j[m],  |k| <= F-1   (its toeplitz block)
    D[(i,p)]       = <s_i(.-p), e>        = sum_m s_i[m-p] e[m],                          0 <= p < F  (its ssef vector)
and the projection of e onto the span S of the delayed references has the energy
    |P_S e|^2 = D_S^T G_S^-1 D_S = |y|^2,   L y = D_S,  G_S = L L^T          (one forward substitution, no back solve).
With j the matched reference, P_j its single-source and P_all the K-source projection, _decompose gives
s_true + e_spat = P_j e, e_interf = P_all e - P_j e and e_artif = e - P_all e; the subspaces are nested, so _criteria is
    SDR = 10 log10( |P_j e|^2   / (|e|^2 - |P_j e|^2) )
    SIR = 10 log10( |P_j e|^2   / (|P_all e|^2 - |P_j e|^2) )
    SAR = 10 log10( |P_all e|^2 / (|e|^2 - |P_all e|^2) )
exactly (_metrics_from_gram).  Only correlations are computed over the track: every R and D is a lagged correlation
C_xy[k] = sum_m x[m+k] y[m], k >= 0 (R_ij[-k] = C_ji[k], D_i(e)[p] = C_{e s_i}[p]), and |e|^2 = C_ee[0].

Stereo stems (`--stereo`): `bss_eval_images` / `bss_eval_images_framewise` restate mir_eval.separation.bss_eval_images (BSS-eval
v3 images, the measure behind the SiSEC / MUSDB figures; PARITY UNPINNED as above) for sources of shape (nsampl, nchan).  Each
channel e_c of an estimate is projected onto ALL channels of reference source j (P_j) and of all sources (P_all) delayed by
0 .. F-1 samples, and with s_j the true image
    e_spat = P_j e - s_j,   e_interf = P_all e - P_j e,   e_artif = e - P_all e       (sums below over samples and channels)
    SDR = |s_j|^2 / |e - s_j|^2,  ISR = |s_j|^2 / |e_spat|^2,  SIR = |P_j e|^2 / |e_interf|^2,  SAR = |P_all e|^2 / |e_artif|^2.
ISR, the image-to-spatial-distortion ratio, is the figure that reacts to a wrong stereo balance or to swapped channels.
The Gram form of the images (_image_metrics_from_gram).  Per estimate a and source j, summed over channels c:
    E_s = sum |s_jc|^2,  E_e = sum |e_c|^2,  X = sum <s_jc, e_c>,  P1 = sum |P_j e_c|^2,  Pa = sum |P_all e_c|^2
    SDR = E_s / (E_e - 2 X + E_s)        |e - s|^2 expanded: only lag-0 terms, no projection
    ISR = E_s / (P1 - 2 X + E_s)         |P_j e_c - s_jc|^2 = |P_j e_c|^2 - 2 <P_j e_c, s_jc> + |s_jc|^2, and s_jc (delay 0 of
                                         channel c of source j) lies in the span P_j projects onto, so <P_j e_c, s_jc> = <e_c, s_jc>
    SIR = P1 / (Pa - P1),   SAR = Pa / (E_e - Pa)            the spans are nested, as in the mono case
with every P a |y|^2 of a system whose references are the nchan (P_j) or nsrc * nchan (P_all) reference channels: order up to
4 * 512 = 2048 for a stereo two-source problem.  Such G are singular as a rule, not as an exception -- a centre-panned vocal
has L == R, a hard-panned stem a silent channel -- so the image entry points run the mono factorisation under another pivot
rule that skips dependent columns (include/svs_hip.h, svs_bss_img_solve_batched): the projection onto the remaining columns
is the projection onto the same span.  The numpy reference is shared the same way: _project and _decompose are the
one-channel cases of _project_images and _decompose_images.

BSS-eval v4 (`--mode v4`): `bss_eval_v4` restates the mode in which MUSDB18 / SiSEC results are published (museval's default;
PARITY UNPINNED as above): the 512-tap filters are estimated once from the whole track (_projection_filters, the solve that
_project_images shares), applied to every frame's references (_apply_filters), and SDR / ISR / SIR / SAR are taken per frame,
the track's figure being the median over frames.  Inside a frame the spans are not nested, so no Gram form serves:
`bss_eval_v4_gpu` gets the coefficients from svs_bss_img_filters_batched (the image solve plus a back substitution) and the
seven per-frame energies from svs_bss_project_frames (csrc/bss_v4.hip), which applies the filters without storing a signal.

Melody (`--melody`): BSS-eval says how much accompaniment leaked into the vocal, not whether its melody survived.  `melody_for_track`
tracks the reference and the estimated vocal (mono downmix, the file's rate) with the same YIN parameters (f0.py: f0.track_gpu under
`--device gpu`, the float64 definition f0.yin_reference otherwise) and scores the estimate's track against the reference's with the
five frame-level measures of the MIREX melody task (f0.melody_metrics): VR, VFA, RPA, RCA, OA, as fractions.  `--rms_gate_db` (-50 dB
re full scale by default in this mode) makes the silent passages of the reference count as unvoiced.  `--f0_smooth` decodes both
tracks with the same default costs (f0.py smooth=True; csrc/f0_smooth.hip on the device): RPA and OA then measure the stem, not the raw
tracker's own octave flips.
"""
from __future__ import annotations

import argparse
import csv
import glob
import itertools
import os
import sys
import warnings

import numpy as np

FILTER_LEN = 512
METRICS = ("SDR", "SIR", "SAR", "NSDR")
IMAGE_METRICS = ("SDR", "ISR", "SIR", "SAR", "NSDR")     # --stereo: ISR between SDR and SIR
WS_BUDGET = 1 << 30          # default workspace bytes of one batch of framewise factorisations
MAX_BATCH = 1024             # systems per batched factorisation (the kernels' grid limit is far above this)


def load_audio_channels(path):
    """wav -> (float64 (n, nchan) waveform, sample rate): every channel kept (a mono file is nchan 1), the file's own rate."""
    from scipy.io import wavfile
    if not os.path.exists(path):
        raise FileNotFoundError(f"File not found: {path}")
    sr, data = wavfile.read(path)
    if data.dtype.kind == "i":
        data = data.astype(np.float64) / float(np.iinfo(data.dtype).max + 1)
    elif data.dtype.kind == "u":
        data = (data.astype(np.float64) - 128.0) / 128.0
    else:
        data = data.astype(np.float64)
    return (data[:, np.newaxis] if data.ndim == 1 else data), sr


def load_mono_audio(path):
    """wav -> (float64 mono waveform, sample rate); the file's own rate is kept (evaluate.py:15-23)."""
    data, sr = load_audio_channels(path)
    return (data[:, 0] if data.shape[1] == 1 else data.mean(axis=1)), sr


def _project(reference_sources, estimated_source, flen):
    """Least-squares projection of the estimate onto the references delayed by 0 .. flen-1 samples: _project_images with
    one estimate row."""
    return _project_images(reference_sources, estimated_source[np.newaxis], flen)[0]


def _decompose(reference_sources, estimated_source, j, flen):
    """estimate = s_true + e_spat + e_interf + e_artif with respect to reference source j: _decompose_images of
    one-channel images."""
    parts = _decompose_images(reference_sources[:, :, np.newaxis], estimated_source[:, np.newaxis], j, flen)
    return tuple(v[0] for v in parts)


def _safe_db(num, den):
    return np.inf if den == 0 else 10.0 * np.log10(num / den)


def _criteria(s_true, e_spat, e_interf, e_artif):
    s_filt = s_true + e_spat
    sdr = _safe_db(np.sum(s_filt ** 2), np.sum((e_interf + e_artif) ** 2))
    sir = _safe_db(np.sum(s_filt ** 2), np.sum(e_interf ** 2))
    sar = _safe_db(np.sum((s_filt + e_interf) ** 2), np.sum(e_artif ** 2))
    return sdr, sir, sar


def bss_eval_sources(reference_sources, estimated_sources, compute_permutation=True, flen=FILTER_LEN):
    """(sdr, sir, sar, perm) per reference source, as mir_eval.separation.bss_eval_sources returns them
    (evaluate.py:58,74): perm[i] is the index of the estimate matched to reference i."""
    ref = np.atleast_2d(np.asarray(reference_sources, dtype=np.float64))
    est = np.atleast_2d(np.asarray(estimated_sources, dtype=np.float64))
    if ref.shape != est.shape:
        raise ValueError(f"reference {ref.shape} and estimate {est.shape} must have the same shape")
    nsrc = ref.shape[0]
    if not compute_permutation:
        out = np.array([_criteria(*_decompose(ref, est[j], j, flen)) for j in range(nsrc)])
        return out[:, 0], out[:, 1], out[:, 2], np.arange(nsrc)
    sdr, sir, sar = (np.empty((nsrc, nsrc)) for _ in range(3))
    for jest in range(nsrc):
        for jtrue in range(nsrc):
            sdr[jest, jtrue], sir[jest, jtrue], sar[jest, jtrue] = _criteria(*_decompose(ref, est[jest], jtrue, flen))
    popt, idx = _best_sir_permutation(sir), np.arange(nsrc)
    return sdr[popt, idx], sir[popt, idx], sar[popt, idx], np.asarray(popt)


def _db(num, den):
    """10 log10(num / den) of the Gram form: a denominator that rounded to <= 0 is +inf (as _safe_db for 0), never NaN."""
    if den <= 0.0:
        return np.inf
    return -np.inf if num <= 0.0 else 10.0 * np.log10(num / den)


def _metrics_from_gram(energy, proj_one, proj_all, compute_permutation=True):
    """(sdr, sir, sar, perm) of bss_eval_sources from projection energies (the formulas in the module docstring).
    energy[a] = |e_a|^2; proj_one[a, i] = |P_i e_a|^2 (estimate a onto reference i alone); proj_all[a] = |P_all e_a|^2
    (onto all K references; proj_one[:, 0] when K == 1).  Same permutation rule as bss_eval_sources: best mean SIR."""
    energy = np.asarray(energy, dtype=np.float64)
    proj_one = np.asarray(proj_one, dtype=np.float64)
    proj_all = np.asarray(proj_all, dtype=np.float64)
    nest, nsrc = proj_one.shape
    sdr, sir, sar = (np.empty((nest, nsrc)) for _ in range(3))
    for a in range(nest):
        for i in range(nsrc):
            p1, pa = proj_one[a, i], proj_all[a]
            sdr[a, i] = _db(p1, energy[a] - p1)
            sir[a, i] = _db(p1, pa - p1)
            sar[a, i] = _db(pa, energy[a] - pa)
    idx = np.arange(nsrc)
    if not compute_permutation:
        return sdr[idx, idx], sir[idx, idx], sar[idx, idx], idx
    popt = _best_sir_permutation(sir)
    return sdr[popt, idx], sir[popt, idx], sar[popt, idx], np.asarray(popt)


def _load_track(mix_path, vocal_ref_path, vocal_est_path):
    mix, sr_mix = load_mono_audio(mix_path)
    vocal_ref, sr_ref = load_mono_audio(vocal_ref_path)
    vocal_est, sr_est = load_mono_audio(vocal_est_path)
    if not (sr_mix == sr_ref == sr_est):
        raise ValueError(f"Sample rate mismatch: mix={sr_mix}, ref={sr_ref}, est={sr_est}")
    n = min(len(mix), len(vocal_ref), len(vocal_est))
    return mix[:n], vocal_ref[:n], vocal_est[:n], sr_mix


def compute_metrics_for_track(mix_path, vocal_ref_path, vocal_est_path, device="cpu"):
    """evaluate.py:26-84: vocal SDR / SIR / SAR on (vocal, mixture - vocal) and NSDR against the mixture."""
    mix, vocal_ref, vocal_est, _ = _load_track(mix_path, vocal_ref_path, vocal_est_path)
    return metrics_from_waveforms(mix, vocal_ref, vocal_est, device)


def melody_for_track(vocal_ref_path, vocal_est_path, device="cpu", **options):
    """{"VR", "VFA", "RPA", "RCA", "OA"} of the estimated vocal's pitch track against the reference vocal's: both files as mono at
    their common rate, cut to the shorter one, tracked as two rows of ONE call with the same parameters (options: f0.track_gpu's
    keywords)."""
    from . import f0 as f0m
    ref, sr_ref = load_mono_audio(vocal_ref_path)
    est, sr_est = load_mono_audio(vocal_est_path)
    if sr_ref != sr_est:
        raise ValueError(f"Sample rate mismatch: ref={sr_ref}, est={sr_est}")
    n = min(len(ref), len(est))
    both = np.stack([ref[:n], est[:n]]).astype(np.float32)
    if device == "gpu":
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("the GPU tracker needs a ROCm device (gfx950 kernels, no CPU path; use device='cpu')")
        track = f0m.track_gpu(torch.from_numpy(both).to("cuda"), sr_ref, **options)
        f0, voiced = track.f0.cpu().numpy(), track.voiced.cpu().numpy()
    elif device == "cpu":
        track = f0m.yin_reference(both, sr_ref, **options)[0]
        f0, voiced = track.f0, track.voiced
    else:
        raise ValueError(f"device must be 'cpu' or 'gpu', got {device!r}")
    return f0m.melody_metrics(f0[0], voiced[0], f0[1], voiced[1])


def frame_samples(seconds, sr):
    """--frame_window / --frame_hop seconds -> samples: int(round(seconds * sr)), at least one."""
    s = int(round(seconds * sr))
    if s < 1:
        raise ValueError(f"{seconds} s at {sr} Hz is less than one sample")
    return s


def compute_frame_metrics_for_track(mix_path, vocal_ref_path, vocal_est_path, window_s, hop_s=None, device="cpu"):
    """metrics_from_waveforms_framewise of one track, windows given in seconds (hop: the window by default); adds
    "start_s", the start of each frame in seconds."""
    mix, vocal_ref, vocal_est, sr = _load_track(mix_path, vocal_ref_path, vocal_est_path)
    window = frame_samples(window_s, sr)
    hop = frame_samples(window_s if hop_s is None else hop_s, sr)
    frames = metrics_from_waveforms_framewise(mix, vocal_ref, vocal_est, window, hop, device)
    frames["start_s"] = frames["start"] / sr
    return frames


def frame_summary(frames, metrics=METRICS):
    """The NaN-ignoring median of each metric over a track's frames and the number of valid frames (SDR not NaN)."""
    out = {}
    for k in metrics:
        v = np.asarray(frames[k], dtype=np.float64)
        v = v[~np.isnan(v)]
        out[k] = float(np.median(v)) if v.size else float("nan")
    out["frames"] = int(np.count_nonzero(~np.isnan(frames["SDR"])))
    return out


def metrics_from_waveforms(mix, vocal_ref, vocal_est, device="cpu"):
    """{"SDR", "SIR", "SAR", "NSDR"} of the vocal.  device="gpu": the one-window case of _vocal_metrics_gpu, with the
    permutation."""
    if device == "gpu":
        frames = _vocal_metrics_gpu(mix, vocal_ref, vocal_est, None, None, compute_permutation=True)
        return {k: float(frames[k][0]) for k in METRICS}
    if device != "cpu":
        raise ValueError(f"device must be 'cpu' or 'gpu', got {device!r}")
    sources_ref = np.stack([vocal_ref, mix - vocal_ref], axis=0)
    sources_est = np.stack([vocal_est, mix - vocal_est], axis=0)
    sdr, sir, sar, perm = bss_eval_sources(sources_ref, sources_est)
    v = int(perm[0])                                   # estimate matched to the vocal reference (evaluate.py:62)
    sdr_mix, _, _, _ = bss_eval_sources(vocal_ref[None, :], mix[None, :])
    return {"SDR": float(sdr[v]), "SIR": float(sir[v]), "SAR": float(sar[v]), "NSDR": float(sdr[v]) - float(sdr_mix[0])}


# ---- framewise ------------------------------------------------------------------------------

def frame_count(n, window, hop):
    """Windows of mir_eval's bss_eval_sources_framewise: floor((n - window + hop) / hop) (< 2: score the whole signal)."""
    return (n - window + hop) // hop


def _frame_args(window, hop):
    for name, v in (("window", window), ("hop", hop)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    return int(window), int(hop)


def _sources_2d(x, what):
    x = np.asarray(x, dtype=np.float64)
    x = x[np.newaxis, :] if x.ndim == 1 else x
    if x.ndim != 2:
        raise ValueError(f"{what} must be 1-D or (nsrc, nsampl), got shape {x.shape}")
    return x


def _any_silent(sources):
    return bool(np.any(np.all(sources == 0, axis=1)))


def bss_eval_sources_framewise(reference_sources, estimated_sources, window=30 * 44100, hop=15 * 44100,
                               compute_permutation=False, flen=FILTER_LEN):
    """(sdr, sir, sar, perm), each (nsrc, nwin): bss_eval_sources of every window [k*hop, k*hop + window) of the signals,
    as mir_eval.separation.bss_eval_sources_framewise (mir_eval 0.8.2) returns them.  PARITY UNPINNED: mir_eval is not
    installed here, and these rules restate its source.  nwin = frame_count(n, window, hop); when it is < 2 the result is
    bss_eval_sources of the whole signals with a trailing axis of length 1.  A window in which a reference or an estimate is
    all zeros is NaN in all four outputs."""
    ref, est = _sources_2d(reference_sources, "reference"), _sources_2d(estimated_sources, "estimate")
    if ref.shape != est.shape:
        raise ValueError(f"reference {ref.shape} and estimate {est.shape} must have the same shape")
    window, hop = _frame_args(window, hop)
    nsrc, n = ref.shape
    nwin = frame_count(n, window, hop)
    if nwin < 2:
        return tuple(np.expand_dims(v, -1) for v in bss_eval_sources(ref, est, compute_permutation, flen))
    sdr, sir, sar, perm = (np.full((nsrc, nwin), np.nan) for _ in range(4))
    for k in range(nwin):
        r, e = ref[:, k * hop:k * hop + window], est[:, k * hop:k * hop + window]
        if not (_any_silent(r) or _any_silent(e)):
            sdr[:, k], sir[:, k], sar[:, k], perm[:, k] = bss_eval_sources(r, e, compute_permutation, flen)
    return sdr, sir, sar, perm


def _frames(sdr, sir, sar, sdr_mix, hop):
    return {"SDR": sdr, "SIR": sir, "SAR": sar, "NSDR": sdr - sdr_mix, "start": np.arange(sdr.size) * hop}


def metrics_from_waveforms_framewise(mix, vocal_ref, vocal_est, window, hop, device="cpu", ws_budget=WS_BUDGET):
    """Framewise metrics_from_waveforms: {"SDR", "SIR", "SAR", "NSDR", "start"}, 1-D arrays over the windows of
    bss_eval_sources_framewise (start: first sample of each window).  The 2-source problem (vocal, mix - vocal) against
    (estimate, mix - estimate) is scored without a permutation, so the vocal is row 0; NSDR = SDR - SDR(mixture taken as
    the vocal estimate), NaN where the vocal or the mixture is silent.  device="gpu": one windowed correlation pass and
    batched factorisations; ws_budget caps the workspace of one batch (the results do not depend on it)."""
    if device == "gpu":
        return _vocal_metrics_gpu(mix, vocal_ref, vocal_est, window, hop, False, ws_budget)
    if device != "cpu":
        raise ValueError(f"device must be 'cpu' or 'gpu', got {device!r}")
    mix, vocal_ref, vocal_est = (np.asarray(x, dtype=np.float64) for x in (mix, vocal_ref, vocal_est))
    sdr, sir, sar, _ = bss_eval_sources_framewise(np.stack([vocal_ref, mix - vocal_ref]),
                                                  np.stack([vocal_est, mix - vocal_est]), window, hop)
    sdr_mix = bss_eval_sources_framewise(vocal_ref, mix, window, hop)[0][0]
    return _frames(sdr[0], sir[0], sar[0], sdr_mix, _frame_args(window, hop)[1])


# ---- the GPU path ---------------------------------------------------------------------------
# A whole signal is one window (window = hop = n); the windows of bss_eval_sources_framewise are the same call with more of
# them.  Per window: a silent row -> NaN (only with two or more windows); a factorisation that met a bad pivot -> the
# outputs that need it come from the numpy bss_eval_sources on that window's slice (_host_windows).

def _device_f64(x):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("the GPU BSS-eval needs a ROCm device (fp64 gfx950 kernels, no CPU path; use device='cpu')")
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=t.device if t.is_cuda else torch.device("cuda"), dtype=torch.float64)


# entry points of the two families; the image family takes up to 4 reference rows per solve and fills a `skipped` buffer
_ENTRY = {False: ("svs_bss_corr_windows", "svs_bss_solve_batched"),
          True: ("svs_bss_img_corr_windows", "svs_bss_img_solve_batched")}


def _gpu_projections(sig, window, hop, nwin, solves, energies, crosses, flen, ws_budget, images):
    """Projection energies of the Gram form for every window [w*hop, w*hop + window) of the rows of `sig` ((S, n) float64 on
    a ROCm device): ONE windowed correlation pass, then per solve batched factorisations over all windows, in batches whose
    workspace stays within ws_budget bytes (at least one system).  solves: [(reference rows, estimate rows)], one Cholesky
    factorisation per window each; energies: rows whose |x|^2 is wanted; crosses: row pairs (a, b) whose lag-0 term
    <sig[a], sig[b]> is wanted.  images: the image entry points (up to 4 reference rows per solve, rank-deficient Gram
    matrices handled on the device) instead of the mono ones.  Returns numpy (energy (nwin, len(energies)), cross (nwin,
    len(crosses)), [|P e|^2 (nwin, nrhs) per solve], [status (nwin,) per solve]); a status that is not 0 marks a window
    whose factorisation met a bad pivot: mono, one that was not > 0 (singular G: _project then solves by least squares);
    images, one below minus the rank tolerance (G numerically indefinite)."""
    import torch
    from . import _lib
    L = _lib.lib()
    corr_name, solve_name = _ENTRY[bool(images)]
    corr_fn, solve_fn = getattr(L, corr_name), getattr(L, solve_name)
    corr_bytes, solve_bytes = getattr(L, corr_name + "_workspace_bytes"), getattr(L, solve_name + "_workspace_bytes")
    pairs, off = [], {}

    def need(a, b, nl):                              # offset of pair (a, b, nl) in one window's correlations
        if (a, b, nl) not in off:
            off[(a, b, nl)] = sum(p[2] for p in pairs)
            pairs.append((a, b, nl))
        return off[(a, b, nl)]

    plans, ycols = [], 0
    for refs, ests in solves:
        gram = [need(i, j, flen) for i in refs for j in refs]
        rhs = [need(e, i, flen) for e in ests for i in refs]
        k, nr = len(refs), len(ests)
        nb = int(max(1, min(nwin, MAX_BATCH, ws_budget // solve_bytes(1, k, flen, nr))))
        plans.append((k, np.asarray(gram, dtype=np.int64), np.asarray(rhs, dtype=np.int64), nr, nb, ycols))
        ycols += nr
    eoff = [need(e, e, 1) for e in energies]
    xoff = [need(a, b, 1) for a, b in crosses]
    stride = sum(p[2] for p in pairs)
    flat = np.asarray([v for p in pairs for v in p], dtype=np.int32)
    dev = sig.device
    n = sig.shape[1]
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr()
        ws_bytes = corr_bytes(window, nwin, len(pairs), flat.ctypes.data)
        if ws_bytes == 0:
            raise ValueError(f"{nwin} windows of {window} samples and {len(pairs)} pairs do not fit one correlation launch")
        # one workspace and one result buffer of each kind for the whole call: the launches share a stream, and every
        # copy back to the host is a synchronisation
        ws_bytes = max([ws_bytes] + [solve_bytes(nb, k, flen, nr) for k, _, _, nr, nb, _ in plans])
        ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
        corr = torch.empty(nwin, stride, dtype=torch.float64, device=dev)
        _lib.check(corr_fn(sig.data_ptr(), sig.stride(0), sig.shape[0], n, window, hop, nwin, flat.ctypes.data, len(pairs),
                           corr.data_ptr(), stride, ws.data_ptr(), ws.numel(), stream), corr_name)
        y = torch.empty(nwin * ycols, dtype=torch.float64, device=dev)      # per solve a contiguous (nwin, nrhs) block
        status = torch.empty(len(plans), nwin, dtype=torch.int32, device=dev)
        skipped = torch.empty(len(plans), nwin, dtype=torch.int32, device=dev) if images else None
        for s, (k, gram, rhs, nr, nb, y0) in enumerate(plans):
            for w0 in range(0, nwin, nb):
                b = min(nb, nwin - w0)
                base = np.arange(w0, w0 + b, dtype=np.int64)[:, None] * stride
                g, r = np.ascontiguousarray(base + gram), np.ascontiguousarray(base + rhs)
                extra = (skipped[s, w0:].data_ptr(),) if images else ()
                _lib.check(solve_fn(corr.data_ptr(), b, k, flen, g.ctypes.data, r.ctypes.data, nr,
                                    y[nwin * y0 + w0 * nr:].data_ptr(), status[s, w0:].data_ptr(), *extra, ws.data_ptr(),
                                    ws.numel(), stream), solve_name)
        energy, y, status = (t.cpu().numpy() for t in (corr[:, eoff], y, status))
        cross = corr[:, xoff].cpu().numpy() if xoff else np.empty((nwin, 0))
    return (energy, cross, [y[nwin * y0:nwin * (y0 + nr)].reshape(nwin, nr) for _, _, _, nr, _, y0 in plans],
            list(status))


def _gpu_window_projections(sig, window, hop, nwin, solves, energies, flen, ws_budget):
    """_gpu_projections through the mono entry points, without cross terms: (energy, [|P e|^2 per solve], [status per
    solve]).  The seam at which the host tests put numpy in place of the library."""
    energy, _, y, status = _gpu_projections(sig, window, hop, nwin, solves, energies, [], flen, ws_budget, images=False)
    return energy, y, status


def _gpu_image_projections(sig, window, hop, nwin, solves, energies, crosses, flen, ws_budget):
    """_gpu_projections through the image entry points: (energy, cross, [|P e|^2 per solve], [status per solve]).  The
    seam at which the host tests put numpy in place of the library."""
    return _gpu_projections(sig, window, hop, nwin, solves, energies, crosses, flen, ws_budget, images=True)


def _windows(n, window, hop):
    """(window, hop, nwin, framed) of a signal of n samples.  window None, or fewer than two windows: one window that is the
    whole signal, not framed (no silence rule)."""
    if window is not None:
        window, hop = _frame_args(window, hop)
        nwin = frame_count(n, window, hop)
        if nwin >= 2:
            return window, hop, nwin, True
    return n, n, 1, False


_FALLBACK_WARNING = ("BSS-eval: a Gram matrix has a pivot that is not > 0 in the GPU Cholesky (singular or numerically "
                     "indefinite); scoring of the affected window(s) falls back to the numpy path")


def _host_windows(signals, window, hop):
    """slices(w) -> window w of each of `signals` as numpy, for the windows that numpy has to score.  The first use copies
    the signals to the host and gives the one RuntimeWarning of the call (attributed to the caller of the public function)."""
    host = []

    def slices(w):
        if not host:
            warnings.warn(_FALLBACK_WARNING, RuntimeWarning, stacklevel=4)
            host.extend(t.cpu().numpy() for t in signals)
        return [x[..., w * hop:w * hop + window] for x in host]
    return slices


def _sources_gpu(reference_sources, estimated_sources, window, hop, compute_permutation, flen, ws_budget=WS_BUDGET):
    """(sdr, sir, sar, perm), each (nsrc, nwin), of K = 1 or 2 references and K estimates over the windows of _windows
    (perm: float64 when framed, since a silent window is NaN).  Every output of a window needs every solve of that window."""
    import torch
    ref, est = (x.reshape(1, -1) if x.dim() == 1 else x for x in map(_device_f64, (reference_sources, estimated_sources)))
    if ref.dim() != 2 or ref.shape != est.shape:
        raise ValueError(f"reference {tuple(ref.shape)} and estimate {tuple(est.shape)} must have the same 2-D shape")
    nsrc, n = ref.shape
    if nsrc not in (1, 2):
        raise ValueError(f"the GPU BSS-eval handles 1 or 2 sources, got {nsrc} (use bss_eval_sources)")
    if not 1 <= flen <= 512:
        raise ValueError(f"flen = {flen}: the GPU path supports filter lengths 1 .. 512")
    window, hop, nwin, framed = _windows(n, window, hop)
    est = est.to(ref.device)
    refs, ests = list(range(nsrc)), [nsrc + a for a in range(nsrc)]
    solves = [((i,), ests) for i in refs] + ([(tuple(refs), ests)] if nsrc == 2 else [])
    energy, y, status = _gpu_window_projections(torch.cat([ref, est]).contiguous(), window, hop, nwin, solves, refs + ests,
                                                flen, ws_budget)
    host = _host_windows((ref, est), window, hop)
    out = [np.full((nsrc, nwin), np.nan) for _ in range(4)]
    for w in range(nwin):
        if framed and (energy[w] == 0).any():          # a silent reference or estimate
            continue
        if any(s[w] for s in status):
            r = bss_eval_sources(*host(w), compute_permutation, flen)
        else:
            proj_one = np.stack([y[i][w] for i in range(nsrc)], axis=1)
            r = _metrics_from_gram(energy[w, nsrc:], proj_one, y[nsrc][w] if nsrc == 2 else proj_one[:, 0],
                                   compute_permutation)
        for o, v in zip(out, r):
            o[:, w] = v
    if not framed:                                     # no NaN: an integer perm, as bss_eval_sources gives
        out[3] = out[3].astype(np.int64)
    return tuple(out)


def bss_eval_sources_gpu(reference_sources, estimated_sources, compute_permutation=True, flen=FILTER_LEN):
    """bss_eval_sources on the GPU (numpy or torch inputs, K = 1 or 2 sources, flen <= 512): the same (sdr, sir, sar,
    perm).  A singular Gram matrix (e.g. a silent reference) makes the call return the numpy bss_eval_sources result, with
    a RuntimeWarning."""
    return tuple(v[:, 0] for v in _sources_gpu(reference_sources, estimated_sources, None, None, compute_permutation, flen))


def bss_eval_sources_framewise_gpu(reference_sources, estimated_sources, window=30 * 44100, hop=15 * 44100,
                                   compute_permutation=False, flen=FILTER_LEN, ws_budget=WS_BUDGET):
    """bss_eval_sources_framewise on the GPU (numpy or torch inputs, K = 1 or 2 sources, flen <= 512): the same
    (sdr, sir, sar, perm).  Silent windows are NaN from the per-window energies; a window whose Gram matrix is singular
    although no row is silent is scored by the numpy bss_eval_sources, with a RuntimeWarning."""
    return _sources_gpu(reference_sources, estimated_sources, window, hop, compute_permutation, flen, ws_budget)


def _vocal_metrics_gpu(mix, vocal_ref, vocal_est, window, hop, compute_permutation, ws_budget=WS_BUDGET):
    """The frames of metrics_from_waveforms_framewise over the windows of _windows: one windowed correlation pass over
    (vocal, mix - vocal, estimate, mix - estimate, mix), the accompaniments formed on the device as numpy forms them, then
    per window K = 1 on (vocal; est, acc_est, mix) and (acc; est, acc_est) and K = 2.  SDR / SIR / SAR of a window need all
    three solves, the mixture's SDR only the vocal-alone one."""
    import torch
    m, v, ve = _device_f64(mix), _device_f64(vocal_ref), _device_f64(vocal_est)
    v, ve = v.to(m.device), ve.to(m.device)
    if m.dim() != 1 or v.shape != m.shape or ve.shape != m.shape:
        raise ValueError(f"mix {tuple(m.shape)}, vocal {tuple(v.shape)} and estimate {tuple(ve.shape)} must be 1-D of "
                         "one length")
    window, hop, nwin, framed = _windows(m.shape[0], window, hop)
    sig = torch.stack([v, m - v, ve, m - ve, m])     # rows: vocal, accompaniment, their estimates, mixture
    energy, (p_v, p_a, p_all), status = _gpu_window_projections(
        sig, window, hop, nwin, [((0,), [2, 3, 4]), ((1,), [2, 3]), ((0, 1), [2, 3])], [0, 1, 2, 3, 4], FILTER_LEN,
        ws_budget)
    host = _host_windows((m, v, ve), window, hop)
    sdr, sir, sar, sdr_mix = (np.full(nwin, np.nan) for _ in range(4))
    for w in range(nwin):
        if not (framed and (energy[w, :4] == 0).any()):
            if status[0][w] or status[1][w] or status[2][w]:
                hm, hv, he = host(w)
                r = bss_eval_sources(np.stack([hv, hm - hv]), np.stack([he, hm - he]), compute_permutation)
            else:
                r = _metrics_from_gram(energy[w, 2:4], np.stack([p_v[w, :2], p_a[w]], axis=1), p_all[w], compute_permutation)
            j = int(r[3][0])                           # estimate matched to the vocal reference (evaluate.py:62)
            sdr[w], sir[w], sar[w] = r[0][j], r[1][j], r[2][j]
        if not (framed and (energy[w, 0] == 0 or energy[w, 4] == 0)):
            if status[0][w]:
                hm, hv, _ = host(w)
                sdr_mix[w] = bss_eval_sources(hv[None], hm[None], compute_permutation=False)[0][0]
            else:
                sdr_mix[w] = _metrics_from_gram(energy[w, 4:5], p_v[w, 2:3, None], p_v[w, 2:3], compute_permutation=False)[0][0]
    return _frames(sdr, sir, sar, sdr_mix, hop)


# ---- stereo: BSS-eval images ------------------------------------------------------------------

def _projection_filters(reference_channels, estimated_channels, flen):
    """The least-squares filters of _project_images: C (flen, R, nchan), C[tau, i, c] the coefficient of reference row i
    delayed by tau samples in the projection of estimate row c."""
    from scipy.linalg import toeplitz
    nref, nsampl = reference_channels.shape
    nchan = estimated_channels.shape[0]
    refs = np.hstack((reference_channels, np.zeros((nref, flen - 1))))
    est = np.hstack((estimated_channels, np.zeros((nchan, flen - 1))))
    n_fft = int(2 ** np.ceil(np.log2(nsampl + flen - 1.0)))
    sf = np.fft.fft(refs, n=n_fft, axis=1)
    sef = np.fft.fft(est, n=n_fft, axis=1)
    G = np.zeros((nref * flen, nref * flen))
    for i in range(nref):
        for j in range(i + 1):
            ssf = np.real(np.fft.ifft(sf[i] * np.conj(sf[j])))
            ss = toeplitz(np.hstack((ssf[0], ssf[-1:-flen:-1])), r=ssf[:flen])
            G[i * flen:(i + 1) * flen, j * flen:(j + 1) * flen] = ss
            G[j * flen:(j + 1) * flen, i * flen:(i + 1) * flen] = ss.T
    D = np.zeros((nref * flen, nchan))
    for k in range(nref):
        for c in range(nchan):
            ssef = np.real(np.fft.ifft(sf[k] * np.conj(sef[c])))
            D[k * flen:(k + 1) * flen, c] = np.hstack((ssef[0], ssef[-1:-flen:-1]))
    try:
        C = np.linalg.solve(G, D)
    except np.linalg.LinAlgError:
        C = np.linalg.lstsq(G, D, rcond=None)[0]
    return C.reshape(flen, nref, nchan, order="F")


def _apply_filters(C, reference_channels):
    """The filters C (flen, R, nchan) of _projection_filters applied to reference_channels (R, nsampl), zero outside
    [0, nsampl): (nchan, nsampl + flen - 1), the filters' tail included."""
    from scipy.signal import fftconvolve
    flen, nref, nchan = C.shape
    nsampl = reference_channels.shape[1]
    refs = np.hstack((reference_channels, np.zeros((nref, flen - 1))))
    sproj = np.zeros((nchan, nsampl + flen - 1))
    for k in range(nref):
        for c in range(nchan):
            sproj[c] += fftconvolve(C[:, k, c], refs[k])[:nsampl + flen - 1]
    return sproj


def _project_images(reference_channels, estimated_channels, flen):
    """_project for images: every row of estimated_channels (nchan, nsampl) projected onto all rows of reference_channels
    (R, nsampl) delayed by 0 .. flen-1 samples; (nchan, nsampl + flen - 1)."""
    return _apply_filters(_projection_filters(reference_channels, estimated_channels, flen), reference_channels)


def _decompose_images(reference_sources, estimated_source, j, flen):
    """estimate (nsampl, nchan) = s_true + e_spat + e_interf + e_artif with respect to the image of reference source j of
    reference_sources (nsrc, nsampl, nchan); each part (nchan, nsampl + flen - 1)."""
    nsrc, nsampl, nchan = reference_sources.shape
    est = estimated_source.T
    s_true = np.hstack((reference_sources[j].T, np.zeros((nchan, flen - 1))))
    e_spat = _project_images(reference_sources[j].T, est, flen) - s_true
    all_channels = reference_sources.transpose(0, 2, 1).reshape(nsrc * nchan, nsampl)
    e_interf = _project_images(all_channels, est, flen) - s_true - e_spat
    e_artif = -s_true - e_spat - e_interf
    e_artif[:, :nsampl] += est
    return s_true, e_spat, e_interf, e_artif


def _image_criteria(s_true, e_spat, e_interf, e_artif):
    sdr = _safe_db(np.sum(s_true ** 2), np.sum((e_spat + e_interf + e_artif) ** 2))
    isr = _safe_db(np.sum(s_true ** 2), np.sum(e_spat ** 2))
    sir = _safe_db(np.sum((s_true + e_spat) ** 2), np.sum(e_interf ** 2))
    sar = _safe_db(np.sum((s_true + e_spat + e_interf) ** 2), np.sum(e_artif ** 2))
    return sdr, isr, sir, sar


def _images_3d(x, what):
    x = np.asarray(x, dtype=np.float64)
    x = x[:, :, np.newaxis] if x.ndim == 2 else x
    if x.ndim != 3:
        raise ValueError(f"{what} must be (nsrc, nsampl) or (nsrc, nsampl, nchan), got shape {x.shape}")
    return x


def _best_sir_permutation(sir):
    """The rule of bss_eval_sources: sir[estimate, reference] -> perm with the best mean SIR."""
    nsrc = sir.shape[1]
    perms = list(itertools.permutations(range(nsrc)))
    idx = np.arange(nsrc)
    return list(perms[int(np.argmax([np.mean(sir[list(p), idx]) for p in perms]))])


def bss_eval_images(reference_sources, estimated_sources, compute_permutation=True, flen=FILTER_LEN):
    """(sdr, isr, sir, sar, perm) per reference source for images of shape (nsrc, nsampl, nchan), as
    mir_eval.separation.bss_eval_images (mir_eval 0.8.2) returns them.  PARITY UNPINNED: mir_eval is not installed here;
    this restates the published BSS-eval v3 image algorithm (Vincent et al.): every channel of the estimate is projected
    onto all channels of the reference source (e_spat) and of all sources (e_interf) delayed by 0 .. flen-1 samples, and
    the sums of the four ratios run over samples and channels.  perm[i] is the estimate matched to reference i."""
    ref, est = _images_3d(reference_sources, "reference"), _images_3d(estimated_sources, "estimate")
    if ref.shape != est.shape:
        raise ValueError(f"reference {ref.shape} and estimate {est.shape} must have the same shape")
    nsrc = ref.shape[0]
    if not compute_permutation:
        out = np.array([_image_criteria(*_decompose_images(ref, est[j], j, flen)) for j in range(nsrc)])
        return out[:, 0], out[:, 1], out[:, 2], out[:, 3], np.arange(nsrc)
    crit = np.empty((4, nsrc, nsrc))
    for jest in range(nsrc):
        for jtrue in range(nsrc):
            crit[:, jest, jtrue] = _image_criteria(*_decompose_images(ref, est[jest], jtrue, flen))
    popt, idx = _best_sir_permutation(crit[2]), np.arange(nsrc)
    return crit[0][popt, idx], crit[1][popt, idx], crit[2][popt, idx], crit[3][popt, idx], np.asarray(popt)


def _any_silent_image(images):
    return bool(np.any(np.all(images == 0, axis=(1, 2))))


def bss_eval_images_framewise(reference_sources, estimated_sources, window=30 * 44100, hop=15 * 44100,
                              compute_permutation=False, flen=FILTER_LEN):
    """(sdr, isr, sir, sar, perm), each (nsrc, nwin): bss_eval_images of every window [k*hop, k*hop + window), with the
    rules of bss_eval_sources_framewise (PARITY UNPINNED, as there): nwin = frame_count(n, window, hop), fewer than two
    windows score the whole signal, and a window in which a reference or an estimate source is all zeros in every channel
    is NaN in all five outputs."""
    ref, est = _images_3d(reference_sources, "reference"), _images_3d(estimated_sources, "estimate")
    if ref.shape != est.shape:
        raise ValueError(f"reference {ref.shape} and estimate {est.shape} must have the same shape")
    window, hop = _frame_args(window, hop)
    nsrc, n, _ = ref.shape
    nwin = frame_count(n, window, hop)
    if nwin < 2:
        return tuple(np.expand_dims(v, -1) for v in bss_eval_images(ref, est, compute_permutation, flen))
    out = tuple(np.full((nsrc, nwin), np.nan) for _ in range(5))
    for k in range(nwin):
        r, e = ref[:, k * hop:k * hop + window], est[:, k * hop:k * hop + window]
        if not (_any_silent_image(r) or _any_silent_image(e)):
            for o, v in zip(out, bss_eval_images(r, e, compute_permutation, flen)):
                o[:, k] = v
    return out


def _image_metrics_from_gram(e_ref, e_est, cross, proj_one, proj_all, compute_permutation=True):
    """(sdr, isr, sir, sar, perm) of bss_eval_images from channel-summed energies (the image formulas in the module
    docstring).  e_ref[j] = |s_j|^2; e_est[a] = |e_a|^2; cross[a, j] = sum_c <s_jc, e_ac>; proj_one[a, j] = |P_j e_a|^2;
    proj_all[a] = |P_all e_a|^2 (proj_one[:, 0] for one source).  Denominators that rounded to <= 0 follow _db."""
    e_ref, e_est, cross, proj_one, proj_all = (np.asarray(v, dtype=np.float64)
                                               for v in (e_ref, e_est, cross, proj_one, proj_all))
    nest, nsrc = proj_one.shape
    crit = np.empty((4, nest, nsrc))
    for a in range(nest):
        for j in range(nsrc):
            p1, pa = proj_one[a, j], proj_all[a]
            crit[0, a, j] = _db(e_ref[j], e_est[a] - 2.0 * cross[a, j] + e_ref[j])
            crit[1, a, j] = _db(e_ref[j], p1 - 2.0 * cross[a, j] + e_ref[j])
            crit[2, a, j] = _db(p1, pa - p1)
            crit[3, a, j] = _db(pa, e_est[a] - pa)
    idx = np.arange(nsrc)
    popt = _best_sir_permutation(crit[2]) if compute_permutation else list(idx)
    return crit[0][popt, idx], crit[1][popt, idx], crit[2][popt, idx], crit[3][popt, idx], np.asarray(popt)


def _images_gpu(reference_sources, estimated_sources, window, hop, compute_permutation, flen, ws_budget=WS_BUDGET,
                mix=None):
    """((sdr, isr, sir, sar, perm), each (nsrc, nwin); image-SDR (nwin,) of `mix` ((n, nchan)) taken as the estimate of
    source 0, or None) of nsrc = 1 or 2 images of nchan = 1 or 2 channels over the windows of _windows.  Rows of the one
    correlation pass: reference channels (source-major), estimate channels, mixture channels."""
    import torch
    ref, est = (x.unsqueeze(-1) if x.dim() == 2 else x for x in map(_device_f64, (reference_sources, estimated_sources)))
    if ref.dim() != 3 or ref.shape != est.shape:
        raise ValueError(f"reference {tuple(ref.shape)} and estimate {tuple(est.shape)} must have the same "
                         "(nsrc, nsampl, nchan) shape")
    nsrc, n, nchan = ref.shape
    if nsrc not in (1, 2) or nchan not in (1, 2):
        raise ValueError(f"the GPU BSS-eval images handle 1 or 2 sources of 1 or 2 channels, got {nsrc} sources of "
                         f"{nchan} channels (use bss_eval_images)")
    if not 1 <= flen <= 512:
        raise ValueError(f"flen = {flen}: the GPU path supports filter lengths 1 .. 512")
    window, hop, nwin, framed = _windows(n, window, hop)
    est = est.to(ref.device)
    R = nsrc * nchan
    rows = [ref.transpose(1, 2).reshape(R, n), est.transpose(1, 2).reshape(R, n)]
    if mix is not None:
        rows.append(_device_f64(mix).to(ref.device).reshape(n, nchan).t())
    src = [tuple(range(j * nchan, (j + 1) * nchan)) for j in range(nsrc)]
    ests = list(range(R, 2 * R))
    solves = [(s, ests) for s in src] + ([(tuple(range(R)), ests)] if nsrc == 2 else [])
    crosses = [(R + a * nchan + c, j * nchan + c) for a in range(nsrc) for j in range(nsrc) for c in range(nchan)]
    crosses += [(2 * R + c, c) for c in range(nchan)] if mix is not None else []
    nrows = 2 * R + (nchan if mix is not None else 0)
    energy, cross, y, status = _gpu_image_projections(torch.cat(rows).contiguous(), window, hop, nwin, solves,
                                                      list(range(nrows)), crosses, flen, ws_budget)
    e_ref = energy[:, :R].reshape(nwin, nsrc, nchan).sum(axis=2)
    e_est = energy[:, R:2 * R].reshape(nwin, nsrc, nchan).sum(axis=2)
    x = cross[:, :nsrc * R].reshape(nwin, nsrc, nsrc, nchan).sum(axis=3)
    proj = [v.reshape(nwin, nsrc, nchan).sum(axis=2) for v in y]
    host = _host_windows((ref.transpose(1, 2), est.transpose(1, 2)), window, hop)      # time last, as it slices
    out = [np.full((nsrc, nwin), np.nan) for _ in range(5)]
    for w in range(nwin):
        if framed and ((e_ref[w] == 0).any() or (e_est[w] == 0).any()):
            continue
        if any(s[w] for s in status):
            r = bss_eval_images(*(v.transpose(0, 2, 1) for v in host(w)), compute_permutation, flen)
        else:
            proj_one = np.stack([proj[j][w] for j in range(nsrc)], axis=1)
            r = _image_metrics_from_gram(e_ref[w], e_est[w], x[w], proj_one, proj[nsrc][w] if nsrc == 2 else proj_one[:, 0],
                                         compute_permutation)
        for o, v in zip(out, r):
            o[:, w] = v
    if not framed:
        out[4] = out[4].astype(np.int64)
    sdr_mix = None
    if mix is not None:
        e_mix, x_mix = energy[:, 2 * R:].sum(axis=1), cross[:, nsrc * R:].sum(axis=1)
        sdr_mix = np.array([np.nan if framed and (e_ref[w, 0] == 0 or e_mix[w] == 0) else
                            _db(e_ref[w, 0], e_mix[w] - 2.0 * x_mix[w] + e_ref[w, 0]) for w in range(nwin)])
    return tuple(out), sdr_mix


def bss_eval_images_gpu(reference_sources, estimated_sources, compute_permutation=True, flen=FILTER_LEN):
    """bss_eval_images on the GPU (numpy or torch inputs, nsrc and nchan 1 or 2, flen <= 512): the same (sdr, isr, sir,
    sar, perm).  Rank-deficient images (identical or silent channels) are handled on the device; a numerically indefinite
    Gram matrix makes the call return the numpy bss_eval_images result, with a RuntimeWarning."""
    out, _ = _images_gpu(reference_sources, estimated_sources, None, None, compute_permutation, flen)
    return tuple(v[:, 0] for v in out)


def bss_eval_images_framewise_gpu(reference_sources, estimated_sources, window=30 * 44100, hop=15 * 44100,
                                  compute_permutation=False, flen=FILTER_LEN, ws_budget=WS_BUDGET):
    """bss_eval_images_framewise on the GPU (nsrc and nchan 1 or 2, flen <= 512): the same (sdr, isr, sir, sar, perm)."""
    return _images_gpu(reference_sources, estimated_sources, window, hop, compute_permutation, flen, ws_budget)[0]


def _stereo_2d(x, what):
    x = np.asarray(x, dtype=np.float64) if not hasattr(x, "dim") else x
    x = x[:, None] if len(x.shape) == 1 else x
    if len(x.shape) != 2:
        raise ValueError(f"{what} must be (n,) or (n, nchan), got shape {tuple(x.shape)}")
    return x


def _image_sdr_direct(ref, est):
    """10 log10(|s|^2 / |e - s|^2) over samples and channels: the image SDR, which needs no projection."""
    return _safe_db(np.sum(ref ** 2), np.sum((est - ref) ** 2))


def _vocal_image_frames(mix, vocal_ref, vocal_est, window, hop, compute_permutation, device, ws_budget=WS_BUDGET):
    """Frames {"SDR", "ISR", "SIR", "SAR", "NSDR", "start"} of the vocal over the windows of _windows, for (n, nchan)
    waveforms: the problem (vocal, mix - vocal) against (estimate, mix - estimate)."""
    mix, vocal_ref, vocal_est = _stereo_2d(mix, "mix"), _stereo_2d(vocal_ref, "vocal"), _stereo_2d(vocal_est, "estimate")
    if not (tuple(mix.shape) == tuple(vocal_ref.shape) == tuple(vocal_est.shape)):
        raise ValueError(f"mix {tuple(mix.shape)}, vocal {tuple(vocal_ref.shape)} and estimate {tuple(vocal_est.shape)} "
                         "must have one (n, nchan) shape")
    n = mix.shape[0]
    w_, h_, nwin, framed = _windows(n, window, hop)
    if device == "gpu":
        m, v, ve = _device_f64(mix), _device_f64(vocal_ref), _device_f64(vocal_est)
        v, ve = v.to(m.device), ve.to(m.device)
        import torch
        out, sdr_mix = _images_gpu(torch.stack([v, m - v]), torch.stack([ve, m - ve]), window if framed else None, hop,
                                   compute_permutation, FILTER_LEN, ws_budget, mix=m)
    elif device == "cpu":
        ref, est = np.stack([vocal_ref, mix - vocal_ref]), np.stack([vocal_est, mix - vocal_est])
        if framed:
            out = bss_eval_images_framewise(ref, est, w_, h_, compute_permutation, FILTER_LEN)
        else:
            out = tuple(np.expand_dims(v, -1) for v in bss_eval_images(ref, est, compute_permutation, FILTER_LEN))
        sdr_mix = np.full(nwin, np.nan)
        for w in range(nwin):
            s, m = vocal_ref[w * h_:w * h_ + w_], mix[w * h_:w * h_ + w_]
            if not (framed and (not s.any() or not m.any())):
                sdr_mix[w] = _image_sdr_direct(s, m)
    else:
        raise ValueError(f"device must be 'cpu' or 'gpu', got {device!r}")
    sdr, isr, sir, sar, perm = out
    sel = [0 if np.isnan(perm[0, w]) else int(perm[0, w]) for w in range(nwin)]     # estimate matched to the vocal
    pick = lambda v: np.array([v[sel[w], w] for w in range(nwin)])
    sdr = pick(sdr)
    return {"SDR": sdr, "ISR": pick(isr), "SIR": pick(sir), "SAR": pick(sar), "NSDR": sdr - sdr_mix,
            "start": np.arange(nwin) * h_}


def image_metrics_from_waveforms(mix, vocal_ref, vocal_est, device="cpu"):
    """{"SDR", "ISR", "SIR", "SAR", "NSDR"} of the vocal image for (n, nchan) waveforms (a 1-D array is nchan 1):
    bss_eval_images of (vocal, mix - vocal) against (estimate, mix - estimate), with the permutation;
    NSDR = SDR - image-SDR of the mixture taken as the vocal estimate (lag-0 terms only: no projection)."""
    frames = _vocal_image_frames(mix, vocal_ref, vocal_est, None, None, True, device)
    return {k: float(frames[k][0]) for k in IMAGE_METRICS}


def image_metrics_from_waveforms_framewise(mix, vocal_ref, vocal_est, window, hop, device="cpu", ws_budget=WS_BUDGET):
    """Framewise image_metrics_from_waveforms: 1-D arrays over the windows of bss_eval_images_framewise plus "start",
    scored without a permutation; NSDR is NaN where the vocal or the mixture is silent."""
    _frame_args(window, hop)
    return _vocal_image_frames(mix, vocal_ref, vocal_est, window, hop, False, device, ws_budget)


def _load_track_channels(mix_path, vocal_ref_path, vocal_est_path):
    mix, sr_mix = load_audio_channels(mix_path)
    vocal_ref, sr_ref = load_audio_channels(vocal_ref_path)
    vocal_est, sr_est = load_audio_channels(vocal_est_path)
    if not (sr_mix == sr_ref == sr_est):
        raise ValueError(f"Sample rate mismatch: mix={sr_mix}, ref={sr_ref}, est={sr_est}")
    if not (mix.shape[1] == vocal_ref.shape[1] == vocal_est.shape[1]):
        raise ValueError(f"Channel count mismatch: mix={mix.shape[1]}, ref={vocal_ref.shape[1]}, est={vocal_est.shape[1]}")
    if mix.shape[1] > 2:
        raise ValueError(f"--stereo scores 1 or 2 channels, got {mix.shape[1]}")
    n = min(len(mix), len(vocal_ref), len(vocal_est))
    return mix[:n], vocal_ref[:n], vocal_est[:n], sr_mix


def compute_image_metrics_for_track(mix_path, vocal_ref_path, vocal_est_path, device="cpu"):
    """compute_metrics_for_track without the downmix: image_metrics_from_waveforms of the files' channels."""
    mix, vocal_ref, vocal_est, _ = _load_track_channels(mix_path, vocal_ref_path, vocal_est_path)
    return image_metrics_from_waveforms(mix, vocal_ref, vocal_est, device)


def compute_image_frame_metrics_for_track(mix_path, vocal_ref_path, vocal_est_path, window_s, hop_s=None, device="cpu"):
    """compute_frame_metrics_for_track without the downmix (image_metrics_from_waveforms_framewise)."""
    mix, vocal_ref, vocal_est, sr = _load_track_channels(mix_path, vocal_ref_path, vocal_est_path)
    window = frame_samples(window_s, sr)
    hop = frame_samples(window_s if hop_s is None else hop_s, sr)
    frames = image_metrics_from_waveforms_framewise(mix, vocal_ref, vocal_est, window, hop, device)
    frames["start_s"] = frames["start"] / sr
    return frames


# ---- BSS-eval v4: filters from the whole track, figures per frame ------------------------------
# The module docstring's Gram form does not reach this mode.  Inside a frame the track-wide filters are not the frame's own
# least-squares filters, so P_j e and P_all e are no orthogonal projections there, the spans are not nested, and the energies
# of e_spat, e_interf and e_artif do not follow from |P e|^2: the projected signals themselves are needed.

def _v4_figures(sums):
    """(SDR, ISR, SIR, SAR) in dB from the seven sums of bss_eval_v4."""
    return (_safe_db(sums[0], sums[1]), _safe_db(sums[0], sums[2]), _safe_db(sums[3], sums[4]), _safe_db(sums[5], sums[6]))


def _v4_frame_sums(ref_frame, est_frame, j, c_one, c_all):
    """The seven sums of one frame and source j: ref_frame (nsrc, nchan, L), est_frame (nchan, L) of estimate j, and the
    track's filters c_one (flen, nchan, nchan) and c_all (flen, nsrc * nchan, nchan) of that source."""
    flen, frame_len = c_one.shape[0], ref_frame.shape[2]
    pad = np.zeros((ref_frame.shape[1], flen - 1))
    s, e = np.hstack((ref_frame[j], pad)), np.hstack((est_frame, pad))
    p1 = _apply_filters(c_one, ref_frame[j])
    pa = _apply_filters(c_all, ref_frame.reshape(-1, frame_len))
    return np.array([np.sum(s ** 2), np.sum((e - s) ** 2), np.sum((p1 - s) ** 2), np.sum(p1 ** 2), np.sum((pa - p1) ** 2),
                     np.sum(pa ** 2), np.sum((e - pa) ** 2)])


def _v4_args(ref, est, window, hop, compute_permutation):
    if tuple(ref.shape) != tuple(est.shape):
        raise ValueError(f"reference {tuple(ref.shape)} and estimate {tuple(est.shape)} must have the same shape")
    if compute_permutation:
        raise ValueError("BSS-eval v4 scores estimate j against reference j: there is no permutation search here "
                         "(compute_permutation must be False)")
    return _frame_args(window, hop)


def bss_eval_v4(reference_sources, estimated_sources, window, hop, flen=FILTER_LEN, compute_permutation=False):
    """(sdr, isr, sir, sar), each (nsrc, nwin): BSS-eval v4, the mode in which MUSDB18 / SiSEC figures are published and the
    default of museval.evaluate -- the distortion filters are estimated ONCE from the whole track, the figures are taken per
    frame (the track's figure is the median over frames: frame_summary).  PARITY UNPINNED: museval is not installed here;
    this is the float64 definition, restated from the published algorithm as bss_eval_images restates mir_eval.  Images
    (nsrc, nsampl, nchan), a 2-D input being one channel; estimate j is scored against reference j.
      filters   per source j and channel c of its estimate: C_j (onto the channels of reference j) and C_all (onto all
                reference channels), the least-squares filters of _project_images on the WHOLE signals;
      frames    nwin = frame_count(n, window, hop), frame w = [w*hop, w*hop + window); fewer than two: the whole signal is the
                one frame, and the result is bss_eval_images(..., compute_permutation=False); a frame in which a reference or
                an estimate source is all zeros in every channel is NaN in all four outputs;
      per frame the frame's own samples, zero outside it, give p1 = C_j * references of j and pa = C_all * all references over
                L + flen - 1 samples (the filters' tail belongs to the frame, the samples before it do not), and
                _image_criteria of (s, p1 - s, pa - p1, e - pa): SDR = |s|^2 / |e - s|^2, ISR = |s|^2 / |p1 - s|^2,
                SIR = |p1|^2 / |pa - p1|^2, SAR = |pa|^2 / |e - pa|^2, summed over samples and channels."""
    ref, est = _images_3d(reference_sources, "reference"), _images_3d(estimated_sources, "estimate")
    window, hop = _v4_args(ref, est, window, hop, compute_permutation)
    nsrc, n, nchan = ref.shape
    rc, ec = ref.transpose(0, 2, 1), est.transpose(0, 2, 1)                      # time last
    all_channels = rc.reshape(nsrc * nchan, n)
    c_one = [_projection_filters(rc[j], ec[j], flen) for j in range(nsrc)]
    c_all = [_projection_filters(all_channels, ec[j], flen) for j in range(nsrc)]
    window, hop, nwin, framed = _windows(n, window, hop)
    out = np.full((4, nsrc, nwin), np.nan)
    for w in range(nwin):
        r, e = rc[:, :, w * hop:w * hop + window], ec[:, :, w * hop:w * hop + window]
        if framed and (np.any(np.all(r == 0, axis=(1, 2))) or np.any(np.all(e == 0, axis=(1, 2)))):
            continue
        for j in range(nsrc):
            out[:, j, w] = _v4_figures(_v4_frame_sums(r, e[j], j, c_one[j], c_all[j]))
    return tuple(out)


def _gpu_v4_sums(sig, window, hop, nwin, nsrc, nchan, flen, energies, crosses):
    """The device half of bss_eval_v4_gpu, and its only caller of the library.  sig: (S, n) float64 on a ROCm device, rows
    0 .. R-1 the reference channels (source-major, R = nsrc * nchan), rows R .. 2R-1 the estimate channels the same way, then
    whatever else `energies` (rows) and `crosses` (row pairs) name.  ONE whole-track correlation pass, the filter solves (the
    nsrc systems onto a source's own channels in one batch, and for two sources the one system onto all R channels with all R
    estimate channels as right-hand sides), one lag-0 correlation pass over the frames for the energies and cross terms, ONE
    svs_bss_project_frames call, and one read-back.  Returns numpy (sums (nwin, nsrc, 7), energy (nwin, len(energies)), cross
    (nwin, len(crosses)), status (int per system)); a status that is not 0 marks a whole-track Gram matrix that is numerically
    indefinite (the sums are then meaningless).  The seam at which the host tests put numpy in place of the library."""
    import torch
    from . import _lib
    L = _lib.lib()
    S, n = sig.shape
    R = nsrc * nchan
    pairs = [(i, j, flen) for i in range(R) for j in range(R)] + [(R + e, i, flen) for e in range(R) for i in range(R)]
    gram = lambda i, j: (i * R + j) * flen
    rhs = lambda e, i: (R * R + e * R + i) * flen
    lag0 = [(e, e, 1) for e in energies] + [(a, b, 1) for a, b in crosses]
    flat, flat0 = (np.asarray(p, dtype=np.int32).ravel() for p in (pairs, lag0))
    stride, stride0 = len(pairs) * flen, len(lag0)
    src = [range(j * nchan, (j + 1) * nchan) for j in range(nsrc)]
    g_one = np.asarray([gram(a, b) for s in src for a in s for b in s], dtype=np.int64)
    r_one = np.asarray([rhs(c, i) for s in src for c in s for i in s], dtype=np.int64)
    g_all = np.asarray([gram(a, b) for a in range(R) for b in range(R)], dtype=np.int64)
    r_all = np.asarray([rhs(c, i) for c in range(R) for i in range(R)], dtype=np.int64)
    rows = np.arange(2 * R, dtype=np.int32)
    dev = sig.device
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr()
        need = [L.svs_bss_img_corr_windows_workspace_bytes(n, 1, len(pairs), flat.ctypes.data),
                L.svs_bss_img_corr_windows_workspace_bytes(window, nwin, len(lag0), flat0.ctypes.data) if lag0 else 1,
                L.svs_bss_img_filters_batched_workspace_bytes(nsrc, nchan, flen, nchan),
                L.svs_bss_img_filters_batched_workspace_bytes(1, R, flen, R),
                L.svs_bss_project_frames_workspace_bytes(window, nwin, nsrc, flen)]
        if min(need) == 0:
            raise ValueError(f"{nwin} frames of {window} samples do not fit one launch")
        ws = torch.empty(int(max(need)), dtype=torch.uint8, device=dev)
        corr = torch.empty(stride, dtype=torch.float64, device=dev)
        _lib.check(L.svs_bss_img_corr_windows(sig.data_ptr(), sig.stride(0), S, n, n, n, 1, flat.ctypes.data, len(pairs),
                                              corr.data_ptr(), stride, ws.data_ptr(), ws.numel(), stream),
                   "svs_bss_img_corr_windows")
        coef_one = torch.empty(nsrc * nchan * nchan * flen, dtype=torch.float64, device=dev)
        coef_all = torch.empty(R * R * flen, dtype=torch.float64, device=dev) if nsrc == 2 else coef_one
        ynorm2 = torch.empty(R * R + nsrc * nchan, dtype=torch.float64, device=dev)
        words = torch.zeros(2, nsrc + 1, dtype=torch.int32, device=dev)           # status, skipped: per system
        _lib.check(L.svs_bss_img_filters_batched(corr.data_ptr(), nsrc, nchan, flen, g_one.ctypes.data, r_one.ctypes.data,
                                                 nchan, ynorm2.data_ptr(), words[0].data_ptr(), words[1].data_ptr(),
                                                 coef_one.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                   "svs_bss_img_filters_batched")
        if nsrc == 2:
            _lib.check(L.svs_bss_img_filters_batched(corr.data_ptr(), 1, R, flen, g_all.ctypes.data, r_all.ctypes.data, R,
                                                     ynorm2[nsrc * nchan:].data_ptr(), words[0, nsrc:].data_ptr(),
                                                     words[1, nsrc:].data_ptr(), coef_all.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), stream), "svs_bss_img_filters_batched")
        out = torch.empty(nwin * (nsrc * 7 + stride0), dtype=torch.float64, device=dev)     # the sums, then the lag-0 terms
        lag0_out = out[nwin * nsrc * 7:]
        if stride0:
            _lib.check(L.svs_bss_img_corr_windows(sig.data_ptr(), sig.stride(0), S, n, window, hop, nwin, flat0.ctypes.data,
                                                  len(lag0), lag0_out.data_ptr(), stride0, ws.data_ptr(), ws.numel(), stream),
                       "svs_bss_img_corr_windows")
        _lib.check(L.svs_bss_project_frames(sig.data_ptr(), sig.stride(0), S, n, window, hop, nwin, flen, nsrc, nchan,
                                            rows[:R].ctypes.data, rows[R:].ctypes.data, coef_one.data_ptr(),
                                            coef_all.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                   "svs_bss_project_frames")
        out, words = out.cpu().numpy(), words.cpu().numpy()
    sums = out[:nwin * nsrc * 7].reshape(nwin, nsrc, 7)
    lag0_host = out[nwin * nsrc * 7:].reshape(nwin, stride0)
    return sums, lag0_host[:, :len(energies)], lag0_host[:, len(energies):], words[0, :nsrc + (nsrc == 2)]


def _v4_gpu(reference_sources, estimated_sources, window, hop, flen, compute_permutation=False, mix=None):
    """((sdr, isr, sir, sar), each (nsrc, nwin); image-SDR (nwin,) of `mix` ((n, nchan)) taken as the estimate of source 0, or
    None) of bss_eval_v4 through _gpu_v4_sums.  Rows: reference channels (source-major), estimate channels, mixture channels."""
    import torch
    ref, est = (x.unsqueeze(-1) if x.dim() == 2 else x for x in map(_device_f64, (reference_sources, estimated_sources)))
    if ref.dim() != 3:
        raise ValueError(f"reference must be (nsrc, nsampl) or (nsrc, nsampl, nchan), got shape {tuple(ref.shape)}")
    window, hop = _v4_args(ref, est, window, hop, compute_permutation)
    nsrc, n, nchan = ref.shape
    if nsrc not in (1, 2) or nchan not in (1, 2):
        raise ValueError(f"the GPU BSS-eval v4 handles 1 or 2 sources of 1 or 2 channels, got {nsrc} sources of {nchan} "
                         "channels (use bss_eval_v4)")
    if not 1 <= flen <= 512:
        raise ValueError(f"flen = {flen}: the GPU path supports filter lengths 1 .. 512")
    window, hop, nwin, framed = _windows(n, window, hop)
    est = est.to(ref.device)
    R = nsrc * nchan
    rows = [ref.transpose(1, 2).reshape(R, n), est.transpose(1, 2).reshape(R, n)]
    crosses = []
    if mix is not None:
        mix = _device_f64(mix).to(ref.device).reshape(n, nchan)
        rows.append(mix.t())
        crosses = [(2 * R + c, c) for c in range(nchan)]
    nrows = 2 * R + (nchan if mix is not None else 0)
    sums, energy, cross, status = _gpu_v4_sums(torch.cat(rows).contiguous(), window, hop, nwin, nsrc, nchan, flen,
                                               list(range(nrows)), crosses)
    e_ref = energy[:, :R].reshape(nwin, nsrc, nchan).sum(axis=2)
    e_est = energy[:, R:2 * R].reshape(nwin, nsrc, nchan).sum(axis=2)
    if np.any(status):                                 # the track's filters are the whole score: numpy for the track
        warnings.warn(_FALLBACK_WARNING, RuntimeWarning, stacklevel=3)
        out = bss_eval_v4(ref.cpu().numpy(), est.cpu().numpy(), window, hop, flen)
    else:
        out = np.full((4, nsrc, nwin), np.nan)
        for w in range(nwin):
            if not (framed and ((e_ref[w] == 0).any() or (e_est[w] == 0).any())):
                for j in range(nsrc):
                    out[:, j, w] = _v4_figures(sums[w, j])
        out = tuple(out)
    sdr_mix = None
    if mix is not None:                                # lag-0 terms only: no filter enters the mixture's SDR
        e_mix, x_mix = energy[:, 2 * R:].sum(axis=1), cross.sum(axis=1)
        sdr_mix = np.array([np.nan if framed and (e_ref[w, 0] == 0 or e_mix[w] == 0) else
                            _db(e_ref[w, 0], e_mix[w] - 2.0 * x_mix[w] + e_ref[w, 0]) for w in range(nwin)])
    return out, sdr_mix


def bss_eval_v4_gpu(reference_sources, estimated_sources, window, hop, flen=FILTER_LEN, compute_permutation=False):
    """bss_eval_v4 on the GPU (numpy or torch inputs, nsrc and nchan 1 or 2, flen <= 512): the same (sdr, isr, sir, sar).  The
    filters come from one whole-track correlation pass and svs_bss_img_filters_batched, the frames from one
    svs_bss_project_frames call (csrc/bss_v4.hip).  Rank-deficient images (identical or silent channels) are handled on the
    device; a numerically indefinite whole-track Gram matrix makes the call return the numpy bss_eval_v4 result, with a
    RuntimeWarning."""
    return _v4_gpu(reference_sources, estimated_sources, window, hop, flen, compute_permutation)[0]


def image_metrics_from_waveforms_v4(mix, vocal_ref, vocal_est, window, hop, device="cpu"):
    """The frames {"SDR", "ISR", "SIR", "SAR", "NSDR", "start"} of the vocal under BSS-eval v4 for (n, nchan) waveforms (a 1-D
    array is nchan 1): bss_eval_v4 of (vocal, mix - vocal) against (estimate, mix - estimate), the vocal being row 0;
    NSDR = SDR - SDR(mixture taken as the vocal estimate), which needs no filter: the direct ratio per frame, NaN where the
    vocal or the mixture is silent.  frame_summary(frames, IMAGE_METRICS) gives the track's figures."""
    mix, vocal_ref, vocal_est = _stereo_2d(mix, "mix"), _stereo_2d(vocal_ref, "vocal"), _stereo_2d(vocal_est, "estimate")
    if not (tuple(mix.shape) == tuple(vocal_ref.shape) == tuple(vocal_est.shape)):
        raise ValueError(f"mix {tuple(mix.shape)}, vocal {tuple(vocal_ref.shape)} and estimate {tuple(vocal_est.shape)} "
                         "must have one (n, nchan) shape")
    _frame_args(window, hop)
    w_, h_, nwin, framed = _windows(mix.shape[0], window, hop)
    if device == "gpu":
        import torch
        m, v, ve = _device_f64(mix), _device_f64(vocal_ref), _device_f64(vocal_est)
        v, ve = v.to(m.device), ve.to(m.device)
        out, sdr_mix = _v4_gpu(torch.stack([v, m - v]), torch.stack([ve, m - ve]), window, hop, FILTER_LEN, mix=m)
    elif device == "cpu":
        out = bss_eval_v4(np.stack([vocal_ref, mix - vocal_ref]), np.stack([vocal_est, mix - vocal_est]), window, hop,
                          FILTER_LEN)
        sdr_mix = np.full(nwin, np.nan)
        for w in range(nwin):
            s, m = vocal_ref[w * h_:w * h_ + w_], mix[w * h_:w * h_ + w_]
            if not (framed and (not s.any() or not m.any())):
                sdr_mix[w] = _image_sdr_direct(s, m)
    else:
        raise ValueError(f"device must be 'cpu' or 'gpu', got {device!r}")
    sdr, isr, sir, sar = (v[0] for v in out)
    return {"SDR": sdr, "ISR": isr, "SIR": sir, "SAR": sar, "NSDR": sdr - sdr_mix, "start": np.arange(nwin) * h_}


def compute_v4_frame_metrics_for_track(mix_path, vocal_ref_path, vocal_est_path, window_s=1.0, hop_s=None, device="cpu",
                                       stereo=False):
    """image_metrics_from_waveforms_v4 of one track, frames given in seconds (hop: the window by default), of the files'
    channels (stereo) or of their downmix; adds "start_s", the start of each frame in seconds."""
    load = _load_track_channels if stereo else _load_track
    mix, vocal_ref, vocal_est, sr = load(mix_path, vocal_ref_path, vocal_est_path)
    window = frame_samples(window_s, sr)
    hop = frame_samples(window_s if hop_s is None else hop_s, sr)
    frames = image_metrics_from_waveforms_v4(mix, vocal_ref, vocal_est, window, hop, device)
    frames["start_s"] = frames["start"] / sr
    return frames


def main(argv=None):
    parser =argparse.ArgumentParser(description="Evaluate SVS results with SDR / SIR / SAR / NSDR (vocal only).")
    parser.add_argument("--est", type=str, required=True, help="folder of predicted vocal wav files")
    parser.add_argument("--mix", type=str, required=True, help="folder of mixture wav files")
    parser.add_argument("--ref", type=str, required=True, help="folder of reference vocal wav files")
    parser.add_argument("--ext", type=str, default="wav")
    parser.add_argument("--out_csv", type=str, default=None)
    parser.add_argument("--device", choices=["cpu", "gpu"], default="cpu",
                        help="gpu: BSS-eval with the fp64 gfx950 kernels (same metrics and CSV)")
    parser.add_argument("--frame_window", type=float, default=None, metavar="SECONDS",
                        help="framewise BSS-eval over windows of this length: each track reports the median over its "
                             "valid frames and their number")
    parser.add_argument("--frame_hop", type=float, default=None, metavar="SECONDS",
                        help="hop between frames (default: the window)")
    parser.add_argument("--frames_csv", type=str, default=None, metavar="PATH",
                        help="write every frame: track, frame, start_s, SDR, SIR, SAR, NSDR")
    parser.add_argument("--stereo", action="store_true",
                        help="score the files' channels as images (BSS-eval images, no downmix): adds ISR, the figure "
                             "that reacts to a wrong stereo balance")
    parser.add_argument("--mode", choices=["v3", "v4"], default="v3",
                        help="v4: BSS-eval v4, the mode of published MUSDB18 / SiSEC figures (museval's default): filters from "
                             "the whole track, SDR / ISR / SIR / SAR / NSDR per frame (--frame_window, default 1 s), the "
                             "median over frames per track; the downmix is scored unless --stereo is given")
    parser.add_argument("--melody", action="store_true",
                        help="also score the melody: YIN pitch tracks of the estimated and the reference vocal, compared by voicing "
                             "recall / false alarm, raw pitch / chroma accuracy and overall accuracy (VR, VFA, RPA, RCA, OA)")
    parser.add_argument("--f0_smooth", action="store_true",
                        help="with --melody: Viterbi-decode both pitch tracks (7 candidates per frame, the same default costs)")
    parser.add_argument("--rms_gate_db", type=float, default=None, metavar="DB",
                        help="with --melody: frames whose rms lies below this level (dB re full scale) are unvoiced (default -50)")
    args = parser.parse_args(argv)
    if args.rms_gate_db is not None and not args.melody:
        parser.error("--rms_gate_db belongs to --melody")
    if args.f0_smooth and not args.melody:
        parser.error("--f0_smooth belongs to --melody")
    melody = ()
    if args.melody:
        from .f0 import MELODY as melody, MELODY_GATE_DB, gate_from_db
        melody_options = dict(rms_gate=gate_from_db(MELODY_GATE_DB if args.rms_gate_db is None else args.rms_gate_db))
        if args.f0_smooth:
            melody_options["smooth"] = True
    v4 = args.mode == "v4"
    if v4 and args.frame_window is None:
        args.frame_window = 1.0
    metrics = IMAGE_METRICS if args.stereo or v4 else METRICS
    track_metrics = compute_image_metrics_for_track if args.stereo else compute_metrics_for_track
    track_frames = compute_image_frame_metrics_for_track if args.stereo else compute_frame_metrics_for_track
    if v4:
        track_frames = lambda *a: compute_v4_frame_metrics_for_track(*a, stereo=args.stereo)
    framewise = args.frame_window is not None
    if framewise and not args.frame_window > 0:
        parser.error("--frame_window must be > 0")
    if args.frame_hop is not None and not (framewise and args.frame_hop > 0):
        parser.error("--frame_hop must be > 0 and needs --frame_window")
    if args.frames_csv is not None and not framewise:
        parser.error("--frames_csv needs --frame_window")
    if args.device == "gpu":
        import torch
        if not torch.cuda.is_available():
            print("evaluate.py --device gpu needs a ROCm device (the BSS-eval kernels are gfx950 code); use --device cpu.")
            sys.exit(1)
    pred_files = sorted(glob.glob(os.path.join(args.est, f"*.{args.ext}")))
    if not pred_files:
        print(f"[Error] No *.{args.ext} files found in {args.est}")
        return
    print("=== Start Evaluation ===")
    print(f"#tracks = {len(pred_files)}\n")
    results, frame_rows = [], []
    for pred_path in pred_files:
        base = os.path.basename(pred_path)
        mix_path, ref_path = os.path.join(args.mix, base), os.path.join(args.ref, base)
        if not os.path.exists(mix_path):
            print(f"[Warning] Mixture file not found, skip: {mix_path}")
            continue
        if not os.path.exists(ref_path):
            print(f"[Warning] Vocal ref file not found, skip: {ref_path}")
            continue
        try:
            if framewise:
                frames = track_frames(mix_path, ref_path, pred_path, args.frame_window, args.frame_hop, args.device)
                m = frame_summary(frames, metrics)
            else:
                m = track_metrics(mix_path, ref_path, pred_path, args.device)
            if melody:
                m = {**m, **melody_for_track(ref_path, pred_path, args.device, **melody_options)}
        except Exception as e:                          # evaluate.py:127-131
            print(f"[Error] Failed on {base}: {e}")
            continue
        name = os.path.splitext(base)[0]
        line = f"{name[:20]}:\t" + ",\t".join(f"{k}={m[k]:.3f} dB" for k in metrics)
        if framewise:
            if m["frames"] == 0:
                print(f"[Error] No valid frame in {base} ({frames['SDR'].size} frames, all silent)")
                continue
            line += f",\tframes={m['frames']}/{frames['SDR'].size}"
            frame_rows += [{"track": name, "frame": i, "start_s": float(frames["start_s"][i]),
                            **{k: float(frames[k][i]) for k in metrics}} for i in range(frames["SDR"].size)]
        print(line + "".join(f",\t{k}={m[k]:.3f}" for k in melody))
        results.append({"track": name, **m})
    if not results:
        print("\n[Error] No valid tracks evaluated.")
        return
    print("\n=== Overall Mean Metrics (vocal) ===" if not framewise else
          "\n=== Overall Mean Metrics (vocal, per-track medians over frames) ===")
    for k in metrics:
        print(f"Mean {k:4s}: {float(np.mean([r[k] for r in results])):.3f} dB")
    for k in melody:
        print(f"Mean {k:4s}: {float(np.mean([r[k] for r in results])):.3f}")
    if args.out_csv is not None:
        with open(args.out_csv, "w", newline="", encoding="utf-8") as f:
            w = csv.DictWriter(f, fieldnames=["track", *metrics] + (["frames"] if framewise else []) + list(melody))
            w.writeheader()
            w.writerows(results)
        print(f"\n[Info] Results saved to {args.out_csv}")
    if args.frames_csv is not None:
        with open(args.frames_csv, "w", newline="", encoding="utf-8") as f:
            w = csv.DictWriter(f, fieldnames=["track", "frame", "start_s", *metrics])
            w.writeheader()
            w.writerows(frame_rows)
        print(f"[Info] Frame results saved to {args.frames_csv}")
    return results


if __name__ == "__main__":
    main()
