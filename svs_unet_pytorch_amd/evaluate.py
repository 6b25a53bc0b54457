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

`bss_eval_sources_gpu` and `metrics_from_waveforms(..., device="gpu")` (CLI `--device gpu`) compute the same metrics with
fp64 gfx950 kernels (csrc/bss.hip) from the Gram-matrix form below; the numpy functions stay the reference they are
tested against.

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


def load_mono_audio(path):
    """wav -> (float64 mono waveform, sample rate); the file's own rate is kept (evaluate.py:15-23)."""
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
    if data.ndim == 2:
        data = data.mean(axis=1)
    return data, sr


def _project(reference_sources, estimated_source, flen):
    """Least-squares projection of the estimate onto the references delayed by 0 .. flen-1 samples."""
    from scipy.linalg import toeplitz
    from scipy.signal import fftconvolve
    nsrc, nsampl = reference_sources.shape
    refs = np.hstack((reference_sources, np.zeros((nsrc, flen - 1))))
    est = np.hstack((estimated_source, np.zeros(flen - 1)))
    n_fft = int(2 ** np.ceil(np.log2(nsampl + flen - 1.0)))
    sf = np.fft.fft(refs, n=n_fft, axis=1)
    sef = np.fft.fft(est, n=n_fft)
    G = np.zeros((nsrc * flen, nsrc * flen))
    for i in range(nsrc):
        for j in range(i + 1):
            ssf = np.real(np.fft.ifft(sf[i] * np.conj(sf[j])))
            ss = toeplitz(np.hstack((ssf[0], ssf[-1:-flen:-1])), r=ssf[:flen])
            G[i * flen:(i + 1) * flen, j * flen:(j + 1) * flen] = ss
            G[j * flen:(j + 1) * flen, i * flen:(i + 1) * flen] = ss.T
    D = np.zeros(nsrc * flen)
    for i in range(nsrc):
        ssef = np.real(np.fft.ifft(sf[i] * np.conj(sef)))
        D[i * flen:(i + 1) * flen] = np.hstack((ssef[0], ssef[-1:-flen:-1]))
    try:
        C = np.linalg.solve(G, D).reshape(flen, nsrc, order="F")
    except np.linalg.LinAlgError:
        C = np.linalg.lstsq(G, D, rcond=None)[0].reshape(flen, nsrc, order="F")
    sproj = np.zeros(nsampl + flen - 1)
    for i in range(nsrc):
        sproj += fftconvolve(C[:, i], refs[i])[:nsampl + flen - 1]
    return sproj


def _decompose(reference_sources, estimated_source, j, flen):
    """estimate = s_true + e_spat + e_interf + e_artif with respect to reference source j."""
    nsampl = estimated_source.size
    s_true = np.hstack((reference_sources[j], np.zeros(flen - 1)))
    e_spat = _project(reference_sources[j, np.newaxis, :], estimated_source, flen) - s_true
    e_interf = _project(reference_sources, estimated_source, flen) - s_true - e_spat
    e_artif = -s_true - e_spat - e_interf
    e_artif[:nsampl] += estimated_source
    return s_true, e_spat, e_interf, e_artif


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
    perms = list(itertools.permutations(range(nsrc)))
    idx = np.arange(nsrc)
    mean_sir = [np.mean(sir[list(p), idx]) for p in perms]
    popt = list(perms[int(np.argmax(mean_sir))])
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
    perms = list(itertools.permutations(range(nsrc)))
    mean_sir = [np.mean(sir[list(p), idx]) for p in perms]
    popt = list(perms[int(np.argmax(mean_sir))])
    return sdr[popt, idx], sir[popt, idx], sar[popt, idx], np.asarray(popt)


def _gpu_projections(sig, solves, energies, flen):
    """Projection energies of the Gram form on the GPU, from ONE correlation pass over the rows of `sig` ((S, n) float64
    on a ROCm device).  solves: [(reference rows, estimate rows)], one Cholesky factorisation each; energies: rows whose
    |x|^2 is wanted.  Returns (energy, [|P e|^2 per estimate of each solve]) as numpy, or None when a factorisation met a
    pivot that was not > 0 (singular G: _project then solves by least squares)."""
    import ctypes
    import torch
    from . import _lib
    L = _lib.lib()
    pairs, off = [], {}

    def need(a, b, nl):                              # offset of pair (a, b, nl) in the correlation output
        if (a, b, nl) not in off:
            off[(a, b, nl)] = sum(p[2] for p in pairs)
            pairs.append((a, b, nl))
        return off[(a, b, nl)]

    plans = []
    for refs, ests in solves:
        gram = [need(i, j, flen) for i in refs for j in refs]
        rhs = [need(e, i, flen) for e in ests for i in refs]
        plans.append((len(refs), gram, rhs, len(ests)))
    eoff = [need(e, e, 1) for e in energies]
    flat = [v for p in pairs for v in p]
    parr = (ctypes.c_int * len(flat))(*flat)
    dev = sig.device
    n = sig.shape[1]
    ws_bytes = max([L.svs_bss_corr_workspace_bytes(n, len(pairs), parr)] +
                   [L.svs_bss_solve_workspace_bytes(k, flen, nr) for k, _, _, nr in plans])
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr()
        ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
        corr = torch.empty(sum(p[2] for p in pairs), dtype=torch.float64, device=dev)
        _lib.check(L.svs_bss_corr(sig.data_ptr(), sig.stride(0), sig.shape[0], n, parr, len(pairs), corr.data_ptr(),
                                  ws.data_ptr(), ws.numel(), stream), "svs_bss_corr")
        status = torch.empty(len(plans), dtype=torch.int32, device=dev)
        ynorm2 = torch.empty(len(plans), max(p[3] for p in plans), dtype=torch.float64, device=dev)
        for s, (k, gram, rhs, nr) in enumerate(plans):
            _lib.check(L.svs_bss_solve(corr.data_ptr(), k, flen, (ctypes.c_int * len(gram))(*gram),
                                       (ctypes.c_int * len(rhs))(*rhs), nr, ynorm2[s].data_ptr(), status[s:].data_ptr(),
                                       ws.data_ptr(), ws.numel(), stream), "svs_bss_solve")
        energy = corr[eoff].cpu().numpy()
        y = ynorm2.cpu().numpy()
        if status.cpu().numpy().any():
            warnings.warn("BSS-eval: a Gram matrix has a pivot that is not > 0 in the GPU Cholesky (singular or "
                          "numerically indefinite); this call falls back to the numpy path", RuntimeWarning, stacklevel=3)
            return None
    return energy, [y[s, :p[3]] for s, p in enumerate(plans)]


def _device_f64(x):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("the GPU BSS-eval needs a ROCm device (fp64 gfx950 kernels, no CPU path; use device='cpu')")
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=t.device if t.is_cuda else torch.device("cuda"), dtype=torch.float64)


def bss_eval_sources_gpu(reference_sources, estimated_sources, compute_permutation=True, flen=FILTER_LEN):
    """bss_eval_sources on the GPU (numpy or torch inputs, K = 1 or 2 sources, flen <= 512): the same (sdr, sir, sar,
    perm).  A singular Gram matrix (e.g. a silent reference) makes the call return the numpy bss_eval_sources result."""
    import torch
    ref, est = _device_f64(reference_sources), _device_f64(estimated_sources)
    ref, est = ref.reshape(1, -1) if ref.dim() == 1 else ref, est.reshape(1, -1) if est.dim() == 1 else est
    if ref.shape != est.shape:
        raise ValueError(f"reference {tuple(ref.shape)} and estimate {tuple(est.shape)} must have the same shape")
    nsrc = ref.shape[0]
    if nsrc not in (1, 2):
        raise ValueError(f"bss_eval_sources_gpu handles 1 or 2 sources, got {nsrc} (use bss_eval_sources)")
    if not 1 <= flen <= 512:
        raise ValueError(f"flen = {flen}: the GPU path supports filter lengths 1 .. 512")
    if est.device != ref.device:
        est = est.to(ref.device)
    refs, ests = list(range(nsrc)), [nsrc + a for a in range(nsrc)]
    solves = [((i,), ests) for i in refs] + ([(tuple(refs), ests)] if nsrc == 2 else [])
    q = _gpu_projections(torch.cat([ref, est]).contiguous(), solves, ests, flen)
    if q is None:
        return bss_eval_sources(ref.cpu().numpy(), est.cpu().numpy(), compute_permutation, flen)
    energy, y = q
    proj_one = np.stack(y[:nsrc], axis=1)
    return _metrics_from_gram(energy, proj_one, y[nsrc] if nsrc == 2 else proj_one[:, 0], compute_permutation)


def compute_metrics_for_track(mix_path, vocal_ref_path, vocal_est_path, device="cpu"):
    """evaluate.py:26-84: vocal SDR / SIR / SAR on (vocal, mixture - vocal) and NSDR against the mixture."""
    mix, sr_mix = load_mono_audio(mix_path)
    vocal_ref, sr_ref = load_mono_audio(vocal_ref_path)
    vocal_est, sr_est = load_mono_audio(vocal_est_path)
    if not (sr_mix == sr_ref == sr_est):
        raise ValueError(f"Sample rate mismatch: mix={sr_mix}, ref={sr_ref}, est={sr_est}")
    n = min(len(mix), len(vocal_ref), len(vocal_est))
    mix, vocal_ref, vocal_est = mix[:n], vocal_ref[:n], vocal_est[:n]
    return metrics_from_waveforms(mix, vocal_ref, vocal_est, device)


def metrics_from_waveforms(mix, vocal_ref, vocal_est, device="cpu"):
    """{"SDR", "SIR", "SAR", "NSDR"} of the vocal.  device="gpu": one correlation pass over (vocal, mix - vocal, estimate,
    mix - estimate, mix) on the GPU serves all four (the accompaniments are formed on the device, as numpy does)."""
    if device == "gpu":
        return _metrics_from_waveforms_gpu(mix, vocal_ref, vocal_est)
    if device != "cpu":
        raise ValueError(f"device must be 'cpu' or 'gpu', got {device!r}")
    sources_ref = np.stack([vocal_ref, mix - vocal_ref], axis=0)
    sources_est = np.stack([vocal_est, mix - vocal_est], axis=0)
    sdr, sir, sar, perm = bss_eval_sources(sources_ref, sources_est)
    v = int(perm[0])                                   # estimate matched to the vocal reference (evaluate.py:62)
    sdr_mix, _, _, _ = bss_eval_sources(vocal_ref[None, :], mix[None, :])
    return {"SDR": float(sdr[v]), "SIR": float(sir[v]), "SAR": float(sar[v]), "NSDR": float(sdr[v]) - float(sdr_mix[0])}


def _metrics_from_waveforms_gpu(mix, vocal_ref, vocal_est):
    import torch
    m, v, ve = _device_f64(mix), _device_f64(vocal_ref), _device_f64(vocal_est)
    v, ve = v.to(m.device), ve.to(m.device)
    sig = torch.stack([v, m - v, ve, m - ve, m])     # rows: vocal, accompaniment, their estimates, mixture
    q = _gpu_projections(sig, [((0,), [2, 3, 4]), ((1,), [2, 3]), ((0, 1), [2, 3])], [2, 3, 4], FILTER_LEN)
    if q is None:
        return metrics_from_waveforms(*(t.cpu().numpy() for t in (m, v, ve)))
    energy, (p_v, p_a, p_all) = q
    sdr, sir, sar, perm = _metrics_from_gram(energy[:2], np.stack([p_v[:2], p_a], axis=1), p_all)
    j = int(perm[0])
    sdr_mix = _metrics_from_gram(energy[2:], p_v[2:, None], p_v[2:])[0]
    return {"SDR": float(sdr[j]), "SIR": float(sir[j]), "SAR": float(sar[j]), "NSDR": float(sdr[j]) - float(sdr_mix[0])}


def main(argv=None):
    parser = argparse.ArgumentParser(description="Evaluate SVS results with SDR / SIR / SAR / NSDR (vocal only).")
    parser.add_argument("--est", type=str, required=True, help="folder of predicted vocal wav files")
    parser.add_argument("--mix", type=str, required=True, help="folder of mixture wav files")
    parser.add_argument("--ref", type=str, required=True, help="folder of reference vocal wav files")
    parser.add_argument("--ext", type=str, default="wav")
    parser.add_argument("--out_csv", type=str, default=None)
    parser.add_argument("--device", choices=["cpu", "gpu"], default="cpu",
                        help="gpu: BSS-eval with the fp64 gfx950 kernels (same metrics and CSV)")
    args = parser.parse_args(argv)
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
    results = []
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
            m = compute_metrics_for_track(mix_path, ref_path, pred_path, args.device)
        except Exception as e:                          # evaluate.py:127-131
            print(f"[Error] Failed on {base}: {e}")
            continue
        name = os.path.splitext(base)[0]
        print(f"{name[:20]}:\tSDR={m['SDR']:.3f} dB,\tSIR={m['SIR']:.3f} dB,\tSAR={m['SAR']:.3f} dB,\tNSDR={m['NSDR']:.3f} dB")
        results.append({"track": name, **m})
    if not results:
        print("\n[Error] No valid tracks evaluated.")
        return
    print("\n=== Overall Mean Metrics (vocal) ===")
    for k in ("SDR", "SIR", "SAR", "NSDR"):
        print(f"Mean {k:4s}: {float(np.mean([r[k] for r in results])):.3f} dB")
    if args.out_csv is not None:
        with open(args.out_csv, "w", newline="", encoding="utf-8") as f:
            w = csv.DictWriter(f, fieldnames=["track", "SDR", "SIR", "SAR", "NSDR"])
            w.writeheader()
            w.writerows(results)
        print(f"\n[Info] Results saved to {args.out_csv}")
    return results


if __name__ == "__main__":
    main()
