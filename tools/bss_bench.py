#!/usr/bin/env python3
"""Per-track cost of the vocal metrics (evaluate.metrics_from_waveforms: SDR / SIR / SAR / NSDR) on the GPU path (csrc/bss.hip)
and the numpy path, on a seeded synthetic 240 s track at 8192 Hz and at 44,100 Hz.

    python tools/bss_bench.py [--rates 8192 44100] [--seconds 240] [--reps 5] [--no-numpy]
    rocprofv3 --kernel-trace --stats -d DIR -o bss --output-format csv -- python tools/bss_bench.py --rates 8192 --no-numpy
    python tools/bss_bench.py --kernel-stats DIR --rates 8192 --seconds 240
    python tools/bss_bench.py --frame_window 1 [--frame_hop 1] [--ws-budget BYTES]   # framewise metrics instead
    python tools/bss_bench.py --stereo [--frame_window 1]       # the image metrics (SDR / ISR / SIR / SAR / NSDR) of a stereo track
    python tools/bss_bench.py --ab-solve                        # the two solve entry points on one batch, and order 2048
    python tools/bss_bench.py --v4                              # BSS-eval v4 (evaluate.py --mode v4) of the stereo track, 1 s frames

Timing: host clock around metrics_from_waveforms(device="gpu") followed by a device synchronise (the call ends with a
copy back to the host anyway), after one warm-up call; median and minimum of --reps calls.  The numpy path is timed once.
With --kernel-stats the tool instead reads a rocprofv3 --stats CSV of a run at ONE rate and reports the correlation
kernel's time and fp64 rate: lag products x n x 2 FLOP (9 pairs x 512 lags + 5 energies per sample).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import evaluate as ev  # noqa: E402

# the pairs metrics_from_waveforms(device="gpu") asks of svs_bss_corr_windows: the Gram and right-hand-side pairs of the
# three solves and the energy of each of the five rows (a whole track is one window and asks what every window asks)
LAG_PRODUCTS = 9 * ev.FILTER_LEN + 5


def track(seconds, rate, seed=0):
    """Seeded stand-in for a song: a gliding, amplitude-modulated tone plus filtered noise as the vocal, coloured noise as
    the accompaniment, the estimate = vocal + 8 % of the accompaniment + noise."""
    rng = np.random.default_rng(seed)
    n = seconds * rate
    t = np.arange(n) / rate
    vocal = np.sin(2 * np.pi * 220 * t * (1 + 0.01 * np.sin(2 * np.pi * 0.5 * t))) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.3 * t))
    vocal += 0.05 * np.convolve(rng.standard_normal(n), np.ones(8) / 8)[:n]
    acc = 0.3 * np.convolve(rng.standard_normal(n), [1.0, -0.5, 0.25])[:n]
    return vocal + acc, vocal, vocal + 0.08 * acc + 0.02 * rng.standard_normal(n)


def stereo_track(seconds, rate, seed=0):
    """track() made stereo, each (n, 2): the vocal near the centre, the accompaniment wide, the estimate with a wrong balance."""
    mix, vocal, est = track(seconds, rate, seed)
    _, vocal2, _ = track(seconds, rate, seed + 1)
    rng = np.random.default_rng(seed + 2)
    n = vocal.size
    v = np.stack([vocal, 0.8 * vocal + 0.2 * vocal2], axis=1)
    acc = np.stack([mix - vocal, 0.3 * np.convolve(rng.standard_normal(n), [1.0, -0.5, 0.25])[:n]], axis=1)
    return v + acc, v, v * [1.0, 0.9] + 0.08 * acc + 0.02 * rng.standard_normal((n, 2))


def stereo_record(args, rate):
    """--stereo: GPU and numpy image metrics on the stereo track (whole track, or frames with --frame_window); the largest
    |delta| over all figures."""
    import torch
    mix, vocal, est = stereo_track(args.seconds, rate)
    if args.frame_window is None:
        run = lambda device: ev.image_metrics_from_waveforms(mix, vocal, est, device)
        rec = {}
    else:
        window = ev.frame_samples(args.frame_window, rate)
        hop = ev.frame_samples(args.frame_window if args.frame_hop is None else args.frame_hop, rate)
        gpu_kw = {"ws_budget": args.ws_budget}
        run = lambda device: ev.image_metrics_from_waveforms_framewise(mix, vocal, est, window, hop, device,
                                                                       **(gpu_kw if device == "gpu" else {}))
        rec = {"window": window, "hop": hop, "ws_budget": args.ws_budget}
    run("gpu")
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        g = run("gpu")
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    rec = {"stereo": True, "rate": rate, "seconds": args.seconds, "n": mix.shape[0], **rec,
           "gpu_ms_median": 1e3 * statistics.median(ts), "gpu_ms_min": 1e3 * min(ts), "reps": args.reps}
    g = {k: np.atleast_1d(g[k]) for k in ev.IMAGE_METRICS}
    rec["frames"] = int(g["SDR"].size)
    rec["gpu_median"] = {k: float(np.nanmedian(g[k])) for k in ev.IMAGE_METRICS}
    if not args.no_numpy:
        t0 = time.perf_counter()
        c = run("cpu")
        rec["numpy_s"] = time.perf_counter() - t0
        c = {k: np.atleast_1d(c[k]) for k in ev.IMAGE_METRICS}
        rec["nan_frames_equal"] = all(np.array_equal(np.isnan(g[k]), np.isnan(c[k])) for k in ev.IMAGE_METRICS)
        rec["max_abs_diff_db"] = max(float(np.max(np.abs(g[k] - c[k])[~np.isnan(c[k])], initial=0.0)) for k in ev.IMAGE_METRICS)
        rec["speedup"] = rec["numpy_s"] / (rec["gpu_ms_median"] / 1e3)
    return rec


def v4_record(args, rate):
    """--v4: BSS-eval v4 of the stereo two-source track, 1 s frames.  In every repetition, one after the other: bss_eval_v4_gpu
    (host clock around the call, which ends in its read-back, then a device synchronise), the existing --stereo --frame_window 1
    device path on the same track (for scale: it re-estimates the filters in every frame) and svs_bss_project_frames alone on
    device-resident inputs (HIP events; seeded coefficients, which the time does not depend on), after one warm-up round;
    medians with min and max.  The float64 numpy definition is timed once on the host.  FMAs of the projection: per source,
    frame, estimate channel and output sample, flen taps of the source's nchan and of all R reference channels."""
    import torch
    from svs_unet_pytorch_amd import _lib
    mix, vocal, est = stereo_track(args.seconds, rate)
    ref2, est2 = np.stack([vocal, mix - vocal]), np.stack([est, mix - est])
    n, nchan, nsrc, flen = mix.shape[0], 2, 2, ev.FILTER_LEN
    window = hop = ev.frame_samples(1.0, rate)
    nwin = ev.frame_count(n, window, hop)
    L, dev, R = _lib.lib(), torch.device("cuda"), 4
    rng = np.random.default_rng(7)
    sig = torch.from_numpy(np.concatenate([ref2.transpose(0, 2, 1).reshape(R, n), est2.transpose(0, 2, 1).reshape(R, n)])).to(dev)
    coef_one = torch.from_numpy(rng.standard_normal(nsrc * nchan * nchan * flen) / flen).to(dev)
    coef_all = torch.from_numpy(rng.standard_normal(R * R * flen) / flen).to(dev)
    sums = torch.empty(nwin * nsrc * 7, dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.svs_bss_project_frames_workspace_bytes(window, nwin, nsrc, flen)), dtype=torch.uint8, device=dev)
    rows = np.arange(2 * R, dtype=np.int32)

    def project():
        _lib.check(L.svs_bss_project_frames(sig.data_ptr(), n, 2 * R, n, window, hop, nwin, flen, nsrc, nchan, rows[:R].ctypes.data,
                                            rows[R:].ctypes.data, coef_one.data_ptr(), coef_all.data_ptr(), sums.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "svs_bss_project_frames")

    def host_timed(fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def event_timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), None

    sides = {"v4_gpu": lambda: host_timed(lambda: ev.bss_eval_v4_gpu(ref2, est2, window, hop)),
             "v3_framewise_gpu": lambda: host_timed(lambda: ev.image_metrics_from_waveforms_framewise(mix, vocal, est, window, hop,
                                                                                                      "gpu")),
             "project_frames": lambda: event_timed(project)}
    ms, last = {k: [] for k in sides}, {}
    for rep in range(args.reps + 1):
        for k, fn in sides.items():
            t, last[k] = fn()
            if rep:                                                    # the first round warms up
                ms[k].append(t)
    fma = float(nsrc * nwin * (window + flen - 1) * nchan * flen * (nchan + R))
    rec = {"v4": True, "rate": rate, "seconds": args.seconds, "n": n, "window": window, "hop": hop, "frames": int(nwin),
           "flen": flen, "reps": args.reps,
           **{f"{k}_ms_{s}": f(v) for k, v in ms.items() for s, f in (("median", statistics.median), ("min", min), ("max", max))},
           "project_frames_fma": fma, "project_frames_fp64_tflops": 2.0 * fma / (statistics.median(ms["project_frames"]) * 1e-3) / 1e12}
    g = last["v4_gpu"]
    rec["gpu_median_vocal"] = {k: float(np.nanmedian(v[0])) for k, v in zip(("SDR", "ISR", "SIR", "SAR"), g)}
    if not args.no_numpy:
        t0 = time.perf_counter()
        c = ev.bss_eval_v4(ref2, est2, window, hop)
        rec["numpy_s"] = time.perf_counter() - t0
        rec["nan_frames_equal"] = all(np.array_equal(np.isnan(a), np.isnan(b)) for a, b in zip(g, c))
        rec["max_abs_diff_db"] = max(float(np.max(np.abs(a - b)[~np.isnan(b)], initial=0.0)) for a, b in zip(g, c))
        rec["speedup"] = rec["numpy_s"] / (rec["v4_gpu_ms_median"] / 1e3)
    return rec


def ab_solve(reps):
    """svs_bss_img_solve_batched (the diagonal tile factored once per step) against svs_bss_solve_batched ("old": every
    panel block factors it) on identical K = 2, flen 512 batches of 120 systems, the two alternating in one process, medians
    of device time.  The two factor a tile with the same operations in the same order, so this row is a standing check
    that they give identical bits on regular systems (max_rel_diff 0.0), and it records what factoring once gains on a
    large batch.  And the image entry point alone at K = 4, flen 512, 30 systems, which the mono one does not take."""
    import torch
    from svs_unet_pytorch_amd import _lib
    L, dev, flen, window = _lib.lib(), torch.device("cuda"), ev.FILTER_LEN, 8192
    out = []
    for K, nrhs, nbatch, sides in ((2, 2, 120, ("img", "old")), (4, 4, 30, ("img",))):
        rng = np.random.default_rng(K)
        sig = torch.from_numpy(rng.standard_normal((K + nrhs, nbatch * window))).to(dev)
        sig[K:] += sig[:K].sum(dim=0)
        pairs = [(i, j, flen) for i in range(K) for j in range(K)] + [(K + e, i, flen) for e in range(nrhs) for i in range(K)]
        flat = np.asarray(pairs, dtype=np.int32).ravel()
        stride = len(pairs) * flen
        corr = torch.empty(nbatch, stride, dtype=torch.float64, device=dev)
        ws = torch.empty(int(max(L.svs_bss_img_corr_windows_workspace_bytes(window, nbatch, len(pairs), flat.ctypes.data),
                                 L.svs_bss_img_solve_batched_workspace_bytes(nbatch, K, flen, nrhs))), dtype=torch.uint8,
                         device=dev)
        stream = _lib.stream_ptr()
        _lib.check(L.svs_bss_img_corr_windows(sig.data_ptr(), sig.stride(0), K + nrhs, sig.shape[1], window, window, nbatch,
                                              flat.ctypes.data, len(pairs), corr.data_ptr(), stride, ws.data_ptr(), ws.numel(),
                                              stream), "svs_bss_img_corr_windows")
        base = np.arange(nbatch, dtype=np.int64)[:, None] * stride
        g = np.ascontiguousarray(base + np.arange(K * K) * flen)
        r = np.ascontiguousarray(base + (K * K + np.arange(K * nrhs)) * flen)
        y = {s: torch.empty(nbatch, nrhs, dtype=torch.float64, device=dev) for s in sides}
        status, skipped = (torch.empty(nbatch, dtype=torch.int32, device=dev) for _ in range(2))

        def call(side):
            if side == "old":
                _lib.check(L.svs_bss_solve_batched(corr.data_ptr(), nbatch, K, flen, g.ctypes.data, r.ctypes.data, nrhs,
                                                   y[side].data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                           "svs_bss_solve_batched")
                return
            _lib.check(L.svs_bss_img_solve_batched(corr.data_ptr(), nbatch, K, flen, g.ctypes.data, r.ctypes.data, nrhs,
                                                   y[side].data_ptr(), status.data_ptr(), skipped.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), stream), "svs_bss_img_solve_batched")

        ms = {s: [] for s in sides}
        for rep in range(reps + 1):
            for s in sides:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call(s)
                t1.record()
                torch.cuda.synchronize()
                if rep:                                                # the first round warms up
                    ms[s].append(t0.elapsed_time(t1))
        rec = {"ab_solve": " vs ".join(sides), "K": K, "flen": flen, "nrhs": nrhs, "nbatch": nbatch, "reps": reps,
               **{f"{s}_ms_median": statistics.median(ms[s]) for s in sides}}
        if len(sides) == 2:
            a, b = (y[s].cpu().numpy() for s in sides)
            rec["ratio"] = statistics.median(ms[sides[1]]) / statistics.median(ms[sides[0]])
            rec["max_rel_diff"] = float(np.max(np.abs(a - b) / np.abs(b)))
        out.append(rec)
    return out


def time_gpu(mix, vocal, est, reps):
    import torch
    ev.metrics_from_waveforms(mix, vocal, est, device="gpu")          # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ts, m = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        m = ev.metrics_from_waveforms(mix, vocal, est, device="gpu")
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts, m


def time_gpu_frames(mix, vocal, est, window, hop, reps, ws_budget):
    import torch
    ev.metrics_from_waveforms_framewise(mix, vocal, est, window, hop, device="gpu", ws_budget=ws_budget)
    torch.cuda.synchronize()
    ts, fr = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        fr = ev.metrics_from_waveforms_framewise(mix, vocal, est, window, hop, device="gpu", ws_budget=ws_budget)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts, fr


def frames_record(args, rate, mix, vocal, est):
    """--frame_window: GPU and numpy metrics_from_waveforms_framewise on the same track; max |delta| over the frames both
    score, and whether their NaN frames agree."""
    window = ev.frame_samples(args.frame_window, rate)
    hop = ev.frame_samples(args.frame_window if args.frame_hop is None else args.frame_hop, rate)
    ts, g = time_gpu_frames(mix, vocal, est, window, hop, args.reps, args.ws_budget)
    rec = {"rate": rate, "seconds": args.seconds, "n": mix.size, "window": window, "hop": hop, "frames": int(g["SDR"].size),
           "gpu_ms_median": 1e3 * statistics.median(ts), "gpu_ms_min": 1e3 * min(ts), "reps": args.reps,
           "ws_budget": args.ws_budget, "gpu_median_sdr": ev.frame_summary(g)["SDR"]}
    if not args.no_numpy:
        t0 = time.perf_counter()
        c = ev.metrics_from_waveforms_framewise(mix, vocal, est, window, hop)
        rec["numpy_s"] = time.perf_counter() - t0
        rec["nan_frames_equal"] = all(np.array_equal(np.isnan(g[k]), np.isnan(c[k])) for k in ev.METRICS)
        ok = {k: ~np.isnan(c[k]) for k in ev.METRICS}
        rec["max_abs_diff_db"] = max(float(np.max(np.abs(g[k][ok[k]] - c[k][ok[k]]), initial=0.0)) for k in ev.METRICS)
        rec["speedup"] = rec["numpy_s"] / (rec["gpu_ms_median"] / 1e3)
    return rec


def kernel_stats(path, n):
    files = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {path}")
    rows = list(csv.DictReader(open(files[0])))
    out = {}
    for r in rows:
        name = r["Name"]
        short = next((k for k in ("bss_corr_reduce_kernel", "bss_corr_kernel", "bss_expand_kernel", "bss_diag_kernel",
                                  "bss_panel_kernel", "bss_update_kernel", "bss_norm_kernel", "bss_img_corr_kernel",
                                  "bss_img_reduce_kernel", "bss_img_panel_kernel") if k in name), None)
        if short:
            out[short] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
                          "total_us": float(r["TotalDurationNs"]) / 1e3}
    corr = out.get("bss_corr_kernel")
    if corr:
        flop = LAG_PRODUCTS * n * 2.0
        corr["fp64_tflops"] = flop / (corr["avg_us"] * 1e-6) / 1e12
        corr["flop_per_call"] = flop
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rates", type=int, nargs="+", default=[8192, 44100])
    ap.add_argument("--seconds", type=int, default=240)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true", help="GPU path only (profiling runs)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --stats CSV (or its directory) of a run at one rate")
    ap.add_argument("--frame_window", type=float, default=None, help="seconds: time the framewise metrics instead")
    ap.add_argument("--frame_hop", type=float, default=None, help="seconds (default: the window)")
    ap.add_argument("--ws-budget", type=int, default=ev.WS_BUDGET, help="workspace bytes of one batch of factorisations")
    ap.add_argument("--stereo", action="store_true", help="the image metrics of a stereo track (evaluate.py --stereo)")
    ap.add_argument("--ab-solve", action="store_true", help="the two solve entry points on identical batches (see ab_solve)")
    ap.add_argument("--v4", action="store_true", help="BSS-eval v4 of the stereo track in 1 s frames (see v4_record)")
    args = ap.parse_args()
    if args.kernel_stats:
        n = args.seconds * args.rates[0]
        print(json.dumps({"rate": args.rates[0], "n": n, "kernels": kernel_stats(args.kernel_stats, n)}))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bss_bench.py needs a ROCm device")
    if args.ab_solve:
        for rec in ab_solve(args.reps):
            print(json.dumps(rec), flush=True)
        return
    for rate in args.rates:
        if args.v4:
            print(json.dumps(v4_record(args, rate)), flush=True)
            continue
        if args.stereo:
            print(json.dumps(stereo_record(args, rate)), flush=True)
            continue
        mix, vocal, est = track(args.seconds, rate)
        if args.frame_window is not None:
            print(json.dumps(frames_record(args, rate, mix, vocal, est)), flush=True)
            continue
        ts, m_gpu = time_gpu(mix, vocal, est, args.reps)
        rec = {"rate": rate, "seconds": args.seconds, "n": mix.size, "gpu_ms_median": 1e3 * statistics.median(ts),
               "gpu_ms_min": 1e3 * min(ts), "reps": args.reps, "corr_gflop": LAG_PRODUCTS * mix.size * 2 / 1e9,
               "gpu_metrics": m_gpu}
        if not args.no_numpy:
            t0 = time.perf_counter()
            m_cpu = ev.metrics_from_waveforms(mix, vocal, est)
            rec["numpy_s"] = time.perf_counter() - t0
            rec["numpy_metrics"] = m_cpu
            rec["max_abs_diff_db"] = max(abs(m_gpu[k] - m_cpu[k]) for k in m_cpu)
            rec["speedup"] = rec["numpy_s"] / (rec["gpu_ms_median"] / 1e3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
