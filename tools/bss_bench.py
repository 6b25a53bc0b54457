#!/usr/bin/env python3
"""Per-track cost of the vocal metrics (evaluate.metrics_from_waveforms: SDR / SIR / SAR / NSDR) on the GPU path (csrc/bss.hip)
and the numpy path, on a seeded synthetic 240 s track at 8192 Hz and at 44,100 Hz.

    python tools/bss_bench.py [--rates 8192 44100] [--seconds 240] [--reps 5] [--no-numpy]
    rocprofv3 --kernel-trace --stats -d DIR -o bss --output-format csv -- python tools/bss_bench.py --rates 8192 --no-numpy
    python tools/bss_bench.py --kernel-stats DIR --rates 8192 --seconds 240
    python tools/bss_bench.py --frame_window 1 [--frame_hop 1] [--ws-budget BYTES]   # framewise metrics instead

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
        short = next((k for k in ("bss_corr_reduce_kernel", "bss_corr_kernel", "bss_expand_kernel", "bss_panel_kernel",
                                  "bss_update_kernel", "bss_norm_kernel") if k in name), None)
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
    args = ap.parse_args()
    if args.kernel_stats:
        n = args.seconds * args.rates[0]
        print(json.dumps({"rate": args.rates[0], "n": n, "kernels": kernel_stats(args.kernel_stats, n)}))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bss_bench.py needs a ROCm device")
    for rate in args.rates:
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
