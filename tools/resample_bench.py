#!/usr/bin/env python3
"""Cost of getting a wav file's PCM to the network rate: the GPU resampler (csrc/resample.hip) against the host path it
replaces (scipy.signal.resample_poly, as data.load_wav_mono runs it), on a seeded 240 s stereo int16 track at 44,100 Hz and
at 48,000 Hz.

    python tools/resample_bench.py [--rates 44100 48000] [--seconds 240] [--reps 5] [--no-separate]
    rocprofv3 --kernel-trace --stats -d DIR -o rs --output-format csv -- python tools/resample_bench.py --rates 44100 --gpu-only
    python tools/resample_bench.py --kernel-stats DIR --rates 44100 --seconds 240
    python tools/resample_bench.py --egress [--rates 44100 48000] [--seconds 240] [--reps 5]

Per rate, medians of --reps synchronised calls after one warm-up call, all in one run on one box:
  (a) gpu_ms          resample_poly_gpu(int16 stereo PCM already on the device, downmix) -> mono float32 at 8,192 Hz
      gpu_h2d_ms      the same, starting from the host array (one copy of the raw PCM, then the kernel)
  (b) host_s          load_wav_mono's arithmetic on the host (int16 -> float32, mean of the channels, resample_poly in float32)
      host_h2d_s      (b) plus the copy of its result to the device
  (c) separate_*      streaming.separate_waveform(model, stereo float32 at the file rate, sr_in=rate) against resample_poly of
                      both channels on the host + copy + today's separate_waveform (44,100 Hz only, skipped by --no-separate)
and max |d| of (a) and (b) against float64 scipy on the same samples.
With --egress the tool times the way OUT instead: --seconds of separated stereo float32 at 8,192 Hz on the device -> peak-normalised
interleaved int16 at the file rate on the host, medians of --reps after one warm-up:
  (a) resample.resample_encode_gpu (FIR twice: svs_resample_peaks, then svs_resample_encode) -- peaks_ms / encode_ms / device_ms
      from device events, to_host_ms the wall time until the int16 bytes are in host memory; encode_store_gbps = the bytes the
      encode launch stores over encode_ms; materialised_device_ms is the other peak strategy (svs_resample_poly to float32 once,
      then peaks and encode of that buffer at 1/1);
  (b) what the parent of that feature offers: resample_poly_gpu to float32, abs().amax(), scale, .cpu(), then numpy rint /
      clip / astype / interleave -- parent_to_host_ms;
and asserts that (a), the materialised form and (b) give the same int16 samples.
With --kernel-stats the tool instead reads a rocprofv3 --stats CSV of a --gpu-only run at ONE rate and reports the kernel's
time and its achieved bytes/s against (i) the input + output bytes (HBM) and (ii) the tap bytes the launch reads from the
packed table (L2), as svs_resample_plan counts them.
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import statistics
import sys
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import _lib  # noqa: E402
from svs_unet_pytorch_amd import resample as rs  # noqa: E402
from svs_unet_pytorch_amd.config import SAMPLE_RATE  # noqa: E402


def track(seconds, rate, seed=0):
    """Seeded stand-in for a stereo int16 file: a gliding tone plus noise, the right channel a scaled, noisier copy."""
    rng = np.random.default_rng(seed)
    n = seconds * rate
    t = np.arange(n) / rate
    left = 0.4 * np.sin(2 * np.pi * 220 * t * (1 + 0.01 * np.sin(2 * np.pi * 0.5 * t))) + 0.1 * rng.standard_normal(n)
    right = 0.8 * left + 0.05 * rng.standard_normal(n)
    return np.clip(np.round(np.stack([left, right], axis=1) * 20000), -32768, 32767).astype(np.int16)


def median_of(fn, reps):
    import torch
    fn()                                                    # warm-up: code objects, allocator, tap table
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), out


def host_mono(pcm, up, down):
    from scipy.signal import resample_poly
    data = pcm.astype(np.float32) / 32768.0
    return resample_poly(data.mean(axis=1), up, down).astype(np.float32)


def plan_of(n_in, up, down, rows):
    plan = (ctypes.c_int64 * 8)()
    _lib.check(_lib.lib().svs_resample_plan(n_in, up, down, 20 * max(up, down) + 1, rows, plan), "svs_resample_plan")
    keys = ("outputs_per_segment", "segments_per_step", "blocks_q", "blocks_signal", "steps_per_block", "span", "lds_bytes", "tap_bytes")
    return dict(zip(keys, (int(v) for v in plan)))


def record(args, rate):
    import torch
    from scipy.signal import resample_poly
    fr = Fraction(SAMPLE_RATE, rate)
    up, down = fr.numerator, fr.denominator
    pcm = track(args.seconds, rate)
    dev = torch.device("cuda")
    pcm_dev = torch.from_numpy(pcm).to(dev)
    rec = {"rate": rate, "seconds": args.seconds, "n_in": pcm.shape[0], "up": up, "down": down, "reps": args.reps,
           "plan": plan_of(pcm.shape[0], up, down, 1)}
    med, mn, y = median_of(lambda: rs.resample_poly_gpu(pcm_dev, up, down, channels=2, downmix=True), args.reps)
    rec.update(gpu_ms=1e3 * med, gpu_ms_min=1e3 * mn, n_out=int(y.numel()))
    if args.gpu_only:
        return rec
    med, mn, _ = median_of(lambda: rs.resample_poly_gpu(torch.from_numpy(pcm).to(dev), up, down, channels=2, downmix=True), args.reps)
    rec.update(gpu_h2d_ms=1e3 * med, gpu_h2d_ms_min=1e3 * mn)
    med, mn, h = median_of(lambda: host_mono(pcm, up, down), args.reps)
    rec.update(host_s=med, host_s_min=mn)
    med, mn, _ = median_of(lambda: torch.from_numpy(host_mono(pcm, up, down)).to(dev), args.reps)
    rec.update(host_h2d_s=med, host_h2d_s_min=mn)
    ref = resample_poly((pcm.astype(np.float32) / 32768.0).mean(axis=1).astype(np.float64), up, down)
    rec["gpu_max_abs_diff_vs_f64"] = float(np.abs(y.cpu().numpy() - ref).max())
    rec["host_max_abs_diff_vs_f64"] = float(np.abs(h - ref).max())
    rec["speedup_device_resident"] = rec["host_s"] / (rec["gpu_ms"] / 1e3)
    rec["speedup_from_host_memory"] = rec["host_h2d_s"] / (rec["gpu_h2d_ms"] / 1e3)
    if rate == 44100 and not args.no_separate:
        from svs_unet_pytorch_amd.streaming import separate_waveform
        from tools._benchlib import closed_form_model
        model = closed_form_model(dev)
        planar = np.ascontiguousarray((pcm.astype(np.float32) / 32768.0).T)               # (2, n) float32 at the file rate
        planar_dev = torch.from_numpy(planar).to(dev)

        def host_then_separate():
            y8 = np.stack([resample_poly(c, up, down).astype(np.float32) for c in planar])
            return separate_waveform(model, torch.from_numpy(y8).to(dev))
        y8_dev = rs.resample_poly_gpu(planar_dev, up, down)
        med_g, _, a = median_of(lambda: separate_waveform(model, planar_dev, sr_in=rate), args.reps)
        med_sep, _, _ = median_of(lambda: separate_waveform(model, y8_dev), args.reps)
        med_h, _, b = median_of(host_then_separate, args.reps)
        rec.update(separate_sr_in_ms=1e3 * med_g, separate_at_8192_ms=1e3 * med_sep, separate_host_resample_s=med_h,
                   separate_max_abs_diff=float((a - b).abs().max()))
    return rec


def event_median(fn, reps):
    """median device ms between events around fn(), after one warm-up call; fn's last result"""
    import torch
    out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), out


def egress_record(args, rate):
    import torch
    fr = Fraction(rate, SAMPLE_RATE)
    up, down = fr.numerator, fr.denominator
    dev = torch.device("cuda")
    y = torch.from_numpy(np.ascontiguousarray((track(args.seconds, SAMPLE_RATE).astype(np.float32) / 32768.0).T)).to(dev)   # (2, n) planar
    channels, n_in = y.shape
    n_out = rs.out_len(n_in, up, down)
    L = _lib.lib()
    table, ntaps = rs.tap_table(up, down, dev)
    one, one_taps = rs.tap_table(1, 1, dev)
    rec = {"mode": "egress", "rate": rate, "seconds": args.seconds, "channels": channels, "n_in": n_in, "n_out": n_out, "up": up, "down": down,
           "reps": args.reps, "fmt": "int16", "peak_strategy": "fir_twice"}

    def gain_of(peaks):
        top = torch.empty(1, dtype=torch.float32, device=dev)
        gain = torch.full((channels,), 0.9, dtype=torch.float32, device=dev)
        _lib.check(L.svs_max(peaks.data_ptr(), channels, top.data_ptr(), _lib.stream_ptr()), "svs_max")
        _lib.check(L.svs_scale_by_inv(gain.data_ptr(), channels, top.data_ptr(), 1.0, _lib.stream_ptr()), "svs_scale_by_inv")
        return gain

    def encode(x, u, d, tab, nt, gain):
        out = torch.empty((rs.out_len(x.shape[1], u, d), channels), dtype=torch.int16, device=dev)
        _lib.check(L.svs_resample_encode(x.data_ptr(), channels, x.shape[1], x.shape[1], tab.data_ptr(), nt, u, d, gain.data_ptr(), rs.PCM_I16,
                                         out.data_ptr(), _lib.stream_ptr()), "svs_resample_encode")
        return out

    def materialised():
        f = rs.resample_poly_gpu(y, up, down)                                   # (2, n_out) float32, written once
        return encode(f, 1, 1, one, one_taps, gain_of(rs.resample_peaks_gpu(f, 1, 1)))

    rec["peaks_ms"], peaks = event_median(lambda: rs.resample_peaks_gpu(y, up, down), args.reps)
    gain = gain_of(peaks)
    rec["encode_ms"], _ = event_median(lambda: encode(y, up, down, table, ntaps, gain), args.reps)
    rec["encode_store_gbps"] = n_out * channels * 2 / (rec["encode_ms"] * 1e-3) / 1e9
    rec["device_ms"], a_dev = event_median(lambda: rs.resample_encode_gpu(y, up, down, fmt="int16", peak=0.9), args.reps)
    rec["materialised_device_ms"], m_dev = event_median(materialised, args.reps)
    med, mn, a = median_of(lambda: rs.resample_encode_gpu(y, up, down, fmt="int16", peak=0.9).cpu().numpy(), args.reps)
    rec.update(to_host_ms=1e3 * med, to_host_ms_min=1e3 * mn)

    def parent():
        f = rs.resample_poly_gpu(y, up, down)
        g = np.float32(0.9) / np.float32(f.abs().amax().item())                 # one gain for both channels; 0 does not occur here
        v = (f * float(g)).cpu().numpy()
        s = np.clip(np.rint(v * np.float32(32767.0)), -32768.0, 32767.0).astype(np.int16)
        return np.ascontiguousarray(s.T)
    med, mn, b = median_of(parent, args.reps)
    rec.update(parent_to_host_ms=1e3 * med, parent_to_host_ms_min=1e3 * mn)
    assert a.shape == b.shape == (n_out, channels) and a.dtype == b.dtype == np.int16
    assert np.array_equal(a, b), "the fused path and the parent path disagree"
    assert np.array_equal(a, a_dev.cpu().numpy()) and np.array_equal(a, m_dev.cpu().numpy()), "the two peak strategies disagree"
    rec["max_abs_sample"] = int(np.abs(a.astype(np.int32)).max())
    rec["speedup_to_host"] = rec["parent_to_host_ms"] / rec["to_host_ms"]
    return rec


def kernel_stats(path, args):
    files = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {path}")
    rate = args.rates[0]
    fr = Fraction(SAMPLE_RATE, rate)
    n_in = args.seconds * rate
    plan = plan_of(n_in, fr.numerator, fr.denominator, 1)
    out = {"plan": plan}
    for r in csv.DictReader(open(files[0])):
        short = next((k for k in ("resample_poly_kernel", "resample_pack_kernel") if k in r["Name"]), None)
        if short:
            out[short] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                          "total_us": float(r["TotalDurationNs"]) / 1e3}
    k = out.get("resample_poly_kernel")
    if k:
        hbm = n_in * 2 * 2 + rs.out_len(n_in, fr.numerator, fr.denominator) * 4         # int16 stereo in, float32 mono out
        k["hbm_bytes"] = hbm
        k["hbm_gbps"] = hbm / (k["avg_us"] * 1e-6) / 1e9
        k["tap_bytes"] = plan["tap_bytes"]
        k["tap_gbps"] = plan["tap_bytes"] / (k["avg_us"] * 1e-6) / 1e9
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rates", type=int, nargs="+", default=[44100, 48000])
    ap.add_argument("--seconds", type=int, default=240)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpu-only", action="store_true", help="only the device-resident GPU call (profiling runs)")
    ap.add_argument("--no-separate", action="store_true", help="skip the separate_waveform comparison")
    ap.add_argument("--egress", action="store_true", help="time the way out (8,192 Hz float32 -> int16 at the file rate on the host) instead")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --stats CSV (or its directory) of a --gpu-only run at one rate")
    args = ap.parse_args()
    if args.kernel_stats:
        print(json.dumps({"rate": args.rates[0], "seconds": args.seconds, "kernels": kernel_stats(args.kernel_stats, args)}))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench.py needs a ROCm device")
    for rate in args.rates:
        print(json.dumps(egress_record(args, rate) if args.egress else record(args, rate)), flush=True)


if __name__ == "__main__":
    main()
