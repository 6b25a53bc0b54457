"""wav -> separated wav in one command: the file's PCM goes to the device as it is stored, every channel is resampled to
the network rate, separated (STFT -> U-Net mask -> inverse STFT), resampled back to the file's rate, peak-normalised to 0.9
and converted to the written sample format there (streaming.separate_to_wav; csrc/resample.hip); only the encoded samples
return to the host.  The output has the source's rate, channel count and (unless --no_keep_length) frame count, so
evaluate.py accepts it beside the source's stems.

    python -m svs_unet_pytorch_amd.separate --model_path CKPT/svs_x.pth --src song.wav --tar out.wav
    python -m svs_unet_pytorch_amd.separate --model_path CKPT/svs_x.pth --src wav_folder --tar out_folder \
        [--vocal_solo 0|1] [--precision bf16] [--subtype PCM_16|PCM_24|PCM_32|FLOAT|source] [--dither none|tpdf|hp] [--dither_seed N] \
        [--no_keep_length] \
        [--win_size 512|1024|2048] [--hop_size N] [--tar_accomp accomp.wav | accomp_folder] [--tile_hop 128|64|32] [--phase_iters N]
        [--wiener_iters N] [--loudness LUFS|source] [--peak_ceiling 0.9] [--true_peak] [--fullband mask|accomp]
        [--limiter [MS]] [--f0_csv track.csv | csv_folder [--f0_smooth]]

A folder as --src means every *.wav in it, written under the same name into the folder --tar.  --subtype PCM_16 (the
default) is what the reference's data.py writes (data.py:166); PCM_24 writes 24-bit files, `source` the word length of each source
file, and --dither tpdf | hp adds TPDF dither under the 16- or 24-bit quantiser (pcm.py; csrc/pcm.hip; off by default: plain
rounding, byte for byte what was written before).  --win_size / --hop_size (the config's 1024 / 768 by default;
data.py:24-25 takes the same two flags) are the window and hop of the two transforms, for a checkpoint trained at another
geometry.  --tar_accomp also writes the accompaniment (a file, or a folder with the names of --tar when --src is a folder) from
the same pass: one STFT, one set of network forwards and one two-stem inverse STFT (svs_istft_stems_n), --tar then holding the
vocal; it excludes --vocal_solo 0.  --tile_hop (128 by default: disjoint 128-frame tiles, inference.py:72-120) below 128 runs the
network on overlapped tiles that start every 64 or 32 frames and cross-fades their masks (overlap.py), at 2x / 4x the network
forwards: no frame's mask then comes from a tile's zero-padded edge alone.  --phase_iters N (0 by default: the masked magnitude
carries the mixture's phase, as the reference writes it) refines the phase before the last inverse transform (rephase.py): N
Griffin-Lim updates of the written stem, or, with --tar_accomp, N MISI updates of both stems, which also share out what the two fail
to add up to.  --wiener_iters N (0 by default; 1..8; files of one or two channels; not beside --phase_iters) runs the multichannel
Wiener filter after the mask (wiener.py): N updates of a power per bin and a spatial covariance per frequency for each of the two
sources, then each written stem re-filtered from the complex stereo mixture -- magnitudes and phases of its own, the mixture's
stereo balance kept, and with --tar_accomp two files that add up to the mixture.  --loudness LUFS (off by default: every file is
peak-normalised to 0.9 on its own, data.py:162-166) brings the written audio to that integrated loudness instead (ITU-R BS.1770-4,
loudness.py; measured on the device on the samples that are written): one file to the target, or, with --tar_accomp, vocal +
accompaniment to the target with one gain for both files, so that their balance is kept; --loudness source (with --tar_accomp only)
aims at the source file's own loudness.  --peak_ceiling (0.9) bounds every written sample under that gain.  --true_peak (off
by default) holds that ceiling, or without --loudness the 0.9 of the peak rule, against the TRUE peak of every written file -- the peak
of the 4x over-sampled signal (ITU-R BS.1770-4 Annex 2; loudness.py, csrc/r128.hip) -- instead of its largest sample: up-sampling
to the file's rate produces inter-sample peaks that a sample-peak bound lets through.  --limiter [MS] (off by default; 2.0 ms when
given without a value; only with --loudness) runs a look-ahead limiter before that gain (limiter.py; csrc/limiter.hip): one gain curve
for every channel of both files dips around the peaks that would otherwise hold the whole file under the target, +-2 MS wide, and
the ceiling then holds as before; the line printed per file names the deepest reduction and the loudness written.  --fullband (off by
default: the network runs at 8,192 Hz, so every written stem is empty above 4,096 Hz) shares the file's band above 4,096 Hz out
between the stems (fullband.py): `mask` by the network's own mask in its highest band, frame by frame; `accomp` all of it to the
accompaniment (the vocal stays band-limited).  With --tar_accomp the two files, each divided by its gain, then add up to the source, and
a stereo file keeps its channel balance.  Not beside --wiener_iters; a file at or below 8,192 Hz has no such band.  --f0_csv PATH
(a folder when --src is one: one NAME.csv per source file) also writes the pitch track of the vocal stem (f0.py; csrc/f0.hip): a YIN
tracker on the mean of the stem's channels at the network's 8,192 Hz, after the Wiener or phase stages and before the way out, one
launch; time,f0,voiced,aperiodicity,rms per 10 ms frame.  The wav files are byte for byte those written without the flag; --vocal_solo 0
writes no vocal stem, so it cannot be combined with it.  --f0_smooth (only with --f0_csv) writes the decoded track instead: 7 period
candidates per frame and an exact Viterbi decode over them and an unvoiced state (csrc/f0_smooth.hip), which removes most octave errors
and voicing drop-outs of the raw tracker on a noisy stem; the csv columns are the same.  The reference has no such command: it goes through
data.py to_spec, inference.py and data.py to_wave with .npy files in between.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from .config import HOP_SIZE, INPUT_LEN, WINDOW_SIZE
from .data import WINDOW_SIZES
from .fullband import MODES, check_fullband
from .inference import load_checkpoint_model
from .limiter import DEFAULT_MS, half_width
from .limiter import describe as describe_limiter
from .loudness import describe, parse_target
from .overlap import check_tile_hop
from .pcm import wav_info
from .streaming import check_refinement, separate_to_wav


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--model_path", type=str, required=True)
    parser.add_argument("--src", type=str, required=True, help="a wav file, or a folder of *.wav files")
    parser.add_argument("--tar", type=str, required=True, help="the wav file to write, or the target folder when --src is a folder")
    parser.add_argument("--vocal_solo", type=int, default=1, help="1: keep the vocal, 0: remove it")
    parser.add_argument("--precision", default=None, choices=["fp32", "bf16"], help="eval precision of the network (default: the model's)")
    parser.add_argument("--subtype", default="PCM_16", choices=["PCM_16", "PCM_32", "FLOAT", "PCM_24", "source"],
                        help="sample format of the written files; source = the format of each source file (8-bit sources are written as PCM_16)")
    parser.add_argument("--dither", default="none", choices=["none", "tpdf", "hp"],
                        help="TPDF dither of 2 LSB peak to peak under the 16- or 24-bit quantiser: tpdf = white, hp = high-passed "
                             "(first difference of one uniform sequence); default none = plain rounding")
    parser.add_argument("--dither_seed", type=int, default=0,
                        help="seed of the dither's counter generator (vocal: N, accompaniment: N + 1); the default 0 makes files reproducible")
    parser.add_argument("--no_keep_length", action="store_true", help="do not cut / pad the output to the source's frame count")
    parser.add_argument("--win_size", type=int, default=WINDOW_SIZE, help="window of the STFT / inverse STFT (512, 1024 or 2048)")
    parser.add_argument("--hop_size", type=int, default=HOP_SIZE, help="hop of the two transforms, 1..win_size")
    parser.add_argument("--tar_accomp", type=str, default=None,
                        help="also write the accompaniment here, from the same pass (a wav file, or a folder when --src is one); --tar holds the vocal")
    parser.add_argument("--tile_hop", type=int, default=INPUT_LEN,
                        help=f"frames between tiles: {INPUT_LEN} = disjoint tiles as the reference cuts them; 64 or 32 = overlapped tiles with cross-faded masks")
    parser.add_argument("--phase_iters", type=int, default=0,
                        help="phase-refinement updates before the last inverse STFT: 0 = the mixture's phase; N > 0 = N Griffin-Lim updates (MISI with --tar_accomp)")
    parser.add_argument("--wiener_iters", type=int, default=0,
                        help="updates of the multichannel Wiener filter after the mask: 0 = none; 1..8 (one or two channels; not with --phase_iters)")
    parser.add_argument("--loudness", type=str, default=None,
                        help="integrated loudness of what is written, in LUFS (for instance -23), instead of peak 0.9 per file; with --tar_accomp "
                             "one gain for both files; `source` (with --tar_accomp only): the source file's own loudness")
    parser.add_argument("--peak_ceiling", type=float, default=0.9, help="with --loudness: no written sample exceeds this (default 0.9)")
    parser.add_argument("--true_peak", action="store_true",
                        help="bound the true peak (the over-sampled signal's) of every written file instead of its largest sample: "
                             "--peak_ceiling under --loudness, 0.9 otherwise")
    parser.add_argument("--limiter", type=float, nargs="?", const=DEFAULT_MS, default=None, metavar="MS",
                        help=f"with --loudness: look-ahead limiter of this half-width in milliseconds ({DEFAULT_MS} when given without a value), one "
                             "gain curve for all written channels, so that a few peaks do not hold the whole file under the target (default: off)")
    parser.add_argument("--fullband", default=None, choices=list(MODES),
                        help="share the file's band above the network's 4,096 Hz out between the stems: mask = by the network's mask in its "
                             "highest band; accomp = all of it to the accompaniment (default: band-limited stems; not with --wiener_iters)")
    parser.add_argument("--f0_csv", type=str, default=None, metavar="PATH",
                        help="also write the vocal stem's pitch track (YIN at the network rate): time,f0,voiced,aperiodicity,rms per frame; "
                             "a csv file, or a folder when --src is one")
    parser.add_argument("--f0_smooth", action="store_true",
                        help="with --f0_csv: write the Viterbi-decoded pitch track (7 candidates per frame, default costs) instead of the raw one")
    parser.add_argument("--ema", action="store_true", help="load the checkpoint's ema_state_dict (train.py --ema_decay) instead of its live weights")
    args = parser.parse_args(argv)
    if args.dither != "none" and args.subtype in ("PCM_32", "FLOAT"):
        parser.error(f"--dither {args.dither} belongs to --subtype PCM_16 or PCM_24: {args.subtype} samples have nothing below the 24th bit "
                     "to linearise")
    if args.phase_iters < 0:
        parser.error(f"--phase_iters {args.phase_iters}: must be 0 (the mixture's phase) or a positive number of updates")
    try:
        check_refinement(args.phase_iters, args.wiener_iters)
    except ValueError as e:
        parser.error(f"--{e}")
    try:
        check_fullband(args.fullband, args.wiener_iters)
    except ValueError as e:
        parser.error(f"--{e}")
    try:
        check_tile_hop(args.tile_hop, INPUT_LEN)
    except ValueError as e:
        parser.error(f"--tile_hop: {e}")
    if args.win_size not in WINDOW_SIZES:
        parser.error(f"--win_size {args.win_size}: the STFT / iSTFT kernels are built for n_fft = {', '.join(map(str, WINDOW_SIZES))}")
    if not 0 < args.hop_size <= args.win_size:
        parser.error(f"--hop_size {args.hop_size}: must be in 1..{args.win_size} (a larger hop leaves samples that no frame covers)")
    if args.loudness is not None:
        try:
            args.loudness = parse_target(args.loudness)
        except ValueError as e:
            parser.error(f"--loudness {e}")
        if args.loudness == "source" and args.tar_accomp is None:
            parser.error("--loudness source aims vocal + accompaniment at the source's loudness: it needs --tar_accomp (give a number of LUFS for one stem)")
        if not args.peak_ceiling > 0:
            parser.error(f"--peak_ceiling {args.peak_ceiling}: must be positive")
    if args.limiter is not None:
        if args.loudness is None:
            parser.error("--limiter belongs to --loudness: the peak rule never exceeds its peak, so there is nothing to limit")
        sources = [os.path.join(args.src, f) for f in sorted(os.listdir(args.src)) if f.endswith(".wav")] if os.path.isdir(args.src) else [args.src]
        for path in sources:                                           # the half-width is counted at the rate that is written: the file's
            head = wav_info(path)
            try:
                half_width(head["rate"] if head else 44100, args.limiter)
            except ValueError as e:
                parser.error(f"--limiter {args.limiter:g}: {path}: {e}")
    if args.f0_csv is not None and not args.vocal_solo:
        parser.error("--f0_csv tracks the vocal stem, and --vocal_solo 0 writes none: drop one of the two")
    if args.f0_smooth and args.f0_csv is None:
        parser.error("--f0_smooth belongs to --f0_csv: it chooses which pitch track that file holds")
    if args.tar_accomp is not None and not args.vocal_solo:
        parser.error("--tar_accomp writes the vocal to --tar and the accompaniment to --tar_accomp: it cannot be combined with --vocal_solo 0")

    if not torch.cuda.is_available():
        print("separate.py needs a ROCm device (hand-written gfx950 kernels, no CPU path).")
        sys.exit(1)
    device = torch.device("cuda")
    model = load_checkpoint_model(args.model_path, device, ema=args.ema, tool="separate.py")

    if os.path.isdir(args.src):
        os.makedirs(args.tar, exist_ok=True)
        if args.tar_accomp is not None:
            os.makedirs(args.tar_accomp, exist_ok=True)
        if args.f0_csv is not None:
            os.makedirs(args.f0_csv, exist_ok=True)
        jobs = [(os.path.join(args.src, f), os.path.join(args.tar, f), None if args.tar_accomp is None else os.path.join(args.tar_accomp, f),
                 None if args.f0_csv is None else os.path.join(args.f0_csv, f[:-4] + ".csv"))
                for f in sorted(os.listdir(args.src)) if f.endswith(".wav")]
    else:
        jobs = [(args.src, args.tar, args.tar_accomp, args.f0_csv)]
    print(f"Found {len(jobs)} files, separating...")
    for src, dst, dst_accomp, f0_csv in jobs:
        report = {}
        frames, channels = separate_to_wav(model, src, dst, vocal_solo=bool(args.vocal_solo), precision=args.precision,
                                           subtype=args.subtype, keep_length=not args.no_keep_length, n_fft=args.win_size,
                                           hop=args.hop_size, dst_accomp_path=dst_accomp, tile_hop=args.tile_hop,
                                           phase_iters=args.phase_iters, wiener_iters=args.wiener_iters, loudness=args.loudness,
                                           ceiling=args.peak_ceiling, report=report, fullband=args.fullband,
                                           true_peak=args.true_peak, dither=args.dither, dither_seed=args.dither_seed,
                                           limiter_ms=args.limiter, f0={"smooth": True} if args.f0_smooth else None, f0_csv_path=f0_csv)
        print(f"{dst}: {frames} frames x {channels}" + ("" if dst_accomp is None else f"; {dst_accomp}: the same")
              + (f"; {describe(report['info'], report['gain'], args.true_peak)}" if "info" in report else "")
              + (f"; {describe_limiter(**report['limiter'])}" if "limiter" in report else "")
              + (f"; true peak {max(max(row) for row in report['true_peaks']):.2f} dBTP" if "true_peaks" in report else "")
              + (f"; {f0_csv}: {report['f0'].f0.shape[-1]} pitch frames" if "f0" in report else ""))
    print("Separation finished!")


if __name__ == "__main__":
    main()
