#!/usr/bin/env python3
"""A/B two builds of libsvs_hip.so on every conv GEMM call of a training step, interleaved in ONE process on
ONE device (devices differ by up to ~12%, so numbers from different gpurun calls cannot be compared).

    python tools/ab_libs.py tools/bin/libsvs_hip_A.so svs_unet_pytorch_amd/libsvs_hip.so [--batch 64]

--full-step times instead the whole full-objective training pass (svs_unet_train_fwd_loss_mr + svs_unet_train_bwd_part: forward,
L1 + MR-STFT losses, backward; no Adam) on 512 x 128 tiles at hop 768, alternating the two libraries round by round, and
prints one JSON line.  Give it two builds of the SAME commit first: the B/A it prints for them is the spread of the harness.
--eval-bf16 [--hw H W] does the same for the bf16 eval forward (svs_unet_forward_eval_bf16) and compares every layer's output bitwise.
--separate does the same for tools/stream_bench.py's case (streaming.separate_waveform on 240 s of stereo, default arguments, so
disjoint tiles), in fp32 and bf16, one JSON line each, and compares the separated samples bitwise.
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svs_unet_pytorch_amd import _lib  # noqa: E402
from svs_unet_pytorch_amd.synth import ENC_CHANNELS as CH  # noqa: E402

DEC = ((512, 256), (512, 128), (256, 64), (128, 32), (64, 16))


def load(path):
    h = ctypes.CDLL(os.path.abspath(path))
    for name in ("svs_enc_block_fwd", "svs_dec_block_fwd", "svs_enc_block_bwd_weight", "svs_unet_train_fwd_loss_mr", "svs_unet_train_bwd_part",
                 "svs_unet_train_workspace_bytes", "svs_unet_train_mr_workspace_bytes", "svs_unet_prepared_bytes", "svs_unet_prepare_eval",
                 "svs_unet_prepared_bf16_bytes", "svs_unet_prepare_eval_bf16", "svs_unet_eval_bf16_workspace_bytes",
                 "svs_unet_forward_eval_bf16", "svs_unet_ws_offset"):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib._SIGS[name]
    return h


def timeit(fn, reps=10):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def full_step(libs, B, rounds=7, reps=10):
    """Best-of-`rounds` ms of the full-objective pass per library, the libraries taking turns inside every round."""
    import json

    from svs_unet_pytorch_amd import synth
    from svs_unet_pytorch_amd.model import UNet
    H, W, hop, dev = 512, 128, 768, "cuda"
    model = UNet().to(dev).train()
    mix_np, voc_np = synth.tiles(B, H, W, first_tile=800)
    mix, voc = torch.from_numpy(mix_np).to(dev), torch.from_numpy(voc_np).to(dev)
    mph, vph = ((torch.rand((B, 1, H, W), device=dev) * 2 - 1) * 3.14159 for _ in range(2))
    drop = (torch.rand(B * (256 + 128 + 64 + 32 + 16), device=dev) > 0.5).float() * 2
    grads, losses = torch.empty_like(model._flat), torch.empty(2, device=dev)
    S = _lib.stream_ptr
    runs, out = [], []
    for Lb in libs:
        ws = torch.empty(int(Lb.svs_unet_train_workspace_bytes(B, H, W)), dtype=torch.uint8, device=dev)
        mr = torch.empty(int(Lb.svs_unet_train_mr_workspace_bytes(B, W, hop)), dtype=torch.uint8, device=dev)

        def run(Lb=Lb, ws=ws, mr=mr):
            rc = Lb.svs_unet_train_fwd_loss_mr(model._flat.data_ptr(), model._bn_flat.data_ptr(), model._nbt_flat.data_ptr(), mix.data_ptr(),
                                               voc.data_ptr(), mph.data_ptr(), vph.data_ptr(), drop.data_ptr(), B, H, W, hop, 166.66, 1.0, None,
                                               losses.data_ptr(), ws.data_ptr(), ws.numel(), mr.data_ptr(), mr.numel(), S())
            rc = rc or Lb.svs_unet_train_bwd_part(model._flat.data_ptr(), grads.data_ptr(), mix.data_ptr(), drop.data_ptr(), B, H, W, 4,
                                                  ws.data_ptr(), ws.numel(), S())
            assert rc == 0, rc
        runs.append(run)
        run()
        torch.cuda.synchronize()
        out.append((grads.clone(), losses.clone()))
    best = [1e9, 1e9]
    for _ in range(rounds):
        for i, r in enumerate(runs):
            best[i] = min(best[i], timeit(r, reps))
    print(json.dumps({"what": "full-objective fwd + losses + bwd, H=512 W=128 hop=768", "batch": B, "ms_A": round(best[0], 4),
                      "ms_B": round(best[1], 4), "B_over_A": round(best[1] / best[0], 4),
                      "grads_bitwise_equal": bool(torch.equal(out[0][0], out[1][0])), "losses_bitwise_equal": bool(torch.equal(out[0][1], out[1][1]))}))


def eval_bf16(libs, B, H, W, rounds=7, reps=10):
    """Best-of-`rounds` ms of svs_unet_forward_eval_bf16 per library, the libraries taking turns inside every round.  Each library
    prepares the closed-form checkpoint itself and runs on the same seeded input into a sentinel-filled workspace; the workspace
    from its start to the end of c6 (every layer's bf16 output) and the mask are compared bitwise."""
    import json

    import numpy as np

    from svs_unet_pytorch_amd import synth
    from svs_unet_pytorch_amd.model import UNet
    dev = "cuda"
    model = UNet()
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state().items()})
    model.to(dev).eval()
    mix = torch.rand((B, 1, H, W), device=dev, generator=torch.Generator(dev).manual_seed(0))
    h6, w6 = H, W
    for _ in range(6):
        h6, w6 = (h6 + 1) // 2, (w6 + 1) // 2
    S = _lib.stream_ptr
    runs, out = [], []
    for Lb in libs:
        f32 = torch.empty(int(Lb.svs_unet_prepared_bytes()), dtype=torch.uint8, device=dev)
        blob = torch.empty(int(Lb.svs_unet_prepared_bf16_bytes()), dtype=torch.uint8, device=dev)
        rc = Lb.svs_unet_prepare_eval(model._flat.data_ptr(), model._bn_flat.data_ptr(), f32.data_ptr(), S())
        rc = rc or Lb.svs_unet_prepare_eval_bf16(f32.data_ptr(), blob.data_ptr(), S())
        assert rc == 0, rc
        nbytes = int(Lb.svs_unet_eval_bf16_workspace_bytes(B, H, W))
        ws = torch.full((nbytes // 2,), 0x7FC1, dtype=torch.int16, device=dev)          # a bf16 NaN no kernel computes
        mask = torch.full_like(mix, float("nan"))
        span = Lb.svs_unet_ws_offset(b"c6", B, H, W, 2) + 2 * B * h6 * w6 * CH[6]

        def run(Lb=Lb, blob=blob, ws=ws, mask=mask, nbytes=nbytes):
            rc = Lb.svs_unet_forward_eval_bf16(blob.data_ptr(), mix.data_ptr(), mask.data_ptr(), B, H, W, ws.data_ptr(), nbytes, S())
            assert rc == 0, rc
        runs.append(run)
        run()
        torch.cuda.synchronize()
        out.append((ws[:span // 2].clone(), mask.clone()))
    best = [1e9, 1e9]
    for _ in range(rounds):
        for i, r in enumerate(runs):
            best[i] = min(best[i], timeit(r, reps))
    print(json.dumps({"what": f"bf16 eval forward, H={H} W={W}", "batch": B, "ms_A": round(best[0], 4), "ms_B": round(best[1], 4),
                      "B_over_A": round(best[1] / best[0], 4), "workspace_bitwise_equal": bool(torch.equal(out[0][0], out[1][0])),
                      "mask_bitwise_equal": bool(torch.equal(out[0][1], out[1][1]))}))


def separate(paths, seconds=240.0, rate=44100, rounds=7, reps=5):
    """Best-of-`rounds` ms of separate_waveform per library, the libraries taking turns inside every round: the package's
    handle (_lib._lib) is swapped between two fully bound ones, and each library has a model of its own (the same checkpoint), so
    that the weights it prepared stay its own."""
    import json

    import numpy as np

    from svs_unet_pytorch_amd import synth
    from svs_unet_pytorch_amd.model import UNet
    from svs_unet_pytorch_amd.streaming import separate_waveform
    handles = []
    for path in paths:
        h = ctypes.CDLL(os.path.abspath(path))
        for name, (res, args) in _lib._SIGS.items():
            if hasattr(h, name):                                     # (an older build lacks the entry points added since)
                fn = getattr(h, name)
                fn.restype, fn.argtypes = res, args
        handles.append(h)
    n = int(seconds * rate)
    y = torch.from_numpy(np.stack([synth.audio(n, 20), synth.audio(n, 21)])).to("cuda")
    for precision in ("fp32", "bf16"):
        models, out = [], []
        for h in handles:
            _lib._lib = h
            model = UNet()
            model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state().items()})
            models.append(model.to("cuda").eval())
            out.append(separate_waveform(models[-1], y, precision=precision).clone())
        best = [1e9, 1e9]
        for _ in range(rounds):
            for i, h in enumerate(handles):
                _lib._lib = h
                best[i] = min(best[i], timeit(lambda: separate_waveform(models[i], y, precision=precision), reps))
        print(json.dumps({"what": f"separate_waveform, {seconds:.0f} s stereo, disjoint tiles (tile_hop 128)", "precision": precision,
                          "ms_A": round(best[0], 4), "ms_B": round(best[1], 4), "B_over_A": round(best[1] / best[0], 4),
                          "samples_bitwise_equal": bool(torch.equal(out[0], out[1]))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--wgrad", action="store_true")
    ap.add_argument("--full-step", action="store_true")
    ap.add_argument("--eval-bf16", action="store_true")
    ap.add_argument("--separate", action="store_true")
    ap.add_argument("--hw", type=int, nargs=2, default=(512, 128), metavar=("H", "W"), help="tile size of --eval-bf16")
    a = ap.parse_args()
    torch.zeros(1, device="cuda")
    if a.separate:
        return separate([a.lib_a, a.lib_b])
    libs = [load(a.lib_a), load(a.lib_b)]
    if a.full_step:
        return full_step(libs, a.batch)
    if a.eval_bf16:
        return eval_bf16(libs, a.batch, *a.hw)
    B, dev = a.batch, "cuda"
    hw = [(512, 128)]
    for _ in range(6):
        hw.append(((hw[-1][0] + 1) // 2, (hw[-1][1] + 1) // 2))
    calls = []
    for k in range(2, 7):
        calls.append((f"conv{k}.fwd", "gather", (*hw[k - 1], CH[k - 1]), (*hw[k], CH[k])))
        calls.append((f"conv{k}.bwd_data", "parity", (*hw[k], CH[k]), (*hw[k - 1], CH[k - 1])))
    for j, (c, n) in enumerate(DEC):
        calls.append((f"deconv{j + 1}.fwd", "parity", (*hw[6 - j], c), (*hw[5 - j], n)))
        calls.append((f"deconv{j + 1}.bwd_data", "gather", (*hw[5 - j], n), (*hw[6 - j], c)))
    ws = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    S = _lib.stream_ptr
    tot = [0.0, 0.0]
    for name, mode, (h, w, C), (ho, wo, N) in calls:
        x = torch.rand((B, h, w, C), device=dev) - 0.5
        wp = (torch.rand(N * C * 25, device=dev) - 0.5) * 0.05
        ys = [torch.empty((B, ho, wo, N), device=dev) for _ in libs]
        runs = []
        for L, y in zip(libs, ys):
            if mode == "gather":
                runs.append(lambda L=L, y=y: L.svs_enc_block_fwd(x.data_ptr(), C, B, h, w, C, wp.data_ptr(), None, None, None, 0.0, y.data_ptr(),
                                                                 N, N, 0, ws.data_ptr(), ws.numel(), S()))
            else:
                runs.append(lambda L=L, y=y: L.svs_dec_block_fwd(x.data_ptr(), C, B, h, w, C, wp.data_ptr(), None, None, None, 0.0, y.data_ptr(),
                                                                 N, ho, wo, N, 0, ws.data_ptr(), ws.numel(), S()))
        for r in runs:
            assert r() == 0
        torch.cuda.synchronize()
        same = (ys[0] - ys[1]).abs().max().item()
        best = [1e9, 1e9]
        for _ in range(3):
            for i, r in enumerate(runs):
                best[i] = min(best[i], timeit(r))
        gflop = 2.0 * B * (ho * wo if mode == "gather" else h * w) * N * C * 25 / 1e9
        tot[0] += best[0]
        tot[1] += best[1]
        print(f"{name:18s} A {best[0] * 1e3:7.1f} us {gflop / best[0]:6.1f} TF   B {best[1] * 1e3:7.1f} us {gflop / best[1]:6.1f} TF   B/A time {best[1] / best[0]:.3f}  maxdiff {same:.1e}",
              flush=True)
    print(f"TOTAL conv A {tot[0] * 1e3:.1f} us   B {tot[1] * 1e3:.1f} us   B/A {tot[1] / tot[0]:.3f}")
    if not a.wgrad:
        return
    tot = [0.0, 0.0]
    wg = [(f"conv{k}.bwd_weight", hw[k], CH[k], hw[k - 1], CH[k - 1]) for k in range(2, 7)]
    wg += [(f"deconv{j + 1}.bwd_weight", hw[6 - j], c, hw[5 - j], n) for j, (c, n) in enumerate(DEC)]
    for name, (hs, wsz), cs, (hl, wl), cl in wg:
        sm = torch.rand((B, hs, wsz, cs), device=dev) - 0.5
        lg = torch.rand((B, hl, wl, cl), device=dev) - 0.5
        dws = [torch.empty(cs * cl * 25, device=dev) for _ in libs]
        runs = [lambda L=L, dw=dw: L.svs_enc_block_bwd_weight(sm.data_ptr(), cs, B, hs, wsz, cs, lg.data_ptr(), cl, hl, wl, cl, dw.data_ptr(),
                                                              None, ws.data_ptr(), ws.numel(), S()) for L, dw in zip(libs, dws)]
        for r in runs:
            assert r() == 0
        torch.cuda.synchronize()
        same = ((dws[0] - dws[1]).abs().max() / dws[0].abs().max()).item()
        best = [1e9, 1e9]
        for _ in range(3):
            for i, r in enumerate(runs):
                best[i] = min(best[i], timeit(r))
        gflop = 2.0 * B * hs * wsz * cs * cl * 25 / 1e9
        tot[0] += best[0]
        tot[1] += best[1]
        print(f"{name:20s} A {best[0] * 1e3:7.1f} us {gflop / best[0]:6.1f} TF   B {best[1] * 1e3:7.1f} us {gflop / best[1]:6.1f} TF   B/A time {best[1] / best[0]:.3f}  reldiff {same:.1e}",
              flush=True)
    print(f"TOTAL wgrad A {tot[0] * 1e3:.1f} us   B {tot[1] * 1e3:.1f} us   B/A {tot[1] / tot[0]:.3f}")


if __name__ == "__main__":
    main()
