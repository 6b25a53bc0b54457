"""Per-stage parity of the training step (-m gpu): after ONE svs_unet_train_fwd_bwd every activation, pre-BatchNorm output,
batch statistic and data gradient is still in the workspace (svs_unet_ws_offset(..., 1)).  Each is checked against
oracle/train_stage_oracle.py's fp64 reference computed from the GPU's OWN buffers one stage upstream, so no error
accumulates and every row is gated like the kernel that wrote it is gated on its own in test_gpu_ops.py (2e-5 / 1e-5; 4e-5
where a BatchNorm backward and a conv backward lie between the buffers) -- not at the 1e-2 the whole-step gates of
test_gpu_unet.py need.  This is the only place that sees the forms the step really calls: svs_enc_block_bwd_data accumulating
into the strided / planar skip half of dcat, the bias gradients out of svs_bn_bwd_run (deferred partials, and the direct
branch under TRAIN_UNFUSED), the planar level-1 forms of conv1 / deconv6, BatchNorm partials from the GEMM epilogue, and all
of it at odd sizes where Ho = 2H - 1 and 2H both occur and every last tile is ragged.

Bias gradients in front of a BatchNorm are zero in exact arithmetic; their row is |db| / (P 2^-24 sum|d_raw_ref|) <= 1 (see
the oracle).  That bound is WEAK at level 1 (one dropped pixel is only 3-16 times the bound there) and strong from level 2
down (a dropped eighth of the pixels is 3e2 .. 4e5 times the bound: tests/test_train_stage_oracle.py).  Every case keeps
P >= 16 at every level; below that the cancellation inside the BatchNorm backward leaves no meaningful relative gate."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import train_stage_oracle as ts
from oracle import unet_oracle as uo
from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7FC17FC1      # an fp32 NaN no kernel computes: read anywhere, it shows
GUARD = 4096               # bytes allocated past the workspace the library is told about

FORCED = (("CONV_WINDOW", 2), ("CONV_GWINDOW", 2), ("CONV_SKIP", 2), ("WGRAD_SKIP", 2), ("WGRAD_WINDOW", 2), ("CONV_C1_TILED", 2))
# key: (B, H, W, planner switches, dropout, loss_scale, first tile, kernel-name fragments that must appear in the plan)
CASES = {
    # levels 65x34, 33x17, 17x9, 9x5, 5x3, 3x2: 2H and 2H-1 in each dimension, ragged last tiles at every level
    "odd_default": (3, 130, 68, (), True, 1.0, 2100, ()),
    # the direct dbias branch of svs_bn_bwd_run, a finalise launch per layer, one shared d_raw
    "odd_one_stream_unfused": (3, 130, 68, (("TRAIN_ONE_STREAM", 1), ("TRAIN_UNFUSED", 1), ("BN_INLINE", 0)), True, 1.0, 2100, ()),
    # every production form where the shape is eligible.  (The tap-skipping weight-gradient GEMM needs a power-of-two batch
    # >= 16: no layer is eligible at B = 3 whatever WGRAD_SKIP says; the planner takes it by itself at B = 64 below, where
    # it is asserted)
    "odd_forced_forms": (3, 130, 68, FORCED, True, 1.0, 2100,
                         ("gather_window_kernel", "parity_window_kernel<", "wgrad_window_kernel<", "conv_gemm_kernel<0, skip", "conv_gemm_kernel<1, skip")),
    # position-uniform kernels with BatchNorm partials from the GEMM epilogue, the batch-64 planner, 1x1 images at levels 5, 6
    "b64_uniform": (64, 32, 8, (("CONV_KSPLIT", 1),), True, 1.0, 2200,
                    ("conv_gemm_kernel<0, uniform", "conv_gemm_kernel<1, uniform", "wgrad_gemm_kernel<skip")),
    "odd_nodrop_scaled": (3, 130, 68, (), False, 166.66, 2100, ()),
}


def describe(L, kind, *shape):
    buf = ctypes.create_string_buffer(160)
    ks = L.svs_describe_plan(kind, *shape, buf, 160)
    return buf.value.decode(), ks


def layer_plans(B, H, W, switches):
    """{layer: {"fwd" | "bwd" | "wgrad": kernel name as svs_describe_plan gives it (+ K-split)}} and the set of name fragments
    the forced-form assertions look for.  conv1 and deconv6 have no planner entry: their single-channel kernels follow
    CONV_C1_TILED alone (special.hip: svs_conv_c1_run)."""
    L = _lib.lib()
    hw = ts.level_sizes(H, W)
    tiled = dict(switches).get("CONV_C1_TILED", -1)
    plans = {"conv1": {"fwd": "conv_c1_tiled_kernel<16>" if tiled == 2 else "conv_c1_kernel<16>", "wgrad": "wgrad_c1"},
             "deconv6": {"fwd": "deconv_to1_kernel", "bwd": "conv_c1_kernel<32>" if tiled == 0 else "conv_c1_tiled_kernel<32>", "wgrad": "wgrad_c1"}}
    seen = set()
    for Ly in ts.LAYERS[1:11]:
        (hi, wi), (ho, wo) = hw[Ly.lin], hw[Ly.lout]
        calls = {"fwd": (1 if Ly.up else 0, B, hi, wi, Ly.C, ho, wo, Ly.N),            # the data gradient is the other mode, roles swapped
                 "bwd": (0 if Ly.up else 1, B, ho, wo, Ly.N, hi, wi, Ly.C),
                 "wgrad": (2, B, hi, wi, Ly.C, 0, 0, Ly.N) if Ly.up else (2, B, ho, wo, Ly.N, 0, 0, Ly.C)}
        plans[Ly.name] = {}
        for what, call in calls.items():
            full, ks = describe(L, *call)
            plans[Ly.name][what] = full if ks == 1 else f"{full} K/{ks}"
            seen.add(full[:full.index("<") + 1] if "<" in full else full)
            args = full[full.index("<") + 1:-1].split(", ") if "<" in full else []
            if full.startswith("conv_gemm_kernel<"):                                       # <mode, BM, BN, WM, WN, uniform, skip, split, ahead>
                seen |= {f"conv_gemm_kernel<{args[0]}, skip"} if args[6] == "true" else set()
                seen |= {f"conv_gemm_kernel<{args[0]}, uniform"} if args[5] == "true" else set()
            if full.startswith("wgrad_gemm_kernel<") and args[4] == "true":                # <BM, BN, WM, WN, skip, split, ahead>
                seen.add("wgrad_gemm_kernel<skip")
    return plans, seen


def row_plan(row, plans):
    names = [n for n in row.stage.replace("(", " ").replace(")", " ").split() if n in plans]      # in the order the stage names them
    what = {"raw": "fwd", "mean": "fwd", "invstd": "fwd", "act": "fwd", "running": "fwd", "dw": "wgrad", "dw out": "wgrad",
            "dx": "bwd", "dx skip": "bwd"}.get(row.kind)
    if row.stage == "mask":
        return plans["deconv6"]["fwd"]
    if what is None or not names:
        return {"dgamma": "bn_bwd", "dbeta": "bn_bwd", "db": "bn_bwd", "db out": "sum", "loss": "l1_mask_loss", "d_logit": "l1_mask_loss"}.get(row.kind, "-")
    return " + ".join(plans[n][what] for n in names)


def read_workspace(ws, model, B, H, W):
    """The named buffers of the training workspace as NCHW float32 CPU tensors (level 1: two dense planes, decoder first;
    levels 2..5: [decoder half | skip half] inside every pixel), the BatchNorm buffers after the step with them."""
    L = _lib.lib()
    hw = ts.level_sizes(H, W)
    f32 = ws.view(torch.float32)

    def take(name, *shape):
        off = L.svs_unet_ws_offset(name.encode(), B, H, W, 1)
        assert off >= 0 and off % 256 == 0, (name, off)
        n = int(np.prod(shape))
        return f32[off // 4:off // 4 + n].view(*shape).cpu()

    def nchw(t):
        return t.permute(0, 3, 1, 2).contiguous()

    out = {}
    for stem in ("cat", "dcat"):
        h, w = hw[1]
        out[stem + "1"] = torch.cat([nchw(p) for p in take(stem + "1", 2, B, h, w, 16)], 1)
        for k in range(2, 6):
            h, w = hw[k]
            out[f"{stem}{k}"] = nchw(take(f"{stem}{k}", B, h, w, 2 * ts.CH[k]))
    h, w = hw[6]
    out["c6"], out["dc6"] = nchw(take("c6", B, h, w, 512)), nchw(take("dc6", B, h, w, 512))
    for Ly in ts.BN_LAYERS:
        l = Ly.index
        h, w = hw[Ly.lout]
        out[f"raw{l}"] = nchw(take(f"raw_e{l + 1}" if l < 6 else f"raw_d{l - 5}", B, h, w, Ly.N))
        out[f"mean{l}"], out[f"invstd{l}"] = take(f"mean{l}", Ly.N), take(f"invstd{l}", Ly.N)
        bn = model._bn_list[l]
        out[f"running_mean{l}"], out[f"running_var{l}"] = bn.running_mean.cpu(), bn.running_var.cpu()
    out["d_logit"], out["mask"] = take("d_logit", B, 1, H, W), take("mask", B, 1, H, W)
    return out


@pytest.mark.parametrize("key", list(CASES))
def test_train_stages_against_oracle(key, report, tune):
    """Every row of train_stage_oracle.check() on the workspace one svs_unet_train_fwd_bwd left behind: relative error to the
    reference's max <= the per-kernel gate of that stage; |db| / bound <= 1 in front of a BatchNorm; and the two conditions
    (elements that follow the device's activation branch, elements left out of d_logit) <= 1e-3 of a layer."""
    B, H, W, switches, dropout, loss_scale, first_tile, must_plan = CASES[key]
    for name, value in switches:               # before the workspace query
        tune(name, value)
    L = _lib.lib()
    plans, seen = layer_plans(B, H, W, switches)
    missing = [m for m in must_plan if m not in seen]
    assert not missing, (missing, plans)       # a forced form no layer took proves nothing

    state = synth.closed_form_state(trained_stats=False)
    model = UNet()
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    model = model.to(DEV).train()
    mix_np, voc_np = synth.tiles(B, H, W, first_tile=first_tile)
    masks = [torch.from_numpy(m) for m in synth.dropout_masks(B, seed=77, step=0)] if dropout else []
    model.set_dropout_masks(masks)
    ws_bytes = int(L.svs_unet_train_workspace_bytes(B, H, W))
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ws = torch.full(((ws_bytes + GUARD) // 4,), SENTINEL, dtype=torch.int32, device=DEV)
    model._ws[("train", B, H, W)] = ws.view(torch.uint8)[:ws_bytes]          # the library is told ws_bytes
    model.optim.zero_grad()
    target, tmp = model._grad_target()
    assert tmp is None                                                        # the library overwrites the flat gradient buffer itself
    target.fill_(float("nan"))
    loss = model.fwd_bwd(torch.from_numpy(mix_np).to(DEV), torch.from_numpy(voc_np).to(DEV), loss_scale=loss_scale)
    torch.cuda.synchronize()
    assert model._ws[("train", B, H, W)].data_ptr() == ws.data_ptr()

    assert bool((ws[ws_bytes // 4:] == SENTINEL).all()), "bytes past the workspace were written"
    loss = loss.item()
    assert np.isfinite(loss)
    buffers = read_workspace(ws, model, B, H, W)
    for name, t in buffers.items():
        assert bool(torch.isfinite(t).all()), f"{name}: elements no kernel wrote"
    grads = {n: p.grad.detach().cpu() for n, p in model.named_parameters()}
    for name, g in grads.items():
        assert bool(torch.isfinite(g).all()), f"gradient of {name}: elements no kernel wrote"

    rows = ts.check(buffers, grads, loss, uo.to_torch_state(state), torch.from_numpy(mix_np), torch.from_numpy(voc_np),
                    masks, loss_scale)
    tag = f"B{B} {H}x{W} {key}"
    bad = []
    for r in rows:
        label = f"train stage {r.stage} [{row_plan(r, plans)}] {tag}"
        print(f"{label}: {r.err:.3e} / {r.bound:.1e}")
        report(label, r.err, r.bound)
        if not r.ok:
            bad.append((label, r.err, r.bound))
    assert not bad, bad
