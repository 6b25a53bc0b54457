"""ORACLE -- TEST INFRASTRUCTURE ONLY.  Never imported by the product package.

The bf16 eval network (csrc/gemm_bf16.hip) restated on the CPU in plain torch, one layer at a time, so that each of its
kernels can be held against a reference of ITS OWN arithmetic instead of against the fp32 network's mask:

  folding      scale = gamma / sqrt(running_var + eps), shift = beta + (bias - running_mean) * scale in fp32 (svs_bn_fold);
               weights = bf16_rne(fp32(w) * fp32(scale[n])) -- one fp32 multiply, then round to nearest even, as the packing
               kernels do; deconv6 = bf16_rne(w) with its fp32 bias and no scale.
  reference    "teacher forced": a layer's exact bf16 input (whoever produced it), its bf16 weights, the convolution in
               fp64 -- every product of two bf16 values is exact there -- plus the fp32 shift, LeakyReLU 0.2 (encoder) or ReLU
               (decoder); deconv6: sigmoid(sum + bias).  conv1 reads fp32 samples as two bf16 limbs, hi = bf16(x),
               lo = bf16(x - hi), so its input is hi + lo.
  bound        a kernel stores bf16_rne(act(acc32 + shift)).  With r the reference, S the fp64 convolution of |input| with
               |weights| plus |shift|, K the reduction length (25 C for a convolution, 9 C -- its largest parity class -- for
               a transposed one) and E = K 2^-23 S (the fp32 summation bound gamma_K S, doubled because the summation order
               inside an MFMA is not documented):
                   |got - r| <= 2^-8 |r| + (1 + 2^-8) E          for every element,
               half a bf16 ulp of the rounded value plus the accumulation error, which may also carry the value across a
               rounding tie.  For the mask: |got - r| <= 0.25 E + 1e-5 (sigmoid' <= 1/4; 1e-5 is what the fp32 path's test
               of the same __expf sigmoid accepts).  Nothing in the bound is fitted to a measurement.
  emulation    a free-running CPU network of the same number formats (fp32 conv2d accumulation, bf16 rounding per layer):
               what the reference and the bound are tried on without a GPU (tests/test_bf16_oracle.py).
"""
from __future__ import annotations

from collections import OrderedDict, namedtuple

import torch
import torch.nn.functional as F

BN_EPS = 1e-5
LEAKY_SLOPE = 0.2
CH = (1, 16, 32, 64, 128, 256, 512)

# name, transposed?, input channels, output channels, input level, output level (level k = the input ceil-halved k times)
Layer = namedtuple("Layer", "name up C N lin lout")
LAYERS = tuple([Layer(f"conv{k}", False, CH[k - 1], CH[k], k - 1, k) for k in range(1, 7)] +
               [Layer("deconv1", True, 512, 256, 6, 5), Layer("deconv2", True, 512, 128, 5, 4), Layer("deconv3", True, 256, 64, 4, 3),
                Layer("deconv4", True, 128, 32, 3, 2), Layer("deconv5", True, 64, 16, 2, 1), Layer("deconv6", True, 32, 1, 1, 0)])
BY_NAME = {L.name: L for L in LAYERS}


def level_sizes(H, W):
    hw = [(H, W)]
    for _ in range(6):
        hw.append(((hw[-1][0] + 1) // 2, (hw[-1][1] + 1) // 2))
    return hw


def bf16_rne(t):
    """fp32 -> nearest bf16 (ties to even) -> fp32."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def _bn_prefix(L):
    return f"{L.name}.1" if not L.up else f"{L.name}_BAD.0"


def _w_key(L):
    return f"{L.name}.0.weight" if not L.up else f"{L.name}.weight"


def fold_scale_shift(state):
    """{layer: (scale, shift)} in fp32 as svs_bn_fold computes them; deconv6: (None, bias)."""
    out = OrderedDict()
    for L in LAYERS:
        bias = state[_w_key(L).replace("weight", "bias")].to(torch.float32)
        if L.name == "deconv6":
            out[L.name] = (None, bias)
            continue
        p = _bn_prefix(L)
        g, b = state[p + ".weight"].to(torch.float32), state[p + ".bias"].to(torch.float32)
        rm, rv = state[p + ".running_mean"].to(torch.float32), state[p + ".running_var"].to(torch.float32)
        s = g / torch.sqrt(rv + torch.tensor(BN_EPS, dtype=torch.float32))
        out[L.name] = (s, b + (bias - rm) * s)
    return out


def fold_weights(state, fold):
    """{layer: weights} in torch's layout (Conv2d (N, C, 5, 5), ConvTranspose2d (C, N, 5, 5)), fp32 tensors whose values are
    the bf16 weights the kernels multiply with."""
    out = OrderedDict()
    for L in LAYERS:
        w = state[_w_key(L)].to(torch.float32)
        s = fold[L.name][0]
        if s is not None:
            w = w * (s[None, :, None, None] if L.up else s[:, None, None, None])
        out[L.name] = bf16_rne(w)
    return out


def split_hi_lo(x):
    """The two bf16 limbs conv1 reads an fp32 sample as."""
    hi = bf16_rne(x)
    return hi, bf16_rne(x.to(torch.float32) - hi)


def _conv(L, x, w, out_hw):
    if not L.up:
        return F.conv2d(x, w, None, stride=2, padding=2)
    op = (out_hw[0] - (2 * x.shape[-2] - 1), out_hw[1] - (2 * x.shape[-1] - 1))
    assert op[0] in (0, 1) and op[1] in (0, 1), (x.shape, out_hw)
    return F.conv_transpose2d(x, w, None, stride=2, padding=2, output_padding=op)


def _out_hw(L, x, out_hw):
    if out_hw is not None:
        return tuple(out_hw)
    assert not L.up, "a transposed layer needs its output size"
    return ((x.shape[-2] + 1) // 2, (x.shape[-1] + 1) // 2)


def layer_reference(L, x, w, shift, out_hw=None):
    """(r, S) in fp64 for layer L on the input x (B, C, H, W): bf16 values in any float dtype, fp32 samples for conv1;
    w = fold_weights()[L.name], shift = fold_scale_shift()[L.name][1]."""
    out_hw = _out_hw(L, x, out_hw)
    if L.name == "conv1":
        hi, lo = split_hi_lo(x)
        x64 = hi.double() + lo.double()
    else:
        x64 = x.double()
    w64, sh = w.double(), shift.double()[None, :, None, None]
    pre = _conv(L, x64, w64, out_hw) + sh
    S = _conv(L, x64.abs(), w64.abs(), out_hw) + sh.abs()
    if L.name == "deconv6":
        r = torch.sigmoid(pre)
    elif L.up:
        r = torch.clamp(pre, min=0.0)
    else:
        r = torch.where(pre > 0, pre, pre * float(torch.tensor(LEAKY_SLOPE, dtype=torch.float32)))
    return r, S


def reduction_length(L):
    return (9 if L.up else 25) * L.C


def tolerance(L, r, S):
    """The derived elementwise bound on |got - r| (module docstring)."""
    E = reduction_length(L) * 2.0 ** -23 * S
    if L.name == "deconv6":
        return 0.25 * E + 1e-5
    return 2.0 ** -8 * r.abs() + (1 + 2.0 ** -8) * E


def worst_ratio(L, got, r, S):
    """max over the elements of |got - r| / bound; inf where got is not finite."""
    err = (got.double() - r).abs()
    ratio = err / tolerance(L, r, S)
    ratio = torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def layer_emulate(L, x, w, shift, out_hw=None):
    """The layer in the kernels' number formats: fp32 accumulation, one rounding to bf16 (the mask stays fp32)."""
    out_hw = _out_hw(L, x, out_hw)
    w = w.to(torch.float32)
    if L.name == "conv1":
        hi, lo = split_hi_lo(x)
        acc = _conv(L, lo, w, out_hw) + _conv(L, hi, w, out_hw)
    else:
        acc = _conv(L, x.to(torch.float32), w, out_hw)
    pre = acc + shift.to(torch.float32)[None, :, None, None]
    if L.name == "deconv6":
        return torch.sigmoid(pre)
    return bf16_rne(F.relu(pre) if L.up else F.leaky_relu(pre, LEAKY_SLOPE))


def layer_input(L, mix, outs):
    """Input of layer L from the outputs of the layers before it: cat([decoder output, skip], 1) for deconv2..deconv6."""
    if L.name == "conv1":
        return mix
    if not L.up:
        return outs[f"conv{L.lin}"]
    if L.name == "deconv1":
        return outs["conv6"]
    return torch.cat([outs[f"deconv{6 - L.lin}"], outs[f"conv{L.lin}"]], dim=1)


def emulate(state, mix, weights=None):
    """Free-running network: {layer: output} (bf16 values as fp32; "deconv6" is the fp32 mask).  `weights` replaces entries of
    fold_weights() (mutation tests)."""
    fold = fold_scale_shift(state)
    w = fold_weights(state, fold)
    if weights:
        w.update(weights)
    hw = level_sizes(*mix.shape[-2:])
    outs = OrderedDict()
    for L in LAYERS:
        outs[L.name] = layer_emulate(L, layer_input(L, mix, outs), w[L.name], fold[L.name][1], hw[L.lout])
    return outs


# ---- the shapes tests/test_gpu_bf16_layers.py runs, and which images of a large batch get a reference ----------------
# (key, shapes (B, H, W), planner switches, what the case reaches)
Case = namedtuple("Case", "key shapes switches reaches")
CASES = (
    Case("a", ((2, 70, 50),), (), "all-GEMM network, ragged at every level, split-K 6 / 12 / 25 and 8 / 8 / 4 / 2 / 1"),
    Case("b", ((3, 31, 17), (1, 1, 1)), (), "levels that collapse to 1x1: every tap but the centre is padding"),
    Case("c", ((1, 512, 128),), (), "the production tile"),
    Case("d", ((130, 66, 126),), (), "the three window kernels on ragged tiles, conv4 on 128x128, wraps in conv2 / conv3 / deconv5 / deconv6"),
    Case("e", ((2100, 16, 32),), (), "wraps in conv1 and the deconv3 window"),
    Case("f", ((260, 72, 136),), (), "wraps in the deconv4 window"),
    Case("g", ((2, 70, 50),), (("BF16_CFG", 0),), "the 128x128 tile on a part-filled M tile"),
    Case("h", ((2, 70, 50),), (("BF16_CFG", 1), ("BF16_KSPLIT", 1)), "the 128x64 gather tile, no split"),
    Case("i", ((2, 70, 50),), (("BF16_KSPLIT", 32),), "the K-split cap, uneven K ranges per split"),
    Case("j", ((16, 64, 128),), (("CONV_WINDOW", 0),), "the GEMM form of the window layers at more than one M tile"),
)
# persistent kernels: (layer, level its tiles cover, tile rows, tile columns, most blocks) -- a block walks tiles
# blockIdx, + grid, ...; the tiles on either side of each multiple of the grid are where that walk can go wrong
PERSISTENT = (("conv1", 1, 16, 32, 2048), ("conv2", 2, 8, 16, 768), ("conv3", 3, 8, 16, 256), ("deconv3", 4, 16, 8, 256),
              ("deconv4", 3, 8, 16, 512), ("deconv5", 2, 8, 16, 512), ("deconv6", 1, 8, 16, 2048))
# a whole batch gets its reference while that takes a second or two on the CPU: up to 1.1 M input pixels in up to 512 images
# (the time grows with the image count too: 2100 images of 16 x 32 take as long as 260 of 72 x 136, about five seconds)
FULL_REFERENCE_PIXELS, FULL_REFERENCE_IMAGES = 1100000, 512


def covered_images(B, H, W):
    """Images of a (B, H, W) batch that get a reference: all of them when that takes a second or two; else images 0, 1, B - 1, the
    images on both sides of every persistent-grid wrap, and eight more spread evenly."""
    if B * H * W <= FULL_REFERENCE_PIXELS and B <= FULL_REFERENCE_IMAGES:
        return list(range(B))
    hw = level_sizes(H, W)
    keep = {0, 1, B - 1}
    for _, lvl, th, tw, grid in PERSISTENT:
        per_image = -(-hw[lvl][0] // th) * -(-hw[lvl][1] // tw)
        for first in range(grid, B * per_image, grid):
            keep.update(((first - 1) // per_image, first // per_image))
    rest = [b for b in range(B) if b not in keep]
    keep.update(rest[(2 * i + 1) * len(rest) // 16] for i in range(8))
    return sorted(keep)


def case_input(H, W, images):
    """mix (len(images), 1, H, W) in [0, 1): image b is the same whichever batch it is part of."""
    import numpy as np
    from svs_unet_pytorch_amd import synth
    x = np.stack([synth.uniform(synth.SEED_MIX, H * W, (5000 + b) << 32).reshape(1, H, W) for b in images])
    return torch.from_numpy(x)


WINDOW_KERNELS = {"parity_window_bf16_kernel<256, 4, 8>": "window<256>", "parity_window_bf16_kernel<128, 2, 16>": "window<128>",
                  "parity_window_bf16_kernel<64, 1, 16>": "window<64>"}
PLANNED = ("conv4", "conv5", "conv6", "deconv1", "deconv2", "deconv3", "deconv4", "deconv5")      # the layers plan_bf16 plans


def describe_plan(lib, L, B, H, W):
    """(kernel name as svs_describe_plan gives it, short form "BMxBN" / "window<C>", K-split) of planned layer L in a
    (B, H, W) forward, under the planner switches now set."""
    import ctypes
    hw = level_sizes(H, W)
    buf = ctypes.create_string_buffer(128)
    ks = lib.svs_describe_plan(4 if L.up else 3, B, hw[L.lin][0], hw[L.lin][1], L.C, hw[L.lout][0], hw[L.lout][1], L.N, buf, 128)
    full = buf.value.decode()
    if full in WINDOW_KERNELS:
        return full, WINDOW_KERNELS[full], ks
    args = full[full.index("<") + 1:-1].split(", ")
    assert full.startswith("conv_gemm_bf16_kernel<") and int(args[0]) == int(L.up), full
    return full, f"{args[1]}x{args[2]}", ks
