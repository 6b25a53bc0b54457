"""ORACLE -- TEST INFRASTRUCTURE ONLY.  Never imported by the product package.

The fp32 eval network (svs_unet_forward_eval: csrc/net.hip, gemm_conv.hip, special.hip) restated on the CPU in plain torch, one
layer at a time, so that each of its kernels can be held against a reference of its own layer instead of against the mask
behind a sigmoid.  The network description (LAYERS, level_sizes, layer_input), the case inputs and the choice of reference
images are oracle/bf16_oracle.py's; what differs is the arithmetic:

  folding      scale = gamma / sqrt(running_var + eps), shift = beta + (bias - running_mean) * scale in fp32 (svs_bn_fold;
               bf16_oracle.fold_scale_shift).  The weights are the fp32 checkpoint values, UNSCALED: here the scale lives in the
               epilogue, not in the weights.  deconv6 has its fp32 bias and no scale.
  reference    "teacher forced": layer L's fp32 input x (whoever produced it), the convolution in fp64,
                   pre = scale * conv(x, w) + shift,
                   r   = leaky_0.2(pre) (encoder), relu(pre) (decoder), sigmoid(conv(x, w) + bias) (deconv6),
                   S   = |scale| * conv(|x|, |w|) + |shift|          (deconv6: conv(|x|, |w|) + |bias|),
               with the slope the fp32 value of 0.2 the kernels multiply with.
  bound        In the default mode (MFMA_SPLIT off) every product x * w is an fp32 MFMA product accumulated in fp32, or an fp32
               fma of a thread-per-pixel kernel.  Write u = 2^-24 (half an fp32 ulp, relative), T = conv(|x|, |w|) = sum |x w|,
               K = the reduction length: 25 C for a convolution, 9 C -- the largest parity class -- for a transposed one.
                 1. accumulation: a sum of K products in ANY order, one rounding per addition (none per product under fma; one
                    under mul + add, which gamma_K also covers), errs by at most gamma_K T, gamma_K = K u / (1 - K u).  The
                    order inside an MFMA is not documented, so the bound is doubled as bf16_oracle does: |acc - conv| <= 2 K u T
                    = K 2^-23 T.  The doubling also covers a K-split: its slabs are partial sums of disjoint K ranges added in
                    one more chain of at most 64 additions -- another summation order of the same K terms plus ksplit - 1 <= K
                    additions of partial sums, each bounded by T.
                 2. epilogue: pre^ = fl(fl(scale * acc) + shift), or one fma.  scale * (acc - conv) contributes |scale| K 2^-23 T;
                    the multiply's rounding at most u |scale| |acc| <= u (1 + K 2^-23) |scale| T; the addition's at most
                    u |pre^| <= u (1 + ...) (|scale| T + |shift|).  With K 2^-23 <= 8e-4 the second-order factors stay below
                    1.001, so
                        |pre^ - pre| <= K 2^-23 |scale| T + 2.002 u |scale| T + 1.001 u |shift| <= (K + 2) 2^-23 S =: E.
                    (2 u = 2^-23: the two epilogue roundings are ONE of the "+ 2" units; the other is slack for the
                    second-order terms, nothing measured.)
                 3. activation: leaky-ReLU and ReLU are 1-Lipschitz, so |act(pre^) - act(pre)| <= E whichever side of the kink
                    either value is on; the slope multiply rounds once more, u |r^| <= 2 u |r| = 2^-23 |r| once E is counted.
                        |got - r| <= (K + 2) 2^-23 S + 2^-23 |r|          for every element of conv1 .. deconv5.
                 4. mask: the pre-sigmoid sum errs by E (no scale: S = T + |bias|, the bias addition is the "+ 2"'s rounding);
                    sigmoid' <= 1/4, and 1e-5 is what the project accepts for the __expf sigmoid (tests/test_gpu_ops.py and
                    bf16_oracle):
                        |got - r| <= 0.25 E + 1e-5.
               Nothing in the bound is fitted to a measurement.
  emulation    a free-running CPU network of the same number formats (fp32 conv2d / conv_transpose2d, fp32 epilogue): what
               the reference and the bound are tried on without a GPU (tests/test_eval_stage_oracle.py).
"""
from __future__ import annotations

from collections import OrderedDict, namedtuple

import torch
import torch.nn.functional as F

from oracle.bf16_oracle import (BY_NAME, CH, LAYERS, LEAKY_SLOPE, _conv, _out_hw, _w_key, case_input, covered_images,      # noqa: F401
                                fold_scale_shift, layer_input, level_sizes, reduction_length)

SLOPE32 = float(torch.tensor(LEAKY_SLOPE, dtype=torch.float32))
MIN_LIVE = 0.25            # least share of non-zero reference outputs of a decoder (ReLU) layer, and of mask pixels in (0.01, 0.99)


def weights(state):
    """{layer: fp32 checkpoint weights} in torch's layout (Conv2d (N, C, 5, 5), ConvTranspose2d (C, N, 5, 5))."""
    return OrderedDict((L.name, state[_w_key(L)].to(torch.float32)) for L in LAYERS)


def _bcast(v):
    return v.double()[None, :, None, None]


def layer_reference(L, x, w, scale, shift, out_hw=None):
    """(r, S) in fp64 for layer L on the fp32 input x (B, C, H, W); scale, shift = fold_scale_shift()[L.name] (or svs_bn_fold's
    own output); scale is None for deconv6, whose shift is its bias."""
    out_hw = _out_hw(L, x, out_hw)
    x64, w64 = x.double(), w.double()
    conv, T = _conv(L, x64, w64, out_hw), _conv(L, x64.abs(), w64.abs(), out_hw)
    if L.name == "deconv6":
        assert scale is None
        return torch.sigmoid(conv + _bcast(shift)), T + _bcast(shift).abs()
    pre = _bcast(scale) * conv + _bcast(shift)
    S = _bcast(scale).abs() * T + _bcast(shift).abs()
    r = torch.clamp(pre, min=0.0) if L.up else torch.where(pre > 0, pre, pre * SLOPE32)
    return r, S


def tolerance(L, r, S):
    """The derived elementwise bound on |got - r| (module docstring)."""
    E = (reduction_length(L) + 2) * 2.0 ** -23 * S
    if L.name == "deconv6":
        return 0.25 * E + 1e-5
    return E + 2.0 ** -23 * r.abs()


def worst_ratio(L, got, r, S):
    """max over the elements of |got - r| / bound; inf where got is not finite."""
    if isinstance(L, str):
        L = BY_NAME[L]
    got = got.double()
    ratio = (got - r).abs() / tolerance(L, r, S)
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def live_share(L, r):
    """Share of the reference outputs a wrong kernel could show at: non-zero ones (a ReLU layer that is all zero passes any
    comparison), mask pixels away from saturation."""
    if L.name == "deconv6":
        return float(((r > 0.01) & (r < 0.99)).double().mean())
    return float((r != 0).double().mean())


def layer_emulate(L, x, w, scale, shift, out_hw=None):
    """The layer in the kernels' number formats: fp32 accumulation, fp32 multiply, add and activation."""
    out_hw = _out_hw(L, x, out_hw)
    acc = _conv(L, x.to(torch.float32), w.to(torch.float32), out_hw)
    sh = shift.to(torch.float32)[None, :, None, None]
    if L.name == "deconv6":
        return torch.sigmoid(acc + sh)
    pre = acc * scale.to(torch.float32)[None, :, None, None] + sh
    return F.relu(pre) if L.up else F.leaky_relu(pre, LEAKY_SLOPE)


def emulate(state, mix):
    """Free-running fp32 network: {layer: output}."""
    fold, w = fold_scale_shift(state), weights(state)
    hw = level_sizes(*mix.shape[-2:])
    outs = OrderedDict()
    for L in LAYERS:
        outs[L.name] = layer_emulate(L, layer_input(L, mix, outs), w[L.name], *fold[L.name], hw[L.lout])
    return outs


# ---- the cases tests/test_gpu_eval_layers.py runs ---------------------------------------------------------------------------
# key, shapes (B, H, W), planner switches, kernel-name fragments the plan of the (first) shape must show (tests assert them: a
# planner change cannot quietly empty a case), what the case is there for
Case = namedtuple("Case", "key shapes switches must reaches")
PLAIN = (("CONV_WINDOW", 0), ("CONV_GWINDOW", 0), ("CONV_SKIP", 0), ("CONV_C1_TILED", 0))
FORCED = (("CONV_WINDOW", 2), ("CONV_GWINDOW", 2), ("CONV_SKIP", 2), ("CONV_C1_TILED", 2))
CASES = (
    Case("small", ((2, 70, 50),), (), ("conv_gemm_kernel<0, ", "conv_gemm_kernel<1, ", "split-K", "conv_c1_kernel<16>", "deconv_to1_kernel<32>"),
         "all-GEMM eval plan, ragged at every level, eval K-splits"),
    Case("collapse", ((3, 31, 17), (1, 1, 1)), (), ("conv_gemm_kernel<0, ", "conv_gemm_kernel<1, ", "split-K"),
         "levels that collapse to 1x1: every tap but the centre is padding"),
    Case("odd_forced", ((3, 130, 68),), FORCED,
         ("gather_window_kernel", "parity_window_kernel<128, 64, 1, 2", "parity_window_kernel<64, 64, 1, 1", "conv_gemm_kernel<0, skip",
          "conv_gemm_kernel<1, skip", "conv_c1_tiled_kernel<16>"),
         "gather_window, parity_window with split channel halves, tap-skipping GEMMs, tiled conv1, all with the eval epilogue; 2H "
         "and 2H - 1 in both dimensions"),
    Case("odd_window_joint", ((3, 130, 68),), (("CONV_WINDOW", 3), ("CONV_GWINDOW", 2)),
         ("gather_window_kernel", "parity_window_kernel<128, 64, 2, 2", "parity_window_kernel<64, 64, 1, 1"),
         "the window kernel with both channel halves in one block"),
    Case("odd_plain", ((3, 130, 68),), PLAIN, ("conv_gemm_kernel<0, generic", "conv_gemm_kernel<1, generic", "conv_gemm_kernel<1, 256, 32",
                                               "conv_gemm_kernel<1, 256, 16", "conv_gemm_kernel<0, 256, 32", "conv_c1_kernel<16>"),
         "the generic GEMM and thread-per-pixel forms of every layer"),
    Case("b64_uniform", ((64, 32, 8),), (("CONV_KSPLIT", 1),), ("conv_gemm_kernel<0, uniform", "conv_gemm_kernel<1, uniform"),
         "position-uniform kernels with the eval epilogue, 1x1 images at levels 5 and 6"),
    Case("b16_tile", ((16, 512, 128),), (),
         ("conv3=conv_gemm_kernel<0, 64, 64, ",         # N = 64 at Mmax = 16384: the inference-only 64x64 rule (training: 128x64)
          "conv4=conv_gemm_kernel<0, 64, 64, ",         # narrow N = 128 below 8192 rows: no 64x128 tile
          "deconv2=conv_gemm_kernel<1, 64, 64, ",       # narrow parity N = 128 below 2048 rows
          "conv5=conv_gemm_kernel<0, 64, 64, ",         # no 64x128 conv5 tile
          "gather_window_kernel", "parity_window_kernel<128, 64, 1, 2", "parity_window_kernel<64, 64, 1, 1", "split-K"),
         "the plan bench.py's eval leg and a real song run: every inference-only tile and split rule"),
    Case("b4096_conv5", ((4096, 1, 1),), (),
         ("conv5=conv_gemm_kernel<0, 64, 64, 2, 2, true, true, ", "conv4=conv_gemm_kernel<0, 64, 64, 2, 2, true, true, ", "split-K"),
         "the smallest shape the training call's 64x128 conv5 tile is planned at (narrow level, 4096 rows): the eval call keeps "
         "64x64 (at batch 16 both kinds plan 64x64, so b16_tile cannot tell); position-uniform tiles with K-splits"),
    Case("b16_direct", ((16, 512, 128),), (("CONV_WINDOW", 0),), ("deconv5=conv_direct_kernel<1, 4, 1>", "deconv4=conv_direct_kernel<1, 4, 2>"),
         "conv_direct_kernel<1, 4, 1> for deconv5 and <1, 4, 2> for deconv4 (Mmax = 16384 is their threshold)"),
)
BY_KEY = {c.key: c for c in CASES}


def describe_plan(lib, L, B, H, W, switches=()):
    """(kernel name, K-split) of layer L in a (B, H, W) fp32 eval forward under the planner switches now set: svs_describe_plan
    kinds 5 / 6 for conv2 .. deconv5; conv1 and deconv6 have no planner entry -- conv1 follows CONV_C1_TILED alone
    (special.hip: svs_conv_c1_run), deconv6 has one kernel."""
    import ctypes
    if L.name == "conv1":
        return ("conv_c1_tiled_kernel<16>" if dict(switches).get("CONV_C1_TILED", -1) == 2 else "conv_c1_kernel<16>"), 1
    if L.name == "deconv6":
        return "deconv_to1_kernel<32>", 1
    hw = level_sizes(H, W)
    buf = ctypes.create_string_buffer(160)
    ks = lib.svs_describe_plan(6 if L.up else 5, B, hw[L.lin][0], hw[L.lin][1], L.C, hw[L.lout][0], hw[L.lout][1], L.N, buf, 160)
    assert ks >= 1, (L.name, ks)
    return buf.value.decode(), ks


def plan_fragments(plans):
    """The set of name fragments Case.must is checked against, from {layer: (kernel name, K-split)}: every full name, every
    name prefix "kernel<a, b, ..." at an argument boundary, both also as "layer=...", "split-K" when any layer is split, and for
    conv_gemm_kernel<mode, BM, BN, WM, WN, uniform, skip, split, ahead> its form as "conv_gemm_kernel<mode, uniform | skip |
    generic" (skip: tap skipping without the position-uniform form)."""
    seen = set()
    for layer, (full, ks) in plans.items():
        frags = {full}
        if "<" in full:
            stem, args = full[:full.index("<") + 1], full[full.index("<") + 1:-1].split(", ")
            frags |= {stem + ", ".join(args[:i]) + (", " if i < len(args) else ">") for i in range(1, len(args) + 1)}
            frags |= {stem + ", ".join(args[:i]) for i in range(1, len(args))}
            if full.startswith("conv_gemm_kernel<"):
                frags.add(f"{stem}{args[0]}, " + ("uniform" if args[5] == "true" else "skip" if args[6] == "true" else "generic"))
        if ks > 1:
            frags.add("split-K")
        seen |= frags | {f"{layer}={f}" for f in frags}
    return seen
