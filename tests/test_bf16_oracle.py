"""CPU suite: oracle/bf16_oracle.py tried on itself, without a GPU.  The teacher-forced fp64 reference and the derived bound
(a) accept a free-running CPU network of the kernels' number formats at every layer, (b) reject one changed tap, tap row or
channel pair at each of the twelve layers, (c) see live (not all-zero, not saturated) outputs at every shape the GPU test
runs; and svs_describe_plan names, for every (case, layer) of tests/test_gpu_bf16_layers.py, the kernel the case is there for."""
import ctypes
import functools
import importlib.util
import os
import subprocess

import pytest
import torch

from oracle import bf16_oracle as bo
from oracle import unet_oracle as uo
from svs_unet_pytorch_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def network():
    state = uo.to_torch_state(synth.closed_form_state())
    fold = bo.fold_scale_shift(state)
    return state, fold, bo.fold_weights(state, fold)


@functools.lru_cache(maxsize=None)
def emulated(B, H, W):
    """Free-running emulation of the covered images of a (B, H, W) batch, and every layer's reference on the emulation's own
    input of that layer: {layer: (input, output, r, S)}.  Computed once per shape, read-only."""
    state, fold, w = network()
    mix = bo.case_input(H, W, bo.covered_images(B, H, W))
    outs = bo.emulate(state, mix)
    hw = bo.level_sizes(H, W)
    res = {}
    for L in bo.LAYERS:
        x = bo.layer_input(L, mix, outs)
        res[L.name] = (x, outs[L.name]) + bo.layer_reference(L, x, w[L.name], fold[L.name][1], hw[L.lout])
    return res


@pytest.mark.parametrize("shape", [(2, 70, 50), (1, 512, 128)])
def test_emulation_satisfies_the_bound_at_every_layer(shape):
    """Observed worst error / bound: 0.99 (conv1: half a bf16 ulp just above a power of two) down to 0.41 (conv6), 0.003 for the
    mask.  The bound has no slack added for this to pass."""
    for L in bo.LAYERS:
        _, out, r, S = emulated(*shape)[L.name]
        ratio = bo.worst_ratio(L, out, r, S)
        print(f"{shape} {L.name}: max err / bound {ratio:.3f}")
        assert ratio <= 1.0, (shape, L.name, ratio)


def _sources(L, oh, ow, H, W):
    """[(kh, kw, ih, iw)]: the taps that reach output pixel (oh, ow) and the input pixel each one reads."""
    out = []
    for kh in range(5):
        for kw in range(5):
            if not L.up:
                ih, iw = 2 * oh - 2 + kh, 2 * ow - 2 + kw
            elif (oh + 2 - kh) % 2 or (ow + 2 - kw) % 2:
                continue
            else:
                ih, iw = (oh + 2 - kh) // 2, (ow + 2 - kw) // 2
            if 0 <= ih < H and 0 <= iw < W:
                out.append((kh, kw, ih, iw))
    return out


def _mutations(L, x, w, r):
    """Three changed copies of the weights, each built so that it cannot be a no-op at this size: the output element the
    layer is most sensitive at (largest r; for the mask, r nearest 1/2) is found, the tap that contributes most to it is
    dropped, that tap's row is rotated by one, and the two input channels whose exchange moves that element most are swapped
    at that tap (conv1 has one input channel: the tap is exchanged with the output channel that differs most)."""
    score = r * (1 - r) if L.name == "deconv6" else r
    b, n, oh, ow = [int(i) for i in torch.unravel_index(torch.argmax(score), r.shape)]
    wt = w.transpose(0, 1) if L.up else w                       # (N, C, 5, 5) either way (a view)
    src = _sources(L, oh, ow, x.shape[-2], x.shape[-1])
    xin = bo.split_hi_lo(x)[0] if L.name == "conv1" else x
    contrib = [float((wt[n, :, kh, kw].double() * xin[b, :, ih, iw].double()).sum()) for kh, kw, ih, iw in src]
    kh, kw, ih, iw = src[max(range(len(src)), key=lambda i: abs(contrib[i]))]
    # (kh, kw) meets data at (b, oh, ow), so dropping it is no no-op; the rotation gives that position its neighbour's weights
    out = {}
    m = w.clone()
    m[:, :, kh, kw] = 0
    out["tap dropped"] = m
    m = w.clone()
    m[:, :, kh, :] = torch.roll(w[:, :, kh, :], 1, dims=-1)
    out["tap row rotated"] = m
    m = w.clone()
    mt = m.transpose(0, 1) if L.up else m
    if L.C == 1:
        n2 = int(torch.argmax((wt[:, 0, kh, kw] - wt[n, 0, kh, kw]).abs()))
        mt[n, 0, kh, kw], mt[n2, 0, kh, kw] = wt[n2, 0, kh, kw], wt[n, 0, kh, kw]
    else:
        wv, xv = wt[n, :, kh, kw].double(), xin[b, :, ih, iw].double()
        move = ((wv[:, None] - wv[None, :]) * (xv[:, None] - xv[None, :])).abs()
        a, c = [int(i) for i in torch.unravel_index(torch.argmax(move), move.shape)]
        assert a != c
        mt[:, a, kh, kw], mt[:, c, kh, kw] = wt[:, c, kh, kw], wt[:, a, kh, kw]
    out["two channels swapped at a tap"] = m
    return out


@pytest.mark.parametrize("layer", [L.name for L in bo.LAYERS])
def test_comparator_rejects_a_changed_layer(layer):
    """A test that cannot fail checks nothing: with one tap dropped, one tap row rotated or two input channels exchanged at
    one tap, the layer's output must leave the bound -- at each of the twelve layers."""
    L = bo.BY_NAME[layer]
    _, fold, w = network()
    B, H, W = 2, 70, 50
    x, out, r, S = emulated(B, H, W)[layer]
    assert bo.worst_ratio(L, out, r, S) <= 1.0
    out_hw = bo.level_sizes(H, W)[L.lout]
    for what, wm in _mutations(L, x, w[layer], r).items():
        assert not torch.equal(wm, w[layer])
        got = bo.layer_emulate(L, x, wm, fold[layer][1], out_hw)
        ratio = bo.worst_ratio(L, got, r, S)
        print(f"{layer}, {what}: max err / bound {ratio:.1f}")
        assert ratio > 1.0, (layer, what, ratio)


def test_comparator_rejects_unwritten_output():
    L = bo.BY_NAME["deconv6"]
    _, out, r, S = emulated(2, 70, 50)["deconv6"]
    got = out.clone()
    got[1, 0, 69, 49] = float("nan")
    assert bo.worst_ratio(L, got, r, S) == float("inf")


@pytest.mark.parametrize("shape", sorted({s for c in bo.CASES for s in c.shapes}))
def test_every_layer_is_live_at_the_test_shapes(shape):
    """A ReLU layer that is all zero, or a saturated mask, would pass any comparison.  Observed: 41-53 % nonzero for the ReLU
    layers, 100 % for the LeakyReLU layers and the mask."""
    for L in bo.LAYERS:
        r = emulated(*shape)[L.name][2]
        if L.name == "deconv6":
            live = float(((r > 0.01) & (r < 0.99)).double().mean())
            assert live >= 0.9, (shape, live)
        else:
            live = float((r != 0).double().mean())
            assert live >= 0.3, (shape, L.name, live)


# case -> the kernel (conv_gemm_bf16_kernel<mode, BM, BN, ...> as "BMxBN", parity_window_bf16_kernel<C, ...> as "window<C>")
# and K-split of conv4, conv5, conv6, deconv1 .. deconv5.  Written down from plan_bf16 by hand: what each case is there for.
PLANS = {
    ("a", (2, 70, 50)): "64x128/6 64x128/12 64x128/25 64x128/8 64x128/8 128x64/4 256x32/2 256x16/1",
    ("b", (3, 31, 17)): "64x128/6 64x128/12 64x128/25 64x128/8 64x128/8 128x64/4 256x32/2 256x16/1",
    ("b", (1, 1, 1)): "64x128/6 64x128/12 64x128/25 64x128/8 64x128/8 128x64/4 256x32/2 256x16/1",
    ("c", (1, 512, 128)): "64x128/6 64x128/12 64x128/25 64x128/8 64x128/8 128x64/4 256x32/2 256x16/1",
    ("d", (130, 66, 126)): "128x128/6 64x128/12 64x128/22 64x128/8 64x128/8 window<256>/1 window<128>/1 window<64>/1",
    ("e", (2100, 16, 32)): "128x128/6 64x128/12 64x128/6 64x128/3 64x128/6 window<256>/1 256x32/2 256x16/1",
    ("f", (260, 72, 136)): "128x128/6 64x128/7 64x128/8 64x128/4 64x128/4 128x64/3 window<128>/1 window<64>/1",
    ("g", (2, 70, 50)): "128x128/6 128x128/12 128x128/25 128x128/8 128x128/8 128x64/4 256x32/2 256x16/1",
    ("h", (2, 70, 50)): "128x64/1 128x64/1 128x64/1 128x64/1 128x64/1 128x64/1 256x32/1 256x16/1",
    ("i", (2, 70, 50)): "64x128/32 64x128/32 64x128/32 64x128/32 64x128/32 128x64/32 256x32/2 256x16/1",
    ("j", (16, 64, 128)): "64x128/6 64x128/12 64x128/25 64x128/8 64x128/8 128x64/4 256x32/2 256x16/1",
}
def test_plans_name_the_kernel_each_case_is_there_for(tune, tmp_path):
    from svs_unet_pytorch_amd import build
    build.build_lib(verbose=False)
    lib = _lib.lib()
    spec = importlib.util.spec_from_file_location("check_isa", os.path.join(ROOT, "tools", "check_isa.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    mangled = []
    for co in isa.device_code_objects(_lib.LIB_PATH, str(tmp_path)):
        syms = subprocess.run([f"{isa.LLVM}/llvm-objdump", "-t", co], capture_output=True, text=True, check=True).stdout
        mangled += [ln.split()[-1] for ln in syms.splitlines() if " F .text" in ln]
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.splitlines()
    kernels = {d.removeprefix("void ").split("(")[0] for d in demangled}
    assert set(bo.WINDOW_KERNELS) <= kernels
    assert {(c.key, s) for c in bo.CASES for s in c.shapes} == set(PLANS)
    for case in bo.CASES:
        for name, value in case.switches:
            tune(name, value)
        for shape in case.shapes:
            got = []
            for name in bo.PLANNED:
                full, short, ks = bo.describe_plan(lib, bo.BY_NAME[name], *shape)
                assert full in kernels, (case.key, name, full)
                got.append(f"{short}/{ks}")
            assert " ".join(got) == PLANS[(case.key, shape)], (case.key, shape)
        tune("*", -1)
    buf = ctypes.create_string_buffer(128)
    assert lib.svs_describe_plan(3, 1, 8, 8, 48, 4, 4, 16, buf, 128) < 0 and b"no bf16 layer" in lib.svs_last_error_string()


def test_tuning_comment_lists_the_switches_that_exist():
    """The comment above svs_tuning_set names exactly the switches of net.hip's table, and the library accepts exactly those."""
    import re
    from svs_unet_pytorch_amd import build
    build.build_lib(verbose=False)
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "svs_hip.h")).read()
    comment = header[:header.index("int svs_tuning_set(")].rsplit("/*", 1)[1]
    listed = set(re.findall(r"\b[A-Z][A-Z0-9]*(?:_[A-Z0-9]+)+\b", comment))
    src = open(os.path.join(ROOT, "svs_unet_pytorch_amd", "csrc", "net.hip")).read()
    table = set(re.findall(r'"([A-Z0-9_]+)"', src[src.index("TUNE_NAMES[SVS_TUNE_COUNT] = {"):].split("};", 1)[0]))
    assert len(table) == 17 and listed == table, listed ^ table
    try:
        for name in table:
            assert lib.svs_tuning_set(name.encode(), 1) == 0, name
        for name in ("BF16_KB", "BF16_CONV3_WINDOW", "BF16_DECONV3_WINDOW", "CONV_PF"):
            assert lib.svs_tuning_set(name.encode(), 1) == -1, name
    finally:
        lib.svs_tuning_set(b"*", -1)
