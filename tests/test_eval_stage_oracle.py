"""CPU suite: oracle/eval_stage_oracle.py tried on itself, without a GPU.  The teacher-forced fp64 reference and the derived
bound (a) accept a free-running fp32 CPU network at every layer of every shape tests/test_gpu_eval_layers.py runs, (b) reject
one zeroed tap, one rotated tap row, one exchanged channel pair and a dropped border row of the input at each of the twelve
layers, (c) give inf for an unwritten element, (d) see live outputs at every case shape; and svs_describe_plan kinds 5 / 6
name, for every case, the kernels the case is there for."""
import functools
import importlib.util
import os
import subprocess

import pytest
import torch

from oracle import eval_stage_oracle as eo
from oracle import unet_oracle as uo
from svs_unet_pytorch_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = sorted({s for c in eo.CASES for s in c.shapes})
# the batch-16 production tile is run on images 0 and 15 (an image's emulation does not depend on the batch it is part of);
# every other case shape whole
WHOLE = 300000


@functools.lru_cache(maxsize=None)
def network():
    state = uo.to_torch_state(synth.closed_form_state())
    return state, eo.fold_scale_shift(state), eo.weights(state)


@functools.lru_cache(maxsize=None)
def emulated(B, H, W):
    """Free-running fp32 emulation of a (B, H, W) case batch and every layer's reference on the emulation's own input of that
    layer: {layer: (input, output, r, S)}.  Computed once per shape, read-only."""
    state, fold, w = network()
    images = range(B) if B * H * W <= WHOLE else (0, B - 1)
    mix = eo.case_input(H, W, images)
    outs = eo.emulate(state, mix)
    hw = eo.level_sizes(H, W)
    res = {}
    for L in eo.LAYERS:
        x = eo.layer_input(L, mix, outs)
        res[L.name] = (x, outs[L.name]) + eo.layer_reference(L, x, w[L.name], *fold[L.name], hw[L.lout])
    return res


@pytest.mark.parametrize("shape", SHAPES)
def test_emulation_satisfies_the_bound_at_every_layer(shape):
    """Observed worst error / bound: 0.064 (conv1, K = 25) down to 1e-4 (conv5, conv6): a worst-case bound over K terms against
    rounding errors that mostly cancel.  The bound has no slack added for this to pass (derivation: the oracle's docstring)."""
    for L in eo.LAYERS:
        _, out, r, S = emulated(*shape)[L.name]
        ratio = eo.worst_ratio(L, out, r, S)
        print(f"{shape} {L.name}: max err / bound {ratio:.4f}")
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


def _weight_mutations(L, x, w, r):
    """Three changed copies of the weights, each built so that it cannot be a no-op at this size (as tests/test_bf16_oracle.py
    builds them): at the output element the layer is most sensitive at (largest r; for the mask, r nearest 1/2) the tap that
    contributes most is zeroed, that tap's row is rotated by one, and the two input channels whose exchange moves that element
    most are swapped at that tap (conv1 has one input channel: the tap is exchanged with the output channel that differs most)."""
    score = r * (1 - r) if L.name == "deconv6" else r
    b, n, oh, ow = [int(i) for i in torch.unravel_index(torch.argmax(score), r.shape)]
    wt = w.transpose(0, 1) if L.up else w                       # (N, C, 5, 5) either way (a view)
    src = _sources(L, oh, ow, x.shape[-2], x.shape[-1])
    contrib = [float((wt[n, :, kh, kw].double() * x[b, :, ih, iw].double()).sum()) for kh, kw, ih, iw in src]
    kh, kw, ih, iw = src[max(range(len(src)), key=lambda i: abs(contrib[i]))]
    out = {}
    m = w.clone()
    m[:, :, kh, kw] = 0
    out["tap zeroed"] = m
    m = w.clone()
    m[:, :, kh, :] = torch.roll(w[:, :, kh, :], 1, dims=-1)
    out["tap row rotated"] = m
    m = w.clone()
    mt = m.transpose(0, 1) if L.up else m
    if L.C == 1:
        n2 = int(torch.argmax((wt[:, 0, kh, kw] - wt[n, 0, kh, kw]).abs()))
        mt[n, 0, kh, kw], mt[n2, 0, kh, kw] = wt[n2, 0, kh, kw], wt[n, 0, kh, kw]
    else:
        wv, xv = wt[n, :, kh, kw].double(), x[b, :, ih, iw].double()
        move = ((wv[:, None] - wv[None, :]) * (xv[:, None] - xv[None, :])).abs()
        a, c = [int(i) for i in torch.unravel_index(torch.argmax(move), move.shape)]
        assert a != c
        mt[:, a, kh, kw], mt[:, c, kh, kw] = wt[:, c, kh, kw], wt[:, a, kh, kw]
    out["two channels swapped at a tap"] = m
    return out


_smallest = {}


@pytest.mark.parametrize("layer", [L.name for L in eo.LAYERS])
def test_comparator_rejects_a_changed_layer(layer):
    """A test that cannot fail checks nothing: with one tap zeroed, one tap row rotated, two input channels exchanged at one
    tap, or the first or the last row of the input taken for padding (what a wrong border predicate does), the layer's output
    must leave the bound -- at each of the twelve layers.  The smallest ratio any mutation reaches is how strong the gate is; it
    is printed (observed: 16.3, deconv2 with two of its 512 input channels exchanged at one tap; a zeroed tap is at least 66,
    a rotated tap row 98, a dropped border row 89 times the bound, conv6 each time; the level-1 layers are rejected by 1e3 ..
    1e5)."""
    L = eo.BY_NAME[layer]
    _, fold, w = network()
    B, H, W = 2, 70, 50
    x, out, r, S = emulated(B, H, W)[layer]
    assert eo.worst_ratio(L, out, r, S) <= 1.0
    out_hw = eo.level_sizes(H, W)[L.lout]
    got = {what: eo.layer_emulate(L, x, wm, *fold[layer], out_hw) for what, wm in _weight_mutations(L, x, w[layer], r).items()}
    for what, row in (("first input row dropped", 0), ("last input row dropped", x.shape[-2] - 1)):
        xm = x.clone()
        xm[:, :, row, :] = 0
        got[what] = eo.layer_emulate(L, xm, w[layer], *fold[layer], out_hw)
    for what, g in got.items():
        ratio = eo.worst_ratio(L, g, r, S)
        print(f"{layer}, {what}: max err / bound {ratio:.1f}")
        assert ratio > 1.0, (layer, what, ratio)
        if ratio < _smallest.get("ratio", float("inf")):
            _smallest.update(ratio=ratio, what=f"{layer}, {what}")
    print(f"smallest ratio of a rejected mutation so far: {_smallest['ratio']:.1f} ({_smallest['what']})")


def test_comparator_rejects_unwritten_output():
    for layer, at in (("deconv6", (1, 0, 69, 49)), ("conv4", (0, 127, 0, 0)), ("deconv2", (1, 5, 4, 3))):
        _, out, r, S = emulated(2, 70, 50)[layer]
        got = out.clone()
        got[at] = float("nan")
        assert eo.worst_ratio(eo.BY_NAME[layer], got, r, S) == float("inf")
        got[at] = float("inf")
        assert eo.worst_ratio(layer, got, r, S) == float("inf")


@pytest.mark.parametrize("shape", SHAPES)
def test_every_layer_is_live_at_the_case_shapes(shape):
    """The condition the GPU test states for its references (eval_stage_oracle.MIN_LIVE): a ReLU layer that is all zero, or a
    saturated mask, would pass any comparison.  The LeakyReLU layers are non-zero everywhere.  Observed with the closed-form
    checkpoint and the case inputs: 37-57 % non-zero per decoder layer, 100 % of the mask inside (0.01, 0.99)."""
    for L in eo.LAYERS:
        live = eo.live_share(L, emulated(*shape)[L.name][2])
        print(f"{shape} {L.name}: live share {live:.3f}")
        assert live >= (eo.MIN_LIVE if L.up else 0.999), (shape, L.name, live)


def test_plans_name_the_kernels_each_case_is_there_for(tune, tmp_path):
    """Host arithmetic only (svs_describe_plan kinds 5 / 6): every kernel an eval layer of a case launches is a kernel of the
    built library, and every case's plan shows the name fragments the case exists for."""
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
    for case in eo.CASES:
        for name, value in case.switches:
            tune(name, value)
        for i, shape in enumerate(case.shapes):
            plans = {L.name: eo.describe_plan(lib, L, *shape, case.switches) for L in eo.LAYERS}
            for layer, (full, ks) in plans.items():
                assert full in kernels and ks >= 1, (case.key, shape, layer, full)
            if i == 0:
                missing = [m for m in case.must if m not in eo.plan_fragments(plans)]
                assert not missing, (case.key, missing, plans)
        tune("*", -1)
