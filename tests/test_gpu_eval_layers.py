"""Per-layer parity of the fp32 eval network (-m gpu): after svs_unet_forward_eval every layer's output is still in the
workspace (svs_unet_ws_offset(..., 0)).  Each of the twelve layers is checked ELEMENTWISE against oracle/eval_stage_oracle.py's
fp64 reference on the GPU's own input of that layer, under the derived bound of that module (no fitted constant), at the
smallest shapes that reach the forms only the eval call takes: the planner's `inference` tile and K-split rules, and the
folded-BatchNorm epilogue of every kernel writing into the strided and planar concat halves (eval_stage_oracle.CASES).

Zero padding in the conv kernels rests on software pointing an out-of-image element past the buffer descriptor's 2 GiB; a wrong
predicate reads real neighbouring memory.  In front of image 0 and behind image B - 1 that is whatever lies beside the tensor,
in a fresh allocator pool very often zeros -- the right answer.  Here everything beside a tensor is NaN: the mixture lies in
the middle of a NaN-filled buffer, the workspace is filled with an fp32 NaN sentinel and has NaN in front of and behind it, the
mask is NaN before the call, and the library is told exactly the workspace size its own query returns."""
import numpy as np
import pytest
import torch

from oracle import eval_stage_oracle as eo
from oracle import unet_oracle as uo
from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7FC17FC1      # an fp32 NaN no kernel computes: read anywhere, it shows
MARGIN = 65536             # NaN bytes on either side of the prepared blob, the mixture and (in front of) the workspace
GUARD = 4096               # sentinel bytes behind the workspace the library is told about
BLOB_BLOCKS = 12 + 2 * 11 + 1          # weights, scale and shift, deconv6's bias: each block of the blob is 256-byte aligned


def nan_arena(nbytes):
    """(arena of int32 sentinels with MARGIN bytes on either side of `nbytes` bytes, the first int32 index of the middle)."""
    assert nbytes % 4 == 0
    return torch.full(((2 * MARGIN + nbytes) // 4,), SENTINEL, dtype=torch.int32, device=DEV), MARGIN // 4


@pytest.fixture(scope="module")
def net():
    """The closed-form checkpoint prepared once through the C ABI into the middle of a NaN-filled arena; scale / shift bit-exactly
    as svs_unet_prepare_eval folds them (svs_bn_fold on the same device arrays); the fp32 checkpoint weights, unscaled."""
    L = _lib.lib()
    state = synth.closed_form_state()
    model = UNet()
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    model = model.to(DEV).eval()
    stream = _lib.stream_ptr()
    nbytes = int(L.svs_unet_prepared_bytes())
    arena, first = nan_arena(nbytes)
    _lib.check(L.svs_unet_prepare_eval(_lib.ptr(model._flat), _lib.ptr(model._bn_flat), arena.data_ptr() + MARGIN, stream), "svs_unet_prepare_eval")
    st = uo.to_torch_state(state)
    fold = eo.fold_scale_shift(st)
    p, q = model._flat.data_ptr(), model._bn_flat.data_ptr()
    for l, layer in enumerate(eo.LAYERS[:11]):
        out = torch.empty(2, layer.N, dtype=torch.float32, device=DEV)
        po = [p + 4 * L.svs_unet_param_offset(4 * l + i) for i in range(4)]                  # w, bias, gamma, beta
        _lib.check(L.svs_bn_fold(po[2], po[3], q + 4 * L.svs_unet_buffer_offset(l, 0), q + 4 * L.svs_unet_buffer_offset(l, 1), po[1],
                                 1e-5, out[0].data_ptr(), out[1].data_ptr(), layer.N, stream), "svs_bn_fold")
        scale, shift = out.cpu()
        assert (scale - fold[layer.name][0]).abs().max() <= 2e-7 * scale.abs().max()          # the oracle's CPU fold agrees to an fp32 ulp
        fold[layer.name] = (scale, shift)
    torch.cuda.synchronize()
    host = arena.cpu()
    return {"arena": arena, "prepared": arena.data_ptr() + MARGIN, "fold": fold, "weights": eo.weights(st),
            "outside_blob_intact": bool((host[:first] == SENTINEL).all() and (host[first + nbytes // 4:] == SENTINEL).all()),
            "blob_unwritten": int((host[first:first + nbytes // 4] == SENTINEL).sum())}


def test_prepare_eval_writes_its_blob_and_nothing_else(net):
    """svs_unet_prepare_eval into a NaN-filled arena: the 64 KiB on either side of svs_unet_prepared_bytes() are untouched, and
    inside the blob nothing but the alignment padding of its blocks (less than 256 bytes each) is left unwritten."""
    assert net["outside_blob_intact"], "svs_unet_prepare_eval wrote outside its blob"
    assert net["blob_unwritten"] < BLOB_BLOCKS * 64, net["blob_unwritten"]


def run_forward(net, mix):
    """One forward through the C ABI: the mixture in the middle of a NaN buffer, a NaN mask, a sentinel workspace of exactly the
    queried size with sentinels in front of and behind it.  Returns (mask, workspace with its surroundings as int32 on the CPU,
    the first int32 index of the workspace proper, its size in bytes)."""
    L = _lib.lib()
    B, _, H, W = mix.shape
    n = B * H * W
    mix_arena, mfirst = nan_arena(4 * n + (-4 * n) % 16)
    mix_arena[mfirst:mfirst + n] = mix.reshape(-1).view(torch.int32).to(DEV)
    before = mix_arena.clone()
    ws_bytes = int(L.svs_unet_eval_workspace_bytes(B, H, W))               # (after the planner switches: the slabs follow the plan)
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    ws = torch.full(((MARGIN + ws_bytes + GUARD) // 4,), SENTINEL, dtype=torch.int32, device=DEV)
    mask = torch.full((B, 1, H, W), float("nan"), device=DEV)
    _lib.check(L.svs_unet_forward_eval(net["prepared"], mix_arena.data_ptr() + MARGIN, _lib.ptr(mask), B, H, W, ws.data_ptr() + MARGIN,
                                       ws_bytes, _lib.stream_ptr()), "svs_unet_forward_eval")
    torch.cuda.synchronize()
    assert torch.equal(mix_arena, before), "the mixture or its surroundings changed"
    return mask.cpu(), ws.cpu(), MARGIN // 4, ws_bytes


def layer_outputs(ws, first, B, H, W, images):
    """{layer: (len(images), N, h, w) fp32} of conv1 .. deconv5 from the workspace (level 1: two dense planes, decoder first;
    levels 2 .. 5: [decoder half | skip half] inside every pixel), and the byte spans of the named buffers."""
    L = _lib.lib()
    hw = eo.level_sizes(H, W)
    outs, spans = {}, []
    for k in range(1, 7):
        name = "c6" if k == 6 else f"cat{k}"
        off = L.svs_unet_ws_offset(name.encode(), B, H, W, 0)
        assert off >= 0 and off % 256 == 0, (name, off)
        h, w = hw[k]
        n = B * h * w * (eo.CH[k] if k == 6 else 2 * eo.CH[k])
        spans.append((off, off + 4 * n, name))
        buf = ws[first + off // 4:first + off // 4 + n]
        assert not (buf == SENTINEL).any(), f"{name}: elements no kernel wrote"
        t = buf.view(torch.float32)
        if k == 6:
            halves = (None, t.view(B, h, w, eo.CH[6]))
        elif k == 1:
            halves = tuple(t.view(2, B, h, w, 16))
        else:
            t = t.view(B, h, w, 2 * eo.CH[k])
            halves = (t[..., :eo.CH[k]], t[..., eo.CH[k]:])
        nchw = [None if v is None else v[images].permute(0, 3, 1, 2).contiguous() for v in halves]
        outs[f"conv{k}"] = nchw[1]
        if k < 6:
            outs[f"deconv{6 - k}"] = nchw[0]
    return outs, spans


def check_case(net, report, case, B, H, W, assert_plan):
    L = _lib.lib()
    plans = {layer.name: eo.describe_plan(L, layer, B, H, W, case.switches) for layer in eo.LAYERS}
    if assert_plan:
        missing = [m for m in case.must if m not in eo.plan_fragments(plans)]
        assert not missing, (missing, plans)            # a case whose kernels no layer took proves nothing
    images = eo.covered_images(B, H, W)
    print(f"{case.key} B{B} {H}x{W}: reference for images {images if len(images) < B else 'all'}")
    mix = eo.case_input(H, W, range(B)).float()
    mask, ws, first, ws_bytes = run_forward(net, mix)
    check_outputs(net, report, case, plans, mix, images, mask, ws, first, ws_bytes)


def check_outputs(net, report, case, plans, mix, images, mask, ws, first, ws_bytes):
    """What one forward left behind -- mask, workspace and its surroundings -- against the sentinels and the oracle."""
    B, _, H, W = mix.shape
    assert torch.isfinite(mask).all(), "mask pixels no kernel wrote"
    outs, spans = layer_outputs(ws, first, B, H, W, images)
    outs["deconv6"] = mask[images]
    # nothing outside the buffers: the arena padding after each one and the bytes on either side of the workspace
    gaps = [(end, -(-end // 256) * 256, f"padding after {name}") for _, end, name in spans]
    gaps += [(-MARGIN, 0, "in front of the workspace"), (ws_bytes, ws_bytes + GUARD, "past the workspace")]
    for a, b, what in gaps:
        assert (ws[first + a // 4:first + b // 4] == SENTINEL).all(), f"{what} was written"
    hw = eo.level_sizes(H, W)
    tag = "".join(f" {n}={v}" for n, v in case.switches)
    bad = []
    for layer in eo.LAYERS:
        x = eo.layer_input(layer, mix[images], outs)
        r, S = eo.layer_reference(layer, x, net["weights"][layer.name], *net["fold"][layer.name], hw[layer.lout])
        live = eo.live_share(layer, r)
        assert live >= (eo.MIN_LIVE if layer.up else 0.999), (layer.name, live)          # tests/test_eval_stage_oracle.py: 37 % and up
        ratio = eo.worst_ratio(layer, outs[layer.name], r, S)
        kernel, ks = plans[layer.name]
        label = kernel if ks == 1 else f"{kernel} K/{ks}"
        print(f"{layer.name:8s} [{label}] max err / bound {ratio:.4f}")
        if not report(f"eval layer {layer.name} [{label}] {case.key} B{B} {H}x{W}{tag}", ratio, 1.0):
            bad.append((layer.name, label, ratio))
    assert not bad, bad


@pytest.mark.parametrize("case", eo.CASES, ids=[c.key for c in eo.CASES])
def test_eval_layers_against_oracle(net, report, tune, case):
    """Every layer of every case: max over the elements of |got - r| / ((K + 2) 2^-23 S + 2^-23 |r|) <= 1 (mask: 0.25 E + 1e-5,
    E = (K + 2) 2^-23 S); see oracle/eval_stage_oracle.py for the derivation and its CASES for what each case reaches and the
    kernel names its plan must show."""
    for name, value in case.switches:           # before the workspace query: the split-K slabs follow the plan
        tune(name, value)
    for i, (B, H, W) in enumerate(case.shapes):
        check_case(net, report, case, B, H, W, assert_plan=i == 0)
