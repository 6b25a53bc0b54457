"""Per-layer parity of the bf16 eval network (-m gpu): after svs_unet_forward_eval_bf16 every layer's bf16 output is still in
the workspace (svs_unet_ws_offset(..., 2)).  Each of the twelve layers is checked ELEMENTWISE against oracle/bf16_oracle.py's
fp64 reference on the GPU's own bf16 input of that layer, under the derived bound of that module (no fitted constant), at the
smallest shapes that reach every kernel, tile shape, K-split and persistent-grid wrap of csrc/gemm_bf16.hip.  The mask-level
gates (test_eval_forward_bf16 and the property tests) cannot see a wrong tap between conv3 and deconv4; these can."""
import numpy as np
import pytest
import torch

from oracle import bf16_oracle as bo
from oracle import unet_oracle as uo
from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7FC1          # a bf16 NaN (and, doubled, an fp32 NaN) that no kernel computes: read anywhere, it shows
GUARD = 4096               # bytes allocated past the workspace the library is told about


@pytest.fixture(scope="module")
def net():
    """The closed-form checkpoint prepared once through the C ABI; scale / shift bit-exactly as svs_unet_prepare_eval folds
    them (svs_bn_fold on the same device arrays), the bf16 weights from the oracle's restatement of the packing kernels."""
    L = _lib.lib()
    state = synth.closed_form_state()
    model = UNet()
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    model = model.to(DEV).eval()
    stream = _lib.stream_ptr()
    prepared = torch.empty(int(L.svs_unet_prepared_bytes()), dtype=torch.uint8, device=DEV)
    _lib.check(L.svs_unet_prepare_eval(_lib.ptr(model._flat), _lib.ptr(model._bn_flat), _lib.ptr(prepared), stream), "svs_unet_prepare_eval")
    prepared_bf16 = torch.empty(int(L.svs_unet_prepared_bf16_bytes()), dtype=torch.uint8, device=DEV)
    _lib.check(L.svs_unet_prepare_eval_bf16(_lib.ptr(prepared), _lib.ptr(prepared_bf16), stream), "svs_unet_prepare_eval_bf16")
    st = uo.to_torch_state(state)
    fold = bo.fold_scale_shift(st)
    p, q = model._flat.data_ptr(), model._bn_flat.data_ptr()
    for l, layer in enumerate(bo.LAYERS[:11]):
        out = torch.empty(2, layer.N, dtype=torch.float32, device=DEV)
        po = [p + 4 * L.svs_unet_param_offset(4 * l + i) for i in range(4)]                  # w, bias, gamma, beta
        _lib.check(L.svs_bn_fold(po[2], po[3], q + 4 * L.svs_unet_buffer_offset(l, 0), q + 4 * L.svs_unet_buffer_offset(l, 1), po[1],
                                 1e-5, out[0].data_ptr(), out[1].data_ptr(), layer.N, stream), "svs_bn_fold")
        scale, shift = out.cpu()
        assert (scale - fold[layer.name][0]).abs().max() <= 2e-7 * scale.abs().max()          # the oracle's CPU fold agrees to an fp32 ulp
        fold[layer.name] = (scale, shift)
    torch.cuda.synchronize()
    return {"model": model, "prepared_bf16": prepared_bf16, "fold": fold, "weights": bo.fold_weights(st, fold)}


def run_forward(net, mix):
    """One forward through the C ABI into a sentinel-filled workspace: (mask, workspace as int16 on the CPU, its size)."""
    L = _lib.lib()
    B, _, H, W = mix.shape
    ws_bytes = int(L.svs_unet_eval_bf16_workspace_bytes(B, H, W))          # (after the planner switches: the slabs follow the plan)
    ws = torch.full(((ws_bytes + GUARD) // 2,), SENTINEL, dtype=torch.int16, device=DEV)
    x = mix.to(DEV)
    mask = torch.full_like(x, float("nan"))
    _lib.check(L.svs_unet_forward_eval_bf16(_lib.ptr(net["prepared_bf16"]), _lib.ptr(x), _lib.ptr(mask), B, H, W, _lib.ptr(ws), ws_bytes,
                                            _lib.stream_ptr()), "svs_unet_forward_eval_bf16")
    torch.cuda.synchronize()
    return mask.cpu(), ws.cpu(), ws_bytes


def layer_outputs(ws, B, H, W, images):
    """{layer: (len(images), N, h, w) fp32} of conv1 .. deconv5 from the workspace, and the byte spans of the named buffers."""
    L = _lib.lib()
    hw = bo.level_sizes(H, W)
    outs, spans = {}, []
    for k in range(1, 7):
        name = "c6" if k == 6 else f"cat{k}"
        off = L.svs_unet_ws_offset(name.encode(), B, H, W, 2)
        assert off >= 0 and off % 256 == 0, (name, off)
        h, w = hw[k]
        n = B * h * w * (bo.CH[k] if k == 6 else 2 * bo.CH[k])
        spans.append((off, off + 2 * n, name))
        buf = ws[off // 2:off // 2 + n]
        assert not (buf == SENTINEL).any(), f"{name}: elements no kernel wrote"
        t = buf.view(torch.bfloat16)
        if k == 6:
            halves = (None, t.view(B, h, w, bo.CH[6]))
        elif k == 1:                                      # two planes, decoder first
            halves = tuple(t.view(2, B, h, w, 16))
        else:                                             # [decoder half | skip half] in every pixel
            t = t.view(B, h, w, 2 * bo.CH[k])
            halves = (t[..., :bo.CH[k]], t[..., bo.CH[k]:])
        nchw = [None if v is None else v[images].float().permute(0, 3, 1, 2).contiguous() for v in halves]
        outs[f"conv{k}"] = nchw[1]
        if k < 6:
            outs[f"deconv{6 - k}"] = nchw[0]
    return outs, spans


def check_case(net, report, B, H, W, switches):
    L = _lib.lib()
    images = bo.covered_images(B, H, W)
    print(f"B{B} {H}x{W}: reference for images {images if len(images) < B else 'all'}")
    mix = bo.case_input(H, W, range(B))
    mask, ws, ws_bytes = run_forward(net, mix)
    assert torch.isfinite(mask).all(), "mask pixels no kernel wrote"
    outs, spans = layer_outputs(ws, B, H, W, images)
    outs["deconv6"] = mask[images]
    # nothing outside the buffers: the arena padding after each one, the spare tail of the scratch and the bytes past the workspace
    gaps = [(end, -(-end // 256) * 256, f"padding after {name}") for _, end, name in spans]
    gaps += [(ws_bytes - 256, ws_bytes, "tail of the scratch"), (ws_bytes, ws_bytes + GUARD, "past the workspace")]
    for a, b, what in gaps:
        assert (ws[a // 2:b // 2] == SENTINEL).all(), f"{what} was written"
    hw = bo.level_sizes(H, W)
    label = {"conv1": "conv1_mfma", "conv2": "conv2_window", "conv3": "conv3_window", "deconv6": "deconv6_mfma"}
    for name in bo.PLANNED:
        _, short, ks = bo.describe_plan(L, bo.BY_NAME[name], B, H, W)
        label[name] = short if ks == 1 else f"{short} K/{ks}"
    tag = "".join(f" {n}={v}" for n, v in switches)
    bad = []
    for layer in bo.LAYERS:
        x = bo.layer_input(layer, mix[images], outs)
        r, S = bo.layer_reference(layer, x, net["weights"][layer.name], net["fold"][layer.name][1], hw[layer.lout])
        ratio = bo.worst_ratio(layer, outs[layer.name], r, S)
        print(f"{layer.name:8s} [{label[layer.name]}] max err / bound {ratio:.3f}")
        if not report(f"bf16 layer {layer.name} [{label[layer.name]}] B{B} {H}x{W}{tag}", ratio, 1.0):
            bad.append((layer.name, ratio))
    assert not bad, bad


@pytest.mark.parametrize("case", bo.CASES, ids=[c.key for c in bo.CASES])
def test_bf16_layers_against_oracle(net, report, tune, case):
    """Every layer of every case: max over the elements of |got - r| / (2^-8 |r| + (1 + 2^-8) E) <= 1 (mask: 0.25 E + 1e-5),
    E = K 2^-23 S; see oracle/bf16_oracle.py for the derivation and its CASES for what each case reaches."""
    for name, value in case.switches:           # before the workspace query: the split-K slabs follow the plan
        tune(name, value)
    for B, H, W in case.shapes:
        check_case(net, report, B, H, W, case.switches)
