"""The LDS-window parity kernel's two epilogues (-m gpu): 16-byte stores on an aligned output view, 4-byte stores on a
misaligned one, both against fp64 conv_transpose2d; the BatchNorm partials the kernel leaves, in a whole train step whose
window layers see ragged tiles; and the names svs_describe_plan gives the four batch-64 launches."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from svs_unet_pytorch_amd import _lib, synth
from test_gpu_ops import DEV, L, S, nchw, nhwc, pack_parity, relerr, rnd, ws_guard, ws_tensor          # noqa: F401  (ws_guard is an autouse fixture)
from test_gpu_unet import _grads_by_name, make_model

pytestmark = pytest.mark.gpu

SHAPES = [
    # B, H, W, C, N, Ho, Wo
    (1, 3, 5, 32, 16, 6, 10),           # smaller than a tile
    (1, 9, 18, 64, 32, 17, 35),         # ragged tile, odd output
    (2, 16, 16, 128, 32, 32, 32),       # two phases
]
SENTINEL = -3.0


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs of a shape and its fp64 references (plain / bias + scale + shift + LeakyReLU(0.2) / accumulated), computed once."""
    B, H, W, C, N, Ho, Wo = shape
    x, w = rnd((B, C, H, W), 61), rnd((C, N, 5, 5), 62, -0.1, 0.1)
    b, sc, sh = rnd((N,), 63), rnd((N,), 64, 0.5, 1.5), rnd((N,), 65)
    base = rnd((B, Ho, Wo, N), 66)
    op = (Ho - (2 * H - 1), Wo - (2 * W - 1))
    plain = F.conv_transpose2d(x.double(), w.double(), None, stride=2, padding=2, output_padding=op)
    epi = F.leaky_relu((plain + b.double()[None, :, None, None]) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None], 0.2)
    want = {"plain": plain, "epilogue": epi, "accumulate": plain + nchw(base).double()}
    dev = {"x": nhwc(x).to(DEV), "wp": pack_parity(w), "b": b.to(DEV), "sc": sc.to(DEV), "sh": sh.to(DEV), "base": base.to(DEV)}
    return want, dev


@pytest.mark.parametrize("variant", ["plain", "epilogue", "accumulate"])
@pytest.mark.parametrize("force", [2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_both_epilogues_against_fp64(shape, force, variant, report, tune):
    B, H, W, C, N, Ho, Wo = shape
    tune("CONV_WINDOW", force)
    want, d = case(shape)
    P = B * Ho * Wo
    bias, scale, shift, slope = (d["b"], d["sc"], d["sh"], 0.2) if variant == "epilogue" else (None, None, None, 0.0)
    acc = 1 if variant == "accumulate" else 0
    ptr = lambda t: t.data_ptr() if t is not None else None                                         # noqa: E731
    ws = ws_tensor(64)
    for align, ldy, lead in (("aligned", 2 * N, 0), ("misaligned", 2 * N + 1, 1)):
        buf = torch.full((lead + P * ldy,), SENTINEL, device=DEV)
        rows = buf[lead:].view(P, ldy)
        rows[:, :N] = d["base"].view(P, N) if acc else float("nan")                                  # every element must be written
        assert (buf.data_ptr() + 4 * lead) % 16 == 4 * lead
        _lib.check(L().svs_dec_block_fwd(d["x"].data_ptr(), C, B, H, W, C, d["wp"].data_ptr(), ptr(bias), ptr(scale), ptr(shift), slope,
                                         buf.data_ptr() + 4 * lead, ldy, Ho, Wo, N, acc, ws.data_ptr(), ws.numel(), S()))
        torch.cuda.synchronize()
        assert torch.all(rows[:, N:] == SENTINEL) and torch.all(buf[:lead] == SENTINEL), f"{align}: wrote outside its channel slice"
        got = rows[:, :N].reshape(B, Ho, Wo, N)
        assert not torch.isnan(got).any(), f"{align}: output elements left unwritten"
        e = relerr(nchw(got), want[variant])
        print(f"window {align} {variant} force {force} {shape}: relerr {e:.3e}")
        assert report(f"window {align} {variant} f{force} B{B} {H}x{W}->{Ho}x{Wo} C{C} N{N}", e, 2e-5)


def test_statistics_on_ragged_window_layers(report, tune):
    """One train forward + backward at B = 3 on an 80 x 48 tile with the window kernel forced: its partial sums against the
    separate statistics pass (TRAIN_UNFUSED), and twice in a row bit for bit."""
    B, H, W = 3, 80, 48
    mix_np, voc_np = synth.tiles(B, H, W, first_tile=900)
    mix, voc = torch.from_numpy(mix_np).to(DEV), torch.from_numpy(voc_np).to(DEV)
    masks = [torch.from_numpy(m) for m in synth.dropout_masks(B, seed=23, step=0)]
    buf = ctypes.create_string_buffer(128)

    def run():
        m = make_model(trained_stats=False).train()
        m.set_dropout_masks(masks)
        m.optim.zero_grad()
        loss = m.fwd_bwd(mix, voc, loss_scale=166.66)
        torch.cuda.synchronize()
        return loss.item(), m._gflat.clone(), m._bn_flat.clone(), _grads_by_name(m)

    tune("CONV_WINDOW", 2)
    L().svs_describe_plan(1, B, H // 4, W // 4, 64, H // 2, W // 2, 16, buf, 128)                    # deconv5 forward
    assert buf.value.decode().startswith("parity_window_kernel<"), buf.value
    loss_a, g_a, bn_a, named_a = run()
    loss_b, g_b, bn_b, _ = run()
    assert loss_a == loss_b and torch.equal(g_a, g_b) and torch.equal(bn_a, bn_b), "production run is not bitwise reproducible"
    tune("TRAIN_UNFUSED", 1)
    loss_u, _, bn_u, named_u = run()
    print(f"loss {abs(loss_a - loss_u) / loss_u:.3e}  bn {relerr(bn_a, bn_u.cpu()):.3e}")
    assert report("B3 80x48 loss: window statistics vs separate pass", abs(loss_a - loss_u) / loss_u, 1e-6)
    assert report("B3 80x48 BatchNorm buffers: window statistics vs separate pass", relerr(bn_a, bn_u.cpu()), 1e-6)
    for n in named_a:
        if n.endswith(".bias") and n != "deconv6.bias":
            continue                                               # bias in front of a BatchNorm: rounding noise around 0
        e = (named_a[n] - named_u[n]).norm().item() / max(named_u[n].norm().item(), 1e-12)
        print(f"grad {n}: {e:.3e}")
        assert report(f"B3 80x48 grad {n}: window statistics vs separate pass", e, 1e-2)


def test_batch_64_plans_name_the_window_kernel():
    buf = ctypes.create_string_buffer(128)
    for name, (h, w, c, ho, wo, n) in (("deconv4.fwd", (64, 16, 128, 128, 32, 32)), ("deconv5.fwd", (128, 32, 64, 256, 64, 16)),
                                       ("conv2.bwd_data", (128, 32, 32, 256, 64, 16)), ("conv3.bwd_data", (64, 16, 64, 128, 32, 32))):
        L().svs_describe_plan(1, 64, h, w, c, ho, wo, n, buf, 128)
        assert buf.value.decode().startswith("parity_window_kernel<"), (name, buf.value)
