"""The position-uniform form of the tap-skipping conv GEMM (conv_gemm_kernel<..., UNI = true, SKIP = true, ...>: batch a multiple of
the tile height, an M-tile is one pixel position of 64 images) through the four calls that reach it, against torch's float64 convolution on the CPU,
and against the generic tap-skipping form: at batches where a tile spans positions (32) or M has a tail (80) the generic form
must still serve, and with one K-split both forms add the same products in the same order, so they must agree as floats.

Shapes: the smallest at which the form can go wrong -- one and two M-tiles per position (B = 64, 128); inputs 4x4, 5x3 (padding on
two sides of a position, parity classes of different sizes) and 16x4; C = 16 (one K-tile per tap, never split) and C = 64 (split-K,
balanced where the planner balances); the 64x64 and the 64x128 tile.  One float64 reference per shape, computed at B = 128 and
shared by the four batch sizes (they run its first B images)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from svs_unet_pytorch_amd import _lib, synth
from test_gpu_ops import ws_guard, ws_tensor          # noqa: F401  (ws_guard is an autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BMAX = 128
TOL = 2e-5                                   # tests/test_gpu_ops.py: every conv call against float64
KINDS = ("enc_fwd", "dec_fwd", "enc_bwd_data", "dec_bwd_data")
GATHER = ("enc_fwd", "dec_bwd_data")         # svs_describe_plan kind 0; the other two are the parity GEMM (kind 1)
INPUTS = ((4, 4), (5, 3), (16, 4))


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr()


def rnd(shape, seed, lo=-1.0, hi=1.0):
    n = int(np.prod(shape))
    return torch.from_numpy((synth.uniform(seed, n) * (hi - lo) + lo).reshape(shape).astype(np.float32))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def relerr(got, want):
    want = want.double()
    return ((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


def out_size(kind, h, w):
    """Output grid of the GEMM for an h x w input: the gather calls halve it, the parity calls double it (odd input sizes give
    the odd output, whose parity classes differ in size)."""
    if kind in GATHER:
        return (h + 1) // 2, (w + 1) // 2
    return (2 * h if h % 2 == 0 else 2 * h - 1), (2 * w if w % 2 == 0 else 2 * w - 1)


_cases = {}


def case(kind, h, w, C, N):
    """Operands (BMAX images, NHWC on the device), packed weights and the float64 result without bias, once per shape.  The two
    calls of a GEMM mode share operands and reference: they differ in the entry point only."""
    mode = "gather" if kind in GATHER else "parity"
    key = (mode, h, w, C, N)
    if key not in _cases:
        ho, wo = out_size(kind, h, w)
        x = rnd((BMAX, C, h, w), 100 + h)
        if mode == "gather":
            wt = rnd((N, C, 5, 5), 200 + C, -0.1, 0.1)
            want = F.conv2d(x.double(), wt.double(), None, stride=2, padding=2)
            wp = torch.empty(N * C * 25, device=DEV)
            _lib.check(L().svs_pack_weight_gather(wt.to(DEV).contiguous().data_ptr(), wp.data_ptr(), N, C, S()))
        else:
            wt = rnd((C, N, 5, 5), 300 + C, -0.1, 0.1)
            op = (ho - (2 * h - 1), wo - (2 * w - 1))
            want = F.conv_transpose2d(x.double(), wt.double(), None, stride=2, padding=2, output_padding=op)
            wp = torch.empty(N * C * 25, device=DEV)
            _lib.check(L().svs_pack_weight_parity(wt.to(DEV).contiguous().data_ptr(), wp.data_ptr(), C, N, S()))
        _cases[key] = (nhwc(x).to(DEV), wp, want, ho, wo)
    return _cases[key]


def plan_name(kind, B, h, w, C, ho, wo, N):
    buf = ctypes.create_string_buffer(160)
    L().svs_describe_plan(0 if kind in GATHER else 1, B, h, w, C, ho, wo, N, buf, 160)
    return buf.value.decode()


def workspace(kind, B, h, w, C, ho, wo, N):
    n = L().svs_enc_block_workspace_bytes(B, h, w, C, N) if kind in GATHER else L().svs_dec_block_workspace_bytes(B, h, w, C, ho, wo, N)
    return ws_tensor(n)                          # sentinel-filled, told to the library at the queried size; ws_guard checks its tail


def run(kind, x, B, h, w, C, wp, bias, scale, shift, slope, y, ldy, ho, wo, N, accumulate, ws):
    """One of the four calls on the first B images of x: (B, h, w, C) -> (B, ho, wo, N) at y (row stride ldy)."""
    p = lambda t: t.data_ptr() if t is not None else None
    if kind == "enc_fwd":
        rc = L().svs_enc_block_fwd(p(x), C, B, h, w, C, p(wp), p(bias), p(scale), p(shift), slope, y, ldy, N, accumulate, p(ws), ws.numel(), S())
    elif kind == "dec_fwd":
        rc = L().svs_dec_block_fwd(p(x), C, B, h, w, C, p(wp), p(bias), p(scale), p(shift), slope, y, ldy, ho, wo, N, accumulate,
                                   p(ws), ws.numel(), S())
    else:
        assert bias is None and scale is None
        fn = L().svs_enc_block_bwd_data if kind == "enc_bwd_data" else L().svs_dec_block_bwd_data
        rc = fn(p(x), C, B, h, w, C, p(wp), y, ldy, ho, wo, N, accumulate, p(ws), ws.numel(), S())     # (dy, its grid and channels; dx, its grid and channels)
    _lib.check(rc, kind)


@pytest.mark.parametrize("B", [64, 128, 32, 80])
@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("C", [16, 64])
@pytest.mark.parametrize("h,w", INPUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_calls_against_float64(kind, h, w, C, N, B, report):
    x, wp, want_all, ho, wo = case(kind, h, w, C, N)
    want = want_all[:B]
    name = plan_name(kind, B, h, w, C, ho, wo, N)
    assert name.startswith("conv_gemm_kernel<") and name.split(", ")[-3] == "true", name     # <..., position-uniform, tap skipping, split-bf16 products, K-tiles ahead>
    assert (name.split(", ")[-4] == "true") == (B % 64 == 0), name
    tag = f"skip_uniform {kind} B{B} {h}x{w} C{C} N{N}"
    ws = workspace(kind, B, h, w, C, ho, wo, N)
    fwd = kind in ("enc_fwd", "dec_fwd")
    # raw output (+ bias in the forward calls) into one half of a wider buffer; the other half keeps its sentinel
    bias = rnd((N,), 400 + N) if fwd else None
    bd = bias.to(DEV) if fwd else None
    half = 1 if kind in GATHER else 0
    y = torch.full((B, ho, wo, 2 * N), 7.0, device=DEV)
    run(kind, x, B, h, w, C, wp, bd, None, None, 0.0, y.data_ptr() + 4 * N * half, 2 * N, ho, wo, N, 0, ws)
    torch.cuda.synchronize()
    assert torch.all(y[..., (1 - half) * N:(2 - half) * N] == 7.0), "wrote outside its channel slice"
    want_raw = want + bias.double()[None, :, None, None] if fwd else want
    e = relerr(nchw(y[..., half * N:(half + 1) * N]), want_raw)
    print(f"{tag} raw: {e:.3e}")
    assert report(tag + " raw", e, TOL)
    # accumulate (the backward-data calls add into the gradient of the skip half)
    if not fwd:
        run(kind, x, B, h, w, C, wp, None, None, None, 0.0, y.data_ptr() + 4 * N * half, 2 * N, ho, wo, N, 1, ws)
        e = relerr(nchw(y[..., half * N:(half + 1) * N]), 2 * want)
        print(f"{tag} accumulate: {e:.3e}")
        assert report(tag + " accumulate", e, TOL)
        assert torch.all(y[..., (1 - half) * N:(2 - half) * N] == 7.0), "wrote outside its channel slice"
        return
    # folded scale / shift / leaky epilogue, then the same call accumulating onto its own result
    sc, sh = rnd((N,), 500 + N, 0.5, 1.5), rnd((N,), 600 + N)
    want2 = F.leaky_relu(want * sc.double()[None, :, None, None] + sh.double()[None, :, None, None], 0.2)
    scd, shd = sc.to(DEV), sh.to(DEV)
    y2 = torch.empty((B, ho, wo, N), device=DEV)
    run(kind, x, B, h, w, C, wp, None, scd, shd, 0.2, y2.data_ptr(), N, ho, wo, N, 0, ws)
    e = relerr(nchw(y2), want2)
    print(f"{tag} folded: {e:.3e}")
    assert report(tag + " folded", e, TOL)
    run(kind, x, B, h, w, C, wp, None, scd, shd, 0.2, y2.data_ptr(), N, ho, wo, N, 1, ws)
    e = relerr(nchw(y2), 2 * want2)
    print(f"{tag} accumulate: {e:.3e}")
    assert report(tag + " accumulate", e, TOL)


@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_uniform_and_generic_forms_add_the_same_products(kind, N, tune):
    """B = 80 holds the B = 64 case's images first.  With one K-split every output is one chain of additions over the K-tiles in
    tap order in either form; a tap that the generic form's wider tile visits for a neighbouring position adds exact zeros.  The
    first 64 images must therefore come out equal as floats (==: the sign of a zero may differ)."""
    h, w, C = 5, 3, 64
    tune("CONV_KSPLIT", 1)
    x, wp, _, ho, wo = case(kind, h, w, C, N)
    outs = {}
    for B in (64, 80):
        name = plan_name(kind, B, h, w, C, ho, wo, N)
        assert name.split(", ")[-3] == "true" and (name.split(", ")[-4] == "true") == (B == 64), name
        ws = workspace(kind, B, h, w, C, ho, wo, N)
        y = torch.full((B, ho, wo, N), 7.0, device=DEV)
        run(kind, x, B, h, w, C, wp, None, None, None, 0.0, y.data_ptr(), N, ho, wo, N, 0, ws)
        torch.cuda.synchronize()
        outs[B] = y
    assert torch.all(outs[80][:64] == outs[64]), f"{kind} N{N}: uniform and generic forms differ"


def test_uniform_form_leaves_batchnorm_partials(tune):
    """The only callers that ask the GEMM's own epilogue for BatchNorm partials are the training forward's: one training forward at
    B = 64 on 32x8 tiles with one K-split, so that the position-uniform launches of conv3..conv6 and deconv1..deconv3 write the
    partials themselves.  The batch mean and 1/sqrt(var + eps) that the step derives from those partials are compared with the
    float64 statistics of the raw outputs the same launches wrote."""
    from svs_unet_pytorch_amd.model import DEC_IO, ENC_CHANNELS, UNet
    B, H, W = 64, 32, 8
    tune("CONV_KSPLIT", 1)
    hw = [(H, W)]
    for _ in range(6):
        hw.append(((hw[-1][0] + 1) // 2, (hw[-1][1] + 1) // 2))
    # (layer index, workspace name of its raw output, describe arguments, output level, output channels)
    layers = [(k - 1, f"raw_e{k}", (0, *hw[k - 1], ENC_CHANNELS[k - 1], *hw[k], ENC_CHANNELS[k]), k, ENC_CHANNELS[k]) for k in range(3, 7)]
    layers += [(5 + j, f"raw_d{j}", (1, *hw[7 - j], DEC_IO[j - 1][0], *hw[6 - j], DEC_IO[j - 1][1]), 6 - j, DEC_IO[j - 1][1]) for j in range(1, 4)]
    buf = ctypes.create_string_buffer(160)
    for _, _, (kind, h, w, c, ho, wo, n), _, _ in layers:
        assert L().svs_describe_plan(kind, B, h, w, c, ho, wo, n, buf, 160) == 1
        assert buf.value.decode().split(", ")[-4:-2] == ["true", "true"], buf.value            # position-uniform, tap skipping
    m = UNet()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state(trained_stats=False).items()}, strict=True)
    m.to(DEV).train()
    m.set_dropout_masks([])
    mix_np, _ = synth.tiles(B, H, W, first_tile=4200)
    with torch.no_grad():
        m(torch.from_numpy(mix_np).to(DEV))
    torch.cuda.synchronize()
    ws = m._workspace("train", B, H, W)

    def view(name, count):
        off = L().svs_unet_ws_offset(name.encode(), B, H, W, 1)
        assert off >= 0, name
        return ws[off:off + 4 * count].view(torch.float32)

    for l, raw_name, _, lvl, n in layers:
        P = B * hw[lvl][0] * hw[lvl][1]
        raw = view(raw_name, P * n).view(P, n).double().cpu()
        mean, var = raw.mean(0), raw.var(0, unbiased=False)
        e_mean = relerr(view(f"mean{l}", n), mean)
        e_inv = relerr(view(f"invstd{l}", n), 1.0 / torch.sqrt(var + 1e-5))
        print(f"skip_uniform partials layer {l}: mean {e_mean:.3e} invstd {e_inv:.3e}")
        assert e_mean <= TOL and e_inv <= TOL, (l, e_mean, e_inv)
