"""Exits of the shared K-loop (csrc/gemm_pipeline.h) on the GPU (-m gpu): blocks that compute 0, 1, 2 and 3 K-tiles -- a first
fetch that does not happen, the `break` after the first phase of the two-ahead schedule, the fall-through after its second --
and, with tap skipping, K positions that next() jumps over.  The planners never make splits that short, so the switches force
them.  Reference: torch convolutions in float64 on the CPU; tolerance and error measure are test_gpu_ops.py's for the same
kernels (2e-5 of the output's magnitude: fp32 MFMA is an exact fmaf chain, the error is summation order)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from svs_unet_pytorch_amd import _lib

from test_gpu_ops import DEV, L, S, nchw, nhwc, pack_gather, pack_parity, relerr, rnd, ws_guard, ws_tensor          # noqa: F401  (ws_guard is an autouse fixture)

pytestmark = pytest.mark.gpu

TILES = [(128, 128), (128, 64), (256, 32), (256, 16), (32, 128), (64, 64), (64, 128)]      # CONV_CFG 0 .. 6: (BM, BN)
C = 16                                # one K-tile per tap: 25 per GATHER row, 9 / 6 / 6 / 4 per PARITY class
H, W = 4, 2                           # GATHER: 2 x 1 outputs, PARITY: 8 x 4; most taps of every position are padding


@functools.lru_cache(maxsize=None)
def conv_reference(mode, B, N):
    x, b = rnd((B, C, H, W), 10), rnd((N,), 12)
    if mode == 0:
        w = rnd((N, C, 5, 5), 11, -0.1, 0.1)
        want = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=2)
        return nhwc(x).to(DEV), pack_gather(w), b.to(DEV), want
    w = rnd((C, N, 5, 5), 11, -0.1, 0.1)
    want = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=2, output_padding=1)
    return nhwc(x).to(DEV), pack_parity(w), b.to(DEV), want


# GATHER: 25 splits of 1 K-tile, 9 of 2-3; PARITY: 4 splits of 2,2,2,3 / 1-2 / 1-2 / 1 K-tiles.
# Batch 128 with tap skipping: B % BM == 0 for the 32-, 64- and 128-row tiles, so those that have the position-uniform form take it
# and 128x128 takes the generic tap-skipping form; whole splits fall into the padding.  Batch 3 without: generic form, M tail.
@pytest.mark.parametrize("B,skip", [(128, 2), (3, 0)])
@pytest.mark.parametrize("mode,ksplit", [(0, 25), (0, 9), (1, 4)])
@pytest.mark.parametrize("cfg", range(7))
def test_conv_gemm_short_splits(cfg, mode, ksplit, B, skip, report, tune):
    BM, BN = TILES[cfg]
    N = BN
    tune("CONV_CFG", cfg)
    tune("CONV_KSPLIT", ksplit)
    tune("CONV_SKIP", skip)
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if mode == 0 else (2 * H, 2 * W)
    buf = ctypes.create_string_buffer(128)
    ks = L().svs_describe_plan(mode, B, H, W, C, Ho, Wo, N, buf, 128)
    name = buf.value.decode()
    skips = skip == 2 and BN >= 64                                 # (the tap-skipping form exists for the tiles at least 64 wide)
    form = ("true, true" if cfg != 0 else "false, true") if skips else "false, false"
    assert name.startswith(f"conv_gemm_kernel<{mode}, {BM}, {BN}, ") and f", {form}, false, " in name, name
    assert ks == ksplit or (skips and ks > 1), (name, ks)          # (balanced splits: the largest split count of a position)
    xd, wp, bd, want = conv_reference(mode, B, N)
    y = torch.full((B, Ho, Wo, 2 * N), 7.0, device=DEV)            # the second half of a wider buffer; the first stays as it is
    if mode == 0:
        ws = ws_tensor(L().svs_enc_block_workspace_bytes(B, H, W, C, N))
        _lib.check(L().svs_enc_block_fwd(xd.data_ptr(), C, B, H, W, C, wp.data_ptr(), bd.data_ptr(), None, None, 0.0,
                                         y.data_ptr() + 4 * N, 2 * N, N, 0, ws.data_ptr(), ws.numel(), S()))
    else:
        ws = ws_tensor(L().svs_dec_block_workspace_bytes(B, H, W, C, Ho, Wo, N))
        _lib.check(L().svs_dec_block_fwd(xd.data_ptr(), C, B, H, W, C, wp.data_ptr(), bd.data_ptr(), None, None, 0.0,
                                         y.data_ptr() + 4 * N, 2 * N, Ho, Wo, N, 0, ws.data_ptr(), ws.numel(), S()))
    torch.cuda.synchronize()
    assert torch.all(y[..., :N] == 7.0), "wrote outside its channel slice"
    e = relerr(nchw(y[..., N:]), want)
    print(f"{name} ksplit {ks} B{B}: relerr {e:.3e}")
    assert report(f"k_loop conv {name} ksplit{ks} B{B}", e, 2e-5)


@functools.lru_cache(maxsize=None)
def wgrad_reference(B, Hl, Cs, Cl):
    x = rnd((B, Cl, Hl, Hl), 80).double()
    w = rnd((Cs, Cl, 5, 5), 81, -0.1, 0.1).double().requires_grad_(True)
    y = F.conv2d(x, w, None, stride=2, padding=2)
    dy = rnd(tuple(y.shape), 83)
    y.backward(dy.double())
    return x.float(), dy, w.grad


# Conv2d weight gradient, S = dy (Cs channels, Hl/2 x Hl/2), L = x (Cl = 16 channels, Hl x Hl); K = pixels, 16 per K-tile.
# 8 x 8 at batch 1, 2, 3: P = 16, 32, 48 -- exactly 1, 2 and 3 K-tiles in one split (one tile ahead).  2 x 2 at batch 16 with
# tap skipping: one K-tile (two ahead on the 64- and 128-row tiles); of the four N-tiles (taps 0-7, 8-15, 16-23, 24) the first
# and the last have every tap in the padding, compute nothing and must write zeros.
@pytest.mark.parametrize("B,Hl,skip", [(1, 8, -1), (2, 8, -1), (3, 8, -1), (16, 2, 2)])
@pytest.mark.parametrize("Cs,cfg", [(32, -1), (128, -1), (128, 0)], ids=["32x128", "64x128", "128x128"])
def test_wgrad_gemm_short_k(Cs, cfg, B, Hl, skip, report, tune):
    Cl, Hs = 16, Hl // 2
    tune("WGRAD_CFG", cfg)
    tune("WGRAD_SKIP", skip)
    buf = ctypes.create_string_buffer(128)
    ks = L().svs_describe_plan(2, B, Hs, Hs, Cs, 0, 0, Cl, buf, 128)
    name = buf.value.decode()
    BM = 128 if cfg == 0 else min(Cs, 64)
    assert ks == 1 and name.startswith(f"wgrad_gemm_kernel<{BM}, 128, ") and f", {'true' if skip == 2 else 'false'}, false, " in name, (name, ks)
    x, dy, want = wgrad_reference(B, Hl, Cs, Cl)
    dyd = torch.full((B, Hs, Hs, Cs + 4), 9.0, device=DEV)          # strided operand views: the padding channels are never read
    dyd[..., :Cs] = nhwc(dy).to(DEV)
    xd = torch.full((B, Hl, Hl, Cl + 8), 9.0, device=DEV)
    xd[..., :Cl] = nhwc(x).to(DEV)
    n = Cs * Cl * 25
    out = torch.full((n + 128,), 7.0, device=DEV)                  # dw with 64 guard floats on either side
    ws = ws_tensor(L().svs_block_bwd_weight_workspace_bytes(B, Hs, Hs, Cs, Cl))
    _lib.check(L().svs_enc_block_bwd_weight(dyd.data_ptr(), Cs + 4, B, Hs, Hs, Cs, xd.data_ptr(), Cl + 8, Hl, Hl, Cl, out.data_ptr() + 4 * 64,
                                            None, ws.data_ptr(), ws.numel(), S()))
    torch.cuda.synchronize()
    assert torch.all(out[:64] == 7.0) and torch.all(out[64 + n:] == 7.0), "wrote outside dw"
    e = relerr(out[64:64 + n].view(Cs, Cl, 5, 5), want)
    print(f"{name} B{B} {Hl}x{Hl}: relerr {e:.3e}")
    assert report(f"k_loop wgrad {name} B{B} {Hl}x{Hl}", e, 2e-5)
