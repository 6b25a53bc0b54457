"""Per-stage, per-tile parity of the full objective's loss stages (-m gpu): after ONE UNet.fwd_bwd with the phase tiles the
mask and d_logit are still in the training workspace (svs_unet_ws_offset(..., 1)) and the two re-synthesised waveforms and
d_wav in the MR workspace (svs_unet_mr_ws_offset).  Each is checked against oracle/loss_stage_oracle.py's fp64 reference
computed from the GPU's OWN buffer one stage upstream, tile by tile, so no error accumulates and every row is gated like the
kernel that wrote it is gated by itself (test_inverse_vs_torch_istft, test_gpu_mrstft.py's noise rule, GATE_LOSS / GATE_DLOGIT,
test_istft_bwd_mask_windows) -- not at the 2e-2 rel-L2 over the whole batch that the whole-step tests need.  The tiles differ
in level and kind (loss_stage_oracle.hetero_tiles): on a loud tile the MR term is 1-4 % of d(total)/d(mask), on a tile with a
silent vocal 95-98 %, and such a tile carries most of the batch's gradient.

Measured on an MI355X, worst err / bound per stage over the five cases (every row is in the parity report):
    wav_pred 1.7e-2 (B = 20, tile 17)   wav_tgt 1.2e-2   MR loss 5.4e-3 (hop 100)   d_wav l2 7.8e-2 (B = 20, tile 9)
    d_wav max 4.9e-2   L1 loss 3.9e-2   d_logit 2.6e-3 (B = 20, tile 2, silent vocal)   d_logit left out 0.73 (a condition)
    all-zero waveforms, the zero gradient of a silent prediction and d_logit of a tile with mix = 0: exactly 0.
    The eval-mode losses on the same tiles: L1 part 4.8e-8, MR part 9.4e-8 relative (gates 1e-5 / 1e-4).
No row failed: the kernels are right at these tiles, the silent-vocal, all-zero and past-waveform-16 ones included.

What the same rows do to a wrong MR half (tests/test_loss_stage_oracle.py plants each fault in a torch-float32 run of the first
case and feeds it to the same check(); times over the bound of the worst row, which is d_logit of the silent-vocal tile 2
unless named):
    MR term of d_logit x 1.05                 491        first frame of the adjoint dropped        6903
    MR term of d_logit x (1 - 1/B)           1963        last frame of the adjoint dropped         4175
    d_wav of tile b applied to tile b + 1    9988        frequency row 0 of the MR term zeroed     4117
    tile 2 from the whole-batch ratio        9806        wav_pred built with voc_phase            80583 (wav_pred, tile 0)
    alpha_l1 and alpha_mr exchanged        125758 (d_wav l2, tile 0)
On a batch of equally loud tiles the first, the frequency-row fault and even a 50 % scale error of the MR term move
d(total)/d(mask) by 1.4e-3, 2.4e-3 and 1.4e-2 rel-L2: under the whole-step tests' 2e-2.
"""
import numpy as np
import pytest
import torch

from oracle import loss_stage_oracle as ls
from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd.model import ALPHA_L1, ALPHA_MR, UNet
from test_gpu_validation import GATE_L1, GATE_MR, call_eval_loss, eval_model, losses64, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7FC17FC1      # an fp32 NaN no kernel computes: read anywhere, it shows
GUARD = 4096               # bytes allocated past each workspace the library is told about
FIRST_TILE = 2300

# (B, H, W, hop): the smallest shapes that reach each form; hop (W - 1) > 2048 everywhere
CASES = [(5, 256, 32, 128),      # n_fft 512, hop = n / 4: the general overlap-add inverse and its adjoint
         (5, 256, 32, 100),      # hop does not divide n_fft: the 1e-4 class
         (5, 512, 8, 768),       # the production window and hop, 3 n / 4: two-frames-per-sample kernel, edges by envelope
         (5, 1024, 4, 1024),     # n_fft 2048 at the n / 2 boundary, the narrowest tile the loss admits
         (20, 256, 32, 128)]     # more than 16 waveforms through the MR kernel and its finalise
CASE_IDS = ["-".join(map(str, c)) for c in CASES]


def to(a):
    return torch.from_numpy(a).to(DEV)


def make_model(B):
    m = UNet()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state(trained_stats=False).items()}, strict=True)
    m = m.to(DEV).train()
    m.set_dropout_masks([torch.from_numpy(x) for x in synth.dropout_masks(B, seed=5, step=0)])
    m.optim.zero_grad()
    return m


def sentinel_workspace(nbytes):
    """(int32 tensor of nbytes + GUARD bytes filled with the sentinel, the uint8 view of nbytes the library is told about)."""
    assert nbytes > 0 and nbytes % 4 == 0
    full = torch.full(((nbytes + GUARD) // 4,), SENTINEL, dtype=torch.int32, device=DEV)
    return full, full.view(torch.uint8)[:nbytes]


def take(full, off, *shape):
    assert off >= 0 and off % 256 == 0, off
    n = int(np.prod(shape))
    return full[off // 4:off // 4 + n].clone().view(*shape)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_loss_stages_against_oracle(case, report):
    """Every row of loss_stage_oracle.check() on what one full-objective fwd_bwd left behind (dropout on, loss_scale = ALPHA_L1,
    the mask left in the workspace as train.py leaves it); no element of the five buffers unwritten, no byte past either
    workspace written."""
    B, H, W, hop = case
    L = _lib.lib()
    length = hop * (W - 1)
    mix_np, voc_np, mph_np, vph_np = ls.hetero_tiles(B, H, W, FIRST_TILE)
    model = make_model(B)
    ws_bytes, mr_bytes = int(L.svs_unet_train_workspace_bytes(B, H, W)), int(L.svs_unet_train_mr_workspace_bytes(B, W, hop))
    ws, ws_view = sentinel_workspace(ws_bytes)
    mr, mr_view = sentinel_workspace(mr_bytes)
    model._ws[("train", B, H, W)] = ws_view
    model._ws[("mr", B, W, hop)] = mr_view
    l1 = model.fwd_bwd(to(mix_np), to(voc_np), loss_scale=ALPHA_L1, mix_phase=to(mph_np), voc_phase=to(vph_np), alpha_mr=ALPHA_MR, hop=hop)
    torch.cuda.synchronize()
    assert model._ws[("train", B, H, W)].data_ptr() == ws.data_ptr() and model._ws[("mr", B, W, hop)].data_ptr() == mr.data_ptr()
    assert bool((ws[ws_bytes // 4:] == SENTINEL).all()), "bytes past the training workspace were written"
    assert bool((mr[mr_bytes // 4:] == SENTINEL).all()), "bytes past the MR workspace were written"
    losses = (l1.item(), model.last_mr_loss.item())
    assert np.isfinite(losses).all(), losses

    raw = {name: take(ws, L.svs_unet_ws_offset(name.encode(), B, H, W, 1), B, 1, H, W) for name in ("mask", "d_logit")}
    raw.update({name: take(mr, L.svs_unet_mr_ws_offset(name.encode(), B, W, hop), B, length) for name in ("wav_pred", "wav_tgt", "d_wav")})
    for name, t in raw.items():
        assert not bool((t == SENTINEL).any()), f"{name}: elements no kernel wrote"
    buffers = {name: t.view(torch.float32).cpu() for name, t in raw.items()}
    for name, t in buffers.items():
        assert bool(torch.isfinite(t).all()), f"{name}: not finite"

    rows = ls.check(buffers, losses, *(torch.from_numpy(a) for a in (mix_np, voc_np, mph_np, vph_np)), hop, ALPHA_L1, ALPHA_MR)
    tag = f"B{B} {H}x{W} hop {hop}"
    bad = []
    for r in rows:
        kind = ls.KINDS[r.tile % 5] if r.tile >= 0 else "batch"
        label = f"loss stage {r.stage} tile {r.tile} ({kind}) {tag}"
        print(f"{label}: {r.err:.3e} / {r.bound:.1e}")
        if not report(label, r.err, r.bound) or not r.ok:
            bad.append((label, r.err, r.bound))
    for stage, (q, tile) in ls.worst_by_stage(rows).items():
        print(f"worst err/bound of {stage} {tag}: {q:.3e} (tile {tile})")
    assert not bad, bad


def test_alpha_mr_zero_with_phases_is_the_l1_call():
    """alpha_mr = 0 with the phase tiles given takes the L1 entry point: d_logit, the loss and the gradients are bitwise those
    of the call without phases, and no MR part is reported."""
    B, H, W, hop = CASES[0]
    L = _lib.lib()
    mix_np, voc_np, mph_np, vph_np = ls.hetero_tiles(B, H, W, FIRST_TILE)
    got = []
    for phases in (True, False):
        model = make_model(B)
        kw = dict(mix_phase=to(mph_np), voc_phase=to(vph_np), alpha_mr=0.0, hop=hop) if phases else {}
        loss = model.fwd_bwd(to(mix_np), to(voc_np), loss_scale=ALPHA_L1, **kw)
        torch.cuda.synchronize()
        assert model.last_mr_loss is None
        ws = model._ws[("train", B, H, W)].view(torch.int32)
        d_logit = take(ws, L.svs_unet_ws_offset(b"d_logit", B, H, W, 1), B, 1, H, W)
        got.append((loss.item(), d_logit, model._gflat.clone()))
    assert got[0][0] == got[1][0] and np.isfinite(got[0][0])
    assert torch.equal(got[0][1], got[1][1]) and bool(got[0][1].view(torch.float32).abs().max() > 0)
    assert torch.equal(got[0][2], got[1][2])


def test_eval_loss_on_heterogeneous_tiles(report):
    """svs_unet_eval_loss on the same uneven tiles with the mask returned: both loss parts against float64 of that mask, at the
    gates of test_gpu_validation.py.  (torch float32 on the CPU holds GATE_MR on these inputs: tests/test_loss_stage_oracle.py.)"""
    case = CASES[0]
    B, H, W, hop = case
    arrays = ls.hetero_tiles(B, H, W, FIRST_TILE)
    tensors = tuple(to(a) for a in arrays)
    model = eval_model()
    mask = torch.full_like(tensors[0], float("nan"))
    rc, losses = call_eval_loss(model, case, tensors, mask=mask)
    _lib.check(rc, "svs_unet_eval_loss")
    l1, mr = losses.tolist()
    assert bool(torch.isfinite(mask).all())
    l1_w, mr_w = losses64(mask.cpu(), *arrays, hop)
    e_l1, e_mr = rel(l1, l1_w), rel(mr, mr_w)
    print(f"eval loss on uneven tiles {case}: L1 {l1!r} rel {e_l1:.3e} (gate {GATE_L1:.0e})  MR {mr!r} rel {e_mr:.3e} (gate {GATE_MR:.0e})")
    ok = report(f"eval loss uneven tiles {case}: L1 part vs float64 of its mask", e_l1, GATE_L1)
    ok &= report(f"eval loss uneven tiles {case}: MR-STFT part vs float64 of its mask", e_mr, GATE_MR)
    assert ok, (e_l1, e_mr)
    assert mr_w > 50           # the silent-vocal tile's row loss (of the order 1e3) is most of the batch's MR part
