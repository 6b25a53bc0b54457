"""The stage-local oracle of the full objective's loss stages (oracle/loss_stage_oracle.py) pinned on the CPU (-m "not gpu"):

consistency  fed its own fp64 stages (mask of unet_oracle in training mode), every row is at rounding, and the chained
             reference of d_logit (term_L1 + term_MR through the numpy adjoint) equals autograd of the WHOLE objective with
             respect to the logits to 1e-10: the stage oracle says what the whole-objective oracle says;
feasibility  every stage restated in torch float32, standing in for the device, keeps every row of every GPU case within its
             bound, and the elements the reference cannot decide stay under 1e-3 of every tile;
sensitivity  nine faults in the MR half of the gradient, planted in that float32 run, each put a row at >= 10 x its bound;
blind spot   on a batch of equally loud tiles two of those faults (and a 50 % scale error of the MR term) move
             d(total)/d(mask) by less than the 2e-2 rel-L2 that the whole-step tests (test_train_step_full_objective,
             test_full_objective_windows) allow the parameter gradients: what those gates cannot see."""
import functools

import numpy as np
import pytest
import torch

from oracle import loss_stage_oracle as ls
from oracle import mrstft_oracle as mo
from oracle import unet_oracle as uo
from svs_unet_pytorch_amd import synth

# the GPU cases of tests/test_gpu_loss_stages.py: (B, H, W, hop)
CASES = [(5, 256, 32, 128), (5, 256, 32, 100), (5, 512, 8, 768), (5, 1024, 4, 1024), (20, 256, 32, 128)]
CASE_IDS = ["-".join(map(str, c)) for c in CASES]
FIRST_TILE = 2300
WHOLE_STEP_GATE = 2e-2


def oracle_mask(mix, B):
    """(mask, logit) of the oracle U-Net in training mode (fresh statistics, dropout masks in place), float64."""
    state = uo.to_torch_state(synth.closed_form_state(trained_stats=False), torch.float64)
    masks = [torch.from_numpy(m).double() for m in synth.dropout_masks(B, seed=5, step=0)]
    taps = {}
    with torch.no_grad():
        mask = uo.forward(state, mix.double(), training=True, dropout_masks=masks, update_stats=True, taps=taps)
    return mask, taps["deconv6.raw"]


@functools.lru_cache(maxsize=None)
def inputs(case):
    B, H, W, _ = case
    mix, voc, mph, vph = (torch.from_numpy(a) for a in ls.hetero_tiles(B, H, W, FIRST_TILE))
    mask, logit = oracle_mask(mix, B)
    return {"mix": mix, "voc": voc, "mph": mph, "vph": vph, "mask": mask, "logit": logit}


@functools.lru_cache(maxsize=None)
def fake(case, dtype):
    """The loss stages of `case` on the CPU in `dtype`; computed once, shared, never written to."""
    i = inputs(case)
    return ls.stages(i["mask"], i["mix"], i["voc"], i["mph"], i["vph"], case[3], dtype=dtype)


def rows_of(case, buffers, losses):
    i = inputs(case)
    return ls.check(buffers, losses, i["mix"], i["voc"], i["mph"], i["vph"], case[3])


def show(rows):
    for r in rows:
        print(f"{r.stage:28s} tile {r.tile:3d} {r.err:.3e} / {r.bound:.1e}{'' if r.ok else '  FAIL'}")


def test_hetero_tiles_are_what_the_tests_rely_on():
    for B in (5, 20):
        mix, voc, mph, vph = ls.hetero_tiles(B, 256, 32, FIRST_TILE)
        again = ls.hetero_tiles(B, 256, 32, FIRST_TILE)
        assert all(np.array_equal(a, b) for a, b in zip((mix, voc, mph, vph), again))             # deterministic
        assert mix.shape == voc.shape == mph.shape == vph.shape == (B, 1, 256, 32) and mix.dtype == voc.dtype == np.float32
        assert np.abs(mph).max() <= np.pi and not np.array_equal(mph, vph)
        base_mix, base_voc = synth.tiles(B, 256, 32, first_tile=FIRST_TILE)
        for rep in range(B // 5):
            t = 5 * rep
            lv = np.float32(0.5 ** rep)
            assert np.array_equal(mix[t], base_mix[t] * lv) and np.array_equal(voc[t], base_voc[t] * lv)
            quiet = np.float32(0.03 * 2.0 ** rep)
            assert np.array_equal(mix[t + 1], base_mix[t + 1] * quiet) and np.array_equal(voc[t + 1], base_voc[t + 1] * quiet)
            assert not voc[t + 2].any() and np.array_equal(mix[t + 2], base_mix[t + 2] * lv)
            assert not mix[t + 3].any() and not voc[t + 3].any()
            assert np.array_equal(voc[t + 4], np.float32(1.5) * base_mix[t + 4] * lv) and not np.maximum(mix[t + 4] - voc[t + 4], 0).any()
        levels = [float(mix[b].max()) for b in range(B) if mix[b].any()]
        assert len({round(v, 6) for v in levels}) >= (2 if B == 5 else 8)                      # distinct levels, past waveform 16 too
    for B, H, W, hop in CASES:
        assert hop * (W - 1) > 2048 and hop <= 2 * H


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_chain_consistency_with_autograd_of_the_whole_objective(case):
    B, H, W, hop = case
    i = inputs(case)
    buffers, losses, _ = fake(case, torch.float64)
    rows = rows_of(case, buffers, losses)
    show(rows)
    assert len([r for r in rows if r.stage.startswith("d_logit left out")]) == B
    for r in rows:
        if r.stage == "d_logit left out":
            assert r.ok, r
        else:
            assert r.err <= 1e-10, r
    # the whole objective (train.py:274-296) in one autograd graph, differentiated with respect to the logits
    logit = i["logit"].detach().clone().requires_grad_(True)
    mask = torch.sigmoid(logit)
    assert torch.equal(mask.detach(), i["mask"])
    mix, voc = i["mix"].double(), i["voc"].double()
    l1 = torch.nn.functional.l1_loss(mask * mix, voc) + torch.nn.functional.l1_loss((1 - mask) * mix, torch.clamp(mix - voc, min=0.0))
    mr = mo.mrstft_loss(ls.specific_istft(mask * mix, i["mph"].double(), 2 * H, hop), ls.specific_istft(voc, i["vph"].double(), 2 * H, hop))
    (mo.ALPHA_L1 * l1 + mo.ALPHA_MR * mr).backward()
    assert bool(torch.isfinite(logit.grad).all())
    assert abs(float(l1.detach()) - losses[0]) <= 1e-12 * losses[0] and abs(float(mr.detach()) - losses[1]) <= 1e-12 * losses[1]
    term_l1, term_mr, _ = ls.d_logit_terms(i["mask"], buffers["d_wav"], i["mix"], i["voc"], i["mph"], hop, mo.ALPHA_L1)
    chained = term_l1 + term_mr
    for b in range(B):
        want = logit.grad[b]
        if not mix[b].any():
            assert not want.any() and not chained[b].any()
        else:
            e = (chained[b] - want).abs().max().item() / want.abs().max().item()
            print(f"chained d_logit vs autograd, tile {b}: {e:.3e}")
            assert e <= 1e-10, (b, e)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_reference_alone_passes_in_float32(case):
    """torch float32 on the CPU through every gate the GPU test applies; prints the worst err / bound per stage."""
    buffers, losses, _ = fake(case, torch.float32)
    assert all(t.dtype == torch.float32 for t in buffers.values())
    rows = rows_of(case, buffers, losses)
    show(rows)
    for stage, (q, tile) in ls.worst_by_stage(rows).items():
        print(f"fp32 restatement {case}: worst err/bound of {stage}: {q:.3e} (tile {tile})")
    bad = [r for r in rows if not r.ok]
    assert not bad, bad
    shares = [r for r in rows if r.stage == "d_logit left out"]
    assert len(shares) == case[0] and all(r.err <= 1e-3 for r in shares)


def test_float32_holds_the_validation_gates_on_these_tiles():
    """test_gpu_loss_stages.py::test_eval_loss_on_heterogeneous_tiles keeps GATE_L1 / GATE_MR of test_gpu_validation.py: torch
    float32 on the CPU (plain and shared-transform MR-STFT) holds them on the uneven tiles, from the eval-mode mask."""
    from test_gpu_validation import GATE_L1, GATE_MR, losses64
    B, H, W, hop = CASES[0]
    arrays = ls.hetero_tiles(B, H, W, FIRST_TILE)
    mix, voc, mph, vph = (torch.from_numpy(a) for a in arrays)
    with torch.no_grad():
        mask = uo.forward(uo.to_torch_state(synth.closed_form_state(), torch.float64), mix.double(), training=False).float()
    l1_w, mr_w = losses64(mask, *arrays, hop)
    buffers, (l1, mr), _ = ls.stages(mask, mix, voc, mph, vph, hop, dtype=torch.float32)
    mr_shared = float(mo.mrstft_loss_shared_fft(buffers["wav_pred"], buffers["wav_tgt"]))
    e = abs(l1 - l1_w) / l1_w, abs(mr - mr_w) / mr_w, abs(mr_shared - mr_w) / mr_w
    print(f"fp32 on the CPU, uneven tiles: L1 rel {e[0]:.3e} (gate {GATE_L1:.0e})  MR rel {e[1]:.3e} plain, {e[2]:.3e} shared transform "
          f"(gate {GATE_MR:.0e}); MR part {mr_w:.1f}")
    assert e[0] <= GATE_L1 and e[1] <= GATE_MR and e[2] <= GATE_MR


# ---- mutants -------------------------------------------------------------------------------------------------------
MUTANT_CASE = CASES[0]


def mutant(name):
    """(buffers, losses) of the float32 run of MUTANT_CASE with one fault planted."""
    case = MUTANT_CASE
    B, H, W, hop = case
    i = inputs(case)
    buffers, losses, parts = fake(case, torch.float32)
    buffers = dict(buffers)
    l1, mrt = parts["term_l1"], parts["term_mr"]
    f32 = lambda k: i[k].float()
    pull = lambda d_wav: ls.mr_term(buffers["mask"], d_wav, f32("mix"), f32("mph"), hop)
    if name == "MR term x 1.05":
        buffers["d_logit"] = l1 + 1.05 * mrt
    elif name == "MR term x (1 - 1/B)":
        buffers["d_logit"] = l1 + (1 - 1 / B) * mrt
    elif name == "d_wav of tile b applied to tile b+1":
        buffers["d_logit"] = l1 + pull(torch.roll(buffers["d_wav"], 1, 0))
    elif name == "first frame of the adjoint dropped":
        t = mrt.clone()
        t[..., 0] = 0
        buffers["d_logit"] = l1 + t
    elif name == "last frame of the adjoint dropped":
        t = mrt.clone()
        t[..., -1] = 0
        buffers["d_logit"] = l1 + t
    elif name == "frequency row 0 of the MR term zeroed":
        t = mrt.clone()
        t[:, :, 0, :] = 0
        buffers["d_logit"] = l1 + t
    elif name == "alpha_l1 and alpha_mr exchanged":
        buffers, losses, _ = ls.stages(i["mask"], i["mix"], i["voc"], i["mph"], i["vph"], hop, alpha_l1=mo.ALPHA_MR, alpha_mr=mo.ALPHA_L1,
                                       dtype=torch.float32)
    elif name == "wav_pred built with voc_phase":
        buffers, losses, _ = ls.stages(i["mask"], i["mix"], i["voc"], i["mph"], i["vph"], hop, dtype=torch.float32, pred_phase=i["vph"])
    elif name == "tile 2 from the whole-batch ratio":
        _, g = mo.mrstft_loss_and_grad_whole_batch_ratio(buffers["wav_pred"], buffers["wav_tgt"])
        d_wav = buffers["d_wav"].clone()
        d_wav[2] = mo.ALPHA_MR * g[2]
        d_logit = buffers["d_logit"].clone()
        d_logit[2] = (l1 + pull(d_wav))[2]
        buffers["d_logit"] = d_logit
    else:
        raise ValueError(name)
    return buffers, losses


MUTANTS = ["MR term x 1.05", "MR term x (1 - 1/B)", "d_wav of tile b applied to tile b+1", "first frame of the adjoint dropped",
           "last frame of the adjoint dropped", "frequency row 0 of the MR term zeroed", "alpha_l1 and alpha_mr exchanged",
           "wav_pred built with voc_phase", "tile 2 from the whole-batch ratio"]


@pytest.mark.parametrize("name", MUTANTS)
def test_mutant_lands_ten_times_over_a_bound(name):
    clean, clean_losses, _ = fake(MUTANT_CASE, torch.float32)
    assert not [r for r in rows_of(MUTANT_CASE, clean, clean_losses) if not r.ok]
    rows = rows_of(MUTANT_CASE, *mutant(name))
    over = {r: (r.err / r.bound if r.bound > 0 else float("inf") if r.err > 0 else 0.0) for r in rows if r.stage != "d_logit left out"}
    worst = max(over, key=over.get)
    print(f"mutant '{name}': {over[worst]:.1f} x the bound at {worst.stage} tile {worst.tile}; rows over their bound: "
          f"{sorted({(r.stage, r.tile) for r in rows if not r.ok})}")
    assert over[worst] >= 10, (name, worst, over[worst])


def test_the_whole_step_gate_cannot_see_these():
    """On five equally loud tiles (synth.tiles as the existing full-objective tests use them) the MR term is a few percent of
    d(total)/d(mask), so a 5 % or even 50 % scale error of it, or a lost frequency row, moves the gradient that enters the
    network's backward by less than the 2e-2 rel-L2 those tests allow; the same faults are >= 10 x over a stage bound above."""
    B, H, W, hop = MUTANT_CASE
    mix, voc = (torch.from_numpy(a) for a in synth.tiles(B, H, W, first_tile=FIRST_TILE))
    mph, vph = torch.from_numpy(ls.angles(30, (B, 1, H, W))), torch.from_numpy(ls.angles(31, (B, 1, H, W)))
    mask, _ = oracle_mask(mix, B)
    _, _, parts = ls.stages(mask, mix, voc, mph, vph, hop)
    per = mask * (1 - mask)
    l1, mrt = parts["term_l1"] / per, parts["term_mr"] / per                   # d/d(mask)
    total = l1 + mrt
    for b in range(B):
        share = mrt[b].norm().item() / total[b].norm().item()
        print(f"loud tile {b}: MR term is {share:.3%} of d(total)/d(mask)")
        assert share < 0.05
    row0 = mrt.clone()
    row0[:, :, 0, :] = 0
    for name, t in (("MR term x 1.05", 1.05 * mrt), ("MR term x 0.5", 0.5 * mrt), ("frequency row 0 of the MR term zeroed", row0)):
        change = (l1 + t - total).norm().item() / total.norm().item()
        print(f"all-loud batch, '{name}': d(total)/d(mask) changes by {change:.3e} rel-L2 (whole-step gate {WHOLE_STEP_GATE:.0e})")
        assert 0 < change < WHOLE_STEP_GATE
