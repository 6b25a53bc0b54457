"""The stage-local training oracle (oracle/train_stage_oracle.py) pinned on the CPU (-m "not gpu"):

consistency  a workspace built from unet_oracle's own fp64 step (taps + retain_grad) satisfies every stage to 1e-12, so the
             stage oracle says what the whole-step oracle says -- and that one is pinned to the reference by tests/golden;
feasibility  the same step in float32 on the CPU, standing in for the device, passes every gate tests/test_gpu_train_stages.py
             applies: the gates leave room for a correct fp32 implementation;
mutations    faults of the kind the whole-step gates let through, planted in that float32 workspace, each make the stage
             named for them fail, and no stage that does not read the mutated buffer."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import train_stage_oracle as ts
from oracle import unet_oracle as uo
from svs_unet_pytorch_amd import synth

# the shapes of the GPU cases: (B, H, W, dropout, loss_scale)
ODD = (3, 130, 68, True, 1.0)
CASES = {"B3_130x68_drop": ODD, "B64_32x8_drop": (64, 32, 8, True, 1.0), "B3_130x68_nodrop_scaled": (3, 130, 68, False, 166.66)}


@functools.lru_cache(maxsize=None)
def fake(case, dtype):
    B, H, W, drop, scale = case
    state = synth.closed_form_state(trained_stats=False)
    mix, voc = (torch.from_numpy(a) for a in synth.tiles(B, H, W, first_tile=700))
    masks = [torch.from_numpy(m) for m in synth.dropout_masks(B, seed=31)] if drop else None
    buffers, grads, loss, taps = ts.whole_step(state, mix, voc, masks, scale, dtype)
    return {"params": uo.to_torch_state(state), "mix": mix, "voc": voc, "masks": masks, "scale": scale,
            "buffers": buffers, "grads": grads, "loss": loss, "taps": taps}


def rows_of(f, buffers=None, grads=None, masks=None):
    return ts.check(buffers or f["buffers"], grads or f["grads"], f["loss"], f["params"], f["mix"], f["voc"],
                    masks if masks is not None else f["masks"], f["scale"])


def show(rows):
    for r in rows:
        print(f"{r.stage:60s} {r.err:.3e} / {r.bound:.1e}{'' if r.ok else '  FAIL'}")


@pytest.mark.parametrize("key", list(CASES))
def test_consistency_with_the_whole_step_oracle(key):
    f = fake(CASES[key], torch.float64)
    rows = rows_of(f)
    show(rows)
    assert len(rows) == 11 * 11 + 6 + 11                  # 7 forward + 4 backward rows per BatchNorm layer; mask, loss, d_logit (2), deconv6 (2); 11 dx
    for r in rows:
        if r.kind == "kinks":
            assert r.ok, r
        elif r.kind == "db":
            # a ratio to a bound made for fp32 sums (P 2^-24 sum|d_raw|), not an error: the fp64 step's own rounding is 2^-29 of
            # the fp32 one, so it stays far below a millionth of the bound
            assert r.err <= 1e-6, r
        else:
            assert r.err <= 1e-12, r
    # what the dcat buffers hold after the step, restated with the adjoint convolutions on the step's own d_raw
    B, H, W = CASES[key][:3]
    hw, taps, p, buf = ts.level_sizes(H, W), f["taps"], f["params"], f["buffers"]
    for k in range(1, 6):
        dec, enc = f"deconv{7 - k}", f"conv{k + 1}"
        d_out = taps[dec + ".raw"].grad
        dx_dec = F.conv2d(d_out, p[dec + ".weight"].double(), None, stride=2, padding=2)
        d_raw = taps[enc + ".raw"].grad
        op = uo._deconv_output_padding(d_raw.shape[-2:], hw[k])
        dx_enc = F.conv_transpose2d(d_raw, p[enc + ".0.weight"].double(), None, stride=2, padding=2, output_padding=op)
        assert ts._relerr(buf[f"dcat{k}"][:, :ts.CH[k]], dx_dec[:, :ts.CH[k]]) <= 1e-12
        assert ts._relerr(buf[f"dcat{k}"][:, ts.CH[k]:], dx_dec[:, ts.CH[k]:] + dx_enc) <= 1e-12
    assert ts._relerr(buf["dc6"], F.conv2d(taps["deconv1.raw"].grad, p["deconv1.weight"].double(), None, stride=2, padding=2)) <= 1e-12


@pytest.mark.parametrize("key", list(CASES))
def test_gates_are_feasible_in_float32(key):
    rows = rows_of(fake(CASES[key], torch.float32))
    show(rows)
    bad = [r for r in rows if not r.ok]
    assert not bad, bad


# ---- mutations -----------------------------------------------------------------------------------------------------
def failing(f, name, tensor=None, masks=None):
    """Rows that fail once buffer / gradient `name` is replaced by `tensor` (or the checker is given other masks)."""
    buffers, grads = dict(f["buffers"]), dict(f["grads"])
    if tensor is not None:
        (buffers if name in buffers else grads)[name] = tensor
    bad = [r for r in rows_of(f, buffers, grads, masks) if not r.ok]
    show(bad)
    return bad


def expect(bad, name, stages):
    """Every named stage fails, and nothing fails that does not read `name`."""
    got = [r.stage for r in bad]
    for s in stages:
        assert any(g.startswith(s) for g in got), (s, got)
    stray = [r.stage for r in bad if name not in r.reads]
    assert not stray, stray


@pytest.fixture(scope="module")
def f32():
    f = fake(ODD, torch.float32)
    assert not [r for r in rows_of(f) if not r.ok]
    return f


def test_mutation_dropped_encoder_term_in_skip_half(f32):
    """The accumulate of svs_enc_block_bwd_data left out: the skip half of dcat2 holds deconv5's part alone."""
    d_raw = f32["taps"]["conv3.raw"].grad
    hw = ts.level_sizes(130, 68)
    op = uo._deconv_output_padding(d_raw.shape[-2:], hw[2])
    dx_enc = F.conv_transpose2d(d_raw, f32["params"]["conv3.0.weight"], None, stride=2, padding=2, output_padding=op)
    t = f32["buffers"]["dcat2"].clone()
    t[:, 32:] -= dx_enc
    expect(failing(f32, "dcat2", t), "dcat2", ["dx dcat2 skip half"])


@pytest.mark.parametrize("level,edge", [(2, "row"), (2, "column"), (1, "row")])
def test_mutation_zeroed_last_row_or_column(f32, level, edge):
    """A ragged last tile not written: 65x34 at level 1, 33x17 at level 2."""
    t = f32["buffers"][f"dcat{level}"].clone()
    assert t.shape[-2 if edge == "row" else -1] % 2 == 1
    if edge == "row":
        t[:, :, -1, :] = 0
    else:
        t[:, :, :, -1] = 0
    expect(failing(f32, f"dcat{level}", t), f"dcat{level}", [f"dx dcat{level} decoder half", f"dx dcat{level} skip half"])


def test_mutation_swapped_level1_planes(f32):
    t = f32["buffers"]["cat1"]
    expect(failing(f32, "cat1", torch.cat([t[:, 16:], t[:, :16]], 1)), "cat1", ["act conv1", "act deconv5", "raw conv2", "mask"])


def test_mutation_dropout_mask_shifted_by_one_sample(f32):
    masks = list(f32["masks"])
    masks[2] = torch.roll(masks[2], 1, 0)
    assert not torch.equal(masks[2], f32["masks"][2])
    expect(failing(f32, "drop2", masks=masks), "drop2", ["act deconv3", "dgamma deconv3", "dw deconv3"])


def test_mutation_one_channel_quad_of_dw_half_a_percent_off(f32):
    t = f32["grads"]["conv4.0.weight"].clone()
    q = int(t.abs().amax((1, 2, 3)).argmax()) // 4
    t[4 * q:4 * q + 4] *= 1.005
    bad = failing(f32, "conv4.0.weight", t)
    expect(bad, "conv4.0.weight", ["dw conv4"])
    assert len(bad) == 1


@pytest.mark.parametrize("name", ["conv2", "conv3", "conv4", "deconv2", "deconv1", "conv6"])     # levels 2, 3, 4, 4, 5, 6
def test_mutation_bias_gradient_misses_the_last_eighth_of_the_pixels(f32, name):
    L = next(l for l in ts.BN_LAYERS if l.name == name)
    d_raw = f32["taps"][name + ".raw"].grad.permute(0, 2, 3, 1).reshape(-1, L.N)           # pixels in the device's order
    db = d_raw[:d_raw.shape[0] * 7 // 8].sum(0)
    bad = failing(f32, ts.bias_key(L), db)
    expect(bad, ts.bias_key(L), [f"db {name} "])
    assert len(bad) == 1


def test_mutation_one_invstd_entry_off_by_1e_4(f32):
    t = f32["buffers"]["invstd3"].clone()
    t[int(t.argmax())] *= 1 + 1e-4
    bad = failing(f32, "invstd3", t)
    expect(bad, "invstd3", ["invstd conv4"])
    assert len(bad) == 1
