"""ORACLE -- TEST INFRASTRUCTURE ONLY.  Never imported by the product package.

Stage-local fp64 reference of one training step (forward, L1 loss, backward).  Where oracle/unet_oracle.py runs the
whole step, this module takes the buffers a step LEFT BEHIND -- the training workspace of svs_unet_train_fwd_bwd read back
as NCHW float32 tensors, or any other run laid out the same way -- and computes, for every layer, what each buffer should
hold from the buffers ONE STAGE UPSTREAM of it.  No error accumulates from stage to stage, so every comparison is one or
two kernels deep and is gated at the size of a per-kernel gate (tests/test_gpu_ops.py), not at the 1e-2 the whole-step
gates need after 22 BatchNorm / conv stages.

Buffers (`buffers`: name -> NCHW float32 tensor, names as svs_unet_ws_offset gives them):
    cat1..cat5      (B, 2 CH[k], h_k, w_k): channels [decoder half | skip half] at EVERY level (the reader undoes the
                    planar layout of level 1);  c6 (B, 512, h_6, w_6)
    raw0..raw10     pre-BatchNorm output of conv1..conv6, deconv1..deconv5;  mean<l>, invstd<l>: (N_l,)
    dcat1..dcat5, dc6, d_logit, mask:  the gradients of the above as they stand AFTER the whole step
    running_mean<l>, running_var<l>:  the BatchNorm buffers after the step
`grads`: state_dict name -> gradient.  `params`: the state_dict BEFORE the step (running statistics included).

Stages (one row of check() each; "reads" are the buffers a row depends on, its own included):
    raw <layer>        conv2d / conv_transpose2d(x_buf, w, b)
    mean / invstd      fp64 biased batch statistics of raw_buf
    act <layer>        leaky / relu(bn(raw_buf; fp64 statistics)) * dropout, against the activation half of cat / c6
    running_*          momentum 0.1 towards the batch mean and the UNBIASED variance of raw_buf
    mask, loss, d_logit
    dgamma, dbeta, dw, db <layer>   BatchNorm + activation + dropout backward of dy_buf on raw_buf (-> d_raw_ref), then the
                                    convolution's weight gradient of d_raw_ref and x_buf
    dx dcat<k> decoder half / skip half, dx dc6:   the data gradients, summed as the step sums them:
        decoder half of dcat[k] = first CH[k] channels of the dx of the decoder that reads cat[k]
        skip half of dcat[k]    = last CH[k] channels of that dx  +  dx of encoder k+1
    kinks <layer>, d_logit left out:  conditions on how much of a layer the reference cannot decide (below)

Activation kinks: where |z_ref| < 1e-5 max|z_ref| the sign of z is within rounding of the device's own, and a flipped branch
changes d_raw by O(1) of one element.  There the reference takes the branch the device took, read from its activation output
(relu: positive or zero; leaky: positive or negative); channels that Dropout2d zeroed tell nothing and are left to the
reference.  check() reports the share of such elements per layer as a row bounded by 1e-3: a condition, not a measurement.

Bias gradients in front of a BatchNorm are identically zero (the BatchNorm backward removes the mean of d_raw), so no
relative gate exists.  Their row is max_c |db[c]| / (P 2^-24 sum_pixels |d_raw_ref[:, c]|), bounded by 1: the worst any
summation order of P fp32 terms whose exact sum is zero can leave (Higham: |fl(sum) - sum| <= (P - 1) u sum |x_i|), with
the rounding of the P terms themselves (u sum |x_i|) inside the same bound once P >= 16.  The bound is WEAK at level 1:
with P of a few thousand to a few million, one dropped pixel of typical size is only 3-16 times the bound.  At levels 2..6 a
dropped eighth of the pixels is orders of magnitude above it.
"""
from __future__ import annotations

from collections import OrderedDict, namedtuple

import torch
import torch.nn.functional as F

from oracle import unet_oracle as uo

CH = (1, 16, 32, 64, 128, 256, 512)
Layer = namedtuple("Layer", "index name up C N lin lout bn_prefix")
LAYERS = tuple([Layer(k - 1, f"conv{k}", False, CH[k - 1], CH[k], k - 1, k, f"conv{k}.1") for k in range(1, 7)] +
               [Layer(5 + j, f"deconv{j}", True, 512 if j == 1 else 2 * CH[7 - j], CH[6 - j] if j < 6 else 1, 7 - j, 6 - j,
                      f"deconv{j}_BAD.0" if j < 6 else None) for j in range(1, 7)])
BN_LAYERS = LAYERS[:11]

# gates: the per-kernel gates of tests/test_gpu_ops.py (relative to the reference's max)
GATE_RAW = 2e-5            # test_enc_block_fwd, test_dec_block_fwd, test_out_block_fwd
GATE_BN = 1e-5             # test_bn_train_fwd_bwd: activation, running statistics; mean and invstd with them
GATE_LOSS = 1e-6           # test_bn_fold_and_loss_and_adam
GATE_DLOGIT = 1e-4         # test_bn_fold_and_loss_and_adam
GATE_BN_BWD = 2e-5         # test_bn_train_fwd_bwd: dgamma, dbeta
GATE_TWO = 4e-5            # BatchNorm backward (2e-5) then conv backward (2e-5)
GATE_OUT_BWD = 2e-5        # deconv6: one kernel from d_logit
KINK_BAND = 1e-5           # |z_ref| < KINK_BAND max|z_ref|: the device's branch
KINK_SHARE = 1e-3
LOSS_KINK = 1e-6           # |d1| or |d2| below this: the sign of the L1 term is not the reference's to decide
U32 = 2.0 ** -24


class Row(namedtuple("Row", "stage err bound")):
    """(stage name, error, bound) of one comparison; `kind` groups rows of a sort, `reads` names what the row depends on."""
    def __new__(cls, stage, err, bound, kind, reads):
        self = super().__new__(cls, stage, float(err), float(bound))
        self.kind, self.reads = kind, frozenset(reads)
        return self

    @property
    def ok(self):
        return self.err <= self.bound           # (a NaN error fails)


def weight_key(L):
    return f"{L.name}.0.weight" if not L.up else f"{L.name}.weight"


def bias_key(L):
    return f"{L.name}.0.bias" if not L.up else f"{L.name}.bias"


def level_sizes(H, W):
    hw = [(H, W)]
    for _ in range(6):
        hw.append(((hw[-1][0] + 1) // 2, (hw[-1][1] + 1) // 2))
    return hw


def x_name(L):
    return "mix" if L.index == 0 else "c6" if L.index == 6 else f"cat{L.lin}"


def act_name(L):
    return "c6" if L.index == 5 else f"cat{L.lout}"


def dy_name(L):
    return "dc6" if L.index == 5 else f"dcat{L.lout}"


def _x(L, buffers, mix):
    """Input of layer L: the mixture, the skip half of cat[k-1], the whole cat[lin], or c6."""
    if L.index == 0:
        return mix
    b = buffers[x_name(L)].double()
    return b[:, CH[L.lin]:] if not L.up else b


def _half(L, t):
    """The half of a level's (d)cat buffer that belongs to layer L's output: skip half for an encoder, decoder half for a decoder."""
    if L.index == 5:
        return t
    return t[:, CH[L.lout]:] if not L.up else t[:, :CH[L.lout]]


def _conv(L, x, w, b, out_hw):
    if not L.up:
        return F.conv2d(x, w, b, stride=2, padding=2)
    op = uo._deconv_output_padding(x.shape[-2:], out_hw)
    return F.conv_transpose2d(x, w, b, stride=2, padding=2, output_padding=op)


def _relerr(got, want):
    want = want.double()
    d = (got.double() - want).abs().max().item()
    return d / max(want.abs().max().item(), 1e-300)


def _c(v):
    return v[None, :, None, None]


def layer_forward(L, buffers, params, drop):
    """fp64 statistics of raw_buf, the expected activation and the branch mask.  Returns a dict: mean, var (biased), invstd,
    xhat, positive (the branch: the reference's own, the device's inside the kink band), act, kink_share."""
    raw = buffers[f"raw{L.index}"].double()
    mean = raw.mean((0, 2, 3))
    var = raw.var((0, 2, 3), unbiased=False)
    invstd = torch.rsqrt(var + uo.BN_EPS)
    xhat = (raw - _c(mean)) * _c(invstd)
    z = xhat * _c(params[L.bn_prefix + ".weight"].double()) + _c(params[L.bn_prefix + ".bias"].double())
    dev = _half(L, buffers[act_name(L)].double())
    band = z.abs() < KINK_BAND * z.abs().max()
    if drop is not None:
        band = band & (drop[:, :, None, None] != 0)
    positive = z > 0
    if L.up:                                            # relu: the device's output is positive or exactly zero
        positive = torch.where(band, dev > 0, positive)
    else:                                               # leaky: positive or negative; an exact zero decides nothing
        positive = torch.where(band & (dev != 0), dev > 0, positive)
    slope = 0.0 if L.up else uo.LEAKY_SLOPE
    act = torch.where(positive, z, slope * z)
    if drop is not None:
        act = act * drop[:, :, None, None]
    return {"mean": mean, "var": var, "invstd": invstd, "xhat": xhat, "positive": positive, "act": act,
            "kink_share": band.double().mean().item()}


def layer_backward(L, fwd, buffers, params, drop, x):
    """One composite backward stage: d_raw_ref = BatchNorm + activation + dropout backward of dy_buf on raw_buf with the fp64
    statistics, then dgamma, dbeta, dw, db, dx from d_raw_ref and x_buf."""
    dy = _half(L, buffers[dy_name(L)].double())
    slope = 0.0 if L.up else uo.LEAKY_SLOPE
    gz = torch.where(fwd["positive"], dy, slope * dy)
    if drop is not None:
        gz = gz * drop[:, :, None, None]
    dbeta = gz.sum((0, 2, 3))
    dgamma = (gz * fwd["xhat"]).sum((0, 2, 3))
    P = gz.numel() // gz.shape[1]
    gamma = params[L.bn_prefix + ".weight"].double()
    d_raw = _c(gamma * fwd["invstd"]) * (gz - _c(dbeta) / P - fwd["xhat"] * _c(dgamma) / P)
    dx, dw = conv_backward(L, x, params[weight_key(L)].double(), d_raw)
    return {"d_raw": d_raw, "dgamma": dgamma, "dbeta": dbeta, "dw": dw, "dx": dx, "P": P,
            "db_bound": P * U32 * d_raw.abs().sum((0, 2, 3))}


def conv_backward(L, x, w, d_out):
    """(dx, dw) of layer L's convolution for the output gradient d_out, by autograd on the fp64 convolution itself."""
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    _conv(L, x, w, None, d_out.shape[-2:]).backward(d_out)
    return x.grad, w.grad


def loss_stage(mask, mix, voc, loss_scale):
    """(loss, d_logit, elements the reference can decide) as svs_l1_mask_loss_fwd_bwd defines them: the loss is unscaled,
    d_logit carries loss_scale / n."""
    d1 = mask * mix - voc
    d2 = (1 - mask) * mix - torch.clamp(mix - voc, min=0.0)
    n = mask.numel()
    loss = (d1.abs().sum() + d2.abs().sum()) / n
    dm = (torch.sign(d1) - torch.sign(d2)) * mix * (loss_scale / n)
    return loss.item(), dm * mask * (1 - mask), (d1.abs() >= LOSS_KINK) & (d2.abs() >= LOSS_KINK)


def check(buffers, grads, loss, params, mix, voc, dropout_masks=None, loss_scale=1.0):
    """Every comparison of one training step as a list of Row(stage, err, bound).  `dropout_masks`: the five (B, C) masks
    of deconv1..deconv5, or None / [] for no dropout."""
    mix, voc = mix.double(), voc.double()
    hw = level_sizes(*mix.shape[-2:])
    drops = [None] * 5 if not dropout_masks else [m.double() for m in dropout_masks]
    rows = []

    def rel(stage, kind, got, want, bound, reads):
        rows.append(Row(stage, _relerr(got, want), bound, kind, reads))

    fwd, xs = {}, {}
    for L in BN_LAYERS:
        l, n = L.index, L.name
        drop, dname = (drops[l - 6], [f"drop{l - 6}"]) if L.up else (None, [])
        x = xs[l] = _x(L, buffers, mix)
        w, b = params[weight_key(L)].double(), params[bias_key(L)].double()
        rel(f"raw {n}", "raw", buffers[f"raw{l}"], _conv(L, x, w, b, hw[L.lout]), GATE_RAW, [x_name(L), f"raw{l}"])
        f = fwd[l] = layer_forward(L, buffers, params, drop)
        rel(f"mean {n}", "mean", buffers[f"mean{l}"], f["mean"], GATE_BN, [f"raw{l}", f"mean{l}"])
        rel(f"invstd {n}", "invstd", buffers[f"invstd{l}"], f["invstd"], GATE_BN, [f"raw{l}", f"invstd{l}"])
        rel(f"act {n}", "act", _half(L, buffers[act_name(L)]), f["act"], GATE_BN, [f"raw{l}", act_name(L)] + dname)
        rows.append(Row(f"kinks {n}", f["kink_share"], KINK_SHARE, "kinks", [f"raw{l}", act_name(L)] + dname))
        P = f["xhat"].numel() // L.N
        rm = (1 - uo.BN_MOMENTUM) * params[L.bn_prefix + ".running_mean"].double() + uo.BN_MOMENTUM * f["mean"]
        rv = (1 - uo.BN_MOMENTUM) * params[L.bn_prefix + ".running_var"].double() + uo.BN_MOMENTUM * f["var"] * (P / max(P - 1, 1))
        rel(f"running_mean {n}", "running", buffers[f"running_mean{l}"], rm, GATE_BN, [f"raw{l}", f"running_mean{l}"])
        rel(f"running_var {n}", "running", buffers[f"running_var{l}"], rv, GATE_BN, [f"raw{l}", f"running_var{l}"])
    OUT = LAYERS[11]
    cat1 = buffers["cat1"].double()
    w11, b11 = params["deconv6.weight"].double(), params["deconv6.bias"].double()
    rel("mask", "raw", buffers["mask"], torch.sigmoid(_conv(OUT, cat1, w11, b11, hw[0])), GATE_RAW, ["cat1", "mask"])
    mask = buffers["mask"].double()
    want_loss, d_logit, decided = loss_stage(mask, mix, voc, loss_scale)
    rows.append(Row("loss", abs(float(loss) - want_loss) / want_loss, GATE_LOSS, "loss", ["mask", "loss"]))
    got = torch.where(decided, buffers["d_logit"].double(), d_logit)
    rel("d_logit", "d_logit", got, d_logit, GATE_DLOGIT, ["mask", "d_logit"])
    rows.append(Row("d_logit left out", 1.0 - decided.double().mean().item(), KINK_SHARE, "kinks", ["mask"]))

    # backward: deconv6 from d_logit_buf, then one composite stage per BatchNorm layer
    dl = buffers["d_logit"].double()
    dx_of = {}
    dx_of[11], dw = conv_backward(OUT, cat1, w11, dl)
    rel("dw deconv6", "dw out", grads["deconv6.weight"], dw, GATE_OUT_BWD, ["d_logit", "cat1", "deconv6.weight"])
    rel("db deconv6", "db out", grads["deconv6.bias"], dl.sum().reshape(1), GATE_OUT_BWD, ["d_logit", "deconv6.bias"])
    reads_of = {11: ["d_logit"]}
    for L in reversed(BN_LAYERS):
        l, n = L.index, L.name
        drop, dname = (drops[l - 6], [f"drop{l - 6}"]) if L.up else (None, [])
        bwd = layer_backward(L, fwd[l], buffers, params, drop, xs[l])
        reads = [dy_name(L), f"raw{l}", act_name(L)] + dname
        rel(f"dgamma {n}", "dgamma", grads[L.bn_prefix + ".weight"], bwd["dgamma"], GATE_BN_BWD, reads + [L.bn_prefix + ".weight"])
        rel(f"dbeta {n}", "dbeta", grads[L.bn_prefix + ".bias"], bwd["dbeta"], GATE_BN_BWD, reads + [L.bn_prefix + ".bias"])
        rel(f"dw {n}", "dw", grads[weight_key(L)], bwd["dw"], GATE_TWO, reads + [x_name(L), weight_key(L)])
        ratio = (grads[bias_key(L)].double().abs() / bwd["db_bound"].clamp_min(1e-300)).max().item()
        rows.append(Row(f"db {n} (|db| / bound, level {L.lout})", ratio, 1.0, "db", reads + [bias_key(L)]))
        dx_of[l], reads_of[l] = bwd["dx"], reads
    for k in range(1, 6):
        dec = 12 - k                                       # the decoder that reads cat[k]: deconv6 at level 1
        gate = GATE_OUT_BWD if k == 1 else GATE_TWO
        got = buffers[f"dcat{k}"]
        rel(f"dx dcat{k} decoder half ({LAYERS[dec].name})", "dx", got[:, :CH[k]], dx_of[dec][:, :CH[k]], gate,
            reads_of[dec] + [f"dcat{k}"])
        # the accumulate: what the decoder left in the skip half plus the data gradient of encoder k+1
        rel(f"dx dcat{k} skip half ({LAYERS[dec].name} + {LAYERS[k].name})", "dx skip", got[:, CH[k]:],
            dx_of[dec][:, CH[k]:] + dx_of[k], GATE_TWO, reads_of[dec] + reads_of[k] + [f"dcat{k}"])
    rel("dx dc6 (deconv1)", "dx", buffers["dc6"], dx_of[6], GATE_TWO, reads_of[6] + ["dc6"])
    return rows


# ----------------------------------------------------------------------------------------------------------------------
# a whole step on the CPU laid out as a workspace: the fake device of tests/test_train_stage_oracle.py
# ----------------------------------------------------------------------------------------------------------------------
def whole_step(np_state, mix, voc, dropout_masks=None, loss_scale=1.0, dtype=torch.float64):
    """unet_oracle's training step in `dtype` with every intermediate tapped (retain_grad on each tap), returned the way a
    workspace would show it: (buffers, grads, loss, taps).  `taps` keeps the tensors themselves (d_raw is taps[...raw].grad)."""
    state = uo.to_torch_state(np_state, dtype)
    keys = uo.param_keys(state)
    leaves = {k: state[k].detach().clone().requires_grad_(True) for k in keys}
    work = OrderedDict((k, leaves.get(k, v.clone())) for k, v in state.items())
    mix, voc = mix.to(dtype), voc.to(dtype)
    masks = [m.to(dtype) for m in dropout_masks] if dropout_masks else None
    taps = {}
    mask = uo.forward(work, mix, training=True, dropout_masks=masks, update_stats=True, taps=taps)
    logit = taps["deconv6.raw"]
    for t in taps.values():
        if t.requires_grad:
            t.retain_grad()
    loss = uo.l1_mask_loss(mask, mix, voc)
    (loss * loss_scale).backward()
    f32 = lambda t: t.detach().to(dtype)                   # buffers keep the run's own precision
    buffers = {"mask": f32(mask), "d_logit": f32(logit.grad)}
    for L in BN_LAYERS:
        raw = taps[L.name + ".raw"]
        buffers[f"raw{L.index}"] = f32(raw)
        buffers[f"mean{L.index}"] = f32(raw.mean((0, 2, 3)))
        buffers[f"invstd{L.index}"] = f32(torch.rsqrt(raw.var((0, 2, 3), unbiased=False) + uo.BN_EPS))
        buffers[f"running_mean{L.index}"] = f32(work[L.bn_prefix + ".running_mean"])
        buffers[f"running_var{L.index}"] = f32(work[L.bn_prefix + ".running_var"])
    for k in range(1, 6):
        d, s = taps[f"deconv{6 - k}.out"], taps[f"conv{k}.out"]
        buffers[f"cat{k}"] = f32(torch.cat([d, s], 1))
        buffers[f"dcat{k}"] = f32(torch.cat([d.grad, s.grad], 1))
    buffers["c6"], buffers["dc6"] = f32(taps["conv6.out"]), f32(taps["conv6.out"].grad)
    grads = {k: f32(leaves[k].grad) for k in keys}
    return buffers, grads, float(loss.detach()), taps
