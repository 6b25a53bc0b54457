"""Training at 512- and 2048-sample STFT windows (-m gpu): the transpose of `specific_istft` (`svs_istft_bwd_mask`) at
n_fft = 512 / 2048, the full objective (L1 + MR-STFT) through UNet.fwd_bwd on 256- and 1024-row tiles against a float64
oracle, the overlapped backward at those shapes, train.py --win_size end to end, and the rejections.  Tolerances are those
the 1024 tests use for the same quantities (test_gpu_ops.py: test_istft_any_hop, test_istft_bwd_mask; test_gpu_unet.py:
test_train_step_full_objective)."""
import functools
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import mrstft_oracle as mo
from oracle import stft_oracle as so
from oracle import unet_oracle as uo
from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd import data as svs_data
from svs_unet_pytorch_amd import train as svs_train
from svs_unet_pytorch_amd.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda"


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr()


def angles(seed, shape):
    return (synth.uniform(seed, int(np.prod(shape))) * 2 * np.pi - np.pi).astype(np.float32).reshape(shape)


# ------------------------------------------------------------------------------------------------
# svs_istft_bwd_mask at n_fft = 512 / 2048
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop_of", ["n/4", "n/2", "3n/4", "100"])
@pytest.mark.parametrize("n_fft", [512, 2048])
def test_istft_bwd_mask_windows(n_fft, hop_of, report):
    """The adjoint against autograd through torch.istft in float64 with a random weight vector (as test_istft_any_hop does at
    1024): mix = 1, mask = 1/2 (factor 1/4), alpha = 4.  T = 40 frames: two full blocks of 16 and a partial one."""
    hop = {"n/4": n_fft // 4, "n/2": n_fft // 2, "3n/4": 3 * n_fft // 4, "100": 100}[hop_of]
    B, T, R = 3, 40, n_fft // 2
    win = torch.hann_window(n_fft, dtype=torch.float64)
    m = synth.uniform(3, B * R * T).reshape(B, 1, R, T)
    a = angles(4, (B, 1, R, T))
    m64 = torch.nn.functional.pad(torch.from_numpy(m).double(), (0, 0, 1, 0)).requires_grad_(True)
    a64 = torch.nn.functional.pad(torch.from_numpy(a).double(), (0, 0, 1, 0))
    want = torch.istft(torch.polar(m64, a64).squeeze(1), n_fft=n_fft, hop_length=hop, win_length=n_fft, window=win, return_complex=False)
    assert want.shape == (B, hop * (T - 1))
    wgt = torch.from_numpy(synth.uniform(8, B * hop * (T - 1)).reshape(B, hop * (T - 1))).double() - 0.5
    (want * wgt).sum().backward()
    dmag = m64.grad[:, :, 1:, :]
    ones, half = torch.ones((B, 1, R, T), device=DEV), torch.full((B, 1, R, T), 0.5, device=DEV)
    d_logit = torch.zeros((B, 1, R, T), device=DEV)
    dw_d, a_d = wgt.float().to(DEV), torch.from_numpy(a).to(DEV)
    _lib.check(L().svs_istft_bwd_mask(dw_d.data_ptr(), a_d.data_ptr(), ones.data_ptr(), half.data_ptr(), d_logit.data_ptr(), 4.0, B, n_fft,
                                      hop, T, S()), "svs_istft_bwd_mask")
    tol = 2e-5 if n_fft % hop == 0 else 1e-4
    e = (d_logit.cpu().double() - dmag).abs().max().item() / dmag.abs().max().item()
    print(f"istft_bwd_mask n_fft={n_fft} hop={hop}: err {e:.3e} gate {5 * tol:.1e}")
    assert report(f"istft_bwd_mask n_fft={n_fft} hop={hop} vs autograd(torch.istft)", e, 5 * tol)


@pytest.mark.parametrize("n_fft", [512, 2048])
def test_istft_bwd_mask_windows_chain_rule(n_fft, report):
    """The fused chain rule of |S| = mask * mix on top of a non-zero d_logit, against the oracle's adjoint; and what the call
    must leave alone.  The tile layout has no padded frames of its own (a row is exactly `frames` long), so the allocation is
    padded as a whole: the call works on batch items 1..2 of a four-item buffer that also has a guard tail, and items 0 and 3,
    the tail, and every input must come back bit for bit."""
    hop, B, T, R = 3 * n_fft // 4, 2, 48, n_fft // 2
    n = B * R * T
    ang = angles(4, (B, 1, R, T))
    wgt = synth.uniform(8, B * hop * (T - 1)).reshape(B, 1, hop * (T - 1)).astype(np.float64) - 0.5
    mix = synth.uniform(10, n).reshape(B, 1, R, T)
    mask = synth.uniform(11, n).reshape(B, 1, R, T) * 0.8 + 0.1
    d0 = synth.uniform(12, n).reshape(B, 1, R, T) - 0.5
    guard = synth.uniform(13, 2 * R * T + 4096) - 0.5
    per = R * T
    buf = torch.from_numpy(np.concatenate([guard[:per], d0.reshape(-1), guard[per:]])).to(DEV)      # item 0 | items 1..2 | item 3 + tail
    before = buf.clone()
    dw = torch.from_numpy(wgt.astype(np.float32)).to(DEV)
    ang_d, mix_d, mask_d = torch.from_numpy(ang).to(DEV), torch.from_numpy(mix).to(DEV), torch.from_numpy(mask).to(DEV)
    _lib.check(L().svs_istft_bwd_mask(dw.data_ptr(), ang_d.data_ptr(), mix_d.data_ptr(), mask_d.data_ptr(), buf.data_ptr() + 4 * per, 0.37, B,
                                      n_fft, hop, T, S()), "svs_istft_bwd_mask")
    term = 0.37 * so.specific_istft_adjoint(wgt, ang, n_fft, hop) * mix * mask * (1 - mask)
    got = buf[per:per + n].cpu().numpy().reshape(B, 1, R, T)
    e = np.abs(got - (d0 + term)).max() / np.abs(term).max()
    print(f"istft_bwd_mask chain rule n_fft={n_fft}: err {e:.3e} gate 2.0e-05")
    assert report(f"istft_bwd_mask n_fft={n_fft} chain rule vs oracle adjoint", e, 2e-5)
    assert torch.equal(buf[:per], before[:per]) and torch.equal(buf[per + n:], before[per + n:])
    assert np.array_equal(ang_d.cpu().numpy(), ang) and np.array_equal(mix_d.cpu().numpy(), mix) and np.array_equal(mask_d.cpu().numpy(), mask)
    # one batch item alone gives the same rows (a block never reads or writes another item's)
    one = torch.from_numpy(d0[1:2].copy()).to(DEV)
    _lib.check(L().svs_istft_bwd_mask(dw[1:].data_ptr(), ang_d[1:].data_ptr(), mix_d[1:].data_ptr(), mask_d[1:].data_ptr(), one.data_ptr(), 0.37, 1,
                                      n_fft, hop, T, S()), "svs_istft_bwd_mask")
    assert np.array_equal(one.cpu().numpy(), got[1:2])


# ------------------------------------------------------------------------------------------------
# the full objective on 256- and 1024-row tiles
# ------------------------------------------------------------------------------------------------
CASES = [(4, 256, 128, 384),       # training shape at 512
         (2, 1024, 128, 1536),     # training shape at 2048
         (2, 1024, 16, 1024),      # hop = n_fft / 2 boundary, narrow tile
         (2, 256, 32, 128)]        # hop = n_fft / 4: the general overlap-add inverse
CASE_IDS = ["-".join(map(str, c)) for c in CASES]


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    B, H, W, _ = case
    mix, voc = synth.tiles(B, H, W, first_tile=800)
    return mix, voc, angles(30, (B, 1, H, W)), angles(31, (B, 1, H, W)), synth.dropout_masks(B, seed=5, step=0)


def specific_istft64(magnitude, phase, n_fft, hop):
    """train.py:33-60 on torch ops for any window: (B,1,n_fft/2,T) magnitude / angle -> (B,1,hop*(T-1)), DC row padded back."""
    m = torch.nn.functional.pad(magnitude, (0, 0, 1, 0))
    a = torch.nn.functional.pad(phase, (0, 0, 1, 0))
    w = torch.hann_window(n_fft, dtype=magnitude.dtype)
    return torch.istft(torch.polar(m, a).squeeze(1), n_fft=n_fft, hop_length=hop, win_length=n_fft, window=w, return_complex=False).unsqueeze(1)


@functools.lru_cache(maxsize=None)
def oracle_full(case):
    """(l1, mr, grads) of the reference's objective (train.py:274-299) in float64: oracle U-Net in training mode, the two L1
    terms, the MR-STFT loss of the two waveforms re-synthesised at the tiles' own window."""
    B, H, W, hop = case
    mix_np, voc_np, mph, vph, masks_np = case_inputs(case)
    state = uo.to_torch_state(synth.closed_form_state(trained_stats=False), torch.float64)
    keys = uo.param_keys(state)
    leaves = {k: state[k].detach().clone().requires_grad_(True) for k in keys}
    work = OrderedDict((k, leaves.get(k, v)) for k, v in state.items())
    mix, voc = torch.from_numpy(mix_np).double(), torch.from_numpy(voc_np).double()
    mask = uo.forward(work, mix, training=True, dropout_masks=[torch.from_numpy(m).double() for m in masks_np], update_stats=True)
    pred = mask * mix
    l1 = torch.nn.functional.l1_loss(pred, voc) + torch.nn.functional.l1_loss((1 - mask) * mix, torch.clamp(mix - voc, min=0.0))
    mr = mo.mrstft_loss(specific_istft64(pred, torch.from_numpy(mph).double(), 2 * H, hop),
                        specific_istft64(voc, torch.from_numpy(vph).double(), 2 * H, hop))
    (mo.ALPHA_L1 * l1 + mo.ALPHA_MR * mr).backward()
    return float(l1.detach()), float(mr.detach()), {k: leaves[k].grad.detach() for k in keys}


def make_model(masks_np):
    m = UNet()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state(trained_stats=False).items()}, strict=True)
    m = m.to(DEV).train()
    m.set_dropout_masks([torch.from_numpy(x) for x in masks_np])
    m.optim.zero_grad()
    return m


def before_batchnorm(n):
    return n.endswith(".0.bias") and n.startswith("conv") or (n.startswith("deconv") and n.endswith(".bias") and n != "deconv6.bias")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_full_objective_windows(case, report):
    """UNet.fwd_bwd with the phase tiles and `hop=` at H = 256 / 1024 against the float64 oracle: both loss parts and every
    parameter gradient.  Reference arithmetic alone (torch fp32 against fp64 on this oracle) is at most 2.5e-3 rel-L2 on a
    gradient (conv6.0.weight at (2, 1024, 128)), 6.3e-6 on the MR part and 8e-8 on the L1 part."""
    B, H, W, hop = case
    mix_np, voc_np, mph, vph, masks_np = case_inputs(case)
    l1_o, mr_o, grads_o = oracle_full(case)
    to = lambda a: torch.from_numpy(a).to(DEV)
    model = make_model(masks_np)
    l1 = model.fwd_bwd(to(mix_np), to(voc_np), loss_scale=mo.ALPHA_L1, mix_phase=to(mph), voc_phase=to(vph), alpha_mr=mo.ALPHA_MR, hop=hop)
    tag = f"full objective {case}"
    e_l1, e_mr = abs(l1.item() - l1_o) / l1_o, abs(model.last_mr_loss.item() - mr_o) / mr_o
    fused = {n: p.grad.detach().cpu().double() for n, p in model.named_parameters()}
    errs = {n: (fused[n] - gw).norm().item() / max(gw.norm().item(), 1e-12) for n, gw in grads_o.items() if not before_batchnorm(n)}
    worst = max(errs, key=errs.get)
    print(f"{tag}: L1 rel {e_l1:.3e} (gate 1e-5)  MR rel {e_mr:.3e} (gate 1e-4)  worst grad rel-L2 {errs[worst]:.3e} {worst} (gate 2e-2)")
    assert report(f"{tag}: L1 part", e_l1, 1e-5)
    assert report(f"{tag}: MR-STFT part", e_mr, 1e-4)
    for n, e in errs.items():
        assert report(f"{tag} grad {n} rel-L2", e, 2e-2), (n, e)
    # the MR term really contributes: gradients differ from the L1-only step
    model2 = make_model(masks_np)
    model2.fwd_bwd(to(mix_np), to(voc_np), loss_scale=mo.ALPHA_L1)
    assert model2.last_mr_loss is None
    d = (model2._gflat - model._gflat).norm().item() / model._gflat.norm().item()
    assert d > 1e-3, d


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[CASE_IDS[0], CASE_IDS[2]])
def test_overlapped_equals_fused_at_windows(case):
    """fwd_bwd and fwd_bwd_overlapped (driven without RCCL, as test_split_backward_equals_fused drives it) give the same
    losses and flat gradients bit for bit at 256- and 1024-row tiles with the full objective."""
    B, H, W, hop = case
    mix_np, voc_np, mph, vph, masks_np = case_inputs(case)
    to = lambda a: torch.from_numpy(a).to(DEV)

    class FakeSync:
        overlap = True

        def __init__(self):
            self.calls = 0

        def reduce_async(self, sl):
            self.calls += 1

            class H_:
                def wait(self_inner):
                    return None
            return H_()

    a, b = make_model(masks_np), make_model(masks_np)
    kw = dict(mix_phase=to(mph), voc_phase=to(vph), alpha_mr=mo.ALPHA_MR, hop=hop)
    la = a.fwd_bwd(to(mix_np), to(voc_np), mo.ALPHA_L1, **kw)
    sync = FakeSync()
    lb, handles = b.fwd_bwd_overlapped(to(mix_np), to(voc_np), mo.ALPHA_L1, sync, **kw)
    torch.cuda.synchronize()
    assert len(handles) == 4 and sync.calls == 4
    assert la.item() == lb.item() and a.last_mr_loss.item() == b.last_mr_loss.item()
    assert np.isfinite(la.item()) and a._gflat.abs().max().item() > 0
    assert torch.equal(a._gflat, b._gflat) and torch.equal(a._bn_flat, b._bn_flat)


# ------------------------------------------------------------------------------------------------
# train.py --win_size 512
# ------------------------------------------------------------------------------------------------
SR = 8192


def _write_song(folder, idx, n):
    from scipy.io import wavfile
    os.makedirs(folder, exist_ok=True)
    voc = synth.audio(n - 1000, 2 * idx) * 0.3
    mix = synth.audio(n, 2 * idx + 1) * 0.5
    mix[: voc.size] += voc
    wavfile.write(os.path.join(folder, "mixture.wav"), SR, mix.astype(np.float32))
    wavfile.write(os.path.join(folder, "vocals.wav"), SR, voc.astype(np.float32))
    return n


def test_train_cli_at_512(tmp_path, monkeypatch, capsys):
    """wav -> data.py to_spec --win_size 512 -> train.py --win_size 512 (two epochs, full objective, validation) -> the
    checkpoint's keys -> separate.py --win_size 512 on it; then the same folder under --win_size 1024 and the checkpoint under --win_size 2048 are refused."""
    monkeypatch.chdir(tmp_path)
    src, spec_dir = tmp_path / "wav", tmp_path / "spec"
    lengths = [_write_song(str(src / name), i, n) for i, (name, n) in enumerate((("songA", 60000), ("songB", 52000)))]
    svs_data.main(["--src", str(src), "--tar", str(spec_dir), "--direction", "to_spec", "--win_size", "512", "--hop_size", "384"])
    names = sorted(f for f in os.listdir(spec_dir / "mixture") if f.endswith("_spec.npy"))
    assert len(names) == 2
    for name, n in zip(names, lengths):
        for track in ("mixture", "vocal"):
            assert np.load(spec_dir / track / name).shape == (257, 1 + n // 384)
            assert np.load(spec_dir / track / name.replace("_spec", "_phase")).shape == (257, 1 + n // 384)

    initial = []

    class Spy(UNet):                       # the parameters train.py starts from
        def __init__(self):
            super().__init__()
            initial.append({k: v.detach().clone() for k, v in self.state_dict().items()})
    monkeypatch.setattr(svs_train, "UNet", Spy)
    common = ["--train_folder", str(spec_dir), "--valid_folder", str(spec_dir), "--batch_size", "4", "--val_interval", "1"]
    svs_train.main(common + ["--label", "w512", "--epoch", "2", "--load_path", "none.pth", "--win_size", "512", "--hop_size", "384"])
    out = capsys.readouterr().out
    objective = [l for l in out.splitlines() if l.startswith("Objective:")]
    assert len(objective) == 1 and "MR-STFT" in objective[0], objective
    lines = open(tmp_path / "LOG" / "log_w512.txt").read().split()
    values = [float(x) for x in lines if x != "Val"]
    assert len([x for x in lines if x == "Val"]) == 2 and len(values) == 4 and all(np.isfinite(v) and v > 0 for v in values)
    ck = torch.load(tmp_path / "CKPT" / "svs_w512.pth", map_location="cpu")
    assert ck["win_size"] == 512 and ck["hop_size"] == 384 and ck["epoch"] == 2 and len(ck["model_state_dict"]) == 79
    best = torch.load(tmp_path / "CKPT" / "svs_best_w512.pth", map_location="cpu")
    assert best["win_size"] == 512 and best["hop_size"] == 384
    assert len(initial) == 1
    moved = (ck["model_state_dict"]["conv1.0.weight"] - initial[0]["conv1.0.weight"]).abs().max().item()
    assert moved > 1e-4 and all(torch.isfinite(v).all() for v in ck["model_state_dict"].values() if v.is_floating_point())

    # separate.py at the same geometry takes the checkpoint (its extra keys are ignored) and writes a file of the source's length
    from scipy.io import wavfile
    from svs_unet_pytorch_amd import separate as svs_separate
    svs_separate.main(["--model_path", str(tmp_path / "CKPT" / "svs_w512.pth"), "--src", str(src / "songA" / "mixture.wav"),
                       "--tar", str(tmp_path / "sep.wav"), "--win_size", "512", "--hop_size", "384"])
    rate, y = wavfile.read(tmp_path / "sep.wav")
    assert rate == SR and y.shape == (lengths[0],) and y.dtype == np.int16 and np.abs(y).max() > 0

    # the same folder under the default window: refused by the row check, before any step
    with pytest.raises(SystemExit) as ei:
        svs_train.main(common + ["--label", "bad", "--epoch", "1", "--load_path", "none.pth", "--win_size", "1024"])
    msg = str(ei.value)
    assert "257 rows" in msg and "--win_size 512 would match" in msg and "0000_songA_spec.npy" in msg, msg
    assert not [f for f in os.listdir(tmp_path / "CKPT") if "bad" in f] and not os.path.exists(tmp_path / "LOG" / "log_bad.txt")
    # the 512 checkpoint under another window: refused by the checkpoint's keys
    with pytest.raises(SystemExit) as ei:
        svs_train.main(common + ["--label", "res", "--epoch", "3", "--load_path", str(tmp_path / "CKPT" / "svs_w512.pth"), "--win_size", "2048",
                                 "--hop_size", "1536"])
    msg = str(ei.value)
    assert "trained at --win_size 512 --hop_size 384" in msg and "--win_size 2048" in msg, msg
    assert not [f for f in os.listdir(tmp_path / "CKPT") if "res" in f]
    assert len(initial) == 1               # neither refused run built a model


# ------------------------------------------------------------------------------------------------
# rejections
# ------------------------------------------------------------------------------------------------
def test_rejections_train_windows():
    """Sizes that are not built and tiles too short for the MR-STFT loss are errors of the entry point itself; every buffer
    is large enough for the largest accepted size, and none of them changes."""
    B, T = 2, 16
    big = B * 2048 * T
    bufs = [torch.full((big,), 0.25, device=DEV) for _ in range(5)]
    for n_fft in (256, 768, 4096):
        with pytest.raises(_lib.SvsError, match="n_fft"):
            _lib.check(L().svs_istft_bwd_mask(*(b.data_ptr() for b in bufs), 1.0, B, n_fft, max(n_fft // 2, 1), T, S()), "svs_istft_bwd_mask")
    with pytest.raises(_lib.SvsError, match="hop"):
        _lib.check(L().svs_istft_bwd_mask(*(b.data_ptr() for b in bufs), 1.0, B, 512, 513, T, S()), "svs_istft_bwd_mask")
    torch.cuda.synchronize()
    assert all(torch.equal(b, torch.full_like(b, 0.25)) for b in bufs)

    model = UNet().to(DEV).train()
    model.set_dropout_masks([])
    model._attach_grads()
    flat0, bn0 = model._flat.clone(), model._bn_flat.clone()

    def call(H, W, hop):
        n = B * 1024 * 128                                   # tiles of the largest accepted size
        t = [torch.full((n,), 0.5, device=DEV) for _ in range(4)]
        ws = torch.empty(int(L().svs_unet_train_workspace_bytes(B, 1024, 128)) + 4096, dtype=torch.uint8, device=DEV)
        mr = torch.empty(int(L().svs_unet_train_mr_workspace_bytes(B, 128, 2048)) + 4096, dtype=torch.uint8, device=DEV)
        losses = torch.full((2,), -1.0, device=DEV)
        rc = L().svs_unet_train_fwd_loss_mr(model._flat.data_ptr(), model._bn_flat.data_ptr(), model._nbt_flat.data_ptr(), t[0].data_ptr(),
                                            t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), None, B, H, W, hop, 1.0, 1.0, None,
                                            losses.data_ptr(), ws.data_ptr(), ws.numel(), mr.data_ptr(), mr.numel(), S())
        torch.cuda.synchronize()
        assert losses.tolist() == [-1.0, -1.0]               # nothing ran
        _lib.check(rc, "svs_unet_train_fwd_loss_mr")

    with pytest.raises(_lib.SvsError, match="H = 300"):
        call(300, 128, 384)
    with pytest.raises(_lib.SvsError, match=r"W = 4.*hop = 384"):
        call(256, 4, 384)                                    # hop * (W - 1) = 1152 <= 2048
    with pytest.raises(_lib.SvsError, match="hop"):
        call(256, 128, 513)
    assert torch.equal(model._flat, flat0) and torch.equal(model._bn_flat, bn0)      # no running statistics were updated
