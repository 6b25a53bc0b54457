"""The optimiser options through the model (FusedAdam.weight_decay / max_grad_norm / ema_decay, UNet.ema_weights,
UNet.ema_state_dict, checkpoints), at the smallest geometry the network tests use: 64 x 16 tiles, B = 2.

The three-step check applies the float64 definition (clip_grad_norm_'s coefficient, AdamW's decoupled decay, Adam, the EMA
recurrence) to the float32 state from before each step and the step's own device gradient, which `_gflat` still holds after
the step: one step of rounding per comparison, gated at the 1e-6 absolute of the Adam check of tests/test_gpu_ops.py."""
import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import synth
from svs_unet_pytorch_amd.model import ALPHA_L1, UNet

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, W = 2, 64, 16
LR, WD, D, B1, B2, EPS = 1e-3, 1e-2, 0.9, 0.9, 0.999, 1e-8


def make_model(**options):
    m = UNet()
    sd = {k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state(trained_stats=False).items()}
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    for k, v in options.items():
        assert hasattr(m.optim, k)
        setattr(m.optim, k, v)
    return m


@pytest.fixture(scope="module")
def tiles():
    mix_np, voc_np = synth.tiles(B, H, W, first_tile=3100)
    return torch.from_numpy(mix_np).to(DEV), torch.from_numpy(voc_np).to(DEV)


@pytest.fixture(scope="module")
def max_norm(tiles):
    """Half the float64 norm of the first step's device gradient: the clip is then certainly active on that step."""
    m = make_model()
    m.optim.zero_grad()
    m.fwd_bwd(*tiles, loss_scale=ALPHA_L1)
    return 0.5 * float(m._gflat.double().norm())


def state_of(m):
    return {"p": m._flat.clone(), "m": m.optim._m.clone(), "v": m.optim._v.clone(), "bn": m._bn_flat.clone(),
            "nbt": m._nbt_flat.clone(), "ema": None if m._ema_flat is None else m._ema_flat.clone()}


def assert_same_state(a, b):
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), k


def test_three_steps_match_float64_definition(tiles, max_norm, report):
    m = make_model(weight_decay=WD, max_grad_norm=max_norm, ema_decay=D)
    m.start_ema()
    clipped = 0
    for t in range(1, 4):
        before = {k: v.double().cpu() for k, v in state_of(m).items() if k in ("p", "m", "v", "ema")}
        loss = m.train_step(*tiles, loss_scale=ALPHA_L1)
        assert np.isfinite(loss.item())
        g = m._gflat.double().cpu()                       # still this step's gradient
        norm = float(g.norm())
        coef = min(1.0, max_norm / (norm + 1e-6))
        clipped += coef < 1.0
        g = g * coef
        p = before["p"] * (1.0 - LR * WD)
        mm = B1 * before["m"] + (1 - B1) * g
        vv = B2 * before["v"] + (1 - B2) * g * g
        p = p - (LR / (1 - B1 ** t)) * mm / (vv.sqrt() / np.sqrt(1 - B2 ** t) + EPS)
        ema = D * before["ema"] + (1 - D) * p
        stats = m.optim_stats.cpu()
        print(f"step {t}: norm {norm:.6e} device {stats[0].item():.6e} coef {coef:.4f} device {stats[1].item():.4f}")
        assert abs(stats[0].item() - norm) <= 1e-12 * norm and abs(stats[1].item() - coef) <= 1e-12
        assert report(f"optim model step {t} param", (m._flat.double().cpu() - p).abs().max().item(), 1e-6)
        assert report(f"optim model step {t} ema", (m._ema_flat.double().cpu() - ema).abs().max().item(), 1e-6)
    assert clipped >= 1
    stats = m.optim_stats.cpu()
    assert stats[2].item() == clipped and stats[3].item() == 0.0
    assert m.optim._step == 3


class LocalSync:
    """`grad_sync` hook of a single rank that exchanges nothing: with `overlap` the step goes through `fwd_bwd_overlapped`."""

    def __init__(self, overlap):
        self.overlap = overlap

    def __call__(self, flat_grad):
        return None

    def reduce_async(self, sl):
        class Done:
            def wait(self):
                return None
        return Done()


def test_norm_follows_the_exchange_in_both_paths(tiles, max_norm):
    """Under data parallelism the norm is that of grad_scale * (the exchanged flat gradient), taken in FusedAdam.step: after the
    plain hook and after the last handle of the overlapped one.  grad_scale = 1/2 as on two ranks; both paths leave the same bits."""
    runs = []
    for overlap in (False, True):
        m = make_model(weight_decay=WD, max_grad_norm=0.25 * max_norm, ema_decay=D)
        m.optim.grad_scale = 0.5
        for _ in range(2):
            m.train_step(*tiles, loss_scale=ALPHA_L1, grad_sync=LocalSync(overlap))
        stats = m.optim_stats.cpu()
        want = 0.5 * float(m._gflat.double().norm())
        assert abs(stats[0].item() - want) <= 1e-12 * want and stats[2].item() >= 1.0
        runs.append(state_of(m))
    assert_same_state(*runs)


def test_defaults_are_todays_step(tiles):
    runs = []
    for options in ({}, {"weight_decay": 0.0, "max_grad_norm": 0.0, "ema_decay": 0.0}):
        m = make_model(**options)
        for _ in range(5):
            m.train_step(*tiles, loss_scale=ALPHA_L1)
        torch.cuda.synchronize()
        assert m._ema_flat is None and m.optim_stats.cpu().abs().sum().item() == 0.0      # neither kernel ran
        runs.append(state_of(m))
    assert_same_state(*runs)


def test_ema_weights_swap(tiles, max_norm):
    mix = tiles[0]
    m = make_model(weight_decay=WD, max_grad_norm=max_norm, ema_decay=D)
    with pytest.raises(RuntimeError, match="no EMA"):
        with m.ema_weights():
            pass
    for _ in range(3):
        m.train_step(*tiles, loss_scale=ALPHA_L1)
    m.eval()
    with torch.no_grad():
        live = m(mix).clone()                             # (folds the live weights: the cache must follow the swaps)
        flat_before, ema_before = m._flat.clone(), m._ema_flat.clone()
        sd = m.ema_state_dict()
        assert list(sd) == list(m.state_dict())
        with m.ema_weights():
            assert torch.equal(m._flat, ema_before) and torch.equal(m._ema_flat, flat_before)
            inside = m(mix).clone()
            sd_inside = m.ema_state_dict()
        other = UNet()
        other.load_state_dict(sd, strict=True)
        other = other.to(DEV).eval()
        want = other(mix)
        assert torch.equal(inside, want)
        assert not torch.equal(inside, live)
        assert all(torch.equal(sd[k], sd_inside[k]) for k in sd)
        assert torch.equal(m._flat, flat_before) and torch.equal(m._ema_flat, ema_before)
        assert torch.equal(m(mix), live)


def test_checkpoint_round_trip(tiles, max_norm, tmp_path):
    options = dict(weight_decay=WD, max_grad_norm=max_norm, ema_decay=D)
    a = make_model(**options)
    for _ in range(2):
        a.train_step(*tiles, loss_scale=ALPHA_L1)
    path = str(tmp_path / "ckpt.pth")
    a.save(path)
    state = torch.load(path, map_location="cpu")
    assert "ema_state_dict" in state and state["ema_decay"] == D and list(state["ema_state_dict"]) == list(state["model_state_dict"])
    a.train_step(*tiles, loss_scale=ALPHA_L1)
    b = make_model(**options)
    b.load(path)
    assert b._ema_flat is not None and b.optim._step == 2
    b.train_step(*tiles, loss_scale=ALPHA_L1)
    torch.cuda.synchronize()
    assert_same_state(state_of(a), state_of(b))
    assert not torch.equal(a._flat, a._ema_flat)
