"""The forks of the side stream are the producing launches themselves (their stop events), not markers behind them: the
side stream must still see every tensor it reads complete, and the main stream must still see the side stream's results at
the join.  A fork that released the side stream too early, or a join that released the main stream too early, changes the
weight gradients and with them everything a train step leaves behind, so the two-stream schedule is compared bit for bit with
the same steps on ONE stream (TRAIN_ONE_STREAM = 1: no forks, no joins), through the fused call and through the split backward."""
import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import synth
from svs_unet_pytorch_amd.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, W, STEPS = 16, 64, 16, 3
NAMES = ("parameters", "Adam m", "Adam v", "BatchNorm buffers", "flat gradient")


def make_model():
    m = UNet()
    sd = {k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state(trained_stats=False).items()}
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).train()


class LocalSync:
    """`grad_sync` hook of a single rank: nothing to exchange, so `train_step` goes through `fwd_bwd_overlapped` (forward + loss,
    four `svs_unet_train_bwd_part` calls, `svs_unet_train_bwd_sync` after each) and the gradients stay as computed."""
    overlap = True

    def __init__(self):
        self.pieces = 0

    def reduce_async(self, sl):
        self.pieces += 1

        class Done:
            def wait(self):
                return None
        return Done()


def run_steps(mix, voc, grad_sync=None):
    m = make_model()                                   # generated dropout masks: the same seed and step counter in every run
    losses = [m.train_step(mix, voc, loss_scale=166.66, grad_sync=grad_sync).item() for _ in range(STEPS)]
    torch.cuda.synchronize()
    return losses, (m._flat.clone(), m.optim._m.clone(), m.optim._v.clone(), m._bn_flat.clone(), m._gflat.clone())


@pytest.fixture(scope="module")
def tiles():
    mix_np, voc_np = synth.tiles(B, H, W, first_tile=3100)
    return torch.from_numpy(mix_np).to(DEV), torch.from_numpy(voc_np).to(DEV)


@pytest.fixture(scope="module")
def one_stream(tiles):
    """The reference state: the three steps with every launch on the caller's stream."""
    from svs_unet_pytorch_amd import _lib
    _lib.tuning("TRAIN_ONE_STREAM", 1)
    try:
        ref = run_steps(*tiles)
    finally:
        _lib.tuning("*", -1)
    assert all(np.isfinite(ref[0]))
    return ref


def test_two_streams_equal_one_stream(tiles, one_stream):
    losses, state = run_steps(*tiles)
    assert losses == one_stream[0], (losses, one_stream[0])
    for got, want, name in zip(state, one_stream[1], NAMES):
        assert torch.equal(got, want), name


def test_split_backward_equals_one_stream(tiles, one_stream):
    sync = LocalSync()
    losses, state = run_steps(*tiles, grad_sync=sync)
    assert sync.pieces == 4 * STEPS
    assert losses == one_stream[0], (losses, one_stream[0])
    for got, want, name in zip(state, one_stream[1], NAMES):
        assert torch.equal(got, want), name
