"""What the benchmark tools share: the spread of a list of times, two callables timed in alternation with HIP events, the torch copy
that is a kernel's yardstick, and the U-Net with the closed-form checkpoint."""
import statistics

import numpy as np
import torch


def stats(v):
    return dict(median_ms=round(statistics.median(v), 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5))


def timed_pair(fa, fb, reps, warmup=5):
    """Median and spread (ms) of fa and fb, alternating a / b inside every repetition."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for i in range(reps):                                        # a b, b a, a b, ...: neither side always finds the other's cache lines
        first, second = (fa, fb) if i % 2 == 0 else (fb, fa)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        first()
        ev[1].record()
        second()
        ev[2].record()
        torch.cuda.synchronize()
        t1, t2 = ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])
        ta.append(t1 if i % 2 == 0 else t2)
        tb.append(t2 if i % 2 == 0 else t1)
    return stats(ta), stats(tb)


def timed(fn, reps, warmup=2):
    """Median and spread (ms) of fn."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return stats(t)


def copy_of(nbytes):
    """A torch device copy that moves `nbytes` in all: nbytes / 2 read and nbytes / 2 written."""
    src = torch.rand(nbytes // 8, device="cuda")
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def closed_form_model(device="cuda"):
    """The U-Net with synth.closed_form_state(), on `device`, in eval mode."""
    from svs_unet_pytorch_amd import synth
    from svs_unet_pytorch_amd.model import UNet
    model = UNet()
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state().items()})
    return model.to(device).eval()
