"""svs_grad_norm and svs_adamw_step through the C ABI (csrc/optim.hip): the global gradient norm and its clip coefficient on
device-resident scalars, and the Adam update with decoupled weight decay, clipping, the skip on a non-finite gradient and the
EMA of the weights.

Bounds.  The norm is a double sum of n non-negative terms: relative error at most n * 2^-52 (2^-53 per addition, doubled)
against float64 numpy on the same float32 data.  The update is gated like the existing Adam check of tests/test_gpu_ops.py --
parameters (and the EMA) to 1e-6 absolute, both moments to 1e-5 relative, against float64 torch -- and bit for bit against
svs_adam_step where the two must coincide."""
import math

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
NORM_SIZES = [1, 63, 64, 65, 255, 256, 257, 1025, 10007, 3 * (1 << 20) + 7]     # the last: three passes of the 1024-block grid
OFFSETS = [0, 1, 3]                                                              # floats into the allocation


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr()


def rnd(shape, seed, lo=-1.0, hi=1.0):
    n = int(np.prod(shape))
    return torch.from_numpy((synth.uniform(seed, n) * (hi - lo) + lo).reshape(shape).astype(np.float32))


def relerr(got, want):
    want = want.double()
    return ((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


def norm_ws(n):
    return torch.empty(int(L().svs_grad_norm_workspace_bytes(n)), dtype=torch.uint8, device=DEV)


def grad_norm(g, max_norm=0.0, grad_scale=1.0, stats=None):
    """Runs svs_grad_norm on the device tensor (or view) g; returns the stats array as numpy float64[4] and the device array."""
    n = g.numel()
    if stats is None:
        stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    ws = norm_ws(n)
    _lib.check(L().svs_grad_norm(g.data_ptr(), n, grad_scale, max_norm, stats.data_ptr(), ws.data_ptr(), ws.numel(), S()), "svs_grad_norm")
    return stats.cpu().numpy(), stats


def coef_ok(got, max_norm, norm):
    """The device's max_norm / (norm + 1e-6) against the host's: one double addition and one division, two ulps allowed."""
    want = max_norm / (norm + 1e-6)
    return abs(got - want) <= 2.0 ** -51 * want


def exact_norm(x32):
    """sqrt(sum x^2) of float32 data: squares and sum in extended precision, rounded once to float64."""
    x = x32.astype(np.longdouble)
    return float(np.sqrt(np.sum(x * x)))


@pytest.fixture(scope="module")
def norm_data():
    rng = np.random.default_rng(20261020)
    return {n: rng.uniform(-1.0, 1.0, n).astype(np.float32) for n in NORM_SIZES}


@pytest.mark.parametrize("n", NORM_SIZES)
def test_norm_matches_float64(norm_data, report, n):
    host = norm_data[n]
    want = exact_norm(host)
    bound = n * 2.0 ** -52
    for off in OFFSETS:
        buf = torch.zeros(n + 8, device=DEV)
        g = buf[off:off + n]
        g.copy_(torch.from_numpy(host))
        assert g.data_ptr() % 16 == (4 * off) % 16
        st, _ = grad_norm(g)
        st2, _ = grad_norm(g)
        err = abs(st[0] - want) / want
        print(f"n={n} offset={off}: norm {st[0]!r} want {want!r} rel err {err:.3e} bound {bound:.3e}")
        assert report(f"grad_norm n={n} offset={off}", err, bound)
        assert st[0].tobytes() == st2[0].tobytes(), "two runs differ"
        assert st[1] == 1.0 and st[2] == 0.0 and st[3] == 0.0          # max_norm = 0: never clips
        assert buf[:off].abs().sum().item() == 0.0 and buf[off + n:].abs().sum().item() == 0.0


def test_norm_grad_scale(norm_data):
    host = norm_data[10007]
    g = torch.from_numpy(host).to(DEV)
    want = exact_norm(host)
    for gs in (0.25, 1.0 / 3.0):
        st, _ = grad_norm(g, grad_scale=gs)
        assert abs(st[0] - float(np.float32(gs)) * want) / want <= (10007 + 1) * 2.0 ** -52


def test_norm_large_entries():
    """Entries of 3e19: their squares overflow float32 (9e38 > 3.4e38), not double."""
    n = 1025
    host = np.full(n, 3e19, np.float32)
    host[1::2] *= -1
    st, _ = grad_norm(torch.from_numpy(host).to(DEV), max_norm=1.0)
    want = exact_norm(host)
    assert math.isfinite(st[0]) and abs(st[0] - want) / want <= n * 2.0 ** -52
    assert coef_ok(st[1], 1.0, st[0]) and st[2] == 1.0 and st[3] == 0.0


def test_norm_zero_gradient():
    st, _ = grad_norm(torch.zeros(1025, device=DEV), max_norm=1.0)
    assert st[0] == 0.0 and st[1] == 1.0 and st[2] == 0.0 and st[3] == 0.0


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_norm_non_finite(norm_data, bad):
    host = norm_data[10007].copy()
    host[5003] = bad
    st, dev = grad_norm(torch.from_numpy(host).to(DEV), max_norm=1.0)
    assert not math.isfinite(st[0]) and st[1] == 0.0 and st[2] == 0.0 and st[3] == 1.0
    st, _ = grad_norm(torch.from_numpy(host).to(DEV), max_norm=0.0, stats=dev)      # clipping off: still a skip
    assert st[1] == 0.0 and st[3] == 2.0


def test_norm_counts_clipped_calls_only(norm_data):
    host = norm_data[10007]
    g = torch.from_numpy(host).to(DEV)
    norm = exact_norm(host)
    stats = None
    for max_norm, want_clip in ((norm / 3, True), (norm * 0.999, True), (norm * 2, False), (0.0, False), (norm / 3, True)):
        st, stats = grad_norm(g, max_norm=max_norm, stats=stats)
        if want_clip:
            assert coef_ok(st[1], max_norm, st[0]) and st[1] < 1.0
        else:
            assert st[1] == 1.0
    assert st[2] == 3.0 and st[3] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# the update
# ---------------------------------------------------------------------------------------------------------------------------
def adam(p, g, m, v, step, gs, lr=1e-3):
    _lib.check(L().svs_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, 0.9, 0.999, 1e-8, step, gs, S()),
               "svs_adam_step")


def adamw(p, g, m, v, step, gs, wd=0.0, stats=None, ema=None, d=0.0, lr=1e-3):
    _lib.check(L().svs_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, 0.9, 0.999, 1e-8, step, gs, wd,
                                  None if stats is None else stats.data_ptr(), None if ema is None else ema.data_ptr(), d, S()),
               "svs_adamw_step")


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def update_state(n):
    p = rnd((n,), 96).to(DEV)
    g = rnd((n,), 97, -0.01, 0.01).to(DEV)
    m = rnd((n,), 98, -0.003, 0.003).to(DEV)
    v = (rnd((n,), 99, 0.0, 0.01) ** 2).to(DEV)
    return p, g, m, v


@pytest.mark.parametrize("n", [10007, (1 << 20) + 4099])          # one pass of the grid; a stride loop that runs twice
def test_update_bitwise_against_adam(n):
    p, g, m, v = update_state(n)
    grad_scale = 0.5
    norm = grad_scale * exact_norm(g.cpu().numpy())
    st, stats = grad_norm(g, max_norm=norm / 3, grad_scale=grad_scale)
    assert 0.3 < st[1] < 0.37                                        # the norm is about three times max_norm
    gs = float(np.float32(grad_scale) * np.float32(st[1]))
    pa, ma, va = p.clone(), m.clone(), v.clone()
    adam(pa, g, ma, va, 7, gs)
    pw, mw, vw = p.clone(), m.clone(), v.clone()
    adamw(pw, g, mw, vw, 7, grad_scale, stats=stats)
    assert same_bits(pw, pa) and same_bits(mw, ma) and same_bits(vw, va)
    assert not same_bits(pw, p)
    # stats = NULL: svs_adam_step at the plain grad_scale
    pa, ma, va = p.clone(), m.clone(), v.clone()
    adam(pa, g, ma, va, 7, grad_scale)
    pn, mn, vn = p.clone(), m.clone(), v.clone()
    adamw(pn, g, mn, vn, 7, grad_scale)
    assert same_bits(pn, pa) and same_bits(mn, ma) and same_bits(vn, va)
    assert not same_bits(pn, pw)                                     # (the clip changed the step)


def test_update_matches_float64_definition(report):
    """Three steps at the shape and data of the Adam check of tests/test_gpu_ops.py against float64 clip_grad_norm_ +
    torch.optim.AdamW + the EMA recurrence."""
    n, lr, wd, d = 10007, 1e-3, 1e-2, 0.9
    p0, gs = rnd((n,), 96), [rnd((n,), 97 + i, -0.01, 0.01) for i in range(3)]
    norms = sorted(float(g.double().norm()) for g in gs)
    max_norm = 0.5 * (norms[1] + norms[2])                           # between the two largest: one step clips, two do not
    pt = p0.clone().double().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=lr, weight_decay=wd)
    ema_t = p0.clone().double()
    pd, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ema = pd.clone()
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    clipped = []
    for i, g in enumerate(gs):
        pt.grad = g.double().clone()
        total = float(torch.nn.utils.clip_grad_norm_([pt], max_norm))
        clipped.append(total > max_norm)
        opt.step()
        ema_t = d * ema_t + (1 - d) * pt.detach()
        gd = g.to(DEV)
        grad_norm(gd, max_norm=max_norm, stats=stats)
        adamw(pd, gd, m, v, i + 1, 1.0, wd=wd, stats=stats, ema=ema, d=d, lr=lr)
    assert any(clipped) and not all(clipped), clipped
    assert stats.cpu()[2].item() == sum(clipped)
    assert report("adamw param", (pd.cpu().double() - pt.detach()).abs().max().item(), 1e-6)
    assert report("adamw ema", (ema.cpu().double() - ema_t).abs().max().item(), 1e-6)
    assert report("adamw exp_avg", relerr(m, opt.state[pt]["exp_avg"]), 1e-5)
    assert report("adamw exp_avg_sq", relerr(v, opt.state[pt]["exp_avg_sq"]), 1e-5)
    assert (ema.cpu() - pd.cpu()).abs().max().item() > 1e-4          # the average is not the weights


def test_update_skips_non_finite_gradient():
    n = 10007
    p, g, m, v = update_state(n)
    ema = rnd((n,), 100).to(DEV)
    g[n // 2] = float("nan")
    before = [t.clone() for t in (p, m, v, ema)]
    st, stats = grad_norm(g, max_norm=1.0)
    assert st[1] == 0.0 and st[3] == 1.0
    adamw(p, g, m, v, 3, 1.0, wd=1e-2, stats=stats, ema=ema, d=0.9)
    for got, want in zip((p, m, v, ema), before):
        assert same_bits(got, want)
    g[n // 2] = 0.0                                                  # and the next finite step moves all four
    grad_norm(g, max_norm=1.0, stats=stats)
    adamw(p, g, m, v, 4, 1.0, wd=1e-2, stats=stats, ema=ema, d=0.9)
    for got, want in zip((p, m, v, ema), before):
        assert not same_bits(got, want)
