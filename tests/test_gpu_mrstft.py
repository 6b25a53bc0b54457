"""Multi-resolution STFT loss kernel (csrc/mrstft.hip) per waveform (-m gpu): batches whose rows differ in level and character
(oracle/mrstft_cases.py), every row judged by itself against the float64 oracle, the waveform edges and the ragged last block
of 8 frames by themselves, and the rows that the k = 0 / k = N/2 weights decide.

Tolerances: the project's rule for this kernel (test_gpu_ops.py, test_mrstft_loss_and_gradient) applied per row or region --
max(6 x noise, floor), `noise` being the deviation from float64 of the float32 shared-transform restatement of the DEFINITION
(oracle/mrstft_oracle.py, mrstft_loss_and_grad_shared_fft) on the same row or region.  No constant comes from the kernel.
tests/test_mrstft_oracle.py shows on the CPU that these inputs put the whole-batch ratio form far outside the tolerances."""
import functools

import pytest
import torch

from oracle import mrstft_cases as mc
from svs_unet_pytorch_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"


def mr(x, y, grad_scale, grad=True):
    """svs_mrstft_loss_fwd_bwd on device tensors (B, L): (loss as float, grad_scale * d loss / d x on the host or None)."""
    lib = _lib.lib()
    B, n = x.shape
    assert x.is_contiguous() and y.is_contiguous()
    ws = torch.empty(int(lib.svs_mrstft_workspace_bytes(B, n)) + 4096, dtype=torch.uint8, device=DEV)
    loss = torch.zeros(1, device=DEV)
    dx = torch.full_like(x, float("nan")) if grad else None
    _lib.check(lib.svs_mrstft_loss_fwd_bwd(x.data_ptr(), y.data_ptr(), B, n, grad_scale, loss.data_ptr(), dx.data_ptr() if grad else None,
                                           ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    return loss.item(), (dx.cpu() if grad else None)


@functools.lru_cache(maxsize=None)
def case(name, n):
    """(x, y on the device, kinds, reference) of one batch; computed once, shared by the tests, never written to."""
    x, y, kinds = {"hetero": mc.hetero_batch, "edge": mc.edge_batch, "bins": mc.bins_batch}[name](n)
    return torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), kinds, mc.reference(x, y)


@functools.lru_cache(maxsize=None)
def kernel_on_hetero():
    """The kernel on the uneven batch: once on the whole batch with grad_scale = B, once per row with B = 1, grad_scale = 1."""
    x, y, kinds, _ = case("hetero", 3600)
    B = len(kinds)
    whole = mr(x, y, float(B))
    rows = [mr(x[b:b + 1].contiguous(), y[b:b + 1].contiguous(), 1.0) for b in range(B)]
    return whole, rows


def check_rows(tag, got_grad, got_row_loss, kinds, ref, report, regions=None):
    """Every row (and region) of `got_grad` (B, L), single-row scale, and every single-row loss against the float64 oracle.
    Returns the failures; reports every figure."""
    bad = []
    n = got_grad.shape[1]
    for b, k in enumerate(kinds):
        if k in mc.SILENT:                               # every |X|^2 under the clamp: the gradient is exactly zero
            if got_grad[b].any():
                bad.append((tag, b, k, "gradient not exactly zero", float(got_grad[b].abs().max())))
        else:
            for rname, (lo, hi) in (regions or {"": (0, n)}).items():
                if hi <= lo:
                    continue
                got, want, g32 = got_grad[b, lo:hi], ref["grad"][b, lo:hi], ref["grad32"][b, lo:hi]
                assert float(want.norm()) > 0
                for what, err, tol in (("rel-L2", mc.rel_l2(got, want), mc.tol_grad_l2(mc.rel_l2(g32, want))),
                                       ("max", mc.rel_max(got, want), mc.tol_grad_max(mc.rel_max(g32, want)))):
                    if not report(f"mrstft {tag} row {b} {k} {rname} gradient {what}", err, tol):
                        bad.append((tag, b, k, rname, what, err, tol))
        want = ref["row_loss"][b]
        err, tol = abs(got_row_loss[b] - want) / want, mc.tol_loss(abs(ref["row_loss32"][b] - want) / want)
        if not report(f"mrstft {tag} row {b} {k} loss", err, tol):
            bad.append((tag, b, k, "loss", err, tol))
    return bad


def test_batch_equals_its_rows(report):
    """No oracle: the log term has the same count per row and the ratio is per row, so loss(batch) is the mean of the row losses
    and d_x[b] of the batch call with grad_scale = B is the B = 1 gradient of row b -- up to the one float rounding of the
    coefficient formed in double.  Any mixing between rows, a slip in the [B][gx] stride of the partial sums or in the walk past
    waveform 16 breaks it."""
    x, y, kinds, _ = case("hetero", 3600)
    (loss, dx), rows = kernel_on_hetero()
    assert len(kinds) == 20 and torch.isfinite(dx).all()
    mean = sum(r[0] for r in rows) / len(rows)
    ok = report("mrstft batch loss vs mean of its rows' losses", abs(loss - mean) / mean, 1e-6)
    for b, k in enumerate(kinds):
        one = rows[b][1][0].double()
        scale = float(one.abs().max())
        if k in mc.SILENT:
            ok &= scale == 0.0 and not dx[b].any()
        else:
            assert scale > 0
            ok &= report(f"mrstft batch row {b} {k} gradient vs its B=1 call (max)", float((dx[b].double() - one).abs().max()) / scale, 1e-6)
    assert ok


def test_rows_against_fp64(report):
    """Every row of the uneven batch by itself -- its own norm, its own maximum -- against the float64 oracle: the batch call's
    gradient rows, the B = 1 calls' loss values, and the batch loss.  Only the two rows built with a silent prediction take no
    ratio: their gradient is exactly zero.

    The near_clamp rows (peak 1.5e-5 / 7.5e-6) are the ones this test found wrong: 1.23 / 4.09 rel-L2 while the two unscaled
    gradient parts of a frame shared the inverse transform as they came; 1e-7 since mr_pass_kernel balances them."""
    _, _, kinds, ref = case("hetero", 3600)
    (loss, dx), rows = kernel_on_hetero()
    assert sum(k in mc.SILENT for k in kinds) <= 2
    bad = check_rows("B=20", dx.double(), [r[0] for r in rows], kinds, ref, report)
    tol = mc.tol_loss(abs(ref["loss32"] - ref["loss"]) / ref["loss"])
    if not report("mrstft B=20 batch loss", abs(loss - ref["loss"]) / ref["loss"], tol):
        bad.append(("batch loss", loss, ref["loss"], tol))
    assert not bad, bad


@pytest.mark.parametrize("n", mc.EDGE_LENGTHS)
def test_edges_and_ragged_blocks(n, report):
    """Lengths at which the last block of 8 frames holds 8 frames or 1, the minimum length, lengths that are multiples of the
    hops: the first and last 1025 samples (two reflect-padding mirrors fold onto them) and the rest, each against its own norm
    and maximum; and the value-only call (d_x = NULL, another kernel) gives bitwise the gradient call's loss."""
    x, y, kinds, ref = case("edge", n)
    B = len(kinds)
    loss, dx = mr(x, y, float(B))
    assert torch.isfinite(dx).all()
    row_loss = [mr(x[b:b + 1].contiguous(), y[b:b + 1].contiguous(), 1.0, grad=False)[0] for b in range(B)]
    regions = {"head": (0, 1025), "tail": (n - 1025, n), "rest": (1025, n - 1025)}
    bad = check_rows(f"L={n}", dx.double(), row_loss, kinds, ref, report, regions)
    tol = mc.tol_loss(abs(ref["loss32"] - ref["loss"]) / ref["loss"])
    if not report(f"mrstft L={n} batch loss", abs(loss - ref["loss"]) / ref["loss"], tol):
        bad.append(("batch loss", loss, ref["loss"], tol))
    assert not bad, bad
    assert mr(x, y, float(B), grad=False)[0] == loss


@pytest.mark.parametrize("n", [2800, 3840])
def test_edge_bins_and_tones(n, report):
    """DC-, Nyquist-dominated and tonal rows alone: an error in the k = 0 or k = N/2 weight is the whole answer here (in white
    noise it is 2 bins of 513)."""
    x, y, kinds, ref = case("bins", n)
    B = len(kinds)
    loss, dx = mr(x, y, float(B))
    assert torch.isfinite(dx).all()
    row_loss = [mr(x[b:b + 1].contiguous(), y[b:b + 1].contiguous(), 1.0, grad=False)[0] for b in range(B)]
    bad = check_rows(f"bins L={n}", dx.double(), row_loss, kinds, ref, report)
    tol = mc.tol_loss(abs(ref["loss32"] - ref["loss"]) / ref["loss"])
    if not report(f"mrstft bins L={n} batch loss", abs(loss - ref["loss"]) / ref["loss"], tol):
        bad.append(("batch loss", loss, ref["loss"], tol))
    assert not bad, bad
