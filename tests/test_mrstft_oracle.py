"""The multi-resolution STFT loss oracle on the uneven-level batch (oracle/mrstft_cases.py), on the CPU: the shared-transform
restatement that the GPU tests take their float32 noise scale from IS the oracle's definition, and the batch tells the
per-waveform spectral-convergence ratio from the whole-batch one -- i.e. tests/test_gpu_mrstft.py can fail."""
import functools

import numpy as np
import torch

from oracle import mrstft_cases as mc
from oracle import mrstft_oracle as mo


@functools.lru_cache(maxsize=None)
def hetero():
    x, y, kinds = mc.hetero_batch()
    return x, y, kinds, mc.reference(x, y)


def nonzero_rows(kinds):
    return [b for b, k in enumerate(kinds) if k not in mc.SILENT]


def test_cases_are_what_the_tests_rely_on():
    x, y, kinds = mc.hetero_batch()
    assert x.shape == y.shape == (20, 3600) and x.dtype == y.dtype == np.float32 and len(kinds) == 20
    assert kinds[:10] == kinds[10:] == mc.KINDS
    x2, y2, _ = mc.hetero_batch()
    assert np.array_equal(x, x2) and np.array_equal(y, y2)                    # deterministic
    rms = np.sqrt((x.astype(np.float64) ** 2).mean(axis=1))
    for b in range(10):                                                       # other seeds, every level halved
        assert not np.array_equal(x[b] * 0.5, x[10 + b]) or kinds[b] == "silent_x"
        if kinds[b] != "silent_x":
            assert abs(rms[10 + b] / rms[b] - 0.5) < 0.02
    assert sum(k in mc.SILENT for k in kinds) == 2 and not x[3].any() and not x[13].any() and not y[2].any() and not y[12].any()
    for L_ in mc.EDGE_LENGTHS:
        assert L_ > 2048
    frames = {L_: [1 + L_ // hop for hop in mo.HOP_SIZES] for L_ in mc.EDGE_LENGTHS}      # hops (120, 240, 50)
    assert frames[2799][2] % 8 == 0 and 2799 % 50 == 49 and frames[2800][2] % 8 == 1 and 2800 % 50 == 0
    assert frames[3839][0] % 8 == 0 and frames[3839][1] % 8 == 0
    assert frames[3840][0] % 8 == 1 and frames[3840][1] % 8 == 1 and 3840 % 120 == 0 and 3840 % 240 == 0


def test_shared_fft_restatement_is_the_oracle_in_fp64():
    x, y, kinds, ref = hetero()
    x64, y64 = torch.from_numpy(x).double(), torch.from_numpy(y).double()
    loss, grad = mo.mrstft_loss_and_grad_shared_fft(x64, y64)
    assert np.isfinite(loss) and np.isfinite(ref["loss"]) and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(ref["grad"]).all())
    assert np.isfinite(ref["loss32"]) and bool(torch.isfinite(ref["grad32"]).all()) and np.isfinite(ref["row_loss"]).all()
    assert abs(loss - ref["loss"]) <= 1e-12 * ref["loss"]
    for b in nonzero_rows(kinds):
        assert mc.rel_l2(grad[b] * len(kinds), ref["grad"][b]) <= 1e-9, (b, kinds[b])
    for b, k in enumerate(kinds):
        if k in mc.SILENT:                                                    # clamp(min=1e-8) passes no gradient below it
            assert not ref["grad"][b].any(), (b, k)
    assert abs(np.mean(ref["row_loss"]) - ref["loss"]) <= 1e-12 * ref["loss"]      # the batch loss is the mean of the row losses


# the rows in which the spectral-convergence term carries the gradient: prediction and target of comparable level, broadband
SC_ROWS = ("loud", "-30dB", "silent_y", "near_clamp")


def test_batch_tells_whole_batch_ratio_from_per_waveform_ratio():
    """What the GPU tests could not see before: with this batch the 0.2.x whole-batch ratio is far outside every tolerance
    that tests/test_gpu_mrstft.py applies.

    Loss: at least 10 x the tolerance of test_batch_equals_its_rows (1e-6) and of test_rows_against_fp64 (tol_loss).
    Gradient, EVERY non-zero row: at least 10 x the tolerance of test_batch_equals_its_rows (1e-6 of the row's maximum).
    Gradient against test_rows_against_fp64's per-row tolerance (max(6 x noise_row, 2e-3), 3e-3 for the maximum): at least
    10 x in the SC_ROWS.  In the other rows no form of the ratio can do that: the ratio scales only the spectral-convergence
    part of the gradient, which is |X| / |Y| of it where the prediction lies 40 / 80 dB under the target (whole-batch form:
    3e-3 / 7e-5 of the row's norm away), and a few 1e-3 .. 1e-2 of it in the DC / Nyquist / tonal rows, whose gradient is the
    log-magnitude term's 1 / |X| on the noise-floor bins; those rows are there for the bins and the float32 noise."""
    x, y, kinds, ref = hetero()
    B = len(kinds)
    loss_w, grad_w = mo.mrstft_loss_and_grad_whole_batch_ratio(torch.from_numpy(x).double(), torch.from_numpy(y).double())
    grad_w = grad_w * B
    loss_tol = max(1e-6, mc.tol_loss(abs(ref["loss32"] - ref["loss"]) / ref["loss"]))
    assert abs(loss_w - ref["loss"]) / ref["loss"] >= 10 * loss_tol
    seen = set()
    for b in nonzero_rows(kinds):
        want = ref["grad"][b]
        l2, mx = mc.rel_l2(grad_w[b], want), mc.rel_max(grad_w[b], want)
        assert mx >= 10 * 1e-6, (b, kinds[b], mx)
        if kinds[b] in SC_ROWS:
            seen.add(kinds[b])
            assert l2 >= 10 * mc.tol_grad_l2(mc.rel_l2(ref["grad32"][b], want)), (b, kinds[b], l2)
            assert mx >= 10 * mc.tol_grad_max(mc.rel_max(ref["grad32"][b], want)), (b, kinds[b], mx)
    assert seen == set(SC_ROWS)
