"""Multichannel Wiener filter with EM updates of a local Gaussian model (Duong, Vincent and Gribonval; norbert.wiener; the
post-filter of Open-Unmix) between the mask and the inverse transform.

The reference writes istft(mag * mask * phase of the mixture) (inference.py:100-107, data.py:159) one channel at a time and has no
such step.  Here the two masked magnitudes start a model of J = 2 sources (0 vocal, 1 accompaniment) in C = 1 or 2 channels; with
x = scale * mag * P the complex mixture on ONE scale for both channels (scale_c = norm_c / max norm, |x| <= 1), an update is

    v_j[t,f] = mean_c |y_jc|^2                                    the source's power per bin
    R_j[f]   = sum_t y_j y_j^H / (eps + sum_t v_j[t,f])           its C x C spatial covariance per frequency
    Cxx[t,f] = sum_j v_j R_j + reg * I
    y_j      = v_j R_j Cxx^-1 x                                   W_j x: the stems add up to x but for reg * Cxx^-1 x

from y_0 = scale * mag * mask * P and y_1 = scale * mag * (1 - mask) * P.  eps = 1e-10 is Open-Unmix's; reg = 1e-7 is its
sqrt(eps) = 1e-5 for a mixture scaled to a maximum of 10, brought to this project's maximum of 1 (variances scale with |x|^2).
The stems come out on the common scale, so the stereo balance of the mixture is kept.  One channel is the power-ratio filter.

    check_wiener_iters  the argument rule of the public interface
    wiener_model        the binding of svs_wiener_model: one update of (v, R)
    wiener_stems        the binding of svs_wiener_stems: y_j = W_j x as magnitude tiles and unit phasors
    wiener_filter       tiles, mask, phasors and maxima of data.stft_to_tiles -> the stems' tiles and phasors
    wiener_reference    the definition in float64 numpy, closed-form 2 x 2 inverse: the oracle of the tests
"""
from __future__ import annotations

import numpy as np

EPS = 1e-10
REG = 1e-7
MAX_ITERS = 8


def check_wiener_iters(wiener_iters: int) -> int:
    """Raises ValueError unless wiener_iters is a count of updates, 0 (no filter) .. 8."""
    if isinstance(wiener_iters, bool) or not isinstance(wiener_iters, (int, np.integer)):
        raise ValueError(f"wiener_iters {wiener_iters!r}: must be an integer in 0..{MAX_ITERS} (0 writes the masked magnitudes as they are)")
    if not 0 <= int(wiener_iters) <= MAX_ITERS:
        raise ValueError(f"wiener_iters {wiener_iters}: must be an integer in 0..{MAX_ITERS} (0 writes the masked magnitudes as they are)")
    return int(wiener_iters)


def _check_tiles(who, tiles, phase, frames):
    import torch

    from .overlap import check_tile_layout
    C, n_tiles, rows, seg = check_tile_layout(who, tiles)
    if C not in (1, 2):
        raise ValueError(f"{who}: {C} channels: the filter is built for 1 or 2")
    if n_tiles != -(-int(frames) // seg):
        raise ValueError(f"{who}: {n_tiles} tiles of {seg} frames do not hold exactly {frames} frames")
    if tuple(phase.shape) != (C, frames, rows + 1) or phase.dtype != torch.complex64:
        raise ValueError(f"{who}: phase {tuple(phase.shape)} {phase.dtype} is not complex64 (channels, frames, rows + 1) = {(C, frames, rows + 1)}")
    return C, n_tiles, rows, seg


def wiener_model(tiles, mask, phase, scale, frames: int, prev=None, eps: float = EPS, reg: float = REG, out=None):
    """One update of the model (svs_wiener_model; two launches).  tiles / mask (channels, n_tiles, 1, rows, seg) float32, phase
    (channels, frames, rows + 1) complex64, scale (channels,) float32, all on the GPU.  prev None: the posterior is the masked
    magnitudes with the mixture's phase (mask required); prev = (v, R) of the update before: the posterior is W(v, R) x.
    -> (v (2, n_tiles, 1, rows, seg) float32, R (2, rows, 4) float64 = R00, R11, Re R01, Im R01).  out = (v, R) to write into;
    it may be prev itself."""
    import torch

    from . import _lib
    from .data import phase_floats
    C, n_tiles, rows, seg = _check_tiles("wiener_model", tiles, phase, frames)
    if prev is None and mask is None:
        raise ValueError("wiener_model: the first update needs the mask")
    if mask is not None and (mask.shape != tiles.shape or mask.dtype != torch.float32 or not mask.is_contiguous()):
        raise ValueError(f"wiener_model: the mask must be a contiguous float32 tensor shaped like the tiles, got {tuple(mask.shape)} {mask.dtype}")
    one = n_tiles * rows * seg
    if out is None:
        out = (torch.empty((2, n_tiles, 1, rows, seg), dtype=torch.float32, device=tiles.device),
               torch.empty((2, rows, 4), dtype=torch.float64, device=tiles.device))
    v, R = out
    L = _lib.lib()
    ws = torch.empty(int(L.svs_wiener_workspace_bytes(C, rows, seg, frames)), dtype=torch.uint8, device=tiles.device)
    v_prev, R_prev = (None, None) if prev is None else prev
    _lib.check(L.svs_wiener_model(tiles.data_ptr(), one, seg, rows, _lib.ptr(mask), phase_floats(phase).data_ptr(), scale.data_ptr(), C,
                                  frames, _lib.ptr(v_prev), one, _lib.ptr(R_prev), float(eps), float(reg), v.data_ptr(), one, R.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "svs_wiener_model")
    return v, R


def wiener_stems(tiles, phase, scale, frames: int, model, stems=(0, 1), reg: float = REG):
    """y_j = W_j(v, R) x for the stems asked for (svs_wiener_stems; one launch): (0,), (1,) or (0, 1).
    -> (magnitude tiles (len(stems), channels, n_tiles, 1, rows, seg) float32, zero in the padded frames, unit phasors
    (len(stems), channels, frames, rows + 1) complex64, exactly 1 + 0i in the DC bin and where y is exactly zero): per stem what
    data.istft_from_tiles(mask=None) takes."""
    import torch

    from . import _lib
    from .data import phase_floats
    C, n_tiles, rows, seg = _check_tiles("wiener_stems", tiles, phase, frames)
    stems = tuple(stems)
    if stems not in ((0,), (1,), (0, 1)):
        raise ValueError(f"wiener_stems: stems {stems} must be (0,), (1,) or (0, 1)")
    v, R = model
    one = n_tiles * rows * seg
    S = len(stems)
    mags = torch.empty((S, C, n_tiles, 1, rows, seg), dtype=torch.float32, device=tiles.device)
    ph = torch.empty((S, C, frames, rows + 1, 2), dtype=torch.float32, device=tiles.device)
    _lib.check(_lib.lib().svs_wiener_stems(tiles.data_ptr(), one, seg, rows, phase_floats(phase).data_ptr(), scale.data_ptr(), C, frames,
                                           v.data_ptr(), one, R.data_ptr(), float(reg), 2 if S == 2 else stems[0], mags.data_ptr(), one,
                                           C * one, ph.data_ptr(), C * frames * (rows + 1) * 2, _lib.stream_ptr()), "svs_wiener_stems")
    return mags, torch.view_as_complex(ph)


def common_scale(norm):
    """(channels,) maxima of data.stft_to_tiles -> scale_c = norm_c / max_c' norm_c' (0 for a file of silence): what brings the
    per-channel normalised tiles back to one scale with |x| <= 1."""
    import torch
    top = norm.max()
    return torch.where(top > 0, norm / top, torch.zeros_like(norm)).float().contiguous()


def wiener_filter(tiles, mask, phase, norm, frames: int, iters: int, stems=(0, 1), eps: float = EPS, reg: float = REG):
    """tiles (each channel divided by its maximum), mask, frame-major phasors and per-channel maxima `norm` as
    data.stft_to_tiles and the network leave them -> (magnitude tiles, phasors) of the stems as wiener_stems returns them, after
    `iters` >= 1 updates: `iters` calls of svs_wiener_model (the model is updated in place) and one of svs_wiener_stems.  The stems
    are on the common scale of the two channels (common_scale), so the stereo balance of the mixture is kept."""
    iters = check_wiener_iters(iters)
    if iters < 1:
        raise ValueError("wiener_filter: iters must be at least 1 (0 is no filter: invert tiles * mask as they are)")
    if mask is None:
        raise ValueError("wiener_filter: the mask is required")
    scale = common_scale(norm)
    model = wiener_model(tiles, mask, phase, scale, frames, None, eps, reg)
    for _ in range(iters - 1):
        model = wiener_model(tiles, None, phase, scale, frames, model, eps, reg, out=model)
    return wiener_stems(tiles, phase, scale, frames, model, stems, reg)


# ---- the float64 definition ------------------------------------------------------------------------------------------------

def wiener_reference(x, mags, iters: int, eps: float = EPS, reg: float = REG):
    """The definition in float64.  x complex (C, F, T): the mixture, C = 1 or 2; mags (2, C, F, T) >= 0: the magnitudes the model
    starts from, which take the mixture's phase, y_j = mags_j * x / |x| (0 where x is 0).  Runs `iters` updates and returns

        y  complex128 (2, C, F, T)   the stems after the last update (the start for iters = 0)
        v  float64 (2, F, T)         the powers the last update was made with (None for iters = 0)
        R  complex128 (2, F, C, C)   its spatial covariances (None for iters = 0)

    The C = 2 inverse is written out, C = 1 is a division: no linear-algebra call.  With Cxx = [[A, c], [c*, B]] it is the
    elimination form z_1 = (x_1 - c* x_0 / A) / (B - |c|^2 / A), z_0 = (x_0 - c z_1) / A, which is backward stable for a Hermitian
    positive definite Cxx.  Adjugate over determinant is not: for a panned point source Cxx = s p p^H + reg I, and both
    A B - |c|^2 and adj(Cxx) x cancel to reg / s of their terms, which costs float64 1e-11 of the peak on these signals."""
    iters = check_wiener_iters(iters)
    x = np.asarray(x, dtype=np.complex128)
    mags = np.asarray(mags, dtype=np.float64)
    if x.ndim != 3 or x.shape[0] not in (1, 2) or mags.shape != (2,) + x.shape:
        raise ValueError(f"wiener_reference: x {x.shape} must be (C, F, T) with C in (1, 2) and mags {mags.shape} (2, C, F, T)")
    C = x.shape[0]
    a = np.abs(x)
    y = mags * np.where(a == 0, 0.0, x / np.where(a == 0, 1.0, a))[None]
    v = R = None
    for _ in range(iters):
        v = (np.abs(y) ** 2).mean(axis=1)                                           # (2, F, T)
        den = eps + v.sum(axis=-1)                                                  # (2, F)
        R = np.einsum("jaft,jbft->jfab", y, y.conj()) / den[:, :, None, None]       # (2, F, C, C)
        if C == 1:
            g = v * R[:, :, 0, 0].real[:, :, None]                                  # (2, F, T)
            y = (g / (g.sum(axis=0) + reg)[None])[:, None] * x[None]
            continue
        r00, r11, r01 = R[:, :, 0, 0].real[:, :, None], R[:, :, 1, 1].real[:, :, None], R[:, :, 0, 1][:, :, None]
        A = (v * r00).sum(axis=0) + reg
        B = (v * r11).sum(axis=0) + reg
        c = (v * r01).sum(axis=0)
        d = B - (c.real ** 2 + c.imag ** 2) / A                                     # the Schur complement of A: det / A
        z1 = (x[1] - c.conj() * (x[0] / A)) / d
        z0 = (x[0] - c * z1) / A
        y = np.stack([v * (r00 * z0 + r01 * z1), v * (r01.conj() * z0 + r11 * z1)], axis=1)
    return y, v, R
