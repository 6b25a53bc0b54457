"""Phase refinement of separated stems: Griffin-Lim for one stem, MISI (multiple-input spectrogram inversion, Gunawan and Sen) for the
two stems of a mask.

The reference writes istft(mag * mask * phase of the mixture) (inference.py:100-107, data.py:159).  A masked magnitude that carries
the mixture's phase is the STFT of no signal: the inverse transform returns the least-squares signal and drops the inconsistent
part.  With M_s the magnitude of stem s (mag * mask, mag * (1 - mask)) and P_s its unit phasors (at first the mixture's), one update is

    x_s = istft(M_s * P_s)                                    the existing inverse (svs_istft_tiles_n), one launch per stem
    e   = (mix - x_0 - x_1) / 2                               two stems only: what the stems fail to add up to, half to each
    P_s = phasor(STFT(x_s + e))                               csrc/stft.hip: svs_stft_rephase_n, ONE launch for all stems and channels,
                                                              the three streams combined on load, only phasors written

and phasor(0) = 1 + 0i (librosa.magphase).  Waveforms are hop * (T - 1) samples (the inverse trims n_fft / 2 from both ends), whose
centred STFT has T frames again.  Nothing is peak-normalised inside the loop.

    rephase            the binding of svs_stft_rephase_n
    refine_phase       the loop on the device: tiles, mask and phasors of data.stft_to_tiles -> one set of phasors per stem
    rephase_reference  the same loop in float64 numpy: the oracle of the tests, independent of the library
    inconsistency      || |STFT(x)| - M ||^2 / || M ||^2 in float64, the measure the iterations lower
"""
from __future__ import annotations

import numpy as np


def check_phase_iters(phase_iters: int) -> int:
    """Raises ValueError unless phase_iters is a count of iterations (0 = none)."""
    if int(phase_iters) != phase_iters or int(phase_iters) < 0:
        raise ValueError(f"phase_iters {phase_iters}: must be an integer >= 0 (0 keeps the mixture's phase)")
    return int(phase_iters)


def _check_stems(stems: int, mix):
    if stems not in (1, 2):
        raise ValueError(f"stems {stems}: must be 1 (Griffin-Lim) or 2 (MISI)")
    if stems == 2 and mix is None:
        raise ValueError("stems=2 is MISI: the mixture `mix` is required (each stem receives half of mix - x_0 - x_1)")
    if stems == 1 and mix is not None:
        raise ValueError("mix is given with stems=1: one stem is Griffin-Lim, which has no mixture to add up to")


def rephase(x, mix, n_fft: int, hop: int, out=None):
    """x float32 (stems, channels, n) contiguous on the GPU, mix (channels, n) or None -> complex64 (stems, channels, T, n_fft/2+1),
    T = 1 + n // hop: the unit phasors of STFT(x_s + (mix - x_0 - x_1) / 2), or of STFT(x_s) without mix.  One launch."""
    import torch

    from . import _lib
    from .data import _check_window
    _check_window(n_fft, hop)
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"rephase: expected contiguous float32 (stems, channels, n) signals, got {tuple(x.shape)} {x.dtype}")
    S, C, n = x.shape
    if mix is not None and (S != 2 or tuple(mix.shape) != (C, n) or mix.dtype != torch.float32 or not mix.is_contiguous() or mix.device != x.device):
        raise ValueError(f"rephase: mix must be a contiguous float32 ({C}, {n}) tensor beside two stems, got {tuple(mix.shape)} {mix.dtype} "
                         f"for {S} stem(s)")
    L = _lib.lib()
    T = int(L.svs_stft_frames(n, hop))
    nbin = n_fft // 2 + 1
    if out is None:
        out = torch.empty((S, C, T, nbin, 2), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (S, C, T, nbin, 2) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"rephase: out must be a contiguous float32 {(S, C, T, nbin, 2)} tensor, got {tuple(out.shape)} {out.dtype}")
    _lib.check(L.svs_stft_rephase_n(x.data_ptr(), C * n, S, _lib.ptr(mix), n, C, n_fft, hop, out.data_ptr(), C * T * nbin * 2,
                                    _lib.stream_ptr()), "svs_stft_rephase_n")
    return torch.view_as_complex(out)


def refine_phase(tiles, mask, phase, frames: int, iters: int, *, stems: int, invert: bool = False, mix=None, n_fft: int, hop: int):
    """tiles / mask (channels, n_tiles, 1, n_fft/2, seg) and frame-major phasors (channels, T, n_fft/2+1) as data.istft_from_tiles takes
    them -> complex64 (stems, channels, T, n_fft/2+1): the phasors after `iters` updates, to be handed to istft_from_tiles per stem.
    stems=1: Griffin-Lim on tiles * mask (invert: tiles * (1 - mask)).  stems=2: MISI on [tiles * mask, tiles * (1 - mask)]; mix
    (channels, hop * (T - 1)) float32, at the scale of the tiles, is required.  The first inverse uses `phase`; update i is one
    svs_stft_rephase_n on the current waveforms and, unless it is the last, one svs_istft_tiles_n per stem with that stem's new
    phasors -- the last update's inverse is the caller's final one (which also takes the caller's peak).  iters=0 returns `phase`
    broadcast over the stems, with no launch."""
    import torch

    from . import _lib
    from .data import _check_window, phase_floats
    iters = check_phase_iters(iters)
    _check_stems(stems, mix)
    _check_window(n_fft, hop)
    C, n_tiles, _, rows, seg = tiles.shape
    nbin = rows + 1
    if tuple(phase.shape) != (C, frames, nbin):
        raise ValueError(f"refine_phase: phase {tuple(phase.shape)} is not (channels, frames, n_fft/2+1) = {(C, frames, nbin)}")
    if iters == 0:
        return phase.unsqueeze(0).expand(stems, C, frames, nbin)
    if mask is None:
        raise ValueError("refine_phase: the mask is required (without one the mixture's own phase is consistent already)")
    n_out = hop * (frames - 1)
    if mix is not None and tuple(mix.shape) != (C, n_out):
        raise ValueError(f"refine_phase: mix {tuple(mix.shape)} is not (channels, hop * (frames - 1)) = {(C, n_out)}")
    L = _lib.lib()
    x = torch.empty((stems, C, n_out), dtype=torch.float32, device=tiles.device)
    ph = torch.empty((stems, C, frames, nbin, 2), dtype=torch.float32, device=tiles.device)
    inv = [0, 1] if stems == 2 else [1 if invert else 0]

    def inverse(s, phasors):
        _lib.check(L.svs_istft_tiles_n(tiles.data_ptr(), n_tiles * rows * seg, seg, rows, 1, mask.data_ptr(), inv[s], phasors.data_ptr(), 1,
                                       C, n_fft, hop, frames, x[s].data_ptr(), None, _lib.stream_ptr()), "svs_istft_tiles_n")

    first = phase_floats(phase)
    for s in range(stems):
        inverse(s, first)
    for it in range(iters):
        rephase(x, mix, n_fft, hop, out=ph)
        if it + 1 < iters:
            for s in range(stems):
                inverse(s, ph[s])
    return torch.view_as_complex(ph)


# ---- the float64 definition ------------------------------------------------------------------------------------------------

def reference_window(n_fft: int):
    """float64 periodic Hann window, sin^2(pi m / n_fft)."""
    return np.sin(np.pi * np.arange(int(n_fft), dtype=np.float64) / int(n_fft)) ** 2


def reference_stft(x, n_fft: int, hop: int):
    """float64 (..., n) -> complex128 (..., n_fft/2+1, 1 + n // hop): centred frames, zero padding, periodic Hann."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    T = 1 + n // hop
    pad = np.zeros(x.shape[:-1] + (n_fft + hop * (T - 1),), dtype=np.float64)
    have = min(n, pad.shape[-1] - n_fft // 2)
    pad[..., n_fft // 2:n_fft // 2 + have] = x[..., :have]
    idx = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]
    return np.moveaxis(np.fft.rfft(pad[..., idx] * reference_window(n_fft), axis=-1), -1, -2)


def reference_istft(spec, n_fft: int, hop: int):
    """complex128 (..., n_fft/2+1, T) -> float64 (..., hop * (T - 1)): irfft, window, overlap-add, divide by the window's sum of
    squares, trim n_fft / 2 from both ends."""
    spec = np.asarray(spec, dtype=np.complex128)
    T = spec.shape[-1]
    w = reference_window(n_fft)
    frames = np.fft.irfft(np.moveaxis(spec, -1, -2), n=n_fft, axis=-1) * w
    out = np.zeros(spec.shape[:-2] + (n_fft + hop * (T - 1),), dtype=np.float64)
    env = np.zeros(out.shape[-1], dtype=np.float64)
    for t in range(T):
        out[..., hop * t:hop * t + n_fft] += frames[..., t, :]
        env[hop * t:hop * t + n_fft] += w * w
    out = np.where(env > 1.1754944e-38, out / np.where(env > 1.1754944e-38, env, 1.0), out)
    return out[..., n_fft // 2:n_fft // 2 + hop * (T - 1)]


def reference_phasor(spec):
    """Unit phasors of a complex array, exactly 1 + 0i where it is exactly zero (librosa.magphase)."""
    a = np.abs(spec)
    return np.where(a == 0, 1.0 + 0.0j, spec / np.where(a == 0, 1.0, a))


def _distance(spec, mags):
    """|| |spec| - M ||^2 / || M ||^2 per leading index (0 where M is all zero)."""
    S = mags.shape[0]
    num, den = ((np.abs(spec) - mags).reshape(S, -1) ** 2).sum(axis=1), (mags.reshape(S, -1) ** 2).sum(axis=1)
    return num / np.where(den > 0, den, 1.0)


def inconsistency(x, mags, n_fft: int, hop: int):
    """|| |STFT(x)| - M ||^2 / || M ||^2 in float64, per leading index: x (S, ..., n), mags (S, ..., n_fft/2+1, T) -> (S,)."""
    x, mags = np.asarray(x, dtype=np.float64), np.asarray(mags, dtype=np.float64)
    return _distance(reference_stft(x, n_fft, hop), mags)


def rephase_reference(mags, phase, iters: int, mix=None, *, n_fft: int, hop: int):
    """The definition in float64.  mags (stems, channels, n_fft/2+1, T): the magnitude of every stem, DC row included; phase
    (channels, n_fft/2+1, T) complex: the phasors of the first inverse, shared by the stems; mix (channels, hop * (T - 1)) or None
    (required for two stems, refused for one).  Runs `iters` updates and returns

        phases  complex128 (stems, channels, n_fft/2+1, T)   after the last update (the input, broadcast, for iters = 0)
        waves   float64 (stems, channels, hop * (T - 1))     istft(mags * phases)
        measure float64 (iters + 1,)                         the inconsistency of the waveforms after 0 .. iters updates, summed over
                                                             the stems; for two stems it is taken on x_s + e, what is re-analysed
    """
    iters = check_phase_iters(iters)
    mags = np.asarray(mags, dtype=np.float64)
    if mags.ndim != 4 or mags.shape[2] != n_fft // 2 + 1:
        raise ValueError(f"rephase_reference: mags {mags.shape} is not (stems, channels, {n_fft // 2 + 1}, T)")
    S, C, nbin, T = mags.shape
    _check_stems(S, mix)
    if n_fft not in (512, 1024, 2048):
        raise ValueError(f"n_fft = {n_fft}: the transforms are built for n_fft in (512, 1024, 2048)")
    if not 0 < hop <= n_fft:
        raise ValueError(f"hop = {hop}: must be in 1..{n_fft}")
    phases = np.broadcast_to(np.asarray(phase, dtype=np.complex128), (S, C, nbin, T)).copy()
    n_out = hop * (T - 1)
    if mix is not None:
        mix = np.asarray(mix, dtype=np.float64)
        if mix.shape != (C, n_out):
            raise ValueError(f"rephase_reference: mix {mix.shape} is not (channels, hop * (T - 1)) = {(C, n_out)}")
    measure = np.empty(iters + 1, dtype=np.float64)

    def analysed(waves):
        return waves if mix is None else waves + 0.5 * (mix - waves[0] - waves[1])[None]

    waves = reference_istft(mags * phases, n_fft, hop)
    for it in range(iters):
        spec = reference_stft(analysed(waves), n_fft, hop)
        measure[it] = _distance(spec, mags).sum()
        phases = reference_phasor(spec)
        waves = reference_istft(mags * phases, n_fft, hop)
    measure[iters] = inconsistency(analysed(waves), mags, n_fft, hop).sum()
    return phases, waves, measure
