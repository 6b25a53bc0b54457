"""Overlapped tiles with cross-faded masks: the option beside the reference's disjoint tiling (inference.py:72-120).

The reference cuts a spectrogram into disjoint INPUT_LEN-frame tiles and sends each through the network alone, so the first and
last frames of every tile see zero padding where their real neighbours are.  With tile_hop < seg, overlapped tile j covers frames
[j * tile_hop, j * tile_hop + seg); every frame is then inside some tile's interior, and the masks are cross-faded:

    b(t) = sum_j w[t - j*tile_hop] * mask_j[t - j*tile_hop] / sum_j w[t - j*tile_hop],   w[i] = sin^2(pi * (i + 0.5) / seg)

over the tiles j that cover t.  Both data movements run on the device (csrc/overlap.hip):

    overlap_tiles   (channels, n_tiles, 1, rows, seg) disjoint tiles  -> (channels * n_ov, 1, rows, seg) overlapped tiles
    blend_masks     (channels * n_ov, 1, rows, seg) masks             -> (channels, n_tiles, 1, rows, seg) blended mask (or mix * b)

blend_reference is the definition as a float64 double loop in numpy: the oracle of the tests, independent of the library.
"""
from __future__ import annotations

import numpy as np

MAX_RATIO = 8          # seg / tile_hop of the kernels (include/svs_hip.h)


def check_tile_hop(tile_hop: int, seg: int):
    """Raises ValueError, naming the rule, unless tile_hop is a hop the kernels take for seg-frame tiles."""
    tile_hop, seg = int(tile_hop), int(seg)
    if tile_hop <= 0:
        raise ValueError(f"tile_hop {tile_hop}: must be positive")
    if tile_hop % 4 or seg % tile_hop:
        raise ValueError(f"tile_hop {tile_hop}: must be a multiple of 4 that divides the tile length {seg}")
    if seg // tile_hop > MAX_RATIO:
        raise ValueError(f"tile_hop {tile_hop}: at most {MAX_RATIO} tiles may cover a frame, so it must be at least {seg // MAX_RATIO}")
    return tile_hop


def overlap_count(n_tiles: int, seg: int, tile_hop: int) -> int:
    """Overlapped tiles that cover n_tiles disjoint seg-frame tiles: (n_tiles - 1) * (seg / tile_hop) + 1."""
    from . import _lib
    n = int(_lib.lib().svs_overlap_count(int(n_tiles), int(seg), int(tile_hop)))
    if n < 0:
        _lib.check(n, "svs_overlap_count")
    return n


def check_tile_layout(who: str, tiles):
    """(channels, n_tiles, rows, seg) of data.stft_to_tiles' layout; raises ValueError in the caller's name for anything else."""
    import torch
    if tiles.dim() != 5 or tiles.shape[2] != 1 or tiles.dtype != torch.float32 or not tiles.is_contiguous():
        raise ValueError(f"{who}: expected contiguous float32 (channels, n_tiles, 1, rows, seg) tiles, got {tuple(tiles.shape)} {tiles.dtype}")
    C, n_tiles, _, rows, seg = tiles.shape
    return C, n_tiles, rows, seg


def overlap_tiles(tiles, tile_hop: int):
    """(channels, n_tiles, 1, rows, seg) contiguous float32 tiles on the GPU (data.stft_to_tiles) -> (channels * n_ov, 1, rows, seg):
    overlapped tile j of a channel holds frames [j * tile_hop, j * tile_hop + seg).  One launch."""
    import torch

    from . import _lib
    C, n_tiles, rows, seg = check_tile_layout("overlap_tiles", tiles)
    n_ov = overlap_count(n_tiles, seg, tile_hop)
    out = torch.empty((C * n_ov, 1, rows, seg), dtype=torch.float32, device=tiles.device)
    _lib.check(_lib.lib().svs_overlap_tiles(tiles.data_ptr(), n_tiles * rows * seg, C, n_tiles, rows, seg, int(tile_hop), out.data_ptr(),
                                            _lib.stream_ptr()), "svs_overlap_tiles")
    return out


def blend_masks(masks, n_tiles: int, tile_hop: int, mix=None, invert: bool = False, out=None):
    """(channels * n_ov, 1, rows, seg) masks of overlap_tiles' tiles -> (channels, n_tiles, 1, rows, seg): the cross-faded mask b
    (invert: 1 - b) in the layout of the disjoint tiles, or, with mix (the disjoint tiles), mix * b / mix * (1 - b).  A frame that
    one tile covers keeps that tile's value bit for bit.  One launch; `out` (contiguous, that shape) is allocated if not given."""
    import torch

    from . import _lib
    if masks.dim() != 4 or masks.shape[1] != 1 or masks.dtype != torch.float32 or not masks.is_contiguous():
        raise ValueError(f"blend_masks: expected contiguous float32 (channels * n_ov, 1, rows, seg) masks, got {tuple(masks.shape)} {masks.dtype}")
    _, _, rows, seg = masks.shape
    n_ov = overlap_count(n_tiles, seg, tile_hop)
    if masks.shape[0] % n_ov:
        raise ValueError(f"blend_masks: {masks.shape[0]} masks are no multiple of the {n_ov} overlapped tiles of {n_tiles} tiles at tile_hop {tile_hop}")
    C = masks.shape[0] // n_ov
    shape = (C, int(n_tiles), 1, rows, seg)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=masks.device)
    for name, t in (("out", out), ("mix", mix)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != masks.device):
            raise ValueError(f"blend_masks: {name} must be a contiguous float32 {shape} tensor on {masks.device}, got {tuple(t.shape)} {t.dtype}")
    stride = int(n_tiles) * rows * seg
    _lib.check(_lib.lib().svs_overlap_blend(masks.data_ptr(), C, int(n_tiles), rows, seg, int(tile_hop), _lib.ptr(mix), stride,
                                            1 if invert else 0, out.data_ptr(), stride, _lib.stream_ptr()), "svs_overlap_blend")
    return out


def reference_window(seg: int):
    """float64 (seg,): w[i] = sin^2(pi * (i + 0.5) / seg), strictly positive and symmetric."""
    return np.sin(np.pi * (np.arange(int(seg), dtype=np.float64) + 0.5) / int(seg)) ** 2


def blend_reference(masks, n_tiles: int, tile_hop: int):
    """The definition, float64: masks (channels * n_ov, rows, seg) or (channels * n_ov, 1, rows, seg) array -> (channels, rows,
    n_tiles * seg), frame t of a channel = sum_j w[t - j*hop] * masks[j][.., t - j*hop] / sum_j w[t - j*hop] over the covering tiles j,
    and the covering tile's own value where there is one tile."""
    m = np.asarray(masks, dtype=np.float64)
    if m.ndim == 4:
        m = m[:, 0]
    seg = m.shape[2]
    n_tiles, tile_hop = int(n_tiles), int(tile_hop)
    if tile_hop <= 0 or seg % tile_hop:
        raise ValueError(f"tile_hop {tile_hop} must divide the tile length {seg}")
    n_ov = (n_tiles - 1) * (seg // tile_hop) + 1
    if m.shape[0] % n_ov:
        raise ValueError(f"{m.shape[0]} masks are no multiple of {n_ov} overlapped tiles")
    C, rows = m.shape[0] // n_ov, m.shape[1]
    w = reference_window(seg)
    out = np.empty((C, rows, n_tiles * seg), dtype=np.float64)
    for c in range(C):
        for t in range(n_tiles * seg):
            cover = [j for j in range(n_ov) if 0 <= t - j * tile_hop < seg]
            if len(cover) == 1:
                out[c, :, t] = m[c * n_ov + cover[0], :, t - cover[0] * tile_hop]
                continue
            num = np.zeros(rows, dtype=np.float64)
            den = 0.0
            for j in cover:
                num += w[t - j * tile_hop] * m[c * n_ov + j, :, t - j * tile_hop]
                den += w[t - j * tile_hop]
            out[c, :, t] = num / den
    return out


def reference_weights(seg: int, n_tiles: int, tile_hop: int):
    """float64 (n_tiles * seg,): the sum of the weights of the tiles that cover each frame (blend_reference's denominator)."""
    w = reference_window(seg)
    n_ov = (n_tiles - 1) * (seg // tile_hop) + 1
    den = np.zeros(n_tiles * seg, dtype=np.float64)
    for j in range(n_ov):
        den[j * tile_hop:j * tile_hop + seg] += w
    return den
