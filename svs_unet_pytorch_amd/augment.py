"""Remix and gain augmentation of the training tiles (Uhlich et al. 2017; Open-Unmix; Demucs), cut on the device from the resident set.

The reference's SpectrogramDataset (train.py:86-143) pairs every crop of a song's mixture with the same crop of its own vocal.  Here
item b takes its vocal from song A at column start_v and, when it is a remix item, its accompaniment from song B at column start_a,
each source with a gain.  `train.ResidentSpectrograms` keeps the magnitude and the angle of every mixture and vocal, both divided
by one per-song norm (data.py:84-85,105), so M cis(phi_m) - V cis(phi_v) is the accompaniment's STFT and, frame for frame,

    z = g_v V_A cis(phi_vA) + g_a (M_B cis(phi_mB) - V_B cis(phi_vB))        mix = |z|, mix_phase = arg z, voc = g_v V_A, voc_phase = phi_vA

is the STFT of the re-mixed waveform -- exact (the transform is linear per frame), not a magnitude-domain approximation; only the
frames within ceil(n_fft / (2 hop)) of a song's edge differ, because they carry the reflect-padding of their own song.  A gain item
(song_a < 0) keeps its own mixture: mix = g_v M_A, voc = g_v V_A, angles copied.  Nothing is renormalised: mix may exceed 1, the mask
is scale-free.

    remix_reference  the definition in float64 numpy on the same fp32 inputs: the oracle of the tests, independent of the library
    draw_epoch       the per-item table of one epoch, a function of (seed, epoch) alone
    upload_table     the range checks on the host arrays, then ONE pinned copy of the items a rank will use, in its order
    crop_remix       items lo..hi-1 of an uploaded table: one svs_crop_remix_tiles launch (csrc/augment.hip)
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass

import numpy as np

MODES = ("none", "gain", "remix")
GAIN_RANGE = (0.25, 1.25)            # Open-Unmix's
REMIX_PROB = 0.5                     # a choice, not a tuned value: half the items keep their own accompaniment

Remix = namedtuple("Remix", "mix voc mix_phase voc_phase z scale")
EpochTable = namedtuple("EpochTable", "song_v start_v song_a start_a gain_v gain_a")
ROWS = EpochTable._fields           # the device table's six rows, in this order: four int32, two float32 (bit patterns)


@dataclass(frozen=True)
class Augment:
    """The settings of --augment / --gain_range / --remix_prob / --augment_seed."""
    mode: str = "none"
    gain_range: tuple = GAIN_RANGE
    remix_prob: float = REMIX_PROB
    seed: int = 0

    def describe(self):
        if self.mode == "none":
            return "Augmentation: none"
        text = f"Augmentation: {self.mode}, gains uniform in [{self.gain_range[0]}, {self.gain_range[1]}]"
        if self.mode == "remix":
            text += f", accompaniment of another crop with probability {self.remix_prob}"
        return text + f", seed {self.seed}"


def check_settings(mode, gain_range, remix_prob):
    """The message for settings that cannot be trained with, or None."""
    if mode not in MODES:
        return f"--augment {mode}: one of {', '.join(MODES)}"
    lo, hi = (float(g) for g in gain_range)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= hi):
        return f"--gain_range {lo} {hi}: needs 0 < LO <= HI, both finite (a gain of 0 silences a source, a negative one inverts it)"
    if not 0.0 <= float(remix_prob) <= 1.0:
        return f"--remix_prob {remix_prob}: a probability, 0 .. 1"
    return None


def _crop64(song, start, seg):
    """Columns [start, start + seg) of an (F, T) array as float64, right zero-padded."""
    out = np.zeros((song.shape[0], seg), np.float64)
    n = max(min(song.shape[1] - start, seg), 0)
    out[:, :n] = song[:, start:start + n]
    return out


def remix_reference(mix_songs, voc_songs, mix_ang, voc_ang, song_v, start_v, song_a, start_a, gain_v, gain_a, seg):
    """The definition of svs_crop_remix_tiles in float64.  mix_songs / voc_songs / mix_ang / voc_ang: one (F, T_s) array per song
    (the angle lists may be None: the gain-only form, every item a gain item); the six tables: one entry per item.  Returns
    Remix(mix, voc, mix_phase, voc_phase, z, scale), each (B, 1, F, seg): float64 (z complex128; the phases None without angles),
    scale = g_v V_A + g_a (M_B + V_B) for a remix item and g_v M_A for a gain item -- what the rounding errors of an fp32 evaluation
    are proportional to."""
    B, F = len(song_v), mix_songs[0].shape[0]
    have = mix_ang is not None
    mix, voc, scale = (np.zeros((B, 1, F, seg), np.float64) for _ in range(3))
    z = np.zeros((B, 1, F, seg), np.complex128)
    voc_phase = np.zeros((B, 1, F, seg), np.float64) if have else None
    copied = {}
    for b in range(B):
        A, sv, gv = int(song_v[b]), int(start_v[b]), float(np.float32(gain_v[b]))
        VA = _crop64(voc_songs[A], sv, seg)
        voc[b, 0] = gv * VA
        pv = _crop64(voc_ang[A], sv, seg) if have else None
        if have:
            voc_phase[b, 0] = pv
        if not have or int(song_a[b]) < 0:
            MA = _crop64(mix_songs[A], sv, seg)
            mix[b, 0] = scale[b, 0] = gv * MA
            z[b, 0] = gv * MA
            if have:                                                     # the angle is copied, also where the magnitude is 0
                copied[b] = _crop64(mix_ang[A], sv, seg)
                z[b, 0] = gv * MA * np.exp(1j * copied[b])
        else:
            Bs, sa, ga = int(song_a[b]), int(start_a[b]), float(np.float32(gain_a[b]))
            MB, VB = _crop64(mix_songs[Bs], sa, seg), _crop64(voc_songs[Bs], sa, seg)
            pm, pb = _crop64(mix_ang[Bs], sa, seg), _crop64(voc_ang[Bs], sa, seg)
            z[b, 0] = gv * VA * np.exp(1j * pv) + ga * (MB * np.exp(1j * pm) - VB * np.exp(1j * pb))
            mix[b, 0] = np.abs(z[b, 0])
            scale[b, 0] = gv * VA + abs(ga) * (MB + VB)
    mix_phase = np.angle(z) if have else None
    for b, angle in copied.items():
        mix_phase[b, 0] = angle
    return Remix(mix, voc, mix_phase, voc_phase, z, scale)


def draw_epoch(n_items, frames_host, seg, epoch, seed=0, gain_range=GAIN_RANGE, remix_prob=REMIX_PROB):
    """The augmentation of every item of one epoch, indexed by item id, as EpochTable(song_v, start_v, song_a, start_a, gain_v, gain_a)
    (int32 x 4, float32 x 2).  song_v is the dataset's rule, item % n_songs; gains are uniform in gain_range; with probability
    remix_prob song_a is uniform over ALL songs (the item's own included), else -1; starts are uniform in [0, T - seg], 0 for a song
    no longer than seg.  The generator is PCG64 seeded by (seed, epoch) and nothing else, so every rank draws the same table (and
    takes its items by train.epoch_order), and a run resumed at epoch e draws what the uninterrupted run would have."""
    frames = np.asarray(frames_host, np.int64)
    n_songs = len(frames)
    if n_songs == 0 or n_items <= 0:
        return EpochTable(*(np.zeros(0, np.int32) for _ in range(4)), *(np.zeros(0, np.float32) for _ in range(2)))
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), int(epoch)])))
    lo, hi = float(gain_range[0]), float(gain_range[1])
    song_v = np.arange(n_items, dtype=np.int64) % n_songs
    gain_v = rng.uniform(lo, hi, n_items).astype(np.float32)
    gain_a = rng.uniform(lo, hi, n_items).astype(np.float32)
    # (uniform in double, rounded to fp32: the rounding may land on an end of the range, never outside it)
    remix = rng.random(n_items) < float(remix_prob)
    other = rng.integers(0, n_songs, n_items)
    room = np.maximum(frames - seg, 0)                                   # last start of each song
    start_v = rng.integers(0, room[song_v], endpoint=True)
    start_a = rng.integers(0, room[other], endpoint=True)
    song_a = np.where(remix, other, -1)
    start_a = np.where(remix, start_a, 0)
    return EpochTable(song_v.astype(np.int32), start_v.astype(np.int32), song_a.astype(np.int32), start_a.astype(np.int32), gain_v, gain_a)


def check_table(table, frames_host, seg, has_angles):
    """The kernel trusts its tables (as svs_crop_tiles does), so they are checked here, on the host arrays, before they go up: song
    indices in range, starts within [0, max(T - seg, 0)], finite gains, and no remix item for a set without angles."""
    frames = np.asarray(frames_host, np.int64)
    n_songs = len(frames)
    t = EpochTable(*(np.asarray(a) for a in table))
    n = len(t.song_v)
    if any(len(a) != n for a in t):
        raise ValueError(f"augmentation table: rows of {[len(a) for a in t]} entries")
    if n == 0:
        return t
    if n_songs == 0:
        raise ValueError("augmentation table: the resident set has no songs")
    if t.song_v.min() < 0 or t.song_v.max() >= n_songs:
        raise ValueError(f"augmentation table: song_v outside 0..{n_songs - 1}")
    if t.song_a.max() >= n_songs:
        raise ValueError(f"augmentation table: song_a outside -1..{n_songs - 1}")
    remix = t.song_a >= 0
    if remix.any() and not has_angles:
        raise ValueError("augmentation table: remix items need the angles of a set with *_phase.npy files (gain items do not)")
    room = np.maximum(frames - seg, 0)
    if (t.start_v < 0).any() or (t.start_v > room[t.song_v]).any():
        raise ValueError("augmentation table: start_v outside [0, max(T - seg, 0)] of its song")
    sa, ra = t.start_a[remix], room[t.song_a[remix]]
    if (sa < 0).any() or (sa > ra).any():
        raise ValueError("augmentation table: start_a outside [0, max(T - seg, 0)] of its song")
    if not (np.isfinite(t.gain_v).all() and np.isfinite(t.gain_a).all()):
        raise ValueError("augmentation table: a gain is not finite")
    return t


def pack_table(table, items=None):
    """The (6, n) int32 host array of a table: rows song_v, start_v, song_a, start_a, then the bit patterns of gain_v, gain_a;
    `items` (optional) picks and orders the columns."""
    rows = [np.asarray(a, np.int32) for a in table[:4]] + [np.asarray(a, np.float32).view(np.int32) for a in table[4:]]
    packed = np.stack(rows)
    return np.ascontiguousarray(packed if items is None else packed[:, np.asarray(items, np.int64)])


def upload_table(resident, table, items=None):
    """check_table, then the packed table of `items` (default: all, in order) as one (6, n) int32 device tensor: one pinned
    host-to-device copy for a whole epoch of a rank."""
    import torch

    from .config import INPUT_LEN
    check_table(table, resident.frames_host, INPUT_LEN, resident.mix_ang is not None)
    return torch.from_numpy(pack_table(table, items)).pin_memory().to(resident.device, non_blocking=True)


def crop_remix(resident, table, lo, hi, with_phase=False):
    """mix, voc [, mix_phase, voc_phase] (hi - lo, 1, rows, INPUT_LEN) on the device for items lo..hi-1 of `table`: an uploaded
    (6, n) tensor of upload_table (a batch is a slice of it: no copy of its own), or an EpochTable, which is checked and uploaded
    first.  One svs_crop_remix_tiles launch.  A set without angles takes the gain-only form."""
    import torch

    from . import _lib
    from .config import INPUT_LEN
    if isinstance(table, tuple):
        table = upload_table(resident, table)
    if with_phase and resident.mix_ang is None:
        raise ValueError("phase tiles asked of a set without *_phase.npy files")
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[0] != len(ROWS) or not table.is_contiguous() \
            or not (0 <= lo < hi <= table.shape[1]):
        raise ValueError(f"items {lo}..{hi} of a table of shape {tuple(table.shape)}")
    B = hi - lo
    out = [torch.empty((B, 1, resident.rows, INPUT_LEN), dtype=torch.float32, device=resident.device) for _ in range(4 if with_phase else 2)]
    row = [table[r, lo:hi].data_ptr() for r in range(len(ROWS))]
    _lib.check(_lib.lib().svs_crop_remix_tiles(resident.mix.data_ptr(), resident.voc.data_ptr(), _lib.ptr(resident.mix_ang),
                                               _lib.ptr(resident.voc_ang), resident.offsets.data_ptr(), resident.frames.data_ptr(), *row,
                                               B, resident.rows, INPUT_LEN, out[0].data_ptr(), out[1].data_ptr(),
                                               out[2].data_ptr() if with_phase else None, out[3].data_ptr() if with_phase else None,
                                               _lib.stream_ptr()), "svs_crop_remix_tiles")
    return tuple(out)
