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

Time-stretch (--stretch_range; Cohen-Hadria, Roebel and Peeters 2019) puts a phase vocoder between "read the source frames" and
"mix": each source is resampled along time at its own rate q / 1024 (magnitudes interpolated, phases re-accumulated from the measured
advance per hop), and the mixture is the sum of the stretched sources -- never a stretched mixture: the vocoder is not linear, and the
training target must add up.  The vocoder is the classic one, the form librosa.phase_vocoder uses (restated, parity unpinned).

    phase_vocoder / stretch_reference   the definition in float64 numpy
    draw_epoch_stretch                  StretchTable: the six rows above plus rate_v, rate_a (int32 Q10), from a seed sequence of its own
    check_stretch_table / pack_stretch_table / upload_stretch_table / crop_stretch     as above, one svs_crop_stretch_tiles launch

Pitch shift (--pitch_range, in semitones; the same study) is the same vocoder with the frequency axis resampled: output bin b takes
its magnitude from the source's fractional bin b / p and its phase from the nearest source bin, whose true advance per hop is
multiplied by p.  It is applied to each source, with or without a stretch, and the mixture is again the sum of the shifted sources.

    pitch_vocoder / pitch_reference     the definition in float64 numpy (at p = 1 it is phase_vocoder / stretch_reference)
    draw_epoch_pitch                    PitchTable: StretchTable's eight rows plus pitch_v, pitch_a (int32 Q10), from a seed sequence of its own
    check_pitch_table / pack_pitch_table / upload_pitch_table / crop_pitch             as above, one svs_crop_pitch_tiles launch
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
STRETCH_RANGE = (0.8, 1.25)          # the range one would start with: a choice, not a tuned value
RATE_ONE, RATE_MIN, RATE_MAX = 1024, 512, 2048      # rates are Q10 integers q, r = q / 1024, within 0.5 .. 2
Stretch = namedtuple("Stretch", "mix voc mix_phase voc_phase z zv scale cond_v cond_a")
StretchTable = namedtuple("StretchTable", EpochTable._fields + ("rate_v", "rate_a"))
STRETCH_ROWS = StretchTable._fields  # the device table's eight rows: the six above, then two int32
PITCH_RANGE = (-2.0, 2.0)            # semitones; the range one would start with: a choice, not a tuned value
PITCH_ONE, PITCH_MIN, PITCH_MAX = 1024, 512, 2048   # pitches are Q10 integers P, p = P / 1024, within an octave either way
SEMITONES_MAX = 12.0
PitchTable = namedtuple("PitchTable", StretchTable._fields + ("pitch_v", "pitch_a"))
PITCH_ROWS = PitchTable._fields      # the device table's ten rows: the eight above, then two int32


@dataclass(frozen=True)
class Augment:
    """The settings of --augment / --gain_range / --remix_prob / --augment_seed."""
    mode: str = "none"
    gain_range: tuple = GAIN_RANGE
    remix_prob: float = REMIX_PROB
    seed: int = 0
    stretch_range: tuple = None      # --stretch_range LO HI: every source time-stretched at a rate of its own (None: off)
    pitch_range: tuple = None        # --pitch_range LO HI (semitones): every source pitch-shifted by an amount of its own (None: off)

    def describe(self):
        if self.mode == "none":
            return "Augmentation: none"
        text = f"Augmentation: {self.mode}, gains uniform in [{self.gain_range[0]}, {self.gain_range[1]}]"
        if self.mode == "remix":
            text += f", accompaniment of another crop with probability {self.remix_prob}"
        if self.stretch_range is not None:
            text += f", each source time-stretched at a rate uniform in [{self.stretch_range[0]}, {self.stretch_range[1]}]"
        if self.pitch_range is not None:
            text += (f", each source pitch-shifted by semitones uniform in [{self.pitch_range[0]}, {self.pitch_range[1]}]"
                     f" ({PITCH_RANGE[0]:g} {PITCH_RANGE[1]:g} is a starting point, not a tuned value)")
        return text + f", seed {self.seed}"


def check_settings(mode, gain_range, remix_prob, stretch_range=None, pitch_range=None):
    """The message for settings that cannot be trained with, or None."""
    if pitch_range is not None:
        if mode == "none":
            return "--pitch_range: the pitch shift is part of the augmented tile cut, it needs --augment gain or --augment remix"
        lo, hi = (float(r) for r in pitch_range)
        if not (np.isfinite(lo) and np.isfinite(hi) and -SEMITONES_MAX <= lo <= hi <= SEMITONES_MAX):
            return f"--pitch_range {lo} {hi}: semitones, needs {-SEMITONES_MAX:g} <= LO <= HI <= {SEMITONES_MAX:g}"
    if stretch_range is not None:
        if mode == "none":
            return "--stretch_range: the stretch is part of the augmented tile cut, it needs --augment gain or --augment remix"
        lo, hi = (float(r) for r in stretch_range)
        if not (np.isfinite(lo) and np.isfinite(hi) and RATE_MIN / RATE_ONE <= lo <= hi <= RATE_MAX / RATE_ONE):
            return f"--stretch_range {lo} {hi}: needs {RATE_MIN / RATE_ONE} <= LO <= HI <= {RATE_MAX / RATE_ONE}"
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


# ---- time-stretch: a phase vocoder on each source before the mix ------------------------------------------------------------

def span(q, seg):
    """Source frames a tile of `seg` output frames reads at rate q / 1024: frames 0 .. ((seg - 1) q >> 10) + 1 past its start."""
    return (((seg - 1) * np.asarray(q, np.int64)) >> 10) + 2


def _polar64(plane):
    """(|S|, arg S) of a complex (F, T) plane; arg of an exactly zero magnitude is 0."""
    mag = np.abs(plane)
    return mag, np.where(mag == 0.0, 0.0, np.angle(plane))


def _columns(a, k):
    """Columns k (an int array) of an (F, T) array, 0 outside [0, T)."""
    T = a.shape[1]
    return np.where(((k >= 0) & (k < T))[None, :], a[:, np.clip(k, 0, T - 1)], 0.0)


def phase_vocoder(plane, start, q, seg, n_fft, hop, weight=None):
    """The classic phase vocoder on one complex (F, T) source plane (rows are bins 1..F: the DC row is dropped), in float64:
    output frame t reads source position n = t q, k = start + (n >> 10), alpha = (n & 1023) / 1024 (exact in integers),
        mag = (1 - alpha) |S[k]| + alpha |S[k+1]|,  out_t = mag cis(acc),  d = arg S[k+1] - arg S[k] - w,  d -= 2 pi round(d / 2 pi),
        acc += w + d,                                   acc_0 = arg S[start],  w = 2 pi ((hop bin) mod n_fft) / n_fft.
    Returns (mag, acc, cond): (F, seg) each; cond is the running sum of `weight` (an (F, T) array, default 1) over the source frames
    whose angles entered acc -- what the phase error of a finite-precision evaluation is proportional to."""
    F = plane.shape[0]
    mag_s, arg_s = _polar64(np.asarray(plane, np.complex128))
    wgt = np.ones(mag_s.shape) if weight is None else np.asarray(weight, np.float64)
    n = np.arange(seg, dtype=np.int64) * int(q)
    k = int(start) + (n >> 10)
    alpha = (n & 1023) / 1024.0
    m0, m1, a0, a1 = _columns(mag_s, k), _columns(mag_s, k + 1), _columns(arg_s, k), _columns(arg_s, k + 1)
    mag = (1.0 - alpha) * m0 + alpha * m1
    w = 2.0 * np.pi * ((hop * np.arange(1, F + 1, dtype=np.int64)) % n_fft) / n_fft
    d = a1 - a0 - w[:, None]
    d -= 2.0 * np.pi * np.round(d / (2.0 * np.pi))
    step = w[:, None] + d
    acc = a0[:, :1] + np.concatenate([np.zeros((F, 1)), np.cumsum(step[:, :-1], axis=1)], axis=1)
    c0, c1 = _columns(wgt, k), _columns(wgt, k + 1)
    cond = c0[:, :1] + np.concatenate([np.zeros((F, 1)), np.cumsum((c0 + c1)[:, :-1], axis=1)], axis=1)
    return mag, acc, cond


def _wrap_pi(a):
    return a - 2.0 * np.pi * np.round(a / (2.0 * np.pi))


def stretch_reference(mix_songs, voc_songs, mix_ang, voc_ang, song_v, start_v, song_a, start_a, gain_v, gain_a, rate_v, rate_a, seg,
                      n_fft, hop):
    """The definition of svs_crop_stretch_tiles in float64 on the same fp32 inputs (one (F, T_s) array per song, one table entry per
    item): z = g_v PV(vocal of A; s_v, q_v) + g_a PV(accompaniment of B; s_a, q_a) with the accompaniment M cis(phi_m) - V cis(phi_v);
    a gain item (song_a < 0) takes B = A, s_a = s_v, q_a = q_v through the same complex path.  Returns Stretch(mix, voc, mix_phase,
    voc_phase, z, zv, scale, cond_v, cond_a), each (B, 1, F, seg): mix = |z|, mix_phase = arg z, voc = g_v mag_v, voc_phase = acc_v
    wrapped to [-pi, pi], a phase being 0 where its magnitude is exactly 0; zv = voc cis(acc_v) is the stretched vocal;
    scale = g_v V + g_a (M + V) with the interpolated magnitudes; cond_v / cond_a: the running sums, over the source frames that
    entered acc, of 1 for the vocal and of (M + V) / |M cis(phi_m) - V cis(phi_v)| (0 where that is 0) for the accompaniment."""
    B, F = len(song_v), mix_songs[0].shape[0]
    shape = (B, 1, F, seg)
    mix, voc, mix_phase, voc_phase, scale, cond_v, cond_a = (np.zeros(shape, np.float64) for _ in range(7))
    z, zv = np.zeros(shape, np.complex128), np.zeros(shape, np.complex128)
    as64 = lambda a: np.asarray(a, np.float64)
    for b in range(B):
        A, sv, qv, gv = int(song_v[b]), int(start_v[b]), int(rate_v[b]), float(np.float32(gain_v[b]))
        Bs, sa, qa, ga = int(song_a[b]), int(start_a[b]), int(rate_a[b]), float(np.float32(gain_a[b]))
        if Bs < 0:
            Bs, sa, qa = A, sv, qv
        mag_v, acc_v, cond_v[b, 0] = phase_vocoder(as64(voc_songs[A]) * np.exp(1j * as64(voc_ang[A])), sv, qv, seg, n_fft, hop)
        M, V = as64(mix_songs[Bs]), as64(voc_songs[Bs])
        acc_plane = M * np.exp(1j * as64(mix_ang[Bs])) - V * np.exp(1j * as64(voc_ang[Bs]))
        size = np.abs(acc_plane)
        with np.errstate(divide="ignore", invalid="ignore"):
            weight = np.where(size > 0.0, (M + V) / size, 0.0)
        mag_a, acc_a, cond_a[b, 0] = phase_vocoder(acc_plane, sa, qa, seg, n_fft, hop, weight)
        voc[b, 0] = gv * mag_v
        zv[b, 0] = voc[b, 0] * np.exp(1j * acc_v)
        z[b, 0] = zv[b, 0] + ga * mag_a * np.exp(1j * acc_a)
        voc_phase[b, 0] = np.where(voc[b, 0] == 0.0, 0.0, _wrap_pi(acc_v))
        n = np.arange(seg, dtype=np.int64) * qa
        alpha = (n & 1023) / 1024.0
        k = sa + (n >> 10)
        scale[b, 0] = voc[b, 0] + abs(ga) * ((1.0 - alpha) * _columns(M + V, k) + alpha * _columns(M + V, k + 1))
    mix = np.abs(z)
    mix_phase = np.where(mix == 0.0, 0.0, np.angle(z))
    return Stretch(mix, voc, mix_phase, voc_phase, z, zv, scale, cond_v, cond_a)


def draw_epoch_stretch(n_items, frames_host, seg, epoch, seed=0, gain_range=GAIN_RANGE, remix_prob=REMIX_PROB, stretch_range=STRETCH_RANGE):
    """The augmentation of every item of one epoch with time-stretch, as StretchTable: EpochTable's six rows plus rate_v, rate_a
    (int32 Q10).  Gains, song_v and song_a follow draw_epoch's rules; rates are uniform integers in [round(1024 lo), round(1024 hi)]
    (a gain item's rate_a is its rate_v); starts are uniform in [0, max(T - span(q), 0)], span(q) = ((seg - 1) q >> 10) + 2.  A
    function of (seed, epoch) from a seed sequence of its own (it need not agree with draw_epoch), so every rank draws the same table."""
    frames = np.asarray(frames_host, np.int64)
    n_songs = len(frames)
    if n_songs == 0 or n_items <= 0:
        return StretchTable(*(np.zeros(0, np.int32) for _ in range(4)), *(np.zeros(0, np.float32) for _ in range(2)),
                            *(np.zeros(0, np.int32) for _ in range(2)))
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), int(epoch), 0x73747265])))     # "stre": its own sequence
    lo, hi = float(gain_range[0]), float(gain_range[1])
    q_lo, q_hi = int(round(RATE_ONE * float(stretch_range[0]))), int(round(RATE_ONE * float(stretch_range[1])))
    song_v = np.arange(n_items, dtype=np.int64) % n_songs
    gain_v = rng.uniform(lo, hi, n_items).astype(np.float32)
    gain_a = rng.uniform(lo, hi, n_items).astype(np.float32)
    remix = rng.random(n_items) < float(remix_prob)
    other = rng.integers(0, n_songs, n_items)
    rate_v = rng.integers(q_lo, q_hi, n_items, endpoint=True)
    rate_a = np.where(remix, rng.integers(q_lo, q_hi, n_items, endpoint=True), rate_v)
    start_v = rng.integers(0, np.maximum(frames[song_v] - span(rate_v, seg), 0), endpoint=True)
    start_a = rng.integers(0, np.maximum(frames[other] - span(rate_a, seg), 0), endpoint=True)
    song_a = np.where(remix, other, -1)
    start_a = np.where(remix, start_a, 0)
    i32 = lambda a: a.astype(np.int32)
    return StretchTable(i32(song_v), i32(start_v), i32(song_a), i32(start_a), gain_v, gain_a, i32(rate_v), i32(rate_a))


def check_stretch_table(table, frames_host, seg, has_angles=True, what="stretch table"):
    """check_table's rules with span(q) in the place of seg -- song indices in range, starts within [0, max(T - span(q), 0)] of their
    song, finite gains -- and 512 <= q <= 2048 (rate_a and start_a of a gain item are not read); the angles are required."""
    frames = np.asarray(frames_host, np.int64)
    n_songs = len(frames)
    t = StretchTable(*(np.asarray(a) for a in table))
    n = len(t.song_v)
    if any(len(a) != n for a in t):
        raise ValueError(f"{what}: rows of {[len(a) for a in t]} entries")
    if n == 0:
        return t
    if not has_angles:
        raise ValueError(f"{what}: the stretch needs the angles of a set with *_phase.npy files")
    if n_songs == 0:
        raise ValueError(f"{what}: the resident set has no songs")
    if t.song_v.min() < 0 or t.song_v.max() >= n_songs:
        raise ValueError(f"{what}: song_v outside 0..{n_songs - 1}")
    if t.song_a.max() >= n_songs:
        raise ValueError(f"{what}: song_a outside -1..{n_songs - 1}")
    remix = t.song_a >= 0
    if (t.rate_v < RATE_MIN).any() or (t.rate_v > RATE_MAX).any():
        raise ValueError(f"{what}: rate_v outside {RATE_MIN}..{RATE_MAX} (Q10)")
    if (t.rate_a[remix] < RATE_MIN).any() or (t.rate_a[remix] > RATE_MAX).any():
        raise ValueError(f"{what}: rate_a outside {RATE_MIN}..{RATE_MAX} (Q10)")
    if (t.start_v < 0).any() or (t.start_v > np.maximum(frames[t.song_v] - span(t.rate_v, seg), 0)).any():
        raise ValueError(f"{what}: start_v outside [0, max(T - span(q), 0)] of its song")
    sa, ra = t.start_a[remix], np.maximum(frames[t.song_a[remix]] - span(t.rate_a[remix], seg), 0)
    if (sa < 0).any() or (sa > ra).any():
        raise ValueError(f"{what}: start_a outside [0, max(T - span(q), 0)] of its song")
    if not (np.isfinite(t.gain_v).all() and np.isfinite(t.gain_a).all()):
        raise ValueError(f"{what}: a gain is not finite")
    return t


def pack_stretch_table(table, items=None):
    """The (8, n) int32 host array of a StretchTable: pack_table's six rows, then rate_v, rate_a; `items` picks and orders the columns."""
    rows = [np.asarray(a, np.int32) for a in table[:4]] + [np.asarray(a, np.float32).view(np.int32) for a in table[4:6]] \
        + [np.asarray(a, np.int32) for a in table[6:]]
    packed = np.stack(rows)
    return np.ascontiguousarray(packed if items is None else packed[:, np.asarray(items, np.int64)])


def upload_stretch_table(resident, table, items=None):
    """check_stretch_table, then the packed table of `items` as one (8, n) int32 device tensor: one pinned copy per epoch and rank."""
    import torch

    from .config import INPUT_LEN
    check_stretch_table(table, resident.frames_host, INPUT_LEN, resident.mix_ang is not None)
    return torch.from_numpy(pack_stretch_table(table, items)).pin_memory().to(resident.device, non_blocking=True)


def crop_stretch(resident, table, lo, hi, n_fft, hop, with_phase=False):
    """mix, voc [, mix_phase, voc_phase] (hi - lo, 1, rows, INPUT_LEN) on the device for items lo..hi-1 of `table`: an uploaded
    (8, n) tensor of upload_stretch_table, or a StretchTable, which is checked and uploaded first.  One svs_crop_stretch_tiles launch
    at the geometry (n_fft, hop) the set was written with."""
    import torch

    from . import _lib
    from .config import INPUT_LEN
    if isinstance(table, tuple):
        table = upload_stretch_table(resident, table)
    if resident.mix_ang is None:
        raise ValueError("the stretch needs the angles of a set with *_phase.npy files")
    if resident.rows != n_fft // 2:
        raise ValueError(f"the resident set has {resident.rows}-row tiles, n_fft {n_fft} needs {n_fft // 2}")
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[0] != len(STRETCH_ROWS) or not table.is_contiguous() \
            or not (0 <= lo < hi <= table.shape[1]):
        raise ValueError(f"items {lo}..{hi} of a table of shape {tuple(table.shape)}")
    B = hi - lo
    out = [torch.empty((B, 1, resident.rows, INPUT_LEN), dtype=torch.float32, device=resident.device) for _ in range(4 if with_phase else 2)]
    row = [table[r, lo:hi].data_ptr() for r in range(len(STRETCH_ROWS))]
    _lib.check(_lib.lib().svs_crop_stretch_tiles(resident.mix.data_ptr(), resident.voc.data_ptr(), resident.mix_ang.data_ptr(),
                                                 resident.voc_ang.data_ptr(), resident.offsets.data_ptr(), resident.frames.data_ptr(), *row,
                                                 B, resident.rows, INPUT_LEN, int(n_fft), int(hop), out[0].data_ptr(), out[1].data_ptr(),
                                                 out[2].data_ptr() if with_phase else None, out[3].data_ptr() if with_phase else None,
                                                 _lib.stream_ptr()), "svs_crop_stretch_tiles")
    return tuple(out)


# ---- pitch shift: the vocoder with the frequency axis resampled and the phase advance scaled -------------------------------

def pitch_bins(F, P):
    """(j0, gamma, j) of the output rows b = 1..F at the Q10 pitch P, exact in integers: N = 1024 b, j0 = N div P and
    gamma = (N mod P) / P are the source's fractional bin b / p, j = clamp((2 N + P) div 2 P, 1, F) is the nearest source bin, ties up."""
    N, P = 1024 * np.arange(1, F + 1, dtype=np.int64), int(P)
    return N // P, (N % P) / float(P), np.clip((2 * N + P) // (2 * P), 1, F)


def _bins(a, i):
    """Rows of the bins i (an int array, 1-based) of an (F, n) array whose rows are bins 1..F; 0 outside 1..F."""
    F = a.shape[0]
    return np.where(((i >= 1) & (i <= F))[:, None], a[np.clip(i, 1, F) - 1], 0.0)


def _bilinear(a, k, alpha, j0, gamma):
    """An (F, T) array at the source frames k + alpha and the source bins j0 + gamma, interpolated linearly in time, then in bin."""
    tm = (1.0 - alpha) * _columns(a, k) + alpha * _columns(a, k + 1)
    return (1.0 - gamma)[:, None] * _bins(tm, j0) + gamma[:, None] * _bins(tm, j0 + 1)


def pitch_vocoder(plane, start, q, P, seg, n_fft, hop, weight=None):
    """phase_vocoder with the pitch scaled by p = P / 1024 (P a Q10 integer, 512..2048), in float64.  Rows of `plane` are bins 1..F
    and every bin outside 1..F is zero.  Time is indexed as there (n = t q, k = start + (n >> 10), alpha = (n & 1023) / 1024); output
    row b = f + 1 has (j0, gamma, j) = pitch_bins and
        tm(i) = (1 - alpha) |S[i, k]| + alpha |S[i, k+1]|,  mag = (1 - gamma) tm(j0) + gamma tm(j0 + 1),  out_t = mag cis(acc),
        w = 2 pi ((hop j) mod n_fft) / n_fft,  d = arg S[j, k+1] - arg S[j, k] - w wrapped to [-pi, pi),
        w' = 2 pi ((hop j P) mod (1024 n_fft)) / (1024 n_fft),  acc += w' + p d,  acc_0 = arg S[j, start]:
    the magnitude of the source's fractional bin b / p, the phase of the nearest source bin with its true advance per hop
    (w + d, whose unreduced centre part is 2 pi hop j / n_fft) multiplied by p.  At P = 1024 this is phase_vocoder, value for value.
    Returns (mag, acc, cond): (F, seg) each; cond is weight[j, start] plus p times the running sum of `weight` (an (F, T) array,
    default 1) over the later source frames of bin j whose angles entered acc -- an error of an angle reaches acc p-fold."""
    F, P = plane.shape[0], int(P)
    p = P / 1024.0
    mag_s, arg_s = _polar64(np.asarray(plane, np.complex128))
    wgt = np.ones(mag_s.shape) if weight is None else np.asarray(weight, np.float64)
    n = np.arange(seg, dtype=np.int64) * int(q)
    k = int(start) + (n >> 10)
    alpha = (n & 1023) / 1024.0
    j0, gamma, j = pitch_bins(F, P)
    mag = _bilinear(mag_s, k, alpha, j0, gamma)
    a0, a1 = _columns(arg_s, k)[j - 1], _columns(arg_s, k + 1)[j - 1]
    w = 2.0 * np.pi * ((hop * j) % n_fft) / n_fft
    d = a1 - a0 - w[:, None]
    d -= 2.0 * np.pi * np.round(d / (2.0 * np.pi))
    d = np.where(d >= np.pi, d - 2.0 * np.pi, d)                         # [-pi, pi): p d depends on the turn that is removed
    w_scaled = 2.0 * np.pi * ((hop * j * P) % (1024 * n_fft)) / (1024 * n_fft)                    # int64: the product reaches 2^32
    step = w_scaled[:, None] + p * d
    acc = a0[:, :1] + np.concatenate([np.zeros((F, 1)), np.cumsum(step[:, :-1], axis=1)], axis=1)
    c0, c1 = _columns(wgt, k)[j - 1], _columns(wgt, k + 1)[j - 1]
    cond = c0[:, :1] + p * np.concatenate([np.zeros((F, 1)), np.cumsum((c0 + c1)[:, :-1], axis=1)], axis=1)
    return mag, acc, cond


def pitch_reference(mix_songs, voc_songs, mix_ang, voc_ang, song_v, start_v, song_a, start_a, gain_v, gain_a, rate_v, rate_a, pitch_v,
                    pitch_a, seg, n_fft, hop):
    """The definition of svs_crop_pitch_tiles in float64 on the same fp32 inputs: stretch_reference with pitch_vocoder in the place of
    phase_vocoder, z = g_v PV(vocal of A; s_v, q_v, P_v) + g_a PV(accompaniment of B; s_a, q_a, P_a); a gain item (song_a < 0) takes
    B = A, s_a = s_v, q_a = q_v, P_a = P_v through the same complex path.  Returns what stretch_reference returns, a Stretch(mix, voc,
    mix_phase, voc_phase, z, zv, scale, cond_v, cond_a): scale = g_v V + g_a (M + V) with the magnitudes interpolated in time and in
    bin, cond_v / cond_a pitch_vocoder's running sums (weights 1 and (M + V) / |M cis(phi_m) - V cis(phi_v)|)."""
    B, F = len(song_v), mix_songs[0].shape[0]
    shape = (B, 1, F, seg)
    mix, voc, mix_phase, voc_phase, scale, cond_v, cond_a = (np.zeros(shape, np.float64) for _ in range(7))
    z, zv = np.zeros(shape, np.complex128), np.zeros(shape, np.complex128)
    as64 = lambda a: np.asarray(a, np.float64)
    for b in range(B):
        A, sv, qv, Pv, gv = int(song_v[b]), int(start_v[b]), int(rate_v[b]), int(pitch_v[b]), float(np.float32(gain_v[b]))
        Bs, sa, qa, Pa, ga = int(song_a[b]), int(start_a[b]), int(rate_a[b]), int(pitch_a[b]), float(np.float32(gain_a[b]))
        if Bs < 0:
            Bs, sa, qa, Pa = A, sv, qv, Pv
        mag_v, acc_v, cond_v[b, 0] = pitch_vocoder(as64(voc_songs[A]) * np.exp(1j * as64(voc_ang[A])), sv, qv, Pv, seg, n_fft, hop)
        M, V = as64(mix_songs[Bs]), as64(voc_songs[Bs])
        acc_plane = M * np.exp(1j * as64(mix_ang[Bs])) - V * np.exp(1j * as64(voc_ang[Bs]))
        size = np.abs(acc_plane)
        with np.errstate(divide="ignore", invalid="ignore"):
            weight = np.where(size > 0.0, (M + V) / size, 0.0)
        mag_a, acc_a, cond_a[b, 0] = pitch_vocoder(acc_plane, sa, qa, Pa, seg, n_fft, hop, weight)
        voc[b, 0] = gv * mag_v
        zv[b, 0] = voc[b, 0] * np.exp(1j * acc_v)
        z[b, 0] = zv[b, 0] + ga * mag_a * np.exp(1j * acc_a)
        voc_phase[b, 0] = np.where(voc[b, 0] == 0.0, 0.0, _wrap_pi(acc_v))
        n = np.arange(seg, dtype=np.int64) * qa
        j0, gamma, _ = pitch_bins(F, Pa)
        scale[b, 0] = voc[b, 0] + abs(ga) * _bilinear(M + V, sa + (n >> 10), (n & 1023) / 1024.0, j0, gamma)
    mix = np.abs(z)
    mix_phase = np.where(mix == 0.0, 0.0, np.angle(z))
    return Stretch(mix, voc, mix_phase, voc_phase, z, zv, scale, cond_v, cond_a)


def semitones_to_pitch(st):
    """The Q10 pitch of a shift by `st` semitones: round(1024 2^(st / 12)), kept within 512..2048 (one octave: exactly the ends)."""
    return np.clip(np.rint(PITCH_ONE * np.exp2(np.asarray(st, np.float64) / 12.0)), PITCH_MIN, PITCH_MAX).astype(np.int64)


def draw_epoch_pitch(n_items, frames_host, seg, epoch, seed=0, gain_range=GAIN_RANGE, remix_prob=REMIX_PROB, pitch_range=PITCH_RANGE,
                     stretch_range=None):
    """The augmentation of every item of one epoch with pitch shift, as PitchTable: StretchTable's eight rows plus pitch_v, pitch_a
    (int32 Q10).  Gains, song_v and song_a follow draw_epoch's rules; semitones are uniform in pitch_range and P =
    round(1024 2^(st / 12)) (a gain item's pitch_a is its pitch_v); rates follow draw_epoch_stretch's rule for `stretch_range`, or are
    all 1024 when that is None; starts are uniform in [0, max(T - span(q), 0)]: the pitch does not change the span.  A function of
    (seed, epoch) from a seed sequence of its own (it need not agree with the other two draws), so every rank draws the same table."""
    frames = np.asarray(frames_host, np.int64)
    n_songs = len(frames)
    if n_songs == 0 or n_items <= 0:
        return PitchTable(*(np.zeros(0, np.int32) for _ in range(4)), *(np.zeros(0, np.float32) for _ in range(2)),
                          *(np.zeros(0, np.int32) for _ in range(4)))
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), int(epoch), 0x70697463])))     # "pitc": its own sequence
    lo, hi = float(gain_range[0]), float(gain_range[1])
    song_v = np.arange(n_items, dtype=np.int64) % n_songs
    gain_v = rng.uniform(lo, hi, n_items).astype(np.float32)
    gain_a = rng.uniform(lo, hi, n_items).astype(np.float32)
    remix = rng.random(n_items) < float(remix_prob)
    other = rng.integers(0, n_songs, n_items)
    pitch_v = semitones_to_pitch(rng.uniform(float(pitch_range[0]), float(pitch_range[1]), n_items))
    pitch_a = np.where(remix, semitones_to_pitch(rng.uniform(float(pitch_range[0]), float(pitch_range[1]), n_items)), pitch_v)
    if stretch_range is None:
        rate_v = rate_a = np.full(n_items, RATE_ONE, np.int64)
    else:
        q_lo, q_hi = int(round(RATE_ONE * float(stretch_range[0]))), int(round(RATE_ONE * float(stretch_range[1])))
        rate_v = rng.integers(q_lo, q_hi, n_items, endpoint=True)
        rate_a = np.where(remix, rng.integers(q_lo, q_hi, n_items, endpoint=True), rate_v)
    start_v = rng.integers(0, np.maximum(frames[song_v] - span(rate_v, seg), 0), endpoint=True)
    start_a = rng.integers(0, np.maximum(frames[other] - span(rate_a, seg), 0), endpoint=True)
    song_a = np.where(remix, other, -1)
    start_a = np.where(remix, start_a, 0)
    i32 = lambda a: a.astype(np.int32)
    return PitchTable(i32(song_v), i32(start_v), i32(song_a), i32(start_a), gain_v, gain_a, i32(rate_v), i32(rate_a), i32(pitch_v), i32(pitch_a))


def check_pitch_table(table, frames_host, seg, has_angles=True):
    """check_stretch_table's rules on the first eight rows, and 512 <= P <= 2048 (pitch_a of a gain item is not read); the angles
    are required."""
    t = PitchTable(*(np.asarray(a) for a in table))
    n = len(t.song_v)
    if any(len(a) != n for a in t):
        raise ValueError(f"pitch table: rows of {[len(a) for a in t]} entries")
    if n == 0:
        return t
    if not has_angles:
        raise ValueError("pitch table: the pitch shift needs the angles of a set with *_phase.npy files")
    check_stretch_table(t[:len(STRETCH_ROWS)], frames_host, seg, True, what="pitch table")
    remix = t.song_a >= 0
    if (t.pitch_v < PITCH_MIN).any() or (t.pitch_v > PITCH_MAX).any():
        raise ValueError(f"pitch table: pitch_v outside {PITCH_MIN}..{PITCH_MAX} (Q10)")
    if (t.pitch_a[remix] < PITCH_MIN).any() or (t.pitch_a[remix] > PITCH_MAX).any():
        raise ValueError(f"pitch table: pitch_a outside {PITCH_MIN}..{PITCH_MAX} (Q10)")
    return t


def pack_pitch_table(table, items=None):
    """The (10, n) int32 host array of a PitchTable: pack_stretch_table's eight rows, then pitch_v, pitch_a; `items` picks and orders
    the columns."""
    packed = np.concatenate([pack_stretch_table(table[:len(STRETCH_ROWS)]), np.stack([np.asarray(a, np.int32) for a in table[len(STRETCH_ROWS):]])])
    return np.ascontiguousarray(packed if items is None else packed[:, np.asarray(items, np.int64)])


def upload_pitch_table(resident, table, items=None):
    """check_pitch_table, then the packed table of `items` as one (10, n) int32 device tensor: one pinned copy per epoch and rank."""
    import torch

    from .config import INPUT_LEN
    check_pitch_table(table, resident.frames_host, INPUT_LEN, resident.mix_ang is not None)
    return torch.from_numpy(pack_pitch_table(table, items)).pin_memory().to(resident.device, non_blocking=True)


def crop_pitch(resident, table, lo, hi, n_fft, hop, with_phase=False):
    """mix, voc [, mix_phase, voc_phase] (hi - lo, 1, rows, INPUT_LEN) on the device for items lo..hi-1 of `table`: an uploaded
    (10, n) tensor of upload_pitch_table, or a PitchTable, which is checked and uploaded first.  One svs_crop_pitch_tiles launch at
    the geometry (n_fft, hop) the set was written with."""
    import torch

    from . import _lib
    from .config import INPUT_LEN
    if isinstance(table, tuple):
        table = upload_pitch_table(resident, table)
    if resident.mix_ang is None:
        raise ValueError("the pitch shift needs the angles of a set with *_phase.npy files")
    if resident.rows != n_fft // 2:
        raise ValueError(f"the resident set has {resident.rows}-row tiles, n_fft {n_fft} needs {n_fft // 2}")
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[0] != len(PITCH_ROWS) or not table.is_contiguous() \
            or not (0 <= lo < hi <= table.shape[1]):
        raise ValueError(f"items {lo}..{hi} of a table of shape {tuple(table.shape)}")
    B = hi - lo
    out = [torch.empty((B, 1, resident.rows, INPUT_LEN), dtype=torch.float32, device=resident.device) for _ in range(4 if with_phase else 2)]
    row = [table[r, lo:hi].data_ptr() for r in range(len(PITCH_ROWS))]
    _lib.check(_lib.lib().svs_crop_pitch_tiles(resident.mix.data_ptr(), resident.voc.data_ptr(), resident.mix_ang.data_ptr(),
                                               resident.voc_ang.data_ptr(), resident.offsets.data_ptr(), resident.frames.data_ptr(), *row,
                                               B, resident.rows, INPUT_LEN, int(n_fft), int(hop), out[0].data_ptr(), out[1].data_ptr(),
                                               out[2].data_ptr() if with_phase else None, out[3].data_ptr() if with_phase else None,
                                               _lib.stream_ptr()), "svs_crop_pitch_tiles")
    return tuple(out)
