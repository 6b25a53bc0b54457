"""Pitch-shift augmentation on the device (-m gpu): svs_crop_pitch_tiles against the float64 definition (augment.pitch_reference).
Outputs are compared only through reconstituted complex values -- mix cis(mix_phase) against z, voc cis(voc_phase) against the
shifted vocal zv -- because an angle alone is ill-conditioned where its magnitude is small.

The bound is test_gpu_stretch.py's, derived the same way from the arithmetic of csrc/pitch.hip (u = 2^-23; the device library's
OpenCL-profile limits: 4 ulp for sin / cos / sqrt / hypot, 6 ulp for atan2; half an ulp, u / 2, per fp32 multiply, add, divide and
conversion), with three more terms:

  the second bin's interpolation.  Each of tm(j0), tm(j0 + 1) is the stretch's time interpolation (1.5 u for the vocal; each
  accompaniment point within 12 u (M + V), so 13.5 u (M + V)_interp).  The weights (P - r) / P and r / P are one division each
  (u / 2; r = N mod P and P are exact in fp32), the two products u / 2 each and the sum of two non-negative terms u / 2: 1.5 u more.
  The vocal's magnitude, gained, is within 3.5 u (the stretch: 2 u) and the accompaniment's within 16.5 u g_a (M + V)_interp
  (the stretch: 15 u), (M + V)_interp now interpolated in time and in bin (the reference's `scale`).

  the p-fold scaling of each atan2f difference error.  arg S of the accompaniment is off by at most 20 u kappa per source frame
  (kappa = (M + V) / |S|, as in the stretch).  acc_0 = arg S[j, s] carries that once; every later step adds p (arg S[j, k+1] -
  arg S[j, k]) and so p 20 u (kappa_k + kappa_(k+1)).  The reference's cond_a is exactly that sum: kappa of the first frame plus
  p times the running sum over the later frames of the phase bin j, and the term is 20 u cond_a, stated as 24 u cond_a.

  the fixed-point product.  The angles' conversions to 32-bit turns (2^-33 turn = 0.006 u rad each) also reach acc p-fold,
  0.006 u (1 + 2 p t), and (int64(d) P) >> 10 drops less than 2^-32 turn = 0.0123 u rad per frame: together at most
  0.006 u (1 + 2 p t) + 0.0123 u t <= u C (2 t + 1) (1 + p) with C = 1 / 64, for 0.5 <= p <= 2.  w' is an exact integer.

Everything after the two sources is the stretch's: 7.2 u per source for the accumulator's one rounding to fp32, sincosf and the
product; 16.5 u |z| for the sum, hypotf and atan2f; voc_phase's rounding to fp32, u.  The constant parts add up to at most
(3.5 + 7.2) u g_v V_interp + (16.5 + 7.2) u g_a (M + V)_interp + 16.5 u scale < 40.2 u scale, and the vocal's to 4.5 u:

    |voc cis(voc_phase) - zv| <= u |zv| (6 + C (2 t + 1) (1 + p_v))
    |mix cis(mix_phase) - z|  <= 50 u scale + u |zv| C (2 t + 1) (1 + p_v) + u |za| (24 cond_a + C (2 t + 1) (1 + p_a))

(50, 6 and 24 leave a fifth for the second-order terms, as the stretch's 48, 4 and 24 do.)

What the inputs must be.  V <= M / 2 and M >= 0.05 (kappa <= 3), one band of M = V = 0: the stretch's.  One condition is new: the
definition is discontinuous where a deviation d = wrap(arg S[j, k+1] - arg S[j, k] - w) is +-pi, because p d, unlike d, depends on
which turn the wrap removes -- at P = 1149 the two choices differ by 0.12 turn, in every later frame.  No evaluation in finite
precision can be bound to the definition inside the angle error (20 u kappa per angle, up to 1.4e-5 rad per deviation here) of that
point, and the uniform random angles of test_gpu_stretch.py put the nearest deviation of a production case 1e-6 to 2e-5 rad from it
(DESIGN.md section 19).  So the angles here advance by their bin's centre advance plus a jitter: phi[i, k] = k w_i + r,
|r| <= pi / 4, which keeps the vocal's |d| <= pi / 2 and the accompaniment's (arg S is within asin(V / M) <= pi / 6 of phi_m)
|d| <= 5 pi / 6.  The deviations at a song's end (the next frame is zero, arg 0) are arbitrary; `wrap_margin` computes in float64
the distance from +-pi of every deviation whose angles are not both exact zeros, and each case asserts it is above 1e-3 rad, a
hundred times the largest angle error.  (Where both magnitudes are 0 both angles are exactly 0 and d = -w exactly, in both
arithmetics.)  test_the_bound_has_teeth evaluates the definition with an fp32 accumulator and the unreduced advance in numpy and
shows it far outside this bound.

Worst error-to-bound ratios seen on an MI355X: see DESIGN.md section 19."""
import functools
import os

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import augment as au
from svs_unet_pytorch_amd import train as svs_train
from svs_unet_pytorch_amd.model import ALPHA_L1, ALPHA_MR, UNet

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.0
GUARD = 64                          # floats before and after every output (a multiple of 4: the tile stays 16-byte aligned)
NAN_TAIL = 64                       # floats of NaN after the last song of every resident buffer
U = 2.0 ** -23
A_Z, A_V, B_COND, C_T = 50.0, 6.0, 24.0, 1.0 / 64.0
STRETCH_A_Z, STRETCH_A_V = 48.0, 4.0                                       # test_gpu_stretch.py's, for the case of every pitch at 1024
MARGIN = 1e-3                       # rad: every deviation stays this far from +-pi (the angle errors are below 24 u 3 2 < 2e-5)


def conditioned(rng, F, T, n_fft, hop, zero_bin=None):
    """M >= 0.05, V <= M / 2 as fp32 (F, T) planes, one silent band; angles that advance by the centre advance of their bin plus a
    jitter within +-pi / 4, wrapped to [-pi, pi]: every deviation stays away from +-pi (the module docstring)."""
    M = (0.05 + rng.random((F, T))).astype(np.float32)
    V = (M * 0.5 * rng.random((F, T))).astype(np.float32)
    if zero_bin is not None:
        M[zero_bin] = V[zero_bin] = 0.0
    w = 2.0 * np.pi * ((hop * np.arange(1, F + 1, dtype=np.int64)) % n_fft) / n_fft

    def angles():
        a = w[:, None] * np.arange(T)[None, :] + rng.uniform(-np.pi / 4, np.pi / 4, (F, T))
        return (a - 2.0 * np.pi * np.round(a / (2.0 * np.pi))).astype(np.float32)
    return M, V, angles(), angles()


class Songs:
    """A resident set built by hand: per-song (F, T) planes (the float64 reference's inputs) and the flat device buffers with a NaN
    tail, so that a read past the last song shows as NaN in an output and never leaves the allocation."""

    def __init__(self, frames, F, n_fft, hop, seed, zero_bin=None):
        rng = np.random.default_rng(seed)
        self.frames_host, self.F, self.geometry = list(frames), F, (n_fft, hop)
        planes = [conditioned(rng, F, T, n_fft, hop, zero_bin) for T in frames]
        self.M, self.V, self.pm, self.pv = (list(p) for p in zip(*planes))
        flat = lambda parts: torch.from_numpy(np.concatenate([p.reshape(-1) for p in parts] + [np.full(NAN_TAIL, np.nan, np.float32)])).to(DEV)
        self.mix, self.voc, self.mix_ang, self.voc_ang = flat(self.M), flat(self.V), flat(self.pm), flat(self.pv)
        sizes = [F * T for T in frames]
        self.offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]), dtype=torch.int64, device=DEV)
        self.frames = torch.tensor(self.frames_host, dtype=torch.int32, device=DEV)

    def reference(self, table, seg):
        return au.pitch_reference(self.M, self.V, self.pm, self.pv, *table, seg, *self.geometry)

    def wrap_margin(self, table, seg):
        """The least distance from +-pi, in float64, of the deviations d that enter any accumulator of the items of `table`;
        deviations between two exactly zero magnitudes (d = -w exactly) are left out."""
        n_fft, hop = self.geometry
        as64 = lambda a: np.asarray(a, np.float64)
        least = np.pi
        for b in range(len(table.song_v)):
            A, Bs = int(table.song_v[b]), int(table.song_a[b])
            sources = [(as64(self.V[A]) * np.exp(1j * as64(self.pv[A])), table.start_v[b], table.rate_v[b], table.pitch_v[b])]
            if Bs < 0:
                Bs, s, q, P = A, table.start_v[b], table.rate_v[b], table.pitch_v[b]
            else:
                s, q, P = table.start_a[b], table.rate_a[b], table.pitch_a[b]
            sources.append((as64(self.M[Bs]) * np.exp(1j * as64(self.pm[Bs])) - as64(self.V[Bs]) * np.exp(1j * as64(self.pv[Bs])), s, q, P))
            for plane, s, q, P in sources:
                mag, arg = au._polar64(plane)
                n = np.arange(seg - 1, dtype=np.int64) * int(q)            # the step of the last frame enters nothing
                k = int(s) + (n >> 10)
                j0, _, j = au.pitch_bins(self.F, int(P))
                rows = j0 <= self.F                                        # above that the magnitude is 0 and the phase is not used
                j = j[rows]
                m0, m1 = au._columns(mag, k)[j - 1], au._columns(mag, k + 1)[j - 1]
                d = au._columns(arg, k + 1)[j - 1] - au._columns(arg, k)[j - 1] - (2.0 * np.pi * ((hop * j) % n_fft) / n_fft)[:, None]
                d -= 2.0 * np.pi * np.round(d / (2.0 * np.pi))
                dist = (np.pi - np.abs(d))[(m0 > 0) | (m1 > 0)]
                if dist.size:
                    least = min(least, float(dist.min()))
        return least


def table_of(items):
    """PitchTable from rows of (song_v, start_v, song_a, start_a, gain_v, gain_a, rate_v, rate_a, pitch_v, pitch_a)."""
    cols = list(zip(*items))
    i32, f32 = (lambda c: np.array(c, np.int32)), (lambda c: np.array(c, np.float32))
    return au.PitchTable(*(i32(c) for c in cols[:4]), *(f32(c) for c in cols[4:6]), *(i32(c) for c in cols[6:]))


def launch(entry, pack, rows, songs, table, seg, n_fft, hop, with_phase):
    B, F = len(table.song_v), songs.F
    n = B * F * seg
    dev_table = torch.from_numpy(pack(table)).to(DEV)
    bufs = [torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(4 if with_phase else 2)]
    ptrs = [b.data_ptr() + 4 * GUARD for b in bufs] + [None] * (4 - len(bufs))
    _lib.check(getattr(_lib.lib(), entry)(songs.mix.data_ptr(), songs.voc.data_ptr(), songs.mix_ang.data_ptr(), songs.voc_ang.data_ptr(),
                                          songs.offsets.data_ptr(), songs.frames.data_ptr(), *(dev_table[r].data_ptr() for r in range(rows)),
                                          B, F, seg, n_fft, hop, *ptrs, _lib.stream_ptr()), entry)
    out = []
    for b in bufs:
        h = b.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[GUARD + n:] == SENTINEL), "a guard float was overwritten"
        out.append(h[GUARD:GUARD + n].reshape(B, 1, F, seg))
    return out


def run(songs, table, seg, with_phase=True):
    """svs_crop_pitch_tiles into guarded buffers -> host tiles (mix, voc[, mix_phase, voc_phase]); the guards are checked here."""
    return launch("svs_crop_pitch_tiles", au.pack_pitch_table, 10, songs, table, seg, *songs.geometry, with_phase)


def bounds(ref, pitch_v, pitch_a, a_z=A_Z, a_v=A_V):
    """(bound on |mix cis(mix_phase) - z|, bound on |voc cis(voc_phase) - zv|): the module docstring's; pitch_a of a gain item
    already replaced by its pitch_v."""
    seg = ref.z.shape[-1]
    n = 2.0 * np.arange(seg) + 1.0
    n_v = n * (1.0 + np.asarray(pitch_v, np.float64) / 1024.0)[:, None, None, None]
    n_a = n * (1.0 + np.asarray(pitch_a, np.float64) / 1024.0)[:, None, None, None]
    zv, za = np.abs(ref.zv), np.abs(ref.z - ref.zv)
    b_z = a_z * U * ref.scale + U * zv * C_T * n_v + U * za * (B_COND * ref.cond_a + C_T * n_a)
    b_v = U * zv * (a_v + C_T * n_v)
    return b_z, b_v


def worst(e, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, e / b, np.where(e > 0, np.inf, 0.0))
    return float(r.max())


def ratios(got, ref, table, **kw):
    """(worst |mix cis(mix_phase) - z| / bound, worst |voc cis(voc_phase) - zv| / bound), an excess where the bound is 0 counting as inf."""
    mix, voc, mix_phase, voc_phase = (g.astype(np.float64) for g in got)
    b_z, b_v = bounds(ref, table.pitch_v, np.where(table.song_a < 0, table.pitch_v, table.pitch_a), **kw)
    return worst(np.abs(mix * np.exp(1j * mix_phase) - ref.z), b_z), worst(np.abs(voc * np.exp(1j * voc_phase) - ref.zv), b_v)


def check_against_reference(tag, songs, table, seg, report):
    au.check_pitch_table(table, songs.frames_host, seg)
    margin = songs.wrap_margin(table, seg)
    assert margin > MARGIN, f"{tag}: a deviation within {margin:.1e} rad of +-pi: the inputs are not conditioned"
    got = run(songs, table, seg)
    ref = songs.reference(table, seg)
    for name, g in zip(("mix", "voc", "mix_phase", "voc_phase"), got):
        assert np.isfinite(g).all(), f"{tag}: {name} has a NaN or an infinity (a read past a song's end?)"
    assert (np.abs(got[2]) <= np.float32(np.pi)).all() and (np.abs(got[3]) <= np.float32(np.pi)).all()
    assert not got[2][got[0] == 0].any() and not got[3][got[1] == 0].any(), f"{tag}: a phase where the magnitude is 0"
    assert not got[0][ref.mix == 0].any() and not got[1][ref.voc == 0].any(), f"{tag}: a magnitude where the definition has exactly 0"
    r_z, r_v = ratios(got, ref, table)
    print(f"{tag}: worst |mix cis(mix_phase) - z| / bound {r_z:.3f}, worst |voc cis(voc_phase) - zv| / bound {r_v:.3f}, wrap margin {margin:.3f} rad")
    ok_z = report(f"{tag}: |mix cis(mix_phase) - z| over its bound", r_z, 1.0)
    ok_v = report(f"{tag}: |voc cis(voc_phase) - zv| over its bound", r_v, 1.0)
    assert ok_z and ok_v, (r_z, r_v)
    return got, ref


# ---- the small shape: every padding case and every edge of the bin arithmetic -----------------------------------------------

SMALL_FRAMES, SMALL_F, SMALL_SEG, SMALL_GEOMETRY = [3, 8, 11, 37], 6, 8, (512, 384)
# (song_v, start_v, song_a, start_a, gain_v, gain_a, rate_v, rate_a, pitch_v, pitch_a); span(q) at seg 8: 512 -> 5, 819 -> 7,
# 1024 -> 9, 1333 -> 11, 2048 -> 16.  At F = 6: P = 512 reads bins 2 b (rows 4..6 fall off the top: exactly 0); P = 2048 reads
# b / 2 (row 1: j0 = 0, the silent DC row, at weight 1/2; odd rows tie at .5 and take the upper bin's phase); P = 768 reads
# 4 b / 3 (row 3 is bin 4 exactly, row 6 is bin 8: off the top)
SMALL_ITEMS = [
    (3, 28, 2, 6, 0.4, 1.2, 1024, 512, 512, 2048),       # both starts at room(q); the two ends of the pitch range
    (3, 21, 3, 2, 0.8, 0.5, 2048, 1333, 2048, 512),      # A = B; q = 2048 from room(q): the last read is frame 36
    (3, 7, 3, 7, 1.0, 1.0, 819, 819, 768, 768),          # A = B, the same start, rate and pitch, gains 1; an exact-integer b / p
    (1, 0, -1, 0, 0.7, 0.9, 1024, 7, 1149, 7),           # a gain item on the song that fills its tile; rate_a and pitch_a unused
    (0, 0, 3, 0, 1.1, 0.9, 1333, 2048, 913, 1448),       # the vocal source ends mid-tile (3 frames), the accompaniment goes on
    (2, 0, 0, 0, 0.6, 1.25, 2048, 1024, 1448, 724),      # the accompaniment source ends (3 frames); the vocal ends later
    (0, 0, 0, 0, 0.25, 0.3, 512, 1024, 2048, 512),       # both sources ended
    (1, 0, -1, 0, 1.0, 1.0, 1333, 1024, 1024, 1024),     # a gain item whose source ends mid-tile, at pitch 1
]


@functools.lru_cache(maxsize=None)
def small_songs():
    return Songs(SMALL_FRAMES, SMALL_F, *SMALL_GEOMETRY, seed=1, zero_bin=2)


def test_small_shape_against_the_definition(report):
    songs, table = small_songs(), table_of(SMALL_ITEMS)
    got, ref = check_against_reference("crop_pitch small (8, 6, 8)", songs, table, SMALL_SEG, report)
    mix, voc, mix_phase, voc_phase = got
    assert voc[0, 0, :3, :].any(axis=1).all() and not voc[0, 0, 3:].any() and not voc_phase[0, 0, 3:].any()     # P = 512: rows 4..6 read bins 8, 10, 12
    assert mix[0, 0, 3].all() and mix[0, 0, 4].all() and not mix[0, 0, 5].any()    # the accompaniment (P = 2048) reads bins 2, 2.5 and 3, the silent band
    assert voc[1, 0, 0, :].all()                                           # P = 2048, row 1: half of bin 1 (j0 = 0 is the silent DC row)
    assert not voc[2, 0, 5].any() and not mix[2, 0, 5].any() and not mix_phase[2, 0, 5].any()          # P = 768, row 6 reads bin 8: both sources
    assert voc[2, 0, 2].all()                                              # row 3 reads bin 4 exactly
    assert voc[4, 0, 0, :2].all() and not voc[4, 0, :, 3:].any() and mix[4, 0, 0, 3:].all()            # q = 1333 on 3 frames: then padding
    assert not mix[6, 0, :, 6:].any() and not mix_phase[6, 0, :, 6:].any()                             # both sources ended
    assert np.abs(ref.z[2] - ref.zv[2]).max() > 0.01


def test_the_full_scan_of_a_row(report):
    """F = 8, seg = 128: two rounds of 64 lanes, the carry of the first into the second, at each rate and several pitches."""
    songs = Songs([400, 150], 8, 512, 128, seed=3, zero_bin=5)
    table = table_of([(0, 144, 1, 3, 0.9, 0.6, 2048, 819, 1149, 913),      # start_v = room(2048) = 400 - 256
                      (0, 17, 0, 230, 0.5, 1.1, 1333, 1333, 724, 1448),
                      (1, 0, 0, 335, 1.25, 0.25, 1024, 512, 2048, 512),    # the 150-frame song: 129 of them; start_a = room(512) = 400 - 65
                      (1, 0, -1, 0, 0.8, 0.8, 1333, 0, 913, 0)])           # a gain item whose source ends at output frame 115
    got, _ = check_against_reference("crop_pitch scan (4, 8, 128)", songs, table, 128, report)
    assert got[1][3, 0, 0, :116].all() and not got[1][3, 0, :, 116:].any()


@pytest.mark.parametrize("n_fft,hop", [(1024, 768), (512, 384)])
def test_production_shape_against_the_definition(n_fft, hop, report):
    """The command line's geometry; P in {913, 1024, 1149} and q in {819, 1024, 1333} over the six sources of three items."""
    songs = Songs([100, 128, 300, 517], n_fft // 2, n_fft, hop, seed=2)
    table = table_of([(2, 133, 3, 350, 0.3, 1.25, 1333, 1333, 913, 1149),  # both starts at room(1333) = T - 167
                      (3, 2, 0, 0, 1.25, 0.25, 1024, 819, 1149, 1024),     # the short song (100 frames) as accompaniment
                      (1, 0, -1, 0, 0.5, 1.0, 819, 819, 1024, 1024)])      # a gain item: 104 of the 128 frames of its song
    check_against_reference(f"crop_pitch production (3, {n_fft // 2}, 128) at ({n_fft}, {hop})", songs, table, 128, report)


def test_the_64_bit_product(report):
    """(2048, 2048), F = 1024, P = 2048 and 2047; the gain item's P = 1025 reads j = 1023 at the top row, where hop j P is just above
    2^31 (with rows 1..F the product stays below 2^32 and leaves a signed 32-bit one; neither 2047 nor 1025 is a power of two that
    would hide a truncated product behind the reduction mod 1024 n_fft)."""
    songs = Songs([40, 30], 1024, 2048, 2048, seed=4, zero_bin=700)
    table = table_of([(0, 5, 1, 3, 0.9, 0.6, 1024, 1333, 2048, 2047),
                      (1, 2, -1, 0, 0.7, 1.0, 819, 0, 1025, 0)])
    check_against_reference("crop_pitch (2, 1024, 16) at (2048, 2048)", songs, table, 16, report)


def test_the_bound_has_teeth():
    """numpy only: the definition with an fp32 accumulator and the unreduced scaled advance p 2 pi hop j / n_fft (about 2,700 rad per
    frame at the top bin of (1024, 768) at P = 1149) leaves the bound by orders of magnitude at frame 127."""
    n_fft, hop, F, seg, T, s, q, P = 1024, 768, 512, 128, 300, 5, 1333, 1149
    rng = np.random.default_rng(8)
    M, V, pm, pv = conditioned(rng, F, T, n_fft, hop)
    g = np.ones(1, np.float32)
    ref = au.pitch_reference([M], [V], [pm], [pv], [0], [s], [-1], [0], g, g, [q], [q], [P], [P], seg, n_fft, hop)
    n = np.arange(seg) * q
    k, alpha = s + (n >> 10), ((n & 1023) / 1024.0).astype(np.float32)
    j0, gamma, j = au.pitch_bins(F, P)
    p32, two_pi = np.float32(P / 1024.0), np.float32(2.0 * np.pi)
    w = (2.0 * np.pi * hop * j / n_fft).astype(np.float32)[:, None]                                 # unreduced
    d = (pv[j - 1][:, k + 1] - pv[j - 1][:, k]) - w
    d = d - two_pi * np.round(d / two_pi)
    step = p32 * w + p32 * d
    acc = np.empty((F, seg), np.float32)
    acc[:, 0] = pv[j - 1, s]
    for t in range(1, seg):
        acc[:, t] = acc[:, t - 1] + step[:, t - 1]                         # the plain fp32 accumulator
    tm = (np.float32(1) - alpha) * V[:, k] + alpha * V[:, k + 1]
    tm = np.concatenate([tm, np.zeros((F + 2, seg), np.float32)])          # bins above F are silent
    rem = (1024 * np.arange(1, F + 1)) % P                                 # the kernel's weights: (P - r) / P and r / P, one division each
    lo, hi = (np.float32(P) - rem.astype(np.float32)) / np.float32(P), rem.astype(np.float32) / np.float32(P)
    mag = lo[:, None] * tm[j0 - 1] + hi[:, None] * tm[j0]                  # (row 1 has j0 = 0: index -1 is a silent row, as the DC row is)
    lossy = mag.astype(np.float64) * np.exp(1j * acc.astype(np.float64))
    _, b_v = bounds(ref, [P], [P])
    e = np.abs(lossy - ref.zv[0, 0])
    last = e[:, -1] / b_v[0, 0, :, -1]
    print(f"fp32 accumulator, frame 127: error / bound median {np.median(last):.0f}, worst {last.max():.0f}; "
          f"error / |zv| median {np.median(e[:, -1] / np.abs(ref.zv[0, 0, :, -1])):.3f}")
    assert np.median(last) > 100.0 and last.max() > 1000.0
    exact = mag.astype(np.float64) * np.exp(1j * ref.voc_phase[0, 0])                               # the same magnitudes with the true phase
    assert worst(np.abs(exact - ref.zv[0, 0]), b_v[0, 0]) <= 1.0


# ---- bit for bit -----------------------------------------------------------------------------------------------------------

def test_an_item_alone_in_a_batch_and_repeated():
    songs, items = small_songs(), SMALL_ITEMS
    whole = run(songs, table_of(items), SMALL_SEG)
    again = run(songs, table_of(items), SMALL_SEG)
    for w, a in zip(whole, again):
        assert np.array_equal(w, a)
    for b in (0, 4, len(items) - 1):
        alone = run(songs, table_of([items[b]]), SMALL_SEG)
        for w, a in zip(whole, alone):
            assert np.array_equal(w[b], a[0]), b
    big = Songs([300, 200], 256, 512, 384, seed=6)
    items = [(0, 3, 1, 20, 0.9, 0.6, 1333, 819, 913, 1149), (1, 30, -1, 0, 0.3, 1.1, 1024, 0, 1448, 0), (1, 7, 0, 40, 0.7, 0.7, 512, 2048, 2048, 724)]
    rev = items[::-1] * 12                                                 # 36 items: 9216 rows, more than one row per wave of the grid
    whole = run(big, table_of(rev), 128)
    for b in (2, 1, 0):
        alone = run(big, table_of([rev[b]]), 128)
        for w, a in zip(whole, alone):
            assert np.array_equal(w[b], a[0]) and np.array_equal(w[b + 33], a[0]), b


def test_without_phase_outputs_mix_and_voc_are_the_same():
    songs, table = small_songs(), table_of(SMALL_ITEMS)
    full, lean = run(songs, table, SMALL_SEG, with_phase=True), run(songs, table, SMALL_SEG, with_phase=False)
    assert len(lean) == 2 and np.array_equal(lean[0], full[0]) and np.array_equal(lean[1], full[1])
    big = Songs([300, 200], 256, 512, 384, seed=5)
    t2 = table_of([(0, 3, 1, 20, 0.9, 0.6, 1333, 819, 1149, 913), (1, 30, 0, 12, 0.3, 1.1, 1024, 2048, 724, 1448)])
    full, lean = run(big, t2, 128, with_phase=True), run(big, t2, 128, with_phase=False)
    assert np.array_equal(lean[0], full[0]) and np.array_equal(lean[1], full[1])


def test_pitch_one_is_the_stretch_launch(report):
    """Every pitch at 1024: voc_phase is bit for bit svs_crop_stretch_tiles' (the accumulator is the stretch's, to the bit), and the
    other outputs stay within the stretch's own bound against the stretch's own reference."""
    for songs, items, seg in ((small_songs(), SMALL_ITEMS, SMALL_SEG),
                              (Songs([300, 200], 256, 512, 384, seed=7, zero_bin=9),
                               [(0, 3, 1, 20, 0.9, 0.6, 1333, 819, 0, 0), (1, 30, -1, 0, 0.3, 1.1, 1024, 0, 0, 0), (1, 7, 0, 40, 0.7, 0.7, 512, 2048, 0, 0)], 128)):
        table = table_of([it[:8] + (1024, 1024) for it in items])
        stretch_table = au.StretchTable(*table[:8])
        got = run(songs, table, seg)
        old = launch("svs_crop_stretch_tiles", au.pack_stretch_table, 8, songs, stretch_table, seg, *songs.geometry, True)
        assert np.array_equal(got[3], old[3])
        ref = au.stretch_reference(songs.M, songs.V, songs.pm, songs.pv, *stretch_table, seg, *songs.geometry)
        seg_n = (2.0 * np.arange(seg) + 1.0)
        zv, za = np.abs(ref.zv), np.abs(ref.z - ref.zv)
        b_z = STRETCH_A_Z * U * ref.scale + U * zv * C_T * seg_n + U * za * (B_COND * ref.cond_a + C_T * seg_n)
        b_v = U * zv * (STRETCH_A_V + C_T * seg_n)
        mix, voc, mix_phase, voc_phase = (g.astype(np.float64) for g in got)
        r_z, r_v = worst(np.abs(mix * np.exp(1j * mix_phase) - ref.z), b_z), worst(np.abs(voc * np.exp(1j * voc_phase) - ref.zv), b_v)
        print(f"pitch 1024, seg {seg}: ratios to the stretch's bound {r_z:.3f} {r_v:.3f}")
        ok = report(f"crop_pitch at pitch 1, seg {seg}: |mix cis(mix_phase) - z| over the stretch's bound", r_z, 1.0)
        ok = report(f"crop_pitch at pitch 1, seg {seg}: |voc cis(voc_phase) - zv| over the stretch's bound", r_v, 1.0) and ok
        assert ok, (r_z, r_v)


# ---- ResidentSpectrograms.augmented_batches --------------------------------------------------------------------------------

FOLDER_FRAMES = [100, 200, 333]      # one song shorter than the 128-frame tile
PER_SONG = 4


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """A synthetic folder of 3 well-conditioned songs at win 512: 257-row magnitude files with unit-phasor phase files."""
    root = tmp_path_factory.mktemp("pitch_set")
    rng = np.random.default_rng(11)
    for d in ("mixture", "vocal"):
        os.makedirs(root / d)
    for i, T in enumerate(FOLDER_FRAMES):
        M, V, pm, pv = conditioned(rng, 257, T, 512, 384)
        for d, mag, ang in (("mixture", M, pm), ("vocal", V, pv)):
            np.save(root / d / f"{i:04d}_song_spec.npy", mag)
            np.save(root / d / f"{i:04d}_song_phase.npy", np.exp(1j * ang.astype(np.float64)).astype(np.complex64))
    return root


@pytest.fixture(scope="module")
def resident(folder):
    dataset = svs_train.SpectrogramDataset(str(folder), samples_per_song=PER_SONG, win_size=512)
    return svs_train.ResidentSpectrograms(dataset, torch.device(DEV))


def test_augmented_batches_take_the_pitch_path_only_with_a_range(resident):
    assert resident.rows == 256 and resident.has_phase and len(resident) == 12
    gains, prob, seed, epoch = (0.25, 1.25), 0.75, 9, 2
    order = svs_train.epoch_order(len(resident), True, 1, 2, epoch)
    # without pitch_range: the remix path and the stretch path, bit for bit what they are today
    a = next(resident.augmented_batches(4, 1, 2, epoch, with_phase=True, aug=au.Augment("remix", gains, prob, seed)))
    table = au.upload_table(resident, au.draw_epoch(len(resident), resident.frames_host, 128, epoch, seed, gains, prob), order)
    for x, y in zip(a, au.crop_remix(resident, table, 0, 4, True)):
        assert torch.equal(x, y)
    a = next(resident.augmented_batches(4, 1, 2, epoch, with_phase=True, aug=au.Augment("remix", gains, prob, seed, (0.8, 1.25)), hop=384))
    table = au.upload_stretch_table(resident, au.draw_epoch_stretch(len(resident), resident.frames_host, 128, epoch, seed, gains, prob, (0.8, 1.25)), order)
    for x, y in zip(a, au.crop_stretch(resident, table, 0, 4, 512, 384, True)):
        assert torch.equal(x, y)
    # with it: draw_epoch_pitch's table, one crop_pitch per batch, with and without a stretch
    for stretch in (None, (0.8, 1.25)):
        aug = au.Augment("remix", gains, prob, seed, stretch, (-2.0, 2.0))
        drawn = au.draw_epoch_pitch(len(resident), resident.frames_host, 128, epoch, seed, gains, prob, (-2.0, 2.0), stretch)
        assert (drawn.song_a >= 0).any() and (drawn.song_a < 0).any() and len(set(drawn.pitch_v.tolist())) > 6
        table = au.upload_pitch_table(resident, drawn, order)
        assert table.shape == (10, 6) and table.dtype == torch.int32
        batches = list(resident.augmented_batches(4, 1, 2, epoch, with_phase=True, aug=aug, hop=384))
        assert [b[0].shape for b in batches] == [(4, 1, 256, 128), (2, 1, 256, 128)] and all(len(b) == 4 for b in batches)
        for lo, batch in zip((0, 4), batches):
            for x, y in zip(batch, au.crop_pitch(resident, table, lo, min(lo + 4, 6), 512, 384, True)):
                assert torch.equal(x, y) and torch.isfinite(x).all()
        two = list(resident.augmented_batches(4, 1, 2, epoch, with_phase=False, aug=aug, hop=384))
        assert all(len(b) == 2 for b in two) and torch.equal(two[0][0], batches[0][0]) and torch.equal(two[1][1], batches[1][1])
        plain = next(resident.augmented_batches(4, 1, 2, epoch, with_phase=True, aug=au.Augment("remix", gains, prob, seed, stretch), hop=384))
        assert not torch.equal(plain[0], batches[0][0])


def test_one_training_step_on_a_shifted_batch(resident):
    """The full objective (L1 + MR-STFT) at win 512 / hop 384 on a shifted and stretched batch: finite losses, parameters that moved."""
    model = UNet().to(DEV).train()
    before = model.state_dict()["conv1.0.weight"].detach().clone()
    aug = au.Augment("remix", (0.25, 1.25), 1.0, seed=1, stretch_range=(0.8, 1.25), pitch_range=(-2.0, 2.0))
    mix, voc, mph, vph = next(resident.augmented_batches(4, 0, 1, 0, with_phase=True, aug=aug, hop=384))
    l1 = model.train_step(mix, voc, loss_scale=ALPHA_L1, mix_phase=mph, voc_phase=vph, alpha_mr=ALPHA_MR, hop=384)
    l1, mr = float(l1), float(model.last_mr_loss)
    assert np.isfinite(l1) and l1 > 0 and np.isfinite(mr) and mr > 0, (l1, mr)
    after = model.state_dict()["conv1.0.weight"]
    assert torch.isfinite(after).all() and (after - before).abs().max().item() > 0


def test_train_cli_with_the_flag(folder, tmp_path, monkeypatch, capsys):
    """train.py --augment remix --pitch_range -2 2 for one epoch (full objective, win 512): the settings line names the range, every
    step is one crop_pitch launch at the folder's geometry, and the checkpoint has the keys it always had."""
    monkeypatch.chdir(tmp_path)
    calls = []
    real = au.crop_pitch

    def counted(res, table, lo, hi, n_fft, hop, with_phase=False):
        calls.append((n_fft, hop, with_phase))
        return real(res, table, lo, hi, n_fft, hop, with_phase)

    def forbidden(*args, **kw):
        raise AssertionError("--pitch_range reached another launch")
    monkeypatch.setattr(au, "crop_pitch", counted)
    monkeypatch.setattr(au, "crop_remix", forbidden)
    monkeypatch.setattr(au, "crop_stretch", forbidden)
    svs_train.main(["--train_folder", str(folder), "--valid_folder", str(tmp_path / "no_valid"), "--batch_size", "32", "--epoch", "1",
                    "--load_path", "none.pth", "--win_size", "512", "--hop_size", "384", "--label", "pt", "--augment", "remix",
                    "--pitch_range", "-2", "2", "--augment_seed", "3"])
    lines = capsys.readouterr().out.splitlines()
    line = [l for l in lines if l.startswith("Augmentation:")]
    assert len(line) == 1 and "pitch-shifted" in line[0] and "[-2.0, 2.0]" in line[0] and "not a tuned value" in line[0] \
        and "time-stretched" not in line[0] and "seed 3" in line[0], lines
    from svs_unet_pytorch_amd.config import SAMPLES_PER_SONG
    assert calls == [(512, 384, True)] * -(-len(FOLDER_FRAMES) * SAMPLES_PER_SONG // 32)                # one launch per step
    value = float(open(tmp_path / "LOG" / "log_pt.txt").read().split()[0])
    assert np.isfinite(value) and value > 0
    ck = torch.load(tmp_path / "CKPT" / "svs_pt.pth", map_location="cpu")
    assert ck["epoch"] == 1 and "pitch_range" not in ck and "stretch_range" not in ck
