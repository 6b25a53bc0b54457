"""Time-stretch augmentation on the device (-m gpu): svs_crop_stretch_tiles against the float64 definition
(augment.stretch_reference).  Outputs are compared only through reconstituted complex values -- mix cis(mix_phase) against z,
voc cis(voc_phase) against the stretched vocal zv -- because an angle alone is ill-conditioned where its magnitude is small.

The bound, from the arithmetic of csrc/stretch.hip (u = 2^-23; the device library's OpenCL-profile limits: 4 ulp for sin / cos /
sqrt / hypot, 6 ulp for atan2; half an ulp, u / 2, per fp32 multiply, add and conversion):

  vocal source.  mag_v = (1 - a) V[k] + a V[k+1] is two products and a sum of non-negative terms (a, 1 - a exact): 1.5 u; times g_v:
  2 u.  The resident angles are the definition's own inputs; each becomes a 32-bit fraction of a turn with one rounding from fp64
  (2^-33 turn = 0.006 u rad) and the sums are exact integers, so after the 2 t + 1 source frames that entered it acc_v is off by at
  most 0.006 u (2 t + 1) rad: a term in t alone, with no factor hop * bin / n_fft (the expected advance cancels identically in
  wrapping arithmetic).  voc_phase is acc_v rounded to fp32 once, at most u rad (half an ulp below 4).  Hence

      |voc cis(voc_phase) - zv| <= u |zv| (4 + C (2 t + 1))                                    C = 1 / 64

  accompaniment source.  Re and Im of M cis(phi_m) - V cis(phi_v) carry 4 u (M + V) from sin / cos and 1.5 u (M + V) from two
  products and a difference: |delta S| <= sqrt(2) 5.5 u (M + V) < 8 u (M + V).  |S| by hypotf: + 4 u |S|, so each frame's magnitude is
  within 12 u (M + V) and the interpolated, gained one within 15 u g_a (M + V)_interp.  arg S by atan2f: the angle moves by at most
  |delta S| / |S| = 8 u kappa, kappa = (M + V) / |S| >= 1, plus 6 ulp of a value below 4 (12 u <= 12 u kappa): 20 u kappa per frame,
  and acc_a, an exact sum of such angles, is off by at most 20 u cond_a + 0.006 u (2 t + 1) with cond_a the running sum of kappa over
  the frames that entered acc (the reference returns it).

  each source's cis: acc rounded to fp32 (u rad), sincosf (4 ulp on each of sin and cos: 5.7 u), the product with the magnitude
  (u / 2): 7.2 u |source|; the sum z: u / 2 |z|; mix = hypotf: 4 u |z|; mix_phase = atan2f: 12 u |z|.  With |zv| <= g_v V_interp,
  |za| <= g_a (M + V)_interp and |z| <= scale = g_v V_interp + g_a (M + V)_interp, the constant parts add up to at most
  (2 + 7.2) u g_v V_interp + (15 + 7.2) u g_a (M + V)_interp + 16.5 u scale < 40 u scale, and

      |mix cis(mix_phase) - z| <= 48 u scale + u |zv| C (2 t + 1) + u |za| (24 cond_a + C (2 t + 1))

(A = 48, B = 24 and C = 1 / 64 leave a fifth for the second-order terms.)  The inputs are well conditioned by construction,
V <= M / 2 and M >= 0.05, so kappa <= 3 by the triangle inequality, with one band of M = V = 0.  test_the_bound_has_teeth evaluates
the definition with an fp32 accumulator and the unreduced advance in numpy and shows it far outside this bound.

Worst error-to-bound ratios seen on an MI355X: see DESIGN.md section 18."""
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
A_Z, A_V, B_COND, C_T = 48.0, 4.0, 24.0, 1.0 / 64.0


def conditioned(rng, F, T, zero_bin=None):
    """M >= 0.05, V <= M / 2 and uniform angles as fp32 (F, T) planes; one silent band."""
    M = (0.05 + rng.random((F, T))).astype(np.float32)
    V = (M * 0.5 * rng.random((F, T))).astype(np.float32)
    if zero_bin is not None:
        M[zero_bin] = V[zero_bin] = 0.0
    return M, V, rng.uniform(-np.pi, np.pi, (F, T)).astype(np.float32), rng.uniform(-np.pi, np.pi, (F, T)).astype(np.float32)


class Songs:
    """A resident set built by hand: per-song (F, T) planes (the float64 reference's inputs) and the flat device buffers with a NaN
    tail, so that a read past the last song shows as NaN in an output and never leaves the allocation."""

    def __init__(self, frames, F, seed, zero_bin=None):
        rng = np.random.default_rng(seed)
        self.frames_host, self.F = list(frames), F
        planes = [conditioned(rng, F, T, zero_bin) for T in frames]
        self.M, self.V, self.pm, self.pv = (list(p) for p in zip(*planes))
        for p in self.pm + self.pv:                                        # the ends of atan2f's range occur too
            p[0, 0], p[-1, -1] = np.float32(np.pi), np.float32(-np.pi)
        flat = lambda parts: torch.from_numpy(np.concatenate([p.reshape(-1) for p in parts] + [np.full(NAN_TAIL, np.nan, np.float32)])).to(DEV)
        self.mix, self.voc, self.mix_ang, self.voc_ang = flat(self.M), flat(self.V), flat(self.pm), flat(self.pv)
        sizes = [F * T for T in frames]
        self.offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]), dtype=torch.int64, device=DEV)
        self.frames = torch.tensor(self.frames_host, dtype=torch.int32, device=DEV)

    def reference(self, table, seg, n_fft, hop):
        return au.stretch_reference(self.M, self.V, self.pm, self.pv, *table, seg, n_fft, hop)


def table_of(items):
    """StretchTable from rows of (song_v, start_v, song_a, start_a, gain_v, gain_a, rate_v, rate_a)."""
    cols = list(zip(*items))
    i32, f32 = (lambda c: np.array(c, np.int32)), (lambda c: np.array(c, np.float32))
    return au.StretchTable(*(i32(c) for c in cols[:4]), *(f32(c) for c in cols[4:6]), *(i32(c) for c in cols[6:]))


def run(songs, table, seg, n_fft, hop, with_phase=True):
    """svs_crop_stretch_tiles into guarded buffers -> host tiles (mix, voc[, mix_phase, voc_phase]); the guards are checked here."""
    B, F = len(table.song_v), songs.F
    n = B * F * seg
    dev_table = torch.from_numpy(au.pack_stretch_table(table)).to(DEV)
    bufs = [torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(4 if with_phase else 2)]
    ptrs = [b.data_ptr() + 4 * GUARD for b in bufs] + [None] * (4 - len(bufs))
    _lib.check(_lib.lib().svs_crop_stretch_tiles(songs.mix.data_ptr(), songs.voc.data_ptr(), songs.mix_ang.data_ptr(), songs.voc_ang.data_ptr(),
                                                 songs.offsets.data_ptr(), songs.frames.data_ptr(), *(dev_table[r].data_ptr() for r in range(8)),
                                                 B, F, seg, n_fft, hop, *ptrs, _lib.stream_ptr()), "svs_crop_stretch_tiles")
    out = []
    for b in bufs:
        h = b.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[GUARD + n:] == SENTINEL), "a guard float was overwritten"
        out.append(h[GUARD:GUARD + n].reshape(B, 1, F, seg))
    return out


def bounds(ref):
    """(bound on |mix cis(mix_phase) - z|, bound on |voc cis(voc_phase) - zv|): the module docstring's."""
    seg = ref.z.shape[-1]
    n = 2.0 * np.arange(seg) + 1.0                                         # source frames that entered acc by frame t
    zv, za = np.abs(ref.zv), np.abs(ref.z - ref.zv)
    b_z = A_Z * U * ref.scale + U * zv * C_T * n + U * za * (B_COND * ref.cond_a + C_T * n)
    b_v = U * zv * (A_V + C_T * n)
    return b_z, b_v


def worst(e, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, e / b, np.where(e > 0, np.inf, 0.0))
    return float(r.max())


def ratios(got, ref):
    """(worst |mix cis(mix_phase) - z| / bound, worst |voc cis(voc_phase) - zv| / bound), an excess where the bound is 0 counting as inf."""
    mix, voc, mix_phase, voc_phase = (g.astype(np.float64) for g in got)
    b_z, b_v = bounds(ref)
    return worst(np.abs(mix * np.exp(1j * mix_phase) - ref.z), b_z), worst(np.abs(voc * np.exp(1j * voc_phase) - ref.zv), b_v)


def check_against_reference(tag, songs, table, seg, n_fft, hop, report):
    got = run(songs, table, seg, n_fft, hop)
    ref = songs.reference(table, seg, n_fft, hop)
    for name, g in zip(("mix", "voc", "mix_phase", "voc_phase"), got):
        assert np.isfinite(g).all(), f"{tag}: {name} has a NaN or an infinity (a read past a song's end?)"
    assert (np.abs(got[2]) <= np.float32(np.pi)).all() and (np.abs(got[3]) <= np.float32(np.pi)).all()
    assert not got[2][got[0] == 0].any() and not got[3][got[1] == 0].any(), f"{tag}: a phase where the magnitude is 0"
    assert not got[0][ref.mix == 0].any() and not got[1][ref.voc == 0].any(), f"{tag}: a magnitude where the definition has exactly 0"
    r_z, r_v = ratios(got, ref)
    print(f"{tag}: worst |mix cis(mix_phase) - z| / bound {r_z:.3f}, worst |voc cis(voc_phase) - zv| / bound {r_v:.3f}")
    ok_z = report(f"{tag}: |mix cis(mix_phase) - z| over its bound", r_z, 1.0)
    ok_v = report(f"{tag}: |voc cis(voc_phase) - zv| over its bound", r_v, 1.0)
    assert ok_z and ok_v, (r_z, r_v)
    return got, ref


# ---- the small shape: every padding case ---------------------------------------------------------------------------------

SMALL_FRAMES, SMALL_F, SMALL_SEG, SMALL_GEOMETRY = [3, 8, 11, 37], 6, 8, (512, 384)
# (song_v, start_v, song_a, start_a, gain_v, gain_a, rate_v, rate_a); span(q) at seg 8: 512 -> 5, 819 -> 7, 1024 -> 9, 1333 -> 11,
# 2048 -> 16, so room(q) = max(T - span(q), 0) of the 37-frame song is 32, 30, 28, 26, 21
SMALL_ITEMS = [
    (3, 28, 2, 6, 0.4, 1.2, 1024, 512),      # both starts at room(q); q = 512: every source frame is used twice
    (3, 21, 3, 2, 0.8, 0.5, 2048, 1333),     # A = B; q = 2048 from room(q): every other frame is skipped, the last read is frame 36
    (3, 7, 3, 7, 1.0, 1.0, 819, 819),        # A = B, the same start and rate, gains 1: the item's own sources
    (1, 0, -1, 0, 0.7, 0.9, 1024, 7),        # a gain item on the song that fills its tile (frame 8 reads as 0 at weight 0); rate_a unused
    (0, 0, 3, 0, 1.1, 0.9, 1333, 2048),      # the vocal source ends mid-tile (3 frames), the accompaniment goes on
    (2, 0, 0, 0, 0.6, 1.25, 2048, 1024),     # the accompaniment source ends (3 frames); the vocal (11 frames at q = 2048) ends later
    (0, 0, 0, 0, 0.25, 0.3, 512, 1024),      # both sources ended
    (1, 0, -1, 0, 1.0, 1.0, 1333, 1024),     # a gain item whose source ends mid-tile (8 frames, span 11)
]


@functools.lru_cache(maxsize=None)
def small_songs():
    return Songs(SMALL_FRAMES, SMALL_F, seed=1, zero_bin=2)


def test_small_shape_against_the_definition(report):
    songs, table = small_songs(), table_of(SMALL_ITEMS)
    au.check_stretch_table(table, SMALL_FRAMES, SMALL_SEG)
    got, ref = check_against_reference("crop_stretch small (8, 6, 8)", songs, table, SMALL_SEG, *SMALL_GEOMETRY, report)
    mix, voc, mix_phase, voc_phase = got
    live = [0, 1, 3, 4, 5]                                                 # the rows that are not the silent band
    assert voc[4, 0, live, :2].all() and not voc[4, 0, :, 3:].any() and mix[4, 0, live, 3:].all()     # q = 1333: frames 0, 1, 2(.6), then padding
    assert voc[5, 0, live, :5].all() and not voc[5, 0, :, 6:].any() and mix[5, 0, live, :5].all() and not mix[5, 0, :, 6:].any()
    assert mix[6, 0, live, :6].all() and not mix[6, 0, :, 6:].any() and not mix_phase[6, 0, :, 6:].any()
    assert voc[7, 0, live, :6].all() and not voc[7, 0, :, 7:].any()
    for b in range(len(SMALL_ITEMS)):                                      # the silent band: exactly 0 in, exactly 0 out
        assert not mix[b, 0, 2].any() and not voc[b, 0, 2].any() and not mix_phase[b, 0, 2].any() and not voc_phase[b, 0, 2].any()
    # item 2 is V cis + (M cis - V cis) of one song at one rate: the stretched vocal and accompaniment add up to the definition's z
    assert np.abs(ref.z[2] - ref.zv[2]).max() > 0.01


def test_the_full_scan_of_a_row(report):
    """F = 8, seg = 128: two rounds of 64 lanes, the carry of the first into the second, at each rate."""
    songs = Songs([400, 150], 8, seed=3, zero_bin=5)
    table = table_of([(0, 144, 1, 3, 0.9, 0.6, 2048, 819),                 # start_v = room(2048) = 400 - 256
                      (0, 17, 0, 230, 0.5, 1.1, 1333, 1333),
                      (1, 0, 0, 335, 1.25, 0.25, 1024, 512),               # the 150-frame song: 129 of them; start_a = room(512) = 400 - 65
                      (1, 0, -1, 0, 0.8, 0.8, 1333, 0)])                   # a gain item whose source ends at output frame 115
    au.check_stretch_table(table, songs.frames_host, 128)
    got, _ = check_against_reference("crop_stretch scan (4, 8, 128)", songs, table, 128, 512, 128, report)
    assert got[1][3, 0, 0, :116].all() and not got[1][3, 0, :, 116:].any()


@pytest.mark.parametrize("n_fft,hop", [(1024, 768), (512, 384)])
def test_production_shape_against_the_definition(n_fft, hop, report):
    songs = Songs([100, 128, 300, 517], n_fft // 2, seed=2)
    table = table_of([(2, 133, 3, 350, 0.3, 1.25, 1333, 1333),             # both starts at room(1333) = T - 167
                      (3, 2, 0, 0, 1.25, 0.25, 1024, 819),                 # the short song (100 frames) as accompaniment
                      (1, 0, -1, 0, 0.5, 1.0, 819, 819)])                  # a gain item: 104 of the 128 frames of its song
    au.check_stretch_table(table, songs.frames_host, 128)
    got, _ = check_against_reference(f"crop_stretch production (3, {n_fft // 2}, 128) at ({n_fft}, {hop})", songs, table, 128, n_fft, hop, report)
    assert got[0][1, 0, :, :120].all() and got[1][1, 0].all()


def test_the_bound_has_teeth():
    """numpy only: the definition with an fp32 accumulator and the unreduced expected advance 2 pi hop bin / n_fft (about 2,400 rad
    per frame at the top bin of (1024, 768)) leaves the bound by orders of magnitude by the end of a 128-frame tile."""
    n_fft, hop, F, seg, T, s, q = 1024, 768, 512, 128, 300, 5, 1333
    rng = np.random.default_rng(8)
    M, V, pm, pv = conditioned(rng, F, T)
    g = np.ones(1, np.float32)
    ref = au.stretch_reference([M], [V], [pm], [pv], [0], [s], [-1], [0], g, g, [q], [q], seg, n_fft, hop)
    n = np.arange(seg) * q
    k, alpha = s + (n >> 10), ((n & 1023) / 1024.0).astype(np.float32)
    w = (2.0 * np.pi * hop * np.arange(1, F + 1) / n_fft).astype(np.float32)[:, None]               # unreduced
    two_pi = np.float32(2.0 * np.pi)
    d = (pv[:, k + 1] - pv[:, k]) - w
    d = d - two_pi * np.round(d / two_pi)
    step = w + d
    acc = np.empty((F, seg), np.float32)
    acc[:, 0] = pv[:, s]
    for t in range(1, seg):
        acc[:, t] = acc[:, t - 1] + step[:, t - 1]                         # the plain fp32 accumulator
    mag = (np.float32(1) - alpha) * V[:, k] + alpha * V[:, k + 1]
    lossy = mag.astype(np.float64) * np.exp(1j * acc.astype(np.float64))
    _, b_v = bounds(ref)
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
    whole = run(songs, table_of(items), SMALL_SEG, *SMALL_GEOMETRY)
    again = run(songs, table_of(items), SMALL_SEG, *SMALL_GEOMETRY)
    for w, a in zip(whole, again):
        assert np.array_equal(w, a)
    for b in (0, 4, len(items) - 1):
        alone = run(songs, table_of([items[b]]), SMALL_SEG, *SMALL_GEOMETRY)
        for w, a in zip(whole, alone):
            assert np.array_equal(w[b], a[0]), b
    big = Songs([300, 200], 256, seed=6)
    items = [(0, 3, 1, 20, 0.9, 0.6, 1333, 819), (1, 30, -1, 0, 0.3, 1.1, 1024, 0), (1, 7, 0, 40, 0.7, 0.7, 512, 2048)]
    rev = items[::-1] * 12                                                 # 36 items: 9216 rows, more than one row per wave of the grid
    whole = run(big, table_of(rev), 128, 512, 384)
    for b in (2, 1, 0):
        alone = run(big, table_of([rev[b]]), 128, 512, 384)
        for w, a in zip(whole, alone):
            assert np.array_equal(w[b], a[0]) and np.array_equal(w[b + 33], a[0]), b


def test_without_phase_outputs_mix_and_voc_are_the_same():
    songs, table = small_songs(), table_of(SMALL_ITEMS)
    full = run(songs, table, SMALL_SEG, *SMALL_GEOMETRY, with_phase=True)
    lean = run(songs, table, SMALL_SEG, *SMALL_GEOMETRY, with_phase=False)
    assert len(lean) == 2 and np.array_equal(lean[0], full[0]) and np.array_equal(lean[1], full[1])
    big = Songs([300, 200], 256, seed=5)
    t2 = table_of([(0, 3, 1, 20, 0.9, 0.6, 1333, 819), (1, 30, 0, 12, 0.3, 1.1, 1024, 2048)])
    full, lean = run(big, t2, 128, 512, 384, with_phase=True), run(big, t2, 128, 512, 384, with_phase=False)
    assert np.array_equal(lean[0], full[0]) and np.array_equal(lean[1], full[1])


# ---- ResidentSpectrograms.augmented_batches --------------------------------------------------------------------------------

FOLDER_FRAMES = [100, 200, 333]      # one song shorter than the 128-frame tile
PER_SONG = 4


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """A synthetic folder of 3 well-conditioned songs at win 512: 257-row magnitude files with unit-phasor phase files."""
    root = tmp_path_factory.mktemp("stretch_set")
    rng = np.random.default_rng(11)
    for d in ("mixture", "vocal"):
        os.makedirs(root / d)
    for i, T in enumerate(FOLDER_FRAMES):
        M, V, pm, pv = conditioned(rng, 257, T)
        for d, mag, ang in (("mixture", M, pm), ("vocal", V, pv)):
            np.save(root / d / f"{i:04d}_song_spec.npy", mag)
            np.save(root / d / f"{i:04d}_song_phase.npy", np.exp(1j * ang.astype(np.float64)).astype(np.complex64))
    return root


@pytest.fixture(scope="module")
def resident(folder):
    dataset = svs_train.SpectrogramDataset(str(folder), samples_per_song=PER_SONG, win_size=512)
    return svs_train.ResidentSpectrograms(dataset, torch.device(DEV))


def host_songs(res):
    """The resident buffers back on the host as per-song (F, T) planes: the reference's fp32 inputs (the angles are the device's)."""
    out = []
    for buf in (res.mix, res.voc, res.mix_ang, res.voc_ang):
        h, off, parts = buf.cpu().numpy(), 0, []
        for T in res.frames_host:
            parts.append(h[off:off + res.rows * T].reshape(res.rows, T))
            off += res.rows * T
        out.append(parts)
    return out


def test_augmented_batches_stretch_against_the_definition(resident, report):
    assert resident.rows == 256 and resident.has_phase and len(resident) == 12
    aug = au.Augment("remix", (0.25, 1.25), 0.75, seed=9, stretch_range=(0.8, 1.25))
    epoch = 5
    drawn = au.draw_epoch_stretch(len(resident), resident.frames_host, 128, epoch, 9, (0.25, 1.25), 0.75, (0.8, 1.25))
    assert (drawn.song_a >= 0).any() and (drawn.song_a < 0).any() and len(set(drawn.rate_v.tolist())) > 6
    M, V, pm, pv = host_songs(resident)
    worst_seen = [0.0, 0.0]
    for rank in range(2):
        order = svs_train.epoch_order(len(resident), True, rank, 2, epoch)
        batches = list(resident.augmented_batches(4, rank, 2, epoch, with_phase=True, aug=aug, hop=384))
        assert [b[0].shape for b in batches] == [(4, 1, 256, 128), (2, 1, 256, 128)] and all(len(b) == 4 for b in batches)
        got = [torch.cat(t).cpu().numpy() for t in zip(*batches)]
        ref = au.stretch_reference(M, V, pm, pv, *(np.asarray(a)[order] for a in drawn), 128, 512, 384)
        assert all(np.isfinite(g).all() for g in got)
        worst_seen = [max(w, x) for w, x in zip(worst_seen, ratios(got, ref))]
        two = list(resident.augmented_batches(4, rank, 2, epoch, with_phase=False, aug=aug, hop=384))
        assert all(len(b) == 2 for b in two) and torch.equal(two[0][0], batches[0][0]) and torch.equal(two[1][1], batches[1][1])
    print(f"augmented_batches stretch: worst ratios {worst_seen[0]:.3f} {worst_seen[1]:.3f}")
    ok = report("augmented_batches stretch: |mix cis(mix_phase) - z| over its bound", worst_seen[0], 1.0)
    ok = report("augmented_batches stretch: |voc cis(voc_phase) - zv| over its bound", worst_seen[1], 1.0) and ok
    assert ok, worst_seen
    # without a range the same settings take the remix path, bit for bit what they were
    plain = au.Augment("remix", (0.25, 1.25), 0.75, seed=9)
    order = svs_train.epoch_order(len(resident), True, 1, 2, 2)
    a = next(resident.augmented_batches(4, 1, 2, 2, with_phase=True, aug=plain))
    table = au.upload_table(resident, au.draw_epoch(len(resident), resident.frames_host, 128, 2, 9, (0.25, 1.25), 0.75), order)
    for x, y in zip(a, au.crop_remix(resident, table, 0, 4, True)):
        assert torch.equal(x, y)


def test_one_training_step_on_a_stretched_batch(resident):
    """The full objective (L1 + MR-STFT) at win 512 / hop 384 on a stretched batch: finite losses, parameters that moved."""
    model = UNet().to(DEV).train()
    before = model.state_dict()["conv1.0.weight"].detach().clone()
    aug = au.Augment("remix", (0.25, 1.25), 1.0, seed=1, stretch_range=(0.8, 1.25))
    mix, voc, mph, vph = next(resident.augmented_batches(4, 0, 1, 0, with_phase=True, aug=aug, hop=384))
    l1 = model.train_step(mix, voc, loss_scale=ALPHA_L1, mix_phase=mph, voc_phase=vph, alpha_mr=ALPHA_MR, hop=384)
    l1, mr = float(l1), float(model.last_mr_loss)
    assert np.isfinite(l1) and l1 > 0 and np.isfinite(mr) and mr > 0, (l1, mr)
    after = model.state_dict()["conv1.0.weight"]
    assert torch.isfinite(after).all() and (after - before).abs().max().item() > 0


def test_train_cli_with_the_flag(folder, tmp_path, monkeypatch, capsys):
    """train.py --augment remix --stretch_range for one epoch (full objective, win 512): the settings line names the range, every
    step is one crop_stretch launch at the folder's geometry, and the checkpoint has the keys it always had."""
    monkeypatch.chdir(tmp_path)
    calls = []
    real = au.crop_stretch

    def counted(res, table, lo, hi, n_fft, hop, with_phase=False):
        calls.append((n_fft, hop, with_phase))
        return real(res, table, lo, hi, n_fft, hop, with_phase)

    def forbidden(*args, **kw):
        raise AssertionError("--stretch_range reached the remix launch")
    monkeypatch.setattr(au, "crop_stretch", counted)
    monkeypatch.setattr(au, "crop_remix", forbidden)
    svs_train.main(["--train_folder", str(folder), "--valid_folder", str(tmp_path / "no_valid"), "--batch_size", "32", "--epoch", "1",
                    "--load_path", "none.pth", "--win_size", "512", "--hop_size", "384", "--label", "st", "--augment", "remix",
                    "--stretch_range", "0.8", "1.25", "--augment_seed", "3"])
    lines = capsys.readouterr().out.splitlines()
    line = [l for l in lines if l.startswith("Augmentation:")]
    assert len(line) == 1 and "time-stretched" in line[0] and "[0.8, 1.25]" in line[0] and "seed 3" in line[0], lines
    from svs_unet_pytorch_amd.config import SAMPLES_PER_SONG
    assert calls == [(512, 384, True)] * -(-len(FOLDER_FRAMES) * SAMPLES_PER_SONG // 32)                # one launch per step
    value = float(open(tmp_path / "LOG" / "log_st.txt").read().split()[0])
    assert np.isfinite(value) and value > 0
    ck = torch.load(tmp_path / "CKPT" / "svs_st.pth", map_location="cpu")
    assert ck["epoch"] == 1 and "stretch_range" not in ck
