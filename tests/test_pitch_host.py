"""Pitch-shift augmentation, the host half (no GPU): svs_crop_pitch_tiles is declared, bound and exported and refuses every bad
argument before any launch (host or null pointers only); the float64 definition (augment.pitch_vocoder / pitch_reference) is
phase_vocoder / stretch_reference at P = 1024, moves stationary partials to p times their frequency (and two mutants of it do not),
and shifts the peak of a real cosine's Hann STFT; draw_epoch_pitch's table is a function of (seed, epoch) with the stated
distributions and is shared by the ranks; check_pitch_table's refusals; the command line's refusals, its help text, and a run
without --pitch_range that reaches none of the new functions."""
import types
from collections import Counter

import numpy as np
import pytest

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import augment as au

NAME = "svs_crop_pitch_tiles"


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def err(lib):
    return lib.svs_last_error_string().decode()


def test_symbol_is_declared_bound_and_exported(lib):
    assert NAME in _lib.header_symbols() and NAME in _lib._SIGS and hasattr(lib, NAME)
    assert len(_lib._SIGS[NAME][1]) == 26 and len(_lib._SIGS["svs_crop_stretch_tiles"][1]) == 24 and lib.svs_version() == 1


# ---- argument rules of the entry point -------------------------------------------------------------------------------------

# positions: 0 mix_songs 1 voc_songs 2 mix_ang 3 voc_ang 4 offset 5 frames 6 song_v 7 start_v 8 song_a 9 start_a 10 gain_v 11 gain_a
#            12 rate_v 13 rate_a 14 pitch_v 15 pitch_a 16 B 17 F 18 seg 19 n_fft 20 hop 21 mix 22 voc 23 mix_phase 24 voc_phase 25 stream
GOOD = [16] * 16 + [2, 256, 8, 512, 384, 16, 32, 48, 64, None]             # never dereferenced: a check comes first


def changed(**kw):
    args = list(GOOD)
    for k, v in kw.items():
        args[int(k[1:])] = v
    return args


RULES = [(changed(**{f"_{i}": None}), "null pointer") for i in (0, 1, 2, 3, 4, 5, 21, 22)]            # the angles are required
RULES += [(changed(_2=None, _3=None, _23=None, _24=None), "null pointer")]                             # no magnitude-only form
RULES += [(changed(**{f"_{i}": None}), "null table") for i in range(6, 16)]                            # pitch_v and pitch_a included
RULES += [
    (changed(_23=None), "mix_phase and voc_phase must both"), (changed(_24=None), "mix_phase and voc_phase must both"),
    (changed(_16=0), "bad geometry"), (changed(_16=-1), "bad geometry"), (changed(_18=0), "bad geometry"), (changed(_18=6), "bad geometry"),
    (changed(_18=-8), "bad geometry"), (changed(_18=130), "bad geometry"),
    (changed(_21=24), "16-byte aligned"), (changed(_22=4), "16-byte aligned"), (changed(_23=40), "16-byte aligned"),
    (changed(_24=8), "16-byte aligned"),
    (changed(_19=0), "n_fft must be 512, 1024 or 2048"), (changed(_19=256), "n_fft must be 512, 1024 or 2048"),
    (changed(_19=1000), "n_fft must be 512, 1024 or 2048"), (changed(_19=4096, _17=2048), "n_fft must be 512, 1024 or 2048"),
    (changed(_17=0), "1 <= F <= n_fft / 2"), (changed(_17=257), "1 <= F <= n_fft / 2"), (changed(_17=512), "1 <= F <= n_fft / 2"),
    (changed(_17=-4), "1 <= F <= n_fft / 2"), (changed(_19=1024, _17=513), "1 <= F <= n_fft / 2"),
    (changed(_20=0), "hop must be in 1..n_fft"), (changed(_20=-384), "hop must be in 1..n_fft"), (changed(_20=513), "hop must be in 1..n_fft"),
]


@pytest.mark.parametrize("args,msg", RULES)
def test_entry_point_refuses_before_any_launch(lib, args, msg):
    assert lib.svs_crop_pitch_tiles(*args) == -1
    assert msg in err(lib) and err(lib).startswith(NAME + ":")


# ---- the definition --------------------------------------------------------------------------------------------------------

def songs_fp32(frames, F, seed, zero_bin=None):
    rng = np.random.default_rng(seed)
    M = [(0.05 + rng.random((F, T))).astype(np.float32) for T in frames]
    V = [(m * 0.5 * rng.random(m.shape)).astype(np.float32) for m in M]
    pm = [rng.uniform(-np.pi, np.pi, (F, T)).astype(np.float32) for T in frames]
    pv = [rng.uniform(-np.pi, np.pi, (F, T)).astype(np.float32) for T in frames]
    if zero_bin is not None:
        for a in M + V:
            a[zero_bin] = 0.0
    return M, V, pm, pv


@pytest.mark.parametrize("n_fft,hop", [(1024, 768), (512, 300)])
@pytest.mark.parametrize("q", [1024, 819, 1333, 512, 2048])
def test_pitch_one_is_the_phase_vocoder_exactly(n_fft, hop, q):
    rng = np.random.default_rng(q + hop)
    F, T, seg, s = n_fft // 2, 300, 128, 9
    plane = rng.random((F, T)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (F, T)))
    plane[7] = 0.0
    weight = 1.0 + rng.random((F, T))
    for x, y in zip(au.pitch_vocoder(plane, s, q, 1024, seg, n_fft, hop, weight), au.phase_vocoder(plane, s, q, seg, n_fft, hop, weight)):
        assert np.array_equal(x, y)                                        # differences of exactly 0.0
    j0, gamma, j = au.pitch_bins(F, 1024)
    assert np.array_equal(j0, np.arange(1, F + 1)) and np.array_equal(j, j0) and not gamma.any()


def test_pitch_one_reference_is_the_stretch_reference():
    frames, F, seg = [40, 9, 23], 6, 8
    M, V, pm, pv = songs_fp32(frames, F, 5, zero_bin=2)
    items = [(0, 3, -1, 0), (0, 20, 2, 9), (2, 1, 2, 9), (1, 4, 0, 21), (1, 0, 1, 0)]
    sv, st, sa, sta = (np.array(c, np.int32) for c in zip(*items))
    gv, ga = np.linspace(0.3, 1.2, len(items)).astype(np.float32), np.linspace(1.25, 0.25, len(items)).astype(np.float32)
    qv, qa = np.array([1024, 819, 1333, 512, 2048], np.int32), np.array([7, 1333, 1024, 2048, 512], np.int32)
    one = np.full(len(items), 1024, np.int32)
    ref = au.pitch_reference(M, V, pm, pv, sv, st, sa, sta, gv, ga, qv, qa, one, one, seg, 512, 384)
    old = au.stretch_reference(M, V, pm, pv, sv, st, sa, sta, gv, ga, qv, qa, seg, 512, 384)
    assert isinstance(ref, au.Stretch)
    for name, x, y in zip(au.Stretch._fields, ref, old):
        assert np.abs(x - y).max() <= 1e-11, name
    other = au.pitch_reference(M, V, pm, pv, sv, st, sa, sta, gv, ga, qv, qa, one, one + 100, seg, 512, 384)
    assert np.array_equal(other.zv, ref.zv) and np.array_equal(other.z[0], ref.z[0])       # the vocal and the gain item: P_a is not theirs
    assert not np.allclose(other.z[1:], ref.z[1:])
    assert (other.scale >= other.mix - 1e-12).all()                        # |z| <= g_v V + g_a (M + V): the triangle inequality


def test_bins_are_exact_integers():
    j0, gamma, j = au.pitch_bins(6, 2048)                                  # b / 2: odd rows tie and go up, row 1 has j0 = 0
    assert j0.tolist() == [0, 1, 1, 2, 2, 3] and gamma.tolist() == [0.5, 0.0, 0.5, 0.0, 0.5, 0.0] and j.tolist() == [1, 1, 2, 2, 3, 3]
    j0, gamma, j = au.pitch_bins(6, 512)                                   # 2 b: rows 4..6 read above F, j is clamped there
    assert j0.tolist() == [2, 4, 6, 8, 10, 12] and not gamma.any() and j.tolist() == [2, 4, 6, 6, 6, 6]
    j0, gamma, j = au.pitch_bins(1024, 2047)
    assert j0[0] == 0 and j[0] == 1 and j0[-1] == 512 and j[-1] == 512 and np.all((j == j0) | (j == j0 + 1))
    rng = np.random.default_rng(0)
    plane = rng.random((6, 20)) * np.exp(1j * rng.uniform(-3, 3, (6, 20)))
    mag, acc, _ = au.pitch_vocoder(plane, 2, 1024, 512, 8, 512, 384)
    assert mag[:3].all() and not mag[3:].any()                             # rows falling off the top are exactly 0
    assert np.array_equal(mag[2], np.abs(plane[5, 2:10]))                  # an exact-integer b / p: the source bin itself
    mag, _, _ = au.pitch_vocoder(plane, 2, 1024, 2048, 8, 512, 384)
    assert np.allclose(mag[0], 0.5 * np.abs(plane[0, 2:10]), rtol=1e-15)   # j0 = 0: the DC row counts as silent


def mutant_vocoder(plane, start, q, P, seg, n_fft, hop, phase_bin="nearest", advance="scaled"):
    """augment.pitch_vocoder restated with two switches: the phase bin taken as j0 (clamped) instead of the nearest bin, and the
    centre advance w in the place of w'.  With neither it is the definition (asserted below)."""
    F, p = plane.shape[0], P / 1024.0
    mag_s, arg_s = au._polar64(np.asarray(plane, np.complex128))
    n = np.arange(seg, dtype=np.int64) * int(q)
    k, alpha = int(start) + (n >> 10), (n & 1023) / 1024.0
    j0, gamma, j = au.pitch_bins(F, P)
    if phase_bin == "j0":
        j = np.clip(j0, 1, F)
    mag = au._bilinear(mag_s, k, alpha, j0, gamma)
    a0, a1 = au._columns(arg_s, k)[j - 1], au._columns(arg_s, k + 1)[j - 1]
    w = 2.0 * np.pi * ((hop * j) % n_fft) / n_fft
    d = a1 - a0 - w[:, None]
    d -= 2.0 * np.pi * np.round(d / (2.0 * np.pi))
    d = np.where(d >= np.pi, d - 2.0 * np.pi, d)
    centre = 2.0 * np.pi * ((hop * j * int(P)) % (1024 * n_fft)) / (1024 * n_fft) if advance == "scaled" else w
    step = centre[:, None] + p * d
    acc = a0[:, :1] + np.concatenate([np.zeros((F, 1)), np.cumsum(step[:, :-1], axis=1)], axis=1)
    return mag, acc


def partials_error(vocoder, n_fft, hop, F, T, seg, s, q, P):
    """Worst |out - want| / A over the rows, for source rows S[i, t] = A_i cis(theta_i + w0_i hop t), one partial per row within the
    unambiguous range of its bin: output row b must be ((1 - gamma) A_j0 + gamma A_(j0+1)) cis(theta_j + w0_j hop s + p w0_j hop t),
    with A = 0 outside 1..F."""
    rng = np.random.default_rng(P + q + n_fft)
    assert s + au.span(q, seg) <= T
    A = rng.uniform(0.1, 1.0, F)
    theta = rng.uniform(-np.pi, np.pi, F)
    off = rng.uniform(-0.45, 0.45, F) * (n_fft / (2.0 * hop))              # bins off the centre, inside the unambiguous range
    w0 = 2.0 * np.pi * (np.arange(1, F + 1) + off) / n_fft
    plane = A[:, None] * np.exp(1j * (theta[:, None] + w0[:, None] * hop * np.arange(T)[None, :]))
    mag, acc = vocoder(plane, s, q, P, seg, n_fft, hop)[:2]
    j0, gamma, j = au.pitch_bins(F, P)
    padded = np.concatenate([[0.0], A, np.zeros(F + 2)])                   # A by bin, 0 at the DC row and above F
    want_mag = (1.0 - gamma) * padded[np.minimum(j0, F + 1)] + gamma * padded[np.minimum(j0 + 1, F + 1)]
    want_phase = theta[j - 1, None] + w0[j - 1, None] * hop * s + (P / 1024.0) * w0[j - 1, None] * hop * np.arange(seg)[None, :]
    e = np.abs(mag * np.exp(1j * acc) - want_mag[:, None] * np.exp(1j * want_phase))
    assert not mag[want_mag == 0.0].any()
    return float((e / np.maximum(want_mag, 0.05)[:, None]).max())


PITCHES = [512, 724, 913, 1149, 1448, 2048]


@pytest.mark.parametrize("n_fft,hop", [(1024, 768), (512, 300)])
@pytest.mark.parametrize("q", [1024, 819, 1333])
@pytest.mark.parametrize("P", PITCHES)
def test_stationary_partials_come_out_at_the_scaled_frequency(n_fft, hop, q, P):
    """1e-8 is the float64 exp of arguments up to p w0 hop T ~ 2e6 rad, the floor of the stretch's own test."""
    e = partials_error(au.pitch_vocoder, n_fft, hop, n_fft // 2, 300, 128, 17, q, P)
    print(f"partials ({n_fft}, {hop}) q={q} P={P}: worst error {e:.2e}")
    assert e <= 1e-8, e


@pytest.mark.parametrize("P", [2047, 2048])
def test_stationary_partials_where_the_product_reaches_two_to_the_32(P):
    """(2048, 2048), F = 1024: hop j P = 2^32 at j = 1024, P = 2048 is the largest product the ranges allow (rows 1..F reach 2^31 at
    P = 2048 and just under it at 2047): the definition forms it in int64."""
    assert 2048 * 1024 * 2048 == 2 ** 32 and 2048 * int(au.pitch_bins(1024, 2048)[2][-1]) * 2048 == 2 ** 31
    e = partials_error(au.pitch_vocoder, 2048, 2048, 1024, 40, 16, 5, 1024, P)
    print(f"partials (2048, 2048) P={P}: worst error {e:.2e}")
    assert e <= 1e-8, e


@pytest.mark.parametrize("n_fft,hop", [(1024, 768), (512, 300)])
@pytest.mark.parametrize("P", [724, 1149, 2048])
def test_mutants_of_the_definition_fail_the_partials(n_fft, hop, P):
    """The phase bin taken as j0 instead of the nearest bin, and w in the place of w': each misses the partials by more than 1e-3 of
    the amplitude on some row.  (At P = 512 every b / p is an integer and the first mutant is the definition: not a case here.)"""
    args = (n_fft, hop, n_fft // 2, 300, 128, 17, 1333, P)
    rng = np.random.default_rng(1)
    plane = rng.random((32, 60)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (32, 60)))
    for x, y in zip(mutant_vocoder(plane, 3, 819, P, 32, n_fft, hop), au.pitch_vocoder(plane, 3, 819, P, 32, n_fft, hop)):
        assert np.array_equal(x, y)                                        # without a switch the restatement is the definition
    assert partials_error(mutant_vocoder, *args) <= 1e-8
    e_bin = partials_error(lambda *a: mutant_vocoder(*a, phase_bin="j0"), *args)
    e_adv = partials_error(lambda *a: mutant_vocoder(*a, advance="centre"), *args)
    print(f"mutants ({n_fft}, {hop}) P={P}: phase bin j0 {e_bin:.3f}, w for w' {e_adv:.3f}")
    assert e_bin > 1e-3 and e_adv > 1e-3, (e_bin, e_adv)


def hann_stft(x, n_fft, hop):
    """Bins 1..n_fft/2 of the Hann STFT of x, frames from sample 0 (no padding): (n_fft / 2, T) complex."""
    T = (len(x) - n_fft) // hop + 1
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    frames = np.stack([x[t * hop:t * hop + n_fft] * win for t in range(T)], axis=1)
    return np.fft.rfft(frames, axis=0)[1:]


@pytest.mark.parametrize("hop", [256, 768])
@pytest.mark.parametrize("P", PITCHES)
def test_a_real_cosine_moves_to_p_times_its_frequency(P, hop):
    """A real cosine at nu = 100.37 bins of a 1024-point Hann STFT: the shifted peak lies within one bin of p nu, and the peak row's
    advance per frame is off from 2 pi p nu hop / n_fft by at most p times the deviation of the source bin it follows (measured
    here: the source bin's own measured advance against 2 pi nu hop / n_fft) plus 1e-9."""
    n_fft, nu, seg, s, p = 1024, 100.37, 32, 3, P / 1024.0
    x = np.cos(2.0 * np.pi * nu * np.arange(n_fft + hop * 60) / n_fft + 0.3)
    plane = hann_stft(x, n_fft, hop)
    mag, acc, _ = au.pitch_vocoder(plane, s, 1024, P, seg, n_fft, hop)
    peak = int(np.argmax(mag.mean(axis=1))) + 1
    assert abs(peak - p * nu) <= 1.0, (peak, p * nu)
    j = int(au.pitch_bins(n_fft // 2, P)[2][peak - 1])
    arg = np.angle(plane[j - 1, s:s + seg])
    wrap = lambda a: a - 2.0 * np.pi * np.round(a / (2.0 * np.pi))
    centre = 2.0 * np.pi * hop * j / n_fft                                 # unreduced
    src_dev = centre + wrap(np.diff(arg) - centre) - 2.0 * np.pi * nu * hop / n_fft        # the source bin's advance against the truth
    out_dev = wrap(np.diff(acc[peak - 1]) - p * 2.0 * np.pi * nu * hop / n_fft)
    print(f"cosine P={P} hop={hop}: peak {peak} for {p * nu:.2f}, source bin {j} off by {np.abs(src_dev).max():.2e}, output by {np.abs(out_dev).max():.2e}")
    assert (np.abs(out_dev) <= p * np.abs(src_dev[:seg - 1]) + 1e-9).all()


# ---- draw_epoch_pitch ------------------------------------------------------------------------------------------------------

FRAMES = [300, 40, 129, 128, 1000]
SEG = 128


def test_draw_is_a_function_of_seed_and_epoch():
    a = au.draw_epoch_pitch(320, FRAMES, SEG, epoch=3, seed=11, stretch_range=(0.8, 1.25))
    b = au.draw_epoch_pitch(320, FRAMES, SEG, epoch=3, seed=11, stretch_range=(0.8, 1.25))
    assert isinstance(a, au.PitchTable) and a._fields == au.StretchTable._fields + ("pitch_v", "pitch_a") and au.PITCH_ROWS == a._fields
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))
    assert [x.dtype for x in a] == [np.int32] * 4 + [np.float32] * 2 + [np.int32] * 4 and all(len(x) == 320 for x in a)
    assert np.array_equal(a.song_v, np.arange(320) % len(FRAMES))
    for other in (au.draw_epoch_pitch(320, FRAMES, SEG, epoch=4, seed=11, stretch_range=(0.8, 1.25)),
                  au.draw_epoch_pitch(320, FRAMES, SEG, epoch=3, seed=12, stretch_range=(0.8, 1.25))):
        for name in ("start_v", "song_a", "gain_v", "gain_a", "rate_v", "rate_a", "pitch_v", "pitch_a"):
            assert not np.array_equal(getattr(a, name), getattr(other, name)), name
    assert len(au.draw_epoch_pitch(0, FRAMES, SEG, 0).pitch_v) == 0 and len(au.draw_epoch_pitch(8, [], SEG, 0).pitch_a) == 0


@pytest.mark.parametrize("pitch_range,stretch_range", [((-2.0, 2.0), None), ((-12.0, 12.0), (0.5, 2.0)), ((0.0, 0.0), (0.8, 1.25)),
                                                        ((3.0, 3.0), None), ((-5.0, -1.0), (1.3, 1.3))])
def test_draw_pitches_rates_and_starts(pitch_range, stretch_range):
    t = au.draw_epoch_pitch(6000, FRAMES, SEG, 2, 7, remix_prob=0.5, pitch_range=pitch_range, stretch_range=stretch_range)
    p_lo, p_hi = (int(round(1024 * 2.0 ** (st / 12.0))) for st in pitch_range)
    remix = t.song_a >= 0
    assert remix.any() and (~remix).any()
    for P in (t.pitch_v, t.pitch_a):
        assert P.min() >= p_lo and P.max() <= p_hi and P.min() >= 512 and P.max() <= 2048
        assert P.min() <= p_lo + (p_hi - p_lo) // 50 and P.max() >= p_hi - (p_hi - p_lo) // 50     # the range is used up to its ends
    assert np.array_equal(t.pitch_a[~remix], t.pitch_v[~remix]) and np.array_equal(t.rate_a[~remix], t.rate_v[~remix])
    if p_hi > p_lo:
        assert not np.array_equal(t.pitch_a[remix], t.pitch_v[remix])      # a remix item's sources have pitches of their own
    if stretch_range is None:
        assert (t.rate_v == 1024).all() and (t.rate_a == 1024).all()
    else:
        q_lo, q_hi = round(1024 * stretch_range[0]), round(1024 * stretch_range[1])
        assert t.rate_v.min() == q_lo and t.rate_v.max() == q_hi and t.rate_a.min() == q_lo and t.rate_a.max() == q_hi
    frames = np.array(FRAMES)
    room_v = np.maximum(frames[t.song_v] - au.span(t.rate_v, SEG), 0)      # the span is the stretch's: the pitch does not change it
    room_a = np.maximum(frames[t.song_a[remix]] - au.span(t.rate_a[remix], SEG), 0)
    assert (t.start_v >= 0).all() and (t.start_v <= room_v).all() and not t.start_a[~remix].any()
    assert (t.start_a[remix] >= 0).all() and (t.start_a[remix] <= room_a).all()
    assert (t.start_v == room_v)[room_v > 0].any() and (t.start_v[room_v > 0] == 0).any()
    au.check_pitch_table(t, FRAMES, SEG)                                   # and what is drawn passes the upload's own checks
    assert au.semitones_to_pitch([-12, 0, 12, 2, -2]).tolist() == [512, 1024, 2048, 1149, 912]


def test_ranks_share_one_table():
    from svs_unet_pytorch_amd.train import epoch_order
    n, frames = 3 * 8, [300, 40, 500]

    def union(world):
        seen = Counter()
        for rank in range(world):
            table = au.draw_epoch_pitch(n, frames, SEG, epoch=6, seed=2, stretch_range=(0.8, 1.25))
            packed = au.pack_pitch_table(table, epoch_order(n, True, rank, world, 6))
            assert packed.dtype == np.int32 and packed.shape[0] == 10 and packed.flags.c_contiguous
            seen.update(map(tuple, packed.T.tolist()))
        return seen
    one = union(1)
    assert sum(one.values()) == n and union(2) == one and union(4) == one
    t = au.draw_epoch_pitch(n, frames, SEG, 6, 2, stretch_range=(0.8, 1.25))
    whole = au.pack_pitch_table(t)
    assert np.array_equal(whole[:8], au.pack_stretch_table(au.StretchTable(*t[:8]))) and np.array_equal(whole[8], t.pitch_v) \
        and np.array_equal(whole[9], t.pitch_a)


# ---- check_pitch_table / crop_pitch ----------------------------------------------------------------------------------------

def fake_resident(angles=True, rows=256):
    return types.SimpleNamespace(frames_host=[300, 40, 129], mix_ang=object() if angles else None, device="no such device", rows=rows)


def table(**kw):
    # room: song 0 at q 1024: 300 - 129 = 171; at 2048: 300 - 256 = 44; song 2 at 512: 129 - 65 = 64
    base = dict(song_v=[0, 1, 2], start_v=[171, 0, 64], song_a=[2, -1, 0], start_a=[64, 0, 44], gain_v=[1.0, 0.5, 1.25], gain_a=[1.0, 1.0, 0.25],
                rate_v=[1024, 819, 512], rate_a=[512, 1024, 2048], pitch_v=[512, 1024, 2048], pitch_a=[2048, 1149, 512])
    base.update(kw)
    i32, f32 = (lambda k: np.array(base[k], np.int32)), (lambda k: np.array(base[k], np.float32))
    return au.PitchTable(i32("song_v"), i32("start_v"), i32("song_a"), i32("start_a"), f32("gain_v"), f32("gain_a"), i32("rate_v"), i32("rate_a"),
                         i32("pitch_v"), i32("pitch_a"))


@pytest.mark.parametrize("kw,msg", [
    (dict(song_v=[0, 3, 2]), "song_v outside"), (dict(song_a=[3, -1, 0]), "song_a outside"),
    (dict(start_v=[172, 0, 64]), "start_v outside"), (dict(start_a=[65, 0, 44]), "start_a outside"),
    (dict(rate_v=[511, 819, 512]), "rate_v outside"), (dict(rate_a=[512, 1024, 2049]), "rate_a outside"),
    (dict(gain_v=[1.0, float("nan"), 1.0]), "not finite"),
    (dict(pitch_v=[511, 1024, 2048]), "pitch_v outside"), (dict(pitch_v=[512, 2049, 2048]), "pitch_v outside"),
    (dict(pitch_v=[512, 0, 2048]), "pitch_v outside"), (dict(pitch_v=[512, 1024, -1024]), "pitch_v outside"),
    (dict(pitch_a=[2049, 1149, 512]), "pitch_a outside"), (dict(pitch_a=[2048, 1149, 511]), "pitch_a outside"),
    (dict(pitch_a=[2048, 1149]), "rows of"), (dict(rate_a=[512, 1024]), "rows of"),
])
def test_crop_pitch_checks_the_host_arrays(kw, msg):
    with pytest.raises(ValueError, match="pitch table: .*" + msg):
        au.crop_pitch(fake_resident(), table(**kw), 0, 3, 512, 384, with_phase=True)


def test_check_pitch_table_accepts_and_needs_angles():
    au.check_pitch_table(table(), [300, 40, 129], 128)
    au.check_pitch_table(table(pitch_a=[2048, 7, 512], rate_a=[512, 7, 2048]), [300, 40, 129], 128)     # a gain item's pitch_a / rate_a are not read
    with pytest.raises(ValueError, match=r"pitch shift needs the angles"):
        au.crop_pitch(fake_resident(angles=False), table(), 0, 3, 512, 384)
    with pytest.raises(ValueError, match=r"pitch shift needs the angles"):
        au.check_pitch_table(table(), [300, 40, 129], 128, has_angles=False)
    with pytest.raises(ValueError, match=r"pitch shift needs the angles"):
        au.crop_pitch(fake_resident(angles=False), object(), 0, 3, 512, 384)                             # an uploaded table of a phaseless set


# ---- command line ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags,msg", [
    (["--augment", "none", "--pitch_range", "-2", "2"], "needs --augment gain or --augment remix"),
    (["--pitch_range", "-2", "2"], "needs --augment gain or --augment remix"),
    (["--augment", "remix", "--pitch_range", "2", "-2"], "--pitch_range"),
    (["--augment", "gain", "--pitch_range", "-12.5", "0"], "--pitch_range"),
    (["--augment", "gain", "--pitch_range", "0", "13"], "--pitch_range"),
    (["--augment", "remix", "--pitch_range", "-2", "nan"], "--pitch_range"),
    (["--augment", "remix", "--pitch_range", "-2", "2", "--stretch_range", "1.25", "0.8"], "--stretch_range"),
])
def test_train_refuses_bad_settings_before_a_device(flags, msg, tmp_path, capsys, monkeypatch):
    from svs_unet_pytorch_amd import train
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        train.main(["--label", "x", "--train_folder", str(tmp_path / "none"), *flags])
    assert e.value.code == 2                                               # parser.error
    assert msg in capsys.readouterr().err
    assert not (tmp_path / "LOG").exists() and not (tmp_path / "CKPT").exists()


def test_train_refuses_phaseless_folders(tmp_path, monkeypatch):
    from svs_unet_pytorch_amd import train
    monkeypatch.chdir(tmp_path)
    for d in ("mixture", "vocal"):
        (tmp_path / "set" / d).mkdir(parents=True)
        np.save(tmp_path / "set" / d / "a_spec.npy", np.zeros((257, 4), np.float32))
    with pytest.raises(SystemExit) as e:
        train.main(["--label", "x", "--train_folder", str(tmp_path / "set"), "--augment", "gain", "--pitch_range", "-2", "2",
                    "--win_size", "512", "--hop_size", "384"])
    assert "*_phase.npy" in str(e.value.code) and "--pitch_range" in str(e.value.code) and "no magnitude-only shift" in str(e.value.code)
    assert not (tmp_path / "LOG").exists()


def test_help_and_settings_line(capsys):
    from svs_unet_pytorch_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--pitch_range", "semitones", "-12 .. 12", "-2 2 is a starting point, not a tuned value", "formants"):
        assert word in text, word
    assert au.Augment().pitch_range is None and au.PITCH_RANGE == (-2.0, 2.0)
    plain = au.Augment("remix", (0.25, 1.25), 0.5, 3, (0.8, 1.25))
    assert "pitch" not in plain.describe()
    text = au.Augment("remix", (0.25, 1.25), 0.5, 3, (0.8, 1.25), (-2.0, 2.0)).describe()
    assert text.startswith(plain.describe()[:-len(", seed 3")]) and "pitch-shifted" in text and "[-2.0, 2.0]" in text and "seed 3" in text
    assert "-2 2 is a starting point, not a tuned value" in text
    assert "pitch-shifted" in au.Augment("gain", (0.25, 1.25), 0.5, 3, None, (-1.0, 1.0)).describe()
    assert au.check_settings("remix", (0.25, 1.25), 0.5, None, None) is None and au.check_settings("gain", (1.0, 1.0), 0.0, None, (-12.0, 12.0)) is None
    assert au.check_settings("gain", (1.0, 1.0), 0.0, (0.8, 1.25), (0.0, 0.0)) is None
    assert "--augment gain" in au.check_settings("none", (0.25, 1.25), 0.5, None, (-2.0, 2.0))
    for bad in ((2.0, -2.0), (-12.01, 0.0), (0.0, 12.01), (float("nan"), 1.0)):
        assert "--pitch_range" in au.check_settings("gain", (0.25, 1.25), 0.5, None, bad)


@pytest.mark.parametrize("extra", [[], ["--stretch_range", "0.8", "1.25"]])
def test_a_run_without_the_flag_reaches_none_of_the_new_functions(extra, tmp_path, capsys, monkeypatch):
    """--augment remix without --pitch_range (with and without --stretch_range) gets as far as the device check (there is no GPU in
    this half; on a machine with one, it is hidden) with every function of the pitch shift made to raise."""
    from svs_unet_pytorch_amd import train

    def forbidden(*args, **kw):
        raise AssertionError("a run without --pitch_range reached the pitch shift")
    for name in ("draw_epoch_pitch", "check_pitch_table", "pack_pitch_table", "upload_pitch_table", "crop_pitch", "pitch_reference",
                 "pitch_vocoder", "pitch_bins", "semitones_to_pitch"):
        monkeypatch.setattr(au, name, forbidden)
    monkeypatch.chdir(tmp_path)
    for d in ("mixture", "vocal"):
        (tmp_path / "set" / d).mkdir(parents=True)
        np.save(tmp_path / "set" / d / "a_spec.npy", np.zeros((257, 4), np.float32))
        np.save(tmp_path / "set" / d / "a_phase.npy", np.ones((257, 4), np.complex64))
    monkeypatch.setattr(train.torch.cuda, "is_available", lambda: False)
    seen = {}
    real = au.Augment
    monkeypatch.setattr(au, "Augment", lambda *a, **k: seen.setdefault("aug", real(*a, **k)))
    with pytest.raises(SystemExit) as e:
        train.main(["--label", "x", "--train_folder", str(tmp_path / "set"), "--augment", "remix", "--win_size", "512", "--hop_size", "384", *extra])
    assert "needs a ROCm device" in str(e.value.code)
    assert seen["aug"].pitch_range is None and seen["aug"].mode == "remix" and (seen["aug"].stretch_range is None) == (not extra)
