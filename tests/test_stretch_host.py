"""Time-stretch augmentation, the host half (no GPU): svs_crop_stretch_tiles is declared, bound and exported and refuses every bad
argument before any launch (host or null pointers only); the float64 definition (augment.phase_vocoder / stretch_reference) moves
stationary partials to where they belong, is the plain crop at rate 1 and is remix_reference's z on remix items; draw_epoch_stretch's
table is a function of (seed, epoch) with the stated distributions and is shared by the ranks; check_stretch_table's refusals; the
command line's refusals, its help text, and a run without --stretch_range that reaches none of the new functions."""
import types
from collections import Counter

import numpy as np
import pytest

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import augment as au

NAME = "svs_crop_stretch_tiles"


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def err(lib):
    return lib.svs_last_error_string().decode()


def test_symbol_is_declared_bound_and_exported(lib):
    assert NAME in _lib.header_symbols() and NAME in _lib._SIGS and hasattr(lib, NAME)
    assert len(_lib._SIGS[NAME][1]) == 24 and len(_lib._SIGS["svs_crop_remix_tiles"][1]) == 20 and lib.svs_version() == 1


# ---- argument rules of the entry point -------------------------------------------------------------------------------------

# positions: 0 mix_songs 1 voc_songs 2 mix_ang 3 voc_ang 4 offset 5 frames 6 song_v 7 start_v 8 song_a 9 start_a 10 gain_v 11 gain_a
#            12 rate_v 13 rate_a 14 B 15 F 16 seg 17 n_fft 18 hop 19 mix 20 voc 21 mix_phase 22 voc_phase 23 stream
GOOD = [16] * 14 + [2, 256, 8, 512, 384, 16, 32, 48, 64, None]             # never dereferenced: a check comes first


def changed(**kw):
    args = list(GOOD)
    for k, v in kw.items():
        args[int(k[1:])] = v
    return args


RULES = [(changed(**{f"_{i}": None}), "null pointer") for i in (0, 1, 2, 3, 4, 5, 19, 20)]            # the angles are required
RULES += [(changed(_2=None, _3=None, _21=None, _22=None), "null pointer")]                             # no magnitude-only form
RULES += [(changed(**{f"_{i}": None}), "null table") for i in range(6, 14)]
RULES += [
    (changed(_21=None), "mix_phase and voc_phase must both"), (changed(_22=None), "mix_phase and voc_phase must both"),
    (changed(_14=0), "bad geometry"), (changed(_14=-1), "bad geometry"), (changed(_16=0), "bad geometry"), (changed(_16=6), "bad geometry"),
    (changed(_16=-8), "bad geometry"), (changed(_16=130), "bad geometry"),
    (changed(_19=24), "16-byte aligned"), (changed(_20=4), "16-byte aligned"), (changed(_21=40), "16-byte aligned"),
    (changed(_22=8), "16-byte aligned"),
    (changed(_17=0), "n_fft must be 512, 1024 or 2048"), (changed(_17=256), "n_fft must be 512, 1024 or 2048"),
    (changed(_17=1000), "n_fft must be 512, 1024 or 2048"), (changed(_17=4096, _15=2048), "n_fft must be 512, 1024 or 2048"),
    (changed(_15=0), "1 <= F <= n_fft / 2"), (changed(_15=257), "1 <= F <= n_fft / 2"), (changed(_15=512), "1 <= F <= n_fft / 2"),
    (changed(_15=-4), "1 <= F <= n_fft / 2"), (changed(_17=1024, _15=513), "1 <= F <= n_fft / 2"),
    (changed(_18=0), "hop must be in 1..n_fft"), (changed(_18=-384), "hop must be in 1..n_fft"), (changed(_18=513), "hop must be in 1..n_fft"),
]


@pytest.mark.parametrize("args,msg", RULES)
def test_entry_point_refuses_before_any_launch(lib, args, msg):
    assert lib.svs_crop_stretch_tiles(*args) == -1
    assert msg in err(lib) and err(lib).startswith(NAME + ":")


# ---- the definition --------------------------------------------------------------------------------------------------------

RATES = [1024, 819, 1333, 512, 2048]


@pytest.mark.parametrize("n_fft,hop", [(1024, 768), (512, 300)])
@pytest.mark.parametrize("q", RATES)
def test_stationary_partials_keep_their_frequency(n_fft, hop, q):
    """S[f, t] = A_f cis(theta_f + w0_f hop t), one partial per row within the unambiguous range of its bin (|w0 hop - w| < pi, i.e.
    within n_fft / (2 hop) bins of the bin's centre): stretched at any rate from any start s, frame t is A_f cis(theta_f +
    w0_f hop (s + t)) -- the magnitude untouched, the frequency kept, the phase continuous.  1e-8 is the float64 exp of arguments
    up to w0 hop T ~ 8e5 rad."""
    rng = np.random.default_rng(q + n_fft)
    F, T, seg, s = n_fft // 2, 300, 128, 17
    assert s + au.span(q, seg) <= T
    A = rng.uniform(0.1, 1.0, F)
    theta = rng.uniform(-np.pi, np.pi, F)
    off = rng.uniform(-0.45, 0.45, F) * (n_fft / (2.0 * hop))              # bins off the centre, inside the unambiguous range
    w0 = 2.0 * np.pi * (np.arange(1, F + 1) + off) / n_fft
    t_src = np.arange(T)
    plane = A[:, None] * np.exp(1j * (theta[:, None] + w0[:, None] * hop * t_src[None, :]))
    mag, acc, cond = au.phase_vocoder(plane, s, q, seg, n_fft, hop)
    want = A[:, None] * np.exp(1j * (theta[:, None] + w0[:, None] * hop * (s + np.arange(seg))[None, :]))
    e = np.abs(mag * np.exp(1j * acc) - want).max()
    print(f"partials ({n_fft}, {hop}) q={q}: worst error {e:.2e}")
    assert e <= 1e-8, e
    assert np.array_equal(cond, np.broadcast_to(1.0 + 2.0 * np.arange(seg), (F, seg)))     # unit weights: 2 t + 1 frames entered acc


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


def test_rate_one_is_the_plain_crop_and_the_remix():
    frames, F, seg = [40, 9, 23], 6, 8
    M, V, pm, pv = songs_fp32(frames, F, 5, zero_bin=2)
    # (song_v, start_v, song_a, start_a): a gain item, remix items A != B and A == B, and sources that end inside the tile
    items = [(0, 3, -1, 0), (0, 30, 2, 15), (2, 1, 2, 9), (1, 4, 0, 31), (1, 0, 1, 0)]
    sv, st, sa, sta = (np.array(c, np.int32) for c in zip(*items))
    gv, ga = np.linspace(0.3, 1.2, len(items)).astype(np.float32), np.linspace(1.25, 0.25, len(items)).astype(np.float32)
    one = np.full(len(items), 1024, np.int32)
    gv[0] = ga[0] = 1.0                                                    # the gain item (g_v V + g_a (M - V), B = A) at unit gains
    ref = au.stretch_reference(M, V, pm, pv, sv, st, sa, sta, gv, ga, one, one, seg, 512, 384)
    remix = au.remix_reference(M, V, pm, pv, sv, st, sa, sta, gv, ga, seg)
    assert np.abs(ref.z[1:] - remix.z[1:]).max() <= 1e-11 and np.abs(ref.mix[1:] - remix.mix[1:]).max() <= 1e-11
    assert np.abs(ref.voc - remix.voc).max() <= 1e-11 and np.abs(ref.zv - remix.voc * np.exp(1j * remix.voc_phase)).max() <= 1e-11
    own = au._crop64(M[0], 3, seg) * np.exp(1j * au._crop64(pm[0], 3, seg)) * float(gv[0])        # the gain item: the plain crop
    assert np.abs(ref.z[0, 0] - own).max() <= 1e-11
    assert np.abs(ref.mix[0, 0] * np.exp(1j * ref.mix_phase[0, 0]) - own).max() <= 1e-11
    assert not ref.mix[:, 0, 2].any() and not ref.mix_phase[:, 0, 2].any() and not ref.voc_phase[:, 0, 2].any()     # the silent band
    assert not ref.voc[3, 0, :, 5:].any() and not ref.voc_phase[3, 0, :, 5:].any() and ref.mix[3, 0, [0, 1, 3, 4, 5], 5:].all()
    assert (np.abs(ref.voc_phase) <= np.pi).all() and (np.abs(ref.mix_phase) <= np.pi).all()
    assert (ref.scale >= ref.mix - 1e-12).all()                            # |z| <= g_v V + g_a (M + V): the triangle inequality
    assert np.array_equal(ref.cond_v[0, 0], np.broadcast_to(1.0 + 2.0 * np.arange(seg), (F, seg)))


def test_reference_gain_item_is_the_remix_item_with_itself():
    M, V, pm, pv = songs_fp32([60, 50], 4, 9)
    g = np.array([0.7], np.float32)
    a = au.stretch_reference(M, V, pm, pv, [1], [5], [-1], [0], g, g, [819], [2048], 16, 512, 128)
    b = au.stretch_reference(M, V, pm, pv, [1], [5], [1], [5], g, g, [819], [819], 16, 512, 128)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c = au.stretch_reference(M, V, pm, pv, [1], [5], [1], [5], g, g, [819], [1333], 16, 512, 128)
    assert np.array_equal(c.zv, a.zv) and not np.allclose(c.z, a.z)        # the sources have rates of their own
    assert (a.cond_a >= a.cond_v - 1e-9).all()                             # (M + V) / |M cis - V cis| >= 1


# ---- draw_epoch_stretch ----------------------------------------------------------------------------------------------------

FRAMES = [300, 40, 129, 128, 1000]
SEG = 128


def test_draw_is_a_function_of_seed_and_epoch():
    a = au.draw_epoch_stretch(320, FRAMES, SEG, epoch=3, seed=11)
    b = au.draw_epoch_stretch(320, FRAMES, SEG, epoch=3, seed=11)
    assert isinstance(a, au.StretchTable) and a._fields == au.EpochTable._fields + ("rate_v", "rate_a")
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))
    assert [x.dtype for x in a] == [np.int32] * 4 + [np.float32] * 2 + [np.int32] * 2 and all(len(x) == 320 for x in a)
    assert np.array_equal(a.song_v, np.arange(320) % len(FRAMES))
    for other in (au.draw_epoch_stretch(320, FRAMES, SEG, epoch=4, seed=11), au.draw_epoch_stretch(320, FRAMES, SEG, epoch=3, seed=12)):
        for name in ("start_v", "song_a", "gain_v", "gain_a", "rate_v", "rate_a"):
            assert not np.array_equal(getattr(a, name), getattr(other, name)), name
    assert len(au.draw_epoch_stretch(0, FRAMES, SEG, 0).rate_v) == 0 and len(au.draw_epoch_stretch(8, [], SEG, 0).rate_a) == 0


@pytest.mark.parametrize("stretch_range", [(0.8, 1.25), (0.5, 2.0), (1.0, 1.0), (1.3, 1.3)])
def test_draw_rates_and_starts(stretch_range):
    t = au.draw_epoch_stretch(6000, FRAMES, SEG, 2, 7, remix_prob=0.5, stretch_range=stretch_range)
    q_lo, q_hi = round(1024 * stretch_range[0]), round(1024 * stretch_range[1])
    remix = t.song_a >= 0
    assert remix.any() and (~remix).any()
    for q in (t.rate_v, t.rate_a):
        assert q.min() == q_lo and q.max() == q_hi                         # both ends of the range are reached
    assert np.array_equal(t.rate_a[~remix], t.rate_v[~remix]) and not t.start_a[~remix].any()
    frames = np.array(FRAMES)
    room_v = np.maximum(frames[t.song_v] - au.span(t.rate_v, SEG), 0)
    room_a = np.maximum(frames[t.song_a[remix]] - au.span(t.rate_a[remix], SEG), 0)
    assert (t.start_v >= 0).all() and (t.start_v <= room_v).all()
    assert (t.start_a[remix] >= 0).all() and (t.start_a[remix] <= room_a).all()
    assert (t.start_v == room_v)[room_v > 0].any() and (t.start_v[room_v > 0] == 0).any()          # both ends of room(q) are reached
    assert not t.start_v[t.song_v == 1].any()                              # a 40-frame song never holds a span: the start is 0
    au.check_stretch_table(t, FRAMES, SEG)                                 # and what is drawn passes the upload's own checks
    assert int(au.span(1024, 128)) == 129 and int(au.span(512, 128)) == 65 and int(au.span(2048, 128)) == 256 and int(au.span(1333, 8)) == 11


def test_ranks_share_one_table():
    from svs_unet_pytorch_amd.train import epoch_order
    n, frames = 3 * 8, [300, 40, 500]

    def union(world):
        seen = Counter()
        for rank in range(world):
            table = au.draw_epoch_stretch(n, frames, SEG, epoch=6, seed=2)
            packed = au.pack_stretch_table(table, epoch_order(n, True, rank, world, 6))
            assert packed.dtype == np.int32 and packed.shape[0] == 8 and packed.flags.c_contiguous
            seen.update(map(tuple, packed.T.tolist()))
        return seen
    one = union(1)
    assert sum(one.values()) == n and union(2) == one and union(4) == one
    t = au.draw_epoch_stretch(n, frames, SEG, 6, 2)
    whole = au.pack_stretch_table(t)
    assert np.array_equal(whole[:6], au.pack_table(au.EpochTable(*t[:6]))) and np.array_equal(whole[6], t.rate_v) and np.array_equal(whole[7], t.rate_a)


# ---- check_stretch_table / crop_stretch ------------------------------------------------------------------------------------

def fake_resident(angles=True, rows=256):
    return types.SimpleNamespace(frames_host=[300, 40, 129], mix_ang=object() if angles else None, device="no such device", rows=rows)


def table(**kw):
    # room: song 0 at q 1024: 300 - 129 = 171; at 2048: 300 - 256 = 44; song 2 at 512: 129 - 65 = 64
    base = dict(song_v=[0, 1, 2], start_v=[171, 0, 64], song_a=[2, -1, 0], start_a=[64, 0, 44], gain_v=[1.0, 0.5, 1.25], gain_a=[1.0, 1.0, 0.25],
                rate_v=[1024, 819, 512], rate_a=[512, 1024, 2048])
    base.update(kw)
    i32, f32 = (lambda k: np.array(base[k], np.int32)), (lambda k: np.array(base[k], np.float32))
    return au.StretchTable(i32("song_v"), i32("start_v"), i32("song_a"), i32("start_a"), f32("gain_v"), f32("gain_a"), i32("rate_v"), i32("rate_a"))


@pytest.mark.parametrize("kw,msg", [
    (dict(song_v=[0, 3, 2]), "song_v outside"), (dict(song_v=[-1, 1, 2]), "song_v outside"), (dict(song_a=[3, -1, 0]), "song_a outside"),
    (dict(start_v=[172, 0, 64]), "start_v outside"), (dict(start_v=[171, 1, 64]), "start_v outside"), (dict(start_v=[171, 0, 65]), "start_v outside"),
    (dict(start_v=[-1, 0, 0]), "start_v outside"), (dict(rate_v=[1040, 819, 512]), "start_v outside"),
    (dict(start_a=[65, 0, 44]), "start_a outside"), (dict(start_a=[64, 0, 45]), "start_a outside"), (dict(start_a=[-1, 0, 0]), "start_a outside"),
    (dict(rate_v=[511, 819, 512]), "rate_v outside"), (dict(rate_v=[1024, 2049, 512]), "rate_v outside"), (dict(rate_v=[0, 819, 512]), "rate_v outside"),
    (dict(rate_a=[511, 1024, 2048]), "rate_a outside"), (dict(rate_a=[512, 1024, 2049]), "rate_a outside"),
    (dict(gain_v=[1.0, float("nan"), 1.0]), "not finite"), (dict(gain_a=[float("inf"), 1.0, 1.0]), "not finite"),
    (dict(rate_a=[512, 1024]), "rows of"),
])
def test_crop_stretch_checks_the_host_arrays(kw, msg):
    with pytest.raises(ValueError, match=msg):
        au.crop_stretch(fake_resident(), table(**kw), 0, 3, 512, 384, with_phase=True)


def test_check_stretch_table_accepts_and_needs_angles():
    au.check_stretch_table(table(), [300, 40, 129], 128)
    au.check_stretch_table(table(rate_a=[512, 7, 2048], start_a=[64, -9, 44]), [300, 40, 129], 128)    # a gain item's rate_a / start_a are not read
    with pytest.raises(ValueError, match=r"needs the angles"):
        au.crop_stretch(fake_resident(angles=False), table(), 0, 3, 512, 384)
    with pytest.raises(ValueError, match=r"needs the angles"):
        au.check_stretch_table(table(), [300, 40, 129], 128, has_angles=False)


# ---- command line ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags,msg", [
    (["--augment", "none", "--stretch_range", "0.8", "1.25"], "needs --augment gain or --augment remix"),
    (["--stretch_range", "0.8", "1.25"], "needs --augment gain or --augment remix"),
    (["--augment", "remix", "--stretch_range", "1.25", "0.8"], "--stretch_range"),
    (["--augment", "gain", "--stretch_range", "0.4", "1.0"], "--stretch_range"),
    (["--augment", "gain", "--stretch_range", "1.0", "2.5"], "--stretch_range"),
    (["--augment", "remix", "--stretch_range", "0.8", "nan"], "--stretch_range"),
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
        train.main(["--label", "x", "--train_folder", str(tmp_path / "set"), "--augment", "gain", "--stretch_range", "0.8", "1.25",
                    "--win_size", "512", "--hop_size", "384"])
    assert "*_phase.npy" in str(e.value.code) and "--stretch_range" in str(e.value.code) and "no magnitude-only stretch" in str(e.value.code)
    assert not (tmp_path / "LOG").exists()


def test_help_and_settings_line(capsys):
    from svs_unet_pytorch_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--stretch_range", "0.8 1.25", "not a tuned value", "2/3 bin", "smaller --hop_size"):
        assert word in text, word
    assert au.Augment().stretch_range is None and au.STRETCH_RANGE == (0.8, 1.25)
    plain = au.Augment("remix", (0.25, 1.25), 0.5, 3)
    assert "stretch" not in plain.describe()
    text = au.Augment("remix", (0.25, 1.25), 0.5, 3, (0.8, 1.25)).describe()
    assert text.startswith(plain.describe()[:-len(", seed 3")]) and "time-stretched" in text and "0.8" in text and "seed 3" in text
    assert au.check_settings("remix", (0.25, 1.25), 0.5) is None and au.check_settings("gain", (1.0, 1.0), 0.0, (0.5, 2.0)) is None
    assert "--augment gain" in au.check_settings("none", (0.25, 1.25), 0.5, (0.8, 1.25))
    for bad in ((1.25, 0.8), (0.49, 1.0), (1.0, 2.01), (float("nan"), 1.0)):
        assert "--stretch_range" in au.check_settings("gain", (0.25, 1.25), 0.5, bad)


def test_a_run_without_the_flag_reaches_none_of_the_new_functions(tmp_path, capsys, monkeypatch):
    """--augment remix without --stretch_range gets as far as the device check (there is no GPU in this half; on a machine with one,
    the folder is missing) with every function of the stretch made to raise: the flag's absence reaches none of them."""
    from svs_unet_pytorch_amd import train

    def forbidden(*args, **kw):
        raise AssertionError("a run without --stretch_range reached the stretch")
    for name in ("draw_epoch_stretch", "check_stretch_table", "pack_stretch_table", "upload_stretch_table", "crop_stretch",
                 "stretch_reference", "phase_vocoder", "span"):
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
        train.main(["--label", "x", "--train_folder", str(tmp_path / "set"), "--augment", "remix", "--win_size", "512", "--hop_size", "384"])
    assert "needs a ROCm device" in str(e.value.code)
    assert seen["aug"].stretch_range is None and seen["aug"].mode == "remix"
