"""Remix and gain augmentation, the host half (no GPU): the entry point is declared, bound and exported; the float64 definition
(augment.remix_reference) IS the STFT of the re-mixed audio; draw_epoch's table is a function of (seed, epoch) with the stated
distributions and is shared by the ranks; every argument rule of svs_crop_remix_tiles is refused before any launch (host or null
pointers only: a call that got as far as a launch would come back with another code); the host-side range checks of crop_remix; and
train.main's refusal of bad settings before a device is touched."""
import types
from collections import Counter

import numpy as np
import pytest

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import augment as au

NAME = "svs_crop_remix_tiles"


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def err(lib):
    return lib.svs_last_error_string().decode()


def test_symbol_is_declared_bound_and_exported(lib):
    assert NAME in _lib.header_symbols() and NAME in _lib._SIGS and hasattr(lib, NAME)
    assert len(_lib._SIGS[NAME][1]) == 20 and lib.svs_version() == 1


# ---- the definition is the STFT of the re-mixed audio ----------------------------------------------------------------------

N_FFT, HOP = 512, 384


def stft64(y):
    """Centred, reflect-padded, periodic-Hann STFT in float64: (n_fft / 2 + 1, 1 + len / hop) complex."""
    pad = np.pad(y, N_FFT // 2, mode="reflect")
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)
    T = 1 + len(y) // HOP
    return np.stack([np.fft.rfft(w * pad[t * HOP:t * HOP + N_FFT]) for t in range(T)], axis=1)


def test_reference_is_the_stft_of_the_remixed_audio():
    """Two songs of 40 frames, vocal + accompaniment = mixture, both spectrograms divided by the mixture's maximum magnitude as data.py
    does and the DC row dropped.  remix_reference on their planes with start_v != start_a and gains (0.4, 1.2) against the STFT of
    y[t] = g_v v_A[t + start_v hop] / norm_A + g_a acc_B[t + start_a hop] / norm_B, on the columns that see no edge padding of y
    (ceil(n_fft / (2 hop)) = 1 frame at each end; the crops themselves lie inside their songs)."""
    rng = np.random.default_rng(7)
    frames, seg, gv, ga, start_v, start_a = 40, 16, 0.4, 1.2, 5, 17
    songs = []
    for s in range(2):
        n = HOP * (frames - 1)
        voc = np.convolve(rng.standard_normal(n + 8), np.ones(9) / 9, "valid") * (1 + 0.5 * np.sin(np.arange(n) / 700.0))
        acc = np.convolve(rng.standard_normal(n + 4), np.ones(5) / 5, "valid") * 0.7
        Xm, Xv = stft64(voc + acc), stft64(voc)
        assert Xm.shape == (N_FFT // 2 + 1, frames)
        norm = np.abs(Xm).max()
        songs.append(dict(voc=voc, acc=acc, norm=norm, M=np.abs(Xm)[1:] / norm, V=np.abs(Xv)[1:] / norm, pm=np.angle(Xm)[1:], pv=np.angle(Xv)[1:]))
    A, B = songs
    pick = lambda key: [s[key] for s in songs]
    ref = au.remix_reference(pick("M"), pick("V"), pick("pm"), pick("pv"), [0], [start_v], [1], [start_a],
                             np.array([gv], np.float32), np.array([ga], np.float32), seg)
    gv, ga = float(np.float32(gv)), float(np.float32(ga))                  # the gains the definition used
    L = HOP * (seg + 1)
    y = gv * A["voc"][start_v * HOP:start_v * HOP + L] / A["norm"] + ga * B["acc"][start_a * HOP:start_a * HOP + L] / B["norm"]
    Y = stft64(y)[1:, :seg]
    interior = slice(1, seg)                                               # frame 0 reflects y's own start; the last is (seg - 1)
    peak = np.abs(Y[:, interior]).max()
    assert peak > 0.05
    e_mag = np.abs(ref.mix[0, 0] - np.abs(Y))[:, interior].max() / peak
    e_z = np.abs(ref.z[0, 0] - Y)[:, interior].max() / peak
    e_polar = np.abs(ref.mix[0, 0] * np.exp(1j * ref.mix_phase[0, 0]) - Y)[:, interior].max() / peak
    assert max(e_mag, e_z, e_polar) <= 1e-10, (e_mag, e_z, e_polar)
    assert np.abs(ref.z[0, 0] - Y)[:, 0].max() / peak > 1e-6              # and the edge frame does carry the padding: the caveat is real
    assert np.array_equal(ref.voc[0, 0], gv * A["V"][:, start_v:start_v + seg]) and np.array_equal(ref.voc_phase[0, 0], A["pv"][:, start_v:start_v + seg])


def test_reference_gain_item_and_padding():
    rng = np.random.default_rng(3)
    M = [rng.random((4, 5)).astype(np.float32), rng.random((4, 20)).astype(np.float32)]
    V = [m * rng.random(m.shape).astype(np.float32) for m in M]
    pm = [rng.uniform(-np.pi, np.pi, m.shape).astype(np.float32) for m in M]
    pv = [rng.uniform(-np.pi, np.pi, m.shape).astype(np.float32) for m in M]
    g = np.array([0.5, 1.25], np.float32)
    ref = au.remix_reference(M, V, pm, pv, [0, 0], [0, 0], [-1, 1], [0, 10], g, g, 8)
    assert np.array_equal(ref.mix[0, 0, :, :5], 0.5 * M[0].astype(np.float64)) and not ref.mix[0, 0, :, 5:].any()
    assert np.array_equal(ref.mix_phase[0, 0, :, :5], pm[0].astype(np.float64)) and not ref.mix_phase[0, 0, :, 5:].any()
    assert not ref.voc[1, 0, :, 5:].any() and ref.mix[1, 0, :, 5:].any()   # the vocal ends, the other song's accompaniment goes on
    both =au.remix_reference(M, V, pm, pv, [0], [0], [1], [16], g[:1], g[:1], 8)
    assert not both.mix[0, 0, :, 5:].any()                                 # columns >= 5 are past song 0's end, columns >= 4 past song 1's
    plain = au.remix_reference(M, V, None, None, [1], [3], [99], [99], g[:1], g[:1], 8)      # the gain-only form reads no song_a
    assert plain.mix_phase is None and np.array_equal(plain.mix[0, 0], 0.5 * M[1][:, 3:11].astype(np.float64))


# ---- draw_epoch ------------------------------------------------------------------------------------------------------------

FRAMES = [300, 40, 129, 128, 1000]                                         # one song shorter than seg, one exactly seg long
SEG = 128


def test_draw_is_a_function_of_seed_and_epoch():
    a = au.draw_epoch(320, FRAMES, SEG, epoch=3, seed=11)
    b = au.draw_epoch(320, FRAMES, SEG, epoch=3, seed=11)
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))
    assert [x.dtype for x in a] == [np.int32] * 4 + [np.float32] * 2 and all(len(x) == 320 for x in a)
    assert np.array_equal(a.song_v, np.arange(320) % len(FRAMES))
    for other in (au.draw_epoch(320, FRAMES, SEG, epoch=4, seed=11), au.draw_epoch(320, FRAMES, SEG, epoch=3, seed=12)):
        for name in ("start_v", "song_a", "gain_v", "gain_a"):
            assert not np.array_equal(getattr(a, name), getattr(other, name)), name
        assert np.array_equal(a.song_v, other.song_v)


def test_draw_remix_probability_ends():
    never = au.draw_epoch(320, FRAMES, SEG, 0, 0, remix_prob=0.0)
    always = au.draw_epoch(320, FRAMES, SEG, 0, 0, remix_prob=1.0)
    assert (never.song_a == -1).all() and not never.start_a.any()
    assert (always.song_a >= 0).all() and (always.song_a < len(FRAMES)).all()
    assert set(always.song_a.tolist()) == set(range(len(FRAMES)))          # all songs are drawn ...
    assert (always.song_a == always.song_v).any()                          # ... the item's own included
    half = au.draw_epoch(4000, FRAMES, SEG, 0, 0, remix_prob=0.5)
    assert abs((half.song_a >= 0).mean() - 0.5) < 0.05                     # 6 sigma of 4000 fair draws is 0.047


@pytest.mark.parametrize("gain_range", [(0.25, 1.25), (1.0, 1.0), (0.9, 0.9000001)])
def test_draw_gains_lie_in_the_range(gain_range):
    t = au.draw_epoch(2000, FRAMES, SEG, 1, 5, gain_range=gain_range, remix_prob=1.0)
    lo, hi = np.float32(gain_range[0]), np.float32(gain_range[1])
    for g in (t.gain_v, t.gain_a):
        assert g.min() >= lo and g.max() <= hi
    if gain_range == (0.25, 1.25):
        assert t.gain_v.min() < 0.3 and t.gain_v.max() > 1.2 and abs(t.gain_v.mean() - 0.75) < 0.05


def test_draw_starts_lie_in_their_songs():
    t = au.draw_epoch(5000, FRAMES, SEG, 2, 0, remix_prob=1.0)
    room = np.maximum(np.array(FRAMES) - SEG, 0)
    assert (t.start_v >= 0).all() and (t.start_v <= room[t.song_v]).all()
    assert (t.start_a >= 0).all() and (t.start_a <= room[t.song_a]).all()
    for s in (1, 3):                                                       # shorter than seg / exactly seg: the start is 0
        assert not t.start_v[t.song_v == s].any() and not t.start_a[t.song_a == s].any()
    assert t.start_v[t.song_v == 2].max() == 1 and t.start_v[t.song_v == 0].max() == 300 - SEG      # both ends are reached
    au.check_table(t, FRAMES, SEG, has_angles=True)                        # and what is drawn passes the upload's own checks
    assert len(au.draw_epoch(0, FRAMES, SEG, 0).song_v) == 0 and len(au.draw_epoch(8, [], SEG, 0).song_v) == 0


def test_ranks_share_one_table():
    """Every rank draws the whole table and takes its items by train.epoch_order: the union over the ranks is, for world 1 / 2 / 4,
    the same multiset of (item, draw)."""
    from svs_unet_pytorch_amd.train import epoch_order
    n = 3 * 8
    frames = [300, 40, 500]

    def union(world):
        seen = Counter()
        for rank in range(world):
            table = au.draw_epoch(n, frames, SEG, epoch=6, seed=2)        # each rank draws its own copy
            packed = au.pack_table(table, epoch_order(n, True, rank, world, 6))
            assert packed.dtype == np.int32 and packed.shape[0] == 6
            seen.update(map(tuple, packed.T.tolist()))
        return seen
    one = union(1)
    assert sum(one.values()) == n and union(2) == one and union(4) == one
    whole = au.pack_table(au.draw_epoch(n, frames, SEG, 6, 2))
    assert Counter(map(tuple, whole.T.tolist())) == one
    assert np.array_equal(whole[4].view(np.float32), au.draw_epoch(n, frames, SEG, 6, 2).gain_v)    # the float rows are bit patterns


# ---- argument rules of the entry point -------------------------------------------------------------------------------------

# positions: 0 mix_songs 1 voc_songs 2 mix_ang 3 voc_ang 4 offset 5 frames 6 song_v 7 start_v 8 song_a 9 start_a 10 gain_v 11 gain_a
#            12 B 13 F 14 seg 15 mix 16 voc 17 mix_phase 18 voc_phase 19 stream
GOOD = [16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 2, 6, 8, 16, 32, 48, 64, None]      # never dereferenced: a check comes first


def changed(**kw):
    args = list(GOOD)
    for k, v in kw.items():
        args[int(k[1:])] = v
    return args


RULES = [
    (changed(_2=None), "mix_ang and voc_ang must both"),
    (changed(_3=None), "mix_ang and voc_ang must both"),
    (changed(_17=None), "mix_phase and voc_phase must both"),
    (changed(_18=None), "mix_phase and voc_phase must both"),
    (changed(_2=None, _3=None), "phase outputs need the angle sources"),
    (changed(_0=None), "null pointer"), (changed(_1=None), "null pointer"), (changed(_4=None), "null pointer"),
    (changed(_5=None), "null pointer"), (changed(_15=None), "null pointer"), (changed(_16=None), "null pointer"),
    (changed(_6=None), "null table"), (changed(_7=None), "null table"), (changed(_8=None), "null table"),
    (changed(_9=None), "null table"), (changed(_10=None), "null table"), (changed(_11=None), "null table"),
    (changed(_2=None, _3=None, _17=None, _18=None, _8=None), "null table"),          # the gain-only form still wants its tables
    (changed(_12=0), "bad geometry"), (changed(_13=0), "bad geometry"), (changed(_14=0), "bad geometry"),
    (changed(_12=-1), "bad geometry"), (changed(_14=6), "bad geometry"), (changed(_14=-8), "bad geometry"),
    (changed(_15=24), "16-byte aligned"), (changed(_16=4), "16-byte aligned"), (changed(_17=40), "16-byte aligned"),
    (changed(_18=8), "16-byte aligned"),
]


@pytest.mark.parametrize("args,msg", RULES)
def test_entry_point_refuses_before_any_launch(lib, args, msg):
    assert lib.svs_crop_remix_tiles(*args) == -1
    assert msg in err(lib) and err(lib).startswith(NAME + ":")


# ---- the binding's host-side checks ----------------------------------------------------------------------------------------

def fake_resident(angles=True):
    """What upload_table reads of a ResidentSpectrograms before anything goes to a device."""
    return types.SimpleNamespace(frames_host=[300, 40, 129], mix_ang=object() if angles else None, device="no such device", rows=4)


def table(**kw):
    base = dict(song_v=[0, 1, 2], start_v=[172, 0, 1], song_a=[2, -1, 0], start_a=[1, 0, 172], gain_v=[1.0, 0.5, 1.25], gain_a=[1.0, 1.0, 0.25])
    base.update(kw)
    return au.EpochTable(np.array(base["song_v"], np.int32), np.array(base["start_v"], np.int32), np.array(base["song_a"], np.int32),
                         np.array(base["start_a"], np.int32), np.array(base["gain_v"], np.float32), np.array(base["gain_a"], np.float32))


@pytest.mark.parametrize("kw,msg", [
    (dict(song_v=[0, 3, 2]), "song_v outside"), (dict(song_v=[-1, 1, 2]), "song_v outside"), (dict(song_a=[3, -1, 0]), "song_a outside"),
    (dict(start_v=[173, 0, 1]), "start_v outside"), (dict(start_v=[172, 1, 1]), "start_v outside"), (dict(start_v=[172, 0, -1]), "start_v outside"),
    (dict(start_a=[2, 0, 172]), "start_a outside"), (dict(start_a=[1, 0, 173]), "start_a outside"), (dict(start_a=[-1, 0, 0]), "start_a outside"),
    (dict(gain_v=[1.0, float("nan"), 1.0]), "not finite"), (dict(gain_a=[float("inf"), 1.0, 1.0]), "not finite"),
    (dict(gain_a=[1.0, 1.0]), "rows of"),
])
def test_crop_remix_checks_the_host_arrays(kw, msg):
    with pytest.raises(ValueError, match=msg):
        au.crop_remix(fake_resident(), table(**kw), 0, 3, with_phase=True)


def test_crop_remix_refuses_remix_items_without_angles():
    with pytest.raises(ValueError, match="remix items need the angles"):
        au.crop_remix(fake_resident(angles=False), table(), 0, 3)
    au.check_table(table(song_a=[-1, -1, -1], start_a=[999, -5, 0]), [300, 40, 129], 128, has_angles=False)     # gain items: start_a is not read
    au.check_table(table(), [300, 40, 129], 128, has_angles=True)


# ---- command line ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags,msg", [
    (["--gain_range", "1.25", "0.25"], "--gain_range"), (["--gain_range", "0", "1"], "--gain_range"),
    (["--gain_range", "-0.5", "1"], "--gain_range"), (["--gain_range", "0.5", "nan"], "--gain_range"),
    (["--remix_prob", "1.5"], "--remix_prob"), (["--remix_prob", "-0.1"], "--remix_prob"),
])
def test_train_refuses_bad_settings_before_a_device(flags, msg, tmp_path, capsys, monkeypatch):
    from svs_unet_pytorch_amd import train
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        train.main(["--label", "x", "--train_folder", str(tmp_path / "none"), "--augment", "remix", *flags])
    assert e.value.code == 2                                               # parser.error
    assert msg in capsys.readouterr().err
    assert not (tmp_path / "LOG").exists() and not (tmp_path / "CKPT").exists()


def test_train_refuses_other_loaders_and_phaseless_folders(tmp_path, capsys, monkeypatch):
    from svs_unet_pytorch_amd import train
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SVS_DATA_LOADER", "cpu")
    with pytest.raises(SystemExit) as e:
        train.main(["--label", "x", "--augment", "gain"])
    assert e.value.code == 2 and "SVS_DATA_LOADER=cpu" in capsys.readouterr().err
    monkeypatch.delenv("SVS_DATA_LOADER")
    for d in ("mixture", "vocal"):                                         # a folder with spectrograms and no phase files
        (tmp_path / "set" / d).mkdir(parents=True)
        np.save(tmp_path / "set" / d / "a_spec.npy", np.zeros((257, 4), np.float32))
    assert not train.folder_has_phase_files(str(tmp_path / "set"))
    with pytest.raises(SystemExit) as e:
        train.main(["--label", "x", "--train_folder", str(tmp_path / "set"), "--augment", "remix", "--win_size", "512", "--hop_size", "384"])
    assert "*_phase.npy" in str(e.value.code) and "--augment gain works without them" in str(e.value.code)
    assert not (tmp_path / "LOG").exists()
    for d in ("mixture", "vocal"):
        np.save(tmp_path / "set" / d / "a_phase.npy", np.ones((257, 4), np.complex64))
    assert train.folder_has_phase_files(str(tmp_path / "set"))


def test_help_names_the_flags_and_the_choice(capsys):
    from svs_unet_pytorch_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--augment", "--gain_range", "--remix_prob", "--augment_seed", "not a tuned value", "Open-Unmix"):
        assert word in text, word


def test_settings_line():
    assert au.Augment().describe() == "Augmentation: none"
    text = au.Augment("remix", (0.25, 1.25), 0.5, 3).describe()
    assert "remix" in text and "0.25" in text and "1.25" in text and "0.5" in text and "seed 3" in text
    assert au.check_settings("remix", (0.25, 1.25), 0.5) is None and au.check_settings("gain", (1.0, 1.0), 0.0) is None
