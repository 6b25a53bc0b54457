"""Remix and gain augmentation on the device (-m gpu): svs_crop_remix_tiles against the float64 definition (augment.remix_reference)
at a small shape that exercises every padding case and at the production shape, with the derived bounds

    |mix - ref| <= 16 * 2^-23 * S                                  S = g_v V_A + g_a (M_B + V_B)
    |mix cis(mix_phase) - z_ref| <= 16 * 2^-23 * S + 8 * 2^-22 * |z_ref|

(at most 4 ulp for sin / cos / sqrt and 6 ulp for atan2 -- the OpenCL-profile limits of the device library --, half an ulp per
multiply and add, and an fp32 angle near pi), voc and voc_phase bit-exact; the gain-only paths bit for bit against svs_crop_tiles;
the form without phase outputs; ResidentSpectrograms.augmented_batches on a synthetic folder; and one training step on an augmented
batch.  Angles are compared only through the reconstituted complex value: an angle alone is ill-conditioned where |z| is small.

Worst error-to-bound ratios seen on an MI355X: see DESIGN.md section 16."""
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


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr()


class Songs:
    """A resident set built by hand: per-song (F, T) planes (the float64 reference's inputs) and the flat device buffers with a NaN
    tail, so that a read past the last song shows as NaN in an output and never leaves the allocation."""

    def __init__(self, frames, F, seed, zero_bin=None):
        rng = np.random.default_rng(seed)
        self.frames_host, self.F = list(frames), F
        self.M = [rng.random((F, T)).astype(np.float32) for T in frames]
        self.V = [(m * rng.random(m.shape)).astype(np.float32) for m in self.M]
        self.pm = [rng.uniform(-np.pi, np.pi, (F, T)).astype(np.float32) for T in frames]
        self.pv = [rng.uniform(-np.pi, np.pi, (F, T)).astype(np.float32) for T in frames]
        if zero_bin is not None:                                           # a source bin with M = V = 0 (a silent band), in every song
            for a in self.M + self.V:
                a[zero_bin] = 0.0
        for p in self.pm + self.pv:                                        # the ends of atan2f's range occur too
            p[0, 0], p[-1, -1] = np.float32(np.pi), np.float32(-np.pi)
        flat = lambda parts: torch.from_numpy(np.concatenate([p.reshape(-1) for p in parts] + [np.full(NAN_TAIL, np.nan, np.float32)])).to(DEV)
        self.mix, self.voc, self.mix_ang, self.voc_ang = flat(self.M), flat(self.V), flat(self.pm), flat(self.pv)
        sizes = [F * T for T in frames]
        self.offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]), dtype=torch.int64, device=DEV)
        self.frames = torch.tensor(self.frames_host, dtype=torch.int32, device=DEV)

    def reference(self, table, seg, angles=True):
        return au.remix_reference(self.M, self.V, self.pm if angles else None, self.pv if angles else None, *table, seg)


def table_of(items):
    """EpochTable from rows of (song_v, start_v, song_a, start_a, gain_v, gain_a)."""
    cols = list(zip(*items))
    return au.EpochTable(*(np.array(c, np.int32) for c in cols[:4]), *(np.array(c, np.float32) for c in cols[4:]))


def run(songs, table, seg, with_phase=True, angles=True):
    """svs_crop_remix_tiles into guarded buffers -> host tiles (mix, voc[, mix_phase, voc_phase]); the guards are checked here."""
    B, F = len(table.song_v), songs.F
    n = B * F * seg
    dev_table = torch.from_numpy(au.pack_table(table)).to(DEV)
    bufs = [torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(4 if with_phase else 2)]
    ptrs = [b.data_ptr() + 4 * GUARD for b in bufs] + [None] * (4 - len(bufs))
    _lib.check(L().svs_crop_remix_tiles(songs.mix.data_ptr(), songs.voc.data_ptr(), songs.mix_ang.data_ptr() if angles else None,
                                        songs.voc_ang.data_ptr() if angles else None, songs.offsets.data_ptr(), songs.frames.data_ptr(),
                                        *(dev_table[r].data_ptr() for r in range(6)), B, F, seg, *ptrs, S()), "svs_crop_remix_tiles")
    out = []
    for b in bufs:
        h = b.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[GUARD + n:] == SENTINEL), "a guard float was overwritten"
        out.append(h[GUARD:GUARD + n].reshape(B, 1, F, seg))
    return out


def crop_plain(songs, song, start, seg, pair):
    """svs_crop_tiles on the magnitudes (pair 0) or the angles (pair 1) -> two host tiles."""
    B = len(song)
    a_src, b_src = ((songs.mix, songs.voc), (songs.mix_ang, songs.voc_ang))[pair]
    tab = torch.tensor([song, start], dtype=torch.int32, device=DEV)
    a = torch.empty((B, 1, songs.F, seg), dtype=torch.float32, device=DEV)
    b = torch.empty_like(a)
    _lib.check(L().svs_crop_tiles(a_src.data_ptr(), b_src.data_ptr(), songs.offsets.data_ptr(), songs.frames.data_ptr(), tab[0].data_ptr(),
                                  tab[1].data_ptr(), B, songs.F, seg, a.data_ptr(), b.data_ptr(), S()), "svs_crop_tiles")
    return a.cpu().numpy(), b.cpu().numpy()


def ratios(got, ref):
    """(worst |mix - ref| / bound, worst |mix cis(mix_phase) - z_ref| / bound), an excess where the bound is 0 counting as inf."""
    mix, _, mix_phase, _ = (g.astype(np.float64) for g in got)
    b_mag = 16 * U * ref.scale
    b_z = 16 * U * ref.scale + 8 * 2.0 ** -22 * np.abs(ref.z)
    e_mag = np.abs(mix - ref.mix)
    e_z = np.abs(mix * np.exp(1j * mix_phase) - ref.z)

    def worst(e, b):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(b > 0, e / b, np.where(e > 0, np.inf, 0.0))
        return float(r.max())
    return worst(e_mag, b_mag), worst(e_z, b_z)


def check_against_reference(tag, songs, table, seg, report):
    got = run(songs, table, seg)
    ref = songs.reference(table, seg)
    for name, g in zip(("mix", "voc", "mix_phase", "voc_phase"), got):
        assert np.isfinite(g).all(), f"{tag}: {name} has a NaN or an infinity (a read past a song's end?)"
    assert (np.abs(got[2]) <= np.float32(np.pi)).all()
    r_mag, r_z = ratios(got, ref)
    print(f"{tag}: worst |mix - ref| / bound {r_mag:.3f}, worst |mix cis(phase) - z| / bound {r_z:.3f}")
    ok_mag = report(f"{tag}: |mix - ref| over 16 * 2^-23 * S", r_mag, 1.0)
    ok_z = report(f"{tag}: |mix cis(mix_phase) - z| over its bound", r_z, 1.0)
    assert ok_mag and ok_z, (r_mag, r_z)
    assert np.array_equal(got[1], ref.voc.astype(np.float32)), f"{tag}: voc is not g_v * V_A bit for bit"
    assert np.array_equal(got[3], ref.voc_phase.astype(np.float32)), f"{tag}: voc_phase is not the copied angle"
    return got, ref


# ---- the small shape: every padding case ---------------------------------------------------------------------------------

SMALL_FRAMES, SMALL_F, SMALL_SEG = [3, 8, 11, 37], 6, 8
# (song_v, start_v, song_a, start_a, gain_v, gain_a); T - seg = 0, 0, 3, 29
SMALL_ITEMS = [
    (3, 1, 2, 3, 0.4, 1.2),        # remix A != B; starts = 1 mod 4 and T - seg (= 3 mod 4)
    (3, 29, 3, 2, 0.8, 0.5),       # remix A = B, different starts: T - seg and = 2 mod 4
    (3, 7, 3, 7, 1.0, 1.0),        # remix A = B, the same start (= 3 mod 4), gains 1: the item's own mixture, through the complex path
    (1, 0, -1, 0, 0.7, 9.0),       # gain-only, on the song that fills its tile exactly (its neighbour follows in the buffer); gain_a unused
    (0, 0, 3, 0, 1.1, 0.9),        # the short song as vocal source: voc is padded from column 3, the accompaniment goes on
    (2, 0, 0, 0, 0.6, 1.25),       # the short song as accompaniment source
    (0, 0, 0, 0, 0.25, 0.3),       # both sources short: columns 3.. are padding in both
]


@functools.lru_cache(maxsize=None)
def small_songs():
    return Songs(SMALL_FRAMES, SMALL_F, seed=1, zero_bin=2)


def test_small_shape_against_the_definition(report):
    songs, table = small_songs(), table_of(SMALL_ITEMS)
    au.check_table(table, SMALL_FRAMES, SMALL_SEG, has_angles=True)
    got, ref = check_against_reference("crop_remix small (7, 6, 8)", songs, table, SMALL_SEG, report)
    mix, voc, mix_phase, voc_phase = got
    for b in (4, 6):                                                       # vocal source of 3 frames: padded columns are exactly 0
        assert not voc[b, 0, :, 3:].any() and not voc_phase[b, 0, :, 3:].any() and voc[b, 0, :, :3].any()
    assert mix[4, 0, :, 3:].any()                                          # ... while the other song's accompaniment goes on
    assert not mix[6, 0, :, 3:].any() and not mix_phase[6, 0, :, 3:].any() # both padded: exactly 0
    assert voc[5, 0, [0, 1, 3, 4, 5], 3:].all() and mix[5, 0, [0, 1, 3, 4, 5], 3:].all()      # accompaniment padded, vocal not
    for b in range(len(SMALL_ITEMS)):                                      # the silent band: exactly 0 in, exactly 0 out
        assert not mix[b, 0, 2].any() and not voc[b, 0, 2].any()
    # item 2 is its own mixture (V cis + (M cis - V cis)): within the same bound of the plain crop
    own = songs.M[3][:, 7:15].astype(np.float64)
    assert np.all(np.abs(mix[2, 0] - own) <= 16 * U * ref.scale[2, 0])


def test_production_shape_against_the_definition(report):
    songs = Songs([100, 128, 300, 517], 512, seed=2)
    table = table_of([(2, 171, 3, 389, 0.3, 1.25),     # remix A != B, odd starts, the second at T - seg
                      (3, 2, 0, 0, 1.25, 0.25),        # the short song (100 < 128) as accompaniment
                      (0, 0, -1, 0, 0.5, 1.0)])        # gain-only on the short song
    au.check_table(table, songs.frames_host, 128, has_angles=True)
    got, _ = check_against_reference("crop_remix production (3, 512, 128)", songs, table, 128, report)
    assert not got[0][2, 0, :, 100:].any() and not got[1][2, 0, :, 100:].any() and got[0][1, 0, :, 100:].all()


# ---- gain-only items and the gain-only form --------------------------------------------------------------------------------

GAIN_SONGS = [0, 1, 2, 2, 3, 3, 3]
GAIN_STARTS = [0, 0, 1, 3, 0, 29, 14]


def gain_table(g, song_a=None):
    """Every (song, start) of GAIN_* as a gain item (song_a -1 unless given), gain_v = g and a gain_a that must not matter."""
    song_a = [-1] * len(GAIN_SONGS) if song_a is None else song_a
    return table_of([(s, st, a, 0, g, 3.0) for s, st, a in zip(GAIN_SONGS, GAIN_STARTS, song_a)])


def test_gain_items_at_one_are_the_plain_crop():
    songs = small_songs()
    got = run(songs, gain_table(1.0), SMALL_SEG)
    want = crop_plain(songs, GAIN_SONGS, GAIN_STARTS, SMALL_SEG, 0) + crop_plain(songs, GAIN_SONGS, GAIN_STARTS, SMALL_SEG, 1)
    for name, g, w in zip(("mix", "voc", "mix_phase", "voc_phase"), got, want):
        assert np.array_equal(g, w), name
    assert np.isfinite(got[0]).all() and not got[0][0, 0, :, 3:].any()


@pytest.mark.parametrize("g", [0.25, 0.7, 1.2345678])
def test_gain_items_are_one_multiply(g):
    songs = small_songs()
    got = run(songs, gain_table(g), SMALL_SEG)
    mix, voc = crop_plain(songs, GAIN_SONGS, GAIN_STARTS, SMALL_SEG, 0)
    ang = crop_plain(songs, GAIN_SONGS, GAIN_STARTS, SMALL_SEG, 1)
    assert np.array_equal(got[0], np.float32(g) * mix) and np.array_equal(got[1], np.float32(g) * voc)
    assert np.array_equal(got[2], ang[0]) and np.array_equal(got[3], ang[1])


def test_gain_only_form_never_reads_song_a():
    """NULL angle sources: every item is a gain item, whatever song_a says (values that are no song of the set)."""
    songs = small_songs()
    n = len(GAIN_SONGS)
    wild = gain_table(0.7, song_a=[4 + i % 4 for i in range(n)])
    got = run(songs, wild, SMALL_SEG, with_phase=False, angles=False)
    mix, voc = crop_plain(songs, GAIN_SONGS, GAIN_STARTS, SMALL_SEG, 0)
    assert len(got) == 2 and np.array_equal(got[0], np.float32(0.7) * mix) and np.array_equal(got[1], np.float32(0.7) * voc)
    same = run(songs, gain_table(0.7), SMALL_SEG, with_phase=False, angles=True)      # and it is the result of gain items with angles
    assert np.array_equal(same[0], got[0]) and np.array_equal(same[1], got[1])
    ref = songs.reference(wild, SMALL_SEG, angles=False)
    assert np.array_equal(got[0], ref.mix.astype(np.float32)) and np.array_equal(got[1], ref.voc.astype(np.float32))


def test_without_phase_outputs_mix_and_voc_are_the_same():
    songs, table = small_songs(), table_of(SMALL_ITEMS)
    full = run(songs, table, SMALL_SEG, with_phase=True)
    lean = run(songs, table, SMALL_SEG, with_phase=False)
    assert len(lean) == 2 and np.array_equal(lean[0], full[0]) and np.array_equal(lean[1], full[1])
    big = Songs([140, 200], 512, seed=5)
    t2 = table_of([(0, 3, 1, 70, 0.9, 0.6), (1, 72, 0, 12, 0.3, 1.1)])
    full, lean = run(big, t2, 128, with_phase=True), run(big, t2, 128, with_phase=False)
    assert np.array_equal(lean[0], full[0]) and np.array_equal(lean[1], full[1])


# ---- ResidentSpectrograms.augmented_batches ----------------------------------------------------------------------------------

FOLDER_FRAMES = [100, 200, 333]      # one song shorter than the 128-frame tile
PER_SONG = 4


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """A synthetic folder of 3 songs at win 512: 257-row magnitude files with unit-phasor phase files."""
    root = tmp_path_factory.mktemp("augment_set")
    rng = np.random.default_rng(11)
    for d in ("mixture", "vocal"):
        os.makedirs(root / d)
    for i, T in enumerate(FOLDER_FRAMES):
        mix = rng.random((257, T)).astype(np.float32)
        for d, mag in (("mixture", mix), ("vocal", (mix * rng.random((257, T))).astype(np.float32))):
            np.save(root / d / f"{i:04d}_song_spec.npy", mag)
            np.save(root / d / f"{i:04d}_song_phase.npy", np.exp(1j * rng.uniform(-np.pi, np.pi, (257, T))).astype(np.complex64))
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


def test_augmented_batches_with_unit_gains_are_the_plain_crops(resident):
    assert resident.rows == 256 and resident.has_phase and len(resident) == 12
    aug = au.Augment("gain", (1.0, 1.0), 0.5, seed=4)                       # mode gain: remix_prob is not used
    epoch, seen = 3, 0
    for rank in range(2):
        order = svs_train.epoch_order(len(resident), True, rank, 2, epoch)
        drawn = au.draw_epoch(len(resident), resident.frames_host, 128, epoch, 4, (1.0, 1.0), 0.0)
        batches = list(resident.augmented_batches(4, rank, 2, epoch, with_phase=True, aug=aug))
        assert [b[0].shape[0] for b in batches] == [4, 2] and all(len(b) == 4 and b[0].shape == (b[0].shape[0], 1, 256, 128) for b in batches)
        for i, batch in enumerate(batches):
            items = order[4 * i:4 * i + 4]
            want = resident.crop(drawn.song_v[items].tolist(), drawn.start_v[items].tolist(), with_phase=True)
            for name, g, w in zip(("mix", "voc", "mix_phase", "voc_phase"), batch, want):
                assert torch.equal(g, w), (rank, i, name)
            seen += len(items)
        two = list(resident.augmented_batches(4, rank, 2, epoch, with_phase=False, aug=aug))
        assert all(len(b) == 2 for b in two) and torch.equal(two[0][0], batches[0][0]) and torch.equal(two[1][1], batches[1][1])
    assert seen == len(resident)
    with pytest.raises(ValueError, match="other than 'none'"):
        next(resident.augmented_batches(4, aug=au.Augment()))


def test_augmented_batches_remix_against_the_definition(resident, report):
    aug = au.Augment("remix", (0.25, 1.25), 0.75, seed=9)
    epoch = 5
    drawn = au.draw_epoch(len(resident), resident.frames_host, 128, epoch, 9, (0.25, 1.25), 0.75)
    assert (drawn.song_a >= 0).any() and (drawn.song_a < 0).any()
    M, V, pm, pv = host_songs(resident)
    worst = [0.0, 0.0]
    for rank in range(2):
        order = svs_train.epoch_order(len(resident), True, rank, 2, epoch)
        got = [torch.cat(t).cpu().numpy() for t in zip(*resident.augmented_batches(4, rank, 2, epoch, with_phase=True, aug=aug))]
        ref = au.remix_reference(M, V, pm, pv, *(np.asarray(a)[order] for a in drawn), 128)
        assert all(np.isfinite(g).all() for g in got)
        r = ratios(got, ref)
        worst = [max(w, x) for w, x in zip(worst, r)]
        assert np.array_equal(got[1], ref.voc.astype(np.float32)) and np.array_equal(got[3], ref.voc_phase.astype(np.float32))
        gain_items = np.asarray(drawn.song_a)[order] < 0
        assert np.array_equal(got[0][gain_items], ref.mix.astype(np.float32)[gain_items])     # gain items: one multiply, exact
        assert np.array_equal(got[2][gain_items], ref.mix_phase.astype(np.float32)[gain_items])
    print(f"augmented_batches remix: worst ratios {worst[0]:.3f} {worst[1]:.3f}")
    ok = report("augmented_batches remix: |mix - ref| over 16 * 2^-23 * S", worst[0], 1.0)
    ok = report("augmented_batches remix: |mix cis(mix_phase) - z| over its bound", worst[1], 1.0) and ok
    assert ok, worst


def test_one_training_step_on_an_augmented_batch(resident):
    """The full objective (L1 + MR-STFT) at win 512 / hop 384 on a remixed batch: finite losses, parameters that moved."""
    model = UNet().to(DEV).train()
    before = model.state_dict()["conv1.0.weight"].detach().clone()
    aug = au.Augment("remix", (0.25, 1.25), 1.0, seed=1)
    mix, voc, mph, vph = next(resident.augmented_batches(4, 0, 1, 0, with_phase=True, aug=aug))
    l1 = model.train_step(mix, voc, loss_scale=ALPHA_L1, mix_phase=mph, voc_phase=vph, alpha_mr=ALPHA_MR, hop=384)
    l1, mr = float(l1), float(model.last_mr_loss)
    assert np.isfinite(l1) and l1 > 0 and np.isfinite(mr) and mr > 0, (l1, mr)
    after = model.state_dict()["conv1.0.weight"]
    assert torch.isfinite(after).all() and (after - before).abs().max().item() > 0


def test_train_cli_with_and_without_augment(folder, tmp_path, monkeypatch, capsys):
    """train.py --augment remix for one epoch (full objective, win 512) prints its settings beside the objective and feeds every step
    from augmented_batches; the default run reaches none of the new code (the augmentation's functions are made to raise) and both
    write checkpoints with the same keys."""
    monkeypatch.chdir(tmp_path)
    calls = {"augmented": 0, "plain": 0}
    real = {"augmented": svs_train.ResidentSpectrograms.augmented_batches, "plain": svs_train.ResidentSpectrograms.batches}

    def counted(kind):
        def method(self, *args, **kw):
            calls[kind] += 1
            return real[kind](self, *args, **kw)
        return method
    monkeypatch.setattr(svs_train.ResidentSpectrograms, "augmented_batches", counted("augmented"))
    monkeypatch.setattr(svs_train.ResidentSpectrograms, "batches", counted("plain"))
    common = ["--train_folder", str(folder), "--valid_folder", str(tmp_path / "no_valid"), "--batch_size", "32", "--epoch", "1",
              "--load_path", "none.pth", "--win_size", "512", "--hop_size", "384"]
    svs_train.main(common + ["--label", "aug", "--augment", "remix", "--augment_seed", "3", "--remix_prob", "0.75"])
    lines = capsys.readouterr().out.splitlines()
    i = [k for k, l in enumerate(lines) if l.startswith("Objective:")]
    assert len(i) == 1 and "MR-STFT" in lines[i[0]] and lines[i[0] + 1].startswith("Augmentation: remix"), lines
    assert "0.75" in lines[i[0] + 1] and "seed 3" in lines[i[0] + 1]
    assert calls == {"augmented": 1, "plain": 0}
    value = float(open(tmp_path / "LOG" / "log_aug.txt").read().split()[0])
    assert np.isfinite(value) and value > 0

    def forbidden(*args, **kw):
        raise AssertionError("--augment none reached the augmentation")
    for name in ("draw_epoch", "upload_table", "crop_remix", "check_settings", "Augment"):
        monkeypatch.setattr(au, name, forbidden)
    svs_train.main(common + ["--label", "plain"])
    out = capsys.readouterr().out
    assert "Augmentation" not in out and calls == {"augmented": 1, "plain": 1}
    a = torch.load(tmp_path / "CKPT" / "svs_aug.pth", map_location="cpu")
    p = torch.load(tmp_path / "CKPT" / "svs_plain.pth", map_location="cpu")
    assert set(a) == set(p) and a["epoch"] == p["epoch"] == 1
