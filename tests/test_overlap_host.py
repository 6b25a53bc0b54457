"""Overlapped tiles with cross-faded masks, the host half (no GPU): the three entry points are declared and bound, svs_overlap_count's
arithmetic, every argument rule of include/svs_hip.h refused with its own message before any launch (all device pointers are NULL,
so a call that got as far as a launch would come back with another code and message), the float64 definition's own properties
(overlap.blend_reference), and the command lines' refusal of a bad --tile_hop before a checkpoint is read."""
import numpy as np
import pytest

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import overlap as ov

NAMES = ("svs_overlap_count", "svs_overlap_tiles", "svs_overlap_blend")


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def err(lib):
    return lib.svs_last_error_string().decode()


def test_symbols_are_declared_and_bound(lib):
    syms = _lib.header_symbols()
    for name in NAMES:
        assert name in syms and name in _lib._SIGS and hasattr(lib, name), name
    assert lib.svs_version() == 1
    header = open(_lib.HEADER_PATH).read()
    assert header.count("inference.py:72-120") >= 3               # each of the three cites the tiling it is an option beside


@pytest.mark.parametrize("args,want", [((1, 128, 64), 1), ((3, 128, 64), 5), ((3, 128, 32), 9), ((2, 16, 16), 2)])
def test_overlap_count(lib, args, want):
    assert lib.svs_overlap_count(*args) == want
    assert ov.overlap_count(*args) == want


@pytest.mark.parametrize("args,msg", [((0, 128, 64), "positive"), ((3, 0, 64), "positive"), ((3, 128, 0), "positive"),
                                      ((3, 128, -64), "positive"), ((3, 128, 48), "divide")])
def test_overlap_count_refuses(lib, args, msg):
    assert lib.svs_overlap_count(*args) == -1
    assert msg in err(lib) and "svs_overlap_count" in err(lib)
    with pytest.raises(_lib.SvsError, match=msg):
        ov.overlap_count(*args)


# (channels, n_tiles, rows, seg, tile_hop, stride) -> the words of the rule's message; stride None = the minimum
RULES = [
    ((0, 3, 5, 16, 8, None), "all sizes must be positive"),
    ((2, 0, 5, 16, 8, None), "all sizes must be positive"),
    ((2, 3, 0, 16, 8, None), "all sizes must be positive"),
    ((2, 3, 5, 0, 8, None), "all sizes must be positive"),
    ((2, 3, 5, 16, 0, None), "all sizes must be positive"),
    ((2, 3, 5, -16, -8, None), "all sizes must be positive"),
    ((2, 3, 5, 18, 6, None), "seg must be a multiple of 4"),
    ((2, 3, 5, 12, 6, None), "tile_hop must be a multiple of 4"),
    ((2, 3, 5, 128, 48, None), "tile_hop must divide seg"),
    ((2, 3, 5, 16, 32, None), "tile_hop must divide seg"),
    ((2, 3, 5, 128, 8, None), "seg / tile_hop must be at most 8"),
    ((2, 3, 5, 64, 4, None), "seg / tile_hop must be at most 8"),
    ((2, 3, 5, 16, 8, 3 * 5 * 16 - 4), "must be at least n_tiles * rows * seg"),
    ((2, 3, 5, 16, 8, 3 * 5 * 16 + 2), "must be a multiple of 4 floats"),
    ((2, 3, 5, 16, 8, None), "null pointer"),
    ((2, 3, 5, 16, 16, None), "null pointer"),                     # tile_hop == seg is legal: only the pointers are wrong
]


@pytest.mark.parametrize("geom,msg", RULES)
def test_overlap_tiles_refuses_before_any_launch(lib, geom, msg):
    C, n_tiles, rows, seg, hop, stride = geom
    stride = n_tiles * rows * seg if stride is None else stride
    assert lib.svs_overlap_tiles(None, stride, C, n_tiles, rows, seg, hop, None, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_overlap_tiles:")


@pytest.mark.parametrize("geom,msg", RULES)
def test_overlap_blend_refuses_before_any_launch(lib, geom, msg):
    C, n_tiles, rows, seg, hop, stride = geom
    stride = n_tiles * rows * seg if stride is None else stride
    assert lib.svs_overlap_blend(None, C, n_tiles, rows, seg, hop, None, 0, 0, None, stride, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_overlap_blend:")
    if "out_chan_stride" in err(lib):                             # the stride rules hold for mix's stride as well, when mix is given
        good = n_tiles * rows * seg
        assert lib.svs_overlap_blend(None, C, n_tiles, rows, seg, hop, 16, stride, 0, None, good, None) == -1
        assert msg in err(lib) and "mix_chan_stride" in err(lib)


def test_misaligned_pointers_are_refused(lib):
    """Pointers that are no multiple of 16 bytes (never dereferenced: the check comes first)."""
    assert lib.svs_overlap_tiles(16, 240, 2, 3, 5, 16, 8, 24, None) == -1 and "16-byte aligned" in err(lib)
    assert lib.svs_overlap_tiles(8, 240, 2, 3, 5, 16, 8, 32, None) == -1 and "16-byte aligned" in err(lib)
    assert lib.svs_overlap_blend(16, 2, 3, 5, 16, 8, None, 0, 0, 40, 240, None) == -1 and "16-byte aligned" in err(lib)
    assert lib.svs_overlap_blend(16, 2, 3, 5, 16, 8, 4, 240, 0, 32, 240, None) == -1 and "16-byte aligned" in err(lib)


# ---- the float64 definition ------------------------------------------------------------------------------------------------

def rand_masks(n, rows, seg, seed=0):
    return np.random.default_rng(seed).random((n, rows, seg))


@pytest.mark.parametrize("seg", [16, 128])
@pytest.mark.parametrize("n_tiles", [2, 3])
def test_half_overlap_interior_weights_sum_to_one(seg, n_tiles):
    den = ov.reference_weights(seg, n_tiles, seg // 2)
    interior = den[seg // 2: n_tiles * seg - seg // 2]
    assert interior.size == (n_tiles - 1) * seg and np.abs(interior - 1.0).max() <= 1e-15
    w = ov.reference_window(seg)
    assert np.array_equal(w, np.sin(np.pi * (np.arange(seg) + 0.5) / seg) ** 2) and w.min() > 0      # strictly positive
    assert np.array_equal(den[:seg // 2], w[:seg // 2])                        # one tile at the song's start


@pytest.mark.parametrize("seg,hop", [(16, 8), (16, 4), (128, 64), (128, 32), (128, 16)])
def test_reference_constant_masks_give_the_constant(seg, hop):
    n_tiles = 3
    n_ov = (n_tiles - 1) * (seg // hop) + 1
    for value in (0.0, 0.375, 1.0):
        got = ov.blend_reference(np.full((2 * n_ov, 3, seg), value), n_tiles, hop)
        # at most 8 products and 7 additions in the numerator, 7 additions in the denominator, one division: 2e-15 covers 16 roundings
        assert got.shape == (2, 3, n_tiles * seg) and np.abs(got - value).max() <= 2e-15


@pytest.mark.parametrize("seg,hop", [(16, 8), (16, 4), (16, 2), (128, 32)])
def test_reference_one_tile_frames_return_the_input(seg, hop):
    n_tiles = 3
    n_ov = (n_tiles - 1) * (seg // hop) + 1
    m = rand_masks(2 * n_ov, 5, seg)
    got = ov.blend_reference(m, n_tiles, hop)
    for c in range(2):
        assert np.array_equal(got[c, :, :hop], m[c * n_ov, :, :hop])                       # the first hop: tile 0 alone
        assert np.array_equal(got[c, :, -hop:], m[c * n_ov + n_ov - 1, :, -hop:])          # the last hop: the last tile alone
        assert not np.array_equal(got[c, :, hop:2 * hop], m[c * n_ov, :, hop:2 * hop])     # two tiles from there on
    one = rand_masks(2, 5, seg, seed=1)                                                    # n_tiles = 1: one tile covers everything
    assert np.array_equal(ov.blend_reference(one, 1, hop), one)


@pytest.mark.parametrize("seg", [16, 128])
def test_reference_disjoint_hop_is_the_identity(seg):
    m = rand_masks(2 * 3, 5, seg, seed=2)
    got = ov.blend_reference(m, 3, seg)
    want = m.reshape(2, 3, 5, seg).transpose(0, 2, 1, 3).reshape(2, 5, 3 * seg)
    assert np.array_equal(got, want)
    assert np.array_equal(ov.blend_reference(m[:, None], 3, seg), want)                    # the network's (n, 1, rows, seg) form


def test_reference_is_the_weighted_mean():
    """One frame by hand: seg 16, tile_hop 4, two disjoint tiles = overlapped tiles 0..4; frame 21 lies in tiles 2, 3, 4 at offsets
    13, 9, 5 (a tile 5 would cover it too, and does not exist)."""
    seg, hop, n_tiles = 16, 4, 2
    n_ov = 5
    m = rand_masks(n_ov, 1, seg, seed=3)
    w = np.sin(np.pi * (np.arange(seg) + 0.5) / seg) ** 2
    got = ov.blend_reference(m, n_tiles, hop)[0, 0, 21]
    num = sum(w[21 - 4 * j] * m[j, 0, 21 - 4 * j] for j in (2, 3, 4))
    den = sum(w[21 - 4 * j] for j in (2, 3, 4))
    assert abs(got - num / den) <= 1e-15


# ---- command lines ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value,msg", [("48", "divides the tile length 128"), ("0", "must be positive"), ("8", "at least 16"),
                                       ("256", "divides the tile length 128")])
@pytest.mark.parametrize("module", ["separate", "inference"])
def test_cli_refuses_bad_tile_hop_before_the_checkpoint(module, value, msg, tmp_path, capsys):
    import importlib
    mod = importlib.import_module(f"svs_unet_pytorch_amd.{module}")
    missing = str(tmp_path / "no_such_checkpoint.pth")             # loading it would fail with another message
    args = ["--model_path", missing, "--tar", str(tmp_path / "out"), "--tile_hop", value]
    args += ["--src", str(tmp_path / "in.wav")] if module == "separate" else ["--mixture_folder", str(tmp_path)]
    with pytest.raises(SystemExit) as e:
        mod.main(args)
    assert e.value.code not in (0, None)
    text = capsys.readouterr().err
    assert "--tile_hop" in text and msg in text
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("entry", ["module", "dropin"])
def test_cli_process_exits_nonzero_on_bad_tile_hop(entry, tmp_path):
    """The same refusal through the entries a user types: `python -m svs_unet_pytorch_amd.separate` and the drop-in
    `python dropin/inference.py`, each as a process of its own: non-zero exit status, the rule on stderr, nothing written."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    missing = str(tmp_path / "no_such_checkpoint.pth")
    if entry == "module":
        cmd = [sys.executable, "-m", "svs_unet_pytorch_amd.separate", "--src", str(tmp_path / "in.wav")]
    else:
        cmd = [sys.executable, os.path.join(root, "dropin", "inference.py"), "--mixture_folder", str(tmp_path)]
    cmd += ["--model_path", missing, "--tar", str(tmp_path / "out"), "--tile_hop", "48"]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode not in (0, None) and r.returncode > 0, (r.returncode, r.stderr[-500:])
    assert "--tile_hop" in r.stderr and "divides the tile length 128" in r.stderr, r.stderr[-500:]
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("module", ["separate", "inference"])
def test_cli_help_names_the_hops(module, capsys):
    import importlib
    mod = importlib.import_module(f"svs_unet_pytorch_amd.{module}")
    with pytest.raises(SystemExit) as e:
        mod.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--tile_hop" in text and "64" in text and "32" in text and "128" in text


def test_default_tile_hop_is_the_tile_length():
    """The functions that take a seg_len default to it (None), not to the constant 128: a caller with another seg_len who never
    names tile_hop keeps disjoint tiles.  separate_waveform and separate_to_wav cut INPUT_LEN-frame tiles only."""
    import inspect

    from svs_unet_pytorch_amd import inference, streaming
    from svs_unet_pytorch_amd.config import INPUT_LEN
    for fn in (inference.separate, streaming.separate_spectrogram_device):
        assert inspect.signature(fn).parameters["tile_hop"].default is None, fn.__name__
    for fn in (streaming.separate_waveform, streaming.separate_to_wav):
        assert inspect.signature(fn).parameters["tile_hop"].default == INPUT_LEN == 128, fn.__name__


def test_a_failing_forward_leaves_the_model_as_it_came():
    """The network stage restores the caller's mode and precision in `finally`: a model in training mode at fp32 whose forward raises
    is in training mode at fp32 afterwards, through separate_spectrogram_device and through its host wrapper inference.separate.
    CPU tensors and disjoint tiles: the forward raises before any library call."""
    import torch

    from svs_unet_pytorch_amd import inference, streaming

    class Stub:
        def __init__(self):
            self.training, self.eval_precision, self.calls = True, "fp32", 0
            self._flat = torch.zeros(1)

        def eval(self):
            return self.train(False)

        def train(self, mode=True):
            self.training = mode
            return self

        def __call__(self, tiles):
            self.calls += 1
            assert not self.training and tiles.shape == (2, 1, 256, 128)
            raise RuntimeError("the forward failed")

    mag = torch.rand(257, 130)
    for call in (lambda m: streaming.separate_spectrogram_device(m, mag), lambda m: inference.separate(m, mag.numpy())):
        stub = Stub()
        with pytest.raises(RuntimeError, match="the forward failed"):
            call(stub)
        assert stub.calls == 1 and stub.training is True and stub.eval_precision == "fp32"


def test_python_check_names_the_rule():
    for hop in (128, 64, 32, 16):
        assert ov.check_tile_hop(hop, 128) == hop
    for hop, msg in ((0, "positive"), (-64, "positive"), (48, "divides"), (6, "multiple of 4"), (8, "at least 16"), (256, "divides")):
        with pytest.raises(ValueError, match=msg):
            ov.check_tile_hop(hop, 128)
