"""CPU suite (-m "not gpu"): host logic that needs no GPU -- the C-ABI library loads and exports every
symbol the header declares, the flat parameter layout agrees between C++ and Python, the model keeps the
reference's checkpoint surface, the synthetic generator is stable, tile bookkeeping, CLI surfaces."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from svs_unet_pytorch_amd import _lib, synth
from svs_unet_pytorch_amd.inference import segment_plan
from svs_unet_pytorch_amd.model import DEC_IO, ENC_CHANNELS, FusedAdam, UNet
from svs_unet_pytorch_amd.parallel import shard_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from svs_unet_pytorch_amd import build
    build.build_lib(verbose=False)
    return _lib.lib()


def test_library_exports_every_header_symbol(lib):
    syms = _lib.header_symbols()
    assert len(syms) >= 40
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert set(syms) == set(_lib._SIGS), set(syms) ^ set(_lib._SIGS)
    assert lib.svs_version() == 1
    assert isinstance(lib.svs_last_error_string(), bytes)


def test_header_is_plain_c(tmp_path):
    """include/svs_hip.h must compile as C (extern "C", plain pointers and sizes, no torch types)."""
    src = tmp_path / "t.c"
    src.write_text('#include "svs_hip.h"\nint (*probe)(void) = svs_version;\nint main(void){return probe != svs_version;}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_flat_layout_matches_state_dict(lib):
    model = UNet()
    names = [n for n, _ in model.named_parameters()]
    spec = [(k, s) for k, s, kind in synth.state_dict_spec() if kind in ("w", "wt", "b", "gamma", "beta")]
    assert names == [k for k, _ in spec]
    assert len(names) == 46
    for i, (p, (off, n)) in enumerate(zip(model._param_list, model._param_spans)):
        assert lib.svs_unet_param_offset(i) == off, names[i]
        assert p.data_ptr() == model._flat.data_ptr() + 4 * off
        assert p.grad.data_ptr() == model._gflat.data_ptr() + 4 * off
        assert off % 4 == 0                     # 16-byte alignment of every tensor inside the flat buffer
    assert lib.svs_unet_param_offset(46) == model._n_params == 9823313
    off = 0
    for i, bn in enumerate(model._bn_list):
        assert lib.svs_unet_buffer_offset(i, 0) == off
        assert lib.svs_unet_buffer_offset(i, 1) == off + bn.num_features
        assert bn.running_mean.data_ptr() == model._bn_flat.data_ptr() + 4 * off
        off += 2 * bn.num_features
    assert lib.svs_unet_buffer_offset(11, 0) == off == 3008
    assert lib.svs_unet_param_offset(47) == -1


def test_workspace_queries_are_consistent(lib):
    assert lib.svs_unet_eval_workspace_bytes(16, 512, 128) > 16 * 4 * (2 * 16 * 256 * 64)
    a, b = lib.svs_unet_train_workspace_bytes(4, 512, 128), lib.svs_unet_train_workspace_bytes(8, 512, 128)
    assert 0 < a < b
    for name in ("cat1", "cat5", "c6", "raw_e1", "raw_d5", "dcat3", "dc6", "d_logit", "mean0", "invstd10"):
        assert lib.svs_unet_ws_offset(name.encode(), 4, 512, 128, 1) >= 0, name
    assert lib.svs_unet_ws_offset(b"nope", 4, 512, 128, 1) == -1
    assert lib.svs_unet_ws_offset(b"cat2", 2, 513, 100, 0) >= 0
    assert lib.svs_stft_frames(97536, 768) == 128 and lib.svs_stft_frames(100000, 768) == 131 and lib.svs_stft_frames(81920, 768) == 107


@pytest.mark.parametrize("training", [0, 1, 2])
def test_named_workspace_buffers_are_aligned_disjoint_and_inside(lib, training):
    """What holds for svs_unet_ws_offset whatever the sizes are, at a shape that is odd at every level: each named
    buffer (fp32, shapes of csrc/net.hip's header comment; training = 2: the bf16 eval workspace, the same shapes in
    2-byte elements) starts 256-byte aligned, overlaps no other and ends inside the workspace; names outside the table
    are unknown."""
    B, H, W = 2, 513, 100
    hw = [(H, W)]
    for _ in range(6):
        hw.append(((hw[-1][0] + 1) // 2, (hw[-1][1] + 1) // 2))
    P = [B * h * w for h, w in hw]
    bn = list(ENC_CHANNELS[1:]) + [n for _, n in DEC_IO[:5]]                   # channels of the 11 BatchNorm layers
    numel = {f"cat{k}": P[k] * 2 * ENC_CHANNELS[k] for k in range(1, 6)}
    numel["c6"] = P[6] * ENC_CHANNELS[6]
    esize = 2 if training == 2 else 4
    if training == 1:
        numel.update({f"raw_e{k}": P[k] * ENC_CHANNELS[k] for k in range(1, 7)})
        numel.update({f"raw_d{j}": P[6 - j] * DEC_IO[j - 1][1] for j in range(1, 6)})      # deconv j writes level 6 - j
        numel.update({"d" + name: n for name, n in list(numel.items()) if name.startswith("c")})   # dcat1..5, dc6
        numel.update({"d_logit": P[0], "mask": P[0]})
        numel.update({f"mean{i}": c for i, c in enumerate(bn)})
        numel.update({f"invstd{i}": c for i, c in enumerate(bn)})
    total = (lib.svs_unet_eval_workspace_bytes, lib.svs_unet_train_workspace_bytes, lib.svs_unet_eval_bf16_workspace_bytes)[training](B, H, W)
    spans = []
    for name, n in numel.items():
        off = lib.svs_unet_ws_offset(name.encode(), B, H, W, training)
        assert off >= 0 and off % 256 == 0, (name, off)
        assert off + esize * n <= total, (name, off, n, total)
        spans.append((off, off + esize * n, name))
    spans.sort()
    for (_, end, a), (start, _, b) in zip(spans, spans[1:]):
        assert end <= start, (a, b)
    for name in ("nope", "cat0", "cat6", "raw_e0", "raw_e7", "raw_d6", "mean11", "invstd11", "dcat6", "dc", "cat", ""):
        assert lib.svs_unet_ws_offset(name.encode(), B, H, W, training) == -1, name
    for k in range(1, 6):          # "dcatK" is a name of its own (training) or unknown (eval), never read as "catK"
        assert lib.svs_unet_ws_offset(b"dcat%d" % k, B, H, W, training) != lib.svs_unet_ws_offset(b"cat%d" % k, B, H, W, training)
    if training != 1:
        assert lib.svs_unet_ws_offset(b"dcat3", B, H, W, training) == lib.svs_unet_ws_offset(b"raw_e1", B, H, W, training) == -1


@pytest.mark.parametrize("B,W,hop", [(5, 32, 100), (20, 32, 128), (5, 4, 1024), (3, 128, 768)])
def test_named_mr_workspace_buffers_are_aligned_disjoint_and_inside(lib, B, W, hop):
    """svs_unet_mr_ws_offset: the two waveforms and d_wav of svs_unet_train_fwd_loss_mr's MR workspace, B rows of hop (W - 1)
    floats each, 256-byte aligned, in the order the call fills them, inside svs_unet_train_mr_workspace_bytes; other names and
    sizes the workspace query refuses are unknown."""
    total = lib.svs_unet_train_mr_workspace_bytes(B, W, hop)
    nbytes = 4 * B * hop * (W - 1)
    offs = [lib.svs_unet_mr_ws_offset(name, B, W, hop) for name in (b"wav_pred", b"wav_tgt", b"d_wav")]
    assert offs[0] == 0 and all(o % 256 == 0 for o in offs)
    assert offs[0] + nbytes <= offs[1] and offs[1] + nbytes <= offs[2] and offs[2] + nbytes < total
    for name in (b"nope", b"", b"d_wav0", b"wav", b"wav_pred ", b"mask", b"d_logit"):
        assert lib.svs_unet_mr_ws_offset(name, B, W, hop) == -1, name
    assert lib.svs_unet_mr_ws_offset(None, B, W, hop) == -1
    for bad in ((0, W, hop), (B, 1, hop), (B, W, 0)):
        assert lib.svs_unet_mr_ws_offset(b"d_wav", *bad) == -1 and lib.svs_unet_train_mr_workspace_bytes(*bad) == 0


def test_invalid_arguments_are_reported_without_touching_the_gpu(lib):
    rc = lib.svs_enc_block_fwd(None, 16, 1, 8, 8, 16, None, None, None, None, 0.0, None, 32, 32, 0, None, 0, None)
    assert rc == -1 and b"null pointer" in lib.svs_last_error_string()
    rc = lib.svs_stft_fwd(ctypes.c_void_p(16), 1000, 512, 128, ctypes.c_void_p(16), None, None)
    assert rc == -1 and b"n_fft=1024" in lib.svs_last_error_string()
    rc = lib.svs_adam_step(None, None, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None)
    assert rc == -1


def test_model_checkpoint_surface():
    model = UNet()
    sd = model.state_dict()
    spec = synth.state_dict_spec()
    assert list(sd.keys()) == [k for k, _, _ in spec] and len(sd) == 79
    for k, shape, _ in spec:
        assert tuple(sd[k].shape) == tuple(shape), k
    assert isinstance(model.optim, FusedAdam) and model.optim.param_groups[0]["lr"] == 1e-3   # model.py:116
    assert isinstance(model.crit, torch.nn.L1Loss)
    assert model.loss_list_total == [] and model.getLoss() == {}
    model.loss_list_total.append(0.1234567)
    assert model.getLoss() == {"loss_list_total": 0.123457}
    cf = {k: torch.from_numpy(np.array(v)) for k, v in synth.closed_form_state().items()}
    model.load_state_dict(cf, strict=True)
    assert torch.equal(model.conv3[0].weight.detach(), cf["conv3.0.weight"])
    assert int(model.deconv2_BAD[0].num_batches_tracked) == 7
    assert float(model._flat[:400].sum()) == pytest.approx(float(cf["conv1.0.weight"].sum()), rel=1e-6)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        model(torch.zeros(1, 1, 512, 128))                                                # no CPU fallback


def test_save_load_roundtrip_and_optimizer_state_format(tmp_path):
    model = UNet()
    model.loss_list_total = [1.0, 0.5]
    model.optim._ensure_state()
    model.optim._m.uniform_()
    model.optim._v.uniform_()
    model.optim._step = 5
    path = str(tmp_path / "svs_x.pth")
    model.save(path)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) >= {"model_state_dict", "optim", "loss_list_total", "loss_list_vocal", "loss_list_accomp"}   # model.py:143-152
    st = ck["optim"]["state"]
    assert len(st) == 46 and set(st[0]) == {"step", "exp_avg", "exp_avg_sq"} and float(st[0]["step"]) == 5.0
    assert st[0]["exp_avg"].shape == (16, 1, 5, 5)
    # the same file loads into torch.optim.Adam over an identically shaped parameter list (reference model.py:116)
    ref_params = [torch.nn.Parameter(torch.zeros_like(p)) for p in model.parameters()]
    torch.optim.Adam(ref_params, lr=1e-3).load_state_dict(ck["optim"])
    m2 = UNet()
    m2.load(path)
    assert m2.loss_list_total == [1.0, 0.5] and m2.optim._step == 5
    assert torch.equal(m2.optim._m, model.optim._m) and torch.equal(m2._flat, model._flat)
    m2.load(str(tmp_path / "missing.pth"))          # prints, does not raise (model.py:137-138)


def test_synth_is_stable():
    # golden numbers of the counter-based generator: the GPU kernel (svs_fill_uniform) is pinned to the same
    assert synth.u32(0, np.array([0, 1, 2 ** 32], np.uint64)).tolist() == synth.u32(0, np.array([0, 1, 2 ** 32], np.uint64)).tolist()
    u = synth.uniform(7, 5, (5 << 32) + 11)
    assert u.dtype == np.float32 and np.all((u >= 0) & (u < 1))
    a, b = synth.tiles(2, 8, 4, first_tile=3)
    assert a.shape == (2, 1, 8, 4) and np.all(b <= a)
    a2, _ = synth.tiles(1, 8, 4, first_tile=4)
    assert np.array_equal(a[1], a2[0])              # tile index, not batch position, selects the stream
    masks = synth.dropout_masks(4, seed=1)
    assert [m.shape for m in masks] == [(4, c) for _, c in DEC_IO[:5]]
    assert all(set(np.unique(m)) <= {0.0, 2.0} for m in masks)
    assert ENC_CHANNELS == (1, 16, 32, 64, 128, 256, 512)


def test_tile_bookkeeping_is_exact():
    assert segment_plan(1) == [(0, 1, 127)]
    assert segment_plan(127) == [(0, 127, 1)]
    assert segment_plan(128) == [(0, 128, 0)]           # T % 128 == 0: the empty last segment is skipped (inference.py:88)
    assert segment_plan(129) == [(0, 128, 0), (128, 129, 127)]
    assert segment_plan(256) == [(0, 128, 0), (128, 256, 0)]
    assert segment_plan(300) == [(0, 128, 0), (128, 256, 0), (256, 300, 84)]
    for T in (0, 1, 5, 127, 128, 129, 1000, 1024):
        plan = segment_plan(T)
        assert sum(e - s for s, e, _ in plan) == T and all(e - s + p == 128 for s, e, p in plan)


def test_shard_range_partitions():
    for n in (0, 1, 7, 64, 513):
        for world in (1, 2, 3, 8):
            parts = [shard_range(n, r, world) for r in range(world)]
            assert parts[0][0] == 0 and parts[-1][1] == n
            assert all(parts[i][1] == parts[i + 1][0] for i in range(world - 1))
            sizes = [e - b for b, e in parts]
            assert max(sizes) - min(sizes) <= 1


@pytest.mark.parametrize("mod,flags", [("inference", ["--model_path", "--tar", "--mixture_folder", "--vocal_solo"]),
                                       ("train", ["--train_folder", "--load_path", "--label", "--epoch", "--batch_size", "--valid_folder", "--val_interval"]),
                                       ("data", ["--src", "--tar", "--phase", "--win_size", "--hop_size", "--sr", "--direction"])])
def test_cli_flags_match_reference(mod, flags):
    """inference.py:30-33, train.py:158-165, data.py:21-27."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "dropin", mod + ".py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for f in flags:
        assert f in r.stdout, f


def test_config_constants():
    from svs_unet_pytorch_amd import config
    assert (config.WINDOW_SIZE, config.HOP_SIZE, config.SAMPLE_RATE, config.INPUT_LEN, config.SAMPLES_PER_SONG) == (1024, 768, 8192, 128, 64)
    assert [config.num2str(n) for n in (0, 7, 42, 999, 1000, 12345)] == ["0000", "0007", "0042", "0999", "1000", "12345"]


def test_epoch_order_covers_all_items():
    """DataLoader / DistributedSampler semantics of the resident training set (train.py:178-185 of the reference)."""
    from svs_unet_pytorch_amd.train import epoch_order
    n = 37
    assert sorted(epoch_order(n, True)) == list(range(n))
    assert epoch_order(n, False) == list(range(n))
    for world in (2, 3, 8):
        parts = [epoch_order(n, True, r, world, epoch=5) for r in range(world)]
        assert len({len(p) for p in parts}) == 1 and len(parts[0]) == (n + world - 1) // world
        assert set(sum(parts, [])) == set(range(n))                       # every item, some twice (wrap-around padding)
        assert parts == [epoch_order(n, True, r, world, epoch=5) for r in range(world)]      # same permutation on every call
        assert parts != [epoch_order(n, True, r, world, epoch=6) for r in range(world)]


def test_crop_oracle_rule():
    from oracle.tiling_oracle import crop_item
    rng = np.random.default_rng(3)
    for T, start in ((300, 0), (300, 172), (128, 0), (50, 0), (129, 1)):
        mix, voc = rng.random((513, T), dtype=np.float32), rng.random((513, T), dtype=np.float32)
        m, v = crop_item(mix, voc, start)
        assert m.shape == v.shape == (1, 512, 128) and m.dtype == np.float32
        w = min(T, 128)
        assert np.array_equal(m[0, :, :w], mix[1:, start:start + w]) and np.array_equal(v[0, :, :w], voc[1:, start:start + w])
        assert not m[0, :, w:].any() and not v[0, :, w:].any()



def test_bss_eval_defining_properties(tmp_path):
    """evaluate.py:26-84 on the restated BSS-eval (mir_eval itself is not installable: parity unpinned).  What the
    metric is DEFINED to do: (1) a (short-)filtered copy of the reference is all target (SDR / SIR / SAR > 45 dB: only the
    truncated last two samples of the filter's tail are not);
    (2) reference + a * interferer -> SIR = -20 log10(a), SAR large; (3) reference + uncorrelated noise -> SDR = SAR = SNR,
    SIR large; (4) the permutation is resolved by SIR; (5) the CLI writes the reference's CSV."""
    from svs_unet_pytorch_amd import evaluate as ev
    rng = np.random.default_rng(3)
    n = 16000
    s1, s2 = rng.standard_normal(n), rng.standard_normal(n)
    refs = np.stack([s1, s2])
    filt = np.convolve(s1, [0.5, 0.3, -0.2])[:n]
    sdr, sir, sar, perm = ev.bss_eval_sources(refs, np.stack([filt, s2]))
    assert list(perm) == [0, 1] and sdr[0] > 45 and sir[0] > 45 and sar[0] > 45 and sdr[1] > 100
    a = 0.1
    sdr, sir, sar, _ = ev.bss_eval_sources(refs, np.stack([s1 + a * s2, s2 + a * s1]))
    assert abs(sir[0] - 20.0) < 0.5 and sar[0] > 60 and abs(sdr[0] - 20.0) < 0.5
    noise = rng.standard_normal(n) * 0.1
    sdr, sir, sar, _ = ev.bss_eval_sources(refs, np.stack([s1 + noise, s2]))
    assert abs(sdr[0] - 20.0) < 1.0 and abs(sar[0] - 20.0) < 1.0 and sir[0] > 30
    _, _, _, perm = ev.bss_eval_sources(refs, np.stack([s2 + 0.05 * s1, s1 + 0.05 * s2]))
    assert list(perm) == [1, 0]
    # CLI on wav files: mixture = vocal + accompaniment, estimate = vocal + 0.1 accompaniment
    from scipy.io import wavfile
    for d in ("est", "mix", "ref"):
        os.makedirs(tmp_path / d)
    voc, acc = (s1 * 0.1).astype(np.float32), (s2 * 0.1).astype(np.float32)
    wavfile.write(tmp_path / "mix" / "a.wav", 8192, voc + acc)
    wavfile.write(tmp_path / "ref" / "a.wav", 8192, voc)
    wavfile.write(tmp_path / "est" / "a.wav", 8192, voc + 0.1 * acc)
    res = ev.main(["--est", str(tmp_path / "est"), "--mix", str(tmp_path / "mix"), "--ref", str(tmp_path / "ref"),
                   "--out_csv", str(tmp_path / "r.csv")])
    assert len(res) == 1 and abs(res[0]["SIR"] - 20.0) < 0.5 and res[0]["NSDR"] > 15
    rows = open(tmp_path / "r.csv").read().splitlines()
    assert rows[0] == "track,SDR,SIR,SAR,NSDR" and rows[1].startswith("a,")


def test_library_has_no_packed_fp32_op_sel_forms():
    """gfx950: a packed-fp32 instruction whose op_sel takes the high half of a source for the low result returns garbage
    while a bf16 MFMA of another wave executes on the CU.  The
    built library must not contain that form anywhere (stft.hip / mrstft.hip are compiled without SLP vectorisation for
    this reason)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "svs_unet_pytorch_amd", "libsvs_hip.so")
    if not os.path.exists(lib):
        import pytest
        pytest.skip("library not built")
    spec = importlib.util.spec_from_file_location("check_isa", os.path.join(root, "tools", "check_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hits, n_inst, n_kernels = mod.scan(lib)
    assert n_kernels > 100 and n_inst > 100000                 # the scan really saw the device code
    assert not hits, hits[:5]


@pytest.mark.parametrize("switch", [None, ("CONV_SKIP", 2), ("CONV_SKIP", 0), ("CONV_WINDOW", 0), ("CONV_WINDOW", 2),
                                    ("CONV_WINDOW", 3), ("CONV_GWINDOW", 2), ("WGRAD_SKIP", 2), ("WGRAD_WINDOW", 2),
                                    ("MFMA_SPLIT", 1)])
def test_described_plans_name_built_kernels_and_fit_the_workspace(lib, tune, tmp_path, switch):
    """Every GEMM call of a train step and an eval forward over batch sizes and tile shapes: the kernel svs_describe_plan names
    (bench.py files its timings under that name) is a kernel of the built library, and the block's workspace query covers the
    K-split slabs of that plan."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_isa", os.path.join(ROOT, "tools", "check_isa.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    spec = importlib.util.spec_from_file_location("bench_calls", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    mangled = []
    for co in isa.device_code_objects(_lib.LIB_PATH, str(tmp_path)):
        syms = subprocess.run([f"{isa.LLVM}/llvm-objdump", "-t", co], capture_output=True, text=True, check=True).stdout
        mangled += [ln.split()[-1] for ln in syms.splitlines() if " F .text" in ln]
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.splitlines()
    kernels = {d.removeprefix("void ").split("(")[0] for d in demangled}
    assert "gather_window_kernel" in kernels and len(kernels) > 100
    if switch:
        tune(*switch)
    buf = ctypes.create_string_buffer(128)
    for H, W in ((512, 128), (513, 100), (512, 512)):
        for B in (1, 3, 16, 64, 128, 216, 512):
            for name, kind, (h, w, c, ho, wo, n), _ in bench.gemm_calls(B, "train", H, W):
                if kind == 2:
                    ks = lib.svs_describe_plan(2, B, h, w, c, 0, 0, n, buf, 128)
                    need, ws = ks * c * 25 * n * 4, lib.svs_block_bwd_weight_workspace_bytes(B, h, w, c, n)
                else:
                    ks = lib.svs_describe_plan(kind, B, h, w, c, ho, wo, n, buf, 128)
                    need = ks * B * ho * wo * n * 4 if ks > 1 else 0
                    ws = (lib.svs_enc_block_workspace_bytes(B, h, w, c, n) if kind == 0 else
                          lib.svs_dec_block_workspace_bytes(B, h, w, c, ho, wo, n))
                where = f"{name} B={B} {H}x{W} {switch}: {buf.value.decode()}"
                assert ks >= 1 and buf.value.decode() in kernels, where
                assert ws >= need, (where, ws, need)
                if name.endswith("fwd") and kind in (0, 1):         # the same call with the folded-BatchNorm epilogue (eval forward)
                    ks = lib.svs_describe_plan(kind + 5, B, h, w, c, ho, wo, n, buf, 128)
                    assert ks >= 1 and buf.value.decode() in kernels, (where, buf.value)
                    assert ws >= (ks * B * ho * wo * n * 4 if ks > 1 else 0), (where, buf.value, ks, ws)


# (layer, (H, W, C, Ho, Wo, N)) of the ten planned forward calls on a 512 x 128 tile
FWD_CALLS = (("conv2", (256, 64, 16, 128, 32, 32)), ("conv3", (128, 32, 32, 64, 16, 64)), ("conv4", (64, 16, 64, 32, 8, 128)),
             ("conv5", (32, 8, 128, 16, 4, 256)), ("conv6", (16, 4, 256, 8, 2, 512)), ("deconv1", (8, 2, 512, 16, 4, 256)),
             ("deconv2", (16, 4, 512, 32, 8, 128)), ("deconv3", (32, 8, 256, 64, 16, 64)), ("deconv4", (64, 16, 128, 128, 32, 32)),
             ("deconv5", (128, 32, 64, 256, 64, 16)))
# batch -> "tile/K-split" (or the window kernel's arguments) per call of FWD_CALLS: the training-kind call (kinds 0 / 1) ...
TRAIN_PLANS = {16: "gather_window 128x64/3 64x128s/6 64x64s/12 64x64s/24 64x64s/16 64x128s/16 64x64s/4 window<128,64,1,2> window<64,64,1,1>",
               64: "gather_window 128x64/1 64x128u/3 64x128u/7 64x64u/7 64x64u/7 64x128u/4 64x64u/1 window<128,64,2,2> window<64,64,1,1>"}
# ... and the call with the folded-BatchNorm epilogue (kinds 5 / 6): the 64x64 tile for N = 64 up to 16384 rows (conv3 at batch 16), no
# 64x128 tile on the narrow N = 128 layers below 8192 / 2048 rows (conv4, deconv2 at batch 16), no 64x128 conv5 tile (batch 64), and
# a K-split target of 512 blocks instead of 768 (conv3 .. conv6 at batch 16, conv4 at batch 64)
EVAL_PLANS = {16: "gather_window 64x64/2 64x64s/4 64x64s/8 64x64s/16 64x64s/16 64x64s/8 64x64s/4 window<128,64,1,2> window<64,64,1,1>",
              64: "gather_window 128x64/1 64x128u/2 64x64u/2 64x64u/7 64x64u/7 64x128u/4 64x64u/1 window<128,64,2,2> window<64,64,1,1>"}


def test_describe_plan_eval_kinds(lib, tune):
    """svs_describe_plan kinds 5 / 6 (host arithmetic only): the gather / parity call with the folded-BatchNorm epilogue, named in
    the format of kinds 0 / 1.  The plans of the ten forward calls at batch 16 and 64 are written down for both kinds of call --
    the training-kind rows are what kinds 0 / 1 gave before kinds 5 / 6 existed -- and differ exactly where plan_gemm_tile's
    `inference` rules say; kinds 2, 3 and 4 still answer, and an unknown kind is an error."""
    import re
    buf = ctypes.create_string_buffer(160)

    def short(kind, B, call):
        ks = lib.svs_describe_plan(kind, B, *call, buf, 160)
        full = buf.value.decode()
        if full == "gather_window_kernel":
            assert ks == 1
            return "gather_window"
        m = re.fullmatch(r"parity_window_kernel<(\d+), (\d+), (\d+), (\d+), true>", full)
        if m:
            assert ks == 1
            return "window<" + ",".join(m.groups()) + ">"
        m = re.fullmatch(r"conv_gemm_kernel<([01]), (\d+), (\d+), (\d+), (\d+), (true|false), (true|false), false, ([12])>", full)
        assert m and int(m.group(1)) == kind % 5, (kind, full)
        return f"{m.group(2)}x{m.group(3)}" + ("u" if m.group(6) == "true" else "s" if m.group(7) == "true" else "") + f"/{ks}"

    for B in (16, 64):
        train = " ".join(short(int(name.startswith("deconv")), B, call) for name, call in FWD_CALLS)
        evalp = " ".join(short(5 + int(name.startswith("deconv")), B, call) for name, call in FWD_CALLS)
        assert train == TRAIN_PLANS[B], (B, train)
        assert evalp == EVAL_PLANS[B], (B, evalp)
    # the kernels that take no tile from plan_gemm_tile do not depend on the kind of call: the direct kernels with the windows off
    tune("CONV_WINDOW", 0)
    for call, want in ((FWD_CALLS[9][1], "conv_direct_kernel<1, 4, 1>"), (FWD_CALLS[8][1], "conv_direct_kernel<1, 4, 2>")):
        for kind in (1, 6):
            assert lib.svs_describe_plan(kind, 16, *call, buf, 160) == 1 and buf.value.decode() == want, (kind, buf.value)
    tune("CONV_WINDOW", -1)
    assert lib.svs_describe_plan(2, 16, 8, 2, 512, 0, 0, 256, buf, 160) == 2 and buf.value == b"wgrad_gemm_kernel<64, 128, 1, 4, true, false, 2>"
    assert lib.svs_describe_plan(3, 16, 64, 16, 64, 32, 8, 128, buf, 160) == 6 and buf.value == b"conv_gemm_bf16_kernel<0, 128, 128, 2, 2, 2>"
    assert lib.svs_describe_plan(4, 16, 16, 4, 512, 32, 8, 128, buf, 160) >= 1 and buf.value.startswith(b"conv_gemm_bf16_kernel<1, ")
    for kind in (-1, 7):
        assert lib.svs_describe_plan(kind, 16, 64, 16, 64, 32, 8, 128, buf, 160) == -1
        assert b"unknown kind" in lib.svs_last_error_string()


def test_each_gemm_tile_is_built_with_one_prefetch_depth(lib, tmp_path):
    """PF (K-tiles requested ahead) is the last template argument of conv_gemm_kernel and wgrad_gemm_kernel and a compile-time
    property of the tile: conv_gemm_pf(BM, BN) in gemm_conv.hip, wgrad_gemm_pf(BM, skip) in gemm_wgrad.hip, mirrored below.  Every
    tile of the built library occurs with exactly that PF and no other (symbol names only: a form the launchers cannot reach is
    compile time and code-object size for nothing)."""
    import importlib.util
    import re
    spec = importlib.util.spec_from_file_location("check_isa", os.path.join(ROOT, "tools", "check_isa.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    mangled = []
    for co in isa.device_code_objects(_lib.LIB_PATH, str(tmp_path)):
        syms = subprocess.run([f"{isa.LLVM}/llvm-objdump", "-t", co], capture_output=True, text=True, check=True).stdout
        mangled += [ln.split()[-1] for ln in syms.splitlines() if " F .text" in ln]
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.splitlines()
    args = lambda d: [a.strip() for a in re.search(r"<(.*)>", d.split("(")[0]).group(1).split(",")]
    conv, wgrad = {}, {}                          # tile -> the PF values it is built with
    for d in demangled:
        if "conv_gemm_kernel<" in d:              # <MODE, BM, BN, WM, WN, UNI, SKIP, SPLIT, PF>
            a = args(d)
            conv.setdefault((int(a[1]), int(a[2]), int(a[3]), int(a[4])), set()).add(int(a[8]))
        elif "wgrad_gemm_kernel<" in d:           # <BM, BN, WM, WN, SKIP, SPLIT, PF>: the tap-skipping form of a tile is a tile of its own
            a = args(d)
            wgrad.setdefault((int(a[0]), int(a[1]), int(a[2]), int(a[3]), a[4] == "true"), set()).add(int(a[6]))
    assert set(conv) == {(128, 128, 2, 2), (128, 64, 2, 2), (256, 32, 4, 1), (256, 16, 4, 1), (32, 128, 1, 4), (64, 64, 2, 2), (64, 128, 2, 2)}
    assert set(wgrad) == {(bm, 128, wm, 4 // wm, skip) for bm, wm in ((128, 2), (64, 1), (32, 1)) for skip in (False, True)}
    for (bm, bn, _, _), pfs in conv.items():
        assert pfs == {1 if (bm, bn) == (128, 128) or bm == 32 else 2}, (bm, bn, pfs)
    for (bm, _, _, _, skip), pfs in wgrad.items():
        assert pfs == {2 if skip and bm != 32 else 1}, (bm, skip, pfs)


def test_bench_gpus_n_launches_child_ranks(tmp_path):
    """`python bench.py --gpus N` with no launcher around it starts N child ranks itself (before any GPU call), forwards rank 0's
    one JSON line and fails when a rank fails.  The ranks here are a stub script (SVS_BENCH_WORKER) that checks the rendezvous
    environment the real worker reads; on this GPU-less box the real worker must fail with a clear message."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stub = tmp_path / "stub_rank.py"
    stub.write_text(
        "import json, os, sys\n"
        "r, w = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])\n"
        "assert int(os.environ['LOCAL_RANK']) == r and os.environ['MASTER_ADDR'] == '127.0.0.1' and int(os.environ['MASTER_PORT']) > 0\n"
        "assert sys.argv[1:] == ['--gpus', str(w), '--steps', '2'], sys.argv\n"
        "if os.environ.get('STUB_FAIL_RANK') == str(r):\n"
        "    sys.exit(3)\n"
        "print('chatter from rank', r)\n"
        "if r == 0:\n"
        "    print(json.dumps({'metric': 'stub', 'n_gpus': w, 'port': int(os.environ['MASTER_PORT'])}))\n")
    env = dict(os.environ, SVS_BENCH_WORKER=str(stub))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "3", "--steps", "2"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 3, r.stdout
    assert "chatter from rank 0" in r.stderr and "chatter from rank 2" in r.stderr
    r = subprocess.run(cmd, env=dict(env, STUB_FAIL_RANK="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 3 and not r.stdout.strip() and "rank 1 exited with code 3" in r.stderr, (r.returncode, r.stdout, r.stderr[-500:])
    if not torch.cuda.is_available():
        env.pop("SVS_BENCH_WORKER")
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and not r.stdout.strip() and "sees no GPU" in r.stderr, (r.returncode, r.stderr[-500:])


def test_bench_dump_outputs_format(tmp_path):
    """bench.dump_outputs on CPU stand-ins of the model's flat buffers at their real sizes: float32 .npy files, 64 MB at most
    in all, the gradient sample drawn at the same indices every time; an eval mask too large for the limit is sampled.
    --steps below 1 is refused."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(3)
    model = types.SimpleNamespace(_flat=torch.randn(9823313, generator=g), _gflat=torch.randn(9823313, generator=g),
                                  _bn_flat=torch.randn(2016, generator=g))
    names = bench.dump_outputs(str(tmp_path / "a"), "train", model, torch.tensor(0.25))
    bench.dump_outputs(str(tmp_path / "b"), "train", model, torch.tensor(0.25))
    assert names == ["bn_running_stats", "grads_sample", "loss", "params"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b), n
        total += (tmp_path / "a" / f"{n}.npy").stat().st_size
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / "a" / "params.npy"), model._flat.numpy())
    gs = np.load(tmp_path / "a" / "grads_sample.npy")
    assert gs.size == bench.GRAD_SAMPLE and np.isin(gs, model._gflat.numpy()).all()
    mask = torch.rand((216, 1, 512, 128), generator=g)
    assert bench.dump_outputs(str(tmp_path / "e"), "eval", None, mask) == ["mask_sample"]
    assert np.load(tmp_path / "e" / "mask_sample.npy").size == bench.MASK_LIMIT
    assert bench.dump_outputs(str(tmp_path / "f"), "eval", None, mask[:16]) == ["mask"]
    assert np.array_equal(np.load(tmp_path / "f" / "mask.npy"), mask[:16].numpy())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr
