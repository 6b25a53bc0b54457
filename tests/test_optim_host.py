"""The optimiser options, the host half (no GPU): svs_grad_norm / svs_adamw_step are declared in a header that stays plain C,
bound, and refuse bad arguments before any launch (all device pointers NULL); train.py's flag messages, its warm-up function and
the rule that --lr switches the epoch-400 drop off; the EMA's state_dict keys; --ema on the three tools' command lines."""
import os
import subprocess

import pytest
import torch

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import train as svs_train
from svs_unet_pytorch_amd.model import FusedAdam, UNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_symbols_are_declared_and_bound(lib, tmp_path):
    syms = _lib.header_symbols()
    for name in ("svs_grad_norm_workspace_bytes", "svs_grad_norm", "svs_adamw_step"):
        assert name in syms and name in _lib._SIGS and hasattr(lib, name), name
    I, P, L, F, D, Z = _lib.I, _lib.P, _lib.L, _lib.F, _lib.D, _lib.Z
    assert _lib._SIGS["svs_grad_norm"] == (I, [P, L, F, D, P, P, Z, P])
    assert _lib._SIGS["svs_adamw_step"] == (I, _lib._SIGS["svs_adam_step"][1][:-1] + [D, P, P, D, P])     # svs_adam_step's, plus four
    src = tmp_path / "t.c"                                       # the header still compiles as C, with these types
    src.write_text('#include "svs_hip.h"\n'
                   "size_t (*ws)(int64_t) = svs_grad_norm_workspace_bytes;\n"
                   "int (*norm)(const float*, int64_t, float, double, double*, void*, size_t, hipStream_t) = svs_grad_norm;\n"
                   "int (*step)(float*, const float*, float*, float*, int64_t, double, double, double, double, int, float, double,\n"
                   "            const double*, float*, double, hipStream_t) = svs_adamw_step;\n"
                   "int main(void){return ws == 0 || norm == 0 || step == 0;}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(_lib.HEADER_PATH).read()
    assert "model.py:116" in text and "train.py:298-300" in text


def test_bad_arguments_are_refused_before_any_launch(lib):
    assert lib.svs_grad_norm_workspace_bytes(10) > 0
    assert lib.svs_grad_norm(None, 10, 1.0, 1.0, None, None, 0, None) == -1
    assert "svs_grad_norm" in lib.svs_last_error_string().decode()
    assert lib.svs_grad_norm(4, 10, 1.0, 1.0, 8, None, 0, None) == -2                 # (never dereferenced: no workspace)
    assert "workspace" in lib.svs_last_error_string().decode()
    assert lib.svs_grad_norm(6, 10, 1.0, 1.0, 8, 8, 1 << 20, None) == -1               # g not 4-byte aligned
    assert lib.svs_adamw_step(None, None, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 0.0, None, None, 0.0, None) == -1
    assert lib.svs_adamw_step(4, 4, 4, 4, 10, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 0.0, None, None, 1.0, None) == -1     # ema_decay = 1
    assert "ema_decay" in lib.svs_last_error_string().decode()
    assert lib.svs_adamw_step(4, 4, 4, 4, 10, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, -1.0, None, None, 0.0, None) == -1    # negative decay
    assert lib.svs_adamw_step(4, 4, 4, 4, 10, 1e-3, 0.9, 0.999, 1e-8, 0, 1.0, 0.0, None, None, 0.0, None) == -1     # step 0


@pytest.mark.parametrize("args,word", [
    ((-1e-3, 0.0, 0.0, None, 0), "--weight_decay"),
    ((float("nan"), 0.0, 0.0, None, 0), "--weight_decay"),
    ((0.0, -1.0, 0.0, None, 0), "--clip_grad_norm"),
    ((0.0, float("inf"), 0.0, None, 0), "--clip_grad_norm"),
    ((0.0, 0.0, 1.0, None, 0), "--ema_decay"),
    ((0.0, 0.0, -0.1, None, 0), "--ema_decay"),
    ((0.0, 0.0, float("nan"), None, 0), "--ema_decay"),
    ((0.0, 0.0, 0.0, 0.0, 0), "--lr"),
    ((0.0, 0.0, 0.0, -1e-3, 0), "--lr"),
    ((0.0, 0.0, 0.0, None, -1), "--warmup_steps"),
])
def test_flag_messages(args, word):
    msg = svs_train.check_optim(*args)
    assert msg is not None and msg.startswith(word + " ") and "must be" in msg


def test_good_flags_pass():
    assert svs_train.check_optim(0.0, 0.0, 0.0, None, 0) is None
    assert svs_train.check_optim(1e-2, 5.0, 0.999, 3e-4, 1000) is None


@pytest.mark.parametrize("flags,word", [(["--ema_decay", "1"], "--ema_decay"), (["--weight_decay", "-1"], "--weight_decay"),
                                        (["--clip_grad_norm", "-2"], "--clip_grad_norm"), (["--lr", "0"], "--lr"),
                                        (["--warmup_steps", "-3"], "--warmup_steps")])
def test_train_refuses_bad_flags_before_any_device(flags, word, capsys, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    with pytest.raises(SystemExit) as e:
        svs_train.main(["--label", "x"] + flags)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_warmup_function():
    lr, n = 3e-4, 8
    assert svs_train.warmup_lr(lr, 0, n) == 0.0
    assert svs_train.warmup_lr(lr, 1, n) == lr * (1 / 8)
    assert svs_train.warmup_lr(lr, n, n) == lr
    assert svs_train.warmup_lr(lr, n + 1, n) == lr
    assert all(svs_train.warmup_lr(lr, t, n) < svs_train.warmup_lr(lr, t + 1, n) for t in range(n))
    assert svs_train.warmup_lr(lr, 0, 0) == lr and svs_train.warmup_lr(lr, 5, 0) == lr          # no warm-up: the rate itself


def test_lr_flag_switches_the_epoch_400_rule_off():
    assert svs_train.lr_drop_applies(400, None) and not svs_train.lr_drop_applies(399, None) and not svs_train.lr_drop_applies(401, None)
    assert not svs_train.lr_drop_applies(400, 1e-3) and not svs_train.lr_drop_applies(400, 5e-4)
    assert svs_train.reference_lr(0) == svs_train.reference_lr(399) == 1e-3 and svs_train.reference_lr(400) == svs_train.reference_lr(900) == 5e-4


def test_optimiser_defaults_and_refusals():
    model = UNet()
    assert (model.optim.weight_decay, model.optim.max_grad_norm, model.optim.ema_decay) == (0.0, 0.0, 0.0)
    assert model._ema_flat is None and model.optim_stats.dtype == torch.float64 and model.optim_stats.shape == (4,)
    assert model.optim.param_groups[0]["weight_decay"] == 0                  # torch.optim.Adam's checkpoint layout, unchanged
    for bad in (dict(weight_decay=-1.0), dict(max_grad_norm=-1.0), dict(ema_decay=1.0), dict(ema_decay=-0.5)):
        with pytest.raises(ValueError):
            FusedAdam(model, **bad)


def test_ema_state_dict_keys_and_swap_on_the_host():
    model = UNet()
    with pytest.raises(RuntimeError, match="no EMA"):
        model.ema_state_dict()
    model.start_ema()
    with torch.no_grad():
        model._ema_flat.mul_(0.5)
    sd, ema = model.state_dict(), model.ema_state_dict()
    assert list(ema) == list(sd) and len(ema) == 79
    params = {n for n, _ in model.named_parameters()}
    for k in sd:
        assert ema[k].shape == sd[k].shape and ema[k].dtype == sd[k].dtype
        assert torch.equal(ema[k], sd[k] * 0.5 if k in params else sd[k]), k
    live, epoch = model._flat.clone(), model._param_epoch
    with model.ema_weights():
        assert torch.equal(model._flat, live * 0.5) and torch.equal(model._ema_flat, live) and model._param_epoch > epoch
        inside = model.ema_state_dict()
        with pytest.raises(RuntimeError, match="nest"):
            with model.ema_weights():
                pass
    assert torch.equal(model._flat, live) and torch.equal(model._ema_flat, live * 0.5) and model._param_epoch > epoch + 1
    assert all(torch.equal(inside[k], ema[k]) for k in ema)
    other = UNet()
    other.load_ema_state_dict(ema)
    assert torch.equal(other._ema_flat, model._ema_flat)


@pytest.mark.parametrize("mod", ["validate", "separate", "inference"])
def test_tools_have_the_ema_flag(mod):
    import importlib
    import inspect
    m = importlib.import_module(f"svs_unet_pytorch_amd.{mod}")
    assert '"--ema"' in inspect.getsource(m.main)
    from svs_unet_pytorch_amd.inference import no_ema_message
    msg = no_ema_message("validate.py", "x.pth")
    assert "x.pth" in msg and "ema_state_dict" in msg and "--ema_decay" in msg
