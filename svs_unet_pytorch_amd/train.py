"""Training driver -- same command line, checkpoint / log file names and dataset semantics as the
reference's train.py (/root/reference/train.py:157-171, 65-143, 244-387), with the optimisation step
(train.py:265-300, L1 terms) running as one fused library call per step on each GPU.

    python -m svs_unet_pytorch_amd.train --train_folder spec/train --valid_folder spec/valid --label run1 \
        --batch_size 64 --epoch 400 --val_interval 10 [--load_path CKPT/svs_run1.pth] [--win_size 512|1024|2048] [--hop_size N]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m svs_unet_pytorch_amd.train ...

What is kept: flags (--train_folder --load_path --label(required) --epoch --batch_size --valid_folder
--val_interval), `SpectrogramDataset` (file pairing, len = songs x SAMPLES_PER_SONG, DC-row drop, shared
random 128-frame crop or right zero-pad, phase as np.angle), LR drop to 5e-4 with a snapshot at epoch 400
(train.py:251-262), per-epoch checkpoint CKPT/svs_<label>.pth with keys {epoch, model_state_dict, optim,
scheduler, loss_list_*} (train.py:369-382), best-validation checkpoint CKPT/svs_best_<label>.pth via
model.save (train.py:353-355), LOG/log_<label>.txt with one float per epoch and `Val <float>` lines
(train.py:314,350,357-363).

The objective is the reference's: alpha_L1 * (L1 vocal + L1 accompaniment) + alpha_MR * MultiResolutionSTFTLoss of
the re-synthesised vocal waveforms (train.py:24-26,281-296 with model.crit = nn.L1Loss), all of it on the GPU
(csrc/mrstft.hip restates the `auraloss` definition, which is not installable here: parity unpinned for that term).
SVS_OBJECTIVE=l1 drops the MR term (the BASELINE "L1-loss step"); it is also dropped, with a warning, when the
data set has no *_phase.npy files.  The logged totals are the same quantity as the reference's.  With WORLD_SIZE > 1 the batch is sharded over ranks and gradients are
all-reduced over RCCL (parallel.py); rank 0 writes the files.  CKPT/ and LOG/ are created if missing (the
reference assumes they exist).

Validation (train.py:317-363) runs from HBM too under the default SVS_DATA_LOADER=resident: the validation folder is a second
`ResidentSpectrograms` and `validation_pass` makes one `UNet.eval_losses` call (svs_unet_eval_loss) per batch, summing on the
device; the pass ends in one read-back and logs the same `Val` value, the mean of per-batch totals.  Any other SVS_DATA_LOADER
keeps the reference's host loop (a 2-worker DataLoader, `l1_terms` / `mr_term`).  `python -m svs_unet_pytorch_amd.validate`
runs the pass on a checkpoint without training.

--win_size / --hop_size (the config's 1024 / 768 by default) name the STFT geometry of the folder that `data.py --direction
to_spec --win_size W --hop_size H` wrote (data.py:24-25 lets both vary): tiles are (win_size / 2, INPUT_LEN), the network is
fully convolutional, and the MR-STFT term re-synthesises its waveforms with that window and hop (its own three resolutions
stay auraloss's).  Every file of the folder is checked against the window before anything is uploaded; checkpoints record
`win_size` / `hop_size`, and resuming one under other flags is an error.  `separate.py --win_size W --hop_size H` takes the
checkpoint.

--augment gain|remix (default none: the path above, unchanged) cuts augmented training tiles from the same resident set
(augment.py, csrc/augment.hip; the reference has no augmentation): a random gain per source and, for remix, the vocal of one crop
over the accompaniment of another, formed from the complex spectra so that it is the STFT of the re-mixed audio.  --gain_range,
--remix_prob and --augment_seed set it; an epoch's table depends on (seed, epoch) only, goes up in one copy, and each step is one
launch.  --stretch_range LO HI (with --augment gain|remix; csrc/stretch.hip) also time-stretches every source before the mix, a phase
vocoder on the resident spectra at a rate of its own per source.  --pitch_range LO HI (semitones; with --augment gain|remix, with or
without --stretch_range; csrc/pitch.hip) also shifts the pitch of every source before the mix: the same vocoder with the frequency
axis resampled and the phase advance scaled.  Validation is never augmented; the checkpoint format is unchanged.

--weight_decay X, --clip_grad_norm X, --ema_decay X (all 0 = off: the optimiser step is then the reference's Adam, one launch) turn on
decoupled weight decay, clipping by the global gradient norm and an exponential moving average of the weights inside the optimiser
step (csrc/optim.hip: `svs_grad_norm` + `svs_adamw_step`, nothing read back inside a step; a step whose gradient norm is not finite
is skipped).  --lr X sets the rate and switches the epoch-400 rule off; --warmup_steps N makes the rate lr * min(1, t / N) at
optimiser step t.  With --ema_decay validation runs on the EMA weights, svs_best_<label>.pth carries them as its model_state_dict,
and the resume checkpoint keeps the live weights and adds `ema_state_dict` / `ema_decay`; per epoch rank 0 prints the last gradient
norm and the counts of clipped and skipped steps.
"""
from __future__ import annotations

import argparse
import contextlib
import os
import random

import numpy as np
import torch
import torch.utils.data as Data

from .config import HOP_SIZE, INPUT_LEN, SAMPLES_PER_SONG, WINDOW_SIZE
from .data import WINDOW_SIZES            # the n_fft the transforms of csrc/stft.hip are built for
from .model import ALPHA_L1, ALPHA_MR, UNet


def check_geometry(win_size, hop_size):
    """The message for a --win_size / --hop_size pair that cannot be trained at, or None (data.py's own rule)."""
    if win_size not in WINDOW_SIZES:
        return (f"--win_size {win_size}: the STFT / iSTFT kernels are built for n_fft = {', '.join(map(str, WINDOW_SIZES))} "
                f"(default {WINDOW_SIZE}, config.WINDOW_SIZE); --hop_size may be anything in 1..win_size")
    if not 0 < hop_size <= win_size:
        return f"--hop_size {hop_size}: must be in 1..{win_size} (a larger hop leaves samples that no frame covers)"
    return None


REFERENCE_LR = 1e-3            # model.py:116
REFERENCE_LR_DROP = (400, 5e-4)      # train.py:251-262: epoch, rate


def check_optim(weight_decay, clip_grad_norm, ema_decay, lr, warmup_steps):
    """The message for optimiser flags that cannot be trained with, or None."""
    import math
    if not (math.isfinite(weight_decay) and weight_decay >= 0):
        return f"--weight_decay {weight_decay}: must be >= 0 (decoupled decay, p *= 1 - lr * weight_decay per step; 0 = off)"
    if not (math.isfinite(clip_grad_norm) and clip_grad_norm >= 0):
        return f"--clip_grad_norm {clip_grad_norm}: must be >= 0 (the largest global gradient norm a step is taken with; 0 = off)"
    if not 0 <= ema_decay < 1:
        return f"--ema_decay {ema_decay}: must be in [0, 1) (ema = d * ema + (1 - d) * weights per step; 0 = off)"
    if lr is not None and not (math.isfinite(lr) and lr > 0):
        return f"--lr {lr}: must be > 0 (without the flag: {REFERENCE_LR}, halved at epoch {REFERENCE_LR_DROP[0]})"
    if warmup_steps < 0:
        return f"--warmup_steps {warmup_steps}: must be >= 0 (the rate is lr * min(1, t / N) at step t; 0 = off)"
    return None


def warmup_lr(lr, t, warmup_steps):
    """The rate of step t (1-based; t = 0 is before the first step) under a linear warm-up of `warmup_steps` steps."""
    return lr if warmup_steps <= 0 else lr * min(1.0, t / warmup_steps)


def lr_drop_applies(epoch, lr_flag):
    """The reference's drop to 5e-4 with its snapshot (train.py:251-262): at epoch 400, unless --lr set the rate."""
    return lr_flag is None and epoch == REFERENCE_LR_DROP[0]


def reference_lr(epoch):
    """The reference's rate while epoch `epoch` runs."""
    return REFERENCE_LR_DROP[1] if epoch >= REFERENCE_LR_DROP[0] else REFERENCE_LR


def checkpoint_geometry(checkpoint):
    """(win_size, hop_size) a checkpoint was trained at; one written before the keys existed was trained at the config's."""
    return int(checkpoint.get("win_size", WINDOW_SIZE)), int(checkpoint.get("hop_size", HOP_SIZE))


def check_rows(path, rows, win_size):
    """A spectrogram file of `rows` rows (DC row included) against the window: data.py writes win_size / 2 + 1 of them."""
    if rows != win_size // 2 + 1:
        fits = 2 * (rows - 1)
        hint = f"--win_size {fits} would match it" if fits in WINDOW_SIZES else f"no built window ({', '.join(map(str, WINDOW_SIZES))}) matches it"
        raise ValueError(f"{path}: {rows} rows, but --win_size {win_size} needs {win_size // 2 + 1} (n_fft / 2 + 1); {hint}")


def _rows_of(path):
    return int(np.load(path, mmap_mode="r").shape[0])          # (the header only: nothing of the array is read)


class SpectrogramDataset(Data.Dataset):
    """train.py:65-143.  Returns (mix, voc, mix_phase, voc_phase), each float32 (1, win_size / 2, INPUT_LEN)."""

    def __init__(self, path, samples_per_song=SAMPLES_PER_SONG, with_phase=True, win_size=WINDOW_SIZE):
        self.path = path
        self.win_size = int(win_size)
        self.with_phase = with_phase          # False: L1-only objective or a set without *_phase.npy -> empty phase tensors
        self.mixture_path = os.path.join(path, "mixture")
        self.vocal_path = os.path.join(path, "vocal")
        self.samples_per_song = samples_per_song
        if not os.path.exists(self.mixture_path):
            raise FileNotFoundError(f"Mixture folder not found: {self.mixture_path}")     # train.py:72-73
        names = sorted(f for f in os.listdir(self.mixture_path) if f.endswith("_spec.npy"))
        self.file_names = [f for f in names if os.path.exists(os.path.join(self.vocal_path, f))]
        for f in self.file_names:                 # every song against the window, before anything is loaded or uploaded
            for d in (self.mixture_path, self.vocal_path):
                check_rows(os.path.join(d, f), _rows_of(os.path.join(d, f)), self.win_size)
        print(f"[{os.path.basename(path)}] {len(self.file_names)} songs x {self.samples_per_song} samples = {len(self)} items.")

    def __len__(self):
        return len(self.file_names) * self.samples_per_song

    def __getitem__(self, idx):
        name = self.file_names[idx % len(self.file_names)]
        pname = name.replace("_spec.npy", "_phase.npy")
        mix = np.load(os.path.join(self.mixture_path, name))
        check_rows(os.path.join(self.mixture_path, name), mix.shape[0], self.win_size)
        mix = mix[1:, :]                                                                  # drop the DC row (train.py:109-112)
        voc = np.load(os.path.join(self.vocal_path, name))[1:, :]
        if self.with_phase:
            mix_phase = np.angle(np.load(os.path.join(self.mixture_path, pname))).astype(np.float32)[1:, :]
            voc_phase = np.angle(np.load(os.path.join(self.vocal_path, pname))).astype(np.float32)[1:, :]
        else:                                                                             # same crop / pad arithmetic on nothing
            mix_phase = voc_phase = np.zeros((0, mix.shape[1]), np.float32)
        target, cur = INPUT_LEN, mix.shape[1]
        if cur > target:
            start = random.randint(0, cur - target)                                       # shared start (train.py:121)
            mix, voc = mix[:, start:start + target], voc[:, start:start + target]
            mix_phase, voc_phase = mix_phase[:, start:start + target], voc_phase[:, start:start + target]
        else:
            pad = ((0, 0), (0, target - cur))                                             # train.py:129-135
            mix, voc = np.pad(mix, pad), np.pad(voc, pad)
            mix_phase, voc_phase = np.pad(mix_phase, pad), np.pad(voc_phase, pad)
        as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a[np.newaxis], dtype=np.float32))
        return as_t(mix), as_t(voc), as_t(mix_phase), as_t(voc_phase)

    def has_phase_files(self):
        pname = lambda n: n.replace("_spec.npy", "_phase.npy")
        return all(os.path.exists(os.path.join(d, pname(n))) for n in self.file_names for d in (self.mixture_path, self.vocal_path))


def folder_has_phase_files(path):
    """SpectrogramDataset.has_phase_files from the listing alone (no file is opened): every paired song of `path` has its
    *_phase.npy in mixture/ and vocal/.  A folder that is not there has none."""
    mixture, vocal = os.path.join(path, "mixture"), os.path.join(path, "vocal")
    if not os.path.isdir(mixture):
        return False
    names = [f for f in sorted(os.listdir(mixture)) if f.endswith("_spec.npy") and os.path.exists(os.path.join(vocal, f))]
    return all(os.path.exists(os.path.join(d, n.replace("_spec.npy", "_phase.npy"))) for n in names for d in (mixture, vocal))


def epoch_order(n, shuffle=True, rank=0, world=1, epoch=0):
    """Item indices of one epoch for one rank -- DataLoader(shuffle=True) on one process, DistributedSampler on several:
    one permutation of all n items (the same on every rank: seeded by the epoch), padded by wrapping around to a multiple
    of `world`, rank r taking positions r, r + world, ..."""
    if shuffle:
        gen = torch.Generator()
        gen.manual_seed(epoch if world > 1 else random.getrandbits(31))
        order = torch.randperm(n, generator=gen).tolist()
    else:
        order = list(range(n))
    if world > 1:
        total = (n + world - 1) // world * world
        order = (order + order[:total - n])[rank:total:world]
    return order


class ResidentSpectrograms:
    """The training set kept in HBM: every song's mixture / vocal magnitude (DC row dropped) is uploaded once, and a batch
    is cut out of them by one kernel (`svs_crop_tiles`) -- no worker processes, no per-step host-to-device copies of
    tiles.  Same items and cropping rule as SpectrogramDataset (train.py:86-143): `samples_per_song` items per song,
    item idx -> song idx % n_songs, one random start shared by mixture and vocal, right zero-padding for short songs.
    A MUSDB18-sized set is ~1 GB of the 288 GB."""

    def __init__(self, dataset: SpectrogramDataset, device, with_phase: bool = True):
        self.n_songs = len(dataset.file_names)
        self.samples_per_song = dataset.samples_per_song
        self.device = device
        mix_parts, voc_parts, offsets, frames, off = [], [], [], [], 0
        ph_mix, ph_voc = [], []
        pname = lambda n: n.replace("_spec.npy", "_phase.npy")
        self.has_phase = with_phase and all(os.path.exists(os.path.join(d, pname(n))) for n in dataset.file_names
                                            for d in (dataset.mixture_path, dataset.vocal_path))
        self.rows = dataset.win_size // 2
        for name in dataset.file_names:          # (again here: the folder may have changed since the dataset listed it)
            for d in (dataset.mixture_path, dataset.vocal_path):
                check_rows(os.path.join(d, name), _rows_of(os.path.join(d, name)), dataset.win_size)
        for name in dataset.file_names:
            if self.has_phase:                       # unit phasors complex64 (513, T) -> rows 1.. (train.py:103-112)
                ph_mix.append(np.ascontiguousarray(np.load(os.path.join(dataset.mixture_path, pname(name)))[1:, :], dtype=np.complex64).reshape(-1))
                ph_voc.append(np.ascontiguousarray(np.load(os.path.join(dataset.vocal_path, pname(name)))[1:, :], dtype=np.complex64).reshape(-1))
            mix = np.load(os.path.join(dataset.mixture_path, name))[1:, :]                   # drop the DC row (train.py:109-112)
            voc = np.load(os.path.join(dataset.vocal_path, name))[1:, :]
            if voc.shape != mix.shape:
                raise ValueError(f"{name}: mixture {mix.shape} and vocal {voc.shape} differ")
            mix_parts.append(np.ascontiguousarray(mix, dtype=np.float32).reshape(-1))
            voc_parts.append(np.ascontiguousarray(voc, dtype=np.float32).reshape(-1))
            offsets.append(off)
            frames.append(mix.shape[1])
            off += mix.size
        empty = np.zeros(0, np.float32)
        self.mix = torch.from_numpy(np.concatenate(mix_parts) if mix_parts else empty).to(device)
        self.voc = torch.from_numpy(np.concatenate(voc_parts) if voc_parts else empty).to(device)
        self.frames_host = list(frames)
        self.offsets = torch.tensor(offsets, dtype=torch.int64, device=device)
        self.frames = torch.tensor(frames, dtype=torch.int32, device=device)
        self.mix_ang = self.voc_ang = None
        if self.has_phase and mix_parts:             # np.angle on the device (train.py:103-104), kept resident like the magnitudes
            from . import _lib
            for attr, parts in (("mix_ang", ph_mix), ("voc_ang", ph_voc)):
                z = torch.view_as_real(torch.from_numpy(np.concatenate(parts)).to(device)).contiguous()
                ang = torch.empty(z.shape[0], dtype=torch.float32, device=device)
                _lib.check(_lib.lib().svs_phase_angle(z.data_ptr(), ang.data_ptr(), ang.numel(), _lib.stream_ptr()), "svs_phase_angle")
                setattr(self, attr, ang)

    def __len__(self):
        return self.n_songs * self.samples_per_song

    def draw(self, items, rng=random):
        """(song, start) per item: the host side of __getitem__ (train.py:115-127)."""
        songs = [int(i) % self.n_songs for i in items]
        starts = [rng.randint(0, self.frames_host[s] - INPUT_LEN) if self.frames_host[s] > INPUT_LEN else 0 for s in songs]
        return songs, starts

    def crop(self, songs, starts, with_phase: bool = False):
        """mix, voc [, mix_phase, voc_phase] (B, 1, win_size / 2, INPUT_LEN) on the device for the given songs / start frames; the
        phase tiles are angles cut with the SAME start (train.py:121-127)."""
        return self.crop_table(self.upload_table(songs, starts), 0, len(songs), with_phase)

    def upload_table(self, songs, starts):
        """The (song, start) table of any number of items -- a batch or a whole pass -- as one (2, N) int32 device tensor:
        one host-to-device copy."""
        return torch.tensor([songs, starts], dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)

    def crop_table(self, table, lo, hi, with_phase: bool = False):
        """`crop` for items lo..hi-1 of an uploaded table: `svs_crop_tiles` reads its songs and starts through pointers, so a
        batch of a pass is a slice of the pass's table and costs no copy of its own."""
        from . import _lib
        B = hi - lo
        if not (0 <= lo < hi <= table.shape[1]) or table.dtype != torch.int32 or table.shape[0] != 2 or not table.is_contiguous():
            raise ValueError(f"items {lo}..{hi} of a table of shape {tuple(table.shape)}")
        if with_phase and self.mix_ang is None:
            raise ValueError("phase tiles asked of a set without *_phase.npy files")
        songs, starts = table[0, lo:hi], table[1, lo:hi]
        out = []
        pairs = [(self.mix, self.voc)] + ([(self.mix_ang, self.voc_ang)] if with_phase else [])
        for a_src, b_src in pairs:
            a = torch.empty((B, 1, self.rows, INPUT_LEN), dtype=torch.float32, device=self.device)
            b = torch.empty_like(a)
            _lib.check(_lib.lib().svs_crop_tiles(a_src.data_ptr(), b_src.data_ptr(), self.offsets.data_ptr(), self.frames.data_ptr(),
                                                 songs.data_ptr(), starts.data_ptr(), B, self.rows, INPUT_LEN, a.data_ptr(), b.data_ptr(),
                                                 _lib.stream_ptr()), "svs_crop_tiles")
            out += [a, b]
        return tuple(out)

    def batches(self, batch_size, shuffle=True, rank=0, world=1, epoch=0, with_phase: bool = False):
        """One epoch of (mix, voc) batches: DataLoader(shuffle) / DistributedSampler semantics -- a permutation of all items
        (the same on every rank, seeded by the epoch), padded to a multiple of `world`, rank r taking items r, r+world, ...;
        the last batch may be short."""
        order = epoch_order(len(self), shuffle, rank, world, epoch)
        for i in range(0, len(order), batch_size):
            yield self.crop(*self.draw(order[i:i + batch_size]), with_phase=with_phase)

    def augmented_batches(self, batch_size, rank=0, world=1, epoch=0, with_phase: bool = False, aug=None, hop=HOP_SIZE):
        """One epoch of `batches` with gain / remix augmentation (augment.py): the same permutation and sharding of the items, each
        item's sources, starts and gains from `augment.draw_epoch` -- a function of (aug.seed, epoch), so every rank draws the same
        table.  The rank's whole epoch goes up in ONE pinned copy (four int32 rows and two float32 rows of one buffer, as
        `validation_pass` uploads its pass); a batch is a slice of it and one `svs_crop_remix_tiles` launch: no per-step
        host-to-device copy, no read-back.  With aug.stretch_range set, every source is also time-stretched at a rate of its own:
        `augment.draw_epoch_stretch`'s table (eight rows) and one `svs_crop_stretch_tiles` launch per batch, at the window the set was
        written with (2 * rows) and `hop`.  With aug.pitch_range set, every source is also pitch-shifted by an amount of its own (and
        stretched if aug.stretch_range is set as well): `augment.draw_epoch_pitch`'s table (ten rows) and one `svs_crop_pitch_tiles`
        launch per batch."""
        from . import augment
        if aug is None or aug.mode == "none":
            raise ValueError("augmented_batches needs augmentation settings other than 'none' (`batches` is the plain path)")
        order = epoch_order(len(self), True, rank, world, epoch)
        if not order:
            return
        remix_prob = aug.remix_prob if aug.mode == "remix" else 0.0
        if aug.pitch_range is not None:
            drawn = augment.draw_epoch_pitch(len(self), self.frames_host, INPUT_LEN, epoch, aug.seed, aug.gain_range, remix_prob,
                                             aug.pitch_range, aug.stretch_range)
            table = augment.upload_pitch_table(self, drawn, order)
            for lo in range(0, len(order), batch_size):
                yield augment.crop_pitch(self, table, lo, min(lo + batch_size, len(order)), 2 * self.rows, hop, with_phase)
            return
        if aug.stretch_range is not None:
            drawn = augment.draw_epoch_stretch(len(self), self.frames_host, INPUT_LEN, epoch, aug.seed, aug.gain_range, remix_prob,
                                               aug.stretch_range)
            table = augment.upload_stretch_table(self, drawn, order)
            for lo in range(0, len(order), batch_size):
                yield augment.crop_stretch(self, table, lo, min(lo + batch_size, len(order)), 2 * self.rows, hop, with_phase)
            return
        drawn = augment.draw_epoch(len(self), self.frames_host, INPUT_LEN, epoch, aug.seed, aug.gain_range,
                                   aug.remix_prob if aug.mode == "remix" else 0.0)
        table = augment.upload_table(self, drawn, order)
        for lo in range(0, len(order), batch_size):
            yield augment.crop_remix(self, table, lo, min(lo + batch_size, len(order)), with_phase)

    def num_batches(self, batch_size, world=1):
        per_rank = (len(self) + world - 1) // world
        return (per_rank + batch_size - 1) // batch_size


def l1_terms(model, mix, voc):
    """Eval-mode loss of train.py:329-338 (no gradient)."""
    mask = model(mix)
    return model.crit(mask * mix, voc) + model.crit((1 - mask) * mix, torch.clamp(mix - voc, min=0.0))


def mr_term(model, mix, voc, mix_phase, voc_phase, n_fft=WINDOW_SIZE, hop=HOP_SIZE):
    """Eval-mode MR-STFT term of train.py:341-343 (no gradient): MR(specific_istft(mask*mix, mix_phase), specific_istft(voc, voc_phase)),
    the waveforms re-synthesised with the window and hop the tiles were made with."""
    from . import _lib
    from .data import specific_istft
    mask = model(mix)
    pred = specific_istft(mask * mix, mix_phase, n_fft, hop)
    tgt = specific_istft(voc, voc_phase, n_fft, hop)
    B, L_ = pred.shape[0], pred.shape[-1]
    L = _lib.lib()
    ws = torch.empty(int(L.svs_mrstft_workspace_bytes(B, L_)), dtype=torch.uint8, device=mix.device)
    out = torch.empty(1, dtype=torch.float32, device=mix.device)
    _lib.check(L.svs_mrstft_loss_fwd_bwd(pred.data_ptr(), tgt.data_ptr(), B, L_, 0.0, out.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                         _lib.stream_ptr()), "svs_mrstft_loss_fwd_bwd")
    return out[0]


def validation_plan(resident, batch_size, rng=random):
    """Host half of a validation pass: (songs, starts, [(lo, hi), ...]).  Items in dataset order, as DataLoader(shuffle=False)
    hands them out (item idx -> song idx % n_songs), starts drawn with `ResidentSpectrograms.draw`, batches of `batch_size`
    with a short last one."""
    n = len(resident)
    songs, starts = resident.draw(range(n), rng)
    return songs, starts, [(lo, min(lo + batch_size, n)) for lo in range(0, n, batch_size)]


def validation_pass(model, resident, batch_size, with_phase, win_size, hop_size, rng=random):
    """The validation loop of train.py:317-363 from the HBM-resident set: the pass's (song, start) table goes up in one copy,
    each batch is one `svs_crop_tiles` per tile pair and one `UNet.eval_losses(..., acc=acc)`; nothing inside reads from the
    device.  Returns (acc, n_batches): acc is the device double[3] of [sum of ALPHA_L1 * l1 + ALPHA_MR * mr, sum of l1, sum of
    mr] over the batches -- the caller's single `acc.cpu()` ends the pass, and acc[0] / n_batches is the logged value (the
    reference's mean of per-batch totals).  with_phase False: the L1 part only."""
    if resident.rows != win_size // 2:
        raise ValueError(f"the resident set has {resident.rows}-row tiles, --win_size {win_size} needs {win_size // 2}")
    songs, starts, bounds = validation_plan(resident, batch_size, rng)
    acc = torch.zeros(3, dtype=torch.float64, device=resident.device)
    if not bounds:
        return acc, 0
    table = resident.upload_table(songs, starts)
    for lo, hi in bounds:
        tiles = resident.crop_table(table, lo, hi, with_phase=with_phase)
        mph, vph = (tiles[2], tiles[3]) if with_phase else (None, None)
        model.eval_losses(tiles[0], tiles[1], mph, vph, hop=hop_size, acc=acc)
    return acc, len(bounds)


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--train_folder", type=str, default="./data/vocals")
    parser.add_argument("--load_path", type=str, default="result.pth")
    parser.add_argument("--label", type=str, required=True)
    parser.add_argument("--epoch", type=int, default=2)
    parser.add_argument("--batch_size", type=int, default=2)
    parser.add_argument("--valid_folder", type=str, default="unet_spectrograms/valid")
    parser.add_argument("--val_interval", type=int, default=20)
    parser.add_argument("--win_size", type=int, default=WINDOW_SIZE, help="STFT window the folders were written with (512, 1024 or 2048)")
    parser.add_argument("--hop_size", type=int, default=HOP_SIZE, help="hop the folders were written with, 1..win_size")
    from . import augment
    parser.add_argument("--augment", choices=augment.MODES, default="none",
                        help="training-set augmentation, cut on the device (augment.py): gain = a random gain per item; remix = a gain per "
                             "source and, with --remix_prob, the accompaniment of another crop under the item's vocal (needs *_phase.npy); "
                             "validation is never augmented")
    parser.add_argument("--gain_range", type=float, nargs=2, metavar=("LO", "HI"), default=list(augment.GAIN_RANGE),
                        help="gains are uniform in [LO, HI] (default: Open-Unmix's 0.25 1.25)")
    parser.add_argument("--remix_prob", type=float, default=augment.REMIX_PROB,
                        help="share of the items whose accompaniment comes from a random crop of a random song (default 0.5: a choice, not a tuned value)")
    parser.add_argument("--augment_seed", type=int, default=0, help="the tables of an epoch depend on (this, epoch) only")
    parser.add_argument("--stretch_range", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                        help="with --augment gain|remix: time-stretch every source before the mix by a phase vocoder on the device, at a "
                             "rate uniform in [LO, HI] within 0.5 .. 2 (needs *_phase.npy; default: no stretch; the range one would start "
                             "with, 0.8 1.25, is a choice, not a tuned value).  At the default 768-of-1024 hop the phase estimate is "
                             "unambiguous only within about +-2/3 bin: folders written with a smaller --hop_size stretch more cleanly")
    parser.add_argument("--pitch_range", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                        help="with --augment gain|remix, with or without --stretch_range: shift the pitch of every source before the mix "
                             "by a frequency-scaling phase vocoder on the device, by semitones uniform in [LO, HI] within -12 .. 12 (needs "
                             "*_phase.npy; default: no shift; -2 2 is a starting point, not a tuned value).  The shift moves formants with "
                             "the pitch and widens every partial by the pitch ratio")
    parser.add_argument("--weight_decay", type=float, default=0.0, help="decoupled weight decay (torch.optim.AdamW), on every parameter; 0 = off")
    parser.add_argument("--clip_grad_norm", type=float, default=0.0,
                        help="clip the global gradient norm to this (after the all-reduce under data parallelism); 0 = off")
    parser.add_argument("--ema_decay", type=float, default=0.0,
                        help="keep an exponential moving average of the weights with this decay, 0 <= d < 1: validation and the best "
                             "checkpoint use it, the resume checkpoint keeps both; 0 = off")
    parser.add_argument("--lr", type=float, default=None,
                        help=f"initial learning rate; without it the reference's {REFERENCE_LR} and its drop at epoch {REFERENCE_LR_DROP[0]}, "
                             "with it no drop")
    parser.add_argument("--warmup_steps", type=int, default=0, help="the rate is lr * min(1, t / N) at step t; 0 = off")
    args = parser.parse_args(argv)
    bad = check_geometry(args.win_size, args.hop_size)          # data.py:24-25 lets both vary; before any device is touched
    if bad:
        parser.error(bad)
    bad = check_optim(args.weight_decay, args.clip_grad_norm, args.ema_decay, args.lr, args.warmup_steps)
    if bad:
        parser.error(bad)
    optim_options = bool(args.weight_decay or args.clip_grad_norm or args.ema_decay)
    aug = None
    if args.stretch_range is not None and args.augment == "none":
        parser.error("--stretch_range: the stretch is part of the augmented tile cut, it needs --augment gain or --augment remix")
    if args.pitch_range is not None and args.augment == "none":
        parser.error("--pitch_range: the pitch shift is part of the augmented tile cut, it needs --augment gain or --augment remix")
    if args.augment != "none":                                  # `none` reaches nothing of augment.py beyond the flags' defaults
        bad = augment.check_settings(args.augment, args.gain_range, args.remix_prob, args.stretch_range, args.pitch_range)
        if bad:
            parser.error(bad)
        loader = os.environ.get("SVS_DATA_LOADER", "resident")
        if loader != "resident":
            parser.error(f"--augment {args.augment}: the augmentation is cut from the HBM-resident set, SVS_DATA_LOADER={loader} has none "
                         "(unset it, or train with --augment none)")
        if args.augment == "remix" and not folder_has_phase_files(args.train_folder):
            raise SystemExit(f"train.py: --augment remix needs the *_phase.npy files of every song of {args.train_folder} (the accompaniment "
                             "is mixture minus vocal as complex spectra); --augment gain works without them")
        if args.stretch_range is not None and not folder_has_phase_files(args.train_folder):
            raise SystemExit(f"train.py: --stretch_range needs the *_phase.npy files of every song of {args.train_folder} (the phase vocoder "
                             "reads the sources' angles; there is no magnitude-only stretch)")
        if args.pitch_range is not None and not folder_has_phase_files(args.train_folder):
            raise SystemExit(f"train.py: --pitch_range needs the *_phase.npy files of every song of {args.train_folder} (the phase vocoder "
                             "reads the sources' angles; there is no magnitude-only shift)")
        pitch = None if args.pitch_range is None else (float(args.pitch_range[0]), float(args.pitch_range[1]))
        stretch = None if args.stretch_range is None else (float(args.stretch_range[0]), float(args.stretch_range[1]))
        aug = augment.Augment(args.augment, (float(args.gain_range[0]), float(args.gain_range[1])), float(args.remix_prob), args.augment_seed,
                              stretch, pitch)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("train.py needs a ROCm device (hand-written gfx950 kernels, no CPU path).")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    print(f"Using device: {device}")
    grad_sync = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        from .parallel import init_process_group
        init_process_group(rank, world, device)

    log_file = f"LOG/log_{args.label}.txt"
    best_weight = f"CKPT/svs_best_{args.label}.pth"
    ckpt_weight = f"CKPT/svs_{args.label}.pth"
    if rank == 0:
        os.makedirs("LOG", exist_ok=True)
        os.makedirs("CKPT", exist_ok=True)

    if os.path.exists(args.load_path):                                     # a checkpoint trained at another geometry: stop here
        ck_geo = checkpoint_geometry(torch.load(args.load_path, map_location="cpu"))
        if ck_geo != (args.win_size, args.hop_size):
            raise SystemExit(f"train.py: {args.load_path} was trained at --win_size {ck_geo[0]} --hop_size {ck_geo[1]}, not at "
                             f"--win_size {args.win_size} --hop_size {args.hop_size}: resume it with its own geometry")
    try:                                                                   # and a folder written at another window
        train_dataset = SpectrogramDataset(args.train_folder, win_size=args.win_size)
        valid_dataset = SpectrogramDataset(args.valid_folder, win_size=args.win_size) if os.path.exists(args.valid_folder) else None
    except ValueError as e:
        raise SystemExit(f"train.py: {e}")
    sampler = train_loader = resident = None
    per_rank_batch = max(args.batch_size // world, 1)
    if os.environ.get("SVS_DATA_LOADER", "resident") == "resident":
        resident = ResidentSpectrograms(train_dataset, device)            # the whole set lives in HBM (see the class)
    else:                                                                  # the reference's loader: 8 worker processes
        sampler = Data.distributed.DistributedSampler(train_dataset, world, rank, shuffle=True) if world > 1 else None
        train_loader = Data.DataLoader(train_dataset, batch_size=per_rank_batch, num_workers=8,
                                       shuffle=sampler is None, sampler=sampler, pin_memory=True)
    valid_loader = None
    valid_on_device = resident is not None and valid_dataset is not None and len(valid_dataset) > 0   # made resident below, once
    if valid_dataset is not None:                                                                     # the objective is known
        if len(valid_dataset) > 0 and not valid_on_device:
            valid_loader = Data.DataLoader(valid_dataset, batch_size=max(args.batch_size // world, 1), num_workers=2,
                                           shuffle=False, pin_memory=True)
    else:
        print(f"Warning: validation folder {args.valid_folder} not found, validation is skipped.")   # train.py:199-200

    model = UNet().to(device)
    geometry = {"win_size": args.win_size, "hop_size": args.hop_size}
    model.stft_geometry = geometry                                        # model.save (the best-validation checkpoint) records it too
    start_epoch = 0
    scheduler = None
    resumed = os.path.exists(args.load_path)
    if os.path.exists(args.load_path):                                    # train.py:205-237
        model.load(args.load_path)
        checkpoint = torch.load(args.load_path, map_location=device)
        model.load_state_dict(checkpoint["model_state_dict"])
        if "optim" in checkpoint:
            model.optim.load_state_dict(checkpoint["optim"])
        start_epoch = checkpoint.get("epoch", 0)
        model.dropout_step = int(checkpoint.get("dropout_step", model.optim._step))      # Dropout2d masks continue, not replay
        for key in checkpoint:
            if key.startswith("loss_list"):
                setattr(model, key, checkpoint[key])
        print(f"Loaded checkpoint from {args.load_path}")
    if world > 1:
        from .parallel import GradAllReduce, broadcast_parameters
        broadcast_parameters(model, 0)
        grad_sync = GradAllReduce(model)
    # optimiser options (all off by default: FusedAdam.step is then the reference's Adam, one launch)
    model.optim.weight_decay, model.optim.max_grad_norm, model.optim.ema_decay = args.weight_decay, args.clip_grad_norm, args.ema_decay
    if args.ema_decay:
        if model._ema_flat is None:                                       # (after the broadcast: every rank starts the same average)
            model.start_ema()
            if resumed:
                print(f"{args.load_path} has no ema_state_dict: the EMA starts from the loaded weights.")
    elif model._ema_flat is not None:
        model._ema_flat = None
        print(f"{args.load_path} carries an EMA of the weights; without --ema_decay it is dropped.")
    # the rate: untouched (the optimiser's own, a checkpoint's included, and the epoch-400 rule) unless --lr or --warmup_steps
    target_lr = args.lr if args.lr is not None else (reference_lr(start_epoch) if args.warmup_steps else None)
    if target_lr is not None:
        for group in model.optim.param_groups:
            group["lr"] = warmup_lr(target_lr, model.optim._step + 1, args.warmup_steps)

    # objective: the reference's alpha_L1 * L1 + alpha_MR * MR-STFT (train.py:296) unless SVS_OBJECTIVE=l1 or no phases
    full = os.environ.get("SVS_OBJECTIVE", "full") != "l1"
    if full and not (resident.has_phase if resident is not None else train_dataset.has_phase_files()):
        print("Warning: no *_phase.npy files next to the spectrograms -- training on the L1 terms only.")
        full = False
    # the CPU-side datasets load phase files only when the objective needs them (and they exist): the L1-only fallback
    # holds for the validation loop and the SVS_DATA_LOADER=cpu path too, not just for the resident loader
    train_dataset.with_phase = full
    valid_resident = None
    if valid_loader is not None or valid_on_device:
        valid_dataset.with_phase = full and valid_dataset.has_phase_files()
        if full and not valid_dataset.with_phase:
            print("Warning: the validation set has no *_phase.npy files -- its loss is the L1 part only.")
        if valid_on_device:                                               # a second resident set (a few hundred MB); no DataLoader
            valid_resident = ResidentSpectrograms(valid_dataset, device, with_phase=valid_dataset.with_phase)
    alpha_mr = ALPHA_MR if full else 0.0
    print(f"Objective: {ALPHA_L1} * L1" + (f" + {ALPHA_MR} * MR-STFT (train.py:296)" if full else " (L1 terms only)"))
    if aug is not None:
        print(aug.describe())

    best_val_loss = 100.0
    log_buffer = []
    print(f"Start training for {args.epoch - start_epoch} epochs...")
    for ep in range(start_epoch, args.epoch):
        model.train()
        if sampler is not None:
            sampler.set_epoch(ep)
        if lr_drop_applies(ep, args.lr):                                   # train.py:251-262
            if target_lr is not None:
                target_lr = 5e-4
            for group in model.optim.param_groups:
                group["lr"] = 5e-4
            if rank == 0:
                torch.save({"epoch": ep + 1, "model_state_dict": model.state_dict(), "optim": model.optim.state_dict(),
                            "scheduler": None}, f"CKPT/svs_{args.label}_400.pth")
            print(f"\n[Info] Epoch {ep}: learning rate manually changed to 5e-4!\n")
        loss_sum = torch.zeros((), device=device)
        if resident is not None:
            steps = resident.num_batches(per_rank_batch, world)
            if aug is None:
                stream = resident.batches(per_rank_batch, True, rank, world, ep, with_phase=full)
            else:
                stream = resident.augmented_batches(per_rank_batch, rank, world, ep, with_phase=full, aug=aug, hop=args.hop_size)
        else:
            steps = len(train_loader)
            to_dev = lambda t: t.to(device, non_blocking=True)
            stream = ((to_dev(m), to_dev(v)) + ((to_dev(a), to_dev(b)) if full else ()) for m, v, a, b in train_loader)
        for batch in stream:
            mix, voc = batch[0], batch[1]
            mph, vph = (batch[2], batch[3]) if full else (None, None)
            if args.warmup_steps:                                          # a double argument of the launch: nothing goes to the device
                for group in model.optim.param_groups:
                    group["lr"] = warmup_lr(target_lr, model.optim._step + 1, args.warmup_steps)
            l1 = model.train_step(mix, voc, loss_scale=ALPHA_L1, grad_sync=grad_sync, mix_phase=mph, voc_phase=vph,
                                  alpha_mr=alpha_mr, hop=args.hop_size)                     # train.py:271-300
            loss_sum += ALPHA_L1 * l1                                                       # no host sync per step
            if model.last_mr_loss is not None:
                loss_sum += alpha_mr * model.last_mr_loss
        avg_train_loss = float(loss_sum) / max(steps, 1)
        log_buffer.append(f"{avg_train_loss}\n")
        if optim_options:                                                  # the epoch's one read-back of the optimiser's device scalars
            norm, _, clipped, skipped = model.optim_stats.cpu().tolist()
            model.optim_stats[2:].zero_()
            if rank == 0:
                print(f"Epoch {ep + 1} last grad norm {norm:.4e} | clipped {int(clipped)} / {steps} steps | skipped (non-finite) {int(skipped)}")

        if world > 1:                                                      # one set of running statistics for validation / checkpoints
            from .parallel import average_bn_buffers
            average_bn_buffers(model)
        if (valid_loader or valid_resident is not None) and (ep + 1) % args.val_interval == 0:             # train.py:317-363
            model.eval()
            # --ema_decay: the pass and the best checkpoint see the EMA weights (model.save inside the context writes them as
            # model_state_dict, so every downstream tool loads them unchanged)
            with model.ema_weights() if args.ema_decay else contextlib.nullcontext():
                if valid_resident is not None:                             # on the device: one library call per batch, one read-back
                    with torch.no_grad():
                        acc, n_val = validation_pass(model, valid_resident, max(args.batch_size // world, 1),
                                                     valid_dataset.with_phase and valid_resident.has_phase, args.win_size, args.hop_size)
                    avg_val_loss = float(acc.cpu()[0]) / n_val
                else:                                                      # SVS_DATA_LOADER != resident: the reference's host loop
                    val_sum = 0.0
                    with torch.no_grad():
                        for mix, voc, mph, vph in valid_loader:
                            mix, voc = mix.to(device), voc.to(device)
                            val_sum += ALPHA_L1 * float(l1_terms(model, mix, voc))
                            if full and valid_dataset.with_phase:          # train.py:341-346
                                val_sum += alpha_mr * float(mr_term(model, mix, voc, mph.to(device), vph.to(device), args.win_size, args.hop_size))
                    avg_val_loss = val_sum / len(valid_loader)
                log_buffer.append(f"Val {avg_val_loss}\n")
                print(f"\n[Epoch {ep + 1}] Train Loss: {avg_train_loss:.4e} | Val Loss: {avg_val_loss:.4e}")
                if avg_val_loss < best_val_loss and rank == 0:
                    best_val_loss = avg_val_loss
                    model.save(best_weight)
            if rank == 0:
                try:
                    with open(log_file, "a") as f:
                        f.writelines(log_buffer)
                    log_buffer = []
                except Exception as e:
                    print(f"Log write failed: {e}")
        else:
            print(f"Epoch {ep + 1} Avg Loss: {avg_train_loss:.4e}")

        if rank == 0:                                                      # train.py:369-382
            checkpoint = {"epoch": ep + 1, "model_state_dict": model.state_dict(), "optim": model.optim.state_dict(),
                          "scheduler": scheduler.state_dict() if scheduler is not None else None,
                          "dropout_step": model.dropout_step, **geometry}
            if args.ema_decay:                                             # the live weights above, the average beside them
                checkpoint["ema_state_dict"] = model.ema_state_dict()
                checkpoint["ema_decay"] = args.ema_decay
            for key in model.__dict__:
                if key.startswith("loss_list"):
                    checkpoint[key] = getattr(model, key)
            torch.save(checkpoint, ckpt_weight)

    if log_buffer and rank == 0:
        with open(log_file, "a") as f:
            f.writelines(log_buffer)
    print("Finish training!")
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
