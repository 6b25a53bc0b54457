"""Smoothing the pitch track, the host half (no GPU): the declarations, every argument rule of the new entry points
before any launch, the candidate rule on hand-made d' rows, the decode against exhaustive enumeration of all 8^T paths, a chunked (min,+)
formulation of it -- the one csrc/f0_smooth.hip runs -- against the sequential recursion for every allowed chunk, the value claim on a
gliding tone in white noise at 6 dB, and the command lines on the CPU.

The value claim's bounds are the issue's: raw RPA <= 0.75 (the raw tracker's octave flips are there to be removed) and, smoothed,
RPA >= 0.95, VR >= 0.95, VFA <= 0.10.  Measured with the definition on the CPU, seeds 0..3: raw RPA 0.584 - 0.618, smoothed RPA 1.0,
VR 0.996 - 1.0, VFA 0.0."""
import functools
import itertools

import numpy as np
import pytest

from svs_unet_pytorch_amd import _lib
from svs_unet_pytorch_amd import f0 as f0m

NAMES = ("svs_f0_dips", "svs_f0_candidates", "svs_f0_viterbi_workspace", "svs_f0_viterbi", "svs_f0_smooth_select")
SR = 8192


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def err(lib):
    return lib.svs_last_error_string().decode()


def test_symbols_are_declared_bound_and_exported(lib):
    syms = _lib.header_symbols()
    for name in NAMES:
        assert name in syms and name in _lib._SIGS and hasattr(lib, name), name


# ------------------------------------------------------------------------------------------------
# argument rules, before any launch
# ------------------------------------------------------------------------------------------------
# svs_f0_viterbi(cand_tau, cand_ap, count, rms, rows, n_frames, cents, tau_min, tau_max, rms_gate, pitch, switch, unvoiced, octave, chunk,
#                workspace, state, cost)
VIT = dict(cand_tau=64, cand_ap=64, count=64, rms=64, rows=2, n_frames=100, cents=64, tau_min=8, tau_max=127, rms_gate=0.0, pitch_cost=4,
           switch_cost=1024, unvoiced_cost=2048, octave_cost=82, chunk=64, workspace=64, state=64, cost=64)


def viterbi_call(lib, **change):
    a = {**VIT, **change}
    return lib.svs_f0_viterbi(*(a[k] for k in VIT), None)


@pytest.mark.parametrize("change,msg", [
    (dict(rows=0), "rows must be in 1..64"),
    (dict(rows=65), "rows must be in 1..64"),
    (dict(n_frames=-1), "n_frames must be in 0..2^20"),
    (dict(n_frames=(1 << 20) + 1), "n_frames must be in 0..2^20"),
    (dict(chunk=0), "chunk must be 16, 32, 64 or 128"),
    (dict(chunk=48), "chunk must be 16, 32, 64 or 128"),
    (dict(chunk=256), "chunk must be 16, 32, 64 or 128"),
    (dict(tau_max=2049), "tau_max must be in 1..2048"),
    (dict(tau_min=0), "tau_min must be in 1..tau_max - 1"),
    (dict(tau_min=127), "tau_min must be in 1..tau_max - 1"),
    (dict(rms_gate=-1.0), "rms_gate must be finite and not negative"),
    (dict(rms_gate=float("inf")), "rms_gate must be finite and not negative"),
    (dict(pitch_cost=-1), "pitch_cost must be in 0..2^20"),
    (dict(pitch_cost=(1 << 20) + 1), "pitch_cost must be in 0..2^20"),
    (dict(switch_cost=-1), "switch_cost must be in 0..2^20"),
    (dict(switch_cost=(1 << 20) + 1), "switch_cost must be in 0..2^20"),
    (dict(unvoiced_cost=-1), "unvoiced_cost must be in 0..2^20"),
    (dict(unvoiced_cost=1 << 21), "unvoiced_cost must be in 0..2^20"),
    (dict(octave_cost=-5), "octave_cost must be in 0..2^20"),
    (dict(octave_cost=1 << 40), "octave_cost must be in 0..2^20"),
    (dict(cand_tau=None), "null pointer"),
    (dict(cents=None), "null pointer"),
    (dict(workspace=None), "null pointer"),
    (dict(state=None), "null pointer"),
    (dict(cost=None), "null pointer"),
    (dict(cand_ap=66), "4-byte aligned"),
    (dict(state=66), "4-byte aligned"),
    (dict(cost=68), "cost must be 8-byte aligned"),
    (dict(workspace=72), "workspace must be 16-byte aligned"),
])
def test_viterbi_refuses_before_any_launch(lib, change, msg):
    assert viterbi_call(lib, **change) == -1
    assert msg in err(lib) and err(lib).startswith("svs_f0_viterbi:"), err(lib)


def test_viterbi_workspace(lib):
    assert lib.svs_f0_viterbi_workspace(1, 100, 48) == 0 and "chunk must be 16, 32, 64 or 128" in err(lib)
    assert lib.svs_f0_viterbi_workspace(0, 100, 64) == 0 and err(lib).startswith("svs_f0_viterbi_workspace: rows must be in 1..64")
    assert lib.svs_f0_viterbi_workspace(1, (1 << 20) + 1, 64) == 0 and "n_frames must be in 0..2^20" in err(lib)
    small, large = lib.svs_f0_viterbi_workspace(1, 100, 64), lib.svs_f0_viterbi_workspace(64, 1 << 20, 16)
    assert small >= 2 * 64 * 8 + 100 * 4 and small % 16 == 0         # two chunk products and a psi word per frame at the least
    assert large >= 64 * (1 << 16) * 64 * 8                          # 2 GiB of chunk products: size_t, not int


# svs_f0_candidates(x, rows, n, ld_row, W, tau_min, tau_max, hop, first_frame, n_frames, threshold, rms_gate, sr, f0, ap, rms, voiced,
#                   cand_tau, cand_f0, cand_ap, count)
CAND = dict(x=64, rows=2, n=1000, ld_row=1000, W=252, tau_min=8, tau_max=127, hop=82, first_frame=0, n_frames=8, threshold=0.15, rms_gate=0.0,
            sr=8192.0, f0=64, ap=64, rms=64, voiced=64, cand_tau=64, cand_f0=64, cand_ap=64, count=64)


@pytest.mark.parametrize("change,msg", [
    (dict(rows=65), "rows must be in 1..64"),
    (dict(W=0), "W must be in 1..4096"),
    (dict(tau_max=2049, n=10000, ld_row=10000), "tau_max must be in 1..2048"),
    (dict(tau_min=127), "tau_min must be in 1..tau_max - 1"),
    (dict(hop=0), "hop must be at least 1"),
    (dict(first_frame=-1), "must not be negative"),
    (dict(n=-1), "n must not be negative"),
    (dict(n_frames=9), "only whole frames are formed"),
    (dict(ld_row=999), "ld_row must be at least n"),
    (dict(threshold=0.0), "threshold must be positive and finite"),
    (dict(rms_gate=-1.0), "rms_gate must be finite and not negative"),
    (dict(sr=0.0), "sr must be positive and finite"),
    (dict(x=None), "null pointer"),
    (dict(voiced=None), "null pointer"),
    (dict(cand_tau=None), "null pointer"),
    (dict(count=None), "null pointer"),
    (dict(x=66), "x must be 4-byte aligned"),
    (dict(cand_f0=66), "4-byte aligned"),
])
def test_candidates_refuses_before_any_launch(lib, change, msg):
    a = {**CAND, **change}
    assert lib.svs_f0_candidates(*(a[k] for k in CAND), None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_f0_candidates:"), err(lib)


# svs_f0_dips(dprime, count, tau_min, tau_max, sr, cand_tau, cand_f0, cand_ap, cand_count)
@pytest.mark.parametrize("args,msg", [
    ((64, 10, 8, 2049, 8192.0, 64, 64, 64, 64), "tau_max must be in 1..2048"),
    ((64, 10, 127, 127, 8192.0, 64, 64, 64, 64), "tau_min must be in 1..tau_max - 1"),
    ((64, 10, 8, 127, -1.0, 64, 64, 64, 64), "sr must be positive and finite"),
    ((64, -1, 8, 127, 8192.0, 64, 64, 64, 64), "frame count must not be negative"),
    ((None, 10, 8, 127, 8192.0, 64, 64, 64, 64), "null pointer"),
    ((64, 10, 8, 127, 8192.0, 64, 64, 64, None), "null pointer"),
    ((64, 10, 8, 127, 8192.0, 64, 66, 64, 64), "4-byte aligned"),
])
def test_dips_refuses_before_any_launch(lib, args, msg):
    assert lib.svs_f0_dips(*args, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_f0_dips:"), err(lib)


# svs_f0_smooth_select(state, cand_f0, cand_ap, raw_f0, raw_ap, count, f0, ap, voiced)
@pytest.mark.parametrize("args,msg", [
    ((64, 64, 64, 64, 64, -1, 64, 64, 64), "frame count must be in 0..2^26"),
    ((64, 64, 64, 64, 64, (1 << 26) + 1, 64, 64, 64), "frame count must be in 0..2^26"),
    ((None, 64, 64, 64, 64, 10, 64, 64, 64), "null pointer"),
    ((64, 64, 64, 64, 64, 10, 64, 64, None), "null pointer"),
    ((64, 64, 66, 64, 64, 10, 64, 64, 64), "4-byte aligned"),
])
def test_select_refuses_before_any_launch(lib, args, msg):
    assert lib.svs_f0_smooth_select(*args, None) == -1
    assert msg in err(lib) and err(lib).startswith("svs_f0_smooth_select:"), err(lib)


def test_no_frames_launch_nothing(lib):
    assert viterbi_call(lib, n_frames=0, cand_tau=None, cand_ap=None, count=None, rms=None, cents=None, workspace=None, state=None, cost=None) == 0
    assert lib.svs_f0_dips(None, 0, 8, 127, 8192.0, None, None, None, None, None) == 0
    assert lib.svs_f0_smooth_select(None, None, None, None, None, 0, None, None, None, None) == 0
    a = {**CAND, **dict(n_frames=0, x=None, f0=None, ap=None, rms=None, voiced=None, cand_tau=None, cand_f0=None, cand_ap=None, count=None)}
    assert lib.svs_f0_candidates(*(a[k] for k in CAND), None) == 0


def test_python_entry_points_check_before_any_device_work(tmp_path, capsys):
    import torch
    from svs_unet_pytorch_amd import evaluate, separate, streaming
    assert f0m.check_costs(True) == f0m.COSTS == {"pitch_cost": 4, "switch_cost": 1024, "unvoiced_cost": 2048, "octave_cost": 82}
    assert f0m.check_costs({"octave_cost": 0}) == {**f0m.COSTS, "octave_cost": 0}
    for name in f0m.COSTS:
        for bad in (-1, (1 << 20) + 1, 1.5):
            with pytest.raises(ValueError, match=f"{name} must be a whole number in 0..2\\^20"):
                f0m.check_costs({name: bad})
    with pytest.raises(ValueError, match="not \\['chunk'\\]"):
        f0m.check_costs({"chunk": 16})
    assert f0m.check_options({"smooth": True}) == {"smooth": True} and f0m.check_options({"smooth": None}) == {"smooth": None}
    with pytest.raises(ValueError, match="pitch_cost must be"):
        f0m.check_options({"smooth": {"pitch_cost": -3}})
    with pytest.raises(ValueError, match="switch_cost must be"):
        f0m.track_gpu(torch.zeros(8), 8192, smooth={"switch_cost": 1 << 21})               # before the tensor is looked at
    with pytest.raises(ValueError, match="device tensor"):
        f0m.track_gpu(torch.zeros(800), 8192, smooth=True)
    with pytest.raises(ValueError, match="device tensor"):
        f0m.candidates_gpu(torch.zeros(800), 8192)
    with pytest.raises(TypeError, match="float32 device tensor"):
        f0m.dips_gpu(torch.zeros(4, 128), 8192, 8)
    with pytest.raises(ValueError, match="chunk must be one of"):
        f0m.viterbi_gpu(None, None, None, None, None, 8, chunk=48)
    with pytest.raises(ValueError, match="unvoiced_cost must be"):
        streaming.separate_to_wav(None, "unused.wav", "unused_out.wav", f0={"smooth": {"unvoiced_cost": -1}})
    with pytest.raises(SystemExit) as e:
        separate.main(["--model_path", "none.pth", "--src", "a.wav", "--tar", "o.wav", "--f0_smooth"])
    assert e.value.code == 2 and "--f0_smooth belongs to --f0_csv" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--est", "e", "--mix", "m", "--ref", "r", "--f0_smooth"])
    assert e.value.code == 2 and "--f0_smooth belongs to --melody" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        f0m.main(["--src", "a.wav", "--csv", "a.csv", "--device", "cpu", "--pitch_cost", "3"])
    assert e.value.code == 2 and "--pitch_cost belongs to --smooth" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        f0m.main(["--src", "a.wav", "--csv", "a.csv", "--device", "cpu", "--smooth", "--octave_cost", "-1"])
    assert e.value.code == 2 and "octave_cost must be a whole number" in capsys.readouterr().err
    for tool in (separate, evaluate):
        with pytest.raises(SystemExit) as e:
            tool.main(["--help"])
        assert e.value.code == 0 and "--f0_smooth" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------
# candidates
# ------------------------------------------------------------------------------------------------
HAND_TAU_MIN, HAND_TAU_MAX = 5, 300                                  # wider than one pass of the wave


def hand_made_rows():
    """(rows float32 (7, 301), the expected taus per row, by hand).  Everything not set is 1, so tau_min = 5 is a dip of depth 1 in
    every row that leaves it alone (1 <= 1 on its right), and no other lag of a flat stretch is one (nothing is < its left neighbour)."""
    rows = np.ones((7, HAND_TAU_MAX + 1), np.float32)
    # 0: ten dips, seven kept by depth (.05 .1 .2 .3 .4 .5 .6), written in ascending tau; .7, .8 and the 1 at tau_min are dropped
    for tau, v in {10: .5, 50: .1, 90: .4, 130: .2, 170: .6, 210: .3, 250: .7, 290: .8, 299: .05}.items():
        rows[0, tau] = v
    # 1: nine dips of one depth, 64 and 128 lags apart among them: the seven smallest taus
    rows[1, [20, 84, 148, 212, 276, 40, 104, 168, 232]] = 0.25
    # 2: plateaus -- 100..103 at .2 is ONE dip at 100 (<= on the right, < on the left); 200, 201 at .5 then 202, 203 at .3: dips at 200 and 202
    rows[2, 100:104] = 0.2
    rows[2, 200:204] = [0.5, 0.5, 0.3, 0.3]
    # 3: dips at tau_min and at tau_max
    rows[3, 5], rows[3, 300] = 0.1, 0.2
    # 4: a constant row: count 1 at tau_min
    rows[4] = 0.7
    # 5: strictly falling: the only dip is tau_max; 6: strictly rising: the only dip is tau_min
    rows[5] = np.linspace(2.0, 0.1, HAND_TAU_MAX + 1)
    rows[6] = np.linspace(0.1, 2.0, HAND_TAU_MAX + 1)
    want = [[10, 50, 90, 130, 170, 210, 299], [20, 40, 84, 104, 148, 168, 212], [5, 100, 200, 202], [5, 300], [5], [300], [5]]
    return rows, want


def test_candidates_on_hand_made_rows():
    rows, want = hand_made_rows()
    tau, f0, ap, count = f0m.candidates_reference(rows, 8192.0, HAND_TAU_MIN, HAND_TAU_MAX)
    assert tau.dtype == count.dtype == np.int32 and f0.dtype == ap.dtype == np.float32 and tau.shape == f0.shape == ap.shape == (7, 7)
    assert count.tolist() == [len(w) for w in want]
    for r, w in enumerate(want):
        assert tau[r, :len(w)].tolist() == w and np.array_equal(ap[r, :len(w)], rows[r, w])
        assert (tau[r, len(w):] == 0).all() and (f0[r, len(w):] == 0).all() and (ap[r, len(w):] == 0).all()          # the empty slots
    # the parabola is the pick's: row 0's dip at 10 has a = c = 1: delta 0; the plateau at 100 has a = 1, b = c = .2: delta 0.5
    assert f0[0, 0] == np.float32(8192.0 / 10) and f0[2, 1] == np.float32(8192.0 / 100.5)
    assert f0[3, 0] == np.float32(8192.0 / 5) and f0[3, 1] == np.float32(8192.0 / 300)       # tau_max has no tau + 1: delta 0
    # one frame's deepest dip is the raw pick's lag wherever nothing lies under the threshold
    pick_tau = f0m.pick_reference(rows, 8192.0, HAND_TAU_MIN, HAND_TAU_MAX, 0.01)[3]
    assert all(int(pick_tau[r]) in tau[r, :count[r]].tolist() for r in range(7))
    with pytest.raises(ValueError, match="tau_max \\+ 1"):
        f0m.candidates_reference(rows, 8192.0, 5, 301)


def test_cents_table():
    c = f0m.cents_table(8192, 127)
    assert c.dtype == np.int32 and c.shape == (128,) and c[0] == 0 and c[1] == 15600 and c[2] == 14400 and c[64] - c[128 - 1] in (1186, 1187)
    assert (np.diff(c[1:]) <= 0).all()


# ------------------------------------------------------------------------------------------------
# the decode
# ------------------------------------------------------------------------------------------------
def brute_force(obs, A):
    """All 8^T paths: the cheapest, and among equals the one with the smallest last state, then the smallest state before it, and so on --
    what 'the smallest j that attains the minimum' and 'the smallest i that attains it' choose."""
    T, S = obs.shape
    best = None
    for path in itertools.product(range(S), repeat=T):
        cost = int(obs[0, path[0]]) + sum(int(A[t, path[t - 1], path[t]]) + int(obs[t, path[t]]) for t in range(1, T))
        key = (cost, path[::-1])
        if best is None or key < best:
            best = key
    return np.array(best[1][::-1], np.int32), best[0]


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_decode_is_exhaustive_enumeration(T):
    rng = np.random.default_rng(T)
    for high in (1, 2, 4, 1000):                                      # high = 1: every cost equal (zero) -- the tie rules alone
        obs, A = rng.integers(0, high, (T, 8)), rng.integers(0, high, (T, 8, 8))
        state, cost = f0m.viterbi_decode(obs, A)
        want, want_cost = brute_force(obs, A)
        assert state.tolist() == want.tolist() and cost == want_cost, (T, high)
        if high == 1:
            assert cost == 0 and (state == 0).all()


def test_decode_is_exhaustive_enumeration_five_frames():
    rng = np.random.default_rng(5)
    obs, A = rng.integers(0, 3, (5, 8)), rng.integers(0, 3, (5, 8, 8))
    state, cost = f0m.viterbi_decode(obs, A)
    want, want_cost = brute_force(obs, A)
    assert state.tolist() == want.tolist() and cost == want_cost
    ones = f0m.viterbi_decode(np.full((5, 8), 7), np.full((5, 8, 8), 7))
    assert ones[0].tolist() == [0] * 5 and ones[1] == 5 * 7 + 4 * 7  # all equal and not zero


def synthetic_candidates(rows, T, seed, tau_min=8, tau_max=127, ap_zero=False):
    """Random candidate buffers as svs_f0_candidates leaves them: count in 1..7, ascending distinct taus in the live slots and zeros in
    the empty ones, ap in [0, 1.5), an rms below the gate (0.5) on about one frame in five -- in runs, so that whole chunks are gated.
    The taus are a slow random walk plus seven of ten fixed offsets, so that consecutive frames hold lags a few cents apart and the
    cheapest path is voiced, unvoiced and changes slot often (random lags alone would leave it unvoiced nearly everywhere)."""
    rng = np.random.default_rng(seed)
    count = rng.integers(1, f0m.K + 1, (rows, T)).astype(np.int32)
    base = np.clip(tau_min + 4 + np.abs(np.cumsum(rng.integers(-1, 2, (rows, T)), axis=1)) % 48, tau_min, tau_max - 56)
    offsets = np.array([0, 1, 2, 3, 5, 8, 13, 21, 34, 55])
    pick = np.sort(np.argsort(rng.random((rows, T, offsets.size)), axis=-1)[..., :f0m.K], axis=-1)
    tau = (base[..., None] + offsets[pick]).astype(np.int32)
    assert tau.min() >= tau_min and tau.max() <= tau_max
    live = np.arange(f0m.K) < count[..., None]
    ap = np.zeros((rows, T, f0m.K), np.float32) if ap_zero else rng.random((rows, T, f0m.K)).astype(np.float32) * np.float32(1.5)
    gated = np.repeat(rng.random((rows, -(-T // 40))) < 0.2, 40, axis=1)[:, :T]
    rms = np.where(gated, 0.1, 0.9).astype(np.float32)
    return np.where(live, tau, 0).astype(np.int32), np.where(live, ap, 0).astype(np.float32), count, rms


def minplus(a, b):
    return (a[:, :, None] + b[None, :, :]).min(axis=1)


def chunked_decode(obs, A, chunk):
    """The decode as csrc/f0_smooth.hip runs it: chunk products, a scan over them, a rerun per chunk, composed psi tables, a walk over the
    tables, a backtrace per chunk.  int64 throughout, no saturation."""
    T, S = obs.shape
    M = A + obs[:, None, :]                                           # A[0] is zero: frame 0 from an all-zero vector is obs_0
    starts = list(range(0, T, chunk))
    prods = []
    for s in starts:                                                  # (a)
        P = M[s]
        for t in range(s + 1, min(s + chunk, T)):
            P = minplus(P, M[t])
        prods.append(P)
    entry, delta = [], np.zeros(S, np.int64)
    for P in prods:                                                   # (b)
        entry.append(delta)
        delta = (delta[:, None] + P).min(axis=0)
    cost, last = int(delta.min()), int(np.argmin(delta))
    psi = np.zeros((T, S), np.int64)
    tables = []
    for s, d in zip(starts, entry):                                   # (c), (d)
        e = min(s + chunk, T)
        for t in range(s, e):
            through = d[:, None] + A[t]
            psi[t] = np.argmin(through, axis=0)
            d = through.min(axis=0) + obs[t]
        table = np.arange(S)
        for t in range(e - 1, max(s, 1) - 1, -1):
            table = psi[t][table]
        tables.append(table)
    ends = [0] * len(starts)                                          # (e)
    st = last
    for c in range(len(starts) - 1, -1, -1):
        ends[c] = st
        st = tables[c][st]
    state = np.zeros(T, np.int32)                                     # (f)
    for c, s in enumerate(starts):
        st = ends[c]
        for t in range(min(s + chunk, T) - 1, s - 1, -1):
            state[t] = st
            st = psi[t][st]
    return state, cost


@pytest.mark.parametrize("chunk", f0m.CHUNKS)
def test_chunked_decode_is_the_sequential_one(chunk):
    cents = f0m.cents_table(SR, 127)
    for T in (1, 2, chunk - 1, chunk, chunk + 1, 3 * chunk + 5):
        for seed, costs, ap_zero in ((T, {}, False), (T + 1, dict.fromkeys(f0m.COSTS, 0), True)):
            tau, ap, count, rms = synthetic_candidates(1, T, seed, ap_zero=ap_zero)
            obs, A = f0m.viterbi_costs(tau[0], ap[0], count[0], rms[0], cents, 8, 0.5, **costs)
            want, want_cost = f0m.viterbi_decode(obs, A)
            got, got_cost = chunked_decode(obs, A, chunk)
            assert got.tolist() == want.tolist() and got_cost == want_cost, (chunk, T, costs)
            assert (obs[rms[0] < 0.5, :7] == f0m.INF).all() and (obs[:, 7] == (0 if costs else 2048)).all()


def test_costs_follow_the_definition():
    cents = f0m.cents_table(SR, 127)
    tau = np.array([[8, 16, 0, 0, 0, 0, 0], [8, 32, 64, 0, 0, 0, 0]], np.int32)
    ap = np.array([[0.5, 0.25, 0, 0, 0, 0, 0], [2.5 / 4096, 3.5 / 4096, 1.0, 0, 0, 0, 0]], np.float32)
    obs, A = f0m.viterbi_costs(tau, ap, np.array([2, 3]), np.array([1.0, 1.0], np.float32), cents, 8, 0.5)
    assert obs[0].tolist() == [2048, 1024 + 82] + [f0m.INF] * 5 + [2048]                 # one octave of lag: 82
    assert obs[1].tolist() == [2, 4 + 164, 4096 + 246] + [f0m.INF] * 4 + [2048]          # 2.5 -> 2, 3.5 -> 4: half to even
    assert A[1, 0, 0] == 0 and A[1, 1, 0] == 4 * 1200 and A[1, 1, 2] == 4 * 2400 and A[1, 2, 0] == 4 * int(cents[8])       # cents[0] = 0
    assert A[1, 0, 7] == A[1, 7, 3] == 1024 and A[1, 7, 7] == 0 and (A[0] == 0).all()
    gated = f0m.viterbi_costs(tau, ap, np.array([2, 3]), np.array([0.4, 0.5], np.float32), cents, 8, 0.5)[0]
    assert (gated[0, :7] == f0m.INF).all() and gated[1, 0] == 2       # the gate's own level passes
    state, cost = f0m.viterbi_reference(tau, ap, np.array([2, 3]), np.array([1.0, 1.0], np.float32), cents, 8, 0.5)
    assert state.tolist() == [0, 0] and cost == 2048 + 0 + 2          # the lag-8 candidates, no pitch step between them
    with pytest.raises(ValueError, match="outside the cents table"):
        f0m.viterbi_costs(np.full((1, 7), 128), np.zeros((1, 7)), np.array([1]), np.ones(1), cents, 8)


# ------------------------------------------------------------------------------------------------
# the value claim
# ------------------------------------------------------------------------------------------------
VALUE_GEOMETRY = dict(fmin=100, fmax=800, hop=82)                    # 297 frames of 3 s at 8,192 Hz


@functools.lru_cache(maxsize=None)
def noisy_tone(seed, snr_db=6.0):
    """(x float32, the reference pitch and voicing per frame): a harmonic tone gliding 160 -> 320 -> 200 Hz with a 5.5 Hz vibrato, silent
    on [1.2 s, 1.5 s), in white noise snr_db under the tone's own level.  Computed once per seed and left unchanged."""
    n = 3 * SR
    i = np.arange(n)
    freq = np.concatenate([np.linspace(160, 320, n // 2), np.linspace(320, 200, n - n // 2)]) * (1 + 0.01 * np.sin(2 * np.pi * 5.5 * i / SR))
    clean = f0m.harmonic_tone(freq, SR)
    env = np.ones(n, np.float32)
    env[int(1.2 * SR):int(1.5 * SR)] = 0.0
    noise = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    snr = 10.0 ** (snr_db / 10.0)
    noise = noise * np.float32(np.sqrt(np.mean(clean.astype(np.float64) ** 2) / (snr * np.mean(noise.astype(np.float64) ** 2))))
    x = (clean * env + noise).astype(np.float32)
    g = f0m.geometry(SR, **VALUE_GEOMETRY)
    frames = f0m.frame_count(n, g.span, g.hop)
    assert frames == 297
    at = np.arange(frames) * g.hop + g.span // 2
    x.setflags(write=False)
    return x, freq[at], env[at] > 0


def value_bounds(ref_f0, ref_voiced, raw, smooth, what):
    """The issue's assertion on a raw and a smoothed (f0, voiced) pair; prints the figures first."""
    m_raw, m = f0m.melody_metrics(ref_f0, ref_voiced, *raw), f0m.melody_metrics(ref_f0, ref_voiced, *smooth)
    print(f"{what}: raw " + " ".join(f"{k}={v:.3f}" for k, v in m_raw.items()) + "; smoothed " + " ".join(f"{k}={v:.3f}" for k, v in m.items()))
    assert m_raw["RPA"] <= 0.75
    assert m["RPA"] >= 0.95 and m["VR"] >= 0.95 and m["VFA"] <= 0.10
    return m_raw, m


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_smoothing_removes_the_octave_errors_at_6_db(seed):
    x, ref_f0, ref_voiced = noisy_tone(seed)
    raw, dp = f0m.yin_reference(x, SR, **VALUE_GEOMETRY)
    g = f0m.geometry(SR, **VALUE_GEOMETRY)
    f0, ap, voiced, state, cost = f0m.smooth_reference(dp, raw.rms, g.sr, g.tau_min, g.tau_max, g.threshold, g.rms_gate)
    value_bounds(ref_f0, ref_voiced, (raw.f0, raw.voiced), (f0, voiced), f"6 dB, seed {seed}")
    assert np.array_equal(voiced, (state < 7).astype(np.int32)) and f0.dtype == ap.dtype == np.float32
    assert np.array_equal(f0[state == 7], raw.f0[state == 7]) and np.array_equal(ap[state == 7], raw.ap[state == 7])     # the raw pick's
    smoothed = f0m.yin_reference(x, SR, smooth=True, **VALUE_GEOMETRY)[0]                 # the same through the one-call interface
    assert np.array_equal(smoothed.f0, f0) and np.array_equal(smoothed.voiced, voiced) and np.array_equal(smoothed.rms, raw.rms)
    assert np.array_equal(f0m.yin_reference(x, SR, smooth=None, **VALUE_GEOMETRY)[0].f0, raw.f0)


# ------------------------------------------------------------------------------------------------
# the command lines on the CPU
# ------------------------------------------------------------------------------------------------
def test_cli_on_the_cpu(tmp_path, capsys):
    from scipy.io import wavfile
    x, ref_f0, ref_voiced = noisy_tone(0)
    src = str(tmp_path / "noisy.wav")
    wavfile.write(src, SR, np.array(x))
    raw_csv, smooth_csv, cheap_csv = (str(tmp_path / n) for n in ("raw.csv", "smooth.csv", "cheap.csv"))
    args = ["--src", src, "--device", "cpu", "--fmin", "100", "--fmax", "800", "--hop", "82"]
    f0m.main(args + ["--csv", raw_csv])
    f0m.main(args + ["--csv", smooth_csv, "--smooth"])
    f0m.main(args + ["--csv", cheap_csv, "--smooth", "--unvoiced_cost", "0", "--switch_cost", "0"])
    said = capsys.readouterr().out
    assert f"{raw_csv}: 297 frames" in said and f"{smooth_csv}: 297 frames" in said

    def cols(path):
        lines = open(path).read().splitlines()
        assert lines[0] == f0m.CSV_HEADER and len(lines) == 298
        return np.array([[float(v) for v in line.split(",")] for line in lines[1:]])
    raw, smooth, cheap = cols(raw_csv), cols(smooth_csv), cols(cheap_csv)
    want = f0m.yin_reference(x, SR, smooth=True, **VALUE_GEOMETRY)[0]
    assert np.array_equal(smooth[:, 2], want.voiced) and np.allclose(smooth[:, 1], want.f0, rtol=0, atol=1e-4)
    assert np.array_equal(raw[:, [0, 4]], smooth[:, [0, 4]])          # time and rms are unchanged
    assert smooth[:, 2].sum() > 200 > raw[:, 2].sum() and cheap[:, 2].sum() == 0          # a free unvoiced state takes every frame


def test_evaluate_melody_smoothed_on_the_cpu(tmp_path, capsys):
    from scipy.io import wavfile

    from svs_unet_pytorch_amd import evaluate
    x, _, _ = noisy_tone(0)
    clean, _, _ = noisy_tone(0, 40.0)
    for folder, y in (("ref", clean), ("est", x), ("mix", x)):
        (tmp_path / folder).mkdir()
        wavfile.write(str(tmp_path / folder / "song.wav"), SR, np.array(y))
    base = ["--est", str(tmp_path / "est"), "--mix", str(tmp_path / "mix"), "--ref", str(tmp_path / "ref"), "--melody"]
    plain = evaluate.main(base)[0]
    smooth = evaluate.main(base + ["--f0_smooth"])[0]
    said = capsys.readouterr().out
    assert all(f"{k}={smooth[k]:.3f}" in said and f"Mean {k:4s}: {smooth[k]:.3f}" in said for k in f0m.MELODY)
    gate = f0m.gate_from_db(f0m.MELODY_GATE_DB)
    tr, te = (f0m.yin_reference(np.array(y), SR, rms_gate=gate, smooth=True)[0] for y in (clean, x))
    assert {k: smooth[k] for k in f0m.MELODY} == f0m.melody_metrics(tr.f0, tr.voiced, te.f0, te.voiced)
    print(plain, smooth)
    assert smooth["OA"] > plain["OA"] and smooth["RPA"] >= plain["RPA"]
