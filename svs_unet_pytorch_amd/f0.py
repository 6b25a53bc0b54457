"""Fundamental frequency of a (separated) voice: the YIN tracker, steps 1 to 5 of de Cheveigne & Kawahara (JASA 2002) -- the float64
definition (numpy), the device path on csrc/f0.hip (include/svs_hip.h), the frame-level melody measures of the
MIREX melody task, and a command line.  The reference has no pitch estimator; pitch.py / csrc/pitch.hip SHIFT pitch for training.

    python -m svs_unet_pytorch_amd.f0 --src song.wav|folder --csv out.csv|folder [--fmin 65] [--fmax 1000] [--window W] [--hop H] \
        [--threshold 0.15] [--rms_gate_db DB] [--device gpu|cpu] [--smooth [--pitch_cost 4] [--switch_cost 1024] [--unvoiced_cost 2048] \
        [--octave_cost 82]]

Geometry, from sr, fmin, fmax, W (the integration window in samples, default 2 tau_max), hop (default round(sr / 100), at least 1):
    tau_min = max(2, floor(sr / fmax)),  tau_max = ceil(sr / fmin),  span = W + tau_max,  frames = 1 + (n - span) // hop
Only whole frames are formed, nothing is zero-padded, and n < span is an error.  Limits (the kernel's, checked before any launch):
1 <= W <= 4096, tau_min < tau_max <= 2048, hop >= 1, 1 <= rows <= 64.

Frame i of a row starts at sample t = i hop:
    d(tau)  = sum_{j=0..W-1} (float64(float32(x[t+j] - x[t+j+tau])))^2,  tau = 0..tau_max     (the difference is ONE float32 subtraction)
    S(tau)  = sum_{k=1..tau} d(k)
    d'(0)   = 1;  d'(tau) = d(tau) tau / S(tau), 1 where S(tau) == 0; stored as float32
    pick (on the float32 d'): the smallest tau in [tau_min, tau_max] with float64(d'(tau)) < threshold, then tau + 1 while that is in
            range and d'(tau+1) < d'(tau); none under the threshold: the smallest tau that attains the minimum of d', found = 0
    delta   = clamp(0.5 (a - c) / (a - 2b + c), -1, 1) with a, b, c = d'(tau-1), d'(tau), d'(tau+1) in float64, where tau - 1 >= 1,
              tau + 1 <= tau_max and a - 2b + c > 0; else 0
    f0 = float32(sr / (tau + delta));  ap = b;  rms = float32(sqrt(mean of the frame's first W samples squared, in float64))
    voiced = found and rms >= rms_gate;  the frame's time is (t + span / 2) / sr
There is no step 6 of the paper (the best local estimate); without `smooth` there is no smoothing over frames and no octave-error
correction either.

Smoothing (smooth=True or a dict of the four costs; csrc/f0_smooth.hip) keeps K = 7 period candidates per frame
and lets an exact Viterbi decode pick the cheapest path through them and one unvoiced state.  All integer arithmetic is int64.
    dip:        tau in [tau_min, tau_max] with (tau == tau_min or d'(tau) < d'(tau-1)) and (tau == tau_max or d'(tau) <= d'(tau+1));
                a frame always has one
    candidates: the 7 dips with the smallest d' (equal d': the smaller tau), stored in ascending tau; count = min(7, dips); per kept
                dip ap = d'(tau), delta by the pick's parabolic rule, f0 = float32(sr / (tau + delta)); slots >= count hold 0, 0, 0
    cents:      cents[0] = 0, cents[tau] = int32(rint(1200 log2(sr / tau))), built on the host (cents_table)
    states:     0..6 the frame's candidates, 7 unvoiced; INF = 2^40
    obs(k):     k < count and rms >= rms_gate: llrint(float64(ap_k) 4096) + (octave_cost (cents[tau_min] - cents[tau_k])) // 1200
                (the product is exact, the rounding half to even); state 7: unvoiced_cost; every other slot INF
    A(i, j):    voiced to voiced pitch_cost |cents[tau_i] - cents[tau_j]| (an empty slot's tau of 0 reads cents[0] = 0); voiced to
                unvoiced or back switch_cost; unvoiced to unvoiced 0
    recursion:  delta_0 = obs_0;  delta_t(j) = min_i(delta_{t-1}(i) + A_t(i, j)) + obs_t(j), psi_t(j) the smallest i that attains it;
                the end state is the smallest j that attains min delta_{T-1} (= cost); backtrace through psi
    track:      state < 7: f0 and ap of that candidate, voiced = 1; state 7: f0 and ap of the raw pick above, voiced = 0
Defaults (starting points, not tuned): pitch_cost 4 per cent, switch_cost 1024, unvoiced_cost 2048, octave_cost 82 per octave of lag
(it keeps the path off the sub-octave 2 T).  Limits: every cost in 0..2^20 and at most 2^20 frames, so every sum stays below 2^62.
The decode is over the frames of ONE call: pieces given by first_frame concatenate for the candidates, NOT for the decoded path.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from . import _lib

FMIN, FMAX, THRESHOLD = 65.0, 1000.0, 0.15
W_MAX, TAU_MAX, ROWS_MAX = 4096, 2048, 64                            # csrc/f0.hip: F0_MAX_W, F0_MAX_TAU, F0_MAX_ROWS
MELODY_GATE_DB = -50.0                                               # evaluate.py --melody: silent reference passages count as unvoiced
CENTS = 50.0
MELODY = ("VR", "VFA", "RPA", "RCA", "OA")
K, UNVOICED, INF = 7, 7, 1 << 40                                     # csrc/f0_smooth.hip: F0_K, VIT_INF
COSTS = {"pitch_cost": 4, "switch_cost": 1024, "unvoiced_cost": 2048, "octave_cost": 82}
COST_MAX, FRAMES_MAX, CHUNKS, CHUNK = 1 << 20, 1 << 20, (16, 32, 64, 128), 64


class Geometry(NamedTuple):
    sr: float
    tau_min: int
    tau_max: int
    W: int
    hop: int
    span: int
    threshold: float
    rms_gate: float


class Track(NamedTuple):
    """Per frame (numpy arrays from yin_reference, device tensors from track_gpu), (frames,) or (rows, frames): the frame's time in
    seconds (always (frames,)), f0 in Hz (float32), voiced (int32), the aperiodicity d'(tau) (float32) and the frame's rms (float32)."""
    time: object
    f0: object
    voiced: object
    ap: object
    rms: object


def geometry(sr, fmin=FMIN, fmax=FMAX, W=None, hop=None, threshold=THRESHOLD, rms_gate=0.0) -> Geometry:
    """The derived values above; every rule is a ValueError with a message of its own, before any device work."""
    sr, fmin, fmax = float(sr), float(fmin), float(fmax)
    if not (math.isfinite(sr) and sr > 0.0):
        raise ValueError(f"sr must be a positive rate in Hz, got {sr}")
    if not (math.isfinite(fmin) and fmin > 0.0 and math.isfinite(fmax) and fmax > 0.0):
        raise ValueError(f"fmin and fmax must be positive frequencies in Hz, got {fmin} and {fmax}")
    tau_min, tau_max = max(2, int(math.floor(sr / fmax))), int(math.ceil(sr / fmin))
    if tau_max > TAU_MAX:
        raise ValueError(f"fmin {fmin:g} Hz at {sr:g} Hz is a longest lag tau_max of {tau_max} samples; at most {TAU_MAX} "
                         f"(fmin >= {sr / TAU_MAX:.2f} Hz at this rate)")
    if not tau_min < tau_max:
        raise ValueError(f"fmin {fmin:g} Hz and fmax {fmax:g} Hz at {sr:g} Hz leave no lag range: tau_min {tau_min} must be below tau_max {tau_max}")
    W = 2 * tau_max if W is None else W
    if int(W) != W or not 1 <= int(W) <= W_MAX:
        raise ValueError(f"the window W must be a whole number of samples in 1..{W_MAX}, got {W}")
    hop = max(1, int(round(sr / 100.0))) if hop is None else hop
    if int(hop) != hop or int(hop) < 1:
        raise ValueError(f"hop must be a whole number of samples, at least 1, got {hop}")
    threshold, rms_gate = float(threshold), float(rms_gate)
    if not (math.isfinite(threshold) and threshold > 0.0):
        raise ValueError(f"the threshold must be positive and finite, got {threshold}")
    if not (math.isfinite(rms_gate) and rms_gate >= 0.0):
        raise ValueError(f"rms_gate is a linear level, finite and not negative, got {rms_gate}")
    return Geometry(sr, tau_min, tau_max, int(W), int(hop), int(W) + tau_max, threshold, rms_gate)


def check_rows(rows) -> int:
    if not 1 <= int(rows) <= ROWS_MAX:
        raise ValueError(f"rows must be in 1..{ROWS_MAX}, got {rows}")
    return int(rows)


def frame_count(n: int, span: int, hop: int) -> int:
    """1 + (n - span) // hop; n < span is a ValueError (nothing is zero-padded)."""
    if int(n) < int(span):
        raise ValueError(f"the signal has {int(n)} samples, one frame needs span = W + tau_max = {int(span)}")
    return 1 + (int(n) - int(span)) // int(hop)


def frame_range(n: int, g: Geometry, first_frame: int = 0, n_frames=None):
    """(first_frame, n_frames) checked against the signal's frame count; n_frames None: every frame from first_frame on."""
    total = frame_count(n, g.span, g.hop)
    first_frame = int(first_frame)
    n_frames = total - first_frame if n_frames is None else int(n_frames)
    if first_frame < 0 or n_frames < 0 or first_frame + n_frames > total:
        raise ValueError(f"frames {first_frame}..{first_frame + n_frames - 1} lie outside the signal's {total} frames")
    return first_frame, n_frames


def frame_times(g: Geometry, n_frames: int, first_frame: int = 0) -> np.ndarray:
    """(t + span / 2) / sr of frames first_frame .. first_frame + n_frames - 1, float64."""
    return ((first_frame + np.arange(int(n_frames), dtype=np.float64)) * g.hop + 0.5 * g.span) / g.sr


def gate_from_db(db) -> float:
    """A gate in dB re full scale as the linear rms_gate; None: off (0)."""
    return 0.0 if db is None else 10.0 ** (float(db) / 20.0)


def harmonic_tone(freq, sr, top: float = 3500.0, level: float = 0.25) -> np.ndarray:
    """A float32 test voice whose instantaneous fundamental at sample i is freq[i] Hz: level * sum_k sin(k phase) / k over the
    harmonics with k freq[i] <= top, phase the running integral of 2 pi freq / sr (trapezoids, float64)."""
    f = np.asarray(freq, dtype=np.float64)
    phase = np.concatenate([[0.0], np.cumsum(np.pi * (f[1:] + f[:-1]) / float(sr))])
    x = np.zeros(f.shape)
    for k in range(1, int(top // f.min()) + 1):
        x += np.where(k * f <= top, np.sin(k * phase) / k, 0.0)
    return (level * x).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# the float64 definition
# ------------------------------------------------------------------------------------------------
def cmnd_reference(x, W: int, tau_max: int, hop: int, first_frame: int = 0, n_frames=None):
    """(d' float32 (rows, frames, tau_max + 1), rms float32 (rows, frames)) of x: (n,) or (rows, n), taken as float32."""
    x = np.asarray(x, dtype=np.float32)
    x = x[None] if x.ndim == 1 else x.reshape(-1, x.shape[-1])
    n, span = x.shape[1], W + tau_max
    total = frame_count(n, span, hop)
    n_frames = total - first_frame if n_frames is None else n_frames
    starts = (first_frame + np.arange(n_frames)) * hop
    view = np.lib.stride_tricks.sliding_window_view
    d = np.zeros((x.shape[0], n_frames, tau_max + 1))
    rms = np.zeros((x.shape[0], n_frames), np.float32)
    for r, row in enumerate(x):
        sq = row.astype(np.float64) ** 2
        rms[r] = np.sqrt(view(sq, W)[starts].sum(axis=1) / W).astype(np.float32) if n_frames else 0
        for tau in range(1, tau_max + 1):
            diff = (row[:n - tau] - row[tau:]).astype(np.float64)    # the float32 subtraction, then exact
            d[r, :, tau] = view(diff * diff, W)[starts].sum(axis=1) if n_frames else 0
    S = np.cumsum(d[..., 1:], axis=-1)
    dp = np.ones_like(d)
    tau = np.arange(1, tau_max + 1, dtype=np.float64)
    np.divide(d[..., 1:] * tau, S, out=dp[..., 1:], where=S != 0.0)
    return dp.astype(np.float32), rms


def pick_reference(dprime, sr, tau_min: int, tau_max: int, threshold=THRESHOLD, rms=None, rms_gate=0.0):
    """The pick and the interpolation on any float32 d' buffer (..., tau_max + 1): (f0 float32, ap float32, voiced int32, tau int64),
    each of shape (...).  rms (...): voiced = found and rms >= rms_gate; None: voiced = found."""
    dp32 = np.asarray(dprime, dtype=np.float32)
    if dp32.shape[-1] != tau_max + 1:
        raise ValueError(f"d' must have tau_max + 1 = {tau_max + 1} values per frame, got {dp32.shape[-1]}")
    lead = dp32.shape[:-1]
    rows = dp32.reshape(-1, tau_max + 1)
    f0 = np.zeros(rows.shape[0], np.float32)
    ap = np.zeros(rows.shape[0], np.float32)
    found = np.zeros(rows.shape[0], bool)
    taus = np.zeros(rows.shape[0], np.int64)
    threshold = float(threshold)
    for i, dp in enumerate(rows):
        under = np.flatnonzero(dp[tau_min:tau_max + 1].astype(np.float64) < threshold)
        if under.size:
            tau = tau_min + int(under[0])
            while tau + 1 <= tau_max and dp[tau + 1] < dp[tau]:
                tau += 1
            found[i] = True
        else:
            tau = tau_min + int(np.argmin(dp[tau_min:tau_max + 1]))   # the first index that attains the minimum
        b, delta = float(dp[tau]), 0.0
        if tau - 1 >= 1 and tau + 1 <= tau_max:
            a, c = float(dp[tau - 1]), float(dp[tau + 1])
            q = a - 2.0 * b + c
            if q > 0.0:
                delta = min(1.0, max(-1.0, 0.5 * (a - c) / q))
        f0[i], ap[i], taus[i] = float(sr) / (tau + delta), dp[tau], tau
    voiced = found if rms is None else found & (np.asarray(rms, dtype=np.float32).reshape(-1) >= np.float32(rms_gate))
    return f0.reshape(lead), ap.reshape(lead), voiced.astype(np.int32).reshape(lead), taus.reshape(lead)


def yin_reference(x, sr, fmin=FMIN, fmax=FMAX, W=None, hop=None, threshold=THRESHOLD, rms_gate=0.0, first_frame: int = 0, n_frames=None,
                  smooth=None):
    """The definition on x: (n,) or (rows, n).  Returns (Track, d') -- d' float32 (frames, tau_max + 1) or (rows, frames, tau_max + 1).
    smooth (None: off; True or a dict of the four costs): the Track is the decoded one (smooth_reference over the call's frames)."""
    g = geometry(sr, fmin, fmax, W, hop, threshold, rms_gate)
    costs = None if smooth is None or smooth is False else check_costs(smooth)
    x = np.asarray(x, dtype=np.float32)
    one = x.ndim == 1
    x = x[None] if one else x.reshape(-1, x.shape[-1])
    check_rows(x.shape[0])
    first_frame, n_frames = frame_range(x.shape[1], g, first_frame, n_frames)
    dp, rms = cmnd_reference(x, g.W, g.tau_max, g.hop, first_frame, n_frames)
    f0, ap, voiced, _ = pick_reference(dp, g.sr, g.tau_min, g.tau_max, g.threshold, rms, g.rms_gate)
    if costs is not None:
        f0, ap, voiced, _, _ = smooth_reference(dp, rms, g.sr, g.tau_min, g.tau_max, g.threshold, g.rms_gate, costs)
    t = frame_times(g, n_frames, first_frame)
    if one:
        f0, ap, voiced, rms, dp = f0[0], ap[0], voiced[0], rms[0], dp[0]
    return Track(t, f0, voiced, ap, rms), dp


# ------------------------------------------------------------------------------------------------
# smoothing: candidates and the Viterbi decode (the definition; module docstring)
# ------------------------------------------------------------------------------------------------
def check_costs(smooth) -> dict:
    """The four costs as ints: True (or an empty dict) gives COSTS; a dict may set any of them.  Each must be a whole number in
    0..2^20 -- a ValueError with the cost's name otherwise, before any device work."""
    given = {} if smooth is True else dict(smooth)
    unknown = set(given) - set(COSTS)
    if unknown:
        raise ValueError(f"smooth= takes {', '.join(COSTS)}, not {sorted(unknown)}")
    out = {}
    for name, default in COSTS.items():
        v = given.get(name, default)
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= COST_MAX:
            raise ValueError(f"{name} must be a whole number in 0..2^20, got {v}")
        out[name] = int(v)
    return out


def cents_table(sr, tau_max: int) -> np.ndarray:
    """int32 (tau_max + 1,): cents[0] = 0, cents[tau] = rint(1200 log2(sr / tau)).  Built on the host; the device takes no logarithm."""
    table = np.zeros(int(tau_max) + 1, np.int32)
    table[1:] = np.rint(1200.0 * np.log2(float(sr) / np.arange(1, int(tau_max) + 1, dtype=np.float64))).astype(np.int32)
    return table


def candidates_reference(dprime, sr, tau_min: int, tau_max: int):
    """The candidates of any float32 d' buffer (..., tau_max + 1): (tau int32 (..., 7), f0 float32 (..., 7), ap float32 (..., 7),
    count int32 (...))."""
    dp32 = np.asarray(dprime, dtype=np.float32)
    if dp32.shape[-1] != tau_max + 1:
        raise ValueError(f"d' must have tau_max + 1 = {tau_max + 1} values per frame, got {dp32.shape[-1]}")
    lead = dp32.shape[:-1]
    rows = dp32.reshape(-1, tau_max + 1)
    tau = np.zeros((rows.shape[0], K), np.int32)
    f0 = np.zeros((rows.shape[0], K), np.float32)
    ap = np.zeros((rows.shape[0], K), np.float32)
    count = np.zeros(rows.shape[0], np.int32)
    for i, dp in enumerate(rows):
        v = dp[tau_min:tau_max + 1]
        left = np.concatenate([[True], v[1:] < v[:-1]])
        right = np.concatenate([v[:-1] <= v[1:], [True]])
        dips = tau_min + np.flatnonzero(left & right)
        keep = np.sort(dips[np.lexsort((dips, dp[dips]))][:K])        # by (d', tau), then back in ascending tau
        count[i] = keep.size
        for k, t in enumerate(keep.tolist()):
            b, delta = float(dp[t]), 0.0
            if t - 1 >= 1 and t + 1 <= tau_max:
                a, c = float(dp[t - 1]), float(dp[t + 1])
                q = a - 2.0 * b + c
                if q > 0.0:
                    delta = min(1.0, max(-1.0, 0.5 * (a - c) / q))
            tau[i, k], f0[i, k], ap[i, k] = t, float(sr) / (t + delta), dp[t]
    return tau.reshape(lead + (K,)), f0.reshape(lead + (K,)), ap.reshape(lead + (K,)), count.reshape(lead)


def viterbi_costs(cand_tau, cand_ap, count, rms, cents, tau_min: int, rms_gate=0.0, **costs):
    """One row's (obs int64 (T, 8), A int64 (T, 8, 8)) -- A[t] leads from frame t - 1 to frame t, A[0] is unused (zero)."""
    c = check_costs(costs)
    cand_tau, count = np.asarray(cand_tau, dtype=np.int64), np.asarray(count, dtype=np.int64)
    T = count.shape[0]
    if cand_tau.shape != (T, K) or np.shape(cand_ap) != (T, K) or np.shape(rms) != (T,):
        raise ValueError(f"one row takes cand_tau and cand_ap (T, {K}), count and rms (T,), got {cand_tau.shape}, {np.shape(cand_ap)}, "
                         f"{count.shape}, {np.shape(rms)}")
    cents = np.asarray(cents, dtype=np.int64)
    if T and (cand_tau.min() < 0 or cand_tau.max() >= cents.shape[0]):
        raise ValueError(f"a candidate's tau lies outside the cents table's 0..{cents.shape[0] - 1}")
    cen = cents[cand_tau]                                             # (T, 7)
    live = (np.arange(K)[None] < count[:, None]) & (np.asarray(rms, dtype=np.float32) >= np.float32(rms_gate))[:, None]
    obs = np.full((T, K + 1), INF, np.int64)
    voiced = np.rint(np.asarray(cand_ap, dtype=np.float32).astype(np.float64) * 4096.0).astype(np.int64) \
        + (c["octave_cost"] * (cents[tau_min] - cen)) // 1200
    obs[:, :K] = np.where(live, voiced, INF)
    obs[:, K] = c["unvoiced_cost"]
    A = np.full((T, K + 1, K + 1), c["switch_cost"], np.int64)
    A[:, K, K] = 0
    if T:
        A[0] = 0
        A[1:, :K, :K] = c["pitch_cost"] * np.abs(cen[:-1, :, None] - cen[1:, None, :])
    return obs, A


def viterbi_decode(obs, A):
    """The textbook recursion on one row's int64 costs (viterbi_costs): (state int32 (T,), cost) with the smallest index on every tie."""
    obs, A = np.asarray(obs, dtype=np.int64), np.asarray(A, dtype=np.int64)
    T, S = obs.shape
    if T == 0:
        return np.zeros(0, np.int32), 0
    psi = np.zeros((T, S), np.int64)
    delta = obs[0].copy()
    for t in range(1, T):
        through = delta[:, None] + A[t]                               # (i, j)
        psi[t] = np.argmin(through, axis=0)                           # the first i that attains the minimum
        delta = through.min(axis=0) + obs[t]
    state = np.zeros(T, np.int32)
    state[-1] = int(np.argmin(delta))
    for t in range(T - 1, 0, -1):
        state[t - 1] = psi[t, state[t]]
    return state, int(delta.min())


def viterbi_reference(cand_tau, cand_ap, count, rms, cents, tau_min: int, rms_gate=0.0, **costs):
    """The decode of candidate buffers (T, 7) / (T,) or (rows, T, 7) / (rows, T): (state int32, like count; cost int64, () or (rows,))."""
    count = np.asarray(count)
    if count.ndim == 1:
        state, cost = viterbi_decode(*viterbi_costs(cand_tau, cand_ap, count, rms, cents, tau_min, rms_gate, **costs))
        return state, np.int64(cost)
    if count.shape[-1] > FRAMES_MAX:
        raise ValueError(f"at most 2^20 frames are decoded at once, got {count.shape[-1]}")
    out = [viterbi_reference(t, a, n, r, cents, tau_min, rms_gate, **costs) for t, a, n, r in zip(cand_tau, cand_ap, count, rms)]
    return np.stack([s for s, _ in out]), np.array([c for _, c in out], np.int64)


def select_reference(state, cand_f0, cand_ap, raw_f0, raw_ap):
    """(f0, ap, voiced) of the decoded path: the candidate's where state < 7, the raw pick's and unvoiced where it is 7."""
    state = np.asarray(state)
    v = state < K
    slot = np.minimum(state, K - 1)[..., None]
    f0 = np.where(v, np.take_along_axis(np.asarray(cand_f0), slot, axis=-1)[..., 0], raw_f0).astype(np.float32)
    ap = np.where(v, np.take_along_axis(np.asarray(cand_ap), slot, axis=-1)[..., 0], raw_ap).astype(np.float32)
    return f0, ap, v.astype(np.int32)


def smooth_reference(dprime, rms, sr, tau_min: int, tau_max: int, threshold=THRESHOLD, rms_gate=0.0, smooth=True):
    """The smoothed (f0 float32, ap float32, voiced int32, state int32, cost int64) of a float32 d' buffer (frames, tau_max + 1) or
    (rows, frames, tau_max + 1) and its rms: pick_reference, candidates_reference, viterbi_reference and select_reference in turn."""
    costs = check_costs(smooth)
    raw_f0, raw_ap, _, _ = pick_reference(dprime, sr, tau_min, tau_max, threshold, rms, rms_gate)
    tau, f0, ap, count = candidates_reference(dprime, sr, tau_min, tau_max)
    state, cost = viterbi_reference(tau, ap, count, np.asarray(rms, dtype=np.float32), cents_table(sr, tau_max), tau_min, rms_gate, **costs)
    return select_reference(state, f0, ap, raw_f0, raw_ap) + (state, cost)


# ------------------------------------------------------------------------------------------------
# melody measures
# ------------------------------------------------------------------------------------------------
def melody_metrics(ref_f0, ref_voiced, est_f0, est_voiced) -> dict:
    """The five frame-level measures of the MIREX audio melody extraction task, as fractions in [0, 1], of two tracks on the same frames:
        VR   voicing recall:       the reference's voiced frames that the estimate calls voiced
        VFA  voicing false alarm:  the reference's unvoiced frames that the estimate calls voiced
        RPA  raw pitch accuracy:   the reference's voiced frames whose estimated f0 lies within 50 cents -- the larger of the two
                                   frequencies over the smaller is at most the double 2^(50/1200), the bound included -- whatever voicing
                                   the estimate reports there (the tracker gives a pitch on every frame)
        RCA  raw chroma accuracy:  the same with the difference folded into one octave (octave errors forgiven)
        OA   overall accuracy:     frames that are right altogether -- voiced in both with the pitch within 50 cents, or unvoiced in both --
                                   over all frames
    A measure over an empty set of frames (no voiced reference frame, no unvoiced one, no frame at all) is 0."""
    ref_f0, est_f0 = np.asarray(ref_f0, dtype=np.float64).reshape(-1), np.asarray(est_f0, dtype=np.float64).reshape(-1)
    rv, ev = np.asarray(ref_voiced).reshape(-1) != 0, np.asarray(est_voiced).reshape(-1) != 0
    if not ref_f0.shape == est_f0.shape == rv.shape == ev.shape:
        raise ValueError(f"the four arrays must have one value per frame, got {ref_f0.shape}, {rv.shape}, {est_f0.shape}, {ev.shape}")
    ok = rv & (ref_f0 > 0.0) & (est_f0 > 0.0) & np.isfinite(ref_f0) & np.isfinite(est_f0)
    ref, est = np.where(ok, ref_f0, 1.0), np.where(ok, est_f0, 1.0)
    octaves = np.round(np.log2(est / ref)).astype(np.int64)
    folded = np.ldexp(est, -octaves)                                  # exact: the estimate brought into the reference's octave

    def within(a, b):                                                 # larger over smaller at most 2^(50/1200), the bound included
        return ok & (np.maximum(a, b) / np.minimum(a, b) <= 2.0 ** (CENTS / 1200.0))
    pitch, fold = within(est, ref), within(folded, ref)

    def ratio(hits, among):
        return float(hits) / float(among) if among else 0.0
    n_v, n_u = int(rv.sum()), int((~rv).sum())
    return {"VR": ratio((rv & ev).sum(), n_v), "VFA": ratio((~rv & ev).sum(), n_u), "RPA": ratio((rv & pitch).sum(), n_v),
            "RCA": ratio((rv & fold).sum(), n_v), "OA": ratio((rv & ev & pitch).sum() + (~rv & ~ev).sum(), n_v + n_u)}


# ------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------
def _rows_gpu(x):
    """(x as (rows, n) with unit stride along n, rows, n, ld_row, whether a row axis was added)."""
    import torch
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError("the device path needs a device tensor (yin_reference is the host path)")
    if x.dtype != torch.float32:
        raise TypeError(f"dtype {x.dtype} (float32)")
    if x.dim() not in (1, 2):
        raise ValueError(f"the signal must be (n,) or (rows, n), got {tuple(x.shape)}")
    one = x.dim() == 1
    x = x[None] if one else x
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    rows, n = check_rows(x.shape[0]), x.shape[1]
    return x, rows, n, (x.stride(0) if rows > 1 else max(n, 1)), one


def cmnd_gpu(x, W: int, tau_max: int, hop: int, first_frame: int = 0, n_frames=None, rms: bool = True):
    """svs_f0_cmnd: (d' float32 (rows, frames, tau_max + 1), rms float32 (rows, frames) or None) of a float32 device signal (n,) or
    (rows, n); a 1-D signal gives (frames, tau_max + 1) and (frames,)."""
    import torch
    x, rows, n, ld_row, one = _rows_gpu(x)
    total = frame_count(n, W + tau_max, hop)
    n_frames = total - int(first_frame) if n_frames is None else int(n_frames)
    dp = torch.empty(rows, n_frames, tau_max + 1, dtype=torch.float32, device=x.device)
    r = torch.empty(rows, n_frames, dtype=torch.float32, device=x.device) if rms else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().svs_f0_cmnd(x.data_ptr(), rows, n, ld_row, int(W), int(tau_max), int(hop), int(first_frame), n_frames, dp.data_ptr(),
                                          _lib.ptr(r), _lib.stream_ptr(x.device)), "svs_f0_cmnd")
    return (dp[0], None if r is None else r[0]) if one else (dp, r)


def pick_gpu(dprime, sr, tau_min: int, threshold=THRESHOLD, rms=None, rms_gate=0.0):
    """svs_f0_pick on a float32 device buffer (..., tau_max + 1): (f0 float32, ap float32, voiced int32), each (...)."""
    import torch
    if not torch.is_tensor(dprime) or not dprime.is_cuda or dprime.dtype != torch.float32 or dprime.dim() < 1:
        raise TypeError("d' must be a float32 device tensor (..., tau_max + 1)")
    dprime = dprime.contiguous()
    lead, tau_max = dprime.shape[:-1], dprime.shape[-1] - 1
    count = int(np.prod(lead, dtype=np.int64))
    if rms is not None:
        if rms.dtype != torch.float32 or rms.device != dprime.device or rms.shape != lead:
            raise ValueError(f"rms must be a float32 tensor {tuple(lead)} on d's device")
        rms = rms.contiguous()
    f0 = torch.empty(lead, dtype=torch.float32, device=dprime.device)
    ap = torch.empty_like(f0)
    voiced = torch.empty(lead, dtype=torch.int32, device=dprime.device)
    with torch.cuda.device(dprime.device):
        _lib.check(_lib.lib().svs_f0_pick(dprime.data_ptr(), count, int(tau_min), tau_max, float(threshold), _lib.ptr(rms), float(rms_gate),
                                          float(sr), f0.data_ptr(), ap.data_ptr(), voiced.data_ptr(), _lib.stream_ptr(dprime.device)), "svs_f0_pick")
    return f0, ap, voiced


def dips_gpu(dprime, sr, tau_min: int):
    """svs_f0_dips on a float32 device buffer (..., tau_max + 1): (tau int32 (..., 7), f0 float32 (..., 7), ap float32 (..., 7),
    count int32 (...)), bitwise candidates_reference's on the same buffer."""
    import torch
    if not torch.is_tensor(dprime) or not dprime.is_cuda or dprime.dtype != torch.float32 or dprime.dim() < 1:
        raise TypeError("d' must be a float32 device tensor (..., tau_max + 1)")
    dprime = dprime.contiguous()
    lead, tau_max = tuple(dprime.shape[:-1]), dprime.shape[-1] - 1
    frames = int(np.prod(lead, dtype=np.int64))
    tau = torch.empty(lead + (K,), dtype=torch.int32, device=dprime.device)
    f0, ap = (torch.empty(lead + (K,), dtype=torch.float32, device=dprime.device) for _ in range(2))
    count = torch.empty(lead, dtype=torch.int32, device=dprime.device)
    with torch.cuda.device(dprime.device):
        _lib.check(_lib.lib().svs_f0_dips(dprime.data_ptr(), frames, int(tau_min), tau_max, float(sr), tau.data_ptr(), f0.data_ptr(), ap.data_ptr(),
                                          count.data_ptr(), _lib.stream_ptr(dprime.device)), "svs_f0_dips")
    return tau, f0, ap, count


def candidates_gpu(x, sr, fmin=FMIN, fmax=FMAX, W=None, hop=None, threshold=THRESHOLD, rms_gate=0.0, first_frame: int = 0, n_frames=None):
    """svs_f0_candidates, ONE launch: (the raw Track of track_gpu, bit for bit; (tau int32, f0 float32, ap float32) (rows, frames, 7) and
    count int32 (rows, frames) -- without the row axis for a 1-D signal)."""
    import torch
    g = geometry(sr, fmin, fmax, W, hop, threshold, rms_gate)
    x, rows, n, ld_row, one = _rows_gpu(x)
    first_frame, n_frames = frame_range(n, g, first_frame, n_frames)
    f0, ap, rms, voiced, cand = _candidates(x, rows, n, ld_row, g, first_frame, n_frames)
    t = torch.from_numpy(frame_times(g, n_frames, first_frame)).to(x.device)
    if one:
        return Track(t, f0[0], voiced[0], ap[0], rms[0]), tuple(c[0] for c in cand)
    return Track(t, f0, voiced, ap, rms), cand


def _candidates(x, rows, n, ld_row, g: Geometry, first_frame: int, n_frames: int):
    import torch
    f0, ap, rms = (torch.empty(rows, n_frames, dtype=torch.float32, device=x.device) for _ in range(3))
    voiced, count = (torch.empty(rows, n_frames, dtype=torch.int32, device=x.device) for _ in range(2))
    c_tau = torch.empty(rows, n_frames, K, dtype=torch.int32, device=x.device)
    c_f0, c_ap = (torch.empty(rows, n_frames, K, dtype=torch.float32, device=x.device) for _ in range(2))
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().svs_f0_candidates(x.data_ptr(), rows, n, ld_row, g.W, g.tau_min, g.tau_max, g.hop, first_frame, n_frames, g.threshold,
                                                g.rms_gate, g.sr, f0.data_ptr(), ap.data_ptr(), rms.data_ptr(), voiced.data_ptr(), c_tau.data_ptr(),
                                                c_f0.data_ptr(), c_ap.data_ptr(), count.data_ptr(), _lib.stream_ptr(x.device)), "svs_f0_candidates")
    return f0, ap, rms, voiced, (c_tau, c_f0, c_ap, count)


_CENTS = {}


def cents_gpu(sr, tau_max: int, device):
    """cents_table on the device, uploaded once per (sr, tau_max, device)."""
    import torch
    device = torch.device(device)
    key = (float(sr), int(tau_max), device.type, torch.cuda.current_device() if device.index is None else device.index)
    if key not in _CENTS:
        _CENTS[key] = torch.from_numpy(cents_table(sr, tau_max)).to(device)
    return _CENTS[key]


def viterbi_gpu(cand_tau, cand_ap, count, rms, cents, tau_min: int, rms_gate=0.0, chunk: int = CHUNK, **costs):
    """svs_f0_viterbi on device candidate buffers (rows, T, 7) / (rows, T) (or without the row axis): (state int32 like count, cost int64
    (rows,) or ()), bitwise viterbi_reference's for every chunk in CHUNKS.  cents: the int32 device table (cents_gpu)."""
    import torch
    c = check_costs(costs)
    if int(chunk) not in CHUNKS:
        raise ValueError(f"chunk must be one of {CHUNKS}, got {chunk}")
    one = count.dim() == 1
    if one:
        cand_tau, cand_ap, count, rms = cand_tau[None], cand_ap[None], count[None], rms[None]
    rows, T = check_rows(count.shape[0]), count.shape[1]
    if T > FRAMES_MAX:
        raise ValueError(f"at most 2^20 frames are decoded at once, got {T}")
    for name, t, dtype, shape in (("cand_tau", cand_tau, torch.int32, (rows, T, K)), ("cand_ap", cand_ap, torch.float32, (rows, T, K)),
                                  ("count", count, torch.int32, (rows, T)), ("rms", rms, torch.float32, (rows, T)),
                                  ("cents", cents, torch.int32, tuple(cents.shape[:1]))):
        if not t.is_cuda or t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(f"{name} must be a {dtype} device tensor {shape}, got {t.dtype} {tuple(t.shape)}")
    cand_tau, cand_ap, count, rms, cents = (t.contiguous() for t in (cand_tau, cand_ap, count, rms, cents))
    tau_max = cents.shape[0] - 1
    lib = _lib.lib()
    ws = torch.empty(max(16, lib.svs_f0_viterbi_workspace(rows, T, int(chunk))), dtype=torch.uint8, device=count.device)
    state = torch.empty(rows, T, dtype=torch.int32, device=count.device)
    cost = torch.zeros(rows, dtype=torch.int64, device=count.device)
    with torch.cuda.device(count.device):
        _lib.check(lib.svs_f0_viterbi(cand_tau.data_ptr(), cand_ap.data_ptr(), count.data_ptr(), rms.data_ptr(), rows, T, cents.data_ptr(),
                                      int(tau_min), tau_max, float(rms_gate), c["pitch_cost"], c["switch_cost"], c["unvoiced_cost"],
                                      c["octave_cost"], int(chunk), ws.data_ptr(), state.data_ptr(), cost.data_ptr(),
                                      _lib.stream_ptr(count.device)), "svs_f0_viterbi")
    return (state[0], cost[0]) if one else (state, cost)


def track_gpu(x, sr, fmin=FMIN, fmax=FMAX, W=None, hop=None, threshold=THRESHOLD, rms_gate=0.0, first_frame: int = 0, n_frames=None,
              smooth=None) -> Track:
    """svs_f0_track, ONE launch: the Track of a float32 device signal (n,) or (rows, n) as device tensors (time: float64 (frames,)).
    The geometry's rules and the frame range are checked before any device work; nothing waits for the host.
    smooth (None: the above, untouched; True or a dict of pitch_cost, switch_cost, unvoiced_cost, octave_cost): svs_f0_candidates,
    svs_f0_viterbi over the call's frames and svs_f0_smooth_select instead -- f0, ap and voiced are the decoded path's, rms and time are
    unchanged.  Pieces given by first_frame do NOT concatenate to the whole-signal decode: the path is the best one of the call."""
    import torch
    g = geometry(sr, fmin, fmax, W, hop, threshold, rms_gate)
    costs = None if smooth is None or smooth is False else check_costs(smooth)
    x, rows, n, ld_row, one = _rows_gpu(x)
    first_frame, n_frames = frame_range(n, g, first_frame, n_frames)
    if costs is not None:
        if n_frames > FRAMES_MAX:
            raise ValueError(f"at most 2^20 frames are decoded at once, got {n_frames}")
        raw_f0, raw_ap, rms, _, (c_tau, c_f0, c_ap, count) = _candidates(x, rows, n, ld_row, g, first_frame, n_frames)
        state, _ = viterbi_gpu(c_tau, c_ap, count, rms, cents_gpu(g.sr, g.tau_max, x.device), g.tau_min, g.rms_gate, **costs)
        f0, ap = torch.empty_like(raw_f0), torch.empty_like(raw_ap)
        voiced = torch.empty(rows, n_frames, dtype=torch.int32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().svs_f0_smooth_select(state.data_ptr(), c_f0.data_ptr(), c_ap.data_ptr(), raw_f0.data_ptr(), raw_ap.data_ptr(),
                                                       rows * n_frames, f0.data_ptr(), ap.data_ptr(), voiced.data_ptr(),
                                                       _lib.stream_ptr(x.device)), "svs_f0_smooth_select")
        t = torch.from_numpy(frame_times(g, n_frames, first_frame)).to(x.device)
        return Track(t, f0[0], voiced[0], ap[0], rms[0]) if one else Track(t, f0, voiced, ap, rms)
    f0, ap, rms = (torch.empty(rows, n_frames, dtype=torch.float32, device=x.device) for _ in range(3))
    voiced = torch.empty(rows, n_frames, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().svs_f0_track(x.data_ptr(), rows, n, ld_row, g.W, g.tau_min, g.tau_max, g.hop, first_frame, n_frames, g.threshold,
                                           g.rms_gate, g.sr, f0.data_ptr(), ap.data_ptr(), rms.data_ptr(), voiced.data_ptr(),
                                           _lib.stream_ptr(x.device)), "svs_f0_track")
    t = torch.from_numpy(frame_times(g, n_frames, first_frame)).to(x.device)
    return Track(t, f0[0], voiced[0], ap[0], rms[0]) if one else Track(t, f0, voiced, ap, rms)


def channel_mean(x):
    """(channels, n) or (n,) device samples -> the (n,) float32 mean of the channels that the tracker reads."""
    return x if x.dim() == 1 else x.float().mean(dim=0)


def check_options(options) -> dict:
    """The keywords of track_gpu that f0= of the separation calls takes (True or None-like: the defaults; smooth among them): a ValueError
    for anything else."""
    options = {} if options is True else dict(options)
    unknown = set(options) - {"fmin", "fmax", "W", "hop", "threshold", "rms_gate", "smooth"}
    if unknown:
        raise ValueError(f"f0= takes fmin, fmax, W, hop, threshold and rms_gate, not {sorted(unknown)}")
    if options.get("smooth") is not None and options["smooth"] is not False:
        check_costs(options["smooth"])                               # smooth: True or a dict of the four costs (track_gpu)
    return options


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------
CSV_HEADER = "time,f0,voiced,aperiodicity,rms"


def write_csv(path: str, track: Track):
    """One row per frame of a one-row Track: time,f0,voiced,aperiodicity,rms."""
    cols = [np.asarray(c.cpu() if hasattr(c, "cpu") else c) for c in track]
    if cols[1].ndim != 1:
        raise ValueError(f"a csv file holds one track, got f0 of shape {cols[1].shape}")
    with open(path, "w", encoding="utf-8") as f:
        f.write(CSV_HEADER + "\n")
        for t, hz, v, a, r in zip(*cols):
            f.write(f"{t:.6f},{hz:.4f},{int(v)},{a:.6f},{r:.6e}\n")
    return len(cols[1])


def file_track(path: str, device=None, **options) -> Track:
    """The track of a wav file at its own rate, from the mean of its channels; device None: yin_reference on the host."""
    if device is None:
        from .data import read_pcm
        rate, data, channels = read_pcm(path)
        if data.dtype.kind == "i":
            data = data.astype(np.float64) / float(np.iinfo(data.dtype).max + 1)
        mono = data.mean(axis=1) if data.ndim == 2 else data
        return yin_reference(mono.astype(np.float32), rate, **options)[0]
    from .pcm import read_pcm_device
    from .resample import resample_poly_gpu
    rate, pcm, channels = read_pcm_device(path, device)             # a 24-bit file crosses as its 3 bytes per sample (pcm.py)
    return track_gpu(channel_mean(resample_poly_gpu(pcm, 1, 1, channels=channels, downmix=False)), rate, **options)


def main(argv=None):
    import argparse
    import os
    import sys
    parser = argparse.ArgumentParser(description="fundamental frequency of wav files (YIN, steps 1 to 5): time,f0,voiced,aperiodicity,rms per frame")
    parser.add_argument("--src", type=str, required=True, help="a wav file, or a folder of *.wav files")
    parser.add_argument("--csv", type=str, required=True, help="the csv file to write, or the target folder when --src is a folder")
    parser.add_argument("--fmin", type=float, default=FMIN, help=f"lowest f0 in Hz (default {FMIN:g})")
    parser.add_argument("--fmax", type=float, default=FMAX, help=f"highest f0 in Hz (default {FMAX:g})")
    parser.add_argument("--window", type=int, default=None, help="integration window W in samples (default: twice the longest lag)")
    parser.add_argument("--hop", type=int, default=None, help="samples between frames (default: 10 ms)")
    parser.add_argument("--threshold", type=float, default=THRESHOLD, help=f"absolute threshold on d' (default {THRESHOLD})")
    parser.add_argument("--rms_gate_db", type=float, default=None, help="frames whose rms lies below this level (dB re full scale) are unvoiced (default: off)")
    parser.add_argument("--device", default="gpu", choices=["gpu", "cpu"], help="gpu: csrc/f0.hip; cpu: the float64 definition")
    parser.add_argument("--smooth", action="store_true",
                        help="decode the track over 7 candidates per frame and an unvoiced state (Viterbi; csrc/f0_smooth.hip): fewer octave errors")
    for name, default in COSTS.items():
        parser.add_argument("--" + name, type=int, default=None, help=f"--smooth: whole number in 0..2^20, unit 1/4096 (default {default})")
    args = parser.parse_args(argv)
    given = {name: getattr(args, name) for name in COSTS if getattr(args, name) is not None}
    if given and not args.smooth:
        parser.error(f"--{sorted(given)[0]} belongs to --smooth")
    try:
        smooth = check_costs(given) if args.smooth else None
    except ValueError as e:
        parser.error(str(e))
    device = None
    if args.device == "gpu":
        import torch
        if not torch.cuda.is_available():
            print("--device gpu needs a ROCm device (hand-written gfx950 kernels); --device cpu runs the float64 definition.")
            sys.exit(1)
        device = torch.device("cuda")
    options = dict(fmin=args.fmin, fmax=args.fmax, W=args.window, hop=args.hop, threshold=args.threshold, rms_gate=gate_from_db(args.rms_gate_db),
                   smooth=smooth)
    if os.path.isdir(args.src):
        os.makedirs(args.csv, exist_ok=True)
        jobs = [(os.path.join(args.src, f), os.path.join(args.csv, f[:-4] + ".csv")) for f in sorted(os.listdir(args.src)) if f.endswith(".wav")]
    else:
        jobs = [(args.src, args.csv)]
    for src, dst in jobs:
        try:
            track = file_track(src, device, **options)
        except ValueError as e:
            parser.error(f"{src}: {e}")
        frames = write_csv(dst, track)
        voiced = int(np.asarray(track.voiced.cpu() if hasattr(track.voiced, "cpu") else track.voiced).sum())
        print(f"{dst}: {frames} frames, {voiced} voiced")


if __name__ == "__main__":
    main()
