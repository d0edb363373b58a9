"""Rule "f12" of include/visinger_hip.h restated sequentially in numpy -- the oracle of tests/test_f0_path_cpu.py and tests/test_f0_path_gpu.py:
``candidates_ref`` in fp64 on the d' rows of ``test_f0_extract_cpu.yin_frames``, ``path_ref`` in integers (its quantiser in fp32: ``quantise_f0`` of the
guide-align restatement, the same one the device shares between the two kernels), and the two signals the path is there for: a fundamental that fades out
for a few frames (plain YIN jumps an octave) and a clean tone under white noise at the level where d' hovers around the threshold (plain YIN flickers)."""
import numpy as np

from test_f0_extract_cpu import F0_MAX, F0_MIN, FRAMES, HOP, SILENCE, SR, TAIL, lag_range, tone
from test_guide_align_cpu import quantise_f0

SLOTS, UNVOICED, ABSENT = 8, 7, 16384
DEFAULTS = dict(gate=0.5, w_unvoiced=160, w_switch=96, w_order=24, w_jump=32, jump_cap=384)
N_SAMPLES = FRAMES * HOP + TAIL
DIP_TONES = (98.0, 146.8, 220.0, 392.0, 523.3)
SEEDS = (1, 2, 3)


def parabola_hz(row, p, sr):
    """step 5 of f6 at lag p"""
    y0, y1, y2 = row[p - 1], row[p], row[p + 1]
    den = y0 - 2 * y1 + y2
    off = min(max(0.5 * (y0 - y2) / den, -0.5), 0.5) if den > 0 else 0.0
    return sr / (p + off)


def candidate_lags(row, tau_min, tau_max, gate):
    """every lag of a d' row that is a candidate, ascending: a local minimum (tau_min needs no left neighbour) below the gate"""
    return [tau for tau in range(tau_min, tau_max + 1)
            if (tau == tau_min or row[tau - 1] > row[tau]) and row[tau] <= row[tau + 1] and row[tau] < gate]


def candidates_ref(dp, e, n_b, sr=SR, f0_min=F0_MIN, f0_max=F0_MAX, window=None, gate=DEFAULTS["gate"], silence=SILENCE):
    """vs_f0_candidates on yin_frames' output: (cand_hz [T, 8], cand_d [T, 8], lags [T, 7] with 0 = empty), fp64"""
    tau_min, tau_max = lag_range(sr, f0_min, f0_max)
    W = 2 * tau_max if window is None else window
    T = len(dp)
    hz, d, lags = np.zeros((T, SLOTS)), np.ones((T, SLOTS)), np.zeros((T, SLOTS - 1), np.int64)
    for t in range(n_b):
        if not np.isfinite(e[t]) or e[t] <= silence * W:
            continue
        for k, tau in enumerate(candidate_lags(dp[t], tau_min, tau_max, gate)[:SLOTS - 1]):
            hz[t, k], d[t, k], lags[t, k] = parabola_hz(dp[t], tau, sr), dp[t, tau], tau
    return hz, d, lags


def local_costs(cand_hz, cand_d, w_unvoiced, w_order):
    """(q [T, 7] int64, present [T, 7], loc [T, 8] int64)"""
    hz, d = np.asarray(cand_hz, np.float32)[:, :UNVOICED], np.asarray(cand_d, np.float32)[:, :UNVOICED]
    q, present = quantise_f0(hz)
    with np.errstate(invalid="ignore"):
        dc = np.where(np.isnan(d), np.float32(1), np.clip(d, np.float32(0), np.float32(1)))
    loc = np.minimum(np.rint(np.float32(1024) * dc).astype(np.int64), 1024) + w_order * np.arange(UNVOICED)[None, :]
    loc = np.where(present, loc, ABSENT)
    return q, present, np.concatenate([loc, np.full((len(hz), 1), w_unvoiced, np.int64)], axis=1)


def path_ref(cand_hz, cand_d, n=None, w_unvoiced=160, w_switch=96, w_order=24, w_jump=32, jump_cap=384):
    """vs_f0_path on one item's candidates [T, 8]: (f0 [T] fp32, state [T] int32, cost)"""
    cand_hz = np.asarray(cand_hz, np.float32)
    T = len(cand_hz)
    N = T if n is None else int(min(max(int(n), 0), T))
    f0, state = np.zeros(T, np.float32), np.full(T, -1, np.int32)
    if N == 0:
        return f0, state, 0
    q, present, loc = local_costs(cand_hz[:N], np.asarray(cand_d)[:N], w_unvoiced, w_order)
    switch = np.zeros((SLOTS, SLOTS), np.int64)                                # trans[i, j] where a state is the unvoiced one
    switch[UNVOICED, :UNVOICED] = switch[:UNVOICED, UNVOICED] = w_switch
    D = loc[0].copy()
    back = np.zeros((N, SLOTS), np.int64)
    for t in range(1, N):
        trans = switch.copy()
        jump = np.minimum((np.abs(q[t - 1][:, None] - q[t][None, :]) * w_jump) >> 4, jump_cap)
        trans[:UNVOICED, :UNVOICED] = np.where(present[t - 1][:, None] & present[t][None, :], jump, 0)
        total = D[:, None] + trans                                              # [i, j]
        back[t] = np.argmin(total, axis=0)                                      # (numpy: the first minimum -- the lowest i)
        D = loc[t] + total[back[t], np.arange(SLOTS)]
    s = int(np.argmin(D))
    cost = int(D[s])
    assert cost < 2 ** 31
    for t in range(N - 1, -1, -1):
        state[t] = s
        if s < UNVOICED and present[t, s]:
            f0[t] = cand_hz[t, s]
        s = int(back[t, s])
    return f0, state, cost


def track_ref(x, length=None, frames=None, **path):
    """extract_f0(path=) on one row: (f0 [T] fp64 of the chosen candidates, state [T], cost, cand_hz, cand_d, lags)"""
    from test_f0_extract_cpu import yin_frames
    opts = dict(DEFAULTS, **path)
    dp, e, n_b = yin_frames(x, length=length, frames=frames)
    hz, d, lags = candidates_ref(dp, e, n_b, gate=opts.pop("gate"))
    n = (len(x) if length is None else length) // HOP
    f32, state, cost = path_ref(hz, d, n, **opts)
    f0 = np.array([hz[t, s] if 0 <= s < UNVOICED else 0.0 for t, s in enumerate(state)])
    return f0, state, cost, hz, d, lags


# ---- signals -------------------------------------------------------------------------------------------------------------------------------

def funddip(f0, rng, sr=SR, hop=HOP, n=N_SAMPLES):
    """a tone whose fundamental and third partial fade out over frames 20 .. 25 while the second and fourth stay: peak 0.2, white noise of sigma 0.002"""
    ph = 2 * np.pi * f0 * np.arange(n) / sr
    env = np.ones(n)
    env[20 * hop:26 * hop] = 0.0
    env = np.convolve(np.pad(env, (200, 199), mode="edge"), np.full(400, 1.0 / 400), mode="valid")
    x = env * (np.sin(ph + 1.0) + 0.4 * np.sin(3 * ph + 2.0)) + 0.8 * np.sin(2 * ph + 0.3) + 0.3 * np.sin(4 * ph)
    return 0.2 * x / np.abs(x).max() + rng.normal(0.0, 0.002, n)


def flicker(f0, rng, sigma, n=N_SAMPLES):
    """the clean six-partial tone of test_f0_extract_cpu under white noise of sigma `sigma`"""
    return tone(f0, n, rng, noise=0.0)[0] + rng.normal(0.0, sigma, n)
