"""The pitch tracker's rule (include/visinger_hip.h "f6") restated sequentially in fp64 numpy -- ``yin_ref``, the oracle of
tests/test_f0_extract_gpu.py -- and held to GROUND TRUTH: synthetic tones whose instantaneous frequency at every frame centre is known.  The project has no
reference implementation of a tracker, so the rule itself is what is tested here: steady tones within 1.5 cents, a 50-cent 5.5 Hz vibrato within 5 cents, noise
and silence unvoiced, and the voicing pattern of a gated signal.  Plus the host-side argument checks of visinger_amd.pitch_track and synth.guide_items."""
import math

import numpy as np
import pytest

SR, HOP, F0_MIN, F0_MAX, THR, SILENCE = 24000, 256, 65.0, 1000.0, 0.15, 1e-8
FRAMES, TAIL = 48, 77                                     # 48 frames and an odd tail: L is no multiple of the hop
TONES = (82.4, 110.0, 146.8, 196.0, 220.0, 293.7, 392.0, 523.3, 659.3, 830.6)
INNER = slice(4, FRAMES - 4)                              # the first and last 4 frames see the signal's edges
GATED_PATTERN = "V" * 14 + "." * 16 + "V" * 23 + "." * 6 + "V" * 20 + "." * 17


def lag_range(sr, f0_min, f0_max):
    return max(2, math.floor(sr / f0_max)), math.ceil(sr / f0_min)


def yin_frames(x, sr=SR, hop=HOP, f0_min=F0_MIN, f0_max=F0_MAX, window=None, length=None, frames=None):
    """steps 1-2 and the energy of step 4 for every frame of one row: d' [T, tau_max + 2] (column 0 unused), e [T], n_b.  fp64, written from the definition:
    samples outside [0, length) read as 0; d(tau) over the lag-centred window; S the running sum; d' = d tau / S where 0 < S < inf, else 1."""
    x = np.asarray(x, np.float64)
    n = len(x) if length is None else min(max(int(length), 0), len(x))
    tau_min, tau_max = lag_range(sr, f0_min, f0_max)
    W = 2 * tau_max if window is None else window
    T = len(x) // hop if frames is None else frames
    n_b = min(n // hop, T)
    pad = W + tau_max + 4
    xp = np.concatenate([np.zeros(pad), x[:n], np.zeros(pad + hop)])          # xp[pad + i] = x[i]
    taus = np.arange(1, tau_max + 2)
    j = np.arange(W)
    dp, e = np.ones((T, tau_max + 2)), np.zeros(T)
    for t in range(n_b):
        c = t * hop + hop // 2
        s = c - W // 2 - taus // 2
        a = xp[pad + s[:, None] + j[None, :]]
        b = xp[pad + s[:, None] + j[None, :] + taus[:, None]]
        with np.errstate(invalid="ignore", over="ignore"):
            d = ((a - b) ** 2).sum(1)
            S = np.cumsum(d)
            ok = (S > 0) & (S < np.inf)
            dp[t, 1:] = np.where(ok, d * taus / np.where(ok, S, 1.0), 1.0)
            e[t] = (xp[pad + c - W // 2 + j] ** 2).sum()
    return dp, e, n_b


def yin_decide(dp, e, n_b, sr=SR, f0_min=F0_MIN, f0_max=F0_MAX, window=None, threshold=THR, silence=SILENCE):
    """steps 3-5 on yin_frames' output: (f0 [T], periodicity [T], integer lag [T], 0 = unvoiced)"""
    tau_min, tau_max = lag_range(sr, f0_min, f0_max)
    W = 2 * tau_max if window is None else window
    T = len(dp)
    f0, per, lag = np.zeros(T), np.zeros(T), np.zeros(T, np.int64)
    for t in range(n_b):
        row = dp[t]
        if not np.isfinite(e[t]):
            continue
        g = tau_min + int(np.argmin(row[tau_min:tau_max + 1]))                # (numpy: the first minimum)
        per[t] = min(max(1.0 - row[g], 0.0), 1.0)
        if e[t] <= silence * W:
            continue
        below = np.nonzero(row[tau_min:tau_max + 1] < threshold)[0]
        if not len(below):
            continue
        p = tau_min + int(below[0])
        while p + 1 <= tau_max and row[p + 1] < row[p]:
            p += 1
        y0, y1, y2 = row[p - 1], row[p], row[p + 1]
        den = y0 - 2 * y1 + y2
        off = min(max(0.5 * (y0 - y2) / den, -0.5), 0.5) if den > 0 else 0.0
        f0[t], lag[t] = sr / (p + off), p
    return f0, per, lag


def yin_ref(x, sr=SR, hop=HOP, f0_min=F0_MIN, f0_max=F0_MAX, window=None, threshold=THR, silence=SILENCE, length=None, frames=None):
    dp, e, n_b = yin_frames(x, sr, hop, f0_min, f0_max, window, length, frames)
    return yin_decide(dp, e, n_b, sr, f0_min, f0_max, window, threshold, silence)


# ---- signals -------------------------------------------------------------------------------------------------------------------------------

def tone(f0, n, rng, vibrato=False, sr=SR, noise=1e-3):
    """(signal, instantaneous frequency per sample): six partials of amplitude 0.6^h with random phases, peak 0.2, white noise of sigma `noise` on top;
    vibrato: 50 cents at 5.5 Hz"""
    t = np.arange(n) / sr
    f = f0 * 2.0 ** (50.0 / 1200.0 * np.sin(2 * np.pi * 5.5 * t)) if vibrato else np.full(n, float(f0))
    phase = 2 * np.pi * (np.cumsum(f) - f) / sr
    x = sum(0.6 ** h * np.sin(h * phase + rng.uniform(0, 2 * np.pi)) for h in range(1, 7))
    x = 0.2 * x / np.abs(x).max()
    return x + rng.normal(0.0, noise, n), f


def make_signals():
    """every signal of the two f0 test files, from one seed: {"steady": {f: (x, f_inst)}, "vibrato": {...}, "noise": x, "zeros": x, "gated": x}"""
    rng = np.random.default_rng(20021)
    n = FRAMES * HOP + TAIL
    out = dict(steady={f: tone(f, n, rng) for f in TONES}, vibrato={f: tone(f, n, rng, vibrato=True) for f in TONES})
    out["noise"] = rng.normal(0.0, 0.1, n)
    out["zeros"] = np.zeros(n)
    out["gated"] = gated(rng)
    return out


def gated(rng):
    """96 frames: bursts at 220, 523.3 and 98 Hz with 400-sample fades, silence between them, white noise of sigma 0.05 at the end, all on a floor of 1e-4"""
    n = 96 * HOP + TAIL
    x = rng.normal(0.0, 1e-4, n)
    fade = 0.5 - 0.5 * np.cos(np.pi * np.arange(400) / 400)
    for f, a, b in ((220.0, 0, 14 * HOP), (523.3, 30 * HOP + 64, 52 * HOP + 64), (98.0, 57 * HOP + 128, 80 * HOP)):
        burst, _ = tone(f, b - a, rng, noise=0.0)
        burst[:400] *= fade
        burst[-400:] *= fade[::-1]
        x[a:b] += burst
    x[83 * HOP:] += rng.normal(0.0, 0.05, n - 83 * HOP)
    return x


@pytest.fixture(scope="module")
def signals():
    return make_signals()


def cents(f, truth):
    return 1200.0 * np.abs(np.log2(f / truth))


def truth_at_centres(f_inst, T, hop=HOP):
    return f_inst[np.arange(T) * hop + hop // 2]


def test_standard_setting():
    assert lag_range(SR, F0_MIN, F0_MAX) == (24, 370)


@pytest.mark.parametrize("kind,bound", [("steady", 1.5), ("vibrato", 5.0)])
def test_rule_against_ground_truth(signals, kind, bound):
    worst = 0.0
    for f, (x, f_inst) in signals[kind].items():
        f0, per, lag = yin_ref(x)
        assert len(f0) == FRAMES and (lag[INNER] > 0).all(), (kind, f)
        err = cents(f0[INNER], truth_at_centres(f_inst, FRAMES)[INNER]).max()
        worst = max(worst, err)
        assert err <= bound, (kind, f, err)
    print(f"{kind}: worst error of the rule in fp64 = {worst:.3f} cents (bound {bound})")


def test_noise_and_silence_are_unvoiced(signals):
    f0, per, lag = yin_ref(signals["noise"])
    assert (f0 == 0).all() and (lag == 0).all() and per.max() <= 0.35
    print(f"white noise: periodicity {per.min():.3f} .. {per.max():.3f}")
    f0, per, lag = yin_ref(signals["zeros"])
    assert (f0 == 0).all() and (per == 0).all()


def test_gated_signal_voicing_pattern(signals):
    f0, per, lag = yin_ref(signals["gated"])
    got = "".join("V" if v else "." for v in f0 > 0)
    assert got == GATED_PATTERN, got


def test_frames_beyond_the_length_and_outside_the_signal(signals):
    x = signals["steady"][220.0][0]
    f0, per, lag = yin_ref(x, length=10 * HOP + 5, frames=20)
    assert len(f0) == 20 and (f0[10:] == 0).all() and (per[10:] == 0).all() and (f0[2:8] > 0).all()
    full = yin_ref(x)[0]
    assert np.array_equal(f0[:7], full[:7])                                    # frames whose span ends before sample 10 * HOP + 5


# ---- host-side argument checks (no GPU) ---------------------------------------------------------------------------------------------------

def test_host_argument_checks():
    import torch
    from visinger_amd import _lib, pitch_track, synth
    assert pitch_track.lag_range(SR, F0_MIN, F0_MAX) == (24, 370)
    assert pitch_track.check_args(HOP, SR) == 740 and pitch_track.check_args(HOP, SR, window=370) == 370
    for bad in (dict(hop_size=0), dict(hop_size=2.5), dict(sample_rate=0), dict(f0_min=0.0), dict(f0_min=float("nan")), dict(f0_max=float("inf")),
                dict(f0_min=500.0, f0_max=400.0), dict(f0_min=400.0, f0_max=400.0), dict(f0_min=20.0), dict(f0_min=1000.0, f0_max=1100.0, sample_rate=2000),
                dict(window=369), dict(window=2049), dict(window=500.0), dict(threshold=0.0), dict(threshold=float("nan")),
                dict(silence=-1e-9), dict(silence=float("nan")), dict(frames=0)):
        kw = dict(dict(hop_size=HOP, sample_rate=SR), **bad)
        with pytest.raises(ValueError):
            pitch_track.check_args(**kw)
        with pytest.raises(ValueError):                                        # ... and before extract_f0 looks at the tensor
            pitch_track.extract_f0(torch.zeros(1, 1024), **kw)
    for wav in (torch.zeros(2, 1024), np.zeros((2, 1024), np.float32), torch.zeros(2, 1024, dtype=torch.int16), torch.zeros(1, 2, 1024)):
        with pytest.raises(_lib.VisingerHipError):                             # a CPU tensor, no tensor, no float tensor: there is no CPU path
            pitch_track.extract_f0(wav, HOP, SR)
    item = dict(text_tokens=np.arange(1, 4), pitch_tokens=np.arange(1, 4), dur_tokens=np.arange(1, 4), mel2ph=np.repeat(np.arange(1, 4), 4))
    wav = np.zeros(12 * HOP, np.float32)
    for items, track in (([dict(item, guide_wav=wav)], dict(f0_min=65.0)),                                        # no sample_rate
                         ([dict(item, guide_wav=wav, f0=np.zeros(12, np.float32))], dict(sample_rate=SR)),       # both
                         ([dict(item, guide_wav=wav[None])], dict(sample_rate=SR)),                              # not 1-D
                         ([dict(item, guide_wav=wav[:HOP - 1])], dict(sample_rate=SR)),                          # shorter than a hop
                         ([dict(item, guide_wav=wav)], dict(sample_rate=SR, frames=3)),                          # not a tracking keyword
                         ([dict(item, guide_wav=wav)], dict(sample_rate=SR, f0_min=5.0))):
        with pytest.raises(ValueError):
            synth.guide_items(items, HOP, "cpu", **track)
    same = synth.guide_items([item], HOP, "cpu", sample_rate=SR)               # nothing to track: copies, no device work
    assert same[0] is not item and same[0].keys() == item.keys() and all(same[0][k] is item[k] for k in item)
