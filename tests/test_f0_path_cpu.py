"""Pitch tracking as a path (include/visinger_hip.h "f12"): the restatement tests/f0_path_reference.py held to what the rule is for.  Plain YIN
(``yin_decide``) jumps an octave where a fundamental fades out and produces gross errors where noise lifts d' to the threshold; the Viterbi path through the
frames' lag candidates does neither, and on clean tones it is plain YIN.  Plus the tie rules on hand-made candidates, the host-side argument checks of
visinger_amd.pitch_track / synth, and the header.  No GPU.  SR 24000, hop 256, 48 frames + 77 samples, INNER = frames 4 .. 43 (test_f0_extract_cpu)."""
import os
import re

import numpy as np
import pytest

from f0_path_reference import (ABSENT, DEFAULTS, DIP_TONES, SEEDS, UNVOICED, candidates_ref, flicker, funddip, path_ref)
from test_f0_extract_cpu import FRAMES, GATED_PATTERN, HOP, INNER, SR, cents, make_signals, truth_at_centres, yin_decide, yin_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = (0.035, 0.045)


def track(x):
    """one fp32-rounded recording through both trackers: dict(yin, lag, cand_hz, cand_d, lags, path, state, cost)"""
    x = np.asarray(x, np.float32)
    dp, e, n_b = yin_frames(x)
    f0, per, lag = yin_decide(dp, e, n_b)
    hz, d, lags = candidates_ref(dp, e, n_b)
    f32, state, cost = path_ref(hz, d, len(x) // HOP)
    path = np.array([hz[t, s] if 0 <= s < UNVOICED else 0.0 for t, s in enumerate(state)])           # the chosen candidates in fp64
    assert np.array_equal(path.astype(np.float32), f32)
    return dict(yin=f0, lag=lag, cand_hz=hz, cand_d=d, lags=lags, path=path, state=state, cost=cost)


@pytest.fixture(scope="module")
def signals():
    return make_signals()


@pytest.fixture(scope="module")
def dips():
    return {(f, seed): track(funddip(f, np.random.default_rng(seed))) for f in DIP_TONES for seed in SEEDS}


@pytest.fixture(scope="module")
def clean(signals):
    return {(kind, f): track(x) for kind in ("steady", "vibrato") for f, (x, _) in signals[kind].items()}


@pytest.fixture(scope="module")
def others(signals):
    return {name: track(signals[name]) for name in ("noise", "zeros", "gated")}


def test_dip_plain_yin_jumps_an_octave_and_the_path_does_not(dips):
    """the fundamental and the third partial fade out over frames 20 .. 25.  Measured: plain YIN 4 INNER frames 1157 - 1212 cents off in all 15 cases; the path
    voiced throughout, worst 5.1 cents (98 Hz, where the lag grid is coarsest against the second partial's period)"""
    worst = 0.0
    for (f, seed), r in dips.items():
        off = cents(np.where(r["yin"][INNER] > 0, r["yin"][INNER], f), f)
        assert (off > 600).sum() >= 1, (f, seed)                                # the premise
        assert (r["path"][INNER] > 0).all(), (f, seed)
        err = cents(r["path"][INNER], f).max()
        worst = max(worst, err)
        assert err <= 8.0, (f, seed, err)
    print(f"dip: the path's worst error {worst:.2f} cents (bound 8)")


def test_flicker_no_voiced_frame_of_the_path_is_grossly_off():
    """a clean tone under white noise of sigma 0.035 / 0.045.  Measured: plain YIN 6 - 14 frames over 50 cents off in 7 of the 30 cases; the path's worst voiced
    frame 39.8 cents off"""
    worst, gross_cases = 0.0, 0
    for sigma in SIGMAS:
        for f in DIP_TONES:
            for seed in SEEDS:
                r = track(flicker(f, np.random.default_rng(seed), sigma))
                yv, pv = r["yin"][INNER] > 0, r["path"][INNER] > 0
                gross_cases += int(yv.any() and (cents(r["yin"][INNER][yv], f) > 50).sum() >= 6)
                if pv.any():
                    err = cents(r["path"][INNER][pv], f).max()
                    worst = max(worst, err)
                    assert err <= 50.0, (sigma, f, seed, err)
    print(f"flicker: the path's worst voiced frame {worst:.1f} cents off (bound 50); plain YIN has 6 or more gross errors in {gross_cases} of 30 cases")
    assert gross_cases >= 1                                                     # the premise: there is something to repair


def test_clean_tones_equal_plain_yin(clean, signals):
    for (kind, f), r in clean.items():
        assert (r["yin"][INNER] > 0).all() and np.array_equal(r["path"][INNER], r["yin"][INNER]), (kind, f)
        assert (r["state"] >= 0).all() and len(r["path"]) == FRAMES


def test_noise_and_zeros_are_unvoiced_and_the_gated_signal_differs_at_one_edge(others):
    for name in ("noise", "zeros"):
        assert (others[name]["path"] == 0).all() and (others[name]["state"] == UNVOICED).all(), name
    assert (others["zeros"]["cand_hz"] == 0).all() and (others["zeros"]["cand_d"] == 1).all()
    got = "".join("V" if v else "." for v in others["gated"]["path"] > 0)
    differs = [t for t, (a, b) in enumerate(zip(got, GATED_PATTERN)) if a != b]
    assert len(differs) <= 1, (got, differs)                                   # (w_switch is a hysteresis: a burst edge may move by a frame)


def test_plain_yin_s_choice_is_one_of_the_candidates(dips, clean, others):
    """a condition, not a share: on every voiced frame of the dip rows, the clean tones, noise, zeros and the gated signal -- 1872 frames -- the lag plain YIN
    decides on is among the frame's seven.  (Not so under heavy noise: flicker 523.3 Hz, seed 3, sigma 0.045 has one frame where YIN's grossly wrong lag 367 is
    the EIGHTH local minimum -- the path cannot, and should not, follow it there.)"""
    frames = misses = 0
    for r in list(dips.values()) + list(clean.values()) + list(others.values()):
        for t in range(len(r["yin"])):
            frames += 1
            if r["yin"][t] > 0 and not ((r["lags"][t] == r["lag"][t]).any() and (r["cand_hz"][t] == r["yin"][t]).any()):
                misses += 1
    print(f"containment: {misses} misses of {frames} frames")
    assert frames == 1872 and misses == 0


def test_candidates_are_ordered_local_minima_below_the_gate(signals):
    x = np.asarray(signals["vibrato"][146.8][0], np.float32)
    dp, e, n_b = yin_frames(x)
    hz, d, lags = candidates_ref(dp, e, n_b)
    assert hz.shape == d.shape == (FRAMES, 8) and (hz[:, 7] == 0).all() and (d[:, 7] == 1).all()
    for t in range(FRAMES):
        k = int((lags[t] > 0).sum())
        assert (lags[t, :k] > 0).all() and (np.diff(lags[t, :k]) > 0).all() and (hz[t, k:] == 0).all() and (d[t, k:] == 1).all()
        for tau, dv in zip(lags[t, :k], d[t, :k]):
            assert dv == dp[t, tau] < DEFAULTS["gate"] and dp[t, tau] <= dp[t, tau + 1] and (tau == 24 or dp[t, tau - 1] > dp[t, tau])
    # a frame beyond the length, a silent frame and a non-finite energy leave every slot empty; a gate below every d' leaves none
    hz2, d2, _ = candidates_ref(dp, np.where(np.arange(FRAMES) == 7, np.inf, np.where(np.arange(FRAMES) == 8, 0.0, e)), n_b - 5)
    assert (hz2[[7, 8]] == 0).all() and (hz2[n_b - 5:] == 0).all() and (d2[n_b - 5:] == 1).all() and np.array_equal(hz2[9:n_b - 5], hz[9:n_b - 5])
    assert (candidates_ref(dp, e, n_b, gate=1e-9)[0] == 0).all()


def cands(frames):
    """[T, 8] arrays from per-frame lists of (hz, d)"""
    hz, d = np.zeros((len(frames), 8), np.float32), np.ones((len(frames), 8), np.float32)
    for t, fr in enumerate(frames):
        for k, (h, dv) in enumerate(fr):
            hz[t, k], d[t, k] = h, dv
    return hz, d


def test_tie_rules_on_hand_made_candidates():
    a = 220.0
    # two identical candidates in every frame: the lower slot wins at the start (argmin), in the backpointers and at the end
    hz, d = cands([[(a, 0.05), (a, 0.05)]] * 3)
    f0, state, cost = path_ref(hz, d, w_order=0)
    assert state.tolist() == [0, 0, 0] and cost == 3 * 51 and (f0 == np.float32(a)).all()
    # ... and with w_order the later slot pays for its place
    assert path_ref(hz, d)[2] == 3 * 51 and path_ref(*cands([[(a, 0.9), (a, 0.05)]] * 3))[1].tolist() == [1, 1, 1]
    # voiced at exactly the price of unvoiced: the lower state, the voiced one
    hz, d = cands([[(a, 0.15625)]] * 3)                                         # rint(1024 * 0.15625) = 160 = w_unvoiced
    f0, state, cost = path_ref(hz, d)
    assert state.tolist() == [0, 0, 0] and cost == 480
    # an empty frame between two voiced ones: unvoiced there costs 160 + 2 * 96, the absent slot 16384
    hz, d = cands([[(a, 0.0)], [], [(a, 0.0)]])
    f0, state, cost = path_ref(hz, d)
    assert state.tolist() == [0, 7, 0] and cost == 160 + 2 * 96 and f0.tolist() == [a, 0.0, a]
    # ... and with switching dearer than 3 frames of unvoiced the path stays unvoiced throughout (loc 0 + 0 + 0 + 2 * 4096 against 3 * 160)
    assert path_ref(hz, d, w_switch=4096)[1].tolist() == [7, 7, 7]
    # an octave jump is capped: a -> 2a -> a costs 2 * min((192 * 32) >> 4, 384) + 24 = 792, staying on the dearer a (d = 0.5: 512) costs less
    # (unvoiced is priced out of it: at the defaults the middle frame would go unvoiced for 160 + 2 * 96)
    hz, d = cands([[(a, 0.0)], [(a, 0.5), (2 * a, 0.0)], [(a, 0.0)]])
    f0, state, cost = path_ref(hz, d, w_unvoiced=4096)
    assert state.tolist() == [0, 0, 0] and cost == 512 and path_ref(hz, d)[1].tolist() == [0, 7, 0] and path_ref(hz, d)[2] == 352
    assert path_ref(hz, d, w_unvoiced=4096, jump_cap=100)[1].tolist() == [0, 1, 0] and path_ref(hz, d, w_unvoiced=4096, jump_cap=100)[2] == 200 + 24
    # d is clamped, a NaN d counts as 1, hz that is not finite or not positive is an absent slot; slot 7 is not read
    hz, d = cands([[(a, -3.0)], [(a, np.nan)], [(np.inf, 0.0), (-a, 0.0), (np.nan, 0.0), (a, 7.0)]])
    hz[:, 7], d[:, 7] = 440.0, 0.0
    f0, state, cost = path_ref(hz, d, w_unvoiced=4096, w_switch=0)
    assert state.tolist() == [0, 0, 3] and cost == 0 + 1024 + 1024 + 3 * 24 and ABSENT > 4096
    # n: frames at or beyond it are not looked at; 0 frames cost 0
    hz, d = cands([[(a, 0.0)], [(a, 0.0)], [(2 * a, 0.0)]])
    f0, state, cost = path_ref(hz, d, n=2)
    assert state.tolist() == [0, 0, -1] and f0.tolist() == [a, a, 0.0] and cost == 0
    assert path_ref(hz, d, n=0)[1].tolist() == [-1, -1, -1] and path_ref(hz, d, n=0)[2] == 0 and path_ref(hz, d, n=-4)[2] == 0
    assert path_ref(hz, d, n=9)[1].tolist() == path_ref(hz, d)[1].tolist() == [0, 0, 7] and path_ref(hz, d, n=9)[2] == 96 + 160


def test_check_path_and_check_args():
    import torch
    from visinger_amd import pitch_track
    assert pitch_track.PATH_DEFAULTS == DEFAULTS and list(pitch_track.PATH_DEFAULTS) == ["gate", "w_unvoiced", "w_switch", "w_order", "w_jump", "jump_cap"]
    assert pitch_track.check_path() == (0.5, (160, 96, 24, 32, 384, 0)) and pitch_track.check_path(gate=1, w_jump=0, jump_cap=4096) == (1.0, (160, 96, 24, 0, 4096, 0))
    for bad in (dict(gate=0.0), dict(gate=-0.5), dict(gate=float("nan")), dict(gate=float("inf")), dict(gate="0.5"), dict(gate=None), dict(w_unvoiced=-1),
                dict(w_switch=4097), dict(w_order=1.5), dict(w_jump=True), dict(jump_cap="3"), dict(jump_cap=None)):
        with pytest.raises(ValueError):
            pitch_track.check_path(**bad)
        with pytest.raises(ValueError):
            pitch_track.check_args(HOP, SR, path=bad)
        with pytest.raises(ValueError):                                         # ... and before extract_f0 looks at the tensor
            pitch_track.extract_f0(torch.zeros(1, 1024), HOP, SR, path=bad)
    with pytest.raises(TypeError):
        pitch_track.check_path(bogus=1)
    for bad in (dict(bogus=1), dict(threshold=0.1), 3, "x", [("gate", 0.5)]):
        with pytest.raises(ValueError):
            pitch_track.check_args(HOP, SR, path=bad)
    assert pitch_track.check_args(HOP, SR, path={}) == pitch_track.check_args(HOP, SR, path=None) == pitch_track.check_args(HOP, SR) == 740
    assert pitch_track.check_args(HOP, SR, 65.0, 1000.0, None, 0.15, 1e-8, None, path=dict(gate=0.3)) == 740
    with pytest.raises(TypeError):                                              # path is a trailing keyword: the positional signature is what it was
        pitch_track.check_args(HOP, SR, 65.0, 1000.0, None, 0.15, 1e-8, None, {})
    with pytest.raises(ValueError):                                             # best_path: gate is candidates' keyword, refused before the tensors are looked at
        pitch_track.best_path(None, None, gate=0.5)
    with pytest.raises(ValueError):
        pitch_track.best_path(None, None, w_jump=-1)


def test_driver_takes_path_inside_guide_track():
    from visinger_amd import pitch_track, synth
    assert "path" in synth.OPTIONS["guide_track"][1] and list(synth.OPTIONS) == ["resample_to", "guide_dynamics", "limit", "guide_correct", "guide_align", "guide_track"]
    got = synth._option("guide_track", dict(sample_rate=SR, path={}), HOP)
    assert got == dict(sample_rate=SR, path={})
    assert synth._option("guide_track", dict(sample_rate=SR, path=dict(w_jump=16, gate=0.4)), HOP)["path"] == dict(w_jump=16, gate=0.4)
    assert synth._option("guide_track", dict(sample_rate=SR, path=None), HOP)["path"] is None
    for bad in (dict(bogus=1), dict(w_switch=-1), dict(gate=0), 5):
        with pytest.raises(ValueError):
            synth._option("guide_track", dict(sample_rate=SR, path=bad), HOP)
    item = dict(text_tokens=np.arange(1, 4), pitch_tokens=np.arange(1, 4), dur_tokens=np.arange(1, 4), mel2ph=np.repeat(np.arange(1, 4), 4))
    with pytest.raises(ValueError):                                             # ... through guide_items and synthesize, before the model is looked at
        synth.guide_items([dict(item, guide_wav=np.zeros(4096, np.float32))], HOP, "cpu", sample_rate=SR, path=dict(bogus=1))
    with pytest.raises(ValueError):
        synth.synthesize(None, [dict(item, guide_wav=np.zeros(4096, np.float32))], HOP, guide_track=dict(sample_rate=SR, path=dict(gate=-1)))
    # a recording of more than 32768 frames: refused by name, before any launch (there is no GPU here)
    long_ = np.zeros((pitch_track.PATH_FRAMES_LIMIT + 1) * 8, np.float32)
    with pytest.raises(ValueError, match="item 1"):
        synth.guide_items([dict(item), dict(item, guide_wav=long_)], 8, "cpu", sample_rate=SR, path={})
    assert pitch_track.PATH_FRAMES_LIMIT == 32768


def test_header_declares_both_symbols_and_the_range():
    text = open(os.path.join(ROOT, "include", "visinger_hip.h")).read()
    syms = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", text))
    assert {"vs_f0_candidates", "vs_f0_path", "vs_f0_yin"} <= syms
    assert "#define VS_F0_PATH_MAX_FRAMES 32768" in text and " f12 " in text and "2^31" in text[text.index(" f12 "):text.index("VS_API int vs_f0_path")]
    assert 32768 * (1024 + 6 * 4096 + 4096) < 2 ** 31
    from visinger_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "vs_f0_candidates") and hasattr(lib, "vs_f0_path") and len(lib.vs_f0_path.argtypes) == 15 and len(lib.vs_f0_candidates.argtypes) == 15
