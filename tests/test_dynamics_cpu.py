"""The guide-dynamics rule (include/visinger_hip.h "f10") without a GPU: the numpy restatements ``level_ref`` (fp64 on the fp32 samples),
``offset_ref``, ``gain_ref`` and ``apply_ref`` -- written from the rule, not from the kernels -- their properties, the dB conversion, every host-side refusal of
visinger_amd/dynamics.py and of the driver's new keys, and every VS_EINVAL of the four entries with its string (the library loads without a GPU).
tests/test_dynamics_gpu.py holds the kernels to these restatements."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_MAX = 1 << 16
OFF_MAX = 1 << 17
K_MAX = 4096
UNITS_PER_DB = 256.0 / (10.0 * math.log10(2.0))


def units(db):
    return int(np.rint(db * UNITS_PER_DB))


def level_of_units(u):
    """fp32 power levels a quarter unit off the quantisation grid: 2^((u + 0.25) / 256) -- q(level) == u in fp32 and in fp64 alike"""
    return np.exp2((np.asarray(u, dtype=np.float64) + 0.25) / 256.0).astype(np.float32)


def level_ref(wav, hop, half=1, length=None, T=None):
    """fp64 mean-square power per frame of one row of fp32 samples: T values (default len // hop), 0 for t >= n_b and where the window's sum is not finite"""
    wav = np.asarray(wav, dtype=np.float32)
    ln = len(wav) if length is None else max(0, min(int(length), len(wav)))
    T = len(wav) // hop if T is None else int(T)
    nb = min(ln // hop, T)
    with np.errstate(over="ignore", invalid="ignore"):
        E = (wav[:nb * hop].astype(np.float64).reshape(nb, hop) ** 2).sum(axis=1)
    out = np.zeros(T)
    for t in range(nb):
        a, e = max(0, t - half), min(nb - 1, t + half)
        s = E[a:e + 1].sum()
        out[t] = s / ((e - a + 1) * hop) if np.isfinite(s) else 0.0
    return out


def quantise(p):
    """(q, has): q = rint(clamp(256 log2 p, -2^16, 2^16)) where p is finite and > 0"""
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    has = np.isfinite(p) & (p > 0)
    q = np.zeros(len(p), np.int64)
    q[has] = np.rint(np.clip(256.0 * np.log2(p[has]), -Q_MAX, Q_MAX)).astype(np.int64)
    return q, has


def deviations(guide, own, n=None, gate=units(-70.0)):
    """(d, active) over the row's T frames: frames at or beyond n are not active"""
    qg, hg = quantise(guide)
    qo, ho = quantise(own)
    n = len(qg) if n is None else max(0, min(int(n), len(qg)))
    active = hg & ho & (qg >= gate) & (qo >= gate) & (np.arange(len(qg)) < n)
    return np.where(active, qg - qo, 0), active


def offset_ref(guide, own, n=None, gate=units(-70.0)):
    d, active = deviations(guide, own, n, gate)
    n_act = int(active.sum())
    return ((2 * int(d.sum()) + n_act) // (2 * n_act) if n_act else 0), n_act


def gain_ref(guide, own, n=None, offset=0, gate=units(-70.0), window=12, depth_q=256, up=units(12.0), down=units(24.0)):
    """k over the row's T frames, S and N as differences of one prefix sum"""
    d, active = deviations(guide, own, n, gate)
    T = len(d)
    n = T if n is None else max(0, min(int(n), T))
    e = np.where(active, d - max(-OFF_MAX, min(OFF_MAX, int(offset))), 0)
    pe, pc = np.concatenate([[0], np.cumsum(e)]), np.concatenate([[0], np.cumsum(active.astype(np.int64))])
    t = np.arange(T)
    a, b = np.maximum(t - window, 0), np.minimum(t + window, max(n - 1, 0)) + 1
    S, N = pe[b] - pe[a], pc[b] - pc[a]
    ok = (t < n) & (N >= 1)
    m = (2 * S + N) // np.maximum(2 * N, 1)                       # numpy's // is floor division
    return np.where(ok, np.clip((depth_q * m + 128) // 256, -down, up), 0).astype(np.int64)


def gain_brute(guide, own, n=None, offset=0, gate=units(-70.0), window=12, depth_q=256, up=units(12.0), down=units(24.0)):
    d, active = deviations(guide, own, n, gate)
    T = len(d)
    n = T if n is None else max(0, min(int(n), T))
    k = np.zeros(T, np.int64)
    for t in range(n):
        us = [u for u in range(max(0, t - window), min(n - 1, t + window) + 1) if active[u]]
        if us:
            S, N = sum(int(d[u]) - int(offset) for u in us), len(us)
            m = math.floor((2 * S + N) / (2 * N)) if abs(S) < 1 << 40 else (2 * S + N) // (2 * N)
            assert m == (2 * S + N) // (2 * N)
            k[t] = max(-down, min(up, (depth_q * m + 128) // 256))
    return k


def apply_ref(x, k, hop, length=None):
    """(y, kappa): y = x 2^(kappa / (1024 hop)) in fp64 over the first n hop samples, x elsewhere; kappa int64 per sample (0 beyond n hop)"""
    x = np.asarray(x, dtype=np.float32)
    k = np.clip(np.asarray(k, dtype=np.int64), -K_MAX, K_MAX)
    ln = len(x) if length is None else max(0, min(int(length), len(x)))
    n = min(ln // hop, len(k))
    i = np.arange(n * hop, dtype=np.int64)
    a = 2 * i + 1 - hop
    t0 = a // (2 * hop)
    w = a - 2 * hop * t0
    kappa = np.zeros(len(x), np.int64)
    if n:
        kappa[:n * hop] = k[np.clip(t0, 0, n - 1)] * (2 * hop - w) + k[np.clip(t0 + 1, 0, n - 1)] * w
    with np.errstate(invalid="ignore", over="ignore"):
        y = x.astype(np.float64) * np.exp2(kappa / (1024.0 * hop))
    return y, kappa


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------------------

def test_quarter_unit_levels_quantise_alike_in_fp32_and_fp64():
    """the margin the GPU tests' bit-for-bit comparison rests on: over u in [-9000, 2000] the fp32 level 2^((u + 0.25) / 256) gives q == u whether 256 log2 is
    taken in fp32 or fp64, and 256 log2 of it stays within 256 2^-24 / ln 2 = 2.2e-5 of u + 0.25 (the level's own rounding to fp32) -- a quarter unit from either
    rounding edge"""
    u = np.arange(-9000, 2001)
    p = level_of_units(u)
    x64 = 256.0 * np.log2(p.astype(np.float64))
    x32 = np.float32(256.0) * np.log2(p)                         # fp32 log2, one fp32 product
    assert x32.dtype == np.float32
    assert np.array_equal(np.rint(x64), u) and np.array_equal(np.rint(x32), u) and np.array_equal(quantise(p)[0], u)
    margin = np.abs(x64 - (u + 0.25)).max()
    print(f"256 log2 of the fp32 levels: at most {margin:.2e} units from u + 0.25; fp32 evaluation at most {np.abs(x32 - x64).max():.2e} from fp64")
    assert margin <= 256.0 * 2.0 ** -24 / math.log(2.0) and np.abs(x32 - x64).max() < 0.2


def test_gain_ref_equals_the_brute_force_windowed_mean():
    rng = np.random.default_rng(1)
    for T, window in ((1, 0), (7, 3), (60, 0), (60, 1), (61, 7), (90, 40), (50, 1024)):
        u_own = rng.integers(-6000, -1000, T)
        guide, own = level_of_units(u_own + rng.integers(-900, 900, T)), level_of_units(u_own)
        guide[rng.random(T) < 0.2] = 0.0                          # frames without a level
        own[rng.random(T) < 0.1] = level_of_units(-8000)          # ... and below the gate
        for n, offset, depth_q in ((None, 0, 256), (T // 2, 37, 200), (T, -411, 77), (0, 5, 256)):
            kw = dict(n=n, offset=offset, window=window, depth_q=depth_q, up=300, down=500)
            assert np.array_equal(gain_ref(guide, own, **kw), gain_brute(guide, own, **kw)), (T, window, kw)


def test_gain_properties():
    rng = np.random.default_rng(2)
    T = 400
    u_own = rng.integers(-3000, -1000, T)
    own = level_of_units(u_own)
    guide = level_of_units(u_own + rng.integers(-700, 700, T))
    assert gain_ref(guide, own).any() and not gain_ref(guide, own, depth_q=0).any()                     # depth = 0
    # the own curve times a constant as the guide: contour mode takes the constant out, absolute mode applies it, limited
    for c in (-2500, -300, 0, 450, 2000):
        louder = level_of_units(u_own + c)
        off, n_act = offset_ref(louder, own)
        assert (off, n_act) == (c, T)
        assert not gain_ref(louder, own, offset=off).any()
        assert (gain_ref(louder, own) == max(-units(24.0), min(units(12.0), c))).all()
    assert (gain_ref(level_of_units(u_own + 900), own, depth_q=128) == 450).all()
    # the limits
    k = gain_ref(guide, own, window=0, up=100, down=50)
    assert k.max() == 100 and k.min() == -50
    # the gate: frames below it on either curve are not active and take their neighbours' mean; a gap longer than the window gets 0
    gated = own.copy()
    gated[100:140] = level_of_units(units(-70.0) - 1)
    d, active = deviations(guide, gated)
    assert not active[100:140].any() and active[:100].all() and active[140:].all()
    k = gain_ref(guide, gated, window=12)
    assert not k[113:127].any() and k[112] == gain_brute(guide, gated, window=12)[112] and np.array_equal(k, gain_brute(guide, gated, window=12))
    at_gate = level_of_units(np.full(T, units(-70.0)))
    assert deviations(at_gate, at_gate)[1].all() and not deviations(at_gate, level_of_units(np.full(T, units(-70.0) - 1)))[1].any()
    # an all-zero guide, values that are no level, lengths
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert not gain_ref(np.full(T, bad, np.float32), own).any() and offset_ref(np.full(T, bad, np.float32), own) == (0, 0)
    assert not gain_ref(guide, own, n=150)[150:].any() and gain_ref(guide, own, n=150)[:150].any() and offset_ref(guide, own, n=0) == (0, 0)
    assert offset_ref(guide, own, n=150) == offset_ref(guide[:150], own[:150])
    assert np.array_equal(gain_ref(guide, own, n=150)[:150], gain_ref(guide[:150], own[:150]))


def test_apply_ref_is_continuous_at_frame_centres_and_held_at_the_ends():
    hop, k = 50, np.array([0, 512, -512, 1024, 1024, 3])
    x = np.ones(len(k) * hop + 30, np.float32)
    y, kappa = apply_ref(x, k, hop)
    lvl = kappa / (2.0 * hop)                                     # the gain in units per sample
    assert (lvl[:hop // 2] == 0).all() and (lvl[5 * hop + hop // 2:6 * hop] == 3).all() and (kappa[6 * hop:] == 0).all() and (y[6 * hop:] == 1).all()
    for t in range(len(k) - 1):                                   # linear in level between the centres t hop + (hop - 1) / 2: the line through k[t], k[t + 1]
        i = np.arange(t * hop + hop // 2, (t + 1) * hop + hop // 2)
        assert np.allclose(lvl[i], k[t] + (k[t + 1] - k[t]) * (i - (t * hop + (hop - 1) / 2.0)) / hop, rtol=0, atol=1e-9)
    assert np.abs(np.diff(lvl[:6 * hop])).max() <= 1536.0 / hop + 1e-9          # no step larger than the steepest ramp's
    assert abs(y[hop + hop // 2] / 2.0 ** ((512 + (-1024) * 0.5 / hop) / 512.0) - 1) < 1e-12
    # odd and even hops: the weight w lies in [0, 2 hop) and t0 = -1 before the first centre
    for hop in (1, 2, 3, 256):
        y, kappa = apply_ref(np.ones(4 * hop, np.float32), [512, 512, -256, -256], hop)
        assert (kappa[:hop] == 1024 * hop).all() and (kappa[3 * hop:] == -512 * hop).all() and (y[:hop] == 2.0).all()
    # k is read clamped, a length cuts whole frames, zero gain and the tail are x itself
    y, kappa = apply_ref(np.full(100, 3.0, np.float32), [100000, -100000], 10, length=19)
    assert (kappa[:5] == K_MAX * 20).all() and (kappa[10:] == 0).all() and (y[10:] == 3.0).all()


def test_level_ref():
    rng = np.random.default_rng(3)
    x = (0.3 * rng.standard_normal(2000)).astype(np.float32)
    lv = level_ref(x, 100, half=0)
    assert lv.shape == (20,) and np.allclose(lv, (x.astype(np.float64).reshape(20, 100) ** 2).mean(axis=1), rtol=1e-15)
    lv1 = level_ref(x, 100, half=1)
    assert np.isclose(lv1[0], lv[:2].mean()) and np.isclose(lv1[5], lv[4:7].mean()) and np.isclose(lv1[19], lv[18:].mean())
    assert np.allclose(level_ref(np.full(999, 0.5, np.float32), 50, half=8), 0.25) and len(level_ref(np.zeros(999), 50)) == 19
    cut = level_ref(x, 100, half=1, length=1250, T=25)
    assert cut.shape == (25,) and np.array_equal(cut[:12], level_ref(x[:1200], 100, half=1)) and not cut[12:].any()
    bad = x.copy()
    bad[730] = np.nan
    lb = level_ref(bad, 100, half=1)
    assert (lb[6:9] == 0).all() and np.array_equal(np.delete(lb, [6, 7, 8]), np.delete(lv1, [6, 7, 8]))
    sine = np.sin(2 * np.pi * 220 * np.arange(24000) / 24000.0).astype(np.float32)
    assert np.abs(level_ref(sine, 300) - 0.5).max() < 0.02


# ---- the module ---------------------------------------------------------------------------------------------------------------------------------------

def test_db_to_units_and_check_args():
    from visinger_amd import dynamics as dy
    assert abs(dy.UNITS_PER_DB - 85.04136) < 1e-5
    assert [dy.db_to_units(v) for v in (0, 3.0102999566398120, 12.0, 24.0, -70.0, 6.0205999132796239, 48.0)] == [0, 256, 1020, 2041, -5953, 512, 4082]
    for db in (-123.4, -0.5, 0.004, 17.0):
        assert dy.db_to_units(db) == int(np.rint(np.float64(db) * 256.0 / (10.0 * np.log10(2.0))))
    assert dy.DEFAULTS == dict(half_width=1, window=12, depth=1.0, max_boost_db=12.0, max_cut_db=24.0, gate_db=-70.0, mode="contour")
    assert dy.check_args() == dy.check_args(**dy.DEFAULTS) == (1, 12, 256, 1020, 2041, -5953, True)
    assert dy.check_args(half_width=8, window=1024, depth=0.5, max_boost_db=0, max_cut_db=48.16, gate_db=-770, mode="absolute") == (8, 1024, 128, 0, 4096, -65482, False)
    for bad in (dict(half_width=-1), dict(half_width=9), dict(half_width=1.0), dict(half_width=True), dict(window=-1), dict(window=1025), dict(window=2.5),
                dict(depth=-0.1), dict(depth=1.01), dict(depth=float("nan")), dict(depth="1"), dict(max_boost_db=-1), dict(max_boost_db=48.2), dict(max_cut_db=-0.5),
                dict(max_cut_db=49), dict(max_cut_db=float("inf")), dict(gate_db=-771), dict(gate_db=771), dict(gate_db=None), dict(mode="shape"), dict(mode=None),
                dict(mode=1)):
        with pytest.raises(ValueError):
            dy.check_args(**bad)
    with pytest.raises(TypeError):
        dy.check_args(bogus=1)


def test_python_constants_are_the_headers():
    from visinger_amd import _lib
    from visinger_amd import dynamics as dy
    header = open(os.path.join(ROOT, "include", "visinger_hip.h")).read()
    assert int(re.search(r"#define VS_LEVEL_GAIN_TILE (\d+)", header).group(1)) == dy.TILE == 1024
    assert _lib.EXPECTED_ABI == 7 == _lib.lib().vs_abi_version()                                       # the new entries join ABI 7
    f10 = re.sub(r"\s*\n \*\s*", " ", header[header.index(" * f10 "):header.index("#define VS_LEVEL_GAIN_TILE")])
    for text in ("hop outside [1, 4096]", "half outside [0, 8]", "T in [1, 65536]", "window in [0, 1024]", "depth_q in [0, 256]", "up and down in [0, 4096]",
                 "gate in [-2^16, 2^16]", "clamped to [-2^17, 2^17]", "clamped to [-4096, 4096]", "hop outside [1, 2048]", "|2 S + N| < 2^31"):
        assert text in f10, text
    assert (dy.TRACK_HOP_LIMIT, dy.HALF_LIMIT, dy.T_LIMIT, dy.WINDOW_LIMIT, dy.GAIN_LIMIT, dy.GATE_LIMIT, dy.OFFSET_LIMIT, dy.HOP_LIMIT) == \
        (4096, 8, 65536, 1024, 4096, 1 << 16, 1 << 17, 2048)
    for name in ("vs_level_track", "vs_level_offset", "vs_level_gain", "vs_level_apply"):
        assert f"VS_API int {name}(" in header and hasattr(_lib.lib(), name)


def test_the_module_refuses_before_it_needs_a_gpu():
    import torch
    from visinger_amd import dynamics as dy
    from visinger_amd._lib import VisingerHipError
    wav, lvl, k = torch.zeros(2, 1000), torch.zeros(2, 10), torch.zeros(2, 10, dtype=torch.int32)
    for kw in (dict(hop_size=0), dict(hop_size=4097), dict(hop_size=100.0), dict(hop_size=True), dict(half_width=9), dict(half_width=-1), dict(frames=0),
               dict(frames=2.5)):
        with pytest.raises(ValueError):
            dy.track_level(wav, **dict(dict(hop_size=100), **kw))
    for bad in (-800, 800, "x", None):
        with pytest.raises(ValueError):
            dy.level_offset(lvl, lvl, gate_db=bad)
    for kw in (dict(window=-1), dict(depth=2), dict(max_boost_db=49), dict(max_cut_db=-1), dict(gate_db=1e4), dict(mode="x"), dict(half_width=99), dict(bogus=1)):
        with pytest.raises(ValueError):
            dy.level_gain(lvl, lvl, **kw)
        with pytest.raises(ValueError):
            dy.match_dynamics(wav, lvl, 100, **kw)
    for hop in (0, 2049, 4096, 1.5, None):
        with pytest.raises(ValueError):
            dy.apply_gain(wav, k, hop)
        with pytest.raises(ValueError):
            dy.match_dynamics(wav, lvl, hop)
    # no CPU path, whatever the values
    for call in (lambda: dy.track_level(wav, 100), lambda: dy.track_level(wav.numpy(), 100), lambda: dy.track_level(None, 100),
                 lambda: dy.level_offset(lvl, lvl), lambda: dy.level_gain(lvl, lvl), lambda: dy.apply_gain(wav, k, 100), lambda: dy.match_dynamics(wav, lvl, 100),
                 lambda: dy.track_level(wav.double(), 100), lambda: dy.level_gain(lvl.numpy(), lvl)):
        with pytest.raises(VisingerHipError):
            call()


def test_the_driver_refuses_the_new_keys():
    from visinger_amd import synth
    item = dict(text_tokens=np.array([1, 2]), pitch_tokens=np.array([1, 2]), dur_tokens=np.array([2, 2]), mel2ph=np.array([1, 1, 2, 2]))
    for bad in ([1], 3, "contour", dict(bogus=1), dict(window=-1), dict(depth=1.5), dict(max_boost_db=100), dict(max_cut_db=-1), dict(gate_db=float("nan")),
                dict(mode="relative"), dict(half_width=9), dict(sample_rate=24000)):
        with pytest.raises(ValueError):
            synth.synthesize(None, [item], 8, guide_dynamics=bad)           # (refused before the model is looked at)
    with pytest.raises(ValueError, match="hop_size"):
        synth.synthesize(None, [item], 4096, guide_dynamics={})
    with pytest.raises(ValueError, match="guide_dynamics"):                  # a level curve in a call that would drop it
        synth.synthesize(None, [dict(item, level=np.ones(4, np.float32))], 8)
    rec = np.zeros(4096, np.float32)
    track = dict(sample_rate=24000, f0_min=65, f0_max=1000)
    for level in (-1, 9, 1.0, True, "1"):
        with pytest.raises(ValueError):
            synth.guide_items([dict(item, guide_wav=rec)], 8, "cpu", level=level, **track)
    with pytest.raises(ValueError, match="guide_track takes"):               # the whitelist of guide_track is what it was
        synth.guide_items([dict(item, guide_wav=rec)], 8, "cpu", half_width=1, **track)
    with pytest.raises(ValueError, match="level"):
        synth.retime_items([dict(item, level=np.ones(3, np.float32))], 2.0, "cpu")


def test_every_einval_of_the_four_entries_with_its_string():
    """the entries validate before they launch, so their refusals are checked without a GPU, on fake addresses"""
    from visinger_amd import _lib
    L = _lib.lib()
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    WAV, LENS, LEVEL, OWN, K, OFF, NACT, OFFS, Y = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000, 0x900000

    def run(call, good, bad, name):
        for word, cases in bad.items():
            for kw in cases:
                assert call(**dict(good, **kw)) == 1, (name, kw)                # VS_EINVAL
                err = L.vs_last_error().decode()
                assert name in err and word in err, (kw, err)

    track = lambda **a: L.vs_level_track(p(a["wav"]), p(a["lens"]), a["B"], a["L"], a["hop"], a["half"], p(a["level"]), a["T"], None)
    run(track, dict(wav=WAV, lens=LENS, B=2, L=4096, hop=256, half=1, level=LEVEL, T=16),
        {"NULL": [dict(wav=None), dict(level=None)], "overlaps": [dict(level=WAV), dict(level=WAV + 4 * 5000), dict(level=LENS), dict(level=LENS + 8)],
         "positive": [dict(B=0), dict(B=-1), dict(L=0), dict(T=0), dict(T=-5)], "2^31": [dict(L=1 << 31), dict(T=1 << 31), dict(B=1 << 61)],
         "hop": [dict(hop=0), dict(hop=-1), dict(hop=4097)], "half": [dict(half=-1), dict(half=9)]}, "vs_level_track")

    offset = lambda **a: L.vs_level_offset(p(a["guide"]), p(a["own"]), p(a["lens"]), a["gate"], p(a["off"]), p(a["nact"]), a["B"], a["T"], None)
    run(offset, dict(guide=LEVEL, own=OWN, lens=LENS, gate=-5953, off=OFF, nact=NACT, B=2, T=1000),
        {"NULL": [dict(guide=None), dict(own=None), dict(off=None), dict(nact=None)],
         "overlaps an input": [dict(off=LEVEL), dict(off=LEVEL + 4000), dict(nact=OWN), dict(off=LENS), dict(nact=LENS + 8)], "off and n_act overlap": [dict(nact=OFF), dict(nact=OFF + 4)],
         "1 <= T": [dict(B=0), dict(T=0), dict(T=65537), dict(B=-3)], "gate": [dict(gate=-65537), dict(gate=65537)]}, "vs_level_offset")

    gain = lambda **a: L.vs_level_gain(p(a["guide"]), p(a["own"]), p(a["lens"]), p(a["offs"]), a["gate"], a["window"], a["depth_q"], a["up"], a["down"], a["reserved"],
                                       p(a["k"]), a["B"], a["T"], None)
    run(gain, dict(guide=LEVEL, own=OWN, lens=LENS, offs=OFFS, gate=-5953, window=12, depth_q=256, up=1020, down=2041, reserved=0, k=K, B=2, T=1000),
        {"NULL": [dict(guide=None), dict(own=None), dict(k=None)], "overlaps": [dict(k=LEVEL), dict(k=OWN + 4 * 1999), dict(k=LENS), dict(k=OFFS + 4)],
         "1 <= T": [dict(B=0), dict(T=0), dict(T=65537)], "gate": [dict(gate=-65537), dict(gate=65537)], "window": [dict(window=-1), dict(window=1025)],
         "depth_q": [dict(depth_q=-1), dict(depth_q=257)], "up =": [dict(up=-1), dict(up=4097), dict(down=-1), dict(down=4097)],
         "reserved": [dict(reserved=1), dict(reserved=-1)]}, "vs_level_gain")

    apply = lambda **a: L.vs_level_apply(p(a["x"]), p(a["k"]), p(a["lens"]), a["hop"], p(a["y"]), a["B"], a["L"], a["T"], None)
    run(apply, dict(x=WAV, k=K, lens=LENS, hop=256, y=Y, B=2, L=4096, T=16),
        {"NULL": [dict(x=None), dict(k=None), dict(y=None)], "in place": [dict(y=WAV + 4), dict(y=WAV + 4 * 8191), dict(y=WAV - 4)],
         "overlaps k or lengths": [dict(y=K), dict(y=K - 4 * 8000), dict(y=LENS)], "positive": [dict(B=0), dict(L=0), dict(T=0)],
         "2^31": [dict(L=1 << 31), dict(T=1 << 31), dict(B=1 << 61)], "hop": [dict(hop=0), dict(hop=2049), dict(hop=4096)]}, "vs_level_apply")
