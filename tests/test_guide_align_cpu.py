"""Guide alignment (include/visinger_hip.h "f7") restated in numpy from the header text, one item at a time: the oracle of
tests/test_guide_align_gpu.py, held here to what the rule is for -- a score's run boundaries recovered from a guide that was sung with another timing --
and to its own invariants.  No GPU."""
import os
import re

import numpy as np
import pytest

INF = (1 << 30) - 1
MAX_DUR = (1 << 24) - 1
WEIGHTS = dict(cap=64, w_voiced_rest=48, w_unvoiced_note=24, drift=32, drift_cap=64, octave_fold=False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------

def quantise_f0(f0):
    """(q [G] int64, voiced [G]): q_t = (int) rintf(clamp(192 log2f(f0 / 440), -40000, 40000)) + 1104 on finite f0 > 0, in fp32"""
    f0 = np.asarray(f0, np.float32)
    with np.errstate(invalid="ignore"):
        voiced = np.isfinite(f0) & (f0 > 0)
    x = np.float32(192) * np.log2(np.where(voiced, f0, np.float32(440)) / np.float32(440)).astype(np.float32)
    return np.rint(np.clip(x, -40000, 40000)).astype(np.int64) + 1104, voiced


def quantise_notes(note_midi):
    """(m [T_ph] int64, pitched [T_ph]): m_i = (int) rintf(min(16 note_midi, 2^20)) on finite note_midi > 0, in fp32"""
    note = np.asarray(note_midi, np.float32)
    with np.errstate(invalid="ignore"):
        pitched = np.isfinite(note) & (note > 0)
    m = np.rint(np.minimum(np.float32(16) * np.where(pitched, note, np.float32(1)), np.float32(1 << 20))).astype(np.int64)
    return m, pitched


def quantise_offset(offset_cents):
    oc = np.float32(offset_cents)
    if not np.isfinite(oc):
        return 0
    return int(np.rint(np.clip(oc * np.float32(0.16), np.float32(-(1 << 20)), np.float32(1 << 20))))


def share_run(n_s, d_s):
    """the run rule, as a literal sequential loop: frames of the k tokens of one run"""
    k, n, D_r = len(n_s), int(sum(n_s)), int(sum(d_s))
    E_prev, C, got = 0, 0, []
    for i in range(1, k + 1):
        C += int(d_s[i - 1])
        R = min((2 * C * n + D_r) // (2 * D_r), n - (k - i))
        E = max(E_prev + 1, R)
        got.append(E - E_prev)
        E_prev = E
    return got


def align_ref(f0_hz, note_midi, dur, g_len=None, offset_cents=0.0, cap=64, w_voiced_rest=48, w_unvoiced_note=24, drift=32, drift_cap=64,
              octave_fold=False, return_path=False):
    """one item: (dur_new int64 [T_ph], cost, status)"""
    f0_hz, dur = np.asarray(f0_hz, np.float32), np.asarray(dur, np.int64)
    Tg, T_ph = len(f0_hz), len(dur)
    G = Tg if g_len is None else int(min(max(int(g_len), 0), Tg))
    d_all = np.clip(dur, 0, MAX_DUR)
    active = np.flatnonzero(d_all > 0)
    S = len(active)
    if S == 0 or G < S:
        return np.maximum(dur, 0), -1, 1
    q, voiced = quantise_f0(f0_hz[:G])
    m_all, pitched_all = quantise_notes(note_midi)
    m, pitched, d = m_all[active], pitched_all[active], d_all[active]
    off = quantise_offset(offset_cents)
    a = np.cumsum(d) - d
    L = int(d.sum())

    def local(t):
        if voiced[t]:
            delta = np.abs(q[t] - m - off)
            if octave_fold:
                delta = delta % 192
                delta = np.minimum(delta, 192 - delta)
            pc = np.where(pitched, np.minimum(delta, cap), w_voiced_rest)
        else:
            pc = np.where(pitched, w_unvoiced_note, 0)
        u = (t * L) // G
        gap = np.maximum(0, np.maximum(a - u, u - (a + d - 1)))
        return pc + np.minimum((gap * drift) >> 8, drift_cap)

    D = np.full(S, INF, np.int64)
    D[0] = min(INF, int(local(0)[0]))
    adv = np.zeros((G, S), bool)
    for t in range(1, G):
        left = np.concatenate(([INF], D[:-1]))
        adv[t] = left < D                                                     # a tie stays
        adv[t, 0] = False
        D = np.minimum(INF, local(t) + np.where(adv[t], left, D))
    cost = int(D[S - 1])
    start = np.zeros(S + 1, np.int64)
    start[S] = G
    s = S - 1
    for t in range(G - 1, 0, -1):
        if adv[t, s]:
            start[s] = t
            s -= 1
    assert s == 0
    n = np.diff(start)
    key = np.where(pitched, m, -1)
    out = np.zeros(T_ph, np.int64)
    r0 = 0
    for s in range(1, S + 1):
        if s == S or key[s] != key[r0]:
            out[active[r0:s]] = share_run(n[r0:s], d[r0:s])
            r0 = s
    if return_path:
        return out, cost, 0, n
    return out, cost, 0


def share_run_closed(n_s, d_s):
    """the run rule as the kernel computes it: E_i - i = max(0, max_{j <= i}(R_j - j))"""
    k, n, D_r = len(n_s), int(sum(n_s)), int(sum(d_s))
    C = np.cumsum(np.asarray(d_s, np.int64))
    i = np.arange(1, k + 1)
    R = np.minimum((2 * C * n + D_r) // (2 * D_r), n - (k - i))
    E = i + np.maximum(0, np.maximum.accumulate(R - i))
    return np.diff(np.concatenate(([0], E))).tolist()


# ---- scores and guides ---------------------------------------------------------------------------------------------------------------------

FPS = 100.0                  # frames a second of the test guides (a 10 ms hop)


def hz_of_q(q, frac=0.25):
    """Hz whose 192 log2(f / 440) is (q - 1104) + frac: with frac = 0.25 fp32 rounding (about 1e-5 there) cannot move the quantisation"""
    return (440.0 * 2.0 ** ((np.asarray(q, np.float64) - 1104 + frac) / 192.0)).astype(np.float32)


def random_score(rng, notes=(6, 20), frames=(12, 60), rest_p=0.2, stretch=(0.6, 1.6)):
    """(note_midi [T_ph], dur [T_ph], runs): notes of `frames` frames, each a consonant token plus a vowel token of the same pitch, adjacent pitches at
    least a semitone apart, rests (one token) mixed in, never two in a row.  runs: (first token, tokens, midi or 0, score frames, stretched frames)"""
    note_midi, dur, runs = [], [], []
    last, was_rest = 0, True
    for _ in range(int(rng.integers(*notes))):
        if not was_rest and rng.random() < rest_p:
            n = int(rng.integers(*frames))
            runs.append((len(dur), 1, 0, n))
            note_midi.append(0.0)
            dur.append(n)
            was_rest = True
            continue
        while True:
            p = int(rng.integers(48, 77))
            if abs(p - last) >= 1:
                break
        last, was_rest = p, False
        n = int(rng.integers(*frames))
        c = int(rng.integers(2, max(3, n // 3)))
        runs.append((len(dur), 2, p, n))
        note_midi += [float(p), float(p)]
        dur += [c, n - c]
    runs = [r + (max(r[1], int(round(r[3] * rng.uniform(*stretch)))),) for r in runs]
    return np.array(note_midi, np.float32), np.array(dur, np.int64), runs


def guide_of(runs, rng=None, vibrato_cents=0.0, jitter_cents=0.0, octave_p=0.0, snap=False):
    """the guide of a score sung with the runs' stretched lengths: 0 on rests; cents of 5.5 Hz vibrato, of per-frame jitter, a share of frames an octave high.
    snap: every frame on the 1/16-semitone grid plus a quarter step (hz_of_q)"""
    out, t = [], 0
    for _, _, midi, _, n in runs:
        if midi == 0:
            out.append(np.zeros(n))
        else:
            cents = vibrato_cents * np.sin(2 * np.pi * 5.5 * (t + np.arange(n)) / FPS)
            if jitter_cents:
                cents = cents + rng.normal(0, jitter_cents, n)
            if octave_p:
                cents = cents + 1200.0 * (rng.random(n) < octave_p)
            hz = 440.0 * 2.0 ** ((midi - 69) / 12.0 + cents / 1200.0)
            out.append(hz_of_q(np.rint(192 * np.log2(hz / 440.0)) + 1104) if snap else hz)
        t += n
    return np.concatenate(out).astype(np.float32)


def run_boundaries(dur_new, runs):
    """(aligned, true) end frames of the runs"""
    ends = np.cumsum(dur_new)
    return np.array([ends[r[0] + r[1] - 1] for r in runs]), np.cumsum([r[4] for r in runs])


def worst_boundary_error(seed, count, **guide):
    rng = np.random.default_rng(seed)
    worst, exact = 0, 0
    for _ in range(count):
        note_midi, dur, runs = random_score(rng)
        f0 = guide_of(runs, rng, **{k: v for k, v in guide.items() if k != "octave_fold"})
        dur_new, cost, status = align_ref(f0, note_midi, dur, octave_fold=guide.get("octave_fold", False))
        assert status == 0 and dur_new.sum() == len(f0) and (dur_new[dur > 0] >= 1).all()
        got, true = run_boundaries(dur_new, runs)
        err = int(np.abs(got - true).max())
        worst, exact = max(worst, err), exact + (err == 0)
    return worst, exact


# ---- tests ---------------------------------------------------------------------------------------------------------------------------------

def test_clean_guides_give_every_run_boundary_exactly():
    worst, exact = worst_boundary_error(11, 60)
    assert worst == 0 and exact == 60


VIBRATO_WORST = 0            # measured by this test over its 60 scores: every boundary exact
OCTAVE_WORST = 1             # ... with 2 % of the frames an octave high: one frame (such a frame AT a boundary costs `cap` under either note)


def test_vibrato_and_jitter_move_a_boundary_by_at_most_the_measured_frames():
    """30-cent 5.5 Hz vibrato and 10-cent (sigma) jitter per frame, then the same with 2 % of the frames an octave high (no octave_fold: the cap bounds what a
    wild frame can cost; with the fold, notes an octave apart become one pitch): the worst run-boundary error over 60 scores each, printed, and held to the
    measured worst plus one frame."""
    worst, exact = worst_boundary_error(12, 60, vibrato_cents=30.0, jitter_cents=10.0)
    print(f"vibrato + jitter: worst boundary error {worst} frames, {exact} of 60 exact")
    worst_o, exact_o = worst_boundary_error(13, 60, vibrato_cents=30.0, jitter_cents=10.0, octave_p=0.02)
    print(f"... with 2 % octave errors: worst {worst_o} frames, {exact_o} of 60 exact")
    assert worst <= VIBRATO_WORST + 1 and worst_o <= OCTAVE_WORST + 1


def test_sums_and_floors():
    rng = np.random.default_rng(5)
    for _ in range(40):
        T_ph, G = int(rng.integers(1, 14)), int(rng.integers(1, 60))
        dur = rng.integers(-2, 9, T_ph)
        note = rng.choice([0.0, 60.0, 60.0, 62.0, 64.5, np.nan], T_ph)
        f0 = rng.choice([0.0, 261.6, 293.7, 339.3, -5.0], G)
        dur_new, cost, status = align_ref(f0, note, dur)
        S = int((dur > 0).sum())
        if S == 0 or G < S:
            assert status == 1 and cost == -1 and np.array_equal(dur_new, np.maximum(dur, 0))
        else:
            assert status == 0 and 0 <= cost < INF and dur_new.sum() == G and (dur_new[dur > 0] >= 1).all() and (dur_new[dur <= 0] == 0).all()


def test_an_unvoiced_guide_follows_the_score():
    """pitch says nothing (every token pitched, every frame unvoiced: 24 a frame wherever the path goes): the drift term alone decides, and with
    drift = 256 -- one unit per frame of gap -- an all-unvoiced guide of the score's own length returns the score's durations; of twice the length, twice"""
    dur = np.array([5, 0, 9, 3, 7], np.int64)
    note = np.array([60, 60, 62, 65, 64], np.float32)
    dur_new, cost, status = align_ref(np.zeros(24, np.float32), note, dur, drift=256)
    assert status == 0 and np.array_equal(dur_new, dur) and cost == 24 * 24
    dur_new, cost, status = align_ref(np.zeros(48, np.float32), note, dur, drift=256)
    assert status == 0 and np.array_equal(dur_new, 2 * dur) and cost == 48 * 24


def test_the_run_rule_against_its_closed_form():
    rng = np.random.default_rng(9)
    for _ in range(300):
        k = int(rng.integers(1, 9))
        d = rng.integers(1, 40, k)
        n = int(rng.integers(k, 5 * k + 60))
        cut = np.sort(rng.choice(np.arange(1, n), k - 1, replace=False)) if k > 1 else np.array([], int)
        n_s = np.diff(np.concatenate(([0], cut, [n])))
        a, b = share_run(n_s, d), share_run_closed(n_s, d)
        assert a == b and sum(a) == n and min(a) >= 1
    assert share_run([10], [3]) == [10] and share_run([7, 5], [2, 10]) == [2, 10] and share_run([1, 1], [50, 1]) == [1, 1]
    assert share_run([30, 30], [1, 1000]) == [1, 59]                              # R_1 = 0: the floor of one frame


def test_check_args():
    from visinger_amd import guide_align
    assert guide_align.check_args() == (64, 48, 24, 32, 64, 0, 0)
    assert guide_align.check_args(octave_fold=True, cap=0, drift_cap=4096) == (0, 48, 24, 32, 4096, 1, 0)
    for kw in (dict(cap=-1), dict(cap=4097), dict(drift=1.5), dict(w_voiced_rest=None), dict(w_unvoiced_note=True), dict(drift_cap=1 << 40),
               dict(octave_fold=2), dict(octave_fold="yes")):
        with pytest.raises(ValueError):
            guide_align.check_args(**kw)
    assert guide_align.workspace_bytes(3, 1024, 256) == 0 and guide_align.workspace_bytes(3, 1281, 256) == 3 * 1281 * 4 * 8
    assert guide_align.workspace_bytes(1, 65536, 1) == 65536 * 8 and guide_align.workspace_bytes(2, 5120, 64) == 0


def test_abi_is_still_7_and_the_export_is_declared():
    import ctypes
    from visinger_amd import _lib, guide_align
    text = open(os.path.join(ROOT, "include", "visinger_hip.h")).read()
    assert re.search(r"VS_API int vs_guide_align\(", text) and "* f7  guide alignment" in text
    assert int(re.search(r"#define\s+VS_GUIDE_ALIGN_LDS_WORDS\s+(\d+)", text).group(1)) == guide_align.LDS_WORDS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "vs_guide_align")
    lib = _lib.lib()
    assert lib.vs_abi_version() == _lib.EXPECTED_ABI == 7 and len(lib.vs_guide_align.argtypes) == 21


def test_arguments_are_validated_before_anything_is_launched():
    """VS_EINVAL cases on HOST pointers: no call here is valid, so nothing may reach the device (the full list, with outputs checked untouched, is in
    tests/test_guide_align_gpu.py)"""
    import ctypes
    from visinger_amd import _lib
    lib = _lib.lib()
    bufs = [(ctypes.c_int64 * 64)() for _ in range(6)]
    f0, note, dur, out, cost, status = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)

    def call(f0=f0, g_len=None, note=note, dur=dur, offs=None, weights=(64, 48, 24, 32, 64, 0, 0), out=out, cost=cost, status=status, work=None, nbytes=0,
             B=1, Tg=8, T_ph=4):
        return lib.vs_guide_align(f0, g_len, note, dur, offs, *weights, out, cost, status, work, nbytes, B, Tg, T_ph, None)

    for kw in (dict(f0=None), dict(out=None), dict(B=0), dict(T_ph=0), dict(T_ph=1025), dict(Tg=0), dict(Tg=65537), dict(weights=(4097, 48, 24, 32, 64, 0, 0)),
               dict(weights=(64, 48, 24, 32, 64, 2, 0)), dict(weights=(64, 48, 24, 32, 64, 0, 1)), dict(out=dur), dict(Tg=5121, T_ph=64)):
        assert call(**kw) == 1, kw
        assert b"vs_guide_align" in lib.vs_last_error()
