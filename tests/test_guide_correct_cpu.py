"""Guide pitch correction (include/visinger_hip.h "f8") restated in numpy from the header text: ``correct_ref`` / ``deviation_ref``, the oracle
of tests/test_guide_correct_gpu.py -- vectorised with prefix sums, held here to the literal per-frame loop -- and the rule itself held to what it is for:
synthetic singing (detuned notes with vibrato and jitter) lands on the score and keeps its vibrato.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OCTAVE = 19200               # units of 1/16 cent
LIM = 1 << 22
FPS = 100.0                  # frames a second of the synthetic singing (a 10 ms hop)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------

def c_ints(**params):
    """window, strength_q, vibrato_q, wild, octave_fold of the C call from correct_guide's keywords"""
    from visinger_amd import guide_correct
    return guide_correct.check_args(**params)[:5]


def quantise(f0_hz, mel2ph, note_midi, length=None, offset_cents=0.0, wild=4800, octave_fold=False):
    """one item: (d int64 [T], correctable bool [T], m int64 [T], pitched bool [T]) -- pitched / correctable are False at t >= n"""
    f0, tok, note = np.asarray(f0_hz, np.float32), np.asarray(mel2ph, np.int64), np.asarray(note_midi, np.float32)
    T, T_ph = len(f0), len(note)
    n = T if length is None else int(min(max(int(length), 0), T))
    has = (tok >= 1) & (tok <= T_ph) & (np.arange(T) < n)
    nt = note[np.clip(tok, 1, T_ph) - 1]
    with np.errstate(invalid="ignore"):
        pitched = has & np.isfinite(nt) & (nt > 0)
        voiced = np.isfinite(f0) & (f0 > 0)
    m = np.rint(np.clip(np.float32(1600) * (np.where(pitched, nt, np.float32(69)) - np.float32(69)), -LIM, LIM)).astype(np.int64)
    x = np.float32(OCTAVE) * np.log2(np.where(voiced, f0, np.float32(440)) / np.float32(440)).astype(np.float32)
    q = np.rint(np.clip(x, -LIM, LIM)).astype(np.int64)
    oc = np.float32(offset_cents)
    with np.errstate(over="ignore"):
        off = int(np.rint(np.clip(np.float32(16) * oc, -LIM, LIM))) if np.isfinite(oc) else 0
    d = q - m - off
    if octave_fold:
        d = d - OCTAVE * ((d + OCTAVE // 2) // OCTAVE)
    return d, pitched & voiced & (np.abs(d) <= wild), m, pitched


def apply_units(f0_hz, k):
    """f0 exp2f((float)(-k) / 19200.0f) in fp32 where k != 0, the input's bits elsewhere"""
    f0 = np.asarray(f0_hz, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        moved = (f0 * np.exp2((-k).astype(np.float32) / np.float32(OCTAVE)).astype(np.float32)).astype(np.float32)
    return np.where(k != 0, moved, f0)


def correct_ref(f0_hz, mel2ph, note_midi, length=None, offset_cents=0.0, **params):
    """one item: (k int64 [T], f0_out fp32 [T]); windowed sums as differences of prefix sums, segment limits by a prefix max and a suffix min"""
    W, a, vq, wild, fold = c_ints(**params)
    b = 256 - vq
    d, corr, m, pitched = quantise(f0_hz, mel2ph, note_midi, length, offset_cents, wild, bool(fold))
    T = len(d)
    t = np.arange(T)
    joins = np.zeros(T, bool)                                                 # frame t continues the segment of t - 1
    joins[1:] = pitched[1:] & pitched[:-1] & (m[1:] == m[:-1])
    seg_lo = np.maximum.accumulate(np.where(joins, -1, t))
    ends = np.ones(T, bool)
    ends[:-1] = ~joins[1:]
    seg_hi = np.minimum.accumulate(np.where(ends, t, T)[::-1])[::-1]
    pd, pc = np.concatenate(([0], np.cumsum(np.where(corr, d, 0)))), np.concatenate(([0], np.cumsum(corr)))
    lo, hi = np.maximum(t - W, seg_lo), np.minimum(t + W, seg_hi)
    S, N = pd[hi + 1] - pd[lo], np.maximum(pc[hi + 1] - pc[lo], 1)
    s = (2 * S + N) // (2 * N)
    k = np.where(corr, (a * s + b * (d - s) + 128) // 256, 0)
    return k, apply_units(f0_hz, k)


def correct_loop(f0_hz, mel2ph, note_midi, length=None, offset_cents=0.0, **params):
    """the same, as the header reads: one frame at a time, walking its segment"""
    W, a, vq, wild, fold = c_ints(**params)
    b = 256 - vq
    d, corr, m, pitched = quantise(f0_hz, mel2ph, note_midi, length, offset_cents, wild, bool(fold))
    T = len(d)
    k = np.zeros(T, np.int64)
    for t in range(T):
        if not corr[t]:
            continue
        S, N = 0, 0
        u = t
        while u >= 0 and t - u <= W and pitched[u] and m[u] == m[t]:
            if corr[u]:
                S, N = S + int(d[u]), N + 1
            u -= 1
        u = t + 1
        while u < T and u - t <= W and pitched[u] and m[u] == m[t]:
            if corr[u]:
                S, N = S + int(d[u]), N + 1
            u += 1
        s = (2 * S + N) // (2 * N)
        k[t] = (a * s + b * (int(d[t]) - s) + 128) // 256
    return k, apply_units(f0_hz, k)


def deviation_ref(f0_hz, mel2ph, note_midi, length=None, offset_cents=0.0, wild_cents=300.0, octave_fold=False):
    """one item: (dev_med, n_corr)"""
    _, _, _, wild, fold = c_ints(wild_cents=wild_cents, octave_fold=octave_fold)
    d, corr, _, _ = quantise(f0_hz, mel2ph, note_midi, length, offset_cents, wild, bool(fold))
    vals = np.sort(d[corr])
    return (int(vals[(len(vals) - 1) // 2]) if len(vals) else 0), len(vals)


# ---- test curves ---------------------------------------------------------------------------------------------------------------------------

def hz_of_units(q, frac=0.25):
    """Hz whose 19200 log2(f / 440) is q + frac: with frac = 0.25 fp32 rounding (about 0.004 there) cannot move the quantisation"""
    return (440.0 * 2.0 ** ((np.asarray(q, np.float64) + frac) / OCTAVE)).astype(np.float32)


def units_of_hz(f0):
    return OCTAVE * np.log2(np.asarray(f0, np.float64) / 440.0)


def random_item(rng, T, T_ph, seg=(1, 40), rest_p=0.15, unvoiced_p=0.1, wild_p=0.05, spread=1200, odd_tokens=False):
    """(f0 [T], mel2ph [T], note_midi [T_ph]): tokens of `seg` frames in score order (a token id may be skipped), pitches on whole and quarter semitones with
    equal neighbours frequent, the curve within `spread` units of its note on the quarter-unit grid, some frames unvoiced, some far off"""
    note = (60 + rng.integers(-8, 9, T_ph) / 4.0).astype(np.float32)
    same = rng.random(T_ph) < 0.4
    for i in range(1, T_ph):
        if same[i]:
            note[i] = note[i - 1]
    note[rng.random(T_ph) < rest_p] = 0.0
    mel2ph = np.zeros(T, np.int64)
    t, tok = 0, 1
    while t < T and tok <= T_ph:
        n = int(rng.integers(seg[0], seg[1] + 1))
        mel2ph[t:t + n] = tok
        t, tok = t + n, tok + int(rng.integers(1, 3))
    if odd_tokens:
        pick = rng.random(T) < 0.05
        mel2ph[pick] = rng.choice(np.array([0, -1, -7, T_ph + 1, T_ph + 9, 1 << 40], np.int64), int(pick.sum()))
    m = np.rint(1600.0 * (note[np.clip(mel2ph, 1, T_ph) - 1].astype(np.float64) - 69)).astype(np.int64)
    q = m + np.cumsum(rng.integers(-40, 41, T)) % (2 * spread + 1) - spread + rng.integers(-200, 201, T)
    q = np.where(rng.random(T) < wild_p, q + rng.choice([-OCTAVE, OCTAVE, 7000, -9000], T), q)
    f0 = hz_of_units(q)
    f0[rng.random(T) < unvoiced_p] = 0.0
    return f0, mel2ph, note


def sung_score(rng, notes=8, frames=(20, 80), detune=40.0, vibrato=30.0, jitter=5.0):
    """(f0 [T], mel2ph [T], note_midi [notes], spans): a score of `notes` notes of 20 .. 79 frames, adjacent pitches distinct, sung with a detune of up to
    +-`detune` cents a note, a `vibrato`-cent 5.5 Hz vibrato and `jitter` cents (sigma) of jitter.  spans: (first frame, end) per note"""
    pitch = [int(rng.integers(55, 75))]
    while len(pitch) < notes:
        p = int(rng.integers(55, 75))
        if p != pitch[-1]:
            pitch.append(p)
    lens = rng.integers(frames[0], frames[1], notes)
    mel2ph = np.repeat(np.arange(1, notes + 1), lens)
    T = len(mel2ph)
    t = np.arange(T)
    cents = 100.0 * (np.repeat(pitch, lens) - 69) + np.repeat(rng.uniform(-detune, detune, notes), lens)
    cents = cents + vibrato * np.sin(2 * np.pi * 5.5 * t / FPS + rng.uniform(0, 2 * np.pi)) + rng.normal(0, jitter, T)
    ends = np.cumsum(lens)
    return (440.0 * 2.0 ** (cents / 1200.0)).astype(np.float32), mel2ph, np.array(pitch, np.float32), list(zip((ends - lens).tolist(), ends.tolist()))


@pytest.fixture(scope="module")
def singing():
    rng = np.random.default_rng(60)
    return [sung_score(rng) for _ in range(60)]


# ---- the restatement against the literal loop ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [0, 1, 5, 300])
def test_prefix_sums_equal_the_frame_loop(W):
    rng = np.random.default_rng(W)
    moved = 0
    for trial in range(24):
        T, T_ph = int(rng.integers(1, 201)), int(rng.integers(1, 30))
        f0, mel2ph, note = random_item(rng, T, T_ph, seg=(1, 25), odd_tokens=trial % 3 == 0)
        kw = dict(window=W, strength=float(rng.choice([0.0, 0.5, 1.0])), vibrato=float(rng.choice([0.0, 0.75, 1.0, 2.0])),
                  wild_cents=float(rng.choice([0.0, 150.0, 300.0, 16384.0])), octave_fold=bool(trial % 2))
        length = None if trial % 4 else int(rng.integers(0, T + 1))
        offset = float(rng.choice([0.0, 25.0, -1200.0]))
        k, out = correct_ref(f0, mel2ph, note, length, offset, **kw)
        k2, out2 = correct_loop(f0, mel2ph, note, length, offset, **kw)
        assert np.array_equal(k, k2), (trial, kw)
        assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))
        moved += int((k != 0).sum())
    assert moved > 50


def test_median_is_the_sorted_values_lower_middle():
    rng = np.random.default_rng(9)
    for trial in range(40):
        T, T_ph = int(rng.integers(1, 120)), int(rng.integers(1, 12))
        f0, mel2ph, note = random_item(rng, T, T_ph)
        med, n = deviation_ref(f0, mel2ph, note, wild_cents=300.0, octave_fold=bool(trial % 2))
        d, corr, _, _ = quantise(f0, mel2ph, note, wild=4800, octave_fold=bool(trial % 2))
        assert n == int(corr.sum())
        if n:
            assert med == np.sort(d[corr])[(n - 1) // 2] and (d[corr] <= med).sum() >= (n + 1) // 2 and (d[corr] < med).sum() <= (n - 1) // 2
        else:
            assert med == 0
    assert deviation_ref(np.zeros(5, np.float32), np.ones(5, np.int64), [60.0]) == (0, 0)
    assert deviation_ref(hz_of_units([-14400 + 7, -14400 - 30, -14400 + 2, -14400 + 90]), np.ones(4, np.int64), [60.0]) == (2, 4)      # the LOWER of 2 and 7


# ---- the rule on synthetic singing -----------------------------------------------------------------------------------------------------------

def note_means(f0, score_units, spans):
    dev = units_of_hz(f0) - score_units
    return np.array([dev[a:e].mean() for a, e in spans]), dev


def test_every_note_lands_on_the_score_and_keeps_its_vibrato(singing):
    worst_mean = worst_fast = 0.0
    for f0, mel2ph, note, spans in singing:
        score = 1600.0 * (note[mel2ph - 1].astype(np.float64) - 69)
        k, out = correct_ref(f0, mel2ph, note, window=1024, strength=1.0)
        assert (k != 0).mean() > 0.9
        before, dev_in = note_means(f0, score, spans)
        after, dev_out = note_means(out, score, spans)
        assert np.abs(before).max() > 100                                     # the detune was there: more than 6 cents on some note
        worst_mean = max(worst_mean, float(np.abs(after).max()))
        for (a, e), mi, mo in zip(spans, before, after):
            worst_fast = max(worst_fast, float(np.abs((dev_out[a:e] - mo) - (dev_in[a:e] - mi)).max()))
    print(f"note means within {worst_mean / 16:.4f} cents of the score, the fast part moved by {worst_fast / 16:.2e} cents at most")
    assert worst_mean <= 1.0 and worst_fast <= 1.0                            # units: 0.0625 cents


def test_vibrato_zero_flattens_and_strength_zero_is_the_identity(singing):
    for f0, mel2ph, note, spans in singing[:20]:
        score = 1600.0 * (note[mel2ph - 1].astype(np.float64) - 69)
        k, out = correct_ref(f0, mel2ph, note, window=1024, strength=1.0, vibrato=0.0)
        assert np.abs(units_of_hz(out) - score).max() <= 1.0
        k, out = correct_ref(f0, mel2ph, note, window=1024, strength=0.0, vibrato=1.0)
        assert not k.any() and np.array_equal(out.view(np.uint32), f0.view(np.uint32))
        k2, out2 = correct_ref(f0, mel2ph, note, window=1024, strength=1.0, vibrato=2.0)      # the fast part doubled, the mean still on the score
        k1, _ = correct_ref(f0, mel2ph, note, window=1024, strength=1.0, vibrato=1.0)
        d = quantise(f0, mel2ph, note)[0]
        assert np.array_equal((d - k2) - (d - k1), d - k1)


def test_a_short_window_follows_drift_inside_a_note():
    """one note of 400 frames that drifts from -30 to +30 cents: the whole-note mean leaves the drift in, a window of 12 frames takes it out"""
    T = 400
    f0 = hz_of_units(np.rint(np.linspace(-480, 480, T)) + 1600 * (64 - 69))
    mel2ph, note = np.ones(T, np.int64), np.array([64.0], np.float32)
    k_all, _ = correct_ref(f0, mel2ph, note, window=1024)
    k_12, out = correct_ref(f0, mel2ph, note, window=12)
    assert np.abs(k_all).max() <= 1
    d = quantise(f0, mel2ph, note)[0]
    assert np.abs((d - k_12)[12:-12]).max() <= 1 and np.abs(d - k_12).max() <= 16


# ---- further cases -------------------------------------------------------------------------------------------------------------------------

def test_an_octave_slip_is_wild_or_folded_and_never_disturbs_its_neighbours(singing):
    f0, mel2ph, note, spans = singing[0]
    t = (spans[2][0] + spans[2][1]) // 2
    slipped, gone = f0.copy(), f0.copy()
    slipped[t] = f0[t] * 2
    gone[t] = 0.0
    for W in (3, 1024):
        k_plain, out_plain = correct_ref(slipped, mel2ph, note, window=W)
        k_gone, _ = correct_ref(gone, mel2ph, note, window=W)
        assert k_plain[t] == 0 and out_plain[t].view(np.uint32) == slipped[t].view(np.uint32)      # wild: left alone
        assert np.array_equal(k_plain, k_gone)                                                     # ... and it counts for nobody
        k_fold, out_fold = correct_ref(slipped, mel2ph, note, window=W, octave_fold=True)
        k_clean, _ = correct_ref(f0, mel2ph, note, window=W, octave_fold=True)
        # folded: corrected an octave up, as if it had not slipped (to the unit that fp32 rounding of 19200 + x may move its q by)
        assert k_fold[t] != 0 and np.abs(k_fold - k_clean).max() <= 1
        assert abs(units_of_hz(out_fold[t]) - OCTAVE - 1600.0 * (note[mel2ph[t] - 1] - 69)) < 16 * 60.0


def test_a_transposed_guide_is_measured_and_corrected_in_its_own_key(singing):
    for f0, mel2ph, note, spans in singing[:20]:
        low = (f0.astype(np.float64) * 2.0 ** (-200.0 / 1200.0)).astype(np.float32)
        med, n = deviation_ref(low, mel2ph, note)
        assert n == len(f0) and abs(med + 3200) <= 16 * 40                    # within the detunes' spread of -200 cents
        auto = np.float32(med) / np.float32(16)                               # what correct_guide(offset_cents="auto") feeds the correction
        k, out = correct_ref(low, mel2ph, note, offset_cents=auto, window=1024)
        score = 1600.0 * (note[mel2ph - 1].astype(np.float64) - 69) + med
        assert np.abs(note_means(out, score, spans)[0]).max() <= 1.0
        k0, _ = correct_ref(low, mel2ph, note, window=1024)                   # without the offset it is pulled up into the score's key
        assert abs(float(np.mean(k0 - k)) - med) <= 1


def test_check_args():
    from visinger_amd import guide_correct
    assert guide_correct.check_args() == (1024, 256, 256, 4800, 0, 0)
    assert guide_correct.check_args(window=0, strength=0.5, vibrato=2.0, wild_cents=16384.0, octave_fold=True) == (0, 128, 512, 1 << 18, 1, 0)
    assert guide_correct.check_args(strength=0, vibrato=0, wild_cents=0) == (1024, 0, 0, 0, 0, 0)
    for kw in (dict(window=-1), dict(window=1025), dict(window=3.0), dict(window=True), dict(strength=-0.1), dict(strength=1.01), dict(strength="1"),
               dict(strength=float("nan")), dict(vibrato=-1), dict(vibrato=2.5), dict(wild_cents=-1), dict(wild_cents=16385), dict(wild_cents=float("inf")),
               dict(octave_fold=2), dict(octave_fold="yes")):
        with pytest.raises(ValueError):
            guide_correct.check_args(**kw)
    header = open(os.path.join(ROOT, "include", "visinger_hip.h")).read()
    assert int(re.search(r"#define VS_GUIDE_CORRECT_TILE (\d+)", header).group(1)) == guide_correct.TILE
    assert "int vs_guide_correct(" in header and "int vs_guide_deviation(" in header
    from visinger_amd import _lib
    assert _lib.EXPECTED_ABI == 7                                             # two exports more, the ABI as it was


def test_the_driver_refuses_bad_input_before_any_launch():
    from visinger_amd import synth
    item = dict(text_tokens=np.arange(1, 4), pitch_tokens=np.array([3, 4, 5]), dur_tokens=np.array([2, 2, 1]), mel2ph=np.array([1, 1, 2, 2, 3]),
                note_midi=np.array([60.0, 62.0, 0.0], np.float32), f0=np.full(5, 260.0, np.float32))
    plain = {k: v for k, v in item.items() if k not in ("f0", "note_midi")}
    with pytest.raises(ValueError, match="dict"):
        synth.synthesize(None, [item], 8, guide_correct=3)
    for bad, kw in ((dict(item, f0=item["f0"][:4]), {}), (dict(item, f0=item["f0"][None]), {}), (dict(item, note_midi=item["note_midi"][:2]), {}),
                    (dict(item, guide_offset_cents=float("nan")), {}), (dict(plain, f0=item["f0"]), dict(midi_of_token=[0.0, 1.0]))):
        with pytest.raises(ValueError, match="item 1"):
            synth.correct_items([plain, bad], "cpu", **kw)
    for kw in (dict(bogus=1), dict(window=2000), dict(strength=2), dict(offset_cents="a"), dict(offset_cents=float("inf")), dict(midi_of_token=[[1.0]])):
        with pytest.raises(ValueError):
            synth.correct_items([item], "cpu", **kw)
    same = synth.correct_items([plain, dict(plain, f0=item["f0"])], "cpu")    # no curve, or no token pitches: passed on, as copies
    assert same[0] is not plain and same[0].keys() == plain.keys() and np.array_equal(same[1]["f0"], item["f0"])
