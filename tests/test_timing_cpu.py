"""Tempo and duration control, the part that needs no GPU: the retiming rule of csrc/timing_ops.hip restated FROM ITS DEFINITION
(include/visinger_hip.h "f5") as plain sequential Python -- one token after the other, one frame after the other -- with the pinned
examples of the rule, its closed form against the recurrence, and its invariants; the two exports exist and validate their arguments before anything
is launched; the host-side ValueErrors.  tests/test_timing_gpu.py compares the kernels with `retime_ref` and `warp_ref` below."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

D_ITEM0 = [3, 4, 2, 5, 3, 6]           # item 0 of tests/golden/visinger_tiny_pitch.npz


def durations(mel2ph, T_ph):
    """d_i = frames equal to i, i = 1 .. T_ph (0 and larger indices are ignored)"""
    d = [0] * T_ph
    for i in mel2ph:
        if 1 <= int(i) <= T_ph:
            d[int(i) - 1] += 1
    return d


def fixed_point(stretch, tempo):
    """s = (int) rint(clamp(stretch / tempo, 2^-6, 2^6) * 65536): ONE fp32 division, a non-finite quotient counts as 1"""
    with np.errstate(all="ignore"):
        f = np.float32(stretch) / np.float32(tempo)
    if not np.isfinite(f):
        f = np.float32(1.0)
    f = min(max(f, np.float32(2.0 ** -6)), np.float32(2.0 ** 6))
    return int(np.rint(np.float32(f) * np.float32(65536.0)))


def retime_ref(d, stretch=None, tempo=None, min_frames=1, max_frames=None):
    """(old ends c, new ends e, new length) of one item by the recurrence e_i = max(e_{i-1} + m_i, R_i), in Python integers"""
    c, e, P, c_prev, e_prev = [], [], 0, 0, 0
    for i, di in enumerate(d):
        di = int(di)
        s = fixed_point(1.0 if stretch is None else stretch[i], 1.0 if tempo is None else tempo)
        P += di * s
        R = (P + 32768) >> 16
        m = min_frames if di > 0 else 0
        e_prev = max(e_prev + m, R)
        c_prev += di
        c.append(c_prev)
        e.append(e_prev)
    n = e[-1] if e else 0
    return c, e, (n if max_frames is None else min(n, max_frames))


def closed_form(d, stretch=None, tempo=None, min_frames=1):
    """e_i = M_i + max(0, max_{j<=i}(R_j - M_j)): a prefix sum plus a prefix max (what a parallel scan computes)"""
    s = [fixed_point(1.0 if stretch is None else stretch[i], 1.0 if tempo is None else tempo) for i in range(len(d))]
    P = np.cumsum([int(di) * si for di, si in zip(d, s)], dtype=np.int64)
    M = np.cumsum([min_frames if di > 0 else 0 for di in d], dtype=np.int64)
    R = (P + 32768) >> 16
    return list(map(int, M + np.maximum(0, np.maximum.accumulate(R - M))))


def align_ref(e, n, T_out):
    """mel2ph' [T_out]: the smallest i (1-based) with e_i > t for t < n, 0 elsewhere"""
    out, i = [0] * T_out, 0
    for t in range(min(n, T_out)):
        while e[i] <= t:             # (e is non-decreasing: the search goes on from the previous frame's token)
            i += 1
        out[t] = i + 1
    return out


def warp_ref(curve, c, e, n, T_out):
    """(curve' [T_out] fp32, blended [T_out] bool): the curve resampled inside each token, frame after frame"""
    curve = np.asarray(curve, dtype=np.float32)
    out, blended, i = np.zeros(T_out, np.float32), np.zeros(T_out, bool), 0
    for t in range(min(n, T_out)):
        while e[i] <= t:
            i += 1
        e0, c0 = (e[i - 1], c[i - 1]) if i else (0, 0)
        u, nn, n2 = t - e0, c[i] - c0, e[i] - e0
        num, den = (2 * u + 1) * nn - n2, 2 * n2
        if num < 0:
            k, w = 0, np.float32(0)
        else:
            k = num // den
            w = np.float32(num - k * den) / np.float32(den)
        if k >= nn - 1:
            k, w = nn - 1, np.float32(0)
        a, b = curve[c0 + k], curve[c0 + min(k + 1, nn - 1)]
        if a > 0 and b > 0:
            out[t] = np.float32(a + w * np.float32(b - a))
            blended[t] = w != 0
        else:
            out[t] = a if w < 0.5 else b
    return out, blended


def random_row(r, T_ph, empty=0.2, lo=0.1, hi=4.0):
    d = r.integers(1, 13, T_ph)
    d[r.uniform(size=T_ph) < empty] = 0
    return [int(x) for x in d], r.uniform(lo, hi, T_ph).astype(np.float32)


def test_item0_of_the_fixture_has_the_pinned_durations():
    _, a = load_golden("visinger_tiny_pitch")
    assert durations(a["mel2ph"][0], 6) == D_ITEM0


def test_pinned_examples_of_the_rule():
    d = D_ITEM0
    assert retime_ref(d, tempo=2.0)[1] == [2, 4, 5, 7, 9, 12]
    assert retime_ref(d, tempo=0.8)[1] == [4, 9, 11, 18, 21, 29]
    assert retime_ref(d, tempo=4.0, min_frames=1)[1] == [1, 2, 3, 4, 5, 6]
    assert retime_ref(d, tempo=4.0, min_frames=0)[1] == [1, 2, 2, 4, 4, 6]
    assert retime_ref(d, stretch=[1, 1, 1, 2.5, 1, 0.5])[1] == [3, 7, 9, 22, 25, 28]
    _, e, n = retime_ref([10] + [1] * 600, stretch=[4] + [1 / 64] * 600)
    assert (e[0], e[1], e[299], e[600], n) == (40, 41, 339, 640, 640)      # the floor region: the prefix max is carried across every scan chunk
    assert retime_ref(d, tempo=0.8, max_frames=20)[2] == 20 and retime_ref(d, tempo=0.8, max_frames=40)[2] == 29


def test_pinned_curve_example():
    curve = [0, 100, 110, 120, 130, 140, 150, 0, 0, 200, 210, 220, 230, 240, 250, 260, 270, 300, 310, 320, 330, 340, 350]
    c, e, n = retime_ref(D_ITEM0, tempo=2.0)
    got, _ = warp_ref(curve, c, e, n, n)
    assert got.tolist() == [0, 107.5, 125, 145, 0, 207.5, 232.5, 252.5, 267.5, 305, 325, 345]
    assert align_ref(e, n, n + 2) == [1, 1, 2, 2, 3, 4, 4, 5, 5, 6, 6, 6, 0, 0]


def test_fixed_point_clamp_rule():
    assert fixed_point(1.0, 1.0) == 65536 and fixed_point(1.0, 2.0) == 32768
    assert fixed_point(float("nan"), 1.0) == 65536 and fixed_point(float("inf"), 1.0) == 65536 and fixed_point(1.0, 0.0) == 65536
    assert fixed_point(0.0, 0.0) == 65536                                   # 0 / 0 = NaN -> 1
    assert fixed_point(0.0, 1.0) == 1024 and fixed_point(-3.0, 1.0) == 1024 and fixed_point(1e-9, 1.0) == 1024      # clamped to 2^-6
    assert fixed_point(1000.0, 1.0) == 64 * 65536
    assert fixed_point(np.float32(1 + 2.0 ** -17), 1.0) == 65536 and fixed_point(np.float32(1 + 3 * 2.0 ** -17), 1.0) == 65538      # ties to even


def test_closed_form_equals_the_recurrence_on_random_rows():
    r = np.random.default_rng(7)
    for n in range(600):
        T_ph = int(r.integers(1, 80))
        d, st = random_row(r, T_ph, lo=1 / 64 if n % 3 == 0 else 0.1)
        tempo, mf = float(r.choice([0.5, 1.0, 3.0, 7.5])), int(r.integers(0, 3))
        assert closed_form(d, st, tempo, mf) == retime_ref(d, st, tempo, mf)[1], (n, d)


def test_identity_at_factor_one_and_the_invariants():
    r = np.random.default_rng(8)
    for n in range(200):
        T_ph = int(r.integers(1, 60))
        d, st = random_row(r, T_ph)
        c, e, total = retime_ref(d)
        assert e == c == list(np.cumsum(d)) and total == sum(d)
        m2p = np.repeat(np.arange(1, T_ph + 1), d)
        assert align_ref(e, total, total + 3) == list(m2p) + [0] * 3 and durations(m2p, T_ph) == d
        curve = r.uniform(80, 900, max(total, 1)).astype(np.float32)
        curve[r.uniform(size=len(curve)) < 0.3] = 0
        got, blended = warp_ref(curve, c, e, total, total)
        assert np.array_equal(got, curve[:total]) and not blended.any()
        for mf in (0, 1, 2):
            _, e, _ = retime_ref(d, st, float(r.choice([0.5, 1.0, 3.0])), mf)
            steps = np.diff([0] + e)
            assert (steps >= 0).all() and all(s >= (mf if di > 0 else 0) for s, di in zip(steps, d))
            assert all(s == 0 for s, di in zip(steps, d) if di == 0)                                   # an empty token stays empty


def test_warp_never_blends_an_unvoiced_frame_nor_reads_across_a_token():
    d = [4, 3]
    curve = np.array([100, 0, 120, 130, 999, 999, 999], np.float32)
    c, e, n = retime_ref(d, stretch=[3.0, 1.0])
    got, blended = warp_ref(curve, c, e, n, n)
    assert e == [12, 15] and blended[:12].any() and not blended[12:].any()
    for v, mixed in zip(got[:12], blended[:12]):                      # token 1: its own values, or between 120 and 130 (its only voiced pair)
        assert (120 < v < 130) if mixed else v in (100.0, 0.0, 120.0, 130.0)
    assert (got[12:] == 999).all()                                    # token 2 at factor 1: a copy; nothing of it leaked into token 1


def test_library_exports_the_timing_entry_points():
    from visinger_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "vs_retime_tokens") and hasattr(lib, "vs_retime_frames")
    assert _lib.lib().vs_abi_version() == _lib.EXPECTED_ABI == 7


def test_timing_arguments_are_validated_before_anything_is_launched():
    """every VS_EINVAL case returns non-zero with the function's name in the message.  The pointers are HOST memory and no call here is valid,
    so nothing may reach the device."""
    from visinger_amd import _lib
    L = _lib.lib()
    bufs = [(ctypes.c_int64 * 64)() for _ in range(5)]
    p, q, r, s, u = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)

    def tokens(mel2ph=p, dur=None, stretch=None, tempo=None, min_frames=1, max_frames=0, cum_old=q, cum_new=r, lengths=s, B=2, T_frames=5, T_tokens=3):
        return L.vs_retime_tokens(mel2ph, dur, stretch, tempo, min_frames, max_frames, cum_old, cum_new, lengths, B, T_frames, T_tokens, None)

    def frames(cum_old=q, cum_new=r, lengths=s, curve=None, curve_T=0, out=p, curve_out=None, B=2, T_tokens=3, T_out=5):
        return L.vs_retime_frames(cum_old, cum_new, lengths, curve, curve_T, out, curve_out, B, T_tokens, T_out, None)

    for kw in [dict(mel2ph=None), dict(dur=u), dict(cum_old=None), dict(cum_new=None), dict(lengths=None), dict(cum_new=q), dict(mel2ph=None, dur=q),
               dict(mel2ph=None, dur=r), dict(B=0), dict(B=-1), dict(T_tokens=0), dict(T_tokens=8193), dict(T_frames=0), dict(T_frames=1 << 24),
               dict(min_frames=-1), dict(min_frames=65537), dict(max_frames=-1)]:
        assert tokens(**kw) != 0, kw
        assert b"vs_retime_tokens" in L.vs_last_error(), kw
    for kw in [dict(cum_old=None), dict(cum_new=None), dict(lengths=None), dict(out=None), dict(curve=u), dict(curve_out=u), dict(curve=u, curve_out=u, curve_T=5),
               dict(curve=u, curve_out=p, curve_T=0), dict(B=0), dict(T_tokens=0), dict(T_tokens=8193), dict(T_out=0), dict(T_out=-4), dict(T_out=1 << 31)]:
        assert frames(**kw) != 0, kw
        assert b"vs_retime_frames" in L.vs_last_error(), kw


def test_python_layer_refuses_cpu_tensors_and_bad_factors():
    from visinger_amd import _lib, timing
    with pytest.raises(_lib.VisingerHipError):
        timing.retime(mel2ph=torch.ones(2, 5, dtype=torch.int64), T_ph=3)
    with pytest.raises(_lib.VisingerHipError):
        timing.retime()
    with pytest.raises(_lib.VisingerHipError):
        timing.retime(mel2ph=torch.ones(2, 5, dtype=torch.int64), dur=torch.ones(2, 3, dtype=torch.int64))
    assert timing.factor_tensor(2, 3, "cpu").tolist() == [2.0] * 3 and timing.factor_tensor([1, 0.5], 2, "cpu").tolist() == [1.0, 0.5]
    assert timing.factor_tensor(np.float32(0.8), 2, "cpu").dtype == torch.float32
    for bad in ([1, 2, 3], 0.0, -1.0, float("nan"), float("inf"), [1.0, 0.0]):
        with pytest.raises(ValueError):
            timing.factor_tensor(bad, 2, "cpu")
    assert timing.stretch_tensor([[1, 2, 3], [1, 1, 0.5]], 2, 3, "cpu").shape == (2, 3)
    for bad in ([[1, 2, 3]], [[1, 2], [1, 2]], [[1, 2, 0], [1, 1, 1]], [[1, 2, float("nan")], [1, 1, 1]]):
        with pytest.raises(ValueError):
            timing.stretch_tensor(bad, 2, 3, "cpu")


def item(n_frames, n_tokens=2, **extra):
    return dict(text_tokens=np.arange(1, n_tokens + 1), pitch_tokens=np.arange(1, n_tokens + 1), dur_tokens=np.arange(1, n_tokens + 1),
                mel2ph=np.repeat(np.arange(1, n_tokens + 1), n_frames // n_tokens + 1)[:n_frames], **extra)


def test_driver_checks_tempos_and_stretches_before_anything_runs():
    from visinger_amd import synth
    model = torch.nn.Linear(2, 2)               # never reached: the arguments are checked first
    a, b = item(6), item(4)
    for bad in (0.0, -2.0, float("nan"), [1.0], [1.0, 0.0]):
        with pytest.raises(ValueError, match="tempo"):
            synth.synthesize(model, [a, b], 8, tempo=bad)
    with pytest.raises(ValueError, match="ph_stretch"):
        synth.synthesize(model, [item(6, ph_stretch=[1.0, 2.0, 3.0])], 8)
    with pytest.raises(ValueError, match="stretch"):
        synth.synthesize(model, [item(6, ph_stretch=[1.0, -2.0])], 8, tempo=1.5)
    with pytest.raises(ValueError, match="frames"):
        synth.synthesize(model, [item(6, f0=np.ones(5))], 8, tempo=2.0)


def test_model_and_graph_refuse_contradicting_tempo_arguments():
    from visinger_amd import synth
    from visinger_amd.models.visinger import VISinger
    fwd = VISinger.forward

    class Stub:
        hparams = {"use_pitch_embed": True}
    x = torch.zeros(1, 3)
    with pytest.raises(ValueError, match="infer"):
        fwd(Stub(), x, x, x, x, tempo=2.0)
    with pytest.raises(ValueError, match="infer"):
        fwd(Stub(), x, x, x, x, ph_stretch=x)
    with pytest.raises(ValueError, match="f0_hz"):
        fwd(Stub(), x, x, x, x, infer=True, tempo=2.0, f0=x, uv=x)
    with pytest.raises(ValueError, match="f0_hz"):
        fwd(Stub(), x, x, x, x, infer=True, ph_stretch=x, uv=x)
    with pytest.raises(ValueError, match="max_frames"):
        fwd(Stub(), x, x, x, x, infer=True, max_frames=40)
    batch = dict(mel2ph=torch.zeros(1, 3, dtype=torch.long), text_tokens=torch.zeros(1, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="max_frames"):
        synth.GraphedStep(None, batch, x, False, tempo=2.0)
    with pytest.raises(ValueError, match="max_frames"):
        synth.GraphedStep(None, batch, x, False, max_frames=40)
