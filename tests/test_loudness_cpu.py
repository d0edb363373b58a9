"""Loudness normalisation (rule "f14", visinger_amd/loudness.py) without a GPU: the K-weighting coefficients against the standard's table, the numpy
restatement against scipy's filter, the standard's calibration tone, both gates on a fixture, the host-side argument checks, the driver's refusals and the three
entries' refusals."""
import ctypes

import numpy as np
import pytest
import torch

from loudness_cases import gate_margin, gating_fixture

ITEM = dict(text_tokens=np.arange(1, 4), pitch_tokens=np.array([3, 4, 5]), dur_tokens=np.array([2, 2, 1]), mel2ph=np.array([1, 1, 2, 2, 3]))

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
SHELF_48K = ([1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -1.69065929318241, 0.73248077421585])
HIGHPASS_48K = ([1.0, -2.0, 1.0], [1.0, -1.99004745483398, 0.99007225036621])


def test_k_weighting_gives_the_standards_table_at_48_khz():
    from visinger_amd import loudness as lo
    (b1, a1), (b2, a2) = lo.k_weighting(48000)
    for got, want in zip((b1, a1, b2, a2), SHELF_48K + HIGHPASS_48K):
        assert got.dtype == np.float64 and got.shape == (3,) and np.abs(got - np.asarray(want)).max() <= 1e-12
    assert np.array_equal(lo.coef_array(48000), np.array([*b1, a1[1], a1[2], *b2, a2[1], a2[2]]))
    # the state matrix is one sample of the cascade under a zero input, the carry table its powers: M = A^c and squares of it, as value + remainder
    A, c, tab = lo.state_matrix(48000), lo.lane_samples(4800), lo.carry_table(48000)
    assert c == 19 and lo.lane_samples(800) == 4 and lo.lane_samples(801) == 4 and tab.shape == (8, 2, 4, 4) and not tab.flags.writeable
    P = np.linalg.matrix_power(A, c)
    for k in range(8):                                                           # (fp64 squaring is what the table is NOT made by: it is good to 1e-6 here)
        assert np.abs(tab[k, 0] - P).max() <= 1e-6 * np.abs(P).max() and np.abs(tab[k, 1]).max() <= 2.0 ** -53 * np.abs(tab[k, 0]).max()
        P = P @ P
    # exactly, in rationals, at 8 kHz: the value is the power rounded once, the remainder what is left rounded once
    from fractions import Fraction
    A8, tab8 = [[Fraction(float(v)) for v in row] for row in lo.state_matrix(8000)], lo.carry_table(8000)
    mul = lambda X, Y: [[sum(X[i][k] * Y[k][j] for k in range(4)) for j in range(4)] for i in range(4)]
    P = mul(mul(A8, A8), mul(A8, A8))
    for k in range(8):
        for i in range(4):
            for j in range(4):
                assert tab8[k, 0, i, j] == float(P[i][j]) and tab8[k, 1, i, j] == float(P[i][j] - Fraction(float(P[i][j]))), (k, i, j)
        P = mul(P, P)


@pytest.mark.parametrize("sr", [8000, 8010, 44100, 48000])
def test_restatement_equals_scipys_filter(sr):
    signal = pytest.importorskip("scipy.signal")
    from visinger_amd import loudness as lo
    s = sr // 10
    x = np.random.default_rng(sr).uniform(-1.0, 1.0, (2, 5 * s + 7)).astype(np.float32)
    lens = [5 * s + 7, 3 * s - 1]
    S, loud, stats, gain = lo.loudness_ref(x, lens, sr)
    (b1, a1), (b2, a2) = lo.k_weighting(sr)
    assert S.shape == (2, 5) and not S[1, 2:].any()
    for b, n in enumerate(lens):
        y = signal.lfilter(b2, a2, signal.lfilter(b1, a1, x[b, :n].astype(np.float64)))
        want = (y[:n // s * s] ** 2).reshape(-1, s).sum(axis=1)
        assert np.abs(S[b, :n // s] - want).max() <= 1e-12 * want.max()
    assert stats.tolist() == [[2, 2, 2], [0, 0, 0]] and loud[1] == -np.inf and gain[1] == 1.0 and np.isfinite(loud[0])


@pytest.mark.parametrize("amplitude", [1.0, 0.1])
def test_the_calibration_tone_measures_what_the_standard_says(amplitude):
    """a 997 Hz sine of amplitude A reads 20 log10 A - 3.01 LKFS (BS.1770-4, annex 1: a full-scale tone reads -3.01)"""
    from visinger_amd import loudness as lo
    sr = 48000
    x = (amplitude * np.sin(2.0 * np.pi * 997.0 * np.arange(5 * sr) / sr)).astype(np.float32)
    S, loud, stats, gain = lo.loudness_ref(x[None], None, sr, target=-23.0, max_gain_db=20.0)
    print(f"997 Hz, amplitude {amplitude}: {loud[0]:.5f} LUFS, off by {loud[0] - (20.0 * np.log10(amplitude) - 3.01):+.2e}")
    assert abs(loud[0] - (20.0 * np.log10(amplitude) - 3.01)) <= 0.01
    assert stats[0].tolist() == [47, 47, 47]
    assert gain[0] == np.float32(10.0 ** (min(-23.0 - loud[0], 20.0) / 20.0))


def test_both_gates_work_on_the_fixture():
    from visinger_amd import loudness as lo
    x, sr = gating_fixture()
    S, loud, stats, gain = lo.loudness_ref(x[None], None, sr)
    print(f"gating fixture: stats {stats[0].tolist()}, {loud[0]:.4f} LUFS, margin {gate_margin(S[0], 80, 800):.3e}")
    assert stats[0].tolist() == [77, 60, 30] and len(set(stats[0].tolist())) == 3
    assert abs(loud[0] - (-9.73)) <= 0.005
    assert gate_margin(S[0], 80, 800) > 1e-6
    # without the relative gate the quiet half would pull the reading down by nearly 3 dB; with it the fixture reads as the loud tone alone does, less what
    # the three blocks that straddle the drop take
    alone = lo.loudness_ref(x[None, :3 * sr], None, sr)[1][0]
    assert alone - 0.3 < loud[0] < alone
    # a row cut inside its fourth step has no block; a NaN makes the loudness a NaN and the gain 1
    assert lo.loudness_ref(x[None], [3199], sr)[2][0].tolist() == [0, 0, 0]
    bad = x.copy()
    bad[40000] = np.nan
    S, loud, stats, gain = lo.loudness_ref(bad[None], None, sr)
    assert np.isnan(loud[0]) and gain[0] == 1.0 and stats[0, 0] == 77 and 0 < stats[0, 1] < 60
    # max_gain_db clamps the boost of a quiet row; attenuation is not limited
    quiet = (x[:3 * sr] * 1e-3)[None]
    assert lo.loudness_ref(quiet, None, sr, -23.0, 20.0)[3][0] == np.float32(10.0)
    assert lo.loudness_ref(x[None], None, sr, -60.0, 20.0)[3][0] == np.float32(10.0 ** ((-60.0 - loud_of(x, sr)) / 20.0))


def loud_of(x, sr):
    from visinger_amd import loudness as lo
    return lo.loudness_ref(x[None], None, sr)[1][0]


def test_the_derived_bound_is_small_and_grows_with_the_rate():
    from visinger_amd import loudness as lo
    bounds = [lo.steps_bound(sr, 3.0) for sr in (8000, 8010, 44100, 48000)]
    print("steps_bound at rho = 3:", ["%.3e" % b for b in bounds])
    assert bounds == sorted(bounds) and bounds[0] > 20 * 2.0 ** -53 and bounds[-1] < 2.0 ** -28
    kappa, scan = lo.error_constants(48000)
    assert scan < kappa                                                           # the lane scan costs less than the serial filter's own rounding


def test_check_args_refuses_what_the_entries_cannot_take():
    from visinger_amd import loudness as lo
    assert lo.DEFAULTS == dict(target_lufs=-23.0, max_gain_db=20.0)
    assert lo.check_args() == (-23.0, 20.0) and lo.check_args(target_lufs=-70, max_gain_db=60, sample_rate=8000) == (-70.0, 60.0)
    assert lo.check_args(0, 0, 48000) == (0.0, 0.0) and lo.check_rate(44100) == 4410
    for bad in (dict(target_lufs=1.0), dict(target_lufs=-70.5), dict(target_lufs=float("nan")), dict(target_lufs="-23"), dict(target_lufs=True),
                dict(max_gain_db=-0.1), dict(max_gain_db=60.5), dict(max_gain_db=float("inf")), dict(max_gain_db=None),
                dict(sample_rate=44101), dict(sample_rate=7990), dict(sample_rate=48010), dict(sample_rate=44100.0), dict(sample_rate=True), dict(sample_rate="48000")):
        with pytest.raises(ValueError):
            lo.check_args(**bad)
    for bad in (44101, 96000, 0, None):
        with pytest.raises(ValueError):
            lo.k_weighting(bad)
    with pytest.raises(ValueError):
        lo.loudness_ref(np.zeros((1, 10), np.float32), None, 44101)


def test_python_layer_refuses_cpu_tensors_and_bad_keys_before_any_launch():
    from visinger_amd import _lib, loudness as lo
    x = torch.zeros(1, 8000)
    with pytest.raises(ValueError, match="normalize takes"):
        lo.normalize(x, 8000, target=-20.0)
    with pytest.raises(ValueError, match="sample_rate"):
        lo.normalize(x, 44101)
    with pytest.raises(ValueError, match="sample_rate"):
        lo.measure(x, 44101)
    with pytest.raises(_lib.VisingerHipError):
        lo.normalize(x, 8000)
    with pytest.raises(_lib.VisingerHipError):
        lo.measure(x, 8000)


def test_driver_refusals_come_before_the_model_is_looked_at():
    from visinger_amd import synth
    for bad, match in ((3, "loudness must be a dict"), ("on", "loudness must be a dict"), (dict(sample_rate=24000, target=-20.0), "loudness takes"),
                       (dict(target_lufs=-20.0), "sample_rate"), (dict(sample_rate=44101), "sample_rate"), (dict(sample_rate=24000, target_lufs=1.0), "target_lufs"),
                       (dict(sample_rate=24000, max_gain_db=61), "max_gain_db")):
        with pytest.raises(ValueError, match=match):
            synth.synthesize(None, [ITEM], 8, loudness=bad)
    # the stage measures at the rate the waveforms leave at: resample_to's output_rate has to be one it takes, and both dicts name the model's rate
    with pytest.raises(ValueError, match="output_rate"):
        synth.synthesize(None, [ITEM], 8, loudness=dict(sample_rate=24000), resample_to=dict(sample_rate=24000, output_rate=96000))
    with pytest.raises(ValueError, match="the model's"):
        synth.synthesize(None, [ITEM], 8, loudness=dict(sample_rate=24000), resample_to=dict(sample_rate=22050, output_rate=44100))
    # OPTIONS and the order of its refusals are as they were: a bad limit is still reported first
    assert list(synth.OPTIONS) == ["resample_to", "guide_dynamics", "limit", "guide_correct", "guide_align", "guide_track"]
    with pytest.raises(ValueError, match="window must be an integer"):
        synth.synthesize(None, [ITEM], 8, limit=dict(window=-1), loudness=dict(sample_rate=44101))
    with pytest.raises(ValueError, match="guide_align must be a dict"):
        synth.synthesize(None, [ITEM], 8, guide_align=3, loudness=3)
    # a good one gets as far as the model
    with pytest.raises(AttributeError):
        synth.synthesize(None, [ITEM], 8, loudness=dict(sample_rate=24000, target_lufs=-16.0, max_gain_db=6.0))


def test_entry_points_validate_their_arguments_before_anything_is_launched():
    from visinger_amd import _lib, loudness as lo
    L = _lib.lib()
    assert _lib.EXPECTED_ABI == 7 == L.vs_abi_version()                             # the new entries join ABI 7
    p, q, r, t = (ctypes.c_void_p(4096 * k) for k in (1, 16, 32, 48))               # never dereferenced: every call below is refused on the host
    coef = (ctypes.c_double * 10)(*lo.coef_array(8000))
    nan_coef = (ctypes.c_double * 10)(*([1.0] * 9 + [float("nan")]))

    def refused(entry, names, ok, bads):
        for bad in bads:
            a = list(ok)
            for k, v in bad.items():
                a[names.index(k)] = v
            assert getattr(L, entry)(*a) != _lib.VS_OK, (entry, bad)
            assert entry.encode() in L.vs_last_error(), (entry, bad, L.vs_last_error())

    refused("vs_loud_steps", ["wav", "lengths", "B", "L", "coef", "carry", "s", "S", "NS", "stream"], [p, None, 2, 8000, coef, q, 800, r, 10, None],
            (dict(wav=None), dict(coef=None), dict(carry=None), dict(S=None), dict(B=0), dict(L=0), dict(NS=0), dict(L=1 << 31), dict(NS=1 << 31), dict(B=1 << 62),
             dict(s=799), dict(s=4801), dict(s=0), dict(coef=nan_coef), dict(S=p), dict(S=q), dict(S=ctypes.c_void_p(4096 + 64000 - 8))))
    refused("vs_loud_gate", ["S", "lengths", "B", "NS", "s", "target", "max_gain_db", "loud", "gain", "stats", "stream"], [p, None, 2, 10, 800, -23.0, 20.0, q, r, t, None],
            (dict(S=None), dict(loud=None), dict(gain=None), dict(stats=None), dict(B=0), dict(NS=0), dict(NS=1 << 31), dict(B=1 << 62), dict(s=799), dict(s=4801),
             dict(target=0.5), dict(target=-71.0), dict(target=float("nan")), dict(max_gain_db=-1.0), dict(max_gain_db=61.0), dict(max_gain_db=float("nan")),
             dict(loud=p), dict(gain=p), dict(stats=ctypes.c_void_p(4096 + 8)), dict(gain=q), dict(stats=q), dict(stats=r)))
    refused("vs_gain_apply", ["x", "gain", "lengths", "y", "B", "L", "stream"], [p, q, None, r, 2, 4000, None],
            (dict(x=None), dict(gain=None), dict(y=None), dict(B=0), dict(L=0), dict(L=1 << 31), dict(B=1 << 62), dict(y=ctypes.c_void_p(4096 + 4)), dict(gain=r),
             dict(y=q), dict(lengths=r)))
