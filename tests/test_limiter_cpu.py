"""The peak-limiter rule (include/visinger_hip.h "f11") without a GPU: the numpy restatement ``limiter.limit_ref`` -- written from the rule, not
from the kernel -- against a brute-force double loop, the reduction table, the properties the construction promises (g >= u, the ceiling, the triangle, the
plateau), the edge values, every host-side refusal of visinger_amd/limiter.py and of the driver's new key, and every VS_EINVAL of the entry with its string
(the library loads without a GPU).  tests/test_limiter_gpu.py holds the kernel to the restatement."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_1DB = np.float32(10.0 ** (-1.0 / 20.0))


def brute(x, n, c, W):
    """(u, M, g) of one row by the rule's own words: a double loop, no prefix sums, no running maxima"""
    from visinger_amd import limiter as lm
    tab = lm.reduction_table()
    x = np.asarray(x, dtype=np.float32)
    u = np.zeros(len(x), np.int64)
    for i in range(n):
        a = np.abs(x[i])
        if a > c:
            with np.errstate(over="ignore"):
                rho = np.float32(a) / np.float32(c)
            bits = int(np.float32(rho).view(np.uint32))
            u[i] = min(512 * ((bits >> 23) - 127) + int(tab[(bits & 0x7FFFFF) >> 14]), lm.U_MAX)
    M, g = np.zeros(len(x), np.int64), np.zeros(len(x), np.int64)
    for j in range(n):
        M[j] = max(u[i] for i in range(max(0, j - W), min(n - 1, j + W) + 1))
    for i in range(n):
        terms = [M[j] for j in range(max(0, i - W), min(n - 1, i + W) + 1)]
        g[i] = -(-sum(terms) // len(terms))
    return u, M, g


def noise(rng, B, n, scale=0.5):
    """lognormal-scaled noise: most samples under -1 dBFS, bursts well over it"""
    return (rng.standard_normal((B, n)) * np.exp(rng.standard_normal((B, n)) * 0.8) * scale).astype(np.float32)


def test_limit_ref_equals_the_brute_force_double_loop():
    from visinger_amd import limiter as lm
    rng = np.random.default_rng(1)
    x = noise(rng, 4, 150)
    lens = [150, 97, 1, 0]
    for W in (0, 1, 7, 64, 200):
        u, M, g, y = lm.limit_ref(x, lens, C_1DB, W)
        for b, n in enumerate(lens):
            bu, bM, bg = brute(x[b], n, C_1DB, W)
            assert np.array_equal(u[b], bu) and np.array_equal(M[b], bM) and np.array_equal(g[b], bg), (W, b)
            assert not g[b, n:].any() and np.array_equal(y[b, n:], x[b, n:].astype(np.float64))
        assert (u > 0).any()
    assert np.array_equal(lm.limit_ref(x, None, C_1DB, 7)[2][1], brute(x[1], 150, C_1DB, 7)[2])      # lengths = None: every row is L long


def test_the_table_is_an_upper_bound_and_a_tight_one():
    from visinger_amd import limiter as lm
    tab = lm.reduction_table()
    assert tab.dtype == np.int32 and tab.shape == (512,) and not tab.flags.writeable and tab[0] == 2 and tab[511] == 512
    for j in range(512):
        # 2^(tab / 512) >= 1 + (j + 1) / 512, exactly: 2^tab >= ((513 + j) / 512)^512 in rationals
        assert Fraction(2) ** int(tab[j]) >= Fraction(513 + j, 512) ** 512, j
        assert Fraction(2) ** (int(tab[j]) - 1) < Fraction(513 + j, 512) ** 512, j                    # ... and the ceiling, not more
        assert tab[j] - 512.0 * math.log2(1.0 + j / 512.0) < 2.5, j                                   # over the bucket's lowest quotient by < 2.5 units
    assert (np.diff(tab) >= 0).all()


@pytest.mark.parametrize("W", [0, 1, 7, 64])
def test_the_gain_covers_every_need_and_holds_the_ceiling(W):
    from visinger_amd import limiter as lm
    rng = np.random.default_rng(2 + W)
    x = noise(rng, 3, 4000)
    lens = [4000, 2500, 4000]
    u, M, g, y = lm.limit_ref(x, lens, C_1DB, W)
    assert (u > 0).sum() > 100 and (g >= u).all() and (M >= u).all() and (g <= M.max()).all()
    exact = np.abs(x.astype(np.float64)) * np.exp2(-g / 512.0)                 # before the guard, in fp64
    for b, n in enumerate(lens):
        assert (exact[b, :n] <= float(C_1DB)).all()
        over = u[b] > 0
        need = 512.0 * np.log2(np.abs(x[b, over].astype(np.float64)) / float(C_1DB))
        assert ((u[b, over] - need) > 0).all() and ((u[b, over] - need) < 2.5).all()     # an upper bound, about 2.3 units over at most
        assert (np.abs(y[b, :n]) <= float(C_1DB)).all()
    assert np.array_equal(y[g == 0], x[g == 0].astype(np.float64))
    if W == 0:
        assert np.array_equal(g, u)                                             # a per-sample soft clip


def test_a_row_under_the_ceiling_gets_no_gain():
    from visinger_amd import limiter as lm
    rng = np.random.default_rng(3)
    x = np.clip(noise(rng, 2, 1000), -C_1DB, C_1DB)
    x[0, 10], x[1, 20] = C_1DB, -C_1DB                                          # |x| = c needs nothing
    u, M, g, y = lm.limit_ref(x, None, C_1DB, 16)
    assert not u.any() and not M.any() and not g.any() and np.array_equal(y, x.astype(np.float64))


@pytest.mark.parametrize("W", [1, 7, 64])
def test_a_lone_peak_gets_a_triangle_of_half_width_2w(W):
    from visinger_amd import limiter as lm
    n = 1000
    for p in (500, 0, 3, n - 1, n - W - 1):
        x = np.zeros((1, n), np.float32)
        x[0, p] = 3.0
        u, M, g, _ = lm.limit_ref(x, None, C_1DB, W)
        U, i = int(u[0, p]), np.arange(n)
        assert U > 0 and (u[0] > 0).sum() == 1 and g[0, p] == U
        assert np.array_equal(g[0] > 0, np.abs(i - p) <= 2 * W)                 # the support, cut at the row's ends
        assert (np.diff(g[0, :p + 1]) >= 0).all() and (np.diff(g[0, p:]) <= 0).all()
        lo, hi = np.maximum(i - W, 0), np.minimum(i + W, n - 1)                 # the overlap of the sample's window with the held stretch, over the window
        ov = np.maximum(0, np.minimum(hi, min(p + W, n - 1)) - np.maximum(lo, max(p - W, 0)) + 1)
        assert np.array_equal(g[0], -(-(U * ov) // (hi - lo + 1)))
        if p == 500:
            assert np.array_equal(g[0], -(-(U * np.maximum(0, 2 * W + 1 - np.abs(i - p))) // (2 * W + 1)))      # linear in the log domain


@pytest.mark.parametrize("W", [1, 7, 64])
def test_two_peaks_2w_apart_share_a_plateau(W):
    from visinger_amd import limiter as lm
    x = np.zeros((2, 1000), np.float32)
    x[0, 400] = x[0, 400 + 2 * W] = x[1, 400] = x[1, 400 + 2 * W + 2] = -2.5
    u, M, g, _ = lm.limit_ref(x, None, C_1DB, W)
    U = int(u[0, 400])
    assert (g[0, 400:400 + 2 * W + 1] == U).all() and g[0, 399] < U and g[0, 400 + 2 * W + 1] < U
    assert g[1, 400] == U == g[1, 400 + 2 * W + 2] and 0 < g[1, 400 + W + 1] < U      # two samples further apart: the held stretches no longer meet


def test_edge_values():
    from visinger_amd import limiter as lm
    tab = lm.reduction_table()
    for c in (C_1DB, np.float32(1.0), np.float32(0.25), np.float32(0.1)):
        x = np.array([[c, np.nextafter(c, np.float32(2)), -np.nextafter(c, np.float32(2)), np.inf, -np.inf, np.nan, 2 * c, c * np.float32(2.0 ** 24), 0.0]], np.float32)
        u, M, g, y = lm.limit_ref(x, None, c, 0)
        assert u[0].tolist() == [0, tab[0], tab[0], lm.U_MAX, lm.U_MAX, 0, 512 + tab[0], lm.U_MAX, 0]      # (a quotient of 2.0 opens the bucket j = 0 of e = 1)
        assert y[0, 3] == float(c) and y[0, 4] == -float(c) and np.isnan(y[0, 5]) and 0.99 * float(c) < y[0, 6] < float(c) and y[0, 0] == float(c)
    # a NaN within 2 W of a peak goes through the product and stays a NaN; further away it is not touched
    x = np.zeros((1, 64), np.float32)
    x[0, 10], x[0, 12], x[0, 40] = np.nan, 5.0, np.nan
    u, M, g, y = lm.limit_ref(x, None, C_1DB, 2)
    assert u[0, 10] == 0 and g[0, 10] > 0 and g[0, 40] == 0 and np.isnan(y[0, 10]) and np.isnan(y[0, 40]) and y[0, 12] <= float(C_1DB)
    assert np.array_equal(np.flatnonzero(g[0]), np.arange(8, 17))


def test_python_constants_are_the_headers():
    from visinger_amd import _lib
    from visinger_amd import limiter as lm
    header = open(os.path.join(ROOT, "include", "visinger_hip.h")).read()
    const = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))
    assert (const("VS_PEAK_LIMIT_TILE"), const("VS_PEAK_LIMIT_MAX_WINDOW"), const("VS_PEAK_LIMIT_TABLE"), const("VS_PEAK_LIMIT_U_MAX")) == \
        (lm.TILE, lm.WINDOW_LIMIT, lm.TABLE, lm.U_MAX) == (4096, 1024, 512, 12288)
    assert _lib.EXPECTED_ABI == 7 == _lib.lib().vs_abi_version()                # the new entry joins ABI 7
    f11 = re.sub(r"\s*\n \*\s*", " ", header[header.index(" * f11 "):header.index("#define VS_PEAK_LIMIT_TILE")])
    for text in ("0 < c <= 1", "tab[j] = ceil(512 log2(1 + (j + 1) / 512))", "min(512 e + tab[m >> 14], VS_PEAK_LIMIT_U_MAX)", "(S_i + N_i - 1) / N_i",
                 "S <= 2049 * 12288", "copysignf(c, y_i)", "exp2f(-(float) g_i / 512.0f)", "window outside [0, 1024]", "true) peaks are not seen"):
        assert text in f11, text
    assert "VS_API int vs_peak_limit(" in header and hasattr(_lib.lib(), "vs_peak_limit")
    assert lm.DEFAULTS == dict(ceiling_db=-1.0, window=128)
    assert lm.check_args() == (float(C_1DB), 128) and lm.check_args(ceiling_db=0, window=0) == (1.0, 0)
    c = lm.check_args(ceiling_db=-6.0)[0]
    assert c == float(np.float32(c)) == float(np.float32(10.0 ** -0.3))        # double, rounded once to fp32


def test_the_module_refuses_before_it_needs_a_gpu():
    import torch
    from visinger_amd import limiter as lm
    from visinger_amd._lib import VisingerHipError
    wav = torch.zeros(2, 1000)
    for kw in (dict(ceiling_db=0.1), dict(ceiling_db=-121), dict(ceiling_db=float("nan")), dict(ceiling_db=float("-inf")), dict(ceiling_db="-1"), dict(ceiling_db=None),
               dict(ceiling_db=True), dict(window=-1), dict(window=1025), dict(window=1.0), dict(window=True), dict(window=None), dict(bogus=1), dict(c=0.5)):
        with pytest.raises(ValueError):
            lm.limit_peaks(wav, **kw)
        if "bogus" not in kw and "c" not in kw:
            with pytest.raises(ValueError):
                lm.check_args(**kw)
    for call in (lambda: lm.limit_peaks(wav), lambda: lm.limit_peaks(wav.numpy()), lambda: lm.limit_peaks(None), lambda: lm.limit_peaks(wav.double()),
                 lambda: lm.limit_peaks(wav[0])):                                # no CPU path, whatever the values
        with pytest.raises(VisingerHipError):
            call()


def test_the_driver_refuses_the_new_key():
    from visinger_amd import synth
    item = dict(text_tokens=np.array([1, 2]), pitch_tokens=np.array([1, 2]), dur_tokens=np.array([2, 2]), mel2ph=np.array([1, 1, 2, 2]))
    for bad in ([1], 3, "soft", -1.0, dict(bogus=1), dict(ceiling_db=1), dict(ceiling_db=-500), dict(ceiling_db=float("nan")), dict(window=-1), dict(window=2000),
                dict(window=3.5), dict(sample_rate=24000)):
        with pytest.raises(ValueError, match="limit|ceiling_db|window"):
            synth.synthesize(None, [item], 8, limit=bad)                         # (refused before the model is looked at)


def test_every_einval_of_the_entry_with_its_string():
    """the entry validates before it launches, so its refusals are checked without a GPU, on fake addresses"""
    from visinger_amd import _lib
    L = _lib.lib()
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    X, LENS, TAB, Y, GAIN, STATS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
    call = lambda **a: L.vs_peak_limit(p(a["x"]), p(a["lens"]), p(a["tab"]), ctypes.c_float(a["c"]), a["window"], p(a["y"]), p(a["gain"]), p(a["stats"]), a["B"],
                                       a["L"], None)
    good = dict(x=X, lens=LENS, tab=TAB, c=0.89, window=128, y=Y, gain=GAIN, stats=STATS, B=2, L=4096)
    bad = {"NULL": [dict(x=None), dict(y=None), dict(tab=None)],
           "ceiling": [dict(c=0.0), dict(c=-0.5), dict(c=1.0000001), dict(c=2.0), dict(c=float("nan")), dict(c=float("inf"))],
           "window": [dict(window=-1), dict(window=1025)],
           "B >= 1 and L >= 1": [dict(B=0), dict(B=-1), dict(L=0), dict(L=-7)],
           "2^31": [dict(L=1 << 31), dict(B=1 << 60)],
           "in place": [dict(y=X + 4), dict(y=X - 4), dict(y=X + 4 * 8191)],
           "overlaps an input": [dict(gain=X), dict(gain=X + 4 * 100), dict(stats=X), dict(y=LENS), dict(gain=LENS + 8), dict(stats=LENS), dict(y=TAB), dict(gain=TAB + 2044),
                                 dict(stats=TAB)],
           "overlap each other": [dict(gain=Y), dict(gain=Y + 4 * 8191), dict(stats=Y + 16), dict(stats=GAIN)]}
    for word, cases in bad.items():
        for kw in cases:
            assert call(**dict(good, **kw)) == 1, kw                             # VS_EINVAL
            err = L.vs_last_error().decode()
            assert "vs_peak_limit" in err and word in err, (kw, err)
