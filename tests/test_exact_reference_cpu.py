"""Self-test of the exact-operand checker (tests/exact_reference.py) on oracle data alone: what it must accept, what it must flag.
A device is emulated in numpy float32, per 16-channel chunk and tap (tap group) the kept products as fp32 block sums onto fp32 accumulators
(exact_reference.blocked_fp32 / blocked_wino: the kernels' order, not the reference's).  (a) the restatements: the bf16 truncation split against torch integer
ops, the F(2,3) algebra against the direct conv; (b) the clean emulation passes at EVERY shape of the GPU file's tables and the serial fp32 chains the constants
F were taken from stay below them; (c) seeded defects are flagged, and for each one `EXACTDET ...` prints whether 2e-5 * (1 + |ref|) -- the bound these kernels
had -- flags it too."""
import numpy as np
import pytest
import torch

import exact_reference as R

B = R.B
MATHS = ("f32", "split6", "wino")
_CACHE = {}


def _sid(s):
    return "%s%d-%d_T%d_k%d_%d_a%d" % (("tr" if s[0] else "c",) + tuple(s[1:]))


def _case(shape):
    """-> (x, w, bias, conv keywords) of a table shape"""
    tr, Cin, Cout, T, k, du, a = shape
    _, x, w, bias, pad = R.conv_inputs(Cin, Cout, T, k, du, a, tr=tr)
    kw = dict(transposed=tr, dil_or_stride=du, padding=pad, lrelu=a in (R.IN_LRELU, R.IN_LRELU_MASK), in_mask=R.ragged_mask(B, T) if a >= R.IN_MASK else None)
    return x, w, bias, kw


def _emulate(oracle, math, x, w, bias, kw, defect=None):
    if math == "wino":
        xt, w32 = R.in_transform(oracle, x, kw["lrelu"], kw["in_mask"]), np.asarray(w, np.float32)
        d = kw["dil_or_stride"]
        tail = R.wino_form(w32.shape[0], w32.shape[2], d)[1]
        return R.blocked_wino(R.wino_U(w32, tail), R.wino_V(xt, w32.shape[2], d, tail), bias, R.wino_first(xt.shape[2], d), d, defect).astype(np.float64)
    if math == "f32":
        xp, wp, kept = [R.in_transform(oracle, x, kw["lrelu"], kw["in_mask"])], [np.asarray(w, np.float32)], [(0, 0)]
    else:
        _, _, xp, wp = R.planes6(oracle, x, w, lrelu=kw["lrelu"], in_mask=kw["in_mask"])
        kept = R.KEPT6
    xp, wp, dil, pad = R.as_conv1d(list(xp), list(wp), kw["transposed"], kw["dil_or_stride"], kw["padding"])
    return R.blocked_fp32(xp, wp, kept, bias, dilation=dil, padding=pad, defect=defect).astype(np.float64)


def _prep(oracle, math, shape):
    """-> (x, w, bias, conv keywords, ref, S, clean emulation, serial figure): computed once, shared by the tests below, never modified"""
    key = (math, shape)
    if key not in _CACHE:
        x, w, bias, kw = _case(shape)
        ref, S = R.expected_pre(oracle, math, x, w, bias, **kw)
        _CACHE[key] = (x, w, bias, kw, ref, S, _emulate(oracle, math, x, w, bias, kw), R.serial_figure(oracle, math, x, w, bias, ref_S=(ref, S), **kw))
    return _CACHE[key]


def _exact(oracle, x, w, bias, kw):
    """the plain fp64 conv: what 2e-5 * (1 + |ref|) was held against"""
    return R.expected_pre(oracle, "f32", x, w, bias, **kw)[0]


CASES = [(m, s) for m in MATHS for s in R.table_shapes(m)]


# ---- (a) the restatements
def test_truncation_split_is_the_integer_split_bit_for_bit():
    """conv_common.h split_pair<3> written with torch integer ops -- bits & 0xffff0000, the remainder by an fp32 subtraction -- against split_bf16x3, on random, tiny
    and huge values.  The exact sum back is asserted for normal planes only (the tables' operands); where the low plane would be subnormal the distance is printed."""
    r = np.random.default_rng(5)
    n = 20000
    groups = {"normal": r.standard_normal(n), "scaled": r.standard_normal(n) * np.exp2(r.integers(-40, 40, n)), "huge": r.standard_normal(n) * 2.0 ** 120,
              "tiny": r.standard_normal(n) * 2.0 ** -118, "edges": np.array([0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23, 3.0e38, 2.0 ** -126, 1.5 * 2.0 ** -100])}
    for name, v in groups.items():
        v = v.astype(np.float32)
        t = torch.from_numpy(v.copy())
        want, rem = [], t
        for _ in range(3):
            p = (rem.view(torch.int32) & -65536).view(torch.float32)
            want.append(p.numpy())
            rem = rem - p
        got = R.split_bf16x3(v, check=name != "tiny")
        for a, b_ in zip(got, want):
            assert np.array_equal(a.view(np.uint32), b_.view(np.uint32)), name
            assert not (a.view(np.uint32) & np.uint32(0xFFFF)).any()
        back = sum(a.astype(np.float64) for a in got)
        nz = v != 0
        print("EXACTSPLIT %s: worst |h + m + l - v| / |v| = %.3e" % (name, float(np.max(np.abs(back - v)[nz] / np.abs(v[nz].astype(np.float64)), initial=0.0))))
        if name != "tiny":
            assert np.array_equal(back, v.astype(np.float64))
            h, m, l = (np.abs(a.astype(np.float64)) for a in got)
            assert (m <= 2.0 ** -7 * np.abs(v)).all() and (l <= 2.0 ** -15 * np.abs(v)).all()      # what C_SPLIT6 is derived from


WINO_FORMS = sorted({(k, d, R.wino_form(Cout, k, d)[1], Cin, Cout) for Cin, Cout, k, d in R.WINO_CASES})


@pytest.mark.parametrize("k,d,tail,Cin,Cout", WINO_FORMS)
def test_wino_restatement_is_the_direct_conv(oracle, k, d, tail, Cin, Cout):
    """with fp64 transforms the F(2,3) restatement equals the direct fp64 conv to 1e-12 of S -- for every (k, dilation, tail form) of the table, on a T that spans
    more than one wave's pair map and ends inside a pair; with the kernel's fp32 transforms it sits within the printed distance: one rounding in V and two in U
    (the halving is exact) -- below 4 * 2^-24 * S_w"""
    T = 2 * (64 // d) * d + 2 * d + 1
    _, x, w, bias, pad = R.conv_inputs(Cin, Cout, T, k, d, R.IN_LRELU_MASK)
    xt = R.in_transform(oracle, x, True, R.ragged_mask(B, T))
    bt = [bias.astype(np.float64)[None, :, None]]
    direct = oracle.conv1d(xt.astype(np.float64), w.astype(np.float64), bias.astype(np.float64), dilation=d, padding=pad)
    S = oracle.conv1d(np.abs(xt).astype(np.float64), np.abs(w).astype(np.float64), np.abs(bias).astype(np.float64), dilation=d, padding=pad)
    y64, _ = R.wino_pre(oracle, xt, w, bt, d, transform=np.float64, tail=tail)
    assert np.abs(y64 - direct).max() <= 1e-12 * S.max(), float(np.abs(y64 - direct).max())
    assert (np.abs(y64 - direct) <= 1e-12 * np.maximum(S, 1e-300))[S > 0].all()
    y32, Sw = R.wino_pre(oracle, xt, w, bt, d, tail=tail)
    dist = R.figures(y32, direct, Sw)[1]
    print("EXACTWINO k%d d%d tail%d: fp32 transforms %.3f * 2^-24 * S_w from the direct conv (S_w / S up to %.2f)" % (k, d, tail, dist, float((Sw / np.maximum(S, 1e-300))[S > 0].max())))
    assert dist <= 4.0, dist
    if tail != 3:      # the zero-padded generic form of the same conv is the same function
        yg, _ = R.wino_pre(oracle, xt, w, bt, d, transform=np.float64, tail=3)
        assert np.abs(yg - direct).max() <= 1e-12 * S.max()


def test_wino_form_restates_the_dispatch_rule():
    for (Cout, k, d), want in {(128, 7, 1): (3, 1), (64, 7, 5): (3, 1), (96, 7, 3): (3, 3), (32, 7, 1): (3, 3), (128, 11, 5): (4, 2), (32, 11, 1): (4, 2),
                               (96, 11, 1): (4, 2), (32, 11, 3): (4, 3), (96, 11, 5): (4, 3), (64, 3, 1): (1, 3), (64, 9, 1): (3, 3), (128, 5, 3): (2, 3)}.items():
        assert R.wino_form(Cout, k, d) == want, (Cout, k, d)
    assert R.wino_instance(96, 11, 1) == "conv_wino_kernel<1, 1, 4, 4, 2>" and R.wino_instance(96, 11, 3) == "conv_wino_kernel<3, 1, 4, 0, 3>"
    assert [int(t) for t in np.nonzero(R.wino_first(140, 3))[0][:7]] == [0, 1, 2, 6, 7, 8, 12] and bool(R.wino_first(140, 3)[126]) and not R.wino_first(140, 3)[125]


# ---- (b) clean emulation, the constants
@pytest.mark.parametrize("math,shape", CASES, ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_clean_emulation_passes_and_serial_chain_is_within_f(oracle, math, shape):
    x, w, _, kw, ref, S, clean, f = _prep(oracle, math, shape)
    R.assert_close(clean, ref, S, "blocked fp32 %s %r" % (math, shape), F=R.F_OF[math])
    print("EXACTSERIAL %s %r: %.2f" % (math, shape, f))
    assert f <= R.F_OF[math], f
    if math == "split6":
        dist = R.split6_distance(oracle, x, w, **kw)
        print("EXACTSPLIT6 %r: the six kept products sit %.3f * 2^-24 * S from the fp64 conv" % (shape, dist))
        assert dist <= R.C_SPLIT6, dist


@pytest.mark.parametrize("math", MATHS)
def test_f_is_the_serial_figure_rounded_up(oracle, math):
    """F = the largest serial-chain figure over the family's table shapes, rounded up to a power of two (and the recorded figure is that maximum)"""
    figs = [_prep(oracle, math, s)[7] for s in R.table_shapes(math)]
    worst = max(figs)
    print("EXACTSERIAL %s: max %.2f over %d shapes (min %.2f, median %.2f)" % (math, worst, len(figs), min(figs), float(np.median(figs))))
    assert R.F_OF[math] / 2 < worst <= R.F_OF[math]
    assert abs(worst - R.SERIAL_MEASURED[math]) <= 0.05 * R.SERIAL_MEASURED[math], (worst, R.SERIAL_MEASURED[math])


def test_gain_case_planes_are_exact_and_pass(oracle):
    """per-channel gains of 2^-6 .. 2^6 and outlier runs: no scale enters the planes, so the split stays exact and the bound has no term for one; its constant is
    this data's own serial figure (an outlier term holds the partial sums at S: exact_reference's docstring)"""
    Cin, Cout, T, k, d = R.GAIN_CASE
    x, w, bias, pad = R.gain_inputs()
    kw = dict(transposed=False, dil_or_stride=d, padding=pad, lrelu=True, in_mask=R.ragged_mask(B, T))
    ref, S = R.expected_pre(oracle, "split6", x, w, bias, **kw)          # (split_bf16x3 asserts h + m + l == v on these operands too)
    per_s, _ = R.assert_close(_emulate(oracle, "split6", x, w, bias, kw), ref, S, "blocked fp32 split6 gains", F=R.F_SPLIT6_GAIN)
    f = R.serial_figure(oracle, "split6", x, w, bias, ref_S=(ref, S), **kw)
    print("EXACTSERIAL split6 gains: %.2f (the blocked emulation: %.2f)" % (f, per_s))
    assert R.F_SPLIT6_GAIN / 2 < f <= R.F_SPLIT6_GAIN and abs(f - R.SERIAL_MEASURED["split6_gain"]) <= 0.05 * f
    assert R.split6_distance(oracle, x, w, **kw) <= R.C_SPLIT6


# ---- (c) seeded defects
def _report(name, bad, clean, ref, S, F, exact):
    hit = bad != clean
    new, old = R.flagged(bad, ref, F * R.EPS32 * S), R.old_flagged(bad, exact)
    print("EXACTDET %s: touches %d outputs; F * 2^-24 * S flags %d, 2e-5 * (1 + |ref|) flags %d (worst %.2f of it)" %
          (name, int(hit.sum()), int(new.sum()), int(old.sum()), float((np.abs(bad - exact) / (R.TOL * (1.0 + np.abs(exact)))).max())))
    assert hit.any() and not new[~hit].any(), name
    assert new.any(), name
    return new, old


SPLIT6_DEFECT_SHAPES = [(False, 64, 96, 129, 5, 5, R.IN_NONE), (False, 200, 136, 261, 1, 1, R.IN_NONE), (False, 64, 136, 257, 4, 1, R.IN_NONE), (False, 40, 136, 257, 1, 1, R.IN_NONE)]
assert set(SPLIT6_DEFECT_SHAPES) <= set(R.table_shapes("split6"))


@pytest.mark.parametrize("shape", SPLIT6_DEFECT_SHAPES, ids=_sid)
def test_split6_dropped_products_are_flagged(oracle, shape):
    """one kept 2^-16-order product -- (1,1) m m, (2,0) l h, (0,2) h l -- dropped on every step of the launch, the same on one wave's 32 x 32 region only, and one
    2^-8-order product of one (chunk, tap) step"""
    _, Cin, Cout, T, k, d, _ = shape
    x, w, bias, kw, ref, S, clean, _ = _prep(oracle, "split6", shape)
    exact = _exact(oracle, x, w, bias, kw)
    region = (slice(0, 1), slice(32, 64), slice(32, 64))
    for prod in ((1, 1), (2, 0), (0, 2)):
        bad = _emulate(oracle, "split6", x, w, bias, kw, defect=("drop", prod, None, None))
        new, _ = _report("split6 %r: %r dropped for the whole launch" % (shape, prod), bad, clean, ref, S, R.F_SPLIT6, exact)
        assert new.mean() >= 0.05, float(new.mean())           # (the median element sits at 5 .. 15 units: not one lucky output)
        with pytest.raises(AssertionError, match="elements above"):
            R.assert_close(bad, ref, S, "dropped %r" % (prod,), F=R.F_SPLIT6)
        if T > 64:
            bad = _emulate(oracle, "split6", x, w, bias, kw, defect=("drop", prod, None, None, region))
            _report("split6 %r: %r dropped on one wave's 32 x 32 region" % (shape, prod), bad, clean, ref, S, R.F_SPLIT6, exact)
    for prod in ((1, 0), (0, 1)):
        bad = _emulate(oracle, "split6", x, w, bias, kw, defect=("drop", prod, Cin // 16 - 1, k // 2))
        new, _ = _report("split6 %r: %r of one (chunk, tap) step dropped" % (shape, prod), bad, clean, ref, S, R.F_SPLIT6, exact)
        assert new[bad != clean].mean() >= 0.9


@pytest.mark.parametrize("math,shape", [("f32", (False, 33, 136, 257, 5, 2, R.IN_NONE)), ("split6", (False, 33, 70, 257, 5, 2, R.IN_NONE)),
                                        ("f32", (False, 200, 170, 261, 4, 1, R.IN_NONE))], ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_tap_read_from_the_neighbouring_column_is_flagged(oracle, math, shape):
    assert shape in R.table_shapes(math)
    x, w, bias, kw, ref, S, clean, _ = _prep(oracle, math, shape)
    col = 255
    bad = _emulate(oracle, math, x, w, bias, kw, defect=("edge", shape[4] // 2, col))
    new, _ = _report("%s %r: column %d reads a tap from its neighbour" % (math, shape, col), bad, clean, ref, S, R.F_OF[math], _exact(oracle, x, w, bias, kw))
    assert new[0, :, col].mean() >= 0.9          # (item 0: its mask is all ones)


def _wino_shape(k, tail):
    return next(s for s in R.table_shapes("wino") if s[4] == k and R.wino_form(s[2], k, s[5])[1] == tail and s[3] > 100 and s[6] == R.IN_LRELU)


@pytest.mark.parametrize("k", [7])
def test_wino_one_tap_tail_not_negated_is_flagged(oracle, k):
    """the direct-form last tap of the k = 7 instances: y[t + d] takes it as -M3, so U3 is packed negated; without the sign every second output is off by twice
    that tap's contribution"""
    for shape in [s for s in R.table_shapes("wino") if s[4] == 7 and R.wino_form(s[2], 7, s[5])[1] == 1 and s[6] == R.IN_LRELU and s[3] > 100][::2]:
        x, w, bias, kw, ref, S, clean, _ = _prep(oracle, "wino", shape)
        bad = _emulate(oracle, "wino", x, w, bias, kw, defect=("u3_sign",))
        new, old = _report("wino %r: U3 of the one-tap tail not negated" % (shape,), bad, clean, ref, S, R.F_WINO, _exact(oracle, x, w, bias, kw))
        assert new[bad != clean].mean() >= 0.99


@pytest.mark.parametrize("k,tail", [(7, 1), (11, 2), (7, 3), (9, 3), (5, 3)])
def test_wino_last_group_missing_on_the_last_pair_column_is_flagged(oracle, k, tail):
    shape = _wino_shape(k, tail)
    T, d = shape[3], shape[5]
    x, w, bias, kw, ref, S, clean, _ = _prep(oracle, "wino", shape)
    base = 2 * (64 // d) * d - d - 1                           # the last pair column of the first wave: outputs base and base + d, the wave's last (inside the
    assert R.wino_first(T, d)[base] and base + d < T                 # sequence: at its end the last group reads the zero padding anyway)
    bad = _emulate(oracle, "wino", x, w, bias, kw, defect=("last_group", base))
    new, _ = _report("wino %r: last tap group missing at pair base %d" % (shape, base), bad, clean, ref, S, R.F_WINO, _exact(oracle, x, w, bias, kw))
    assert not (bad != clean)[:, :, [t for t in range(T) if t not in (base, base + d)]].any()


def _pair_emulate(oracle, math, x, w1, b1, w2, b2, k, d, res, zeroed=True):
    """the pair with the intermediate in fp32 between two blocked accumulations; zeroed=False: the intermediate's halo columns keep what conv1 computes there
    (bias + partial sums) instead of conv2's zero padding"""
    def planes(a):
        a = np.ascontiguousarray(a, np.float32)
        return ([a], [(0, 0)]) if math == "f32" else (list(R.split_bf16x3(a)), R.KEPT6)
    T, pad1, pad2 = x.shape[2], d * (k - 1) // 2, (k - 1) // 2
    xp, kept = planes(R.in_transform(oracle, x, True))
    t = R.blocked_fp32(xp, planes(w1)[0], kept, b1, dilation=d, padding=pad1 + pad2)
    if zeroed:
        t[:, :, :pad2] = 0
        t[:, :, T + pad2:] = 0
    a = R.in_transform(oracle, t, True)
    y = R.blocked_fp32(planes(a)[0], planes(w2)[0], kept, b2, dilation=1, padding=0)
    return (y + np.asarray(res, np.float32)).astype(np.float64)


@pytest.mark.parametrize("math", ["f32", "split6"])
@pytest.mark.parametrize("C,k,d,T", R.PAIR_CASES)
def test_pair_bound_passes_clean_and_flags_a_halo_that_is_not_zeroed(oracle, math, C, k, d, T):
    x, w1, b1, w2, b2, _ = R.pair_inputs(C, k, d, T)
    ref, bound, _ = R.pair_expected(oracle, math, x, w1, b1, w2, b2, k=k, d=d, res=x)
    clean = _pair_emulate(oracle, math, x, w1, b1, w2, b2, k, d, x)
    R.assert_close(clean, ref, None, "blocked fp32 pair %s C%d k%d d%d T%d" % (math, C, k, d, T), bound=bound)
    print("EXACTPAIR %s C%d k%d d%d T%d: of_bound %.3f" % (math, C, k, d, T, float((np.abs(clean - ref) / bound).max())))
    bad = _pair_emulate(oracle, math, x, w1, b1, w2, b2, k, d, x, zeroed=False)
    hit = bad != clean
    new, old = R.flagged(bad, ref, bound), R.old_flagged(bad, ref)
    print("EXACTDET pair %s C%d k%d d%d T%d: halo not zeroed touches %d outputs; the propagated bound flags %d, 2e-5 * (1 + |ref|) flags %d" %
          (math, C, k, d, T, int(hit.sum()), int(new.sum()), int(old.sum())))
    pad2 = (k - 1) // 2
    assert hit.any() and not hit[:, :, pad2:T - pad2].any() and new.any() and not new[~hit].any()
