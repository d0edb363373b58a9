"""Self-test of the weight-gradient checker (tests/wgrad_reference.py) on the CPU alone: what it must accept, what it must flag.

(a) split_bf16x3 is exact and its planes carry the value's sign; the dispatch rule restated gives the counts the tables were chosen for; the plain fp64
    gradient agrees with the oracle's conv1d run as a correlation.
(b) the serial fp32 chain the bounds are derived from passes assert_close at EVERY table shape, the recomputed figures are the recorded constants and each F
    is the power of two above its figure (printed as `WGRADSERIAL ...`).  The arithmetic's own distance from the plain fp64 gradient -- the three dropped
    plane products, derived <= (2^-22 + 2^-22 + 2^-30) |gy| |x| = 8.004 units per product -- printed per group (`WGRADOWN ...`): A 0.24 .. 0.38, B 0.11 .. 0.18,
    D 0.29 .. 0.34 * 2^-24 * S (randn: the signs cancel), impulse group 4.2 .. 6.9 (one product per output: nothing cancels), which is why the plane reference is
    required there.
(c) a device-like accumulation (wgrad_reference.emulate_split: 64-position units dealt to the reduction slices, fp32 block products, fp32 plane sum) passes,
    the impulse group at 0.96 .. 1.01 units against F_IMPULSE = 10 (a rounding adder); with a seeded defect it is flagged (printed as `WGRADDET <defect> <case>:
    flagged <share of all outputs> touched <share of the outputs the defect changed> (median, worst units)`):
      one small cross product (g1 x1 | g2 x0 | g0 x2) dropped   impulse group: every case, 0.81 .. 1.00 of the outputs outside the padding (median 59 .. 140 units);
                                                                group A: every shape (DROP_NOT_FLAGGED_ON_A is empty), but on 0.15 .. 0.22 of its outputs only
                                                                (median 7.5 .. 8.7 units, worst 40 .. 58 against F_WGRAD = 16) -- the impulse group covers this class;
      a tap read one position off; odd offsets one position off (not where every offset is even); the ragged last unit not zeroed (not at K = 1 or under full
      padding, where x is zero there anyway); one unit skipped; one partial plane left out; the absent last tap of a tap half stored (K = 9, 11); bias sums
      on the wrong rows                                         group A: every shape it applies to, >= 0.99 of the outputs it touches;
      planes rounded to nearest even instead of truncated       NOT flagged anywhere (DOES_NOT_FLAG): the rounded split is as exact as the truncated one; it moves
                                                                group A by 0.6 .. 1.1 units and stays inside F_IMPULSE on the impulse group."""
import numpy as np
import pytest

import wgrad_reference as R

_OPS = None
_CACHE = {}


def _operands():
    global _OPS
    if _OPS is None:
        _OPS = {cid: (a, bw, split) for cid, a, bw, split in R.table_operands()}
    return _OPS


OP_IDS = [cid for cid, _, _, _ in R.table_operands()]


def _prep(cid):
    """-> (a, bw, split, ref, S, serial figure, own distance) of a table shape: computed once, shared, never modified"""
    if cid not in _CACHE:
        a, bw, split = _operands()[cid]
        ref, S = R._core(a, bw, rounded=split)
        ca, cb = R.serial_subset(a.shape[1], bw.shape[1], bw.shape[2])
        sub = np.ix_(ca, cb)
        ser = R.serial_fp32(a, bw, split=split, ca=ca, cb=cb).astype(np.float64)
        f = R.assert_close(ser, ref[sub], S[sub], "serial_fp32 " + cid, F=R.F_WGRAD if split else R.F_WGRAD_F32)[0]
        own = R.figures(ref, R._core(a, bw, rounded=False)[0], S)[1] if split else 0.0
        _CACHE[cid] = (a, bw, split, ref, S, f, own)
    return _CACHE[cid]


# ---- (a)
def test_split_is_exact_and_planes_carry_the_sign():
    r = np.random.default_rng(5)
    v = np.concatenate([r.standard_normal(4096) * np.exp2(r.integers(-40, 40, 4096)), [0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, -(2.0 - 2.0 ** -23), 2.0 ** -60, 3e38]]).astype(np.float32)
    p = R.split_bf16x3(v)
    assert p.dtype == np.float32 and np.array_equal(p.astype(np.float64).sum(0), v.astype(np.float64))        # the value, exactly
    assert np.all((p.view(np.uint32) & 0xFFFF) == 0)                                                          # bf16 numbers
    assert np.all(p * np.sign(v)[None] >= 0)                                                                  # truncation: no plane against the value's sign
    assert np.all(np.abs(p[1]) <= 2.0 ** -7 * np.abs(v)) and np.all(np.abs(p[2]) <= 2.0 ** -15 * np.abs(v))
    one = R.split_bf16x3(np.float32(1.0 + 2.0 ** -8 + 2.0 ** -23))
    assert list(one) == [1.0, 2.0 ** -8, 2.0 ** -23]                                                          # truncated, not rounded
    with pytest.raises(AssertionError):
        R.split_bf16x3(np.float32(2.0 ** -70))


def test_dispatch_rule_restated_gives_the_counts_the_tables_mean():
    assert R.split_slices(3, 384, 192, 708) == 29 and 3 * R.ceil_div(708, 64) == 36            # group B: 36 units on 29 slices
    assert R.split_slices(1, 64, 32, 2304) == 36                                               # 36 planes for the finish kernel
    assert R.f32_planes(3, 192, 192, 2561, 5) == 29 and 3 * R.ceil_div(2561, 256) == 33        # group E: 33 units on 29 slices
    assert R.wgrad_split_ok(2, 72, 256, 5) and not R.wgrad_split_ok(1, 72, 508, 5) and not R.wgrad_split_ok(2, 72, 258, 5)
    assert not R.wgrad_split_ok(2, 40, 260, 5) and not R.wgrad_split_ok(2, 72, 260, 13)
    for c in R.table_cases() + R.C_CASES + [R.C_GAINS]:
        ok = R.wgrad_split_ok(c.B, c.Cout, c.Tout, c.K)
        assert ok or not c.split, c
        if ok:          # the plane count tells the two kernels apart -- but for the shapes listed, which the rule alone vouches for
            differ = R.split_slices(c.B, c.Cout, c.Cin, c.Tout) != R.f32_planes(c.B, c.Cout, c.Cin, c.Tout, c.K)
            assert differ == ((c.B, c.Cout, c.Cin, c.Tout, c.K) not in R.COUNTS_COINCIDE), c
        assert (c.K - 1) * c.dil <= 64 and c.K <= 16
    assert [R.transposed_role(*tr[:6]) in R.COUNTS_COINCIDE for tr in R.D_TRANSPOSED] == [True, False, True]
    assert {R.kernel_by_rule(2, 72, 40, 260, k) for k, _ in R.A_TAPS} == {"conv_wgrad_split_kernel<%d, %d>" % kt for kt in
                                                                          [(k, 1) for k in range(1, 8)] + [(4, 2), (5, 2), (6, 2)]}
    assert max((k - 1) * d for k, d in R.A_TAPS) == 64 and 63 in {(k - 1) * d for k, d in R.A_TAPS}
    for tr in R.D_TRANSPOSED:
        B, Co, Ci, T, Q = R.transposed_role(*tr[:6])
        assert R.wgrad_split_ok(B, Co, T, Q)
    B, Co, Ci, T, Q = R.strided_role(*R.D_STRIDED)
    assert R.wgrad_split_ok(B, Co, T, Q) and R.split_slices(B, Co, Ci, T) != R.f32_planes(B, Co, Ci, T, Q)
    assert Co * Ci < 256 * 256 and Q <= 16                                                     # StridedConv1dFn's own rule: the conv_wgrad branch


def test_plain_gradient_agrees_with_the_oracle_conv(oracle):
    """rounded=False against the oracle's conv1d taken as a correlation of x (channels = items) with gy: another code path for the same sum"""
    c = R.Case("A", 2, 40, 72, 260, 5, 16)
    gy, x, pad = R.inputs(c)
    ref, _ = R.expected(gy, x, c.K, c.dil, pad, rounded=False)
    full = oracle.conv1d(x.transpose(1, 0, 2).astype(np.float64), gy.transpose(1, 0, 2).astype(np.float64), None, dilation=1, padding=pad)      # [C_in, C_out, span + 1]
    want = full[:, :, ::c.dil].transpose(1, 0, 2)
    assert want.shape == ref.shape and np.abs(want - ref).max() <= 1e-12 * np.abs(ref).max()


# ---- (b)
@pytest.mark.parametrize("cid", OP_IDS)
def test_serial_chain_is_within_its_bound(cid):
    _, _, split, _, _, f, own = _prep(cid)
    print("WGRADSERIAL %s: %.2f (%s) own distance %.3f" % (cid, f, "split" if split else "fp32", own))
    assert f <= (R.F_WGRAD if split else R.F_WGRAD_F32)
    assert own <= 8.01


def _pow2_above(v):
    return 2.0 ** np.ceil(np.log2(v))


def test_bounds_are_the_serial_figures_rounded_up():
    figs = {True: [], False: []}
    for cid in OP_IDS:
        p = _prep(cid)
        figs[p[2]].append(p[5])
    for split, rec, F in ((True, R.SERIAL_F_MEASURED, R.F_WGRAD), (False, R.SERIAL_F32_MEASURED, R.F_WGRAD_F32)):
        worst = max(figs[split])
        print("WGRADSERIAL %s: %.2f .. %.2f over %d shapes" % ("split" if split else "fp32", min(figs[split]), worst, len(figs[split])))
        assert abs(worst - rec) <= 0.005 + 1e-9, (worst, rec)
        assert F == _pow2_above(rec)
    bias = []
    for c in R.table_cases():
        gy, _, _ = R.inputs(c)
        ref, S = R.expected_bias(gy)
        bias.append(float((np.abs(R.serial_bias(gy) - ref) / (R.EPS32 * S)).max()))
    print("WGRADSERIAL bias: %.2f .. %.2f over %d shapes" % (min(bias), max(bias), len(bias)))
    assert abs(max(bias) - R.SERIAL_BIAS_MEASURED) <= 0.005 + 1e-9 and R.F_BIAS == _pow2_above(R.SERIAL_BIAS_MEASURED)
    assert (R.F_IMPULSE, R.F_IMPULSE_F32) == (10.0, 4.0)          # derived, not measured: 5 additions x one ulp; one product + one addition


def test_own_distance_per_group():
    by = {}
    for cid in OP_IDS:
        p = _prep(cid)
        if p[2]:
            by.setdefault(cid.split("_")[0], []).append(p[6])
    for g, v in sorted(by.items()):
        print("WGRADOWN group %s: kept six against the plain fp64 gradient %.3f .. %.3f" % (g, min(v), max(v)))
        assert max(v) < 1.0            # randn: far under F_WGRAD -- the fp64 gradient would do there; not so on the impulse group (below)


# ---- (c)
A_IDS = [R.case_id(c) for c in R.A_CASES]
_A = {}


def _a_case(c):
    if c not in _A:
        gy, x, pad = R.inputs(c)
        ref, S = R.expected(gy, x, c.K, c.dil, pad)
        clean, gb = R.emulate_split(gy, x, c.K, c.dil, pad, bias=True)
        _A[c] = (gy, x, pad, ref, S, clean, gb)
    return _A[c]


@pytest.mark.parametrize("c", R.A_CASES + R.B_CASES[:1], ids=R.case_id)
def test_clean_emulation_passes(c):
    gy, x, pad, ref, S, clean, gb = _a_case(c)
    R.assert_close(clean, ref, S, "emulate_split " + R.case_id(c))
    bref, bS = R.expected_bias(gy)
    assert np.all(np.abs(gb - bref) <= R.F_BIAS * R.EPS32 * bS)


@pytest.mark.parametrize("c", R.E_CASES[:8] + R.EDGE_CASES[1:], ids=R.case_id)
def test_clean_fp32_emulation_passes(c):
    gy, x, pad = R.inputs(c)
    ref, S = R.expected(gy, x, c.K, c.dil, pad, rounded=False)
    R.assert_close(R.emulate_f32(gy, x, c.K, c.dil, pad), ref, S, "emulate_f32 " + R.case_id(c), F=R.F_WGRAD_F32)


DROP_NOT_FLAGGED_ON_A = []          # group-A shapes on which a dropped small cross product passes F_WGRAD (none: each has outputs above 16 units)
DOES_NOT_FLAG = ["rne"]             # planes rounded to nearest even: see the module docstring


def _flag(bad, ref, S, clean, what, F=R.F_WGRAD):
    """-> (share of all outputs flagged, share of the outputs the defect changed)"""
    hit = bad != clean
    allf = R.flagged_fraction(bad, ref, S, F=F)
    touched = R.flagged_fraction(bad, ref, S, hit, F=F) if hit.any() else 0.0
    med, worst = R.per_s_quantiles(bad, ref, S)
    print("WGRADDET %s: flagged %.4f touched %.4f (median %.1f worst %.1f units)" % (what, allf, touched, med, worst))
    return allf, touched


@pytest.mark.parametrize("c", R.A_CASES, ids=R.case_id)
def test_dropped_small_cross_product_on_group_a(c):
    gy, x, pad, ref, S, clean, _ = _a_case(c)
    for pair in R.SMALL:
        allf, _ = _flag(R.emulate_split(gy, x, c.K, c.dil, pad, defect=("drop", pair)), ref, S, clean, "drop g%d x%d %s" % (pair + (R.case_id(c),)))
        assert (allf > 0) == (R.case_id(c) not in DROP_NOT_FLAGGED_ON_A), (pair, allf)
        assert allf < 0.5          # ... and on a minority of the outputs: what the impulse group is for


@pytest.mark.parametrize("c", R.C_CASES + [R.C_GAINS], ids=R.case_id)
def test_impulse_group_emulation_and_dropped_cross_products(c):
    """one nonzero product per output: the device-like sum stays within the DERIVED F_IMPULSE (and far inside: a rounding adder), outputs in the padding are
    exactly 0, every dropped small cross product is flagged on most outputs of every case, and the plain fp64 gradient is NOT a usable reference here"""
    for col in R.C_COLS:
        gy, x, pad = R.inputs(c, impulse=col)
        ref, S = R.expected(gy, x, c.K, c.dil, pad)
        what = "%s col %r" % (R.case_id(c), col)
        clean = R.emulate_split(gy, x, c.K, c.dil, pad)
        per_s, _ = R.assert_close(clean, ref, S, "emulate_split impulse " + what, F=R.F_IMPULSE)
        assert per_s <= 5.0, per_s          # a ROUNDING adder: five additions, half an ulp (one unit) each -- half of what F_IMPULSE grants a truncating one
        n = col[1] + np.arange(c.K) * c.dil - pad
        outside = (n < 0) | (n >= x.shape[2])
        assert np.all(S[:, :, outside] == 0) and np.all(S[:, :, ~outside] > 0) and np.all(clean[:, :, outside] == 0)
        own = R.figures(ref, R.expected(gy, x, c.K, c.dil, pad, rounded=False)[0], S)[1]
        print("WGRADOWN impulse %s: kept six against the plain fp64 gradient %.2f" % (what, own))
        assert 4.0 < own <= 8.01, own
        for pair in R.SMALL:
            allf, _ = _flag(R.emulate_split(gy, x, c.K, c.dil, pad, defect=("drop", pair)), ref, S, clean, "drop g%d x%d impulse %s" % (pair + (what,)), F=R.F_IMPULSE)
            assert allf >= 0.75 * (~outside).mean(), (pair, allf)
        rne = R.emulate_split(gy, x, c.K, c.dil, pad, defect=("rne",))
        assert R.flagged_fraction(rne, ref, S, F=R.F_IMPULSE) == 0.0          # (DOES_NOT_FLAG)


@pytest.mark.parametrize("c", R.A_CASES, ids=R.case_id)
def test_structural_defects_are_flagged_on_group_a(c):
    gy, x, pad, ref, S, clean, gb = _a_case(c)
    K = c.K
    defects = [("tap_off", K // 2), ("skip_unit", 3), ("skip_plane", 2)]
    if c.Tout - pad < x.shape[2]:          # x has positions at or past T_out - pad: what the ragged unit's stale gy columns meet (not at K = 1, not under full padding)
        defects.append(("ragged",))
    if np.any((np.arange(K) * c.dil) % 2 == 1):
        defects.append(("odd_off",))
    if K in (9, 11):
        defects.append(("absent_tap",))
    for d in defects:
        bad = R.emulate_split(gy, x, K, c.dil, pad, defect=d)
        _, touched = _flag(bad, ref, S, clean, "%s %s" % (" ".join(str(v) for v in d), R.case_id(c)))
        assert touched >= 0.99, (d, touched)
        with pytest.raises(AssertionError, match="elements above"):
            R.assert_close(bad, ref, S, str(d))
    bref, bS = R.expected_bias(gy)
    _, bad_gb = R.emulate_split(gy, x, K, c.dil, pad, defect=("bias_rows",), bias=True)
    share = float((np.abs(bad_gb - bref) > R.F_BIAS * R.EPS32 * bS).mean())
    print("WGRADDET bias_rows %s: flagged %.4f" % (R.case_id(c), share))
    assert share >= 0.99
    rne = R.emulate_split(gy, x, K, c.dil, pad, defect=("rne",))
    allf, _ = _flag(rne, ref, S, clean, "rne %s" % R.case_id(c))
    assert (allf == 0.0) == ("rne" in DOES_NOT_FLAG)
