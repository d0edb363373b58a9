"""Self-test of the plain-bf16 checker (tests/bf16_reference.py) on oracle data alone: what it must accept, what it must flag.
(a) the oracle's own fp32-accumulated result on bf16-rounded operands passes; (b) ONE dropped product -- a zeroed weight element: output row
3, last input channel, last tap -- is flagged on >= 90 % of the outputs it contributes to (a condition on the bound: the rms and
3e-2 * (1 + |ref|) bounds the plain-bf16 kernels were held to before let it pass on most of them); (c) the un-rounded fp64 oracle FAILS: the checker
tells bf16 operands from fp32 ones.  One shape per tile family of tests/test_conv_bf16_oracle_gpu.py and every shape of the fused pair."""
import numpy as np
import pytest

import bf16_reference as R

# (transposed, C_in, C_out, T, k, dilation / stride, leaky-relu, masked)
SINGLE = [(False, 33, 70, 257, 5, 2, False, True),       # 128 x 256 tile, C_in off the 16-channel chunk
          (False, 200, 136, 261, 1, 1, False, False),    # 64 x 256
          (False, 33, 20, 129, 4, 1, True, True),        # 32 x 256, even k
          (False, 40, 136, 129, 5, 3, True, False),      # 32 x 128
          (False, 64, 96, 261, 7, 1, True, True),        # ktap, 128 x 256
          (False, 32, 128, 300, 11, 5, True, False),     # ktap k = 11, widest window
          (False, 64, 128, 140, 5, 1, False, False),     # the paired kinds' conv (k = 5)
          (True, 48, 24, 33, 11, 5, True, False)]        # transposed, polyphase


def _single(oracle, tr, Cin, Cout, T, k, du, lrelu, masked):
    r = np.random.default_rng(Cin + 3 * Cout + T + k)
    B = 2
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    w = (r.standard_normal((Cin, Cout, k) if tr else (Cout, Cin, k)) / np.sqrt(Cin * k / (du if tr else 1))).astype(np.float32)
    bias = r.standard_normal(Cout).astype(np.float32)
    kw = dict(transposed=tr, dil_or_stride=du, padding=(k - du) // 2 if tr else du * (k - 1) // 2, lrelu=lrelu,
              in_mask=R.ragged_mask(B, T) if masked else None)
    return x, w, bias, kw


@pytest.mark.parametrize("case", SINGLE, ids=lambda c: "%s%d-%d_T%d_k%d_%d" % (("tr" if c[0] else "c",) + c[1:6]))
def test_checker_on_single_convs(oracle, case):
    tr = case[0]
    x, w, bias, kw = _single(oracle, *case)
    ref, S = R.expected(oracle, x, w, bias, **kw)
    got32, _ = R.expected(oracle, x, w, bias, dtype=np.float32, **kw)              # (a) fp32 sums, serial: the longest error path
    scaled, per_s = R.assert_close(got32, ref, S=S, what="oracle fp32 %r" % (case,))
    assert scaled <= 0.25 and per_s <= 8.0, (scaled, per_s)
    wz = w.copy()                                                                   # (b)
    idx = (-1, 3, -1) if tr else (3, -1, -1)
    wz[idx] = 0
    bad, _ = R.expected(oracle, x, wz, bias, dtype=np.float32, **kw)
    only = np.zeros_like(w)
    only[idx] = w[idx]
    contrib, _ = R.expected(oracle, x, only, None, **kw)
    hit = contrib != 0
    assert hit[:, 3].any() and not hit[:, :3].any() and not hit[:, 4:].any()
    frac = R.flagged_fraction(bad, ref, hit)
    assert frac >= 0.9, frac
    with pytest.raises(AssertionError, match="elements above"):
        R.assert_close(bad, ref, what="dropped product")
    unrounded, _ = R.expected(oracle, x, w, bias, rounded=False, **kw)               # (c)
    assert R.flagged_fraction(unrounded, ref, np.ones(ref.shape, bool)) >= 0.5
    with pytest.raises(AssertionError, match="elements above"):
        R.assert_close(unrounded, ref, what="fp32 operands")
    # a bf16-resident output: rounded once, half an ulp on top -- accepted; the dropped product is still seen on most of its outputs
    R.assert_close(oracle.round_bf16(got32), ref, bf16_out=True, what="oracle fp32, bf16 out")


def _pair_fp32(oracle, x, w1, b1, w2, b2, k, d, res):
    """the fused pair as the device computes it, with the oracle's serial fp32 sums: intermediate in fp32, leaky-relu in fp32, rounded to bf16"""
    t, _ = R.expected_pre(oracle, x, w1, b1, dil_or_stride=d, padding=d * (k - 1) // 2, lrelu=True, dtype=np.float32)
    a = oracle.leaky_relu(t.astype(np.float32))
    y, _ = R.expected_pre(oracle, a, w2, b2, padding=(k - 1) // 2, dtype=np.float32)
    return (y.astype(np.float32) + res).astype(np.float64)


@pytest.mark.parametrize("C,k,d,T", R.PAIR_CASES)
def test_checker_on_the_fused_pair(oracle, C, k, d, T):
    x, w1, b1, w2, b2, _ = R.pair_inputs(C, k, d, T)
    ref, extra, _, _ = R.pair_expected(oracle, x, w1, b1, w2, b2, k=k, d=d, res=x)
    got = _pair_fp32(oracle, x, w1, b1, w2, b2, k, d, x)
    R.assert_close(got, ref, extra, what="oracle fp32 pair %r" % ((C, k, d, T),))     # (a)
    w2z = w2.copy()                                                                  # (b): conv2's weight, output row 3
    w2z[3, -1, -1 if k // 2 < T else k // 2] = 0                                     # (T = 4 under k = 11: the last tap reaches no frame -- the centre tap)
    bad = _pair_fp32(oracle, x, w1, b1, w2z, b2, k, d, x)
    changed = bad != got
    assert changed[:, 3].any() and not changed[:, :3].any() and not changed[:, 4:].any()
    frac = R.flagged_fraction(bad, ref, changed, extra)
    assert frac >= 0.9, frac
    unrounded = oracle.conv1d(oracle.leaky_relu(oracle.conv1d(oracle.leaky_relu(x.astype(np.float64)), w1, b1, dilation=d, padding=d * (k - 1) // 2)),
                              w2, b2, padding=(k - 1) // 2) + x                      # (c)
    with pytest.raises(AssertionError, match="elements above"):
        R.assert_close(unrounded, ref, extra, what="fp32 operands")
    assert R.flagged_fraction(unrounded, ref, np.ones(ref.shape, bool), extra) >= 0.5


def test_ulp_and_midpoint_marking(oracle):
    assert R.ulp_bf16(1.0) == 2.0 ** -7 and R.ulp_bf16(-1.99) == 2.0 ** -7 and R.ulp_bf16(2.0) == 2.0 ** -6 and R.ulp_bf16(0.0) == 0.0
    a = np.array([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -7], np.float64)
    r = oracle.round_bf16(a)
    assert r[0] == 1.0 and r[1] == 1.0 + 2.0 ** -7 and r[2] == a[2]          # ties to even; just above the midpoint: up
