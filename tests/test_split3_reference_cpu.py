"""Self-test of the split-f16 checker (tests/split3_reference.py) on oracle data alone: what it must accept, what it must flag.
A device is emulated by summing the plane products in fp32 per (16-channel chunk, tap) block, chunk outer and tap inner (split3_reference.blocked_fp32:
the order of conv_split_body.inc, not the reference's).  (a) the clean emulation passes at EVERY shape of the GPU file's tables, and the serial fp32 sum
F_SPLIT was derived from stays <= F_SPLIT; (b) seeded defects are flagged on the stated share of the outputs they touch (printed as `SPLIT3DET ...`);
(c) contrast: the dropped low cross product stays under 2e-5 * (1 + |ref|) on most outputs and under the 2e-6 rms bound altogether -- the blind spot of
the tests these kernels had."""
import numpy as np
import pytest

import split3_reference as R

B = R.B


_CACHE = {}


def _case(oracle, shape):
    """-> (x, w, bias, conv keywords) of a table shape"""
    tr, Cin, Cout, T, k, du, a = shape
    _, x, w, bias, pad = R.conv_inputs(Cin, Cout, T, k, du, a, tr=tr)
    kw = dict(transposed=tr, dil_or_stride=du, padding=pad, lrelu=a in (R.IN_LRELU, R.IN_LRELU_MASK),
              in_mask=R.ragged_mask(B, T) if a >= R.IN_MASK else None)
    return x, w, bias, kw


def _as_conv1d(xh, xl, wh, wl, kw):
    """a transposed conv as the plain conv the emulation takes: zero-stuffed planes, channel-transposed tap-reversed weight, padding k - 1 - p"""
    if not kw["transposed"]:
        return xh, xl, wh, wl, kw["dil_or_stride"], kw["padding"]
    u, k = kw["dil_or_stride"], wh.shape[2]

    def stuff(a):
        o = np.zeros(a.shape[:2] + ((a.shape[2] - 1) * u + 1,), a.dtype)
        o[:, :, ::u] = a
        return o

    flip = lambda a: np.ascontiguousarray(a.transpose(1, 0, 2)[:, :, ::-1])
    return stuff(xh), stuff(xl), flip(wh), flip(wl), 1, k - 1 - kw["padding"]


def _emulate(oracle, x, w, bias, kw, defect=None, sw=None, wl_scale=None):
    _, _, xh, xl, wh, wl, sx, sw_ = R.planes(oracle, x, w, lrelu=kw["lrelu"], in_mask=kw["in_mask"])
    if wl_scale is not None:        # the low weight plane made under wl_scale * s_w, taken out under s_w
        wl = wl * wl_scale
    xh, xl, wh, wl, dil, pad = _as_conv1d(xh, xl, wh, wl, kw)
    return R.blocked_fp32(xh, xl, wh, wl, sx, sw_, bias, dilation=dil, padding=pad, defect=defect).astype(np.float64)


def _prep(oracle, shape):
    """-> (x, w, bias, conv keywords, ref, S, clean emulation, serial figure) of a table shape: computed once, shared by the tests below, never modified"""
    if shape not in _CACHE:
        x, w, bias, kw = _case(oracle, shape)
        ref, S = R.expected_pre(oracle, x, w, bias, **kw)
        _CACHE[shape] = (x, w, bias, kw, ref, S, _emulate(oracle, x, w, bias, kw), R.serial_figure(oracle, x, w, bias, ref_S=(ref, S), **kw))
    return _CACHE[shape]


SHAPES = R.table_shapes()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s%d-%d_T%d_k%d_%d_a%d" % (("tr" if s[0] else "c",) + tuple(s[1:])))
def test_clean_emulation_passes_and_serial_sum_is_within_f_split(oracle, shape):
    _, _, _, _, ref, S, clean, f = _prep(oracle, shape)
    R.assert_close(clean, ref, S, "blocked fp32 %r" % (shape,))
    print("SPLIT3SERIAL %r: %.2f" % (shape, f))
    assert f <= R.F_SPLIT, f


def test_f_split_is_the_serial_figure_rounded_up(oracle):
    """F_SPLIT = the largest serial-sum figure over the table shapes, rounded up to a power of two (and the recorded figure is that maximum)"""
    figs = [_prep(oracle, s)[7] for s in SHAPES]
    worst = max(figs)
    print("SPLIT3SERIAL max %.2f over %d shapes (min %.2f)" % (worst, len(figs), min(figs)))
    assert R.F_SPLIT / 2 < worst <= R.F_SPLIT
    assert abs(worst - R.SERIAL_F_MEASURED) <= 0.05 * R.SERIAL_F_MEASURED, (worst, R.SERIAL_F_MEASURED)


def test_scale_and_split_restate_the_device_rule():
    # f16_scale(eb) = 2^(141 - eb), eb the biased exponent of the largest magnitude: every magnitude lands in [2^14, 2^15)
    for m, s in ((1.0, 2.0 ** 14), (1.999, 2.0 ** 14), (2.0, 2.0 ** 13), (7.3, 2.0 ** 12), (0.03, 2.0 ** 20), (2.0 ** 12, 4.0), (0.0, 2.0 ** 117), (1e-35, 2.0 ** 117)):
        assert R.scale_of(m) == s, (m, R.scale_of(m), s)
        if m > 2.0 ** -102:
            assert 2.0 ** 14 <= m * R.scale_of(m) < 2.0 ** 15
            eb = int(np.float32(m).view(np.uint32) >> 23) & 255
            assert R.scale_of(m) == float(np.uint32((268 - eb) << 23).view(np.float32))          # conv_common.h f16_scale, bit for bit
    v = np.array([1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10 + 2.0 ** -20, 3.0 * 2.0 ** -20, -0.7], np.float32)
    h, l = R.split_f16(v, 2.0 ** 14)
    assert h[0] == 2.0 ** 14 and l[0] == 8.0                         # a tie rounds to even, the low plane holds the rest
    assert np.all(np.abs(v * 2.0 ** 14 - (h + l)) <= 2.0 ** -22 * np.abs(v) * 2.0 ** 14 + 2.0 ** -25)      # 22 significant bits, or the subnormal floor
    assert np.all(h == h.astype(np.float16)) and np.all(l == l.astype(np.float16))


def test_pin_scale_gives_every_chunk_and_column_the_same_exponent():
    r = np.random.default_rng(3)
    for C in (16, 33, 40, 200):
        x = R.pin_scale(r.standard_normal((B, C, 37)).astype(np.float32) * 3.0, r)
        top = np.stack([np.abs(x[:, c0:c0 + 16]).max(axis=1) for c0 in range(0, C, 16)])        # [chunks, B, T]
        e = np.frexp(top)[1]
        assert (e == e.flat[0]).all()
        lr = np.where(x >= 0, x, x * np.float32(0.1))
        assert np.array_equal(np.abs(lr).max(axis=1), top.max(axis=0))                            # leaky-relu leaves the pinned rows on top


# ---- seeded defects.  (transposed, C_in, C_out, T, k, dilation / stride, in_act): every table shape with a whole 16-channel chunk and C_in * k <= 704 (a transposed
# conv in the zero-stuffed plain form the emulation takes: the dropped step is 16 channels at one of its k taps)
DEFECT_SHAPES = [s for s in SHAPES if s[1] >= 16 and s[1] * s[4] <= 704]
DEFECT_IDS = ["%s%d-%d_T%d_k%d_%d_a%d" % (("tr" if s[0] else "c",) + tuple(s[1:])) for s in DEFECT_SHAPES]
PLAIN_LONG = [s for s in DEFECT_SHAPES if not s[0] and s[3] >= 129 and s[1] % 16 == 0]


def _touched(bad, clean):
    return bad != clean


@pytest.mark.parametrize("shape", DEFECT_SHAPES, ids=DEFECT_IDS)
def test_dropped_low_cross_product_of_one_step_is_flagged(oracle, shape):
    """one dropped w_l x_h (`lh`) or w_h x_l (`hl`) product block -- 16 channels, one tap -- is flagged on >= half of the outputs it touches (what the
    2e-5 * (1 + |ref|) bound flags of them is printed next to it)"""
    x, w, bias, kw, ref, S, clean, _ = _prep(oracle, shape)
    k = shape[4]
    exact = R._conv(oracle, R.in_transform(oracle, x, kw["lrelu"], kw["in_mask"]).astype(np.float64), w.astype(np.float64), shape[0], shape[5], kw["padding"]) + bias[None, :, None]
    for term in ("lh", "hl"):
        bad = _emulate(oracle, x, w, bias, kw, defect=("drop", term, shape[1] // 16 - 1, k // 2))
        hit = _touched(bad, clean)
        assert hit.sum() >= 20, int(hit.sum())
        frac = R.flagged_fraction(bad, ref, S, hit)
        old = float((np.abs(bad - exact)[hit] > R.TOL * (1.0 + np.abs(exact[hit]))).mean())
        rms = float(np.sqrt(((bad - exact) ** 2).mean() / (exact ** 2).mean()))
        print("SPLIT3DET drop %s %r: flagged %.3f (2e-5 bound flags %.3f, rms %.2e)" % (term, shape, frac, old, rms))
        assert frac >= 0.5, frac
        with pytest.raises(AssertionError, match="elements above"):
            R.assert_close(bad, ref, S, "dropped %s" % term)


def test_contrast_the_existing_bounds_pass_the_dropped_low_product(oracle):
    """The blind spot this checker closes, at the shape family and on the inputs of tests/test_conv_ktap_gpu.py (128 -> 128, T = 4096 of one item, standard
    normal activations, not pinned): a w_l x_h block dropped in ONE wave's 32 x 32 output tile -- 16 channels, one tap -- stays under 2e-5 * (1 + |ref|) on
    more than half of the 1024 outputs it touches and under the 2e-6 rms bound of the launch altogether; the plane bound flags most of them."""
    Cin, Cout, T, k, d = 128, 128, 4096, 5, 1
    r, x, w, bias, pad = R.conv_inputs(Cin, Cout, T, k, d, R.IN_NONE, pin=False)
    x, kw = x[:1], dict(transposed=False, dil_or_stride=d, padding=pad, lrelu=False, in_mask=None)
    ref, S = R.expected_pre(oracle, x, w, bias, **kw)
    exact = oracle.conv1d(x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64), dilation=d, padding=pad)
    tile = (slice(0, 1), slice(32, 64), slice(256, 288))
    bad = _emulate(oracle, x, w, bias, kw, defect=("drop", "lh", Cin // 16 - 1, k // 2, tile))
    hit = np.zeros(ref.shape, bool)
    hit[tile] = True
    assert not (bad != _emulate(oracle, x, w, bias, kw))[~hit].any()
    frac = R.flagged_fraction(bad, ref, S, hit)
    old = float((np.abs(bad - exact)[hit] > R.TOL * (1.0 + np.abs(exact[hit]))).mean())
    rms = float(np.sqrt(((bad - exact) ** 2).mean() / (exact ** 2).mean()))
    print("SPLIT3DET contrast: plane bound flags %.3f, 2e-5 * (1 + |ref|) flags %.3f, rms %.2e" % (frac, old, rms))
    assert frac >= 0.5 and old < 0.5 and rms <= 2e-6, (frac, old, rms)


@pytest.mark.parametrize("shape", PLAIN_LONG[::4], ids=lambda s: "c%d-%d_T%d_k%d_%d_a%d" % tuple(s[1:]))
def test_other_seeded_defects_are_flagged(oracle, shape):
    _, Cin, Cout, T, k, d, a = shape
    x, w, bias, kw, ref, S, clean, _ = _prep(oracle, shape)
    shares = {}
    # one dropped h h product: output row 3, an ordinary (not pinned) input channel, the centre tap
    _, _, xh, _, wh, _, _, _ = R.planes(oracle, x, w, lrelu=kw["lrelu"], in_mask=kw["in_mask"])
    bad = _emulate(oracle, x, w, bias, kw, defect=("hh", 3, Cin - 2, k // 2))
    only = np.zeros_like(wh)
    only[3, Cin - 2, k // 2] = wh[3, Cin - 2, k // 2]
    contrib = oracle.conv1d(xh, only, None, dilation=d, padding=kw["padding"])
    assert (contrib != 0).any() and not (bad != clean)[contrib == 0].any()
    shares["hh"] = R.flagged_fraction(bad, ref, S, contrib != 0)
    # one chunk's planes made under half / double the scale the accumulator is taken out under
    for fac in (0.5, 2.0):
        bad = _emulate(oracle, x, w, bias, kw, defect=("scale", Cin // 16 - 1, fac))
        shares["scale x%g" % fac] = R.flagged_fraction(bad, ref, S, _touched(bad, clean))
    # the low weight plane made under half the weight scale
    bad = _emulate(oracle, x, w, bias, kw, wl_scale=0.5)
    shares["s_w"] = R.flagged_fraction(bad, ref, S, _touched(bad, clean))
    # one masked column left unmasked: the first masked frame of item 1
    if kw["in_mask"] is not None:
        m2 = kw["in_mask"].copy()
        col = int(m2[1].sum())
        m2[1, col] = 1.0
        bad = _emulate(oracle, x, w, bias, dict(kw, in_mask=m2))
        hit = np.zeros(ref.shape, bool)
        hit[1, :, [t for t in range(ref.shape[2]) if any(t + j * d - kw["padding"] == col for j in range(k))]] = True
        shares["unmasked column"] = R.flagged_fraction(bad, ref, S, hit)
    # a tap read from the neighbouring column at the 256-column tile edge
    if ref.shape[2] > 257:
        bad = _emulate(oracle, x, w, bias, kw, defect=("edge", k // 2, 256))
        hit = np.zeros(ref.shape, bool)
        hit[0, :, 256] = True            # (item 0: its mask is all ones)
        shares["tile edge"] = R.flagged_fraction(bad, ref, S, hit)
    print("SPLIT3DET %r: %s" % (shape, ", ".join("%s %.3f" % kv for kv in shares.items())))
    for name, frac in shares.items():
        assert frac >= 0.9, (name, frac)
