"""Reference and bound for the default split-f16 arithmetic (VS_MATH_SPLIT3), element by element, built from the device's own operand planes.

The arithmetic (csrc/conv_common.h, conv_split_body.inc, conv_ktap.inc): an fp32 operand v becomes two f16 planes under a power-of-two scale s,
h = f16(v * s), l = f16(v * s - h) (split_pair_h: round to nearest even, the subtraction exact), s = 2^(14 - floor(log2 max)) -- for the activations
the largest transformed magnitude staged so far in the tile (a RUNNING scale: a later chunk with a larger one rescales the accumulators), for the
weights the largest |w| of the conv (pack_split_f16_body).  Per 16-channel chunk and tap the three cross products w_l x_h + w_h x_l + w_h x_h go through
v_mfma_f32_32x32x16_f16 -- every product of two f16 numbers is exact in fp32 -- onto an fp32 accumulator; the epilogue takes both scales out and adds
the bias with one fma.  So against ref = (conv(x_h, w_h) + conv(x_h, w_l) + conv(x_l, w_h)) / (s_x s_w) + bias taken in fp64 from the SAME planes only
the order of the fp32 accumulation (and the epilogue's few roundings) is left: |got - ref| <= F_SPLIT * 2^-24 * S, S = the sum of the absolute terms.
The arithmetic's own distance from the fp64 conv (22-bit operands, the dropped l l term) is 0.4 .. 1.4 * 2^-24 * S, and one dropped low cross product
of one (chunk, tap) step 17 .. 76 * 2^-24 * S on the median output -- under the 2e-5 * (1 + |ref|) bound of tests/test_conv_gpu.py, far above this one.

The planes are floating-point numbers, so their VALUES do not depend on the scale short of f16 under- and overflow; what the scale decides is where the
low plane goes subnormal (|l s| < 2^-14).  `pin_scale` makes that independent of the tile geometry: one row per 16-channel chunk holds, at every column,
positive values of one binade above every other magnitude, so every non-empty staged region of every chunk has the same largest exponent and ONE scale
per item reproduces the device's planes exactly, whatever the tile shape, chunk order or halo width.

F_SPLIT is not taken from the kernels.  It is the error of the reference's own fp32 accumulation: `serial_fp32` takes the reference expression with the
oracle's dtype = float32 conv -- every cross product's N plane products in ONE serial fp32 chain, for a given term count the order with the most
sequential roundings; the device sums in MFMA blocks of 16 -- and `serial_figure` compares it with the fp64 sum in units of 2^-24 * S.  Measured on the
CPU over all 155 distinct shapes of the tables below, pinned inputs (tests/test_split3_reference_cpu.py recomputes it): 0.89 .. 11.89, median 4.5
(SERIAL_F_MEASURED; the worst at 200 -> 136, k = 4, T = 261 behind lrelu + mask); rounded up to a power of two, F_SPLIT = 16.  (The pinned rows cost
something here: a sixteenth of the products is ~8 times the others, which raises a sum's error against S by about half.  For comparison, the device figure
recorded for the plain-bf16 kernels is 6.74, bf16_reference.PAIR_F_MEASURED.)

Measured on an MI355X, the largest |got - ref| / (2^-24 * S) the 216 comparisons of tests/test_conv_split3_oracle_gpu.py printed, by instance family:
conv_split_kernel<1, ..., 3> 5.43 / 5.54 / 5.54 / 5.39 (128 x 256, 64 x 256, 32 x 256, 32 x 128); conv_ktap_kernel<K, ACT, 2, 0, ...> 6.45 / 6.34 / 3.62 / 4.22
(the same tiles; the worst at 11 taps behind lrelu + mask); transposed: conv_split_tr_kernel 4.78, the polyphase conv_ktap instance 4.69; adjoint packs 4.51;
split_row / flip-in 2.95; the paired kinds at most 0.20 of their propagated bound; the un-pinned moving-scale group 13.15 against the fp64 conv, of its
derived 12 + 16 = 28 (the same figure on all three instances: it is the arithmetic's representation error under an outlier's scale, not the summation).
No instance above 6.5 of F_SPLIT = 16.
The weight scale itself (wscale, device memory of the handle) cannot be read back.  scale_of is checked bit for bit against f16_scale's formula in the
CPU self-test, and against the pack on the device where a plane's value does depend on the scale: output rows whose weights are f16 subnormals under s_w
(test_weight_scale_is_the_packs: 3.89 under s_w; the same reference under 2 s_w or s_w / 2 is flagged on 0.998 of those outputs).

Plain helper module (like bf16_reference.py): no fixtures, no tests.  ragged_mask, in_transform, finish and to_np are bf16_reference's.
"""
import numpy as np

from bf16_reference import finish, in_transform, ragged_mask, to_np  # noqa: F401  (re-exported: one definition for both checkers)

EPS32 = 2.0 ** -24
TOL = 2e-5                      # the bound of tests/test_conv_gpu.py, printed for comparison
SERIAL_F_MEASURED = 11.89       # the largest |serial fp32 sum - fp64 sum| / (2^-24 S) over the table shapes (module docstring)
F_SPLIT = 16.0                  # ... rounded up to a power of two

IN_NONE, IN_LRELU, IN_MASK, IN_LRELU_MASK = 0, 1, 2, 3        # (visinger_amd._lib.IN_*: this module imports nothing of the package)


# ---------------------------------------------------------------------------------------------------------------- the split, restated
def split_f16(v, s):
    """conv_common.h split_pair_h on v * s: h = f16(v s), l = f16(v s - h), round to nearest even (numpy's float16 conversion, subnormals
    included).  -> (h, l) as float64, in SCALED units"""
    vs = np.asarray(v, np.float32) * np.float32(s)               # (a power of two: exact)
    h = vs.astype(np.float16)
    l = (vs - h.astype(np.float32)).astype(np.float16)           # (the difference is exact in fp32)
    return h.astype(np.float64), l.astype(np.float64)


def scale_of(max_abs):
    """the scale of a tile / a weight whose largest magnitude is max_abs: 2^(14 - floor(log2 max)) -- f16_scale(eb) = 2^(141 - eb) with eb the biased
    exponent of the largest magnitude, floored at F16_EB_MIN = 24 (max below 2^-102, all zeros included); the weight pack's wscale[0] likewise"""
    m = np.float32(max_abs)
    eb = max(int(np.frexp(m)[1]) + 126, 24) if m > 0 else 24     # frexp: m = f * 2^e, f in [0.5, 1): floor(log2 m) = e - 1, biased e + 126
    return float(np.ldexp(1.0, 141 - eb))


def pin_scale(x, rng, mask=None):
    """-> a copy of x [B, C, T] whose every 16-channel chunk holds one row (the chunk's last) of positive values drawn from one binade
    [2^e, 2^(e+1)), 2^e above every other |x| (e >= 2), at every column.  Positive: the leaky-relu leaves them alone; a masked column zeroes them and
    the running maximum ignores zeros.  `mask` is not needed to place them (it zeroes whole columns) and is accepted for symmetry with the call sites."""
    x = np.array(x, np.float32)
    B, C, T = x.shape
    rows = [min(c0 + 15, C - 1) for c0 in range(0, C, 16)]
    other = np.ones(C, bool)
    other[rows] = False
    m = float(np.abs(x[:, other]).max()) if other.any() and x.size else 1.0
    e = max(2, int(np.floor(np.log2(max(m, 1e-30)))) + 1)
    x[:, rows] = np.ldexp(1.0 + rng.random((B, len(rows), T)), e).astype(np.float32)
    assert np.abs(x[:, other]).max(initial=0.0) < 2.0 ** e <= x[:, rows].min() and x[:, rows].max() < 2.0 ** (e + 1)
    return x


def _conv(oracle, x, w, transposed, dil_or_stride, padding, dtype=np.float64):
    if transposed:
        return oracle.conv_transpose1d(x, w, None, stride=dil_or_stride, padding=padding, dtype=dtype)
    return oracle.conv1d(x, w, None, dilation=dil_or_stride, padding=padding, dtype=dtype)


def planes(oracle, x, w, *, lrelu=False, in_mask=None, sx=None, sw=None):
    """-> (xt, w32, xh, xl, wh, wl, sx [B], sw): the transformed fp32 input, the fp32 weight, their planes (float64, scaled units) and the scales --
    one per item from the item's largest transformed magnitude, one per conv"""
    xt = in_transform(oracle, x, lrelu, in_mask)
    w32 = np.ascontiguousarray(to_np(w), np.float32)
    if sx is None:
        sx = np.array([scale_of(np.abs(xt[b]).max(initial=0.0)) for b in range(xt.shape[0])])
    if sw is None:
        sw = scale_of(np.abs(w32).max(initial=0.0))
    xh, xl = split_f16(xt, 1.0)
    for b in range(xt.shape[0]):
        xh[b], xl[b] = split_f16(xt[b], sx[b])
    wh, wl = split_f16(w32, sw)
    return xt, w32, xh, xl, wh, wl, np.asarray(sx, np.float64), float(sw)


def expected_pre(oracle, x, w, bias=None, *, transposed=False, dil_or_stride=1, padding=0, lrelu=False, in_mask=None, bias_b=None, rounded=True,
                 dtype=np.float64, sw=None):
    """-> (pre, S): (conv(x_h, w_h) + conv(x_h, w_l) + conv(x_l, w_h)) / (s_x s_w) + bias + per-item bias in fp64 from the device's planes (the first two
    as ONE conv with w_h + w_l, which fp64 holds exactly); S = conv(|x|, |w|) + |bias| + |bias_b| on the transformed fp32 input and the fp32 weight.
    w: the fp32 EFFECTIVE weight the library splits (weight-norm cases: ops.weightnorm_fold on the device), [C_out, C_in, k] or, transposed, [C_in, C_out, k].
    The keywords of bf16_reference.expected_pre: rounded=False -- the fp32 operands as they are (the plain fp64 conv); dtype=np.float32 -- serial_fp32.
    sw: a weight scale other than scale_of(max |w|) (what a mis-stated scale rule would give: tests/test_conv_split3_oracle_gpu.py)."""
    xt, w32, xh, xl, wh, wl, sx, sw = planes(oracle, x, w, lrelu=lrelu, in_mask=in_mask, sw=sw)
    if not rounded:
        pre = _conv(oracle, xt, w32, transposed, dil_or_stride, padding, dtype).astype(np.float64)
    elif np.dtype(dtype) == np.float32:
        pre = serial_fp32(oracle, xh, xl, wh, wl, sx, sw, None, transposed=transposed, dil_or_stride=dil_or_stride, padding=padding).astype(np.float64)
    else:
        pre = _conv(oracle, xh, wh + wl, transposed, dil_or_stride, padding) + _conv(oracle, xl, wh, transposed, dil_or_stride, padding)
        pre = pre / (sx[:, None, None] * sw)
    S = _conv(oracle, np.abs(xt), np.abs(w32), transposed, dil_or_stride, padding)
    for b_ in (None if bias is None else to_np(bias)[None, :, None], None if bias_b is None else to_np(bias_b)[:, :, None]):
        if b_ is not None:
            pre = pre + b_
            S = S + np.abs(b_)
    return pre, S


def expected(oracle, x, w, bias=None, *, res=None, acc=None, scale=1.0, out_act=None, out_mask=None, **conv):
    """expected_pre + bf16_reference.finish.  -> (ref, S)"""
    pre, S = expected_pre(oracle, x, w, bias, **conv)
    return finish(pre, S, res=res, acc=acc, scale=scale, out_act=out_act, out_mask=out_mask)


def figures(got, ref, S):
    """-> (err, worst |err| / (2^-24 S) over S > 0 [inf if an element with S = 0 differs], worst |err| / (2e-5 (1 + |ref|)))"""
    got, ref = to_np(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    per_s = 0.0
    if S is not None and err.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(S > 0, err / (EPS32 * np.where(S > 0, S, 1.0)), np.where(err > 0, np.inf, 0.0))
        per_s = float(np.nanmax(q))
    scaled = float(np.nanmax(err / (TOL * (1.0 + np.abs(ref))))) if err.size else 0.0
    return err, per_s, scaled


def assert_close(got, ref, S, what="", *, bound=None, F=None, tag="SPLIT3REF"):
    """Element-wise over ALL elements: |got - ref| <= F_SPLIT * 2^-24 * S (or `bound`, an array: the paired kinds and the moving-scale group state
    theirs), everything finite.  Prints `SPLIT3REF <what>: per_S <..> scaled <..>` (`tag`: another first word -- tests/exact_reference.py) before it
    asserts; the message names the worst index and how many elements exceed the bound.  -> (per_S, scaled)"""
    err, per_s, scaled = figures(got, ref, S)
    print(f"{tag} {what}: per_S {per_s:.3f} scaled {scaled:.4f}")
    g = to_np(got)
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} non-finite elements"
    bound = (F_SPLIT if F is None else F) * EPS32 * S if bound is None else np.asarray(bound, np.float64)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0.0))), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements above the bound; worst at {tuple(int(j) for j in i)}: "
                             f"got {g[i]!r}, ref {ref[i]!r}, |err| {err[i]:.3e}, bound {bound[i]:.3e}")
    return per_s, scaled


def flagged_fraction(got, ref, S, where, F=None):
    """share of the elements selected by `where` that assert_close would flag"""
    err, _, _ = figures(got, ref, None)
    return float((err[where] > (F_SPLIT if F is None else F) * EPS32 * S[where]).mean())


# ---------------------------------------------------------------------------------------------------------------- fp32 accumulations of the plane products
def serial_fp32(oracle, xh, xl, wh, wl, sx, sw, bias, *, transposed=False, dil_or_stride=1, padding=0):
    """the reference expression itself with fp32 sums: each cross product's N plane products in one serial fp32 chain (the oracle's float32 conv), the
    three chains added smallest first, scales taken out and the bias added in fp32 -- the accumulation F_SPLIT is derived from"""
    f = np.float32
    c = lambda a, b: _conv(oracle, a.astype(f), b.astype(f), transposed, dil_or_stride, padding, dtype=f)
    acc = (c(xh, wl) + c(xl, wh)) + c(xh, wh)
    assert acc.dtype == f
    y = acc * (1.0 / sx).astype(f)[:, None, None] * f(1.0 / sw)
    return (y + (0 if bias is None else np.asarray(bias, f)[None, :, None])).astype(f)


def blocked_fp32(xh, xl, wh, wl, sx, sw, bias, *, dilation=1, padding=0, defect=None):
    """A device-like accumulation for the checker's self-test: per 16-channel chunk and tap the three cross products w_l x_h, w_h x_l, w_h x_h, each a
    16-term fp32 block sum, added onto an fp32 accumulator (chunk outer, tap inner -- the order of conv_split_body.inc, and not the reference's);
    plain conv1d on [B, C, T] planes.  defect: None or
      ("drop", term, chunk, tap)  -- term "lh" (w_l x_h) / "hl" (w_h x_l): that cross product of that step is not taken
                                     (a fifth element, an index expression on [B, C_out, T_out]: only there -- one wave's 32 x 32 tile);
      ("hh", row, channel, tap)   -- ONE w_h x_h product of that output row is not taken;
      ("edge", tap, col)          -- output column `col` reads that tap from the neighbouring input column (col + 1), in every chunk;
      ("scale", chunk, factor)    -- that chunk's activation planes were made under factor * s_x while the accumulator is taken out under s_x"""
    f = np.float32
    B, C, T = xh.shape
    Cout, _, K = wh.shape
    Tout = T + 2 * padding - dilation * (K - 1)
    pad = ((0, 0), (0, 0), (padding, padding + 1))
    xh, xl = np.pad(xh.astype(f), pad), np.pad(xl.astype(f), pad)
    wh, wl = wh.astype(f), wl.astype(f)
    acc = np.zeros((B, Cout, Tout), f)
    for c, c0 in enumerate(range(0, C, 16)):
        cs = slice(c0, c0 + 16)
        fac = f(defect[2]) if defect and defect[0] == "scale" and defect[1] == c else f(1.0)
        for k in range(K):
            ts = slice(k * dilation, k * dilation + Tout)
            for term, wa, xb in (("lh", wl, xh), ("hl", wh, xl), ("hh", wh, xh)):
                region = None
                if defect and defect[0] == "drop" and defect[1:4] == (term, c, k):
                    if len(defect) == 4:
                        continue
                    region = defect[4]
                xs = np.ascontiguousarray(xb[:, cs, ts])                  # (contiguous 2-D operands: one sgemm per item)
                if fac != 1:
                    xs *= fac
                if defect and defect[0] == "edge" and defect[1] == k:
                    xs[:, :, defect[2]] = xb[:, cs, k * dilation + defect[2] + 1] * fac
                wk = np.ascontiguousarray(wa[:, cs, k])
                if defect and defect[0] == "hh" and term == "hh" and defect[3] == k and defect[2] // 16 == c:
                    wk[defect[1], defect[2] - c0] = 0
                prod = np.stack([wk @ xs[b] for b in range(B)])
                if region is not None:
                    prod[region] = 0
                acc += prod
    y = acc * (1.0 / sx).astype(f)[:, None, None] * f(1.0 / sw)
    return (y + (0 if bias is None else np.asarray(bias, f)[None, :, None])).astype(f)


def serial_figure(oracle, x, w, bias, ref_S=None, **conv):
    """worst |serial fp32 sum - fp64 sum| / (2^-24 S) of one case (ref_S: expected_pre's result where the caller has it)"""
    kw = {k: v for k, v in conv.items() if k in ("transposed", "dil_or_stride", "padding")}
    _, _, xh, xl, wh, wl, sx, sw = planes(oracle, x, w, lrelu=conv.get("lrelu", False), in_mask=conv.get("in_mask"))
    ref, S = ref_S if ref_S is not None else expected_pre(oracle, x, w, bias, **conv)
    return figures(serial_fp32(oracle, xh, xl, wh, wl, sx, sw, bias, **kw), ref, S)[1]


# ---------------------------------------------------------------------------------------------------------------- the shapes, shared by the GPU test and the CPU self-test
B = 2
# the tile kernel conv_split_kernel<1, NT_W, WAVES_M, WAVES_N, 3>: (tile, C_in, C_out, T, k, dilation) -- the grid of tests/test_conv_bf16_oracle_gpu.py TILE_CASES
TILE_CASES = [
    ("128x256", 33, 70, 257, 5, 2), ("128x256", 200, 136, 261, 1, 1), ("128x256", 40, 136, 5, 5, 3), ("128x256", 16, 70, 2, 4, 1), ("128x256", 64, 96, 129, 5, 5),
    ("128x256", 33, 70, 1, 5, 1),
    ("64x256", 33, 70, 261, 5, 3), ("64x256", 200, 136, 129, 4, 1), ("64x256", 16, 70, 1, 5, 2), ("64x256", 40, 136, 257, 1, 1), ("64x256", 48, 96, 5, 5, 5),
    ("64x256_nocfg", 40, 64, 257, 5, 2),
    ("32x256", 33, 20, 257, 5, 2), ("32x256", 200, 136, 261, 4, 1), ("32x256", 48, 70, 2, 5, 5), ("32x256", 16, 20, 5, 1, 1), ("32x256", 33, 70, 1, 5, 3),
    ("32x256_nocfg", 33, 20, 129, 5, 3),
    ("32x128", 33, 20, 129, 5, 3), ("32x128", 200, 70, 261, 1, 1), ("32x128", 64, 136, 257, 4, 1), ("32x128", 16, 20, 1, 5, 1), ("32x128", 40, 136, 5, 5, 2),
    ("32x128", 200, 20, 2, 1, 1),
]


def tile_variants(k):
    """the three launches of a tile case: (in_act, out_mask, res)"""
    return [(IN_NONE, False, False), (IN_LRELU_MASK, k % 2 == 1, False), (IN_LRELU if k > 1 else IN_MASK, False, True)]


_KTAP_DIL = {1: 1, 2: 1, 3: 2, 5: 1, 7: 3, 9: 1, 11: 5}
# every conv_ktap_kernel<K, ACT, 2, 0, ...> instance ktap_instance(3, cfg, kt, 0, in_act) admits (csrc/conv_ktap.hip): (tile, k, dilation, in_act)
KTAP_CASES = [("128x256", k, d, a) for k, d in ((3, 2), (7, 3), (11, 5)) for a in (IN_NONE, IN_LRELU, IN_MASK, IN_LRELU_MASK)] + \
             [("128x256", 9, 1, a) for a in (IN_NONE, IN_MASK)] + \
             [(t, k, _KTAP_DIL[k], IN_NONE) for t in ("64x256", "32x256", "32x128") for k in (1, 2, 3, 5, 7, 9, 11)] + \
             [(t, k, 1, IN_MASK) for t in ("64x256", "32x256", "32x128") for k in (1, 9)] + \
             [("64x256", k, d, IN_LRELU) for k, d in ((3, 1), (7, 3), (11, 5))]


def ktap_shapes(tile, k):
    """the two launches of a conv_ktap case: (C_in, C_out, T) -- an odd and an even chunk count, one past the column tile; C_out off the 32-row tile where
    the tile shape can be reached with one row tile"""
    T = 129 if tile == "32x128" else 261
    return [(48, 96, T), (32, 20 if tile in ("32x256", "32x128") else 136, T + 40)]


TR_SHAPES = [(64, 32, 16, 8, 40), (32, 32, 4, 2, 300), (48, 24, 11, 5, 33), (32, 16, 7, 3, 50), (512, 256, 16, 8, 16), (10, 6, 8, 4, 13),
             (48, 32, 11, 5, 159), (128, 64, 7, 3, 40)]          # (C_in, C_out, k, stride, T): tests/test_conv_gpu.py::test_conv_transpose1d
TR_KTAP = [(128, 64, 4, 2, 130), (128, 64, 4, 2, 261)]           # the polyphase conv_ktap instance
PAIR_TILES = [(64, 64, 140, 5, 1, "ktap_pair"), (64, 64, 140, 5, 1, "128x128"), (40, 24, 70, 3, 2, "128x128_k3"), (16, 16, 37, 5, 1, "64x256")]   # (H, C_in, T, k, d, id)


def conv_inputs(Cin, Cout, T, k, du, in_act, *, tr=False, seed=0, pin=True):
    """the inputs of one single-conv launch, the same on the GPU and in the self-test: x (pinned), w, bias, padding"""
    r = np.random.default_rng(1000 * Cin + 10 * Cout + T + 7 * k + du + in_act + seed)
    pad = (k - du) // 2 if tr else du * (k - 1) // 2
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    if pin:
        x = pin_scale(x, r)
    wshape = (Cin, Cout, k) if tr else (Cout, Cin, k)
    w = (r.standard_normal(wshape) / np.sqrt(Cin * k / (du if tr else 1))).astype(np.float32)
    bias = r.standard_normal(Cout).astype(np.float32)
    return r, x, w, bias, pad


def table_shapes():
    """every distinct (transposed, C_in, C_out, T, k, dilation / stride, in_act) the GPU file's tables launch"""
    out = []
    for _, Cin, Cout, T, k, d in TILE_CASES:
        out += [(False, Cin, Cout, T, k, d, a) for a, _, _ in tile_variants(k)]
    for tile, k, d, a in KTAP_CASES:
        out += [(False, Cin, Cout, T, k, d, a) for Cin, Cout, T in ktap_shapes(tile, k)]
    for Cin, Cout, k, u, T in TR_SHAPES:
        out += [(True, Cin, Cout, T, k, u, IN_LRELU), (True, Cin, Cout, T, k, u, IN_LRELU_MASK)]
    out += [(True, Cin, Cout, T, k, u, IN_LRELU) for Cin, Cout, k, u, T in TR_KTAP]
    out += [(False, Cin, 2 * H, T, k, d, IN_NONE) for H, Cin, T, k, d, _ in PAIR_TILES]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq
