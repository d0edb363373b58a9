"""Reference and bound for the plain-bf16 arithmetic (VS_MATH_BF16), element by element.

That arithmetic rounds both operands of every product to bfloat16 (round to nearest even, the activation AFTER its input transform) and
accumulates in fp32.  A product of two bf16 numbers is exact in fp32, so against a reference that rounds the operands the same way only the
ORDER of the fp32 accumulation is left -- exactly what the fp32-class bound of tests/test_conv_gpu.py, 2e-5 * (1 + |ref|), allows the
exact-fp32 engine.  `expected` builds that reference on the CPU oracle (fp64 sums under oracle.operand_rounding("bf16")), `assert_close`
holds a result to it, `pair_expected` does the same for the fused residual pair, whose intermediate is rounded to bf16 inside the launch.

Plain helper module (like aten_backend.py): no fixtures, no tests.
"""
import numpy as np

TOL = 2e-5                 # |got - ref| <= TOL * (1 + |ref|): the bound of tests/test_conv_gpu.py
EPS32 = 2.0 ** -24         # unit roundoff of fp32

# The fused pair's intermediate t = conv1(...) + b1 is an fp32 sum on the device and an fp64 sum here; the two differ by at most
# F_PAIR * 2^-24 * S, S = the sum of the absolute products (+ |b1|).  Where the reference's value lies that close to a bf16 rounding
# midpoint the device may round to the other neighbour (pair_expected).  F_PAIR is four times the largest |got - ref| / (2^-24 * S) the
# single-conv cases of tests/test_conv_bf16_oracle_gpu.py print, rounded up to a power of two.  Measured on an MI355X over the 169
# single-conv launches of that file: 6.74 (conv_split_kernel<1, 2, 1, 4, 1>, transposed 512 -> 256, k = 16: 1024 products per output);
# 4.58 at the reduction lengths of the pairs (<= 704 products).  4 * 6.74 = 27 -> 32.  (The oracle's own serial fp32 sum reaches 8.)
PAIR_F_MEASURED = 6.74
F_PAIR = 32.0


def to_np(t):
    """torch tensor (any float dtype, any device) or array -> float64 array"""
    if hasattr(t, "detach"):
        t = t.detach().float().cpu().numpy()
    return np.asarray(t, np.float64)


def ulp_bf16(a):
    """spacing of the bf16 numbers (8 significant bits) in the binade of |a|; 0 at 0"""
    a = np.abs(np.asarray(a, np.float64))
    _, e = np.frexp(a)                       # |a| = m * 2^e, m in [0.5, 1)
    return np.where(a > 0, np.ldexp(1.0, e - 8), 0.0)


def ragged_mask(B, T):
    """[B, T] 0/1 prefix mask: item 0 whole, the others cut at ~2/3, ~1/3 ... (at least one frame)"""
    lens = [max(1, T - (i * T) // 3 - (1 if i else 0)) for i in range(B)]
    return (np.arange(T)[None] < np.asarray(lens)[:, None]).astype(np.float32)


def in_transform(oracle, x, lrelu=False, mask=None):
    """the device's input transform, in FLOAT32 as the device applies it: leaky-relu (one fp32 multiply by 0.1f), then the exact 0/1 mask"""
    x = np.ascontiguousarray(x, np.float32)
    if lrelu:
        x = oracle.leaky_relu(x)
        assert x.dtype == np.float32
    if mask is not None:
        x = x * np.asarray(mask, np.float32)[:, None]
    return x


def _conv(oracle, x, w, transposed, dil_or_stride, padding, dtype=np.float64):
    if transposed:
        return oracle.conv_transpose1d(x, w, None, stride=dil_or_stride, padding=padding, dtype=dtype)
    return oracle.conv1d(x, w, None, dilation=dil_or_stride, padding=padding, dtype=dtype)


def expected_pre(oracle, x, w, bias=None, *, transposed=False, dil_or_stride=1, padding=0, lrelu=False, in_mask=None, bias_b=None, rounded=True,
                 dtype=np.float64):
    """-> (pre, S): conv(transform(x), w) + bias + per-item bias, operands rounded to bf16 (rounded=False: the fp32 operands as they are --
    the C_out <= 4 VALU instance), sums in `dtype`; S = conv(|x_r|, |w_r|) + |bias| + |bias_b|, the sum of the absolute terms in fp64.
    w: the fp32 EFFECTIVE weight the library rounds (weight-norm cases: ops.weightnorm_fold on the device), [C_out, C_in, k] or, transposed,
    [C_in, C_out, k]."""
    xt = in_transform(oracle, x, lrelu, in_mask)
    w = np.ascontiguousarray(to_np(w), np.float32)
    if rounded:
        xt, w = oracle.round_bf16(xt), oracle.round_bf16(w)
    with oracle.operand_rounding("bf16" if rounded else None):
        pre = _conv(oracle, xt, w, transposed, dil_or_stride, padding, dtype).astype(np.float64)
        S = _conv(oracle, np.abs(xt), np.abs(w), transposed, dil_or_stride, padding)
    for b_ in (None if bias is None else to_np(bias)[None, :, None], None if bias_b is None else to_np(bias_b)[:, :, None]):
        if b_ is not None:
            pre = pre + b_
            S = S + np.abs(b_)
    return pre, S


def finish(pre, S, *, res=None, acc=None, scale=1.0, out_act=None, out_mask=None):
    """the fused epilogue in fp64, unrounded: + residual + accumulate, * scale, activation ("tanh" / "relu"), output mask.  -> (ref, S)"""
    for t in (res, acc):
        if t is not None:
            pre = pre + to_np(t)
            S = S + np.abs(to_np(t))
    s = float(np.float32(scale))
    pre, S = pre * s, S * abs(s)
    if out_act == "tanh":
        pre = np.tanh(pre)
    elif out_act == "relu":
        pre = np.maximum(pre, 0.0)
    else:
        assert out_act is None, out_act
    if out_mask is not None:
        pre = pre * np.asarray(out_mask, np.float64)[:, None]
    return pre, S


def expected(oracle, x, w, bias=None, *, res=None, acc=None, scale=1.0, out_act=None, out_mask=None, **conv):
    """expected_pre + finish.  -> (ref, S)"""
    pre, S = expected_pre(oracle, x, w, bias, **conv)
    return finish(pre, S, res=res, acc=acc, scale=scale, out_act=out_act, out_mask=out_mask)


def figures(got, ref, S=None, extra=0.0, bf16_out=False):
    """-> (bound, err, worst |err| / (TOL * (1 + |ref|)) [the part of the error the fp32 sum is allowed], worst |err| / (2^-24 * S) or None)"""
    got, ref = to_np(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    allow = np.asarray(extra, np.float64) + (0.5 * ulp_bf16(ref) if bf16_out else 0.0)
    bound = TOL * (1.0 + np.abs(ref)) + allow
    scaled = float((np.maximum(err - allow, 0.0) / (TOL * (1.0 + np.abs(ref)))).max()) if err.size else 0.0
    per_s = None
    if S is not None and not bf16_out:
        ok = S > 0
        per_s = float((err[ok] / (EPS32 * S[ok])).max()) if ok.any() else 0.0
    return bound, err, scaled, per_s


def assert_close(got, ref, extra=0.0, *, bf16_out=False, S=None, what=""):
    """Element-wise |got - ref| <= 2e-5 * (1 + |ref|) + extra, everything finite; bf16_out: the result was rounded to bf16 once -- half a
    bf16 ulp at ref on top.  Prints the figures (instance / case in `what`; of_bound: the worst |err| / bound, `extra` and the half ulp
    included) before it asserts; the message names the worst index and how many elements exceed the bound.  -> (worst |err| / (2e-5 * (1 + |ref|)), worst |err| / (2^-24 * S) or None)"""
    bound, err, scaled, per_s = figures(got, ref, S, extra, bf16_out)
    of_bound = float((err / bound).max()) if err.size else 0.0
    print(f"BF16REF {what}: scaled {scaled:.3f}" + ("" if per_s is None else f" per_S {per_s:.3f}") + f" of_bound {of_bound:.3f}")
    g = to_np(got)
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} non-finite elements"
    bad = err > bound
    if bad.any():
        i = np.unravel_index(int(np.argmax(err / bound)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements above 2e-5 * (1 + |ref|) + extra; worst at {tuple(int(j) for j in i)}: "
                             f"got {g[i]!r}, ref {ref[i]!r}, |err| {err[i]:.3e}, bound {bound[i]:.3e}")
    return scaled, per_s


def flagged_fraction(got, ref, where, extra=0.0, bf16_out=False):
    """share of the elements selected by `where` (an index expression) that assert_close would flag"""
    bound, err, _, _ = figures(got, ref, None, extra, bf16_out)
    return float((err[where] > bound[where]).mean())


def pair_expected(oracle, x, w1, b1, w2, b2, *, k, d, res=None, acc=None, scale=1.0, F=None):
    """The fused residual pair y = (conv2(lrelu(conv1(lrelu(x)) + b1)) + b2 + res [+ acc]) * scale in plain bf16: both convs on operands
    rounded to bf16, the intermediate a = lrelu(t) rounded to bf16 INSIDE the launch.  -> (ref, extra, t, a_r).
    An intermediate element on a rounding boundary may round the other way on the device than here; that is bounded exactly instead of
    loosening the tolerance: with S = conv(|x_r|, |w1_r|) + |b1| and delta = F * 2^-24 * S (F_PAIR above), every element whose distance to
    a bf16 rounding midpoint is <= delta is marked, and extra = conv(ulp_bf16(a) * marked, |w2_r|) * scale: a marked element moves by one
    ulp at most, an unmarked one rounds as it does here.  (Elements with |t| <= delta may also change the branch of the leaky-relu; they
    move by no more than 2 * delta and are marked with that.)"""
    F = F_PAIR if F is None else F
    pad1, pad2 = d * (k - 1) // 2, (k - 1) // 2
    t, S1 = expected_pre(oracle, x, w1, b1, dil_or_stride=d, padding=pad1, lrelu=True)
    slope = float(np.float32(oracle.LRELU_SLOPE))
    a = np.where(t >= 0, t, t * slope)
    a_r = oracle.round_bf16(a)                                     # (through fp32: a value that changes there sits on a midpoint and is marked)
    delta = F * EPS32 * S1 + EPS32 * np.abs(a)                     # (+ the fp32 rounding of the leaky-relu's multiply)
    u = ulp_bf16(a)                                                # the bf16 grid is uniform inside a's binade: midpoints at (n + 1/2) * u
    q = np.abs(a) / np.where(u > 0, u, 1.0)
    marked = (np.abs(q - np.floor(q) - 0.5) * u <= delta) & (a != 0)
    move = np.where(marked, u, 0.0)
    move = np.maximum(move, np.where(np.abs(t) <= delta, 2.0 * delta, 0.0))
    w2r = oracle.round_bf16(np.ascontiguousarray(to_np(w2), np.float32))
    y, S2 = expected_pre(oracle, a_r, w2r, b2, padding=pad2)     # (a_r, w2r: bf16 numbers already)
    extra = oracle.conv1d(move, np.abs(w2r), None, padding=pad2)
    ref, _ = finish(y, S2, res=res, acc=acc, scale=scale)
    return ref, extra * abs(float(np.float32(scale))), t, a_r


# the fused pair's shapes, shared by the GPU test and the CPU self-test of this checker: (C, k, dilation of conv1, T); B = 2.
# (Wider pairs dilute what the bound can see -- the marked share of an output's receptive field grows with C * k -- so the shapes stop at
# 64 channels, where tests/test_bf16_reference_cpu.py still finds one dropped product on >= 90 % of its outputs.)
PAIR_CASES = [(32, 3, 1, 4), (32, 3, 3, 250), (32, 7, 3, 37), (32, 7, 5, 777), (32, 11, 1, 37), (32, 11, 5, 250),
              (64, 3, 1, 37), (64, 3, 5, 777), (64, 7, 1, 250), (64, 7, 3, 4), (64, 11, 3, 777), (64, 11, 5, 4)]


def pair_inputs(C, k, d, T, B=2):
    r = np.random.default_rng(C * 31 + k * 7 + d + T)
    x = r.standard_normal((B, C, T)).astype(np.float32)
    w1 = (r.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32)
    w2 = (r.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32)
    b1, b2 = r.standard_normal(C).astype(np.float32), r.standard_normal(C).astype(np.float32)
    acc = r.standard_normal((B, C, T)).astype(np.float32)
    return x, w1, b1, w2, b2, acc
