"""Reference and bound for the three arithmetics whose operands are EXACT fp32 numbers -- the fp32 MFMA engine (VS_MATH_F32: conv_mfma_kernel, respair_kernel),
its minimal-filtering variant (F(2,3): conv_wino_kernel), the split-bf16 x6 engine (VS_MATH_SPLIT6: conv_split_kernel<..., 6>, respair_split_kernel<..., 6, false>)
and the VALU conv for C_out <= 4 (conv_small_kernel) -- element by element: |got - ref| <= F * 2^-24 * S over ALL elements, S = the sum of the absolute terms.
No tile scale enters any of them, so there is nothing to pin (split3_reference.pin_scale) and the references are short.

Direct fp32 (`math="f32"`, also conv_small_kernel).  ref = the fp64 conv of the fp32 operands (the activation after its input transform, the weight after
ops.weightnorm_fold where weight norm is used), S = conv(|x|, |w|) + |bias|: split3_reference.expected_pre(rounded=False).

Split-bf16 x6 (`math="split6"`).  conv_common.h split_pair<3>: an fp32 number v becomes three bf16 planes by TRUNCATION to the top 16 bits, h = top(v),
m = top(v - h), l = top(v - h - m), every remainder exact, and h + m + l == v bit for bit (24 significant bits in 3 x 8; `split_bf16x3` asserts it for every
operand it is given).  Of the nine plane products conv_split_body.inc keeps six -- mm(weight plane, activation plane) = (1,1) (2,0) (0,2) (1,0) (0,1) (0,0),
smallest first -- each exact in fp32 on v_mfma_f32_32x32x16_bf16.  ref = the fp64 sum of exactly those six (three fp64 convs: x_h with w, x_m with w_h + w_m,
x_l with w_h), so the three dropped products (1,2) (2,1) (2,2) belong to the reference and not to the error budget.  Their size: |m| < 2^-7 |v|,
|l| < 2^-15 |v|, so per product |w_m x_l| + |w_l x_m| + |w_l x_l| < (2 * 2^-7 * 2^-15 + 2^-30) |w x| = (8 + 2^-6) * 2^-24 |w x| (C_SPLIT6); `split6_distance`
prints what it is on a case's data (0.1 .. 0.5 * 2^-24 * S on the tables below).

F(2,3) (`math="wino"`).  conv_wino_kernel cuts the taps into groups of three; for a pair of outputs (y[t], y[t + d]) and group g, with x_j = x[t + (3 g + j) d - pad]:
  V0 = x0 - x2, V1 = x1 + x2, V2 = x2 - x1, V3 = x1 - x3          (wino_half_step<DIL, 3>, fp32)
  U0 = w0, U1 = 0.5f * ((w0 + w1) + w2), U2 = 0.5f * ((w0 - w1) + w2), U3 = w2     (pack_wino_kernel, fp32, taps beyond k are zeros)
  M_xi = sum over input channels and groups of U_xi V_xi;  y[t] = M0 + M1 + M2 + bias,  y[t + d] = M1 - M2 - M3 + bias.
The k-specialised handles take the LAST group in a shorter form (pack_wino_kernel's wino_tail1 branches / wino_half_step<DIL, 2 | 1>): two taps as F(2,2) --
U = (w0, w0 + w1, -, w1), V = (x0 - x1, x1, -, x1 - x2); one tap in the direct form -- U = (w0, -, -, -w0), V = (x0, -, -, x1).  Which form a handle takes is
vs_conv_create's rule (`wino_form`): with MT = ceil(C_out / 32) row tiles, k = 7 on an even MT -> one-tap tail (wino_k7); k = 11 on an even MT, or at dilation 1 on
any MT -> two-tap tail (wino_k11); everything else (k = 3, 5, 9; k = 7 / 11 on the remaining tile counts) the generic zero-padded F(2,3) group.  Which outputs
are the FIRST of their pair is the kernel's column map t(c) = (c / d) 2d + c % d inside a wave's 2 * (64 / d) * d outputs (`wino_first`).  ref = the fp64
M_xi sums of the fp32 U and V, combined as above; S_w = the same sums of |U| |V|, + |bias|.  With fp64 transforms the same code IS the direct conv
(tests/test_exact_reference_cpu.py holds it to 1e-12); with the fp32 transforms it sits 0.1 .. 0.5 * 2^-24 * S from it.

The pair kernels (respair_kernel, respair_split_kernel<..., 6, false>): y = (conv2(lrelu(conv1(lrelu(x)) + b1)) + b2 + x [+ acc]) * scale.  The intermediate is the
device's own fp32 tensor and cannot be reproduced, so ref is the fp64 chain and the bound is propagated (`pair_expected`):
  delta1 = (F + 1) * 2^-24 * S1 on the intermediate (F: conv1's accumulation against its reference -- for split6 the six kept products of conv1, whose operands
           are exact; + 1: the one more fp32 rounding on its way, the leaky-relu's multiply);
  bound  = (conv(|w2|, delta1) + (F + c) * 2^-24 * S2 + 2^-24 * |ref| / scale) * scale,   S2 = conv(|lrelu(t_ref)|, |w2|) + |b2| + |x| + |acc|,
  c = 0 for fp32; for split6 c = C_SPLIT6 = 8 + 2^-6, the dropped products of conv2 derived above (its activation operand, the device's intermediate, is not
  available to take them into the reference).

Behind tanh (`bound_of`): with delta = F * 2^-24 * S on the pre-activation, |tanh(a + e) - tanh(a)| <= (1 - tanh(a)^2) |e| + e^2 (|tanh''| < 1), + 1e-7 for the
device's tanh (conv_common.h tanh_fast, as tests/test_conv_split3_oracle_gpu.py::test_paired_kinds states it; conv_small_kernel's tanhf is closer) + 2^-24 |ref|.
Behind relu the bound is delta (1-Lipschitz); under an output mask it is multiplied by the mask: a masked output must be exactly zero.

The constants F are not taken from the kernels.  Each is the error of the reference's OWN expression summed in serial fp32 chains -- the oracle's
dtype = float32 conv, for a given term count the order with the most sequential roundings (the devices sum in MFMA blocks of 2 .. 16) -- against the fp64 sum, in
units of 2^-24 * S (S_w for F(2,3), a chain per M_xi; for split6 a chain per kept product, the six added smallest first, as split3_reference.serial_fp32 adds
its three), the largest over every distinct shape of the tables below, rounded up to the next power of two.  The chains START FROM THE BIAS, as the oracle's
float32 conv does when it is handed one and as every accumulator of these kernels does (conv_mfma_kernel, conv_split_body.inc for TERMS != 3: "accumulators
start from the bias"; conv_wino_kernel: M0 from the bias, M3 from its negative): every later rounding is then taken at |bias + partial sum| and not at
|partial sum|, which on rows with a large bias doubles the figure (without the bias in the chain the three maxima are 6.91 / 3.25 / 5.19; a first version of
this module measured those and the device exceeded them on exactly such rows).
Measured on the CPU (tests/test_exact_reference_cpu.py recomputes them):
  direct   SERIAL_MEASURED["f32"]    = 11.71 over 90 shapes  (1.13 .. 11.71, median 5.8)  -> F_DIRECT = 16
  F(2,3)   SERIAL_MEASURED["wino"]   = 6.78  over 144 shapes (1.37 .. 6.78, median 4.3)   -> F_WINO = 8
  split6   SERIAL_MEASURED["split6"] = 8.40  over 100 shapes (0.87 .. 8.40, median 3.7)   -> F_SPLIT6 = 16
The one case whose DATA is not standard normal is held apart (GAIN_CASE: per-channel gains of 2^-6 .. 2^6 and outlier runs of 2^9 .. 2^12).  Where one term
carries most of S the partial sum sits at S from that term on and every later rounding counts in full, so the same chains give 20.76 there
(SERIAL_MEASURED["split6_gain"]) -> F_SPLIT6_GAIN = 32.  Folding that case into F_SPLIT6 would double the bound of every other split6 case -- one dropped
2^-16-order product on a wave's 32 x 32 region is 33 .. 104 units at its worst element -- so it keeps a constant of its own, measured the same way.  What the
case shows is unchanged: no term for a scale enters its bound (compare the (12 + 16) * 2^-24 * S + floor of split3_reference's moving-scale group).

Measured on an MI355X, the largest |got - ref| / (2^-24 * S) the comparisons of tests/test_conv_exact_oracle_gpu.py printed, by instance family:
conv_mfma_kernel<1, ...> 8.40 / 8.50 / 14.67 / 7.73 (128 x 256, 64 x 512, 64 x 256, 32 x 512; the worst at 200 -> 170, k = 4, T = 261 behind lrelu, on rows with a
large bias), its transposed launch 10.00, of F_DIRECT = 16; conv_wino_kernel: 2.75 .. 5.76 over the 22 instances (the worst <1, 2, 2, 3, 1>, k = 7, T = 260), of
F_WINO = 8; conv_split_kernel<1, ..., 6> 15.04* / 11.53 / 9.39 / 8.03 (the same tiles as split3_reference; *: the gain case, of its 32; 7.77 on the tile table),
transposed 15.51 (512 -> 256, k = 16: 1024 products per output per kept plane product) / 8.52 / 4.59, of F_SPLIT6 = 16; conv_small_kernel 3.98 (40 -> 4, T = 900),
2.94 on conv_post, of F_DIRECT; the paired kinds at most 0.33 (fp32) / 0.28 (split6) of their propagated bounds; respair_kernel 0.11, respair_split_kernel<...,
6, false> 0.09 of theirs.  The two figures near their constant, 14.67 and 15.51, are reductions of 800 and 1024 terms on rows whose bias is 2 .. 3 times the
conv's own standard deviation: the bias-first chain above reaches 11.7 on the first of them.

Plain helper module (like split3_reference.py): no fixtures, no tests; imports nothing from the package.  finish, in_transform, ragged_mask, to_np are
bf16_reference's; figures / assert_close split3_reference's (lines tagged EXACTREF)."""
import numpy as np

import split3_reference as S3
from bf16_reference import PAIR_CASES, finish, in_transform, pair_inputs, ragged_mask, to_np  # noqa: F401  (re-exported: one definition for all checkers)
from split3_reference import EPS32, IN_LRELU, IN_LRELU_MASK, IN_MASK, IN_NONE, TOL, TR_SHAPES, figures, tile_variants  # noqa: F401

B = S3.B
SERIAL_MEASURED = {"f32": 11.71, "wino": 6.78, "split6": 8.40, "split6_gain": 20.76}      # the largest serial-chain figure per family over the table shapes (module docstring)
F_DIRECT, F_WINO, F_SPLIT6, F_SPLIT6_GAIN = 16.0, 8.0, 16.0, 32.0      # ... rounded up to a power of two
F_OF = {"f32": F_DIRECT, "wino": F_WINO, "split6": F_SPLIT6}
C_SPLIT6 = 8.0 + 2.0 ** -6                                        # the three dropped plane products, in units of 2^-24 |w x| (module docstring)
KEPT6 = [(1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0)]          # conv_split_body.inc mm(weight plane, activation plane), in its order
TANH_ABS = 1e-7


def assert_close(got, ref, S, what="", *, bound=None, F=None):
    """split3_reference.assert_close, printing `EXACTREF <what>: per_S .. scaled ..`; F or bound must be given"""
    assert (bound is None) != (F is None)
    return S3.assert_close(got, ref, S, what, bound=bound, F=F, tag="EXACTREF")


def flagged(got, ref, bound):
    """the elements assert_close(bound=...) would flag"""
    return np.abs(to_np(got) - ref) > bound


def old_flagged(got, exact):
    """the elements 2e-5 * (1 + |ref|) against the plain fp64 result flags (the bound of tests/test_conv_gpu.py)"""
    return np.abs(to_np(got) - exact) > TOL * (1.0 + np.abs(exact))


# ---------------------------------------------------------------------------------------------------------------- split-bf16 x6, restated
def _top16(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split_bf16x3(v, check=True):
    """conv_common.h split_pair<3>: -> (h, m, l) float32, each a bf16 number (low 16 bits zero): truncation, remainders exact.
    check: assert h + m + l == v bit for bit (false only where a plane would be subnormal: the device's planes may then flush)"""
    v = np.ascontiguousarray(v, np.float32)
    h = _top16(v)
    r = v - h
    m = _top16(r)
    r2 = r - m
    l = _top16(r2)
    if check:
        s = h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64)
        assert np.array_equal(s, v.astype(np.float64)), "h + m + l != v"      # (fp64 holds the sum exactly: equal values are equal bits, -0 aside)
    return h, m, l


def _conv(oracle, x, w, transposed, dil_or_stride, padding, dtype=np.float64):
    return S3._conv(oracle, x, w, transposed, dil_or_stride, padding, dtype)


def planes6(oracle, x, w, *, lrelu=False, in_mask=None):
    """-> (xt, w32, (x_h, x_m, x_l), (w_h, w_m, w_l)): the transformed fp32 input, the fp32 weight and their planes (float32)"""
    xt = in_transform(oracle, x, lrelu, in_mask)
    w32 = np.ascontiguousarray(to_np(w), np.float32)
    return xt, w32, split_bf16x3(xt), split_bf16x3(w32)


def _six(oracle, xp, wp, transposed, dil_or_stride, padding):
    """the fp64 sum of the six kept plane products: x_h (w_h + w_m + w_l) + x_m (w_h + w_m) + x_l w_h"""
    d = lambda a: a.astype(np.float64)
    c = lambda a, b: _conv(oracle, a, b, transposed, dil_or_stride, padding)
    return c(d(xp[0]), d(wp[0]) + d(wp[1]) + d(wp[2])) + c(d(xp[1]), d(wp[0]) + d(wp[1])) + c(d(xp[2]), d(wp[0]))


def _six_serial(oracle, xp, wp, bias, transposed, dil_or_stride, padding):
    """the same expression with fp32 sums, as split3_reference.serial_fp32 takes its three: each kept product's terms in one serial fp32 chain (the oracle's
    float32 conv), the six chains added in the kernel's order, smallest first -- the last and largest, h h, starting from the bias as the kernel's accumulator does"""
    f = np.float32
    acc = None
    for ta, tb in KEPT6:
        b = None if (bias is None or (ta, tb) != (0, 0)) else np.asarray(bias, f)
        if transposed:
            t = oracle.conv_transpose1d(xp[tb], wp[ta], b, stride=dil_or_stride, padding=padding, dtype=f)
        else:
            t = oracle.conv1d(xp[tb], wp[ta], b, dilation=dil_or_stride, padding=padding, dtype=f)
        acc = t if acc is None else acc + t
    assert acc.dtype == f
    return acc


# ---------------------------------------------------------------------------------------------------------------- F(2,3), restated
def wino_form(Cout, k, dil):
    """vs_conv_create's wino_groups / wino_k7 / wino_k11 -> (groups, taps of the last group in the form the handle takes: 1, 2, or 3 = zero-padded F(2,3))"""
    MT, G = -(-Cout // 32), -(-k // 3)
    k7 = G == 3 and k == 7 and MT % 2 == 0
    k11 = G == 4 and k == 11 and (MT % 2 == 0 or dil == 1)
    return G, (k - 3 * (G - 1)) if (k7 or k11) else 3


def wino_instance(Cout, k, dil):
    """launch_wino_dil: the instance a (C_out, k, dilation) handle reaches"""
    MT = -(-Cout // 32)
    wm, wn = (4, 1) if MT % 4 == 0 else ((2, 2) if MT % 2 == 0 else (1, 4))
    tg, tt = {1: (3, 1), 2: (4, 2), 3: (0, 3)}[wino_form(Cout, k, dil)[1]]
    return "conv_wino_kernel<%d, %d, %d, %d, %d>" % (dil, wm, wn, tg, tt)


def wino_block(Cout, dil):
    """outputs per workgroup along the sequence: 2 * (64 / d) * d per wave, WAVES_N waves side by side"""
    MT = -(-Cout // 32)
    return 2 * (64 // dil) * dil * (1 if MT % 4 == 0 else (2 if MT % 2 == 0 else 4))


def wino_first(T, dil):
    """[T] bool: output t is the first of its pair (y[t] = M0 + M1 + M2 at base t); otherwise y[t] = M1 - M2 - M3 at base t - d"""
    t = np.arange(T) % (2 * (64 // dil) * dil)
    return (t % (2 * dil)) < dil


def wino_U(w, tail, dtype=np.float32):
    """pack_wino_kernel: -> [4] arrays [C_out, C_in, G], in `dtype` with its operation order"""
    f = np.dtype(dtype).type
    Cout, Cin, k = w.shape
    G = -(-k // 3)
    wz = np.zeros((Cout, Cin, 3 * G), dtype)
    wz[:, :, :k] = w
    w0, w1, w2 = wz[:, :, 0::3], wz[:, :, 1::3], wz[:, :, 2::3]
    U = [w0.copy(), f(0.5) * ((w0 + w1) + w2), f(0.5) * ((w0 - w1) + w2), w2.copy()]
    g = G - 1
    if tail == 1:
        U[0][:, :, g], U[1][:, :, g], U[2][:, :, g], U[3][:, :, g] = w0[:, :, g], 0, 0, -w0[:, :, g]
    elif tail == 2:
        U[0][:, :, g], U[1][:, :, g], U[2][:, :, g], U[3][:, :, g] = w0[:, :, g], w0[:, :, g] + w1[:, :, g], 0, w1[:, :, g]
    return U


def wino_V(xt, k, dil, tail, dtype=np.float32):
    """wino_half_step<DIL, TAPS>: -> [4] arrays [B, C_in, G, T]: V_xi of group g at pair base t, from the transformed input, in `dtype`"""
    Bn, Cin, T = xt.shape
    G, pad = -(-k // 3), dil * (k - 1) // 2
    xp = np.zeros((Bn, Cin, T + 3 * G * dil), dtype)
    xp[:, :, pad:pad + T] = xt
    V = [np.zeros((Bn, Cin, G, T), dtype) for _ in range(4)]
    for g in range(G):
        x0, x1, x2, x3 = (xp[:, :, (3 * g + j) * dil:(3 * g + j) * dil + T] for j in range(4))
        taps = tail if g == G - 1 else 3
        if taps == 3:
            V[0][:, :, g], V[1][:, :, g], V[2][:, :, g], V[3][:, :, g] = x0 - x2, x1 + x2, x2 - x1, x1 - x3
        elif taps == 2:
            V[0][:, :, g], V[1][:, :, g], V[3][:, :, g] = x0 - x1, x1, x1 - x2
        else:
            V[0][:, :, g], V[3][:, :, g] = x0, x1
    return V


def _wino_sums(oracle, U, V, dtype, bias=None):
    """M_xi[b, o, t] = sum over (c, g) of U_xi[o, c, g] V_xi[b, c, g, t]: fp64 -- a matrix product; fp32 -- the oracle's serial chain (a 1-tap conv), M0 starting
    from the bias and M3 from its negative as the kernel's accumulators do"""
    out = []
    for xi, (u, v) in enumerate(zip(U, V)):
        Bn, Cin, G, T = v.shape
        u2, v2 = u.reshape(u.shape[0], Cin * G), v.reshape(Bn, Cin * G, T)
        if np.dtype(dtype) == np.float32:
            b = None if (bias is None or xi in (1, 2)) else np.asarray(bias if xi == 0 else -bias, np.float32)
            out.append(oracle.conv1d(v2.astype(np.float32), u2.astype(np.float32)[:, :, None], b, dtype=np.float32))
        else:
            out.append(np.matmul(u2.astype(np.float64)[None], v2.astype(np.float64)))
    return out


def wino_combine(M, bias_terms, first, dil):
    """y[t] = M0 + M1 + M2 + bias where t is the first of its pair, M1 - M2 - M3 + bias taken at base t - d otherwise; in the dtype of M"""
    y0 = M[0] + M[1] + M[2]
    y1 = M[1] - M[2] - M[3]
    y = np.where(first[None, None, :], y0, np.roll(y1, dil, axis=2))       # (a second output has t >= d: the roll never wraps into one)
    for b_ in bias_terms:
        y = y + b_.astype(y.dtype)
    return y


def wino_pre(oracle, xt, w32, bias_terms, dil, *, transform=np.float32, dtype=np.float64, tail=None, chain_bias=None):
    """-> (pre, S_w) of the F(2,3) form the handle takes (tail: override of wino_form's; chain_bias: dtype = float32 -- the per-row bias the chains start from,
    then not among bias_terms)"""
    Cout, _, k = w32.shape
    T = xt.shape[2]
    tail = wino_form(Cout, k, dil)[1] if tail is None else tail
    U, V = wino_U(w32.astype(transform), tail, transform), wino_V(xt.astype(transform), k, dil, tail, transform)
    first = wino_first(T, dil)
    pre = wino_combine(_wino_sums(oracle, U, V, dtype, chain_bias), bias_terms, first, dil).astype(np.float64)
    A = _wino_sums(oracle, [np.abs(u) for u in U], [np.abs(v) for v in V], np.float64)
    S = np.where(first[None, None, :], A[0] + A[1] + A[2], np.roll(A[1] + A[2] + A[3], dil, axis=2))
    for b_ in bias_terms + ([] if chain_bias is None else [to_np(chain_bias)[None, :, None]]):
        S = S + np.abs(b_)
    return pre, S


# ---------------------------------------------------------------------------------------------------------------- references
def expected_pre(oracle, math, x, w, bias=None, *, transposed=False, dil_or_stride=1, padding=0, lrelu=False, in_mask=None, bias_b=None, dtype=np.float64):
    """-> (pre, S) of one conv in arithmetic `math` ("f32" / "split6" / "wino"), before the epilogue.  w: the fp32 EFFECTIVE weight.  dtype = np.float32: the
    reference's own expression in serial fp32 chains that START FROM THE BIAS, as the oracle's float32 conv does when it is given one and as these kernels'
    accumulators do (what the constants F are measured on; a per-item bias is added behind the chain)"""
    serial = np.dtype(dtype) == np.float32
    bt = lambda b_, sh: [] if b_ is None else [to_np(b_)[sh]]
    bias_terms = ([] if serial else bt(bias, (None, slice(None), None))) + bt(bias_b, (slice(None), slice(None), None))
    chain_bias = bias if serial else None
    xt, w32 = in_transform(oracle, x, lrelu, in_mask), np.ascontiguousarray(to_np(w), np.float32)
    if math == "wino":
        assert not transposed and padding == dil_or_stride * (w32.shape[2] - 1) // 2
        return wino_pre(oracle, xt, w32, bias_terms, dil_or_stride, dtype=dtype, chain_bias=None if chain_bias is None else to_np(chain_bias))
    if math == "f32":
        if serial:
            b = None if chain_bias is None else np.asarray(to_np(chain_bias), np.float32)
            pre = (oracle.conv_transpose1d(xt, w32, b, stride=dil_or_stride, padding=padding, dtype=np.float32) if transposed else
                   oracle.conv1d(xt, w32, b, dilation=dil_or_stride, padding=padding, dtype=np.float32))
        else:
            pre = _conv(oracle, xt, w32, transposed, dil_or_stride, padding)
    else:
        assert math == "split6", math
        xp, wp = split_bf16x3(xt), split_bf16x3(w32)
        pre = (_six_serial(oracle, xp, wp, chain_bias if chain_bias is None else to_np(chain_bias), transposed, dil_or_stride, padding) if serial else
               _six(oracle, xp, wp, transposed, dil_or_stride, padding))
    for b_ in bias_terms:
        pre = pre + b_.astype(pre.dtype)
    S = _conv(oracle, np.abs(xt), np.abs(w32), transposed, dil_or_stride, padding)      # (as split3_reference.expected_pre(rounded=False) takes it)
    for b_ in bias_terms + ([] if chain_bias is None else [to_np(chain_bias)[None, :, None]]):
        S = S + np.abs(b_)
    return pre.astype(np.float64), S


def split6_distance(oracle, x, w, **conv):
    """how far the six kept products sit from the plain fp64 conv, worst element, in units of 2^-24 * S (derived: below C_SPLIT6)"""
    kw = {k: v for k, v in conv.items() if k in ("transposed", "dil_or_stride", "padding", "lrelu", "in_mask")}
    six, S = expected_pre(oracle, "split6", x, w, None, **kw)
    plain, _ = expected_pre(oracle, "f32", x, w, None, **kw)
    return figures(six, plain, S)[1]


def bound_of(F, ref, S, out_act=None, out_mask=None, scale=1.0):
    """the element-wise bound behind the epilogue `finish` applied (S as finish returns it: under the scale).  (module docstring)"""
    delta = F * EPS32 * S
    if out_act == "tanh":
        delta = (1.0 - ref * ref) * delta + delta * delta + TANH_ABS + EPS32 * np.abs(ref)
    else:
        assert out_act in (None, "relu"), out_act
    if out_mask is not None:
        delta = delta * np.asarray(out_mask, np.float64)[:, None]
    return delta


def expected(oracle, math, x, w, bias=None, *, res=None, acc=None, scale=1.0, out_act=None, out_mask=None, F=None, **conv):
    """expected_pre + bf16_reference.finish + bound_of.  -> (ref, S, bound)"""
    pre, S = expected_pre(oracle, math, x, w, bias, **conv)
    ref, S = finish(pre, S, res=res, acc=acc, scale=scale, out_act=out_act, out_mask=out_mask)
    return ref, S, bound_of(F_OF[math] if F is None else F, ref, S, out_act, out_mask)


def serial_figure(oracle, math, x, w, bias, ref_S=None, **conv):
    """worst |serial fp32 chains - fp64 sums| / (2^-24 S) of one case"""
    ref, S = ref_S if ref_S is not None else expected_pre(oracle, math, x, w, bias, **conv)
    ser, _ = expected_pre(oracle, math, x, w, bias, dtype=np.float32, **conv)
    return figures(ser, ref, S)[1]


def pair_expected(oracle, math, x, w1, b1, w2, b2, *, k, d, res=None, acc=None, scale=1.0, F=None):
    """the fused residual pair in arithmetic "f32" / "split6" (module docstring).  -> (ref, bound, t_ref)"""
    F = F_OF[math] if F is None else F
    c = C_SPLIT6 if math == "split6" else 0.0
    pad1, pad2 = d * (k - 1) // 2, (k - 1) // 2
    t, S1 = expected_pre(oracle, math, x, w1, b1, dil_or_stride=d, padding=pad1, lrelu=True)
    slope = float(np.float32(oracle.LRELU_SLOPE))
    a = np.where(t >= 0, t, t * slope)
    w2d = np.ascontiguousarray(to_np(w2), np.float64)
    y = oracle.conv1d(a, w2d, to_np(b2), padding=pad2)
    S2 = oracle.conv1d(np.abs(a), np.abs(w2d), np.abs(to_np(b2)), padding=pad2)
    delta1 = (F + 1.0) * EPS32 * S1
    carried = oracle.conv1d(delta1, np.abs(w2d), None, padding=pad2)
    ref, S2 = finish(y, S2, res=res, acc=acc, scale=scale)
    s = abs(float(np.float32(scale)))
    bound = carried * s + (F + c) * EPS32 * S2 + EPS32 * np.abs(ref)
    return ref, bound, t


# ---------------------------------------------------------------------------------------------------------------- device-like fp32 accumulations (the self-test's "device")
def as_conv1d(planes_x, planes_w, transposed, dil_or_stride, padding):
    """a transposed conv as the plain conv the emulation takes: zero-stuffed activation planes, channel-transposed tap-reversed weight planes, padding k - 1 - p"""
    if not transposed:
        return planes_x, planes_w, dil_or_stride, padding
    u, k = dil_or_stride, planes_w[0].shape[2]

    def stuff(a):
        o = np.zeros(a.shape[:2] + ((a.shape[2] - 1) * u + 1,), a.dtype)
        o[:, :, ::u] = a
        return o

    flip = lambda a: np.ascontiguousarray(a.transpose(1, 0, 2)[:, :, ::-1])
    return [stuff(a) for a in planes_x], [flip(a) for a in planes_w], 1, k - 1 - padding


def blocked_fp32(xp, wp, kept, bias, *, dilation=1, padding=0, defect=None):
    """per 16-channel chunk and tap the `kept` plane products (weight plane, activation plane), each a 16-term fp32 block sum, onto an fp32 accumulator (chunk
    outer, tap inner: conv_split_body.inc; one plane and kept = [(0, 0)]: the fp32 MFMA engine), which starts from the bias.  plain conv1d on [B, C, T] planes.  defect: None or
      ("drop", (ta, tb), chunk | None, tap | None [, region]) -- that product is not taken: in that step (None: every chunk / tap), everywhere or on the index
                                                                 expression `region` of [B, C_out, T_out] only (one wave's 32 x 32 tile);
      ("edge", tap, col)                                      -- output column `col` reads that tap from the neighbouring input column, in every chunk"""
    f = np.float32
    Bn, C, T = xp[0].shape
    Cout, _, K = wp[0].shape
    Tout = T + 2 * padding - dilation * (K - 1)
    pad = ((0, 0), (0, 0), (padding, padding + 1))
    xp, wp = [np.pad(a.astype(f), pad) for a in xp], [a.astype(f) for a in wp]
    acc = np.zeros((Bn, Cout, Tout), f) + (0 if bias is None else np.asarray(bias, f)[None, :, None])      # (the accumulators start from the bias)
    for c, c0 in enumerate(range(0, C, 16)):
        cs = slice(c0, c0 + 16)
        for k in range(K):
            ts = slice(k * dilation, k * dilation + Tout)
            for ta, tb in kept:
                region = None
                if defect and defect[0] == "drop" and defect[1] == (ta, tb) and defect[2] in (None, c) and defect[3] in (None, k):
                    if len(defect) == 4:
                        continue
                    region = defect[4]
                xs = np.ascontiguousarray(xp[tb][:, cs, ts])
                if defect and defect[0] == "edge" and defect[1] == k:
                    xs[:, :, defect[2]] = xp[tb][:, cs, k * dilation + defect[2] + 1]
                wk = np.ascontiguousarray(wp[ta][:, cs, k])
                prod = np.stack([wk @ xs[b] for b in range(Bn)])
                if region is not None:
                    prod[region] = 0
                acc += prod
    assert acc.dtype == f
    return acc


def blocked_wino(U, V, bias, first, dil, defect=None):
    """the F(2,3) accumulation: per 16-channel chunk and tap group, U_xi V_xi as fp32 block sums onto four fp32 accumulators M_xi, combined in fp32.
    defect: None, ("u3_sign",) -- the last group's U3 with the wrong sign (the one-tap tail not negated), or ("last_group", t) -- the last tap group contributes
    nothing at pair base t"""
    f = np.float32
    Bn, C, G, T = V[0].shape
    U, V = [u.astype(f) for u in U], [v.astype(f).copy() for v in V]
    if defect and defect[0] == "u3_sign":
        U[3][:, :, G - 1] = -U[3][:, :, G - 1]
    if defect and defect[0] == "last_group":
        for v in V:
            v[:, :, G - 1, defect[1]] = 0
    M = [np.zeros((Bn, U[0].shape[0], T), f) for _ in range(4)]
    if bias is not None:                                       # (M0 starts from the row's bias and M3 from its negative: y[t + d] = M1 - M2 - M3)
        M[0] += np.asarray(bias, f)[None, :, None]
        M[3] -= np.asarray(bias, f)[None, :, None]
    for c0 in range(0, C, 16):
        cs = slice(c0, c0 + 16)
        for g in range(G):
            for xi in range(4):
                uk = np.ascontiguousarray(U[xi][:, cs, g])
                M[xi] += np.stack([uk @ np.ascontiguousarray(V[xi][b, cs, g]) for b in range(Bn)])
    y = wino_combine(M, [], first, dil)
    assert y.dtype == f
    return y


# ---------------------------------------------------------------------------------------------------------------- the shapes, shared by the GPU test and the CPU self-test
# conv_mfma_kernel<1, NT_W, WAVES_M, WAVES_N>: (tile, C_in, C_out, T, k, dilation).  The tile follows the 32-row tile count (5 -> 128 x 256, 2 -> 64 x 512, 6 on a
# short launch -> 64 x 256, 1 -> 32 x 512) or VS_CONV_CFG; C_in off the 16-channel chunk (33, 200, 40), C_out off the 32-row tile (136, 50, 170, 20), T one past a column
# tile (257 / 513), T in {1, 2, 5} with halos wider than the sequence
MFMA_CASES = [
    ("128x256", 33, 136, 257, 5, 2), ("128x256", 200, 136, 261, 1, 1), ("128x256", 40, 136, 5, 5, 3), ("128x256", 16, 136, 2, 4, 1), ("128x256", 33, 136, 1, 5, 1),
    ("64x512", 33, 50, 513, 5, 3), ("64x512", 200, 50, 129, 4, 1), ("64x512", 16, 50, 1, 5, 2), ("64x512", 40, 50, 5, 5, 5), ("64x512_cfg", 40, 136, 517, 1, 1),
    ("64x256", 33, 170, 257, 5, 2), ("64x256", 200, 170, 261, 4, 1), ("64x256", 48, 170, 2, 5, 5), ("64x256", 16, 170, 5, 1, 1), ("64x256_cfg", 40, 136, 257, 5, 4),
    ("32x512", 33, 20, 513, 5, 3), ("32x512", 200, 20, 261, 1, 1), ("32x512", 64, 20, 257, 4, 1), ("32x512", 16, 20, 1, 5, 1), ("32x512", 40, 20, 5, 5, 2),
    ("32x512_cfg", 33, 70, 129, 5, 1),
]
PAIR_TILES = [p for p in S3.PAIR_TILES if p[5] != "ktap_pair"]      # (H, C_in, T, k, d, id): the paired kinds <2, 2, 2, 2> (two shapes) and <2, 2, 1, 4>
FUSED_CASE = (64, 64, 333, 7, 3)                                     # weight norm + residual + accumulate + scale, in place; tanh output
RELU_CASE = (48, 96, 211, 9, 1)                                      # relu + output mask + per-item bias
ADJ_CASE = (48, 96, 129, 5, 1)                                       # the grad-input conv of a 96 -> 48 conv
TR_F32 = TR_SHAPES[2]                                                # (48, 24, 11, 5, 33): the fp32 engine's transposed launch

# conv_wino_kernel<D, WM, WN, TG, TT> under VS_WINO_FORCE: (C_in, C_out, k, dilation) -- all 22 instances (WINO_INSTANCES) and the two handles that fall back to the
# generic zero-padded form on an odd tile count (k = 7 at 96 rows, k = 11 at 32 rows and dilation 3)
WINO_CASES = [
    (24, 128, 3, 1), (33, 64, 5, 1), (48, 32, 9, 1), (33, 128, 5, 3), (24, 64, 9, 3), (40, 96, 3, 3), (24, 128, 9, 5), (40, 64, 3, 5), (33, 32, 5, 5),
    (33, 128, 7, 1), (24, 64, 7, 1), (24, 128, 7, 3), (40, 64, 7, 3), (40, 128, 7, 5), (33, 64, 7, 5),
    (40, 128, 11, 1), (33, 64, 11, 1), (33, 128, 11, 3), (24, 64, 11, 3), (24, 128, 11, 5), (40, 64, 11, 5), (24, 96, 11, 1),
    (33, 96, 7, 3), (24, 32, 11, 3),
]
WINO_INSTANCES = sorted({"conv_wino_kernel<%d, %s, %s>" % (d, t, f) for d in (1, 3, 5) for t in ("4, 1", "2, 2") for f in ("0, 3", "3, 1", "4, 2")} |
                        {"conv_wino_kernel<%d, 1, 4, 0, 3>" % d for d in (1, 3, 5)} | {"conv_wino_kernel<1, 1, 4, 4, 2>"})
assert len(WINO_INSTANCES) == 22 and {wino_instance(c[1], c[2], c[3]) for c in WINO_CASES} == set(WINO_INSTANCES)


def wino_launches(Cout, k, dil):
    """the launches of one F(2,3) case: (T, in_act, res, acc, scale, out_act, out_mask) -- a T one block plus a remainder off the float4 grid (element-wise
    epilogue everywhere), a T on it (vector epilogue in the whole blocks: plain, residual only, everything), a T shorter than the receptive span"""
    bn = wino_block(Cout, dil)
    t_el, t_vec, t_short = bn + 5, (bn + 7) // 4 * 4, min(5, dil * (k - 1))
    assert t_el % 4 and t_vec % 4 == 0 and t_vec >= bn + 4 and t_short < dil * (k - 1) + 1
    return [(t_el, IN_LRELU, True, True, 1.0 / 3.0, None, False), (t_el, IN_LRELU_MASK, True, False, 1.0, "tanh", True),
            (t_vec, IN_LRELU, False, False, 1.0, None, False), (t_vec, IN_NONE, True, False, 1.0, None, False),
            (t_vec, IN_LRELU_MASK, True, True, 1.0 / 3.0, "tanh", True), (t_short, IN_LRELU_MASK, False, False, 1.0, "tanh", True)]


# conv_small_kernel: (C_in, C_out, T, k, in_act, out_act) -- conv_post (32 -> 1, k = 7, tanh; T % 4 == 0: the <1, 7, 3> window instance), C_out in {2, 4} behind
# mask and leaky-relu, T in {1, 7, 900}
SMALL_CASES = [(32, 1, 900, 7, IN_LRELU, "tanh"), (32, 1, 7, 7, IN_LRELU, "tanh"), (32, 1, 1, 7, IN_LRELU, "tanh"),
               (192, 2, 900, 1, IN_MASK, None), (192, 2, 7, 3, IN_MASK, None), (40, 4, 900, 3, IN_LRELU_MASK, None), (40, 4, 1, 3, IN_LRELU, None), (33, 4, 7, 5, IN_LRELU_MASK, None)]

GAIN_CASE = (64, 96, 600, 7, 1)                                      # split6 under per-channel gains of 2^-6 .. 2^6 and outlier runs


def conv_inputs(Cin, Cout, T, k, du, in_act, *, tr=False, seed=0):
    """the inputs of one single-conv launch, the same on the GPU and in the self-test: rng, x, w, bias, padding (split3_reference.conv_inputs, nothing pinned)"""
    return S3.conv_inputs(Cin, Cout, T, k, du, in_act, tr=tr, seed=seed, pin=False)


def gain_inputs():
    """GAIN_CASE's inputs: per-channel gains and outlier runs (tests/test_conv_split3_oracle_gpu.py::test_moving_scale).  The planes carry no scale, so the
    bound has no term for one: F_SPLIT6_GAIN * 2^-24 * S (module docstring)"""
    Cin, Cout, T, k, d = GAIN_CASE
    r, x, w, bias, pad = conv_inputs(Cin, Cout, T, k, d, IN_LRELU_MASK)
    x[:, : Cin // 2] *= np.exp2(r.integers(-6, 7, (B, Cin // 2, 1))).astype(np.float32)
    x[0, 3, 100:180] = 2.0 ** 9
    x[0, Cin - 2, 300:340] = -(2.0 ** 12)
    x[1, 20, 10:14] = 2.0 ** 11
    return x, w, bias, pad


def _uniq(out):
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def table_shapes(math):
    """every distinct (transposed, C_in, C_out, T, k, dilation / stride, in_act) the GPU file's tables launch in arithmetic `math`"""
    out = []
    if math == "wino":
        for Cin, Cout, k, d in WINO_CASES:
            out += [(False, Cin, Cout, l[0], k, d, l[1]) for l in wino_launches(Cout, k, d)]
        return _uniq(out)
    tiles = MFMA_CASES if math == "f32" else S3.TILE_CASES
    for _, Cin, Cout, T, k, d in tiles:
        out += [(False, Cin, Cout, T, k, d, a) for a, _, _ in tile_variants(k)]
    for Cin, Cout, k, u, T in ([TR_F32] if math == "f32" else TR_SHAPES):
        out += [(True, Cin, Cout, T, k, u, IN_LRELU), (True, Cin, Cout, T, k, u, IN_LRELU_MASK)][: 1 if math == "f32" else 2]
    out += [(False, Cin, 2 * H, T, k, d, IN_NONE) for H, Cin, T, k, d, _ in PAIR_TILES]
    out += [(False, C, C, T, k, d, IN_LRELU) for C, k, d, T in PAIR_CASES]
    if math == "f32":          # (GAIN_CASE is not a shape of these tables: its data is its own -- gain_inputs, F_SPLIT6_GAIN)
        Cin, Cout, T, k, d = FUSED_CASE
        out.append((False, Cin, Cout, T, k, d, IN_LRELU))
        Cin, Cout, T, k, d = RELU_CASE
        out.append((False, Cin, Cout, T, k, d, IN_MASK))
        Cin, Cout, T, k, d = ADJ_CASE
        out.append((False, Cin, Cout, T, k, d, IN_NONE))
        out += [(False, Cin, Cout, T, k, 1, a) for Cin, Cout, T, k, a, _ in SMALL_CASES]
    return _uniq(out)
