"""Reference and bounds for the weight-gradient kernels of the training step (csrc/conv_backward.hip), element by element, built from the device's own
operand planes.

    gw[co, ci, k] = sum_{b, t} gy[b, co, t] * x[b, ci, t + k dil - pad]                      (x = 0 outside [0, T_in))

The arithmetic restated here:
  conv_wgrad_split_kernel<KT, TS>   both operands are split EXACTLY into three bf16 planes (conv_common.h split_pair<3>: a plane is the high 16 bits of the
           fp32 value -- truncation, not rounding --, the subtraction is exact, three times: v = v0 + v1 + v2 with nothing left).  Per 16-position step
           and tap six of the nine plane products go through v_mfma_f32_32x32x16_bf16 -- every product of two bf16 numbers is exact in fp32 -- onto an fp32
           accumulator, smallest first: (g1, x1) (g2, x0) (g0, x2) (g1, x0) (g0, x1) (g0, x0): the pairs (i, j) with i + j <= 2.  A symmetric set: the role
           swap of the transposed conv's caller (autograd.conv_backward: x in the place of gy) keeps it.
  conv_wgrad_kernel                 the fp32 operands as they are on v_mfma_f32_32x32x2_f32.
  wgrad_finish_kernel               every reduction slice leaves a partial plane; the planes are summed in a fixed order.
So against ref = sum_{b, t} of the six kept plane products in fp64 (`expected`: g0 x + g1 (x0 + x1) + g2 x0, three matmuls per tap) only the ORDER of the
fp32 accumulation is left:  |got - ref| <= F * 2^-24 * S,  S = sum_{b, t} |gy| |x|,  over ALL elements; an element with S = 0 (every product in the padding,
or a zero operand) must be exactly 0.  The fp32 kernel's reference is the plain fp64 gradient (rounded=False).

The bounds are not taken from the kernels.
  F_WGRAD, F_WGRAD_F32   the error of the reference's own fp32 accumulation: `serial_fp32` puts every product of one output into ONE serial fp32 chain -- for a
           given term count the order with the most sequential roundings; per 16-position step the six plane products in the kernel's order (the fp32 kernel:
           every product rounded to fp32 first) -- and compares with the fp64 sum in units of 2^-24 * S.  Measured on the CPU over all shapes of the tables
           below (`table_operands`: groups A, B, E, F, the dispatch edge and the callers' layouts of group D; tests/test_wgrad_reference_cpu.py recomputes
           them; shapes of more than 40000 outputs on a regular sub-grid of the channels, `serial_subset`): split arithmetic 6.40 .. 11.15 over 41 shapes
           (SERIAL_F_MEASURED; the worst at group B, k = 7), fp32 2.45 .. 5.74 over 13 (SERIAL_F32_MEASURED; the worst at k = 16, dil = 4); rounded up to a
           power of two F_WGRAD = 16, F_WGRAD_F32 = 8.
  F_BIAS   likewise from a serial fp32 sum of gy over (b, t) against its fp64 sum in units of 2^-24 * sum |gy|: 0.68 .. 2.50 (SERIAL_BIAS_MEASURED), F_BIAS = 4.
  F_IMPULSE = 10, F_IMPULSE_F32 = 4   DERIVED, no measurement: with ONE nonzero position (b, t*) in gy an output has one nonzero product.  Split kernel: six
           exact plane products of one sign (the planes of a truncated split carry the value's sign) added onto a zero accumulator: five additions, each
           result within one fp32 ulp (2 units of 2^-24 of the running sum <= |gy| |x|) whether the matrix unit rounds or truncates: 10.  fp32 kernel: one
           product (one ulp), one addition onto zero: 4.  Every partial plane but one holds zeros, so the finish kernel adds nothing.
The arithmetic's own distance from the plain fp64 gradient (the three dropped products: <= (2^-22 + 2^-22 + 2^-30) |gy| |x|, 8.004 units, per product):
0.11 .. 0.38 * 2^-24 * S on the randn groups, where the signs cancel, 4.2 .. 6.9 on the impulse group -- there the plane reference is required; the fp64 gradient
would eat most of F_IMPULSE.

What seeded defects cost (tests/test_wgrad_reference_cpu.py on `emulate_split`, printed as `WGRADDET ...`): one dropped small cross product is flagged on
every group-A shape but only on 0.15 .. 0.22 of its outputs (median 7.5 .. 8.7 units, worst 40 .. 58, against 16) and on 0.81 .. 1.00 of the outputs of every
impulse case (median 59 .. 140 units against 10): the impulse group is what covers it.  A tap or the odd offsets read one position off, the ragged unit not
zeroed, a unit skipped, a plane left out of the sum, the absent tap stored, bias sums on the wrong rows: >= 0.99 of the outputs they touch.  Planes rounded
to nearest even instead of truncated: not flagged anywhere (the rounded split is exact too; 0.6 .. 1.1 units on group A).

Measured on an MI355X, the largest |got - ref| / (2^-24 * S) of the 161 comparisons tests/test_wgrad_oracle_gpu.py printed (DEVICE_FIGURES; measurements, nothing
is tuned to them): conv_wgrad_split_kernel on randn data 0.89 (group A: <5, 2> at k = 9, dil 8, full padding; <6, 2> 0.89, <4, 2> 0.85, the TS = 1 instances
0.55 .. 0.77), 0.54 with several units per workgroup (group B), 0.79 through the callers (group D), 1.96 on the impulse group (of F_IMPULSE = 10: one
truncation); conv_wgrad_kernel 2.49 (T_out = 258; group E 2.27), impulse 1.00 (of 4); the fused bias sums 0.31 (of F_BIAS = 4).  The matrix unit sums a block
of 16 products far more exactly than a serial chain: no family above 0.16 of its F on randn data, 0.25 on the impulse group.

Plain helper module (like split3_reference.py): no fixtures, no tests, imports nothing of the package.
"""
from collections import namedtuple

import numpy as np

EPS32 = 2.0 ** -24
TOL = 2e-5                        # the bound of the other callers' tests, 2e-5 * (1 + |ref|), printed for comparison
SERIAL_F_MEASURED = 11.15         # split arithmetic: the largest |serial fp32 chain - fp64 sum| / (2^-24 S) over table_operands() (module docstring)
F_WGRAD = 16.0                    # ... rounded up to a power of two
SERIAL_F32_MEASURED = 5.74        # the same for the fp32 kernel's arithmetic against the plain fp64 gradient
F_WGRAD_F32 = 8.0
SERIAL_BIAS_MEASURED = 2.50       # a serial fp32 sum of gy against its fp64 sum, in units of 2^-24 sum |gy|, over table_cases()
F_BIAS = 4.0
F_IMPULSE = 10.0                  # derived (module docstring): five additions of same-sign terms, one ulp each
F_IMPULSE_F32 = 4.0               # one product, one addition

# the largest per_S printed by tests/test_wgrad_oracle_gpu.py on an MI355X, by family (measurements: nothing reads them)
DEVICE_FIGURES = {"split A": 0.89, "split B": 0.54, "split D": 0.79, "split impulse": 1.96, "fp32 E": 2.27, "fp32 edge": 2.49, "fp32 impulse": 1.00, "bias": 0.31}

# mm(ta, tb) of conv_wgrad_split_kernel, in its order: (plane of gy, plane of x)
KEPT = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))
SMALL = ((1, 1), (2, 0), (0, 2))  # the three small cross products


def to_np(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


# ---------------------------------------------------------------------------------------------------------------- the split, restated
def split_bf16x3(v, rne=False):
    """conv_common.h split_pair<3>: plane = the high 16 bits of the fp32 value, v -= plane (exact), three times.  -> [3, ...] float32 planes whose sum is v
    exactly (asserted: nothing is left after three planes; inputs are 0 or >= 2^-60 in magnitude, so no plane is an fp32 subnormal).
    rne=True: a seeded defect -- planes rounded to nearest even instead of truncated (the remainder need not vanish then and is not asserted)"""
    r = np.ascontiguousarray(v, np.float32).copy()
    a = np.abs(r)
    assert np.all((a == 0) | (a >= 2.0 ** -60)), "split_bf16x3: magnitudes below 2^-60"
    out = np.empty((3,) + r.shape, np.float32)
    for pl in range(3):
        u = r.view(np.uint32)
        if rne:
            u = u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
        out[pl] = (u & np.uint32(0xFFFF0000)).view(np.float32)
        r = r - out[pl]
    if not rne:
        assert not r.any(), "split_bf16x3: a remainder after three planes"
    return out


def windows(x, K, dil, pad, T, shift=None):
    """-> xw [B, C, K, T]: xw[b, c, k, t] = x[b, c, t + k dil - pad (+ shift[k])], 0 outside [0, T_in)"""
    x = np.asarray(x)
    n = np.arange(T)[None, :] + (np.arange(K) * dil - pad + (0 if shift is None else np.asarray(shift)))[:, None]
    ok = (n >= 0) & (n < x.shape[2])
    return np.where(ok[None, None], x[:, :, np.clip(n, 0, x.shape[2] - 1)], x.dtype.type(0))


def windows_transposed(gy, K, u, p, T):
    """-> [B, C_out, K, T]: gy[b, co, m u - p + k], 0 outside [0, n_out)"""
    gy = np.asarray(gy)
    n = np.arange(T)[None, :] * u - p + np.arange(K)[:, None]
    ok = (n >= 0) & (n < gy.shape[2])
    return np.where(ok[None, None], gy[:, :, np.clip(n, 0, gy.shape[2] - 1)], gy.dtype.type(0))


def windows_strided(x, K, stride, pad, T):
    """-> [N, C, K, T]: x[n, c, t stride + k - pad], 0 outside [0, T_in)"""
    x = np.asarray(x)
    n = np.arange(T)[None, :] * stride - pad + np.arange(K)[:, None]
    ok = (n >= 0) & (n < x.shape[2])
    return np.where(ok[None, None], x[:, :, np.clip(n, 0, x.shape[2] - 1)], x.dtype.type(0))


def _mat(a):
    """[B, C, T] -> [C, B T] float64"""
    return np.ascontiguousarray(np.asarray(a, np.float64).transpose(1, 0, 2)).reshape(a.shape[1], -1)


def _wmat(w):
    """[B, C, K, T] -> [B T, C K] float64"""
    return np.ascontiguousarray(np.asarray(w, np.float64).transpose(0, 3, 1, 2)).reshape(w.shape[0] * w.shape[3], -1)


def _core(a, bw, rounded=True, dtype=np.float64):
    """a [B, Ca, T] (the operand in the place of gy), bw [B, Cb, K, T] (the other one, windowed) -> (ref [Ca, Cb, K], S)"""
    a, bw = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(bw, np.float32)
    shape = (a.shape[1], bw.shape[1], bw.shape[2])
    S = (np.abs(_mat(a)) @ np.abs(_wmat(bw))).reshape(shape)
    if np.dtype(dtype) == np.float32:
        return serial_fp32(a, bw, split=rounded).astype(np.float64), S
    if not rounded:
        return (_mat(a) @ _wmat(bw)).reshape(shape), S
    ap, bp = split_bf16x3(a).astype(np.float64), split_bf16x3(bw).astype(np.float64)
    ref = _mat(ap[0]) @ _wmat(bw) + _mat(ap[1]) @ _wmat(bp[0] + bp[1]) + _mat(ap[2]) @ _wmat(bp[0])      # g0 x + g1 (x0 + x1) + g2 x0: the six kept products
    return ref.reshape(shape), S


def expected(gy, x, K, dil, pad, *, rounded=True, dtype=np.float64):
    """-> (ref [C_out, C_in, K], S): the sum over (b, t) of the six kept plane products in fp64 -- g0 x + g1 (x0 + x1) + g2 x0 --; S the same sum over
    |gy| |x|.  rounded=False: the plain fp64 gradient (the fp32 kernel's reference).  dtype=np.float32: serial_fp32 of the same products."""
    gy = np.ascontiguousarray(gy, np.float32)
    return _core(gy, windows(np.ascontiguousarray(x, np.float32), K, dil, pad, gy.shape[2]), rounded, dtype)


def expected_transposed(gy, x, K, u, p, *, rounded=True, dtype=np.float64):
    """the transposed conv's weight gradient gw[ci, co, k] = sum_{b, m} x[b, ci, m] gy[b, co, m u - p + k] (gy = 0 outside [0, n_out)) from the planes: the
    kept set of plane pairs is symmetric, so x in the place of gy (autograd.conv_backward) keeps it.  -> (ref [C_in, C_out, K], S)"""
    x = np.ascontiguousarray(x, np.float32)
    return _core(x, windows_transposed(np.ascontiguousarray(gy, np.float32), K, u, p, x.shape[2]), rounded, dtype)


def expected_strided(gy, x, K, stride, pad, *, rounded=True, dtype=np.float64):
    """a dense strided conv's weight gradient gw[co, c, k] = sum_{n, t} gy[n, co, t] x[n, c, t stride + k - pad] from the planes (StridedConv1dFn lays the
    phases of x out as channels and the items end to end: copies and zeros, the planes are the elements' own).  -> (ref [C_out, C, K], S)"""
    gy = np.ascontiguousarray(gy, np.float32)
    return _core(gy, windows_strided(np.ascontiguousarray(x, np.float32), K, stride, pad, gy.shape[2]), rounded, dtype)


def expected_bias(gy):
    """-> (sum over (b, t) of gy in fp64 [C_out], sum |gy|)"""
    g = np.asarray(to_np(gy), np.float64)
    return g.sum((0, 2)), np.abs(g).sum((0, 2))


def serial_bias(gy):
    """gy's rows summed over (b, t) in one serial fp32 chain"""
    g = _mat(np.asarray(gy, np.float32)).astype(np.float32)
    return np.add.accumulate(g, axis=1, dtype=np.float32)[:, -1].astype(np.float64)


def serial_subset(Ca, Cb, K, limit=40000):
    """the output channels serial_fp32 takes: all of them up to `limit` outputs, else a regular sub-grid (~48 x ~32 channels, every tap)"""
    if Ca * Cb * K <= limit:
        return np.arange(Ca), np.arange(Cb)
    return np.arange(0, Ca, max(1, Ca // 48)), np.arange(0, Cb, max(1, Cb // 32))


def serial_fp32(a, bw, split=True, ca=None, cb=None):
    """every product of one output in ONE serial fp32 chain: items in order, 16 positions at a time; split: per step the six plane products in the kernel's
    order (KEPT), each product exact in fp32; else the fp32 operands themselves, every product rounded to fp32 first.  -> [len(ca), len(cb), K] float32"""
    f = np.float32
    a, bw = np.ascontiguousarray(a, f), np.ascontiguousarray(bw, f)
    B, Ca, T = a.shape
    _, Cb, K, _ = bw.shape
    ca = np.arange(Ca) if ca is None else ca
    cb = np.arange(Cb) if cb is None else cb
    aT = lambda v: np.ascontiguousarray(v[:, ca].transpose(0, 2, 1))                                   # [B, T, ca]
    bT = lambda v: np.ascontiguousarray(v[:, cb].transpose(0, 3, 1, 2)).reshape(B, T, len(cb) * K)     # [B, T, cb K]
    if split:
        ap, bp = split_bf16x3(a), split_bf16x3(bw)
        terms = [(aT(ap[i]), bT(bp[j])) for i, j in KEPT]
    else:
        terms = [(aT(a), bT(bw))]
    acc = np.zeros((len(ca), len(cb) * K), f)
    tmp = np.empty_like(acc)
    for b in range(B):
        for t0 in range(0, T, 16):
            for ga, xb in terms:
                for t in range(t0, min(t0 + 16, T)):
                    np.multiply(ga[b, t][:, None], xb[b, t][None, :], out=tmp)
                    acc += tmp
    assert acc.dtype == f
    return acc.reshape(len(ca), len(cb), K)


# ---------------------------------------------------------------------------------------------------------------- the dispatch rule, restated
def ceil_div(a, b):
    return -(-a // b)


def wgrad_split_ok(B, Cout, Tout, K):
    """csrc/conv_backward.hip wgrad_split_ok (without its VS_NO_WGRAD_SPLIT switch)"""
    return 1 <= K <= 12 and Cout >= 64 and Tout % 4 == 0 and B * Tout >= 512


def split_slices(B, Cout, Cin, Tout):
    """wgrad_split_slices: partial planes of the split kernel -- 64-position units over ceil(512 / tiles) reduction slices"""
    return max(1, min(B * ceil_div(Tout, 64), ceil_div(512, ceil_div(Cin, 32) * ceil_div(Cout, 128))))


def f32_planes(B, Cout, Cin, Tout, K):
    """wgrad_slices x (4 planes per slice where the waves split the positions, K <= 4): partial planes of the fp32 kernel"""
    slices = max(1, min(B * ceil_div(Tout, 256), ceil_div(1024, ceil_div(Cin, 32) * ceil_div(Cout, 32))))
    return slices * (1 if K > 4 else 4)


def kernel_by_rule(B, Cout, Cin, Tout, K, split=True):
    """the kernel (instance) the shape reaches by the rule: the `switch` of wgrad_launch picks <KT, TS> from K"""
    if not (split and wgrad_split_ok(B, Cout, Tout, K)):
        return "conv_wgrad_kernel"
    kt, ts = (K, 1) if K <= 7 else ((4, 2) if K == 8 else ((5, 2) if K <= 10 else (6, 2)))
    return "conv_wgrad_split_kernel<%d, %d>" % (kt, ts)


# ---------------------------------------------------------------------------------------------------------------- comparison
def figures(got, ref, S):
    """-> (err, worst |err| / (2^-24 S) [inf if an element with S = 0 differs from 0], worst |err| / (2e-5 (1 + |ref|)))"""
    got, ref, S = to_np(got), np.asarray(ref, np.float64), np.asarray(S, np.float64)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(S > 0, err / (EPS32 * np.where(S > 0, S, 1.0)), np.where(got != 0, np.inf, 0.0))
    per_s = float(np.nanmax(q)) if err.size else 0.0
    scaled = float(np.nanmax(err / (TOL * (1.0 + np.abs(ref))))) if err.size else 0.0
    return err, per_s, scaled


def assert_close(got, ref, S, what="", *, F=F_WGRAD):
    """Element-wise over ALL elements: |got - ref| <= F * 2^-24 * S, an element with S = 0 exactly 0, everything finite.  Prints
    `WGRADREF <what>: per_S <..> scaled <..>` before it asserts.  -> (per_S, scaled)"""
    err, per_s, scaled = figures(got, ref, S)
    print(f"WGRADREF {what}: per_S {per_s:.3f} scaled {scaled:.4f}")
    g = to_np(got)
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} non-finite elements"
    S = np.asarray(S, np.float64)
    bound = F * EPS32 * S
    bad = (err > bound) | ((S == 0) & (g != 0))
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0.0))), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements above the bound; worst at {tuple(int(j) for j in i)}: "
                             f"got {g[i]!r}, ref {ref[i]!r}, |err| {err[i]:.3e}, bound {bound[i]:.3e}")
    return per_s, scaled


def flagged_fraction(got, ref, S, where=None, F=F_WGRAD):
    """share of the elements (selected by `where`) that assert_close would flag"""
    g, S = to_np(got), np.asarray(S, np.float64)
    bad = (np.abs(g - ref) > F * EPS32 * S) | ((S == 0) & (g != 0))
    return float(bad.mean() if where is None else bad[where].mean())


def per_s_quantiles(got, ref, S):
    """(median, largest) |err| / (2^-24 S) over the elements with S > 0"""
    q = (np.abs(to_np(got) - ref) / (EPS32 * np.where(S > 0, S, 1.0)))[S > 0]
    return float(np.median(q)), float(q.max())


# ---------------------------------------------------------------------------------------------------------------- a device-like accumulation, with seeded defects
def emulate_split(gy, x, K, dil, pad, defect=None, bias=False):
    """conv_wgrad_split_kernel + wgrad_finish_kernel restated for the checker's self-test: 64-position units dealt round-robin to split_slices(...) reduction
    slices, per 16-position step and plane pair one fp32 block product onto the slice's fp32 plane, the planes summed in fp32.  defect: None or
      ("drop", (i, j))     -- the plane product (g_i, x_j) is not taken;
      ("tap_off", k)       -- tap k reads x one position further on;
      ("odd_off",)         -- every tap with an odd offset (k dil) & 1 reads one position further on (the v_alignbyte path);
      ("ragged",)          -- the last unit of an item is not zeroed past T_out: gy holds what the clamped float4 loads fetched (t -> min(t - t % 4, T_out - 4) + t % 4);
      ("skip_unit", u)     -- unit u is not accumulated;
      ("skip_plane", z)    -- partial plane z is left out of the plane sum;
      ("absent_tap",)      -- K odd above 8: the absent last tap of the second tap half (index K of a row of K) is stored anyway, a zero on tap 0 of the next (co, ci);
      ("bias_rows",)       -- the bias sums land one row further on;
      ("rne",)             -- planes rounded to nearest even instead of truncated.
    -> gw [C_out, C_in, K] float64 (bias: (gw, gb))"""
    f = np.float32
    gy, x = np.ascontiguousarray(gy, f), np.ascontiguousarray(x, f)
    B, Cout, Tout = gy.shape
    Cin = x.shape[1]
    kind = defect[0] if defect else None
    nsl, upi = split_slices(B, Cout, Cin, Tout), ceil_div(Tout, 64)
    Tp = upi * 64
    g = np.zeros((B, Cout, Tp), f)
    g[:, :, :Tout] = gy
    if kind == "ragged":
        t = np.arange(Tout, Tp)
        g[:, :, Tout:] = gy[:, :, np.minimum(t - t % 4, Tout - 4) + t % 4]
    shift = np.zeros(K, np.int64)
    if kind == "tap_off":
        shift[defect[1]] = 1
    if kind == "odd_off":
        shift[(np.arange(K) * dil) % 2 == 1] = 1
    xw = windows(x, K, dil, pad, Tp, shift)
    gp, xp = split_bf16x3(g, rne=kind == "rne"), split_bf16x3(xw, rne=kind == "rne")
    xT = [np.ascontiguousarray(xp[j].transpose(0, 3, 1, 2)).reshape(B, Tp, Cin * K) for j in range(3)]
    pairs = [p for p in KEPT if not (kind == "drop" and p == tuple(defect[1]))]
    planes = np.zeros((nsl, Cout, Cin * K), f)
    bplanes = np.zeros((nsl, Cout), f)
    for u in range(B * upi):
        if kind == "skip_unit" and u == defect[1]:
            continue
        z, b, t0 = u % nsl, u // upi, (u % upi) * 64
        bplanes[z] += g[b, :, t0:t0 + 64].sum(axis=1, dtype=f)
        for s in range(t0, t0 + 64, 16):
            for i, j in pairs:
                planes[z] += gp[i][b, :, s:s + 16] @ xT[j][b, s:s + 16]
    keep = [z for z in range(nsl) if not (kind == "skip_plane" and z == defect[1])]
    out, gb = np.zeros((Cout, Cin * K), f), np.zeros(Cout, f)
    for z in keep:
        out += planes[z]
        gb += bplanes[z]
    assert out.dtype == f
    if kind == "absent_tap":
        assert K in (9, 11)
        flat = out.reshape(-1)
        flat[K::K] = 0
    if kind == "bias_rows":
        gb = np.roll(gb, 1)
    out = out.reshape(Cout, Cin, K).astype(np.float64)
    return (out, gb.astype(np.float64)) if bias else out


def emulate_f32(gy, x, K, dil, pad):
    """conv_wgrad_kernel likewise: 256-position units, fp32 block products onto fp32 planes, the planes summed in fp32"""
    f = np.float32
    gy, x = np.ascontiguousarray(gy, f), np.ascontiguousarray(x, f)
    B, Cout, Tout = gy.shape
    Cin = x.shape[1]
    xT = np.ascontiguousarray(windows(x, K, dil, pad, Tout).transpose(0, 3, 1, 2)).reshape(B, Tout, Cin * K)
    out = np.zeros((Cout, Cin * K), f)
    for b in range(B):
        for t0 in range(0, Tout, 256):
            part = np.zeros_like(out)
            for s in range(t0, min(t0 + 256, Tout), 16):
                part += gy[b, :, s:s + 16] @ xT[b, s:s + 16]
            out += part
    return out.reshape(Cout, Cin, K).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- the cases, shared by the GPU test and the CPU self-test
# pad: "same" = dil (K - 1) // 2 (T_in = T_out for odd K), "valid" = 0, "full" = (K - 1) dil; T_in follows from T_out.  gains: per-channel gains 2^-6 .. 2^6 on both
# operands.  split: the kernel the case means to reach (False: the exact-fp32 one -- by the rule, or under VS_NO_WGRAD_SPLIT)
Case = namedtuple("Case", "group B Cin Cout Tout K dil pad gains split", defaults=("same", False, True))


def pad_of(c):
    return {"same": c.dil * (c.K - 1) // 2, "valid": 0, "full": (c.K - 1) * c.dil}[c.pad]


def case_id(c):
    return "%s_B%d_%d-%d_T%d_k%d_d%d_%s%s%s" % (c.group, c.B, c.Cin, c.Cout, c.Tout, c.K, c.dil, c.pad, "_gains" if c.gains else "", "" if c.split else "_f32")


# A. split kernel, every tap count, shortest reduction: C_in = 40 a ragged second 32-row tile, C_out = 72 a ragged 128-row (K < 8) / second 64-row (K >= 8) tile,
# T_out = 260 four units and one of 4 positions, N = 520 just above the dispatch floor
A_TAPS = [(1, 1), (2, 1), (2, 64), (3, 1), (3, 32), (4, 1), (4, 3), (5, 1), (5, 16), (6, 2), (7, 1), (7, 3), (8, 1), (8, 9), (9, 1), (9, 8), (10, 7),
          (11, 1), (11, 5), (11, 6), (12, 1), (12, 5)]
A_PADDED = [(5, 1), (9, 8), (12, 5)]
A_CASES = [Case("A", 2, 40, 72, 260, k, d) for k, d in A_TAPS] + [Case("A", 2, 40, 72, 260, k, d, p) for p in ("valid", "full") for k, d in A_PADDED] + \
          [Case("A", 2, 40, 72, 260, 7, 3, gains=True)]
# the dispatch edge: B T_out = 512 exactly -> split; 508, and T_out % 4 != 0 -> fp32 (K = 5: the plane counts of the two kernels differ)
EDGE_CASES = [Case("edge", 2, 40, 72, 256, 5, 1), Case("edge", 1, 40, 72, 508, 5, 1, split=False), Case("edge", 2, 40, 72, 258, 5, 1, split=False)]
# B. workgroups that walk several units: 36 units on 29 slices (seven slices take two, the second across the item boundary); the five staging variants; and 36
# planes for the eight-deep loop of wgrad_finish_kernel and its tail
B_CASES = [Case("B", 3, 192, 384, 708, k, 1) for k in (3, 5, 7, 9, 11)] + [Case("B", 3, 192, 384, 708, 5, 1, gains=True), Case("B", 1, 32, 64, 2304, 1, 1)]
# C. impulse group: shape A, gy zero but for ONE column (b, t*)
C_TAPS = [(1, 1), (2, 64), (3, 1), (5, 16), (7, 3), (8, 9), (9, 8), (11, 6), (12, 5)]
C_COLS = [(0, 0), (0, 63), (1, 64), (0, 129), (1, 259)]
C_CASES = [Case("C", 2, 40, 72, 260, k, d) for k, d in C_TAPS]
C_GAINS = Case("C", 2, 40, 72, 260, 7, 3, gains=True)
# D. the callers' layouts: (C_in, C_out, K, stride, B, T, gains) of a HipConvTranspose1d (padding (K - u) // 2); the strided dense conv (N, C, C_out, K, stride, pad, T)
D_TRANSPOSED = [(64, 16, 8, 4, 2, 256, False), (80, 12, 11, 5, 2, 260, False), (64, 16, 8, 4, 2, 256, True)]
D_STRIDED = (24, 8, 64, 5, 3, 2, 61)          # T_out = 21, Q = 2, H_q = 22: conv_wgrad(gyF [1, 64, 528], XF [1, 24, 529], 2, 1, 0, bias=True)
# E. exact-fp32 kernel (C_out = 40 < 64): K <= 4 positions over the waves (four planes per slice), K > 4 taps over the waves (2/1/1/1, 4/3/3/3, 4/4/4/4);
# spans of 64 and 60; 33 units on 29 slices; one group-A shape under VS_NO_WGRAD_SPLIT
E_CASES = [Case("E", 2, 40, 40, 261, k, d, split=False) for k, d in ((1, 1), (3, 1), (4, 1), (3, 32), (5, 1), (13, 1), (16, 4), (5, 16))] + \
          [Case("E", 3, 192, 192, 2561, 5, 1, split=False), Case("E", 2, 40, 72, 260, 7, 3, split=False), Case("E", 2, 40, 40, 261, 5, 1, gains=True, split=False)]
# F. fused bias gradient: one case of A, one of B, one of E
F_CASES = [Case("A", 2, 40, 72, 260, 9, 8), Case("B", 3, 192, 384, 708, 5, 1), Case("E", 2, 40, 40, 261, 4, 1, split=False)]


# (B, C_out, C_in, T_out, K) of the two prescribed shapes at which both kernels would leave the SAME number of planes (36 = 9 units x 4 wave planes; 8 = 2 x 4): there
# the count agrees with the split kernel's and the restated rule alone says which kernel ran; every other shape tells them apart by the count
COUNTS_COINCIDE = [(1, 64, 32, 2304, 1), (2, 64, 64, 256, 2)]


def _seed(*v):
    s = 0
    for i in v:
        s = (s * 1000003 + int(i)) % (2 ** 31)
    return s


def gains(r, C):
    return np.exp2(r.uniform(-6.0, 6.0, (1, C, 1))).astype(np.float32)


def inputs(c, impulse=None):
    """-> (gy [B, C_out, T_out], x [B, C_in, T_in], pad) of a case, the same on the GPU and in the self-test.  impulse = (b, t): gy zero but for that column"""
    pad = pad_of(c)
    r = np.random.default_rng(_seed(c.B, c.Cin, c.Cout, c.Tout, c.K, c.dil, pad, c.gains))
    Tin = c.Tout + (c.K - 1) * c.dil - 2 * pad
    assert Tin >= 1
    gy = r.standard_normal((c.B, c.Cout, c.Tout)).astype(np.float32)
    x = r.standard_normal((c.B, c.Cin, Tin)).astype(np.float32)
    if c.gains:
        gy, x = gy * gains(r, c.Cout), x * gains(r, c.Cin)
    if impulse is not None:
        col = gy[impulse[0], :, impulse[1]].copy()
        gy[:] = 0
        gy[impulse[0], :, impulse[1]] = col
    return gy, x, pad


def transposed_inputs(Cin, Cout, K, u, B, T, with_gains):
    """-> (x [B, C_in, T], gy [B, C_out, (T - 1) u - 2 p + K], p)"""
    p = (K - u) // 2
    r = np.random.default_rng(_seed(Cin, Cout, K, u, B, T, with_gains))
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    gy = r.standard_normal((B, Cout, (T - 1) * u - 2 * p + K)).astype(np.float32)
    if with_gains:
        x, gy = x * gains(r, Cin), gy * gains(r, Cout)
    return x, gy, p


def transposed_role(Cin, Cout, K, u, B, T):
    """the conv_wgrad call autograd.conv_backward makes for a transposed conv: (B, `C_out` = C_in, `C_in` = u C_out, `T_out` = T, Q taps)"""
    return B, Cin, u * Cout, T, ceil_div(K, u)


def strided_inputs(N, C, Cout, K, stride, pad, T):
    r = np.random.default_rng(_seed(N, C, Cout, K, stride, pad, T))
    Tout = (T + 2 * pad - K) // stride + 1
    return r.standard_normal((N, C, T)).astype(np.float32), r.standard_normal((N, Cout, Tout)).astype(np.float32)


def strided_role(N, C, Cout, K, stride, pad, T):
    """the conv_wgrad call StridedConv1dFn.backward makes: (1, C_out, stride C, N H_q, Q taps)"""
    Tout, Q = (T + 2 * pad - K) // stride + 1, ceil_div(K, stride)
    return 1, Cout, stride * C, N * (Tout + Q - 1), Q


def table_cases():
    """every distinct conv_wgrad case of the tables (groups A, B, E and the dispatch edge); the impulse group takes a derived bound and group D is listed by
    table_operands"""
    seen, out = set(), []
    for c in A_CASES + EDGE_CASES + B_CASES + E_CASES + F_CASES:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def table_operands():
    """-> [(id, a, bw, split)]: the operands of every table shape in _core's form -- table_cases() and the callers' layouts of group D"""
    out = []
    for c in table_cases():
        gy, x, pad = inputs(c)
        out.append((case_id(c), gy, windows(x, c.K, c.dil, pad, c.Tout), c.split))
    for Cin, Cout, K, u, B, T, g in D_TRANSPOSED:
        x, gy, p = transposed_inputs(Cin, Cout, K, u, B, T, g)
        out.append(("D_tconv_%d-%d_k%d_u%d%s" % (Cin, Cout, K, u, "_gains" if g else ""), x, windows_transposed(gy, K, u, p, T), True))
    xs, gys = strided_inputs(*D_STRIDED)
    out.append(("D_strided", gys, windows_strided(xs, D_STRIDED[3], D_STRIDED[4], D_STRIDED[5], gys.shape[2]), True))
    return out
