"""Every default-arithmetic (VS_MATH_SPLIT3) conv instance, element by element, against the fp64 sum of the device's own operand planes
(tests/split3_reference.py): |got - ref| <= F_SPLIT * 2^-24 * S over ALL elements of ALL items, S = the sum of the absolute terms.  The other tests of these
kernels hold conv_ktap_kernel to conv_split_kernel bit for bit (a defect in the shared split, running scale, staging or epilogue passes), hold them to fp64 by an
rms bound on item 0 (whose mask is all ones), or element-wise at 2e-5 * (1 + |ref|) on shapes that reach neither the wide tiles nor the transposed / adjoint
instances -- a bound one dropped low cross product passes on most outputs (tests/test_split3_reference_cpu.py).  Each case names the instance it must reach
(ConvOp.kernel_instance); B = 2 with a ragged mask; inputs go through pin_scale, so one scale per item reproduces the device's planes whatever the tile shape.
Every assert_close prints `SPLIT3REF <instance> <case>: per_S <|err| / (2^-24 S)> scaled <|err| / (2e-5 (1 + |ref|))>`."""
import numpy as np
import pytest
import torch

import split3_reference as R
from visinger_amd import _lib as L

pytestmark = pytest.mark.gpu

B = R.B
OUT_ACT = {L.OUT_NONE: None, L.OUT_TANH: "tanh", L.OUT_RELU: "relu"}
assert (L.IN_NONE, L.IN_LRELU, L.IN_MASK, L.IN_LRELU_MASK) == (R.IN_NONE, R.IN_LRELU, R.IN_MASK, R.IN_LRELU_MASK)

# tile shape -> (dispatch switches of the tile kernel, its template tail, switches of the conv_ktap instance, its template tail)
TILES = {
    "128x256": ({"VS_NO_KTAP": 1, "VS_NO_SMALL_GRID": 1}, "8, 4, 1", {"VS_NO_SMALL_GRID": 1}, "4, 1, 8"),
    "64x256": ({"VS_NO_KTAP": 1, "VS_CONV_CFG": 3}, "4, 2, 2", {"VS_CONV_CFG": 3}, "2, 2, 4"),
    "64x256_nocfg": ({"VS_NO_KTAP": 1, "VS_NO_SMALL_GRID": 1}, "4, 2, 2", None, None),          # two row tiles: this shape without VS_CONV_CFG
    "32x256": ({"VS_NO_KTAP": 1, "VS_CONV_CFG": 2}, "2, 1, 4", {"VS_CONV_CFG": 2}, "1, 4, 2"),
    "32x256_nocfg": ({"VS_NO_KTAP": 1, "VS_NO_SMALL_GRID": 1}, "2, 1, 4", None, None),          # one row tile: likewise
    "32x128": ({"VS_NO_KTAP": 1}, "1, 1, 4", {}, "1, 4, 1"),                                    # what a short launch takes by itself
}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def conv_case(oracle, vs_option, opts, expect, Cin, Cout, T, k, du, in_act, *, tr=False, wn=False, res=False, acc=False, scale=1.0,
              out_act=L.OUT_NONE, out_mask=False, bias_b=False, inplace=False, seed=0):
    """one launch of a split-f16 conv against the plane reference.  opts: dispatch switches; expect: the instance name (or a predicate on it)"""
    from visinger_amd.ops import ConvOp, weightnorm_fold
    for name, v in opts.items():
        vs_option(name, v)
    r, x, w, bias, pad = R.conv_inputs(Cin, Cout, T, k, du, in_act, tr=tr, seed=seed)
    op = ConvOp(L.CONV_TRANSPOSE1D if tr else L.CONV1D, Cin, Cout, k, du, pad).set_math(L.MATH_SPLIT3)
    if wn:
        v, g = dev(w * 3.0), dev(0.5 + r.random((w.shape[0], 1, 1)))
        op.set_weights(v, g, dev(bias))
        w = weightnorm_fold(v, g).cpu().numpy()          # the fp32 effective weight the library splits
    else:
        op.set_weights(dev(w), None, dev(bias))
    Tout = op.out_len(T)
    mask = R.ragged_mask(B, T)
    masked_in = in_act in (L.IN_MASK, L.IN_LRELU_MASK)
    rv = r.standard_normal((B, Cout, Tout)).astype(np.float32) if res else None
    av = r.standard_normal((B, Cout, Tout)).astype(np.float32) if acc else None
    rt, at = (None if a is None else dev(a) for a in (rv, av))
    bb = r.standard_normal((B, Cout)).astype(np.float32) if bias_b else None
    y = at if inplace else torch.empty((B, Cout, Tout), device="cuda")
    op.forward(dev(x), y=y, in_act=in_act, mask=dev(mask) if (masked_in or out_mask) else None, bias_b=None if bb is None else dev(bb),
               res=rt, acc=at, scale=scale, out_act=out_act, out_mask=out_mask)
    torch.cuda.synchronize()
    inst = op.kernel_instance()
    ref, S = R.expected(oracle, x, w, bias, transposed=tr, dil_or_stride=du, padding=pad, lrelu=in_act in (L.IN_LRELU, L.IN_LRELU_MASK),
                        in_mask=mask if masked_in else None, bias_b=bb, res=rv, acc=av, scale=scale, out_act=OUT_ACT[out_act],
                        out_mask=mask if out_mask else None)
    assert y.shape == ref.shape
    what = f"{inst} {'tconv' if tr else 'conv'} {Cin}->{Cout} T{T} k{k} d{du} in{in_act}"
    assert expect(inst) if callable(expect) else inst == expect, (what, expect)
    return R.assert_close(y, ref, S, what)


# ---- the tile kernel conv_split_kernel<1, NT_W, WAVES_M, WAVES_N, 3>: all four tile shapes; C_in off the 16-channel chunk (33, 200, 40), C_out off the 32-row
# tile (20, 70, 136), T one past a column tile (129: the 128-column tile; 257, 261: the 256-column ones), T in {1, 2, 5} with halos wider than the sequence
@pytest.mark.parametrize("tile,Cin,Cout,T,k,d", R.TILE_CASES)
def test_tile_kernel(oracle, vs_option, tile, Cin, Cout, T, k, d):
    opts, tail, _, _ = TILES[tile]
    expect = "conv_split_kernel<1, %s, 3>" % tail
    for in_act, out_mask, res in R.tile_variants(k):
        conv_case(oracle, vs_option, opts, expect, Cin, Cout, T, k, d, in_act, out_mask=out_mask, res=res)


# ---- conv_ktap_kernel<taps, transform, 2 planes, fp32 tensors, WAVES_M, WAVES_N, NT, MT_W>: every instance ktap_instance(3, cfg, kt, 0, in_act) admits
@pytest.mark.parametrize("tile,k,d,in_act", R.KTAP_CASES)
def test_ktap_instances(oracle, vs_option, tile, k, d, in_act):
    _, _, opts, tail = TILES[tile]
    expect = "conv_ktap_kernel<%d, %d, 2, 0, %s, 1>" % (k, in_act, tail)
    (c0, o0, t0), (c1, o1, t1) = R.ktap_shapes(tile, k)
    conv_case(oracle, vs_option, opts, expect, c0, o0, t0, k, d, in_act, out_mask=(k % 2 == 1))      # (an output mask needs T_out == T: not behind the 2-tap conv)
    conv_case(oracle, vs_option, opts, expect, c1, o1, t1, k, d, in_act, res=True, bias_b=True)


# ---- transposed convs
@pytest.mark.parametrize("Cin,Cout,k,u,T", R.TR_SHAPES)
def test_transposed(oracle, vs_option, Cin, Cout, k, u, T):
    """polyphase transposed convs behind a leaky-relu, weight norm over the input channel: conv_split_tr_kernel<1, ..., 3> on the 128- / 64-row tiles (more than one
    32-row tile of the C_out * stride virtual rows), and whichever tile a short launch takes by itself (the 32-row tile has no polyphase store path and runs
    conv_split_kernel<1, 2, 1, 4, 3>)"""
    wide = lambda inst: inst.startswith("conv_split_tr_kernel<1, ") and inst.endswith(", 3>")
    anyt = lambda inst: wide(inst) or inst == "conv_split_kernel<1, 2, 1, 4, 3>"
    conv_case(oracle, vs_option, {"VS_NO_SMALL_GRID": 1, "VS_NO_KTAP": 1}, wide if Cout * u > 32 else "conv_split_kernel<1, 2, 1, 4, 3>", Cin, Cout, T, k, u, L.IN_LRELU,
              tr=True, wn=True)
    conv_case(oracle, vs_option, {}, anyt, Cin, Cout, T, k, u, L.IN_LRELU_MASK, tr=True)


@pytest.mark.parametrize("Cin,Cout,k,u,T", R.TR_KTAP)
def test_transposed_ktap_instance(oracle, vs_option, Cin, Cout, k, u, T):
    """the generator's upsampler shape (k = 2 * stride, two taps per phase): the polyphase conv_ktap instance and its tile twin"""
    conv_case(oracle, vs_option, {"VS_NO_SMALL_GRID": 1}, "conv_ktap_kernel<2, 1, 2, 4, 4, 1, 8, 1>", Cin, Cout, T, k, u, L.IN_LRELU, tr=True, wn=True)
    conv_case(oracle, vs_option, {"VS_NO_SMALL_GRID": 1, "VS_NO_KTAP": 1}, "conv_split_tr_kernel<1, 8, 4, 1, 3>", Cin, Cout, T, k, u, L.IN_LRELU, tr=True, seed=1)


# ---- paired kinds
PAIR_EXPECT = {"ktap_pair": ({}, "conv_ktap_kernel<5, 0, 2, 0, 2, 2, 2, 2>"), "128x128": ({"VS_NO_KTAP": 1}, "conv_split_kernel<2, 2, 2, 2, 3>"),
               "128x128_k3": ({}, "conv_split_kernel<2, 2, 2, 2, 3>"), "64x256": ({}, "conv_split_kernel<2, 2, 1, 4, 3>")}


@pytest.mark.parametrize("mode", ["gate", "coupling_fwd", "coupling_inv"])
@pytest.mark.parametrize("H,Cin,T,k,d,tile", R.PAIR_TILES, ids=[p[5] for p in R.PAIR_TILES])
def test_paired_kinds(oracle, vs_option, H, Cin, T, k, d, tile, mode):
    """VS_CONV1D_PAIRED: the WaveNet gate tanh(a) * sigmoid(b) over the row pair (c, H + c) with the conditioning as a per-item bias, and the affine coupling
    update x1' = m + x1 * exp(logs) (with its log-determinant) / x1' = (x1 - m) * exp(-logs), under the mask.  The pre-activations come from the planes, the
    expressions are taken in fp64; the bound is the conv's, delta = F_SPLIT * 2^-24 * S per pre-activation, carried through the expression's first derivative
    (delta <= 1e-5: the second-order term is below 1e-10 of the output), plus the fp32 evaluation of the expression itself -- expf and the
    division at <= 2^-22 relative, tanh_fast at <= 1e-7 absolute (csrc/conv_common.h), the products at 2^-24 each: 2^-21 of the largest factor product."""
    from visinger_amd.ops import ConvOp
    opts, expect = PAIR_EXPECT[tile]
    for name, v in opts.items():
        vs_option(name, v)
    r = np.random.default_rng(H + T + k)
    x = R.pin_scale(r.standard_normal((B, Cin, T)).astype(np.float32), r)
    gain = 1.0 if mode == "gate" else 0.5
    w = (gain * r.standard_normal((2 * H, Cin, k)) / np.sqrt(Cin * k) / 4.0).astype(np.float32)      # (/ 4: the pinned rows carry magnitudes of 4 .. 8)
    bias = ((1.0 if mode == "gate" else 0.1) * r.standard_normal(2 * H)).astype(np.float32)
    pad = d * (k - 1) // 2
    op = ConvOp(L.CONV1D_PAIRED, Cin, 2 * H, k, d, pad).set_math(L.MATH_SPLIT3)
    op.set_weights(dev(w), None, dev(bias))
    mask = R.ragged_mask(B, T)
    EV = 2.0 ** -21
    if mode == "gate":
        gl = r.standard_normal((B, 2 * H)).astype(np.float32)
        pre, S = R.expected_pre(oracle, x, w, bias, dil_or_stride=d, padding=pad, bias_b=gl)
        delta = R.F_SPLIT * R.EPS32 * S
        ta, sb = np.tanh(pre[:, :H]), oracle.sigmoid(pre[:, H:])
        ref = ta * sb
        bound = sb * (1.0 - ta * ta) * delta[:, :H] + np.abs(ta) * sb * (1.0 - sb) * delta[:, H:] + EV * sb
        y = op.forward(dev(x), bias_b=dev(gl), pair_mode=L.PAIR_GATE)
    else:
        x1 = r.standard_normal((B, H, T)).astype(np.float32)
        stats, S = R.expected_pre(oracle, x, w, bias, dil_or_stride=d, padding=pad)
        m3 = mask[:, None].astype(np.float64)
        stats, delta = stats * m3, R.F_SPLIT * R.EPS32 * S * m3
        m, logs = stats[:, :H], stats[:, H:]
        ld = torch.zeros(B, device="cuda")
        if mode == "coupling_fwd":
            ref = m + x1 * np.exp(logs) * m3
            bound = delta[:, :H] + np.abs(x1) * np.exp(logs) * delta[:, H:] + EV * (np.abs(m) + np.abs(x1) * np.exp(logs)) * m3
            y = op.forward(dev(x), mask=dev(mask), res=dev(x1), pair_mode=L.PAIR_COUPLING_FWD, logdet=ld)
            ref_ld = logs.sum(axis=(1, 2))
            assert np.abs(ld.cpu().double().numpy() - ref_ld).max() <= 1e-4 * np.abs(ref_ld).max()
        else:
            ref = (x1 - m) * np.exp(-logs) * m3
            bound = np.exp(-logs) * delta[:, :H] + np.abs(ref) * delta[:, H:] + EV * (np.abs(x1) + np.abs(m)) * np.exp(-logs) * m3
            y = op.forward(dev(x), mask=dev(mask), res=dev(x1), pair_mode=L.PAIR_COUPLING_INV)
    torch.cuda.synchronize()
    assert op.kernel_instance() == expect, op.kernel_instance()
    assert y.shape == (B, H, T)
    R.assert_close(y, ref, None, f"{expect} {mode} H{H} {Cin} T{T} k{k} d{d}", bound=bound)
    # (per_S of the pre-activation itself is not observable through the expression; the largest |err| / bound is what the case reports)
    print("SPLIT3REF   of_bound %.3f" % float((np.abs(R.to_np(y) - ref) / np.maximum(bound, 1e-300))[bound > 0].max()))


# ---- fused options and the other conv kinds of the default arithmetic
@pytest.mark.parametrize("H,opts,expect", [(32, {}, "conv_ktap_kernel<1, 0, 2, 0, 2, 2, 4, 1>"), (32, {"VS_NO_KTAP": 1}, "conv_split_kernel<1, 4, 2, 2, 3>"),
                                           (16, {}, "conv_split_kernel<1, 1, 1, 4, 3>")], ids=["32_ktap", "32_tile", "16"])
def test_split_row(oracle, vs_option, H, opts, expect):
    """the WaveNet's res / skip 1 x 1 conv with its two destinations: split_row on a 32-row tile edge (one launch) and inside a tile (two passes)"""
    from visinger_amd.ops import ConvOp
    for name, v in opts.items():
        vs_option(name, v)
    r = np.random.default_rng(H)
    T = 137
    acts, x, out = (r.standard_normal((B, H, T)).astype(np.float32) for _ in range(3))
    acts = R.pin_scale(acts, r)
    w = (r.standard_normal((2 * H, H, 1)) / np.sqrt(H)).astype(np.float32)
    bias = r.standard_normal(2 * H).astype(np.float32)
    mask = R.ragged_mask(B, T)
    op = ConvOp(L.CONV1D, H, 2 * H, 1, 1, 0).set_math(L.MATH_SPLIT3)
    op.set_weights(dev(w), None, dev(bias))
    xt, ot = dev(x), dev(out)
    op.forward(dev(acts), y=xt, res=xt, out_mask=True, mask=dev(mask), split_row=H, out1=dict(y=ot, acc=ot))
    torch.cuda.synchronize()
    assert op.kernel_instance() == expect, op.kernel_instance()
    rs, S = R.expected_pre(oracle, acts, w, bias)
    what = f"{expect} split_row {H}"
    R.assert_close(xt, (x + rs[:, :H]) * mask[:, None], S[:, :H] + np.abs(x), what + " rows < split")
    R.assert_close(ot, out + rs[:, H:], S[:, H:] + np.abs(out), what + " rows >= split")


@pytest.mark.parametrize("opts,expect", [({}, "conv_ktap_kernel<1, 0, 2, 0, 2, 2, 4, 1>"), ({"VS_NO_KTAP": 1}, "conv_split_kernel<1, 4, 2, 2, 3>")], ids=["ktap", "tile"])
def test_flip_in_and_channel_window(oracle, vs_option, opts, expect):
    """the coupling layer's `pre` conv reading the logical x0 half from the physical tensor (upper half, reversed)"""
    from visinger_amd.ops import ConvOp, _off
    for name, v in opts.items():
        vs_option(name, v)
    r = np.random.default_rng(21)
    half, H, T = 48, 64, 130
    C = 2 * half
    xfull = r.standard_normal((B, C, T)).astype(np.float32)
    xfull[:, half:] = R.pin_scale(xfull[:, ::-1][:, :half], r)[:, ::-1]          # (the LOGICAL input -- upper half, reversed -- carries the pinned rows)
    w = (r.standard_normal((H, half, 1)) / np.sqrt(half)).astype(np.float32)
    bias = r.standard_normal(H).astype(np.float32)
    mask = R.ragged_mask(B, T)
    op = ConvOp(L.CONV1D, half, H, 1, 1, 0, L.FLIP_IN).set_math(L.MATH_SPLIT3)
    op.set_weights(dev(w), None, dev(bias))
    xt = dev(xfull)
    y = torch.empty(B, H, T, device="cuda")
    op.forward(None, B=B, T=T, x_ptr=_off(xt, half * T), x_bs=C * T, y=y, mask=dev(mask), out_mask=True)
    torch.cuda.synchronize()
    assert op.kernel_instance() == expect, op.kernel_instance()
    ref, S = R.expected(oracle, np.ascontiguousarray(xfull[:, ::-1][:, :half]), w, bias, out_mask=mask)
    R.assert_close(y, ref, S, expect + " flip-in, channel window")


@pytest.mark.parametrize("opts,expect", [({}, "conv_ktap_kernel<7, 1, 2, 0, 2, 2, 4, 1>"), ({"VS_NO_KTAP": 1}, "conv_split_kernel<1, 4, 2, 2, 3>")], ids=["ktap", "tile"])
def test_weightnorm_residual_accumulate_scale_in_place_and_tanh(oracle, vs_option, opts, expect):
    conv_case(oracle, vs_option, opts, expect, 64, 64, 333, 7, 3, L.IN_LRELU, wn=True, res=True, acc=True, scale=1.0 / 3.0)
    conv_case(oracle, vs_option, opts, expect, 64, 64, 333, 7, 3, L.IN_LRELU, wn=True, res=True, acc=True, scale=1.0 / 3.0, inplace=True)
    conv_case(oracle, vs_option, opts, expect, 64, 64, 333, 7, 3, L.IN_LRELU, wn=True, acc=True, inplace=True, out_act=L.OUT_TANH)


def test_relu_output_mask_and_per_item_bias(oracle, vs_option):
    conv_case(oracle, vs_option, {}, "conv_ktap_kernel<9, 2, 2, 0, 1, 4, 1, 1>", 48, 96, 211, 9, 1, L.IN_MASK, bias_b=True, out_act=L.OUT_RELU, out_mask=True)
    conv_case(oracle, vs_option, {"VS_NO_KTAP": 1}, "conv_split_kernel<1, 1, 1, 4, 3>", 48, 96, 211, 9, 1, L.IN_MASK, bias_b=True, out_act=L.OUT_RELU, out_mask=True)


@pytest.mark.parametrize("k,paired_pack", [(5, False), (9, True)], ids=["k5", "k9_pair_pack"])
def test_adjoint_handles(oracle, vs_option, k, paired_pack):
    """VS_CONV_ADJOINT: the grad-input conv of a forward conv, packed from the FORWARD weight [C_out_fwd = this conv's C_in, C_in_fwd, k] -- alone
    (vs_conv_set_weights) and together with the forward handle (vs_conv_set_weights_pair).  Its reference is the conv with the channel-transposed,
    tap-reversed weight; on the conv_ktap instance a short launch takes and on the tile kernel."""
    from visinger_amd.ops import ConvOp
    cf_in, cf_out, T = 96, 48, 129                 # the forward conv: 96 -> 48; its grad-input: 48 -> 96
    r = np.random.default_rng(50 + k)
    wf = (r.standard_normal((cf_out, cf_in, k)) / np.sqrt(cf_out * k)).astype(np.float32)
    bias = r.standard_normal(cf_out).astype(np.float32)
    gy = R.pin_scale(r.standard_normal((B, cf_out, T)).astype(np.float32), r)
    pad = (k - 1) // 2
    adj = ConvOp(L.CONV1D, cf_out, cf_in, k, 1, (k - 1) - pad, L.CONV_ADJOINT).set_math(L.MATH_SPLIT3)
    if paired_pack:
        fwd = ConvOp(L.CONV1D, cf_in, cf_out, k, 1, pad).set_math(L.MATH_SPLIT3)
        fwd.bind(None, lambda: (dev(wf), None, dev(bias)), adjoint=adj)
        xin = R.pin_scale(r.standard_normal((B, cf_in, T)).astype(np.float32), r)
        y = fwd.forward(dev(xin))
        torch.cuda.synchronize()
        inst = fwd.kernel_instance()
        assert inst == "conv_ktap_kernel<%d, 0, 2, 0, 2, 2, 4, 1>" % k, inst          # (two row tiles: the 64-row tile)
        ref, S = R.expected(oracle, xin, wf, bias, padding=pad)
        R.assert_close(y, ref, S, f"{inst} forward handle of the paired pack k{k}")
    else:
        adj.set_weights(dev(wf), None, None)
    wa = np.ascontiguousarray(wf.transpose(1, 0, 2)[:, :, ::-1])
    ref, S = R.expected(oracle, gy, wa, None, padding=(k - 1) - pad)
    for opts, expect in (({}, "conv_ktap_kernel<%d, 0, 2, 0, 1, 4, 1, 1>" % k), ({"VS_NO_KTAP": 1}, "conv_split_kernel<1, 1, 1, 4, 3>")):
        for name, v in opts.items():
            vs_option(name, v)
        y = adj.forward(dev(gy))
        torch.cuda.synchronize()
        assert adj.kernel_instance() == expect, adj.kernel_instance()
        R.assert_close(y, ref, S, f"{expect} adjoint k{k}")


@pytest.mark.parametrize("opts,expect", [({}, "conv_ktap_kernel<3, 0, 2, 0, 1, 4, 1, 1>"), ({"VS_NO_KTAP": 1}, "conv_split_kernel<1, 1, 1, 4, 3>")], ids=["ktap", "tile"])
def test_weight_scale_is_the_packs(oracle, vs_option, opts, expect):
    """scale_of against the weight pack's wscale (device memory of the handle: not readable), through the only place a plane's VALUE depends on the scale --
    where it is subnormal.  Output rows 32 .. 63 carry weights 2^-30 of the conv's largest and no bias: under s_w their high planes are f16 subnormals
    (8 bits or fewer, no low plane), S of those rows is as small as they are, and the bound holds only if the reference rounds them on the device's grid.
    The same reference under 2 s_w or s_w / 2 -- a scale rule off by one -- is flagged on most of those outputs."""
    from visinger_amd.ops import ConvOp
    for name, v in opts.items():
        vs_option(name, v)
    Cin, Cout, T, k, d = 48, 96, 129, 3, 1
    _, x, w, bias, pad = R.conv_inputs(Cin, Cout, T, k, d, L.IN_NONE)
    w[32:64] *= np.float32(2.0 ** -30)
    bias[32:64] = 0.0
    op = ConvOp(L.CONV1D, Cin, Cout, k, d, pad).set_math(L.MATH_SPLIT3)
    op.set_weights(dev(w), None, dev(bias))
    y = op.forward(dev(x))
    torch.cuda.synchronize()
    assert op.kernel_instance() == expect, op.kernel_instance()
    ref, S = R.expected(oracle, x, w, bias, padding=pad)
    sw = R.scale_of(np.abs(w).max())
    assert np.abs(w[32:64]).max() * sw < 2.0 ** -14                      # f16 subnormals under the pack's scale
    R.assert_close(y, ref, S, f"{expect} subnormal weight planes")
    rows = np.zeros(ref.shape, bool)
    rows[:, 32:64] = True
    for wrong in (2.0 * sw, 0.5 * sw):
        off, _ = R.expected(oracle, x, w, bias, padding=pad, sw=wrong)
        frac = R.flagged_fraction(y, off, S, rows)
        print("SPLIT3REF   a reference under %g s_w is flagged on %.3f of the subnormal rows" % (wrong / sw, frac))
        assert frac >= 0.5, frac


# ---- one moving-scale group: inputs NOT pinned -- the running scale drops mid-tile and the accumulators follow
@pytest.mark.parametrize("opts,expect", [({"VS_NO_KTAP": 1, "VS_NO_SMALL_GRID": 1}, "conv_split_kernel<1, 8, 4, 1, 3>"),
                                         ({"VS_NO_SMALL_GRID": 1}, "conv_ktap_kernel<7, 3, 2, 0, 4, 1, 8, 1>"),
                                         ({"VS_NO_KTAP": 1}, "conv_split_kernel<1, 1, 1, 4, 3>")], ids=["128x256", "128x256_ktap", "32x128"])
def test_moving_scale(oracle, vs_option, opts, expect):
    """Per-channel gains of 2^-6 .. 2^6 and two outlier runs (as tests/test_conv_ktap_gpu.py): a tile's scale is whatever the chunks staged so far made it, so
    the planes are not reproduced here and the reference is the plain fp64 conv.  The bound is derived:
    |err| <= (12 + F_SPLIT) * 2^-24 * S + 2^-40 * (M_b * sum|w| + W_max * sum|x|): 12 * 2^-24 = 3 * 2^-22 -- the two operand representations at 2^-22 relative
    each and the dropped l l term; F_SPLIT for the fp32 accumulation; the floor for low planes that go subnormal under the tile's scale (M_b: the item's
    largest transformed magnitude, W_max: the largest |w|; the sums over the output's receptive field)."""
    from visinger_amd.ops import ConvOp
    for name, v in opts.items():
        vs_option(name, v)
    Cin, Cout, T, k, d = 64, 96, 600, 7, 1
    r, x, w, bias, pad = R.conv_inputs(Cin, Cout, T, k, d, L.IN_LRELU_MASK, pin=False)
    x[:, : Cin // 2] *= np.exp2(r.integers(-6, 7, (B, Cin // 2, 1))).astype(np.float32)
    x[0, 3, 100:180] = 2.0 ** 9
    x[0, Cin - 2, 300:340] = -(2.0 ** 12)
    x[1, 20, 10:14] = 2.0 ** 11
    mask = R.ragged_mask(B, T)
    op = ConvOp(L.CONV1D, Cin, Cout, k, d, pad).set_math(L.MATH_SPLIT3)
    op.set_weights(dev(w), None, dev(bias))
    y = op.forward(dev(x), in_act=L.IN_LRELU_MASK, mask=dev(mask), out_mask=True)
    torch.cuda.synchronize()
    assert op.kernel_instance() == expect, op.kernel_instance()
    xt = R.in_transform(oracle, x, True, mask).astype(np.float64)
    w64 = w.astype(np.float64)
    pre = oracle.conv1d(xt, w64, bias.astype(np.float64), dilation=d, padding=pad)
    S = oracle.conv1d(np.abs(xt), np.abs(w64), None, dilation=d, padding=pad) + np.abs(bias)[None, :, None]
    sum_w = oracle.conv1d(np.ones_like(xt), np.abs(w64), None, dilation=d, padding=pad)
    sum_x = oracle.conv1d(np.abs(xt), np.ones_like(w64), None, dilation=d, padding=pad)
    Mb = np.abs(xt).max(axis=(1, 2))[:, None, None]
    bound = (12.0 + R.F_SPLIT) * R.EPS32 * S + 2.0 ** -40 * (Mb * sum_w + np.abs(w64).max() * sum_x)
    R.assert_close(y, pre * mask[:, None], S, f"{expect} moving scale", bound=bound)
