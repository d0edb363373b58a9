"""Every conv instance of the three arithmetics whose operands are exact fp32 numbers -- VS_MATH_F32 (conv_mfma_kernel, the F(2,3) kernel conv_wino_kernel, the
fused pair respair_kernel), VS_MATH_SPLIT6 (conv_split_kernel<..., 6>, its paired and transposed uses, respair_split_kernel<..., 6, false>) and the VALU conv
conv_small_kernel -- element by element against tests/exact_reference.py: |got - ref| <= F * 2^-24 * S over ALL elements of ALL items (S: the sum of the absolute
terms; F: the family's constant, measured on the CPU from the reference's own serial fp32 chain), or the propagated bound the helper states for the pair kernels,
the paired kinds and a tanh output.  Masked outputs must be exactly zero, anything non-finite fails.  Until now these kernels were held to 2e-5 * (1 + |ref|),
to rms ratios, or to each other -- bounds one dropped 2^-16-order plane product, or a tap group missing on some columns, passes on most outputs
(tests/test_exact_reference_cpu.py).  Each case names the instance it must reach (ConvOp.kernel_instance); B = 2 with a ragged mask on item 1.
Every comparison prints `EXACTREF <instance> <case>: per_S <|err| / (2^-24 S)> scaled <|err| / (2e-5 (1 + |ref|))>`."""
import numpy as np
import pytest
import torch

import exact_reference as R
from visinger_amd import _lib as L

pytestmark = pytest.mark.gpu

B = R.B
OUT_ACT = {None: L.OUT_NONE, "tanh": L.OUT_TANH, "relu": L.OUT_RELU}
MATH = {"f32": L.MATH_F32, "wino": L.MATH_F32, "split6": L.MATH_SPLIT6}
assert (L.IN_NONE, L.IN_LRELU, L.IN_MASK, L.IN_LRELU_MASK) == (R.IN_NONE, R.IN_LRELU, R.IN_MASK, R.IN_LRELU_MASK)

NW = {"VS_NO_WINO": 1}
# tile -> (dispatch switches, template tail) of conv_mfma_kernel: the tile follows the 32-row tile count of the case (exact_reference.MFMA_CASES) or VS_CONV_CFG
MFMA_TILES = {"128x256": (NW, "1, 8, 4, 1"), "64x512": (NW, "1, 8, 2, 2"), "64x256": (NW, "1, 4, 2, 2"), "32x512": (NW, "1, 4, 1, 4"),
              "64x512_cfg": (dict(NW, VS_CONV_CFG=1), "1, 8, 2, 2"), "64x256_cfg": (dict(NW, VS_CONV_CFG=3), "1, 4, 2, 2"), "32x512_cfg": (dict(NW, VS_CONV_CFG=2), "1, 4, 1, 4")}
# ... of conv_split_kernel<1, ..., 6> (the switches of tests/test_conv_split3_oracle_gpu.py)
SPLIT_TILES = {"128x256": ({"VS_NO_SMALL_GRID": 1}, "8, 4, 1"), "64x256": ({"VS_CONV_CFG": 3}, "4, 2, 2"), "64x256_nocfg": ({"VS_NO_SMALL_GRID": 1}, "4, 2, 2"),
               "32x256": ({"VS_CONV_CFG": 2}, "2, 1, 4"), "32x256_nocfg": ({"VS_NO_SMALL_GRID": 1}, "2, 1, 4"), "32x128": ({}, "1, 1, 4")}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def mfma_instance(Cout):
    """choose_cfg of the fp32 engine on a short launch without VS_CONV_CFG"""
    MT = -(-Cout // 32)
    return "conv_mfma_kernel<%s>" % ("1, 4, 1, 4" if MT == 1 else "1, 8, 2, 2" if MT == 2 else "1, 4, 2, 2" if MT % 4 == 2 else "1, 8, 4, 1")


def conv_case(oracle, vs_option, math, opts, expect, Cin, Cout, T, k, du, in_act, *, tr=False, wn=False, res=False, acc=False, scale=1.0, out_act=None,
              out_mask=False, bias_b=False, inplace=False, seed=0, F=None, inputs=None, small_math=None):
    """one launch against the reference of arithmetic `math`.  opts: dispatch switches; expect: the instance name (or a predicate on it)"""
    from visinger_amd.ops import ConvOp, weightnorm_fold
    for name, v in opts.items():
        vs_option(name, v)
    r, x, w, bias, pad = R.conv_inputs(Cin, Cout, T, k, du, in_act, tr=tr, seed=seed)
    if inputs is not None:
        x, w, bias, pad = inputs
    op = ConvOp(L.CONV_TRANSPOSE1D if tr else L.CONV1D, Cin, Cout, k, du, pad).set_math(MATH[math] if small_math is None else small_math)
    if wn:
        v, g = dev(w * 3.0), dev(0.5 + r.random((w.shape[0], 1, 1)))
        op.set_weights(v, g, dev(bias))
        w = weightnorm_fold(v, g).cpu().numpy()          # the fp32 effective weight
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
               res=rt, acc=at, scale=scale, out_act=OUT_ACT[out_act], out_mask=out_mask)
    torch.cuda.synchronize()
    inst = op.kernel_instance()
    ref, S, bound = R.expected(oracle, math, x, w, bias, transposed=tr, dil_or_stride=du, padding=pad, lrelu=in_act in (L.IN_LRELU, L.IN_LRELU_MASK),
                               in_mask=mask if masked_in else None, bias_b=bb, res=rv, acc=av, scale=scale, out_act=out_act,
                               out_mask=mask if out_mask else None, F=F)
    assert y.shape == ref.shape
    what = f"{inst} {'tconv' if tr else 'conv'} {Cin}->{Cout} T{T} k{k} d{du} in{in_act}" + (f" {out_act}" if out_act else "") + (" omask" if out_mask else "")
    assert expect(inst) if callable(expect) else inst == expect, (what, expect)
    return R.assert_close(y, ref, S, what, bound=bound)


# ---- conv_mfma_kernel<1, NT_W, WAVES_M, WAVES_N>: all four tile shapes
@pytest.mark.parametrize("tile,Cin,Cout,T,k,d", R.MFMA_CASES)
def test_mfma_tile_kernel(oracle, vs_option, tile, Cin, Cout, T, k, d):
    opts, tail = MFMA_TILES[tile]
    for in_act, out_mask, res in R.tile_variants(k):
        conv_case(oracle, vs_option, "f32", opts, "conv_mfma_kernel<%s>" % tail, Cin, Cout, T, k, d, in_act, out_mask=out_mask, res=res)


# ---- conv_split_kernel<1, NT_W, WAVES_M, WAVES_N, 6>: split3_reference.TILE_CASES with their switches
@pytest.mark.parametrize("tile,Cin,Cout,T,k,d", R.S3.TILE_CASES)
def test_split6_tile_kernel(oracle, vs_option, tile, Cin, Cout, T, k, d):
    opts, tail = SPLIT_TILES[tile]
    for in_act, out_mask, res in R.tile_variants(k):
        conv_case(oracle, vs_option, "split6", opts, "conv_split_kernel<1, %s, 6>" % tail, Cin, Cout, T, k, d, in_act, out_mask=out_mask, res=res)


@pytest.mark.parametrize("tile", ["128x256", "32x128"])
def test_split6_under_channel_gains_and_outliers(oracle, vs_option, tile):
    """per-channel gains of 2^-6 .. 2^6 and outlier runs: the planes carry no scale, so the bound has no term for one (exact_reference: F_SPLIT6_GAIN, the same
    serial-chain measurement on this data)"""
    Cin, Cout, T, k, d = R.GAIN_CASE
    opts, tail = SPLIT_TILES[tile]
    conv_case(oracle, vs_option, "split6", opts, "conv_split_kernel<1, %s, 6>" % tail, Cin, Cout, T, k, d, L.IN_LRELU_MASK, out_mask=True,
              F=R.F_SPLIT6_GAIN, inputs=R.gain_inputs())


# ---- transposed convs
@pytest.mark.parametrize("Cin,Cout,k,u,T", R.TR_SHAPES)
def test_split6_transposed(oracle, vs_option, Cin, Cout, k, u, T):
    """polyphase transposed convs behind a leaky-relu, weight norm over the input channel, on the wide tiles and on whichever tile a short launch takes"""
    six = lambda inst: (inst.startswith("conv_split_tr_kernel<1, ") or inst.startswith("conv_split_kernel<1, ")) and inst.endswith(", 6>")
    conv_case(oracle, vs_option, "split6", {"VS_NO_SMALL_GRID": 1}, six, Cin, Cout, T, k, u, L.IN_LRELU, tr=True, wn=True)
    conv_case(oracle, vs_option, "split6", {}, six, Cin, Cout, T, k, u, L.IN_LRELU_MASK, tr=True)


def test_f32_transposed(oracle, vs_option):
    Cin, Cout, k, u, T = R.TR_F32
    conv_case(oracle, vs_option, "f32", NW, lambda inst: inst.startswith("conv_mfma_kernel<1, "), Cin, Cout, T, k, u, L.IN_LRELU, tr=True, wn=True)


# ---- paired kinds: conv_mfma_kernel<2, 2, 2, 2> / <2, 2, 1, 4> and conv_split_kernel<2, 2, 2, 2, 6> / <2, 2, 1, 4, 6>
@pytest.mark.parametrize("mode", ["gate", "coupling_fwd", "coupling_inv"])
@pytest.mark.parametrize("math", ["f32", "split6"])
@pytest.mark.parametrize("H,Cin,T,k,d,tile", R.PAIR_TILES, ids=[p[5] for p in R.PAIR_TILES])
def test_paired_kinds(oracle, vs_option, H, Cin, T, k, d, tile, math, mode):
    """VS_CONV1D_PAIRED: the WaveNet gate and the affine coupling update (forward with its log-determinant, inverse) under the mask.  The bounds of
    tests/test_conv_split3_oracle_gpu.py::test_paired_kinds with this arithmetic's F: delta = F * 2^-24 * S per pre-activation carried through the expression's
    first derivative (delta <= 1e-5: the second-order term is below 1e-10 of the output), plus the fp32 evaluation of the expression itself -- expf and the
    division at <= 2^-22 relative, tanh_fast at <= 1e-7 absolute, the products at 2^-24 each: 2^-21 of the largest factor product."""
    from visinger_amd.ops import ConvOp
    vs_option("VS_NO_KTAP", 1)
    tail = "2, 2, 1, 4" if tile == "64x256" else "2, 2, 2, 2"
    expect = "conv_mfma_kernel<%s>" % tail if math == "f32" else "conv_split_kernel<%s, 6>" % tail
    F = R.F_OF[math]
    r = np.random.default_rng(H + T + k)
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    w = ((1.0 if mode == "gate" else 0.5) * r.standard_normal((2 * H, Cin, k)) / np.sqrt(Cin * k)).astype(np.float32)
    bias = ((1.0 if mode == "gate" else 0.1) * r.standard_normal(2 * H)).astype(np.float32)
    pad = d * (k - 1) // 2
    op = ConvOp(L.CONV1D_PAIRED, Cin, 2 * H, k, d, pad).set_math(MATH[math])
    op.set_weights(dev(w), None, dev(bias))
    mask = R.ragged_mask(B, T)
    EV = 2.0 ** -21
    if mode == "gate":
        gl = r.standard_normal((B, 2 * H)).astype(np.float32)
        pre, S = R.expected_pre(oracle, math, x, w, bias, dil_or_stride=d, padding=pad, bias_b=gl)
        delta = F * R.EPS32 * S
        ta, sb = np.tanh(pre[:, :H]), oracle.sigmoid(pre[:, H:])
        ref = ta * sb
        bound = sb * (1.0 - ta * ta) * delta[:, :H] + np.abs(ta) * sb * (1.0 - sb) * delta[:, H:] + EV * sb
        y = op.forward(dev(x), bias_b=dev(gl), pair_mode=L.PAIR_GATE)
    else:
        x1 = r.standard_normal((B, H, T)).astype(np.float32)
        stats, S = R.expected_pre(oracle, math, x, w, bias, dil_or_stride=d, padding=pad)
        m3 = mask[:, None].astype(np.float64)
        stats, delta = stats * m3, F * R.EPS32 * S * m3
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
    print("EXACTREF   of_bound %.3f" % float((np.abs(R.to_np(y) - ref) / np.maximum(bound, 1e-300))[bound > 0].max()))


# ---- one fp32 launch each of the fused options and the other conv kinds
def test_f32_weightnorm_residual_accumulate_scale_in_place_and_tanh(oracle, vs_option):
    Cin, Cout, T, k, d = R.FUSED_CASE
    expect = mfma_instance(Cout)
    conv_case(oracle, vs_option, "f32", NW, expect, Cin, Cout, T, k, d, L.IN_LRELU, wn=True, res=True, acc=True, scale=1.0 / 3.0, inplace=True)
    conv_case(oracle, vs_option, "f32", NW, expect, Cin, Cout, T, k, d, L.IN_LRELU, wn=True, acc=True, inplace=True, out_act="tanh")


def test_f32_relu_output_mask_and_per_item_bias(oracle, vs_option):
    Cin, Cout, T, k, d = R.RELU_CASE
    conv_case(oracle, vs_option, "f32", NW, mfma_instance(Cout), Cin, Cout, T, k, d, L.IN_MASK, bias_b=True, out_act="relu", out_mask=True)


@pytest.mark.parametrize("H", [32, 16], ids=["on_tile_edge", "inside_tile"])
def test_f32_split_row(oracle, vs_option, H):
    """the WaveNet's res / skip 1 x 1 conv with its two destinations: split_row on a 32-row tile edge (one launch) and inside a tile (two passes)"""
    from visinger_amd.ops import ConvOp
    vs_option("VS_NO_WINO", 1)
    r = np.random.default_rng(H)
    T = 137
    acts, x, out = (r.standard_normal((B, H, T)).astype(np.float32) for _ in range(3))
    w = (r.standard_normal((2 * H, H, 1)) / np.sqrt(H)).astype(np.float32)
    bias = r.standard_normal(2 * H).astype(np.float32)
    mask = R.ragged_mask(B, T)
    op = ConvOp(L.CONV1D, H, 2 * H, 1, 1, 0).set_math(L.MATH_F32)
    op.set_weights(dev(w), None, dev(bias))
    xt, ot = dev(x), dev(out)
    op.forward(dev(acts), y=xt, res=xt, out_mask=True, mask=dev(mask), split_row=H, out1=dict(y=ot, acc=ot))
    torch.cuda.synchronize()
    expect = mfma_instance(2 * H)
    assert op.kernel_instance() == expect, op.kernel_instance()
    rs, S = R.expected_pre(oracle, "f32", acts, w, bias)
    what = f"{expect} split_row {H}"
    S0 = S[:, :H] + np.abs(x)
    R.assert_close(xt, (x + rs[:, :H]) * mask[:, None], S0, what + " rows < split", bound=R.F_DIRECT * R.EPS32 * S0 * mask[:, None])
    R.assert_close(ot, out + rs[:, H:], S[:, H:] + np.abs(out), what + " rows >= split", F=R.F_DIRECT)


def test_f32_flip_in_and_channel_window(oracle, vs_option):
    """the coupling layer's `pre` conv reading the logical x0 half from the physical tensor (upper half, reversed)"""
    from visinger_amd.ops import ConvOp, _off
    vs_option("VS_NO_WINO", 1)
    r = np.random.default_rng(21)
    half, H, T = 48, 64, 130
    C = 2 * half
    xfull = r.standard_normal((B, C, T)).astype(np.float32)
    w = (r.standard_normal((H, half, 1)) / np.sqrt(half)).astype(np.float32)
    bias = r.standard_normal(H).astype(np.float32)
    mask = R.ragged_mask(B, T)
    op = ConvOp(L.CONV1D, half, H, 1, 1, 0, L.FLIP_IN).set_math(L.MATH_F32)
    op.set_weights(dev(w), None, dev(bias))
    xt = dev(xfull)
    y = torch.empty(B, H, T, device="cuda")
    op.forward(None, B=B, T=T, x_ptr=_off(xt, half * T), x_bs=C * T, y=y, mask=dev(mask), out_mask=True)
    torch.cuda.synchronize()
    expect = mfma_instance(H)
    assert op.kernel_instance() == expect, op.kernel_instance()
    ref, S, bound = R.expected(oracle, "f32", np.ascontiguousarray(xfull[:, ::-1][:, :half]), w, bias, out_mask=mask)
    R.assert_close(y, ref, S, expect + " flip-in, channel window", bound=bound)


def test_f32_adjoint_handle(oracle, vs_option):
    """VS_CONV_ADJOINT: the grad-input conv of a forward conv, packed from the FORWARD weight; its reference is the conv with the channel-transposed, tap-reversed
    weight"""
    from visinger_amd.ops import ConvOp
    vs_option("VS_NO_WINO", 1)
    cf_out, cf_in, T, k, _ = R.ADJ_CASE                # the forward conv: 96 -> 48; its grad-input: 48 -> 96
    r = np.random.default_rng(50 + k)
    wf = (r.standard_normal((cf_out, cf_in, k)) / np.sqrt(cf_out * k)).astype(np.float32)
    gy = r.standard_normal((B, cf_out, T)).astype(np.float32)
    pad = (k - 1) // 2
    adj = ConvOp(L.CONV1D, cf_out, cf_in, k, 1, (k - 1) - pad, L.CONV_ADJOINT).set_math(L.MATH_F32)
    adj.set_weights(dev(wf), None, None)
    y = adj.forward(dev(gy))
    torch.cuda.synchronize()
    expect = mfma_instance(cf_in)
    assert adj.kernel_instance() == expect, adj.kernel_instance()
    wa = np.ascontiguousarray(wf.transpose(1, 0, 2)[:, :, ::-1])
    ref, S, bound = R.expected(oracle, "f32", gy, wa, None, padding=(k - 1) - pad)
    R.assert_close(y, ref, S, f"{expect} adjoint k{k}", bound=bound)


# ---- conv_wino_kernel<D, WM, WN, TG, TT> under VS_WINO_FORCE: all 22 instances (exact_reference.WINO_INSTANCES: the table covers exactly that set)
@pytest.mark.parametrize("Cin,Cout,k,d", R.WINO_CASES, ids=["%s_%d-%d_k%d" % ((R.wino_instance(c[1], c[2], c[3])[17:-1].replace(", ", "."),) + c[:3]) for c in R.WINO_CASES])
def test_wino_instances(oracle, vs_option, Cin, Cout, k, d):
    """each instance at a T one block plus a remainder off the float4 grid, a T on it and a T shorter than the receptive span; behind leaky-relu and leaky-relu +
    mask, with residual / accumulate / scale, with tanh + output mask (exact_reference.wino_launches)"""
    expect = R.wino_instance(Cout, k, d)
    assert expect in R.WINO_INSTANCES
    for T, in_act, res, acc, scale, out_act, out_mask in R.wino_launches(Cout, k, d):
        conv_case(oracle, vs_option, "wino", {"VS_WINO_FORCE": 1}, expect, Cin, Cout, T, k, d, in_act, res=res, acc=acc, scale=scale, out_act=out_act, out_mask=out_mask)


# ---- the fused residual pairs respair_kernel<1, 4> / <2, 2> and respair_split_kernel<2, 1, 4 | 2, 2, 6, false>
@pytest.mark.parametrize("math", ["f32", "split6"])
@pytest.mark.parametrize("C,k,d,T", R.PAIR_CASES)
def test_fused_residual_pair(oracle, math, C, k, d, T):
    """y = conv2(lrelu(conv1(lrelu(x)) + b1)) + b2 + x [+ acc] [* scale] in one launch, every (k, dilation) of the MRF blocks; T in the interior, at both
    sequence ends, below one tile and not a multiple of 4; the accumulate input with scale 1 / 3, in place.  The propagated bound of exact_reference.pair_expected"""
    from visinger_amd.ops import ConvOp, respair_forward, respair_supported
    x, w1, b1, w2, b2, accb = R.pair_inputs(C, k, d, T)
    op1 = ConvOp(L.CONV1D, C, C, k, d, d * (k - 1) // 2).set_math(MATH[math])
    op2 = ConvOp(L.CONV1D, C, C, k, 1, (k - 1) // 2).set_math(MATH[math])
    op1.set_weights(dev(w1), None, dev(b1))
    op2.set_weights(dev(w2), None, dev(b2))
    assert respair_supported(op1, op2)
    if math == "f32":
        expect = "respair_kernel<%s>" % ("1, 4" if C == 32 else "2, 2")
    else:
        expect = "respair_split_kernel<%s, 6, false>" % ("2, 1, 4" if C == 32 else "2, 2, 2")
    xd = dev(x)
    y = respair_forward(op1, op2, xd, torch.empty_like(xd), res=xd)
    torch.cuda.synchronize()
    assert op1.kernel_instance() == expect, op1.kernel_instance()
    what = f"{expect} C{C} k{k} d{d} T{T}"
    ref, bound, _ = R.pair_expected(oracle, math, x, w1, b1, w2, b2, k=k, d=d, res=x)
    R.assert_close(y, ref, None, what, bound=bound)
    print("EXACTREF   of_bound %.3f" % float((np.abs(R.to_np(y) - ref) / bound).max()))
    acc_t = dev(accb)
    respair_forward(op1, op2, xd, acc_t, res=xd, acc=acc_t, scale=1.0 / 3.0)             # in-place accumulate, MRF average
    torch.cuda.synchronize()
    ref, bound, _ = R.pair_expected(oracle, math, x, w1, b1, w2, b2, k=k, d=d, res=x, acc=accb, scale=1.0 / 3.0)
    R.assert_close(acc_t, ref, None, what + " acc scale", bound=bound)
    print("EXACTREF   of_bound %.3f" % float((np.abs(R.to_np(acc_t) - ref) / bound).max()))


# ---- conv_small_kernel: the VALU conv for C_out <= 4, whatever the handle's arithmetic
@pytest.mark.parametrize("Cin,Cout,T,k,in_act,out_act", R.SMALL_CASES)
def test_small_conv(oracle, vs_option, Cin, Cout, T, k, in_act, out_act):
    """conv_post (32 -> 1, k = 7, tanh output) and C_out in {2, 4} behind mask and leaky-relu, T in {1, 7, 900}: the fp64 conv of the fp32 operands, F_DIRECT"""
    want = "conv_small_kernel<%d, " % (4 if Cout > 2 else Cout)
    tail = "7, 3>" if (k == 7 and T % 4 == 0) else ("1, 0>" if (k == 1 and T % 4 == 0) else "0, 0>")
    for m in (L.MATH_SPLIT3, L.MATH_F32, L.MATH_SPLIT6):
        conv_case(oracle, vs_option, "f32", {}, want + tail, Cin, Cout, T, k, 1, in_act, out_act=out_act, out_mask=in_act in (L.IN_MASK, L.IN_LRELU_MASK),
                  bias_b=Cout == 2, small_math=m)
