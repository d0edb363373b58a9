"""Every plain-bf16 (VS_MATH_BF16) conv instance, element by element, against the oracle on bf16-rounded operands (tests/bf16_reference.py):
|got - ref| <= 2e-5 * (1 + |ref|), the bound the exact-fp32 engine is held to in tests/test_conv_gpu.py -- with both operands of every product
rounded the way the device rounds them, a product is exact in fp32 and only the order of the fp32 sums is left.  The other tests of these
kernels are rms bounds of 6e-3 .. 5e-2 (which a dropped product passes, tests/test_bf16_reference_cpu.py) or kernel against kernel (which a
defect in the shared staging code passes).  Each case names the instance it must reach (vs_last_kernel_name); B = 2 with a ragged mask.
Every assert_close prints `BF16REF <instance> <case>: scaled <|err| / (2e-5 (1 + |ref|))> per_S <|err| / (2^-24 * sum |products|)>`."""
import numpy as np
import pytest
import torch

import bf16_reference as R
from visinger_amd import _lib as L

pytestmark = pytest.mark.gpu

B = 2
OUT_ACT = {L.OUT_NONE: None, L.OUT_TANH: "tanh", L.OUT_RELU: "relu"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def bf(a):
    """-> (bf16 CUDA tensor, its values as a float32 array)"""
    t = dev(a).bfloat16()
    return t, t.float().cpu().numpy()


def conv_case(oracle, vs_option, opts, expect, Cin, Cout, T, k, du, in_act, *, tr=False, wn=False, res=False, acc=False, scale=1.0,
              out_act=L.OUT_NONE, out_mask=False, bias_b=False, io=0, inplace=False, seed=0):
    """one launch of a plain-bf16 conv against the reference.  opts: dispatch switches; expect: the instance name; io: bit 0 -- x, bit 1 -- y / res / acc
    bf16-resident.  The reference rounds the operands unless the launch went to the VALU instance of C_out <= 4, which keeps fp32 operands."""
    from visinger_amd.ops import ConvOp, weightnorm_fold
    for name, v in opts.items():
        vs_option(name, v)
    r = np.random.default_rng(1000 * Cin + 10 * Cout + T + 7 * k + du + in_act + seed)
    pad = (k - du) // 2 if tr else du * (k - 1) // 2
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    wshape = (Cin, Cout, k) if tr else (Cout, Cin, k)
    w = (r.standard_normal(wshape) / np.sqrt(Cin * k / (du if tr else 1))).astype(np.float32)
    bias = r.standard_normal(Cout).astype(np.float32)
    op = ConvOp(L.CONV_TRANSPOSE1D if tr else L.CONV1D, Cin, Cout, k, du, pad).set_math(L.MATH_BF16)
    if wn:
        v, g = dev(w * 3.0), dev(0.5 + r.random((wshape[0], 1, 1)))
        op.set_weights(v, g, dev(bias))
        w = weightnorm_fold(v, g).cpu().numpy()          # the fp32 effective weight the library rounds
    else:
        op.set_weights(dev(w), None, dev(bias))
    Tout = op.out_len(T)
    mask = R.ragged_mask(B, T)
    masked_in = in_act in (L.IN_MASK, L.IN_LRELU_MASK)
    xt, xv = bf(x) if io & 1 else (dev(x), x)
    ydt = torch.bfloat16 if io & 2 else torch.float32
    conv = lambda a: bf(a) if io & 2 else (dev(a), a)
    rt, rv = conv(r.standard_normal((B, Cout, Tout)).astype(np.float32)) if res else (None, None)
    at, av = conv(r.standard_normal((B, Cout, Tout)).astype(np.float32)) if acc else (None, None)
    bb = r.standard_normal((B, Cout)).astype(np.float32) if bias_b else None
    y = at if inplace else torch.empty((B, Cout, Tout), device="cuda", dtype=ydt)
    op.forward(xt, y=y, in_act=in_act, mask=dev(mask) if (masked_in or out_mask) else None, bias_b=None if bb is None else dev(bb),
               res=rt, acc=at, scale=scale, out_act=out_act, out_mask=out_mask)
    torch.cuda.synchronize()
    inst = op.kernel_instance()
    assert expect(inst) if callable(expect) else inst == expect, (inst, expect)
    ref, S = R.expected(oracle, xv, w, bias, transposed=tr, dil_or_stride=du, padding=pad, lrelu=in_act in (L.IN_LRELU, L.IN_LRELU_MASK),
                        in_mask=mask if masked_in else None, bias_b=bb, rounded=not inst.startswith("conv_small_kernel"),
                        res=rv, acc=av, scale=scale, out_act=OUT_ACT[out_act], out_mask=mask if out_mask else None)
    what = f"{inst} {'tconv' if tr else 'conv'} {Cin}->{Cout} T{T} k{k} d{du} in{in_act} io{io}"
    return R.assert_close(y, ref, bf16_out=bool(io & 2), S=S, what=what)


# ---- the tile kernel conv_split_kernel<1, NT_W, WAVES_M, WAVES_N, 1>: all four tile shapes; C_in off the 16-channel chunk (33, 200, 40), C_out off the 32-row
# tile (20, 70, 136), T one past a column tile (129: the 128-column tile; 257, 261: the 256-column ones), T in {1, 2, 5}, halos wider than the sequence
# (k = 5 at dilation 3 / 5 on T <= 5), k in {1, 4, 5}, dilations 2, 3, 5
T8 = ({"VS_NO_KTAP": 1, "VS_NO_SMALL_GRID": 1}, "conv_split_kernel<1, 8, 4, 1, 1>", "128x256")
T4 = ({"VS_NO_KTAP": 1, "VS_CONV_CFG": 3}, "conv_split_kernel<1, 4, 2, 2, 1>", "64x256")
T2 = ({"VS_NO_KTAP": 1, "VS_CONV_CFG": 2}, "conv_split_kernel<1, 2, 1, 4, 1>", "32x256")
T1 = ({"VS_NO_KTAP": 1}, "conv_split_kernel<1, 1, 1, 4, 1>", "32x128")           # what a short launch takes by itself
TILE_CASES = [
    # tile, C_in, C_out, T, k, dilation
    (T8, 33, 70, 257, 5, 2), (T8, 200, 136, 261, 1, 1), (T8, 40, 136, 5, 5, 3), (T8, 16, 70, 2, 4, 1), (T8, 64, 96, 129, 5, 5), (T8, 33, 70, 1, 5, 1),
    (T4, 33, 70, 261, 5, 3), (T4, 200, 136, 129, 4, 1), (T4, 16, 70, 1, 5, 2), (T4, 40, 136, 257, 1, 1), (T4, 48, 96, 5, 5, 5),
    (({"VS_NO_KTAP": 1, "VS_NO_SMALL_GRID": 1}, T4[1], "64x256_nocfg"), 40, 64, 257, 5, 2),                # two row tiles: this shape without VS_CONV_CFG
    (T2, 33, 20, 257, 5, 2), (T2, 200, 136, 261, 4, 1), (T2, 48, 70, 2, 5, 5), (T2, 16, 20, 5, 1, 1), (T2, 33, 70, 1, 5, 3),
    (({"VS_NO_KTAP": 1, "VS_NO_SMALL_GRID": 1}, T2[1], "32x256_nocfg"), 33, 20, 129, 5, 3),                # one row tile: likewise
    (T1, 33, 20, 129, 5, 3), (T1, 200, 70, 261, 1, 1), (T1, 64, 136, 257, 4, 1), (T1, 16, 20, 1, 5, 1), (T1, 40, 136, 5, 5, 2), (T1, 200, 20, 2, 1, 1),
]


@pytest.mark.parametrize("tile,Cin,Cout,T,k,d", TILE_CASES, ids=lambda v: v[2] if isinstance(v, tuple) else None)
def test_tile_kernel(oracle, vs_option, tile, Cin, Cout, T, k, d):
    opts, expect, _ = tile
    conv_case(oracle, vs_option, opts, expect, Cin, Cout, T, k, d, L.IN_NONE)
    conv_case(oracle, vs_option, opts, expect, Cin, Cout, T, k, d, L.IN_LRELU_MASK, out_mask=(k % 2 == 1))
    conv_case(oracle, vs_option, opts, expect, Cin, Cout, T, k, d, L.IN_LRELU if k > 1 else L.IN_MASK, res=True)


# ---- conv_ktap_kernel<taps, transform, 1 plane, tensors, WAVES_M, WAVES_N, NT, MT_W>: C_in % 16 == 0
K8 = ({"VS_NO_SMALL_GRID": 1}, "conv_ktap_kernel<%d, %d, 1, 0, 4, 1, 8, 1>", "128x256")
K4 = ({"VS_CONV_CFG": 3}, "conv_ktap_kernel<%d, %d, 1, 0, 2, 2, 4, 1>", "64x256")
K1 = ({}, "conv_ktap_kernel<%d, %d, 1, 0, 1, 4, 1, 1>", "32x128")
KTAP_CASES = [(K8, 7, 3, a) for a in (L.IN_NONE, L.IN_LRELU, L.IN_MASK, L.IN_LRELU_MASK)] + \
             [(K8, k, 1, a) for k in (1, 9) for a in (L.IN_NONE, L.IN_MASK)] + \
             [(K8, k, d, a) for k, d in ((3, 2), (11, 5)) for a in (L.IN_LRELU, L.IN_LRELU_MASK)] + \
             [(tile, k, 1, a) for tile in (K4, K1) for k in (1, 9) for a in (L.IN_NONE, L.IN_MASK)]


@pytest.mark.parametrize("tile,k,d,in_act", KTAP_CASES, ids=lambda v: v[2] if isinstance(v, tuple) else None)
def test_ktap_instances(oracle, vs_option, tile, k, d, in_act):
    opts, expect, _ = tile
    T = 129 if tile is K1 else 261
    conv_case(oracle, vs_option, opts, expect % (k, in_act), 48, 96, T, k, d, in_act, out_mask=in_act >= L.IN_MASK)
    conv_case(oracle, vs_option, opts, expect % (k, in_act), 32, 136, T + 40, k, d, in_act, res=True, bias_b=True)


def test_masked_launch_without_an_instance_on_its_tile_takes_another(oracle, vs_option):
    """plain bf16 behind a masked input transform: a launch whose chosen tile shape has no conv_ktap instance takes another shape that has one"""
    # 32 x 128 chosen (a short launch), no 7-tap instance there or on 64 x 256: the 128 x 256 tile
    conv_case(oracle, vs_option, {}, "conv_ktap_kernel<7, 3, 1, 0, 4, 1, 8, 1>", 32, 96, 261, 7, 3, L.IN_LRELU_MASK, out_mask=True)
    # 32 x 256 forced, which has no instance at all: the 64 x 256 tile
    conv_case(oracle, vs_option, {"VS_CONV_CFG": 2}, "conv_ktap_kernel<9, 2, 1, 0, 2, 2, 4, 1>", 48, 96, 261, 9, 1, L.IN_MASK, out_mask=True)


# ---- fused options, as tests/test_conv_gpu.py exercises them in the default arithmetic
def test_weightnorm_residual_accumulate_scale_in_place_and_tanh(oracle, vs_option):
    name = "conv_split_kernel<1, 4, 2, 2, 1>"
    conv_case(oracle, vs_option, {}, name, 64, 64, 333, 7, 3, L.IN_LRELU, wn=True, res=True, acc=True, scale=1.0 / 3.0)
    conv_case(oracle, vs_option, {}, name, 64, 64, 333, 7, 3, L.IN_LRELU, wn=True, res=True, acc=True, scale=1.0 / 3.0, inplace=True)
    conv_case(oracle, vs_option, {}, name, 64, 64, 333, 7, 3, L.IN_LRELU, wn=True, acc=True, inplace=True, out_act=L.OUT_TANH)


def test_relu_output_mask_and_per_item_bias(oracle, vs_option):
    conv_case(oracle, vs_option, {}, "conv_ktap_kernel<9, 2, 1, 0, 1, 4, 1, 1>", 48, 96, 211, 9, 1, L.IN_MASK, bias_b=True, out_act=L.OUT_RELU, out_mask=True)
    conv_case(oracle, vs_option, {"VS_NO_KTAP": 1}, "conv_split_kernel<1, 1, 1, 4, 1>", 48, 96, 211, 9, 1, L.IN_MASK, bias_b=True, out_act=L.OUT_RELU, out_mask=True)


def test_small_c_out_instance_keeps_fp32_operands(oracle, vs_option):
    """C_out <= 4 runs conv_small_kernel (VALU, fp32 weights and activations in every arithmetic): its reference is the un-rounded oracle"""
    conv_case(oracle, vs_option, {}, "conv_small_kernel<1, 7, 3>", 32, 1, 300, 7, 1, L.IN_LRELU, out_act=L.OUT_TANH)
    conv_case(oracle, vs_option, {}, "conv_small_kernel<2, 0, 0>", 192, 2, 131, 3, 1, L.IN_MASK, out_mask=True)
    conv_case(oracle, vs_option, {}, "conv_small_kernel<4, 1, 0>", 40, 3, 132, 1, 1, L.IN_NONE)


def test_single_frame_1x1_instance(oracle, vs_option):
    conv_case(oracle, vs_option, {}, "conv_t1_kernel", 200, 70, 1, 1, 1, L.IN_NONE, bias_b=True, scale=0.5)


@pytest.mark.parametrize("H,expect", [(32, "conv_ktap_kernel<1, 0, 1, 0, 2, 2, 4, 1>"), (16, "conv_split_kernel<1, 1, 1, 4, 1>")], ids=["32", "16"])
def test_split_row(oracle, H, expect):
    """the WaveNet's res / skip 1 x 1 conv with its two destinations: split_row on a 32-row tile edge (one launch) and inside a tile (two passes)"""
    from visinger_amd.ops import ConvOp
    r = np.random.default_rng(H)
    T = 137
    acts, x, out = (r.standard_normal((B, H, T)).astype(np.float32) for _ in range(3))
    w = (r.standard_normal((2 * H, H, 1)) / np.sqrt(H)).astype(np.float32)
    bias = r.standard_normal(2 * H).astype(np.float32)
    mask = R.ragged_mask(B, T)
    op = ConvOp(L.CONV1D, H, 2 * H, 1, 1, 0).set_math(L.MATH_BF16)
    op.set_weights(dev(w), None, dev(bias))
    xt, ot = dev(x), dev(out)
    op.forward(dev(acts), y=xt, res=xt, out_mask=True, mask=dev(mask), split_row=H, out1=dict(y=ot, acc=ot))
    assert op.kernel_instance() == expect, op.kernel_instance()
    rs, S = R.expected_pre(oracle, acts, w, bias)
    what = f"{expect} split_row {H}"
    R.assert_close(xt, (x + rs[:, :H]) * mask[:, None], S=S[:, :H] + np.abs(x), what=what + " rows < split")
    R.assert_close(ot, out + rs[:, H:], S=S[:, H:] + np.abs(out), what=what + " rows >= split")


def test_flip_in_and_channel_window(oracle):
    """the coupling layer's `pre` conv reading the logical x0 half from the physical tensor (upper half, reversed)"""
    from visinger_amd.ops import ConvOp, _off
    r = np.random.default_rng(21)
    half, H, T = 48, 64, 130
    C = 2 * half
    xfull = r.standard_normal((B, C, T)).astype(np.float32)
    w = (r.standard_normal((H, half, 1)) / np.sqrt(half)).astype(np.float32)
    bias = r.standard_normal(H).astype(np.float32)
    mask = R.ragged_mask(B, T)
    op = ConvOp(L.CONV1D, half, H, 1, 1, 0, L.FLIP_IN).set_math(L.MATH_BF16)
    op.set_weights(dev(w), None, dev(bias))
    xt = dev(xfull)
    y = torch.empty(B, H, T, device="cuda")
    op.forward(None, B=B, T=T, x_ptr=_off(xt, half * T), x_bs=C * T, y=y, mask=dev(mask), out_mask=True)
    assert op.kernel_instance() == "conv_ktap_kernel<1, 0, 1, 0, 2, 2, 4, 1>", op.kernel_instance()
    ref, S = R.expected(oracle, np.ascontiguousarray(xfull[:, ::-1][:, :half]), w, bias, out_mask=mask)
    R.assert_close(y, ref, S=S, what=op.kernel_instance() + " flip-in, channel window")


PAIR_TILES = [
    # H, C_in, T, k, dilation, switches, instance: both tile shapes of the tile kernel and the k = 5 conv_ktap pair instance
    (64, 64, 140, 5, 1, {}, "conv_ktap_kernel<5, 0, 1, 0, 2, 2, 2, 2>"),
    (64, 64, 140, 5, 1, {"VS_NO_KTAP": 1}, "conv_split_kernel<2, 2, 2, 2, 1>"),
    (40, 24, 70, 3, 2, {}, "conv_split_kernel<2, 2, 2, 2, 1>"),
    (16, 16, 37, 5, 1, {}, "conv_split_kernel<2, 2, 1, 4, 1>"),
]


@pytest.mark.parametrize("mode", ["gate", "coupling_fwd", "coupling_inv"])
@pytest.mark.parametrize("H,Cin,T,k,d,opts,expect", PAIR_TILES, ids=["ktap_pair", "128x128", "128x128_k3", "64x256"])
def test_paired_kinds(oracle, vs_option, H, Cin, T, k, d, opts, expect, mode):
    """VS_CONV1D_PAIRED: the WaveNet gate tanh(a) * sigmoid(b) over the row pair (c, H + c) with the conditioning as a per-item bias, and the affine coupling
    update x1' = m + x1 * exp(logs) (with its log-determinant) / x1' = (x1 - m) * exp(-logs), under the mask"""
    from visinger_amd.ops import ConvOp
    for name, v in opts.items():
        vs_option(name, v)
    r = np.random.default_rng(H + T + k)
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    gain = 1.0 if mode == "gate" else 0.5
    w = (gain * r.standard_normal((2 * H, Cin, k)) / np.sqrt(Cin * k)).astype(np.float32)
    bias = ((1.0 if mode == "gate" else 0.1) * r.standard_normal(2 * H)).astype(np.float32)
    pad = d * (k - 1) // 2
    op = ConvOp(L.CONV1D_PAIRED, Cin, 2 * H, k, d, pad).set_math(L.MATH_BF16)
    op.set_weights(dev(w), None, dev(bias))
    mask = R.ragged_mask(B, T)
    if mode == "gate":
        gl = r.standard_normal((B, 2 * H)).astype(np.float32)
        pre, _ = R.expected_pre(oracle, x, w, bias, dil_or_stride=d, padding=pad, bias_b=gl)
        ref = np.tanh(pre[:, :H]) * oracle.sigmoid(pre[:, H:])
        y = op.forward(dev(x), bias_b=dev(gl), pair_mode=L.PAIR_GATE)
    else:
        x1 = r.standard_normal((B, H, T)).astype(np.float32)
        stats, _ = R.expected_pre(oracle, x, w, bias, dil_or_stride=d, padding=pad)
        stats = stats * mask[:, None]
        m, logs = stats[:, :H], stats[:, H:]
        ld = torch.zeros(B, device="cuda")
        if mode == "coupling_fwd":
            ref = m + x1 * np.exp(logs) * mask[:, None]
            y = op.forward(dev(x), mask=dev(mask), res=dev(x1), pair_mode=L.PAIR_COUPLING_FWD, logdet=ld)
            ref_ld = logs.sum(axis=(1, 2))
            assert np.abs(ld.cpu().double().numpy() - ref_ld).max() <= 1e-4 * np.abs(ref_ld).max()
        else:
            ref = (x1 - m) * np.exp(-logs) * mask[:, None]
            y = op.forward(dev(x), mask=dev(mask), res=dev(x1), pair_mode=L.PAIR_COUPLING_INV)
    assert op.kernel_instance() == expect, op.kernel_instance()
    assert y.shape == (B, H, T)
    R.assert_close(y, ref, what=f"{expect} {mode} H{H} {Cin} T{T} k{k} d{d}")


TR_SHAPES = [(64, 32, 16, 8, 40), (32, 32, 4, 2, 300), (48, 24, 11, 5, 33), (32, 16, 7, 3, 50), (512, 256, 16, 8, 16), (10, 6, 8, 4, 13),
             (48, 32, 11, 5, 159), (128, 64, 7, 3, 40)]          # the shapes of tests/test_conv_gpu.py::test_conv_transpose1d


@pytest.mark.parametrize("Cin,Cout,k,u,T", TR_SHAPES)
def test_transposed(oracle, vs_option, Cin, Cout, k, u, T):
    """polyphase transposed convs behind a leaky-relu, weight norm over the input channel, on fp32 tensors"""
    name = lambda inst: inst.startswith("conv_split_kernel<1, ") and inst.endswith(", 1>")        # (whichever tile the launch size takes)
    conv_case(oracle, vs_option, {}, name, Cin, Cout, T, k, u, L.IN_LRELU, tr=True, wn=True)
    conv_case(oracle, vs_option, {}, name, Cin, Cout, T, k, u, L.IN_LRELU_MASK, tr=True)


# ---- bf16-RESIDENT tensors, held directly to the reference: the output is rounded once, half a bf16 ulp at ref on top of the bound
@pytest.mark.parametrize("io", [1, 2, 3])
def test_bf16_resident_tile_kernel(oracle, vs_option, io):
    name = "conv_split_kernel_bf16io<1, 8, 4, 1, 1, %d>" % io
    conv_case(oracle, vs_option, {}, name, 40, 128, 261, 5, 2, L.IN_LRELU, io=io)
    conv_case(oracle, vs_option, {}, name, 40, 136, 300, 5, 1, L.IN_LRELU_MASK, io=io, bias_b=True, out_mask=True)
    if io != 1:
        conv_case(oracle, vs_option, {}, name, 33, 128, 257, 3, 3, L.IN_LRELU, io=io, res=(io == 3), acc=(io == 3), scale=1.0 / 3.0, out_act=L.OUT_RELU)
    if io == 3:             # bf16 in AND out also on the narrow tiles
        conv_case(oracle, vs_option, {}, "conv_split_kernel_bf16io<1, 4, 2, 2, 1, 3>", 40, 64, 261, 5, 2, L.IN_LRELU, io=3, res=True)
        conv_case(oracle, vs_option, {}, "conv_split_kernel_bf16io<1, 2, 1, 4, 1, 3>", 33, 32, 257, 7, 1, L.IN_LRELU, io=3, res=True)


@pytest.mark.parametrize("Cin,Cout,k,u,T,tile", [(64, 32, 16, 8, 40, "8, 4, 1"), (128, 64, 7, 3, 40, "4, 2, 2"), (128, 64, 4, 2, 515, "8, 4, 1")],
                         ids=["64-32_k16_u8", "128-64_k7_u3", "128-64_k4_u2"])
def test_bf16_resident_transposed(oracle, vs_option, Cin, Cout, k, u, T, tile):
    conv_case(oracle, vs_option, {}, "conv_split_tr_kernel_bf16io<1, %s, 1, 3>" % tile, Cin, Cout, T, k, u, L.IN_LRELU, tr=True, io=3)


@pytest.mark.parametrize("k,d", [(3, 1), (7, 3), (11, 5)])
def test_bf16_resident_ktap(oracle, vs_option, k, d):
    conv_case(oracle, vs_option, {}, "conv_ktap_kernel<%d, 1, 1, 3, 4, 1, 8, 1>" % k, 32, 128, 261, k, d, L.IN_LRELU, io=3, res=True)
    conv_case(oracle, vs_option, {}, "conv_ktap_kernel<%d, 3, 1, 3, 4, 1, 8, 1>" % k, 48, 128, 300, k, d, L.IN_LRELU_MASK, io=3, res=True, acc=True,
              scale=1.0 / 3.0, out_mask=True)


# ---- the fused residual pair respair_split_kernel<..., 1, PB>
@pytest.mark.parametrize("C,k,d,T", R.PAIR_CASES)
def test_fused_residual_pair(oracle, C, k, d, T):
    """y = conv2(lrelu(conv1(lrelu(x)) + b1)) + b2 + x [+ acc] [* scale] in one launch, the intermediate rounded to bf16 inside it: the same bound, plus -- exactly --
    what the intermediate elements on a rounding boundary can move (bf16_reference.pair_expected), on fp32 and on bf16-resident tensors"""
    from visinger_amd.ops import ConvOp, respair_forward, respair_supported
    x, w1, b1, w2, b2, accb = R.pair_inputs(C, k, d, T)
    op1 = ConvOp(L.CONV1D, C, C, k, d, d * (k - 1) // 2).set_math(L.MATH_BF16)
    op2 = ConvOp(L.CONV1D, C, C, k, 1, (k - 1) // 2).set_math(L.MATH_BF16)
    op1.set_weights(dev(w1), None, dev(b1))
    op2.set_weights(dev(w2), None, dev(b2))
    assert respair_supported(op1, op2)
    tile = "2, 1, 4" if C == 32 else "2, 2, 2"
    xd = dev(x)
    y = respair_forward(op1, op2, xd, torch.empty_like(xd), res=xd)
    assert op1.kernel_instance() == "respair_split_kernel<%s, 1, false>" % tile, op1.kernel_instance()
    ref, extra, _, _ = R.pair_expected(oracle, x, w1, b1, w2, b2, k=k, d=d, res=x)
    what = f"{op1.kernel_instance()} C{C} k{k} d{d} T{T}"
    R.assert_close(y, ref, extra, what=what)
    acc_t = dev(accb)
    respair_forward(op1, op2, xd, acc_t, res=xd, acc=acc_t, scale=1.0 / 3.0)             # in-place accumulate, MRF average
    ref, extra, _, _ = R.pair_expected(oracle, x, w1, b1, w2, b2, k=k, d=d, res=x, acc=accb, scale=1.0 / 3.0)
    R.assert_close(acc_t, ref, extra, what=what + " acc scale")
    xb, xv = bf(x)
    ab, av = bf(accb)
    yb = respair_forward(op1, op2, xb, torch.empty_like(xb), res=xb, acc=ab, scale=1.0 / 3.0)
    assert op1.kernel_instance() == "respair_split_kernel<%s, 1, true>" % tile, op1.kernel_instance()
    ref, extra, _, _ = R.pair_expected(oracle, xv, w1, b1, w2, b2, k=k, d=d, res=xv, acc=av, scale=1.0 / 3.0)
    R.assert_close(yb, ref, extra, bf16_out=True, what=f"{op1.kernel_instance()} C{C} k{k} d{d} T{T} acc scale")
