"""csrc/resblock_f16.hip on v_mfma_f32_16x16x32_f16: the lane maps of the new tiling (an exact probe: one-hot weights, small integers), every
dispatched instance against a float64 chain (ragged / edge / interior tiles, both epilogues, whole blocks and single pairs, the MRF
accumulate input and scale), the fused launch against the conv-by-conv launches, and inputs that move the tile's scale."""
import functools

import pytest
import torch
import torch.nn.functional as F

from visinger_amd import _lib as L

pytestmark = pytest.mark.gpu


def _chain64(x, convs, acc=None, scale=1.0):
    """float64 on the CPU: for each pair x = conv2(lrelu(conv1(lrelu(x)))) + x; convs: [(weight, bias, dilation), ...]"""
    x = x.double().cpu()
    for (w1, b1, d1), (w2, b2, d2) in zip(convs[0::2], convs[1::2]):
        k = w1.shape[2]
        xt = F.conv1d(F.leaky_relu(x, 0.1), w1.double().cpu(), b1.double().cpu(), padding=d1 * (k - 1) // 2, dilation=d1)
        xt = F.conv1d(F.leaky_relu(xt, 0.1), w2.double().cpu(), b2.double().cpu(), padding=d2 * (k - 1) // 2, dilation=d2)
        x = xt + x
    if acc is not None:
        x = x + acc.double().cpu()
    return x * scale


def _ops(convs):
    from visinger_amd.ops import ConvOp
    ops = []
    for w, b, d in convs:
        C, k = w.shape[0], w.shape[2]
        op = ConvOp(L.CONV1D, C, C, k, d, d * (k - 1) // 2).set_math(L.MATH_SPLIT3)
        op.set_weights(w.cuda().contiguous(), None, b.cuda().contiguous())
        ops.append(op)
    return ops


# ---- 1. the lane maps, exactly
@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("k,d", [(3, 1), (11, 3)])
def test_layout_probe_one_hot_weights_small_integers(C, k, d):
    """W[o][(o + tap) % C][tap] = 1: every output is a sum of k inputs, each from its own (channel, tap); x holds the integers 1 .. 15 in a
    pattern of (item, channel, position).  lrelu is the identity on them, every intermediate an integer below 2^20, exact in the two f16
    planes and the fp32 accumulators: a wrong row, column or K-group map of the operands, the accumulators or the tile gives another integer."""
    from visinger_amd.ops import resblock_forward
    B, T = 2, 700
    w = torch.zeros(C, C, k)
    for tap in range(k):
        w[torch.arange(C), (torch.arange(C) + tap) % C, tap] = 1.0
    zero = torch.zeros(C)
    convs = [(w, zero, d), (w, zero, 1)]
    b_, c_, t_ = torch.meshgrid(torch.arange(B), torch.arange(C), torch.arange(T), indexing="ij")
    x = (1 + (7 * b_ + 3 * c_ + 5 * t_ + (c_ // 8) * (t_ // 16)) % 15).float()
    want = _chain64(x, convs)
    assert float(want.max()) < 2 ** 20
    ops = _ops(convs)
    y = resblock_forward(ops, x.cuda(), torch.empty(B, C, T, device="cuda")).cpu()
    assert ops[0].kernel_instance().startswith("resblock_f16_kernel<"), ops[0].kernel_instance()
    if not torch.equal(y.double(), want):
        bad = (y.double() != want).nonzero()
        b0, c0, t0 = (int(v) for v in bad[0])
        pytest.fail(f"{len(bad)} of {y.numel()} outputs differ [{ops[0].kernel_instance()}]; first at item {b0}, channel {c0} (row {c0 % 32} of its 32-row tile: "
                    f"row tile {(c0 % 32) // 16}, lane group {(c0 % 16) // 4}, register {c0 % 4}), position {t0}: {float(y[b0, c0, t0])} for {float(want[b0, c0, t0])}; "
                    f"channels hit {sorted(set(bad[:, 1].tolist()))[:16]}, positions mod 16 hit {sorted(set((bad[:, 2] % 16).tolist()))}")


# ---- 2. bounds against the float64 chain, instance by instance
def _block(C, k, seed):
    from visinger_amd.modules.hipconv import set_conv_math
    from visinger_amd.modules.visinger.decoder import ResBlock1
    torch.manual_seed(seed)
    m = ResBlock1(C, k, (1, 3, 5))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("weight_g"):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p.shape[1] * p.shape[2]) ** 0.5)
    return set_conv_math(m.cuda().eval(), L.MATH_SPLIT3)


def _folded(m):
    """[(weight, bias, dilation)] of the block's chain, the weight norm folded in float64"""
    out = []
    for c1, c2 in zip(m.convs1, m.convs2):
        for c in (c1, c2):
            v, g = c.weight_v.detach().double().cpu(), c.weight_g.detach().double().cpu()
            out.append((g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1), c.bias.detach().double().cpu(), c.dilation[0]))
    return out


@functools.lru_cache(maxsize=None)
def _case(C, k, T, gains=False):
    """the block, its inputs and the float64 results, once per shape (shared by the whole-block and the pair-by-pair case; never modified)"""
    m = _block(C, k, C + k)
    g = torch.Generator().manual_seed(C * 7 + k + T)
    x = 2.0 * torch.randn(2, C, T, generator=g)
    if gains:       # per-channel gains 2^-6 .. 2^6 on half the channels and one 2^12 outlier: the tile's scale moves from tile to tile and conv to conv
        x[:, : C // 2] *= torch.exp2(torch.randint(-6, 7, (2, C // 2, 1), generator=g).float())
        x[0, C - 2, 300:340] = -(2.0 ** 12)
    acc = torch.randn(2, C, T, generator=g)
    convs = _folded(m)
    want = _chain64(x, convs)
    return m, x, acc, want, (want + acc.double()) / 3.0, float(want.pow(2).mean().sqrt())


def _run_and_check(vs_option, C, k, T, pairs, conv, inst, gains=False):
    m, x, acc, want, want_acc, scale = _case(C, k, T, gains)
    vs_option("VS_RESBLOCK_PAIRS", pairs)
    xd = x.cuda()
    with torch.no_grad():
        y = m._run_fused(xd, torch.empty_like(xd), first=True, scale=1.0)
        name = m.convs1[conv]._op().kernel_instance()
        acc_t = acc.cuda()
        m._run_fused(xd, acc_t, first=False, scale=1.0 / 3.0)
    e_y = float((y.double().cpu() - want).abs().max()) / scale
    e_a = float((acc_t.double().cpu() - want_acc).abs().max()) / scale
    print(f"\n   C={C} k={k} T={T} pairs={pairs} [{name}]: max abs error {e_y:.2e} / with acc and scale {e_a:.2e} of the output rms")
    assert name.startswith("resblock_f16_kernel" + inst), (name, inst)
    assert e_y <= 1e-5 and e_a <= 1e-5
    assert torch.equal(xd.cpu(), x)


INSTANCES = [  # C, k, pairs per launch, the pair whose launch is named, its instance
    (32, 3, 3, 0, "<2, 1, 4, 8>"), (32, 7, 3, 0, "<4, 1, 4, 16>"), (32, 11, 3, 0, "<4, 1, 4, 28>"),
    (64, 7, 1, 0, "<4, 2, 2, 8>"), (64, 11, 1, 2, "<4, 2, 2, 28>"), (128, 3, 3, 0, "<4, 4, 2, 8>"),
    (32, 3, 1, 2, "<2, 1, 4, 8>"), (64, 3, 3, 0, "<4, 2, 2, 8>"), (128, 3, 1, 0, "<4, 4, 1, 8>"),
]


@pytest.mark.parametrize("T", [700, 1024])          # a ragged last tile + both edge tiles (the element-wise epilogue) / whole tiles (the fast one)
@pytest.mark.parametrize("C,k,pairs,conv,inst", INSTANCES, ids=lambda v: str(v).replace(", ", "_").strip("<>"))
def test_instances_vs_float64_chain(vs_option, C, k, pairs, conv, inst, T):
    _run_and_check(vs_option, C, k, T, pairs, conv, inst)


def test_wide64_instance_vs_float64_chain():
    """64 channels, k = 11, the pair at dilation 5 on a launch that fills the chip twice over: 512-column tiles on eight waves.  Items 2 .. 7 repeat
    items 0 and 1, so the float64 chain is taken on two items and the others are compared bit for bit with their originals."""
    from visinger_amd.ops import resblock_forward
    m = _block(64, 11, 75)
    convs = _folded(m)[4:6]
    g = torch.Generator().manual_seed(29)
    x2 = 2.0 * torch.randn(2, 64, 29000, generator=g)
    acc2 = torch.randn(2, 64, 29000, generator=g)
    want = (_chain64(x2, convs) + acc2.double()) / 3.0
    scale = float((want * 3.0 - acc2.double()).pow(2).mean().sqrt())
    ops = [m.convs1[2]._op(), m.convs2[2]._op()]
    with torch.no_grad():
        m._run_fused(x2[:, :, :256].cuda(), torch.empty(2, 64, 256, device="cuda"))       # (binds the weights of every conv of the block)
        y = resblock_forward(ops, x2.repeat(4, 1, 1).cuda(), torch.empty(8, 64, 29000, device="cuda"), acc=acc2.repeat(4, 1, 1).cuda(), scale=1.0 / 3.0).cpu()
    name = ops[0].kernel_instance()
    err = float((y[:2].double() - want).abs().max()) / scale
    print(f"\n   [{name}]: max abs error {err:.2e} of the output rms")
    assert name.startswith("resblock_f16_kernel<4, 2, 4, 28>"), name
    assert err <= 1e-5
    for i in range(1, 4):
        assert torch.equal(y[2 * i:2 * i + 2], y[:2]), i


# ---- 3. against the conv-by-conv path
def test_fused_launch_equals_conv_by_conv_launches(vs_option):
    m = _block(64, 7, 5)
    x = torch.randn(2, 64, 8192, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    with torch.no_grad():
        y_f = m._run_fused(x, torch.empty_like(x)).clone()
        name = m.convs1[0]._op().kernel_instance()
        y_g = m._run_fused(x, torch.empty_like(x)).clone()
        vs_option("VS_NO_RESBLOCK_FUSED", 1)
        y_u = m._run_fused(x, torch.empty_like(x))
    assert name.startswith("resblock_f16_kernel<") and not m.convs1[0]._op().kernel_instance().startswith("resblock_"), (name, m.convs1[0]._op().kernel_instance())
    rel = float((y_f - y_u).abs().max()) / float(y_u.abs().max())
    print(f"\n   fused against conv by conv: {rel:.2e} of max |y|")
    assert rel <= 2e-6
    assert torch.equal(y_f, y_g)                     # two runs, bit for bit


# ---- 4. inputs that move the tile's scale
@pytest.mark.parametrize("C,k,pairs,conv,inst", [(32, 3, 3, 0, "<2, 1, 4, 8>"), (64, 7, 1, 0, "<4, 2, 2, 8>"), (128, 3, 3, 0, "<4, 4, 2, 8>")],
                         ids=lambda v: str(v).replace(", ", "_").strip("<>"))
def test_inputs_that_move_the_tile_scale(vs_option, C, k, pairs, conv, inst):
    _run_and_check(vs_option, C, k, 700, pairs, conv, inst, gains=True)
