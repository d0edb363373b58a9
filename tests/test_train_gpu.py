"""Training-mode path: HIP forward + PyTorch-ROCm backward.
  * train-mode forward (unfused, autograd-recorded) == eval-mode forward (fused HIP epilogues) on the same inputs;
  * gradients of a scalar functional of the training forward == the reference's own autograd (golden vectors);
  * one full GAN iteration (generator pass + discriminator pass, AdamW x2, ExponentialLR x2, clipping) runs and
    updates both networks; the checkpoint written afterwards has the reference's layout."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tiny_model():
    from visinger_amd.models.visinger import VISinger
    w, a = load_golden("visinger_tiny")
    hp = json.load(open(os.path.join(GOLDEN, "visinger_tiny_hparams.json")))
    m = VISinger(13, 9, 7, hp)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return m.cuda(), a, hp


def test_train_forward_equals_eval_forward():
    m, a, hp = tiny_model()
    args = (cu(a["text"]), cu(a["pitch"]), cu(a["dur"]), cu(a["mel2ph"]))
    kw = dict(spk_id=cu(a["spk_id"]), mel=cu(a["lin"]), infer=False, noise_q=cu(a["noise_q"]), u_slice=torch.from_numpy(a["u_slice"]))
    m.eval()
    with torch.no_grad():
        ev = m(*args, **kw)
    m.train()
    tr = m(*args, **kw)
    assert tr["wav_out"].requires_grad and tr["kl"].requires_grad
    for k in ("wav_out", "z_p", "ph_pred", "kl"):
        d = float((tr[k].detach() - ev[k]).abs().max())
        assert d <= 2e-5 * max(1.0, float(ev[k].abs().max())), (k, d)
    assert torch.equal(tr["ids_slice"], ev["ids_slice"])
    # and both equal the reference's golden training forward
    assert float((tr["wav_out"].detach().cpu() - torch.from_numpy(a["t_wav_out"])).abs().max()) <= 1e-4


def test_gradients_match_reference_autograd():
    m, a, hp = tiny_model()
    _, g = load_golden("visinger_tiny_grads")
    m.train()
    out = m(cu(a["text"]), cu(a["pitch"]), cu(a["dur"]), cu(a["mel2ph"]), spk_id=cu(a["spk_id"]), mel=cu(a["lin"]), infer=False,
            noise_q=cu(g["noise_q"]), u_slice=torch.from_numpy(g["u_slice"]))
    loss = out["kl"] + 0.1 * (out["wav_out"] * cu(g["c_w"])).sum() + 0.01 * (out["ph_pred"] * cu(g["c_p"])).sum() + \
        0.01 * (out["z_p"] * cu(g["c_z"])).sum()
    assert abs(float(loss) - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))
    loss.backward()
    named = dict(m.named_parameters())
    checked = 0
    for key in g:
        if not key.startswith("g."):
            continue
        ref = g[key]
        got = named[key[2:]].grad.detach().cpu().numpy()
        scale = np.abs(ref).max() + 1e-8
        err = np.abs(got - ref).max() / scale
        assert err <= 2e-3, (key, err, scale)
        checked += 1
    assert checked >= 20


def test_full_gan_training_step_runs_and_updates():
    from visinger_amd import ckpt
    from visinger_amd.train import VISingerTrainer, synthetic_train_batch
    hp = json.load(open(os.path.join(GOLDEN, "visinger_tiny_hparams.json")))
    hp = dict(hp, use_pitch_embed=True, pitch_predictor_layers=1, segment_size=8, p_dropout=0.1)
    torch.manual_seed(0)
    tr = VISingerTrainer(64, 117, 131, hp, dict(fft_size=64, win_size=32, num_mel_bins=16, fmin=0.0, fmax=4000.0, sample_rate=8000))
    tr = tr.cuda().train().configure()
    hop = tr.hop
    batch = synthetic_train_batch(2, 48, 6, hop, 64, hp["num_linear_bins"], 1, "cuda")
    before_g = tr.model.decoder.conv_pre.weight.detach().clone()
    before_d = tr.mel_disc.discriminators[0].convs[0].weight_v.detach().clone()
    logs1 = tr.training_step(batch)
    logs2 = tr.training_step(batch)
    for logs in (logs1, logs2):
        assert set(logs) >= {"kl", "mel_l1", "ctc", "generator", "feature_match", "discriminator", "uv", "f0"}
        assert all(np.isfinite(v) for v in logs.values()), logs
    assert not torch.equal(before_g, tr.model.decoder.conv_pre.weight)
    assert not torch.equal(before_d, tr.mel_disc.discriminators[0].convs[0].weight_v)
    # endless_ds: false (config/models/visinger.yaml:106): the rate decays per EPOCH, not per step (tasks/visinger.py:225-227)
    assert tr.global_step == 2 and tr.opt_gen.param_groups[0]["lr"] == 2e-4 and tr.opt_disc.param_groups[0]["lr"] == 2e-4
    tr.on_epoch_end()
    tr.training_step(batch)
    for o in (tr.opt_gen, tr.opt_disc):
        assert abs(o.param_groups[0]["lr"] - 2e-4 * 0.999875) < 1e-15
    assert all(p.grad is None for p in tr.parameters())      # zero_grad right after each optimizer step (trainer.py:373-374)
    tr.global_step = 2
    # inference after training uses the fused HIP path with the updated weights (packed copies follow the versions)
    tr.eval()
    with torch.no_grad():
        wav = tr.model(batch["text_tokens"], batch["note_pitch"], batch["note_dur"], batch["mel2ph"], spk_id=batch["spk_ids"],
                       infer=True)["wav_out"]
    assert wav.shape == (2, 48 * hop) and torch.isfinite(wav).all()
    p = ckpt.save_checkpoint("/tmp/model_ckpt_steps_2.ckpt", {"model": tr.model, "mel_disc": tr.mel_disc}, [tr.opt_gen, tr.opt_disc],
                             global_step=2)
    raw, _ = ckpt.read_checkpoint(p)
    assert set(raw["state_dict"]) == {"model", "mel_disc"} and len(raw["optimizer_states"]) == 2


@pytest.mark.parametrize("kind,Cin,Cout,K,d_or_u,T", [("conv", 24, 40, 5, 1, 77), ("conv", 32, 32, 7, 3, 130), ("conv", 16, 48, 1, 1, 50),
                                                      ("conv", 32, 32, 11, 5, 200), ("tconv", 32, 16, 8, 4, 37), ("tconv", 24, 12, 11, 5, 20),
                                                      ("tconv", 16, 16, 4, 2, 64), ("tconv", 64, 32, 16, 8, 9), ("tconv", 20, 10, 7, 3, 15)])
def test_conv_backward_matches_aten(kind, Cin, Cout, K, d_or_u, T):
    """HIP-engine grad-input + GEMM grad-weight (visinger_amd.autograd.conv_backward) vs aten::convolution_backward (fp32)."""
    from visinger_amd.autograd import conv_backward
    from visinger_amd.modules.hipconv import HipConv1d, HipConvTranspose1d
    torch.manual_seed(K * 100 + T)
    B = 3
    if kind == "conv":
        m = HipConv1d(Cin, Cout, K, dilation=d_or_u, padding=d_or_u * (K - 1) // 2).cuda()
        w = torch.randn(Cout, Cin, K, device="cuda") / (Cin * K) ** 0.5
        y_shape = (B, Cout, T)
        args = ([1], [m.padding[0]], [d_or_u], False)
    else:
        m = HipConvTranspose1d(Cin, Cout, K, d_or_u, padding=(K - d_or_u) // 2).cuda()
        w = torch.randn(Cin, Cout, K, device="cuda") / (Cin * K) ** 0.5
        y_shape = (B, Cout, (T - 1) * d_or_u - 2 * m.padding[0] + K)
        args = ([d_or_u], [m.padding[0]], [1], True)
    x = torch.randn(B, Cin, T, device="cuda")
    gy = torch.randn(*y_shape, device="cuda")
    gx, gw = conv_backward(m, x, w, gy, True, True)
    rx, rw, _ = torch.ops.aten.convolution_backward(gy, x, w, None, args[0], args[1], args[2], args[3], [0], 1, [True, True, False])
    for got, ref in ((gx, rx), (gw, rw)):
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) <= 2e-5 * (1.0 + float(ref.abs().max()))


def test_training_forward_follows_weight_updates():
    """The training path folds weight_g * v / ||v|| into a NEW tensor every step; the caching allocator places it at the
    previous step's address with version 0, so the packed-weight cache must not be keyed on (data_ptr, version) there:
    three 'optimizer steps' in a row, each forward must use the current weights."""
    import torch.nn.functional as F
    from torch.nn.utils import weight_norm
    from visinger_amd.modules.hipconv import HipConv1d
    torch.manual_seed(5)
    m = weight_norm(HipConv1d(24, 40, 5, padding=2)).cuda().train()
    x = torch.randn(2, 24, 100, device="cuda")
    for step in range(3):
        y = m(x)
        w = torch._weight_norm(m.weight_v, m.weight_g, 0)
        ref = F.conv1d(x, w, m.bias, padding=2)
        assert float((y - ref).abs().max()) <= 2e-5 * (1 + float(ref.abs().max())), step
        with torch.no_grad():
            m.weight_v.mul_(1.5).add_(0.1)
            m.weight_g.add_(0.3)
            m.bias.sub_(0.2)
        del y, w, ref


def test_wavenet_odd_split_two_pass_epilogue_stays_in_bounds():
    """hidden = 16: the res/skip conv splits its 32 rows at 16 (not a tile multiple) and runs as two row-windowed passes; the
    second pass addresses its destination through a pointer moved back by split_row rows, and the epilogue's unconditional
    loads for the rows of the OTHER pass used to land below the buffer (a page fault when it starts a mapping)."""
    from visinger_amd.modules.visinger.encoder import WaveNet
    torch.manual_seed(6)
    m = WaveNet(16, 5, 1, 3, gin_channels=0).cuda().eval()
    x = torch.randn(2, 16, 48, device="cuda")
    mask = torch.ones(2, 1, 48, device="cuda")
    with torch.no_grad():
        for _ in range(20):
            torch.cuda.empty_cache()                       # fresh mappings: destinations start at segment boundaries
            y = m(x, mask)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()


def test_backward_random_sweep(monkeypatch):
    """tools/backward_fuzz.py: 120 random conv / transposed / strided-dense / grouped cases, gradients vs aten"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import backward_fuzz
    monkeypatch.setattr(sys, "argv", ["backward_fuzz.py", "120", "9"])
    backward_fuzz.main()


def test_fused_gate_and_layernorm_functions_match_torch_autograd():
    """visinger_amd.autograd.GateFn / LayerNormFn (csrc/train_ops.hip: one forward + one backward launch each) against PyTorch autograd of
    the reference expressions (encoder.py:177-180, 206-213; rel_transformer.py:33-42, 305): values and every gradient, odd sizes."""
    from visinger_amd.autograd import GateFn, LayerNormFn
    torch.manual_seed(11)
    for B, H, T, Lyr in ((2, 192, 512, 3), (3, 24, 37, 1), (1, 16, 1030, 2)):
        x_in = torch.randn(B, 2 * H, T, device="cuda", requires_grad=True)
        gall = torch.randn(B, 2 * H * Lyr, 1, device="cuda", requires_grad=True)
        i = Lyr - 1
        w = torch.randn(B, H, T, device="cuda")
        acts = GateFn.apply(x_in, gall[:, i * 2 * H:(i + 1) * 2 * H, :])
        gx, gg = torch.autograd.grad((acts * w).sum(), [x_in, gall])
        xr, gr = x_in.detach().clone().requires_grad_(True), gall.detach().clone().requires_grad_(True)
        z = xr + gr[:, i * 2 * H:(i + 1) * 2 * H, :]
        ref = torch.tanh(z[:, :H]) * torch.sigmoid(z[:, H:])
        rx, rg = torch.autograd.grad((ref * w).sum(), [xr, gr])
        assert float((acts - ref).abs().max()) <= 2e-6
        assert float((gx - rx).abs().max()) <= 2e-6 * (1 + float(rx.abs().max()))
        assert float((gg - rg).abs().max()) <= 2e-5 * (1 + float(rg.abs().max()))            # sum over T of fp32 terms, atomics
        acts0 = GateFn.apply(x_in, None)                                                        # no conditioning (gin_channels = 0)
        assert float((acts0 - torch.tanh(x_in[:, :H]) * torch.sigmoid(x_in[:, H:])).abs().max()) <= 2e-6
    for B, C, T in ((2, 192, 512), (3, 24, 65), (1, 512, 130)):
        a = torch.randn(B, C, T, device="cuda", requires_grad=True)
        r = torch.randn(B, C, T, device="cuda", requires_grad=True)
        gamma = (1 + 0.2 * torch.randn(C, device="cuda")).requires_grad_(True)
        beta = (0.1 * torch.randn(C, device="cuda")).requires_grad_(True)
        w = torch.randn(B, C, T, device="cuda")
        for res in (r, None):
            y = LayerNormFn.apply(a, res, gamma, beta, 1e-4)
            ins = [a, gamma, beta] + ([r] if res is not None else [])
            got = torch.autograd.grad((y * w).sum(), ins)
            x = a if res is None else a + r
            mean = x.mean(1, keepdim=True)
            var = ((x - mean) ** 2).mean(1, keepdim=True)
            ref = (x - mean) * torch.rsqrt(var + 1e-4) * gamma.view(1, -1, 1) + beta.view(1, -1, 1)
            want = torch.autograd.grad((ref * w).sum(), ins)
            assert float((y - ref).abs().max()) <= 1e-5
            for gg_, ww_ in zip(got, want):
                assert float((gg_ - ww_).abs().max()) <= 3e-5 * (1 + float(ww_.abs().max())), (B, C, T, res is None)


@pytest.mark.parametrize("Cin,Cout,K,d,T,B", [(192, 384, 5, 1, 512, 4), (192, 768, 9, 1, 64, 8), (128, 128, 11, 5, 2048, 2), (64, 64, 3, 3, 1000, 2),
                                              (96, 200, 7, 1, 516, 2), (32, 64, 11, 1, 8192, 1), (256, 256, 7, 3, 256, 3), (100, 130, 2, 1, 261, 2), (64, 96, 8, 1, 519, 2), (64, 128, 4, 1, 1027, 1), (80, 64, 6, 1, 133, 4)])
def test_wgrad_split_kernel_matches_aten(Cin, Cout, K, d, T, B):
    """vs_conv_wgrad on the bf16 matrix instruction in the split-bf16 x6 arithmetic (csrc/conv_backward.hip conv_wgrad_split_kernel: 2..12
    taps, >= 64 output channels): weight gradient vs aten::convolution_backward in fp32 -- both tap layouts (all taps per wave; taps split
    over wave pairs for K > 8), even and odd tap offsets (the v_alignbyte path), dilations, channel counts off the tile sizes, a ragged
    last unit."""
    from visinger_amd.ops import conv_wgrad
    torch.manual_seed(Cin + Cout + K + T)
    pad = d * (K - 1) // 2
    x = torch.randn(B, Cin, T, device="cuda")
    gy = torch.randn(B, Cout, T + 2 * pad - d * (K - 1), device="cuda")        # (K = 2: an even kernel, T_out = T - 1)
    w = torch.zeros(Cout, Cin, K, device="cuda")
    got = conv_wgrad(gy, x, K, d, pad)
    _, ref, _ = torch.ops.aten.convolution_backward(gy, x, w, None, [1], [pad], [d], False, [0], 1, [False, True, False])
    ref64 = torch.ops.aten.convolution_backward(gy.double(), x.double(), w.double(), None, [1], [pad], [d], False, [0], 1, [False, True, False])[1]
    e_got = float((got.double() - ref64).abs().max()), float((ref.double() - ref64).abs().max())
    scale = float(ref64.abs().max())
    assert got.shape == ref.shape
    assert e_got[0] <= 3e-6 * scale + 2.5 * e_got[1], (e_got, scale)        # fp32 class: within the library's own error of the fp64 result


@pytest.mark.parametrize("B,C,T", [(16, 192, 512), (32, 32, 8192), (3, 7, 260), (2, 5, 1001), (1, 1, 12), (16, 1536, 1), (5, 64, 4)])
def test_bias_grad_and_single_position_wgrad(B, C, T):
    """vs_bias_grad (gb[c] = sum over (b, t) of gy: one launch, fixed order) against an fp64 sum -- float4 path with full and ragged batches of
    eight loads, the scalar path for T % 4 != 0 -- run-to-run bit-identical; and the T = 1 weight gradient (a library GEMM: ops.conv_wgrad)."""
    from visinger_amd.ops import bias_grad, conv_wgrad
    torch.manual_seed(B * 1000 + C + T)
    gy = torch.randn(B, C, T, device="cuda")
    got = bias_grad(gy)
    ref = gy.double().sum((0, 2))
    assert got.shape == (C,)
    assert float((got.double() - ref).abs().max()) <= 1e-5 * (1.0 + float(gy.abs().double().sum((0, 2)).max()) * 0.05)
    assert torch.equal(got, bias_grad(gy))
    if T == 1:
        x = torch.randn(B, 24, 1, device="cuda")
        gw = conv_wgrad(gy, x, 1, 1, 0)
        want = torch.einsum("bot,bit->oi", gy.double(), x.double()).unsqueeze(2)
        assert gw.shape == (C, 24, 1)
        assert float((gw.double() - want).abs().max()) <= 1e-5 * (1.0 + float(want.abs().max()))


@pytest.mark.parametrize("Cin,Cout,K,d,T,B", [(192, 384, 5, 1, 512, 4), (192, 768, 9, 1, 64, 8), (96, 200, 7, 1, 516, 2), (32, 64, 11, 1, 8192, 1),
                                              (192, 192, 1, 1, 512, 16), (24, 40, 5, 1, 77, 2), (16, 48, 1, 1, 50, 3), (40, 33, 3, 2, 301, 2), (64, 1, 3, 1, 640, 2)])
def test_wgrad_with_fused_bias_gradient(Cin, Cout, K, d, T, B):
    """ops.conv_wgrad(..., bias=True) (vs_conv_wgrad_bias): the weight gradient is the one of the plain call bit for bit, and the bias gradient -- the
    gy row sums taken by the weight-gradient kernel's first c_in tile, both kernels (split-bf16 and exact-fp32, taps split over waves or positions), then
    the fixed-order plane reduction -- equals the fp64 sum and is run-to-run bit-identical."""
    from visinger_amd.ops import conv_wgrad
    torch.manual_seed(Cin * 7 + Cout + K + T)
    pad = d * (K - 1) // 2
    x = torch.randn(B, Cin, T, device="cuda")
    gy = torch.randn(B, Cout, T + 2 * pad - d * (K - 1), device="cuda")
    gw0 = conv_wgrad(gy, x, K, d, pad)
    gw, gb = conv_wgrad(gy, x, K, d, pad, bias=True)
    assert torch.equal(gw, gw0) and gb.shape == (Cout,)
    ref = gy.double().sum((0, 2))
    assert float((gb.double() - ref).abs().max()) <= 1e-5 * (1.0 + float(gy.abs().double().sum((0, 2)).max()) * 0.05)
    gw2, gb2 = conv_wgrad(gy, x, K, d, pad, bias=True)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
    ref64 = torch.ops.aten.convolution_backward(gy.double(), x.double(), torch.zeros(Cout, Cin, K, device="cuda", dtype=torch.double), None, [1], [pad], [d],
                                                False, [0], 1, [False, True, False])[1]
    assert float((gw.double() - ref64).abs().max()) <= 2e-5 * float(ref64.abs().max())


def test_wavenet_step_and_l1_mean_functions_match_torch_autograd():
    """autograd.WnStepFn (vs_wn_step_fwd / _bwd) and autograd.L1MeanFn (vs_l1_mean_fwd / _bwd) against PyTorch autograd of the reference expressions
    (encoder.py:186-193; tasks/visinger.py:162-169): values and gradients, odd sizes, the first layer's missing accumulator, permuted dense layouts."""
    from visinger_amd.autograd import L1MeanFn, WnStepFn, l1_mean
    torch.manual_seed(5)
    for B, H, T in ((2, 192, 512), (3, 24, 37), (1, 16, 1030)):
        x = torch.randn(B, H, T, device="cuda", requires_grad=True)
        rs = torch.randn(B, 2 * H, T, device="cuda", requires_grad=True)
        acc = torch.randn(B, H, T, device="cuda", requires_grad=True)
        mask = (torch.rand(B, 1, T, device="cuda") > 0.2).float()
        wx, wo = torch.randn(B, H, T, device="cuda"), torch.randn(B, H, T, device="cuda")
        for a in (acc, None):
            xn, on = WnStepFn.apply(x, rs, a, mask.reshape(B, T).contiguous())
            rx = (x + rs[:, :H]) * mask
            ro = rs[:, H:] if a is None else a + rs[:, H:]
            assert torch.equal(xn, rx) and torch.equal(on, ro)
            ins = [x, rs] + ([a] if a is not None else [])
            got = torch.autograd.grad((xn * wx).sum() + (on * wo).sum(), ins, retain_graph=True)
            want = torch.autograd.grad((rx * wx).sum() + (ro * wo).sum(), ins)
            for g_, w_ in zip(got, want):
                assert torch.equal(g_, w_)
            got1 = torch.autograd.grad((on * wo).sum(), [rs])[0]              # only one of the outputs takes a gradient
            assert torch.equal(got1, torch.autograd.grad((ro * wo).sum(), [rs])[0])
    for shape, perm in (((4, 64, 33, 3), (0, 2, 3, 1)), ((2, 1024, 7), None), ((1, 1, 5), None), ((3, 300000), None)):
        a = torch.randn(shape, device="cuda")
        b = torch.randn(shape, device="cuda")
        if perm:
            a, b = a.permute(perm), b.permute(perm)
        a.requires_grad_(True)
        assert L1MeanFn.dense_pair(a, b)
        got = l1_mean(a, b)
        ref = torch.mean(torch.abs(b - a))
        assert abs(float(got) - float(ref)) <= 2e-6 * float(ref)
        assert float(l1_mean(a, b)) == float(got)                               # deterministic (fixed-order partials)
        ga = torch.autograd.grad(got * 3.0, [a])[0]
        ra = torch.autograd.grad(ref * 3.0, [a])[0]
        assert ga.stride() == a.stride() and float((ga - ra).abs().max()) <= 1e-9
    a = torch.randn(4, 8, 6, device="cuda", requires_grad=True)
    assert not L1MeanFn.dense_pair(a[:, :, :5], torch.randn(4, 8, 5, device="cuda"))      # a gap in the layout: the PyTorch formulation
    assert float(l1_mean(a[:, :, :5], torch.zeros(4, 8, 5, device="cuda"))) == float(a[:, :, :5].abs().mean())


def _attn_core_torch(q, k, v, rel_k, rel_v, mask, nh, w, keep=None):
    """rel_transformer.py:148-179 + 181-243 with plain torch ops on [B, nh, T, T] (fp64): the definition the streaming kernels are
    checked against.  keep: dropout factor per (b, h, query, key) (0 or 1 / (1 - p)), or None."""
    B, C, T = q.shape
    dk = C // nh
    qh, kh, vh = (t.view(B, nh, dk, T).transpose(2, 3) for t in (q, k, v))
    scale = 1.0 / np.sqrt(dk)
    scores = torch.matmul(qh, kh.transpose(-2, -1)) * scale
    i = torch.arange(T, device=q.device)
    if rel_k is not None:
        idx = i[None, :] - i[:, None] + w                                  # [T(query), T(key)]
        band = (idx >= 0) & (idx <= 2 * w)
        qr = torch.matmul(qh, rel_k.unsqueeze(0).transpose(-2, -1)) * scale      # [B, nh, T, R]
        scores = scores + torch.where(band, qr.gather(-1, idx.clamp(0, 2 * w).expand(B, nh, T, T)), torch.zeros_like(scores))
    if mask is not None:
        am = mask.view(B, 1, T, 1) * mask.view(B, 1, 1, T)
        scores = scores.masked_fill(am == 0, -1e4)
    p = torch.softmax(scores, -1)
    if keep is not None:
        p = p * keep
    out = torch.matmul(p, vh)
    if rel_k is not None:
        pw = torch.stack([torch.where((i + r - w >= 0) & (i + r - w < T), p.gather(-1, (i + r - w).clamp(0, T - 1).view(1, 1, T, 1).expand(B, nh, T, 1))[..., 0],
                                      torch.zeros_like(p[..., 0])) for r in range(2 * w + 1)], -1)           # [B, nh, T, R]
        out = out + torch.matmul(pw, rel_v.unsqueeze(0))
    return out.transpose(2, 3).reshape(B, C, T)


def _hash_keep(seed, B, nh, T, p_drop, device):
    """csrc/attention_train.hip drop_factor(), restated on int64 tensors"""
    M = 0xFFFFFFFF
    lo, hi = seed & M, (seed >> 32) & M
    qi = torch.arange(T, dtype=torch.int64, device=device).view(1, T, 1)
    ki = torch.arange(T, dtype=torch.int64, device=device).view(1, 1, T)
    bh = torch.arange(B * nh, dtype=torch.int64, device=device).view(B * nh, 1, 1)
    x = (qi * T + ki) & M
    x = x ^ lo
    x = (x * 0x9E3779B1) & M
    x = x ^ (x >> 16)
    x = (x + bh * 0x85EBCA6B + hi) & M
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & M
    x = x ^ (x >> 16)
    thr = int(p_drop * 4294967296.0)
    return ((x >= thr).double() / (1.0 - p_drop)).view(B, nh, T, T)


@pytest.mark.parametrize("B,nh,dk,T,w,nh_rel,p_drop", [(2, 2, 96, 100, 4, 1, 0.0), (3, 2, 96, 64, 4, 1, 0.0), (1, 4, 32, 33, 4, 4, 0.0),
                                                       (2, 2, 48, 70, 2, 1, 0.0), (1, 1, 128, 257, 7, 1, 0.0), (2, 2, 64, 40, None, 1, 0.0),
                                                       (2, 2, 96, 512, 4, 1, 0.0), (2, 2, 96, 100, 4, 1, 0.1), (1, 2, 32, 37, 4, 2, 0.5),
                                                       (2, 3, 16, 5, 4, 1, 0.0)])
def test_training_attention_kernels_match_torch_autograd(B, nh, dk, T, w, nh_rel, p_drop):
    """csrc/attention_train.hip (forward with log-sum-exp, backward for dQ + d rel_k + d rel_v, backward for dK / dV; exact-fp32 MFMA,
    streaming, dropout by a counter-based hash) against the [T, T] definition of rel_transformer.py:148-179 / 181-243 in fp64 with
    torch autograd: outputs and every gradient; lengths off the 32-tile, head widths off the 32-channel tile, ragged masks with an
    all-padding item, per-head and shared relative tables, no window, dropout with the kernel's own mask restated on the host."""
    from visinger_amd.autograd import AttnCoreFn
    g = torch.Generator().manual_seed(B * 1000 + nh * 100 + dk + T)
    C = nh * dk
    q, k, v = (torch.randn(B, C, T, generator=g).cuda().requires_grad_(True) for _ in range(3))
    R = 2 * w + 1 if w is not None else 0
    rel_k = (torch.randn(nh_rel, R, dk, generator=g) * dk ** -0.5).cuda().requires_grad_(True) if w is not None else None
    rel_v = (torch.randn(nh_rel, R, dk, generator=g) * dk ** -0.5).cuda().requires_grad_(True) if w is not None else None
    mask = torch.ones(B, T)
    if B > 1:
        mask[1, (2 * T) // 3:] = 0
    if B > 2:
        mask[2] = 0                                                       # all padding: uniform rows, as the reference's -1e4 fill gives
    mask = mask.cuda()
    gout = torch.randn(B, C, T, generator=g).cuda()
    torch.manual_seed(77)
    state = torch.get_rng_state()
    out = AttnCoreFn.apply(q, k, v, rel_k, rel_v, mask, nh, w if w is not None else -1, p_drop)
    leaves = [t for t in (q, k, v, rel_k, rel_v) if t is not None]
    grads = torch.autograd.grad(out, leaves, gout)
    keep = None
    if p_drop > 0:
        torch.set_rng_state(state)
        seed = int(torch.empty((), dtype=torch.int64).random_())          # the draw AttnCoreFn.forward made
        keep = _hash_keep(seed, B, nh, T, p_drop, "cuda")
        assert abs(float((keep > 0).double().mean()) - (1 - p_drop)) < 0.03
    dl = [t.detach().double().requires_grad_(True) for t in leaves]
    it = iter(dl)
    qd, kd, vd = next(it), next(it), next(it)
    rkd, rvd = (next(it), next(it)) if w is not None else (None, None)
    ref = _attn_core_torch(qd, kd, vd, rkd, rvd, mask.double(), nh, w, keep)
    rgrads = torch.autograd.grad(ref, dl, gout.double())
    err = float((out.detach().double() - ref.detach()).abs().max())
    assert err <= 2e-5 * max(1.0, float(ref.abs().max())), err
    for name, a, b in zip(("dq", "dk", "dv", "drel_k", "drel_v"), grads, rgrads):
        e = float((a.double() - b).abs().max())
        assert e <= 3e-5 * max(1.0, float(b.abs().max())), (name, e, float(b.abs().max()))


def test_training_transformer_layer_uses_the_streaming_attention(vs_option):
    """autograd.attention routes the training-mode core through AttnCoreFn: a relative encoder's output and parameter gradients are those of
    the PyTorch [T, T] version of the same function (VS_NO_TRAIN_ATTN) with dropout off."""
    from visinger_amd import autograd as A
    from visinger_amd.modules.rel_transformer import RelativeEncoder
    torch.manual_seed(5)
    enc = RelativeEncoder(192, 768, 2, 2, kernel_size=9, p_dropout=0.0, window_size=4).cuda().train()
    x = torch.randn(2, 192, 90).cuda()
    mask = torch.ones(2, 1, 90).cuda()
    mask[1, :, 61:] = 0
    res = []
    for off in (False, True):
        if off:
            vs_option("VS_NO_TRAIN_ATTN", 1)
        xi = x.clone().requires_grad_(True)
        y = A.rel_encoder(enc, xi, mask)
        ps = [p for p in enc.parameters() if p.requires_grad]
        gs = torch.autograd.grad((y * torch.linspace(-1, 1, 90, device="cuda")).sum(), [xi] + ps, allow_unused=True)
        res.append((y.detach(), gs))
    (y1, g1), (y2, g2) = res
    assert float((y1 - y2).abs().max()) <= 2e-5 * float(y2.abs().max())
    for a, b in zip(g1, g2):
        assert (a is None) == (b is None)
        if a is not None:
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-6


def test_fused_qkv_projection_is_one_handle_for_inference_and_training():
    """The q | k | v projection of an attention layer is ONE handle in the layer's table (ops.handles), shared by the fused inference path and the
    training path and keyed by ops.param_key over the three convs: packed once per version of their parameters whichever mode asks first, re-packed
    after bump_weight_epoch() / repack_weights() (edits through `.data`), and moved between arithmetics by set_math alone (no pack), with the bits
    of a fresh pack in that arithmetic."""
    from visinger_amd import _lib as L
    from visinger_amd import ops
    from visinger_amd.modules.hipconv import repack_weights, set_conv_math
    from visinger_amd.modules.rel_transformer import RelativeEncoder

    def build():
        return RelativeEncoder(64, 128, 2, 1, kernel_size=3, p_dropout=0.0, window_size=4).cuda()

    torch.manual_seed(11)
    enc = build()
    att = enc.attn_layers[0]
    x = torch.randn(2, 64, 40).cuda()
    mask = torch.ones(2, 1, 40).cuda()
    mask[1, :, 27:] = 0

    def infer(m):
        m.eval()
        with torch.no_grad():
            return m(x, mask)

    def qkv_op():
        return ops.handles(att).get(("fwd", L.CONV1D, 0))

    packed, orig = [], ops.ConvOp._pack

    def counting(self, *args):
        packed.append(self)
        return orig(self, *args)

    def packs():
        return sum(o is qkv_op() for o in packed)

    ops.ConvOp._pack = counting
    try:
        y0 = infer(enc)
        op = qkv_op()
        assert op is not None and (op.c_in, op.c_out, op.k) == (64, 192, 1) and packs() == 1
        enc.train()
        yt = enc(x.clone().requires_grad_(True), mask)
        yt.sum().backward()
        assert att.conv_q.weight.grad is not None and ops.handles(att).get("dxa") is not None      # (its grad-input twin, in the same table)
        y1 = infer(enc)
        assert qkv_op() is op and packs() == 1
        assert torch.equal(y1, y0)
        d = float((yt.detach() - y0).abs().max())
        print("train vs eval forward: max |d| =", d, "of", float(y0.abs().max()))
        assert d <= 2e-5 * max(1.0, float(y0.abs().max())), d              # (the bound of test_train_forward_equals_eval_forward)
        # another arithmetic and back: set_math re-packs from the fp32 fragments the handle keeps
        set_conv_math(enc, L.MATH_F32)
        yf = infer(enc)
        assert qkv_op() is op and op.math == L.MATH_F32
        set_conv_math(enc, None)
        y2 = infer(enc)
        assert packs() == 1 and torch.equal(y2, y0)
        fresh = build()
        fresh.load_state_dict(enc.state_dict())
        assert torch.equal(infer(set_conv_math(fresh, L.MATH_F32)), yf)
        # an edit the parameter versions cannot see
        att.conv_q.weight.data.mul_(1.5)
        ops.bump_weight_epoch()
        y3 = infer(enc)
        assert qkv_op() is op and packs() == 2 and not torch.equal(y3, y0)
        repack_weights(enc)
        y4 = infer(enc)
        assert packs() == 3 and torch.equal(y4, y3)
    finally:
        ops.ConvOp._pack = orig


def test_training_step_packs_each_weight_version_once(vs_option):
    """ConvOp.bind / ops.param_key: within one optimizer step the discriminators' convs see their (unchanged)
    parameters three times (real + generated batch in the generator pass, both in the discriminator pass) and every handle packs them
    once; after an optimizer step the versions differ and they are packed again.  The cached and the uncached run produce the SAME
    losses and parameters bit for bit (the packed bytes are identical), at fewer packs."""
    from visinger_amd import ops
    from visinger_amd.train import VISingerTrainer, synthetic_train_batch
    hp = json.load(open(os.path.join(GOLDEN, "visinger_tiny_hparams.json")))
    hp = dict(hp, use_pitch_embed=True, pitch_predictor_layers=1, segment_size=8, p_dropout=0.0)

    def run(no_cache):
        vs_option("VS_NO_PACK_CACHE", 1 if no_cache else 0)
        torch.manual_seed(0)
        tr = VISingerTrainer(64, 117, 131, hp, dict(fft_size=64, win_size=32, num_mel_bins=16, fmin=0.0, fmax=4000.0, sample_rate=8000))
        tr = tr.cuda().train().configure()
        batch = synthetic_train_batch(2, 48, 6, tr.hop, 64, hp["num_linear_bins"], 1, "cuda")
        g = torch.Generator().manual_seed(3)
        batch["noise_q"] = torch.randn(2, hp["hidden_size"], 48, generator=g).cuda()
        batch["u_slice"] = torch.rand(2, generator=g).cuda()
        packs, orig = [0], ops.ConvOp._pack

        def counting(self, *args):
            packs[0] += 1
            return orig(self, *args)

        ops.ConvOp._pack = counting
        try:
            logs = [tr.training_step(batch) for _ in range(3)]
        finally:
            ops.ConvOp._pack = orig
        return logs, packs[0], [p.detach().clone() for p in tr.parameters()]

    logs_c, packs_c, params_c = run(False)
    logs_u, packs_u, params_u = run(True)
    assert packs_c < 0.8 * packs_u, (packs_c, packs_u)
    assert logs_c == logs_u                                                   # three steps, every loss term, bit for bit
    assert all(torch.equal(a, b) for a, b in zip(params_c, params_u))


@pytest.mark.gpu
def test_config3_training_step_at_full_size(vs_option):
    """BASELINE config 3 at ITS OWN size (B = 16, T_mel = 512, segment 32, hop 256, the reference-width generator and
    MPD / MSD, dropout 0): the gradients of every parameter of both passes from the HIP path against PyTorch-ROCm autograd of the SAME module
    graph with stock aten ops in place of every HIP kernel (tests/aten_backend.py: F.conv1d / F.conv_transpose1d, torch gate / LayerNorm /
    [T, T] attention).  At this size the dispatch takes other instances than at the fixture size of test_gradients_match_reference_autograd
    (which pins the graph itself to the reference's autograd): they are asserted by name.  The mel transform stays on the engine in both runs
    (parity unpinned: SURVEY 8c).  Tolerance: 2e-3 of each gradient's largest magnitude."""
    from visinger_amd import _lib as L
    from visinger_amd.models.visinger import hop256_hparams
    from visinger_amd.ops import PROFILER
    from visinger_amd.train import VISingerTrainer, synthetic_train_batch
    vs_option("VS_CONV_MATH", 3)
    hp = hop256_hparams(p_dropout=0.0)
    torch.manual_seed(1234)
    tr = VISingerTrainer(64, 117, 131, hp).cuda().configure().train()
    B, T = 16, 512
    batch = synthetic_train_batch(B, T, T // 8, tr.hop, 64, hp["num_linear_bins"], 1234, torch.device("cuda"))
    g = torch.Generator().manual_seed(7)
    batch["noise_q"] = torch.randn(B, hp["hidden_size"], T, generator=g).cuda()          # the posterior's reparameterisation draw
    batch["u_slice"] = torch.rand(B, generator=g)                                         # the segment starts
    with torch.no_grad():                                                                # non-trivial flow (post convs are zero-initialised)
        for f in range(4):
            post = tr.model.flow.flows[2 * f].post
            post.weight.copy_(0.05 * torch.randn(post.weight.shape, generator=g))
            post.bias.copy_(0.05 * torch.randn(post.bias.shape, generator=g))

    def grads(aten):
        import contextlib
        from aten_backend import aten_backend
        with (aten_backend() if aten else contextlib.nullcontext()):
            return grads_(aten)

    def grads_(aten):
        out = {}
        for opt_idx in (0, 1):
            tr.zero_grad(set_to_none=True)
            if not aten and opt_idx == 0:
                PROFILER.start(count_only=True)
            parts = tr.backward_pass(batch, opt_idx)
            if not aten and opt_idx == 0:
                PROFILER.stop()
            own = tr.model if opt_idx == 0 else tr.mel_disc
            for n, p_ in own.named_parameters():
                if p_.grad is not None:
                    out[(opt_idx, n)] = p_.grad.detach().clone()
            out[("loss", opt_idx)] = {k: float(v.detach()) for k, v in parts.items()}
        for p_ in tr.parameters():
            p_.requires_grad_(True)
        return out

    hip = grads(False)
    instances = set(PROFILER.counts())
    ref = grads(True)
    # the instances this size dispatches to (the fixture-size test never reaches the first three)
    for name in ("conv_ktap_kernel<5, 0, 2, 0, 1, 4, 1, 1>", "conv_ktap_kernel<9, 0, 2, 0, 2, 2, 4, 1>", "conv_wgrad (vs_conv_wgrad)", "relattn_train_bwd"):
        assert any(k.startswith(name) for k in instances), (name, sorted(instances))
    for opt_idx in (0, 1):
        for k, v in ref[("loss", opt_idx)].items():
            assert abs(hip[("loss", opt_idx)][k] - v) <= 2e-3 * max(1.0, abs(v)), (k, hip[("loss", opt_idx)][k], v)
    checked, errs = 0, []
    for key, r in ref.items():
        if key[0] == "loss":
            continue
        assert key in hip, key
        # (a gradient that is zero in exact arithmetic -- the key bias of an attention layer: softmax is invariant to it -- is rounding noise
        #  of the order of 1e-8 on both sides: such tensors are held to an absolute bound on both sides instead of a relative one)
        if float(r.abs().max()) < 1e-5:
            assert float(hip[key].abs().max()) < 1e-5, key
            continue
        scale = float(r.abs().max())
        errs.append((float((hip[key] - r).abs().max()) / scale, float((hip[key] - r).norm() / r.norm()), key))
        checked += 1
    errs.sort(reverse=True)
    print("worst tensors (max error / scale, relative L2 error):")
    for e in errs[:12]:
        print("   %.2e  %.2e  %s" % e)
    print("median max-error / scale: %.2e" % errs[len(errs) // 2][0])
    worst = errs[0]
    # every tensor within 2e-3 of its scale in the L2 sense; the largest single element of any tensor within 5e-3 (two fp32 pipelines --
    # ours and MIOpen's -- through a 100-layer GAN graph with leaky-relu kinks: a handful of elements per tensor sit on a flipped kink)
    assert max(e[1] for e in errs) <= 2e-3, max(errs, key=lambda e: e[1])
    assert worst[0] <= 5e-3, worst
    assert checked >= 650, checked           # 859 tensors in the task: the rest receive no (or an exactly-zero) gradient in their pass
    print(f"config-3 full-size gradients: {checked} tensors, worst max-error / scale {worst[0]:.2e} ({worst[2]})")
