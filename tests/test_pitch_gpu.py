"""Pitch-curve control on the GPU (csrc/pitch_ops.hip, visinger_amd/pitch.py) and through the model, the synthesis driver and the graph replay:
the kernels against the reference's own norm_interp_f0 outputs and the fp64 restatements of tests/test_pitch_cpu.py, the no-shift path bit for
bit against the aten expression it replaces, and the model on a guide curve against the reference's teacher-forced synthesis
(tests/golden/visinger_tiny_guide.npz)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from test_pitch_cpu import condition_ref, golden_rows, norm_interp_ref

pytestmark = pytest.mark.gpu

CHUNK = 256          # frames per step of vs_f0_norm_interp's walk (csrc/pitch_ops.hip): the T cases 255 / 256 / 257 straddle it


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def tiny_pitch():
    from visinger_amd.models.visinger import VISinger
    w, a = load_golden("visinger_tiny_pitch")
    hp = json.load(open(os.path.join(GOLDEN, "visinger_tiny_pitch_hparams.json")))
    m = VISinger(13, 9, 7, hp)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    guide = dict(np.load(os.path.join(GOLDEN, "visinger_tiny_guide.npz")))
    return m.cuda().eval(), a, hp, guide


@pytest.fixture(scope="module")
def guided_pair():
    """the item pair of test_sampling_gpu.py's `pair` fixture -- item 0 and its 5-frames-shorter twin (same tokens) -- built on visinger_tiny_pitch (the
    weights with a pitch condition), each with a guide curve"""
    from visinger_amd.models.visinger import VISinger
    w, a = load_golden("visinger_tiny_pitch")
    hp = json.load(open(os.path.join(GOLDEN, "visinger_tiny_pitch_hparams.json")))
    m = VISinger(13, 9, 7, hp)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    n, nph = int((a["mel2ph"][0] > 0).sum()), int((a["text"][0] > 0).sum())
    item = dict(text_tokens=a["text"][0][:nph], pitch_tokens=a["pitch"][0][:nph], dur_tokens=a["dur"][0][:nph], mel2ph=a["mel2ph"][0][:n])
    r = np.random.default_rng(17)
    f0 = r.uniform(80.0, 900.0, n).astype(np.float32)
    f0[:2], f0[7:11], f0[-7:-5], f0[-1] = 0, 0, 0, 0
    items = [dict(item, f0=f0), dict(item, mel2ph=item["mel2ph"][:n - 5], f0=f0[:n - 5].copy())]
    return m.cuda().eval(), items, int(np.prod(hp["upsample_rates"]))


def interp_rows(T):
    """three fp32 rows [3, T] with every kind of gap, and lengths (T, T - 5 or 1, 1)"""
    r = np.random.default_rng(1000 + T)
    f0 = r.uniform(80.0, 900.0, (3, T)).astype(np.float32)
    f0[r.uniform(size=(3, T)) < 0.4] = 0
    if T == 600:
        f0[0] = golden_rows()["two_anchors_600"][0]           # voiced at frames 3 and 580 only: the gap spans whole chunks
    elif T > 40:
        f0[0, :5] = 0
        f0[0, T - 9:] = 0
        f0[0, T // 2 - 20:T // 2 + 17] = 0
    return f0, [T, max(T - 5, 1), 1]


@pytest.mark.parametrize("T", [1, CHUNK - 1, CHUNK, CHUNK + 1, 600])
def test_norm_interp_matches_the_reference_and_the_restatement(T):
    """uv exact; voiced frames within 2e-6 (2 ulp of log2f at 8-16); interpolated frames within 1e-5 absolute (slope and one fma in fp32 on values
    <= 10.3: < 4e-6); frames beyond the lengths exactly 0.  Measured on an MI355X (max over the five T): voiced 9.4e-7, interpolated 1.3e-6; against the reference's own rows (next test) 9.5e-7."""
    from visinger_amd import pitch
    f0, lens = interp_rows(T)
    ref_norm, ref_uv = norm_interp_ref(f0, lens)
    got_norm, got_uv = pitch.norm_interp_f0(cu(f0), torch.tensor(lens, dtype=torch.int64, device="cuda"))
    assert got_norm.shape == got_uv.shape == (3, T) and got_norm.dtype == got_uv.dtype == torch.float32
    gn, gu = got_norm.cpu().double().numpy(), got_uv.cpu().numpy()
    inside = np.arange(T)[None, :] < np.array(lens)[:, None]
    voiced = inside & (f0 > 0)
    err_v = float(np.abs(gn - ref_norm)[voiced].max()) if voiced.any() else 0.0
    err_i = float(np.abs(gn - ref_norm)[inside & ~voiced].max()) if (inside & ~voiced).any() else 0.0
    print(f"norm_interp_f0 T={T}: max |kernel - fp64| voiced {err_v:.3e}, interpolated {err_i:.3e}")
    assert np.array_equal(gu, ref_uv)
    assert err_v <= 2e-6 and err_i <= 1e-5
    assert (gn[~inside] == 0).all() and (gu[~inside] == 0).all()
    # lengths = None: every row is T long
    full_norm, full_uv = pitch.norm_interp_f0(cu(f0))
    rn, ru = norm_interp_ref(f0)
    assert np.array_equal(full_uv.cpu().numpy(), ru) and float(np.abs(full_norm.cpu().double().numpy() - rn).max()) <= 1e-5
    if T == 600:                                               # ... and the reference's own output on that row
        _, want_norm, want_uv = golden_rows()["two_anchors_600"]
        assert np.array_equal(gu[0], want_uv) and float(np.abs(gn[0] - want_norm).max()) <= 1e-5


def test_norm_interp_matches_every_golden_row_and_is_invariant_bit_for_bit():
    from visinger_amd import pitch
    rows = golden_rows()
    Tmax = max(len(f0) for f0, _, _ in rows.values())
    batch = np.zeros((len(rows), Tmax), np.float32)
    for b, (f0, _, _) in enumerate(rows.values()):
        batch[b, :len(f0)] = f0
        batch[b, len(f0):] = 444.0                             # voiced rubbish beyond the length: takes no part
    lens = torch.tensor([len(f0) for f0, _, _ in rows.values()], dtype=torch.int64, device="cuda")
    got_norm, got_uv = pitch.norm_interp_f0(cu(batch), lens)
    worst = 0.0
    for b, (name, (f0, f0_norm, uv)) in enumerate(rows.items()):
        n = len(f0)
        assert np.array_equal(got_uv[b, :n].cpu().numpy(), uv), name
        voiced = f0 > 0
        err = np.abs(got_norm[b, :n].cpu().numpy().astype(np.float64) - f0_norm)
        assert (err[voiced] <= 2e-6).all() and (err[~voiced] <= 1e-5).all(), (name, float(err.max()))
        worst = max(worst, float(err.max()))
        assert float(got_norm[b, n:].abs().max() if n < Tmax else 0) == 0 and float(got_uv[b, n:].abs().max() if n < Tmax else 0) == 0
        # the row alone, unpadded, as row 0 of a batch of one: the same bits
        alone_norm, alone_uv = pitch.norm_interp_f0(cu(f0[None, :]))
        assert torch.equal(alone_norm[0], got_norm[b, :n]) and torch.equal(alone_uv[0], got_uv[b, :n]), name
    print(f"norm_interp_f0 against the reference's rows: max |kernel - reference| = {worst:.3e}")


def test_condition_without_a_shift_is_the_aten_expression_bit_for_bit():
    from visinger_amd import pitch
    B, T = 3, 67
    g = torch.Generator().manual_seed(11)
    raw = torch.randn(B, 2, T, generator=g)
    raw[:, 0] = raw[:, 0] * 1.5 + 7.5                           # log2 f0 around 180 Hz
    pred = raw.cuda().permute(0, 2, 1)                          # [B, T, 2] as the pitch predictor returns it: a strided view
    assert not pred.is_contiguous()
    lens = [67, 40, 1]
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()[:, None, :].cuda()      # [B, 1, T]
    f0n = (torch.rand(B, T, generator=g) * 4 + 6).cuda()
    uv = (torch.rand(B, T, generator=g) < 0.35).float().cuda()
    want_pred = (pred[:, :, 0] * (pred[:, :, 1] <= 0)).unsqueeze(1) * mask
    want_given = (f0n * (uv == 0)).unsqueeze(1) * mask
    got_pred = pitch.pitch_condition(mask, pred=pred)
    got_given = pitch.pitch_condition(mask, f0_norm=f0n, uv=uv)
    assert got_pred.shape == (B, 1, T) and torch.equal(got_pred, want_pred) and torch.equal(got_given, want_given)
    assert torch.equal(pitch.pitch_condition(mask, pred=pred, f0_norm=f0n, uv=uv), want_given)      # pred is then not looked at
    mixed = pitch.pitch_condition(mask, pred=pred, f0_norm=f0n)                                       # the given curve under the predicted voicing
    assert torch.equal(mixed, (f0n * (pred[:, :, 1] <= 0)).unsqueeze(1) * mask)
    assert torch.equal(pitch.pitch_condition(None, pred=pred), (pred[:, :, 0] * (pred[:, :, 1] <= 0)).unsqueeze(1))
    assert float(want_pred.abs().max()) > 1 and float(want_given.abs().max()) > 1
    # zero shifts, and zero-shift rows beside shifted ones: the same bits
    assert torch.equal(pitch.pitch_condition(mask, pred=pred, cents=0.0), want_pred)
    some, hz_some = pitch.pitch_condition(mask, f0_norm=f0n, uv=uv, cents=[0.0, 300.0, 0.0], return_hz=True)
    none, hz_none = pitch.pitch_condition(mask, f0_norm=f0n, uv=uv, return_hz=True)
    assert torch.equal(some[0], want_given[0]) and torch.equal(some[2], want_given[2]) and not torch.equal(some[1], want_given[1])
    assert torch.equal(hz_some[0], hz_none[0]) and torch.equal(hz_some[2], hz_none[2])
    dev = pitch.pitch_condition(mask, f0_norm=f0n, uv=uv, cents=torch.tensor([0.0, 300.0, 0.0], device="cuda"))
    assert torch.equal(dev, some)                                # the shifts as a device tensor


def test_shift_and_hz_output_match_the_fp64_restatement():
    """f0_hz_out within 1e-5 relative of the fp64 restatement (exp2f / log2f composed twice: a few ulp), cond within 1e-5 absolute; an octave up /
    down doubles / halves the curve where no clamp applies; clamped frames read exactly 50 / 1250, masked and unvoiced frames exactly 0.
    Measured on an MI355X: f0_hz_out 6.3e-7 relative shifted (5.1e-8 unshifted), cond 9.5e-7."""
    from visinger_amd import pitch
    B, T = 3, 67
    g = torch.Generator().manual_seed(12)
    f0n = torch.rand(B, T, generator=g) * 5.5 + 5.0              # 31 Hz .. 1450 Hz: both clamps are met, shifted and not
    uv = (torch.rand(B, T, generator=g) < 0.3).float()
    lens = [67, 40, 1]
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()
    cents = [1200.0, -1200.0, 37.5]
    cond, hz = pitch.pitch_condition(mask.cuda(), f0_norm=f0n.cuda(), uv=uv.cuda(), cents=cents, return_hz=True)
    base_cond, base_hz = pitch.pitch_condition(mask.cuda(), f0_norm=f0n.cuda(), uv=uv.cuda(), return_hz=True)
    ref_cond, ref_hz = condition_ref(mask.numpy(), f0_norm=f0n.numpy(), uv=uv.numpy(), cents=cents)
    ref_base_cond, ref_base_hz = condition_ref(mask.numpy(), f0_norm=f0n.numpy(), uv=uv.numpy())
    hz, base_hz, cond = hz.cpu().double().numpy(), base_hz.cpu().double().numpy(), cond[:, 0].cpu().double().numpy()
    on = (uv.numpy() == 0) & (mask.numpy() != 0)
    for name, got, ref in (("shifted", hz, ref_hz), ("unshifted", base_hz, ref_base_hz)):
        clamped = on & ((ref == 50.0) | (ref == 1250.0))
        free = on & ~clamped
        rel = float((np.abs(got - ref)[free] / ref[free]).max())
        print(f"pitch_condition f0_hz_out {name}: max relative error = {rel:.3e}")
        assert rel <= 1e-5
        assert clamped.any() and np.array_equal(got[clamped], ref[clamped]) and (got[~on] == 0).all()
    err = float(np.abs(cond - ref_cond).max())
    print(f"pitch_condition cond shifted: max |kernel - fp64| = {err:.3e}")
    assert err <= 1e-5 and (cond[~on] == 0).all()
    assert float(np.abs(base_cond[:, 0].cpu().double().numpy() - ref_base_cond).max()) <= 1e-6
    raw = 2.0 ** f0n.double().numpy() - 1.0
    for b, factor in ((0, 2.0), (1, 0.5)):
        free = on[b] & (raw[b] > 50) & (raw[b] < 1250) & (raw[b] * factor > 50) & (raw[b] * factor < 1250)
        assert free.sum() > 5
        assert float((np.abs(hz[b][free] - factor * base_hz[b][free]) / (factor * base_hz[b][free])).max()) <= 2e-5      # (both sides carry 1e-5)


def model_args(a):
    return [cu(a[k]) for k in ("text", "pitch", "dur", "mel2ph")], dict(spk_id=cu(a["spk_id"]), infer=True, noise=cu(a["noise"]))


def test_model_on_a_guide_curve_matches_the_reference(tiny_pitch):
    """m(..., f0_hz=) against the reference's forward(f0=, uv=) on its own norm_interp_f0 of each item: wav_out 1e-4, f0_pred 5e-5 (the bars these
    weights have in test_production_dispatch_gpu.py); ret["f0_hz"] within 1e-5 relative of denorm_f0 of the fixture's curve.
    Measured on an MI355X: wav_out 5.7e-7, f0_pred 9.5e-7, f0_hz 6.9e-7."""
    m, a, _, guide = tiny_pitch
    args, kw = model_args(a)
    with torch.no_grad():
        ret = m(*args, f0_hz=cu(guide["f0_hz"]), **kw)
        plain = m(*args, **kw)
        teacher = m(*args, f0=cu(guide["f0_norm"]), uv=cu(guide["uv"]), **kw)
    e_wav = float(np.abs(ret["wav_out"].cpu().numpy() - guide["wav_out"]).max())
    e_f0 = float(np.abs(ret["f0_pred"].cpu().numpy() - guide["f0_pred"]).max())
    print(f"model on a guide: max |d wav| = {e_wav:.3e}, max |d f0_pred| = {e_f0:.3e}")
    assert ret["wav_out"].shape == guide["wav_out"].shape and e_wav <= 1e-4 and e_f0 <= 5e-5
    assert float(np.abs(guide["wav_out"]).max()) > 1e-3
    # the curve that conditioned the prior, in Hz
    on = (guide["uv"] == 0) & (a["mel2ph"] > 0)
    want = np.where(on, np.clip(2.0 ** guide["f0_norm"].astype(np.float64) - 1.0, 50.0, 1250.0), 0.0)
    got = ret["f0_hz"].cpu().double().numpy()
    rel = float((np.abs(got - want)[on] / want[on]).max())
    print(f"model on a guide: f0_hz max relative error = {rel:.3e}")
    assert got.shape == want.shape and rel <= 1e-5 and (got[~on] == 0).all() and on.sum() > 10
    # without a new argument: today's path, no new key
    assert "f0_hz" not in plain and "f0_hz" not in teacher
    assert float(np.abs(plain["wav_out"].cpu().numpy() - a["wav_out"]).max()) <= 1e-4
    assert float((plain["wav_out"] - ret["wav_out"]).abs().max()) > 1e-3                     # the guide is heard
    assert float((teacher["wav_out"] - ret["wav_out"]).abs().max()) <= 1e-4


def test_model_voicing_and_shift_options(tiny_pitch):
    m, a, _, guide = tiny_pitch
    args, kw = model_args(a)
    f0_hz = cu(guide["f0_hz"])
    with torch.no_grad():
        guided = m(*args, f0_hz=f0_hz, **kw)
        by_model = m(*args, f0_hz=f0_hz, voicing="model", **kw)
        pred = by_model["f0_pred"]
        lengths = (args[3] > 0).sum(1)
        from visinger_amd import pitch
        f0n, _ = pitch.norm_interp_f0(f0_hz, lengths)
        by_hand = m(*args, f0=f0n, uv=(pred[:, :, 1] > 0).float(), **kw)
        assert torch.equal(by_model["wav_out"], by_hand["wav_out"]) and "f0_hz" in by_model and "f0_hz" not in by_hand
        assert not torch.equal(by_model["wav_out"], guided["wav_out"])
        zero = m(*args, f0_hz=f0_hz, pitch_shift_cents=0.0, **kw)
        assert torch.equal(zero["wav_out"], guided["wav_out"]) and torch.equal(zero["f0_hz"], guided["f0_hz"])
        up = m(*args, f0_hz=f0_hz, pitch_shift_cents=[700.0, 0.0], **kw)
        assert not torch.equal(up["wav_out"][0], guided["wav_out"][0]) and torch.equal(up["f0_hz"][1], guided["f0_hz"][1])
        # the predicted curve, shifted: no guide needed; a zero shift is today's waveform
        own = m(*args, pitch_shift_cents=0.0, **kw)
        plain = m(*args, **kw)
        assert torch.equal(own["wav_out"], plain["wav_out"]) and own["f0_hz"].shape == f0_hz.shape
        voiced = (pred[:, :, 1] <= 0) & (args[3] > 0)
        assert torch.equal(own["f0_hz"] > 0, voiced)
        for bad in (dict(f0_hz=f0_hz, f0=f0n), dict(f0_hz=f0_hz, uv=f0n), dict(voicing="tracker")):
            with pytest.raises(ValueError):
                m(*args, **bad, **kw)


def test_driver_on_guides_is_per_item(guided_pair):
    from visinger_amd import synth
    m, items, hop = guided_pair
    s = [5, 99]
    kw = dict(equal_tokens=True, seeds=s)
    both = synth.synthesize(m, items, hop, return_f0=True, **kw)
    assert [len(w) for w, _ in both] == [len(it["mel2ph"]) * hop for it in items]
    assert [len(f) for _, f in both] == [len(it["mel2ph"]) for it in items] and all(f.dtype == np.float32 for _, f in both)
    for i in range(2):
        wav, f0 = synth.synthesize(m, [items[i]], hop, seeds=[s[i]], equal_tokens=True, return_f0=True)[0]
        err = float(np.abs(wav - both[i][0]).max())
        print(f"driver item {i} alone: max |d wav| = {err:.3e}")
        assert err <= 2e-6 and np.array_equal(f0, both[i][1])
        assert np.array_equal(f0 > 0, items[i]["f0"] > 0)                   # voicing="guide": voiced where the guide is
        v = f0 > 0
        assert np.abs(f0[v] - np.clip(items[i]["f0"][v], 50, 1250)).max() <= 1e-5 * 1250
    plain = synth.synthesize(m, items, hop, **kw)
    assert all(np.array_equal(x, y[0]) for x, y in zip(plain, both))         # asking the curve back changes nothing
    shifted = synth.synthesize(m, items, hop, pitch_shift_cents=[0.0, -200.0], **kw)
    assert np.array_equal(shifted[0], plain[0]) and np.abs(shifted[1] - plain[1]).max() > 1e-4
    # guided and unguided items in one call: never one batch, each as if alone
    bare = {k: v for k, v in items[1].items() if k != "f0"}
    mixed = synth.synthesize(m, [items[0], bare], hop, **kw)
    assert np.abs(mixed[0] - plain[0]).max() <= 2e-6
    assert np.array_equal(mixed[1], synth.synthesize(m, [bare], hop, seeds=[s[1]], equal_tokens=True)[0])
    assert np.abs(mixed[1] - plain[1]).max() > 1e-4


def test_graph_replays_under_another_curve_and_shift(guided_pair):
    from visinger_amd import synth
    m, items, hop = guided_pair
    batch = synth.collate(items, "cuda")
    seeds = torch.tensor([5, 99], dtype=torch.int64, device="cuda")
    cents = torch.tensor([100.0, 0.0], device="cuda")
    with torch.no_grad():
        step = synth.GraphedStep(m, batch, None, True, seeds=seeds, cents=cents)
        other = dict(batch, f0_hz=torch.roll(batch["f0_hz"], 3, dims=1) * 1.25)
        other_cents = torch.tensor([-350.0, 1200.0], device="cuda")
        wav = step(other, None, seeds=seeds, cents=other_cents).clone()
        f0 = step.f0_hz_out.clone()
        eager = m(other["text_tokens"], other["pitch_tokens"], other["dur_tokens"], other["mel2ph"], spk_id=other["spk_id"], infer=True, mask_decoder=True,
                  seeds=seeds, f0_hz=other["f0_hz"], pitch_shift_cents=other_cents)
        first = m(batch["text_tokens"], batch["pitch_tokens"], batch["dur_tokens"], batch["mel2ph"], spk_id=batch["spk_id"], infer=True, mask_decoder=True,
                  seeds=seeds, f0_hz=batch["f0_hz"], pitch_shift_cents=cents)
    assert torch.equal(wav, eager["wav_out"]) and torch.equal(f0, eager["f0_hz"])
    assert not torch.equal(wav, first["wav_out"])
    with pytest.raises(ValueError):
        step(other, None, seeds=seeds)                                        # captured with a shift: replayed with one
