"""Seeded per-item sampling on the GPU (csrc/sample_ops.hip, visinger_amd/sampling.py) and through the model, the synthesis driver and the
graph replay: the kernel against the fp64 restatement of the stream (tests/test_sampling_cpu.py, written from the definition), the
invariances bit for bit, and (model, item, seed) -> waveform whatever else is in the batch."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from test_sampling_cpu import noise_ref

pytestmark = pytest.mark.gpu

S_MAX, S_HEX = (1 << 63) - 1, 0x0123456789abcdef


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def tiny():
    from visinger_amd.models.visinger import VISinger
    w, a = load_golden("visinger_tiny")
    hp = json.load(open(os.path.join(GOLDEN, "visinger_tiny_hparams.json")))
    m = VISinger(13, 9, 7, hp)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return m.cuda().eval(), a, hp, w


@pytest.fixture(scope="module")
def pair(tiny):
    """the items of test_batched_synthesis_driver_matches_single_items: item 0 and its 5-frames-shorter twin (same tokens)"""
    m, a, hp, _ = tiny
    n, nph = int((a["mel2ph"][0] > 0).sum()), int((a["text"][0] > 0).sum())
    item = dict(text_tokens=a["text"][0][:nph], pitch_tokens=a["pitch"][0][:nph], dur_tokens=a["dur"][0][:nph], mel2ph=a["mel2ph"][0][:n])
    return [item, dict(item, mel2ph=item["mel2ph"][:n - 5])], int(np.prod(hp["upsample_rates"]))


@pytest.mark.parametrize("B,H,T,takes,first", [(3, 6, 1, 1, 0), (1, 5, 300, 1, 0), (2, 192, 67, 3, 2)])
def test_stream_matches_the_fp64_restatement(B, H, T, takes, first):
    """1e-5 absolute: |n| <= 5.77 and logf, sqrtf, sincospif are good to a few fp32 ulp -> <~ 3e-6; the bar leaves 3x.
    Measured on an MI355X: 3.7e-8, 3.8e-7 and 5.5e-7 for the three cases."""
    from visinger_amd import sampling
    seeds = [0, S_MAX, S_HEX][:B] if B > 1 else [S_HEX]
    got = sampling.item_noise(seeds, H, T, takes=takes, first_take=first)
    assert got.shape == (B * takes, H, T) and got.dtype == torch.float32
    err = float(np.abs(got.cpu().double().numpy() - noise_ref(seeds, H, T, takes, first)).max())
    print(f"item_noise {(B, H, T, takes, first)}: max |kernel - fp64| = {err:.3e}")
    assert err <= 1e-5
    dev = sampling.item_noise(torch.tensor(seeds, dtype=torch.int64, device="cuda"), H, T, takes=takes, first_take=first)
    assert torch.equal(dev, got)                    # seeds as a device tensor: the same stream


def test_stream_is_invariant_bit_for_bit():
    from visinger_amd import sampling
    s = S_HEX
    row2 = sampling.item_noise([5, 11, s], 6, 40)[2, :, :24]
    alone = sampling.item_noise([s], 6, 24)[0]
    assert torch.equal(row2, alone)                                     # batch size, row, padded T
    three = sampling.item_noise([s, 9], 6, 24, takes=3)
    for k in range(3):
        one = sampling.item_noise([s, 9], 6, 24, takes=1, first_take=k)
        assert torch.equal(three[k], one[0]) and torch.equal(three[3 + k], one[1])      # K, and the item-major row order
    assert torch.equal(sampling.item_noise([s], 8, 24)[:, :6], alone[None])             # H
    assert not torch.equal(three[0], three[1]) and not torch.equal(three[0], three[3])


def test_prior_sample_matches_fp64_and_masks_exactly():
    """|z - ref| <= 1e-5 (1 + |ref|): about 8 fp32 ulp of the largest term.  Measured on an MI355X: 1.3e-7."""
    from visinger_amd import sampling
    B, H, T, takes, ns = 3, 6, 40, 2, 0.667
    g = torch.Generator().manual_seed(3)
    stats = torch.randn(B, 2 * H, T, generator=g)
    stats[:, H:] = torch.rand(B, H, T, generator=g) * 4.0 - 3.0                     # logs uniform in [-3, 1]
    lens = [40, 24, 1]
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()[:, None, :]        # [B, 1, T]
    seeds = [0, S_MAX, S_HEX]
    dstats, dmask = stats.cuda(), mask.cuda()
    mu, logs = torch.split(dstats, H, dim=1)                                           # the views FramePriorNetwork returns
    assert not mu.is_contiguous()
    z, eps = sampling.prior_sample(mu, logs, dmask, seeds, takes=takes, noise_scale=ns, return_noise=True)
    assert z.shape == eps.shape == (B * takes, H, T)
    assert torch.equal(eps, sampling.item_noise(seeds, H, T, takes=takes))
    n = noise_ref(seeds, H, T, takes)
    mu64, logs64 = (x.double().numpy().repeat(takes, axis=0) for x in torch.split(stats, H, dim=1))
    m64 = mask.double().numpy().repeat(takes, axis=0)
    ref = (mu64 + ns * n * np.exp(logs64)) * m64
    rel = float((np.abs(z.cpu().double().numpy() - ref) / (1.0 + np.abs(ref))).max())
    print(f"prior_sample: max |z - fp64| / (1 + |ref|) = {rel:.3e}")
    assert rel <= 1e-5
    zc = z.cpu().numpy()
    assert all((zc[b * takes + k, :, lens[b]:] == 0).all() for b in range(B) for k in range(takes))      # masked frames: exactly 0
    assert torch.equal(sampling.prior_sample(mu, logs, dmask, seeds, takes=takes, noise_scale=ns), z)    # without the noise output
    z0 = sampling.prior_sample(mu, logs, dmask, seeds, takes=takes, noise_scale=0.0)
    assert torch.equal(z0, (mu * dmask).repeat_interleave(takes, dim=0))
    # no mask = all ones; contiguous inputs and the split views give the same bits
    z1 = sampling.prior_sample(mu, logs, None, seeds, noise_scale=ns)
    assert torch.equal(z1, sampling.prior_sample(mu.contiguous(), logs.contiguous(), torch.ones(B, T, device="cuda"), seeds, noise_scale=ns))
    assert torch.equal(z1[0], z[0])                                                                        # (item 0 is unmasked, take 0)
    zb = sampling.prior_sample(mu.bfloat16(), logs.bfloat16(), dmask, seeds)
    assert zb.dtype == torch.bfloat16 and zb.shape == (B, H, T)


def test_model_seeded_matches_injected_noise(tiny):
    """the seeded path against the injected-noise path the reference golden pins: 1e-4 absolute (the waveform bar); the two may differ in
    the last bit of z_p (contraction, expf)"""
    from visinger_amd import sampling
    m, a, hp, _ = tiny
    args = [cu(a[k]) for k in ("text", "pitch", "dur", "mel2ph")]
    B, T = a["mel2ph"].shape
    seeds = [S_HEX, 17][:B]
    with torch.no_grad():
        seeded = m(*args, spk_id=cu(a["spk_id"]), infer=True, seeds=seeds)["wav_out"]
        injected = m(*args, spk_id=cu(a["spk_id"]), infer=True, noise=sampling.item_noise(seeds, m.hidden_size, T))["wav_out"]
        with pytest.raises(ValueError):
            m(*args, spk_id=cu(a["spk_id"]), infer=True, seeds=seeds, noise=cu(a["noise"]))
    err = float((seeded - injected).abs().max())
    print(f"model seeded vs injected: max |d wav| = {err:.3e}")
    assert seeded.shape == injected.shape and err <= 1e-4
    assert float(injected.abs().max()) > 1e-3


def test_driver_waveform_depends_on_item_and_seed_only(tiny, pair):
    from visinger_amd import synth
    m, _, _, _ = tiny
    items, hop = pair
    s = [S_HEX, 99]
    kw = dict(equal_tokens=True)
    both = synth.synthesize(m, items, hop, seeds=s, **kw)
    assert [len(w) for w in both] == [len(it["mel2ph"]) * hop for it in items] and all(w.dtype == np.float32 for w in both)
    alone = [synth.synthesize(m, [items[i]], hop, seeds=[s[i]], **kw)[0] for i in range(2)]
    rev = synth.synthesize(m, items[::-1], hop, seeds=s[::-1], **kw)[::-1]
    split = synth.synthesize(m, items, hop, seeds=s, max_frames_per_batch=len(items[0]["mel2ph"]), **kw)
    assert len(synth.bucket_by_length([len(it["mel2ph"]) for it in items], len(items[0]["mel2ph"]))) == 2
    for name, other in (("alone", alone), ("reversed", rev), ("split", split)):
        errs = [float(np.abs(x - y).max()) for x, y in zip(both, other)]
        print(f"driver {name}: max |d wav| = {errs}")
        assert max(errs) <= 2e-6, name
    assert all(np.array_equal(x, y) for x, y in zip(both, synth.synthesize(m, items, hop, seeds=s, **kw)))                # run to run
    budget = len(items[0]["mel2ph"])                                                                                       # two batches, two streams
    one = synth.synthesize(m, items * 2, hop, seeds=s + s, max_frames_per_batch=2 * budget, streams=1, **kw)
    two = synth.synthesize(m, items * 2, hop, seeds=s + s, max_frames_per_batch=2 * budget, streams=2, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(one, two))
    other = synth.synthesize(m, items, hop, seeds=[S_HEX + 1, 99], **kw)
    assert np.abs(other[0] - both[0]).max() > 1e-4 and np.abs(other[1] - both[1]).max() <= 2e-6
    base = synth.synthesize(m, items, hop, seeds=7, **kw)                                                                  # one int: item i gets 7 + i
    assert all(np.array_equal(x, y) for x, y in zip(base, synth.synthesize(m, items, hop, seeds=[7, 8], **kw)))


def test_takes_share_one_prior_pass(tiny, pair):
    from visinger_amd import synth
    m, a, _, _ = tiny
    items, hop = pair
    s = [S_HEX, 99]
    seen = []
    hook = m.frame_prior.register_forward_hook(lambda mod, inp, out: seen.append((inp[0].shape[0], out[0].shape[0])))
    try:
        three = synth.synthesize(m, items, hop, seeds=s, takes=3, equal_tokens=True)
    finally:
        hook.remove()
    assert seen == [(2, 2)]                                          # the prior ran once, on B rows, not 3B
    assert [w.shape for w in three] == [(3, len(it["mel2ph"]) * hop) for it in items] and all(w.dtype == np.float32 for w in three)
    for k in range(3):
        one = synth.synthesize(m, items, hop, seeds=s, takes=1, first_take=k, equal_tokens=True)
        errs = [float(np.abs(three[i][k] - one[i]).max()) for i in range(2)]
        print(f"take {k}: max |d wav| = {errs}")
        assert max(errs) <= 2e-6
    assert np.abs(three[0][0] - three[0][1]).max() > 1e-4
    # the model's own rows are item-major: row b * takes + k is take k of item b
    batch = synth.collate(items, "cuda")
    call = lambda **kw: m(batch["text_tokens"], batch["pitch_tokens"], batch["dur_tokens"], batch["mel2ph"], spk_id=batch["spk_id"], infer=True,
                          mask_decoder=True, seeds=s, **kw)["wav_out"]
    with torch.no_grad():
        wav = call(takes=3)
        assert wav.shape[0] == 6
        for k in range(3):
            one = call(takes=1, first_take=k)
            assert float((wav[k] - one[0]).abs().max()) <= 2e-6 and float((wav[3 + k] - one[1]).abs().max()) <= 2e-6


def test_seeded_graph_replays_under_new_seeds(tiny, pair):
    from visinger_amd import synth
    m, _, _, _ = tiny
    items, hop = pair
    s, s2 = [S_HEX, 99], [4, S_MAX]
    plain = synth.synthesize(m, items, hop, seeds=s, equal_tokens=True)
    graphs = {}
    for _ in range(2):                                               # capture, then replay
        replayed = synth.synthesize(m, items, hop, seeds=s, equal_tokens=True, graphs=graphs)
        assert all(np.array_equal(x, y) for x, y in zip(replayed, plain))
    again = synth.synthesize(m, items, hop, seeds=s2, equal_tokens=True, graphs=graphs)      # same graph, seeds buffer overwritten
    plain2 = synth.synthesize(m, items, hop, seeds=s2, equal_tokens=True)
    assert all(np.array_equal(x, y) for x, y in zip(again, plain2))
    assert not np.array_equal(again[0], plain[0])
    assert len(graphs) == 1
    step = next(iter(graphs.values()))
    assert step.noise is None and step.seeds is not None
    # several takes per item capture and replay as well (their own graph: takes is part of the key)
    takes2 = synth.synthesize(m, items, hop, seeds=s, takes=2, equal_tokens=True)
    for _ in range(2):
        replayed = synth.synthesize(m, items, hop, seeds=s, takes=2, equal_tokens=True, graphs=graphs)
        assert all(np.array_equal(x, y) for x, y in zip(replayed, takes2))
    assert len(graphs) == 2
