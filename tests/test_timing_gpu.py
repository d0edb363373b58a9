"""Tempo and duration control on the GPU (csrc/timing_ops.hip, visinger_amd/timing.py) and through the model, the synthesis driver and the graph
replay: the two kernels bit for bit against the sequential restatement of tests/test_timing_cpu.py on every integer output, the warped curve exact
where it copies and within a few fp32 roundings where it blends, and the model / driver / graph on the retimed alignment."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from test_timing_cpu import D_ITEM0, align_ref, retime_ref, warp_ref

pytestmark = pytest.mark.gpu

CHUNK = 256          # tokens per step of vs_retime_tokens' scan (csrc/timing_ops.hip): the T_ph cases 255 / 256 / 257 / 775 straddle it
TEMPOS = (0.5, 1.0, 3.0)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def load_tiny_pitch():
    from visinger_amd.models.visinger import VISinger
    w, a = load_golden("visinger_tiny_pitch")
    hp = json.load(open(os.path.join(GOLDEN, "visinger_tiny_pitch_hparams.json")))
    m = VISinger(13, 9, 7, hp)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return m.cuda().eval(), a, hp


@pytest.fixture(scope="module")
def tiny_pitch():
    return load_tiny_pitch()


@pytest.fixture(scope="module")
def guided_pair():
    """test_pitch_gpu.py's item pair: item 0 of visinger_tiny_pitch and its 5-frames-shorter twin (same tokens), each with a guide curve"""
    m, a, hp = load_tiny_pitch()
    n, nph = int((a["mel2ph"][0] > 0).sum()), int((a["text"][0] > 0).sum())
    item = dict(text_tokens=a["text"][0][:nph], pitch_tokens=a["pitch"][0][:nph], dur_tokens=a["dur"][0][:nph], mel2ph=a["mel2ph"][0][:n])
    r = np.random.default_rng(17)
    f0 = r.uniform(80.0, 900.0, n).astype(np.float32)
    f0[:2], f0[7:11], f0[-7:-5], f0[-1] = 0, 0, 0, 0
    items = [dict(item, f0=f0), dict(item, mel2ph=item["mel2ph"][:n - 5], f0=f0[:n - 5].copy())]
    return m, items, int(np.prod(hp["upsample_rates"]))


def rows(T_ph):
    """three items (d [3][T_ph], stretch fp32 [3, T_ph], tempo [3]): random durations in [0, 12] with about 20 % empty tokens, stretch in [0.1, 4];
    row 1 carries a NaN, an inf, a 0 and a negative factor (the clamp rule); row 2 is all padding (length 0)"""
    r = np.random.default_rng(2000 + T_ph)
    d = r.integers(1, 13, (3, T_ph))
    d[r.uniform(size=(3, T_ph)) < 0.2] = 0
    d[2] = 0
    st = r.uniform(0.1, 4.0, (3, T_ph)).astype(np.float32)
    for j, bad in enumerate((np.nan, np.inf, 0.0, -2.0)):
        st[1, (j * 7) % T_ph] = bad
    return d, st, [TEMPOS[(T_ph + b) % 3] for b in range(3)]


def m2p_of(d, T):
    out = np.zeros((len(d), T), np.int64)
    for b, row in enumerate(d):
        m = np.repeat(np.arange(1, len(row) + 1), row)
        out[b, :len(m)] = m
    return out


@pytest.mark.parametrize("min_frames", [0, 1])
@pytest.mark.parametrize("T_ph", [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7])
def test_retime_matches_the_restatement_bit_for_bit(T_ph, min_frames):
    """cum_old, cum_new, lengths and mel2ph' equal retime_ref / align_ref exactly, from both input forms (mel2ph: the LDS histogram; dur), with and
    without a capacity that cuts a row, for T_out in {1, 255, 256, 257} and the natural width."""
    from visinger_amd import _lib, timing
    import ctypes
    d, st, tempo = rows(T_ph)
    refs = [retime_ref(d[b], st[b], tempo[b], min_frames) for b in range(3)]
    T = max(1, int(d.sum(1).max()))
    m2p = np.concatenate([m2p_of(d, T), np.zeros((3, 3), np.int64)], 1)                     # three frames of padding behind the longest row
    m2p[0, -1] = T_ph + 1                                                                    # ... and an index above T_ph, which is ignored
    dev = dict(stretch=cu(st), tempo=tempo, min_frames=min_frames)
    for form in (dict(mel2ph=cu(m2p), T_ph=T_ph), dict(dur=cu(d.astype(np.int64)))):
        got, lens, _ = timing.retime(**form, **dev)
        want_n = [r[2] for r in refs]
        assert lens.dtype == torch.int64 and lens.tolist() == want_n and want_n[2] == 0
        assert got.shape == (3, max(want_n)) and got.dtype == torch.int64
        for b in range(3):
            assert got[b].tolist() == align_ref(refs[b][1], want_n[b], max(want_n)), (form.keys(), b)
        cap = max(1, want_n[0] - 2)                                                          # row 0 is cut by the capacity
        for T_out in sorted({1, 255, 256, 257, cap}):
            got, lens, _ = timing.retime(**form, **dev, max_frames=T_out)
            assert got.shape == (3, T_out) and lens.tolist() == [min(n, T_out) for n in want_n]
            for b in range(3):
                assert got[b].tolist() == align_ref(refs[b][1], min(want_n[b], T_out), T_out), (form.keys(), b, T_out)
    # the token ends themselves, through the C ABI (timing.retime keeps them to itself)
    L = _lib.require_gpu()
    co, ce = torch.empty((3, T_ph), dtype=torch.int64, device="cuda"), torch.empty((3, T_ph), dtype=torch.int64, device="cuda")
    ln = torch.empty(3, dtype=torch.int64, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    m, s, tp = cu(m2p), cu(st), torch.tensor(tempo, dtype=torch.float32, device="cuda")
    _lib.check(L.vs_retime_tokens(vp(m), None, vp(s), vp(tp), min_frames, 0, vp(co), vp(ce), vp(ln), 3, m.shape[1], T_ph, _lib.stream_ptr()))
    for b in range(3):
        assert co[b].tolist() == refs[b][0] and ce[b].tolist() == refs[b][1], b
    steps = np.diff(np.concatenate([np.zeros((3, 1), np.int64), ce.cpu().numpy()], 1), axis=1)
    assert (steps >= np.where(d > 0, min_frames, 0)).all() and (steps[d == 0] == 0).all()


def test_floor_region_carries_the_prefix_max_across_every_chunk():
    from visinger_amd import timing
    d = np.array([[10] + [1] * 600], np.int64)
    st = np.array([[4.0] + [1 / 64] * 600], np.float32)
    c, e, n = retime_ref(d[0], st[0])
    assert (e[0], e[1], e[299], e[600], n) == (40, 41, 339, 640, 640)
    for form in (dict(dur=cu(d)), dict(mel2ph=cu(m2p_of(d, 610)), T_ph=601)):
        got, lens, _ = timing.retime(**form, stretch=cu(st))
        assert lens.tolist() == [640] and got[0].tolist() == align_ref(e, n, n)
    assert got[0, 39].item() == 1 and got[0, 40].item() == 2 and got[0, 639].item() == 601
    # pinned rows of the rule on item 0's durations
    d0 = cu(np.array([D_ITEM0], np.int64))
    for kw, ends in ((dict(tempo=2.0), [2, 4, 5, 7, 9, 12]), (dict(tempo=0.8), [4, 9, 11, 18, 21, 29]), (dict(tempo=4.0), [1, 2, 3, 4, 5, 6]),
                     (dict(tempo=4.0, min_frames=0), [1, 2, 2, 4, 4, 6]), (dict(stretch=[[1, 1, 1, 2.5, 1, 0.5]]), [3, 7, 9, 22, 25, 28])):
        got, lens, _ = timing.retime(dur=d0, **kw)
        assert lens.tolist() == [ends[-1]] and got[0].tolist() == align_ref(ends, ends[-1], ends[-1]), kw
    # device-side factors are used as they are: a tempo of 0 or NaN on the device gives a non-finite quotient, which counts as 1
    got, lens, _ = timing.retime(dur=d0.repeat(2, 1), tempo=torch.tensor([0.0, float("nan")], device="cuda"))
    assert lens.tolist() == [23, 23]


def test_curve_is_copied_exactly_and_blended_within_fp32_rounding():
    """zeros and copied frames (w = 0, or a neighbour unvoiced) equal warp_ref bit for bit; blended frames within 1e-6 * max(a, b) (the lerp is a handful
    of fp32 roundings, about 4 * 2^-24 relative); factor 1 reproduces the input bit for bit.  Measured on an MI355X: blended frames 2.1e-7 relative."""
    from visinger_amd import timing
    pinned = np.array([[0, 100, 110, 120, 130, 140, 150, 0, 0, 200, 210, 220, 230, 240, 250, 260, 270, 300, 310, 320, 330, 340, 350]], np.float32)
    d0 = cu(np.array([D_ITEM0], np.int64))
    _, _, got = timing.retime(dur=d0, tempo=2.0, curve=cu(pinned))
    assert got[0].tolist() == [0, 107.5, 125, 145, 0, 207.5, 232.5, 252.5, 267.5, 305, 325, 345]
    worst = 0.0
    for T_ph in (5, 70, CHUNK + 1):
        d, st, tempo = rows(T_ph)
        T = max(1, int(d.sum(1).max()))
        r = np.random.default_rng(T_ph)
        curve = r.uniform(80.0, 900.0, (3, T)).astype(np.float32)
        curve[r.uniform(size=(3, T)) < 0.3] = 0
        m2p = cu(m2p_of(d, T))
        same_m2p, same_len, same = timing.retime(mel2ph=m2p, T_ph=T_ph, curve=cu(curve))
        assert torch.equal(same_m2p, m2p) and same_len.tolist() == d.sum(1).tolist()
        inside = np.arange(T)[None, :] < d.sum(1)[:, None]
        assert np.array_equal(same.cpu().numpy(), np.where(inside, curve, 0))
        got_m2p, lens, got = timing.retime(mel2ph=m2p, T_ph=T_ph, stretch=cu(st), tempo=tempo, curve=cu(curve))
        got, n_blended = got.cpu().numpy(), 0
        for b in range(3):
            c, e, n = retime_ref(d[b], st[b], tempo[b])
            want, blended = warp_ref(curve[b], c, e, n, got.shape[1])
            assert np.array_equal(got[b][~blended], want[~blended]), (T_ph, b)
            assert ((got[b] == 0) == (want == 0)).all()
            if blended.any():
                lo = np.float32(1e-6) * want[blended]                           # want lies between a and b: a bound no wider than 1e-6 * max(a, b)
                err = np.abs(got[b][blended].astype(np.float64) - want[blended])
                worst = max(worst, float((err / want[blended]).max()))
                assert (err <= lo).all(), (T_ph, b, float((err / want[blended]).max()))
                n_blended += int(blended.sum())
        assert n_blended > 0 or T_ph == 5
    print(f"warped curve, blended frames: max relative |kernel - restatement| = {worst:.3e}")


def model_args(a):
    return [cu(a[k]) for k in ("text", "pitch", "dur", "mel2ph")], dict(spk_id=cu(a["spk_id"]), infer=True)


def test_model_tempo_one_is_the_plain_call(tiny_pitch):
    m, a, _ = tiny_pitch
    args, kw = model_args(a)
    with torch.no_grad():
        plain = m(*args, noise=cu(a["noise"]), **kw)
        one = m(*args, noise=cu(a["noise"]), tempo=1.0, **kw)
    assert torch.equal(one["mel2ph"], args[3]) and torch.equal(one["wav_out"], plain["wav_out"])
    assert one["frame_lengths"].tolist() == (args[3] > 0).sum(1).tolist() and "mel2ph" not in plain and "frame_lengths" not in plain


def test_model_under_a_tempo_and_a_stretch(tiny_pitch):
    from visinger_amd import timing
    m, a, hp = tiny_pitch
    hop = int(np.prod(hp["upsample_rates"]))
    args, kw = model_args(a)
    B, T_ph = args[0].shape
    seeds = torch.tensor([5, 99], dtype=torch.int64, device="cuda")
    tempo = [2.0, 0.8]
    st = np.ones((B, T_ph), np.float32)
    st[0, 3], st[1, 0] = 2.5, 0.5
    r = np.random.default_rng(3)
    f0 = r.uniform(80.0, 900.0, tuple(args[3].shape)).astype(np.float32)
    f0[:, 4:8] = 0
    f0[a["mel2ph"] == 0] = 0
    with torch.no_grad():
        ret = m(*args, seeds=seeds, tempo=tempo, ph_stretch=cu(st), f0_hz=cu(f0), **kw)
        new, lens, curve = timing.retime(mel2ph=args[3], T_ph=T_ph, stretch=cu(st), tempo=tempo, curve=cu(f0))
        by_hand = m(args[0], args[1], args[2], new, seeds=seeds, f0_hz=curve, **kw)
        plain = m(*args, seeds=seeds, f0_hz=cu(f0), **kw)
        unguided = m(*args, seeds=seeds, tempo=tempo, ph_stretch=st.tolist(), **kw)
    want = []
    for b in range(B):
        d = [int((a["mel2ph"][b] == i + 1).sum()) for i in range(T_ph)]
        want.append(retime_ref(d, st[b], tempo[b])[2])
    assert ret["frame_lengths"].tolist() == lens.tolist() == want and want[0] != int((a["mel2ph"][0] > 0).sum())
    assert torch.equal(ret["mel2ph"], new) and torch.equal(ret["wav_out"], by_hand["wav_out"]) and torch.equal(ret["f0_hz"], by_hand["f0_hz"])
    assert ret["wav_out"].shape == (B, max(want) * hop)
    n = min(ret["wav_out"].shape[1], plain["wav_out"].shape[1])
    assert float((ret["wav_out"][:, :n] - plain["wav_out"][:, :n]).abs().max()) > 1e-3                  # the tempo is heard
    # the sung curve is on the new timeline, voiced where the warped guide is
    assert ret["f0_hz"].shape == new.shape and torch.equal(ret["f0_hz"] > 0, (curve > 0) & (new > 0))
    assert torch.equal(unguided["mel2ph"], new) and "f0_hz" not in unguided and unguided["wav_out"].shape == ret["wav_out"].shape
    for bad in (dict(tempo=2.0, f0=cu(f0), uv=cu(f0)), dict(tempo=0.0), dict(tempo=[1.0]), dict(max_frames=64), dict(ph_stretch=[[1.0]])):
        with pytest.raises(ValueError):
            m(*args, seeds=seeds, **bad, **kw)
    with pytest.raises(ValueError):
        m(*args, tempo=2.0, spk_id=kw["spk_id"])                                                        # infer=False


def test_driver_retimes_per_item_and_leaves_the_items_alone(guided_pair):
    """each item of a two-item call under per-item tempos within 2e-6 of its own single-item call (the bar test_pitch_gpu.py has for ragged batches; measured
    on an MI355X: 0 for both), output lengths len' * hop, the caller's dicts untouched, and a call without the new arguments bit for bit today's."""
    from visinger_amd import synth
    m, items, hop = guided_pair
    s = [5, 99]
    kw = dict(equal_tokens=True, seeds=s)
    nph = len(items[0]["text_tokens"])
    st = np.ones(nph, np.float32)
    st[2] = 3.0
    timed = [dict(items[0]), dict(items[1], ph_stretch=st)]
    before = [{k: np.array(v, copy=True) for k, v in it.items()} for it in timed]
    tempo = [2.0, 0.8]
    both = synth.synthesize(m, timed, hop, tempo=tempo, return_f0=True, **kw)
    for it, was in zip(timed, before):
        assert it.keys() == was.keys() and all(np.array_equal(it[k], was[k]) for k in it)
    want = []
    for i, it in enumerate(timed):
        d = [int((it["mel2ph"] == j + 1).sum()) for j in range(nph)]
        want.append(retime_ref(d, it.get("ph_stretch"), tempo[i])[2])
    assert [len(w) for w, _ in both] == [n * hop for n in want] and [len(f) for _, f in both] == want
    for i in range(2):
        wav, f0 = synth.synthesize(m, [timed[i]], hop, seeds=[s[i]], equal_tokens=True, tempo=tempo[i], return_f0=True)[0]
        err = float(np.abs(wav - both[i][0]).max())
        print(f"driver item {i} alone under its tempo: max |d wav| = {err:.3e}")
        assert err <= 2e-6 and np.array_equal(f0, both[i][1])
    # a call without the new arguments: today's path, the same bits -- and tempo 1 with unit stretches is that path on equal inputs
    plain = synth.synthesize(m, items, hop, **kw)
    again = synth.synthesize(m, items, hop, tempo=None, **kw)
    unit = synth.synthesize(m, items, hop, tempo=1.0, **kw)
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(plain, again, unit))
    assert len(both[0][0]) != len(plain[0])


def test_graph_replays_under_another_tempo(guided_pair):
    from visinger_amd import synth
    m, items, hop = guided_pair
    batch = synth.collate(items, "cuda")
    T = batch["mel2ph"].shape[1]
    seeds = torch.tensor([5, 99], dtype=torch.int64, device="cuda")
    with torch.no_grad():
        step = synth.GraphedStep(m, batch, None, True, seeds=seeds, tempo=[1.0, 1.5], max_frames=2 * T)
        other = torch.tensor([0.6, 2.0], device="cuda")
        wav = step(batch, None, seeds=seeds, tempo=other).clone()
        lens, f0 = step.frame_lengths_out.clone(), step.f0_hz_out.clone()
        eager = m(batch["text_tokens"], batch["pitch_tokens"], batch["dur_tokens"], batch["mel2ph"], spk_id=batch["spk_id"], infer=True, mask_decoder=True,
                  seeds=seeds, f0_hz=batch["f0_hz"], tempo=other, max_frames=2 * T)
        first = m(batch["text_tokens"], batch["pitch_tokens"], batch["dur_tokens"], batch["mel2ph"], spk_id=batch["spk_id"], infer=True, mask_decoder=True,
                  seeds=seeds, f0_hz=batch["f0_hz"], tempo=[1.0, 1.5], max_frames=2 * T)
    assert wav.shape == (2, 2 * T * hop) and torch.equal(wav, eager["wav_out"]) and torch.equal(f0, eager["f0_hz"])
    assert torch.equal(lens, eager["frame_lengths"]) and not torch.equal(lens, first["frame_lengths"]) and not torch.equal(wav, first["wav_out"])
    want = [retime_ref([int((it["mel2ph"] == j + 1).sum()) for j in range(len(it["text_tokens"]))], None, t)[2] for it, t in zip(items, (0.6, 2.0))]
    assert lens.tolist() == want and max(want) <= 2 * T
    with pytest.raises(ValueError):
        step(batch, None, seeds=seeds)                                        # captured with a tempo: replayed with one
    with pytest.raises(ValueError):
        synth.GraphedStep(m, batch, None, True, seeds=seeds, tempo=2.0)       # no capacity
