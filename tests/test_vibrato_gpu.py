"""Vibrato on the device (rule "f13", csrc/vibrato.hip, visinger_amd/vibrato.py): the offsets bit for bit against the numpy restatement at the
sizes where the two-direction scan can go wrong, the modulated curve against fp64, row independence, and the control through the model, the driver and a
captured graph."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

CHUNK = 256          # frames per step of vs_pitch_vibrato's walk (csrc/vibrato.hip): the T cases 255 / 256 / 257 straddle it, 513 two of them
SR = 24000
T_PH = 24


def cu(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared cases are read-only)


def runs_to_row(runs, T):
    """(mel2ph int64 [T], note_of_token int32 [T_PH]) of a list of (frames, note id) runs, one token a run, cut at T"""
    m2p, notes, t = np.zeros(T, np.int64), np.zeros(T_PH, np.int32), 0
    for k, (n, note) in enumerate(runs):
        assert k < T_PH
        notes[k] = note
        m2p[t:t + n] = k + 1
        t += n
        if t >= T:
            break
    return m2p, notes


# row 0, laid out against CHUNK = 256: a rest at the row's start; note 1 over frames 5 .. 599 -- three chunks -- on TWO tokens (its depth is read at the first);
# note 2 of one frame; note 3 ends exactly on the chunk boundary 768 and note 4 starts there: two adjacent notes; a rest; note 5; a rest at the row's end
ROW0 = [(5, 0), (295, 1), (300, 1), (1, 2), (167, 3), (132, 4), (40, 0), (120, 5), (40, 0)]


@functools.lru_cache(maxsize=None)
def case(T, variant):
    """a batch of three rows, its settings and its restatement (computed once, shared, read-only): variant 0 has the lengths (T, T - 1, 1), variant 1 the lengths
    (1, 0, T) and the settings rotated by one row, so that the row that is one long note meets the deepest setting -- one of the three has depth 0"""
    from visinger_amd import vibrato as V
    r = np.random.default_rng(4200 + T)
    rows = [runs_to_row(ROW0, T)]
    random_runs = [(int(r.integers(1, 41)) if k % 5 else int(r.integers(60, 200)), 0 if r.uniform() < 0.25 else 1 + k) for k in range(T_PH)]
    rows.append(runs_to_row(random_runs, T))                             # the row ends in padding when the runs do not fill it: mel2ph 0 inside the length
    rows.append(runs_to_row([(T, 7)], T))                                # one note over the whole row: every chunk carries both boundaries
    m2p, notes = np.stack([x[0] for x in rows]), np.stack([x[1] for x in rows])
    hop = 256
    settings = [V.check_args(SR, hop, depth_cents=50.0, rate_hz=5.5, delay_s=3.2 / 93.75, attack_s=7 / 93.75, release_s=5 / 93.75, min_note_s=2 / 93.75),
                V.check_args(SR, hop, depth_cents=1200.0, rate_hz=7.9, delay_s=0.0, attack_s=300 / 93.75, release_s=200 / 93.75, min_note_s=0.0),
                V.check_args(SR, hop, depth_cents=0.0, rate_hz=4.0)]
    lens = [T, max(T - 1, 0), 1]
    if variant:
        settings, lens = settings[-1:] + settings[:-1], [1, 0, T]
    prm = np.asarray(settings, dtype=np.int32)
    depth_q = np.full((3, T_PH), -1, np.int32)
    depth_q[0, 1], depth_q[0, 2] = 900, 5                                # note 1 of row 0: 900 at its first token; the 5 on its second token is never read
    depth_q[1, 5] = 0                                                    # one note of the random row is silenced
    curve = r.uniform(6.5, 9.5, (3, T)).astype(np.float32)
    off, out = V.vibrato_ref(curve, m2p, notes, prm, note_depth_q=depth_q, lengths=lens)
    for a in (m2p, notes, prm, depth_q, curve, off, out):
        a.setflags(write=False)
    return dict(curve=curve, mel2ph=m2p, notes=notes, params=prm, depth_q=depth_q, lengths=lens, off=off, out=out)


def launch(c, stride, with_depths=True):
    from visinger_amd import vibrato as V
    kw = dict(note_depth_q=cu(c["depth_q"]) if with_depths else None, lengths=torch.tensor(c["lengths"], dtype=torch.int64, device="cuda"))
    if stride == 1:
        return V.vibrato(cu(c["curve"]), cu(c["mel2ph"]), cu(c["notes"]), cu(c["params"]), **kw)
    pred = np.stack([c["curve"], np.random.default_rng(3).normal(size=c["curve"].shape).astype(np.float32)], axis=2)
    return V.vibrato(None, cu(c["mel2ph"]), cu(c["notes"]), cu(c["params"]), pred=cu(pred), **kw)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("T", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 1100])
def test_offsets_equal_the_restatement_bit_for_bit_and_the_curve_follows(T, stride):
    """offset_q bit for bit; curve_out the input's bits where the offset is 0 and within 1e-5 absolute of the fp64 restatement elsewhere -- the figure
    tests/test_pitch_gpu.py holds the same exp2f / log2f composition to for its cents.
    Measured on an MI355X: every offset equal; max |d curve| = 1.12e-6 (T = 1100: 1624 and 1099 modulated frames in the two batches)."""
    for variant in (0, 1):
        c = case(T, variant)
        out, off = launch(c, stride)
        torch.cuda.synchronize()
        assert off.dtype == torch.int32 and out.dtype == torch.float32 and tuple(off.shape) == tuple(out.shape) == (3, T)
        off, out = off.cpu().numpy(), out.cpu().numpy()
        assert np.array_equal(off, c["off"]), np.argwhere(off != c["off"])[:5]
        inside = np.arange(T)[None] < np.asarray(c["lengths"])[:, None]
        still = inside & (off == 0)
        assert np.array_equal(out[still].view(np.uint32), c["curve"][still].view(np.uint32))
        assert (out[~inside] == 0).all() and (off[~inside] == 0).all()
        moved = off != 0
        err = float(np.abs(out[moved] - c["out"][moved]).max()) if moved.any() else 0.0
        print(f"T = {T}, stride {stride}, variant {variant}: {int(moved.sum())} modulated frames, max |d curve| = {err:.3e}")
        assert err <= 1e-5
        if T >= CHUNK - 1:
            assert moved[0 if variant == 0 else 2].any()
    if T == 1100:                                                        # the fixture does what it says
        c = case(T, 0)
        o = c["off"]
        assert np.abs(o[0, 8:600]).max() > 700 and np.abs(o[0, 8:600]).max() <= 900           # the three-chunk note, at its own depth
        assert o[0, 600] == 0 and o[0, :5].sum() == 0 and not o[0, 900:940].any() and not o[0, 1060:].any()
        assert np.abs(o[0, 605:768]).max() > 700 and np.abs(o[0, 772:900]).max() > 700 and o[0, 768 + 3] == 0
        assert np.abs(o[2]).max() == 0 and np.abs(case(T, 1)["off"][2]).max() > 18000          # depth 0; one octave on the rotated settings


def test_default_depths_and_default_lengths():
    """note_depth_q = None is -1 everywhere; lengths = None is the count of non-zero frames of mel2ph, taken on the device"""
    from visinger_amd import vibrato as V
    c = case(2 * CHUNK + 1, 0)
    T = c["curve"].shape[1]
    m2p = c["mel2ph"].copy()
    m2p[0, T - 40:] = 0
    want, _ = V.vibrato_ref(c["curve"], m2p, c["notes"], c["params"])
    out, off = V.vibrato(cu(c["curve"]), cu(m2p), cu(c["notes"]), cu(c["params"]))
    assert np.array_equal(off.cpu().numpy(), want) and not want[0, T - 40:].any() and np.abs(want[0]).max() > 700
    assert (out[0, T - 40:] == 0).all()


def test_a_row_does_not_depend_on_the_batch_the_row_index_or_the_padding():
    from visinger_amd import vibrato as V
    T0, T1 = 2 * CHUNK + 1, 1100
    c, big = case(T0, 0), case(T1, 0)
    alone = V.vibrato(cu(c["curve"][:1]), cu(c["mel2ph"][:1]), cu(c["notes"][:1]), cu(c["params"][:1]), note_depth_q=cu(c["depth_q"][:1]),
                      lengths=torch.tensor([T0], device="cuda"))
    curve, m2p, notes, prm, dq = (big[k].copy() for k in ("curve", "mel2ph", "notes", "params", "depth_q"))
    curve[2, :T0], m2p[2, :T0], notes[2], prm[2], dq[2] = c["curve"][0], c["mel2ph"][0], c["notes"][0], c["params"][0], c["depth_q"][0]      # (the tail: other frames)
    both = V.vibrato(cu(curve), cu(m2p), cu(notes), cu(prm), note_depth_q=cu(dq), lengths=torch.tensor([T1, T1 - 1, T0], device="cuda"))
    assert torch.equal(both[1][2, :T0], alone[1][0]) and torch.equal(both[0][2, :T0].view(torch.int32), alone[0][0].view(torch.int32))
    assert not both[1][2, T0:].any() and not both[0][2, T0:].any() and alone[1][0].abs().max() > 700


def test_python_layer_refuses_the_wrong_tensors():
    from visinger_amd import _lib, vibrato as V
    c = case(CHUNK, 0)
    good = [cu(c["curve"]), cu(c["mel2ph"]), cu(c["notes"]), cu(c["params"])]
    for i, bad in ((0, good[0].double()[:, :5]), (1, good[1].int()), (1, good[1][:, :-1]), (2, good[2].long()), (2, good[2][:2]), (3, good[3].float()),
                   (3, good[3][:, :5]), (0, good[0].cpu())):
        args = list(good)
        args[i] = bad
        with pytest.raises(_lib.VisingerHipError):
            V.vibrato(*args)
    with pytest.raises(_lib.VisingerHipError):
        V.vibrato(*good, note_depth_q=good[2][:, :-1])
    with pytest.raises(_lib.VisingerHipError):
        V.vibrato(*good, lengths=torch.tensor([1, 2, 3], device="cuda", dtype=torch.int32))
    with pytest.raises(_lib.VisingerHipError):
        V.vibrato(good[0].clone().requires_grad_(), *good[1:])
    with pytest.raises(_lib.VisingerHipError):
        V.vibrato(good[0], *good[1:], pred=torch.zeros(3, CHUNK, 2, device="cuda"))


# ---- the model, the driver, a captured graph ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    from visinger_amd.models.visinger import VISinger
    w, a = load_golden("visinger_tiny_pitch")
    hp = json.load(open(os.path.join(GOLDEN, "visinger_tiny_pitch_hparams.json")))
    m = VISinger(13, 9, 7, hp)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    guide = dict(np.load(os.path.join(GOLDEN, "visinger_tiny_guide.npz")))
    n, nph = int((a["mel2ph"][0] > 0).sum()), int((a["text"][0] > 0).sum())
    item = dict(text_tokens=a["text"][0][:nph], pitch_tokens=a["pitch"][0][:nph], dur_tokens=a["dur"][0][:nph], mel2ph=a["mel2ph"][0][:n])
    items = [item, dict(item, mel2ph=item["mel2ph"][:n - 5])]
    return m.cuda().eval(), a, guide, items, int(np.prod(hp["upsample_rates"]))


def model_args(a):
    return [cu(a[k]) for k in ("text", "pitch", "dur", "mel2ph")], dict(spk_id=cu(a["spk_id"]), infer=True, noise=cu(a["noise"]))


def settings(B, hop, **kw):
    """settings that reach every note of a short score: no delay, no minimum length, ramps of two frames"""
    from visinger_amd import vibrato as V
    fps = SR / hop
    return V.params(B, SR, hop, "cuda", **dict(dict(depth_cents=100.0, rate_hz=fps / 7.3, delay_s=0.0, attack_s=2 / fps, release_s=2 / fps, min_note_s=0.0), **kw))


def test_model_sings_the_modulated_curve(tiny):
    from visinger_amd import pitch, vibrato as V
    m, a, guide, _, hop = tiny
    args, kw = model_args(a)
    B, T = a["mel2ph"].shape
    prm = settings(B, hop)
    one_note = torch.ones((B, a["text"].shape[1]), dtype=torch.int32, device="cuda")         # the whole item as one long note
    with torch.no_grad():
        plain = m(*args, **kw)
        none = m(*args, vibrato=None, **kw)
        assert sorted(plain) == sorted(none) and all(torch.equal(plain[k], none[k]) for k in plain)
        own = m(*args, pitch_shift_cents=0.0, **kw)                       # the unmodulated curve, reported
        ret = m(*args, vibrato=prm, note_of_token=one_note, **kw)
        pred = ret["f0_pred"]
        assert torch.equal(pred, plain["f0_pred"])
        curve, q = V.vibrato(None, args[3], one_note, prm, pred=pred)
        mask = (args[3] > 0).float().unsqueeze(1)
        _, want = pitch.pitch_condition(mask, pred=pred, f0_norm=curve, return_hz=True)
    assert torch.equal(ret["vibrato_q"], q) and q.dtype == torch.int32 and tuple(q.shape) == (B, T)
    got, want = ret["f0_hz"].double().cpu().numpy(), want.double().cpu().numpy()
    on = want > 0
    rel = float((np.abs(got - want)[on] / want[on]).max()) if on.any() else 0.0
    print(f"model under vibrato: {int(on.sum())} voiced frames, f0_hz max relative error = {rel:.3e}, max |q| = {int(q.abs().max())}")
    assert rel <= 1e-5 and np.array_equal(got > 0, on) and np.array_equal(on, own["f0_hz"].cpu().numpy() > 0)
    # the condition moves on voiced frames of the long note.  (ret["f0_hz"] reports the curve clamped to 50 .. 1250 Hz, and this fixture's untrained predictor sings
    # below that floor: the Hz report shows the modulation where the unmodulated curve is inside the range -- on the guide below -- so the curve itself is compared.)
    moved = ((curve != pred[..., 0]) & torch.from_numpy(on).cuda()).cpu().numpy()
    changed = (ret["f0_hz"] != own["f0_hz"]).cpu().numpy()
    audible = on & (own["f0_hz"].cpu().numpy() > 50.0) & (own["f0_hz"].cpu().numpy() < 1250.0) & (q.cpu().numpy() != 0)
    assert int(q.abs().max()) > 1000 and moved.any() and not changed[~on].any() and (changed[audible].all() if audible.any() else True)
    assert not torch.equal(ret["wav_out"], plain["wav_out"])             # the vibrato is heard
    # the default notes are those of the pitch tokens, made on the device
    by_tokens = m(*args, vibrato=prm, **kw)
    ref_q, _ = V.vibrato_ref(pred[..., 0].cpu().numpy(), a["mel2ph"], V.notes_of_tokens(a["pitch"]).numpy(), prm.cpu().numpy())
    assert np.array_equal(by_tokens["vibrato_q"].cpu().numpy(), ref_q)
    # a transposition moves the modulated curve
    up = m(*args, vibrato=prm, note_of_token=one_note, pitch_shift_cents=1200.0, **kw)
    both = on & (got < 600) & (got > 55)                                 # (kept clear of the clamp to 50 .. 1250 Hz)
    if both.any():
        assert np.abs(up["f0_hz"].cpu().numpy()[both] / (2.0 * got[both] + 1.0) - 1.0).max() <= 1e-4      # an octave up: Hz + 1 doubles
    # on a guide with the guide's voicing: unvoiced frames stay 0, voiced ones move
    f0_hz = cu(guide["f0_hz"])
    guided = m(*args, f0_hz=f0_hz, **kw)
    sung = m(*args, f0_hz=f0_hz, vibrato=prm, note_of_token=one_note, **kw)
    off = (guide["uv"] != 0) | (a["mel2ph"] == 0)
    g, s = guided["f0_hz"].cpu().numpy(), sung["f0_hz"].cpu().numpy()
    assert (s[off] == 0).all() and np.array_equal(s > 0, g > 0) and (s != g)[~off].any() and (~off).sum() > 10
    for bad in (dict(note_of_token=one_note), dict(note_depth_q=one_note), dict(vibrato=prm, infer=False)):
        with pytest.raises(ValueError):
            m(*args, **dict(kw, **bad))


def test_model_modulates_the_retimed_alignment(tiny):
    from visinger_amd import vibrato as V
    m, a, _, _, hop = tiny
    args, kw = model_args(a)
    B = a["mel2ph"].shape[0]
    prm = settings(B, hop, depth_cents=80.0)
    seeds = torch.arange(B, dtype=torch.int64, device="cuda") + 11
    with torch.no_grad():
        ret = m(*args, spk_id=kw["spk_id"], infer=True, seeds=seeds, tempo=0.8, vibrato=prm)
    m2p = ret["mel2ph"].cpu().numpy()
    assert m2p.shape[1] > a["mel2ph"].shape[1] and ret["vibrato_q"].shape == ret["mel2ph"].shape
    want, _ = V.vibrato_ref(ret["f0_pred"][..., 0].cpu().numpy(), m2p, V.notes_of_tokens(a["pitch"]).numpy(), prm.cpu().numpy())
    assert np.array_equal(ret["vibrato_q"].cpu().numpy(), want) and np.abs(want).max() > 100


def test_driver_option_shows_in_the_curve_and_zero_depth_is_todays_waveform(tiny):
    from visinger_amd import synth
    m, _, _, bare_items, hop = tiny
    r = np.random.default_rng(17)
    items = []
    for it in bare_items:                # on guide curves inside the 50 .. 1250 Hz range return_f0 reports (the fixture's untrained predictor sings below it)
        f0 = r.uniform(80.0, 900.0, len(it["mel2ph"])).astype(np.float32)
        f0[:2], f0[7:11], f0[-1] = 0, 0, 0
        items.append(dict(it, f0=f0))
    fps = SR / hop
    opt = dict(sample_rate=SR, depth_cents=100.0, rate_hz=fps / 7.3, delay_s=0.0, attack_s=2 / fps, release_s=2 / fps, min_note_s=0.0)
    kw = dict(equal_tokens=True, seeds=[5, 99])
    plain = synth.synthesize(m, items, hop, return_f0=True, **kw)
    sung = synth.synthesize(m, items, hop, return_f0=True, vibrato=opt, **kw)
    for (w0, f0), (w1, f1) in zip(plain, sung):
        assert w0.shape == w1.shape and f0.shape == f1.shape and np.array_equal(f0 > 0, f1 > 0)
        if (f0 > 0).any():
            assert (f0 != f1).any() and np.abs(w0 - w1).max() > 1e-6
            cents = 1200 * np.log2((f1[f0 > 0] + 1) / (f0[f0 > 0] + 1))
            inside = (f0[f0 > 0] > 51) & (f0[f0 > 0] < 1249) & (f1[f0 > 0] > 51) & (f1[f0 > 0] < 1249)
            assert np.abs(cents[inside]).max(initial=0.0) <= 100.0 + 0.1
    assert any((f > 0).any() for _, f in plain)
    # a depth of 0 on every token, items' own notes given: bit for bit the call without the option, on the same seeds -- on the predictor's own curve
    # (today's aten path) and on a guide
    nph = len(items[0]["text_tokens"])
    for its in (bare_items, items):
        silent = [dict(it, vibrato_depth_cents=np.zeros(nph), note_of_token=np.arange(1, nph + 1)) for it in its]
        bare = synth.synthesize(m, its, hop, **kw)
        quiet = synth.synthesize(m, silent, hop, vibrato=opt, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(bare, quiet))
    assert all(np.array_equal(x, y[0]) for x, y in zip(bare, plain))
    own = synth.synthesize(m, bare_items, hop, vibrato=opt, **kw)        # the predicted curve under vibrato: heard
    assert all(np.abs(x - y).max() > 1e-6 for x, y in zip(own, synth.synthesize(m, bare_items, hop, **kw)))
    # per-token depths: None / NaN fall back to the call's depth
    mixed = [dict(items[0], vibrato_depth_cents=[None] * nph), dict(items[1], vibrato_depth_cents=[float("nan")] * nph)]
    again = synth.synthesize(m, mixed, hop, return_f0=True, vibrato=opt, **kw)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(sung, again))
    # through captured graphs: the same waveforms
    graphs = {}
    graphed = synth.synthesize(m, items, hop, return_f0=True, vibrato=opt, graphs=graphs, **kw)
    assert len(graphs) == 1 and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(sung, graphed))


def test_graph_replays_under_other_settings(tiny):
    from visinger_amd import synth
    m, _, _, items, hop = tiny
    batch = synth.collate(items, "cuda")
    seeds = torch.tensor([5, 99], dtype=torch.int64, device="cuda")
    first, other = settings(2, hop), settings(2, hop, depth_cents=[30.0, 250.0], rate_hz=[4.0, 9.0], attack_s=0.05)

    def eager(prm):
        return m(batch["text_tokens"], batch["pitch_tokens"], batch["dur_tokens"], batch["mel2ph"], spk_id=batch["spk_id"], infer=True, mask_decoder=True,
                 seeds=seeds, vibrato=prm)
    with torch.no_grad():
        step = synth.GraphedStep(m, batch, None, True, seeds=seeds, vibrato=first)
        for prm in (other, first):                                        # each replay equals the eager call under the same tensor
            wav = step(batch, None, seeds=seeds, vibrato=prm).clone()
            want = eager(prm)
            assert torch.equal(wav, want["wav_out"]) and torch.equal(step.f0_hz_out, want["f0_hz"]) and torch.equal(step.vibrato_q_out, want["vibrato_q"])
        assert not torch.equal(eager(first)["vibrato_q"], eager(other)["vibrato_q"])
    with pytest.raises(ValueError):
        step(batch, None, seeds=seeds)                                    # captured with settings: replayed with some
