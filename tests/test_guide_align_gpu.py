"""Guide alignment on the GPU (csrc/guide_align.hip, visinger_amd/guide_align.py) and through the synthesis driver: the kernel against the numpy
restatement ``align_ref`` of tests/test_guide_align_cpu.py BIT FOR BIT (the rule is integer once quantised; every test curve sits a quarter step off the
quantisation grid, where fp32 rounding cannot move it), independent of the launch, on every VS_EINVAL, under a graph replay, and as the driver's
``guide_align=`` pre-pass."""
import ctypes

import numpy as np
import pytest
import torch

from test_f0_extract_cpu import tone
from test_guide_align_cpu import align_ref, guide_of, hz_of_q, random_score, run_boundaries
from test_timing_gpu import load_tiny_pitch

pytestmark = pytest.mark.gpu

GRID = np.arange(52, 77)     # the coarse pitch grid of the random items: whole semitones, so equal costs -- ties -- are frequent


def cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def random_item(rng, T_ph, G, S=None, rest_p=0.2, unvoiced_p=0.2, max_dur=6):
    """(f0 [G], note_midi [T_ph], dur [T_ph]) with exactly S tokens of dur > 0 (default: about 80 %), pitches and guide segments from GRID"""
    S = int(round(0.8 * T_ph)) if S is None else S
    dur = np.zeros(T_ph, np.int64)
    dur[rng.choice(T_ph, S, replace=False)] = rng.integers(1, max_dur + 1, S)
    note = rng.choice(GRID, T_ph).astype(np.float32)
    note[rng.random(T_ph) < rest_p] = 0.0
    f0 = np.zeros(G, np.float32)
    t = 0
    while t < G:
        n = int(rng.integers(1, 9))
        f0[t:t + n] = 0.0 if rng.random() < unvoiced_p else hz_of_q(16 * int(rng.choice(GRID)))
        t += n
    return f0, note, dur


def device_align(items, Tg=None, T_ph=None, lengths="device", offsets=None, fill=(0.0, 0.0, 0), **kw):
    """items: (f0, note_midi, dur) per row, collated into one launch with `fill` beyond each row's own sizes; returns numpy (dur_new, cost, status)"""
    from visinger_amd import guide_align
    B = len(items)
    Tg = max(len(it[0]) for it in items) if Tg is None else Tg
    T_ph = max(len(it[1]) for it in items) if T_ph is None else T_ph
    f0, note, dur = np.full((B, Tg), fill[0], np.float32), np.full((B, T_ph), fill[1], np.float32), np.full((B, T_ph), fill[2], np.int64)
    for b, (f, n, d) in enumerate(items):
        f0[b, :len(f)], note[b, :len(n)], dur[b, :len(d)] = f, n, d
    g = [len(it[0]) for it in items]
    g = None if lengths is None else (torch.tensor(g, device="cuda") if lengths == "device" else g)
    offsets = None if offsets is None else cu(offsets)                                    # (a device tensor: used as it is, non-finite values included)
    out = guide_align.align_guide(cu(f0), cu(note), dur=cu(dur, np.int64), guide_lengths=g, offset_cents=offsets, **kw)
    assert out[0].shape == (B, T_ph) and out[0].dtype == torch.int64 and out[1].dtype == out[2].dtype == torch.int32 and out[1].shape == out[2].shape == (B,)
    return tuple(o.cpu().numpy() for o in out)


def check(items, offsets=None, **kw):
    """one launch over `items`, every row against the restatement of that row alone; returns the device result"""
    got = device_align(items, offsets=offsets, **kw)
    ref_kw = {k: v for k, v in kw.items() if k not in ("Tg", "T_ph", "lengths", "fill")}
    for b, (f0, note, dur) in enumerate(items):
        ref, cost, status = align_ref(f0, note, dur, offset_cents=0.0 if offsets is None else offsets[b], **ref_kw)
        n = len(dur)
        assert np.array_equal(got[0][b, :n], ref) and (got[0][b, n:] == 0).all(), (b, got[0][b].tolist(), ref.tolist())
        assert got[1][b] == cost and got[2][b] == status, (b, got[1][b], cost, got[2][b], status)
    return got


def test_one_wave():
    rng = np.random.default_rng(1)
    got = check([random_item(rng, 7, 40), random_item(rng, 7, 40, S=7), random_item(rng, 1, 1, S=1), random_item(rng, 3, 40, S=1)])
    assert (got[2] == 0).all() and got[0].sum(1).tolist() == [40, 40, 1, 40]


@pytest.mark.parametrize("S", [64, 65, 130])
def test_across_the_wave_boundary(S):
    """S = 64: the last column of a lone wave, no barrier; 65: one column beyond the boundary; 130: three waves"""
    rng = np.random.default_rng(S)
    items = [random_item(rng, S + 6, 3 * S + 11, S=S), random_item(rng, S, 2 * S, S=S, rest_p=0.0, unvoiced_p=0.0), random_item(rng, S + 1, S + 40, S=S, max_dur=2)]
    got = check(items)
    assert (got[2] == 0).all()


def test_the_largest_score():
    rng = np.random.default_rng(1024)
    got = check([random_item(rng, 1024, 1100, S=1024, max_dur=3)])
    assert got[2][0] == 0 and got[0].sum() == 1100 and (got[0] >= 1).all()


def test_forced_path_one_spare_frame_and_one_too_few():
    rng = np.random.default_rng(4)
    for S, T_ph in ((9, 12), (70, 70)):
        f0, note, dur = random_item(rng, T_ph, S + 1, S=S)
        got = check([(f0[:S], note, dur), (f0, note, dur), (f0[:S - 1], note, dur)])
        assert got[2].tolist() == [0, 0, 1] and got[1][2] == -1 and np.array_equal(got[0][2], dur)
        assert np.array_equal(got[0][0], (dur > 0).astype(np.int64))                      # G = S: one frame each


def test_backpointers_in_lds_and_in_the_workspace():
    """T_ph = 130 is three words a frame: G = 2000 is 6000 words -- beyond the 5120 of LDS, the workspace path; G = 400 fits.  Both in one launch (the
    shape needs the workspace, the short row does not use it), then the short one alone (no workspace allocated at all)"""
    from visinger_amd import guide_align
    rng = np.random.default_rng(6)
    long_, short = random_item(rng, 130, 2000, S=130, max_dur=30), random_item(rng, 130, 400, S=130)
    assert guide_align.workspace_bytes(2, 2000, 130) == 2 * 2000 * 3 * 8 and guide_align.workspace_bytes(1, 400, 130) == 0
    both = check([long_, short])
    alone = check([short])
    assert np.array_equal(both[0][1], alone[0][0]) and both[1][1] == alone[1][0]
    one_word = random_item(rng, 40, 5200, S=33, max_dur=300)                              # one word a frame, 5200 > 5120
    check([one_word])


def test_zero_durations_and_rest_padding():
    f0 = np.concatenate([hz_of_q(16 * 60 + np.zeros(9)), np.zeros(4), hz_of_q(16 * 64 + np.zeros(12)), np.zeros(6)]).astype(np.float32)
    note = np.array([60, 60, 99, 0, 64, 64, 0, 0, 0, 0], np.float32)
    dur = np.array([2, 5, 0, 3, 0, 11, 5, 0, 0, 0], np.int64)
    got = check([(f0, note, dur)])
    assert got[0][0].tolist() == [3, 6, 0, 4, 0, 12, 6, 0, 0, 0]


def test_an_unvoiced_guide_and_values_that_are_no_pitch():
    rng = np.random.default_rng(8)
    _, note, dur = random_item(rng, 90, 300, S=80)
    silent = np.zeros(300, np.float32)
    odd = rng.choice(np.array([np.nan, np.inf, -np.inf, -220.0, 0.0, -0.0], np.float32), 300)
    mixed = np.where(rng.random(300) < 0.5, odd, hz_of_q(16 * rng.choice(GRID, 300))).astype(np.float32)
    got = check([(silent, note, dur), (odd, note, dur), (mixed, note, dur)])
    assert np.array_equal(got[0][0], got[0][1]) and got[1][0] == got[1][1]                # every one of them is an unvoiced frame
    note2 = note.copy()
    note2[::7] = np.nan
    note2[3::7] = np.inf
    note2[5::7] = -60.0
    check([(mixed, note2, dur)])


def test_octave_fold_and_offsets():
    rng = np.random.default_rng(10)
    note, dur, runs = random_score(rng, notes=(8, 9))
    f0 = guide_of(runs, rng, octave_p=0.3, snap=True)
    plain = check([(f0, note, dur)])
    folded = check([(f0, note, dur)], octave_fold=True)
    assert folded[1][0] < plain[1][0]
    clean = guide_of(runs, snap=True)
    up, down = (clean * 2).astype(np.float32), (clean / 2).astype(np.float32)
    quarter = np.where(clean > 0, hz_of_q(np.rint(192 * np.log2(np.maximum(clean, 1) / 440.0)) + 1104 + 4), 0).astype(np.float32)
    got = check([(up, note, dur), (down, note, dur), (quarter, note, dur), (clean, note, dur)], offsets=[1200.0, -1200.0, 25.0, 0.0])
    assert (got[0] == got[0][3]).all() and (got[1] == got[1][3]).all()                    # the offset takes the transposition out again
    check([(up, note, dur), (clean, note, dur)], offsets=[float("nan"), float("inf")])    # a non-finite offset is 0


@pytest.mark.parametrize("kw", [dict(cap=7), dict(w_voiced_rest=5), dict(w_unvoiced_note=90), dict(drift=700), dict(drift_cap=3), dict(drift=0), dict(cap=0),
                                dict(cap=4096, w_voiced_rest=4096, w_unvoiced_note=4096, drift=4096, drift_cap=4096)])
def test_each_weight(kw):
    rng = np.random.default_rng(12)
    check([random_item(rng, 20, 70), random_item(rng, 70, 260, S=66)], **kw)


def test_fuzz_batch_of_256():
    rng = np.random.default_rng(256)
    items = []
    for _ in range(256):
        T_ph, G = int(rng.integers(1, 13)), int(rng.integers(1, 41))
        items.append(random_item(rng, T_ph, G, S=int(rng.integers(0, T_ph + 1))))
    got = check(items)
    assert 0 < got[2].sum() < 200


def test_an_item_does_not_depend_on_the_launch():
    from visinger_amd import guide_align
    rng = np.random.default_rng(14)
    f0, note, dur = random_item(rng, 100, 333, S=90)
    alone = guide_align.align_guide(cu(f0[None]), cu(note[None]), dur=cu(dur[None], np.int64))
    rows = [random_item(rng, 140, 500, S=140), random_item(rng, 30, 100, S=20), (f0, note, dur)]
    Tg, T_ph = 520, 150
    F0, N, D = np.full((3, Tg), 1e3, np.float32), np.full((3, T_ph), 61.0, np.float32), np.full((3, T_ph), -5, np.int64)
    F0[:, ::3] = np.nan
    for b, (f, n, d) in enumerate(rows):
        F0[b, :len(f)], N[b, :len(n)], D[b, :len(d)] = f, n, d
    lens = torch.tensor([500, 100, 333], device="cuda")
    got = guide_align.align_guide(cu(F0), cu(N), dur=cu(D, np.int64), guide_lengths=lens)
    assert torch.equal(got[0][2, :100], alone[0][0]) and (got[0][2, 100:] == 0).all() and got[1][2] == alone[1][0] and got[2][2] == alone[2][0] == 0
    ref = align_ref(f0, note, dur)
    assert np.array_equal(alone[0][0].cpu().numpy(), ref[0]) and int(alone[1][0]) == ref[1]
    # mel2ph instead of dur: the same durations through ops.mel2token_to_dur
    m2p = np.repeat(np.arange(1, 101), dur)
    via = guide_align.align_guide(cu(f0[None]), cu(note[None]), mel2ph=cu(m2p[None], np.int64))
    assert all(torch.equal(a, b) for a, b in zip(via, alone))


def test_every_einval_through_the_c_abi():
    from visinger_amd import _lib, guide_align
    L = _lib.require_gpu()
    B, Tg, T_ph = 2, 48, 9
    rng = np.random.default_rng(16)
    rows = [random_item(rng, T_ph, Tg) for _ in range(B)]
    f0, note = cu(np.stack([r[0] for r in rows])), cu(np.stack([r[1] for r in rows]))
    dur, lens, offs = cu(np.stack([r[2] for r in rows]), np.int64), torch.full((B,), Tg, dtype=torch.int64, device="cuda"), torch.zeros(B, device="cuda")
    out = torch.full((B, T_ph), -7, dtype=torch.int64, device="cuda")
    cost, status = torch.full((B,), -7, dtype=torch.int32, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda")
    work = torch.zeros(B * 6000 * 8, dtype=torch.int64, device="cuda")
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    good = dict(f0=f0, g_len=lens, note=note, dur=dur, offs=offs, cap=64, wvr=48, wun=24, drift=32, drift_cap=64, fold=0, reserved=0, out=out, cost=cost,
                status=status, work=None, nbytes=0, B=B, Tg=Tg, T_ph=T_ph)

    def call(**kw):
        a = dict(good, **kw)
        return L.vs_guide_align(vp(a["f0"]), vp(a["g_len"]), vp(a["note"]), vp(a["dur"]), vp(a["offs"]), a["cap"], a["wvr"], a["wun"], a["drift"], a["drift_cap"],
                                a["fold"], a["reserved"], vp(a["out"]), vp(a["cost"]), vp(a["status"]), vp(a["work"]), a["nbytes"], a["B"], a["Tg"], a["T_ph"],
                                _lib.stream_ptr())

    big = dict(Tg=6000, T_ph=1)                                                          # 6000 words a row: the workspace is required (f0 is not read: EINVAL)
    bad = [dict(f0=None), dict(note=None), dict(dur=None), dict(out=None), dict(cost=None), dict(status=None), dict(out=dur), dict(out=lens), dict(status=cost),
           dict(note=f0), dict(B=0), dict(B=-1), dict(T_ph=0), dict(T_ph=1025), dict(Tg=0), dict(Tg=65537), dict(cap=-1), dict(cap=4097), dict(wvr=-1),
           dict(wvr=4097), dict(wun=-1), dict(wun=4097), dict(drift=-1), dict(drift=4097), dict(drift_cap=-1), dict(drift_cap=4097), dict(fold=2), dict(fold=-1),
           dict(reserved=1), dict(big), dict(big, work=work, nbytes=B * 6000 * 8 - 1), dict(big, work=work, nbytes=0)]
    for kw in bad:
        assert call(**kw) == 1, kw                                             # VS_EINVAL
        assert b"vs_guide_align" in L.vs_last_error()
    torch.cuda.synchronize()
    assert (out == -7).all() and (cost == -7).all() and (status == -7).all()     # nothing was launched
    assert call() == 0 and call(g_len=None) == 0 and call(offs=None) == 0 and call(work=work, nbytes=8) == 0
    torch.cuda.synchronize()
    for b in range(B):
        ref = align_ref(*rows[b])
        assert np.array_equal(out[b].cpu().numpy(), ref[0]) and int(cost[b]) == ref[1] and int(status[b]) == ref[2]
    # the Python entry: ValueError / VisingerHipError before any launch
    for kw in (dict(cap=5000), dict(octave_fold=3), dict(guide_lengths=[Tg + 1, 0]), dict(guide_lengths=[1]), dict(offset_cents=float("inf")), dict(offset_cents=[0.0])):
        with pytest.raises(ValueError):
            guide_align.align_guide(f0, note, dur=dur, **kw)
    for args, kw in (((f0.cpu(), note), dict(dur=dur)), ((f0, note), dict()), ((f0, note), dict(dur=dur, mel2ph=dur)), ((f0.double(), note), dict(dur=dur)),
                     ((f0, note), dict(dur=dur.int())), ((f0, note[:, :5]), dict(dur=dur)), ((f0, note), dict(dur=dur, guide_lengths=lens.int())),
                     ((f0, note), dict(dur=dur, offset_cents=offs.double())), ((f0[0], note), dict(dur=dur))):
        with pytest.raises(_lib.VisingerHipError):
            guide_align.align_guide(*args, **kw)


def test_graph_replays_on_another_guide():
    from visinger_amd import guide_align
    rng = np.random.default_rng(18)
    Tg, T_ph = 1500, 200                                                                  # 1500 x 4 words: the workspace, allocated inside the capture
    f0, note = torch.zeros((2, Tg), device="cuda"), torch.zeros((2, T_ph), device="cuda")
    dur, lens = torch.zeros((2, T_ph), dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")

    def load(rows):
        F0, N, D = np.full((2, Tg), 1e3, np.float32), np.zeros((2, T_ph), np.float32), np.zeros((2, T_ph), np.int64)
        for b, (f, n, d) in enumerate(rows):
            F0[b, :len(f)], N[b, :len(n)], D[b, :len(d)] = f, n, d
        f0.copy_(cu(F0)), note.copy_(cu(N)), dur.copy_(cu(D, np.int64)), lens.copy_(torch.tensor([len(r[0]) for r in rows], device="cuda"))

    run = lambda: guide_align.align_guide(f0, note, dur=dur, guide_lengths=lens)
    load([random_item(rng, 200, 1500, S=190), random_item(rng, 60, 300)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    first = out[0].clone()
    rows = [random_item(rng, 150, 700, S=150), random_item(rng, 200, 1400, S=160)]
    load(rows)
    graph.replay()
    eager = run()
    assert all(torch.equal(a, b) for a, b in zip(out, eager)) and not torch.equal(out[0], first)
    for b, r in enumerate(rows):
        assert np.array_equal(out[0][b, :len(r[2])].cpu().numpy(), align_ref(*r)[0])


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------

TRACK = dict(sample_rate=24000, f0_min=300, f0_max=1000)     # tau_max = 80, W = 160 samples: 20 of the tiny model's 8-sample hops
DRIVER_WORST = 10            # frames: the worst run-boundary error of test_driver_sings_the_recordings_timing, measured on an MI355X (see its docstring)


@pytest.fixture(scope="module")
def driver():
    """visinger_tiny_pitch, item 0's tokens on a score of 40 frames a token, note pitches in pairs (consonant + vowel) with a rest between, and a recording of
    tone bursts that sings those notes with other lengths"""
    m, a, hp = load_tiny_pitch()
    nph = int((a["text"][0] > 0).sum())
    assert nph >= 5
    pitches = [72.0, 72.0, 0.0, 79.0, 79.0] + [67.0 + 5 * (j % 2) for j in range(nph - 5)]
    item = dict(text_tokens=a["text"][0][:nph], pitch_tokens=a["pitch"][0][:nph], dur_tokens=a["dur"][0][:nph], mel2ph=np.repeat(np.arange(1, nph + 1), 40),
                note_midi=np.array(pitches, np.float32))
    hop = int(np.prod(hp["upsample_rates"]))
    runs, j = [], 0                                                                       # (first token, tokens, midi) of each run
    while j < nph:
        k = j
        while k + 1 < nph and pitches[k + 1] == pitches[j]:
            k += 1
        runs.append((j, k - j + 1, pitches[j]))
        j = k + 1
    sung = [int(40 * r[1] * s) for r, s in zip(runs, [1.5, 0.6, 1.25, 0.8, 1.4, 0.7, 1.1, 0.9][:len(runs)])]
    rng = np.random.default_rng(21)
    rec = np.concatenate([np.zeros(n * hop) if r[2] == 0 else tone(440.0 * 2 ** ((r[2] - 69) / 12), n * hop, rng)[0] for r, n in zip(runs, sung)])
    return m, item, hop, runs, sung, rec.astype(np.float32)


def test_driver_sings_the_recordings_timing(driver):
    """synthesize(guide_align={}) on an item with "guide_wav" and "note_midi" equals synthesize on the items align_items returns, bit for bit; the waveform
    has G hop samples; the aligned run boundaries are where the recording has them within DRIVER_WORST + 1 frames.  Measured on an MI355X: the worst boundary
    error is printed by this test (the tracker's 160-sample window is 20 frames of this model's 8-sample hop: an onset is smeared over about that many)."""
    from visinger_amd import synth
    m, item, hop, runs, sung, rec = driver
    G = len(rec) // hop
    sung_item = dict(item, guide_wav=rec)
    before = {k: np.array(v, copy=True) for k, v in sung_item.items()}
    wav, f0 = synth.synthesize(m, [sung_item], hop, guide_track=TRACK, guide_align={}, seeds=7, return_f0=True)[0]
    assert sung_item.keys() == before.keys() and all(np.array_equal(sung_item[k], before[k]) for k in sung_item)
    tracked = synth.guide_items([sung_item], hop, "cuda", fit=False, **TRACK)
    assert tracked[0]["f0"].shape == (G,) and G == sum(sung) and G != len(item["mel2ph"])
    aligned = synth.align_items(tracked, "cuda")
    assert np.array_equal(aligned[0]["f0"], tracked[0]["f0"]) and len(aligned[0]["mel2ph"]) == G and np.array_equal(aligned[0]["dur_tokens"], item["dur_tokens"])
    wav2, f02 = synth.synthesize(m, aligned, hop, seeds=7, return_f0=True)[0]
    assert np.array_equal(wav, wav2) and np.array_equal(f0, f02) and len(wav) == G * hop
    dur_new = np.bincount(aligned[0]["mel2ph"], minlength=len(item["text_tokens"]) + 1)[1:]
    got, true = np.cumsum(dur_new)[[r[0] + r[1] - 1 for r in runs]], np.cumsum(sung)
    err = int(np.abs(got - true).max())
    print(f"driver: run boundaries {got.tolist()} against the recording's {true.tolist()}: worst error {err} frames (bar {DRIVER_WORST + 1})")
    assert (dur_new >= 1).all() and err <= DRIVER_WORST + 1
    # fit=True, the existing path, still cuts the curve at the score's frames
    fitted = synth.guide_items([sung_item], hop, "cuda", **TRACK)
    n = len(item["mel2ph"])
    assert fitted[0]["f0"].shape == (n,) and np.array_equal(fitted[0]["f0"][:min(n, G)], tracked[0]["f0"][:min(n, G)])


def test_driver_tempo_acts_on_the_aligned_item(driver):
    from visinger_amd import synth
    m, item, hop, runs, sung, rec = driver
    G = len(rec) // hop
    wav = synth.synthesize(m, [dict(item, guide_wav=rec)], hop, guide_track=TRACK, guide_align={}, seeds=7, tempo=2)[0]
    chain = synth.retime_items(synth.align_items(synth.guide_items([dict(item, guide_wav=rec)], hop, "cuda", fit=False, **TRACK), "cuda"), 2, "cuda")
    n2 = len(chain[0]["mel2ph"])
    assert len(wav) == n2 * hop and abs(n2 - G / 2) <= len(item["text_tokens"])          # half the aligned length, to a rounding per token
    assert np.array_equal(wav, synth.synthesize(m, chain, hop, seeds=7)[0])


def test_driver_token_table_errors_and_no_regression(driver):
    from visinger_amd import synth
    m, item, hop, runs, sung, rec = driver
    G = len(rec) // hop
    curve = synth.guide_items([dict(item, guide_wav=rec)], hop, "cuda", fit=False, **TRACK)[0]["f0"]
    # "pitch_tokens" through midi_of_token gives what "note_midi" gives
    table = np.zeros(16, np.float32)
    bare = {k: v for k, v in item.items() if k != "note_midi"}
    ids = np.asarray(bare["pitch_tokens"])
    assert ids.max() < 16
    for j, t in enumerate(ids):
        table[t] = item["note_midi"][j] if table[t] == 0 else table[t]
    by_table = synth.align_items([dict(bare, f0=curve)], "cuda", midi_of_token=table)
    by_notes = synth.align_items([dict(bare, f0=curve, note_midi=table[ids])], "cuda")
    assert np.array_equal(by_table[0]["mel2ph"], by_notes[0]["mel2ph"]) and len(by_table[0]["mel2ph"]) == G
    # items without a curve, or without token pitches, pass through
    same = synth.align_items([dict(bare), dict(bare, f0=np.zeros(len(bare["mel2ph"]), np.float32))], "cuda")
    assert all(np.array_equal(s["mel2ph"], bare["mel2ph"]) for s in same)
    for items, kw in (([dict(item, f0=curve)], dict(guide_align=dict(cap=-1))), ([dict(item, f0=curve)], dict(guide_align=dict(bogus=1))),
                      ([dict(item, f0=curve)], dict(guide_align=3)), ([dict(item, f0=curve[:2])], dict(guide_align={})),
                      ([dict(item, f0=curve, note_midi=item["note_midi"][:3])], dict(guide_align={})), ([dict(item, f0=curve[None])], dict(guide_align={})),
                      ([dict(bare, f0=curve)], dict(guide_align=dict(midi_of_token=table[:2]))), ([dict(item, f0=curve)], dict(guide_align=dict(offset_cents="a")))):
        with pytest.raises(ValueError):
            synth.synthesize(m, items, hop, seeds=7, **kw)
    with pytest.raises(ValueError, match="item 1"):
        synth.align_items([dict(item, f0=curve), dict(item, f0=curve[:2])], "cuda")
    # without guide_align nothing changes: the parent's path, a curve fitted to the score's frames
    sung_item = dict(item, guide_wav=rec)
    plain = synth.synthesize(m, [sung_item], hop, guide_track=TRACK, seeds=7)[0]
    given = synth.synthesize(m, synth.guide_items([sung_item], hop, "cuda", **TRACK), hop, seeds=7)[0]
    assert np.array_equal(plain, given) and len(plain) == len(item["mel2ph"]) * hop
    assert np.array_equal(synth.synthesize(m, [bare], hop, seeds=7)[0], synth.synthesize(m, [bare], hop, seeds=7, guide_align={})[0])
