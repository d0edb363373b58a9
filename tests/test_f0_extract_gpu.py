"""The pitch tracker on the GPU (csrc/pitch_track.hip, visinger_amd/pitch_track.py) and through the synthesis driver: the kernel against the fp64
restatement ``yin_ref`` of tests/test_f0_extract_cpu.py on the frames the restatement itself decides unambiguously, against ground truth, bit-identical under
another launch shape, on the edges of the rule, under a graph replay, and as the driver's "guide_wav" pre-pass."""
import ctypes

import numpy as np
import pytest
import torch

from test_f0_extract_cpu import (F0_MAX, F0_MIN, FRAMES, HOP, INNER, SILENCE, SR, THR, cents, lag_range, make_signals, tone, truth_at_centres, yin_decide,
                                 yin_frames)
from test_timing_gpu import load_tiny_pitch

pytestmark = pytest.mark.gpu

# The two bars of test 1: |kernel - fp64 restatement| on decided frames.  MEASURED on an MI355X on this test's inputs, times 8 for the summation-order freedom
# between machines (see the docstring of test_kernel_against_the_restatement); the issue's ceilings are 0.05 cent and 1e-4.
CENTS_BAR = 8 * 1.378e-4
PER_BAR = 8 * 1.738e-7
assert CENTS_BAR <= 0.05 and PER_BAR <= 1e-4


def cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


@pytest.fixture(scope="module")
def signals():
    return make_signals()


def decided_ref(x, length=None, frames=None, thr=THR, **setting):
    """yin_ref at thr (1 - 1e-3), thr and thr (1 + 1e-3): (f0, periodicity, lag at thr, decided [T])"""
    pick = {k: v for k, v in setting.items() if k != "hop"}
    dp, e, n_b = yin_frames(x, length=length, frames=frames, **setting)
    f0, per, lag = yin_decide(dp, e, n_b, threshold=thr, **pick)
    decided = np.ones(len(f0), bool)
    for scale in (1 - 1e-3, 1 + 1e-3):
        decided &= yin_decide(dp, e, n_b, threshold=thr * scale, **pick)[2] == lag
    return f0, per, lag, decided


def compare(got_f0, got_per, ref, what):
    """voicing identical, f0 within CENTS_BAR, periodicity within PER_BAR on decided frames; returns the two measured maxima"""
    f0, per, lag, decided = ref
    assert decided.mean() >= 0.95, (what, decided.mean())
    g, gp = got_f0[decided].astype(np.float64), got_per[decided].astype(np.float64)
    r, rp = f0[decided], per[decided]
    assert np.array_equal(g > 0, r > 0), what
    v = r > 0
    dc = float(cents(g[v], r[v]).max()) if v.any() else 0.0
    dper = float(np.abs(gp - rp).max())
    print(f"{what}: {int(decided.sum())}/{len(decided)} frames decided, max |kernel - fp64| = {dc:.3e} cents, {dper:.3e} periodicity")
    return dc, dper


def test_kernel_against_the_restatement(signals):
    """B = 3 ragged rows (vibrato 146.8 Hz, the gated signal, 830.6 Hz), device lengths, 1e3 beyond each length, T = the longest row's frames.
    Measured on an MI355X: at most 1.378e-4 cents and 1.738e-7 periodicity from the fp64 restatement, every frame decided; the bars are 8 times that,
    1.10e-3 cents and 1.39e-6 (ceilings: 0.05 cent, 1e-4).  The kernel's sums run 32 terms to a chain and the chains are added in order: about where numpy's
    pairwise fp32 evaluation of the rule lands (1.7e-4 cents), three orders below the rule's own error of 0.1 - 0.8 cents."""
    from visinger_amd import pitch_track
    rows = [signals["vibrato"][146.8][0], signals["gated"], signals["steady"][830.6][0]]
    n = max(len(r) for r in rows) + 1000
    wav = np.full((3, n), 1e3, np.float32)
    for b, r in enumerate(rows):
        wav[b, :len(r)] = r
    lens = [len(r) for r in rows]
    T = max(lens) // HOP
    f0, per = pitch_track.extract_f0(cu(wav), HOP, SR, lengths=torch.tensor(lens, device="cuda"), frames=T, return_periodicity=True)
    assert f0.shape == per.shape == (3, T) and f0.dtype == per.dtype == torch.float32
    f0, per = f0.cpu().numpy(), per.cpu().numpy()
    worst = [0.0, 0.0]
    for b, r in enumerate(rows):
        ref = decided_ref(r.astype(np.float32), frames=T)
        dc, dper = compare(f0[b], per[b], ref, f"row {b}")
        worst = [max(worst[0], dc), max(worst[1], dper)]
        n_b = lens[b] // HOP
        assert (f0[b, n_b:] == 0).all() and (per[b, n_b:] == 0).all()
    print(f"kernel vs fp64 restatement: {worst[0]:.3e} cents (bar {CENTS_BAR:.1e}), {worst[1]:.3e} periodicity (bar {PER_BAR:.1e})")
    assert worst[0] <= CENTS_BAR and worst[1] <= PER_BAR


@pytest.mark.parametrize("kind,bound", [("steady", 1.5), ("vibrato", 5.0)])
def test_ground_truth_on_the_device(signals, kind, bound):
    from visinger_amd import pitch_track
    tones = (82.4, 220.0, 830.6)
    wav = np.stack([signals[kind][f][0] for f in tones])
    f0 = pitch_track.extract_f0(cu(wav), HOP, SR).cpu().numpy().astype(np.float64)
    assert f0.shape == (3, FRAMES)
    for b, f in enumerate(tones):
        assert (f0[b, INNER] > 0).all(), (kind, f)
        err = cents(f0[b, INNER], truth_at_centres(signals[kind][f][1], FRAMES)[INNER]).max()
        print(f"{kind} {f} Hz: {err:.3f} cents from the truth")
        assert err <= bound, (kind, f, err)


def test_a_frame_does_not_depend_on_the_launch(signals):
    from visinger_amd import pitch_track
    x = signals["vibrato"][146.8][0].astype(np.float32)
    alone_f0, alone_per = pitch_track.extract_f0(cu(x), HOP, SR, return_periodicity=True)
    assert alone_f0.shape == (1, FRAMES)
    n = len(signals["gated"]) + 333
    wav = np.full((3, n), 1e3, np.float32)
    wav[0, :len(signals["gated"])] = signals["gated"]
    wav[1, :] = np.random.default_rng(5).normal(0, 0.1, n)
    wav[2, :len(x)] = x
    lens = torch.tensor([len(signals["gated"]), n, len(x)], device="cuda")
    f0, per = pitch_track.extract_f0(cu(wav), HOP, SR, lengths=lens, frames=131, return_periodicity=True)
    assert f0.shape == (3, 131)
    assert torch.equal(f0[2, :FRAMES], alone_f0[0]) and torch.equal(per[2, :FRAMES], alone_per[0])
    assert (f0[2, FRAMES:] == 0).all() and (per[2, FRAMES:] == 0).all() and (alone_f0 > 0).sum() >= FRAMES - 8


def test_edges_of_the_rule(signals):
    from visinger_amd import pitch_track
    x = signals["steady"][220.0][0].astype(np.float32)
    # a recording of exactly one hop: one frame, its span mostly outside the signal
    f0, per = pitch_track.extract_f0(cu(x[:HOP]), HOP, SR, return_periodicity=True)
    assert f0.shape == (1, 1)
    compare(f0[0].cpu().numpy(), per[0].cpu().numpy(), decided_ref(x[:HOP]), "one hop")
    # a row of length 0 beside a full one
    f0, per = pitch_track.extract_f0(cu(np.stack([x, x])), HOP, SR, lengths=[0, len(x)], return_periodicity=True)
    assert (f0[0] == 0).all() and (per[0] == 0).all() and (f0[1, INNER] > 0).all()
    # the smallest and the largest window
    for W in (370, 2048):
        f0, per = pitch_track.extract_f0(cu(x), HOP, SR, window=W, return_periodicity=True)
        compare(f0[0].cpu().numpy(), per[0].cpu().numpy(), decided_ref(x, window=W), f"window {W}")


def test_a_second_setting(signals):
    """sr = 16000, hop = 200, 80 - 400 Hz (tau 40 .. 200, W = 400), ragged, with an odd frame count per workgroup's span"""
    from visinger_amd import pitch_track
    setting = dict(sr=16000, hop=200, f0_min=80.0, f0_max=400.0)
    assert lag_range(16000, 80.0, 400.0) == (40, 200)
    rng = np.random.default_rng(77)
    n = 41 * 200 + 13
    rows = [tone(123.5, n, rng, vibrato=True, sr=16000)[0].astype(np.float32), tone(311.1, n - 777, rng, sr=16000)[0].astype(np.float32)]
    wav = np.full((2, n), 1e3, np.float32)
    for b, r in enumerate(rows):
        wav[b, :len(r)] = r
    f0, per = pitch_track.extract_f0(cu(wav), 200, 16000, f0_min=80.0, f0_max=400.0, lengths=[len(r) for r in rows], return_periodicity=True)
    assert f0.shape == (2, 41)
    for b, r in enumerate(rows):
        compare(f0[b].cpu().numpy(), per[b].cpu().numpy(), decided_ref(r, frames=41, **setting), f"16 kHz row {b}")


def test_odd_hop_takes_the_shifted_image(signals):
    """hop = 255: every other frame's window starts on an odd sample, where the kernel reads its second, shifted LDS image"""
    from visinger_amd import pitch_track
    x = signals["vibrato"][220.0][0].astype(np.float32)
    f0, per = pitch_track.extract_f0(cu(x), 255, SR, return_periodicity=True)
    compare(f0[0].cpu().numpy(), per[0].cpu().numpy(), decided_ref(x, hop=255), "hop 255")


def test_a_nan_sample(signals):
    from visinger_amd import pitch_track
    x = signals["steady"][220.0][0].astype(np.float32).copy()
    at = 20 * HOP + 31
    x[at] = np.nan
    f0, per = pitch_track.extract_f0(cu(x), HOP, SR, return_periodicity=True)
    f0, per = f0[0].cpu().numpy(), per[0].cpu().numpy()
    W = 740
    centre = np.arange(FRAMES) * HOP + HOP // 2
    holds = (centre - W // 2 <= at) & (at < centre - W // 2 + W)
    assert holds.sum() == 3 and (f0[holds] == 0).all() and (per[holds] == 0).all()
    assert np.isfinite(f0).all() and np.isfinite(per).all()
    ref = decided_ref(x)
    assert (ref[0][holds] == 0).all()
    compare(f0[~holds], per[~holds], tuple(r[~holds] for r in ref), "beside a NaN")


def test_every_einval_through_the_c_abi():
    from visinger_amd import _lib
    L = _lib.require_gpu()
    B, n, T = 2, 4096, 16
    wav = torch.zeros((B, n), device="cuda")
    lens = torch.full((B,), n, dtype=torch.int64, device="cuda")
    f0, per = torch.full((B, T), -7.0, device="cuda"), torch.full((B, T), -7.0, device="cuda")
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    good = dict(wav=wav, lengths=lens, B=B, L=n, sr=SR, hop=HOP, f0_min=F0_MIN, f0_max=F0_MAX, window=0, threshold=THR, silence=SILENCE, f0=f0, per=per, T=T)

    def call(**kw):
        a = dict(good, **kw)
        return L.vs_f0_yin(vp(a["wav"]), vp(a["lengths"]), a["B"], a["L"], a["sr"], a["hop"], a["f0_min"], a["f0_max"], a["window"], a["threshold"],
                           a["silence"], vp(a["f0"]), vp(a["per"]), a["T"], _lib.stream_ptr())

    nan, inf = float("nan"), float("inf")
    bad = [dict(wav=None), dict(f0=None), dict(f0=wav), dict(per=wav), dict(per=f0), dict(lengths=f0), dict(B=0), dict(L=0), dict(T=0), dict(B=-1),
           dict(L=1 << 31), dict(hop=0), dict(sr=0), dict(f0_min=0.0), dict(f0_min=-65.0), dict(f0_min=nan), dict(f0_max=inf), dict(f0_max=nan),
           dict(threshold=0.0), dict(threshold=nan), dict(threshold=inf), dict(f0_min=1000.0, f0_max=1000.0), dict(f0_min=1000.0, f0_max=65.0),
           dict(f0_min=23.0), dict(sr=2000, f0_min=1000.0, f0_max=1100.0), dict(window=369), dict(window=2049), dict(window=-1), dict(silence=-1e-9), dict(silence=nan)]
    for kw in bad:
        assert call(**kw) == 1, kw                                             # VS_EINVAL
        assert L.vs_last_error()
    torch.cuda.synchronize()
    assert (f0 == -7).all() and (per == -7).all()                              # nothing was launched
    assert call() == 0 and call(per=None) == 0 and call(lengths=None) == 0 and call(window=370) == 0 and call(window=2048) == 0
    torch.cuda.synchronize()
    assert (f0 == 0).all() and (per == 0).all()                                # (all zeros: unvoiced, periodicity exactly 0)


def test_graph_replays_on_another_recording(signals):
    from visinger_amd import pitch_track
    a, b = signals["vibrato"][146.8][0], signals["steady"][523.3][0]
    n = len(a) + 500
    wav, lens = torch.zeros((2, n), device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")

    def load(rows, lengths):
        host = np.full((2, n), 1e3, np.float32)
        for i, r in enumerate(rows):
            host[i, :len(r)] = r
        wav.copy_(cu(host))
        lens.copy_(torch.tensor(lengths, device="cuda"))

    run = lambda: pitch_track.extract_f0(wav, HOP, SR, lengths=lens, frames=FRAMES + 2, return_periodicity=True)
    load([a, b], [len(a), len(b)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f0, per = run()
    first = f0.clone()
    load([b, signals["gated"][:n]], [len(b) - 3 * HOP, n - 100])
    graph.replay()
    eager_f0, eager_per = run()
    assert torch.equal(f0, eager_f0) and torch.equal(per, eager_per) and not torch.equal(f0, first)
    assert (f0[0, FRAMES - 3:] == 0).all() and (f0[0, INNER.start:FRAMES - 8] > 0).all()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver():
    """visinger_tiny_pitch and item 0's tokens on a LONG alignment, 40 frames a token: the model's hop is 8 samples, so the item's 240 frames are 1920
    samples -- room for frames whose whole span (W + tau_max = 1110 samples at 24 kHz, 65 Hz) lies inside a recording of that length"""
    m, a, hp = load_tiny_pitch()
    nph = int((a["text"][0] > 0).sum())
    item = dict(text_tokens=a["text"][0][:nph], pitch_tokens=a["pitch"][0][:nph], dur_tokens=a["dur"][0][:nph], mel2ph=np.repeat(np.arange(1, nph + 1), 40))
    return m, item, int(np.prod(hp["upsample_rates"])), 40 * nph


TRACK = dict(sample_rate=24000, f0_min=65, f0_max=1000)


def recording(frames, hop, seed=3):
    return tone(220.0, frames * hop, np.random.default_rng(seed))[0].astype(np.float32)


def test_driver_prepass_equals_a_given_curve(driver):
    from visinger_amd import synth
    m, item, hop, n = driver
    sung = dict(item, guide_wav=recording(n + 3, hop))
    before = {k: np.array(v, copy=True) for k, v in sung.items()}
    wav, f0 = synth.synthesize(m, [sung], hop, guide_track=TRACK, seeds=7, return_f0=True)[0]
    assert sung.keys() == before.keys() and all(np.array_equal(sung[k], before[k]) for k in sung)
    given = synth.guide_items([sung], hop, "cuda", **TRACK)
    assert "guide_wav" not in given[0] and given[0]["f0"].shape == (n,) and given[0]["f0"].dtype == np.float32
    wav2, f02 = synth.synthesize(m, given, hop, seeds=7, return_f0=True)[0]
    assert np.array_equal(wav, wav2) and np.array_equal(f0, f02) and len(wav) == n * hop
    # the sung curve: 220 Hz within 2 cents on the voiced inner frames
    lo, hi = -(-(370 + 186) // hop), (len(sung["guide_wav"]) - 370 - 186) // hop - 1      # frames whose span lies inside the recording
    inner = f0[lo:hi]
    assert hi - lo >= 64 and (given[0]["f0"][lo:hi] > 0).all() and (inner > 0).all()
    err = cents(inner.astype(np.float64), 220.0).max()
    print(f"sung curve on a 220 Hz recording: {err:.3f} cents")
    assert err <= 2.0


def test_driver_fits_the_curve_to_the_alignment(driver):
    from visinger_amd import pitch_track, synth
    m, item, hop, n = driver
    short, long_ = recording(n - 5, hop), recording(n + 9, hop, seed=4)
    got = synth.guide_items([dict(item, guide_wav=short), dict(item, guide_wav=long_), dict(item)], hop, "cuda", **TRACK)
    for rec, it in zip((short, long_), got):
        curve = pitch_track.extract_f0(cu(rec), hop, 24000, f0_min=65, f0_max=1000)[0].cpu().numpy()
        k = min(len(curve), n)
        assert it["f0"].shape == (n,) and np.array_equal(it["f0"][:k], curve[:k]) and (it["f0"][k:] == 0).all()
    assert (got[0]["f0"][n - 5:] == 0).all() and (got[0]["f0"][:n - 5] > 0).any() and (got[1]["f0"] > 0).any() and "f0" not in got[2]
    out = synth.synthesize(m, [dict(item, guide_wav=short), dict(item, guide_wav=long_)], hop, guide_track=TRACK, seeds=7, equal_tokens=True)
    assert [len(w) for w in out] == [n * hop, n * hop]


def test_driver_tempo_warps_the_tracked_curve(driver):
    from visinger_amd import synth
    m, item, hop, n = driver
    sung = dict(item, guide_wav=recording(n, hop))
    wav, f0 = synth.synthesize(m, [sung], hop, guide_track=TRACK, seeds=7, return_f0=True, tempo=2)[0]
    given = synth.retime_items(synth.guide_items([sung], hop, "cuda", **TRACK), 2, "cuda")
    n2 = len(given[0]["mel2ph"])
    assert n2 < n and len(f0) == n2 and len(wav) == n2 * hop
    wav2, f02 = synth.synthesize(m, given, hop, seeds=7, return_f0=True)[0]
    assert np.array_equal(wav, wav2) and np.array_equal(f0, f02)


def test_driver_errors_and_no_regression(driver):
    from visinger_amd import synth
    m, item, hop, n = driver
    rec = recording(n, hop)
    for items, kw in (([dict(item, guide_wav=rec)], dict()), ([dict(item, guide_wav=rec)], dict(guide_track=dict(f0_min=65))),
                      ([dict(item, guide_wav=rec, f0=np.zeros(n, np.float32))], dict(guide_track=TRACK)),
                      ([dict(item, guide_wav=rec[None])], dict(guide_track=TRACK)), ([dict(item, guide_wav=rec[:hop - 1])], dict(guide_track=TRACK))):
        with pytest.raises(ValueError):
            synth.synthesize(m, items, hop, seeds=7, **kw)
    plain = synth.synthesize(m, [item], hop, seeds=7)
    again = synth.synthesize(m, [item], hop, seeds=7, guide_track=TRACK)      # no recording: the argument is not looked at
    assert np.array_equal(plain[0], again[0]) and np.array_equal(plain[0], synth.synthesize(m, [item], hop, seeds=7)[0])
