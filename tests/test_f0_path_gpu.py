"""Pitch tracking as a path on the GPU (include/visinger_hip.h "f12"; csrc/pitch_track.hip: vs_f0_candidates, csrc/pitch_path.hip: vs_f0_path,
visinger_amd/pitch_track.py): the candidates against the fp64 restatement on the frames the restatement decides unambiguously, plain YIN's choice among them bit
for bit, the path bit for bit against the integer restatement, against ground truth, independent of the launch, every EINVAL, under a graph replay, and as the
driver's "guide_wav" pre-pass."""
import ctypes

import numpy as np
import pytest
import torch

from f0_path_reference import DEFAULTS, UNVOICED, candidate_lags, candidates_ref, flicker, funddip, path_ref
from test_f0_extract_cpu import F0_MAX, F0_MIN, FRAMES, HOP, INNER, SILENCE, SR, cents, lag_range, make_signals, truth_at_centres, yin_frames
from test_f0_extract_gpu import CENTS_BAR, PER_BAR
from test_guide_align_cpu import hz_of_q
from test_timing_gpu import load_tiny_pitch

pytestmark = pytest.mark.gpu

GATE = DEFAULTS["gate"]
OTHER_WEIGHTS = dict(w_unvoiced=300, w_switch=7, w_order=0, w_jump=4096, jump_cap=50)


def cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def padded(rows, extra=1000, fill=1e3):
    """(wav [B, longest + extra] with `fill` beyond each row, lengths)"""
    n = max(len(r) for r in rows) + extra
    wav = np.full((len(rows), n), fill, np.float32)
    for b, r in enumerate(rows):
        wav[b, :len(r)] = r
    return wav, [len(r) for r in rows]


@pytest.fixture(scope="module")
def signals():
    return make_signals()


@pytest.fixture(scope="module")
def rows(signals):
    """the three ragged rows of tests 1 - 3: a dip at 220 Hz, the gated signal, a flicker at 523.3 Hz (sigma 0.04), rounded to fp32"""
    return [np.asarray(x, np.float32) for x in (funddip(220.0, np.random.default_rng(1)), signals["gated"], flicker(523.3, np.random.default_rng(1), 0.04))]


@pytest.fixture(scope="module")
def device_candidates(rows):
    """(cand_hz, cand_d) [3, T, 8] on the device, lengths, T: one launch over the ragged batch, device lengths, 1e3 beyond each length"""
    from visinger_amd import pitch_track
    wav, lens = padded(rows)
    T = max(lens) // HOP
    hz, d = pitch_track.candidates(cu(wav), HOP, SR, lengths=torch.tensor(lens, device="cuda"), frames=T)
    assert hz.shape == d.shape == (3, T, 8) and hz.dtype == d.dtype == torch.float32
    return hz, d, lens, T


def decided_frames(dp, e, n_b):
    """frames the fp64 restatement decides with room to spare: the candidate lags are the same at gate (1 -+ 1e-3), every comparison of neighbours that can make
    or break a candidate (one of the two below the gate) has a relative margin over 1e-5, and the energy is not within 1e-3 of the silence bound"""
    tau_min, tau_max = lag_range(SR, F0_MIN, F0_MAX)
    W = 2 * tau_max
    out = np.zeros(len(dp), bool)
    for t in range(n_b):
        row = dp[t]
        lags = [candidate_lags(row, tau_min, tau_max, GATE * s) for s in (1 - 1e-3, 1.0, 1 + 1e-3)]
        a, b = row[tau_min - 1:tau_max + 1], row[tau_min:tau_max + 2]
        near = np.minimum(a, b) < GATE * (1 + 1e-3)
        ok = lags[0] == lags[1] == lags[2] and bool((np.abs(a - b)[near] > 1e-5 * np.maximum(a, b)[near]).all())
        if abs(e[t] - SILENCE * W) <= 1e-3 * SILENCE * W and lags[2]:
            ok = False
        out[t] = ok
    out[n_b:] = True                                                           # (beyond the row: empty, whatever the samples are)
    return out


def test_candidates_against_the_restatement(rows, device_candidates):
    """on decided frames the candidates sit in the same slots (a lag apart is 4.7 cents or more: within CENTS_BAR means the same lag), cand_hz within CENTS_BAR and
    cand_d within PER_BAR of the fp64 restatement -- the same d' feeds the same formula as in vs_f0_yin; empty slots hold (0, 1) exactly.
    Measured on an MI355X: 192 of 192 frames decided, 717 candidates, at most 1.771e-4 cents and 8.07e-8 from the restatement (bars 1.10e-3 and 1.39e-6)."""
    hz, d, lens, T = device_candidates
    hz, d = hz.cpu().numpy(), d.cpu().numpy()
    worst, decided_n, frames_n = [0.0, 0.0], 0, 0
    for b, x in enumerate(rows):
        dp, e, n_b = yin_frames(x, frames=T)
        rhz, rd, rlags = candidates_ref(dp, e, n_b)
        ok = decided_frames(dp, e, n_b)
        decided_n, frames_n = decided_n + int(ok[:n_b].sum()), frames_n + n_b
        assert n_b == lens[b] // HOP and (hz[b, n_b:] == 0).all() and (d[b, n_b:] == 1).all()
        assert (hz[b, :, 7] == 0).all() and (d[b, :, 7] == 1).all()
        g, gd, r, rdd = hz[b][ok].astype(np.float64), d[b][ok].astype(np.float64), rhz[ok], rd[ok]
        assert np.array_equal(g > 0, r > 0), f"row {b}: the candidates of a decided frame sit in other slots"
        assert ((gd == 1) | (g > 0)).all() and ((hz[b] > 0) | ((hz[b] == 0) & (d[b] == 1))).all()
        m = r > 0
        lag_dev = SR / g[m]
        assert (np.abs(lag_dev - rlags[ok][m[:, :7]]) <= 0.5 + 1e-3).all()
        dc, dd = float(cents(g[m], r[m]).max()), float(np.abs(gd - rdd).max())
        print(f"row {b}: {int(ok[:n_b].sum())}/{n_b} frames decided, {int(m.sum())} candidates, max |kernel - fp64| = {dc:.3e} cents, {dd:.3e} d'")
        worst = [max(worst[0], dc), max(worst[1], dd)]
    print(f"candidates vs fp64 restatement: {worst[0]:.3e} cents (bar {CENTS_BAR:.1e}), {worst[1]:.3e} d' (bar {PER_BAR:.1e}), {decided_n}/{frames_n} decided")
    assert decided_n >= 0.95 * frames_n
    assert worst[0] <= CENTS_BAR and worst[1] <= PER_BAR


def test_plain_yin_s_choice_is_one_of_the_candidates_bit_for_bit(rows, signals):
    from visinger_amd import pitch_track
    wav, lens = padded(rows + [np.asarray(signals["steady"][f][0], np.float32) for f in (82.4, 830.6)])
    lens_d = torch.tensor(lens, device="cuda")
    f0 = pitch_track.extract_f0(cu(wav), HOP, SR, lengths=lens_d)
    hz, _ = pitch_track.candidates(cu(wav), HOP, SR, lengths=lens_d)
    assert hz.shape[:2] == f0.shape
    voiced = f0 > 0
    among = (hz.view(torch.int32) == f0.view(torch.int32)[..., None]).any(-1)
    print(f"containment on the device: {int((voiced & ~among).sum())} misses of {int(voiced.sum())} voiced frames")
    assert int(voiced.sum()) >= 150 and bool(among[voiced].all())


def check_path(hz, d, n, weights):
    """best_path on [B, T, 8] host arrays (n: per row, any integers) bit for bit against path_ref"""
    from visinger_amd import pitch_track
    B, T = hz.shape[:2]
    nd = None if n is None else torch.tensor(n, dtype=torch.int64, device="cuda")
    f0, state, cost = pitch_track.best_path(cu(hz), cu(d), nd, return_state=True, return_cost=True, **weights)
    assert f0.shape == state.shape == (B, T) and cost.shape == (B,) and state.dtype == cost.dtype == torch.int32
    alone = pitch_track.best_path(cu(hz), cu(d), nd, **weights)
    assert torch.equal(alone.view(torch.int32), f0.view(torch.int32))        # (state = cost = NULL is the same path)
    f0, state, cost = f0.cpu().numpy(), state.cpu().numpy(), cost.cpu().numpy()
    for b in range(B):
        rf, rs, rc = path_ref(hz[b], d[b], None if n is None else n[b], **weights)
        assert np.array_equal(state[b], rs), (b, T, np.flatnonzero(state[b] != rs)[:5])
        assert np.array_equal(f0[b].view(np.int32), rf.view(np.int32)) and int(cost[b]) == rc, (b, T, int(cost[b]), rc)
    return state


def test_path_on_the_device_s_own_candidates(device_candidates):
    hz, d, lens, T = device_candidates
    state = check_path(hz.cpu().numpy(), d.cpu().numpy(), [n // HOP for n in lens], {})
    assert (state[0, :lens[0] // HOP] >= 0).all() and (state[0, lens[0] // HOP:] == -1).all() and (state[1, 2:12] < UNVOICED).all()


def random_candidates(rng, B, T):
    """[B, T, 8] candidates on the quantiser's grid plus a quarter step (fp32 rounding of log2 cannot move q): 0 .. 7 present slots a frame, whole empty frames,
    duplicated slots and frames (ties), NaN / inf / negative entries, d from a few values and from [-0.2, 1.2]"""
    q = rng.integers(560, 1341, (B, T, 8))
    hz = hz_of_q(q).astype(np.float32)
    d = rng.uniform(-0.2, 1.2, (B, T, 8)).astype(np.float32)
    few = rng.random((B, T, 8)) < 0.5
    d[few] = rng.choice(np.array([0.0, 0.05, 0.15625, 0.3, 0.5, 1.0], np.float32), int(few.sum()))
    count = rng.integers(0, 8, (B, T))
    count[rng.random((B, T)) < 0.15] = 0
    hz[np.arange(8)[None, None, :] >= count[..., None]] = 0.0
    dup = rng.random((B, T, 8)) < 0.25                                          # a slot repeats its left neighbour
    dup[..., 0] = False
    for k in range(1, 7):
        take = dup[..., k] & (hz[..., k] > 0)
        hz[..., k], d[..., k] = np.where(take, hz[..., k - 1], hz[..., k]), np.where(take, d[..., k - 1], d[..., k])
    same = rng.random((B, T)) < 0.2                                             # a frame repeats the one before it
    for t in range(1, T):
        hz[:, t] = np.where(same[:, t, None], hz[:, t - 1], hz[:, t])
        d[:, t] = np.where(same[:, t, None], d[:, t - 1], d[:, t])
    odd = rng.random((B, T, 8))
    hz[odd < 0.02] = np.nan
    hz[(odd >= 0.02) & (odd < 0.04)] = np.inf
    hz[(odd >= 0.04) & (odd < 0.06)] *= -1.0
    d[(odd >= 0.06) & (odd < 0.09)] = np.nan
    d[(odd >= 0.09) & (odd < 0.11)] = np.inf
    hz[..., 7], d[..., 7] = 440.0, 0.0                                          # slot 7 is not read
    return hz, d


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 700])
def test_path_on_random_candidates(T):
    rng = np.random.default_rng(1200 + T)
    hz, d = random_candidates(rng, 5, T)
    n = [T, 0, max(T - 1, 0), T + 5, int(rng.integers(0, T + 1))]              # ragged, 0, beyond T (clamped)
    check_path(hz, d, n, {})
    check_path(hz, d, [T, -3, T // 2, T, 1], OTHER_WEIGHTS)
    check_path(hz[:1], d[:1], None, dict(w_order=4096, w_unvoiced=4096, w_switch=4096, w_jump=4096, jump_cap=4096))     # the worst sums stay in int32


def test_path_at_the_lds_ceiling():
    T = 32768
    hz, d = random_candidates(np.random.default_rng(5), 1, T)
    check_path(hz, d, None, {})


def test_ground_truth_on_the_device(signals):
    """Measured on an MI355X: the dip rows within 5.00 / 1.04 / 0.46 cents under the path, 4 frames 1158 - 1210 cents off without it; the flicker rows' worst
    voiced frame 39.8 cents off (98 Hz, sigma 0.045) -- the figures of the fp64 restatement"""
    from visinger_amd import pitch_track
    dip_tones = (98.0, 220.0, 523.3)
    wav = cu(np.stack([funddip(f, np.random.default_rng(1)) for f in dip_tones]))
    plain, path = pitch_track.extract_f0(wav, HOP, SR).cpu().numpy().astype(np.float64), pitch_track.extract_f0(wav, HOP, SR, path={})
    assert path.shape == (3, FRAMES) and path.dtype == torch.float32
    path = path.cpu().numpy().astype(np.float64)
    for b, f in enumerate(dip_tones):
        off = cents(np.where(plain[b, INNER] > 0, plain[b, INNER], f), f)
        assert (off > 600).any(), f                                            # the premise: plain YIN jumps
        assert (path[b, INNER] > 0).all(), f
        err = cents(path[b, INNER], f).max()
        print(f"dip {f} Hz: plain YIN {int((off > 600).sum())} frames up to {off.max():.0f} cents off, the path {err:.2f} cents")
        assert err <= 8.0, (f, err)
    cases = [(98.0, 3, 0.035), (220.0, 1, 0.045), (392.0, 1, 0.045), (523.3, 2, 0.045), (98.0, 2, 0.045)]
    wav = cu(np.stack([flicker(f, np.random.default_rng(seed), sigma) for f, seed, sigma in cases]))
    path = pitch_track.extract_f0(wav, HOP, SR, path={}).cpu().numpy().astype(np.float64)
    for b, (f, seed, sigma) in enumerate(cases):
        v = path[b, INNER] > 0
        err = cents(path[b, INNER][v], f).max() if v.any() else 0.0
        print(f"flicker {f} Hz seed {seed} sigma {sigma}: {int(v.sum())} voiced INNER frames, worst {err:.1f} cents")
        assert err <= 50.0, (f, seed, sigma, err)
    for kind in ("steady", "vibrato"):
        wav = cu(np.stack([signals[kind][f][0] for f in (82.4, 220.0, 830.6)]))
        plain, path = pitch_track.extract_f0(wav, HOP, SR), pitch_track.extract_f0(wav, HOP, SR, path={})
        assert (plain[:, INNER] > 0).all() and torch.equal(plain[:, INNER].view(torch.int32), path[:, INNER].view(torch.int32)), kind
    noise = pitch_track.extract_f0(cu(np.stack([signals["noise"], signals["zeros"]])), HOP, SR, path={}, return_periodicity=True)
    assert (noise[0] == 0).all() and (noise[1] == 0).all()


def test_a_row_does_not_depend_on_the_launch(signals):
    from visinger_amd import pitch_track
    x = np.asarray(funddip(146.8, np.random.default_rng(2)), np.float32)
    alone_f0, alone_per = pitch_track.extract_f0(cu(x), HOP, SR, path={}, return_periodicity=True)
    assert alone_f0.shape == (1, FRAMES) and (alone_f0[0, INNER] > 0).all()
    assert ((alone_per > 0) == (alone_f0 > 0)).all() and float(alone_per.max()) <= 1.0 and float(alone_per[0, INNER].min()) > 0.5
    wav, lens = padded([signals["gated"], np.random.default_rng(5).normal(0, 0.1, len(signals["gated"]) + 333), x], extra=333)
    f0, per = pitch_track.extract_f0(cu(wav), HOP, SR, lengths=torch.tensor(lens, device="cuda"), frames=131, path={}, return_periodicity=True)
    assert f0.shape == per.shape == (3, 131)
    assert torch.equal(f0[2, :FRAMES].view(torch.int32), alone_f0[0].view(torch.int32)) and torch.equal(per[2, :FRAMES], alone_per[0])
    assert (f0[2, FRAMES:] == 0).all() and (per[2, FRAMES:] == 0).all() and (f0[1] == 0).all()
    host = pitch_track.extract_f0(cu(wav), HOP, SR, lengths=lens, frames=131, path={})          # host lengths: the same frames
    assert torch.equal(host.view(torch.int32), f0.view(torch.int32))


def test_every_einval_through_the_c_abi():
    from visinger_amd import _lib
    L = _lib.require_gpu()
    B, n, T = 2, 4096, 16
    wav = torch.zeros((B, n), device="cuda")
    lens = torch.full((B,), n, dtype=torch.int64, device="cuda")
    hz, d = torch.full((B, T, 8), -7.0, device="cuda"), torch.full((B, T, 8), -7.0, device="cuda")
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    good = dict(wav=wav, lengths=lens, B=B, L=n, sr=SR, hop=HOP, f0_min=F0_MIN, f0_max=F0_MAX, window=0, gate=GATE, silence=SILENCE, hz=hz, d=d, T=T)

    def cand(**kw):
        a = dict(good, **kw)
        return L.vs_f0_candidates(vp(a["wav"]), vp(a["lengths"]), a["B"], a["L"], a["sr"], a["hop"], a["f0_min"], a["f0_max"], a["window"], a["gate"],
                                  a["silence"], vp(a["hz"]), vp(a["d"]), a["T"], _lib.stream_ptr())

    nan, inf = float("nan"), float("inf")
    bad = [dict(wav=None), dict(hz=None), dict(d=None), dict(hz=wav), dict(d=wav), dict(d=hz), dict(lengths=hz), dict(lengths=d), dict(B=0), dict(L=0), dict(T=0),
           dict(B=-1), dict(L=1 << 31), dict(T=1 << 31), dict(B=1 << 60), dict(hop=0), dict(sr=0), dict(f0_min=0.0), dict(f0_min=-65.0), dict(f0_min=nan),
           dict(f0_max=inf), dict(f0_max=nan), dict(gate=0.0), dict(gate=-0.5), dict(gate=nan), dict(gate=inf), dict(f0_min=1000.0, f0_max=1000.0),
           dict(f0_min=1000.0, f0_max=65.0), dict(f0_min=23.0), dict(sr=2000, f0_min=1000.0, f0_max=1100.0), dict(window=369), dict(window=2049), dict(window=-1),
           dict(silence=-1e-9), dict(silence=nan)]
    for kw in bad:
        assert cand(**kw) == 1, kw                                             # VS_EINVAL
        assert b"vs_f0_candidates" in L.vs_last_error()
    torch.cuda.synchronize()
    assert (hz == -7).all() and (d == -7).all()                                # nothing was launched
    assert cand() == 0 and cand(lengths=None) == 0 and cand(window=370) == 0 and cand(window=2048) == 0 and cand(gate=2.0) == 0
    torch.cuda.synchronize()
    assert (hz == 0).all() and (d == 1).all()                                  # (all zeros: silent, every slot empty)

    f0, state, cost = torch.full((B, T), -7.0, device="cuda"), torch.full((B, T), -7, dtype=torch.int32, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda")
    nfr = torch.full((B,), T, dtype=torch.int64, device="cuda")
    good_p = dict(hz=hz, d=d, n=nfr, B=B, T=T, w_unvoiced=160, w_switch=96, w_order=24, w_jump=32, jump_cap=384, reserved=0, f0=f0, state=state, cost=cost)

    def path(**kw):
        a = dict(good_p, **kw)
        return L.vs_f0_path(vp(a["hz"]), vp(a["d"]), vp(a["n"]), a["B"], a["T"], a["w_unvoiced"], a["w_switch"], a["w_order"], a["w_jump"], a["jump_cap"],
                            a["reserved"], vp(a["f0"]), vp(a["state"]), vp(a["cost"]), _lib.stream_ptr())

    bad = [dict(hz=None), dict(d=None), dict(f0=None), dict(d=hz), dict(f0=hz), dict(f0=d), dict(state=f0), dict(cost=state), dict(n=cost), dict(state=hz), dict(cost=d),
           dict(n=f0), dict(B=0), dict(B=-2), dict(T=0), dict(T=-1), dict(T=32769), dict(B=1 << 60), dict(reserved=1), dict(reserved=-1)]
    bad += [{k: v} for k in ("w_unvoiced", "w_switch", "w_order", "w_jump", "jump_cap") for v in (-1, 4097)]
    for kw in bad:
        assert path(**kw) == 1, kw
        assert b"vs_f0_path" in L.vs_last_error()
    torch.cuda.synchronize()
    assert (f0 == -7).all() and (state == -7).all() and (cost == -7).all()
    assert path() == 0 and path(n=None) == 0 and path(state=None) == 0 and path(cost=None) == 0 and path(state=None, cost=None) == 0
    assert path(w_unvoiced=0, w_switch=0, w_order=0, w_jump=0, jump_cap=0) == 0 and path(w_unvoiced=4096, w_switch=4096, w_order=4096, w_jump=4096, jump_cap=4096) == 0
    torch.cuda.synchronize()
    assert (f0 == 0).all() and (state == UNVOICED).all() and (cost == T * 4096).all()


def test_graph_replays_on_another_recording(signals):
    from visinger_amd import pitch_track
    a, b = np.asarray(funddip(220.0, np.random.default_rng(3)), np.float32), np.asarray(signals["steady"][523.3][0], np.float32)
    n = len(a) + 500
    wav, lens = torch.zeros((2, n), device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")

    def load(recordings, lengths):
        host = np.full((2, n), 1e3, np.float32)
        for i, r in enumerate(recordings):
            host[i, :len(r)] = r
        wav.copy_(cu(host))
        lens.copy_(torch.tensor(lengths, device="cuda"))

    run = lambda: pitch_track.extract_f0(wav, HOP, SR, lengths=lens, frames=FRAMES + 2, path={}, return_periodicity=True)
    load([a, b], [len(a), len(b)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f0, per = run()
    graph.replay()                                                             # (a capture runs nothing: the first replay fills the buffers)
    first = f0.clone()
    assert (first[0, INNER] > 0).all() and torch.equal(first, run()[0])
    load([b, signals["gated"][:n]], [len(b) - 3 * HOP, n - 100])
    graph.replay()
    eager_f0, eager_per = run()
    assert torch.equal(f0, eager_f0) and torch.equal(per, eager_per) and not torch.equal(f0, first)
    assert (f0[0, FRAMES - 3:] == 0).all() and (f0[0, INNER.start:FRAMES - 8] > 0).all()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------

def test_driver_prepass_equals_a_given_path_tracked_curve():
    """visinger_tiny_pitch on a long alignment (40 frames a token, the model's hop is 8 samples), as in test_f0_extract_gpu"""
    from visinger_amd import pitch_track, synth
    m, a, hp = load_tiny_pitch()
    nph = int((a["text"][0] > 0).sum())
    item = dict(text_tokens=a["text"][0][:nph], pitch_tokens=a["pitch"][0][:nph], dur_tokens=a["dur"][0][:nph], mel2ph=np.repeat(np.arange(1, nph + 1), 40))
    hop, n = int(np.prod(hp["upsample_rates"])), 40 * nph
    track = dict(sample_rate=24000, f0_min=65, f0_max=1000)
    rec = funddip(220.0, np.random.default_rng(1), hop=hop, n=(n + 3) * hop).astype(np.float32)
    sung = dict(item, guide_wav=rec)
    wav, f0 = synth.synthesize(m, [sung], hop, guide_track=dict(track, path={}), seeds=7, return_f0=True)[0]
    curve = pitch_track.extract_f0(cu(rec), hop, path={}, **track)[0].cpu().numpy()
    given = synth.guide_items([sung], hop, "cuda", path={}, **track)
    assert "guide_wav" not in given[0] and np.array_equal(given[0]["f0"], curve[:n]) and len(curve) == n + 3
    wav2, f02 = synth.synthesize(m, [dict(item, f0=curve[:n])], hop, seeds=7, return_f0=True)[0]
    assert np.array_equal(wav, wav2) and np.array_equal(f0, f02) and len(wav) == n * hop
    other = synth.guide_items([sung], hop, "cuda", path=dict(gate=1e-6), **track)                  # the dict reaches the kernels: no candidate passes this gate
    assert (other[0]["f0"] == 0).all() and (given[0]["f0"] > 0).any()
