"""Loudness normalisation on an MI355X (csrc/loudness.hip, include/visinger_hip.h "f14"): vs_loud_steps' step sums against the serial fp64
restatement ``loudness.loudness_ref`` under the derived bound ``loudness.steps_bound``, vs_loud_gate's counts exactly and its loudness and gain against the
restatement, vs_gain_apply bit for bit, the 16-byte / 4-byte and the in-place paths, a graph replay, and ``synthesize(loudness=)`` bit for bit ``normalize()`` of
each plain waveform.  tests/test_loudness_cpu.py holds the restatement to the standard."""
import numpy as np
import pytest
import torch

from visinger_amd import loudness as lo
from loudness_cases import gate_margin, gating_fixture
from test_resample_gpu import driver  # noqa: F401  (the tiny model and three ragged items)

pytestmark = pytest.mark.gpu


def cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def noise_and_tone(n, seed):
    r = np.random.default_rng(seed)
    return (0.3 * r.uniform(-1.0, 1.0, n) + 0.5 * np.sin(2 * np.pi * 0.013 * np.arange(n) + r.uniform(0, 6))).astype(np.float32)


def hold_steps(x, lens, sr, what):
    """vs_loud_steps on the batch x held, element by element, to |S_dev - S_ref| <= steps_bound(sr, rho) max_i S_ref[row], rho = s max|x|^2 / max_i S_ref[row] of
    the row's own counted samples: a figure of the inputs and the restatement, not of the kernel.  Exact zeros where no complete step is.  Returns S_dev."""
    s = sr // 10
    S = lo.step_sums(cu(x), sr, lengths=None if lens is None else torch.tensor(lens, device="cuda")).cpu().numpy()
    ref = lo.loudness_ref(x, lens, sr)[0]
    assert S.dtype == np.float64 and S.shape == ref.shape == (len(x), max(x.shape[1] // s, 1))
    worst = 0.0
    for b in range(len(x)):
        ns = (x.shape[1] if lens is None else lens[b]) // s
        assert not S[b, ns:].any() and not ref[b, ns:].any(), (what, b)
        if ns == 0:
            continue
        top = ref[b, :ns].max()
        rho = s * float(np.abs(x[b, :ns * s]).max()) ** 2 / top
        bound = lo.steps_bound(sr, rho)
        err = np.abs(S[b, :ns] - ref[b, :ns]).max() / top
        worst = max(worst, err / bound)
        assert err <= bound, (what, b, err, bound)
    print(f"{what}: sr {sr}, worst |S_dev - S_ref| / (bound max S) = {worst:.3e}")
    return S


def test_step_sums_of_a_ragged_batch_off_the_16_byte_boundaries():
    """sr 8000, s = 800, c = 4: rows that end before, on and behind a step's and a block's edge; L is odd, so every second row starts 4 bytes off a 16-byte
    boundary and the staged head is 0 .. 3 samples long"""
    lens = [0, 799, 800, 801, 3199, 3200, 3201, 4000, 8013]
    L = 8013
    x = np.stack([np.where(np.arange(L) < n, noise_and_tone(L, 20 + b), 1e3).astype(np.float32) for b, n in enumerate(lens)])
    S = hold_steps(x, lens, 8000, "ragged")
    assert [int((S[b] > 0).sum()) for b in range(len(lens))] == [0, 0, 1, 1, 3, 4, 4, 5, 10]
    # a row's sums depend on its own samples only: alone, without lengths, on an aligned base
    alone = lo.step_sums(cu(x[8:9]), 8000).cpu().numpy()
    assert np.array_equal(alone, S[8:9])
    one = lo.step_sums(cu(x[6:7, :3201]), 8000).cpu().numpy()
    assert np.array_equal(one[0], S[6, :4])


@pytest.mark.parametrize("sr", [8010, 44100, 48000])
def test_step_sums_at_other_rates(sr):
    """s = 801: the lanes split unevenly (200 lanes of 4 samples and one of 1); 44.1 and 48 kHz: 18 and 19 samples a lane, the high-pass's poles at 0.995"""
    s = sr // 10
    x = np.stack([noise_and_tone(5 * s + 3, sr), noise_and_tone(5 * s + 3, sr + 1)])
    hold_steps(x, [5 * s + 3, 5 * s], sr, "five steps")


@pytest.mark.parametrize("sr", [8000, 48000])
def test_step_sums_of_a_burst_before_silence_and_of_dc(sr):
    s = sr // 10
    burst = np.zeros(6 * s, np.float32)
    burst[:2 * s] = noise_and_tone(2 * s, 5)                                     # ends exactly at a step's end: the silent steps hold the carried ringing only
    dc = np.full(6 * s, 0.5, np.float32)                                         # the high-pass removes it: the first step holds the transient
    S = hold_steps(np.stack([burst, dc]), None, sr, "burst, dc")
    assert (S[0, 2:] > 0).all() and (np.diff(S[0, 2:]) < 0).all() and S[0, 2] < 0.1 * S[0, 1]
    assert S[1, 0] > 0 and S[1, 1] < 1e-6 * S[1, 0]


@pytest.fixture(scope="module")
def gate_rows():
    """the gating fixture, an all-zero row, the fixture cut at 3199 samples (no block), the fixture with one NaN, a tone at -60 dBFS; and their restatement"""
    x, sr = gating_fixture()
    rows = np.stack([x, np.zeros_like(x), x, x, x])
    rows[3, 40000] = np.nan
    rows[4] = (1e-3 * np.sin(2 * np.pi * 440.0 * np.arange(len(x)) / sr)).astype(np.float32)
    lens = [len(x), len(x), 3199, len(x), len(x)]
    return rows, lens, sr, lo.loudness_ref(rows, lens, sr, -23.0, 20.0)


def test_gates_loudness_and_gain_against_the_restatement(gate_rows):
    rows, lens, sr, (S_ref, loud_ref, stats_ref, gain_ref) = gate_rows
    for b, n in enumerate(lens):                                                 # a condition on the inputs: no block within 1e-6 of a gate
        assert gate_margin(S_ref[b], n // 800, 800) > 1e-6, b
    y, loud, stats, gain = lo.normalize(cu(rows), sr, lengths=lens, return_loudness=True, return_stats=True, return_gain=True)
    loud, stats, gain = loud.cpu().numpy(), stats.cpu().numpy(), gain.cpu().numpy()
    print(f"gate: stats {stats.tolist()}, loud {loud.tolist()}, gain {gain.tolist()}")
    assert stats.dtype == np.int32 and np.array_equal(stats, stats_ref) and stats[0].tolist() == [77, 60, 30]
    assert stats[1].tolist() == [77, 0, 0] and stats[2].tolist() == [0, 0, 0] and stats[3, 0] == 77
    finite = np.isfinite(loud_ref)
    assert finite.tolist() == [True, False, False, False, True]
    assert loud.dtype == np.float64 and np.abs(loud[finite] - loud_ref[finite]).max() <= 1e-6
    assert loud[1] == loud[2] == -np.inf and np.isnan(loud[3])
    assert gain.dtype == np.float32 and (gain[~finite] == 1.0).all()
    assert np.abs(gain.view(np.int32).astype(np.int64) - gain_ref.view(np.int32)).max() <= 1     # one fp32 ulp
    assert gain[4] == np.float32(10.0) and loud[4] < -60.0                      # max_gain_db clamps the -60 dBFS row
    m_loud, m_stats = lo.measure(cu(rows), sr, lengths=lens)                     # measure() is the same two launches
    assert np.array_equal(m_loud.cpu().numpy(), loud, equal_nan=True) and np.array_equal(m_stats.cpu().numpy(), stats)


def test_apply_is_bit_exact_and_leaves_the_rest_alone(gate_rows):
    rows, lens, sr, _ = gate_rows
    L = rows.shape[1]
    x = rows.copy()
    x[2, 3199:] = 1e3                                                            # beyond a length: comes back as it is
    lens = [L, L, 3199, L, L - 5]
    x[4, L - 5:] = -7.0
    y, gain = lo.normalize(cu(x), sr, lengths=lens, return_gain=True, target_lufs=-16.0, max_gain_db=60.0)
    y, g = y.cpu().numpy(), gain.cpu().numpy()
    assert g[0] != 1.0 and g[4] != 1.0 and g[1] == g[2] == g[3] == 1.0

    def scaled(x, lens, g):
        """x * gain, one fp32 product, inside each length; x's bits beyond it and on gain-1 rows (the NaN's too)"""
        inside = np.arange(x.shape[1])[None] < np.asarray(lens)[:, None]
        want = np.where(inside, x * g[:, None], x).astype(np.float32)
        want[g == 1.0] = x[g == 1.0]
        return want

    assert np.array_equal(bits(y), bits(scaled(x, lens, g)))
    # in place; into a given tensor
    xs = cu(x)
    back = lo.normalize(xs, sr, lengths=lens, out=xs, target_lufs=-16.0, max_gain_db=60.0)
    assert back.data_ptr() == xs.data_ptr() and np.array_equal(bits(xs), bits(y))
    out = torch.full(x.shape, -3.0, device="cuda")
    assert lo.normalize(cu(x), sr, lengths=lens, out=out, target_lufs=-16.0, max_gain_db=60.0) is out and np.array_equal(bits(out), bits(y))
    # the 4-byte path: a base 4 bytes off, and an odd L
    buf = torch.zeros(5 * L + 1, device="cuda")
    off = buf[1:].view(5, L)
    off.copy_(cu(x))
    assert off.data_ptr() % 16 == 4
    assert np.array_equal(bits(lo.normalize(off, sr, lengths=lens, target_lufs=-16.0, max_gain_db=60.0)), bits(y))
    lo.normalize(off, sr, lengths=lens, out=off, target_lufs=-16.0, max_gain_db=60.0)
    assert np.array_equal(bits(off), bits(y))
    odd, odd_lens = x[:, :L - 1].copy(), [min(n, L - 1) for n in lens]            # (one step less on the full rows: other gains)
    yo, go = lo.normalize(cu(odd), sr, lengths=odd_lens, return_gain=True, target_lufs=-16.0, max_gain_db=60.0)
    go = go.cpu().numpy()
    assert go[0] != 1.0 and np.array_equal(bits(yo), bits(scaled(odd, odd_lens, go)))
    # the normalised rows measure the target: fp32 rounding of the samples moves the power by under 2^-23
    loud, _ = lo.measure(cu(y), sr, lengths=lens)
    loud = loud.cpu().numpy()
    print(f"measure(normalize(x)) - target: {(loud[[0, 4]] + 16.0).tolist()}")
    assert np.abs(loud[[0, 4]] + 16.0).max() <= 1e-4


def test_graph_replays_on_other_data():
    sr, L = 8000, 8013
    wav, lens = torch.zeros((3, L), device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")

    def load(seed):
        x = np.stack([noise_and_tone(L, seed + b) * (0.1 + 0.4 * b) for b in range(3)])
        n = [L - 7 * seed, 4000 + seed, 3199]
        wav.copy_(cu(x)), lens.copy_(torch.tensor(n, device="cuda"))
        return x, n

    run = lambda: lo.normalize(wav, sr, lengths=lens, return_loudness=True, return_stats=True, return_gain=True)
    load(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    first = out[3].clone()
    x, n = load(2)
    graph.replay()
    assert not torch.equal(out[3], first)
    eager = lo.normalize(cu(x), sr, lengths=n, return_loudness=True, return_stats=True, return_gain=True)
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    S_ref, loud_ref, stats_ref, gain_ref = lo.loudness_ref(x, n, sr)
    assert np.array_equal(out[2].cpu().numpy(), stats_ref) and np.abs(out[1].cpu().numpy()[:2] - loud_ref[:2]).max() <= 1e-6


def test_refused_calls_launch_nothing():
    """the refusals themselves are tests/test_loudness_cpu.py's; here: a refused call leaves its outputs alone"""
    import ctypes
    from visinger_amd import _args, _lib
    lib = _lib.require_gpu()
    x, y = torch.full((2, 4000), 0.5, device="cuda"), torch.full((2, 4000), -7.0, device="cuda")
    S = torch.full((2, 5), -7.0, dtype=torch.float64, device="cuda")
    gain = torch.full((2,), 2.0, device="cuda")
    p, st = _args.vp, _lib.stream_ptr()
    coef = (ctypes.c_double * 10)(*lo.coef_array(8000))
    assert lib.vs_loud_steps(p(x), None, 2, 4000, coef, p(lo.carry_table(8000, "cuda")), 799, p(S), 5, st) == 1
    assert lib.vs_gain_apply(p(x), p(gain), None, p(y.view(-1)[1:]), 2, 1999, st) == 0       # (a valid call on other sizes: y[1 : 3999] = 1.0)
    assert lib.vs_gain_apply(p(x), p(gain), None, p(x.view(-1)[1:]), 2, 1999, st) == 1       # y overlaps x partly
    torch.cuda.synchronize()
    assert (S == -7).all() and (x == 0.5).all() and (y.view(-1)[1:3999] == 1.0).all() and y.view(-1)[0] == -7 and (y.view(-1)[3999:] == -7).all()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------------------

RATE = 8000                       # the tiny model's waveforms read as 8 kHz audio: a 400 ms block is 3200 samples, 400 of its frames


def normalized_alone(w, rate=RATE, **kw):
    return lo.normalize(cu(np.atleast_2d(w)), rate, **kw).cpu().numpy()


@pytest.fixture(scope="module")
def long_items(driver):
    """the driver's tokens spread over 640, 600 and 440 frames (hop 8: 5120, 4800 and 3520 samples -- 3, 3 and 1 block at 8 kHz)"""
    m, items, hop, nph = driver
    return [dict(it, mel2ph=np.repeat(np.arange(1, nph + 1), -(-frames // nph))) for it, frames in zip(items, (640, 600, 440))]


@pytest.mark.parametrize("case", ["ragged", "takes", "streams", "graphs"])
def test_driver_normalises_the_output(driver, long_items, case):
    """synthesize(loudness=) equals, bit for bit, normalize() of each waveform -- of each take -- the call returns without loudness"""
    from visinger_amd import synth
    m, _, hop, nph = driver
    items = long_items
    kw = dict(ragged=dict(), takes=dict(takes=2), streams=dict(streams=2, max_frames_per_batch=700), graphs=dict(graphs={}))[case]
    opt = dict(sample_rate=RATE, target_lufs=-20.0, max_gain_db=60.0)
    plain = synth.synthesize(m, items, hop, seeds=11, equal_tokens=True, **dict(kw, **(dict(graphs={}) if case == "graphs" else {})))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(plain, synth.synthesize(m, items, hop, seeds=11, equal_tokens=True, loudness=None, **dict(kw, **(dict(graphs={}) if case == "graphs" else {})))))
    for again in range(2 if case == "graphs" else 1):                            # (the second call replays the captured steps)
        out = synth.synthesize(m, items, hop, seeds=11, equal_tokens=True, loudness=opt, **kw)
        for i, w in enumerate(out):
            assert w.dtype == np.float32 and w.shape == plain[i].shape
            for got, alone in zip(np.atleast_2d(w), np.atleast_2d(plain[i])):     # every take on its own
                want = normalized_alone(alone, target_lufs=-20.0, max_gain_db=60.0)
                assert np.array_equal(bits(got[None]), bits(want)), (case, i)
        assert all(not np.array_equal(w, p) for w, p in zip(out, plain))          # every item has a block over the gates: every item is scaled
    if case == "streams":
        one = synth.synthesize(m, items, hop, seeds=11, equal_tokens=True, loudness=opt, streams=1, max_frames_per_batch=700)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(out, one))
    if case == "takes":                                                          # two takes of an item differ, and so do their gains
        loud = [lo.measure(cu(w), RATE)[0].cpu().numpy() for w in out]
        print(f"takes: delivered loudness {[l.tolist() for l in loud]}")
        assert all(np.abs(l + 20.0).max() <= 1e-3 for l in loud)


def test_driver_runs_the_stage_between_the_converter_and_the_limiter(driver, long_items):
    """resample_to, loudness and limit in one call: each waveform equals, bit for bit, limit_peaks(normalize(resample())) of the plain one, the loudness measured
    at the output rate with the rows' lengths at that rate"""
    from visinger_amd import limiter as lm
    from visinger_amd import resample as rs
    from visinger_amd import synth
    m, _, hop, nph = driver
    items = long_items
    to = dict(sample_rate=RATE, output_rate=12000)
    opt = dict(sample_rate=RATE, target_lufs=-14.0, max_gain_db=60.0)
    plain = synth.synthesize(m, items, hop, seeds=11, streams=1)
    before = [lo.normalize(rs.resample(cu(w[None]), RATE, 12000), 12000, target_lufs=-14.0, max_gain_db=60.0) for w in plain]
    peak = max(float(w.abs().max()) for w in before)
    lim = dict(ceiling_db=min(0.0, 20.0 * np.log10(peak) - 6.0), window=16)       # 6 dB under the loudest normalised sample
    c = np.float32(lm.check_args(**lim)[0])
    want = [lm.limit_peaks(w, **lim).cpu().numpy() for w in before]
    for streams in (1, 2):
        out = synth.synthesize(m, items, hop, seeds=11, streams=streams, resample_to=to, loudness=opt, limit=lim)
        for i, w in enumerate(out):
            assert w.shape == (rs.out_length(len(plain[i]), RATE, 12000),) and np.array_equal(bits(w[None]), bits(want[i])), (streams, i)
            assert (np.abs(w) <= c).all()
    assert any((w.abs() > float(c)).any() for w in before)
    # the limiter's reduction lowers the delivered loudness of the item it reaches
    loud = [float(lo.measure(cu(w[None]), 12000)[0][0]) for w in out]
    print(f"delivered behind the limiter: {loud} (target -14)")
    assert any(l < -14.0 - 1e-3 for l in loud)
