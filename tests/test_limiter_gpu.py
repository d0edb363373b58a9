"""The peak limiter on an MI355X (csrc/limiter.hip, include/visinger_hip.h "f11"): vs_peak_limit's gain and stats bit for bit against the numpy
restatement ``limiter.limit_ref`` at the tile and halo edges, the waveform against the restatement's fp64 value, the ceiling exactly, the 16-byte / 4-byte and the
in-place paths, batching, a graph replay, and ``synthesize(limit=)`` bit for bit ``limit_peaks()`` of each plain waveform.  tests/test_limiter_cpu.py holds the
restatement to the rule."""
import numpy as np
import pytest
import torch

from visinger_amd import limiter as lm
from test_resample_gpu import driver  # noqa: F401  (the tiny model and three ragged items)

pytestmark = pytest.mark.gpu

TILE = lm.TILE                  # VS_PEAK_LIMIT_TILE (test_limiter_cpu.py holds the Python constant to the header)
WINDOWS = (0, 1, 7, 1024)
C = np.float32(10.0 ** (-1.0 / 20.0))
REL_WORST = 1.1751e-7           # the worst relative error of vs_peak_limit against fp64 over every launch of this file, measured on an MI355X
REL_BAR = 8 * REL_WORST


def cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def amplitudes(rng, k, c=C):
    """k finite over-ceiling values below c 2^24, either sign"""
    return (float(c) * np.exp2(rng.uniform(0.001, 23.9, k)) * rng.choice([-1.0, 1.0], k)).astype(np.float32)


def edge_rows(rng, L, W, c=C):
    """(x [5, L], lens): quiet noise with 1e3 beyond each length and peaks at sample 0, n - 1, the tile's edge, the far edge of the halo, pairs 2 W and 2 W + 2
    apart across a tile boundary, and a run longer than 4 W"""
    lens = [L, 0, max(L - 1, 0), (L + 1) // 2, min(L, TILE + 1)]
    x = (rng.uniform(-0.5, 0.5, (5, L)) * float(c)).astype(np.float32)
    spots = [0, TILE - 1, TILE, TILE - 2 * W, TILE + 2 * W, TILE - 2 * W - 1, TILE + 2 * W + 1, 2 * TILE - 1, 2 * TILE + 2]
    pairs = [(TILE - W - 1, TILE + W - 1), (2 * TILE - W - 1, 2 * TILE + W + 1), (TILE // 4, TILE // 4 + 2 * W), (TILE // 4 + 4 * W + 9, TILE // 4 + 6 * W + 11)]
    for b, n in enumerate(lens):
        mine = [p for p in spots[b % 2::2] + [n - 1] + [q for pr in pairs[b % 2::2] for q in pr] if 0 <= p < n]
        x[b, mine] = amplitudes(rng, len(mine), c)
        run = TILE // 2 + 13 * b
        if run < n:
            stop = min(n, run + 4 * W + 5)
            x[b, run:stop] = amplitudes(rng, stop - run, c)
        x[b, n:] = 1e3
    return x, lens


def hold(x, lens, W, c=C, y=None, g=None, stats=None):
    """the kernel's (y, g, stats) -- computed here unless given -- held to the restatement; returns them as numpy arrays"""
    if y is None:
        y, g, stats = lm.limit_peaks(cu(x), lengths=None if lens is None else torch.tensor(lens, device="cuda"), return_gain=True, return_stats=True,
                                     ceiling_db=20.0 * np.log10(float(c)), window=W)
        assert lm.check_args(ceiling_db=20.0 * np.log10(float(c)))[0] == float(c)
    y, g, stats = (t.cpu().numpy() if torch.is_tensor(t) else t for t in (y, g, stats))
    B, L = x.shape
    n = np.full(B, L) if lens is None else np.asarray(lens)
    u, M, gr, y64 = lm.limit_ref(x, lens, c, W)
    # gain and stats: integers, bit for bit
    assert g.dtype == np.int32 and np.array_equal(g, gr), (W, np.flatnonzero((g != gr).any(axis=1)))
    assert np.array_equal(stats[:, 0], (u > 0).sum(axis=1)) and np.array_equal(stats[:, 1], gr.max(axis=1))
    # the waveform
    inside = np.arange(L)[None] < n[:, None]
    assert np.array_equal(bits(y)[g == 0], bits(x)[g == 0])                     # x's bits wherever g = 0: beyond each length too
    assert (np.abs(y[inside & ~np.isnan(y)]) <= c).all()                         # the ceiling, exactly
    assert np.array_equal(np.isnan(y), np.isnan(x))
    on = (g > 0) & ~np.isnan(x)
    with np.errstate(over="ignore", invalid="ignore"):
        exact = np.abs(x.astype(np.float64)) * np.exp2(-gr / 512.0)             # before the guard
    must, at_c = on & (exact > float(c) * (1 + REL_BAR)), on & (np.abs(y) == c)  # the guard has moved these for certain / can only have moved these
    assert (must.sum(axis=1) <= stats[:, 2]).all() and (stats[:, 2] <= at_c.sum(axis=1)).all() and not (must & ~at_c).any()
    err = np.abs(y[on].astype(np.float64) - y64[on])
    rel = float((err[y64[on] != 0] / np.abs(y64[on][y64[on] != 0])).max()) if (y64[on] != 0).any() else 0.0
    print(f"limiter rel {rel:.4e} L {L} W {W} moved {int(stats[:, 2].sum())}")
    assert rel <= REL_BAR and not err[y64[on] == 0].any()
    return y, g, stats


@pytest.mark.parametrize("L", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_gain_and_stats_bit_for_bit_at_the_tile_and_halo_edges_under_every_window(L):
    rng = np.random.default_rng(100 + L)
    for W in WINDOWS:
        x, lens = edge_rows(rng, L, W)
        y, g, stats = hold(x, lens, W)
        if L > 1:
            assert g.any() and not g[1].any() and stats[1].tolist() == [0, 0, 0]
    x, lens = edge_rows(rng, L, 7)                                               # lengths = None: every row is L long, the 1e3 of the padding included
    hold(x, None, 7)


def test_other_ceilings_and_the_default_window():
    rng = np.random.default_rng(7)
    for c_db in (0.0, -6.0, -40.0):
        c = np.float32(lm.check_args(ceiling_db=c_db)[0])
        x, lens = edge_rows(rng, TILE + 200, 128, c)
        hold(x, lens, 128, c)


def test_an_infinity_and_a_nan_in_a_row():
    rng = np.random.default_rng(8)
    W, L = 7, TILE + 64
    x = (rng.uniform(-0.5, 0.5, (2, L)) * float(C)).astype(np.float32)
    x[0, TILE - 3], x[0, 100], x[0, TILE - 9], x[0, 3000] = np.inf, -np.inf, np.nan, np.nan
    x[1, 50] = np.nan
    y, g, stats = hold(x, None, W)
    assert y[0, TILE - 3] == C and y[0, 100] == -C and stats[0].tolist() == [2, lm.U_MAX, 2]
    assert (g[0, TILE - 3 - W:TILE - 3 + W + 1] > lm.U_MAX // 2).all() and (np.abs(y[0, TILE - 3 - W:TILE - 3 + W + 1][~np.isin(np.arange(2 * W + 1), (1, W))]) < 1e-3).all()      # (but the NaN and the infinity itself)
    assert np.isnan(y[0, TILE - 9]) and g[0, TILE - 9] > 0                      # within 2 W of the infinity: through the product, still a NaN
    assert bits(y)[0, 3000] == bits(x)[0, 3000] and g[0, 3000] == 0              # out of reach: its own bits
    assert not g[1].any() and np.array_equal(bits(y[1]), bits(x[1])) and stats[1].tolist() == [0, 0, 0]


def test_the_4_byte_path_gives_the_16_byte_paths_bits():
    rng = np.random.default_rng(9)
    W, L = 7, 2 * TILE + 8
    x, lens = edge_rows(rng, L, W)
    y, g, stats = hold(x, lens, W)                                              # L % 4 == 0, an aligned base: 16-byte loads
    buf = torch.zeros(5 * L + 1, device="cuda")
    off = buf[1:].view(5, L)                                                     # the row base offset by one float
    off.copy_(cu(x))
    assert off.data_ptr() % 16 == 4
    y2, g2, s2 = lm.limit_peaks(off, lengths=lens, return_gain=True, return_stats=True, window=W)
    assert np.array_equal(bits(y2), bits(y)) and np.array_equal(g2.cpu().numpy(), g) and np.array_equal(s2.cpu().numpy(), stats)
    # an odd L: the same rows one sample shorter
    xo, lo = x[:, :L - 1].copy(), [min(n, L - 1) for n in lens]
    yo, go, so = hold(xo, lo, W)
    keep = TILE                                                                  # (far from the cut end the two runs see the same samples)
    assert np.array_equal(bits(yo[:, :keep]), bits(y[:, :keep])) and np.array_equal(go[:, :keep], g[:, :keep])


@pytest.mark.parametrize("L", [2 * TILE + 3, 3 * TILE])
def test_in_place_and_without_gain_and_stats(L):
    rng = np.random.default_rng(10 + L)
    for W in WINDOWS:
        x, lens = edge_rows(rng, L, W)
        y, g, stats = hold(x, lens, W)
        only = lm.limit_peaks(cu(x), lengths=lens, window=W)                     # gain and stats NULL
        assert torch.is_tensor(only) and np.array_equal(bits(only), bits(y))
        xs = cu(x)
        back, g2, s2 = lm.limit_peaks(xs, lengths=lens, out=xs, return_gain=True, return_stats=True, window=W)
        assert back.data_ptr() == xs.data_ptr()
        assert np.array_equal(bits(xs), bits(y)) and np.array_equal(g2.cpu().numpy(), g) and np.array_equal(s2.cpu().numpy(), stats)
        xs = cu(x)
        lm.limit_peaks(xs, lengths=lens, out=xs, window=W)
        assert np.array_equal(bits(xs), bits(y))
        out = torch.full((5, L), -7.0, device="cuda")
        assert lm.limit_peaks(cu(x), lengths=lens, out=out, window=W) is out and np.array_equal(bits(out), bits(y))


def test_a_row_does_not_depend_on_the_launch():
    rng = np.random.default_rng(11)
    W, L = 7, 2 * TILE + 3
    x, lens = edge_rows(rng, L, W)
    y, g, stats = hold(x, lens, W)
    for b in (0, 2, 3):
        n = lens[b]
        alone = lm.limit_peaks(cu(x[b:b + 1, :n]), return_gain=True, return_stats=True, window=W)
        wide = np.full((1, n + 777), -1e3, np.float32)
        wide[0, :n] = x[b, :n]
        padded = lm.limit_peaks(cu(wide), lengths=[n], return_gain=True, return_stats=True, window=W)
        for got in (alone, padded):
            assert np.array_equal(bits(got[0][:, :n]), bits(y[b:b + 1, :n])) and np.array_equal(got[1].cpu().numpy()[:, :n], g[b:b + 1, :n])
            assert np.array_equal(got[2].cpu().numpy(), stats[b:b + 1])
        assert np.array_equal(bits(padded[0][:, n:]), bits(wide[:, n:])) and not padded[1][:, n:].any()


def test_graph_replays_on_other_data():
    rng = np.random.default_rng(13)
    W, L = 7, 2 * TILE + 3
    wav, lens = torch.zeros((5, L), device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda")

    def load():
        x, n = edge_rows(rng, L, W)
        order = rng.permutation(5)
        x, n = x[order], [n[i] for i in order]
        wav.copy_(cu(x)), lens.copy_(torch.tensor(n, device="cuda"))
        return x, n

    run = lambda: lm.limit_peaks(wav, lengths=lens, return_gain=True, return_stats=True, window=W)
    load()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    first = out[1].clone()
    x, n = load()
    graph.replay()
    assert not torch.equal(out[1], first)
    hold(x, n, W, y=out[0], g=out[1], stats=out[2])


def test_refused_calls_launch_nothing():
    """the refusals themselves are tests/test_limiter_cpu.py's; here: a refused call leaves its outputs alone"""
    from visinger_amd import _args, _lib
    import ctypes
    lib = _lib.require_gpu()
    x = torch.full((2, 64), 5.0, device="cuda")
    y, g, s = torch.full((2, 64), -7.0, device="cuda"), torch.full((2, 64), 9, dtype=torch.int32, device="cuda"), torch.full((2, 3), 9, dtype=torch.int32, device="cuda")
    tab, p, st = lm.reduction_table("cuda"), _args.vp, _lib.stream_ptr()
    for c, W, out in ((0.0, 4, y), (0.5, 1025, y), (0.5, 4, x.view(-1)[1:])):
        assert lib.vs_peak_limit(p(x), None, p(tab), ctypes.c_float(c), W, p(out), p(g), p(s), 2, 64 if out is y else 63, st) == 1
    torch.cuda.synchronize()
    assert (y == -7).all() and (g == 9).all() and (s == 9).all() and (x == 5).all()
    assert lib.vs_peak_limit(p(x), None, p(tab), ctypes.c_float(0.5), 4, p(y), p(g), p(s), 2, 64, st) == 0
    torch.cuda.synchronize()
    assert (y.abs() <= 0.5).all() and (g > 0).all() and (s[:, 0] == 64).all()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------------------

def limited_alone(w, **kw):
    return lm.limit_peaks(cu(np.atleast_2d(w)), **kw).cpu().numpy()


def peak_db(wavs, plus):
    """a ceiling `plus` dB from the loudest sample of the waveforms, at most full scale"""
    return min(0.0, 20.0 * float(np.log10(max(np.abs(w).max() for w in wavs))) + plus)


@pytest.mark.parametrize("case", ["ragged", "takes", "streams", "graphs", "dynamics", "resample"])
def test_driver_limits_the_output(driver, case):
    """synthesize(limit=) equals, bit for bit, limit_peaks() of each waveform the call returns without limit"""
    from visinger_amd import synth
    m, items, hop, nph = driver
    kw = dict(ragged=dict(), takes=dict(takes=2), streams=dict(streams=2, max_frames_per_batch=40 * nph), graphs=dict(graphs={}),
              resample=dict(resample_to=dict(sample_rate=24000, output_rate=44100)),
              dynamics=dict(guide_dynamics=dict(mode="absolute", max_boost_db=12.0, gate_db=-150.0), resample_to=dict(sample_rate=24000, output_rate=44100)))[case]
    bare = synth.synthesize(m, items, hop, seeds=11, equal_tokens=True)
    if case == "dynamics":                                                       # a level far over full scale: every frame takes the whole +12 dB
        items = [dict(it, level=np.full(len(it["mel2ph"]), 1e6, np.float32)) for it in items[:-1]] + [items[-1]]
    plain = synth.synthesize(m, items, hop, seeds=11, equal_tokens=True, **dict(kw, **(dict(graphs={}) if case == "graphs" else {})))
    # dynamics: a ceiling just over what the model itself reaches, which the boost then exceeds; otherwise one 6 dB under the loudest sample
    lim = dict(ceiling_db=peak_db(bare, 1.0) if case == "dynamics" else peak_db(plain, -6.0), window=16)
    c = np.float32(lm.check_args(**lim)[0])
    assert any((np.abs(w) > c).any() for w in plain)
    if case == "dynamics":
        assert all((np.abs(w) > c).any() for w in plain[:-1])
    for again in range(2 if case == "graphs" else 1):                            # (the second call replays the captured steps)
        out = synth.synthesize(m, items, hop, seeds=11, equal_tokens=True, limit=lim, **kw)
        for i, w in enumerate(out):
            want = limited_alone(plain[i], **lim)
            assert w.dtype == np.float32 and w.shape == plain[i].shape and np.array_equal(bits(np.atleast_2d(w)), bits(want)), (case, i)
            assert (np.abs(w) <= c).all()
        assert any(not np.array_equal(w, p) for w, p in zip(out, plain))


@pytest.mark.parametrize("takes", [1, 2])
@pytest.mark.parametrize("route", ["one_stream", "streams", "graphs"])
def test_driver_runs_all_three_stages_on_every_route(driver, route, takes):
    """guide_dynamics, resample_to and limit in one call, with the curve asked back: each waveform equals, bit for bit, limit_peaks(resample(match_dynamics()))
    of the waveform the same call on the same route returns without the three -- the item without a level skipping match_dynamics -- and the f0 curve is the
    plain call's.  This holds the one row-length tensor, the post chain's bundle and the one issue path.  It cannot see a tensor missing from what is recorded
    on a batch's stream: that is held by construction -- the recorded list is the batch record, into which every device tensor of a batch goes as it is made --
    and no test tries to provoke the race."""
    from visinger_amd import dynamics as dy
    from visinger_amd import resample as rs
    from visinger_amd import synth
    m, items, hop, nph = driver
    frames = [len(it["mel2ph"]) for it in items]
    route_kw = dict(one_stream=dict(streams=1), streams=dict(streams=2, max_frames_per_batch=40 * nph), graphs=dict(graphs={}))[route]
    kw = dict(route_kw, seeds=11, takes=takes, return_f0=True)
    dyn, to = dict(mode="absolute", max_boost_db=12.0, gate_db=-150.0), dict(sample_rate=24000, output_rate=44100)
    levelled = [dict(it, level=np.full(len(it["mel2ph"]), 1e6, np.float32)) for it in items[:2]] + [items[2]]      # item 2 carries none
    plain = synth.synthesize(m, items, hop, **dict(kw, **(dict(graphs={}) if route == "graphs" else {})))
    before = []                                                                  # the first two stages by hand, on the device
    for (w, _), it in zip(plain, levelled):
        w = cu(np.atleast_2d(w))
        if "level" in it:
            w = dy.match_dynamics(w, cu(np.repeat(it["level"][None], len(w), axis=0)), hop, **dyn)
        before.append(rs.resample(w, 24000, 44100))
    lim = dict(ceiling_db=peak_db([w.cpu().numpy() for w in before], -6.0), window=16)      # 6 dB under the loudest sample in front of the limiter
    c = np.float32(lm.check_args(**lim)[0])
    assert any((w.abs() > float(c)).any() for w in before)
    want = [lm.limit_peaks(w, **lim).cpu().numpy() for w in before]
    for again in range(2 if route == "graphs" else 1):                           # (the second call replays the captured steps)
        out = synth.synthesize(m, levelled, hop, guide_dynamics=dyn, resample_to=to, limit=lim, **kw)
        for i, (w, f0) in enumerate(out):
            assert w.dtype == np.float32 and w.shape == ((takes,) if takes > 1 else ()) + (rs.out_length(frames[i] * hop, 24000, 44100),), (route, i, w.shape)
            assert np.array_equal(bits(np.atleast_2d(w)), bits(want[i])), (route, takes, i)
            assert (np.abs(w) <= c).all()
            assert f0.shape == (frames[i],) and np.array_equal(bits(f0), bits(plain[i][1])), (route, takes, i)


def test_driver_quiet_items_and_no_key(driver):
    from visinger_amd import synth
    m, items, hop, nph = driver
    plain = synth.synthesize(m, items, hop, seeds=11)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(plain, synth.synthesize(m, items, hop, seeds=11, limit=None)))
    peaks = sorted(float(np.abs(w).max()) for w in plain)
    lim = dict(ceiling_db=min(0.0, 20.0 * np.log10(peaks[-1]) + 0.5), window=64)  # at or over every item's peak, unless the model itself leaves full scale
    c = lm.check_args(**lim)[0]
    out = synth.synthesize(m, items, hop, seeds=11, limit=lim)
    quiet = [float(np.abs(w).max()) <= c for w in plain]
    assert any(quiet) and all(np.array_equal(bits(a), bits(b)) for a, b, q in zip(plain, out, quiet) if q)
    if peaks[0] < peaks[-1]:                                                     # a ceiling between the quietest and the loudest item
        lim = dict(ceiling_db=min(0.0, 10.0 * np.log10(peaks[0] * peaks[-1])), window=64)
        c = lm.check_args(**lim)[0]
        out = synth.synthesize(m, items, hop, seeds=11, limit=lim)
        for a, b in zip(plain, out):
            assert np.array_equal(bits(a), bits(b)) == (float(np.abs(a).max()) <= c) and (np.abs(b) <= np.float32(c)).all()
    for bad in (3, dict(bogus=1), dict(window=-1)):
        with pytest.raises(ValueError):
            synth.synthesize(m, items, hop, seeds=11, limit=bad)
