"""Guide dynamics on the GPU (csrc/dynamics.hip, visinger_amd/dynamics.py) and through the synthesis driver: the four kernels against the numpy restatements
of tests/test_dynamics_cpu.py -- ``vs_level_track`` element by element under the derived bound of its fixed summation tree, ``vs_level_offset`` and
``vs_level_gain`` BIT FOR BIT (the rule is integer once quantised; every test curve sits a quarter unit off the quantisation grid), ``vs_level_apply`` the
input's bits where the gain is 0 and within REL_BAR of the fp64 value elsewhere -- at the tile edges, on both load paths, independent of the launch, under a
graph replay, and as the driver's ``guide_dynamics=``."""
import numpy as np
import pytest
import torch

from test_dynamics_cpu import apply_ref, gain_ref, level_of_units, level_ref, offset_ref, units
from test_guide_align_gpu import TRACK, driver as sung_driver  # noqa: F401  (the tiny model, its score and the tone-burst recording of the alignment test)
from test_resample_gpu import driver  # noqa: F401  (the tiny model and three ragged items)

pytestmark = pytest.mark.gpu

TILE = 1024                  # VS_LEVEL_GAIN_TILE (test_dynamics_cpu.py holds the Python constant to the header)
REL_WORST = 2.689e-7            # the worst relative error of vs_level_apply against fp64 over every launch of this file, measured on an MI355X
REL_BAR = 8 * REL_WORST


def cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def bits(t):
    return (t if isinstance(t, np.ndarray) else t.cpu().numpy()).view(np.uint32)


# ---- vs_level_track -----------------------------------------------------------------------------------------------------------------------------------

def ragged_wavs(rng, hop, counts, beyond=1e3):
    """rows of counts[b] whole frames plus a part of one, `beyond` behind each row's length"""
    lens = [c * hop + (b * 7) % hop for b, c in enumerate(counts)]
    wav = np.full((len(counts), max(lens) + 5), beyond, np.float32)
    for b, n in enumerate(lens):
        wav[b, :n] = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0)
    return wav, lens


def hold_track(got, wav, lens, hop, half, T):
    """every element within (4 ceil(hop / 256) + 2 half + 7) 2^-24 of level_ref, relative: all terms are non-negative, a lane's chain is 4 ceil(hop / 256) fmas
    deep, the butterfly 6 additions, the window 2 half + 1 more (the first onto 0, exact), the division one rounding"""
    bound = (4 * -(-hop // 256) + 2 * half + 7) * 2.0 ** -24
    worst = 0.0
    for b in range(len(lens)):
        ref = level_ref(wav[b], hop, half, length=lens[b], T=T)
        nb = min(lens[b] // hop, T)
        assert not got[b, nb:].any() and (ref[:nb] > 0).all(), b                 # exact zeros for t >= n_b
        err = np.abs(got[b, :nb].astype(np.float64) / ref[:nb] - 1.0)
        worst = max(worst, float(err.max()) if nb else 0.0)
    print(f"hop {hop}, half {half}: worst relative error {worst / 2.0 ** -24:.2f} x 2^-24 (bound {bound / 2.0 ** -24:.0f} x 2^-24)")
    assert worst <= bound


@pytest.mark.parametrize("hop", [256, 300, 50])
@pytest.mark.parametrize("half", [0, 1, 8])
def test_track_against_the_restatement(hop, half):
    """hop 256: the 16-byte path; 300: two loads a lane, the second partly filled; 50: hop % 4 != 0, the 4-byte path.  Frame counts around the tile and the wave"""
    from visinger_amd import dynamics as dy
    rng = np.random.default_rng(hop + half)
    wav, lens = ragged_wavs(rng, hop, [1, 63, 64, 65, 131, 255, 256, 257, 2 * 256 + 3])
    T = wav.shape[1] // hop
    got = dy.track_level(cu(wav), hop, lengths=torch.tensor(lens, device="cuda"), half_width=half)
    assert got.shape == (len(lens), T) and got.dtype == torch.float32
    hold_track(got.cpu().numpy(), wav, lens, hop, half, T)
    host = dy.track_level(cu(wav), hop, lengths=lens, half_width=half)
    assert np.array_equal(bits(host), bits(got))
    for frames in (T + 70, 200, 1):                                              # a capacity wider and narrower than the rows
        part = dy.track_level(cu(wav), hop, lengths=lens, half_width=half, frames=frames).cpu().numpy()
        hold_track(part, wav, lens, hop, half, frames)


def test_track_three_ragged_rows_without_lengths_and_with_zero():
    from visinger_amd import dynamics as dy
    rng = np.random.default_rng(4)
    wav, lens = ragged_wavs(rng, 256, [40, 7, 0])
    lens[2] = 100                                                                # shorter than a hop: no frame
    got = dy.track_level(cu(wav), 256, lengths=lens, half_width=1).cpu().numpy()
    hold_track(got, wav, lens, 256, 1, got.shape[1])
    assert not got[2].any()
    full = dy.track_level(cu(wav), 256).cpu().numpy()                            # lengths = None: the padding counts
    hold_track(full, wav, [wav.shape[1]] * 3, 256, 1, full.shape[1])
    assert full[1, 30] > 1e5


def test_track_a_misaligned_row_gives_the_vector_paths_bits():
    from visinger_amd import dynamics as dy
    rng = np.random.default_rng(5)
    wav, lens = ragged_wavs(rng, 256, [131, 64, 70])                             # (L = 131 * 256 + 5 is odd: rows 1 and 2 start off a 16-byte boundary anyway)
    wide = np.zeros((3, (wav.shape[1] + 4) & ~3), np.float32)
    wide[:, :wav.shape[1]] = wav
    aligned = dy.track_level(cu(wide), 256, lengths=lens)                        # every row on a 16-byte boundary: the 16-byte path
    store = torch.zeros(wide.size + 1, device="cuda")
    shifted = store[1:].view(3, -1)                                              # every row 4 bytes off one: the 4-byte path
    shifted.copy_(cu(wide))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    moved = dy.track_level(shifted, 256, lengths=lens)
    odd = dy.track_level(cu(wav), 256, lengths=lens)
    assert np.array_equal(bits(aligned), bits(moved)) and np.array_equal(bits(aligned)[:, :odd.shape[1]], bits(odd)[:, :aligned.shape[1]])


def test_track_a_nan_zeroes_exactly_the_frames_whose_blocks_hold_it():
    from visinger_amd import dynamics as dy
    rng = np.random.default_rng(6)
    wav = (0.1 * rng.standard_normal((2, 200 * 256))).astype(np.float32)
    clean = dy.track_level(cu(wav), 256, half_width=1).cpu().numpy()
    bad = wav.copy()
    bad[0, 100 * 256 + 17], bad[1, 64 * 256 - 1], bad[1, 0] = np.nan, np.inf, np.nan
    got = dy.track_level(cu(bad), 256, half_width=1).cpu().numpy()
    hit = np.zeros((2, 200), bool)
    hit[0, 99:102], hit[1, 62:65], hit[1, 0:2] = True, True, True
    assert (got[hit] == 0).all() and np.array_equal(bits(got[~hit]), bits(clean[~hit])) and (clean > 0).all()


# ---- vs_level_offset / vs_level_gain ------------------------------------------------------------------------------------------------------------------

def curve_pair(rng, T, stretches):
    """(guide, own): active on the frames of `stretches` ((first, end) pairs), every other frame inactive in one of four ways"""
    u_own = rng.integers(-5000, -1000, T)
    own, guide = level_of_units(u_own), level_of_units(u_own + rng.integers(-1500, 1500, T))
    on = np.zeros(T, bool)
    for a, e in stretches:
        on[max(a, 0):max(e, 0)] = True
    how = rng.integers(0, 4, T)
    guide[~on & (how == 0)] = 0.0
    guide[~on & (how == 1)] = np.nan
    own[~on & (how == 2)] = level_of_units(units(-70.0) - 1 - rng.integers(0, 2000))       # below the gate
    own[~on & (how == 3)] = -1.0
    return guide, own


def edge_rows(rng, T, window):
    rows = [curve_pair(rng, T, [(0, T)]),
            curve_pair(rng, T, [(TILE, 2 * TILE)]) if T > TILE else curve_pair(rng, T, [(T // 2, T)]),      # starts at a tile edge
            curve_pair(rng, T, [(0, TILE), (2 * TILE, T)]),                                                  # ends at one
            curve_pair(rng, T, [(TILE - 8, TILE + 7), (2 * TILE - 1, 2 * TILE + 1)]),                        # straddles
            curve_pair(rng, T, [(0, 3), (3 + 2 * window + 2, 3 + 2 * window + 6), (T - 2, T)]),              # a gap longer than 2 window
            curve_pair(rng, T, [(t, t + 1) for t in range(0, T, 37)]),
            curve_pair(rng, T, [])]                                                                          # all inactive
    lens = [T, T, max(T - 1, 0), T, T, T // 2, T]
    return rows, lens


def check_gain(rows, lens, offsets=None, lengths="device", **kw):
    """one launch of each kernel; every row bit for bit against the restatement of that row alone.  offsets: None (no offset), 'kernel' (vs_level_offset's own,
    as a device tensor) or a list"""
    from visinger_amd import dynamics as dy
    guide, own = cu(np.stack([r[0] for r in rows])), cu(np.stack([r[1] for r in rows]))
    B, T = guide.shape
    lens_arg = None if lengths is None else (torch.tensor(lens, device="cuda") if lengths == "device" else lens)
    gate_db = kw.get("gate_db", -70.0)
    off, n_act = dy.level_offset(guide, own, lengths=lens_arg, gate_db=gate_db)
    assert off.dtype == n_act.dtype == torch.int32 and off.shape == n_act.shape == (B,)
    arg = None if offsets is None else (off if offsets == "kernel" else offsets)
    k = dy.level_gain(guide, own, lengths=lens_arg, offset_units=arg, **kw)
    assert k.shape == (B, T) and k.dtype == torch.int32
    k, off, n_act = k.cpu().numpy(), off.cpu().tolist(), n_act.cpu().tolist()
    depth_q, window = int(round(256 * kw.get("depth", 1.0))), kw.get("window", 12)
    for b, (g, o) in enumerate(rows):
        n = T if lengths is None else lens[b]
        assert (off[b], n_act[b]) == offset_ref(g, o, n, units(gate_db)), b
        o_b = 0 if offsets is None else (off[b] if offsets == "kernel" else offsets[b])
        ref = gain_ref(g, o, n, o_b, units(gate_db), window, depth_q, units(kw.get("max_boost_db", 12.0)), units(kw.get("max_cut_db", 24.0)))
        assert np.array_equal(k[b], ref), (b, np.flatnonzero(k[b] != ref)[:8], k[b][k[b] != ref][:8], ref[k[b] != ref][:8])
    return k, off, n_act


@pytest.mark.parametrize("T", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_gain_and_offset_bit_for_bit_at_the_tile_edges_under_every_window(T):
    """T = TILE: the 16-byte path; the others: 4-byte.  Contour mode (the offset read from vs_level_offset's device tensor) and absolute mode"""
    rng = np.random.default_rng(T)
    for window in (0, 1, 7, 1024):
        rows, lens = edge_rows(rng, T, window)
        k, off, n_act = check_gain(rows, lens, offsets="kernel", window=window)
        check_gain(rows, lens, window=window, max_boost_db=3.0, max_cut_db=5.0)
        assert n_act[-1] == 0 and off[-1] == 0 and not k[-1].any() and (window >= T // 2 or k[:-1].any())      # (a window over the whole row: the offset takes the mean out)


def test_gain_parameters_offsets_and_values_that_are_no_level():
    rng = np.random.default_rng(9)
    T = TILE + 300
    rows, lens = edge_rows(rng, T, 12)
    check_gain(rows, lens, lengths=None, depth=0.5, window=20)
    check_gain(rows, lens, lengths="host", depth=0.3, gate_db=-40.0, window=3)
    assert not check_gain(rows, lens, depth=0.0)[0].any()
    check_gain(rows, lens, offsets=[0, 17, -900, 5000, -5000, 1 << 17, -(1 << 17)], max_boost_db=48.0, max_cut_db=48.0)
    odd = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -3.0, 1e-45, 3e38], np.float32), T)      # a denormal and a huge level quantise like any
    k = check_gain([(odd, rows[0][1]), (rows[0][0], odd), (odd, odd)], [T, T, T], gate_db=-700.0, max_boost_db=48.0, max_cut_db=48.0)[0]
    assert k.any()
    # the own curve times a constant: contour mode returns 0, absolute mode the constant
    own = rows[0][1]
    q = np.rint(256.0 * np.log2(own.astype(np.float64)) - 0.25).astype(np.int64)
    louder = (level_of_units(q + 450), own)
    assert not check_gain([louder], [T], offsets="kernel")[0].any() and (check_gain([louder], [T])[0] == 450).all()
    # an offset tensor outside [-2^17, 2^17] is read clamped
    from visinger_amd import dynamics as dy
    big = torch.tensor([1 << 30], dtype=torch.int32, device="cuda")
    assert np.array_equal(dy.level_gain(cu(louder[0][None]), cu(own[None]), offset_units=big).cpu().numpy()[0], gain_ref(louder[0], own, offset=1 << 30))


# ---- vs_level_apply -----------------------------------------------------------------------------------------------------------------------------------

def check_apply(x, k, hop, lens, worst):
    """out of place and in place; every row against apply_ref of that row alone; returns the worst relative error seen so far"""
    from visinger_amd import dynamics as dy
    xd, kd = cu(x), cu(k, np.int32)
    lens_arg = None if lens is None else torch.tensor(lens, device="cuda")
    y = dy.apply_gain(xd, kd, hop, lengths=lens_arg)
    assert y.data_ptr() != xd.data_ptr() and np.array_equal(bits(xd), bits(x))   # the input is left alone
    place = xd.clone()
    assert dy.apply_gain(place, kd, hop, lengths=lens_arg, out=place) is place and np.array_equal(bits(place), bits(y))
    y = y.cpu().numpy()
    for b in range(len(x)):
        ref, kappa = apply_ref(x[b], k[b], hop, None if lens is None else lens[b])
        still = kappa == 0
        assert np.array_equal(bits(y[b][still]), bits(x[b][still])), b            # the input's bits: NaNs, the tail and the padding included
        moved = ~still & np.isfinite(x[b]) & (x[b] != 0)
        assert moved.any() or not kappa.any()
        if moved.any():
            worst = max(worst, float(np.abs(y[b][moved] / ref[moved] - 1.0).max()))
        rest = ~still & ~moved
        assert np.array_equal(np.isnan(y[b][rest]), np.isnan(x[b][rest])) and np.array_equal(y[b][rest][~np.isnan(x[b][rest])], x[b][rest][~np.isnan(x[b][rest])])
    return worst


@pytest.mark.parametrize("hop", [256, 300, 50])
def test_apply_against_the_restatement(hop):
    """hop 256 with L % 4 == 0: 16-byte loads and stores; the odd row lengths: 4-byte; k beyond +-4096 is read clamped"""
    rng = np.random.default_rng(hop)
    worst = 0.0
    for T, extra in ((1, 0), (67, 0), (67, 3), (40, 2 * hop)):
        B, L = 4, T * hop + extra
        x = rng.standard_normal((B, L)).astype(np.float32)
        x[rng.random((B, L)) < 0.01] = np.nan
        x[rng.random((B, L)) < 0.01] = 0.0
        k = rng.integers(-1400, 1400, (B, T))
        k[1, T // 3:2 * T // 3 + 1] = 0                                          # a stretch that is left alone, ramps into and out of it
        k[2] = rng.integers(-6000, 6000, T)                                      # beyond the clamp
        k[3] = 0
        lens = [L, max(L - hop - 1, 0), L // 2, L]
        worst = check_apply(x, k, hop, lens, worst)
        worst = check_apply(x, k, hop, None, worst)
    print(f"hop {hop}: y relative error against fp64: {worst:.3e} (bar {REL_BAR:.3e})")
    assert worst <= REL_BAR


# ---- all four -----------------------------------------------------------------------------------------------------------------------------------------

def chain(dy, wav, guide, lens, hop, **kw):
    """(own, off, n_act, k, y) of the four kernels in match_dynamics' order"""
    T = guide.shape[1]
    frames = None if lens is None else torch.div(lens, hop, rounding_mode="floor").clamp(max=T)
    own = dy.track_level(wav, hop, lengths=lens, frames=T)
    off, n_act = dy.level_offset(guide, own, lengths=frames)
    k = dy.level_gain(guide, own, lengths=frames, offset_units=off, **kw)
    return own, off, n_act, k, dy.apply_gain(wav, k, hop, lengths=lens)


def phrase(rng, frames, hop):
    """a waveform with a loudness contour and a guide level curve with another one, on the quarter-unit grid"""
    env = np.repeat(10.0 ** rng.uniform(-2.5, -0.5, frames // 8 + 1), 8)[:frames]
    wav = (np.repeat(env, hop) * rng.standard_normal(frames * hop)).astype(np.float32)
    return wav, level_of_units(rng.integers(-4000, -500, frames))


@pytest.mark.parametrize("hop", [256, 50])
def test_a_row_does_not_depend_on_the_launch(hop):
    """a row alone, as row 2 of 5, and under other padding: the bits of all five results"""
    from visinger_amd import dynamics as dy
    rng = np.random.default_rng(12)
    frames = TILE + 77
    wav, guide = phrase(rng, frames, hop)
    alone = chain(dy, cu(wav[None]), cu(guide[None]), None, hop, window=9)
    assert alone[3].any() and int(alone[2][0]) > frames // 2
    B, T, L = 5, 2 * TILE + 8, (2 * TILE + 8) * hop + 3
    wavs, guides = np.full((B, L), 1e3, np.float32), np.full((B, T), 0.5, np.float32)
    for b in (0, 1, 3, 4):
        n = int(rng.integers(1, T))
        wavs[b, :n * hop], guides[b, :n] = phrase(rng, n, hop)
    wavs[2, :frames * hop], guides[2, :frames] = wav, guide
    lens = torch.tensor([L, 5 * hop, frames * hop, 0, 900 * hop + 1], device="cuda")
    batch = chain(dy, cu(wavs), cu(guides), lens, hop, window=9)
    for a, r in zip(alone, batch):                                                # own, off, n_act, k, y: the row's own frames / samples
        a, r = np.atleast_1d(a[0].cpu().numpy()), np.atleast_1d(r[2].cpu().numpy())
        assert np.array_equal(bits(a), bits(r[:len(a)])), (a.shape, r.shape)
    assert not batch[3][2, frames:].any() and not batch[0][2, frames:].any() and np.array_equal(bits(batch[4][2, frames * hop:]), bits(wavs[2, frames * hop:]))
    assert not batch[3][3].any() and np.array_equal(bits(batch[4][3]), bits(wavs[3]))          # a row of length 0 comes back as it is


def test_graph_replays_on_other_data():
    from visinger_amd import dynamics as dy
    rng = np.random.default_rng(13)
    hop, T = 256, TILE + 40
    wav, guide = torch.zeros((2, T * hop), device="cuda"), torch.zeros((2, T), device="cuda")
    lens = torch.zeros(2, dtype=torch.int64, device="cuda")

    def load(frames):
        w, g = np.full((2, T * hop), 1e3, np.float32), np.zeros((2, T), np.float32)
        for b, n in enumerate(frames):
            w[b, :n * hop], g[b, :n] = phrase(rng, n, hop)
        wav.copy_(cu(w)), guide.copy_(cu(g)), lens.copy_(torch.tensor([n * hop for n in frames], device="cuda"))
        return w, g

    run = lambda: chain(dy, wav, guide, lens, hop, window=5)
    load([T, 300])
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
    frames = [700, T - 3]
    w, g = load(frames)
    graph.replay()
    eager = run()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(out, eager)) and not torch.equal(out[3], first)
    for b, n in enumerate(frames):                                                # ... on the new rows' lengths (the tracked level is off the quarter-unit grid:
        assert n // 2 < int(out[2][b]) <= n and not out[3][b, n:].any() and out[3][b, :n].any()      # the restatement is held to in the tests above)
        assert np.array_equal(bits(out[4][b, n * hop:]), bits(w[b, n * hop:]))


def test_refused_calls_launch_nothing():
    """the refusals themselves are tests/test_dynamics_cpu.py's; here: a refused call leaves its outputs alone, the accepted one writes every element"""
    from visinger_amd import _args, _lib
    L = _lib.require_gpu()
    B, T, hop = 2, 48, 8
    wav, lvl = torch.rand((B, T * hop), device="cuda") + 0.1, torch.rand((B, T), device="cuda") + 0.1
    own, y = torch.full((B, T), -7.0, device="cuda"), torch.full((B, T * hop), -7.0, device="cuda")
    k, off, nact = (torch.full(s, 1 << 20, dtype=torch.int32, device="cuda") for s in ((B, T), (B,), (B,)))
    p, s = _args.vp, _lib.stream_ptr()
    assert L.vs_level_track(p(wav), None, B, T * hop, 0, 1, p(own), T, s) == 1 and L.vs_level_track(p(wav), None, B, T * hop, hop, 9, p(own), T, s) == 1
    assert L.vs_level_offset(p(lvl), p(own), None, 1 << 17, p(off), p(nact), B, T, s) == 1 and L.vs_level_offset(p(lvl), p(own), None, 0, p(off), p(off), B, T, s) == 1
    assert L.vs_level_gain(p(lvl), p(own), None, None, 0, 2000, 256, 100, 100, 0, p(k), B, T, s) == 1
    assert L.vs_level_gain(p(lvl), p(own), None, None, 0, 12, 256, 100, 100, 1, p(k), B, T, s) == 1
    assert L.vs_level_apply(p(wav), p(k), None, 4096, p(y), B, T * hop, T, s) == 1 and L.vs_level_apply(p(y), p(k), None, hop, p(y.view(-1)[1:]), B, T * hop, T, s) == 1
    torch.cuda.synchronize()
    assert (own == -7).all() and (k == 1 << 20).all() and (off == 1 << 20).all() and (nact == 1 << 20).all() and (y == -7).all()
    assert L.vs_level_track(p(wav), None, B, T * hop, hop, 1, p(own), T, s) == 0 and L.vs_level_offset(p(lvl), p(own), None, -60000, p(off), p(nact), B, T, s) == 0
    assert L.vs_level_gain(p(lvl), p(own), None, p(off), -60000, 12, 256, 1000, 1000, 0, p(k), B, T, s) == 0
    assert L.vs_level_apply(p(wav), p(k), None, hop, p(y), B, T * hop, T, s) == 0
    torch.cuda.synchronize()
    assert (own > 0).all() and (k.abs() <= 1000).all() and (nact == T).all() and (y > 0).all()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------------------

def levelled(items, rng):
    """the items, all but the last with a level curve of their own"""
    return [dict(it, level=level_of_units(rng.integers(-4000, -1000, len(it["mel2ph"])))) for it in items[:-1]] + [items[-1]]


def matched_alone(w, level, hop, **kw):
    from visinger_amd import dynamics as dy
    w = np.atleast_2d(w)
    return dy.match_dynamics(cu(w), cu(np.repeat(level[None], len(w), axis=0)), hop, **kw).cpu().numpy()


@pytest.mark.parametrize("case", ["ragged", "takes", "streams", "graphs", "resample"])
def test_driver_matches_the_dynamics(driver, case):
    """synthesize(guide_dynamics={}) equals, bit for bit, match_dynamics() of each plain waveform taken alone; an item without a level returns the plain bits"""
    from visinger_amd import resample as rs
    from visinger_amd import synth
    m, items, hop, nph = driver
    items = levelled(items, np.random.default_rng(31))
    bare = [{k: v for k, v in it.items() if k != "level"} for it in items]
    to = dict(sample_rate=24000, output_rate=44100)
    kw = dict(ragged=dict(), takes=dict(takes=2), streams=dict(streams=2, max_frames_per_batch=40 * nph), graphs=dict(graphs={}), resample=dict(resample_to=to))[case]
    dyn = dict(window=3, mode="absolute", max_boost_db=20.0) if case == "takes" else {}
    plain = synth.synthesize(m, bare, hop, seeds=11, equal_tokens=True, **dict(kw, **(dict(graphs={}) if case == "graphs" else {}), resample_to=None))
    before = [{k: np.array(v, copy=True) for k, v in it.items()} for it in items]
    for again in range(2 if case == "graphs" else 1):                            # (the second call replays the captured steps)
        out = synth.synthesize(m, items, hop, seeds=11, equal_tokens=True, guide_dynamics=dyn, **kw)
        for i, w in enumerate(out):
            want = matched_alone(plain[i], items[i]["level"], hop, **dyn) if "level" in items[i] else np.atleast_2d(plain[i])
            if case == "resample":
                want = rs.resample(cu(want), 24000, 44100).cpu().numpy()
            assert w.dtype == np.float32 and np.array_equal(bits(np.atleast_2d(w)), bits(want)), (case, i)
            assert ("level" in items[i]) == (not np.array_equal(np.atleast_2d(w), np.atleast_2d(plain[i]))) or case == "resample"
    assert all(a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a) for a, b in zip(items, before))      # the caller's items are not modified


def test_driver_without_the_new_keys_nothing_changes(driver):
    from visinger_amd import synth
    m, items, hop, nph = driver
    plain = synth.synthesize(m, items, hop, seeds=11)
    for kw in (dict(guide_dynamics=None), dict(guide_dynamics={}), dict(guide_dynamics=dict(depth=0.5))):      # no item carries a level: nothing is launched
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(plain, synth.synthesize(m, items, hop, seeds=11, **kw)))
    lv = levelled(items, np.random.default_rng(32))
    still = synth.synthesize(m, lv, hop, seeds=11, guide_dynamics=dict(depth=0.0))                            # depth 0: k = 0, the bits of the plain waveforms
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(plain, still))
    for bad, kw in ((lv, {}), ([dict(lv[0], level=lv[0]["level"][:-1])], dict(guide_dynamics={})), ([dict(lv[0], level=lv[0]["level"][None])], dict(guide_dynamics={}))):
        with pytest.raises(ValueError):
            synth.synthesize(m, bad, hop, seeds=11, **kw)


def test_driver_tracks_the_level_and_tempo_warps_it(sung_driver):
    """a tracked "level" is track_level of the (converted) recording, fitted as the f0 curve is; the alignment pre-pass leaves it alone; tempo warps it as
    timing.retime(curve=) does; the chain of the pre-passes by hand gives the call's waveform"""
    from visinger_amd import dynamics as dy
    from visinger_amd import resample as rs
    from visinger_amd import synth, timing
    m, item, hop, runs, sung, rec = sung_driver
    sung_item, G, n = dict(item, guide_wav=rec), len(rec) // hop, len(item["mel2ph"])
    own = dy.track_level(cu(rec[None]), hop, half_width=2).cpu().numpy()[0]
    free = synth.guide_items([sung_item], hop, "cuda", fit=False, level=2, **TRACK)[0]
    assert free["level"].dtype == np.float32 and np.array_equal(bits(free["level"]), bits(own)) and len(own) == G == len(free["f0"]) and "guide_wav" not in free
    fitted = synth.guide_items([sung_item], hop, "cuda", level=2, **TRACK)[0]
    assert fitted["level"].shape == (n,) and np.array_equal(fitted["level"][:min(n, G)], own[:min(n, G)]) and not fitted["level"][G:].any()
    assert "level" not in synth.guide_items([sung_item], hop, "cuda", **TRACK)[0]
    kept = synth.guide_items([dict(sung_item, level=np.ones(n, np.float32))], hop, "cuda", level=2, **TRACK)[0]           # an item's own curve stays
    assert (kept["level"] == 1).all()
    # a recording at another rate: tracked from the converted samples
    at48 = synth.guide_items([sung_item], hop, "cuda", fit=False, level=1, **dict(TRACK, recording_rate=48000))[0]
    conv = rs.resample(cu(rec[None]), 48000, 24000)
    assert np.array_equal(bits(at48["level"]), bits(dy.track_level(conv, hop, half_width=1)[0, :len(at48["level"])]))
    # alignment leaves it alone, tempo warps it
    aligned = synth.align_items([free], "cuda")[0]
    assert np.array_equal(aligned["level"], free["level"]) and len(aligned["mel2ph"]) == G
    fast = synth.retime_items([aligned], 2, "cuda")[0]
    m2p = torch.from_numpy(np.asarray(aligned["mel2ph"], dtype=np.int64))[None].cuda()
    _, lens, warped = timing.retime(mel2ph=m2p, T_ph=len(item["text_tokens"]), stretch=torch.ones((1, len(item["text_tokens"])), device="cuda"), tempo=[2.0],
                                    curve=cu(free["level"][None]))
    assert len(fast["level"]) == len(fast["mel2ph"]) == int(lens[0]) and np.array_equal(bits(fast["level"]), bits(warped[0, :int(lens[0])]))
    # the whole call is the chain by hand
    dyn = dict(half_width=2, window=20)
    wav = synth.synthesize(m, [sung_item], hop, seeds=7, guide_track=TRACK, guide_align={}, tempo=2, guide_dynamics=dyn)[0]
    by_hand = synth.synthesize(m, [fast], hop, seeds=7, guide_dynamics=dyn)[0]
    plain = synth.synthesize(m, [{k: v for k, v in fast.items() if k != "level"}], hop, seeds=7)[0]
    assert np.array_equal(bits(wav), bits(by_hand)) and np.array_equal(bits(wav), bits(matched_alone(plain, fast["level"], hop, **dyn)[0]))
    assert not np.array_equal(wav, plain) and len(wav) == len(fast["mel2ph"]) * hop
