"""Guide pitch correction on the GPU (csrc/guide_correct.hip, visinger_amd/guide_correct.py) and through the synthesis driver: both kernels against the numpy
restatement ``correct_ref`` / ``deviation_ref`` of tests/test_guide_correct_cpu.py -- k, dev_med and n_corr BIT FOR BIT (the rule is integer once quantised; every
test curve sits a quarter unit off the quantisation grid, where fp32 rounding cannot move it), f0_out the input's bits where k == 0 and within REL_BAR of the
fp64 value f0 2^(-k / 19200) elsewhere -- at the tile edges, independent of the launch, on every VS_EINVAL, under a graph replay, and as the driver's
``guide_correct=`` pre-pass."""
import ctypes

import numpy as np
import pytest
import torch

from test_guide_align_gpu import TRACK, driver  # noqa: F401  (the tiny model, its score and the tone-burst recording of the alignment test)
from test_guide_correct_cpu import OCTAVE, correct_ref, deviation_ref, hz_of_units, quantise, random_item, sung_score, units_of_hz

pytestmark = pytest.mark.gpu

TILE = 1024                  # VS_GUIDE_CORRECT_TILE (test_guide_correct_cpu.py::test_check_args holds the Python constant to the header)
REL_WORST = 1.266e-7         # the worst relative error of f0_out against fp64 over every launch of this file, measured on an MI355X
REL_BAR = 8 * REL_WORST


def cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def collate(items, T=None, T_ph=None, fill=(0.0, 0, 0.0)):
    """items: (f0, mel2ph, note_midi) per row -> padded numpy [B, T], [B, T], [B, T_ph] with `fill` beyond each row's own sizes, and the rows' lengths"""
    B = len(items)
    T = max(len(it[0]) for it in items) if T is None else T
    T_ph = max(len(it[2]) for it in items) if T_ph is None else T_ph
    f0, m2p, note = np.full((B, T), fill[0], np.float32), np.full((B, T), fill[1], np.int64), np.full((B, T_ph), fill[2], np.float32)
    for b, (f, m, n) in enumerate(items):
        f0[b, :len(f)], m2p[b, :len(m)], note[b, :len(n)] = f, m, n
    return f0, m2p, note, [len(it[0]) for it in items]


def check(items, offsets=None, lengths="device", T=None, T_ph=None, fill=(0.0, 0, 0.0), **kw):
    """one launch of each kernel over `items`, every row against the restatement of that row alone; returns (k, f0_out, dev_med, n_corr, worst relative error)"""
    from visinger_amd import guide_correct
    f0, m2p, note, lens = collate(items, T, T_ph, fill)
    B, T = f0.shape
    lens_arg = None if lengths is None else (torch.tensor(lens, device="cuda") if lengths == "device" else lens)
    offs = None if offsets is None else cu(offsets)                                       # (a device tensor: used as it is, non-finite values included)
    out, k = guide_correct.correct_guide(cu(f0), cu(m2p, np.int64), cu(note), lengths=lens_arg, offset_cents=offs, return_units=True, **kw)
    dev_kw = {key: v for key, v in kw.items() if key in ("wild_cents", "octave_fold")}
    med, n_corr = guide_correct.guide_deviation(cu(f0), cu(m2p, np.int64), cu(note), lengths=lens_arg, offset_cents=offs, **dev_kw)
    assert out.shape == k.shape == (B, T) and out.dtype == torch.float32 and k.dtype == med.dtype == n_corr.dtype == torch.int32 and med.shape == n_corr.shape == (B,)
    out, k, med, n_corr = out.cpu().numpy(), k.cpu().numpy(), med.cpu().numpy(), n_corr.cpu().numpy()
    worst = 0.0
    for b, (f, m, nt) in enumerate(items):
        n = len(f) if lengths is not None else T
        oc = 0.0 if offsets is None else offsets[b]
        ref_k, _ = correct_ref(f0[b, :n], m2p[b, :n], note[b], offset_cents=oc, **kw)      # (the row's T_ph tokens, padding included)
        assert np.array_equal(k[b, :n], ref_k), (b, np.flatnonzero(k[b, :n] != ref_k)[:8], k[b, :n][k[b, :n] != ref_k][:8], ref_k[k[b, :n] != ref_k][:8])
        assert not k[b, n:].any()
        still = k[b] == 0
        assert np.array_equal(out[b][still].view(np.uint32), f0[b][still].view(np.uint32))    # the input's bits, padding, NaNs and garbage included
        if (~still).any():
            exact = f0[b][~still].astype(np.float64) * 2.0 ** (-k[b][~still].astype(np.float64) / OCTAVE)
            worst = max(worst, float(np.abs(out[b][~still] / exact - 1.0).max()))
        assert (int(med[b]), int(n_corr[b])) == deviation_ref(f0[b, :n], m2p[b, :n], note[b], offset_cents=oc, **dev_kw), b
    print(f"f0_out relative error against fp64: {worst:.3e} (bar {REL_BAR:.3e})")
    assert worst <= REL_BAR
    return k, out, med, n_corr, worst


def stepped(rng, T, bounds, T_ph=None):
    """an item whose tokens change exactly at the frames `bounds` (a new token with another pitch starts there), voiced throughout, detuned up to a semitone"""
    bounds = sorted(set(b for b in bounds if 0 < b < T))
    mel2ph = np.ones(T, np.int64)
    for b in bounds:
        mel2ph[b:] += 1
    n_tok = len(bounds) + 1
    note = (60 + (np.arange(n_tok) % 2) * 3 + rng.integers(0, 4, n_tok) / 4.0).astype(np.float32)      # neighbours always differ
    m = np.rint(1600.0 * (note[mel2ph - 1].astype(np.float64) - 69)).astype(np.int64)
    f0 = hz_of_units(m + rng.integers(-1600, 1601, T))
    return f0, mel2ph, np.concatenate([note, np.zeros((T_ph or n_tok) - n_tok, np.float32)])


def test_one_frame():
    note = np.array([64.0, 0.0], np.float32)
    one = lambda hz, tok: (np.array([hz], np.float32), np.array([tok], np.int64), note)
    k, out, med, n_corr, _ = check([one(hz_of_units(-8000 + 333), 1), one(0.0, 1), one(300.0, 2), one(300.0, 0)])
    assert k[:, 0].tolist() == [333, 0, 0, 0] and med.tolist() == [333, 0, 0, 0] and n_corr.tolist() == [1, 0, 0, 0]
    check([one(hz_of_units(-8000 - 41), 1)], lengths=None, window=0)


@pytest.mark.parametrize("T", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_tile_edges_and_every_window(T):
    """segments that start, end and straddle exactly at the tile edges, under W = 0, 1, 7, TILE and 1024 (T = TILE: the 16-byte path; the others: scalar)"""
    rng = np.random.default_rng(T)
    rows = [stepped(rng, T, [TILE, 2 * TILE]),                                            # start at the edge
            stepped(rng, T, [TILE - 1, TILE + 1, 2 * TILE - 1, 2 * TILE + 1]),            # one frame before and after it
            stepped(rng, T, [TILE - 8, TILE + 7, 2 * TILE - 3]),                          # straddling, inside a small window
            stepped(rng, T, [5, TILE - 600, TILE + 500]),                                 # straddling, longer than TILE
            stepped(rng, T, []),                                                          # one segment for the whole row
            random_item(rng, T, 200, seg=(1, 30))]
    for W in (0, 1, 7, TILE, 1024):
        k = check(rows, window=W)[0]
        assert (k != 0).mean() > 0.5


def test_a_segment_longer_than_two_windows_and_a_tile():
    rng = np.random.default_rng(5)
    T = 4 * TILE + 40
    for W in (7, 300, 1024):
        n = 2 * W + TILE + 50
        rows = [stepped(rng, T, [100, 100 + n]), stepped(rng, T, [TILE - W - 1, TILE - W - 1 + n, T - 3])]
        check(rows, window=W)


def test_lengths_zero_short_and_garbage_beyond():
    """beyond a row's length the buffers hold a voiced, pitched curve: it must not be read (k = 0, f0_out its bits) and not count for the frames before it"""
    rng = np.random.default_rng(7)
    rows = [random_item(rng, n, 40) for n in (0, 1, 700, TILE - 1, TILE + 300, 1500)]
    for W in (5, 1024):
        k, out, med, n_corr, _ = check(rows, T=1500, fill=(float(hz_of_units(-14400 + 900)), 1, 60.0), window=W)
        assert n_corr[0] == 0 and med[0] == 0
    host = check(rows, T=1500, lengths="host", window=5)
    assert np.array_equal(host[0], check(rows, T=1500, window=5)[0])


def test_unvoiced_rows_rest_rows_and_values_that_are_no_pitch():
    rng = np.random.default_rng(8)
    f0, mel2ph, note = random_item(rng, 900, 60, unvoiced_p=0.0)
    silent, rests = (np.zeros(900, np.float32), mel2ph, note), (f0, mel2ph, np.zeros(60, np.float32))
    odd = rng.choice(np.array([np.nan, np.inf, -np.inf, -220.0, 0.0, -0.0], np.float32), 900)
    mixed = np.where(rng.random(900) < 0.3, odd, f0).astype(np.float32)
    note2 = note.copy()
    note2[::7], note2[3::7], note2[5::7] = np.nan, np.inf, -60.0
    k, out, med, n_corr, _ = check([silent, rests, (odd, mel2ph, note), (mixed, mel2ph, note), (mixed, mel2ph, note2)], window=20)
    assert not k[:3].any() and n_corr[:3].tolist() == [0, 0, 0] and k[3].any() and k[4].any()
    # mel2ph with 0, negative ids and ids above T_ph: frames without a token, which split segments
    check([random_item(rng, 1300, 50, odd_tokens=True) for _ in range(4)], window=9)
    check([random_item(rng, 600, 50, odd_tokens=True)], T_ph=64, fill=(0.0, 0, 61.0), window=1024)      # ids 51 .. 64 now name (pitched) padding tokens


@pytest.mark.parametrize("kw", [dict(octave_fold=True), dict(wild_cents=0.0), dict(wild_cents=16384.0), dict(wild_cents=16384.0, octave_fold=True),
                                dict(wild_cents=30.0)])
def test_octave_fold_and_wild(kw):
    rng = np.random.default_rng(10)
    rows = [random_item(rng, 1100, 90, wild_p=0.2), random_item(rng, 300, 20, wild_p=0.5, spread=4000)]
    rows[1] = (rows[1][0], rows[1][1], np.where(rows[1][2] > 0, 60.0, 0.0).astype(np.float32))
    rows[1][0][::5] = hz_of_units(-14400 + 0 * rows[1][1][::5])                            # every fifth frame exactly on MIDI 60: d = 0, correctable under wild = 0
    k, _, _, n_corr, _ = check(rows, window=30, **kw)
    assert n_corr.sum() > 0


def test_offsets_from_a_device_tensor():
    rng = np.random.default_rng(11)
    f0, mel2ph, note = random_item(rng, 1200, 80, wild_p=0.0)
    up, down = (f0 * 2).astype(np.float32), (f0 / 2).astype(np.float32)
    quarter = np.where(f0 > 0, hz_of_units(np.rint(units_of_hz(np.maximum(f0, 1.0)) - 0.25) + 400), 0).astype(np.float32)
    rows = [(up, mel2ph, note), (down, mel2ph, note), (quarter, mel2ph, note), (f0, mel2ph, note)]
    k, out, med, _, _ = check(rows, offsets=[1200.0, -1200.0, 25.0, 0.0], window=40)
    assert (np.abs(k - k[3]) <= 1).all() and (np.abs(med - med[3]) <= 1).all()           # the offset takes the transposition out again
    check([(up, mel2ph, note), (f0, mel2ph, note)], offsets=[float("nan"), float("inf")], window=40)      # a non-finite offset is 0
    check([(f0, mel2ph, note)], offsets=[3e38], window=40)                                # clamped to 2^22 units: everything is wild


@pytest.mark.parametrize("strength", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("vibrato", [0.0, 1.0, 2.0])
def test_strength_and_vibrato(strength, vibrato):
    rng = np.random.default_rng(12)
    rows = [sung_score(rng)[:3], random_item(rng, 1030, 70)]
    rows[0] = (hz_of_units(np.rint(units_of_hz(rows[0][0]))), rows[0][1], rows[0][2])     # synthetic singing, put on the quarter-unit grid
    k, out, _, _, _ = check(rows, window=25, strength=strength, vibrato=vibrato)
    if strength == 0.0 and vibrato == 1.0:
        assert not k.any()


def test_without_k_out():
    from visinger_amd import guide_correct
    rng = np.random.default_rng(13)
    f0, m2p, note, _ = collate([random_item(rng, TILE + 9, 60), random_item(rng, 800, 60)])
    both = guide_correct.correct_guide(cu(f0), cu(m2p, np.int64), cu(note), return_units=True, window=11)
    alone = guide_correct.correct_guide(cu(f0), cu(m2p, np.int64), cu(note), window=11)
    assert torch.is_tensor(alone) and torch.equal(alone.view(torch.int32), both[0].view(torch.int32)) and both[1].any()


def test_fuzz_batch_of_256():
    rng = np.random.default_rng(256)
    items = []
    for _ in range(256):
        T, T_ph = int(rng.integers(1, 161)), int(rng.integers(1, 13))
        items.append(random_item(rng, T, T_ph, seg=(1, 30), odd_tokens=bool(rng.integers(0, 2))))
    k = check(items, T=160, window=6)[0]
    assert (k != 0).sum() > 5000


def test_the_median_beyond_the_cached_frames():
    """the deviation kernel keeps d of a row's first 12288 frames in LDS and recomputes the rest every step"""
    rng = np.random.default_rng(14)
    f0, mel2ph, note = random_item(rng, 16001, 1000, seg=(12, 40), wild_p=0.0)
    f0[12288:] = hz_of_units(np.rint(units_of_hz(np.maximum(f0[12288:], 1.0))) + 700) * (f0[12288:] > 0)      # the tail sits 700 units higher: it moves the median
    _, _, med, n_corr, _ = check([(f0, mel2ph, note), (f0[:12288], mel2ph[:12288], note)], window=3)
    assert n_corr[0] > n_corr[1] + 1000 and n_corr[1] > 5000 and med[0] > med[1]


def test_an_item_does_not_depend_on_the_launch():
    from visinger_amd import guide_correct
    rng = np.random.default_rng(15)
    item = random_item(rng, 1333, 100)
    alone = check([item], lengths=None, window=50)
    rows = [random_item(rng, 2500, 140), random_item(rng, 100, 30), item]
    f0, m2p, note, lens = collate(rows, T=2600, T_ph=150, fill=(float(hz_of_units(-14400 + 77)), 2, 61.0))
    f0[:, 2500::3] = np.nan
    out, k = guide_correct.correct_guide(cu(f0), cu(m2p, np.int64), cu(note), lengths=torch.tensor(lens, device="cuda"), return_units=True, window=50)
    med, n_corr = guide_correct.guide_deviation(cu(f0), cu(m2p, np.int64), cu(note), lengths=lens)
    assert np.array_equal(k[2, :1333].cpu().numpy(), alone[0][0]) and not k[2, 1333:].any()
    assert np.array_equal(out[2, :1333].cpu().numpy().view(np.uint32), alone[1][0].view(np.uint32))
    assert int(med[2]) == alone[2][0] and int(n_corr[2]) == alone[3][0]


def test_every_einval_through_the_c_abi():
    from visinger_amd import _lib, guide_correct
    L = _lib.require_gpu()
    B, T, T_ph = 2, 48, 9
    rng = np.random.default_rng(16)
    rows = [random_item(rng, T, T_ph, seg=(3, 9)) for _ in range(B)]
    f0, m2p, note = cu(np.stack([r[0] for r in rows])), cu(np.stack([r[1] for r in rows]), np.int64), cu(np.stack([r[2] for r in rows]))
    lens, offs = torch.full((B,), T, dtype=torch.int64, device="cuda"), torch.zeros(B, device="cuda")
    out, k = torch.full((B, T), -7.0, device="cuda"), torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    med, nc = torch.full((B,), -7, dtype=torch.int32, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda")
    before = [t.clone() for t in (f0, m2p, note, lens, offs)]
    vp = lambda t: None if t is None else (t if isinstance(t, ctypes.c_void_p) else ctypes.c_void_p(t.data_ptr()))
    good = dict(f0=f0, lens=lens, m2p=m2p, note=note, offs=offs, window=12, a=256, vq=256, wild=4800, fold=0, reserved=0, out=out, k=k, med=med, nc=nc,
                B=B, T=T, T_ph=T_ph)

    def correct(**kw):
        a = dict(good, **kw)
        return L.vs_guide_correct(vp(a["f0"]), vp(a["lens"]), vp(a["m2p"]), vp(a["note"]), vp(a["offs"]), a["window"], a["a"], a["vq"], a["wild"], a["fold"],
                                  a["reserved"], vp(a["out"]), vp(a["k"]), a["B"], a["T"], a["T_ph"], _lib.stream_ptr())

    def deviation(**kw):
        a = dict(good, **kw)
        return L.vs_guide_deviation(vp(a["f0"]), vp(a["lens"]), vp(a["m2p"]), vp(a["note"]), vp(a["offs"]), a["wild"], a["fold"], vp(a["med"]), vp(a["nc"]),
                                    a["B"], a["T"], a["T_ph"], _lib.stream_ptr())

    inside = ctypes.c_void_p(f0.data_ptr() + 4 * (T + 8))                                 # a buffer that starts inside f0: overlap without equal pointers
    sizes = [dict(B=0), dict(B=-1), dict(T=0), dict(T=65537), dict(T_ph=0), dict(T_ph=1025), dict(wild=-1), dict(wild=(1 << 18) + 1), dict(fold=2), dict(fold=-1)]
    bad = [dict(f0=None), dict(m2p=None), dict(note=None), dict(out=None), dict(out=f0), dict(out=m2p), dict(out=note), dict(out=lens), dict(out=offs),
           dict(out=inside), dict(k=f0), dict(k=m2p), dict(k=note), dict(k=lens), dict(k=offs), dict(k=out), dict(k=inside), dict(window=-1), dict(window=1025),
           dict(a=-1), dict(a=257), dict(vq=-1), dict(vq=513), dict(reserved=1), dict(reserved=-1)] + sizes
    for kw in bad:
        assert correct(**kw) == 1, kw                                           # VS_EINVAL
        assert b"vs_guide_correct" in L.vs_last_error()
    bad = [dict(f0=None), dict(m2p=None), dict(note=None), dict(med=None), dict(nc=None), dict(med=nc), dict(med=f0), dict(nc=m2p), dict(med=note), dict(nc=lens),
           dict(med=offs), dict(nc=inside)] + sizes
    for kw in bad:
        assert deviation(**kw) == 1, kw
        assert b"vs_guide_deviation" in L.vs_last_error()
    torch.cuda.synchronize()
    assert (out == -7).all() and (k == -7).all() and (med == -7).all() and (nc == -7).all()          # nothing was launched
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip((f0, m2p, note, lens, offs), before))
    assert correct() == 0 and deviation() == 0
    torch.cuda.synchronize()
    for b in range(B):
        assert np.array_equal(k[b].cpu().numpy(), correct_ref(*rows[b], window=12)[0])
        assert (int(med[b]), int(nc[b])) == deviation_ref(*rows[b])
    k.fill_(-7)
    assert correct(lens=None, offs=None) == 0 and correct(k=None) == 0 and deviation(lens=None, offs=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(k[0].cpu().numpy(), correct_ref(*rows[0], window=12)[0])
    # the Python entry: ValueError / VisingerHipError before any launch
    for kw in (dict(window=2000), dict(strength=1.5), dict(vibrato=-1), dict(wild_cents=1e6), dict(octave_fold=3), dict(bogus=1), dict(lengths=[T + 1, 0]),
               dict(lengths=[1]), dict(offset_cents=float("inf")), dict(offset_cents=[0.0]), dict(offset_cents="bogus")):
        with pytest.raises(ValueError):
            guide_correct.correct_guide(f0, m2p, note, **kw)
    with pytest.raises(ValueError):
        guide_correct.guide_deviation(f0, m2p, note, offset_cents="auto")
    for args, kw in (((f0.cpu(), m2p, note), {}), ((f0.double(), m2p, note), {}), ((f0, m2p.int(), note), {}), ((f0, m2p[:, :5], note), {}), ((f0, m2p, note[:1]), {}),
                     ((f0, m2p, note.double()), {}), ((f0[0], m2p, note), {}), ((f0, m2p, note), dict(lengths=lens.int())),
                     ((f0, m2p, note), dict(offset_cents=offs.double())), ((f0, m2p.cpu(), note), {})):
        with pytest.raises(_lib.VisingerHipError):
            guide_correct.correct_guide(*args, **kw)
        with pytest.raises(_lib.VisingerHipError):
            guide_correct.guide_deviation(*args, **kw)


def test_graph_replays_on_another_guide():
    from visinger_amd import guide_correct
    rng = np.random.default_rng(18)
    T, T_ph = 2 * TILE + 100, 200
    f0, note = torch.zeros((2, T), device="cuda"), torch.zeros((2, T_ph), device="cuda")
    m2p, lens, offs = torch.zeros((2, T), dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(2, device="cuda")

    def load(rows, cents):
        F0, M, N, n = collate(rows, T, T_ph, fill=(1e3, 1, 60.0))
        f0.copy_(cu(F0)), m2p.copy_(cu(M, np.int64)), note.copy_(cu(N)), lens.copy_(torch.tensor(n, device="cuda")), offs.copy_(cu(cents))

    def run():
        out, k = guide_correct.correct_guide(f0, m2p, note, lengths=lens, offset_cents=offs, return_units=True, window=64)
        return (out, k) + guide_correct.guide_deviation(f0, m2p, note, lengths=lens, offset_cents=offs)

    load([random_item(rng, T, 200), random_item(rng, 300, 60)], [0.0, 0.0])
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
    rows = [random_item(rng, 1500, 150), random_item(rng, T - 7, 200)]
    load(rows, [25.0, -50.0])
    graph.replay()
    eager = run()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, eager)) and not torch.equal(out[1], first)
    for b, r in enumerate(rows):
        assert np.array_equal(out[1][b, :len(r[0])].cpu().numpy(), correct_ref(*r, offset_cents=[25.0, -50.0][b], window=64)[0])
        assert (int(out[2][b]), int(out[3][b])) == deviation_ref(*r, offset_cents=[25.0, -50.0][b])


def test_auto_equals_the_two_explicit_calls():
    from visinger_amd import guide_correct
    rng = np.random.default_rng(19)
    rows = []
    for cents in (-200, 0, 130):
        f0, mel2ph, note = random_item(rng, 1400, 90, wild_p=0.02)
        rows.append((np.where(f0 > 0, hz_of_units(np.rint(units_of_hz(np.maximum(f0, 1.0)) - 0.25) + 16 * cents), 0).astype(np.float32), mel2ph, note))
    f0, m2p, note, lens = collate(rows)
    args = (cu(f0), cu(m2p, np.int64), cu(note))
    auto = guide_correct.correct_guide(*args, lengths=lens, offset_cents="auto", return_units=True, window=33, wild_cents=400.0)
    med, n_corr = guide_correct.guide_deviation(*args, lengths=lens, wild_cents=400.0)
    assert (np.abs(med.cpu().numpy() - 16 * np.array([-200, 0, 130])) < 1500).all() and (n_corr.cpu().numpy() > 700).all()
    explicit = guide_correct.correct_guide(*args, lengths=lens, offset_cents=med.float() / 16, return_units=True, window=33, wild_cents=400.0)
    assert torch.equal(auto[1], explicit[1]) and torch.equal(auto[0].view(torch.int32), explicit[0].view(torch.int32))
    for b, r in enumerate(rows):                                                          # ... which is the restatement under that offset: each guide in its own key
        assert np.array_equal(auto[1][b].cpu().numpy(), correct_ref(*r, offset_cents=np.float32(int(med[b])) / np.float32(16), window=33, wild_cents=400.0)[0])


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------

def detuned_curve(item, rng):
    """a guide on the item's own frames: every note 20 .. 40 cents off, with a vibrato; rests unvoiced"""
    note = item["note_midi"][item["mel2ph"] - 1]
    t = np.arange(len(note))
    cents = 100.0 * (note - 69) + rng.choice([-1, 1], len(item["note_midi"]))[item["mel2ph"] - 1] * rng.uniform(20, 40) + 25 * np.sin(2 * np.pi * t / 18.0)
    return np.where(note > 0, 440.0 * 2.0 ** (cents / 1200.0), 0.0).astype(np.float32)


def test_driver_corrects_before_it_sings(driver):
    from visinger_amd import synth
    m, item, hop, runs, sung, rec = driver
    guided = dict(item, f0=detuned_curve(item, np.random.default_rng(3)))
    before = {k: np.array(v, copy=True) for k, v in guided.items()}
    wav, f0 = synth.synthesize(m, [guided], hop, seeds=7, return_f0=True, guide_correct={})[0]
    assert guided.keys() == before.keys() and all(np.array_equal(guided[k], before[k]) for k in guided)       # the caller's item is not modified
    fixed = synth.correct_items([guided], "cuda")
    assert fixed[0] is not guided and not np.array_equal(fixed[0]["f0"], guided["f0"]) and np.array_equal(fixed[0]["mel2ph"], item["mel2ph"])
    wav2, f02 = synth.synthesize(m, fixed, hop, seeds=7, return_f0=True)[0]
    assert np.array_equal(wav, wav2) and np.array_equal(f0, f02)
    ref_k, ref_out = correct_ref(guided["f0"], item["mel2ph"], item["note_midi"])
    moved = ref_k != 0
    assert moved.sum() > 100 and np.array_equal(fixed[0]["f0"][~moved], guided["f0"][~moved])
    assert np.abs(units_of_hz(fixed[0]["f0"][moved]) - units_of_hz(ref_out[moved])).max() < 2.5       # (a tracked-style curve off the quarter grid: q may round the other way)
    # tempo warps the corrected curve: the chain of the pre-passes, by hand
    fast = synth.synthesize(m, [guided], hop, seeds=7, guide_correct=dict(window=20), tempo=2)[0]
    chain = synth.retime_items(synth.correct_items([guided], "cuda", window=20), 2, "cuda")
    assert np.array_equal(fast, synth.synthesize(m, chain, hop, seeds=7)[0])
    # an item's own offset goes before the call's; "auto" is the item's own median
    low = dict(guided, f0=(guided["f0"] * 2.0 ** (-200.0 / 1200.0)).astype(np.float32))
    own = synth.correct_items([dict(low, guide_offset_cents=-200.0)], "cuda", offset_cents=500.0)[0]["f0"]
    call = synth.correct_items([low], "cuda", offset_cents=-200.0)[0]["f0"]
    auto = synth.correct_items([low], "cuda", offset_cents="auto")[0]["f0"]
    assert np.array_equal(own, call) and np.abs(units_of_hz(auto[moved]) - units_of_hz(call[moved])).max() < 16 * 45
    assert np.abs(units_of_hz(call[moved]) - units_of_hz(fixed[0]["f0"][moved]) + 3200).max() < 3


def test_driver_chained_with_the_alignment_puts_every_segment_on_the_score(driver):
    """the tone-burst recording of the alignment test, tracked, aligned and corrected: wherever the tracker voiced it (and the frame is not wild), the mean of each
    segment's deviation from the score is within 1 unit -- half a unit from q's rounding, half from s's"""
    from visinger_amd import synth
    m, item, hop, runs, sung, rec = driver
    sung_item = dict(item, guide_wav=rec)
    aligned = synth.align_items(synth.guide_items([sung_item], hop, "cuda", fit=False, **TRACK), "cuda")
    fixed = synth.correct_items(aligned, "cuda")
    wav = synth.synthesize(m, [sung_item], hop, guide_track=TRACK, guide_align={}, guide_correct={}, seeds=7)[0]
    assert np.array_equal(wav, synth.synthesize(m, fixed, hop, seeds=7)[0]) and len(wav) == len(aligned[0]["mel2ph"]) * hop
    f0, mel2ph = aligned[0]["f0"], aligned[0]["mel2ph"]
    d, corr, mq, pitched = quantise(f0, mel2ph, item["note_midi"])
    assert corr.sum() > 0.5 * pitched.sum() and not (np.abs(np.abs(d[pitched & (f0 > 0)]) - 4800) <= 2).any()      # (no frame on the edge of wild: the set is the device's)
    dev = units_of_hz(np.where(corr, fixed[0]["f0"], 440.0)) - mq
    edges = np.flatnonzero(np.concatenate(([True], (mq[1:] != mq[:-1]) | (pitched[1:] != pitched[:-1]), [True])))
    worst, segments = 0.0, 0
    for a, e in zip(edges[:-1], edges[1:]):
        if corr[a:e].any():
            worst, segments = max(worst, abs(float(dev[a:e][corr[a:e]].mean()))), segments + 1
    print(f"driver: {segments} segments, {int(corr.sum())} correctable frames of {len(f0)}, worst segment mean {worst:.3f} units off the score")
    assert segments >= 3 and worst <= 1.0


def test_driver_without_guide_correct_nothing_changes(driver):
    from visinger_amd import synth
    m, item, hop, runs, sung, rec = driver
    guided = dict(item, f0=detuned_curve(item, np.random.default_rng(3)))
    plain = synth.synthesize(m, [guided], hop, seeds=7)[0]
    assert np.array_equal(plain, synth.synthesize(m, [guided], hop, seeds=7, guide_correct=None)[0])
    assert not np.array_equal(plain, synth.synthesize(m, [guided], hop, seeds=7, guide_correct={})[0])
    # items without a curve, or without token pitches, pass through the pre-pass
    bare = {k: v for k, v in guided.items() if k != "note_midi"}
    assert np.array_equal(plain, synth.synthesize(m, [bare], hop, seeds=7, guide_correct={})[0])
    none = {k: v for k, v in item.items() if k != "f0"}
    assert np.array_equal(synth.synthesize(m, [none], hop, seeds=7)[0], synth.synthesize(m, [none], hop, seeds=7, guide_correct={})[0])
    for items, kw in (([guided], dict(guide_correct=dict(window=-1))), ([guided], dict(guide_correct=dict(bogus=1))), ([guided], dict(guide_correct=3)),
                      ([dict(guided, f0=guided["f0"][:2])], dict(guide_correct={})), ([dict(guided, note_midi=item["note_midi"][:3])], dict(guide_correct={}))):
        with pytest.raises(ValueError):
            synth.synthesize(m, items, hop, seeds=7, **kw)
