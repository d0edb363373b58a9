"""The sample-rate converter on the GPU (csrc/resample.hip, visinger_amd/resample.py) and at both ends of the synthesis driver: the kernel against the fp64
restatement ``resample_ref`` of tests/test_resample_cpu.py element by element under the derived summation bound, on the edges of the rule, bit-identical under
another launch shape, past 2^31 in n M, under a graph replay, as ``synthesize(resample_to=)`` and as the guide pre-pass of recordings at another rate."""
import numpy as np
import pytest
import torch

from test_f0_extract_cpu import cents, tone
from test_resample_cpu import design, out_length, resample_ref
from test_timing_gpu import load_tiny_pitch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                    # unit roundoff of fp32


def cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def noise_and_tone(n, seed):
    r = np.random.default_rng(seed)
    return (0.3 * r.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 0.013 * np.arange(n) + r.uniform(0, 6))).astype(np.float32)


def padded(rows, width, fill=1e3):
    host = np.full((len(rows), width), fill, np.float32)
    for b, r in enumerate(rows):
        host[b, :len(r)] = r
    return host


def hold_to_the_bound(y, x, length, sr_in, sr_out, what):
    """every element of the row y within (P + 1) 2^-24 sum |x_i h| of the restatement over its own terms; exact zeros beyond the row; returns the worst ratio"""
    P = design(sr_in, sr_out)[3]
    ref, mass = resample_ref(x, sr_in, sr_out, length=length, n_out=len(y), with_bound=True)
    bound = (P + 1) * U * mass
    err = np.abs(y.astype(np.float64) - ref)
    assert (err <= bound).all(), (what, int(np.argmax(err - bound)), float(err.max()))
    n = min(out_length(length, sr_in, sr_out), len(y))
    assert (y[n:] == 0).all() and np.isfinite(y).all(), what
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{what}: {n} outputs, worst |kernel - fp64| / bound = {worst:.3f}, max error {err.max():.3e}")
    return worst


@pytest.mark.parametrize("sr_in,sr_out", [(1, 2), (2, 1), (2, 3), (80, 147), (147, 80), (147, 160)])
def test_kernel_against_the_restatement(sr_in, sr_out):
    """B = 3 ragged rows of noise plus a tone, lengths on the device, 1e3 beyond each length.  The bar is the standard bound of any fp32 summation order of P
    rounded products, (P + 1) 2^-24 sum |x_i h| over the element's own terms: derived, not measured.  Measured on an MI355X: the worst ratio of an element's
    error to its bound over the six ratios is 0.126 (80 -> 147, row 0; printed per row), the largest error 7.2e-7."""
    from visinger_amd import resample as rs
    lens = [19999, 13337, 7001]
    rows = [noise_and_tone(n, 10 + b) for b, n in enumerate(lens)]
    n_in = 20004
    y, out_lens = rs.resample(cu(padded(rows, n_in)), sr_in, sr_out, lengths=torch.tensor(lens, device="cuda"), return_lengths=True)
    assert y.shape == (3, out_length(n_in, sr_in, sr_out)) and y.dtype == torch.float32
    assert out_lens.dtype == torch.int64 and out_lens.tolist() == [out_length(n, sr_in, sr_out) for n in lens]
    y = y.cpu().numpy()
    for b in range(3):
        hold_to_the_bound(y[b], rows[b], lens[b], sr_in, sr_out, f"{sr_in} -> {sr_out} row {b}")


@pytest.mark.parametrize("sr_in,sr_out,around_a_tile", [(2, 1, (2045, 2047, 2049)), (147, 160, (1175, 1176, 1177)), (1, 2, (511, 512, 513))])
def test_edges_of_the_rule(sr_in, sr_out, around_a_tile):
    """rows of length 0 and 1, one shorter than the filter's reach, output lengths of a tile - 1, a tile and a tile + 1 (as far as the ratio has them), an
    out_len larger than needed (zeros) and a smaller one (the rows are cut; the reported lengths are not)"""
    from visinger_amd import _lib
    from visinger_amd import resample as rs
    TILE = rs.tile(design(sr_in, sr_out)[0])                              # the kernel's tile at this ratio: 1024, 1280, 1024 outputs
    assert TILE == _lib.lib().vs_resample_tile(design(sr_in, sr_out)[0]) == {1: 1024, 160: 1280, 2: 1024}[design(sr_in, sr_out)[0]]
    lens = [0, 1, 5] + list(around_a_tile)
    assert {TILE - 1, TILE, TILE + 1} & {out_length(n, sr_in, sr_out) for n in around_a_tile} and out_length(around_a_tile[1], sr_in, sr_out) == TILE
    rows = [noise_and_tone(n, 20 + b) for b, n in enumerate(lens)]
    x, dl = cu(padded(rows, 2052)), torch.tensor(lens, device="cuda")
    wide, out_lens = rs.resample(x, sr_in, sr_out, lengths=dl, out_len=3 * TILE + 5, return_lengths=True)
    assert wide.shape == (6, 3 * TILE + 5) and out_lens.tolist() == [out_length(n, sr_in, sr_out) for n in lens]
    w = wide.cpu().numpy()
    assert (w[0] == 0).all()
    for b in range(6):
        hold_to_the_bound(w[b], rows[b], lens[b], sr_in, sr_out, f"{sr_in} -> {sr_out} length {lens[b]}")
    for cut in (1000, TILE, 1):
        small, cut_lens = rs.resample(x, sr_in, sr_out, lengths=dl, out_len=cut, return_lengths=True)
        assert small.shape == (6, cut) and torch.equal(small, wide[:, :cut]) and torch.equal(cut_lens, out_lens)
    plain = rs.resample(x, sr_in, sr_out, lengths=lens)                                                                  # host lengths, the default width
    k = min(out_length(2052, sr_in, sr_out), 3 * TILE + 5)
    assert plain.shape == (6, out_length(2052, sr_in, sr_out)) and torch.equal(plain[:, :k], wide[:, :k]) and (plain[:, k:] == 0).all()
    one = rs.resample(x[3], sr_in, sr_out)                                                                               # [n]: one row, every sample valid
    assert one.shape == (out_length(2052, sr_in, sr_out),)


@pytest.mark.parametrize("sr_in,sr_out", [(1, 2), (147, 80), (80, 147)])
def test_an_output_does_not_depend_on_the_launch(sr_in, sr_out):
    """a row alone, as row 2 of 5, under more padding (a width that is no multiple of 4: the element-wise staging), with a larger out_len, and as one of 64 rows
    (whose workgroups walk several tiles each): the same bits"""
    from visinger_amd import resample as rs
    n, TILE = 11000, rs.tile(design(sr_in, sr_out)[0])
    row = noise_and_tone(n, 31)
    alone = rs.resample(cu(row), sr_in, sr_out)
    k = out_length(n, sr_in, sr_out)
    assert alone.shape == (k,) and float(alone.abs().max()) > 0.1
    others = [noise_and_tone(m, 40 + b) for b, m in enumerate((12000, 500, 9000, 11999))]
    five = rs.resample(cu(padded(others[:2] + [row] + others[2:], 12000)), sr_in, sr_out, lengths=[12000, 500, n, 9000, 11999])
    assert torch.equal(five[2, :k], alone) and (five[2, k:] == 0).all()
    odd = rs.resample(cu(padded([row], n + 1237)), sr_in, sr_out, lengths=torch.tensor([n], device="cuda"), out_len=k + 3001)
    assert torch.equal(odd[0, :k], alone) and (odd[0, k:] == 0).all()
    many = rs.resample(cu(padded([row] * 64, n + 2)), sr_in, sr_out, lengths=[n - (b % 3) * 4000 for b in range(64)], out_len=25 * TILE)
    assert torch.equal(many[63, :k], alone) and torch.equal(many[0, :k], alone) and torch.equal(many[1], many[61]) and (many[:, k:] == 0).all()


def test_index_arithmetic_is_64_bit():
    """one row at 44100 -> 24000, 27 M samples made on the device: n M passes 2^31 at output 14.6 M.  The last 4096 outputs against the restatement, evaluated
    there alone: on the input from a multiple of M on (the outputs then shift by a multiple of L)."""
    from visinger_amd import resample as rs
    sr_in, sr_out, n_in = 44100, 24000, 27_000_000
    L, M, W, P, _ = design(sr_in, sr_out)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(n_in, device="cuda", generator=g) * 0.3
    y = rs.resample(x, sr_in, sr_out)
    n_out = out_length(n_in, sr_in, sr_out)
    first = n_out - 4096
    assert y.shape == (n_out,) and first * M > 1 << 31
    k = (first * M - W) // L // M - 1                       # the tail starts at input k M, a whole number of periods before the first term of output `first`
    tail = x[k * M:].cpu().numpy()
    ref, mass = resample_ref(tail, sr_in, sr_out, first=first - k * L, with_bound=True)
    got = y[first:].cpu().numpy().astype(np.float64)
    assert ref.shape == got.shape == (4096,)
    err, bound = np.abs(got - ref), (P + 1) * U * mass
    print(f"outputs {first} .. {n_out - 1}: worst |kernel - fp64| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all() and np.abs(got).max() > 0.1


def test_graph_replays_on_other_samples_and_lengths():
    from visinger_amd import resample as rs
    n, cap = 6000, 2 * rs.tile(80) + 300
    wav, lens = torch.zeros((2, n), device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")

    def load(rows, lengths):
        wav.copy_(cu(padded(rows, n)))
        lens.copy_(torch.tensor(lengths, device="cuda"))

    run = lambda: rs.resample(wav, 44100, 24000, lengths=lens, out_len=cap, return_lengths=True)
    a, b, c = (noise_and_tone(m, 50 + i) for i, m in enumerate((6000, 3500, 4100)))
    load([a, b], [6000, 3500])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, out_lens = run()
    graph.replay()
    first = y.clone()
    load([c, a], [4100, 5999])
    graph.replay()
    eager, eager_lens = run()
    assert torch.equal(y, eager) and torch.equal(out_lens, eager_lens) and not torch.equal(y, first)
    assert out_lens.tolist() == [out_length(4100, 44100, 24000), out_length(5999, 44100, 24000)]
    hold_to_the_bound(y[0].cpu().numpy(), c, 4100, 44100, 24000, "replayed row 0")


def test_every_einval_leaves_the_output_alone():
    """the refusals themselves are tests/test_resample_cpu.py's; here: nothing is launched by a refused call, and the accepted one writes every element"""
    from visinger_amd import _args, _lib
    L = _lib.require_gpu()
    Lr, M, W, P, table = design(24000, 44100)
    x, y, t = torch.ones((2, 4096), device="cuda"), torch.full((2, 8192), -7.0, device="cuda"), cu(table)
    call = lambda **kw: L.vs_resample_poly(*[dict(dict(x=_lib.ptr(x), l=None, B=2, n=4096, t=_lib.ptr(t), L=Lr, M=M, P=P, y=_lib.ptr(y), o=8192, ol=None), **kw)[k]
                                             for k in ("x", "l", "B", "n", "t", "L", "M", "P", "y", "o", "ol")], _lib.stream_ptr())
    for kw in (dict(x=None), dict(B=0), dict(P=64), dict(L=200), dict(M=0), dict(y=_lib.ptr(x)), dict(t=_args.vp(t.view(-1)[1:]))):
        assert call(**kw) == 1 and L.vs_last_error(), kw
    torch.cuda.synchronize()
    assert (y == -7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (y[:, :out_length(4096, 24000, 44100)] != -7).all() and (y[:, out_length(4096, 24000, 44100):] == 0).all()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------

TO_44K = dict(sample_rate=24000, output_rate=44100)


@pytest.fixture(scope="module")
def driver():
    """visinger_tiny_pitch (hop 8) and three items on item 0's tokens: 40, 37 and 12 frames a token"""
    m, a, hp = load_tiny_pitch()
    nph = int((a["text"][0] > 0).sum())
    item = lambda per: dict(text_tokens=a["text"][0][:nph], pitch_tokens=a["pitch"][0][:nph], dur_tokens=a["dur"][0][:nph],
                            mel2ph=np.repeat(np.arange(1, nph + 1), per))
    return m, [item(40), item(37), item(12)], int(np.prod(hp["upsample_rates"])), nph


def converted_alone(w):
    from visinger_amd import resample as rs
    return rs.resample(cu(w), 24000, 44100).cpu().numpy()


@pytest.mark.parametrize("case", ["ragged", "takes", "streams", "graphs"])
def test_driver_converts_the_output(driver, case):
    """synthesize(resample_to = 24000 -> 44100) equals, bit for bit, resample() of each plain waveform taken alone, trimmed to out_length(frames hop)"""
    from visinger_amd import synth
    m, items, hop, nph = driver
    frames = [len(it["mel2ph"]) for it in items]
    kw = dict(ragged=dict(), takes=dict(takes=2), streams=dict(streams=2, max_frames_per_batch=40 * nph), graphs=dict(graphs={}))[case]
    plain = synth.synthesize(m, items, hop, seeds=11, equal_tokens=True, **dict(kw, **(dict(graphs={}) if case == "graphs" else {})))      # the same call without
    for again in range(2 if case == "graphs" else 1):                    # (the second call replays the captured steps)
        out = synth.synthesize(m, items, hop, seeds=11, equal_tokens=True, resample_to=TO_44K, **kw)
        for i, w in enumerate(out):
            want = plain[i]
            assert w.dtype == np.float32 and w.shape[-1] == out_length(frames[i] * hop, 24000, 44100) and w.shape[:-1] == want.shape[:-1]
            for got_take, want_take in zip(np.atleast_2d(w), np.atleast_2d(want)):
                assert np.array_equal(got_take, converted_alone(want_take)), (case, i)
    if case == "ragged":
        wav, f0 = synth.synthesize(m, items[:2], hop, seeds=11, equal_tokens=True, resample_to=dict(TO_44K, zeros=16), return_f0=True)[1]
        assert len(f0) == frames[1] and len(wav) == out_length(frames[1] * hop, 24000, 44100)           # the curve stays per frame
        same = synth.synthesize(m, items, hop, seeds=11, equal_tokens=True, resample_to=dict(sample_rate=24000, output_rate=24000))
        none = synth.synthesize(m, items, hop, seeds=11, equal_tokens=True, resample_to=None)
        assert all(np.array_equal(a, p) and np.array_equal(b, p) for a, b, p in zip(same, none, plain))


TRACK = dict(sample_rate=24000, f0_min=65, f0_max=1000)


def test_driver_tracks_recordings_at_another_rate(driver):
    """recording_rate = 48000: the curve is extract_f0 of the resample()d recording, bit for bit; an item's "guide_sr" goes before it; a steady 220 Hz tone made
    at 44100 Hz tracks within the tracker's steady-tone bar of 1.5 cents; items without either key give the parent's result"""
    from visinger_amd import pitch_track, synth
    from visinger_amd import resample as rs
    m, items, hop, nph = driver
    item, n = items[0], 40 * nph
    r = np.random.default_rng(9)
    rec48, rec48b = (tone(f, k, r, sr=48000)[0].astype(np.float32) for f, k in ((196.0, 2 * n * hop + 11), (330.0, 2 * n * hop - 500)))
    rec44 = tone(220.0, int(n * hop * 44100 / 24000) + 7, r, sr=44100)[0].astype(np.float32)
    rec24 = tone(220.0, n * hop + 3, r)[0].astype(np.float32)

    def alone(rec, rate):
        w = rs.resample(cu(rec), rate, 24000) if rate != 24000 else cu(rec)
        return pitch_track.extract_f0(w, hop, 24000, f0_min=65, f0_max=1000)[0].cpu().numpy()

    sung = [dict(item, guide_wav=rec48), dict(item, guide_wav=rec48b), dict(item, guide_wav=rec44, guide_sr=44100), dict(item, guide_wav=rec24, guide_sr=24000)]
    got = synth.guide_items(sung, hop, "cuda", fit=False, **dict(TRACK, recording_rate=48000))
    for it, rec, rate in zip(got, (rec48, rec48b, rec44, rec24), (48000, 48000, 44100, 24000)):
        want = alone(rec, rate)
        assert "guide_wav" not in it and "guide_sr" not in it and it["f0"].shape == (out_length(len(rec), rate, 24000) // hop,) == want.shape
        assert np.array_equal(it["f0"], want), rate
    assert "guide_sr" in sung[2] and "guide_wav" in sung[2]                                             # the caller's items are not modified
    # the 220 Hz tone made at 44100 Hz: frames whose span (W + tau_max = 1110 samples at 65 Hz) lies inside the converted recording
    f0 = got[2]["f0"]
    lo, hi = -(-(370 + 186) // hop), (out_length(len(rec44), 44100, 24000) - 370 - 186) // hop - 1
    err = cents(f0[lo:hi].astype(np.float64), 220.0).max()
    print(f"a 220 Hz tone made at 44100 Hz, converted and tracked: {err:.3f} cents over {hi - lo} frames")
    assert hi - lo >= 64 and (f0[lo:hi] > 0).all() and err <= 1.5
    # fitted to the item's frames and through synthesize; the item's own rate wins there too
    wav, curve = synth.synthesize(m, [sung[2]], hop, guide_track=dict(TRACK, recording_rate=48000), seeds=7, return_f0=True)[0]
    fitted = synth.guide_items([sung[2]], hop, "cuda", **TRACK)[0]["f0"]
    k = min(n, len(f0))
    assert fitted.shape == (n,) and np.array_equal(fitted[:k], f0[:k]) and len(wav) == n * hop and len(curve) == n
    # without either key: the parent's path (recordings at the model's rate), bit for bit what extract_f0 gives
    old = synth.guide_items([dict(item, guide_wav=rec24)], hop, "cuda", fit=False, **TRACK)[0]["f0"]
    assert np.array_equal(old, alone(rec24, 24000)) and np.array_equal(old, got[3]["f0"])
