"""Self-test of the split-f16 attention checker (tests/attn_split3_reference.py) on CPU data alone: what it must accept, what it must flag.
(a) the reference against the live oracle's fp64 attention, at the representation error of the planes: a kept triple h h + l h + h l is the product x y
    to 2^-21 |x y| (each pair of planes holds its number to 2^-23, the dropped l l is at most 2^-22), so the scores agree to 8 * 2^-24 * S and the outputs to
    (8 + 32 max S) * 2^-24 * So -- the numerator's own products, and twice what the score differences of a key and of the row maximum move p by;
(b) the serial fp32 restatement (R.emulate) is inside the bound on EVERY element of EVERY case the GPU file launches -- the condition that lets the GPU
    test compare everything -- and its figures are the ones F_SCORE3 and F_OUT3 are rounded up from;
(c) seeded defects, each confined to the smallest unit the kernel has, on cases that reach them; every line prints the share of the touched, unpadded
    outputs the bound flags, the dropped-term lines also the share above the 2e-5 of tests/test_conv_split_gpu.py::test_split_attention_is_fp32_class.
Findings (what the bound does NOT see, asserted as such so that a change shows):
  * a row sum built from the plane-rounded p moves l by ~2^-25 relative: invisible in the outputs and in l_k, at every shape (the planes hold p to 2^-23;
    the sum of hundreds of such roundings averages out).  Only a bit-exact l would show it.
  * a padded channel read as its clamped neighbour by ONE of K / Q staging changes nothing at all (the other operand's zero fill); the defect seeded
    here is the double misread.
  * a dropped LOW cross product (l h or h l) of one k-step is flagged in the OUTPUTS on 0.64 .. 0.81 of those it touches at dk 32, T 36, on 0.17 .. 0.24 at
    dk 64, T 132, on 0.02 .. 0.10 at dk 96, T 260 and on about 0.01 at dk 128, T 516 -- three to ten times the share the 2e-5 bound flags, and every case
    raises, but far from all: the worst-case allowance for the score errors (F_SCORE3 * 2^-24 * S per key, S ~ sqrt(dk)) and F_OUT3 = 64 of the serial
    chain are the size of the defect (~2^-12 of 16 / T of the row).  In the SCORES it is flagged on 0.91 .. 0.98 at every shape; the device shows its
    scores only in the partial buffer of a key split (row maxima, in-window scores), which is why the GPU file reads it.  The dropped h h term is flagged
    on 0.998 and more of the outputs everywhere.
  * a key range that inherits the previous range's ev loses nothing unless it lies far below it (the planes are floating-point numbers): ramp_down over 3
    ranges is 8 binades and shows nothing; ev_drop (90 binades) flushes the later ranges' V planes -- seen on every partial row of those ranges and on
    none of the merged outputs, to which they contribute nothing measurable."""
import numpy as np
import pytest

import attn_split3_reference as R

f32 = np.float32
_CACHE = {}


def pow2_ceil(x):
    return float(2.0 ** np.ceil(np.log2(x)))


def live_of(mask, shape):
    return np.broadcast_to((mask != 0)[:, None, :], shape)


def serial_figures(case):
    """(score figure, output figure) of the serial fp32 restatement on one GPU case; the whole output and the partial rows inside the bound"""
    name, qkv, nh, rel_k, rel_v, mask, ws, ks = case
    if name not in _CACHE:
        ref, So, extra, parts = R.expected(qkv, nh, rel_k, rel_v, mask, ws, ksplit=ks)
        got, work, sc = R.emulate_batch(qkv, nh, rel_k, rel_v, mask, ws, ks)
        fs = R.score_figure(sc, parts["s"], parts["S"])
        per_s, ofb = R.check(got, ref, So, extra, what=f"serial fp32 {name}")
        B, C, T = ref.shape
        if ks > 1:
            R.check_partials(R.partials(work, B, nh, C // nh, T, 0 if ws is None else 2 * ws + 1, ks), parts, what=f"serial fp32 {name}")
        got_p, _, _ = R.emulate_batch(qkv, nh, rel_k, rel_v, mask, ws, ks, parts=parts)      # the reference's own p: the accumulation alone
        _, _, fo, _ = R.figures(got_p, ref, So, extra)
        print(f"ATTN3REF serial fp32 {name}: score figure {fs:.3f} output figure {fo:.3f} (whole restatement: per_S {per_s:.3f}, {ofb:.3f} of the bound)")
        _CACHE[name] = (fs, fo)
    return _CACHE[name]


CASES = list(R.all_cases())


@pytest.mark.parametrize("n", range(len(CASES)), ids=[c[0].replace(" ", "_") for c in CASES])
def test_the_serial_restatement_is_inside_the_bound(n):
    fs, fo = serial_figures(CASES[n])                                                 # (b): R.check / R.check_partials assert every element
    assert fs <= R.F_SCORE3 and fo <= R.F_OUT3, (fs, fo)


def test_the_constants_are_the_measured_figures_rounded_up():
    figs = [serial_figures(c) for c in CASES]
    fs, fo = max(f[0] for f in figs), max(f[1] for f in figs)
    print(f"ATTN3REF serial fp32, all {len(CASES)} cases: score figure {fs:.3f} (recorded {R.SERIAL_SCORE_MEASURED}, F_SCORE3 {R.F_SCORE3}), "
          f"output figure {fo:.3f} (recorded {R.SERIAL_OUT_MEASURED}, F_OUT3 {R.F_OUT3})")
    assert R.F_SCORE3 == pow2_ceil(R.SERIAL_SCORE_MEASURED) and R.F_OUT3 == pow2_ceil(R.SERIAL_OUT_MEASURED)
    assert fs <= R.F_SCORE3 and fo <= R.F_OUT3
    assert abs(fs - R.SERIAL_SCORE_MEASURED) <= 0.25 * fs and abs(fo - R.SERIAL_OUT_MEASURED) <= 0.25 * fo      # (the exponentials and one BLAS product are the platform's)


@pytest.mark.parametrize("n", range(0, len(R.SHAPE_CASES), 3))
def test_the_reference_is_the_oracles_attention_at_the_planes_precision(oracle, n):
    dk, nh, T, ws, share, B = R.SHAPE_CASES[n]                                        # (a)
    qkv, rel_k, rel_v, mask = R.inputs(B, nh, dk, T, ws, share)
    C = dk * nh
    eye = np.eye(C)
    sel = lambda o: np.concatenate([np.zeros((C, o * C)), eye, np.zeros((C, (2 - o) * C))], 1)[:, :, None]
    sd = {"conv_q.weight": sel(0), "conv_k.weight": sel(1), "conv_v.weight": sel(2), "conv_o.weight": eye[:, :, None],
          "conv_q.bias": np.zeros(C), "conv_k.bias": np.zeros(C), "conv_v.bias": np.zeros(C), "conv_o.bias": np.zeros(C)}
    if ws is not None:
        sd["emb_rel_k"], sd["emb_rel_v"] = rel_k.astype(np.float64), rel_v.astype(np.float64)
    x64 = qkv.astype(np.float64)
    want = oracle.mha_rel(sd, x64, x64, mask, n_heads=nh, window_size=ws)
    ref, So, extra, parts = R.expected(qkv, nh, rel_k, rel_v, mask, ws)
    Smax = np.repeat(parts["S"].max((2, 3)), dk, axis=1)[:, :, None]                  # [B, C, 1]
    tol = R.EPS32 * So * (8.0 + 32.0 * Smax) + 1e-300
    worst = float((np.abs(ref - want) / tol).max())
    print(f"ATTN3REF reference against the fp64 oracle dk{dk} T{T} ws{ws}: {worst:.3f} of the planes' representation error; "
          f"max |diff| {float(np.abs(ref - want).max()):.2e}")
    assert worst <= 1.0, worst
    assert worst > 1e-4, "the planes cost nothing: is this the split arithmetic?"


def _run_defect(inp, nh, ws, defect, ks=1, refs=None):
    qkv, rel_k, rel_v, mask = inp
    ref, So, extra, parts = refs if refs is not None else R.expected(qkv, nh, rel_k, rel_v, mask, ws, ksplit=ks)
    clean = R.emulate_batch(qkv, nh, rel_k, rel_v, mask, ws, ks)
    bad = R.emulate_batch(qkv, nh, rel_k, rel_v, mask, ws, ks, defect=defect)
    live = live_of(mask, ref.shape)
    touched = live & ~(bad[0] == clean[0])
    assert R.flagged_fraction(clean[0], ref, So, extra, live) == 0.0
    f = R.flagged_fraction(bad[0], ref, So, extra, touched)
    old = float((~(np.abs(bad[0] - ref)[touched] <= R.TOL)).mean()) if touched.any() else 0.0
    return f, old, int(touched.sum()), (ref, So, extra, parts), bad, clean


# four shapes from under one tile to 17 tiles, smallest first
DROP_SHAPES = [(32, 36), (64, 132), (96, 260), (128, 516)]
# the least share of the touched outputs a dropped LOW cross product must be flagged on (seen: 0.64 .. 0.81, 0.17 .. 0.24, 0.02 .. 0.10, 0.002 .. 0.013; the
# h h term: 0.998 and more everywhere); the scores themselves are flagged on 0.91 and more at every shape
DROP_FLOOR = {(32, 36): 0.5, (64, 132): 0.1, (96, 260): 0.01, (128, 516): 0.001}


@pytest.mark.parametrize("dk,T", DROP_SHAPES)
def test_a_dropped_cross_product_of_one_k_step_is_flagged(dk, T):
    inp = R.inputs(2, 1, dk, T, 4, True)
    nt = -(-T // R.AKT)
    tile = nt // 2 if nt > 2 else 0
    refs = None
    for where, ks_ in (("drop_s", (dk // 16) // 2), ("drop_o", 1 if tile < nt - 1 else 0)):
        for term in ("lh", "hl", "hh"):
            f, old, n, refs, bad, clean = _run_defect(inp, 1, 4, (where, term, ks_, tile), refs=refs)
            sc = ""
            if where == "drop_s":                                                     # the scores themselves: what the key-split launches show of them (row maxima, window)
                ts = ~(bad[2] == clean[2])
                fsc = float((np.abs(bad[2] - refs[3]["s"])[ts] > R.F_SCORE3 * R.EPS32 * refs[3]["S"][ts]).mean())
                sc = f"; {fsc:.3f} of {int(ts.sum())} touched scores"
                assert fsc >= (0.9 if term == "hh" else 0.5), fsc
            print(f"ATTN3REF self-test dk{dk} T{T}: {where} {term} (k-step {ks_}, tile {tile}) flagged on {f:.3f} of {n} touched outputs{sc}; above 2e-5: {old:.4f}")
            assert n > 0 and f >= (0.99 if term == "hh" else DROP_FLOOR[(dk, T)]), (where, term, f)


def test_moving_scale_defects_are_flagged():
    # a tile's K planes under the previous tile's exponent: needs exponents that differ between neighbours
    inp = R.moving_inputs("ramp_up", 96, 260)
    ek = R.tile_exponents(np.ascontiguousarray(inp[0][0, 96:192]), 260)
    tile = int(np.argmax(np.diff(ek) != 0)) + 1
    assert ek[tile] != ek[tile - 1]
    f, _, n, refs, _, _ = _run_defect(inp, 1, 4, ("k_stale", tile))
    print(f"ATTN3REF self-test ramp_up dk96 T260: K tile {tile} under its neighbour's exponent flagged on {f:.3f} of {n}")
    assert f >= 0.9, f
    f, _, n, _, _, _ = _run_defect(inp, 1, 4, ("no_rescale",), refs=refs)
    print(f"ATTN3REF self-test ramp_up dk96 T260: accumulators not brought down flagged on {f:.3f} of {n}")
    assert f >= 0.9, f
    # a range that inherits ev: the planes are floating-point numbers, so only a range far below its predecessor loses anything (ramp_down over 3 ranges: 8
    # binades, nothing) -- ev_drop, 90 binades: the later ranges' V planes flush to zero.  Their rows are negligible in the merged output: the partial rows show it
    inp = R.moving_inputs("ev_drop", 96, 260)
    f, _, n, refs, bad, clean = _run_defect(inp, 1, 4, ("inherit_ev",), ks=3)
    got, parts = R.partials(bad[1], 2, 1, 96, 260, 9, 3), refs[3]
    with pytest.raises(AssertionError, match="partial rows O_k"):
        R.check_partials(got, parts, what="inherited ev")
    later = np.zeros(parts["O"].shape, bool)
    later[0, :, 1:] = True                                                            # item 0 (no padding), the ranges behind the first
    fo = float((np.abs(got["O"] - parts["O"])[later] > (R.F_OUT3 * R.EPS32 * parts["Oabs"] + parts["dO"])[later]).mean())
    print(f"ATTN3REF self-test ev_drop dk96 T260, 3 ranges: a range inheriting ev flagged on {fo:.3f} of the later ranges' partial rows, {f:.3f} of {n} merged outputs")
    assert fo >= 0.95, fo
    inp = R.moving_inputs("lane_halves", 96, 260)
    f, _, n, _, _, _ = _run_defect(inp, 1, 4, ("eq_half",))
    print(f"ATTN3REF self-test lane_halves dk96 T260: query exponent from one lane half flagged on {f:.3f} of {n}")
    assert f >= 0.45, f                                                               # (every other query: the ones whose largest channel is in the other half)


def test_window_and_padding_defects_are_flagged():
    inp = R.inputs(2, 1, 64, 132, 4, True)
    qkv, rel_k, rel_v, mask = inp
    f, _, n, refs, bad, clean = _run_defect(inp, 1, 4, ("win_slot",))
    # touched: the queries whose band crosses a tile edge, i % 32 in 28 .. 31 and 0 .. 3
    i = np.arange(132)
    crossing = ((i % 32 >= 28) & (i + 4 >= (i // 32 + 1) * 32) & ((i // 32 + 1) * 32 < 132)) | ((i % 32 < 4) & (i >= 32))
    changed = ~(bad[0] == clean[0]).all(1)
    assert not changed[:, ~crossing].any() and changed[0, crossing].all()
    print(f"ATTN3REF self-test dk64 T132: window slot off by one across a tile edge flagged on {f:.3f} of {n}")
    assert f >= 0.9, f
    for dk, T in ((48, 36), (80, 132)):
        f, _, n, _, _, _ = _run_defect(R.inputs(2, 1, dk, T, 4, True), 1, 4, ("pad_clamp",))
        print(f"ATTN3REF self-test dk{dk} T{T}: padded channel read as its neighbour flagged on {f:.3f} of {n}")
        assert f >= 0.9, f


def test_a_row_sum_from_the_rounded_p_is_a_finding():
    """not seen by the output bound, nor by l_k in the partial rows: module docstring"""
    worst = 0.0
    for dk, T, ks in ((32, 36, 1), (96, 260, 3)):
        inp = R.inputs(2, 1, dk, T, 4, True)
        f, _, n, refs, bad, clean = _run_defect(inp, 1, 4, ("l_rounded",), ks=ks)
        rel = 0.0
        if ks > 1:
            got = R.partials(bad[1], 2, 1, dk, T, 9, ks)
            R.check_partials(got, refs[3], what=f"row sum from the rounded p dk{dk} T{T}")      # passes: the finding
            rel = float((np.abs(got["l"] - R.partials(clean[1], 2, 1, dk, T, 9, ks)["l"]) / refs[3]["l"]).max() / R.EPS32)
        print(f"ATTN3REF self-test dk{dk} T{T}: row sum from the plane-rounded p flagged on {f:.4f} of {n}; l_k off by {rel:.2f} * 2^-24 at most -- NOT SEEN")
        worst = max(worst, f)
    assert worst <= 0.01, worst


def test_exponents_ranges_and_flush():
    assert R.key_ranges(260, 32, 4) == [(0, 64), (64, 128), (128, 192), (192, 260)] and R.key_ranges(516, 32, 5)[1] == (96, 192)
    b = R.biased_exponent(np.array([0.0, 1e-45, 2.0 ** -126, 1.0, 1.5, 2.0, 65504.0, 3.4e38], f32))
    assert list(b) == [0, 0, 1, 127, 127, 128, 142, 254], b
    # a value with biased exponent e lands in [2^14, 2^15) under 2^(141 - e): below the f16 maximum
    assert 2.0 ** 14 <= 1.5 * 2.0 ** (141 - 127) < 2.0 ** 15
    # ev_jump: the first tile's contribution is multiplied by 0 on the device and here; the reference says so by leaving it out
    qkv, rel_k, rel_v, mask = R.moving_inputs("ev_jump", 96, 260)
    ref, So, extra, parts = R.expected(qkv, 1, rel_k, rel_v, mask, 4)
    got, _, _ = R.emulate_batch(qkv, 1, rel_k, rel_v, mask, 4)
    R.check(got, ref, So, extra, what="ev_jump, emulation")
    # an all-padding item: every score the exact -1e4, every p exactly 1: the output is the mean of v over the planes
    qkv, rel_k, rel_v, mask = R.inputs(3, 1, 32, 36, None, True)
    ref, So, extra, parts = R.expected(qkv, 1, None, None, mask, None)
    assert np.all(parts["m"][2] == -1e4) and np.all(parts["l"][2] == 36)
    np.testing.assert_allclose(ref[2], np.broadcast_to(qkv[2, 64:].astype(np.float64).mean(1, keepdims=True), (32, 36)), rtol=2e-6, atol=1e-7)
