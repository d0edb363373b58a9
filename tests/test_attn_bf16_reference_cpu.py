"""Self-test of the plain-bf16 attention checker (tests/attn_bf16_reference.py) on CPU data alone: what it must accept, what it must flag.
The "device" is a numpy float32 emulation of relattn_bf16_kernel<.., 1> / relattn_combine_kernel: bf16-rounded operands, fp32 matmuls, fp32 np.exp, the
tile streaming with its fp32 rescales, the key-split merge.
(a) the emulation passes, with one key range and with three;
(b) seeded defects are flagged on the stated share of the unpadded outputs they touch and assert_close raises: one key dropped from the P V of a middle
    tile, the relative-key slot off by one, the relative-value row off by one, p left unrounded, operands left in fp32, a reference built for other key
    ranges;
(c) the limit of the output check: a row sum taken from the ROUNDED p is not visible in the output at T = 1028 -- check_partials sees it in l_k, which is
    why tests/test_attention_bf16_oracle_gpu.py reads the partial buffer too.
Shares seen with the measured F_SCORE = 16, E_EXP = 4 and unit-variance tables (in brackets: with the provisional F = 32), smallest at dk 256, T 1028, 32-key
tiles: dropped key 0.88 (0.83; >= 0.97 at T <= 260), window slots 0.99 (0.99), unrounded p 0.53 (0.34), fp32 operands 0.79 (0.67), a reference for other key ranges
0.45 (0.28).  The clean emulation leaves (|err| - extra) <= 0.02 of 2e-5 * (1 + |ref|); its scores are within 2.2 * 2^-24 * S of the reference's."""
import numpy as np
import pytest

import attn_bf16_reference as A

# (dk, T, ws, key tile)
SHAPES = [(48, 36, 4, 64), (80, 132, 7, 64), (256, 260, 4, 32), (256, 1028, 4, 32)]
NH, B = 1, 2
f32 = np.float32


def emulate(oracle, qkv, nh, rel_k, rel_v, mask, ws, akt, ksplit=1, *, drop=None, relk_shift=0, relv_shift=0, round_p=True, round_ops=True, l_rounded=False):
    """-> (out [B, C, T], partial buffer [B * nh * ksplit, dk + 2 + nrel, T]) in float32.  Defects: drop = (tile, key in tile) left out of P V;
    relk_shift / relv_shift: the window slot / row taken from its neighbour; round_p / round_ops False: p / q, k, v left in fp32; l_rounded: the row
    sum from the rounded p."""
    Bn, C3, T = qkv.shape
    C = C3 // 3
    dk = C // nh
    nrel = 0 if ws is None else 2 * ws + 1
    rb = (lambda a: oracle.round_bf16(np.ascontiguousarray(a, f32))) if round_ops else (lambda a: np.ascontiguousarray(a, f32))
    out = np.zeros((Bn, C, T), f32)
    part = np.zeros((Bn, nh, ksplit, dk + 2 + nrel, T), f32)
    scale = f32(1.0) / np.sqrt(f32(dk))
    ar = np.arange(T)
    for b in range(Bn):
        for h in range(nh):
            q, k, v = (qkv[b, o * C + h * dk:o * C + (h + 1) * dk] for o in range(3))
            qs = q.astype(f32) * scale
            s = rb(k).T @ rb(qs)                                        # [j, i], fp32 sums
            if nrel:
                rk, rv = rel_k[0 if rel_k.shape[0] == 1 else h], rel_v[0 if rel_v.shape[0] == 1 else h]
                QR = rk @ qs
                for r in range(nrel):
                    j = ar + r - ws
                    ok = (j >= 0) & (j < T)
                    s[j[ok], ar[ok]] += QR[(r + relk_shift) % nrel, ok]
            off = (mask[b][:, None] * mask[b][None, :]) == 0
            s[off] = f32(-1e4)
            v_r = rb(v)
            for ksi, (lo, hi) in enumerate(A.key_ranges(T, akt, ksplit)):
                m, l, O = np.full(T, -np.inf, f32), np.zeros(T, f32), np.zeros((dk, T), f32)
                for t, j0 in enumerate(range(lo, hi, akt)):
                    st = s[j0:min(j0 + akt, hi)]
                    m_new = np.maximum(m, st.max(0))
                    with np.errstate(invalid="ignore"):
                        alpha = np.where(np.isinf(m), f32(0), np.exp(m - m_new)).astype(f32)
                    p = np.exp(st - m_new[None]).astype(f32)
                    pr = oracle.round_bf16(p) if round_p else p
                    l = l * alpha + (pr if l_rounded else p).sum(0, dtype=f32)
                    if drop is not None and j0 // akt == drop[0]:
                        pr = pr.copy()
                        pr[drop[1]] = 0
                    O = O * alpha[None] + v_r[:, j0:j0 + st.shape[0]] @ pr
                    m = m_new
                part[b, h, ksi, :dk], part[b, h, ksi, dk], part[b, h, ksi, dk + 1] = O, m, l
                if nrel:
                    part[b, h, ksi, dk + 2:] = A.window(s, ws, lo, hi, -np.inf).astype(f32)
            pb = part[b, h]
            mm = pb[:, dk].max(0)
            wk = np.exp(pb[:, dk] - mm[None]).astype(f32)
            L = (pb[:, dk + 1] * wk).sum(0, dtype=f32)
            o = (pb[:, :dk] * wk[:, None]).sum(0, dtype=f32) / L[None]
            if nrel:
                wr = (np.exp(pb[:, dk + 2:].max(0) - mm[None]) / L[None]).astype(f32)
                o = o + np.roll(rv, relv_shift, 0).T @ wr
            out[b, h * dk:(h + 1) * dk] = o
    return out, part.reshape(-1)


_CASES = {}
shapes = pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "dk%d_T%d_ws%d_akt%d" % c)


def case_of(oracle, shape):
    """inputs and the references for one and for three key ranges, computed once per shape and left unchanged"""
    if shape not in _CASES:
        dk, T, ws, akt = shape
        qkv, rel_k, rel_v, mask = A.inputs(B, NH, dk, T, ws, True)
        refs = {ks: A.expected(oracle, qkv, NH, rel_k, rel_v, mask, ws, akt=akt, ksplit=ks) for ks in ((1, 3) if T > 2 * akt else (1,))}      # (three ranges need three tiles)
        _CASES[shape] = (shape, (qkv, NH, rel_k, rel_v, mask, ws, akt), refs)
    return _CASES[shape]


@shapes
def test_the_emulation_passes(oracle, shape):
    (dk, T, ws, akt), args, refs = case_of(oracle, shape)
    for ks in refs:                                                                  # (a)
        ref, extra, parts = refs[ks]
        got, work = emulate(oracle, *args, ksplit=ks)
        scaled, of_bound = A.check(got, ref, extra, parts, what=f"emulation dk{dk} T{T} ksplit{ks}")
        assert scaled <= 0.25, scaled       # (of_bound comes close to 1 wherever a marked p did flip: that element uses the whole of its allowance)
        fig = A.check_partials(A.partials(work, B, NH, dk, T, 2 * ws + 1, ks), parts, what=f"emulation dk{dk} T{T} ksplit{ks}")
        assert fig <= A.F_SCORE / 4, fig                                             # (the margin F_SCORE is meant to keep over what is measured)


@shapes
def test_seeded_defects_are_flagged(oracle, shape):
    (dk, T, ws, akt), args, refs = case_of(oracle, shape)
    mask = args[4]
    ref, extra, _ = refs[1]
    live = np.broadcast_to((mask != 0)[:, None, :], ref.shape)                       # the unpadded outputs
    clean, _ = emulate(oracle, *args)
    long_ = T > 260

    def share(bad, where=live, r=refs[1]):
        with pytest.raises(AssertionError, match="elements above"):
            A.assert_close(bad, r[0], r[1], what=f"self-test dk{dk} T{T} seeded defect")
        with pytest.raises(AssertionError, match="elements above"):
            A.check(bad, r[0], r[1], what=f"self-test dk{dk} T{T} seeded defect")
        return A.flagged_fraction(bad, r[0], where, r[1])

    nt = -(-T // akt)
    tile, key = nt // 2 if nt > 2 else 0, 5                                          # (the key is inside item 1's length in every shape)
    bad, _ = emulate(oracle, *args, drop=(tile, key))
    touched = live & (bad != clean)
    f = share(bad, touched)
    print(f"ATTNREF self-test dk{dk} T{T}: dropped key flagged on {f:.3f} of {int(touched.sum())}")
    assert touched[0].mean() > 0.9 and f >= (0.85 if long_ else 0.95), f
    for kw in ({"relk_shift": 1}, {"relv_shift": 1}):
        f = share(emulate(oracle, *args, **kw)[0])
        print(f"ATTNREF self-test dk{dk} T{T}: {kw} flagged on {f:.3f}")
        assert f >= 0.98, (kw, f)
    f = share(emulate(oracle, *args, round_p=False)[0])
    print(f"ATTNREF self-test dk{dk} T{T}: unrounded p flagged on {f:.3f}")
    assert f >= 0.45, f
    f = share(emulate(oracle, *args, round_ops=False)[0])
    print(f"ATTNREF self-test dk{dk} T{T}: fp32 operands flagged on {f:.3f}")
    assert f >= 0.7, f
    if 3 in refs:                                                                    # one key range against the reference for three
        f = share(clean, r=refs[3])
        print(f"ATTNREF self-test dk{dk} T{T}: other key ranges flagged on {f:.3f}")
        assert f >= 0.35, f


def test_a_row_sum_from_the_rounded_p_shows_only_in_the_partials(oracle):
    (dk, T, ws, akt), args, refs = case_of(oracle, SHAPES[-1])                      # (c): T = 1028
    ref, extra, parts = refs[3]
    got, work = emulate(oracle, *args, ksplit=3, l_rounded=True)
    live = np.broadcast_to((args[4] != 0)[:, None, :], ref.shape)
    f = A.flagged_fraction(got, ref, live, extra)
    print(f"ATTNREF self-test dk{dk} T{T}: row sum from the rounded p flagged on {f:.4f} of the outputs")
    assert f <= 0.02, f
    with pytest.raises(AssertionError, match="row sums l_k"):
        A.check_partials(A.partials(work, B, NH, dk, T, 2 * ws + 1, 3), parts, what="row sum from the rounded p")


def test_key_ranges_and_midpoint_marking(oracle):
    assert A.key_ranges(260, 64, 3) == [(0, 64), (64, 192), (192, 260)] and A.key_ranges(1028, 32, 5) == [(0, 192), (192, 416), (416, 608), (608, 832), (832, 1028)]
    assert A.key_ranges(36, 64, 1) == [(0, 36)]
    # an all-padding item: every score is the exact -1e4, every p exactly 1 -- nothing marked, the output is the mean of v_r
    qkv, rel_k, rel_v, mask = A.inputs(3, 1, 32, 36, None, True)
    ref, extra, parts = A.expected(oracle, qkv, 1, None, None, mask, None, akt=64)
    assert not extra[2].any() and np.all(parts["m"][2] == -1e4) and np.all(parts["l"][2] == 36)
    np.testing.assert_allclose(ref[2], np.broadcast_to(oracle.round_bf16(qkv[2, 64:]).astype(np.float64).mean(1, keepdims=True), (32, 36)), rtol=1e-12)
