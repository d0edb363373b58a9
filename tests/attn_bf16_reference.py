"""Reference and bound for the plain-bf16 attention core (VS_MATH_BF16: relattn_bf16_kernel<DT, AKT, 1[, true]>, attn_pack_kv_kernel,
relattn_dma_kernel, relattn_combine_kernel), element by element.

The arithmetic restated here, per (item, head), read from csrc/attention_bf16.hip and csrc/attention_dma.hip:
  qs = fl32(q * fl32(1 / sqrt(dk)));  q_r = bf16(qs), k_r = bf16(k), v_r = bf16(v)  (round to nearest even);
  s[j, i] = sum_d k_r[d, j] q_r[d, i]  (+ QR[i, j - i + ws] = sum_d qs[d, i] rel_k[j - i + ws, d] inside the band |j - i| <= ws: the UNROUNDED fp32
  qs and table);  mask[i] * mask[j] == 0 -> s = -1e4;
  streaming softmax over key tiles of `akt` keys, walked in order inside the key range of the workgroup (range ksi of `ksplit` owns the tiles
  [ksi * nt / ksplit, (ksi + 1) * nt / ksplit), nt = ceil(T / akt)): with m_t the running row maximum up to and including the key's own tile,
  p = __expf(s - m_t); the row sum takes the UNROUNDED p, the numerator v_r * bf16(p); both rescaled by __expf(m_old - m_new) in fp32;
  out = O / l + sum_r expf(s[i + r - ws, i] - m) / l * rel_v[r]  (fp32, unrounded);  key split: every range leaves its un-normalised rows, m_k, l_k
  and in-window scores in the partial buffer, relattn_combine_kernel merges them with e^(m_k - m).
A product of two bf16 numbers is exact in fp32: against this reference only the order of the fp32 sums is left -- the fp32-class bound
2e-5 * (1 + |ref|) of bf16_reference.py -- and which way a p close to a bf16 rounding midpoint rounds, which `expected` bounds exactly (`extra`)
instead of loosening the tolerance.  bf16(p) depends on m_t, so the reference follows the kernel's tile width and key ranges.

Everything is numpy fp64 with the rounding points above (oracle.round_bf16 is numpy too); plain helper module: no fixtures, no tests.
"""
import numpy as np

from bf16_reference import EPS32, TOL, assert_close, figures, flagged_fraction, to_np, ulp_bf16  # noqa: F401  (assert_close, flagged_fraction: for the tests)

# A device score (fp32 MFMA sum of exact products, + the fp32 window logit) and the fp64 one here differ by at most F_SCORE * 2^-24 * S, S = the sum
# of the absolute products (the window term's included).  F_SCORE is four times the largest |s_dev - s_ref| / (2^-24 * S) that
# tests/test_attention_bf16_oracle_gpu.py prints for the row maxima and in-window scores the key-split launches leave in their partial buffer,
# rounded up to a power of two.  Measured on an MI355X over the key-split launches of that file: 2.11 (relattn_bf16_kernel<8, 32, 1, true>, dk 256, T 1028,
# three ranges: a row maximum, 256 products per score); the in-window scores, with their fp32 logit of up to 256 more products, reach 1.40.
# 4 * 2.11 = 8.4 -> 16.  (The fp32 BLAS sums of the CPU self-test reach 2.2.)
SCORE_F_MEASURED = 2.11
F_SCORE = 16.0

# p = __expf(x), x = s - m_t <= 0, is __builtin_amdgcn_exp2f(fl32(log2e_f32 * x)) (v_exp_f32: 1 ulp).  In units of 2^-24, relative to p:
#   x = fl32(s - m_t): half an ulp of x, <= |x| * 2^-24 absolute -> |x|;   t = fl32(log2e_f32 * x): |t| * 2^-24 absolute, times ln 2 -> |x|;
#   log2e_f32 = 0x1.715476p+0 is 1.3e-8 = 0.22 * 2^-24 above log2(e) -> 0.22 |x|;   v_exp_f32: one ulp of the result, <= 2^-23 relative -> 2.
# 2.22 |x| + 2 <= E_EXP * (1 + |x|) with E_EXP = 4 (the fp32 np.exp of the CPU self-test stays inside it as well).
E_EXP = 4.0

MASK_FILL = -1e4


def key_ranges(T, akt, ksplit):
    """[(first key, end key)] of the key ranges: whole tiles, [ksi * nt / ksplit, (ksi + 1) * nt / ksplit)"""
    nt = -(-T // akt)
    return [(min(T, (k * nt // ksplit) * akt), min(T, ((k + 1) * nt // ksplit) * akt)) for k in range(ksplit)]


def operands(oracle, q, k, v):
    """-> (qs fp32 [unrounded, scaled], q_r, k_r, v_r as fp64 arrays holding bf16 numbers); q, k, v: [dk, T]"""
    dk = q.shape[0]
    scale = np.float32(1.0) / np.sqrt(np.float32(dk))                  # 1.0f / sqrtf((float)dk)
    qs = np.ascontiguousarray(q, np.float32) * scale
    r = lambda a: oracle.round_bf16(np.ascontiguousarray(a, np.float32)).astype(np.float64)
    return qs, r(qs), r(k), r(v)


def scores(oracle, q, k, v, relk, mask, ws):
    """-> (s [key j, query i], S likewise, v_r): the masked, windowed scores in fp64 and the sums of their absolute products"""
    T = q.shape[1]
    qs, q_r, k_r, v_r = operands(oracle, q, k, v)
    s = k_r.T @ q_r
    S = np.abs(k_r).T @ np.abs(q_r)
    if ws is not None:
        QR = np.asarray(relk, np.float64) @ qs.astype(np.float64)      # [nrel, T]
        QRa = np.abs(np.asarray(relk, np.float64)) @ np.abs(qs.astype(np.float64))
        i = np.arange(T)
        for r in range(2 * ws + 1):
            j = i + r - ws
            ok = (j >= 0) & (j < T)
            s[j[ok], i[ok]] += QR[r, ok]
            S[j[ok], i[ok]] += QRa[r, ok]
    if mask is not None:
        m = np.asarray(mask, np.float64)
        off = (m[:, None] * m[None, :]) == 0
        s[off] = MASK_FILL                                             # (an exact fp32 number: S = 0)
        S[off] = 0.0
    return s, S, v_r


def window(a, ws, lo, hi, fill):
    """[nrel, T]: a[i + r - ws, i] where that key lies in [lo, hi), `fill` elsewhere"""
    T = a.shape[1]
    out = np.full((2 * ws + 1, T), fill, np.float64)
    i = np.arange(T)
    for r in range(2 * ws + 1):
        j = i + r - ws
        ok = (j >= lo) & (j < hi)
        out[r, ok] = a[j[ok], i[ok]]
    return out


def head_expected(oracle, q, k, v, relk, relv, mask, ws, akt, ksplit, F, E):
    """one (item, head): q, k, v [dk, T]; relk, relv [nrel, dk] or None -> (ref [dk, T], extra [dk, T], parts dict of [ksplit, ...] arrays)"""
    dk, T = q.shape
    s, S, v_r = scores(oracle, q, k, v, relk, mask, ws)
    nrel = 0 if ws is None else 2 * ws + 1
    parts = {"m": [], "l": [], "l_margin": [], "Sm": [], "win": [], "Swin": []}
    O, flip, n_marked = [], [], 0
    for lo, hi in key_ranges(T, akt, ksplit):
        sr, Sr = s[lo:hi], S[lo:hi]
        mt, Smt = np.empty_like(sr), np.empty_like(sr)
        m_run, Sm_run = np.full(T, -np.inf), np.zeros(T)
        for j0 in range(0, hi - lo, akt):
            st, St = sr[j0:j0 + akt], Sr[j0:j0 + akt]
            tm, am = st.max(0), st.argmax(0)
            Stm = St[am, np.arange(T)]
            Sm_run = np.where(tm > m_run, Stm, np.where(tm == m_run, np.maximum(Sm_run, Stm), Sm_run))
            m_run = np.maximum(m_run, tm)
            mt[j0:j0 + akt], Smt[j0:j0 + akt] = m_run, Sm_run
        x = sr - mt
        p = np.exp(x)
        relerr = F * EPS32 * (Sr + Smt) + E * EPS32 * (1.0 + np.abs(x))
        u = ulp_bf16(p)
        g = p / np.where(u > 0, u, 1.0)
        marked = (np.abs(g - np.floor(g) - 0.5) * u <= p * relerr) & (p > 0)
        w = np.exp(mt - m_run[None])
        O.append(v_r[:, lo:hi] @ (oracle.round_bf16(p) * w))
        flip.append(np.abs(v_r[:, lo:hi]) @ (np.where(marked, u, 0.0) * w))
        parts["m"].append(m_run)
        parts["l"].append((p * w).sum(0))
        parts["l_margin"].append((p * w * relerr).sum(0))
        # the device's maximum may be the score of another key than here when two lie within their errors of each other: the largest S among those
        near = sr >= m_run[None] - F * EPS32 * (Sr + Sm_run[None])
        parts["Sm"].append(np.where(near, Sr, 0.0).max(0))
        if nrel:
            parts["win"].append(window(s, ws, lo, hi, -np.inf))
            parts["Swin"].append(window(S, ws, lo, hi, 0.0))
        n_marked += int(marked.sum())
    parts = {n: np.stack(a) for n, a in parts.items() if a}
    parts["marked"] = np.int64(n_marked)
    m = parts["m"].max(0)
    a = np.exp(parts["m"] - m[None])                                   # [ksplit, T]
    Lsum = (parts["l"] * a).sum(0)
    ref = sum(o * ak[None] for o, ak in zip(O, a)) / Lsum[None]
    extra = sum(f * ak[None] for f, ak in zip(flip, a)) / Lsum[None]
    if nrel:
        wr = np.exp(parts["win"].max(0) - m[None]) / Lsum[None]        # [nrel, T]; a key belongs to one range, -inf in the others
        ref = ref + np.asarray(relv, np.float64).T @ wr
    return ref, extra, parts


def expected(oracle, qkv, n_heads, rel_k, rel_v, mask, ws, *, akt, ksplit=1, F=None, E=None):
    """qkv [B, 3C, T] (q | k | v), rel_k / rel_v [1 or n_heads, 2 ws + 1, dk] or None, mask [B, T] of 0 / 1 or None, ws = window or None;
    akt = the kernel's key tile (64 for dk <= 128, 32 for wider heads and the DMA kernel), ksplit = its key ranges.
    -> (ref [B, C, T], extra [B, C, T], parts): hold a result to |got - ref| <= 2e-5 * (1 + |ref|) + extra (assert_close).
    extra: a p[i, j] whose distance to a bf16 rounding midpoint is <= p * relerr, relerr = F * 2^-24 * (S[i, j] + S of the element that set m_t) +
    E * 2^-24 * (1 + |s - m_t|) (F_SCORE, E_EXP above), may round to the other neighbour on the device: it is marked and moves the output by at most
    ulp_bf16(p) * e^(m_t - m) * |v_r[d, j]| / L; an unmarked p rounds as it does here.
    parts: [B, n_heads, ksplit, ...] arrays per key range -- m (row maximum), l (row sum, relative to m), l_margin (what the errors of the exponentials'
    arguments may move l by), Sm (the S that bounds m), win / Swin ([.., nrel, T]: the in-window scores, -inf outside the range, and their S); marked
    (count of marked p)."""
    F = F_SCORE if F is None else F
    E = E_EXP if E is None else E
    x = to_np(qkv)
    B, C3, T = x.shape
    C = C3 // 3
    dk = C // n_heads
    rk = None if ws is None else to_np(rel_k).astype(np.float32)
    rv = None if ws is None else to_np(rel_v).astype(np.float32)
    mk = None if mask is None else to_np(mask)
    ref, extra = np.empty((B, C, T)), np.empty((B, C, T))
    parts = {}
    for b in range(B):
        for h in range(n_heads):
            sl = slice(h * dk, (h + 1) * dk)
            hr = 0 if rk is None or rk.shape[0] == 1 else h
            r, e, pt = head_expected(oracle, x[b, sl], x[b, C + h * dk:C + (h + 1) * dk], x[b, 2 * C + h * dk:2 * C + (h + 1) * dk],
                                     None if rk is None else rk[hr], None if rv is None else rv[hr], None if mk is None else mk[b], ws, akt, ksplit, F, E)
            ref[b, sl], extra[b, sl] = r, e
            for n, a in pt.items():
                parts.setdefault(n, []).append(a)
    out = {n: np.stack(a).reshape((B, n_heads) + a[0].shape) for n, a in parts.items()}
    out["marked"] = int(out["marked"].sum())
    return ref, extra, out


def partials(work, B, n_heads, dk, T, nrel, ksplit):
    """the key-split partial buffer [B * n_heads * ksplit][dk + 2 + nrel][T] -> dict of [B, n_heads, ksplit, ...] fp64 arrays: O, m, l, win"""
    rows = dk + 2 + nrel
    w = to_np(work)[:B * n_heads * ksplit * rows * T].reshape(B, n_heads, ksplit, rows, T)
    return {"O": w[:, :, :, :dk], "m": w[:, :, :, dk], "l": w[:, :, :, dk + 1], "win": w[:, :, :, dk + 2:]}


def score_figure(dev, ref, S):
    """largest |s_dev - s_ref| / (2^-24 * S) over the finite scores with S > 0; where S = 0 (masked: the exact -1e4) or the score is -inf the two must be equal"""
    dev, ref, S = np.asarray(dev, np.float64), np.asarray(ref, np.float64), np.asarray(S, np.float64)
    assert dev.shape == ref.shape == S.shape, (dev.shape, ref.shape, S.shape)
    exact = ~np.isfinite(ref) | (S == 0)
    assert np.array_equal(dev[exact], ref[exact]), "masked / out-of-range scores differ"
    ok = ~exact
    return float((np.abs(dev[ok] - ref[ok]) / (EPS32 * S[ok])).max()) if ok.any() else 0.0


def check_partials(got, parts, F=None, what=""):
    """the device's per-range row maxima, in-window scores and row sums (partials()) against the reference's (expected()'s parts):
    m_k and the in-window scores within F * 2^-24 * S, l_k within 2e-5 * l_k + l_margin.  -> the largest |s_dev - s_ref| / (2^-24 * S)"""
    F = F_SCORE if F is None else F
    fm = score_figure(got["m"], parts["m"], parts["Sm"])
    fw = score_figure(got["win"], parts["win"], parts["Swin"]) if "win" in parts else 0.0
    lerr = np.abs(got["l"] - parts["l"])
    lbound = TOL * parts["l"] + parts["l_margin"]
    print(f"ATTNREF {what}: partials score_m {fm:.3f} score_win {fw:.3f} l_of_bound {float((lerr / lbound).max()):.3f}")
    assert fm <= F and fw <= F, f"{what}: device scores off by {max(fm, fw):.2f} * 2^-24 * S, allowed {F}"
    bad = lerr > lbound
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} row sums l_k outside 2e-5 * l_k + the exp margin; worst {float((lerr / lbound).max()):.2f} of the bound"
    return max(fm, fw)


def check(got, ref, extra, parts=None, what=""):
    """bf16_reference.assert_close under the ATTNREF line: element-wise |got - ref| <= 2e-5 * (1 + |ref|) + extra, everything finite.  Prints
    scaled = worst (|err| - extra) / (2e-5 * (1 + |ref|)), of_bound = worst |err| / bound (close to 1 wherever a marked p did flip: that element uses the whole of its
    allowance) and the count of marked p before it asserts.  -> (scaled, of_bound)"""
    bound, err, scaled, _ = figures(got, ref, None, extra)
    of_bound = float((err / bound).max()) if err.size else 0.0
    print(f"ATTNREF {what}: scaled {scaled:.3f} of_bound {of_bound:.3f} marked {'-' if parts is None else parts['marked']}")
    g = to_np(got)
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} non-finite elements"
    bad = err > bound
    if bad.any():
        i = np.unravel_index(int(np.argmax(err / bound)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements above 2e-5 * (1 + |ref|) + extra; worst at {tuple(int(j) for j in i)}: "
                             f"got {g[i]!r}, ref {ref[i]!r}, |err| {err[i]:.3e}, bound {bound[i]:.3e} (extra {np.broadcast_to(extra, err.shape)[i]:.3e})")
    return scaled, of_bound


def inputs(B, n_heads, dk, T, ws, share, unit=True, seed=0):
    """-> (qkv [B, 3C, T], rel_k, rel_v [1 | n_heads, 2 ws + 1, dk] or None, mask [B, T]) as float32 arrays.  Tables of unit variance per element, or
    (unit=False) scaled by dk ** -0.5 like the model's.  Mask: item 0 whole, item 1 cut at ~2/3 (off every tile edge), a third item all padding."""
    r = np.random.default_rng(1000 * dk + 10 * T + n_heads + 7 * (ws or 0) + seed)
    C = dk * n_heads
    qkv = r.standard_normal((B, 3 * C, T)).astype(np.float32)
    rel_k = rel_v = None
    if ws is not None:
        sc = 1.0 if unit else dk ** -0.5
        rel_k = (r.standard_normal((1 if share else n_heads, 2 * ws + 1, dk)) * sc).astype(np.float32)
        rel_v = (r.standard_normal((1 if share else n_heads, 2 * ws + 1, dk)) * sc).astype(np.float32)
    lens = np.asarray([T, max(1, (2 * T) // 3 + (1 if T > 4 else 0)), 0][:B])
    mask = (np.arange(T)[None] < lens[:, None]).astype(np.float32)
    return qkv, rel_k, rel_v, mask
