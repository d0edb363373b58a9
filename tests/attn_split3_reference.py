"""Reference and bound for the split-f16 attention core (VS_MATH_SPLIT3: relattn_bf16_kernel<2 | 3 | 4, 32, 3>, relattn_combine_kernel behind a key
split), element by element, built from the device's own operand planes.

The arithmetic restated here, per (item, head), read from csrc/attention_bf16.hip and csrc/conv_common.h (split_pair_h, f16_maxkey, f16_key_exponent,
f16_scale, F16_EB_MIN):
  planes   an fp32 number x under a power-of-two scale 2^(141 - e) becomes h = f16(x 2^(141 - e)), l = f16(x 2^(141 - e) - h) (round to nearest even, f16
           subnormals kept, the subtraction exact); e is the biased fp32 exponent of the largest FINITE magnitude of the group, floored at F16_EB_MIN = 24;
  query    qs = fl32(q * fl32(1 / sqrt(dk))); query i has its own e: eq[i] from max_d |qs[d, i]| over the head's channels (both lane halves);
  K tile   the 32 keys [32 t, 32 t + 32) inside T share ek[t], from the largest |k| of the tile -- masked keys count, the channels the kernel clamps
           (d >= dk reads d = dk - 1) and the keys it clamps (cells beyond T read the last keys of the sequence, which the last tile holds anyway) change
           nothing, the zero fill of both changes nothing;
  score    raw = sum_d (k_l q_h + k_h q_l + k_h q_h) (products of two f16 numbers are exact in fp32; fp32 MFMA sums, here fp64), times the exact
           2^(ek - 141) 2^(eq - 141); inside the band |j - i| <= ws the window logit sum_d qs[d, i] rel_k[j - i + ws, d] of the UNROUNDED fp32 qs is added;
           mask[i] * mask[j] == 0 -> -1e4;
  softmax  streams over the 32-key tiles of the workgroup's key range (range ksi of `ksplit` owns the tiles [ksi nt / ksplit, (ksi + 1) nt / ksplit)):
           m_t = the running row maximum up to and including the key's own tile, p = exp_nonpos(s - m_t); the row sum takes the UNROUNDED p; the numerator
           the planes of fl32(p * 2^14);
  V tile   planes under ev[t] = the running maximum of the tiles' own exponents from the range's FIRST tile up to and including t (floor 24): when a tile
           raises it the output accumulators are multiplied by the exact 2^(ev_old - ev_new) -- by 0 when that is below 2^-126, restated here;
  output   out = O / l + sum_r expf(win_r - m) / l * rel_v[r]; key split: every range leaves O, m, l and its in-window scores, relattn_combine_kernel
           merges them with expf(m_k - m).
The q, k, v planes are a deterministic function of the fp32 inputs and of those exponents, so device and reference hold the SAME numbers; what is left:
  * the order of the fp32 sums:  |s_dev - s_ref| <= F_SCORE3 * 2^-24 * S,  S = sum of the absolute kept products + the window term's;
    |out_dev - out_ref| <= F_OUT3 * 2^-24 * So + extra,  So = sum_j p_j e^(m_t - m) |v[d, j]| / L + sum_r w_r |rel_v[r, d]|;
  * extra, derived and not fitted -- what the device's p may differ from the reference's by.  The device's unrounded p'_j = p_j (1 + c) (1 + e_j): c, the
    error of the row maximum, is the same for every key and window slot of the row (the partial maxima are fp32 numbers that p, the rescales and the merge
    all use: they cancel) and leaves out = N / D unchanged; |e_j| <= rho_j,
      rho_j = F_SCORE3 * 2^-24 * S[j, i]                                                                            (the score's own error)
            + E_EXP3 * 2^-24 * (1 + |s - m_t| + (m_k - m_t) + the number of later tiles that raised the maximum     (exp_nonpos of p and of every rescale)
                                + [key split: 1 + (m - m_k)])                                                        (the merge's expf)
    the row sum takes p', the numerator planes(p') = p' (1 + 4 * 2^-24) + 2^-38 against the reference's planes(fl32(p)) -- planes(a) holds an fp32 a to
    2^-23 a (h keeps 11 bits, the 13-bit remainder loses at most one bit in l), on the device and here: 4 units, the fp32 rounding of the fp64 p here a
    fifth; 2^-38: a low plane under the f16 subnormal range (|l| < 2^-14 under 2^14: spacing 2^-24 2^-14, half of it on either side).  To first order
      N' - out D' = sum_j p_j e_j (v[d, j] - out[d]) + plane terms + sum_r w_r e_r rel_v[r, d], so
      extra = (sum_j p_j rho_j |v[d, j] - out[d]| + sum_j (5 * 2^-24 p_j + 2^-38) |v[d, j]|) / L / (1 - sum_j p_j rho_j / L) + sum_r w_r rho_r |rel_v[r, d]|
    (a key whose tile the accumulators' flush removed: v = 0; rho_r: the slot's score error and the finish's expf).  The partial rows of a key range are
    relative to the range's own maximum, where c does NOT cancel: relerr = rho + F_SCORE3 * 2^-24 * (S of the element that set the maximum), l_margin =
    sum p relerr, dO = sum (p (relerr + 5 * 2^-24) + 2^-38) |v|.
E_EXP3, from exp_nonpos's code: t = fl32(x c1), e = fma(x, c2, fma(x, c1, -t)) is x log2(e) - t to 2^-48 |t| (c1 + c2 = log2 e to 2^-50), y = v_exp_f32(t)
(1 ulp: 2 units of 2^-24), the result fma(y, e ln2, y) rounds once (1 unit) and drops (e ln 2)^2 / 2 <= 2^-33; the argument x = fl32(s - m) or one fma carries
half an ulp of x: |x| units relative to p.  3.01 + |x| <= E_EXP3 * (1 + |x|) with E_EXP3 = 4; expf of the finish and of the merge is inside it too.

Neither F is taken from the kernels.  `emulate` is the serial fp32 restatement: the same planes, the same tile walk, fp32 accumulators, every score ONE
chain of 3 dk roundings (per 16-channel k-step h h first, then l h, h l: the small terms meet the largest partial sums), every output one chain of 3 * 32
roundings per tile.  SERIAL_SCORE_MEASURED / SERIAL_OUT_MEASURED are its largest errors against the fp64 sums of the same planes in units of 2^-24 S and
2^-24 So (the output figure with the reference's own p, so that only the accumulation is left), over every case of tests/test_attention_split3_oracle_gpu.py,
computed on the CPU (tests/test_attn_split3_reference_cpu.py recomputes them); the constants are those figures rounded up to a power of two.

VS_MATH_SPLIT6 (three bf16 planes, an exact split of an fp32 number; the same tiles, exponential and tile walk): `exact=True` takes the unsplit fp32
operands and the unsplit fl32(p).  The kernel drops the cross products m l, l m and l l of the nine: |m| <= 2^-8 |x|, |l| <= 2^-16 |x|, so a dropped
triple is at most (2^-24 + 2^-24 + 2^-32) |a b|: DROP6 = 2 + 2^-8 more units of 2^-24 S / 2^-24 So on both F.

Measured on an MI355X, the largest |got - ref| / (2^-24 So) the 63 launches of tests/test_attention_split3_oracle_gpu.py printed, by instance:
relattn_bf16_kernel<2, 32, 3> 30.1 (three key ranges on outlier keys), <3, 32, 3> 49.4 (channel gains), <4, 32, 3> 42.7 (outlier keys); on unit data 3.5 .. 11.6;
never above 0.16 of the bound.  The scores the partial buffer shows: 2.63 (row maxima) and 1.99 (in-window) of 2^-24 S; l_k 0.056 and the rows O_k 0.069 of
their bounds; <2 | 3 | 4, 32, 6>: 6.6 / 6.3 / 9.5.  None of these figures enters a bound.

Plain helper module (like attn_bf16_reference.py): no fixtures, no tests.  split_f16 is split3_reference's; key_ranges, window, partials, score_figure and
inputs are attn_bf16_reference's.
"""
import numpy as np

from attn_bf16_reference import MASK_FILL, inputs, key_ranges, partials, score_figure, window  # noqa: F401  (re-exported for the tests)
from bf16_reference import to_np
from split3_reference import EPS32, TOL, split_f16

f32, f64 = np.float32, np.float64
AKT = 32                         # keys per tile of every split instance
EB_MIN = 24                      # conv_common.h F16_EB_MIN
P_EXP = 14                       # the probabilities' fixed scale 2^14

SERIAL_SCORE_MEASURED = 12.70    # the largest |serial fp32 score - fp64 score| / (2^-24 S) over the GPU file's cases (ksplit5 unit dk128 T516; median case 8.4)
F_SCORE3 = 16.0                  # ... rounded up to a power of two
SERIAL_OUT_MEASURED = 42.43      # the largest |serial fp32 output - fp64 output| / (2^-24 So), the reference's own p (outlier_keys dk128 T516: one key carries the
F_OUT3 = 64.0                    # row and ~1500 small terms are rounded against it; unit data 2.9 .. 13.7); rounded up to a power of two
E_EXP3 = 4.0
DROP6 = 2.0 + 2.0 ** -8


# ---------------------------------------------------------------------------------------------------------------- exponents and planes
def biased_exponent(m):
    """f16_key_exponent(f16_maxkey(..)) of a largest magnitude m >= 0 (fp32): its biased exponent, 0 for zero and the fp32 subnormals"""
    m = np.asarray(m, f32)
    e = np.frexp(m)[1].astype(np.int64) + 126                      # m = f 2^e, f in [0.5, 1): floor(log2 m) = e - 1
    return np.where(m > 0, np.maximum(e, 0), 0)


def _scaled_planes(x32, e, exact):
    """planes of x32 under 2^(141 - e) (e broadcastable) -> (h, l) float64 in scaled units; exact: (x, 0)"""
    if exact:
        return x32.astype(f64), np.zeros(x32.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        return split_f16(x32 * np.ldexp(1.0, 141 - np.asarray(e)).astype(f32), 1.0)


def tile_exponents(x32, T):
    """[nt]: max(biased exponent of the largest |x32[:, tile]|, 24) per 32-key tile"""
    return np.array([max(int(biased_exponent(np.abs(x32[:, j0:j0 + AKT]).max(initial=0.0))), EB_MIN) for j0 in range(0, T, AKT)], np.int64)


class Operands:
    """qs [dk, T] fp32; eq [T]; qh, ql [dk, T]; ek [nt], ekj [T] (per key); kh, kl [dk, T]; v32; evt [nt]: the V tiles' own exponents"""

    def __init__(self, q, k, v, *, exact=False, eq_half=False, k_stale=None):
        dk, T = q.shape
        self.dk, self.T, self.exact = dk, T, exact
        scale = f32(1.0) / np.sqrt(f32(dk))                            # 1.0f / sqrtf((float)dk)
        self.qs = np.ascontiguousarray(q, f32) * scale
        self.k32, self.v32 = np.ascontiguousarray(k, f32), np.ascontiguousarray(v, f32)
        src = self.qs[(np.arange(dk) & 8) == 0] if eq_half else self.qs      # (defect: one lane half's channels only)
        self.eq = np.full(T, 141, np.int64) if exact else np.maximum(biased_exponent(np.abs(src).max(0)), EB_MIN)
        self.qh, self.ql = _scaled_planes(self.qs, self.eq[None], exact)
        nt = -(-T // AKT)
        self.ek = np.full(nt, 141, np.int64) if exact else tile_exponents(self.k32, T)
        self.evt = np.full(nt, 141, np.int64) if exact else tile_exponents(self.v32, T)
        self.ekj = np.repeat(self.ek, AKT)[:T]
        ekp = self.ekj.copy()
        if k_stale is not None:                                        # (defect: this tile's planes made under the previous tile's exponent)
            ekp[k_stale * AKT:(k_stale + 1) * AKT] = self.ek[k_stale - 1]
        self.kh, self.kl = _scaled_planes(self.k32, ekp[None], exact)

    def sfix(self):
        """[key j, query i] 2^(ek - 141) 2^(eq - 141), exact in fp64"""
        return np.ldexp(1.0, self.ekj - 141)[:, None] * np.ldexp(1.0, self.eq - 141)[None]


def _band(T, ws):
    """[(r, queries i, keys j = i + r - ws)] inside the sequence"""
    i = np.arange(T)
    out = []
    for r in range(2 * ws + 1):
        j = i + r - ws
        ok = (j >= 0) & (j < T)
        out.append((r, i[ok], j[ok]))
    return out


def scores(op, relk, mask, ws):
    """-> (s [key j, query i], S likewise): the masked, windowed scores in fp64 from the planes and the sums of their absolute products"""
    fix = op.sfix()
    s = (op.kl.T @ op.qh + op.kh.T @ op.ql + op.kh.T @ op.qh) * fix
    a = np.abs
    S = (a(op.kl).T @ a(op.qh) + a(op.kh).T @ a(op.ql) + a(op.kh).T @ a(op.qh)) * fix
    if ws is not None:
        QR = np.asarray(relk, f64) @ op.qs.astype(f64)                 # [nrel, T]
        QRa = a(np.asarray(relk, f64)) @ a(op.qs.astype(f64))
        for r, i, j in _band(op.T, ws):
            s[j, i] += QR[r, i]
            S[j, i] += QRa[r, i]
    if mask is not None:
        m = np.asarray(mask, f64)
        off = (m[:, None] * m[None, :]) == 0
        s[off] = MASK_FILL                                             # (an exact fp32 number: S = 0)
        S[off] = 0.0
    return s, S


# ---------------------------------------------------------------------------------------------------------------- the reference
def head_expected(q, k, v, relk, relv, mask, ws, ksplit, F, E, exact=False):
    """one (item, head): q, k, v [dk, T]; relk, relv [nrel, dk] or None -> (ref, So, extra [dk, T], parts dict of [ksplit, ...] arrays, s, S)"""
    dk, T = q.shape
    op = Operands(q, k, v, exact=exact)
    s, S = scores(op, relk, mask, ws)
    nrel = 0 if ws is None else 2 * ws + 1
    av = np.abs(op.v32.astype(f64))
    parts = {n: [] for n in ("O", "Oabs", "dO", "m", "l", "l_margin", "Sm", "win", "Swin")}
    ar = np.arange(T)
    terms = []                                                         # per range, per tile: what the allowance needs once the output is known
    for lo, hi in key_ranges(T, AKT, ksplit):
        terms.append([])
        tiles = list(range(lo, hi, AKT))
        # first pass: the running maxima, the S of the element that set them, how often a later tile raises them
        mt, m_run, Sm_run = [], np.full(T, -np.inf), np.zeros(T)
        raised = []
        for j0 in tiles:
            st, St = s[j0:min(j0 + AKT, hi)], S[j0:min(j0 + AKT, hi)]
            tm, am = st.max(0), st.argmax(0)
            Stm = St[am, ar]
            Sm_run = np.where(tm > m_run, Stm, np.where(tm == m_run, np.maximum(Sm_run, Stm), Sm_run))
            raised.append(tm > m_run)
            m_run = np.maximum(m_run, tm)
            mt.append(m_run)
        later = np.zeros(T)
        n_later = [None] * len(tiles)
        for t in range(len(tiles) - 1, -1, -1):
            n_later[t] = later.copy()
            later = later + raised[t]
        O, Oabs, dO = np.zeros((dk, T)), np.zeros((dk, T)), np.zeros((dk, T))
        l, lm = np.zeros(T), np.zeros(T)
        ev = EB_MIN
        for t, j0 in enumerate(tiles):
            j1 = min(j0 + AKT, hi)
            x = s[j0:j1] - mt[t][None]
            p = np.exp(x)
            w = np.exp(mt[t] - m_run)                                  # e^(m_t - m), [T]
            rho = F * EPS32 * S[j0:j1] + E * EPS32 * (1.0 + np.abs(x) + (m_run - mt[t])[None] + n_later[t][None])
            relerr = rho + F * EPS32 * Sm_run[None]
            ev_new = max(ev, int(op.evt[j0 // AKT]))
            if t and ev_new - ev > 126:                                # the accumulators are multiplied by 0
                O[:], Oabs[:], dO[:] = 0.0, 0.0, 0.0
                for e_ in terms[-1]:
                    e_[4] = True
            ev = ev_new
            vh, vl = _scaled_planes(op.v32[:, j0:j1], ev, exact)
            p32 = p.astype(f32)
            ph, pl = (p32.astype(f64), np.zeros(p.shape)) if exact else split_f16(p32, 2.0 ** P_EXP)
            unscale = 1.0 if exact else np.ldexp(1.0, ev - 141 - P_EXP)
            O += ((vl @ ph + vh @ pl + vh @ ph) * unscale) * w[None]
            Oabs += av[:, j0:j1] @ (p * w[None])
            dO += av[:, j0:j1] @ ((p * (relerr + 5 * EPS32) + 2.0 ** -38) * w[None])
            l += (p * w[None]).sum(0)
            lm += (p * w[None] * relerr).sum(0)
            terms[-1].append([j0, j1, p * w[None], rho, False, w])
        parts["O"].append(O), parts["Oabs"].append(Oabs), parts["dO"].append(dO)
        parts["m"].append(m_run), parts["l"].append(l), parts["l_margin"].append(lm)
        # the device's maximum may be the score of another key than here when two lie within their errors of each other: the largest S among those
        near = s[lo:hi] >= m_run[None] - F * EPS32 * (S[lo:hi] + Sm_run[None])
        parts["Sm"].append(np.where(near, S[lo:hi], 0.0).max(0))
        if nrel:
            parts["win"].append(window(s, ws, lo, hi, -np.inf))
            parts["Swin"].append(window(S, ws, lo, hi, 0.0))
    parts = {n: np.stack(a_) for n, a_ in parts.items() if a_}
    m = parts["m"].max(0)
    a = np.exp(parts["m"] - m[None])                                   # [ksplit, T]
    rk = np.where(parts["m"] == m[None], 0.0, E * EPS32 * (1.0 + (m[None] - parts["m"]))) if ksplit > 1 else np.zeros_like(a)      # the merge's expf(m_k - m); expf(0) = 1
    L = (parts["l"] * a).sum(0)
    ref = (parts["O"] * a[:, None]).sum(0) / L[None]
    So = (parts["Oabs"] * a[:, None]).sum(0) / L[None]
    if nrel:
        win, Swin = parts["win"].max(0), parts["Swin"].max(0)          # a key belongs to one range, -inf / 0 in the others
        wr = np.exp(win - m[None]) / L[None]                           # [nrel, T]
        rv = np.asarray(relv, f64)
        ref = ref + rv.T @ wr
        So = So + np.abs(rv).T @ wr
    # the allowance (module docstring), with the finished output
    PR, PL, veff = np.zeros((T, T)), np.zeros((T, T)), op.v32.astype(f64)       # [key, query]: p rho and the planes' term; v with the flushed tiles at 0
    for k_, tl in enumerate(terms):
        for j0, j1, pw, rho, flushed, w in tl:
            PR[j0:j1] = pw * (rho + rk[k_][None]) * a[k_][None]
            if flushed:
                veff[:, j0:j1] = 0.0
            else:
                PL[j0:j1] = (5 * EPS32 * pw + 2.0 ** -38 * w[None]) * a[k_][None]
    num = av @ PL
    for d in range(dk):
        num[d] += (np.abs(veff[d][:, None] - ref[d][None, :]) * PR).sum(0)
    lrel = PR.sum(0)
    lrel = lrel / L
    extra = num / L[None] / (1.0 - np.minimum(lrel, 0.5))[None]
    if nrel:
        with np.errstate(invalid="ignore"):
            xr = np.where(np.isfinite(win), m[None] - win, 0.0)
        extra = extra + np.abs(rv).T @ (wr * (F * EPS32 * Swin + E * EPS32 * (1.0 + xr)))
    return ref, So, extra, parts, s, S


def expected(qkv, n_heads, rel_k, rel_v, mask, ws, *, ksplit=1, F=None, E=None, exact=False):
    """qkv [B, 3C, T] (q | k | v), rel_k / rel_v [1 or n_heads, 2 ws + 1, dk] or None, mask [B, T] of 0 / 1 or None, ws = window or None, ksplit = the
    launch's key ranges; exact: the VS_MATH_SPLIT6 form (module docstring).
    -> (ref, So, extra [B, C, T], parts): hold a result to |got - ref| <= F_OUT3 * 2^-24 * So + extra (check).
    parts: [B, n_heads, ksplit, ...] arrays per key range -- O, Oabs, dO ([.., dk, T]: the un-normalised rows relative to the range's maximum, their sums of
    absolute terms and their allowance), m, l, l_margin, Sm, win / Swin ([.., nrel, T]); s, S [B, n_heads, T, T]: the scores and their absolute sums."""
    F = F_SCORE3 if F is None else F
    E = E_EXP3 if E is None else E
    x = to_np(qkv)
    B, C3, T = x.shape
    C = C3 // 3
    dk = C // n_heads
    rk = None if ws is None else to_np(rel_k).astype(f32)
    rv = None if ws is None else to_np(rel_v).astype(f32)
    mk = None if mask is None else to_np(mask)
    ref, So, extra = np.empty((B, C, T)), np.empty((B, C, T)), np.empty((B, C, T))
    parts = {}
    for b in range(B):
        for h in range(n_heads):
            sl = slice(h * dk, (h + 1) * dk)
            hr = 0 if rk is None or rk.shape[0] == 1 else h
            r, so, e, pt, s, S = head_expected(x[b, sl], x[b, C + h * dk:C + (h + 1) * dk], x[b, 2 * C + h * dk:2 * C + (h + 1) * dk],
                                               None if rk is None else rk[hr], None if rv is None else rv[hr], None if mk is None else mk[b], ws, ksplit, F, E, exact)
            ref[b, sl], So[b, sl], extra[b, sl] = r, so, e
            pt = dict(pt, s=s, S=S)
            for n, a in pt.items():
                parts.setdefault(n, []).append(a)
    return ref, So, extra, {n: np.stack(a).reshape((B, n_heads) + a[0].shape) for n, a in parts.items()}


# ---------------------------------------------------------------------------------------------------------------- the checks
def out_bound(So, extra, F=None):
    return (F_OUT3 if F is None else F) * EPS32 * So + extra


def figures(got, ref, So, extra, F=None):
    """-> (err, bound, per_S = worst |err| / (2^-24 So) over So > 0, of_bound = worst |err| / bound [inf where an element with bound 0 differs])"""
    g = to_np(got)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    err = np.abs(g - ref)
    bound = out_bound(So, extra, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_s = np.where(So > 0, err / (EPS32 * np.where(So > 0, So, 1.0)), 0.0)
        ofb = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return err, bound, float(np.nanmax(per_s)) if err.size else 0.0, float(np.nanmax(ofb)) if err.size else 0.0


def check(got, ref, So, extra, what="", F=None):
    """Element-wise over ALL elements: |got - ref| <= F_OUT3 * 2^-24 * So + extra, everything finite.  Prints the ATTN3REF line before it asserts.
    -> (per_S, of_bound)"""
    err, bound, per_s, ofb = figures(got, ref, So, extra, F)
    print(f"ATTN3REF {what}: per_S {per_s:.3f} of_bound {ofb:.3f}")
    g = to_np(got)
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} non-finite elements"
    bad = err > bound
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0.0))), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements above the bound; worst at {tuple(int(j) for j in i)}: "
                             f"got {g[i]!r}, ref {ref[i]!r}, |err| {err[i]:.3e}, bound {bound[i]:.3e} (extra {extra[i]:.3e})")
    return per_s, ofb


def flagged_fraction(got, ref, So, extra, where, F=None):
    """share of the elements selected by `where` that check would flag (a non-finite element counts as flagged)"""
    err, bound, _, _ = figures(got, ref, So, extra, F)
    return float((~(err[where] <= bound[where])).mean()) if where.any() else 0.0


def check_partials(got, parts, what="", F=None, F_out=None):
    """the device's per-range rows (partials()) against the reference's (expected()'s parts): m_k and the in-window scores within F_SCORE3 * 2^-24 * S,
    l_k within F_OUT3 * 2^-24 * l_k (its fp32 sum: every term positive, So = l_k) + l_margin, the rows O_k within F_OUT3 * 2^-24 * Oabs_k + dO_k.
    -> the largest |s_dev - s_ref| / (2^-24 * S)"""
    F = F_SCORE3 if F is None else F
    Fo = F_OUT3 if F_out is None else F_out
    fm = score_figure(got["m"], parts["m"], parts["Sm"])
    fw = score_figure(got["win"], parts["win"], parts["Swin"]) if "win" in parts else 0.0
    lerr = np.abs(got["l"] - parts["l"])
    lbound = Fo * EPS32 * parts["l"] + parts["l_margin"]
    oerr = np.abs(got["O"] - parts["O"])
    obound = Fo * EPS32 * parts["Oabs"] + parts["dO"]
    with np.errstate(divide="ignore", invalid="ignore"):
        o_of = float(np.nanmax(np.where(obound > 0, oerr / np.where(obound > 0, obound, 1.0), np.where(oerr > 0, np.inf, 0.0))))
    print(f"ATTN3REF {what}: partials score_m {fm:.3f} score_win {fw:.3f} l_of_bound {float((lerr / lbound).max()):.3f} O_of_bound {o_of:.3f}")
    assert fm <= F and fw <= F, f"{what}: device scores off by {max(fm, fw):.2f} * 2^-24 * S, allowed {F}"
    bad = lerr > lbound
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} row sums l_k outside their margin; worst {float((lerr / lbound).max()):.2f} of the bound"
    bad = ~(oerr <= obound)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} partial rows O_k above the bound; worst {o_of:.2f} of it"
    return max(fm, fw)


# ---------------------------------------------------------------------------------------------------------------- the serial fp32 restatement, with seeded defects
def emulate(q, k, v, relk, relv, mask, ws, ksplit=1, *, defect=None, s_exact=None):
    """One (item, head) in float32 (module docstring): -> (out [dk, T], partial rows [ksplit, dk + 2 + nrel, T], scores s [key, query]), all float32.
    s_exact: fp64 scores to take INSTEAD of the fp32 chains, with the softmax in fp64 up to the fp32 p -- the planes of p are then the reference's and only
    the fp32 accumulation of V P^T, the rescales and the finish are left (SERIAL_OUT_MEASURED).
    defect: None or
      ("drop_s", term, ks, tile)  -- term "lh" (k_l q_h) / "hl" (k_h q_l) / "hh": that cross product of the 16-channel k-step ks of that key tile of K^T Q is not taken;
      ("drop_o", term, s4, tile)  -- the same in the 16-key k-step s4 of that tile of V P^T (term: v_l p_h / v_h p_l / v_h p_h);
      ("k_stale", tile)           -- that tile's K planes are made under the PREVIOUS tile's exponent, the scores unscaled by its own;
      ("no_rescale",)             -- the output accumulators are not brought down when ev rises;
      ("inherit_ev",)             -- a key range starts from the previous range's ev instead of the floor;
      ("eq_half",)                -- the query exponent from the channels with (d & 8) == 0 only: one lane half's;
      ("win_slot",)               -- the window logit of the neighbouring slot, where key and query lie in different 32-key tiles;
      ("l_rounded",)              -- the row sum from the plane-rounded p;
      ("pad_clamp",)              -- the first padded channel (d = dk, dk % 32 != 0) read as its clamped neighbour dk - 1 by BOTH the K and the Q staging
                                     (either alone meets the other's zero and changes nothing)."""
    kind = defect[0] if defect else None
    dk, T = q.shape
    op = Operands(q, k, v, eq_half=kind == "eq_half", k_stale=defect[1] if kind == "k_stale" else None)
    nrel = 0 if ws is None else 2 * ws + 1
    F = lambda a_: np.ascontiguousarray(a_, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        kh, kl, qh, ql = F(op.kh), F(op.kl), F(op.qh), F(op.ql)
    if s_exact is None:
        raw = np.zeros((T, T), f32)
        with np.errstate(over="ignore", invalid="ignore"):
            for ks in range(-(-dk // 16)):
                for term, a_, b_ in (("hh", kh, qh), ("lh", kl, qh), ("hl", kh, ql)):
                    cut = kind == "drop_s" and defect[1:3] == (term, ks)
                    for d in range(16 * ks, min(16 * ks + 16, dk)):
                        prod = a_[d][:, None] * b_[d][None, :]                 # (a product of two f16 numbers: exact in fp32)
                        if cut:
                            prod[defect[3] * AKT:(defect[3] + 1) * AKT] = 0
                        raw += prod
            if kind == "pad_clamp" and dk % 32:
                for a_, b_ in ((kh, qh), (kl, qh), (kh, ql)):
                    raw += a_[dk - 1][:, None] * b_[dk - 1][None, :]
            s = raw * (np.ldexp(1.0, op.ekj - 141).astype(f32)[:, None] * np.ldexp(1.0, op.eq - 141).astype(f32)[None])
        if nrel:
            QR = F(relk) @ op.qs                                               # [nrel, T] fp32
            for r, i, j in _band(T, ws):
                if kind == "win_slot":
                    rr = np.where(j // AKT != i // AKT, (r + 1) % nrel, r)
                    s[j, i] += QR[rr, i]
                else:
                    s[j, i] += QR[r, i]
        if mask is not None:
            mk = np.asarray(mask, f32)
            s[(mk[:, None] * mk[None, :]) == 0] = f32(MASK_FILL)
        xd = f32
    else:
        s, xd = np.asarray(s_exact, f64), f64
    part = np.zeros((ksplit, dk + 2 + nrel, T), xd)                    # (s_exact: m and the in-window scores stay fp64 -- on the device they ARE fp32 numbers)
    ev_end = EB_MIN
    for ksi, (lo, hi) in enumerate(key_ranges(T, AKT, ksplit)):
        m, l, O = np.full(T, -np.inf, xd), np.zeros(T, f32), np.zeros((dk, T), f32)
        ev_run = ev_end if kind == "inherit_ev" else EB_MIN
        ev_acc = None
        for j0 in range(lo, hi, AKT):
            j1 = min(j0 + AKT, hi)
            st = s[j0:j1]
            m_new = np.maximum(m, st.max(0))
            with np.errstate(invalid="ignore", over="ignore"):
                alpha = np.where(np.isinf(m), 0, np.exp((m - m_new).astype(xd))).astype(f32)
                p = np.exp((st - m_new[None]).astype(xd)).astype(f32)
                ph, pl = split_f16(p, 2.0 ** P_EXP)
                ph, pl = F(ph), F(pl)
                psum = ((ph + pl) * f32(2.0 ** -P_EXP) if kind == "l_rounded" else p).sum(0, dtype=f32)
                l = l * alpha + psum
                m = m_new
                ev_run = max(ev_run, int(op.evt[j0 // AKT]))
                oresc = alpha
                if ev_acc is None:
                    ev_acc = ev_run
                elif ev_run != ev_acc:
                    dl = ev_acc - ev_run
                    if kind != "no_rescale":
                        oresc = alpha * (f32(0) if dl < -126 else f32(np.ldexp(1.0, dl)))
                    ev_acc = ev_run
                O = O * oresc[None]
                vh, vl = _scaled_planes(op.v32[:, j0:j1], ev_run, False)
                vh, vl = F(vh), F(vl)
                for s4 in range(-(-(j1 - j0) // 16)):
                    for term, a_, b_ in (("hh", vh, ph), ("lh", vl, ph), ("hl", vh, pl)):
                        if kind == "drop_o" and defect[1:] == (term, s4, j0 // AKT):
                            continue
                        for jj in range(16 * s4, min(16 * s4 + 16, j1 - j0)):
                            O += a_[:, jj][:, None] * b_[jj][None, :]
        ev_end = ev_run
        with np.errstate(invalid="ignore", over="ignore"):
            part[ksi, :dk] = O * f32(2.0 ** -P_EXP) * f32(np.ldexp(1.0, (ev_acc if ev_acc is not None else EB_MIN) - 141))
        part[ksi, dk], part[ksi, dk + 1] = m, l
        if nrel:
            part[ksi, dk + 2:] = window(s, ws, lo, hi, -np.inf)
    mm = part[:, dk].max(0)
    with np.errstate(invalid="ignore", over="ignore"):
        wk = np.exp(part[:, dk] - mm[None]).astype(f32)
        L = (part[:, dk + 1] * wk).sum(0, dtype=f32)
        o = (part[:, :dk] * wk[:, None]).sum(0, dtype=f32) / L[None]
        if nrel:
            wr = (np.exp(part[:, dk + 2:].max(0) - mm[None]) / L[None]).astype(f32)
            o = o + F(relv).T @ wr
    return o.astype(f32), part.astype(f32), np.asarray(s, f32)


def emulate_batch(qkv, n_heads, rel_k, rel_v, mask, ws, ksplit=1, *, defect=None, parts=None):
    """emulate over [B, 3C, T] -> (out [B, C, T], partial buffer flat, scores [B, n_heads, T, T]); parts (expected()'s): take its fp64 scores (s_exact)"""
    x = to_np(qkv)
    B, C3, T = x.shape
    C = C3 // 3
    dk = C // n_heads
    nrel = 0 if ws is None else 2 * ws + 1
    out, part, sc = np.zeros((B, C, T), f32), np.zeros((B, n_heads, ksplit, dk + 2 + nrel, T), f32), np.zeros((B, n_heads, T, T), f32)
    for b in range(B):
        for h in range(n_heads):
            hr = 0 if rel_k is None or rel_k.shape[0] == 1 else h
            o, pt, s = emulate(x[b, h * dk:(h + 1) * dk], x[b, C + h * dk:C + (h + 1) * dk], x[b, 2 * C + h * dk:2 * C + (h + 1) * dk],
                               None if rel_k is None else rel_k[hr], None if rel_v is None else rel_v[hr], None if mask is None else mask[b], ws, ksplit,
                               defect=defect, s_exact=None if parts is None else parts["s"][b, h])
            out[b, h * dk:(h + 1) * dk], part[b, h], sc[b, h] = o, pt, s
    return out, part.reshape(-1), sc


# ---------------------------------------------------------------------------------------------------------------- the cases, shared by the GPU test and the CPU self-test
WS = [None, 1, 4, 7]
DT_OF = {32: 2, 48: 2, 64: 2, 80: 3, 96: 3, 112: 4, 128: 4}
# every dk x T: (dk, heads, T, window, shared tables, B) -- the window rotates so that every dk and every T meets None, 1, 4 and 7 (7 at T = 4: wider than
# the sequence); T = 4: a last tile of 4 keys; 36 / 68 / 132 / 260: a last tile of 4 keys behind 1 / 2 / 4 / 8 whole ones; 132 and 260: a query block one past 128.
# Item 0 (no padding) away from / near the diagonal takes the plain / plain near-diagonal score loop, item 1 (cut off every tile edge) the masked one.
SHAPE_CASES = [(dk, 1 if (share and b % 2) else 2, T, WS[(a + b) % 4], share, 3 if (a + b) % 3 == 0 else 2)
               for a, dk in enumerate([32, 48, 64, 80, 96, 112, 128]) for b, T in enumerate([4, 36, 68, 132, 260]) for share in [(b + a // 2) % 2 == 0]]
MODEL_TABLE_CASE = (96, 2, 132, 4, True, 2)
MOVING_KINDS = ["ramp_up", "ramp_down", "channel_gains", "outlier_keys", "tiny", "huge", "zero_tile", "zero_query", "lane_halves", "masked_outliers", "ev_jump"]
_MOVING_SHAPES = [(96, 516), (128, 260), (96, 260), (128, 516)]
MOVING_CASES = [(kind,) + _MOVING_SHAPES[n % 4] + (3 if n % 3 == 0 else 2,) for n, kind in enumerate(MOVING_KINDS)]      # (kind, dk, T, B): every third with an all-padding item
# (dk, T, window, ranges, data, B): 9 tiles at T = 260 in 2 and 4 ranges (which do not divide them) and 3 (which does), 17 at T = 516 in 3 and 5
_KSPLIT = [(64, 260, 4, 2, "unit"), (96, 260, 7, 4, "ramp_up"), (128, 260, 4, 3, "ramp_down"), (64, 516, 1, 3, "outlier_keys"), (96, 516, 4, 5, "ramp_down"),
           (128, 516, None, 5, "unit"), (96, 260, 4, 3, "outlier_keys"), (128, 516, 4, 3, "ramp_up"), (64, 260, 7, 4, "ramp_down"), (96, 260, 4, 3, "ev_drop")]
KSPLIT_CASES = [c + (3 if n % 3 == 2 else 2,) for n, c in enumerate(_KSPLIT)]
SPLIT6_CASES = [(48, 2, 36, 1, False, 3), (96, 1, 132, 4, True, 2), (128, 1, 260, 7, True, 2), (64, 2, 260, None, True, 2)]


def moving_inputs(kind, dk, T, ws=4, B=2, nh=1):
    """inputs() with q, k, v changed so that the scales move (the first six: tests/test_conv_split_gpu.py::test_split_f16_attention_scales_follow_the_data);
    rel_v follows the mean |v|, so that the relative-value term does not hide the rest.  "unit": inputs() as it is."""
    qkv, rel_k, rel_v, mask = inputs(B, nh, dk, T, ws, True, unit=kind == "unit", seed=len(kind))       # (tables of dk ** -0.5, as in that test)
    if kind == "unit":
        return qkv, rel_k, rel_v, mask
    r = np.random.default_rng(dk + T + len(kind))
    C = dk * nh
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]              # (views)
    t = np.arange(T, dtype=f32) / f32(T - 1)
    if kind in ("ramp_up", "ramp_down"):
        e = f32(24.0) * (t if kind == "ramp_up" else 1 - t) - f32(12.0)
        v *= np.exp2(e)[None, None]
        k *= np.exp2(e / 8)[None, None]                                # (scores stay in a range where several keys share a row's weight)
        q *= f32(0.2)
    elif kind == "channel_gains":
        gain = np.exp2(r.random(3 * C) * 16 - 8).astype(f32)
        gain[:C] = 1.0 / gain[C:2 * C]                                 # q against k: the products stay O(1), the operands do not
        qkv *= gain[None, :, None]
    elif kind == "outlier_keys":
        pos = r.integers(0, T, 12)
        v[:, :, pos] *= f32(4096.0)
        k[:, :, pos] *= f32(4.0)
    elif kind == "tiny":
        v *= f32(2.0 ** -60)
        k *= f32(2.0 ** -30)
        q *= f32(2.0 ** 30)
    elif kind == "huge":
        v *= f32(2.0 ** 40)
        k *= f32(2.0 ** 20)
        q *= f32(2.0 ** -20)
    elif kind == "zero_tile":                                          # a K / V tile of zeros: both exponents at the floor
        k[:, :, 64:96] = 0
        v[:, :, 64:96] = 0
        k[:, :, :32] = 0                                               # (and the FIRST tile's K alone: the range starts from the floor)
    elif kind == "zero_query":
        q[:, :, 40] = 0
        q[:, :, 192:224] = 0
    elif kind == "lane_halves":                                        # the largest channel of query i in the lane half (d >> 3) & 1 == i & 1, 8 times the others
        big = ((np.arange(C)[:, None] >> 3) & 1) == (np.arange(T)[None, :] & 1)
        q *= np.where(big, f32(8.0), f32(1.0))[None]
        q *= f32(0.25)
    elif kind == "masked_outliers":                                    # the padded keys of item 1 hold the largest magnitudes of their tiles
        off = mask[1] == 0
        k[1][:, off] *= f32(2.0 ** 10)
        v[1][:, off] *= f32(2.0 ** 12)
    elif kind == "ev_jump":                                            # 130 binades between the first tile's V and the second's: the accumulators flush
        v[:, :, :32] *= f32(2.0 ** -100)
        v[:, :, 32:] *= f32(2.0 ** 30)
    elif kind == "ev_drop":                                            # the reverse: every later tile 90 binades under the first (a key range that inherited
        v[:, :, :32] *= f32(2.0 ** 30)                                 # the first range's ev would flush its V planes to zero)
        v[:, :, 32:] *= f32(2.0 ** -60)
    else:
        raise ValueError(kind)
    if rel_v is not None:
        rel_v = (rel_v * f32(np.abs(v).mean())).astype(f32)
    return qkv, rel_k, rel_v, mask


def all_cases():
    """every (name, qkv, heads, rel_k, rel_v, mask, window, ranges) the GPU file launches in the split-f16 arithmetic"""
    for dk, nh, T, ws, share, B in SHAPE_CASES:
        yield (f"dk{dk} nh{nh} T{T} ws{ws}", *_with(inputs(B, nh, dk, T, ws, share), nh, ws, 1))
    dk, nh, T, ws, share, B = MODEL_TABLE_CASE
    yield (f"dk{dk} T{T} model tables", *_with(inputs(B, nh, dk, T, ws, share, unit=False), nh, ws, 1))
    for kind, dk, T, B in MOVING_CASES:
        yield (f"{kind} dk{dk} T{T} B{B}", *_with(moving_inputs(kind, dk, T, B=B), 1, 4, 1))
    for dk, T, ws, ks, kind, B in KSPLIT_CASES:
        yield (f"ksplit{ks} {kind} dk{dk} T{T} B{B}", *_with(moving_inputs(kind, dk, T, ws, B=B), 1, ws, ks))


def _with(inp, nh, ws, ks):
    qkv, rel_k, rel_v, mask = inp
    return qkv, nh, rel_k, rel_v, mask, ws, ks
