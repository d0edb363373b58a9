"""Loudness normalisation on the device (csrc/loudness.hip): a batch of ragged waveforms delivered at a target programme loudness in LUFS --
mono ITU-R BS.1770-4 / EBU R128: K-weighted, gated.  Three launches, nothing read back in between: ``vs_loud_steps`` runs the K-weighting cascade in fp64 over
every sample -- a recursive filter made parallel across the lanes of a workgroup by a log-step scan of the filter state -- and sums its squares per 100 ms step;
``vs_loud_gate`` forms the 400 ms blocks, the two gates, the loudness and the gain of every row; ``vs_gain_apply`` scales the samples.  The rule is fully
specified in include/visinger_hip.h "f14".  The reference has no counterpart (it peak-normalises on the host).  Sample peaks are not looked at: a boost can
leave a waveform over full scale, which is what the limiter behind this stage is for.

Everything that changes between two calls -- the samples, the lengths -- is read from device tensors, so a captured graph replays on other data by overwriting
those buffers.  GPU tensors only; there is no CPU path and no backward.  ``loudness_ref`` is the rule restated in numpy, for the tests."""
import ctypes
import functools
import math

import numpy as np
import torch

from . import _args as A
from . import _lib as L

THREADS = 256                # VS_LOUD_THREADS: lanes of vs_loud_steps' workgroup
RATE_MIN, RATE_MAX = 8000, 48000         # VS_LOUD_MIN_RATE, VS_LOUD_MAX_RATE
ABS_GATE = 1.1724653045822981e-07                # VS_LOUD_ABS_GATE = 10^((-70 + 0.691) / 10): -70 LUFS as a mean square of the weighted signal
REL_GATE = 0.1                                   # -10 LU under the loudness of the blocks over the absolute gate
OFFSET = -0.691
DEFAULTS = dict(target_lufs=-23.0, max_gain_db=20.0)
U64 = 2.0 ** -53             # fp64 unit roundoff


def check_rate(sample_rate):
    """ValueError unless sample_rate is an integer in [8000, 48000] divisible by 10 (a step of 100 ms is a whole number of samples); returns s = rate / 10"""
    if not (A.is_int(sample_rate, RATE_MIN, RATE_MAX) and sample_rate % 10 == 0):
        raise ValueError(f"sample_rate must be an integer in [{RATE_MIN}, {RATE_MAX}] Hz divisible by 10, got {sample_rate!r}")
    return int(sample_rate) // 10


def check_args(target_lufs=-23.0, max_gain_db=20.0, sample_rate=None):
    """ValueError for host values the entries would refuse; returns (target_lufs, max_gain_db) as floats.  sample_rate: None (not looked at) or check_rate's"""
    if not A.is_real(target_lufs, -70.0, 0.0):
        raise ValueError(f"target_lufs must be a number in [-70, 0] LUFS, got {target_lufs!r}")
    if not A.is_real(max_gain_db, 0.0, 60.0):
        raise ValueError(f"max_gain_db must be a number in [0, 60] dB, got {max_gain_db!r}")
    if sample_rate is not None:
        check_rate(sample_rate)
    return float(target_lufs), float(max_gain_db)


@functools.lru_cache(maxsize=None)
def k_weighting(sample_rate):
    """((b1, a1), (b2, a2)): the two biquads of BS.1770's K-weighting at sample_rate, fp64 arrays of 3 with a[0] = 1 -- the bilinear transform of the standard's
    analogue prototypes (a high shelf of +4 dB at 1682 Hz, a high-pass at 38 Hz), which gives the standard's 48 kHz table to the printed digits"""
    check_rate(sample_rate)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sample_rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sample_rate)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    for v in (b1, a1, b2, a2):
        v.setflags(write=False)
    return (b1, a1), (b2, a2)


def coef_array(sample_rate):
    """the 10 doubles vs_loud_steps takes: b0, b1, b2, a1, a2 of the shelf, then of the high-pass"""
    (b1, a1), (b2, a2) = k_weighting(sample_rate)
    return np.array([*b1, a1[1], a1[2], *b2, a2[1], a2[2]], dtype=np.float64)


def state_matrix(sample_rate):
    """A, fp64 [4, 4]: one sample of the cascade -- each biquad in transposed direct form II -- on the state (z1, z2 of the shelf, z1, z2 of the high-pass) under
    a zero input; the output of that sample is (B0, 0, 1, 0) . state, B0 the high-pass's b[0]"""
    (b1, a1), (b2, a2) = k_weighting(sample_rate)
    return np.array([[-a1[1], 1.0, 0.0, 0.0],
                     [-a1[2], 0.0, 0.0, 0.0],
                     [b2[1] - a2[1] * b2[0], 0.0, -a2[1], 1.0],
                     [b2[2] - a2[2] * b2[0], 0.0, -a2[2], 0.0]])


def lane_samples(s):
    """c = ceil(s / 256): the consecutive samples of a step that one lane of vs_loud_steps owns"""
    return -(-s // THREADS)


@functools.lru_cache(maxsize=None)
def _carry(sample_rate):
    """the eight matrices M^(2^k), k = 0 .. 7, M = A^c, as pairs of doubles: fp64 [8, 2, 4, 4] -- [k, 0] is the exact power of A's doubles, formed in integers
    and rounded once, [k, 1] what that rounding left, rounded once"""
    A4 = state_matrix(sample_rate)
    ratios = [[float(v).as_integer_ratio() for v in row] for row in A4]
    E = max(d.bit_length() - 1 for row in ratios for _, d in row)               # every denominator is a power of two: a common 2^E
    N = [[n * ((1 << E) // d) for n, d in row] for row in ratios]
    mul = lambda P, Q: [[sum(P[i][k] * Q[k][j] for k in range(4)) for j in range(4)] for i in range(4)]
    P, e = N, E
    for _ in range(lane_samples(check_rate(sample_rate)) - 1):
        P, e = mul(P, N), e + E
    out = np.empty((8, 2, 4, 4))
    for k in range(8):
        for i in range(4):
            for j in range(4):
                hi = P[i][j] / (1 << e)                                         # (int / int: correctly rounded)
                n, d = hi.as_integer_ratio()
                out[k, 0, i, j], out[k, 1, i, j] = hi, (P[i][j] * d - (n << e)) / (d << e)
        P, e = mul(P, P), 2 * e
    out.setflags(write=False)
    return out


def carry_table(sample_rate, device=None):
    """The state transitions vs_loud_steps' scan needs at this rate: M^(2^k), k = 0 .. 7, M = A^c the transition over one lane's c samples, each as a pair of
    doubles (value, remainder): fp64 [8, 2, 4, 4].  device=None: the read-only numpy array; otherwise its copy on that device, made on first use and kept"""
    return _carry(sample_rate) if device is None else A.device_table(device, ("loudness", sample_rate), lambda: _carry(sample_rate))


def _impulse(b, a, n):
    """the first n samples of the impulse response of b / a (a[0] = 1)"""
    b, a = [float(v) for v in b], [float(v) for v in a]
    h, z1, z2 = np.empty(n), 0.0, 0.0
    for i in range(n):
        x = 1.0 if i == 0 else 0.0
        y = b[0] * x + z1
        z1, z2 = b[1] * x - a[1] * y + z2, b[2] * x - a[2] * y
        h[i] = y
    return h


@functools.lru_cache(maxsize=None)
def error_constants(sample_rate):
    """(kappa, scan) of DESIGN.md 4.21: to first order in u = 2^-53, a weighted sample is off by at most kappa u max|x| in a serial fp64 filter -- loudness_ref,
    and every lane's two passes on the device -- and by scan u max|x| more through the rounding of the device's lane scan.
    kappa: a biquad's roundings (three in y, five in z1, three in z2, no fused product assumed) are at most u (beta X + alpha Y) a sample, beta = |b0| + 3 |b1| +
    3 |b2|, alpha = 1 + 3 |a1| + 3 |a2|, X and Y the largest input and output; they reach its output through 1 / a.  With |.| the l1 norm of an impulse response:
    kappa = |h2| |1/a1| (beta1 + alpha1 |h1|) + |1/a2| (beta2 |h1| + alpha2 |h1 h2|).
    scan: a level of the scan rounds its result once -- the pairs keep what the products and sums lose, but for a second-order term 64 u mu, mu the largest
    absolute row sum of a M^(2^k) -- and the result is a state of the filter under a windowed input, at most Z max|x|;  eight levels.  Such an error in front of a
    lane reaches the output as the cascade's zero-input response, and the lanes' first samples are at least c apart: G = the sum over j of g(j c), g(m) the
    non-increasing majorant of the l1 norm of the output row of A^m.  scan = 8 (1 + 64 u mu) Z G."""
    (b1, a1), (b2, a2) = k_weighting(sample_rate)
    n = 2 * sample_rate // 5                                                     # 0.4 s: the slowest pole (radius 0.9705 at 8 kHz, 0.995 at 48 kHz) is below 1e-40 there
    one = (1.0, 0.0, 0.0)
    h1, h2, g1, g2 = _impulse(b1, a1, n), _impulse(b2, a2, n), _impulse(one, a1, n), _impulse(one, a2, n)
    H1, H2, G1, G2, H = (float(np.abs(v).sum()) for v in (h1, h2, g1, g2, np.convolve(h1, h2)[:n]))
    beta = lambda b: abs(b[0]) + 3 * abs(b[1]) + 3 * abs(b[2])
    alpha = lambda a: 1 + 3 * abs(a[1]) + 3 * abs(a[2])
    kappa = H2 * G1 * (beta(b1) + alpha(a1) * H1) + G2 * (beta(b2) * H1 + alpha(a2) * H)
    Z = max((abs(b1[1]) + abs(b1[2])) + (abs(a1[1]) + abs(a1[2])) * H1, (abs(b2[1]) + abs(b2[2])) * H1 + (abs(a2[1]) + abs(a2[2])) * H)
    mu = float(np.abs(_carry(sample_rate)[:, 0]).sum(axis=2).max())
    A4, c = state_matrix(sample_rate), lane_samples(sample_rate // 10)
    row, g = np.array([b2[0], 0.0, 1.0, 0.0]), np.empty(n)
    for i in range(n):
        g[i] = np.abs(row).sum()
        row = row @ A4
    g = np.maximum.accumulate(g[::-1])[::-1]
    return float(kappa), float(8 * (1 + 64 * U64 * mu) * Z * g[::c].sum())


def steps_bound(sample_rate, rho):
    """The bound on |S_dev - S_ref| / max_i S_ref[row] of a row whose samples have s max|x|^2 <= rho max_i S_ref[row]: with eps the error of a
    filtered sample relative to max|x| -- the device's and the restatement's together -- a step sum moves by at most 2 sqrt(s S) eps + s eps^2, and its own
    fp64 summation by (s + 2) 2^-53 S on either side"""
    kappa, scan = error_constants(sample_rate)
    eps = (2 * kappa + scan) * U64
    return 2.0 * math.sqrt(rho) * eps + rho * eps * eps + 2 * (sample_rate // 10 + 2) * U64


def _steps(who, wav, sample_rate, lengths):
    """the first launch: (wav, lengths, B, n, s, S) with S fp64 [B, max(n // s, 1)]"""
    s = check_rate(sample_rate)
    wav, B, n = A.waveform(who, wav)
    lengths = A.lengths_i64(who, "lengths", lengths, B, n, wav.device)
    lib = L.require_gpu()
    S = torch.empty((B, max(n // s, 1)), device=wav.device, dtype=torch.float64)
    coef = (ctypes.c_double * 10)(*coef_array(sample_rate))
    L.check(lib.vs_loud_steps(L.ptr(wav), A.vp(lengths), B, n, coef, A.vp(carry_table(sample_rate, wav.device)), s, A.vp(S), S.shape[1], L.stream_ptr()))
    return lib, wav, lengths, B, n, s, S


def _gate(lib, S, lengths, B, s, target, max_gain_db):
    loud = torch.empty(B, device=S.device, dtype=torch.float64)
    gain = torch.empty(B, device=S.device, dtype=torch.float32)
    stats = torch.empty((B, 3), device=S.device, dtype=torch.int32)
    L.check(lib.vs_loud_gate(A.vp(S), A.vp(lengths), B, S.shape[1], s, ctypes.c_double(target), ctypes.c_double(max_gain_db), A.vp(loud), A.vp(gain), A.vp(stats),
                             L.stream_ptr()))
    return loud, gain, stats


def step_sums(wav, sample_rate, lengths=None):
    """S, fp64 [B, max(L // s, 1)]: the sum of squares of the K-weighted samples of every complete 100 ms step inside a row's length, 0 elsewhere"""
    return _steps("step_sums", wav, sample_rate, lengths)[-1]


def measure(wav, sample_rate, lengths=None):
    """(loud, stats): the integrated loudness of every row of wav -- fp32 GPU [B, L] at sample_rate Hz -- in LUFS, fp64 [B] (-inf: no block passes the gates, or
    the row is shorter than 400 ms; NaN: a block that is not finite), and int32 [B, 3]: the row's 400 ms blocks, those over the absolute gate, those over both.
    lengths as in normalize."""
    lib, wav, lengths, B, n, s, S = _steps("measure", wav, sample_rate, lengths)
    loud, _, stats = _gate(lib, S, lengths, B, s, 0.0, 0.0)
    return loud, stats


def normalize(wav, sample_rate, lengths=None, out=None, return_loudness=False, return_stats=False, return_gain=False, **params):
    """wav -- fp32 GPU [B, L] at sample_rate Hz -- with every row scaled to target_lufs: y = x gain[b] inside the row's length, gain = 10^(min(target_lufs -
    loud, max_gain_db) / 20) rounded once to fp32.  A row without a finite loudness (shorter than 400 ms, silent, a NaN or an infinity in it) has gain 1 and
    comes back bit for bit, as does everything beyond a row's length.
    lengths: None (every row is L long), a host sequence of B integers in [0, L], or an int64 GPU tensor [B] -- used as it is, never read back (the kernels
    clamp it).  out: None (a new tensor), wav itself (in place) or an fp32 GPU tensor of wav's shape that does not overlap it.  return_loudness: also loud, fp64
    [B], the loudness measured BEFORE the gain;  return_stats: also int32 [B, 3] (measure);  return_gain: also gain, fp32 [B].  The result is y, or a tuple
    (y[, loud][, stats][, gain]).  params: DEFAULTS' keys -- target_lufs in [-70, 0] (default -23) and max_gain_db in [0, 60] (default 20; attenuation is not
    limited).  ValueError for host values out of range, VisingerHipError for tensors of the wrong kind; both before any launch."""
    target, max_gain_db = check_args(**A.keys("normalize", params, DEFAULTS))
    check_rate(sample_rate)
    wav_c, B, n = A.waveform("normalize", wav)
    out = A.out_like("normalize", wav_c, out)
    lib, wav_c, lengths, B, n, s, S = _steps("normalize", wav_c, sample_rate, lengths)
    loud, gain, stats = _gate(lib, S, lengths, B, s, target, max_gain_db)
    L.check(lib.vs_gain_apply(L.ptr(wav_c), A.vp(gain), A.vp(lengths), L.ptr(out), B, n, L.stream_ptr()))
    res = (out,) + ((loud,) if return_loudness else ()) + ((stats,) if return_stats else ()) + ((gain,) if return_gain else ())
    return res[0] if len(res) == 1 else res


def loudness_ref(x, lengths, sr, target=-23.0, max_gain_db=20.0):
    """(S, loud, stats, gain): the rule "f14" restated in numpy for a batch x -- fp32 [B, L] -- with lengths (None or B integers) at sr Hz: S fp64 [B, max(L // s,
    1)], loud fp64 [B], stats int64 [B, 3], gain fp32 [B].  A serial filter in fp64.  Written from the rule, used only by the tests."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, n_all = x.shape
    s = check_rate(sr)
    (b1, a1), (b2, a2) = k_weighting(sr)
    lens = [n_all] * B if lengths is None else [max(0, min(int(v), n_all)) for v in lengths]
    S = np.zeros((B, max(n_all // s, 1)))
    loud, stats, gain = np.full(B, -np.inf), np.zeros((B, 3), np.int64), np.ones(B, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b, n in enumerate(lens):
            ns = n // s
            v = x[b, :ns * s].astype(np.float64)
            for bq, aq in ((b1, a1), (b2, a2)):
                y, z1, z2 = np.empty_like(v), 0.0, 0.0
                for i, xi in enumerate(v.tolist()):
                    yi = bq[0] * xi + z1
                    z1, z2 = bq[1] * xi - aq[1] * yi + z2, bq[2] * xi - aq[2] * yi
                    y[i] = yi
                v = y
            S[b, :ns] = (v * v).reshape(ns, s).sum(axis=1)
            if ns < 4:
                continue
            z = (S[b, 0:ns - 3] + S[b, 1:ns - 2] + S[b, 2:ns - 1] + S[b, 3:ns]) / (4.0 * s)
            over = z > ABS_GATE
            both = over & (z > REL_GATE * (z[over].sum() / over.sum())) if over.any() else over
            stats[b] = len(z), over.sum(), both.sum()
            if not np.isfinite(z).all():
                loud[b] = np.nan
            elif both.any():
                loud[b] = OFFSET + 10.0 * np.log10(z[both].sum() / both.sum())
            if np.isfinite(loud[b]):
                gain[b] = np.float32(10.0 ** (min(target - loud[b], max_gain_db) / 20.0))
    return S, loud, stats, gain
