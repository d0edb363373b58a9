"""A look-ahead peak limiter on the device (csrc/limiter.hip): the ceiling behind a ``guide_dynamics`` boost and a ``resample_to`` conversion,
both of which can leave a waveform above full scale.  Every sample gets the reduction it needs on its own -- an integer, in units of 1/512 of a doubling of
amplitude, f10's unit -- the needs are held over ``window`` samples on both sides and smoothed over as many again, so that the gain ramps in before a peak and
never lets it through; a last guard makes ``|y| <= ceiling`` exact.  The rule is fully specified in include/visinger_hip.h "f11".  The reference has no
counterpart (it peak-normalises on the host).  A sample-peak limiter: inter-sample (true) peaks are not seen.

Everything that changes between two calls -- the samples, the lengths -- is read from device tensors, so a captured graph replays on other data by overwriting
those buffers.  GPU tensors only; there is no CPU path and no backward.  ``limit_ref`` is the rule restated in numpy, for the tests."""
import ctypes
import functools

import numpy as np
import torch

from . import _args as A
from . import _lib as L

TILE = 4096                  # VS_PEAK_LIMIT_TILE: samples a workgroup of vs_peak_limit writes
WINDOW_LIMIT = 1024          # VS_PEAK_LIMIT_MAX_WINDOW: samples on each side
TABLE = 512                  # VS_PEAK_LIMIT_TABLE: entries of the reduction table
U_MAX = 12288                # VS_PEAK_LIMIT_U_MAX: units, 24 doublings
UNITS_PER_DOUBLING = 512
CEILING_DB_MIN = -120.0      # a ceiling below this is no ceiling of a waveform (and 10^(dB / 20) stays a normal fp32 number)
DEFAULTS = dict(ceiling_db=-1.0, window=128)


def check_args(ceiling_db=-1.0, window=128):
    """ValueError for host values vs_peak_limit would refuse; returns (c, window): c the ceiling as the entry takes it -- 10^(ceiling_db / 20) in double, rounded
    once to fp32 (a Python float that holds that fp32 value)"""
    if not A.is_real(ceiling_db, CEILING_DB_MIN, 0):
        raise ValueError(f"ceiling_db must be a number in [{CEILING_DB_MIN:.0f}, 0] dB (full scale = 0), got {ceiling_db!r}")
    if not A.is_int(window, 0, WINDOW_LIMIT):
        raise ValueError(f"window must be an integer in [0, {WINDOW_LIMIT}] samples, got {window!r}")
    return float(np.float32(10.0 ** (float(ceiling_db) / 20.0))), int(window)


@functools.lru_cache(maxsize=1)
def _table():
    j = np.arange(TABLE, dtype=np.float64)
    tab = np.ceil(UNITS_PER_DOUBLING * np.log2(1.0 + (j + 1.0) / TABLE)).astype(np.int32)
    tab.setflags(write=False)
    return tab


def reduction_table(device=None):
    """tab[j] = ceil(512 log2(1 + (j + 1) / 512)), j = 0 .. 511, in double: the reduction in units that a quotient whose leading 9 mantissa bits are j needs at
    most.  device=None: the read-only int32 numpy array; otherwise its copy on that device, made on first use and kept"""
    return _table() if device is None else A.device_table(device, "limiter", _table)


def limit_peaks(wav, lengths=None, out=None, return_gain=False, return_stats=False, **params):
    """wav -- fp32 GPU [B, L] -- held under the ceiling: fp32 [B, L] with |y| <= 10^(ceiling_db / 20) for every sample of a row that is not a NaN; samples that
    no reduction reaches -- a whole row with nothing over the ceiling -- and everything beyond a row's length come back bit for bit.
    lengths: None (every row is L long), a host sequence of B integers in [0, L], or an int64 GPU tensor [B] -- used as it is, never read back (the kernel
    clamps it).  out: None (a new tensor), wav itself (in place: one workgroup per row walks it, slower on few long rows) or an fp32 GPU tensor of wav's shape
    that does not overlap it.  return_gain: also g, int32 [B, L], the reduction per sample in units of 1/512 of a doubling of amplitude.  return_stats: also
    int32 [B, 3]: the samples over the ceiling, the largest reduction, the samples the last guard moved.  The result is y, or a tuple (y[, g][, stats]).
    params: DEFAULTS' keys -- ceiling_db (<= 0, default -1.0) and window (samples on each side, default 128; 0: a per-sample soft clip).
    ValueError for host values out of range, VisingerHipError for tensors of the wrong kind; both before any launch."""
    c, window = check_args(**A.keys("limit_peaks", params, DEFAULTS))
    wav, B, n = A.waveform("limit_peaks", wav)
    lengths = A.lengths_i64("limit_peaks", "lengths", lengths, B, n, wav.device)
    out = A.out_like("limit_peaks", wav, out)
    lib = L.require_gpu()
    gain = torch.empty((B, n), device=wav.device, dtype=torch.int32) if return_gain else None
    stats = torch.empty((B, 3), device=wav.device, dtype=torch.int32) if return_stats else None
    L.check(lib.vs_peak_limit(L.ptr(wav), A.vp(lengths), A.vp(reduction_table(wav.device)), ctypes.c_float(c), window, L.ptr(out), A.vp(gain), A.vp(stats), B, n,
                              L.stream_ptr()))
    res = (out,) + ((gain,) if return_gain else ()) + ((stats,) if return_stats else ())
    return res[0] if len(res) == 1 else res


def _sliding_max(u, W):
    """max of u over |i - j| <= W, cut at the ends (u >= 0): van Herk / Gil-Werman -- running maxima from both ends of blocks of 2 W + 1"""
    n, w = len(u), 2 * W + 1
    if n == 0 or W == 0:
        return u.copy()
    pad = np.zeros(-(-(n + 2 * W) // w) * w, dtype=u.dtype)
    pad[W:W + n] = u                                                  # sample j sits at W + j: its window is pad[j .. j + 2 W]
    blocks = pad.reshape(-1, w)
    fwd = np.maximum.accumulate(blocks, axis=1).ravel()               # from the block's first sample up to here
    bwd = np.maximum.accumulate(blocks[:, ::-1], axis=1)[:, ::-1].ravel()        # from here to the block's last sample
    j = np.arange(n)
    return np.maximum(bwd[j], fwd[j + 2 * W])


def limit_ref(x, lengths, c, W):
    """(u, M, g, y): the rule "f11" restated in numpy for a batch x -- fp32 [B, L] -- with lengths (None or B integers), the ceiling c (an fp32 value) and the
    window W: u, M, g int64 [B, L], y fp64 [B, L] -- x 2^(-g / 512) in double, brought to +-c where it exceeds c, x itself where g = 0.  Written from the rule,
    used only by the tests."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, n_all = x.shape
    c = np.float32(c)
    tab = reduction_table().astype(np.int64)
    lens = [n_all] * B if lengths is None else [max(0, min(int(v), n_all)) for v in lengths]
    u, M, g = (np.zeros((B, n_all), np.int64) for _ in range(3))
    y = x.astype(np.float64)
    for b, n in enumerate(lens):
        a = np.abs(x[b, :n])
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            over = a > c                                              # (False for a NaN)
            rho = (a[over] / c).astype(np.float32)                    # one fp32 division, correctly rounded; inf stays inf
        bits = rho.view(np.uint32).astype(np.int64)
        u[b, :n][over] = np.minimum(512 * ((bits >> 23) - 127) + tab[(bits & 0x7FFFFF) >> 14], U_MAX)
        M[b, :n] = _sliding_max(u[b, :n], W)
        cs = np.concatenate([[0], np.cumsum(M[b, :n])])
        i = np.arange(n)
        lo, hi = np.maximum(i - W, 0), np.minimum(i + W, n - 1)
        S, N = cs[hi + 1] - cs[lo], hi - lo + 1
        g[b, :n] = (S + N - 1) // N
        on = g[b] > 0
        with np.errstate(invalid="ignore", over="ignore"):
            v = y[b, on] * np.exp2(-g[b, on] / 512.0)
            y[b, on] = np.where(np.abs(v) > float(c), np.copysign(float(c), v), v)
    return u, M, g, y
