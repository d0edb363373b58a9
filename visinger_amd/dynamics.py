"""Guide dynamics on the device (csrc/dynamics.hip): the loudness contour of a recording -- crescendi, accents, phrase shapes -- carried onto
the synthesised waveform.  The model has no energy condition, so a phrase comes out at the network's loudness whatever the guide did; this tracks the level of
both per frame (``track_level``), forms a smoothed, limited gain per frame from their difference (``level_gain``, after ``level_offset`` in "contour" mode) and
applies it per sample (``apply_gain``); ``match_dynamics`` is the composition.  The rule is fully specified in include/visinger_hip.h "f10".  The reference has
no counterpart.

A level curve is fp32 mean-square power per frame (not finite or <= 0: no level there), so ``timing.retime(curve=)`` warps it as it warps an f0 curve.  Gains
are integers in units of 1/256 of a doubling of power (UNITS_PER_DB units a dB).

Everything that changes between two calls -- the samples, the curves, the lengths, the offset -- is read from device tensors, so a captured graph replays on
other data by overwriting those buffers.  GPU tensors only; there is no CPU path and no backward."""
import math

import torch

from . import _args as A
from . import _lib as L

TILE = 1024                  # VS_LEVEL_GAIN_TILE: frames a workgroup of vs_level_gain writes
T_LIMIT = 65536              # frames (vs_level_offset, vs_level_gain)
HOP_LIMIT = 2048             # vs_level_apply (vs_level_track alone takes 4096: TRACK_HOP_LIMIT)
TRACK_HOP_LIMIT = 4096
HALF_LIMIT = 8               # blocks on each side of a frame that its level is the mean of
WINDOW_LIMIT = 1024          # frames on each side of a frame that its gain is the mean of
GAIN_LIMIT = 4096            # units: max_boost_db and max_cut_db, about 48.16 dB
GATE_LIMIT = 1 << 16         # units: |gate_db|, about 770 dB
OFFSET_LIMIT = 1 << 17       # units: what vs_level_gain clamps an offset to
UNITS_PER_DB = 256.0 / (10.0 * math.log10(2.0))
DEFAULTS = dict(half_width=1, window=12, depth=1.0, max_boost_db=12.0, max_cut_db=24.0, gate_db=-70.0, mode="contour")


def db_to_units(db):
    """rint(dB 256 / (10 log10 2)), in double: a level difference in dB in units of 1/256 of a doubling of power"""
    return int(round(float(db) * UNITS_PER_DB))          # (Python's round is rint: half to even)


def check_args(half_width=1, window=12, depth=1.0, max_boost_db=12.0, max_cut_db=24.0, gate_db=-70.0, mode="contour"):
    """ValueError for host values the four entries would refuse; returns (half, window, depth_q = round(256 depth), up, down, gate, contour): the limits and
    the gate in units, contour = (mode == "contour")"""
    if not A.is_int(half_width, 0, HALF_LIMIT):
        raise ValueError(f"half_width must be an integer in [0, {HALF_LIMIT}] frames, got {half_width!r}")
    if not A.is_int(window, 0, WINDOW_LIMIT):
        raise ValueError(f"window must be an integer in [0, {WINDOW_LIMIT}] frames, got {window!r}")
    if not A.is_real(depth, 0, 1):
        raise ValueError(f"depth must be a number in [0, 1], got {depth!r}")
    top = GAIN_LIMIT / UNITS_PER_DB
    for name, v in (("max_boost_db", max_boost_db), ("max_cut_db", max_cut_db)):
        if not A.is_real(v, 0, top):
            raise ValueError(f"{name} must be a number in [0, {top:.2f}] dB, got {v!r}")
    if not A.is_real(gate_db, -GATE_LIMIT / UNITS_PER_DB, GATE_LIMIT / UNITS_PER_DB):
        raise ValueError(f"gate_db must be a number in [{-GATE_LIMIT / UNITS_PER_DB:.1f}, {GATE_LIMIT / UNITS_PER_DB:.1f}] dB, got {gate_db!r}")
    if not (isinstance(mode, str) and mode in ("contour", "absolute")):
        raise ValueError(f"mode must be 'contour' or 'absolute', got {mode!r}")
    return int(half_width), int(window), int(round(256 * float(depth))), db_to_units(max_boost_db), db_to_units(max_cut_db), db_to_units(gate_db), mode == "contour"


def _check_hop(who, hop_size, limit):
    if not A.is_int(hop_size, 1, limit):
        raise ValueError(f"{who}: hop_size must be an integer in [1, {limit}], got {hop_size!r}")
    return int(hop_size)


def _curves(who, guide, own, lengths):
    guide = A.gpu_tensor(who, "guide", guide, torch.float32, (None, None))
    B, T = guide.shape
    own = A.gpu_tensor(who, "own", own, torch.float32, (B, T))
    if B < 1 or not 1 <= T <= T_LIMIT:
        raise L.VisingerHipError(f"{who}: B >= 1 and 1 <= T <= {T_LIMIT} are required, got B = {B}, T = {T}")
    return guide, own, A.lengths_i64(who, "lengths", lengths, B, T, guide.device), B, T


def track_level(wav, hop_size, lengths=None, half_width=1, frames=None):
    """level fp32 [B, T]: the mean-square power of wav -- fp32 GPU [B, L] -- per frame of hop_size samples, over the frame's block and half_width blocks on
    each side (cut at the row's ends).  Row b has lengths[b] // hop_size frames; the rest of it, and a frame whose sum is not finite, comes back 0: no level.
    lengths: None (every row is L long), a host sequence of B integers in [0, L], or an int64 GPU tensor [B] -- used as it is, never read back (the kernel
    clamps it).  frames=None: T = L // hop_size; otherwise the result is `frames` wide.  ValueError for host values out of range, VisingerHipError for tensors
    of the wrong kind; both before any launch."""
    hop = _check_hop("track_level", hop_size, TRACK_HOP_LIMIT)
    half = check_args(half_width=half_width)[0]
    if frames is not None and not A.is_int(frames, 1, (1 << 31) - 1):
        raise ValueError(f"frames must be an integer in [1, 2^31), got {frames!r}")
    wav, B, n = A.waveform("track_level", wav)
    lengths = A.lengths_i64("track_level", "lengths", lengths, B, n, wav.device)
    T = n // hop if frames is None else int(frames)
    if T < 1:
        raise ValueError(f"a waveform of {n} samples has no frame of {hop}: give at least hop_size samples (or frames=)")
    lib = L.require_gpu()
    level = torch.empty((B, T), device=wav.device, dtype=torch.float32)
    L.check(lib.vs_level_track(L.ptr(wav), A.vp(lengths), B, n, hop, half, L.ptr(level), T, L.stream_ptr()))
    return level


def level_offset(guide, own, lengths=None, gate_db=DEFAULTS["gate_db"]):
    """(off, n_act): int32 [B] each -- the rounded mean of the guide's level over the own curve's, in units, over the frames where both are at or above the
    gate (0 when there are none), and their number.  guide, own: fp32 GPU [B, T] level curves;  lengths: in frames, see track_level."""
    gate = check_args(gate_db=gate_db)[5]
    guide, own, lengths, B, T = _curves("level_offset", guide, own, lengths)
    lib = L.require_gpu()
    off = torch.empty((B,), device=guide.device, dtype=torch.int32)
    n_act = torch.empty((B,), device=guide.device, dtype=torch.int32)
    L.check(lib.vs_level_offset(L.ptr(guide), L.ptr(own), A.vp(lengths), gate, A.vp(off), A.vp(n_act), B, T, L.stream_ptr()))
    return off, n_act


def _offset_tensor(offset_units, B, device):
    """int32 [B] on the device, or None: None, an integer (every item), a sequence of B integers -- within OFFSET_LIMIT -- or an int32 GPU tensor [B]"""
    if offset_units is None:
        return None
    if torch.is_tensor(offset_units) and offset_units.is_cuda:
        if not (offset_units.dtype == torch.int32 and tuple(offset_units.shape) == (B,)):
            raise L.VisingerHipError(f"level_gain: offset_units as a GPU tensor must be int32 [{B}], got {offset_units.dtype} {tuple(offset_units.shape)}")
        return offset_units.contiguous()
    if torch.is_tensor(offset_units):
        offset_units = offset_units.tolist()
    vals = [offset_units] * B if A.is_int(offset_units, -OFFSET_LIMIT, OFFSET_LIMIT) else offset_units
    if isinstance(vals, (str, bytes)) or not hasattr(vals, "__len__") or len(vals) != B or not all(A.is_int(v, -OFFSET_LIMIT, OFFSET_LIMIT) for v in vals):
        raise ValueError(f"offset_units must be an integer or {B} integers in [{-OFFSET_LIMIT}, {OFFSET_LIMIT}], got {offset_units!r:.60}")
    return torch.tensor([int(v) for v in vals], dtype=torch.int32).to(device)


def level_gain(guide, own, lengths=None, offset_units=None, **params):
    """k int32 [B, T]: the gain per frame in units -- the windowed mean of the guide's level over the own curve's, less offset_units, scaled by depth and
    limited to [-max_cut_db, max_boost_db]; a frame below the gate takes its neighbours' gain; 0 where no active frame lies within `window`, and beyond the
    row's length.  offset_units: None (0), an integer, B integers, or an int32 GPU tensor [B] (level_offset's `off`: used as it is, never read back).
    params: DEFAULTS' keys (half_width and mode are checked and not used here)."""
    _, window, depth_q, up, down, gate, _ = check_args(**A.keys("level_gain", params, DEFAULTS))
    guide, own, lengths, B, T = _curves("level_gain", guide, own, lengths)
    offset = _offset_tensor(offset_units, B, guide.device)
    lib = L.require_gpu()
    k = torch.empty((B, T), device=guide.device, dtype=torch.int32)
    L.check(lib.vs_level_gain(L.ptr(guide), L.ptr(own), A.vp(lengths), A.vp(offset), gate, window, depth_q, up, down, 0, A.vp(k), B, T, L.stream_ptr()))
    return k


def apply_gain(wav, k, hop_size, lengths=None, out=None):
    """wav 2^(k / 512) per sample: fp32 [B, L], the gain k -- int32 GPU [B, T], units per frame -- linear in level between frame centres and held before the
    first and after the last one.  lengths: in SAMPLES (see track_level); row b is scaled over its first min(lengths[b] // hop_size, T) hop_size samples, the
    rest -- and every sample whose gain is 0 -- comes back bit for bit.  out: None (a new tensor), wav itself (in place) or an fp32 GPU tensor of wav's shape
    that does not overlap it."""
    hop = _check_hop("apply_gain", hop_size, HOP_LIMIT)
    wav, B, n = A.waveform("apply_gain", wav)
    k = A.gpu_tensor("apply_gain", "k", k, torch.int32, (B, None))
    T = k.shape[1]
    if T < 1:
        raise L.VisingerHipError("apply_gain: k must have at least one frame")
    lengths = A.lengths_i64("apply_gain", "lengths", lengths, B, n, wav.device)
    out = A.out_like("apply_gain", wav, out)
    L.check(L.require_gpu().vs_level_apply(L.ptr(wav), A.vp(k), A.vp(lengths), hop, L.ptr(out), B, n, T, L.stream_ptr()))
    return out


def match_dynamics(wav, guide_level, hop_size, lengths=None, return_gain=False, **params):
    """wav with the dynamics of guide_level: fp32 [B, L] -- or (that, k) with return_gain.  wav: fp32 GPU [B, L];  guide_level: fp32 GPU [B, T], the guide's
    level curve on wav's frames (a row of zeros: that row comes back bit for bit);  lengths: in SAMPLES, see track_level.  The composition: own =
    track_level(wav, frames=T); in mode "contour" (the default) offset = level_offset(guide_level, own), used as a device tensor and never read back -- the
    guide's SHAPE at the synthesiser's own mean level, the right default since the microphone level of a guide is arbitrary -- in mode "absolute" no offset:
    the guide's level itself;  k = level_gain(..);  apply_gain(wav, k).  params: DEFAULTS' keys.  A boost can leave the waveform above full scale:
    limiter.limit_peaks is the peak guard behind it."""
    half, _, _, _, _, _, contour = check_args(**A.keys("match_dynamics", params, DEFAULTS))
    hop = _check_hop("match_dynamics", hop_size, HOP_LIMIT)
    wav, B, n = A.waveform("match_dynamics", wav)
    guide_level = A.gpu_tensor("match_dynamics", "guide_level", guide_level, torch.float32, (B, None))
    T = guide_level.shape[1]
    if not 1 <= T <= T_LIMIT:
        raise L.VisingerHipError(f"match_dynamics: 1 <= T <= {T_LIMIT} frames are required, got {T}")
    lengths = A.lengths_i64("match_dynamics", "lengths", lengths, B, n, wav.device)
    frames = None if lengths is None else torch.div(lengths.clamp(0, n), hop, rounding_mode="floor").clamp_(max=T)
    own = track_level(wav, hop, lengths=lengths, half_width=half, frames=T)
    gain_kw = {key: v for key, v in params.items() if key not in ("half_width", "mode")}
    offset = level_offset(guide_level, own, lengths=frames, gate_db=params.get("gate_db", DEFAULTS["gate_db"]))[0] if contour else None
    k = level_gain(guide_level, own, lengths=frames, offset_units=offset, **gain_kw)
    out = apply_gain(wav, k, hop, lengths=lengths)
    return (out, k) if return_gain else out
