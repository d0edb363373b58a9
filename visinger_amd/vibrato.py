"""Vibrato for the curve the model sings (csrc/vibrato.hip): a per-note pitch modulation added on the device between the pitch predictor (or a
guide curve) and ``pitch.pitch_condition``.  ``guide_correct`` can keep, scale or remove the vibrato a recording has; this op ADDS one -- to the predictor's own
curve, the case of every item without a guide, or to a guide that was flattened.  A note is a run of frames whose tokens carry one note id; behind an onset
delay the modulation fades in over ``attack`` frames, runs at ``rate_hz`` from phase 0 and fades out over the note's last ``release`` frames; notes shorter than
``min_note_s`` and rests get none.  The offset is integer arithmetic in 1/16 cent on a host-built sine table; the rule is fully specified in
include/visinger_hip.h "f13".  The reference has no counterpart.

Everything that changes between two calls -- the curve, the alignment, the notes, the six settings per item -- is read from device tensors, so a captured graph
replays under other settings by overwriting them.  GPU tensors only; there is no CPU path and no backward (an input that requires grad is refused while autograd
records).  ``vibrato_ref`` is the rule restated in numpy, for the tests."""
import functools
import math
import numbers

import numpy as np
import torch

from . import _args as A
from . import _lib as L

N_PARAMS = 6                 # VS_VIBRATO_PARAMS: depth_q, inc, delay, attack, release, min_len
SINE = 1024                  # VS_VIBRATO_SINE: steps of the sine table per cycle (the table has one entry more)
SINE_SCALE = 16384
UNITS_PER_CENT = 16
UNITS_PER_OCTAVE = 19200
DEPTH_Q_MAX = 19200          # VS_VIBRATO_MAX_DEPTH_Q: one octave
RAMP_MAX = 4096              # VS_VIBRATO_MAX_RAMP: attack and release, frames (at least 1)
DELAY_MAX = 65535            # VS_VIBRATO_MAX_DELAY: delay and min_len, frames
REST = 0                     # the pitch token of a rest and of the padding: the reference's pitch map gives MIDI note 0 -- a rest -- index 0, its collate pads note_pitch
#                              with 0, and TextEncoder.padding_idx is 0 (preprocessor/base_binarizer.py:318-323, tasks/dataset_utils.py:182, encoder.py:26)
DEFAULTS = dict(depth_cents=50.0, rate_hz=5.5, delay_s=0.25, attack_s=0.2, release_s=0.1, min_note_s=0.4)


def _frames(name, seconds, frame_rate, lo, hi):
    if not A.is_real(seconds, 0.0):
        raise ValueError(f"{name} must be a finite number >= 0 seconds, got {seconds!r}")
    n = max(lo, int(math.floor(float(seconds) * frame_rate + 0.5)))
    if n > hi:
        raise ValueError(f"{name} = {seconds!r} s is {n} frames at {frame_rate:.2f} frames a second: over the kernel's limit of {hi}")
    return n


def check_args(sample_rate=None, hop_size=None, **kw):
    """ValueError for an unknown key, a value that is no finite number, or one that maps outside vs_pitch_vibrato's limits at the frame rate sample_rate /
    hop_size (both required); returns the item's six integers (depth_q, inc, delay, attack, release, min_len) -- DEFAULTS where a key is missing.
    depth_cents in [0, 1200];  rate_hz with 0 < inc < 2^31 (below half the frame rate);  attack_s, release_s up to 4096 frames (at least one frame is taken);
    delay_s, min_note_s up to 65535 frames."""
    o = dict(DEFAULTS, **A.keys("vibrato", kw, DEFAULTS))
    if not (A.is_real(sample_rate, 1.0) and A.is_int(hop_size, 1, 1 << 20)):
        raise ValueError(f"vibrato needs sample_rate (a number >= 1, the model's) and hop_size (an integer >= 1), got {sample_rate!r}, {hop_size!r}")
    frame_rate = float(sample_rate) / hop_size
    if not A.is_real(o["depth_cents"], 0.0, DEPTH_Q_MAX / UNITS_PER_CENT):
        raise ValueError(f"depth_cents must be a number in [0, {DEPTH_Q_MAX // UNITS_PER_CENT}], got {o['depth_cents']!r}")
    if not A.is_real(o["rate_hz"], 0.0):
        raise ValueError(f"rate_hz must be a finite number > 0, got {o['rate_hz']!r}")
    inc = int(math.floor(float(o["rate_hz"]) / frame_rate * 4294967296.0 + 0.5))
    if not 0 < inc < 1 << 31:
        raise ValueError(f"rate_hz = {o['rate_hz']!r} is a phase step of {inc} / 2^32 cycles a frame at {frame_rate:.2f} frames a second: it must be in (0, 2^31)")
    return (int(math.floor(float(o["depth_cents"]) * UNITS_PER_CENT + 0.5)), inc, _frames("delay_s", o["delay_s"], frame_rate, 0, DELAY_MAX),
            _frames("attack_s", o["attack_s"], frame_rate, 1, RAMP_MAX), _frames("release_s", o["release_s"], frame_rate, 1, RAMP_MAX),
            _frames("min_note_s", o["min_note_s"], frame_rate, 0, DELAY_MAX))


def params_rows(B, sample_rate, hop_size, **kw):
    """B rows of six integers (check_args of every item): each keyword is a number -- every item's -- or a sequence of B numbers"""
    A.keys("vibrato", kw, DEFAULTS)
    per_item = {}
    for k, v in kw.items():
        if isinstance(v, numbers.Real) or isinstance(v, str) or v is None:
            per_item[k] = [v] * B
        else:
            per_item[k] = list(v.tolist() if hasattr(v, "tolist") else v)
            if len(per_item[k]) != B:
                raise ValueError(f"vibrato: {len(per_item[k])} values of {k} for a batch of {B}")
    return [check_args(sample_rate, hop_size, **{k: v[b] for k, v in per_item.items()}) for b in range(B)]


def params(B, sample_rate, hop_size, device, **kw):
    """int32 [B, 6] on the device: the settings vs_pitch_vibrato reads, one row per item (params_rows)"""
    rows = np.asarray(params_rows(B, sample_rate, hop_size, **kw), dtype=np.int64)
    return torch.from_numpy(rows.astype(np.uint32).view(np.int32).reshape(B, N_PARAMS)).to(device)


def params_tensor(value, B, device=None):
    """the int32 GPU tensor [B, 6] a caller made with params(): checked for kind only, used as it is and never read back (the kernel clamps what is out of range)"""
    return A.gpu_tensor("vibrato", "params", value, torch.int32, (B, N_PARAMS))


@functools.lru_cache(maxsize=1)
def _table():
    tab = np.rint(SINE_SCALE * np.sin(2.0 * np.pi * np.arange(SINE + 1, dtype=np.float64) / SINE)).astype(np.int32)
    tab.setflags(write=False)
    return tab


def sine_table(device=None):
    """tab[i] = round(16384 sin(2 pi i / 1024)), i = 0 .. 1024, in double.  device=None: the read-only int32 numpy array; otherwise its copy on that device, made
    on first use and kept"""
    return _table() if device is None else A.device_table(device, "vibrato", _table)


def notes_of_tokens(pitch_tokens, rest=REST):
    """int32, the shape of pitch_tokens ([B, T_ph] or [T_ph]; a torch tensor on any device, or an array): the note every token belongs to, counted from 1 along
    the row -- a new note starts where the pitch token differs from the previous token's -- and 0 on rest tokens (`rest`, which is also the padding).  The same
    pitch on both sides of a rest is two notes.  Torch ops on the tokens' device, nothing is read back."""
    t = pitch_tokens if torch.is_tensor(pitch_tokens) else torch.as_tensor(np.asarray(pitch_tokens))
    sung = t != rest
    first = torch.ones_like(sung)
    first[..., 1:] = t[..., 1:] != t[..., :-1]
    return (torch.cumsum((first & sung).to(torch.int32), dim=-1) * sung).to(torch.int32)


def depth_q_of_tokens(depth_cents, T_ph=None):
    """int32 numpy [T_ph]: a per-token depth in cents -- NaN or None = the item's default -- as vs_pitch_vibrato's note_depth_q (1/16 cent, -1 = default), padded
    with -1 to T_ph; ValueError for a value outside [0, 1200]"""
    vals = [float("nan") if v is None else float(v) for v in (depth_cents.tolist() if hasattr(depth_cents, "tolist") else depth_cents)]
    out = np.full(len(vals) if T_ph is None else T_ph, -1, dtype=np.int32)
    for i, v in enumerate(vals):
        if not math.isnan(v):
            if not 0.0 <= v <= DEPTH_Q_MAX / UNITS_PER_CENT:
                raise ValueError(f"vibrato_depth_cents must be in [0, {DEPTH_Q_MAX // UNITS_PER_CENT}] (NaN or None: the default), got {v!r} at token {i}")
            out[i] = int(math.floor(v * UNITS_PER_CENT + 0.5))
    return out


def vibrato(curve, mel2ph, note_of_token, params, note_depth_q=None, lengths=None, pred=None):
    """(curve_out, offset_q): fp32 [B, T], the modulated curve, and int32 [B, T], the offset in 1/16 cent; both 0 beyond a row's length.
    The curve, in the model's domain log2(Hz + 1), is `curve` -- fp32 [B, T] or [B, 1, T], a normalised curve as pitch.norm_interp_f0 returns it -- or column 0
    of `pred`, the pitch predictor's fp32 [B, T, 2] (give one of the two; pred is read in place with a stride of 2).  mel2ph: int64 [B, T], 0 = padding.
    note_of_token: int32 [B, T_ph] (notes_of_tokens), 0 = a rest.  params: int32 [B, 6] (params()).  note_depth_q: None or int32 [B, T_ph], the depth of a note in
    1/16 cent read at the note's first token, -1 = the item's.  lengths: None (a row's count of non-zero frames of mel2ph, taken on the device) or an int64 GPU
    tensor [B].  curve_out holds the curve's own bits wherever offset_q is 0."""
    if (curve is None) == (pred is None):
        raise L.VisingerHipError("vibrato: give curve ([B, T]) or pred ([B, T, 2]), one of the two")
    src = curve if pred is None else pred
    if not (torch.is_tensor(src) and src.is_cuda):
        raise L.VisingerHipError("vibrato: the curve must be a tensor on the GPU (there is no CPU path)")
    if torch.is_grad_enabled() and src.requires_grad:
        raise L.VisingerHipError("vibrato: the curve requires grad: the vibrato kernel has no backward (detach it, or run under no_grad)")
    if pred is not None:
        if not (src.dim() == 3 and src.shape[2] == 2):
            raise L.VisingerHipError(f"vibrato: pred must be [B, T, 2], got {tuple(src.shape)}")
        stride = 2
    else:
        if src.dim() == 3 and src.shape[1] == 1:
            src = src[:, 0]
        if src.dim() != 2:
            raise L.VisingerHipError(f"vibrato: curve must be [B, T], got {tuple(src.shape)}")
        stride = 1
    src = src.float().contiguous()
    B, T = src.shape[:2]
    if B == 0 or T == 0 or T >= (1 << 31) - 256:
        raise L.VisingerHipError(f"vibrato: B, T must be positive and T < 2^31 - 256, got {(B, T)}")
    mel2ph = A.gpu_tensor("vibrato", "mel2ph", mel2ph, torch.int64, (B, T))
    note_of_token = A.gpu_tensor("vibrato", "note_of_token", note_of_token, torch.int32, (B, None))
    T_ph = note_of_token.shape[1]
    if T_ph == 0:
        raise L.VisingerHipError("vibrato: note_of_token must hold at least one token per row")
    params = params_tensor(params, B)
    if note_depth_q is not None:
        note_depth_q = A.gpu_tensor("vibrato", "note_depth_q", note_depth_q, torch.int32, (B, T_ph))
    lengths = (mel2ph > 0).sum(dim=1) if lengths is None else A.gpu_tensor("vibrato", "lengths", lengths, torch.int64, (B,))
    lib = L.require_gpu()
    out = torch.empty((B, T), device=src.device, dtype=torch.float32)
    offset_q = torch.empty((B, T), device=src.device, dtype=torch.int32)
    L.check(lib.vs_pitch_vibrato(L.ptr(src), stride, A.vp(mel2ph), A.vp(lengths), A.vp(note_of_token), A.vp(note_depth_q), A.vp(params),
                                 A.vp(sine_table(src.device)), A.vp(offset_q), L.ptr(out), B, T, T_ph, L.stream_ptr()))
    return out, offset_q


def vibrato_ref(curve, mel2ph, note_of_token, params, note_depth_q=None, lengths=None):
    """(offset_q, curve_out): the rule "f13" restated in numpy, note by note, for a batch: curve [B, T] (the model's domain), mel2ph [B, T], note_of_token
    [B, T_ph], params [B, 6] integers (inc as uint32 or its int32 image), note_depth_q None or [B, T_ph], lengths None (the count of non-zero frames of mel2ph)
    or B integers.  offset_q int64 [B, T];  curve_out fp64 [B, T]: the curve itself where the offset is 0 inside the row, log2((2^x - 1) 2^(offset_q / 19200) +
    1) in double elsewhere, 0 beyond the row.  Written from the rule, used only by the tests."""
    x = np.asarray(curve, dtype=np.float64)
    m2p, notes, prm = np.asarray(mel2ph, dtype=np.int64), np.asarray(note_of_token, dtype=np.int64), np.asarray(params, dtype=np.int64)
    B, T = m2p.shape
    T_ph = notes.shape[1]
    tab = sine_table().astype(np.int64)
    lens = (m2p > 0).sum(axis=1) if lengths is None else [max(0, min(int(v), T)) for v in lengths]
    off = np.zeros((B, T), np.int64)
    out = np.zeros((B, T), np.float64)
    for b in range(B):
        n_frames = int(lens[b])
        depth_item, inc, delay, attack, release, min_len = (int(v) for v in prm[b])
        depth_item, inc = min(max(depth_item, 0), DEPTH_Q_MAX), inc & 0xFFFFFFFF
        attack, release = min(max(attack, 1), RAMP_MAX), min(max(release, 1), RAMP_MAX)
        delay, min_len = min(max(delay, 0), DELAY_MAX), min(max(min_len, 0), DELAY_MAX)
        tok = np.clip(m2p[b, :n_frames], 0, T_ph)
        n = np.where(tok > 0, notes[b, np.maximum(tok, 1) - 1], 0)
        bounds = [0] + [s for s in range(1, n_frames) if n[s] != n[s - 1]] + [n_frames]
        for start, end in zip(bounds[:-1], bounds[1:]):
            if end <= start or n[start] == 0 or end - start < min_len:
                continue
            depth = depth_item
            if note_depth_q is not None and int(note_depth_q[b][tok[start] - 1]) >= 0:
                depth = min(int(note_depth_q[b][tok[start] - 1]), DEPTH_Q_MAX)
            t = np.arange(start + delay, end, dtype=np.int64)
            if depth == 0 or len(t) == 0:
                continue
            p = t - start - delay
            ph = (inc * p) & 0xFFFFFFFF
            i, f = ph >> 22, (ph >> 6) & 0xFFFF
            s = tab[i] + (((tab[i + 1] - tab[i]) * f) >> 16)                  # (numpy's >> on a signed integer is arithmetic: floor)
            v = [depth * int(sv) * min(int(pv), attack) * min(end - int(tv), release) for sv, pv, tv in zip(s, p, t)]      # Python integers: no overflow
            den = SINE_SCALE * attack * release
            off[b, t] = [(abs(w) + den // 2) // den * (1 if w >= 0 else -1) for w in v]
        out[b, :n_frames] = x[b, :n_frames]
        on = off[b] != 0
        out[b, on] = np.log2((np.exp2(x[b, on]) - 1.0) * np.exp2(off[b, on] / float(UNITS_PER_OCTAVE)) + 1.0)
    return off, out
