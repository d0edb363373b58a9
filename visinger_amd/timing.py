"""Tempo and duration control of synthesis on the device (csrc/timing_ops.hip): the frame alignment ``mel2ph`` -- produced once
per utterance on the host (``align.get_note2dur``) and taken as data by the model -- is retimed by a factor per token (``stretch``) and a tempo per
item, and a curve on its timeline (a guide f0 in Hz) is warped along with it.  The reference has no length regulator: its inference replays the
score's own timing.

Everything that changes between two calls -- the alignment, the factors, the tempos, the curve -- is read from device tensors; with a capacity
``max_frames`` nothing is read back on the host, so a captured graph replays under another tempo by overwriting those buffers.  GPU tensors only;
there is no CPU path and no backward (an alignment is data).

The rule (include/visinger_hip.h "f5"): d_i = frames of token i, s_i = rint(clamp(stretch_i / tempo, 2^-6, 2^6) * 65536), new token ends
e_i = max(e_{i-1} + (d_i > 0 ? min_frames : 0), (sum_{j<=i} d_j s_j + 32768) >> 16): cumulative rounding, so the total never drifts from the
exact product by more than half a frame, and a token that had frames keeps min_frames of them however fast the tempo.  The alignment must be
monotonic over its valid prefix, as get_note2dur always produces it (not checked on the device)."""
import math

import torch

from . import _args as A
from . import _lib as L

T_FRAMES_LIMIT = 1 << 24     # vs_retime_tokens: frames of the old alignment
T_TOKENS_LIMIT = 8192        # ... and tokens (its LDS histogram)


def factor_tensor(tempo, B, device):
    """fp32 [B] on the device: a number (every item), a sequence of B numbers, or a 1-D fp32 GPU tensor [B] -- used as it is and never read back
    (the kernel treats a value that gives a non-finite factor as 1 and clamps the factor to [1/64, 64]).  Host values must be finite and > 0."""
    return A.per_item_f32("tempos", tempo, B, device, positive=True)


def stretch_tensor(stretch, B, T_ph, device):
    """fp32 [B, T_ph] on the device: an fp32 GPU tensor of that shape (used as it is, never read back), or host values [B, T_ph] (finite, > 0)"""
    if torch.is_tensor(stretch) and stretch.is_cuda:
        return A.gpu_tensor("retime", "ph_stretch", stretch, torch.float32, (B, T_ph))
    t = torch.as_tensor(stretch, dtype=torch.float32)
    if tuple(t.shape) != (B, T_ph):
        raise ValueError(f"ph_stretch has shape {tuple(t.shape)} for {B} items of {T_ph} tokens (one factor per token)")
    vals = t.flatten().tolist()
    if not all(math.isfinite(v) and v > 0 for v in vals):
        raise ValueError(f"a stretch factor must be a finite number > 0, got {A.short(vals)}")
    return t.to(device)


def retime(mel2ph=None, dur=None, T_ph=None, stretch=None, tempo=None, min_frames=1, max_frames=None, curve=None):
    """(mel2ph', lengths, curve'): the alignment retimed by stretch[b, i] / tempo[b] per token.
    mel2ph: int64 GPU [B, T] (1-based token per frame, 0 = padding, monotonic) -- or dur: int64 GPU [B, T_ph], frames per token (the
    length-regulator use); exactly one of them.  T_ph: the token count with mel2ph (default: stretch's, else mel2ph.max() read back).
    stretch: fp32 GPU [B, T_ph] or None (1);  tempo: see factor_tensor, or None (1);  min_frames: what a token that had frames keeps;
    curve: fp32 GPU [B, T_curve] on the old timeline (Hz, <= 0 = unvoiced) or None.
    max_frames=None: the result is lengths.max() frames wide -- ONE host synchronisation, like ops.mel2token_to_dur with T_txt=None.
    max_frames=N: the result is N frames wide, items are cut at N, nothing is read on the host (graph-capturable).
    Returns mel2ph' int64 [B, T'], lengths int64 [B] (on the device) and curve' fp32 [B, T'] (None without a curve)."""
    if (mel2ph is None) == (dur is None):
        raise L.VisingerHipError("retime: give exactly one of mel2ph and dur")
    src = A.gpu_tensor("retime", "mel2ph" if dur is None else "dur", mel2ph if dur is None else dur, torch.int64, (None, None))
    B = src.shape[0]
    if dur is not None:
        if T_ph is not None and T_ph != src.shape[1]:
            raise L.VisingerHipError(f"retime: T_ph = {T_ph} but dur has {src.shape[1]} tokens")
        T_ph, T_frames = src.shape[1], 0
    else:
        T_frames = src.shape[1]
        if T_ph is None:
            T_ph = stretch.shape[1] if torch.is_tensor(stretch) and stretch.dim() == 2 else int(src.max()) if src.numel() else 0
    T_ph = int(T_ph)
    if B == 0 or T_ph <= 0 or T_ph > T_TOKENS_LIMIT or (dur is None and not 0 < T_frames < T_FRAMES_LIMIT):
        raise L.VisingerHipError(f"retime: B > 0, 0 < T_ph <= {T_TOKENS_LIMIT} and 0 < T_frames < 2^24 are required, got B = {B}, T_ph = {T_ph}, T_frames = {T_frames}")
    if not 0 <= int(min_frames) <= 65536:
        raise ValueError(f"min_frames must be in [0, 65536], got {min_frames}")
    if max_frames is not None and int(max_frames) <= 0:
        raise ValueError(f"max_frames must be positive, got {max_frames}")
    dev = src.device
    stretch = None if stretch is None else stretch_tensor(stretch, B, T_ph, dev)
    tempo = None if tempo is None else factor_tensor(tempo, B, dev)
    if curve is not None:
        if not (torch.is_tensor(curve) and curve.is_cuda and curve.dim() == 2 and curve.shape[0] == B and curve.shape[1] > 0):
            raise L.VisingerHipError(f"retime: curve must be a [B, T] tensor on the GPU with B = {B}")
        curve = curve.float().contiguous()
    lib = L.require_gpu()
    cum_old = torch.empty((B, T_ph), device=dev, dtype=torch.int64)
    cum_new, lengths = torch.empty_like(cum_old), torch.empty((B,), device=dev, dtype=torch.int64)
    L.check(lib.vs_retime_tokens(A.vp(src) if dur is None else None, A.vp(src) if dur is not None else None, L.ptr(stretch), L.ptr(tempo),
                                 int(min_frames), 0 if max_frames is None else int(max_frames), A.vp(cum_old), A.vp(cum_new), A.vp(lengths), B, T_frames,
                                 T_ph, L.stream_ptr()))
    T_out = int(lengths.max()) if max_frames is None else int(max_frames)        # (None: the one synchronisation)
    out = torch.empty((B, T_out), device=dev, dtype=torch.int64)
    curve_out = None if curve is None else torch.empty((B, T_out), device=dev, dtype=torch.float32)
    if T_out > 0:
        L.check(lib.vs_retime_frames(A.vp(cum_old), A.vp(cum_new), A.vp(lengths), L.ptr(curve), 0 if curve is None else curve.shape[1], A.vp(out),
                                     L.ptr(curve_out), B, T_ph, T_out, L.stream_ptr()))
    return out, lengths, curve_out
