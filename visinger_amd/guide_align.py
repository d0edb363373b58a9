"""Guide alignment on the device (csrc/guide_align.hip): the score timed to a recording.  ``pitch_track.extract_f0`` turns a recording
into a guide curve on the recording's own timeline; this decides which of its frames belong to which token of the score -- a monotonic Viterbi
alignment of the quantised curve against the score's note pitches, fully specified in include/visinger_hip.h "f7" -- and returns new frames per token.
``timing.retime(dur=dur_new)`` makes the alignment of them, and the curve is then a guide on that alignment as it is: the score is sung with the
recording's timing and the recording's pitch.  The reference has no counterpart (its inference replays the score's own timing).

Everything that changes between two calls -- the curve, its length, the note pitches, the durations, the offset -- is read from device tensors, so a
captured graph replays on another guide by overwriting those buffers.  GPU tensors only; there is no CPU path and no backward (an alignment is data)."""
import ctypes
import numbers

import torch

from . import _lib as L

T_PH_LIMIT = 1024            # vs_guide_align: tokens (one column of the recurrence per lane of a workgroup)
TG_LIMIT = 65536             # ... and guide frames
WEIGHT_LIMIT = 4096
LDS_WORDS = 5120             # VS_GUIDE_ALIGN_LDS_WORDS: backpointer words a workgroup keeps in LDS; beyond it they go to a workspace
DEFAULTS = dict(octave_fold=False, cap=64, w_voiced_rest=48, w_unvoiced_note=24, drift=32, drift_cap=64)


def check_args(octave_fold=False, cap=64, w_voiced_rest=48, w_unvoiced_note=24, drift=32, drift_cap=64):
    """ValueError for host values vs_guide_align would refuse; returns the seven ints of the C call (the last one is reserved: 0)"""
    if not isinstance(octave_fold, (bool, numbers.Integral)) or octave_fold not in (0, 1):
        raise ValueError(f"octave_fold must be False or True, got {octave_fold!r}")
    weights = (("cap", cap), ("w_voiced_rest", w_voiced_rest), ("w_unvoiced_note", w_unvoiced_note), ("drift", drift), ("drift_cap", drift_cap))
    for name, v in weights:
        if not (isinstance(v, numbers.Integral) and not isinstance(v, bool) and 0 <= v <= WEIGHT_LIMIT):
            raise ValueError(f"{name} must be an integer in [0, {WEIGHT_LIMIT}], got {v!r}")
    return tuple(int(v) for _, v in weights) + (int(octave_fold), 0)


def workspace_bytes(B, Tg, T_ph):
    """bytes of backpointer workspace vs_guide_align needs for this shape: 0 when every item fits the LDS"""
    words_row = -(-T_ph // 64)
    return B * Tg * words_row * 8 if Tg * words_row > LDS_WORDS else 0


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def align_guide(f0_hz, note_midi, dur=None, mel2ph=None, guide_lengths=None, offset_cents=None, octave_fold=False, cap=64, w_voiced_rest=48,
                w_unvoiced_note=24, drift=32, drift_cap=64):
    """(dur_new, cost, status): int64 [B, T_ph] frames of the guide per token, int32 [B] the alignment's cost, int32 [B] 0 = aligned, 1 = not
    (no token with frames, or fewer guide frames than tokens with frames: dur_new is then max(dur, 0) and cost -1).
    f0_hz: fp32 GPU [B, Tg], the guide curve in Hz on its own timeline (0, negative, NaN, inf = unvoiced);  note_midi: fp32 GPU [B, T_ph], the score pitch
    of each token as a MIDI number (fractions allowed; not finite or <= 0 = a rest: rests and padding);  exactly one of dur -- int64 GPU [B, T_ph], score
    frames per token -- and mel2ph -- int64 GPU [B, T] (through ops.mel2token_to_dur);  guide_lengths: None (every row is Tg long), a host sequence of B
    integers in [0, Tg], or an int64 GPU tensor [B] -- used as it is, never read back;  offset_cents: None, a number, a sequence of B numbers, or an fp32
    GPU tensor [B]: the guide's transposition against the score (a guide sung a tone below the score: -200).  The weights: see check_args and "f7".
    Where status is 0, dur_new sums to the row's guide length and every token that had frames keeps at least one.
    ValueError for host values out of range, VisingerHipError for tensors of the wrong kind; both before any launch."""
    weights = check_args(octave_fold, cap, w_voiced_rest, w_unvoiced_note, drift, drift_cap)
    if not (torch.is_tensor(f0_hz) and f0_hz.is_cuda and f0_hz.dtype == torch.float32 and f0_hz.dim() == 2):
        raise L.VisingerHipError(f"align_guide: f0_hz must be an fp32 tensor [B, Tg] on the GPU (there is no CPU path), got {f0_hz!r:.80}")
    B, Tg = f0_hz.shape
    if not (torch.is_tensor(note_midi) and note_midi.is_cuda and note_midi.dtype == torch.float32 and note_midi.dim() == 2 and note_midi.shape[0] == B):
        raise L.VisingerHipError(f"align_guide: note_midi must be an fp32 tensor [{B}, T_ph] on the GPU, got {note_midi!r:.80}")
    T_ph = note_midi.shape[1]
    if (dur is None) == (mel2ph is None):
        raise L.VisingerHipError("align_guide: give exactly one of dur and mel2ph")
    src = dur if mel2ph is None else mel2ph
    if not (torch.is_tensor(src) and src.is_cuda and src.dtype == torch.int64 and src.dim() == 2 and src.shape[0] == B and
            (mel2ph is not None or src.shape[1] == T_ph)):
        raise L.VisingerHipError(f"align_guide: {'dur' if mel2ph is None else 'mel2ph'} must be an int64 tensor [{B}, {T_ph if mel2ph is None else 'T'}] on the GPU, "
                                 f"got {src!r:.80}")
    if B < 1 or not 1 <= T_ph <= T_PH_LIMIT or not 1 <= Tg <= TG_LIMIT or (mel2ph is not None and src.shape[1] < 1):
        raise L.VisingerHipError(f"align_guide: B >= 1, 1 <= T_ph <= {T_PH_LIMIT} and 1 <= Tg <= {TG_LIMIT} are required, got B = {B}, T_ph = {T_ph}, Tg = {Tg}")
    dev = f0_hz.device
    if torch.is_tensor(guide_lengths) and guide_lengths.is_cuda:
        if not (guide_lengths.dtype == torch.int64 and tuple(guide_lengths.shape) == (B,)):
            raise L.VisingerHipError(f"align_guide: guide_lengths as a GPU tensor must be int64 [{B}], got {guide_lengths.dtype} {tuple(guide_lengths.shape)}")
        guide_lengths = guide_lengths.contiguous()
    elif guide_lengths is not None:
        vals = [int(v) for v in (guide_lengths.tolist() if torch.is_tensor(guide_lengths) else guide_lengths)]
        if len(vals) != B or not all(0 <= v <= Tg for v in vals):
            raise ValueError(f"guide_lengths must be {B} integers in [0, {Tg}], got {vals if len(vals) <= 8 else vals[:8] + ['...']}")
        guide_lengths = torch.tensor(vals, dtype=torch.int64).to(dev)
    if torch.is_tensor(offset_cents) and offset_cents.is_cuda:
        if not (offset_cents.dtype == torch.float32 and tuple(offset_cents.shape) == (B,)):
            raise L.VisingerHipError(f"align_guide: offset_cents as a GPU tensor must be fp32 [{B}], got {offset_cents.dtype} {tuple(offset_cents.shape)}")
        offset_cents = offset_cents.contiguous()
    elif offset_cents is not None:
        if torch.is_tensor(offset_cents):
            offset_cents = offset_cents.tolist()
        vals = [float(offset_cents)] * B if isinstance(offset_cents, numbers.Real) else [float(v) for v in offset_cents]
        if len(vals) != B or not all(abs(v) < float("inf") for v in vals):
            raise ValueError(f"offset_cents must be a finite number, or {B} of them, got {vals if len(vals) <= 8 else vals[:8] + ['...']}")
        offset_cents = torch.tensor(vals, dtype=torch.float32).to(dev)
    lib = L.require_gpu()
    f0_hz, note_midi = f0_hz.contiguous(), note_midi.contiguous()
    if mel2ph is not None:
        from . import ops
        dur = ops.mel2token_to_dur(mel2ph, T_ph)
    dur = dur.contiguous()
    dur_new = torch.empty((B, T_ph), device=dev, dtype=torch.int64)
    cost, status = torch.empty((B,), device=dev, dtype=torch.int32), torch.empty((B,), device=dev, dtype=torch.int32)
    need = workspace_bytes(B, Tg, T_ph)
    work = torch.empty((need // 8,), device=dev, dtype=torch.int64) if need else None      # (torch's allocator: stream-aware, kept by a capture's pool)
    L.check(lib.vs_guide_align(L.ptr(f0_hz), _vp(guide_lengths), L.ptr(note_midi), _vp(dur), L.ptr(offset_cents), *weights, _vp(dur_new), _vp(cost),
                               _vp(status), _vp(work), need, B, Tg, T_ph, L.stream_ptr()))
    return dur_new, cost, status
