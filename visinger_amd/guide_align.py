"""Guide alignment on the device (csrc/guide_align.hip): the score timed to a recording.  ``pitch_track.extract_f0`` turns a recording
into a guide curve on the recording's own timeline; this decides which of its frames belong to which token of the score -- a monotonic Viterbi
alignment of the quantised curve against the score's note pitches, fully specified in include/visinger_hip.h "f7" -- and returns new frames per token.
``timing.retime(dur=dur_new)`` makes the alignment of them, and the curve is then a guide on that alignment as it is: the score is sung with the
recording's timing and the recording's pitch.  The reference has no counterpart (its inference replays the score's own timing).

Everything that changes between two calls -- the curve, its length, the note pitches, the durations, the offset -- is read from device tensors, so a
captured graph replays on another guide by overwriting those buffers.  GPU tensors only; there is no CPU path and no backward (an alignment is data)."""
import torch

from . import _args as A
from . import _lib as L

T_PH_LIMIT = 1024            # vs_guide_align: tokens (one column of the recurrence per lane of a workgroup)
TG_LIMIT = 65536             # ... and guide frames
WEIGHT_LIMIT = 4096
LDS_WORDS = 5120             # VS_GUIDE_ALIGN_LDS_WORDS: backpointer words a workgroup keeps in LDS; beyond it they go to a workspace
DEFAULTS = dict(octave_fold=False, cap=64, w_voiced_rest=48, w_unvoiced_note=24, drift=32, drift_cap=64)


def check_args(octave_fold=False, cap=64, w_voiced_rest=48, w_unvoiced_note=24, drift=32, drift_cap=64):
    """ValueError for host values vs_guide_align would refuse; returns the seven ints of the C call (the last one is reserved: 0)"""
    if not (isinstance(octave_fold, bool) or A.is_int(octave_fold, 0, 1)):
        raise ValueError(f"octave_fold must be False or True, got {octave_fold!r}")
    weights = (("cap", cap), ("w_voiced_rest", w_voiced_rest), ("w_unvoiced_note", w_unvoiced_note), ("drift", drift), ("drift_cap", drift_cap))
    for name, v in weights:
        if not A.is_int(v, 0, WEIGHT_LIMIT):
            raise ValueError(f"{name} must be an integer in [0, {WEIGHT_LIMIT}], got {v!r}")
    return tuple(int(v) for _, v in weights) + (int(octave_fold), 0)


def workspace_bytes(B, Tg, T_ph):
    """bytes of backpointer workspace vs_guide_align needs for this shape: 0 when every item fits the LDS"""
    words_row = -(-T_ph // 64)
    return B * Tg * words_row * 8 if Tg * words_row > LDS_WORDS else 0


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
    f0_hz = A.gpu_tensor("align_guide", "f0_hz", f0_hz, torch.float32, (None, None))
    B, Tg = f0_hz.shape
    note_midi = A.gpu_tensor("align_guide", "note_midi", note_midi, torch.float32, (B, None))
    T_ph = note_midi.shape[1]
    if (dur is None) == (mel2ph is None):
        raise L.VisingerHipError("align_guide: give exactly one of dur and mel2ph")
    if mel2ph is None:
        dur = A.gpu_tensor("align_guide", "dur", dur, torch.int64, (B, T_ph))
    else:
        mel2ph = A.gpu_tensor("align_guide", "mel2ph", mel2ph, torch.int64, (B, None))
    if B < 1 or not 1 <= T_ph <= T_PH_LIMIT or not 1 <= Tg <= TG_LIMIT or (mel2ph is not None and mel2ph.shape[1] < 1):
        raise L.VisingerHipError(f"align_guide: B >= 1, 1 <= T_ph <= {T_PH_LIMIT} and 1 <= Tg <= {TG_LIMIT} are required, got B = {B}, T_ph = {T_ph}, Tg = {Tg}")
    dev = f0_hz.device
    guide_lengths = A.lengths_i64("align_guide", "guide_lengths", guide_lengths, B, Tg, dev)
    if offset_cents is not None:
        offset_cents = A.per_item_f32("align_guide: offset_cents", offset_cents, B, dev)
    lib = L.require_gpu()
    if mel2ph is not None:
        from . import ops
        dur = ops.mel2token_to_dur(mel2ph, T_ph)
    dur_new = torch.empty((B, T_ph), device=dev, dtype=torch.int64)
    cost, status = torch.empty((B,), device=dev, dtype=torch.int32), torch.empty((B,), device=dev, dtype=torch.int32)
    need = workspace_bytes(B, Tg, T_ph)
    work = torch.empty((need // 8,), device=dev, dtype=torch.int64) if need else None      # (torch's allocator: stream-aware, kept by a capture's pool)
    L.check(lib.vs_guide_align(L.ptr(f0_hz), A.vp(guide_lengths), L.ptr(note_midi), A.vp(dur), L.ptr(offset_cents), *weights, A.vp(dur_new), A.vp(cost),
                               A.vp(status), A.vp(work), need, B, Tg, T_ph, L.stream_ptr()))
    return dur_new, cost, status
