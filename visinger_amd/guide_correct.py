"""Guide pitch correction on the device (csrc/guide_correct.hip): a tracked guide curve pulled onto the score it was sung to.
``pitch_track.extract_f0`` delivers a recording's pitch exactly as it was sung -- flat notes, slow drift, octave slips of the tracker and all.  This takes the
slow part of the curve's deviation from each note out (its mean over a window inside the note) and keeps, scales or removes the fast part (vibrato, scoops,
jitter); the rule is fully specified in include/visinger_hip.h "f8".  ``guide_deviation`` gives the median deviation of a curve from its score: the key the
guide was sung in.  The reference has no counterpart (its pitch tools are offline host programs).

Everything that changes between two calls -- the curve, its length, the alignment, the note pitches, the offset -- is read from device tensors, so a captured
graph replays on another guide by overwriting those buffers.  GPU tensors only; there is no CPU path and no backward."""
import torch

from . import _args as A
from . import _lib as L

TILE = 1024                  # VS_GUIDE_CORRECT_TILE: frames a workgroup of vs_guide_correct writes
T_LIMIT = 65536              # frames
T_PH_LIMIT = 1024            # tokens
WINDOW_LIMIT = 1024          # frames on each side of a frame that its slow part is the mean of
WILD_LIMIT = 1 << 18         # units of 1/16 cent
DEFAULTS = dict(window=1024, strength=1.0, vibrato=1.0, wild_cents=300.0, octave_fold=False)


def check_args(window=1024, strength=1.0, vibrato=1.0, wild_cents=300.0, octave_fold=False):
    """ValueError for host values vs_guide_correct would refuse; returns the six ints of the C call: window, strength_q = round(256 strength),
    vibrato_q = round(256 vibrato), wild = round(16 wild_cents), octave_fold and the reserved 0"""
    if not A.is_int(window, 0, WINDOW_LIMIT):
        raise ValueError(f"window must be an integer in [0, {WINDOW_LIMIT}] frames, got {window!r}")
    for name, v, top in (("strength", strength, 1.0), ("vibrato", vibrato, 2.0), ("wild_cents", wild_cents, WILD_LIMIT / 16.0)):
        if not A.is_real(v, 0, top):
            raise ValueError(f"{name} must be a number in [0, {top:g}], got {v!r}")
    if not (isinstance(octave_fold, bool) or A.is_int(octave_fold, 0, 1)):
        raise ValueError(f"octave_fold must be False or True, got {octave_fold!r}")
    return int(window), int(round(256 * float(strength))), int(round(256 * float(vibrato))), int(round(16 * float(wild_cents))), int(octave_fold), 0


def _inputs(who, f0_hz, mel2ph, note_midi, lengths, offset_cents):
    """the checked, contiguous device tensors of a call (lengths and offset_cents possibly None) and B, T, T_ph"""
    f0_hz = A.gpu_tensor(who, "f0_hz", f0_hz, torch.float32, (None, None))
    B, T = f0_hz.shape
    mel2ph = A.gpu_tensor(who, "mel2ph", mel2ph, torch.int64, (B, T))
    note_midi = A.gpu_tensor(who, "note_midi", note_midi, torch.float32, (B, None))
    T_ph = note_midi.shape[1]
    if B < 1 or not 1 <= T_ph <= T_PH_LIMIT or not 1 <= T <= T_LIMIT:
        raise L.VisingerHipError(f"{who}: B >= 1, 1 <= T_ph <= {T_PH_LIMIT} and 1 <= T <= {T_LIMIT} are required, got B = {B}, T_ph = {T_ph}, T = {T}")
    lengths = A.lengths_i64(who, "lengths", lengths, B, T, f0_hz.device)
    if offset_cents is not None:
        offset_cents = A.per_item_f32(f"{who}: offset_cents", offset_cents, B, f0_hz.device)
    return f0_hz, mel2ph, note_midi, lengths, offset_cents, B, T, T_ph


def _deviation(lib, f0_hz, mel2ph, note_midi, lengths, offset_cents, wild, octave_fold, B, T, T_ph):
    dev_med = torch.empty((B,), device=f0_hz.device, dtype=torch.int32)
    n_corr = torch.empty((B,), device=f0_hz.device, dtype=torch.int32)
    L.check(lib.vs_guide_deviation(L.ptr(f0_hz), A.vp(lengths), A.vp(mel2ph), L.ptr(note_midi), L.ptr(offset_cents), wild, octave_fold, A.vp(dev_med), A.vp(n_corr),
                                   B, T, T_ph, L.stream_ptr()))
    return dev_med, n_corr


def guide_deviation(f0_hz, mel2ph, note_midi, lengths=None, offset_cents=None, wild_cents=300.0, octave_fold=False):
    """(dev_med, n_corr): int32 [B] each -- the lower median of the curve's deviation from its score over the correctable frames, in units of 1/16 cent
    (0 when there are none), and their number.  With offset_cents=None and a large wild_cents, dev_med / 16 is the guide's transposition against the score
    in cents.  The arguments are correct_guide's (offset_cents: not 'auto')."""
    _, _, _, wild, fold, _ = check_args(wild_cents=wild_cents, octave_fold=octave_fold)
    f0_hz, mel2ph, note_midi, lengths, offset_cents, B, T, T_ph = _inputs("guide_deviation", f0_hz, mel2ph, note_midi, lengths, offset_cents)
    return _deviation(L.require_gpu(), f0_hz, mel2ph, note_midi, lengths, offset_cents, wild, fold, B, T, T_ph)


def correct_guide(f0_hz, mel2ph, note_midi, lengths=None, offset_cents=None, return_units=False, **params):
    """f0_out: fp32 [B, T], the corrected curve -- or (f0_out, k) with return_units: k int32 [B, T], what each frame was moved down by in units of 1/16 cent
    (f0_out = f0_hz 2^(-k / 19200); 0 where the frame was left alone, and there f0_out is f0_hz bit for bit).
    f0_hz: fp32 GPU [B, T], the guide curve in Hz on the item's own frames (0, negative, NaN, inf = unvoiced);  mel2ph: int64 GPU [B, T], the 1-based token of
    each frame, 0 = padding;  note_midi: fp32 GPU [B, T_ph], the score pitch of each token as a MIDI number (not finite or <= 0 = a rest);  lengths: None (every
    row is T long), a host sequence of B integers in [0, T], or an int64 GPU tensor [B] -- used as it is, never read back;  offset_cents: None, a number, a
    sequence of B numbers, an fp32 GPU tensor [B] -- the guide's transposition against the score (a guide sung a tone below the score: -200) -- or 'auto':
    guide_deviation with offset 0 runs first and its dev_med / 16 is the offset, a device tensor that is never read back: the guide is corrected in the key it
    was sung in.  params: window (frames on each side that the slow part is the mean of, inside the note), strength (how much of the slow part is taken out,
    0 .. 1), vibrato (the factor on the fast part, 0 .. 2), wild_cents (a frame farther than this from its note is left alone), octave_fold: see check_args
    and "f8".  ValueError for host values out of range, VisingerHipError for tensors of the wrong kind; both before any launch."""
    window, strength_q, vibrato_q, wild, fold, reserved = check_args(**A.keys("correct_guide", params, DEFAULTS))
    auto = isinstance(offset_cents, str) and offset_cents == "auto"
    f0_hz, mel2ph, note_midi, lengths, offset_cents, B, T, T_ph = _inputs("correct_guide", f0_hz, mel2ph, note_midi, lengths, None if auto else offset_cents)
    lib = L.require_gpu()
    if auto:
        offset_cents = _deviation(lib, f0_hz, mel2ph, note_midi, lengths, None, wild, fold, B, T, T_ph)[0].float() / 16
    f0_out = torch.empty_like(f0_hz)
    k = torch.empty((B, T), device=f0_hz.device, dtype=torch.int32) if return_units else None
    L.check(lib.vs_guide_correct(L.ptr(f0_hz), A.vp(lengths), A.vp(mel2ph), L.ptr(note_midi), L.ptr(offset_cents), window, strength_q, vibrato_q, wild, fold,
                                 reserved, L.ptr(f0_out), A.vp(k), B, T, T_ph, L.stream_ptr()))
    return (f0_out, k) if return_units else f0_out
