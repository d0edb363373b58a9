"""Pitch tracking on the device (csrc/pitch_track.hip): a batch of recordings becomes the per-frame f0 curve the rest of the library
speaks -- Hz, 0 = unvoiced, one value per hop -- as ``VISinger.forward(f0_hz=)``, items with ``"f0"`` and ``timing.retime(curve=)`` take it.  The
reference extracts f0 offline, one file at a time on the host, through ``parselmouth`` or ``pyworld`` (``utils/audio/pitch_extractors.py``); neither is
reproduced.  This is YIN (de Cheveigne & Kawahara 2002) with a lag-centred difference function, fully specified in include/visinger_hip.h "f6".

Everything that changes between two calls -- the samples, the lengths -- is read from device tensors; with a device ``lengths`` and ``frames=`` nothing
is read on the host, so a captured graph replays on another recording by overwriting those buffers.  GPU tensors only; there is no CPU path and no
backward (a recording is data: an input that requires grad is refused while autograd records).

``extract_f0`` decides every frame on its own.  With ``path=`` (include/visinger_hip.h "f12") a frame keeps up to seven lag candidates
(``candidates``: vs_f0_candidates, the local minima of the same d' row below a gate) and a Viterbi path over the phrase chooses among them (``best_path``:
vs_f0_path, csrc/pitch_path.hip): a weak fundamental no longer costs a few frames an octave up, a d' near the threshold no longer makes the voicing flicker."""
import math
import numbers

import torch

from . import _args as A
from . import _lib as L

TAU_LIMIT = 1024             # vs_f0_yin: ceil(sample_rate / f0_min)
WINDOW_LIMIT = 2048          # ... and the window
PATH_FRAMES_LIMIT = 32768    # vs_f0_path: frames of an item (VS_F0_PATH_MAX_FRAMES: 4 bytes of LDS a frame)
PATH_WEIGHT_LIMIT = 4096
SLOTS = 8                    # candidate slots a frame: 0 .. 6 hold lags, 7 is the unvoiced state's and always empty
PATH_DEFAULTS = dict(gate=0.5, w_unvoiced=160, w_switch=96, w_order=24, w_jump=32, jump_cap=384)


def lag_range(sample_rate, f0_min, f0_max):
    """(tau_min, tau_max) as vs_f0_yin derives them"""
    return max(2, math.floor(sample_rate / f0_max)), math.ceil(sample_rate / f0_min)


def check_path(gate=0.5, w_unvoiced=160, w_switch=96, w_order=24, w_jump=32, jump_cap=384):
    """ValueError for host values vs_f0_candidates (gate) and vs_f0_path (the weights) would refuse; returns (gate, the six ints of the C call -- the last one is
    reserved: 0)"""
    if not (A.is_real(gate) and gate > 0):
        raise ValueError(f"gate must be a finite number > 0, got {gate!r}")
    weights = (("w_unvoiced", w_unvoiced), ("w_switch", w_switch), ("w_order", w_order), ("w_jump", w_jump), ("jump_cap", jump_cap))
    for name, v in weights:
        if not A.is_int(v, 0, PATH_WEIGHT_LIMIT):
            raise ValueError(f"{name} must be an integer in [0, {PATH_WEIGHT_LIMIT}], got {v!r}")
    return float(gate), tuple(int(v) for _, v in weights) + (0,)


def check_args(hop_size, sample_rate, f0_min=65.0, f0_max=1000.0, window=None, threshold=0.15, silence=1e-8, frames=None, *, path=None):
    """ValueError for host values vs_f0_yin would refuse (with path -- None or a dict of PATH_DEFAULTS keys -- also those of check_path); returns the window W"""
    if path is not None:
        check_path(**A.keys("path", path, PATH_DEFAULTS))
    for name, v in (("hop_size", hop_size), ("sample_rate", sample_rate)):
        if not A.is_int(v, 1, (1 << 31) - 1):
            raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    for name, v in (("f0_min", f0_min), ("f0_max", f0_max), ("threshold", threshold)):
        if not (isinstance(v, numbers.Real) and math.isfinite(v) and v > 0):
            raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
    if not f0_min < f0_max:
        raise ValueError(f"f0_min = {f0_min} must be below f0_max = {f0_max}")
    if not (isinstance(silence, numbers.Real) and silence >= 0):
        raise ValueError(f"silence must be a number >= 0, got {silence!r}")
    tau_min, tau_max = lag_range(sample_rate, f0_min, f0_max)
    if tau_max > TAU_LIMIT or tau_min >= tau_max:
        raise ValueError(f"the lag range [{tau_min}, {tau_max}] of {f0_min} .. {f0_max} Hz at {sample_rate} Hz must be non-empty and end at or below {TAU_LIMIT}")
    if window is not None and not A.is_int(window, tau_max, WINDOW_LIMIT):
        raise ValueError(f"window must be an integer in [tau_max = {tau_max}, {WINDOW_LIMIT}], got {window!r}")
    W = 2 * tau_max if window is None else int(window)
    if W > WINDOW_LIMIT:
        raise ValueError(f"the default window 2 * tau_max = {W} exceeds {WINDOW_LIMIT}: give window=")
    if frames is not None and not (isinstance(frames, numbers.Integral) and 1 <= frames < 1 << 31):
        raise ValueError(f"frames must be an integer in [1, 2^31), got {frames!r}")
    return W


def _recordings(who, wav, hop_size, lengths, frames):
    """(wav fp32 [B, L] contiguous, B, L, lengths int64 [B] on the device or None, T) of extract_f0's and candidates' tensor arguments"""
    if not (torch.is_tensor(wav) and wav.is_cuda and wav.is_floating_point() and wav.dim() in (1, 2)):
        raise L.VisingerHipError(f"{who}: wav must be a float tensor [B, L] or [L] on the GPU (there is no CPU path), got {wav!r:.80}")
    if torch.is_grad_enabled() and wav.requires_grad:
        raise L.VisingerHipError(f"{who}: wav requires grad: the tracker has no backward (detach it)")
    wav = (wav[None] if wav.dim() == 1 else wav).float().contiguous()
    B, n = wav.shape
    if B == 0 or n == 0 or n >= 1 << 31:
        raise L.VisingerHipError(f"{who}: B > 0 and 0 < L < 2^31 are required, got {(B, n)}")
    lengths = A.lengths_i64(who, "lengths", lengths, B, n, wav.device)
    T = n // int(hop_size) if frames is None else int(frames)
    if T < 1:
        raise ValueError(f"a recording of {n} samples has no frame of {hop_size}: give at least hop_size samples (or frames=)")
    return wav, B, n, lengths, T


def candidates(wav, hop_size, sample_rate, f0_min=65.0, f0_max=1000.0, lengths=None, window=None, silence=1e-8, frames=None, gate=0.5):
    """(cand_hz, cand_d), fp32 [B, T, 8]: the lag candidates of every frame of recordings wav -- the local minima of YIN's d' below `gate`, ascending in lag, the
    first seven of a frame in slots 0 .. 6 as a frequency in Hz (the parabola of extract_f0) and the d' there; an empty slot holds hz = 0, d = 1 (slot 7 always;
    every slot of a silent frame and of a frame beyond the row).  The other arguments are extract_f0's.  One launch (vs_f0_candidates)."""
    check_args(hop_size, sample_rate, f0_min, f0_max, window, 0.15, silence, frames, path=dict(gate=gate))
    wav, B, n, lengths, T = _recordings("candidates", wav, hop_size, lengths, frames)
    lib = L.require_gpu()
    cand_hz = torch.empty((B, T, SLOTS), device=wav.device, dtype=torch.float32)
    cand_d = torch.empty_like(cand_hz)
    L.check(lib.vs_f0_candidates(L.ptr(wav), A.vp(lengths), B, n, int(sample_rate), int(hop_size), float(f0_min), float(f0_max),
                                 0 if window is None else int(window), float(gate), float(silence), L.ptr(cand_hz), L.ptr(cand_d), T, L.stream_ptr()))
    return cand_hz, cand_d


def best_path(cand_hz, cand_d, n_frames=None, return_state=False, return_cost=False, **weights):
    """f0_hz fp32 [B, T]: the cheapest path through the candidates of `candidates` -- fp32 GPU tensors [B, T, 8] -- by vs_f0_path (the rule: include/visinger_hip.h
    "f12"); with return_state also the state of every frame (int32 [B, T]: the slot 0 .. 6, 7 = unvoiced, -1 beyond the row), with return_cost the path's
    cost (int32 [B]), in that order.  n_frames: None (every row is T long), a host sequence of B integers in [0, T], or an int64 GPU tensor [B] -- used as it is,
    never read back.  weights: w_unvoiced, w_switch, w_order, w_jump, jump_cap (PATH_DEFAULTS), integers in [0, 4096].
    ValueError for host values out of range, VisingerHipError for tensors of the wrong kind or more than 32768 frames; both before any launch."""
    _, w = check_path(**A.keys("best_path", weights, [k for k in PATH_DEFAULTS if k != "gate"]))
    cand_hz = A.gpu_tensor("best_path", "cand_hz", cand_hz, torch.float32, (None, None, None))
    B, T, slots = cand_hz.shape
    cand_d = A.gpu_tensor("best_path", "cand_d", cand_d, torch.float32, (B, T, slots))
    if B < 1 or not 1 <= T <= PATH_FRAMES_LIMIT or slots != SLOTS:
        raise L.VisingerHipError(f"best_path: candidates [B >= 1, 1 <= T <= {PATH_FRAMES_LIMIT}, {SLOTS}] are required, got {(B, T, slots)}")
    n_frames = A.lengths_i64("best_path", "n_frames", n_frames, B, T, cand_hz.device)
    lib = L.require_gpu()
    f0 = torch.empty((B, T), device=cand_hz.device, dtype=torch.float32)
    state = torch.empty((B, T), device=cand_hz.device, dtype=torch.int32) if return_state else None
    cost = torch.empty((B,), device=cand_hz.device, dtype=torch.int32) if return_cost else None
    L.check(lib.vs_f0_path(L.ptr(cand_hz), L.ptr(cand_d), A.vp(n_frames), B, T, *w, L.ptr(f0), A.vp(state), A.vp(cost), L.stream_ptr()))
    out = (f0,) + ((state,) if return_state else ()) + ((cost,) if return_cost else ())
    return out if len(out) > 1 else f0


def _extract_path(wav, hop_size, sample_rate, f0_min, f0_max, lengths, window, silence, frames, return_periodicity, path):
    """extract_f0(path=): candidates, then the path over each row's lengths // hop_size frames (formed on the device)"""
    opts = dict(PATH_DEFAULTS, **path)
    wav, B, n, lengths, T = _recordings("extract_f0", wav, hop_size, lengths, frames)
    if T > PATH_FRAMES_LIMIT:
        raise ValueError(f"path tracking takes at most {PATH_FRAMES_LIMIT} frames a row, got {T}: split the recording (or track it without path)")
    cand_hz, cand_d = candidates(wav, hop_size, sample_rate, f0_min, f0_max, lengths, window, silence, T, opts.pop("gate"))
    if lengths is None:
        n_frames = torch.full((B,), n // int(hop_size), device=wav.device, dtype=torch.int64)
    else:
        n_frames = torch.div(lengths.clamp(0, n), int(hop_size), rounding_mode="floor")
    if not return_periodicity:
        return best_path(cand_hz, cand_d, n_frames, **opts)
    f0, state = best_path(cand_hz, cand_d, n_frames, return_state=True, **opts)
    chosen = torch.gather(cand_d, 2, state.clamp(0, SLOTS - 1).long()[..., None])[..., 0]
    return f0, torch.where(f0 > 0, (1.0 - chosen).clamp(0.0, 1.0), torch.zeros_like(f0))


def extract_f0(wav, hop_size, sample_rate, f0_min=65.0, f0_max=1000.0, lengths=None, window=None, threshold=0.15, silence=1e-8, frames=None,
               return_periodicity=False, path=None):
    """f0_hz fp32 [B, T] (with return_periodicity also the periodicity, fp32 [B, T] in [0, 1]) of recordings wav: a float GPU tensor [B, L], or [L]
    taken as one row (fp32 is used as it is, other float types are converted).  Frame t is centred on sample t * hop_size + hop_size // 2; row b has
    lengths[b] // hop_size frames, the rest of it comes back 0.
    lengths: None (every row is L long), a host sequence of B integers, or an int64 GPU tensor [B] -- used as it is, never read back (the kernel clamps
    it to [0, L]).  frames=None: T = L // hop_size; otherwise the result is `frames` wide (graph capture: a capacity).
    f0_min, f0_max: the search range in Hz (ceil(sample_rate / f0_min) <= 1024);  window: samples per difference sum, None = 2 * ceil(sample_rate / f0_min),
    at most 2048;  threshold: YIN's absolute threshold on d';  silence: a frame whose mean square is at or below it is unvoiced.
    path: None -- every frame is decided on its own (vs_f0_yin) -- or a dict of PATH_DEFAULTS keys, possibly empty: the curve is the cheapest path through the
    frames' lag candidates (candidates, then best_path over lengths // hop_size frames, at most 32768 a row); threshold is then not used, and the periodicity
    is 1 - d' of the chosen candidate, 0 where the path is unvoiced.
    ValueError for host values out of range, VisingerHipError for tensors of the wrong kind; both before any launch."""
    check_args(hop_size, sample_rate, f0_min, f0_max, window, threshold, silence, frames, path=path)
    if path is not None:
        return _extract_path(wav, hop_size, sample_rate, f0_min, f0_max, lengths, window, silence, frames, return_periodicity, path)
    if not (torch.is_tensor(wav) and wav.is_cuda and wav.is_floating_point() and wav.dim() in (1, 2)):
        raise L.VisingerHipError(f"extract_f0: wav must be a float tensor [B, L] or [L] on the GPU (there is no CPU path), got {wav!r:.80}")
    if torch.is_grad_enabled() and wav.requires_grad:
        raise L.VisingerHipError("extract_f0: wav requires grad: the tracker has no backward (detach it)")
    wav = (wav[None] if wav.dim() == 1 else wav).float().contiguous()
    B, n = wav.shape
    if B == 0 or n == 0 or n >= 1 << 31:
        raise L.VisingerHipError(f"extract_f0: B > 0 and 0 < L < 2^31 are required, got {(B, n)}")
    lengths = A.lengths_i64("extract_f0", "lengths", lengths, B, n, wav.device)
    T = n // int(hop_size) if frames is None else int(frames)
    if T < 1:
        raise ValueError(f"a recording of {n} samples has no frame of {hop_size}: give at least hop_size samples (or frames=)")
    lib = L.require_gpu()
    f0 = torch.empty((B, T), device=wav.device, dtype=torch.float32)
    per = torch.empty_like(f0) if return_periodicity else None
    L.check(lib.vs_f0_yin(L.ptr(wav), A.vp(lengths), B, n, int(sample_rate), int(hop_size), float(f0_min),
                          float(f0_max), 0 if window is None else int(window), float(threshold), float(silence), L.ptr(f0), L.ptr(per), T, L.stream_ptr()))
    return (f0, per) if return_periodicity else f0
