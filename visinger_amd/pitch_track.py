"""Pitch tracking on the device (csrc/pitch_track.hip): a batch of recordings becomes the per-frame f0 curve the rest of the library
speaks -- Hz, 0 = unvoiced, one value per hop -- as ``VISinger.forward(f0_hz=)``, items with ``"f0"`` and ``timing.retime(curve=)`` take it.  The
reference extracts f0 offline, one file at a time on the host, through ``parselmouth`` or ``pyworld`` (``utils/audio/pitch_extractors.py``); neither is
reproduced.  This is YIN (de Cheveigne & Kawahara 2002) with a lag-centred difference function, fully specified in include/visinger_hip.h "f6".

Everything that changes between two calls -- the samples, the lengths -- is read from device tensors; with a device ``lengths`` and ``frames=`` nothing
is read on the host, so a captured graph replays on another recording by overwriting those buffers.  GPU tensors only; there is no CPU path and no
backward (a recording is data: an input that requires grad is refused while autograd records)."""
import math
import numbers

import torch

from . import _args as A
from . import _lib as L

TAU_LIMIT = 1024             # vs_f0_yin: ceil(sample_rate / f0_min)
WINDOW_LIMIT = 2048          # ... and the window


def lag_range(sample_rate, f0_min, f0_max):
    """(tau_min, tau_max) as vs_f0_yin derives them"""
    return max(2, math.floor(sample_rate / f0_max)), math.ceil(sample_rate / f0_min)


def check_args(hop_size, sample_rate, f0_min=65.0, f0_max=1000.0, window=None, threshold=0.15, silence=1e-8, frames=None):
    """ValueError for host values vs_f0_yin would refuse; returns the window W"""
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


def extract_f0(wav, hop_size, sample_rate, f0_min=65.0, f0_max=1000.0, lengths=None, window=None, threshold=0.15, silence=1e-8, frames=None,
               return_periodicity=False):
    """f0_hz fp32 [B, T] (with return_periodicity also the periodicity, fp32 [B, T] in [0, 1]) of recordings wav: a float GPU tensor [B, L], or [L]
    taken as one row (fp32 is used as it is, other float types are converted).  Frame t is centred on sample t * hop_size + hop_size // 2; row b has
    lengths[b] // hop_size frames, the rest of it comes back 0.
    lengths: None (every row is L long), a host sequence of B integers, or an int64 GPU tensor [B] -- used as it is, never read back (the kernel clamps
    it to [0, L]).  frames=None: T = L // hop_size; otherwise the result is `frames` wide (graph capture: a capacity).
    f0_min, f0_max: the search range in Hz (ceil(sample_rate / f0_min) <= 1024);  window: samples per difference sum, None = 2 * ceil(sample_rate / f0_min),
    at most 2048;  threshold: YIN's absolute threshold on d';  silence: a frame whose mean square is at or below it is unvoiced.
    ValueError for host values out of range, VisingerHipError for tensors of the wrong kind; both before any launch."""
    check_args(hop_size, sample_rate, f0_min, f0_max, window, threshold, silence, frames)
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
