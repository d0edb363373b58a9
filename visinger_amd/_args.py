"""Host-argument rules of the control ops (pitch, timing, pitch_track, guide_align, guide_correct) and of the waveform ops (resample, dynamics, limiter), written
once: the key check of a keyword dict, the waveform and `out=` checks, the per-device cache of a host table.  A per-item value comes
as host numbers -- checked here, ValueError, and copied to the device -- or as a GPU tensor, which is checked for kind only (VisingerHipError), used as it
is and never read back: a captured graph replays on other values by overwriting that tensor."""
import ctypes
import math
import numbers

import torch

from ._lib import VisingerHipError


def vp(t):
    """device pointer of a tensor of any dtype (None -> NULL); _lib.ptr is the checked fp32 form"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def is_int(v, lo, hi):
    """an integer, no bool, in [lo, hi] (the exact type first: the abstract-class test is the slow part, and the checks run in front of every launch)"""
    return (type(v) is int or (isinstance(v, numbers.Integral) and not isinstance(v, bool))) and lo <= v <= hi


def is_real(v, lo=-math.inf, hi=math.inf):
    """a real number, no bool, finite and in [lo, hi]"""
    return (type(v) is float or type(v) is int or (isinstance(v, numbers.Real) and not isinstance(v, bool))) and lo <= v <= hi and math.isfinite(v)


def short(vals):
    return vals if len(vals) <= 8 else vals[:8] + ["..."]


def gpu_tensor(who, name, t, dtype, shape):
    """t.contiguous() of a GPU tensor of this dtype and shape; VisingerHipError for anything else.  None stands for a size that is free; free sizes come
    last, so that the test is one comparison (it runs in front of every launch)"""
    if torch.is_tensor(t) and t.is_cuda and t.dtype == dtype:
        have, free = tuple(t.shape), shape.index(None) if None in shape else None
        if have == shape if free is None else (len(have) == len(shape) and have[:free] == shape[:free]):
            return t.contiguous()
    want = ", ".join("*" if s is None else str(s) for s in shape)
    raise VisingerHipError(f"{who}: {name} must be a {dtype} tensor [{want}] on the GPU (there is no CPU path), got {t!r:.80}")


def keys(name, given, allowed, none_ok=False):
    """a copy of the dict `given` whose keys are all among `allowed` (any container of names; a dict lists its keys); ValueError for anything that is no
    dict and for an unknown key.  none_ok: None is passed on"""
    if type(given) is dict or isinstance(given, dict):                 # (the exact type first, as in is_int)
        for k in given:
            if k not in allowed:
                raise ValueError(f"{name} takes {', '.join(allowed)}, got {sorted(given, key=str)}")
        return given.copy()
    if given is None and none_ok:
        return None
    raise ValueError(f"{name} must be a dict{' or None' if none_ok else ''} (keys: {', '.join(allowed)}), got {given!r:.60}")


def waveform(who, wav):
    """(wav.contiguous(), B, L) of an fp32 GPU tensor [B, L] with B > 0 and 0 < L < 2^31; VisingerHipError for anything else"""
    wav = gpu_tensor(who, "wav", wav, torch.float32, (None, None))
    B, n = wav.shape
    if B == 0 or n == 0 or n >= 1 << 31:
        raise VisingerHipError(f"{who}: B > 0 and 0 < L < 2^31 are required, got {(B, n)}")
    return wav, B, n


def out_like(who, wav, out):
    """the tensor a waveform op writes: a new one for None; wav itself or a contiguous fp32 GPU tensor of wav's shape is passed on; VisingerHipError otherwise"""
    if out is None:
        return torch.empty_like(wav)
    if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == wav.shape and out.is_contiguous()):
        raise VisingerHipError(f"{who}: out must be a contiguous fp32 GPU tensor of wav's shape {tuple(wav.shape)}, got {out!r:.80}")
    return out


_tables = {}


def device_table(device, key, make):
    """the device copy of the host table make() -- a numpy array -- on `device`: one per (device, key), made on first use and kept"""
    dev = torch.device(device)
    k = (dev.type, torch.cuda.current_device() if dev.index is None else dev.index, key)
    t = _tables.get(k)
    if t is None:
        t = _tables[k] = torch.from_numpy(make().copy()).to(dev)
    return t


def per_item_f32(what, value, B, device, positive=False):
    """fp32 [B] on the device: a number (every item), a sequence of B numbers -- finite, with `positive` also > 0 -- or an fp32 GPU tensor [B]"""
    if torch.is_tensor(value) and value.is_cuda:
        if not (value.dtype == torch.float32 and tuple(value.shape) == (B,)):
            raise VisingerHipError(f"{what} as a GPU tensor must be fp32 [{B}], got {value.dtype} {tuple(value.shape)}")
        return value.contiguous()
    if torch.is_tensor(value):
        value = value.tolist()
    if isinstance(value, str):
        raise ValueError(f"{what} must be numbers, got {value!r}")
    vals = [float(value)] * B if isinstance(value, numbers.Real) else [float(v) for v in value]
    if len(vals) != B:
        raise ValueError(f"{len(vals)} {what} for a batch of {B}")
    if not all(math.isfinite(v) and (v > 0 or not positive) for v in vals):
        raise ValueError(f"{what} must be finite numbers{' > 0' if positive else ''}, got {short(vals)}")
    return torch.tensor(vals, dtype=torch.float32).to(device)


def lengths_i64(who, name, value, B, upper, device):
    """int64 [B] on the device, or None: None, a host sequence of B integers in [0, upper], or an int64 GPU tensor [B]"""
    if value is None:
        return None
    if torch.is_tensor(value) and value.is_cuda:
        if not (value.dtype == torch.int64 and tuple(value.shape) == (B,)):
            raise VisingerHipError(f"{who}: {name} as a GPU tensor must be int64 [{B}], got {value.dtype} {tuple(value.shape)}")
        return value.contiguous()
    vals = [int(v) for v in (value.tolist() if torch.is_tensor(value) else value)]
    if len(vals) != B or not all(0 <= v <= upper for v in vals):
        raise ValueError(f"{who}: {name} must be {B} integers in [0, {upper}], got {short(vals)}")
    return torch.tensor(vals, dtype=torch.int64).to(device)
