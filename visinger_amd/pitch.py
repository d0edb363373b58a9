"""The pitch curve of synthesis on the device (csrc/pitch_ops.hip): a guide curve in Hz becomes the model's normalised,
gap-interpolated curve (the reference's ``utils/audio/pitch/utils.py:42-57`` ``norm_interp_f0``, which runs one item at a time through
``.cpu().numpy()`` and ``np.interp``), and the frame prior's pitch condition (``models/visinger.py:129-135``) is formed in one launch, with an
optional transposition in cents per item and the sung curve back in Hz.

Everything that changes between two calls -- the curve, the lengths, the shifts -- is read from device tensors, never on the host: a captured
graph replays under another curve or another shift by overwriting those buffers.  GPU tensors only; there is no CPU path and no backward
(an input that requires grad is refused while autograd records)."""
import torch

from . import _args as A
from . import _lib as L

T_LIMIT = 1 << 24            # vs_f0_norm_interp: frame distances are exact in fp32 below it


def _rows(name, t, B=None, T=None):
    """fp32 contiguous [B, T] view of a GPU tensor holding B * T values ([B, T] or [B, 1, T])"""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise L.VisingerHipError(f"{name} must be a tensor on the GPU (there is no CPU path)")
    if t.dim() == 3 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 2 or (B is not None and tuple(t.shape) != (B, T)):
        raise L.VisingerHipError(f"{name} must be [B, T]" + (f" = [{B}, {T}]" if B is not None else "") + f", got {tuple(t.shape)}")
    if torch.is_grad_enabled() and t.requires_grad:
        raise L.VisingerHipError(f"{name} requires grad: the pitch kernels have no backward (detach it, or feed the curve as data)")
    return t.float().contiguous()


def norm_interp_f0(f0_hz, lengths=None):
    """(f0_norm, uv), both fp32 [B, T], of a curve in Hz [B, T] with 0 on unvoiced frames: uv = (f0_hz == 0), f0_norm = log2(f0_hz + 1)
    on voiced frames and interpolated over the gaps (straight line between the voiced neighbours; the first / last voiced value before /
    after them; 0 on a row without a voiced frame).  lengths: int64 GPU tensor [B] (read on the device) -- row b is its first lengths[b]
    frames, the rest comes back as f0_norm = 0, uv = 0; None = every row is T long.  A negative or non-finite value counts as unvoiced
    (the reference gives NaN there)."""
    f0 = _rows("f0_hz", f0_hz)
    B, T = f0.shape
    if B == 0 or T == 0 or T >= T_LIMIT:
        raise L.VisingerHipError(f"norm_interp_f0: B, T must be positive and T < 2^24, got {(B, T)}")
    if lengths is not None:
        lengths = A.gpu_tensor("norm_interp_f0", "lengths", lengths, torch.int64, (B,))
    lib = L.require_gpu()
    f0_norm, uv = torch.empty_like(f0), torch.empty_like(f0)
    L.check(lib.vs_f0_norm_interp(L.ptr(f0), A.vp(lengths), L.ptr(f0_norm), L.ptr(uv), B, T, L.stream_ptr()))
    return f0_norm, uv


def cents_tensor(cents, B, device):
    """fp32 [B] on the device: a number (every item), a sequence of B numbers, or a 1-D fp32 GPU tensor [B] -- used as it is and never read
    back (its values are the caller's to keep finite)."""
    return A.per_item_f32("pitch shifts", cents, B, device)


def pitch_condition(frame_mask, pred=None, f0_norm=None, uv=None, cents=None, return_hz=False):
    """The frame prior's pitch condition, fp32 [B, 1, T] (with return_hz also the conditioning curve in Hz, fp32 [B, T]):
    curve x = f0_norm if given, else pred[..., 0]; voiced = (uv == 0) if uv is given, else (pred[..., 1] <= 0); rows with cents != 0 are
    transposed, x = log2((2^x - 1) * 2^(cents / 1200) + 1); cond = x * mask on voiced, unmasked frames and 0 elsewhere -- with no shift bit
    for bit ``(f0 * voiced).unsqueeze(1) * frame_mask``.  Hz: clamp(2^x - 1, 50, 1250) on those frames, 0 elsewhere.
    frame_mask: [B, 1, T] / [B, T] or None (all ones); pred: [B, T, 2] as the pitch predictor returns it (a strided view is made dense first:
    the kernel reads the (curve, logit) pair of a frame as one load); cents: see cents_tensor."""
    if pred is None and f0_norm is None:
        raise L.VisingerHipError("pitch_condition: give pred or f0_norm (the curve)")
    if pred is None and uv is None:
        raise L.VisingerHipError("pitch_condition: without uv the voicing comes from pred, which is missing")
    if pred is not None:
        if not (torch.is_tensor(pred) and pred.is_cuda and pred.dim() == 3 and pred.shape[2] == 2):
            raise L.VisingerHipError("pitch_condition: pred must be a [B, T, 2] tensor on the GPU (there is no CPU path)")
        if torch.is_grad_enabled() and pred.requires_grad:
            raise L.VisingerHipError("pitch_condition: pred requires grad: the pitch kernels have no backward (train on the aten path, or under no_grad)")
        B, T = pred.shape[:2]
        pred = pred.float().contiguous()
    else:
        B, T = _rows("f0_norm", f0_norm).shape
    if B == 0 or T == 0:
        raise L.VisingerHipError(f"pitch_condition: B, T must be positive, got {(B, T)}")
    f0_norm = None if f0_norm is None else _rows("f0_norm", f0_norm, B, T)
    uv = None if uv is None else _rows("uv", uv, B, T)
    mask = None if frame_mask is None else _rows("frame_mask", frame_mask, B, T)
    dev = (pred if pred is not None else f0_norm).device
    cents = None if cents is None else cents_tensor(cents, B, dev)
    lib = L.require_gpu()
    cond = torch.empty((B, 1, T), device=dev, dtype=torch.float32)
    hz = torch.empty((B, T), device=dev, dtype=torch.float32) if return_hz else None
    L.check(lib.vs_pitch_condition(L.ptr(pred), L.ptr(f0_norm), L.ptr(uv), L.ptr(mask), L.ptr(cents), L.ptr(cond), L.ptr(hz), B, T, L.stream_ptr()))
    return (cond, hz) if return_hz else cond
