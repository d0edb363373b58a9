"""Seeded per-item sampling on the device (csrc/sample_ops.hip): ``(item seed, take, channel, frame) -> normal value``, whatever batch,
row, padding or number of takes the item is synthesised with, and the reparameterised prior sample of the synthesis path
(reference models/visinger.py:107: ``randn_like`` + ``exp`` + ``mul`` + ``add`` + ``mul``) as one launch on that stream.

The stream (DESIGN.md "Seeded sampling"): Philox4x32-10 keyed by the item seed, counter (frame, channel // 4, take, 0), two Box-Muller
pairs per call.  ``seeds`` is one integer in [0, 2^63) per item: a sequence of Python ints (checked here, copied to the device) or an
int64 CUDA tensor [B] (used as it is and never read back: no host synchronisation, so a captured graph replays with whatever the buffer
holds; its values are the caller's to keep in range)."""
import torch

from . import _lib as L
from ._args import vp

SEED_LIMIT = 1 << 63
TAKE_LIMIT = 1 << 32


def check_seeds(seeds):
    """list of Python ints from a sequence of seeds; ValueError for anything outside [0, 2^63)"""
    out = []
    for s in seeds:
        if isinstance(s, bool) or not isinstance(s, int):
            try:
                s = s.__index__()
            except (AttributeError, TypeError):
                raise ValueError(f"a seed must be an integer in [0, 2^63), got {s!r}") from None
        if not 0 <= s < SEED_LIMIT:
            raise ValueError(f"a seed must be an integer in [0, 2^63), got {s}")
        out.append(int(s))
    return out


def item_seeds(seeds, n):
    """one checked seed for each of n items: a single integer s gives item i the seed (s + i) mod 2^63, a sequence must hold n seeds (ValueError)"""
    if isinstance(seeds, int) and not isinstance(seeds, bool):
        seeds = [(s + i) % SEED_LIMIT for s in check_seeds([seeds]) for i in range(n)]
    seeds = check_seeds(seeds)
    if len(seeds) != n:
        raise ValueError(f"{len(seeds)} seeds for {n} items")
    return seeds


def check_takes(takes, first_take):
    takes, first_take = int(takes), int(first_take)
    if takes < 1 or first_take < 0 or first_take + takes > TAKE_LIMIT:
        raise ValueError(f"takes must be >= 1 and 0 <= first_take, first_take + takes <= 2^32 (got takes={takes}, first_take={first_take})")
    return takes, first_take


def seeds_tensor(seeds, device=None):
    """int64 [B] on the device: an int64 CUDA tensor passes through, a sequence of ints is range-checked and copied over"""
    if torch.is_tensor(seeds):
        if not (seeds.is_cuda and seeds.dtype == torch.int64 and seeds.dim() == 1):
            raise L.VisingerHipError(f"seeds must be a 1-D int64 tensor on the GPU (or a sequence of ints), got {seeds.dtype} {seeds.device} "
                                     f"{tuple(seeds.shape)}")
        return seeds.contiguous()
    vals = check_seeds(seeds)
    L.require_gpu()
    return torch.tensor(vals, dtype=torch.int64).to(device if device is not None else "cuda")


def item_noise(seeds, H, T, takes=1, first_take=0, device=None):
    """fp32 [B * takes, H, T]: row b * takes + k holds take first_take + k of item b's stream"""
    takes, first_take = check_takes(takes, first_take)
    sd = seeds_tensor(seeds, device)
    lib = L.require_gpu()
    out = torch.empty((sd.shape[0] * takes, int(H), int(T)), device=sd.device, dtype=torch.float32)
    L.check(lib.vs_normal_fill(vp(sd), first_take, takes, L.ptr(out), sd.shape[0], int(H), int(T), L.stream_ptr()))
    return out


def _stat_rows(t):
    """fp32 [B, H, T] whose rows are contiguous (row stride T, any batch stride >= H * T): the torch.split views of a [B, 2H, T] projection
    output pass as they are, anything else is converted / copied"""
    if t.dtype != torch.float32:
        t = t.float()
    B, H, T = t.shape
    if not (t.stride(2) == 1 and t.stride(1) == T and (B == 1 or t.stride(0) >= H * T)):
        t = t.contiguous()
    return t


def prior_sample(mu_p, logs_p, frame_mask, seeds, takes=1, first_take=0, noise_scale=1.0, return_noise=False):
    """z [B * takes, H, T] = (mu_p + noise_scale * n * exp(logs_p)) * frame_mask with n the seeded stream of each item, row b * takes + k =
    take first_take + k of item b; with return_noise also n (fp32, bit-identical to item_noise).  mu_p / logs_p: [B, H, T], e.g. the two
    torch.split views FramePriorNetwork returns (read in place through their batch stride); frame_mask: [B, 1, T] / [B, T] or None.  The
    kernel computes in fp32; z comes back in mu_p's dtype."""
    takes, first_take = check_takes(takes, first_take)
    if not (torch.is_tensor(mu_p) and mu_p.is_cuda and logs_p.is_cuda and mu_p.dim() == 3 and mu_p.shape == logs_p.shape):
        raise L.VisingerHipError("prior_sample: mu_p / logs_p must be [B, H, T] tensors of one shape on the GPU (there is no CPU path)")
    lib = L.require_gpu()
    B, H, T = mu_p.shape
    sd = seeds_tensor(seeds, mu_p.device)
    if sd.shape[0] != B or sd.device != mu_p.device:
        raise L.VisingerHipError(f"prior_sample: {sd.shape[0]} seeds on {sd.device} for a batch of {B} on {mu_p.device}")
    mu, logs = _stat_rows(mu_p), _stat_rows(logs_p)
    bs = mu.stride(0) if B > 1 else max(mu.stride(0), H * T)
    if B > 1 and logs.stride(0) != bs:
        mu, logs = mu.contiguous(), logs.contiguous()
        bs = H * T
    mask = None
    if frame_mask is not None:
        if not frame_mask.is_cuda or frame_mask.numel() != B * T:
            raise L.VisingerHipError(f"prior_sample: frame_mask must hold [B, T] = [{B}, {T}] values on the GPU, got {tuple(frame_mask.shape)} {frame_mask.device}")
        mask = frame_mask.reshape(B, T).float().contiguous()
    z = torch.empty((B * takes, H, T), device=mu.device, dtype=torch.float32)
    eps = torch.empty_like(z) if return_noise else None
    L.check(lib.vs_prior_sample(vp(mu), vp(logs), bs, L.ptr(mask), vp(sd),
                                first_take, takes, float(noise_scale), L.ptr(z), L.ptr(eps), B, H, T, L.stream_ptr()))
    if z.dtype != mu_p.dtype:
        z = z.to(mu_p.dtype)
    return (z, eps) if return_noise else z
