"""Sample-rate conversion on the device (csrc/resample.hip): a rational polyphase converter, so that guide recordings at 44.1 / 48 kHz go into
the guide chain and waveforms come out of ``synth.synthesize`` at the rate a deliverable wants.  The reference resamples on the host (librosa); nothing of it is
reproduced.  The rule -- a Kaiser-windowed sinc prototype, evaluated in fp64 on the host and rounded once to fp32 -- is fully specified in
include/visinger_hip.h "f9"; the device sees the fp32 table only.

Everything that changes between two calls -- the samples, the lengths -- is read from device tensors, and the converted lengths are written on the device; with a
device ``lengths`` and ``out_len=`` nothing is read on the host, so a captured graph replays on another recording by overwriting those buffers.  GPU tensors
only; there is no CPU path and no backward."""
import functools
import math

import numpy as np
import torch

from . import _args as A
from . import _lib as L

TABLE_BYTES = 49152              # VS_RESAMPLE_TABLE_BYTES
LDS_BYTES = 65536                # VS_RESAMPLE_LDS_BYTES
M_LIMIT = 1 << 20                # VS_RESAMPLE_MAX_M
DEFAULTS = dict(zeros=32, beta=10.0, rolloff=0.90)


def ratio(sr_in, sr_out):
    """(L, M) = (sr_out, sr_in) / gcd; ValueError for rates that are not integers >= 1"""
    for name, v in (("sr_in", sr_in), ("sr_out", sr_out)):
        if not A.is_int(v, 1, (1 << 31) - 1):
            raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    g = math.gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g


def tile(Lr):
    """vs_resample_tile, restated: the outputs of one tile of a workgroup -- four groups of G = g L outputs, G about 256"""
    return 4 * Lr * max(1, (256 + Lr // 2) // Lr)


def fits(Lr, M, P):
    """vs_resample_fits, restated: the table within its budget, table and one tile's input span within the workgroup's LDS"""
    span = (3 + (tile(Lr) - 1) * M // Lr + P + 4) & ~3
    return M <= M_LIMIT and Lr * P * 4 <= TABLE_BYTES and (((Lr * P + 3) & ~3) + span) * 4 <= LDS_BYTES


@functools.lru_cache(maxsize=64)
def _design(sr_in, sr_out, zeros, beta, rolloff):
    Lr, M = ratio(sr_in, sr_out)
    S = max(Lr, M)
    W = zeros * S
    C = -(-W // Lr)
    P = 2 * C + 1
    if not fits(Lr, M, P):
        raise ValueError(f"{sr_in} -> {sr_out} Hz with zeros = {zeros} needs a table of L = {Lr} rows of P = {P} taps ({Lr * P * 4} bytes) and a tile span for "
                         f"M = {M}: over the kernel's budget ({TABLE_BYTES} bytes of table, {LDS_BYTES} with the span)")
    fc = rolloff / (2.0 * S)
    rho, j = np.arange(Lr, dtype=np.int64)[:, None], np.arange(P, dtype=np.int64)[None, :]
    m = (C - j) * Lr + (rho * M) % Lr                                    # row rho: the phase of the outputs n with n mod L = rho
    inside = np.abs(m) <= W
    u = np.where(inside, m, 0).astype(np.float64)
    h = Lr * 2.0 * fc * np.sinc(2.0 * fc * u) * np.i0(beta * np.sqrt(1.0 - (u / W) ** 2)) / np.i0(beta)
    table = np.where(inside, h, 0.0).astype(np.float32)
    table.setflags(write=False)
    return Lr, M, W, P, table


def check_quality(zeros=32, beta=10.0, rolloff=0.90):
    if not A.is_int(zeros, 1, 1 << 16):
        raise ValueError(f"zeros must be an integer >= 1, got {zeros!r}")
    if not (A.is_real(beta) and beta > 0):
        raise ValueError(f"beta must be a finite number > 0, got {beta!r}")
    if not (A.is_real(rolloff) and 0 < rolloff <= 1):
        raise ValueError(f"rolloff must be a number in (0, 1], got {rolloff!r}")
    return int(zeros), float(beta), float(rolloff)


def design(sr_in, sr_out, zeros=32, beta=10.0, rolloff=0.90):
    """(L, M, W, P, table) of the converter sr_in -> sr_out (visinger_hip.h "f9"): table is the read-only fp32 array [L, P] the kernel takes -- row rho holds the
    phase (rho M) mod L, table[rho, j] = h((C - j) L + phase), C = (P - 1) / 2 = ceil(W / L).  Cached per arguments.  ValueError for a value out of range and
    for a ratio whose table does not fit the kernel's budget."""
    ratio(sr_in, sr_out)
    return _design(int(sr_in), int(sr_out), *check_quality(zeros, beta, rolloff))


def out_length(n, sr_in, sr_out):
    """ceil(n L / M): the samples a row of n samples becomes"""
    Lr, M = ratio(sr_in, sr_out)
    if not A.is_int(n, 0, 1 << 40):
        raise ValueError(f"n must be an integer in [0, 2^40], got {n!r}")
    return -(-int(n) * Lr // M)


def resample(wav, sr_in, sr_out, lengths=None, out_len=None, return_lengths=False, **quality):
    """wav -- a float GPU tensor [B, n], or [n] taken as one row (fp32 is used as it is, other float types are converted) -- at sr_in Hz converted to sr_out Hz:
    fp32 [B, out_len].  Row b has lengths[b] samples and becomes ceil(lengths[b] L / M); the rest of its row comes back 0, and what lies at or beyond
    lengths[b] in wav is never read into a result.
    lengths: None (every row is n long), a host sequence of B integers, or an int64 GPU tensor [B] -- used as it is, never read back (the kernel clamps it to
    [0, n]).  out_len=None: out_length(n, sr_in, sr_out); otherwise the result is out_len wide (graph capture: a capacity; a smaller one cuts the rows).
    return_lengths: also the converted lengths, an int64 GPU tensor [B] written by the kernel (not cut at out_len).
    quality: zeros, beta, rolloff (design()).  Equal rates return wav as it is (and, with return_lengths, lengths as a device tensor).
    ValueError for host values out of range, VisingerHipError for tensors of the wrong kind; both before any launch."""
    Lr, M, _, P, _ = design(sr_in, sr_out, **A.keys("resample", quality, DEFAULTS))
    key = (int(sr_in), int(sr_out)) + check_quality(**quality)
    if out_len is not None and not A.is_int(out_len, 1, (1 << 40) - 1):
        raise ValueError(f"out_len must be an integer in [1, 2^40), got {out_len!r}")
    if not (torch.is_tensor(wav) and wav.is_cuda and wav.is_floating_point() and wav.dim() in (1, 2)):
        raise L.VisingerHipError(f"resample: wav must be a float tensor [B, n] or [n] on the GPU (there is no CPU path), got {wav!r:.80}")
    if torch.is_grad_enabled() and wav.requires_grad:
        raise L.VisingerHipError("resample: wav requires grad: the converter has no backward (detach it)")
    one_row = wav.dim() == 1
    B, n = (1, wav.shape[0]) if one_row else wav.shape
    if B == 0 or n == 0 or n >= 1 << 40:
        raise L.VisingerHipError(f"resample: B > 0 and 0 < n < 2^40 are required, got {(B, n)}")
    lengths = A.lengths_i64("resample", "lengths", lengths, B, n, wav.device)
    if Lr == M:
        if not return_lengths:
            return wav
        return wav, (torch.full((B,), n, dtype=torch.int64, device=wav.device) if lengths is None else lengths)
    x = (wav[None] if one_row else wav).float().contiguous()
    n_out = out_length(n, sr_in, sr_out) if out_len is None else int(out_len)
    lib = L.require_gpu()
    table = A.device_table(x.device, key, lambda: _design(*key)[4])             # (one copy of the host table per device, made on first use)
    y = torch.empty((B, n_out), device=x.device, dtype=torch.float32)
    out_lengths = torch.empty((B,), device=x.device, dtype=torch.int64) if return_lengths else None
    L.check(lib.vs_resample_poly(L.ptr(x), A.vp(lengths), B, n, L.ptr(table), Lr, M, P, L.ptr(y), n_out, A.vp(out_lengths), L.stream_ptr()))
    y = y[0] if one_row else y
    return (y, out_lengths) if return_lengths else y
