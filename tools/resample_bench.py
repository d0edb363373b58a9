#!/usr/bin/env python3
"""The one launch of csrc/resample.hip (resample.resample: vs_resample_poly) on 32 rows of 262144 samples at 24000 -> 48000, 24000 -> 44100 and 44100 -> 24000,
and beside it what a user can do today: the same polyphase stated with torch ops on the same GPU in the same process -- a conv1d with L output channels (one
per table row) and stride M over the zero-padded row, its [B, L, n / L] result interleaved into the waveform.  The torch statement is timed on a row padded
beforehand and both with and without the interleave; the kernel is compared with the faster of the two (the conv1d alone).
HIP events around every call; per ratio `--rounds` rounds that alternate the two, each with its own warm-up (10 + 100 kernel launches, 3 + 20 torch calls);
the medians of the rounds' medians and their spread are reported.  Two floors, both derived from the shapes: the bytes one pass must move (x read once, y
written once) at 8 TB/s, and P fused multiply-adds per output at the fp32 vector peak.  Ends with one JSON line (--out: also written there)."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visinger_amd import resample as rs  # noqa: E402
from _bench import emit, timed  # noqa: E402

HBM_BYTES_PER_S = 8.0e12                                 # MI355X HBM3E peak (spec)
VALU_PEAK_FLOPS = 256 * 4 * 16 * 2 * 2 * 2.4e9           # fp32 vector peak (spec), packed: 157.3 TFLOP/s = 78.6e12 fused multiply-adds a second


def torch_statement(x, sr_in, sr_out, n_out):
    """(padded input [B, 1, *], weight [L, 1, K], conv, whole): out[b, rho, a] = y[b, a L + rho].  Output n = a L + rho reads x[a M + o + j - C] table[rho][j],
    o = floor(rho M / L): row rho of the weight is the table row shifted right by o, the input is padded by C on the left."""
    L, M, W, P, table = rs.design(sr_in, sr_out)
    C = (P - 1) // 2
    off = (np.arange(L) * M) // L
    K = P + int(off.max())
    w = np.zeros((L, 1, K), np.float32)
    for rho in range(L):
        w[rho, 0, off[rho]:off[rho] + P] = table[rho]
    A = -(-n_out // L)
    need = (A - 1) * M + K
    xp = F.pad(x, (C, max(0, need - C - x.shape[1])))[:, None, :].contiguous()
    w = torch.from_numpy(w).to(x.device)
    conv = lambda: F.conv1d(xp, w, stride=M)
    whole = lambda: conv().transpose(1, 2).reshape(x.shape[0], -1)[:, :n_out].contiguous()
    return xp, w, conv, whole


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", default="24000:48000,24000:44100,44100:24000")
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, n = args.rows, args.samples
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((B, n), device="cuda", generator=g) * 0.3
    lens = torch.full((B,), n, dtype=torch.int64, device="cuda")
    results = []
    for pair in args.rates.split(","):
        sr_in, sr_out = (int(v) for v in pair.split(":"))
        L, M, W, P, _ = rs.design(sr_in, sr_out)
        n_out = rs.out_length(n, sr_in, sr_out)
        kernel = lambda: rs.resample(x, sr_in, sr_out, lengths=lens)
        xp, w, conv, whole = torch_statement(x, sr_in, sr_out, n_out)
        y, yt = kernel(), whole()
        diff = float((y - yt).abs().max())
        rounds = []
        for _ in range(args.rounds):                                     # alternating: the box is shared
            rounds.append((timed(kernel, 10, 100)[0], timed(conv, 3, 20)[0], timed(whole, 3, 20)[0]))
        k_us, c_us, w_us = (float(np.median([r[i] for r in rounds])) for i in range(3))
        spread = [round(max(r[i] for r in rounds) / min(r[i] for r in rounds), 3) for i in range(3)]
        bytes_moved = 4.0 * B * (n + n_out)
        fma = float(B) * n_out * P
        floor_bytes_us, floor_fma_us = bytes_moved / HBM_BYTES_PER_S * 1e6, 2.0 * fma / VALU_PEAK_FLOPS * 1e6
        print(f"{sr_in} -> {sr_out} (L = {L}, M = {M}, P = {P}, table {L * P * 4} B, tile {rs.tile(L)}): B = {B} x {n} -> {n_out}: kernel median {k_us:.1f} us "
              f"({B * n_out / (k_us * 1e-6):.3e} samples/s out; floors: {floor_bytes_us:.1f} us for {bytes_moved / 1e6:.1f} MB at 8 TB/s, {floor_fma_us:.1f} us for "
              f"{fma:.3e} fma at the packed fp32 peak); torch conv1d [{L}, 1, {w.shape[2]}] stride {M}: {c_us:.1f} us, with the interleave {w_us:.1f} us: "
              f"{c_us / k_us:.1f}x / {w_us / k_us:.1f}x the kernel; max |kernel - torch| = {diff:.2e}; max / min over {args.rounds} rounds {spread}", flush=True)
        results.append(dict(sr_in=sr_in, sr_out=sr_out, L=L, M=M, P=P, table_bytes=L * P * 4, tile=rs.tile(L), rows=B, n_in=n, n_out=n_out,
                            kernel_us=round(k_us, 1), samples_out_per_s=round(B * n_out / (k_us * 1e-6)), samples_in_per_s=round(B * n / (k_us * 1e-6)),
                            floor_bytes_us=round(floor_bytes_us, 1), bytes_moved=bytes_moved, floor_fma_us=round(floor_fma_us, 1), fma=fma,
                            kernel_over_larger_floor=round(k_us / max(floor_bytes_us, floor_fma_us), 2),
                            torch_conv1d_us=round(c_us, 1), torch_conv1d_interleaved_us=round(w_us, 1), torch_conv1d_kernel_taps=int(w.shape[2]),
                            torch_over_kernel=round(c_us / k_us, 2), max_abs_diff_to_torch=diff, rounds=args.rounds, max_over_min_by_round=spread))
        del xp, w, y, yt
    emit({"tool": "resample_bench", "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "valu_peak_flops": VALU_PEAK_FLOPS,
          "warmup": [10, 3], "iters": [100, 20], "results": results}, args.out)
    if not all(r["kernel_us"] < r["torch_conv1d_us"] for r in results):
        sys.exit("the kernel is not faster than the torch statement at every ratio")


if __name__ == "__main__":
    main()
