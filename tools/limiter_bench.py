#!/usr/bin/env python3
"""The peak limiter of csrc/limiter.hip -- vs_peak_limit (limiter.limit_peaks) -- on 32 rows of 262144 samples at window 128, in two cases: about 1 % of the
samples over the ceiling, in bursts, and none over it (every tile takes the copy path).  Beside each what a user can do today: the same statement with torch
ops on the same GPU in the same process -- clamp(512 log2(|x| / c), 0), max_pool1d over 2 W + 1, avg_pool1d over 2 W + 1 that does not count the padding,
exp2, one product, one clamp.  (The torch statement's gain is a float and its mean is not rounded up: it is the same shape of work, not the same bits.)
HIP events around every call; `--rounds` rounds that alternate kernel and torch statement, each with its own warm-up (10 + 100 calls each); the medians of the
rounds' medians and their spread are reported, and the floor of the pass: 8 bytes a sample at 8 TB/s.  Ends with one JSON line (--out: also written there) and
exits non-zero if the kernel is not faster than the torch statement in every round, or if the case without peaks is slower than the one with."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visinger_amd import limiter as lm  # noqa: E402
from _bench import emit, timed  # noqa: E402

HBM_BYTES_PER_S = 8.0e12                                 # MI355X HBM3E peak (spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--ceiling-db", type=float, default=-1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, n, W = args.rows, args.samples, args.window
    c = lm.check_args(ceiling_db=args.ceiling_db, window=W)[0]
    g = torch.Generator(device="cuda").manual_seed(1)
    quiet = (torch.rand((B, n), device="cuda", generator=g) * 2 - 1) * (0.9 * c)
    # bursts of 64 samples, one block of 64 in 100 at random: about 1 % of the samples at 1 .. 4 times the ceiling
    burst = (torch.rand((B, n // 64), device="cuda", generator=g) < 0.01).repeat_interleave(64, dim=1)
    loud = torch.where(burst, quiet.sign() * c * (1 + 3 * torch.rand((B, n), device="cuda", generator=g)), quiet)
    lens = torch.full((B,), n, dtype=torch.int64, device="cuda")
    y = torch.empty_like(quiet)

    def torch_statement(x):
        need = torch.clamp(512.0 * torch.log2(x.abs() / c), min=0)[:, None]
        held = F.max_pool1d(need, 2 * W + 1, 1, W)
        gain = F.avg_pool1d(held, 2 * W + 1, 1, W, count_include_pad=False)[:, 0]
        return torch.clamp(torch.mul(x, torch.exp2(gain / -512.0)), -c, c, out=y)

    cases, ok = {}, True
    for name, x in (("peaks", loud), ("no_peaks", quiet)):
        kernel = lambda x=x: lm.limit_peaks(x, lengths=lens, out=y, ceiling_db=args.ceiling_db, window=W)
        torch_fn = lambda x=x: torch_statement(x)
        _, gain, stats = lm.limit_peaks(x, lengths=lens, return_gain=True, return_stats=True, ceiling_db=args.ceiling_db, window=W)
        over = float(stats[:, 0].sum()) / (B * n)
        diff = float((kernel().clone() - torch_fn()).abs().max())
        rounds = []
        for _ in range(args.rounds):                                     # alternating: the box is shared
            rounds.append((timed(kernel, 10, 100)[0], timed(torch_fn, 10, 100)[0]))
        k_us, t_us = (float(np.median([r[i] for r in rounds])) for i in range(2))
        spread = [round(max(r[i] for r in rounds) / min(r[i] for r in rounds), 3) for i in range(2)]
        ok = ok and all(r[0] < r[1] for r in rounds)
        bytes_moved = 8.0 * B * n
        floor = bytes_moved / HBM_BYTES_PER_S * 1e6
        print(f"{name}: B = {B} x {n} samples, window {W}, {100 * over:.2f} % over the ceiling, largest reduction {int(stats[:, 1].max())} units\n"
              f"  kernel median {k_us:.1f} us ({B * n / (k_us * 1e-6):.3e} samples/s; floor {floor:.1f} us for {bytes_moved / 1e6:.1f} MB at 8 TB/s: "
              f"{k_us / floor:.1f}x), torch {t_us:.1f} us: {t_us / k_us:.2f}x the kernel; max difference {diff:.2e}; max / min over {args.rounds} rounds {spread}",
              flush=True)
        cases[name] = dict(over_fraction=round(over, 5), max_reduction_units=int(stats[:, 1].max()), kernel_us=round(k_us, 1), torch_us=round(t_us, 1),
                           torch_over_kernel=round(t_us / k_us, 2), kernel_us_by_round=[round(r[0], 1) for r in rounds],
                           torch_us_by_round=[round(r[1], 1) for r in rounds], max_over_min_by_round=spread, bytes_moved=bytes_moved,
                           floor_bytes_us=round(floor, 1), kernel_over_floor=round(k_us / floor, 2), samples_per_s=round(B * n / (k_us * 1e-6)),
                           max_abs_diff_to_torch=diff)
    emit({"tool": "limiter_bench", "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "rows": B, "samples": n, "window": W,
          "ceiling_db": args.ceiling_db, "warmup": 10, "iters": 100, "rounds": args.rounds, **cases}, args.out)
    if not ok:
        sys.exit("the kernel is not faster than its torch statement in every round")
    if cases["no_peaks"]["kernel_us"] > cases["peaks"]["kernel_us"]:
        sys.exit("the case without peaks is slower than the case with peaks")


if __name__ == "__main__":
    main()
