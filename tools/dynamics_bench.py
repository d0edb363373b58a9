#!/usr/bin/env python3
"""The two bandwidth kernels of csrc/dynamics.hip -- vs_level_track (dynamics.track_level) and vs_level_apply (dynamics.apply_gain) -- on 32 rows of 262144
samples at hop 256, and beside each what a user can do today: the same statement with torch ops on the same GPU in the same process.  track: the squares'
mean per hop, then an average pool over 2 half + 1 frames that does not count the padding.  apply: the gain curve interpolated linearly between frame centres
(F.interpolate, align_corners=False: held at the ends), exp2, one product.  The two small kernels (vs_level_offset, vs_level_gain) are timed alone.
HIP events around every call; `--rounds` rounds that alternate kernel and torch statement, each with its own warm-up (10 + 100 calls each); the medians of
the rounds' medians and their spread are reported, and the floor of each pass: the bytes it must move at 8 TB/s.  Ends with one JSON line (--out: also
written there) and exits non-zero if either kernel is slower than its torch statement."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visinger_amd import dynamics as dy  # noqa: E402
from _bench import emit, timed  # noqa: E402

HBM_BYTES_PER_S = 8.0e12                                 # MI355X HBM3E peak (spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--half", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, n, hop, half = args.rows, args.samples, args.hop, args.half
    T = n // hop
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((B, n), device="cuda", generator=g) * 0.3
    lens = torch.full((B,), n, dtype=torch.int64, device="cuda")
    frames = torch.full((B,), T, dtype=torch.int64, device="cuda")
    guide = torch.exp2(torch.randn((B, T), device="cuda", generator=g) * 2 - 6)
    y = torch.empty_like(x)

    track = lambda: dy.track_level(x, hop, lengths=lens, half_width=half)
    track_torch = lambda: F.avg_pool1d((x * x).view(B, T, hop).mean(2)[:, None], 2 * half + 1, 1, half, count_include_pad=False)[:, 0]
    own = track()
    off = dy.level_offset(guide, own, lengths=frames)[0]
    k = dy.level_gain(guide, own, lengths=frames, offset_units=off)
    apply = lambda: dy.apply_gain(x, k, hop, lengths=lens, out=y)
    apply_torch = lambda: torch.mul(x, torch.exp2(F.interpolate(k.float()[:, None], size=n, mode="linear", align_corners=False)[:, 0] / 512.0), out=y)
    rel = lambda got, want: float((got - want).abs().max() / want.abs().max())      # against the largest value: a sample may be 0
    track_diff = rel(own, track_torch())
    apply_diff = rel(apply().clone(), apply_torch())
    rounds = []
    for _ in range(args.rounds):                                         # alternating: the box is shared
        rounds.append((timed(track, 10, 100)[0], timed(track_torch, 10, 100)[0], timed(apply, 10, 100)[0], timed(apply_torch, 10, 100)[0]))
    t_us, tt_us, a_us, at_us = (float(np.median([r[i] for r in rounds])) for i in range(4))
    spread = [round(max(r[i] for r in rounds) / min(r[i] for r in rounds), 3) for i in range(4)]
    off_us = timed(lambda: dy.level_offset(guide, own, lengths=frames), 10, 100)[0]
    gain_us = timed(lambda: dy.level_gain(guide, own, lengths=frames, offset_units=off), 10, 100)[0]
    track_bytes, apply_bytes = 4.0 * B * (n + T), 4.0 * B * (2 * n + T)
    track_floor, apply_floor = track_bytes / HBM_BYTES_PER_S * 1e6, apply_bytes / HBM_BYTES_PER_S * 1e6
    print(f"B = {B} x {n} samples, hop {hop}, half {half} ({T} frames a row)\n"
          f"  track: kernel median {t_us:.1f} us ({B * n / (t_us * 1e-6):.3e} samples/s; floor {track_floor:.1f} us for {track_bytes / 1e6:.1f} MB at 8 TB/s: "
          f"{t_us / track_floor:.1f}x), torch {tt_us:.1f} us: {tt_us / t_us:.2f}x the kernel; max difference {track_diff:.2e} of the largest value\n"
          f"  apply: kernel median {a_us:.1f} us ({B * n / (a_us * 1e-6):.3e} samples/s; floor {apply_floor:.1f} us for {apply_bytes / 1e6:.1f} MB at 8 TB/s: "
          f"{a_us / apply_floor:.1f}x), torch {at_us:.1f} us: {at_us / a_us:.2f}x the kernel; max difference {apply_diff:.2e} of the largest value\n"
          f"  offset {off_us:.1f} us, gain {gain_us:.1f} us; max / min over {args.rounds} rounds {spread}", flush=True)
    emit({"tool": "dynamics_bench", "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "rows": B, "samples": n, "hop": hop, "half": half,
          "frames": T, "warmup": 10, "iters": 100, "rounds": args.rounds, "max_over_min_by_round": spread,
          "track": dict(kernel_us=round(t_us, 1), torch_us=round(tt_us, 1), torch_over_kernel=round(tt_us / t_us, 2), bytes_moved=track_bytes,
                        floor_bytes_us=round(track_floor, 1), kernel_over_floor=round(t_us / track_floor, 2), samples_per_s=round(B * n / (t_us * 1e-6)),
                        max_rel_diff_to_torch=track_diff),
          "apply": dict(kernel_us=round(a_us, 1), torch_us=round(at_us, 1), torch_over_kernel=round(at_us / a_us, 2), bytes_moved=apply_bytes,
                        floor_bytes_us=round(apply_floor, 1), kernel_over_floor=round(a_us / apply_floor, 2), samples_per_s=round(B * n / (a_us * 1e-6)),
                        max_rel_diff_to_torch=apply_diff),
          "offset_us": round(off_us, 1), "gain_us": round(gain_us, 1)}, args.out)
    if not (t_us < tt_us and a_us < at_us):
        sys.exit("a kernel is not faster than its torch statement")


if __name__ == "__main__":
    main()
