#!/usr/bin/env python3
"""vs_prior_sample (one launch, seeded per-item streams) against the five-op aten chain it replaces on the seeded path
(models/visinger.py:_sample_and_decode: randn_like, exp, mul, add, mul), on the same mu / logs / mask: the two split views of one
[B, 2H, T] projection output and a [B, 1, T] frame mask.  HIP events around every iteration, 20 warm-up + 100 timed; prints the median and
the minimum per shape and one JSON line.  Default shapes: the headline batch (B = 32, H = 192, T = 1024) and a single utterance (B = 1)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visinger_amd import sampling  # noqa: E402
from _bench import emit, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x192x1024,1x192x1024", help="comma-separated BxHxT")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    results = []
    for shape in args.shapes.split(","):
        B, H, T = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        stats = torch.randn(B, 2 * H, T, device="cuda", generator=g)
        stats[:, H:].mul_(0.5).sub_(1.0)
        lens = torch.randint(T // 2, T + 1, (B,), device="cuda", generator=g)
        mask = (torch.arange(T, device="cuda")[None, :] < lens[:, None]).float()[:, None, :]
        mu, logs = torch.split(stats, H, dim=1)
        seeds = torch.arange(B, dtype=torch.int64, device="cuda") + 12345

        def chain():
            return (mu + torch.randn_like(mu) * torch.exp(logs)) * mask

        def kernel():
            return sampling.prior_sample(mu, logs, mask, seeds)

        with torch.no_grad():
            c_med, c_min = timed(chain, args.warmup, args.iters)
            k_med, k_min = timed(kernel, args.warmup, args.iters)
        mb = B * H * T * 12 / 1e6
        print(f"B={B} H={H} T={T}: aten chain median {c_med:.1f} us (min {c_min:.1f}); vs_prior_sample median {k_med:.1f} us (min {k_min:.1f}), "
              f"{mb:.1f} MB -> {mb / k_med:.2f} TB/s at the median", flush=True)      # (MB / us = TB/s)
        results.append(dict(B=B, H=H, T=T, chain_us_median=round(c_med, 2), chain_us_min=round(c_min, 2), kernel_us_median=round(k_med, 2),
                            kernel_us_min=round(k_min, 2), kernel_tb_s=round(mb / k_med, 3)))
    emit({"tool": "sample_bench", "warmup": args.warmup, "iters": args.iters, "results": results})


if __name__ == "__main__":
    main()
