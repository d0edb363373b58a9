#!/usr/bin/env python3
"""The two launches of csrc/pitch_ops.hip against what they replace, on the same inputs:
  vs_pitch_condition against the aten chain of forward_pitch's tail, ``(pred[:, :, 0] * (pred[:, :, 1] <= 0)).unsqueeze(1) * mask`` (two slices, a compare,
  two multiplies), pred being the pitch predictor's strided [B, T, 2] view;
  vs_f0_norm_interp against the host chain of the reference (norm_interp_f0 per item: ``.cpu().numpy()``, ``np.interp``, back to the device, padded) --
  restated here with numpy, wall-clock time including the two transfers, since that chain synchronises with the host by construction.
HIP events around every iteration for the device-only paths, 20 warm-up + 100 timed; prints the medians and one JSON line.  Default: B = 32, T = 1024."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visinger_amd import pitch  # noqa: E402
from _bench import emit, timed  # noqa: E402


def host_norm_interp(f0_dev, lengths):
    """the reference's route: every item through numpy on the host, padded, back to the device"""
    f0 = f0_dev.cpu().numpy()
    out, uvs = np.zeros_like(f0), np.zeros_like(f0)
    for b, n in enumerate(lengths):
        row = f0[b, :n]
        uv = row == 0
        y = np.log2(row + 1)
        if uv.all():
            y[:] = 0
        elif uv.any():
            y[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], y[~uv])
        out[b, :n], uvs[b, :n] = y, uv
    return torch.from_numpy(out).to(f0_dev.device), torch.from_numpy(uvs).to(f0_dev.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x1024,1x1024", help="comma-separated BxT")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    results = []
    for shape in args.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        raw = torch.randn(B, 2, T, device="cuda", generator=g)
        raw[:, 0].mul_(1.5).add_(7.5)
        pred = raw.permute(0, 2, 1)
        lens = torch.randint(T // 2, T + 1, (B,), device="cuda", generator=g)
        mask = (torch.arange(T, device="cuda")[None, :] < lens[:, None]).float()[:, None, :]
        f0_hz = torch.rand(B, T, device="cuda", generator=g) * 800 + 80
        f0_hz[torch.rand(B, T, device="cuda", generator=g) < 0.4] = 0
        host_lens = lens.tolist()
        cents = torch.full((B,), 50.0, device="cuda")

        def chain():
            return (pred[:, :, 0] * (pred[:, :, 1] <= 0)).unsqueeze(1) * mask

        def cond_kernel():
            return pitch.pitch_condition(mask, pred=pred)

        def cond_kernel_full():
            return pitch.pitch_condition(mask, pred=pred, cents=cents, return_hz=True)

        def interp_kernel():
            return pitch.norm_interp_f0(f0_hz, lens)

        with torch.no_grad():
            c_med, c_min = timed(chain, args.warmup, args.iters)
            k_med, k_min = timed(cond_kernel, args.warmup, args.iters)
            f_med, f_min = timed(cond_kernel_full, args.warmup, args.iters)
            i_med, i_min = timed(interp_kernel, args.warmup, args.iters)
            torch.cuda.synchronize()
            walls = []
            for _ in range(max(5, args.iters // 10)):
                t0 = time.perf_counter()
                host_norm_interp(f0_hz, host_lens)
                torch.cuda.synchronize()
                walls.append((time.perf_counter() - t0) * 1e6)
            h_med = sorted(walls)[len(walls) // 2]
        print(f"B={B} T={T}: condition: aten chain median {c_med:.1f} us (min {c_min:.1f}); pitch_condition median {k_med:.1f} us (min {k_min:.1f}), "
              f"with shift and Hz output {f_med:.1f} us (min {f_min:.1f})", flush=True)
        print(f"B={B} T={T}: norm_interp_f0: host chain (numpy per item, wall clock with both transfers) median {h_med:.0f} us; vs_f0_norm_interp median "
              f"{i_med:.1f} us (min {i_min:.1f})", flush=True)
        results.append(dict(B=B, T=T, chain_us_median=round(c_med, 2), condition_us_median=round(k_med, 2), condition_full_us_median=round(f_med, 2),
                            host_interp_us_median=round(h_med, 1), interp_us_median=round(i_med, 2), interp_us_min=round(i_min, 2)))
    emit({"tool": "pitch_bench", "warmup": args.warmup, "iters": args.iters, "results": results})


if __name__ == "__main__":
    main()
