#!/usr/bin/env python3
"""The two launches of csrc/timing_ops.hip (timing.retime with a capacity: vs_retime_tokens + vs_retime_frames, alignment and guide curve) against the
host chain they replace, on the same inputs: per item the durations from mel2ph, the new token ends by the same rule (vectorised numpy),
``np.repeat`` for the new alignment, the curve resampled inside each token, padded, and both transfers (mel2ph and curve to the host, the results back)
-- wall clock, since that chain synchronises with the host by construction.
HIP events around every iteration for the device path, 20 warm-up + 100 timed; prints the medians and one JSON line.  Default: B = 32, T = 1024, 128 tokens."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visinger_amd import timing  # noqa: E402
from _bench import emit, timed  # noqa: E402


def host_retime(m2p_dev, curve_dev, stretch, tempo, T_ph, cap):
    """every item through numpy on the host, padded to `cap`, back to the device"""
    m2p, curve = m2p_dev.cpu().numpy(), curve_dev.cpu().numpy()
    out, warped = np.zeros((len(m2p), cap), np.int64), np.zeros((len(m2p), cap), np.float32)
    for b in range(len(m2p)):
        d = np.bincount(m2p[b], minlength=T_ph + 1)[1:T_ph + 1].astype(np.int64)
        s = np.rint(np.clip(stretch[b] / np.float32(tempo[b]), 2.0 ** -6, 2.0 ** 6) * 65536).astype(np.int64)
        R = (np.cumsum(d * s) + 32768) >> 16
        M = np.cumsum(d > 0)
        e = M + np.maximum(0, np.maximum.accumulate(R - M))
        n2 = np.diff(e, prepend=0)
        new = np.repeat(np.arange(1, T_ph + 1), n2)[:cap]
        out[b, :len(new)] = new
        tok = new - 1
        c0, e0 = (np.cumsum(d) - d)[tok], (e - n2)[tok]
        u, n, n2 = np.arange(len(new)) - e0, d[tok], n2[tok]
        num, den = (2 * u + 1) * n - n2, 2 * n2
        k = np.where(num < 0, 0, num // den)
        w = np.where(num < 0, 0, (num - k * den) / den).astype(np.float32)
        last = k >= n - 1
        k, w = np.where(last, n - 1, k), np.where(last, 0, w).astype(np.float32)
        a, bb = curve[b][c0 + k], curve[b][c0 + np.minimum(k + 1, n - 1)]
        warped[b, :len(new)] = np.where((a > 0) & (bb > 0), a + w * (bb - a), np.where(w < 0.5, a, bb))
    return torch.from_numpy(out).to(m2p_dev.device), torch.from_numpy(warped).to(m2p_dev.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x1024x128,1x1024x128", help="comma-separated BxTxT_ph")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    results = []
    for shape in args.shapes.split(","):
        B, T, T_ph = (int(v) for v in shape.split("x"))
        r = np.random.default_rng(1)
        m2p = np.zeros((B, T), np.int64)
        for b in range(B):
            cuts = np.sort(r.choice(np.arange(1, T), T_ph - 1, replace=False))
            m2p[b] = np.repeat(np.arange(1, T_ph + 1), np.diff(np.concatenate([[0], cuts, [T]])))
        stretch = r.uniform(0.5, 2.0, (B, T_ph)).astype(np.float32)
        tempo = r.uniform(0.8, 1.25, B).astype(np.float32)
        curve = r.uniform(80, 900, (B, T)).astype(np.float32)
        curve[r.uniform(size=(B, T)) < 0.3] = 0
        cap = 4 * T
        m2p_d, st_d, tp_d, curve_d = (torch.from_numpy(x).cuda() for x in (m2p, stretch, tempo, curve))

        def device():
            return timing.retime(mel2ph=m2p_d, T_ph=T_ph, stretch=st_d, tempo=tp_d, curve=curve_d, max_frames=cap)

        def device_alignment_only():
            return timing.retime(mel2ph=m2p_d, T_ph=T_ph, stretch=st_d, tempo=tp_d, max_frames=cap)

        got, lens, warped = device()
        want, want_curve = host_retime(m2p_d, curve_d, stretch, tempo, T_ph, cap)
        assert torch.equal(got, want), "the host chain and the kernels disagree on the alignment"
        assert float((warped - want_curve).abs().max()) <= 1e-3, "the host chain and the kernels disagree on the curve"
        d_med, d_min = timed(device, args.warmup, args.iters)
        a_med, a_min = timed(device_alignment_only, args.warmup, args.iters)
        torch.cuda.synchronize()
        walls = []
        for _ in range(max(5, args.iters // 10)):
            t0 = time.perf_counter()
            host_retime(m2p_d, curve_d, stretch, tempo, T_ph, cap)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e6)
        h_med = sorted(walls)[len(walls) // 2]
        print(f"B={B} T={T} T_ph={T_ph} (capacity {cap}, longest retimed item {int(lens.max())}): host chain (numpy per item, wall clock with both transfers) "
              f"median {h_med:.0f} us; timing.retime (two launches) median {d_med:.1f} us (min {d_min:.1f}), alignment only {a_med:.1f} us (min {a_min:.1f})",
              flush=True)
        results.append(dict(B=B, T=T, T_ph=T_ph, capacity=cap, host_us_median=round(h_med, 1), retime_us_median=round(d_med, 2), retime_us_min=round(d_min, 2),
                            alignment_only_us_median=round(a_med, 2)))
    emit({"tool": "timing_bench", "warmup": args.warmup, "iters": args.iters, "results": results})


if __name__ == "__main__":
    main()
