#!/usr/bin/env python3
"""The two launches of csrc/guide_correct.hip -- guide_correct.correct_guide (vs_guide_correct) and guide_correct.guide_deviation (vs_guide_deviation) -- on a
batch of sung scores, and beside them what a host would do instead: the vectorised numpy restatement of the same rule (tests/test_guide_correct_cpu.py:
correct_ref, deviation_ref) on ONE item, wall clock.
HIP events around every launch, 10 warm-up + 50 timed; prints the median and the minimum per shape B x T x T_ph and window, and the effective bytes a second:
what the launch must move once (f0 in and out 4 + 4 bytes a frame, mel2ph 8, k 4; the deviation: f0 4 + mel2ph 8) over the median.  Writes one JSON file."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from visinger_amd import guide_correct  # noqa: E402
from _bench import emit, timed  # noqa: E402


def sung(rng, T, T_ph):
    """T_ph tokens over T frames in notes of two (consonant + vowel) on a semitone grid, sung up to 40 cents off with a 30-cent vibrato, a quarter unit off
    the quantisation grid"""
    from test_guide_correct_cpu import hz_of_units
    notes = (T_ph + 1) // 2
    pitch = 52 + np.cumsum(rng.integers(1, 6, notes) * rng.choice([-1, 1], notes)) % 24
    note_midi = np.repeat(pitch, 2)[:T_ph].astype(np.float32)
    w = np.cumsum(rng.uniform(0.5, 1.5, T_ph))
    ends = np.rint(w * T / w[-1]).astype(np.int64)                            # the last frame + 1 of each token
    mel2ph = np.searchsorted(ends, np.arange(T), side="right").clip(0, T_ph - 1) + 1
    cents = np.repeat(rng.uniform(-40, 40, notes), 2)[:T_ph][mel2ph - 1] + 30 * np.sin(2 * np.pi * 5.5 * np.arange(T) / 100.0)
    f0 = hz_of_units(np.rint(1600.0 * (note_midi[mel2ph - 1] - 69) + 16 * cents))
    return f0, mel2ph.astype(np.int64), note_midi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x1024x256,1x1024x256,1x65536x1024", help="comma-separated B x T x T_ph")
    ap.add_argument("--windows", default="12,1024")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correct_bench.json"))
    args = ap.parse_args()
    from test_guide_correct_cpu import correct_ref, deviation_ref
    results = []
    for shape in args.shapes.split(","):
        B, T, T_ph = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(1)
        rows = [sung(rng, T, T_ph) for _ in range(min(B, 4))]
        pick = np.arange(B) % len(rows)
        f0 = torch.from_numpy(np.stack([r[0] for r in rows])[pick]).cuda()
        m2p = torch.from_numpy(np.stack([r[1] for r in rows])[pick]).cuda()
        note = torch.from_numpy(np.stack([r[2] for r in rows])[pick]).cuda()
        lens = torch.full((B,), T, dtype=torch.int64, device="cuda")
        med, n_corr = guide_correct.guide_deviation(f0, m2p, note, lengths=lens)
        t0 = time.perf_counter()
        ref = deviation_ref(*rows[0])
        host_ms = (time.perf_counter() - t0) * 1e3
        same = (int(med[0]), int(n_corr[0])) == ref
        us, best = timed(lambda: guide_correct.guide_deviation(f0, m2p, note, lengths=lens), args.warmup, args.iters)
        gbs = B * T * 12 / us * 1e-3
        print(f"B={B} T={T} T_ph={T_ph}: guide_deviation (one launch) median {us:.1f} us (min {best:.1f}), {gbs:.1f} GB/s effective; numpy restatement of one item: "
              f"{host_ms:.2f} ms; equal to it: {same}", flush=True)
        results.append(dict(kernel="vs_guide_deviation", B=B, T=T, T_ph=T_ph, launch_us_median=round(us, 1), launch_us_min=round(best, 1),
                            effective_gb_per_s=round(gbs, 1), host_numpy_one_item_ms=round(host_ms, 2), equal_to_restatement=bool(same)))
        for W in (int(v) for v in args.windows.split(",")):
            out, k = guide_correct.correct_guide(f0, m2p, note, lengths=lens, return_units=True, window=W)
            t0 = time.perf_counter()
            ref_k, _ = correct_ref(*rows[0], window=W)
            host_ms = (time.perf_counter() - t0) * 1e3
            same = bool(np.array_equal(k[0].cpu().numpy(), ref_k))
            us, best = timed(lambda: guide_correct.correct_guide(f0, m2p, note, lengths=lens, return_units=True, window=W), args.warmup, args.iters)
            gbs = B * T * 20 / us * 1e-3
            staged = min(T, 1024 + 2 * W) / min(T, 1024)
            print(f"B={B} T={T} T_ph={T_ph} W={W}: correct_guide (one launch, {staged:.2f} frames staged per frame written) median {us:.1f} us (min {best:.1f}), "
                  f"{gbs:.1f} GB/s effective; numpy restatement of one item: {host_ms:.2f} ms; equal to it: {same}", flush=True)
            results.append(dict(kernel="vs_guide_correct", B=B, T=T, T_ph=T_ph, window=W, frames_staged_per_frame=round(staged, 2), launch_us_median=round(us, 1),
                                launch_us_min=round(best, 1), effective_gb_per_s=round(gbs, 1), host_numpy_one_item_ms=round(host_ms, 2),
                                equal_to_restatement=same))
    line = {"tool": "correct_bench", "warmup": args.warmup, "iters": args.iters, "results": results}
    emit(line, args.out)


if __name__ == "__main__":
    main()
