#!/usr/bin/env python3
"""The one launch of csrc/guide_align.hip (guide_align.align_guide: vs_guide_align) on a batch of scores and guides, and beside it what a host would do
instead: the numpy restatement of the same rule (tests/test_guide_align_cpu.py: align_ref) on ONE item, wall clock -- and the pitch tracker's launch it
follows (profiles/f0_bench.json).
HIP events around every launch, 10 warm-up + 50 timed; prints the median and the minimum per shape B x G x T_ph, the time per frame step (the kernel is a
dependent chain of G steps: one barrier plus one LDS exchange each, none when the score fits one wave), and writes one JSON file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from visinger_amd import guide_align  # noqa: E402
from _bench import emit, timed  # noqa: E402


def score_and_guide(rng, G, T_ph):
    """T_ph tokens, all with frames, in notes of two (consonant + vowel) on a semitone grid; the guide sings them over G frames with every note stretched
    by 0.6 .. 1.6, a quarter step off the quantisation grid"""
    from test_guide_align_cpu import hz_of_q
    notes = (T_ph + 1) // 2
    pitch = 52 + np.cumsum(rng.integers(1, 6, notes) * rng.choice([-1, 1], notes)) % 24
    note_midi = np.repeat(pitch, 2)[:T_ph].astype(np.float32)
    per = max(2, int(0.9 * G) // T_ph)
    dur = rng.integers(1, 2 * per, T_ph).astype(np.int64)
    w = np.repeat(rng.uniform(0.6, 1.6, notes), 2)[:T_ph] * dur
    ends = np.maximum(np.rint(np.cumsum(w) * G / w.sum()).astype(np.int64), np.arange(1, T_ph + 1))
    ends[-1] = G
    f0 = np.zeros(G, np.float32)
    lo = 0
    for i, hi in enumerate(ends):
        f0[lo:hi] = hz_of_q(16 * int(note_midi[i]))
        lo = int(hi)
    return f0, note_midi, dur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x1024x256,1x1024x256,1x4096x1024,32x1024x64", help="comma-separated B x G x T_ph")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    args = ap.parse_args()
    from test_guide_align_cpu import align_ref
    try:
        tracker = json.load(open(os.path.join(ROOT, "profiles", "f0_bench.json")))["results"][0]
    except (OSError, ValueError, KeyError, IndexError):
        tracker = None
    results = []
    for shape in args.shapes.split(","):
        B, G, T_ph = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(1)
        rows = [score_and_guide(rng, G, T_ph) for _ in range(min(B, 4))]
        pick = np.arange(B) % len(rows)
        f0 = torch.from_numpy(np.stack([r[0] for r in rows])[pick]).cuda()
        note = torch.from_numpy(np.stack([r[1] for r in rows])[pick]).cuda()
        dur = torch.from_numpy(np.stack([r[2] for r in rows])[pick]).cuda()
        lens = torch.full((B,), G, dtype=torch.int64, device="cuda")

        def device():
            return guide_align.align_guide(f0, note, dur=dur, guide_lengths=lens)

        dur_new, cost, status = device()
        t0 = time.perf_counter()
        ref = align_ref(*rows[0])
        host_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(dur_new[0].cpu().numpy(), ref[0]) and int(cost[0]) == ref[1] and int(status[0]) == ref[2])
        med, best = timed(device, args.warmup, args.iters)
        waves = -(-T_ph // 64)
        where = "LDS" if guide_align.workspace_bytes(B, G, T_ph) == 0 else "workspace"
        print(f"B={B} G={G} T_ph={T_ph} ({waves} wave{'s' if waves > 1 else ''} a workgroup, backpointers in {where}): align_guide (one launch) median {med:.1f} us "
              f"(min {best:.1f}), {1e3 * med / G:.0f} ns a frame step; numpy restatement of one item: {host_ms:.0f} ms; equal to it: {same}", flush=True)
        results.append(dict(B=B, G=G, T_ph=T_ph, waves=waves, backpointers=where, launch_us_median=round(med, 1), launch_us_min=round(best, 1),
                            ns_per_frame_step=round(1e3 * med / G, 1), host_numpy_one_item_ms=round(host_ms, 1), equal_to_restatement=same))
    line = {"tool": "align_bench", "warmup": args.warmup, "iters": args.iters, "results": results,
            "tracker_launch_us_32x1024": None if tracker is None else tracker.get("launch_us_median")}
    emit(line, args.out)


if __name__ == "__main__":
    main()
