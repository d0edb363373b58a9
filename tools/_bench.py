"""What the launch benchmarks of the control ops share (f0_bench, align_bench, correct_bench, pitch_bench, timing_bench, sample_bench): HIP-event timing of a
short call, and the one JSON line a tool ends with."""
import json

import torch


def timed(fn, warmup, iters):
    """(median, minimum) in us of fn(), HIP events around every call (the host time in front of a short launch is inside them: the GPU waits for it)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
    return us[len(us) // 2], us[0]


def emit(line, out=None):
    """print the result as one JSON line; with `out` also write it there"""
    print(json.dumps(line))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(line) + "\n")
