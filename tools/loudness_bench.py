#!/usr/bin/env python3
"""The three launches of csrc/loudness.hip -- vs_loud_steps, vs_loud_gate, vs_gain_apply (loudness.normalize) -- at 48 kHz in two shapes: 32 rows of 262144
samples, and one row of 8 M samples.  Beside them, in the same process on the same bytes: vs_level_track (dynamics.track_level, hop 256: the project's other
pass that reads every sample once and reduces it) and a device-to-device copy.  HIP events around every call; `--rounds` rounds that alternate the five calls,
each with its own warm-up; the medians of the rounds' medians and their spread are reported.  vs_loud_steps walks a row with ONE workgroup, a step of 100 ms
after the other: its time is rows-independent up to 256 rows and grows with a row's length, which is what the two shapes show.  Ends with one JSON line (--out:
also written there)."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visinger_amd import _args as A  # noqa: E402
from visinger_amd import _lib as L  # noqa: E402
from visinger_amd import dynamics as dy  # noqa: E402
from visinger_amd import loudness as lo  # noqa: E402
from _bench import emit, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sr, s = args.rate, lo.check_rate(args.rate)
    lib = L.require_gpu()
    coef = (ctypes.c_double * 10)(*lo.coef_array(sr))
    carry = lo.carry_table(sr, "cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    shapes = {}
    for name, (B, n) in (("rows_32", (32, 262144)), ("row_1", (1, 8 * 1024 * 1024))):
        x = (torch.rand((B, n), device="cuda", generator=g) * 2 - 1) * 0.25
        y = torch.empty_like(x)
        NS = n // s
        S = torch.empty((B, NS), device="cuda", dtype=torch.float64)
        loud = torch.empty(B, device="cuda", dtype=torch.float64)
        gain = torch.empty(B, device="cuda", dtype=torch.float32)
        stats = torch.empty((B, 3), device="cuda", dtype=torch.int32)
        st = L.stream_ptr
        calls = dict(
            loud_steps=lambda: L.check(lib.vs_loud_steps(L.ptr(x), None, B, n, coef, A.vp(carry), s, A.vp(S), NS, st())),
            loud_gate=lambda: L.check(lib.vs_loud_gate(A.vp(S), None, B, NS, s, -23.0, 20.0, A.vp(loud), A.vp(gain), A.vp(stats), st())),
            gain_apply=lambda: L.check(lib.vs_gain_apply(L.ptr(x), A.vp(gain), None, L.ptr(y), B, n, st())),
            level_track=lambda: dy.track_level(x, 256),
            copy=lambda: y.copy_(x))
        rounds = []
        for _ in range(args.rounds):                                             # alternating: the box is shared
            rounds.append({k: timed(fn, 3, args.iters)[0] for k, fn in calls.items()})
        us = {k: float(np.median([r[k] for r in rounds])) for k in calls}
        spread = {k: round(max(r[k] for r in rounds) / min(r[k] for r in rounds), 3) for k in calls}
        steps = B * NS
        print(f"{name}: B = {B} x {n} samples at {sr} Hz ({NS} steps a row), loudness {loud.tolist()[:2]} LUFS, stats {stats[0].tolist()}\n"
              f"  loud_steps {us['loud_steps']:.1f} us ({us['loud_steps'] / NS:.2f} us a step of a row, {B * n / (us['loud_steps'] * 1e-6):.3e} samples/s), "
              f"loud_gate {us['loud_gate']:.1f} us, gain_apply {us['gain_apply']:.1f} us; level_track {us['level_track']:.1f} us, copy {us['copy']:.1f} us; "
              f"loud_steps / level_track = {us['loud_steps'] / us['level_track']:.1f}; max / min over {args.rounds} rounds {spread}", flush=True)
        shapes[name] = dict(rows=B, samples=n, steps_per_row=NS, us={k: round(v, 1) for k, v in us.items()}, us_by_round=[{k: round(v, 1) for k, v in r.items()} for r in rounds],
                            max_over_min_by_round=spread, loud_steps_us_per_row_step=round(us["loud_steps"] / NS, 3),
                            loud_steps_over_level_track=round(us["loud_steps"] / us["level_track"], 2), loud_steps_over_copy=round(us["loud_steps"] / us["copy"], 2),
                            gain_apply_over_copy=round(us["gain_apply"] / us["copy"], 2), total_steps=steps)
    emit({"tool": "loudness_bench", "device": torch.cuda.get_device_name(0), "rate": sr, "warmup": 3, "iters": args.iters, "rounds": args.rounds, **shapes}, args.out)


if __name__ == "__main__":
    main()
