#!/usr/bin/env python3
"""The one launch of csrc/pitch_track.hip (pitch_track.extract_f0: vs_f0_yin) on a batch of recordings, and beside it what a host would do instead: the
fp64 numpy restatement of the same rule (tests/test_f0_extract_cpu.py: yin_ref) on ONE row, wall clock.
HIP events around every launch, 10 warm-up + 50 timed; prints the medians and one JSON line with the time per launch, frames/s and the fraction of the fp32
VALU peak for 3 * W * (tau_max + 1) flop per frame (a subtract and a multiply-add per term).  Default: B = 32, T = 1024, hop 256, 24 kHz, 65 - 1000 Hz.
--path: the two launches of tracking as a path instead -- vs_f0_candidates and vs_f0_path, each timed alone, and vs_f0_yin in the same process:
median and minimum per launch, the candidates / yin ratio and the path kernel's time per frame (its frames run one after another: T of them whatever B is)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from visinger_amd import pitch_track  # noqa: E402
from _bench import emit, timed  # noqa: E402

# MI355X fp32 vector peak (spec): 256 CUs x 4 SIMDs x 16 lanes x 2 (packed) x 2 flop (fma) at 2.4 GHz = 157.3 TFLOP/s.  A subtract and a multiply-add per term
# are 3 flop in two instruction slots of 4, so 3/4 of it is this sum's own ceiling when every instruction is packed.
VALU_PEAK_FLOPS = 256 * 4 * 16 * 2 * 2 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x1024,1x1024", help="comma-separated BxT (frames)")
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--sr", type=int, default=24000)
    ap.add_argument("--f0-min", type=float, default=65.0)
    ap.add_argument("--f0-max", type=float, default=1000.0)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-frames", type=int, default=128, help="frames of one row the numpy restatement is timed on (scaled to T)")
    ap.add_argument("--path", action="store_true", help="time vs_f0_candidates, vs_f0_path and vs_f0_yin (tracking as a path, DESIGN.md 4.19)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.path:
        return path_main(args)
    from test_f0_extract_cpu import tone, yin_ref
    tau_min, tau_max = pitch_track.lag_range(args.sr, args.f0_min, args.f0_max)
    W = 2 * tau_max
    flop_per_frame = 3.0 * W * (tau_max + 1)
    results = []
    for shape in args.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(1)
        n = T * args.hop
        rows = np.stack([tone(rng.uniform(90.0, 800.0), n, rng, vibrato=True, sr=args.sr)[0] for _ in range(min(B, 4))]).astype(np.float32)
        wav = torch.from_numpy(rows[np.arange(B) % len(rows)]).cuda()
        lens = torch.full((B,), n, dtype=torch.int64, device="cuda")

        def device():
            return pitch_track.extract_f0(wav, args.hop, args.sr, f0_min=args.f0_min, f0_max=args.f0_max, lengths=lens, frames=T)

        f0 = device()
        voiced = float((f0 > 0).float().mean())
        med, best = timed(device, args.warmup, args.iters)
        k = min(T, args.host_frames)
        t0 = time.perf_counter()
        ref = yin_ref(rows[0][:k * args.hop], sr=args.sr, hop=args.hop, f0_min=args.f0_min, f0_max=args.f0_max)[0]
        host_us = (time.perf_counter() - t0) * 1e6 * T / k
        same = float(((f0[0, :k].cpu().numpy() > 0) == (ref > 0)).mean())
        frac = flop_per_frame * B * T / (med * 1e-6) / VALU_PEAK_FLOPS
        print(f"B={B} T={T} hop={args.hop} sr={args.sr} tau {tau_min}..{tau_max} W={W}: extract_f0 (one launch) median {med:.1f} us (min {best:.1f}), "
              f"{B * T / (med * 1e-6):.3e} frames/s, {100 * frac:.1f} % of the fp32 VALU peak; numpy fp64 restatement, one row of {T} frames (from {k}): "
              f"{host_us / 1e3:.0f} ms; voiced {voiced:.2f}, voicing agrees with it on {same:.3f} of {k} frames", flush=True)
        results.append(dict(B=B, T=T, launch_us_median=round(med, 1), launch_us_min=round(best, 1), frames_per_s=round(B * T / (med * 1e-6)),
                            valu_peak_fraction=round(frac, 4), host_numpy_one_row_ms=round(host_us / 1e3, 1)))
    emit({"tool": "f0_bench", "hop": args.hop, "sr": args.sr, "f0_min": args.f0_min, "f0_max": args.f0_max, "window": W, "tau_max": tau_max,
          "flop_per_frame": flop_per_frame, "warmup": args.warmup, "iters": args.iters, "results": results})


def path_main(args):
    from test_f0_extract_cpu import tone
    results = []
    for shape in args.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(1)
        n = T * args.hop
        rows = np.stack([tone(rng.uniform(90.0, 800.0), n, rng, vibrato=True, sr=args.sr)[0] for _ in range(min(B, 4))]).astype(np.float32)
        wav = torch.from_numpy(rows[np.arange(B) % len(rows)]).cuda()
        lens = torch.full((B,), n, dtype=torch.int64, device="cuda")
        setting = dict(f0_min=args.f0_min, f0_max=args.f0_max, lengths=lens, frames=T)
        n_frames = torch.full((B,), T, dtype=torch.int64, device="cuda")
        cand_hz, cand_d = pitch_track.candidates(wav, args.hop, args.sr, **setting)
        f0 = pitch_track.best_path(cand_hz, cand_d, n_frames)
        plain = pitch_track.extract_f0(wav, args.hop, args.sr, **setting)
        same = float((f0.view(torch.int32) == plain.view(torch.int32)).float().mean())
        per_frame = float((cand_hz > 0).sum(-1).float().mean())
        t_yin = timed(lambda: pitch_track.extract_f0(wav, args.hop, args.sr, **setting), args.warmup, args.iters)
        t_cand = timed(lambda: pitch_track.candidates(wav, args.hop, args.sr, **setting), args.warmup, args.iters)
        t_path = timed(lambda: pitch_track.best_path(cand_hz, cand_d, n_frames), args.warmup, args.iters)
        ratio = t_cand[0] / t_yin[0]
        print(f"B={B} T={T}: vs_f0_yin median {t_yin[0]:.1f} us (min {t_yin[1]:.1f}), vs_f0_candidates {t_cand[0]:.1f} us (min {t_cand[1]:.1f}), ratio {ratio:.3f}; "
              f"vs_f0_path {t_path[0]:.1f} us (min {t_path[1]:.1f}), {1e3 * t_path[0] / T:.1f} ns a frame; {per_frame:.2f} candidates a frame, "
              f"the path equals plain YIN on {same:.4f} of the frames", flush=True)
        results.append(dict(B=B, T=T, yin_us_median=round(t_yin[0], 1), yin_us_min=round(t_yin[1], 1), candidates_us_median=round(t_cand[0], 1),
                            candidates_us_min=round(t_cand[1], 1), candidates_over_yin=round(ratio, 3), path_us_median=round(t_path[0], 1),
                            path_us_min=round(t_path[1], 1), path_ns_per_frame=round(1e3 * t_path[0] / T, 1), candidates_per_frame=round(per_frame, 2),
                            path_equals_yin=round(same, 4)))
    emit({"tool": "f0_bench --path", "hop": args.hop, "sr": args.sr, "f0_min": args.f0_min, "f0_max": args.f0_max, "warmup": args.warmup, "iters": args.iters,
          "weights": pitch_track.PATH_DEFAULTS, "results": results}, args.out)


if __name__ == "__main__":
    main()
