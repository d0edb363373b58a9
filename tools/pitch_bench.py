#!/usr/bin/env python3
"""The two launches of csrc/pitch_ops.hip against what they replace, on the same inputs:
  vs_pitch_condition against the aten chain of forward_pitch's tail, ``(pred[:, :, 0] * (pred[:, :, 1] <= 0)).unsqueeze(1) * mask`` (two slices, a compare,
  two multiplies), pred being the pitch predictor's strided [B, T, 2] view;
  vs_f0_norm_interp against the host chain of the reference (norm_interp_f0 per item: ``.cpu().numpy()``, ``np.interp``, back to the device, padded) --
  restated here with numpy, wall-clock time including the two transfers, since that chain synchronises with the host by construction.
HIP events around every iteration for the device-only paths, 20 warm-up + 100 timed; prints the medians and one JSON line.  Default: B = 32, T = 1024.
--vibrato: instead, vs_pitch_vibrato (csrc/vibrato.hip) beside vs_f0_norm_interp -- the closest existing kernel: the same two-direction row scan,
the same traffic class -- in one process: both through the C entry on prepared pointers (the launch alone) and vibrato.vibrato as Python calls it, 10 warm-up +
30 timed launches each, on a score of notes of 20 .. 120 frames with rests; the ratio of the medians; whether the launch equals the numpy restatement on row 0."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visinger_amd import pitch, vibrato  # noqa: E402
from visinger_amd import _args as A, _lib as L  # noqa: E402
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


def vibrato_main(args):
    lib = L.require_gpu()
    warmup, iters = 10, 30
    results = []
    for shape in args.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        r = np.random.default_rng(7)
        T_ph = T // 16
        m2p, notes = np.zeros((B, T), np.int64), np.zeros((B, T_ph), np.int32)
        for b in range(B):
            t, k = 0, 0
            while t < T and k < T_ph:
                n = int(r.integers(20, 121))
                notes[b, k] = 0 if r.uniform() < 0.2 else k + 1
                m2p[b, t:t + n] = k + 1
                t, k = t + n, k + 1
        lens_host = (m2p > 0).sum(axis=1)
        g = torch.Generator(device="cuda").manual_seed(1)
        pred = torch.randn(B, T, 2, device="cuda", generator=g)
        pred[:, :, 0].mul_(0.5).add_(8.0)
        curve = pred[:, :, 0].contiguous()
        f0_hz = torch.rand(B, T, device="cuda", generator=g) * 800 + 80
        f0_hz[torch.rand(B, T, device="cuda", generator=g) < 0.4] = 0
        m2p_d, notes_d, lens = torch.from_numpy(m2p).cuda(), torch.from_numpy(notes).cuda(), torch.from_numpy(lens_host).cuda()
        prm = vibrato.params(B, 24000, 256, "cuda")
        sine = vibrato.sine_table("cuda")
        off, out = torch.empty((B, T), dtype=torch.int32, device="cuda"), torch.empty((B, T), device="cuda")
        f0n, uv = torch.empty_like(f0_hz), torch.empty_like(f0_hz)
        st = L.stream_ptr()

        def vib_launch(stride):
            src = curve if stride == 1 else pred
            return lambda: L.check(lib.vs_pitch_vibrato(L.ptr(src), stride, A.vp(m2p_d), A.vp(lens), A.vp(notes_d), None, A.vp(prm), A.vp(sine), A.vp(off),
                                                        L.ptr(out), B, T, T_ph, st))

        def interp_launch():
            L.check(lib.vs_f0_norm_interp(L.ptr(f0_hz), A.vp(lens), L.ptr(f0n), L.ptr(uv), B, T, st))

        with torch.no_grad():
            i_med, i_min = timed(interp_launch, warmup, iters)
            v1_med, v1_min = timed(vib_launch(1), warmup, iters)
            v2_med, v2_min = timed(vib_launch(2), warmup, iters)
            i2_med, i2_min = timed(interp_launch, warmup, iters)                 # (again behind the vibrato launches: the order is not what the ratio shows)
            p_med, p_min = timed(lambda: vibrato.vibrato(curve, m2p_d, notes_d, prm, lengths=lens), warmup, iters)
            vib_launch(1)()
            torch.cuda.synchronize()
        want, _ = vibrato.vibrato_ref(curve[:1].cpu().numpy(), m2p[:1], notes[:1], prm[:1].cpu().numpy())
        equal = bool(np.array_equal(off[0].cpu().numpy(), want[0]))
        interp = min(i_med, i2_med)
        print(f"B={B} T={T}: vs_pitch_vibrato median {v1_med:.1f} us (min {v1_min:.1f}), stride 2 {v2_med:.1f} us (min {v2_min:.1f}); vs_f0_norm_interp median "
              f"{i_med:.1f} / {i2_med:.1f} us (min {min(i_min, i2_min):.1f}); ratio {v1_med / interp:.2f}; vibrato.vibrato {p_med:.1f} us; row 0 equals the "
              f"restatement: {equal}; modulated frames of row 0: {int((want != 0).sum())}", flush=True)
        results.append(dict(B=B, T=T, T_ph=T_ph, vibrato_us_median=round(v1_med, 2), vibrato_us_min=round(v1_min, 2), vibrato_stride2_us_median=round(v2_med, 2),
                            vibrato_stride2_us_min=round(v2_min, 2), interp_us_median=round(i_med, 2), interp_again_us_median=round(i2_med, 2),
                            interp_us_min=round(min(i_min, i2_min), 2), ratio_to_interp=round(v1_med / interp, 3), python_call_us_median=round(p_med, 2),
                            equals_restatement=equal, modulated_frames_row0=int((want != 0).sum())))
    emit({"tool": "pitch_bench --vibrato", "warmup": warmup, "iters": iters, "results": results}, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x1024,1x1024", help="comma-separated BxT")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--vibrato", action="store_true", help="time vs_pitch_vibrato beside vs_f0_norm_interp (10 warm-up + 30 timed) instead")
    ap.add_argument("--out", default=None, help="with --vibrato: also write the JSON line there (profiles/vibrato_bench.json)")
    args = ap.parse_args()
    if args.vibrato:
        return vibrato_main(args)
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
