#!/usr/bin/env python3
"""The fused resblock launches of the headline step (csrc/resblock_f16.hip) on two builds of the library in ONE process, interleaved: the production
library against an A/B variant (python tools/build_variant.py rb_mfma32 -DVS_RB_MFMA32 resblock_f16.hip).  B = 32 production shapes, random data, each launch
group as the production table cuts the block; per arm N rounds of REPS back-to-back launches between two HIP events (ms per launch: median, min, max) and
the in-kernel shader clock of one stamped launch.
   python tools/resblock_shape_ab.py build/rb_mfma32/libvisinger_hip.so        Env: N (12), REPS (4), RB_B (32)"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visinger_amd import _lib as L                                   # noqa: E402
from visinger_amd.modules.hipconv import set_conv_math               # noqa: E402
from visinger_amd.modules.visinger.decoder import ResBlock1          # noqa: E402
from visinger_amd.ops import resblock_forward                        # noqa: E402

variant = sys.argv[1]
N, REPS, B = int(os.environ.get("N", 12)), int(os.environ.get("REPS", 4)), int(os.environ.get("RB_B", 32))
WARM = 3

# two libraries in one process: visinger_amd._lib binds whichever `_lib` names; a conv handle belongs to the library that made it
libs = {"production": L.lib()}
L._lib, L.LIB_PATH, os.environ["VS_LIB"] = None, variant, variant
libs[variant] = L.lib()
for lb in libs.values():
    lb.vs_debug_set_stamp_buffer.argtypes = [ctypes.c_void_p]


def use(name):
    L._lib = libs[name]


def groups_of(name, C, k):
    use(name)
    torch.manual_seed(0)
    m = ResBlock1(C, k, (1, 3, 5)).cuda().eval()
    set_conv_math(m, L.MATH_SPLIT3)
    with torch.no_grad():
        m._run_fused(torch.randn(1, C, 512, device="cuda"), torch.empty(1, C, 512, device="cuda"))      # binds the weights
    return m, m._fused_groups(torch.float32)


def clock_of(name, ops, x, out):
    buf = torch.zeros(65536 * 64, dtype=torch.int64, device="cuda")
    libs[name].vs_debug_set_stamp_buffer(ctypes.c_void_p(buf.data_ptr()))
    resblock_forward(ops, x, out)
    torch.cuda.synchronize()
    libs[name].vs_debug_set_stamp_buffer(None)
    full = buf.cpu().numpy().reshape(-1, 64)
    full = full[full[:, 0] != 0]
    end = 2 + 4 * len(ops)
    return float(((full[:, 32 + end] - full[:, 32]) / ((full[:, end] - full[:, 0]) * 10.0)).mean())      # cycles per ns (s_memrealtime: 100 MHz)


for C, T in ((32, 262144), (64, 131072), (128, 65536)):
    x = torch.randn(B, C, T, device="cuda")
    out = torch.empty_like(x)
    for k in (3, 7, 11):
        arms = {name: groups_of(name, C, k) for name in libs}
        if arms["production"][1] is None:
            print(f"C={C} k={k}: conv by conv in production, no fused launch")
            continue
        for gi in range(len(arms["production"][1])):
            times, inst = {name: [] for name in libs}, {}
            with torch.no_grad():
                for rnd in range(N + WARM):
                    for name in libs:
                        use(name)
                        ops = arms[name][1][gi]
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(REPS):
                            resblock_forward(ops, x, out)
                        e1.record()
                        torch.cuda.synchronize()
                        if rnd >= WARM:
                            times[name].append(e0.elapsed_time(e1) / REPS)
                        inst[name] = ops[0].kernel_instance()
                clocks = {}
                for name in libs:
                    use(name)
                    clocks[name] = clock_of(name, arms[name][1][gi], x, out)
            dil = [op.dil for op in arms["production"][1][gi]]
            print(f"C={C} k={k} dil {dil} {inst['production']}  (n = {N} rounds of {REPS} launches per arm, interleaved)")
            for name in libs:
                t = times[name]
                print(f"   {name:38s} median {statistics.median(t):7.3f} min {min(t):7.3f} max {max(t):7.3f} ms   shader clock {clocks[name]:.3f} GHz   [{inst[name]}]")
            a, b = statistics.median(times["production"]), statistics.median(times[variant])
            spread = {n_: max(times[n_]) - min(times[n_]) for n_ in libs}
            print(f"   production / variant = {a / b:.3f}   variant - production = {b - a:+.3f} ms; max - min of the arms {spread['production']:.3f} / {spread[variant]:.3f} ms; "
                  f"slowest production round {'<' if max(times['production']) < min(times[variant]) else '>='} fastest variant round", flush=True)
use("production")
