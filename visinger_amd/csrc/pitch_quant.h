// The frame quantiser of include/visinger_hip.h "f7" (unit: 1/16 semitone), written once: guide_align.hip quantises a guide curve with it, pitch_path.hip the
// lag candidates of a frame ("f12").  The numpy restatement of both is tests/test_guide_align_cpu.py: quantise_f0.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

namespace vs {

constexpr int GA_NONE = INT_MIN;                        // an unvoiced frame / a rest token / an absent candidate

__device__ __forceinline__ int ga_quant(float f) {
    if (!(f > 0.f && f < INFINITY)) return GA_NONE;                           // (NaN fails the compare)
    const float x = 192.f * log2f(f / 440.f);
    return (int)rintf(fminf(fmaxf(x, -40000.f), 40000.f)) + 1104;
}

}  // namespace vs
