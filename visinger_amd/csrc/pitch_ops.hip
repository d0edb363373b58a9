// pitch_ops.hip -- the pitch curve of synthesis on the device: a guide curve in Hz -> the model's normalised, gap-interpolated curve, and the frame prior's
// pitch condition (with a transposition in cents and the sung curve back in Hz) in ONE launch each.  DESIGN.md 4.9.
//   vs_f0_norm_interp restates the reference's utils/audio/pitch/utils.py:42-57 (norm_interp_f0: one item at a time through .cpu().numpy() and np.interp) per row of
//   a padded batch: uv = (f0 == 0), f0_norm = log2(f0 + 1) on voiced frames, the straight line between the two voiced neighbours on an unvoiced frame between them,
//   the nearest voiced value before the first / after the last voiced frame (np.interp's edge rule), 0 on a row without a voiced frame and beyond the row's length.
//   A negative or non-finite value counts as unvoiced (the reference gives NaN there).
//   vs_pitch_condition replaces the tail of forward_pitch (models/visinger.py:129-135: two slices, a compare, two multiplies, an unsqueeze) and adds the edits.
// The interpolation is a segmented scan: every frame needs its nearest voiced frame on either side.  One workgroup per row walks the row in chunks of CHUNK = 256
// frames, twice: right to left for the next voiced frame (its index parked in f0_norm, the lane's own output slot), then left to right for the previous one; the
// boundary frame is carried from chunk to chunk in a register.  The two anchor values are re-read from f0_hz (two gathers that hit the cache), so the result of a
// frame depends on the row's own frames only: not on B, the row index or T.  No workspace, no atomics, no host synchronisation; precise log2f / exp2f.
#include "vs_internal.h"

#include <cmath>

namespace vs {

constexpr int CHUNK = 256;          // frames per step of the walk = threads of the workgroup (4 waves)

__device__ __forceinline__ bool is_voiced(float hz) { return hz > 0.f && hz < INFINITY; }      // (NaN fails both compares)

// inclusive max over the lanes <= this one of the workgroup (wave scan by lane shifts, the four wave totals through LDS)
__device__ __forceinline__ int block_prefix_max(int v, int *wave_tot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v = max(v, o);
    }
    if (lane == 63) wave_tot[w] = v;
    __syncthreads();
    for (int i = 0; i < w; ++i) v = max(v, wave_tot[i]);
    __syncthreads();
    return v;
}

// inclusive min over the lanes >= this one of the workgroup
__device__ __forceinline__ int block_suffix_min(int v, int *wave_tot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(v, d);
        if (lane + d < 64) v = min(v, o);
    }
    if (lane == 0) wave_tot[w] = v;
    __syncthreads();
    for (int i = w + 1; i < CHUNK / 64; ++i) v = min(v, wave_tot[i]);
    __syncthreads();
    return v;
}

__global__ void __launch_bounds__(CHUNK) f0_norm_interp_kernel(const float *__restrict__ f0_hz, const long long *__restrict__ lengths, float *f0_norm,
                                                               float *__restrict__ uv, long long B, int T) {
    __shared__ int wave_tot[CHUNK / 64];
    const int NONE = 0x7fffffff;                   // "no voiced frame on this side" of the suffix scan (prefix scan: -1)
    for (long long row = blockIdx.x; row < B; row += gridDim.x) {
        const float *src = f0_hz + row * T;
        float *dst = f0_norm + row * T, *duv = uv + row * T;
        int *next = reinterpret_cast<int *>(dst);
        int L = T;
        if (lengths) {
            const long long l = lengths[row];
            L = l < 0 ? 0 : (l > T ? T : (int)l);
        }
        const int chunks = (L + CHUNK - 1) / CHUNK;
        // pass 1, right to left: index of the nearest voiced frame at or after t
        int carry = NONE;
        for (int c = chunks - 1; c >= 0; --c) {
            const int t = c * CHUNK + (int)threadIdx.x;
            const bool v = t < L && is_voiced(src[t]);
            int r = block_suffix_min(v ? t : NONE, wave_tot);
            r = min(r, carry);
            if (t < L) next[t] = r;
            if (threadIdx.x == 0) wave_tot[0] = r;      // thread 0's suffix covers the chunk and everything after it
            __syncthreads();
            carry = wave_tot[0];
            __syncthreads();
        }
        // pass 2, left to right: nearest voiced frame at or before t, then the value.  (next[t] was written by this very lane.)
        carry = -1;
        for (int c = 0; c * CHUNK < T; ++c) {
            const int t = c * CHUNK + (int)threadIdx.x;
            if (c >= chunks) {                     // whole chunk beyond the row's length: the padding the reference's collate writes
                if (t < T) {
                    dst[t] = 0.f;
                    duv[t] = 0.f;
                }
                continue;
            }
            const float hz = t < L ? src[t] : 0.f;
            const bool v = t < L && is_voiced(hz);
            const int ri = t < L ? next[t] : NONE;
            int li = block_prefix_max(v ? t : -1, wave_tot);
            li = max(li, carry);
            if ((int)threadIdx.x == CHUNK - 1) wave_tot[0] = li;
            __syncthreads();
            carry = wave_tot[0];
            __syncthreads();
            if (t >= T) continue;
            float y = 0.f;
            if (t < L) {
                if (v) {
                    y = log2f(hz + 1.f);
                } else if (li >= 0 && ri != NONE) {
                    const float a = log2f(src[li] + 1.f), b = log2f(src[ri] + 1.f);
                    y = fmaf((b - a) / (float)(ri - li), (float)(t - li), a);       // np.interp's form: slope * (x - x0) + y0; distances < 2^24 are exact
                } else if (li >= 0) {
                    y = log2f(src[li] + 1.f);
                } else if (ri != NONE) {
                    y = log2f(src[ri] + 1.f);
                }
            }
            dst[t] = y;
            duv[t] = (t < L && !v) ? 1.f : 0.f;
        }
    }
}

// one lane per (row, frame), lanes along t; pred is [B, T, 2] (curve, voicing logit): one 8-byte load per lane
__global__ void __launch_bounds__(256) pitch_condition_kernel(const float *__restrict__ pred, const float *__restrict__ f0_norm, const float *__restrict__ uv,
                                                              const float *__restrict__ mask, const float *__restrict__ cents, float *__restrict__ cond,
                                                              float *__restrict__ f0_hz_out, long long B, long long T) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    for (long long b = blockIdx.y; b < B; b += gridDim.y) {
        const long long i = b * T + t;
        float2 p = make_float2(0.f, 0.f);
        if (pred) p = reinterpret_cast<const float2 *>(pred)[i];
        float x = f0_norm ? f0_norm[i] : p.x;
        const bool voiced = uv ? uv[i] == 0.f : p.y <= 0.f;
        const float c = cents ? cents[b] : 0.f;
        if (c != 0.f) x = log2f((exp2f(x) - 1.f) * exp2f(c / 1200.f) + 1.f);
        const float m = mask ? mask[i] : 1.f;
        const bool on = voiced && m != 0.f;
        cond[i] = on ? x * m : 0.f;
        if (f0_hz_out) f0_hz_out[i] = on ? fminf(fmaxf(exp2f(x) - 1.f, 50.f), 1250.f) : 0.f;      // denorm_f0's default range (pitch/utils.py:12-13, 60-69)
    }
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_f0_norm_interp(const float *f0_hz, const int64_t *lengths, float *f0_norm, float *uv, int64_t B, int64_t T, void *stream) {
    VS_REQUIRE(f0_hz && f0_norm && uv, "vs_f0_norm_interp: f0_hz, f0_norm and uv must not be NULL");
    VS_REQUIRE(B > 0 && T > 0, "vs_f0_norm_interp: B, T must be positive (got %lld, %lld)", (long long)B, (long long)T);
    VS_REQUIRE(T < (1ll << 24), "vs_f0_norm_interp: T = %lld is not below 2^24 (frame distances must be exact in fp32)", (long long)T);
    VS_REQUIRE(f0_norm != f0_hz && uv != f0_hz && uv != f0_norm, "vs_f0_norm_interp: f0_hz, f0_norm and uv must be three buffers (f0_hz is re-read, f0_norm parks the scan)");
    VS_REQUIRE(B <= INT64_MAX / T, "vs_f0_norm_interp: B * T out of range");
    hipLaunchKernelGGL(f0_norm_interp_kernel, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(CHUNK), 0, as_stream(stream), f0_hz, (const long long *)lengths,
                       f0_norm, uv, (long long)B, (int)T);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

int vs_pitch_condition(const float *pred, const float *f0_norm, const float *uv, const float *mask, const float *cents, float *cond, float *f0_hz_out,
                       int64_t B, int64_t T, void *stream) {
    VS_REQUIRE(cond, "vs_pitch_condition: cond must not be NULL");
    VS_REQUIRE(B > 0 && T > 0, "vs_pitch_condition: B, T must be positive (got %lld, %lld)", (long long)B, (long long)T);
    VS_REQUIRE(pred || f0_norm, "vs_pitch_condition: one of pred and f0_norm is required (the curve)");
    VS_REQUIRE(pred || uv, "vs_pitch_condition: uv == NULL takes the voicing from pred, which is NULL");
    VS_REQUIRE(B <= INT64_MAX / 2 / T, "vs_pitch_condition: B * T out of range");
    VS_REQUIRE((reinterpret_cast<uintptr_t>(pred) & 7) == 0, "vs_pitch_condition: pred must be 8-byte aligned (its [t, 2] pairs are read as one load)");
    VS_REQUIRE(ceil_div(T, 256) <= 0x7fffffff, "vs_pitch_condition: T = %lld exceeds the grid", (long long)T);
    hipLaunchKernelGGL(pitch_condition_kernel, dim3((unsigned)ceil_div(T, 256), (unsigned)(B < 65535 ? B : 65535)), dim3(256), 0, as_stream(stream), pred, f0_norm,
                       uv, mask, cents, cond, f0_hz_out, (long long)B, (long long)T);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // extern "C"
