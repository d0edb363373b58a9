// vibrato.hip -- vibrato for the curve the model sings (rule "f13"): a per-note pitch modulation added on the device between the pitch predictor
// (or a guide curve) and vs_pitch_condition, in ONE launch for a padded ragged batch.
// A frame belongs to the note of its token (note_of_token[mel2ph[t] - 1], 0 = a rest); a note is a run of frames with one note id.  Every frame needs the first
// frame of its run and the frame behind its last one -- a segmented scan, as in pitch_ops.hip: one workgroup per row walks the row in chunks of CHUNK = 256 frames,
// twice: right to left for the run's end (parked in offset_q, the lane's own output slot), then left to right for its start; the boundary is carried from chunk
// to chunk in a register, so a note may be longer than any chunk.  Behind the scan everything is integer arithmetic on the frame's own numbers: the phase is a
// 32-bit accumulator step times the frame's position in the note, the sine comes from a host-built table by linear interpolation (no transcendental function is
// evaluated for the offset), the onset delay, the attack and release ramps and the depth are one 64-bit product and one rounded division.  The offset, in 1/16
// cent, then moves the curve by the exp2f / log2f composition pitch_condition_kernel uses for its cents; where the offset is 0 the curve's bits pass through.
// A frame's result depends on its own row's frames only: not on B, the row index or T.  No workspace, no atomics, no host synchronisation.
#include "vs_internal.h"

#include <cmath>

namespace vs {
namespace {

constexpr int CHUNK = 256;          // frames per step of the walk = threads of the workgroup (4 waves)
constexpr int NONE = 0x7fffffff;    // "no boundary on this side yet" of the suffix scan

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

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// token of frame t, clamped to [0, T_ph] (0 = padding), and the note it belongs to (0 = none)
__device__ __forceinline__ int token_at(const long long *__restrict__ m2p, int t, int T_ph) {
    const long long m = m2p[t];
    return m < 0 ? 0 : (m > T_ph ? T_ph : (int)m);
}
__device__ __forceinline__ int note_at(const long long *__restrict__ m2p, const int *__restrict__ notes, int t, int T_ph) {
    const int m = token_at(m2p, t, T_ph);
    return m > 0 ? notes[m - 1] : 0;
}

__global__ void __launch_bounds__(CHUNK) pitch_vibrato_kernel(const float *__restrict__ curve, int stride, const long long *__restrict__ mel2ph,
                                                             const long long *__restrict__ lengths, const int *__restrict__ note_of_token,
                                                             const int *__restrict__ note_depth_q, const int *__restrict__ params,
                                                             const int *__restrict__ sine, int *offset_q, float *__restrict__ curve_out, long long B, int T,
                                                             int T_ph) {
    __shared__ int wave_tot[CHUNK / 64];
    for (long long row = blockIdx.x; row < B; row += gridDim.x) {
        const float *src = curve + row * T * stride;
        const long long *m2p = mel2ph + row * T;
        const int *notes = note_of_token + row * T_ph;
        const int *ndq = note_depth_q ? note_depth_q + row * T_ph : nullptr;
        int *doff = offset_q + row * T;
        float *dst = curve_out + row * T;
        int L = T;
        if (lengths) {
            const long long l = lengths[row];
            L = l < 0 ? 0 : (l > T ? T : (int)l);
        }
        // the item's settings (the caller keeps them in range; out-of-range values are clamped, never trusted)
        const int *pr = params + row * VS_VIBRATO_PARAMS;
        const int depth_item = clampi(pr[0], 0, VS_VIBRATO_MAX_DEPTH_Q);
        const unsigned inc = (unsigned)pr[1];
        const int delay = clampi(pr[2], 0, VS_VIBRATO_MAX_DELAY);
        const int attack = clampi(pr[3], 1, VS_VIBRATO_MAX_RAMP);
        const int release = clampi(pr[4], 1, VS_VIBRATO_MAX_RAMP);
        const int min_len = clampi(pr[5], 0, VS_VIBRATO_MAX_DELAY);
        const long long den = 16384ll * attack * release;

        const int chunks = (L + CHUNK - 1) / CHUNK;
        // pass 1, right to left: end[t], the first frame behind t at which another note begins (L at the latest), parked in offset_q[t]
        int carry = NONE;
        for (int c = chunks - 1; c >= 0; --c) {
            const int t = c * CHUNK + (int)threadIdx.x;
            int v = NONE;
            if (t < L) {
                if (t + 1 == L)
                    v = L;
                else if (note_at(m2p, notes, t + 1, T_ph) != note_at(m2p, notes, t, T_ph))
                    v = t + 1;
            }
            int r = block_suffix_min(v, wave_tot);
            r = min(r, carry);
            if (t < L) doff[t] = r;
            if (threadIdx.x == 0) wave_tot[0] = r;      // thread 0's suffix covers the chunk and everything after it
            __syncthreads();
            carry = wave_tot[0];
            __syncthreads();
        }
        // pass 2, left to right: start[t], the last frame at or before t at which its note begins; then the offset.  (doff[t] was written by this very lane.)
        carry = -1;
        for (int c = 0; c * CHUNK < T; ++c) {
            const int t = c * CHUNK + (int)threadIdx.x;
            if (c >= chunks) {                     // whole chunk beyond the row's length
                if (t < T) {
                    doff[t] = 0;
                    dst[t] = 0.f;
                }
                continue;
            }
            int n = 0, v = -1;
            if (t < L) {
                n = note_at(m2p, notes, t, T_ph);
                if (t == 0 || note_at(m2p, notes, t - 1, T_ph) != n) v = t;
            }
            const int end = t < L ? doff[t] : 0;
            int start = block_prefix_max(v, wave_tot);
            start = max(start, carry);
            if ((int)threadIdx.x == CHUNK - 1) wave_tot[0] = start;
            __syncthreads();
            carry = wave_tot[0];
            __syncthreads();
            if (t >= T) continue;
            if (t >= L) {
                doff[t] = 0;
                dst[t] = 0.f;
                continue;
            }
            const float x = src[(long long)t * stride];
            int off = 0;
            const int p = t - start - delay;
            if (n != 0 && end - start >= min_len && p >= 0) {
                int depth = depth_item;
                if (ndq) {                          // the note's own depth, read at its first token (0 <= start <= t, and n != 0 there: its token is >= 1)
                    const int tok = token_at(m2p, max(start, 0), T_ph);
                    const int dq = tok > 0 ? ndq[tok - 1] : -1;
                    if (dq >= 0) depth = min(dq, VS_VIBRATO_MAX_DEPTH_Q);
                }
                const unsigned ph = inc * (unsigned)p;
                const int i = (int)(ph >> 22), f = (int)((ph >> 6) & 0xFFFFu);
                const int s0 = sine[i], s1 = sine[i + 1];
                const int s = s0 + (((s1 - s0) * f) >> 16);              // arithmetic shift: floor
                const int ea = min(p, attack), er = min(end - t, release);      // end - t = rem + 1
                const long long val = (long long)depth * s * ea * er;
                const long long mag = ((val < 0 ? -val : val) + den / 2) / den;
                off = (int)(val < 0 ? -mag : mag);
            }
            doff[t] = off;
            dst[t] = off == 0 ? x : log2f((exp2f(x) - 1.f) * exp2f((float)off / 19200.f) + 1.f);
        }
    }
}

}  // namespace
}  // namespace vs

using namespace vs;

extern "C" {

int vs_pitch_vibrato(const float *curve, int curve_stride, const int64_t *mel2ph, const int64_t *lengths, const int32_t *note_of_token,
                     const int32_t *note_depth_q, const int32_t *params, const int32_t *sine, int32_t *offset_q, float *curve_out, int64_t B, int64_t T,
                     int64_t T_ph, void *stream) {
    VS_REQUIRE(curve && mel2ph && note_of_token && params && sine && offset_q && curve_out,
               "vs_pitch_vibrato: curve, mel2ph, note_of_token, params, sine, offset_q and curve_out must not be NULL");
    VS_REQUIRE(B > 0 && T > 0 && T_ph > 0, "vs_pitch_vibrato: B, T, T_ph must be positive (got %lld, %lld, %lld)", (long long)B, (long long)T, (long long)T_ph);
    VS_REQUIRE(T < (1ll << 31) - CHUNK && T_ph < (1ll << 31), "vs_pitch_vibrato: T = %lld, T_ph = %lld must be below 2^31", (long long)T, (long long)T_ph);
    VS_REQUIRE(curve_stride == 1 || curve_stride == 2, "vs_pitch_vibrato: curve_stride must be 1 (a [B, T] curve) or 2 (column 0 of [B, T, 2]), got %d", curve_stride);
    VS_REQUIRE(curve_stride == 1 || (reinterpret_cast<uintptr_t>(curve) & 7) == 0, "vs_pitch_vibrato: a [B, T, 2] curve must be 8-byte aligned");
    VS_REQUIRE(B <= INT64_MAX / 2 / T && B <= INT64_MAX / T_ph, "vs_pitch_vibrato: B * T out of range");
    VS_REQUIRE((const void *)curve != (const void *)curve_out && (const void *)offset_q != (const void *)curve_out && (const void *)offset_q != (const void *)curve,
               "vs_pitch_vibrato: curve, offset_q and curve_out must be three buffers (offset_q parks the scan)");
    hipLaunchKernelGGL(pitch_vibrato_kernel, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(CHUNK), 0, as_stream(stream), curve, curve_stride,
                       (const long long *)mel2ph, (const long long *)lengths, note_of_token, note_depth_q, params, sine, offset_q, curve_out, (long long)B, (int)T,
                       (int)T_ph);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // extern "C"
