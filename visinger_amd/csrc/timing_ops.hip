// timing_ops.hip -- tempo and duration control of synthesis on the device: the frame alignment mel2ph (and a curve that lives on its timeline) retimed by a
// factor per token and a tempo per item, in TWO launches.  DESIGN.md 4.10.  Not in the reference, which can only replay the score's own timing
// (utils/audio/align.py builds mel2ph once per utterance on the host; there is no length regulator).
//   vs_retime_tokens  per item: old durations d_i (an integer LDS histogram of mel2ph, or given), factor f_i = stretch_i / tempo in 16.16 fixed point,
//                     new token ends e_i = max(e_{i-1} + m_i, (sum_{j<=i} d_j s_j + 2^15) >> 16) with m_i = min_frames on tokens that had frames.
//   vs_retime_frames  per new frame: its token (upper bound in the row of new ends) and, optionally, a curve resampled inside that token.
// The recurrence has the closed form e_i = M_i + max(0, max_{j<=i}(R_j - M_j)), M = prefix sum of m, R the rounded prefix sum: one workgroup per item walks
// the tokens in chunks of CHUNK = 256, a wave64 scan by lane shifts inside a chunk, the four wave totals through LDS, and three running values (sum of d s,
// sum of m, max of R - M; plus the sum of d for the old ends) carried from chunk to chunk.  Everything after the one fp32 division and the rintf is int64: no
// float atomics, nothing depends on the launch shape, and a row's result depends on that row only.  No workspace, no host synchronisation.
#include "vs_internal.h"

#include <cmath>

namespace vs {

constexpr int CHUNK = 256;                     // tokens per step of the scan = threads of the workgroup (4 waves)
constexpr int MAX_TOKENS = 8192;               // the LDS histogram: 8192 x 4 bytes = 32 KiB of the workgroup's 64 KiB
constexpr long long MAX_DUR = (1ll << 24) - 1; // a token's frames (given durations are clamped to it): d s stays below 2^46, 8192 of them below 2^59
constexpr long long NEG = -(1ll << 62);        // identity of the prefix max (tokens beyond the row)

// inclusive sums over the lanes <= this one of the workgroup, three at a time
__device__ __forceinline__ void block_prefix_add3(long long &a, long long &b, long long &c, long long (*wave_tot)[3]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long oa = __shfl_up(a, d), ob = __shfl_up(b, d), oc = __shfl_up(c, d);
        if (lane >= d) {
            a += oa;
            b += ob;
            c += oc;
        }
    }
    if (lane == 63) {
        wave_tot[w][0] = a;
        wave_tot[w][1] = b;
        wave_tot[w][2] = c;
    }
    __syncthreads();
    for (int i = 0; i < w; ++i) {
        a += wave_tot[i][0];
        b += wave_tot[i][1];
        c += wave_tot[i][2];
    }
    __syncthreads();
}

// inclusive max over the lanes <= this one of the workgroup
__device__ __forceinline__ long long block_prefix_max(long long v, long long (*wave_tot)[3]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(v, d);
        if (lane >= d) v = max(v, o);
    }
    if (lane == 63) wave_tot[w][0] = v;
    __syncthreads();
    for (int i = 0; i < w; ++i) v = max(v, wave_tot[i][0]);
    __syncthreads();
    return v;
}

__global__ void __launch_bounds__(CHUNK) retime_tokens_kernel(const long long *__restrict__ mel2ph, const long long *__restrict__ dur,
                                                              const float *__restrict__ stretch, const float *__restrict__ tempo, long long min_frames,
                                                              long long max_frames, long long *__restrict__ cum_old, long long *__restrict__ cum_new,
                                                              long long *__restrict__ lengths, long long B, int T_frames, int T_tokens) {
    __shared__ unsigned int hist[MAX_TOKENS];
    __shared__ long long wave_tot[CHUNK / 64][3];
    __shared__ long long carry[4];
    for (long long row = blockIdx.x; row < B; row += gridDim.x) {
        if (mel2ph) {
            for (int i = threadIdx.x; i < T_tokens; i += CHUNK) hist[i] = 0u;
            __syncthreads();
            const long long *src = mel2ph + row * T_frames;
            for (int t = threadIdx.x; t < T_frames; t += CHUNK) {
                const long long i = src[t];
                if (i > 0 && i <= T_tokens) atomicAdd(&hist[i - 1], 1u);      // integer: order-independent
            }
            __syncthreads();
        }
        const float tp = tempo ? tempo[row] : 1.f;
        long long sum_d = 0, sum_p = 0, sum_m = 0, top = 0;                   // the carries: c, P, M and max(0, max(R - M)) up to the previous chunk
        for (int c0 = 0; c0 < T_tokens; c0 += CHUNK) {
            const int i = c0 + (int)threadIdx.x;
            const bool in = i < T_tokens;
            long long d = 0;
            float f = 1.f;
            if (in) {
                if (mel2ph) {
                    d = (long long)hist[i];
                } else {
                    d = dur[row * T_tokens + i];
                    d = d < 0 ? 0 : (d > MAX_DUR ? MAX_DUR : d);
                }
                f = (stretch ? stretch[row * T_tokens + i] : 1.f) / tp;
            }
            if (!(fabsf(f) < INFINITY)) f = 1.f;                              // (NaN fails the compare)
            f = fminf(fmaxf(f, 0.015625f), 64.f);
            const long long s = (long long)rintf(f * 65536.f);                // exact: a power of two, then ties-to-even
            long long p = d * s, m = d > 0 ? min_frames : 0;
            block_prefix_add3(d, p, m, wave_tot);
            d += sum_d;
            p += sum_p;
            m += sum_m;
            const long long r = (p + 32768) >> 16;
            long long x = block_prefix_max(in ? r - m : NEG, wave_tot);
            x = max(x, top);
            if (in) {
                cum_old[row * T_tokens + i] = d;
                cum_new[row * T_tokens + i] = m + x;
            }
            if ((int)threadIdx.x == CHUNK - 1) {                              // (lanes beyond the row added nothing: the row's totals)
                carry[0] = d;
                carry[1] = p;
                carry[2] = m;
                carry[3] = x;
            }
            __syncthreads();
            sum_d = carry[0];
            sum_p = carry[1];
            sum_m = carry[2];
            top = carry[3];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const long long e = sum_m + top;
            lengths[row] = (max_frames > 0 && e > max_frames) ? max_frames : e;
        }
    }
}

// one lane per (row, new frame), lanes along t
__global__ void __launch_bounds__(256) retime_frames_kernel(const long long *__restrict__ cum_old, const long long *__restrict__ cum_new,
                                                            const long long *__restrict__ lengths, const float *__restrict__ curve, long long curve_T,
                                                            long long *__restrict__ mel2ph_out, float *__restrict__ curve_out, long long B, int T_tokens,
                                                            long long T_out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T_out) return;
    for (long long b = blockIdx.y; b < B; b += gridDim.y) {
        const long long *ce = cum_new + b * T_tokens, *co = cum_old + b * T_tokens;
        long long token = 0;
        float v = 0.f;
        if (t < lengths[b]) {
            int lo = 0, hi = T_tokens;                                        // the smallest i with e_i > t
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ce[mid] > t) hi = mid;
                else lo = mid + 1;
            }
            if (lo < T_tokens) {
                token = lo + 1;
                const long long e0 = lo ? ce[lo - 1] : 0, c0 = lo ? co[lo - 1] : 0;
                const long long n = co[lo] - c0, n2 = ce[lo] - e0, u = t - e0;
                if (curve_out && n > 0 && n2 > 0 && u >= 0) {
                    const long long num = (2 * u + 1) * n - n2, den = 2 * n2;
                    long long k = 0;
                    float w = 0.f;
                    if (num >= 0) {
                        k = num / den;
                        w = (float)(num - k * den) / (float)den;
                    }
                    if (k >= n - 1) {
                        k = n - 1;
                        w = 0.f;
                    }
                    const long long ia = c0 + k, ib = c0 + (k + 1 < n ? k + 1 : n - 1);
                    const float *src = curve + b * curve_T;
                    const float ya = (ia >= 0 && ia < curve_T) ? src[ia] : 0.f, yb = (ib >= 0 && ib < curve_T) ? src[ib] : 0.f;
                    if (w == 0.f) v = ya;                                     // (a copy keeps its bits)
                    else if (ya > 0.f && yb > 0.f) v = ya + w * (yb - ya);
                    else v = w < 0.5f ? ya : yb;                              // an unvoiced frame is never blended
                }
            }
        }
        mel2ph_out[b * T_out + t] = token;
        if (curve_out) curve_out[b * T_out + t] = v;
    }
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_retime_tokens(const int64_t *mel2ph, const int64_t *dur, const float *stretch, const float *tempo, int64_t min_frames, int64_t max_frames,
                     int64_t *cum_old, int64_t *cum_new, int64_t *lengths, int64_t B, int64_t T_frames, int64_t T_tokens, void *stream) {
    VS_REQUIRE((mel2ph != nullptr) != (dur != nullptr), "vs_retime_tokens: give exactly one of mel2ph and dur");
    VS_REQUIRE(cum_old && cum_new && lengths, "vs_retime_tokens: cum_old, cum_new and lengths must not be NULL");
    VS_REQUIRE(cum_old != cum_new && cum_old != dur && cum_new != dur, "vs_retime_tokens: dur, cum_old and cum_new must be distinct buffers");
    VS_REQUIRE(B > 0 && T_tokens > 0, "vs_retime_tokens: B, T_tokens must be positive (got %lld, %lld)", (long long)B, (long long)T_tokens);
    VS_REQUIRE(T_tokens <= MAX_TOKENS, "vs_retime_tokens: T_tokens = %lld exceeds %d (the LDS histogram)", (long long)T_tokens, MAX_TOKENS);
    VS_REQUIRE(!mel2ph || (T_frames > 0 && T_frames < (1ll << 24)), "vs_retime_tokens: T_frames = %lld is not in [1, 2^24)", (long long)T_frames);
    VS_REQUIRE(min_frames >= 0 && min_frames <= 65536, "vs_retime_tokens: min_frames = %lld is not in [0, 65536]", (long long)min_frames);
    VS_REQUIRE(max_frames >= 0, "vs_retime_tokens: max_frames = %lld is negative (0 = no capacity)", (long long)max_frames);
    hipLaunchKernelGGL(retime_tokens_kernel, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(CHUNK), 0, as_stream(stream), (const long long *)mel2ph,
                       (const long long *)dur, stretch, tempo, (long long)min_frames, (long long)max_frames, (long long *)cum_old, (long long *)cum_new,
                       (long long *)lengths, (long long)B, (int)(mel2ph ? T_frames : 0), (int)T_tokens);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

int vs_retime_frames(const int64_t *cum_old, const int64_t *cum_new, const int64_t *lengths, const float *curve, int64_t curve_T, int64_t *mel2ph_out,
                     float *curve_out, int64_t B, int64_t T_tokens, int64_t T_out, void *stream) {
    VS_REQUIRE(cum_old && cum_new && lengths && mel2ph_out, "vs_retime_frames: cum_old, cum_new, lengths and mel2ph_out must not be NULL");
    VS_REQUIRE((curve != nullptr) == (curve_out != nullptr), "vs_retime_frames: curve and curve_out go together (both or neither)");
    VS_REQUIRE(!curve || (curve_T > 0 && curve != curve_out), "vs_retime_frames: curve needs curve_T > 0 (got %lld) and its own output buffer", (long long)curve_T);
    VS_REQUIRE(B > 0 && T_tokens > 0 && T_out > 0, "vs_retime_frames: B, T_tokens, T_out must be positive (got %lld, %lld, %lld)", (long long)B,
               (long long)T_tokens, (long long)T_out);
    VS_REQUIRE(T_tokens <= MAX_TOKENS, "vs_retime_frames: T_tokens = %lld exceeds %d", (long long)T_tokens, MAX_TOKENS);
    VS_REQUIRE(T_out < (1ll << 31) && B <= INT64_MAX / T_out, "vs_retime_frames: T_out = %lld is not below 2^31, or B * T_out is out of range", (long long)T_out);
    hipLaunchKernelGGL(retime_frames_kernel, dim3((unsigned)ceil_div(T_out, 256), (unsigned)(B < 65535 ? B : 65535)), dim3(256), 0, as_stream(stream),
                       (const long long *)cum_old, (const long long *)cum_new, (const long long *)lengths, curve, (long long)curve_T, (long long *)mel2ph_out,
                       curve_out, (long long)B, (int)T_tokens, (long long)T_out);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // extern "C"
