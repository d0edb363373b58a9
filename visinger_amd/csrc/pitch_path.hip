// pitch_path.hip -- the pitch curve as a path: a Viterbi choice among the lag candidates of every frame (vs_f0_candidates, pitch_track.hip) over a whole phrase,
// the pYIN / "Tony" construction in integers (include/visinger_hip.h "f12").  Not in the reference, whose extractors run on the host.
// Eight states a frame: the candidate slots 0 .. 6 and "unvoiced" (7).  ONE wave per item, one launch for the batch:
//   staging    64 frames at a time: lane l quantises 8 of the 512 (frame, slot) entries (f7's quantiser) into LDS -- q and the local cost; the next chunk's raw
//              candidates are fetched into registers before the frames of the current one run, so the global latency sits under the serial loop.
//   forward    sequential over the frames.  Lane (j = lane >> 3, i = lane & 7) forms D(t-1, i) + trans(i -> j); three xor steps inside the 8 lanes of a group
//              leave min_i and the lowest argmin in all of them; one lane shuffle hands D(t, i) of group i back to the lanes (., i).  Lane (j, 0) writes the
//              backpointer of state j as a byte; after the chunk lane l packs frame l's eight bytes into 8 x 3 bits of one dword of dynamic LDS (4 T bytes).
//   backtrack  64 frames at a time: lane l fetches the dword of frame t0 - l, the chain is resolved on read-lane values, then every lane writes its own frame.
// Integer throughout once quantised: bit-reproducible, and a row's result depends on that row's first N frames only.  No atomics, no workspace, no host
// synchronisation.  The wave's LDS operations complete in order; the barriers of the one-wave workgroup only keep the compiler from moving them.
#include "vs_internal.h"
#include "pitch_quant.h"

#include <cmath>

namespace vs {

constexpr int FP_MAX_FRAMES = VS_F0_PATH_MAX_FRAMES;    // 4 T bytes of backpointers: 128 KiB of the CU's 160
constexpr int FP_WEIGHT_MAX = 4096;
constexpr int FP_ABSENT = 16384;                        // local cost of a slot that holds no candidate
constexpr int FP_CHUNK = 64;

struct FpWeights {
    int w_unvoiced, w_switch, w_order, w_jump, jump_cap;
};

// (min, argmin) over the 8 lanes of a group, the lowest index on a tie; every lane of the group ends with the result
__device__ __forceinline__ void fp_min8(int &v, int &a) {
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) {
        const int ov = __shfl_xor(v, s), oa = __shfl_xor(a, s);
        if (ov < v || (ov == v && oa < a)) v = ov, a = oa;
    }
}

__global__ void __launch_bounds__(64) f0_path_kernel(const float *__restrict__ cand_hz, const float *__restrict__ cand_d, const long long *__restrict__ n_frames,
                                                     FpWeights wt, float *__restrict__ f0_hz, int *__restrict__ state, int *__restrict__ cost, long long B, int T) {
    extern __shared__ unsigned bp[];                                         // [T]: frame t's eight backpointers, 3 bits each (word 0 is never read)
    __shared__ int sq[FP_CHUNK * 8], sl[FP_CHUNK * 8];                       // q(t, k) (GA_NONE: absent, or k = 7) and loc(t, k) of the current chunk
    __shared__ unsigned sb[FP_CHUNK * 2];                                    // the chunk's backpointers as bytes [frame][state]
    unsigned char *sbb = reinterpret_cast<unsigned char *>(sb);
    const int lane = threadIdx.x, i = lane & 7, j = lane >> 3;
    for (long long row = blockIdx.x; row < B; row += gridDim.x) {
        const long long n_raw = n_frames ? n_frames[row] : (long long)T;
        const int N = (int)(n_raw < 0 ? 0 : (n_raw > T ? (long long)T : n_raw));
        const float *hz = cand_hz + row * T * 8, *dd = cand_d + row * T * 8;
        float *out = f0_hz + row * T;
        int *st = state ? state + row * T : nullptr;
        for (int t = N + lane; t < T; t += 64) {                             // frames beyond the row
            out[t] = 0.f;
            if (st) st[t] = -1;
        }
        if (N == 0) {
            if (cost && lane == 0) cost[row] = 0;
            continue;
        }
        // entry r of a lane in chunk c: (frame c 64 + r 8 + j, slot i) -- index r 64 + lane of the chunk's 512
        float rh[8], rd[8];
        auto fetch = [&](int c) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int t = c * FP_CHUNK + r * 8 + j;
                rh[r] = t < N ? hz[(long long)t * 8 + i] : 0.f;
                rd[r] = t < N ? dd[(long long)t * 8 + i] : 1.f;
            }
        };
        auto stage = [&]() {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                int q = GA_NONE, loc = wt.w_unvoiced;
                if (i < 7) {
                    q = ga_quant(rh[r]);
                    const float d = rd[r] != rd[r] ? 1.f : fminf(fmaxf(rd[r], 0.f), 1.f);     // (a NaN counts as 1)
                    loc = q == GA_NONE ? FP_ABSENT : min((int)rintf(1024.f * d), 1024) + wt.w_order * i;
                }
                sq[r * 64 + lane] = q;
                sl[r * 64 + lane] = loc;
            }
        };
        fetch(0);
        __syncthreads();                                                     // (the previous row's readers of sq / sl / bp are done)
        stage();
        __syncthreads();
        int D = sl[i], qp = sq[i];                                           // D(0, i), q(0, i): the lanes (., i) hold state i of the previous frame
        for (int c = 0; c * FP_CHUNK < N; ++c) {
            const bool more = (c + 1) * FP_CHUNK < N;
            if (more) fetch(c + 1);                                          // (in flight under this chunk's frames)
            const int t_end = min(N, (c + 1) * FP_CHUNK);
            for (int t = max(1, c * FP_CHUNK); t < t_end; ++t) {
                const int o = (t & (FP_CHUNK - 1)) * 8;
                const int qj = sq[o + j], lj = sl[o + j], qn = sq[o + i];
                int tr;                                                      // trans(i -> j): does not wait for D
                if (i == 7 || j == 7) tr = i == j ? 0 : wt.w_switch;
                else if (qp == GA_NONE || qj == GA_NONE) tr = 0;
                else tr = min((abs(qp - qj) * wt.w_jump) >> 4, wt.jump_cap);
                int v = D + tr, a = i;
                fp_min8(v, a);
                v += lj;                                                     // D(t, j), in the 8 lanes of group j
                if (i == 0) sbb[o + j] = (unsigned char)a;
                D = __shfl(v, i * 8);                                        // D(t, i) from group i
                qp = qn;
            }
            __syncthreads();
            {                                                                // lane l packs frame c 64 + l
                const int t = c * FP_CHUNK + lane;
                if (t >= 1 && t < t_end) {
                    const unsigned lo = sb[lane * 2], hi = sb[lane * 2 + 1];
                    unsigned w = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) w |= (((lo >> (8 * k)) & 7u) << (3 * k)) | (((hi >> (8 * k)) & 7u) << (3 * k + 12));
                    bp[t] = w;
                }
            }
            if (more) {
                __syncthreads();                                             // (the pack has read sb, the frames have read sq / sl)
                stage();
            }
            __syncthreads();
        }
        // the end state: the lowest argmin of D(N - 1, .); lanes (0, i) hold D(N - 1, i)
        int v = D, s = i;
        fp_min8(v, s);
        v = __builtin_amdgcn_readfirstlane(v);
        s = __builtin_amdgcn_readfirstlane(s);
        if (cost && lane == 0) cost[row] = v;
        for (int t0 = N - 1; t0 >= 0; t0 -= 64) {
            const int t = t0 - lane;
            const int w = t >= 1 ? (int)bp[t] : 0;
            int mine = 0;
#pragma unroll
            for (int l = 0; l < 64; ++l) {                                   // s is the state of frame t0 - l; rows before frame 1 hold 0 and are not written
                if (lane == l) mine = s;
                s = (int)(((unsigned)__builtin_amdgcn_readlane(w, l) >> (3 * s)) & 7u);
            }
            if (t >= 0) {
                float f = 0.f;
                if (mine < 7) {
                    const float h = hz[(long long)t * 8 + mine];
                    if (h > 0.f && h < INFINITY) f = h;
                }
                out[t] = f;
                if (st) st[t] = mine;
            }
        }
        __syncthreads();
    }
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_f0_path(const float *cand_hz, const float *cand_d, const int64_t *n_frames, int64_t B, int64_t T, int w_unvoiced, int w_switch, int w_order, int w_jump,
               int jump_cap, int reserved, float *f0_hz, int32_t *state, int32_t *cost, void *stream) {
    VS_REQUIRE(cand_hz && cand_d && f0_hz, "vs_f0_path: cand_hz, cand_d and f0_hz must not be NULL");
    const void *bufs[6] = {cand_hz, cand_d, n_frames, f0_hz, state, cost};
    for (int x = 0; x < 6; ++x)
        for (int y = x + 1; y < 6; ++y) VS_REQUIRE(!bufs[x] || bufs[x] != bufs[y], "vs_f0_path: cand_hz, cand_d, n_frames, f0_hz, state and cost must be distinct buffers");
    VS_REQUIRE(B >= 1 && T >= 1 && T <= FP_MAX_FRAMES && B <= INT64_MAX / (T * 8), "vs_f0_path: B >= 1 and 1 <= T <= %d are required (got %lld, %lld)", FP_MAX_FRAMES,
               (long long)B, (long long)T);
    const int ws[5] = {w_unvoiced, w_switch, w_order, w_jump, jump_cap};
    for (int v : ws) VS_REQUIRE(v >= 0 && v <= FP_WEIGHT_MAX, "vs_f0_path: a weight of %d is not in [0, %d]", v, FP_WEIGHT_MAX);
    VS_REQUIRE(reserved == 0, "vs_f0_path: the reserved argument must be 0 (got %d)", reserved);
    static bool attr_set = false;
    if (!attr_set) {
        VS_CHECK_HIP(hipFuncSetAttribute((const void *)f0_path_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * FP_MAX_FRAMES));
        attr_set = true;
    }
    const FpWeights wt = {w_unvoiced, w_switch, w_order, w_jump, jump_cap};
    hipLaunchKernelGGL(f0_path_kernel, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(64), (size_t)4 * (size_t)T, as_stream(stream), cand_hz, cand_d,
                       (const long long *)n_frames, wt, f0_hz, (int *)state, (int *)cost, (long long)B, (int)T);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // extern "C"
