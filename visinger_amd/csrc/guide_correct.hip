// guide_correct.hip -- guide pitch correction: a tracked f0 curve pulled onto the score it was sung to (include/visinger_hip.h "f8").
// Not in the reference (its pitch tools are offline host programs).  Integer once the inputs are quantised to 1/16 cent: bit-reproducible, a row's result
// depends on that row only.  Two kernels, one launch each, no atomics, no host synchronisation:
//   guide_correct_kernel    grid (tiles of VS_GUIDE_CORRECT_TILE frames, B), 256 threads.
//     stage   the tile plus a halo of W frames on both sides (cut at the row's first frame and at its length n): d_u, the correctable flag and m_u of every
//             frame go to LDS -- coalesced, 16 bytes a lane where the rows are 16-byte aligned; note_midi is gathered through mel2ph.
//     scan    thread i takes K consecutive frames of the span (K odd: its stride-K LDS walk is conflict-free) and one workgroup scan carries four things
//             across the threads: the prefix sums of d and of the flags, the prefix max of the segment starts and the suffix min of the segment ends.  A
//             boundary farther than W from a frame never bounds its window, so the halo is enough; every sum is exact in int32.
//     write   lane l takes 4 consecutive frames of the tile: S_t and N_t are differences of the prefix sums at the clipped window's ends, then s, v, k, f0_out.
//   guide_deviation_kernel  one workgroup of 1024 threads per item: n_corr by one count, the lower median of d by bisection on the value over [-wild, wild]
//             (<= 20 steps, each one workgroup count).  d of the row's first GC_DEV_CACHE frames is kept in LDS, the rest is recomputed from the row each step.
#include "vs_internal.h"

#include <climits>
#include <cmath>

namespace vs {

constexpr int GC_TILE = VS_GUIDE_CORRECT_TILE;
constexpr int GC_THREADS = 256;
constexpr int GC_MAX_WINDOW = 1024;
constexpr int GC_MAX_FRAMES = 65536;
constexpr int GC_MAX_TOKENS = 1024;
constexpr int GC_MAX_WILD = 1 << 18;
constexpr int GC_SPAN = 13 * GC_THREADS;                // >= GC_TILE + 2 GC_MAX_WINDOW + 3 (the span starts on a multiple of 4 frames), K <= 13
constexpr int GC_NONE = INT_MIN;                        // no pitched token / not correctable
constexpr int GC_DEV_THREADS = 1024;
constexpr int GC_DEV_CACHE = 12288;                     // frames of d the deviation kernel keeps in LDS (48 KiB)
static_assert(GC_TILE == 4 * GC_THREADS, "the write pass: 4 frames a lane");
static_assert(GC_SPAN >= GC_TILE + 2 * GC_MAX_WINDOW + 3, "the staged span");

struct GcParams {
    int window, strength_q, b_q, wild, octave_fold;
};

struct GcShared {
    int pd[GC_SPAN + 1];                                // d of the correctable frames (0 elsewhere) at [i + 1], then their inclusive sums; [0] = 0
    int pc[GC_SPAN + 1];                                // the correctable flags likewise
    int m[GC_SPAN];                                     // m_u, GC_NONE without a pitched token
    int seg_lo[GC_TILE], seg_hi[GC_TILE];               // the tile's frames: first and last frame of the segment, as span indices
    int wave[4][4];
};
static_assert(sizeof(GcShared) <= 65536, "the workgroup's LDS");

// off = (int) rintf(clamp(16 offset_cents, -2^22, 2^22)), 0 for a non-finite offset
__device__ __forceinline__ int gc_offset(const float *offset_cents, long long row) {
    const float oc = offset_cents ? offset_cents[row] : 0.f;
    if (!(fabsf(oc) < INFINITY)) return 0;
    return (int)rintf(fminf(fmaxf(16.f * oc, -4194304.f), 4194304.f));
}

// m of the frame's token (GC_NONE: no token, or a rest) and d of the frame (GC_NONE: not correctable)
__device__ __forceinline__ void gc_frame(float f, long long tok, const float *__restrict__ note_row, int T_ph, int off, int fold, int wild, int &m, int &d) {
    m = GC_NONE;
    d = GC_NONE;
    if (tok < 1 || tok > T_ph) return;
    const float note = note_row[tok - 1];
    if (!(note > 0.f && note < INFINITY)) return;                             // (NaN fails the compare)
    m = (int)rintf(fminf(fmaxf(1600.f * (note - 69.f), -4194304.f), 4194304.f));
    if (!(f > 0.f && f < INFINITY)) return;
    const int q = (int)rintf(fminf(fmaxf(19200.f * log2f(f / 440.f), -4194304.f), 4194304.f));
    int dv = q - m - off;
    if (fold) {
        const int a = dv + 9600;
        dv -= 19200 * (a / 19200 - (a % 19200 < 0));                          // floor division
    }
    if (abs(dv) <= wild) d = dv;
}

template <bool VEC>
__global__ void __launch_bounds__(GC_THREADS) guide_correct_kernel(const float *__restrict__ f0_hz, const long long *__restrict__ lengths,
                                                                   const long long *__restrict__ mel2ph, const float *__restrict__ note_midi,
                                                                   const float *__restrict__ offset_cents, GcParams p, float *__restrict__ f0_out,
                                                                   int *__restrict__ k_out, long long B, int T, int T_ph) {
    __shared__ GcShared sh;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int t0 = blockIdx.x * GC_TILE, W = p.window;
    for (long long row = blockIdx.y; row < B; row += gridDim.y) {
        const float *f0 = f0_hz + row * T;
        const long long *m2p = mel2ph + row * T;
        const float *note_row = note_midi + row * T_ph;
        const long long len = lengths ? lengths[row] : (long long)T;
        const int n = (int)(len < 0 ? 0 : (len > T ? (long long)T : len));
        const int g0 = max(0, t0 - W) & ~3, g1 = min(n, t0 + GC_TILE + W);  // the span [g0, g1); empty when the tile lies beyond n
        const int span = max(0, g1 - g0);
        if (t0 < n) {
            // ---- stage: 4 frames a lane
            const int off = gc_offset(offset_cents, row);
            if (tid == 0) sh.pd[0] = sh.pc[0] = 0;
            for (int i = 4 * tid; i < span; i += 4 * GC_THREADS) {
                const int u = g0 + i;
                float f[4] = {0.f, 0.f, 0.f, 0.f};
                long long tok[4] = {0, 0, 0, 0};
                if (VEC) {                                                    // T % 4 == 0 and u % 4 == 0: u + 3 < T
                    const float4 fv = *reinterpret_cast<const float4 *>(f0 + u);
                    const longlong2 ta = *reinterpret_cast<const longlong2 *>(m2p + u), tb = *reinterpret_cast<const longlong2 *>(m2p + u + 2);
                    f[0] = fv.x, f[1] = fv.y, f[2] = fv.z, f[3] = fv.w;
                    tok[0] = ta.x, tok[1] = ta.y, tok[2] = tb.x, tok[3] = tb.y;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (u + j < g1) {
                            f[j] = f0[u + j];
                            tok[j] = m2p[u + j];
                        }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i + j < span) {
                        int m, d;
                        gc_frame(f[j], tok[j], note_row, T_ph, off, p.octave_fold, p.wild, m, d);
                        sh.m[i + j] = m;
                        sh.pd[i + j + 1] = d == GC_NONE ? 0 : d;
                        sh.pc[i + j + 1] = d != GC_NONE;
                    }
            }
            __syncthreads();

            // ---- scan: thread tid takes the frames [i0, i1) of the span
            const int K = ((span + GC_THREADS - 1) / GC_THREADS) | 1;
            const int i0 = min(span, tid * K), i1 = min(span, i0 + K);
            int sd = 0, sc = 0, lo = -1, hi = INT_MAX;                       // sums, the last segment start and the first segment end among the own frames
            for (int i = i0; i < i1; ++i) {
                const int m = sh.m[i];
                sd += sh.pd[i + 1];
                sc += sh.pc[i + 1];
                if (!(m != GC_NONE && i > 0 && sh.m[i - 1] == m)) lo = i;
                if (!(m != GC_NONE && i + 1 < span && sh.m[i + 1] == m)) hi = min(hi, i);
            }
            int xd = sd, xc = sc, xlo = lo, xhi = hi;                         // inclusive over the wave: sums and max upwards, min downwards
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const int od = __shfl_up(xd, s), oc = __shfl_up(xc, s), ol = __shfl_up(xlo, s), oh = __shfl_down(xhi, s);
                if (lane >= s) {
                    xd += od;
                    xc += oc;
                    xlo = max(xlo, ol);
                }
                if (lane + s < 64) xhi = min(xhi, oh);
            }
            if (lane == 63) {
                sh.wave[w][0] = xd;
                sh.wave[w][1] = xc;
                sh.wave[w][2] = xlo;
            }
            if (lane == 0) sh.wave[w][3] = xhi;
            __syncthreads();
            // exclusive: what the threads below (above, for the min) bring
            int ed = xd - sd, ec = xc - sc, elo = __shfl_up(xlo, 1), ehi = __shfl_down(xhi, 1);
            if (lane == 0) elo = -1;
            if (lane == 63) ehi = INT_MAX;
            for (int j = 0; j < 4; ++j) {
                if (j < w) {
                    ed += sh.wave[j][0];
                    ec += sh.wave[j][1];
                    elo = max(elo, sh.wave[j][2]);
                }
                if (j > w) ehi = min(ehi, sh.wave[j][3]);
            }
            const int tile_lo = t0 - g0;                                      // span index of the tile's first frame
            for (int i = i0; i < i1; ++i) {
                const int m = sh.m[i];
                if (!(m != GC_NONE && i > 0 && sh.m[i - 1] == m)) elo = i;
                ed += sh.pd[i + 1];
                ec += sh.pc[i + 1];
                sh.pd[i + 1] = ed;                                            // (own frames only: nobody else reads or writes them in this pass)
                sh.pc[i + 1] = ec;
                if (i >= tile_lo && i < tile_lo + GC_TILE) sh.seg_lo[i - tile_lo] = elo;
            }
            for (int i = i1 - 1; i >= i0; --i) {
                const int m = sh.m[i];
                if (!(m != GC_NONE && i + 1 < span && sh.m[i + 1] == m)) ehi = i;
                if (i >= tile_lo && i < tile_lo + GC_TILE) sh.seg_hi[i - tile_lo] = ehi;
            }
            __syncthreads();
        }

        // ---- write: 4 frames a lane
        const int t = t0 + 4 * tid;
        if (t < T) {
            float f[4] = {0.f, 0.f, 0.f, 0.f};
            if (VEC) {
                const float4 fv = *reinterpret_cast<const float4 *>(f0 + t);
                f[0] = fv.x, f[1] = fv.y, f[2] = fv.z, f[3] = fv.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (t + j < T) f[j] = f0[t + j];
            }
            float out[4];
            int k[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                out[j] = f[j];
                k[j] = 0;
                const int i = t + j - g0;                                     // span index
                if (t + j < n && sh.pc[i + 1] != sh.pc[i]) {
                    const int d = sh.pd[i + 1] - sh.pd[i];
                    const int a = max(i - W, sh.seg_lo[4 * tid + j]), e = min(i + W, sh.seg_hi[4 * tid + j]);
                    const int S = sh.pd[e + 1] - sh.pd[a], N = sh.pc[e + 1] - sh.pc[a];          // N >= 1: the frame itself
                    const int num = 2 * S + N, den = 2 * N;
                    const int s = num / den - (num % den < 0);                // floor division
                    const int v = d - s;
                    k[j] = (p.strength_q * s + p.b_q * v + 128) >> 8;         // floor division by 256
                    if (k[j] != 0) out[j] = f[j] * exp2f((float)(-k[j]) / 19200.0f);
                }
            }
            if (VEC) {
                *reinterpret_cast<float4 *>(f0_out + row * T + t) = make_float4(out[0], out[1], out[2], out[3]);
                if (k_out) *reinterpret_cast<int4 *>(k_out + row * T + t) = make_int4(k[0], k[1], k[2], k[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (t + j < T) {
                        f0_out[row * T + t + j] = out[j];
                        if (k_out) k_out[row * T + t + j] = k[j];
                    }
            }
        }
        __syncthreads();                                                      // the next row stages into the same LDS
    }
}

// the workgroup's sum of v; every thread gets it
__device__ __forceinline__ int gc_block_sum(int v, int *wave_tot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    if (lane == 0) wave_tot[w] = v;
    __syncthreads();
    int tot = 0;
    for (int j = 0; j < GC_DEV_THREADS / 64; ++j) tot += wave_tot[j];
    __syncthreads();
    return tot;
}

__global__ void __launch_bounds__(GC_DEV_THREADS) guide_deviation_kernel(const float *__restrict__ f0_hz, const long long *__restrict__ lengths,
                                                                         const long long *__restrict__ mel2ph, const float *__restrict__ note_midi,
                                                                         const float *__restrict__ offset_cents, int wild, int fold,
                                                                         int *__restrict__ dev_med, int *__restrict__ n_corr, long long B, int T, int T_ph) {
    __shared__ int cache[GC_DEV_CACHE];
    __shared__ int wave_tot[GC_DEV_THREADS / 64];
    const int tid = threadIdx.x;
    for (long long row = blockIdx.x; row < B; row += gridDim.x) {
        const float *f0 = f0_hz + row * T;
        const long long *m2p = mel2ph + row * T;
        const float *note_row = note_midi + row * T_ph;
        const long long len = lengths ? lengths[row] : (long long)T;
        const int n = (int)(len < 0 ? 0 : (len > T ? (long long)T : len));
        const int off = gc_offset(offset_cents, row);
        auto dev = [&](int t) {
            int m, d;
            gc_frame(f0[t], m2p[t], note_row, T_ph, off, fold, wild, m, d);
            return d;
        };
        int cnt = 0;
        for (int t = tid; t < n; t += GC_DEV_THREADS) {
            const int d = dev(t);
            if (t < GC_DEV_CACHE) cache[t] = d;                               // (thread tid reads back only what it wrote)
            cnt += d != GC_NONE;
        }
        const int total = gc_block_sum(cnt, wave_tot);
        int lo = -wild, hi = wild;                                            // the smallest x with #{d <= x} >= rank + 1
        const int rank = (total - 1) / 2;
        while (total > 0 && lo < hi) {                                        // uniform: every thread holds the same counts
            const int mid = lo + ((hi - lo) >> 1);
            cnt = 0;
            for (int t = tid; t < n; t += GC_DEV_THREADS) {
                const int d = t < GC_DEV_CACHE ? cache[t] : dev(t);
                cnt += d != GC_NONE && d <= mid;
            }
            if (gc_block_sum(cnt, wave_tot) >= rank + 1) hi = mid;
            else lo = mid + 1;
        }
        if (tid == 0) {
            n_corr[row] = total;
            dev_med[row] = total > 0 ? lo : 0;
        }
    }
}

static bool gc_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_guide_correct(const float *f0_hz, const int64_t *lengths, const int64_t *mel2ph, const float *note_midi, const float *offset_cents, int window,
                     int strength_q, int vibrato_q, int wild, int octave_fold, int reserved, float *f0_out, int32_t *k_out, int64_t B, int64_t T,
                     int64_t T_ph, void *stream) {
    VS_REQUIRE(f0_hz && mel2ph && note_midi && f0_out, "vs_guide_correct: f0_hz, mel2ph, note_midi and f0_out must not be NULL");
    VS_REQUIRE(B >= 1 && B <= INT64_MAX / (8 * GC_MAX_FRAMES) && T_ph >= 1 && T_ph <= GC_MAX_TOKENS && T >= 1 && T <= GC_MAX_FRAMES,
               "vs_guide_correct: B >= 1, 1 <= T_ph <= %d and 1 <= T <= %d are required (got %lld, %lld, %lld)", GC_MAX_TOKENS, GC_MAX_FRAMES, (long long)B,
               (long long)T_ph, (long long)T);
    VS_REQUIRE(window >= 0 && window <= GC_MAX_WINDOW, "vs_guide_correct: window = %d is not in [0, %d]", window, GC_MAX_WINDOW);
    VS_REQUIRE(strength_q >= 0 && strength_q <= 256, "vs_guide_correct: strength_q = %d is not in [0, 256]", strength_q);
    VS_REQUIRE(vibrato_q >= 0 && vibrato_q <= 512, "vs_guide_correct: vibrato_q = %d is not in [0, 512]", vibrato_q);
    VS_REQUIRE(wild >= 0 && wild <= GC_MAX_WILD, "vs_guide_correct: wild = %d is not in [0, %d]", wild, GC_MAX_WILD);
    VS_REQUIRE(octave_fold == 0 || octave_fold == 1, "vs_guide_correct: octave_fold = %d is not 0 or 1", octave_fold);
    VS_REQUIRE(reserved == 0, "vs_guide_correct: the reserved argument must be 0 (got %d)", reserved);
    const size_t frames = (size_t)(B * T);
    const struct {
        const void *p;
        size_t n;
    } ins[5] = {{f0_hz, frames * 4}, {lengths, (size_t)B * 8}, {mel2ph, frames * 8}, {note_midi, (size_t)(B * T_ph) * 4}, {offset_cents, (size_t)B * 4}};
    for (const auto &in : ins)
        VS_REQUIRE(!gc_overlap(in.p, in.n, f0_out, frames * 4) && !gc_overlap(in.p, in.n, k_out, frames * 4),
                   "vs_guide_correct: an output overlaps an input (the buffers must be distinct)");
    VS_REQUIRE(!gc_overlap(f0_out, frames * 4, k_out, frames * 4), "vs_guide_correct: f0_out and k_out overlap");
    const GcParams p = {window, strength_q, 256 - vibrato_q, wild, octave_fold};
    const dim3 grid((unsigned)ceil_div(T, GC_TILE), (unsigned)(B < 65535 ? B : 65535));
    const bool vec = T % 4 == 0 && (((uintptr_t)f0_hz | (uintptr_t)mel2ph | (uintptr_t)f0_out | (uintptr_t)k_out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(guide_correct_kernel<true>, grid, dim3(GC_THREADS), 0, as_stream(stream), f0_hz, (const long long *)lengths,
                           (const long long *)mel2ph, note_midi, offset_cents, p, f0_out, (int *)k_out, (long long)B, (int)T, (int)T_ph);
    else
        hipLaunchKernelGGL(guide_correct_kernel<false>, grid, dim3(GC_THREADS), 0, as_stream(stream), f0_hz, (const long long *)lengths,
                           (const long long *)mel2ph, note_midi, offset_cents, p, f0_out, (int *)k_out, (long long)B, (int)T, (int)T_ph);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

int vs_guide_deviation(const float *f0_hz, const int64_t *lengths, const int64_t *mel2ph, const float *note_midi, const float *offset_cents, int wild,
                       int octave_fold, int32_t *dev_med, int32_t *n_corr, int64_t B, int64_t T, int64_t T_ph, void *stream) {
    VS_REQUIRE(f0_hz && mel2ph && note_midi && dev_med && n_corr, "vs_guide_deviation: f0_hz, mel2ph, note_midi, dev_med and n_corr must not be NULL");
    VS_REQUIRE(B >= 1 && B <= INT64_MAX / (8 * GC_MAX_FRAMES) && T_ph >= 1 && T_ph <= GC_MAX_TOKENS && T >= 1 && T <= GC_MAX_FRAMES,
               "vs_guide_deviation: B >= 1, 1 <= T_ph <= %d and 1 <= T <= %d are required (got %lld, %lld, %lld)", GC_MAX_TOKENS, GC_MAX_FRAMES, (long long)B,
               (long long)T_ph, (long long)T);
    VS_REQUIRE(wild >= 0 && wild <= GC_MAX_WILD, "vs_guide_deviation: wild = %d is not in [0, %d]", wild, GC_MAX_WILD);
    VS_REQUIRE(octave_fold == 0 || octave_fold == 1, "vs_guide_deviation: octave_fold = %d is not 0 or 1", octave_fold);
    const size_t frames = (size_t)(B * T);
    const struct {
        const void *p;
        size_t n;
    } ins[5] = {{f0_hz, frames * 4}, {lengths, (size_t)B * 8}, {mel2ph, frames * 8}, {note_midi, (size_t)(B * T_ph) * 4}, {offset_cents, (size_t)B * 4}};
    for (const auto &in : ins)
        VS_REQUIRE(!gc_overlap(in.p, in.n, dev_med, (size_t)B * 4) && !gc_overlap(in.p, in.n, n_corr, (size_t)B * 4),
                   "vs_guide_deviation: an output overlaps an input (the buffers must be distinct)");
    VS_REQUIRE(!gc_overlap(dev_med, (size_t)B * 4, n_corr, (size_t)B * 4), "vs_guide_deviation: dev_med and n_corr overlap");
    hipLaunchKernelGGL(guide_deviation_kernel, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(GC_DEV_THREADS), 0, as_stream(stream), f0_hz,
                       (const long long *)lengths, (const long long *)mel2ph, note_midi, offset_cents, wild, octave_fold, (int *)dev_med, (int *)n_corr,
                       (long long)B, (int)T, (int)T_ph);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // extern "C"
