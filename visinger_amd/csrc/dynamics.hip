// dynamics.hip -- guide dynamics: the loudness contour of a recording carried onto the synthesised waveform (include/visinger_hip.h "f10").
// Not in the reference (the model has no energy condition).  Levels are fp32 mean-square power per frame; once quantised to 1/256 of a doubling of power the
// gain rule is integer: bit-reproducible, a row's result depends on that row only.  Four kernels, one launch each, no atomics, no host synchronisation:
//   level_track_kernel   grid (tiles of LT_TILE frames, B), 256 threads.  A wave takes one block of `hop` samples at a time: lane l loads samples 4 l .. 4 l + 3
//             of every 256 (one 16-byte load where the row is 16-byte aligned and hop % 4 == 0, four 4-byte loads otherwise: the same chain), squares them into
//             ONE fma chain, and the 64 chains meet in an xor butterfly.  The block energies of the tile plus `half` blocks on both sides go to LDS (one
//             word per block, written by lane 0: no banking question), then thread t sums its frame's window, ascending.
//   level_offset_kernel  one workgroup of 1024 threads per item: the int64 sum of d over the active frames and their count, one workgroup reduction.
//   level_gain_kernel    grid (tiles of VS_LEVEL_GAIN_TILE frames, B), 256 threads, the layout of guide_correct_kernel without its segments:
//     stage   the tile plus a halo of W frames on both sides (cut at the row's first frame and at n): e_u and the active flag of every frame go to LDS.
//     scan    thread i takes K consecutive frames of the span (K odd: its stride-K LDS walk falls on 32 different banks per 32 lanes) and one workgroup scan
//             carries the prefix sums of e and of the flags across the threads.  Every sum is exact in int32.
//     write   lane l takes 4 consecutive frames of the tile: S_t and N_t are differences of the prefix sums at the clipped window's ends.
//   level_apply_kernel   grid (chunks of 1024 samples, B), 256 threads, 4 consecutive samples a lane (16-byte loads and stores where L % 4 == 0 and x, y
//             are 16-byte aligned); k of the two frame centres around a sample is gathered from global memory (consecutive lanes: the same words).
#include "vs_internal.h"

#include <climits>
#include <cmath>

namespace vs {

constexpr int LT_TILE = 64;                              // frames a workgroup of level_track_kernel writes
constexpr int LT_THREADS = 256;
constexpr int LT_MAX_HALF = 8;
constexpr int LT_MAX_HOP = 4096;
constexpr int LG_TILE = VS_LEVEL_GAIN_TILE;
constexpr int LG_THREADS = 256;
constexpr int LG_MAX_WINDOW = 1024;
constexpr int LG_MAX_FRAMES = 65536;
constexpr int LG_MAX_LIMIT = 4096;                       // up, down and |k| as vs_level_apply reads it
constexpr int LG_Q_MAX = 1 << 16;                        // |q|, |gate|
constexpr int LG_OFF_MAX = 1 << 17;                      // |offset| as vs_level_gain reads it
constexpr int LG_SPAN = 13 * LG_THREADS;                 // >= LG_TILE + 2 LG_MAX_WINDOW + 3 (the span starts on a multiple of 4 frames), K <= 13
constexpr int LO_THREADS = 1024;
constexpr int LA_THREADS = 256;
constexpr int LA_MAX_HOP = 2048;
constexpr int LG_NONE = INT_MIN;                         // a frame without a level
static_assert(LG_TILE == 4 * LG_THREADS, "the write pass: 4 frames a lane");
static_assert(LG_SPAN >= LG_TILE + 2 * LG_MAX_WINDOW + 3, "the staged span");
static_assert(LT_TILE <= LT_THREADS, "the frame pass: one frame a thread");

// One multiply as an opaque scalar instruction (conv_common.h: mul_f32_scalar): the four products of a lane's 16 bytes would otherwise be paired by hipcc's SLP
// vectoriser into v_pk_mul_f32, with op_sel:[_,1] where the gains sit in odd registers -- the form that returns wrong low results in lanes 48-63 beside another
// wave's MFMAs on gfx950, which is where level_apply_kernel runs under synthesize(streams=2).  build.py refuses an object that holds one.
__device__ __forceinline__ float mul_f32_scalar(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the row's length, clamped to [0, top]
__device__ __forceinline__ long long row_len(const long long *lengths, long long row, long long top) {
    const long long len = lengths ? lengths[row] : top;
    return len < 0 ? 0 : (len > top ? top : len);
}

// ---- vs_level_track -------------------------------------------------------------------------------------------------------------------------------------

// E_u of the block that starts at `src`, on every lane of the wave
template <bool VEC>
__device__ __forceinline__ float block_energy(const float *__restrict__ src, int hop, int lane) {
    float acc = 0.f;
    for (int j = 4 * lane; j < hop; j += 256) {
        if (VEC) {                                                            // hop % 4 == 0: j + 3 < hop
            const float4 v = *reinterpret_cast<const float4 *>(src + j);
            acc = fmaf(v.x, v.x, acc);
            acc = fmaf(v.y, v.y, acc);
            acc = fmaf(v.z, v.z, acc);
            acc = fmaf(v.w, v.w, acc);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (j + q < hop) {
                    const float v = src[j + q];
                    acc = fmaf(v, v, acc);
                }
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
    return acc;
}

__global__ void __launch_bounds__(LT_THREADS) level_track_kernel(const float *__restrict__ wav, const long long *__restrict__ lengths, long long B, long long L,
                                                                 int hop, int half, float *__restrict__ level, long long T) {
    __shared__ float E[LT_TILE + 2 * LT_MAX_HALF];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long t0 = (long long)blockIdx.x * LT_TILE;
    for (long long row = blockIdx.y; row < B; row += gridDim.y) {
        const float *src = wav + row * L;
        float *dst = level + row * T;
        const long long nb = row_len(lengths, row, L) / hop, n = nb < T ? nb : T;
        if (t0 >= n) {                                                        // (uniform over the workgroup)
            if (tid < LT_TILE && t0 + tid < T) dst[t0 + tid] = 0.f;
            continue;
        }
        const long long u0 = t0 - half > 0 ? t0 - half : 0;                   // the blocks [u0, u1) enter the tile's frames
        const long long u1 = t0 + LT_TILE + half < n ? t0 + LT_TILE + half : n;
        const int blocks = (int)(u1 - u0);
        const bool vec = hop % 4 == 0 && ((uintptr_t)src & 15) == 0;
        if (vec) {
#pragma unroll 2
            for (int i = w; i < blocks; i += LT_THREADS / 64) {
                const float e = block_energy<true>(src + (u0 + i) * hop, hop, lane);
                if (lane == 0) E[i] = e;
            }
        } else {
            for (int i = w; i < blocks; i += LT_THREADS / 64) {
                const float e = block_energy<false>(src + (u0 + i) * hop, hop, lane);
                if (lane == 0) E[i] = e;
            }
        }
        __syncthreads();
        if (tid < LT_TILE && t0 + tid < T) {
            const long long t = t0 + tid;
            float p = 0.f;
            if (t < n) {
                const long long a = t - half > 0 ? t - half : 0, e = t + half < n - 1 ? t + half : n - 1;
                float s = 0.f;
                for (long long u = a; u <= e; ++u) s += E[u - u0];
                p = s / (float)((int)(e - a + 1) * hop);
                if (!(fabsf(s) < INFINITY)) p = 0.f;
            }
            dst[t] = p;
        }
        __syncthreads();                                                      // the next row's energies go to the same LDS
    }
}

// ---- the quantised level of a frame ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int level_q(float p) {
    if (!(p > 0.f && p < INFINITY)) return LG_NONE;                           // (NaN fails the compare)
    return (int)rintf(fminf(fmaxf(256.f * log2f(p), -65536.f), 65536.f));
}

// d of the frame where it is active, LG_NONE elsewhere
__device__ __forceinline__ int level_d(float g, float o, int gate) {
    const int qg = level_q(g), qo = level_q(o);
    if (qg == LG_NONE || qo == LG_NONE || qg < gate || qo < gate) return LG_NONE;
    return qg - qo;
}

// ---- vs_level_offset ------------------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(LO_THREADS) level_offset_kernel(const float *__restrict__ guide, const float *__restrict__ own,
                                                                  const long long *__restrict__ lengths, int gate, int *__restrict__ off,
                                                                  int *__restrict__ n_act, long long B, int T) {
    __shared__ long long wave_sum[LO_THREADS / 64];
    __shared__ int wave_cnt[LO_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (long long row = blockIdx.x; row < B; row += gridDim.x) {
        const float *g = guide + row * T, *o = own + row * T;
        const int n = (int)row_len(lengths, row, T);
        long long sum = 0;
        int cnt = 0;
        for (int t = tid; t < n; t += LO_THREADS) {
            const int d = level_d(g[t], o[t], gate);
            if (d != LG_NONE) {
                sum += d;
                ++cnt;
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            sum += __shfl_xor(sum, s);
            cnt += __shfl_xor(cnt, s);
        }
        if (lane == 0) {
            wave_sum[w] = sum;
            wave_cnt[w] = cnt;
        }
        __syncthreads();
        if (tid == 0) {
            long long S = 0, N = 0;
            for (int j = 0; j < LO_THREADS / 64; ++j) {
                S += wave_sum[j];
                N += wave_cnt[j];
            }
            int res = 0;
            if (N > 0) {
                const long long num = 2 * S + N, den = 2 * N;
                res = (int)(num / den - (num % den < 0));                     // floor division
            }
            off[row] = res;
            n_act[row] = (int)N;
        }
        __syncthreads();
    }
}

// ---- vs_level_gain --------------------------------------------------------------------------------------------------------------------------------------

struct LgParams {
    int gate, window, depth_q, up, down;
};

struct LgShared {
    int pe[LG_SPAN + 1];                                // e of the active frames (0 elsewhere) at [i + 1], then their inclusive sums; [0] = 0
    int pc[LG_SPAN + 1];                                // the active flags likewise
    int wave[LG_THREADS / 64][2];
};

template <bool VEC>
__global__ void __launch_bounds__(LG_THREADS) level_gain_kernel(const float *__restrict__ guide, const float *__restrict__ own,
                                                                const long long *__restrict__ lengths, const int *__restrict__ offset, LgParams p,
                                                                int *__restrict__ k_out, long long B, int T) {
    __shared__ LgShared sh;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int t0 = blockIdx.x * LG_TILE, W = p.window;
    for (long long row = blockIdx.y; row < B; row += gridDim.y) {
        const float *g = guide + row * T, *o = own + row * T;
        const int n = (int)row_len(lengths, row, T);
        const int g0 = max(0, t0 - W) & ~3, g1 = min(n, t0 + LG_TILE + W);    // the span [g0, g1); empty when the tile lies beyond n
        const int span = max(0, g1 - g0);
        if (t0 < n) {
            // ---- stage: 4 frames a lane
            const int off = offset ? clampi(offset[row], -LG_OFF_MAX, LG_OFF_MAX) : 0;
            if (tid == 0) sh.pe[0] = sh.pc[0] = 0;
            for (int i = 4 * tid; i < span; i += 4 * LG_THREADS) {
                const int u = g0 + i;
                float gv[4] = {0.f, 0.f, 0.f, 0.f}, ov[4] = {0.f, 0.f, 0.f, 0.f};
                if (VEC) {                                                    // T % 4 == 0 and u % 4 == 0: u + 3 < T
                    const float4 a = *reinterpret_cast<const float4 *>(g + u), b = *reinterpret_cast<const float4 *>(o + u);
                    gv[0] = a.x, gv[1] = a.y, gv[2] = a.z, gv[3] = a.w;
                    ov[0] = b.x, ov[1] = b.y, ov[2] = b.z, ov[3] = b.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (u + j < g1) {
                            gv[j] = g[u + j];
                            ov[j] = o[u + j];
                        }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i + j < span) {
                        const int d = level_d(gv[j], ov[j], p.gate);
                        sh.pe[i + j + 1] = d == LG_NONE ? 0 : d - off;
                        sh.pc[i + j + 1] = d != LG_NONE;
                    }
            }
            __syncthreads();

            // ---- scan: thread tid takes the frames [i0, i1) of the span
            const int K = ((span + LG_THREADS - 1) / LG_THREADS) | 1;
            const int i0 = min(span, tid * K), i1 = min(span, i0 + K);
            int se = 0, sc = 0;
            for (int i = i0; i < i1; ++i) {
                se += sh.pe[i + 1];
                sc += sh.pc[i + 1];
            }
            int xe = se, xc = sc;                                             // inclusive over the wave
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const int oe = __shfl_up(xe, s), oc = __shfl_up(xc, s);
                if (lane >= s) {
                    xe += oe;
                    xc += oc;
                }
            }
            if (lane == 63) {
                sh.wave[w][0] = xe;
                sh.wave[w][1] = xc;
            }
            __syncthreads();
            int ee = xe - se, ec = xc - sc;                                   // exclusive: what the threads below bring
            for (int j = 0; j < LG_THREADS / 64; ++j)
                if (j < w) {
                    ee += sh.wave[j][0];
                    ec += sh.wave[j][1];
                }
            for (int i = i0; i < i1; ++i) {
                ee += sh.pe[i + 1];
                ec += sh.pc[i + 1];
                sh.pe[i + 1] = ee;                                            // (own frames only: nobody else reads or writes them in this pass)
                sh.pc[i + 1] = ec;
            }
            __syncthreads();
        }

        // ---- write: 4 frames a lane
        const int t = t0 + 4 * tid;
        if (t < T) {
            int k[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = t + j - g0;                                     // span index
                if (t + j < n) {
                    const int a = max(i - W, 0), e = min(i + W, span - 1);
                    const int S = sh.pe[e + 1] - sh.pe[a], N = sh.pc[e + 1] - sh.pc[a];
                    if (N >= 1) {
                        const int num = 2 * S + N, den = 2 * N;
                        const int m = num / den - (num % den < 0);            // floor division
                        k[j] = clampi((p.depth_q * m + 128) >> 8, -p.down, p.up);      // floor division by 256
                    }
                }
            }
            if (VEC) {
                *reinterpret_cast<int4 *>(k_out + row * T + t) = make_int4(k[0], k[1], k[2], k[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (t + j < T) k_out[row * T + t + j] = k[j];
            }
        }
        __syncthreads();                                                      // the next row stages into the same LDS
    }
}

// ---- vs_level_apply -------------------------------------------------------------------------------------------------------------------------------------

template <bool VEC>
__global__ void __launch_bounds__(LA_THREADS) level_apply_kernel(const float *x, const int *__restrict__ k, const long long *__restrict__ lengths, int hop,
                                                                 float *y, long long B, long long L, long long T) {
    const long long i0 = ((long long)blockIdx.x * LA_THREADS + threadIdx.x) * 4;
    if (i0 >= L) return;
    const float den = (float)(1024 * hop);
    for (long long row = blockIdx.y; row < B; row += gridDim.y) {
        const float *src = x + row * L;
        float *dst = y + row * L;
        const int *kr = k + row * T;
        const long long nb = row_len(lengths, row, L) / hop, n = nb < T ? nb : T, end = n * hop;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {                                                            // L % 4 == 0: i0 + 3 < L
            const float4 a = *reinterpret_cast<const float4 *>(src + i0);
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < L) v[j] = src[i0 + j];
        }
        if (i0 < end) {
            // i = f hop + r: a = 2 hop f + (2 r + 1 - hop), so t0 = f or f - 1 and w follows without a 64-bit division
            long long f = (unsigned)i0 / (unsigned)hop;                       // (i0 < L < 2^31)
            int r = (int)(i0 - f * hop);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i0 + j < end) {
                    const int c = 2 * r + 1 - hop;
                    const long long ta = c >= 0 ? f : f - 1;
                    const int wgt = c >= 0 ? c : c + 2 * hop;
                    const long long ia = ta < 0 ? 0 : (ta > n - 1 ? n - 1 : ta), ib = ta + 1 > n - 1 ? n - 1 : ta + 1;
                    const int ka = clampi(kr[ia], -LG_MAX_LIMIT, LG_MAX_LIMIT), kb = clampi(kr[ib], -LG_MAX_LIMIT, LG_MAX_LIMIT);
                    const int kappa = ka * (2 * hop - wgt) + kb * wgt;
                    if (kappa != 0) v[j] = mul_f32_scalar(v[j], exp2f((float)kappa / den));
                }
                if (++r == hop) {
                    r = 0;
                    ++f;
                }
            }
        }
        if (VEC) {
            *reinterpret_cast<float4 *>(dst + i0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < L) dst[i0 + j] = v[j];
        }
    }
}

static bool dyn_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_level_track(const float *wav, const int64_t *lengths, int64_t B, int64_t L, int hop, int half, float *level, int64_t T, void *stream) {
    VS_REQUIRE(wav && level, "vs_level_track: wav and level must not be NULL");
    VS_REQUIRE(B > 0 && L > 0 && T > 0, "vs_level_track: B, L, T must be positive (got %lld, %lld, %lld)", (long long)B, (long long)L, (long long)T);
    VS_REQUIRE(L < (1ll << 31) && T < (1ll << 31) && B <= INT64_MAX / 8 / L && B <= INT64_MAX / 8 / T,
               "vs_level_track: L = %lld or T = %lld is not below 2^31, or B * L / B * T is out of range", (long long)L, (long long)T);
    VS_REQUIRE(hop >= 1 && hop <= LT_MAX_HOP, "vs_level_track: hop = %d is not in [1, %d]", hop, LT_MAX_HOP);
    VS_REQUIRE(half >= 0 && half <= LT_MAX_HALF, "vs_level_track: half = %d is not in [0, %d]", half, LT_MAX_HALF);
    const size_t in = (size_t)(B * L) * 4, out = (size_t)(B * T) * 4;
    VS_REQUIRE(!dyn_overlap(wav, in, level, out) && !dyn_overlap(lengths, (size_t)B * 8, level, out),
               "vs_level_track: level overlaps an input (the buffers must be distinct)");
    const dim3 grid((unsigned)ceil_div(T, LT_TILE), (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL(level_track_kernel, grid, dim3(LT_THREADS), 0, as_stream(stream), wav, (const long long *)lengths, (long long)B, (long long)L, hop, half,
                       level, (long long)T);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

int vs_level_offset(const float *guide, const float *own, const int64_t *lengths, int gate, int32_t *off, int32_t *n_act, int64_t B, int64_t T, void *stream) {
    VS_REQUIRE(guide && own && off && n_act, "vs_level_offset: guide, own, off and n_act must not be NULL");
    VS_REQUIRE(B >= 1 && B <= INT64_MAX / (8 * LG_MAX_FRAMES) && T >= 1 && T <= LG_MAX_FRAMES, "vs_level_offset: B >= 1 and 1 <= T <= %d are required (got %lld, %lld)",
               LG_MAX_FRAMES, (long long)B, (long long)T);
    VS_REQUIRE(gate >= -LG_Q_MAX && gate <= LG_Q_MAX, "vs_level_offset: gate = %d is not in [%d, %d]", gate, -LG_Q_MAX, LG_Q_MAX);
    const size_t frames = (size_t)(B * T) * 4, items = (size_t)B * 4;
    const struct {
        const void *p;
        size_t n;
    } ins[3] = {{guide, frames}, {own, frames}, {lengths, (size_t)B * 8}};
    for (const auto &in : ins)
        VS_REQUIRE(!dyn_overlap(in.p, in.n, off, items) && !dyn_overlap(in.p, in.n, n_act, items),
                   "vs_level_offset: an output overlaps an input (the buffers must be distinct)");
    VS_REQUIRE(!dyn_overlap(off, items, n_act, items), "vs_level_offset: off and n_act overlap");
    hipLaunchKernelGGL(level_offset_kernel, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(LO_THREADS), 0, as_stream(stream), guide, own,
                       (const long long *)lengths, gate, (int *)off, (int *)n_act, (long long)B, (int)T);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

int vs_level_gain(const float *guide, const float *own, const int64_t *lengths, const int32_t *offset, int gate, int window, int depth_q, int up, int down,
                  int reserved, int32_t *k_out, int64_t B, int64_t T, void *stream) {
    VS_REQUIRE(guide && own && k_out, "vs_level_gain: guide, own and k_out must not be NULL");
    VS_REQUIRE(B >= 1 && B <= INT64_MAX / (8 * LG_MAX_FRAMES) && T >= 1 && T <= LG_MAX_FRAMES, "vs_level_gain: B >= 1 and 1 <= T <= %d are required (got %lld, %lld)",
               LG_MAX_FRAMES, (long long)B, (long long)T);
    VS_REQUIRE(gate >= -LG_Q_MAX && gate <= LG_Q_MAX, "vs_level_gain: gate = %d is not in [%d, %d]", gate, -LG_Q_MAX, LG_Q_MAX);
    VS_REQUIRE(window >= 0 && window <= LG_MAX_WINDOW, "vs_level_gain: window = %d is not in [0, %d]", window, LG_MAX_WINDOW);
    VS_REQUIRE(depth_q >= 0 && depth_q <= 256, "vs_level_gain: depth_q = %d is not in [0, 256]", depth_q);
    VS_REQUIRE(up >= 0 && up <= LG_MAX_LIMIT && down >= 0 && down <= LG_MAX_LIMIT, "vs_level_gain: up = %d or down = %d is not in [0, %d]", up, down, LG_MAX_LIMIT);
    VS_REQUIRE(reserved == 0, "vs_level_gain: the reserved argument must be 0 (got %d)", reserved);
    const size_t frames = (size_t)(B * T) * 4;
    const struct {
        const void *p;
        size_t n;
    } ins[4] = {{guide, frames}, {own, frames}, {lengths, (size_t)B * 8}, {offset, (size_t)B * 4}};
    for (const auto &in : ins)
        VS_REQUIRE(!dyn_overlap(in.p, in.n, k_out, frames), "vs_level_gain: k_out overlaps an input (the buffers must be distinct)");
    const LgParams p = {gate, window, depth_q, up, down};
    const dim3 grid((unsigned)ceil_div(T, LG_TILE), (unsigned)(B < 65535 ? B : 65535));
    const bool vec = T % 4 == 0 && (((uintptr_t)guide | (uintptr_t)own | (uintptr_t)k_out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(level_gain_kernel<true>, grid, dim3(LG_THREADS), 0, as_stream(stream), guide, own, (const long long *)lengths, (const int *)offset, p,
                           (int *)k_out, (long long)B, (int)T);
    else
        hipLaunchKernelGGL(level_gain_kernel<false>, grid, dim3(LG_THREADS), 0, as_stream(stream), guide, own, (const long long *)lengths, (const int *)offset, p,
                           (int *)k_out, (long long)B, (int)T);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

int vs_level_apply(const float *x, const int32_t *k, const int64_t *lengths, int hop, float *y, int64_t B, int64_t L, int64_t T, void *stream) {
    VS_REQUIRE(x && k && y, "vs_level_apply: x, k and y must not be NULL");
    VS_REQUIRE(B > 0 && L > 0 && T > 0, "vs_level_apply: B, L, T must be positive (got %lld, %lld, %lld)", (long long)B, (long long)L, (long long)T);
    VS_REQUIRE(L < (1ll << 31) && T < (1ll << 31) && B <= INT64_MAX / 8 / L && B <= INT64_MAX / 8 / T,
               "vs_level_apply: L = %lld or T = %lld is not below 2^31, or B * L / B * T is out of range", (long long)L, (long long)T);
    VS_REQUIRE(hop >= 1 && hop <= LA_MAX_HOP, "vs_level_apply: hop = %d is not in [1, %d]", hop, LA_MAX_HOP);
    const size_t samples = (size_t)(B * L) * 4, frames = (size_t)(B * T) * 4;
    VS_REQUIRE(x == y || !dyn_overlap(x, samples, y, samples), "vs_level_apply: y must be x itself (in place) or must not overlap it");
    VS_REQUIRE(!dyn_overlap(k, frames, y, samples) && !dyn_overlap(lengths, (size_t)B * 8, y, samples),
               "vs_level_apply: y overlaps k or lengths (the buffers must be distinct)");
    const dim3 grid((unsigned)ceil_div(L, 4 * LA_THREADS), (unsigned)(B < 65535 ? B : 65535));
    const bool vec = L % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(level_apply_kernel<true>, grid, dim3(LA_THREADS), 0, as_stream(stream), x, (const int *)k, (const long long *)lengths, hop, y,
                           (long long)B, (long long)L, (long long)T);
    else
        hipLaunchKernelGGL(level_apply_kernel<false>, grid, dim3(LA_THREADS), 0, as_stream(stream), x, (const int *)k, (const long long *)lengths, hop, y,
                           (long long)B, (long long)L, (long long)T);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // extern "C"
