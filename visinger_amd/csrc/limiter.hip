// limiter.hip -- a look-ahead sample-peak limiter behind guide dynamics and sample-rate conversion (include/visinger_hip.h "f11").
// Not in the reference (it peak-normalises on the host).  The reduction is integer, in f10's unit seen from the amplitude (1/512 of a doubling): the kernel is
// held bit for bit, and a row's result depends on that row only.  One kernel, one launch:
//   peak_limit_kernel   grid (tiles of PL_TILE samples, B), 1024 threads, one workgroup per tile (WALK: grid (1, B), see below).
//     stage   lane l takes the 4 samples t0 + 4 l .. + 3 of the tile -- kept in registers for the apply pass -- and one 4-sample vector of the two halos of
//             H2 = 2 W rounded up to 4 samples (16-byte loads where VEC); the need u of each goes to LDS, 16 bytes a lane.  One __syncthreads_or tells whether
//             any staged u is > 0: if not, the tile is a copy of x's bits (nothing at all in place).
//     hold    the running maximum over 2 W + 1 samples by log-step doubling between two LDS arrays: A_2s[k] = max(A_s[k], A_s[k + s]), then
//             M_j = max(A_s[j - W], A_s[j + W + 1 - s]) with s the largest power of two <= 2 W + 1.  (van Herk / Gil-Werman runs one serial chain per block of
//             2 W + 1 samples: 18 chains of 257 steps at the default W = 128, 4 of 2049 at W = 1024, in a workgroup of 1024 threads; doubling keeps every lane
//             busy for floor(log2(2 W + 1)) <= 11 short steps.)  M = 0 outside [0, n).
//     scan    thread i takes K consecutive M of the tile plus W on both sides (K odd) and one workgroup scan carries the prefix sums, as level_gain_kernel.
//     smooth  thread i takes the outputs i + 1024 j: S from the prefix sums at the clipped window's ends, N from the indices, g = ceil(S / N) to LDS.
//     apply   lane l reads its 4 g as 16 bytes, scales its 4 samples, guards them, writes y, gain and its share of stats.
//   WALK (y == x): a neighbour's output would be this tile's halo, so one workgroup walks its row's tiles in ascending order: the right halo and the tile are
//   still x when they are read, the left halo's u is carried over in LDS from the tile before.
#include "vs_internal.h"

#include <cmath>

namespace vs {

constexpr int PL_TILE = VS_PEAK_LIMIT_TILE;
constexpr int PL_THREADS = 1024;
constexpr int PL_WAVES = PL_THREADS / 64;
constexpr int PL_MAX_WINDOW = VS_PEAK_LIMIT_MAX_WINDOW;
constexpr int PL_HALO = 2 * PL_MAX_WINDOW;               // the u a tile's outputs depend on reach 2 W beyond it
constexpr int PL_SPAN = PL_TILE + 2 * PL_HALO;           // words of a staged span at most
constexpr int PL_U_MAX = VS_PEAK_LIMIT_U_MAX;
static_assert(PL_TILE == 4 * PL_THREADS, "the stage and apply passes: 4 samples a lane");
static_assert(2 * (PL_HALO / 4) <= PL_THREADS, "the halos: one vector a lane");
static_assert(7 * PL_THREADS >= PL_TILE + 2 * PL_MAX_WINDOW, "the scan: K <= 7");
static_assert((long long)(PL_TILE + 2 * PL_MAX_WINDOW) * PL_U_MAX < (1ll << 31), "the prefix sums fit int32");

// One multiply as an opaque scalar instruction (conv_common.h: mul_f32_scalar; dynamics.hip): the four products of a lane's 16 bytes would otherwise be paired
// by hipcc's SLP vectoriser into v_pk_mul_f32, the form that returns wrong low results in lanes 48-63 beside another wave's MFMAs on gfx950,
// which is where peak_limit_kernel runs under synthesize(streams=2).  build.py refuses an object that holds one.
__device__ __forceinline__ float pl_mul_f32_scalar(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// the row's length, clamped to [0, top]
__device__ __forceinline__ long long pl_row_len(const long long *lengths, long long row, long long top) {
    const long long len = lengths ? lengths[row] : top;
    return len < 0 ? 0 : (len > top ? top : len);
}

// u of one sample (rule step 1); an infinite quotient has e = 128 and takes U_MAX through the min
__device__ __forceinline__ int peak_need(float x, float c, const int *__restrict__ tab) {
    const float a = fabsf(x);
    if (!(a > c)) return 0;                                                   // (NaN fails the compare)
    const unsigned bits = __float_as_uint(__fdiv_rn(a, c));
    const int e = (int)(bits >> 23) - 127, m = (int)(bits & 0x7fffffu);
    const int u = 512 * e + tab[m >> 14];
    return u < PL_U_MAX ? u : PL_U_MAX;
}

struct PlShared {
    alignas(16) int buf[2][PL_SPAN + 4];                // u and its doubled maxima, ping-pong; then the prefix sums of M ([0] = 0) and g
    alignas(16) int carry[PL_HALO];                     // WALK: u of the H2 samples in front of the next tile
    int wave[PL_WAVES];
    int stat[3];
};

// the 4 samples from i on (0 where outside [0, L)) and their u (0 outside [0, n))
template <bool VEC>
__device__ __forceinline__ void stage4(const float *src, long long i, long long L, long long n, float c, const int *__restrict__ tab, float v[4], int u[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (VEC) {                                                                // L % 4 == 0 and i % 4 == 0: inside as a whole or not at all
        if (i >= 0 && i < L) {
            const float4 a = *reinterpret_cast<const float4 *>(src + i);
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j >= 0 && i + j < L) v[j] = src[i + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = (i + j >= 0 && i + j < n) ? peak_need(v[j], c, tab) : 0;
}

template <bool VEC, bool WALK>
__global__ void __launch_bounds__(PL_THREADS, 8) peak_limit_kernel(const float *x, const long long *__restrict__ lengths, const int *__restrict__ tab, float c, int W,
                                                                float *y, int *__restrict__ gain, int *__restrict__ stats, long long B, long long L) {
    __shared__ PlShared sh;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int H2 = (2 * W + 3) & ~3, hv = H2 / 4;                             // the staged halo, a whole number of vectors
    const int SZ = PL_TILE + 2 * H2, MS = PL_TILE + 2 * W, win = 2 * W + 1;   // staged u; M and its prefix sums; the window
    const long long tiles = (L + PL_TILE - 1) / PL_TILE;
    for (long long row = blockIdx.y; row < B; row += gridDim.y) {
        const float *src = x + row * L;
        float *dst = y + row * L;
        int *gr = gain ? gain + row * L : nullptr;
        const long long n = pl_row_len(lengths, row, L);
        if (WALK) {                                                           // nothing lies in front of the row's first tile
            for (int k = tid; k < H2; k += PL_THREADS) sh.carry[k] = 0;
            __syncthreads();
        }
        for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const long long t0 = tile * PL_TILE;                              // local word k of the span is sample t0 - H2 + k
            // ---- stage: the tile's 4 samples of this lane, then one vector of the halos
            float xv[4];
            int uv[4];
            stage4<VEC>(src, t0 + 4 * tid, L, n, c, tab, xv, uv);
            *reinterpret_cast<int4 *>(&sh.buf[0][H2 + 4 * tid]) = make_int4(uv[0], uv[1], uv[2], uv[3]);
            int any = uv[0] | uv[1] | uv[2] | uv[3];
            if (tid < 2 * hv) {
                const bool left = tid < hv;
                const int k = left ? 4 * tid : PL_TILE + 4 * tid;             // (right: H2 + PL_TILE + 4 (tid - hv))
                int4 h;
                if (WALK && left) {
                    h = *reinterpret_cast<const int4 *>(&sh.carry[k]);
                } else {
                    float hx[4];
                    int hu[4];
                    stage4<VEC>(src, t0 - H2 + k, L, n, c, tab, hx, hu);
                    h = make_int4(hu[0], hu[1], hu[2], hu[3]);
                }
                *reinterpret_cast<int4 *>(&sh.buf[0][k]) = h;
                any |= h.x | h.y | h.z | h.w;
            }
            any = __syncthreads_or(any);
            if (WALK)                                                         // (read again only behind this iteration's last barrier)
                for (int k = tid; k < H2; k += PL_THREADS) sh.carry[k] = sh.buf[0][PL_TILE + k];

            const long long i0 = t0 + 4 * tid;
            if (!any) {                                                       // (uniform) nothing to reduce within reach: x's bits, g = 0
                if (VEC) {
                    if (i0 < L) {
                        if (!WALK) *reinterpret_cast<float4 *>(dst + i0) = make_float4(xv[0], xv[1], xv[2], xv[3]);
                        if (gr) *reinterpret_cast<int4 *>(gr + i0) = make_int4(0, 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (i0 + j < L) {
                            if (!WALK) dst[i0 + j] = xv[j];
                            if (gr) gr[i0 + j] = 0;
                        }
                }
                __syncthreads();                                              // the next tile stages into the same LDS
                continue;
            }

            // ---- hold: doubling maxima, buf[cur] -> buf[cur ^ 1]
            if (tid < 3) sh.stat[tid] = 0;
            int cur = 0, s = 1;
            for (; 2 * s <= win; s <<= 1) {
                const int *a = sh.buf[cur];
                int *b = sh.buf[cur ^ 1];
                for (int k = tid; k < SZ; k += PL_THREADS) {
                    int v = a[k];
                    if (k + s < SZ) v = max(v, a[k + s]);                     // (a window that leaves the span belongs to no M that is used)
                    b[k] = v;
                }
                __syncthreads();
                cur ^= 1;
            }
            const int *A = sh.buf[cur];                                       // A[k] = max u over the s samples from k on
            int *P = sh.buf[cur ^ 1];                                         // P[q + 1]: M of sample t0 - W + q, then the inclusive sums; P[0] = 0
            if (tid == 0) P[0] = 0;
            for (int q = tid; q < MS; q += PL_THREADS) {
                const long long j = t0 - W + q;
                const int ks = q + H2 - 2 * W;                                // the window's first sample, j - W, in the span
                P[q + 1] = (j >= 0 && j < n) ? max(A[ks], A[ks + win - s]) : 0;
            }
            __syncthreads();

            // ---- scan: thread tid takes the words [q0, q1) of M
            const int K = ((MS + PL_THREADS - 1) / PL_THREADS) | 1;
            const int q0 = min(MS, tid * K), q1 = min(MS, q0 + K);
            int own = 0;
            for (int q = q0; q < q1; ++q) own += P[q + 1];
            int inc = own;                                                    // inclusive over the wave
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(inc, d);
                if (lane >= d) inc += o;
            }
            if (lane == 63) sh.wave[w] = inc;
            __syncthreads();
            int run = inc - own;                                              // exclusive: what the threads below bring
            for (int j = 0; j < PL_WAVES; ++j)
                if (j < w) run += sh.wave[j];
            for (int q = q0; q < q1; ++q) {
                run += P[q + 1];
                P[q + 1] = run;                                               // (own words only: nobody else reads or writes them in this pass)
            }
            __syncthreads();

            // ---- smooth: thread tid takes the outputs tid + 1024 j (consecutive lanes, consecutive words); g goes to the array the maxima have left
            int *G = sh.buf[cur];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = tid + PL_THREADS * j;
                const long long i = t0 + r;
                int g = 0;
                if (i < n) {
                    const long long a = i - W > 0 ? i - W : 0, e = i + W < n - 1 ? i + W : n - 1;
                    const int qa = (int)(a - (t0 - W)), qe = (int)(e - (t0 - W));
                    const int S = P[qe + 1] - P[qa], N = (int)(e - a) + 1;
                    g = (S + N - 1) / N;
                }
                G[r] = g;
            }
            __syncthreads();

            // ---- apply: 4 samples a lane
            const int4 g4 = *reinterpret_cast<const int4 *>(&G[4 * tid]);
            const int gv[4] = {g4.x, g4.y, g4.z, g4.w};
            int over = 0, top = 0, moved = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                over += uv[j] > 0;
                top = max(top, gv[j]);
                if (gv[j] != 0) {
                    float v = pl_mul_f32_scalar(xv[j], exp2f(pl_mul_f32_scalar((float)gv[j], -0.001953125f)));      // (-g / 512, exact)
                    if (fabsf(v) > c) {                                       // (NaN fails the compare)
                        v = copysignf(c, v);
                        ++moved;
                    }
                    xv[j] = v;
                }
            }
            if (VEC) {
                if (i0 < L) {
                    if (!WALK || top != 0) *reinterpret_cast<float4 *>(dst + i0) = make_float4(xv[0], xv[1], xv[2], xv[3]);
                    if (gr) *reinterpret_cast<int4 *>(gr + i0) = g4;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i0 + j < L) {
                        if (!WALK || gv[j] != 0) dst[i0 + j] = xv[j];
                        if (gr) gr[i0 + j] = gv[j];
                    }
            }
            if (stats) {                                                      // (uniform) a wave's share, then the workgroup's, then one atomic each
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    over += __shfl_xor(over, d);
                    moved += __shfl_xor(moved, d);
                    top = max(top, __shfl_xor(top, d));
                }
                if (lane == 0) {
                    if (over) atomicAdd(&sh.stat[0], over);
                    if (top) atomicMax(&sh.stat[1], top);
                    if (moved) atomicAdd(&sh.stat[2], moved);
                }
                __syncthreads();
                if (tid == 0) {
                    if (sh.stat[0]) atomicAdd(&stats[row * 3 + 0], sh.stat[0]);
                    if (sh.stat[1]) atomicMax(&stats[row * 3 + 1], sh.stat[1]);
                    if (sh.stat[2]) atomicAdd(&stats[row * 3 + 2], sh.stat[2]);
                }
            }
            __syncthreads();                                                  // the next tile stages into the same LDS
        }
    }
}

static bool pl_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + nb && q < p + na;
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_peak_limit(const float *x, const int64_t *lengths, const int32_t *tab, float c, int window, float *y, int32_t *gain, int32_t *stats, int64_t B, int64_t L,
                  void *stream) {
    VS_REQUIRE(x && y && tab, "vs_peak_limit: x, y and tab must not be NULL");
    VS_REQUIRE(c > 0.f && c <= 1.f, "vs_peak_limit: the ceiling c = %g is not in (0, 1]", (double)c);
    VS_REQUIRE(window >= 0 && window <= PL_MAX_WINDOW, "vs_peak_limit: window = %d is not in [0, %d]", window, PL_MAX_WINDOW);
    VS_REQUIRE(B >= 1 && L >= 1, "vs_peak_limit: B >= 1 and L >= 1 are required (got %lld, %lld)", (long long)B, (long long)L);
    VS_REQUIRE(L < (1ll << 31) && B <= INT64_MAX / 16 / L, "vs_peak_limit: L = %lld is not below 2^31, or B * L is out of range", (long long)L);
    const size_t samples = (size_t)(B * L) * 4, items = (size_t)B * 12;
    VS_REQUIRE(x == y || !pl_overlap(x, samples, y, samples), "vs_peak_limit: y must be x itself (in place) or must not overlap it");
    const struct {
        const void *p;
        size_t n;
    } ins[3] = {{x, samples}, {lengths, (size_t)B * 8}, {tab, (size_t)VS_PEAK_LIMIT_TABLE * 4}}, outs[3] = {{y, samples}, {gain, samples}, {stats, items}};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 3; ++i)
            VS_REQUIRE((o == 0 && i == 0) || !pl_overlap(ins[i].p, ins[i].n, outs[o].p, outs[o].n),
                       "vs_peak_limit: y, gain or stats overlaps an input (the buffers must be distinct)");
        for (int q = o + 1; q < 3; ++q)
            VS_REQUIRE(!pl_overlap(outs[o].p, outs[o].n, outs[q].p, outs[q].n), "vs_peak_limit: y, gain and stats overlap each other");
    }
    if (stats) VS_CHECK_HIP(hipMemsetAsync(stats, 0, items, as_stream(stream)));
    const bool vec = L % 4 == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gain) & 15) == 0;
    const bool walk = x == y;
    const unsigned rows = (unsigned)(B < 65535 ? B : 65535);
    const dim3 grid(walk ? 1u : (unsigned)ceil_div(L, PL_TILE), rows);
#define VS_PL_LAUNCH(VEC, WALK)                                                                                                                        \
    hipLaunchKernelGGL((peak_limit_kernel<VEC, WALK>), grid, dim3(PL_THREADS), 0, as_stream(stream), x, (const long long *)lengths, (const int *)tab, c, \
                       window, y, (int *)gain, (int *)stats, (long long)B, (long long)L)
    if (vec && walk)
        VS_PL_LAUNCH(true, true);
    else if (vec)
        VS_PL_LAUNCH(true, false);
    else if (walk)
        VS_PL_LAUNCH(false, true);
    else
        VS_PL_LAUNCH(false, false);
#undef VS_PL_LAUNCH
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // extern "C"
