// loudness.hip -- programme loudness (mono ITU-R BS.1770-4, gated) and the gain to a target, for a batch of ragged waveforms (include/visinger_hip.h "f14",
// DESIGN.md 4.21).  Not in the reference (it peak-normalises on the host).  Three kernels, three launches, nothing read back in between:
//   loud_steps_kernel   grid (rows), 256 threads: one workgroup walks its row one 100 ms step (s samples) at a time.  The K-weighting cascade is recursive; it is
//     made parallel across the lanes: lane l owns the c = ceil(s / 256) consecutive samples from l c on.
//     stage   the step's samples go to LDS by 16-byte loads (a scalar head and tail of at most 3 samples where the step does not start on a 16-byte boundary),
//             lane l's samples c | 1 words apart; the next step's loads are issued before this step's arithmetic and land in registers under it.
//     pass A  every lane runs the cascade over its samples from a zero state -- lane 0 from the state the step before left -- in fp64: its end state e_l.
//     scan    the true state in front of lane l + 1 is sigma_(l+1) = M sigma_l + e_l, M = A^c the cascade's state transition over c samples.  A log-step scan
//             over the 256 lanes through LDS, level k adding M^(2^k) times the value 2^k lanes below, leaves sigma_(l+1) in lane l.  The products and sums of a
//             level are formed as pairs of doubles (the host passes M^(2^k) as such pairs) and rounded once: a level costs one rounding of its result, not one of
//             its cancelling terms -- the high-pass has a double pole at 0.995 and |M^(2^k)| reaches 70 where its product with a state stays of the state's size.
//     pass B  every lane reruns its samples from sigma_l, squares and accumulates; a wave butterfly and a sum of the four waves in a fixed order give S[b, i];
//             the last active lane's end state is the next step's sigma_0.
//   loud_gate_kernel    grid (rows), 256 threads: the 400 ms blocks of a row, the two gates, the loudness and the gain, in fp64 with fixed-order sums.
//   gain_apply_kernel   grid (tiles of 1024 samples, rows): y = x gain[b] inside the row, x's bits elsewhere and where the gain is 1; 16 bytes a lane.
#include "vs_internal.h"

#include <cmath>

namespace vs {

constexpr int LD_THREADS = VS_LOUD_THREADS;
constexpr int LD_WAVES = LD_THREADS / 64;
constexpr int LD_MIN_S = VS_LOUD_MIN_RATE / 10, LD_MAX_S = VS_LOUD_MAX_RATE / 10;
constexpr int LD_MAX_C = (LD_MAX_S + LD_THREADS - 1) / LD_THREADS;           // 19 samples a lane at 48 kHz
constexpr int LD_PITCH = LD_MAX_C | 1;                                     // words between two lanes' samples in LDS, at most
constexpr int LD_MAX_V = (LD_MAX_S / 4 + LD_THREADS - 1) / LD_THREADS;       // 16-byte loads a lane and step, at most
constexpr int LD_LEVELS = 8;
static_assert(LD_THREADS == 256 && (1 << LD_LEVELS) == LD_THREADS && LD_LEVELS * 2 * 16 == LD_THREADS, "the scan: eight levels over 256 lanes, 256 doubles of carry");
static_assert(LD_MAX_V * LD_THREADS * 4 >= LD_MAX_S, "the staging covers a step");

struct LdCoef {
    double b1[3], a1[2], b2[3], a2[2];                  // the shelf, the high-pass: b0 b1 b2, a1 a2 (a0 = 1)
};

struct LdState {
    double z[4];                                        // z1, z2 of the shelf, z1, z2 of the high-pass (transposed direct form II)
};

// one sample through the cascade; returns the weighted sample
__device__ __forceinline__ double ld_sample(const LdCoef &k, LdState &q, double x) {
    const double y1 = k.b1[0] * x + q.z[0];
    q.z[0] = k.b1[1] * x - k.a1[0] * y1 + q.z[1];
    q.z[1] = k.b1[2] * x - k.a1[1] * y1;
    const double y2 = k.b2[0] * y1 + q.z[2];
    q.z[2] = k.b2[1] * y1 - k.a2[0] * y2 + q.z[3];
    q.z[3] = k.b2[2] * y1 - k.a2[1] * y2;
    return y2;
}

// (hi, lo) += (m_hi + m_lo) v as a pair of doubles: the product's and the sum's rounding errors are kept in lo.  No contraction here: the error terms are
// exact only for the separately rounded product and sum.
__device__ __forceinline__ void ld_pair_fma(double &hi, double &lo, double m_hi, double m_lo, double v) {
#pragma clang fp contract(off)
    const double p = m_hi * v;
    const double pe = __builtin_fma(m_hi, v, -p);       // exact: m_hi v - p
    const double t = hi + p;
    const double bb = t - hi;
    const double se = (hi - (t - bb)) + (p - bb);       // exact: hi + p - t
    hi = t;
    lo += se + pe + m_lo * v;
}

// the row's length, clamped to [0, top]
__device__ __forceinline__ long long ld_row_len(const long long *lengths, long long row, long long top) {
    const long long len = lengths ? lengths[row] : top;
    return len < 0 ? 0 : (len > top ? top : len);
}

struct LdShared {
    alignas(16) float x[LD_THREADS * LD_PITCH];          // the step's samples, lane l's from l * pitch on
    alignas(16) double sc[2][LD_THREADS][4];             // the scan, ping-pong
    double m[LD_LEVELS][2][16];                          // M^(2^k) as pairs, row major
    double next[4];                                      // the state behind the step's last sample
    double red[LD_WAVES];
};

__global__ void __launch_bounds__(LD_THREADS) loud_steps_kernel(const float *__restrict__ wav, const long long *__restrict__ lengths, long long B, long long L,
                                                                 LdCoef k, const double *__restrict__ carry, int s, double *__restrict__ S, long long NS) {
    __shared__ LdShared sh;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = (s + LD_THREADS - 1) / LD_THREADS, pitch = c | 1;
    const int nact = (s + c - 1) / c;                                         // lanes with samples; the last one may own fewer than c
    const int cnt = tid < nact ? min(c, s - tid * c) : 0;
    (&sh.m[0][0][0])[tid] = carry[tid];                                       // LD_LEVELS * 2 * 16 == LD_THREADS doubles
    for (long long row = blockIdx.x; row < B; row += gridDim.x) {
        const float *src = wav + row * L;
        const long long nsteps = min(ld_row_len(lengths, row, L) / s, NS);
        for (long long i = nsteps + tid; i < NS; i += LD_THREADS) S[row * NS + i] = 0.0;
        if (tid < 4) sh.next[tid] = 0.0;
        // the staged step in registers: head (< 4 samples up to a 16-byte boundary), nvec vectors, tail
        float4 pv[LD_MAX_V];
        float ph = 0.f, pt = 0.f;
        int head = 0, nvec = 0;
        auto fetch = [&](long long step) {
            const float *p = src + step * s;
            head = (int)((4 - (((uintptr_t)p >> 2) & 3)) & 3);                // (s >= 800: the head never swallows the step)
            nvec = (s - head) >> 2;
            const int tail = s - head - 4 * nvec;
            if (tid < head) ph = p[tid];
            if (tid < tail) pt = p[head + 4 * nvec + tid];
#pragma unroll
            for (int v = 0; v < LD_MAX_V; ++v) {
                const int q = tid + LD_THREADS * v;
                if (q < nvec) pv[v] = *reinterpret_cast<const float4 *>(p + head + 4 * q);
            }
        };
        auto put = [&](int i, float v) { sh.x[(i / c) * pitch + i % c] = v; };     // sample i of the step
        if (nsteps > 0) fetch(0);
        for (long long step = 0; step < nsteps; ++step) {
            // ---- stage
            {
                const int tail = s - head - 4 * nvec;
                if (tid < head) put(tid, ph);
                if (tid < tail) put(head + 4 * nvec + tid, pt);
#pragma unroll
                for (int v = 0; v < LD_MAX_V; ++v) {
                    const int q = tid + LD_THREADS * v;
                    if (q < nvec) {
                        const int i = head + 4 * q;
                        put(i, pv[v].x), put(i + 1, pv[v].y), put(i + 2, pv[v].z), put(i + 3, pv[v].w);
                    }
                }
            }
            __syncthreads();                                                  // the samples, sh.next (and, the first time, sh.m) are visible
            if (step + 1 < nsteps) fetch(step + 1);
            // ---- pass A
            float xr[LD_MAX_C];
#pragma unroll
            for (int j = 0; j < LD_MAX_C; ++j) xr[j] = j < cnt ? sh.x[tid * pitch + j] : 0.f;
            LdState first;
#pragma unroll
            for (int i = 0; i < 4; ++i) first.z[i] = tid == 0 ? sh.next[i] : 0.0;
            LdState q = first;
#pragma unroll
            for (int j = 0; j < LD_MAX_C; ++j)
                if (j < cnt) (void)ld_sample(k, q, (double)xr[j]);
            // ---- scan: sc[cur][l] = the sum over j <= l of M^(l - j) e_j
#pragma unroll
            for (int i = 0; i < 4; ++i) sh.sc[0][tid][i] = q.z[i];
            int cur = 0;
            for (int lev = 0; lev < LD_LEVELS; ++lev) {
                __syncthreads();
                const int d = 1 << lev;
                double v[4] = {sh.sc[cur][tid][0], sh.sc[cur][tid][1], sh.sc[cur][tid][2], sh.sc[cur][tid][3]};
                if (tid >= d) {
                    const double *below = sh.sc[cur][tid - d];
                    const double u[4] = {below[0], below[1], below[2], below[3]};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        double hi = v[i], lo = 0.0;
#pragma unroll
                        for (int j = 0; j < 4; ++j) ld_pair_fma(hi, lo, sh.m[lev][0][4 * i + j], sh.m[lev][1][4 * i + j], u[j]);
                        v[i] = hi + lo;
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) sh.sc[cur ^ 1][tid][i] = v[i];
                cur ^= 1;
            }
            __syncthreads();
            // ---- pass B
            if (tid > 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) first.z[i] = sh.sc[cur][tid - 1][i];
            }
            q = first;
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < LD_MAX_C; ++j)
                if (j < cnt) {
                    const double y = ld_sample(k, q, (double)xr[j]);
                    acc = fma(y, y, acc);
                }
            if (tid == nact - 1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sh.next[i] = q.z[i];
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
            if (lane == 0) sh.red[w] = acc;
            __syncthreads();
            if (tid == 0) S[row * NS + step] = (sh.red[0] + sh.red[1]) + (sh.red[2] + sh.red[3]);
        }
        __syncthreads();                                                      // the next row clears sh.next
    }
}

// the workgroup's sum of v and of n in a fixed order: every thread gets both
__device__ __forceinline__ void ld_block_sum(double &v, long long &n, double *red_v, long long *red_n) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        v += __shfl_xor(v, d);
        n += __shfl_xor(n, d);
    }
    __syncthreads();                                                          // (the arrays' last readers are done)
    if (lane == 0) red_v[w] = v, red_n[w] = n;
    __syncthreads();
    v = (red_v[0] + red_v[1]) + (red_v[2] + red_v[3]);
    n = (red_n[0] + red_n[1]) + (red_n[2] + red_n[3]);
}

__global__ void __launch_bounds__(LD_THREADS) loud_gate_kernel(const double *__restrict__ S, const long long *__restrict__ lengths, long long B, long long NS, int s,
                                                                double target, double max_gain_db, double *__restrict__ loud, float *__restrict__ gain,
                                                                int *__restrict__ stats) {
    __shared__ double red_v[LD_WAVES];
    __shared__ long long red_n[LD_WAVES];
    const int tid = threadIdx.x;
    const double den = 4.0 * (double)s;
    for (long long row = blockIdx.x; row < B; row += gridDim.x) {
        const double *Sr = S + row * NS;
        long long nsteps = NS;
        if (lengths) {
            const long long len = lengths[row];
            nsteps = len < 0 ? 0 : min(len / s, NS);
        }
        const long long nblk = nsteps >= 4 ? nsteps - 3 : 0;
        auto block = [&](long long j) { return (((Sr[j] + Sr[j + 1]) + Sr[j + 2]) + Sr[j + 3]) / den; };
        // the absolute gate; a block that is not finite makes the row's loudness a NaN
        double sum = 0.0;
        long long n = 0, bad = 0;
        for (long long j = tid; j < nblk; j += LD_THREADS) {
            const double z = block(j);
            if (z > VS_LOUD_ABS_GATE) sum += z, ++n;
            if (!(fabs(z) <= 1.7976931348623157e308)) ++bad;
        }
        double unused = 0.0;
        ld_block_sum(sum, n, red_v, red_n);
        ld_block_sum(unused, bad, red_v, red_n);
        const long long n_abs = n;
        const double rel = n_abs > 0 ? 0.1 * (sum / (double)n_abs) : 0.0;
        // the relative gate
        sum = 0.0, n = 0;
        if (n_abs > 0)
            for (long long j = tid; j < nblk; j += LD_THREADS) {
                const double z = block(j);
                if (z > VS_LOUD_ABS_GATE && z > rel) sum += z, ++n;
            }
        ld_block_sum(sum, n, red_v, red_n);
        if (tid == 0) {
            double lk = -INFINITY;
            if (bad > 0)
                lk = NAN;
            else if (n > 0)
                lk = -0.691 + 10.0 * log10(sum / (double)n);
            float g = 1.0f;
            if (fabs(lk) <= 1.7976931348623157e308) g = (float)pow(10.0, fmin(target - lk, max_gain_db) / 20.0);
            loud[row] = lk;
            gain[row] = g;
            stats[row * 3 + 0] = (int)min(nblk, (long long)INT32_MAX);
            stats[row * 3 + 1] = (int)min(n_abs, (long long)INT32_MAX);
            stats[row * 3 + 2] = (int)min(n, (long long)INT32_MAX);
        }
    }
}

// One multiply as an opaque scalar instruction (limiter.hip: pl_mul_f32_scalar): the four products of a lane's 16 bytes are not to be paired into v_pk_mul_f32
// by the SLP vectoriser; this kernel runs beside another stream's MFMAs under synthesize(streams=2).  build.py refuses an object that holds the bad form.
__device__ __forceinline__ float ld_mul_f32_scalar(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

constexpr int GA_TILE = 4 * LD_THREADS;

template <bool VEC>
__global__ void __launch_bounds__(LD_THREADS) gain_apply_kernel(const float *x, const float *__restrict__ gain, const long long *__restrict__ lengths, float *y,
                                                                 long long B, long long L, bool in_place) {
    const long long i0 = (long long)blockIdx.x * GA_TILE + 4 * threadIdx.x;
    if (i0 >= L) return;
    for (long long row = blockIdx.y; row < B; row += gridDim.y) {
        const float g = gain[row];
        const long long n = g == 1.0f ? 0 : ld_row_len(lengths, row, L);      // a gain of 1 (and a NaN never equals it: it scales) leaves x's bits
        if (in_place && i0 >= n) continue;
        const float *src = x + row * L;
        float *dst = y + row * L;
        if (VEC) {                                                            // L % 4 == 0: the four samples are inside L
            float4 v = *reinterpret_cast<const float4 *>(src + i0);
            if (i0 < n) v.x = ld_mul_f32_scalar(v.x, g);
            if (i0 + 1 < n) v.y = ld_mul_f32_scalar(v.y, g);
            if (i0 + 2 < n) v.z = ld_mul_f32_scalar(v.z, g);
            if (i0 + 3 < n) v.w = ld_mul_f32_scalar(v.w, g);
            *reinterpret_cast<float4 *>(dst + i0) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < L) {
                    const float v = src[i0 + j];
                    if (i0 + j < n)
                        dst[i0 + j] = ld_mul_f32_scalar(v, g);
                    else if (!in_place)
                        dst[i0 + j] = v;
                }
        }
    }
}

static bool ld_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + nb && q < p + na;
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_loud_steps(const float *wav, const int64_t *lengths, int64_t B, int64_t L, const double *coef, const double *carry, int s, double *S, int64_t NS,
                  void *stream) {
    VS_REQUIRE(wav && coef && carry && S, "vs_loud_steps: wav, coef, carry and S must not be NULL");
    VS_REQUIRE(s >= LD_MIN_S && s <= LD_MAX_S, "vs_loud_steps: s = %d samples a step is not in [%d, %d] (rates of 8 to 48 kHz)", s, LD_MIN_S, LD_MAX_S);
    VS_REQUIRE(B >= 1 && L >= 1 && NS >= 1, "vs_loud_steps: B >= 1, L >= 1 and NS >= 1 are required (got %lld, %lld, %lld)", (long long)B, (long long)L, (long long)NS);
    VS_REQUIRE(L < (1ll << 31) && NS < (1ll << 31) && B <= INT64_MAX / 16 / L && B <= INT64_MAX / 16 / NS,
               "vs_loud_steps: L = %lld or NS = %lld is not below 2^31, or B times it is out of range", (long long)L, (long long)NS);
    LdCoef k;
    for (int i = 0; i < 10; ++i) VS_REQUIRE(std::isfinite(coef[i]), "vs_loud_steps: coef[%d] is not finite", i);
    std::memcpy(&k, coef, sizeof k);
    static_assert(sizeof(LdCoef) == 10 * sizeof(double), "the ten coefficients, packed");
    const size_t samples = (size_t)(B * L) * 4, sums = (size_t)(B * NS) * 8;
    VS_REQUIRE(!ld_overlap(S, sums, wav, samples) && !ld_overlap(S, sums, lengths, (size_t)B * 8) && !ld_overlap(S, sums, carry, (size_t)LD_THREADS * 8),
               "vs_loud_steps: S overlaps an input (the buffers must be distinct)");
    const unsigned rows = (unsigned)(B < 65535 ? B : 65535);
    hipLaunchKernelGGL(loud_steps_kernel, dim3(rows), dim3(LD_THREADS), 0, as_stream(stream), wav, (const long long *)lengths, (long long)B, (long long)L, k, carry,
                       s, S, (long long)NS);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

int vs_loud_gate(const double *S, const int64_t *lengths, int64_t B, int64_t NS, int s, double target, double max_gain_db, double *loud, float *gain,
                 int32_t *stats, void *stream) {
    VS_REQUIRE(S && loud && gain && stats, "vs_loud_gate: S, loud, gain and stats must not be NULL");
    VS_REQUIRE(s >= LD_MIN_S && s <= LD_MAX_S, "vs_loud_gate: s = %d samples a step is not in [%d, %d]", s, LD_MIN_S, LD_MAX_S);
    VS_REQUIRE(B >= 1 && NS >= 1 && NS < (1ll << 31) && B <= INT64_MAX / 16 / NS, "vs_loud_gate: B >= 1 and 1 <= NS < 2^31 are required (got %lld, %lld)",
               (long long)B, (long long)NS);
    VS_REQUIRE(target >= -70.0 && target <= 0.0, "vs_loud_gate: target = %g LUFS is not in [-70, 0]", target);
    VS_REQUIRE(max_gain_db >= 0.0 && max_gain_db <= 60.0, "vs_loud_gate: max_gain_db = %g is not in [0, 60]", max_gain_db);
    const struct {
        const void *p;
        size_t n;
    } ins[2] = {{S, (size_t)(B * NS) * 8}, {lengths, (size_t)B * 8}}, outs[3] = {{loud, (size_t)B * 8}, {gain, (size_t)B * 4}, {stats, (size_t)B * 12}};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 2; ++i)
            VS_REQUIRE(!ld_overlap(ins[i].p, ins[i].n, outs[o].p, outs[o].n), "vs_loud_gate: loud, gain or stats overlaps an input (the buffers must be distinct)");
        for (int q = o + 1; q < 3; ++q) VS_REQUIRE(!ld_overlap(outs[o].p, outs[o].n, outs[q].p, outs[q].n), "vs_loud_gate: loud, gain and stats overlap each other");
    }
    const unsigned rows = (unsigned)(B < 65535 ? B : 65535);
    hipLaunchKernelGGL(loud_gate_kernel, dim3(rows), dim3(LD_THREADS), 0, as_stream(stream), S, (const long long *)lengths, (long long)B, (long long)NS, s, target,
                       max_gain_db, loud, gain, (int *)stats);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

int vs_gain_apply(const float *x, const float *gain, const int64_t *lengths, float *y, int64_t B, int64_t L, void *stream) {
    VS_REQUIRE(x && gain && y, "vs_gain_apply: x, gain and y must not be NULL");
    VS_REQUIRE(B >= 1 && L >= 1, "vs_gain_apply: B >= 1 and L >= 1 are required (got %lld, %lld)", (long long)B, (long long)L);
    VS_REQUIRE(L < (1ll << 31) && B <= INT64_MAX / 16 / L, "vs_gain_apply: L = %lld is not below 2^31, or B * L is out of range", (long long)L);
    const size_t samples = (size_t)(B * L) * 4;
    VS_REQUIRE(x == y || !ld_overlap(x, samples, y, samples), "vs_gain_apply: y must be x itself (in place) or must not overlap it");
    VS_REQUIRE(!ld_overlap(y, samples, gain, (size_t)B * 4) && !ld_overlap(y, samples, lengths, (size_t)B * 8),
               "vs_gain_apply: y overlaps gain or lengths (the buffers must be distinct)");
    const bool vec = L % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    const dim3 grid((unsigned)ceil_div(L, GA_TILE), (unsigned)(B < 65535 ? B : 65535));
    if (vec)
        hipLaunchKernelGGL((gain_apply_kernel<true>), grid, dim3(LD_THREADS), 0, as_stream(stream), x, gain, (const long long *)lengths, y, (long long)B, (long long)L,
                           x == y);
    else
        hipLaunchKernelGGL((gain_apply_kernel<false>), grid, dim3(LD_THREADS), 0, as_stream(stream), x, gain, (const long long *)lengths, y, (long long)B,
                           (long long)L, x == y);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // extern "C"
